// Micro-benchmark: the tail of one Krylov step and the head of the next on the flagship workload (216^3 7-point Laplacian, basis streaming from HBM) as
// today's THREE launches - final Gram-Schmidt update of column k (two pending passes, scaled, written through), pair-form dictionary product y = A v_k,
// dot sweep of y against columns 0..k and itself - against ONE "forward" launch: one workgroup per CU keeps the row panel V(r,0:k) of its tile in
// registers after the update, publishes the stored tile behind a per-tile flag and, one round later, forms the tile's rows of y and the k + 2 dots from
// the registers. Between the two forms v_k and y must have the same bits; the dots are the same products summed in another fixed order.
// Hand-off (one row of the "Valid forms" table): 16-byte sc1 stores of v_k, every storing wave drains (s_waitcnt vmcnt(0)), workgroup barrier, ONE lane
// stores the tile's flag (relaxed, agent scope: an sc1 store) with the launch's epoch; the consumer's wave 0 polls the flags of the neighbour tiles with
// relaxed agent-scope loads (sc1) and s_sleep, the other waves load behind a workgroup barrier; EVERY load of v_k in the A-phase is a buffer_load sc1
// (the centre pair comes from registers: a uniform branch around its load). hipMalloc memory, one workgroup per CU.
// Waits are bounded by wall time (s_memrealtime, 100 MHz): a wave whose budget runs out sets the abort word, every workgroup that sees it skips its
// remaining A-phases and still completes every C-phase; the host then runs the ordinary product and dot sweep. Wait graph: a C-phase never waits, the
// A-phase of round i - 1 waits for C-phases of rounds <= i only, and every workgroup runs C(i) before A(i - 1): the graph descends in the round index.
// k_forward_pipe: four variants of the forward launch with the next tile's panel loads in flight through the hand-off and one panel parked in LDS (which
// panel; polls in front of the loads or behind), each compared with k_forward bit for bit - v, y and the dots - and timed alternating with it.
// k_forward_round: the kept pipelined variant with its round reordered - the tile's dots a round later in the shadow of the store drain, the park in front
// of the drain or behind the flag, a part of the next panel issued behind the neighbour loads - compared and timed the same way.
// build: hipcc -O3 --offload-arch=gfx950 -I../../slepc_amd/csrc step_forward.hip -o step_forward        run: ./step_forward [side = 216]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <vector>
#include <array>
#include <algorithm>
#include "ks_dict_pairs.h"
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)
constexpr int BLOCK = 256, TILE = 512, NBT = 5;
typedef double d2 __attribute__((ext_vector_type(2)));
constexpr unsigned OOB = 0xfffffff0u;

// DPP-free wave sum (fixed shuffle tree)
__device__ __forceinline__ double wave_sum(double v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }

// how a lane of the pair walk reaches x. SC1: every load bypasses this CU's L1 (aux 16). own >= 0: the pair at index `own` is the lane's own rows, held in c.
template <bool SC1, bool OWN>
struct Lane {
  __amdgpu_buffer_rsrc_t rs; long long n; long long own; ksp::D2 c;
  __device__ __forceinline__ Lane(const double *x, long long n_, long long own_, ksp::D2 c_) : rs(__builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(x), 0, (int)(unsigned)(n_ * 8), 0x00020000)), n(n_), own(own_), c(c_) {}
  __device__ __forceinline__ unsigned off(long long i, bool want = true) const { return want && (unsigned long long)i < (unsigned long long)n ? (unsigned)(i * 8) : OOB; }
  __device__ __forceinline__ int lane() const { return threadIdx.x & 63; }
  __device__ __forceinline__ ksp::D2 pair(long long i) const
  {
    // i - own is the base's offset, the same in every lane: a uniform branch, so that no select stands behind a load (it would wait for it, and the
    // loads of the bases would go out one round trip after the other)
    if (OWN && __builtin_amdgcn_readfirstlane((int)(i == own))) return c;
    ksp::D2 v; const auto t = __builtin_amdgcn_raw_buffer_load_b128(rs, off(i), 0, SC1 ? 16 : 0); __builtin_memcpy(&v, &t, 16);
    return v;
  }
  __device__ __forceinline__ double one(long long i, bool want) const { double v; const auto t = __builtin_amdgcn_raw_buffer_load_b64(rs, off(i, want), 0, SC1 ? 16 : 0); __builtin_memcpy(&v, &t, 8); return v; }
  __device__ __forceinline__ double up(double v, long long) const { return __shfl_up(v, 1); }
  __device__ __forceinline__ double down(double v, long long) const { return __shfl_down(v, 1); }
};

extern __shared__ __attribute__((aligned(16))) double dyn_lds[];
__device__ __forceinline__ void fill_tables(const ksp::PairArgs &pa, const double *pcoef, const unsigned *pmask, int npat, double *&sc, unsigned *&sm)
{
  sc = dyn_lds; sm = reinterpret_cast<unsigned *>(sc + npat * 3 * pa.nb);
  for (int i = threadIdx.x; i < npat * 3 * pa.nb; i += BLOCK) sc[i] = pcoef[i];
  for (int i = threadIdx.x; i < npat; i += BLOCK) sm[i] = pmask[i];
}
__host__ __device__ inline size_t park_offset(int npat, int nb) { return ((size_t)npat * (3 * nb * sizeof(double) + sizeof(unsigned)) + 15) & ~(size_t)15; }      // the parked panel of the pipelined form, behind the tables
template <int NACC>
__device__ __forceinline__ void put_partials(const double (&acc)[NACC], int ncols, double *__restrict__ partials)
{
  __shared__ double red[4][NACC];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < NACC; c++) { const double s = wave_sum(acc[c]); if (lane == 0) red[w][c] = s; }
  __syncthreads();
  if ((int)threadIdx.x < ncols) partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// ---- today's three launches -------------------------------------------------------------------------------------------------------------------
// final update: v = (v - V c1 - V c2) * alpha, pass by pass, stored write-through
template <int KT>
__global__ __launch_bounds__(BLOCK) void k_final(const double *V, long long ld, int n, double *v, const double *__restrict__ cg, double alpha)
{
  double cc[2][KT];
#pragma unroll
  for (int p = 0; p < 2; p++)
#pragma unroll
    for (int i = 0; i < KT; i++) cc[p][i] = -cg[p * KT + i];
  const long long ntiles = ((long long)n + TILE - 1) / TILE;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long r = t * TILE + 2LL * threadIdx.x;
    if (r + 1 < n) {
      d2 s = *reinterpret_cast<const d2 *>(v + r);
      d2 xv[KT];
#pragma unroll
      for (int i = 0; i < KT; i++) xv[i] = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(V + (long long)i * ld + r));
#pragma unroll
      for (int p = 0; p < 2; p++)
#pragma unroll
        for (int i = 0; i < KT; i++) { s.x = fma(cc[p][i], xv[i].x, s.x); s.y = fma(cc[p][i], xv[i].y, s.y); }
      s.x *= alpha; s.y *= alpha;
      asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(reinterpret_cast<d2 *>(v + r)), "v"(s) : "memory");
    }
  }
}
// pair-form product, every XCD one contiguous eighth of the row groups
__global__ __launch_bounds__(BLOCK) void k_spmv(int n, const unsigned char *__restrict__ rowpat, int npat, const double *__restrict__ x, double *__restrict__ y,
                                                ksp::PairArgs pa, const double *__restrict__ pcoef, const unsigned *__restrict__ pmask)
{
  double *sc; unsigned *sm;
  fill_tables(pa, pcoef, pmask, npat, sc, sm);
  __syncthreads();
  const long long groups = ((long long)n + TILE - 1) / TILE, gper = (groups + 7) / 8;
  const long long g0 = (blockIdx.x % 8) * gper, g1 = g0 + gper < groups ? g0 + gper : groups;
  const Lane<false, false> ln(x, n, -1, ksp::D2{0.0, 0.0});
  for (long long g = g0 + blockIdx.x / 8; g < g1; g += gridDim.x / 8) {
    const long long r = g * TILE + 2LL * threadIdx.x;
    const unsigned pp = *reinterpret_cast<const unsigned short *>(rowpat + (r < n ? r : 0));
    double y0, y1;
    ksp::dict_pair_walk<NBT>(pa, sc, sm, (int)(pp & 255u), (int)(pp >> 8), r, ln, y0, y1);
    if (r + 1 < n) __builtin_nontemporal_store(d2{y0, y1}, reinterpret_cast<d2 *>(y + r));
  }
}
// dot sweep: partials <- [V(:,0:ncols-1), y]^T y  (ncols - 1 columns in memory, the self dot last)
template <int KT>
__global__ __launch_bounds__(BLOCK) void k_dots(const double *__restrict__ V, long long ld, int n, const double *__restrict__ y, double *__restrict__ partials)
{
  double acc[KT + 1];
#pragma unroll
  for (int i = 0; i <= KT; i++) acc[i] = 0.0;
  const long long ntiles = ((long long)n + TILE - 1) / TILE;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long r = t * TILE + 2LL * threadIdx.x;
    if (r + 1 < n) {
      d2 xv[KT];
#pragma unroll
      for (int i = 0; i < KT; i++) xv[i] = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(V + (long long)i * ld + r));
      const d2 yv = *reinterpret_cast<const d2 *>(y + r);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < KT; i++) { acc[i] = fma(xv[i].x, yv.x, acc[i]); acc[i] = fma(xv[i].y, yv.y, acc[i]); }
      acc[KT] = fma(yv.x, yv.x, acc[KT]); acc[KT] = fma(yv.y, yv.y, acc[KT]);
    }
  }
  put_partials<KT + 1>(acc, KT + 1, partials);
}

// ---- the forward launch -----------------------------------------------------------------------------------------------------------------------
// ctl[0]: abort word (the epoch of the launch that gave up), ctl[1]: waits that ran out of budget, ctl[2]: polls that did not match at once (telemetry)
// hooks: bit 0: odd workgroups sleep before they publish (uneven load); budget: wall ticks of 10 ns a wait may take (0: every wait that has to wait gives up)
template <int KT>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_forward(const double *V, long long ld, int n, double *v, double *__restrict__ y, const double *__restrict__ cg, double alpha,
                                                   const unsigned char *__restrict__ rowpat, int npat, ksp::PairArgs pa, const double *__restrict__ pcoef, const unsigned *__restrict__ pmask,
                                                   unsigned *flags, unsigned epoch, unsigned *ctl, double *__restrict__ partials, unsigned long long budget, int hooks)
{
  __shared__ double cc[2][KT];
  __shared__ int go_sh;
  double *sc; unsigned *sm;
  fill_tables(pa, pcoef, pmask, npat, sc, sm);
  for (int i = threadIdx.x; i < 2 * KT; i += BLOCK) cc[i / KT][i % KT] = -cg[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long ntiles = ((long long)n + TILE - 1) / TILE;
  double acc[KT + 2];
#pragma unroll
  for (int i = 0; i < KT + 2; i++) acc[i] = 0.0;
  d2 pv[KT]; d2 ps = {0.0, 0.0};                      // the panel and the new rows of the tile whose A-phase is still to come
#pragma unroll
  for (int i = 0; i < KT; i++) pv[i] = d2{0.0, 0.0};
  long long pt = -1;
  bool dead = false;                                   // uniform: this workgroup has seen the abort word
  for (long long t = blockIdx.x;; t += gridDim.x) {
    const bool has = t < ntiles;
    d2 cv[KT]; d2 cs = {0.0, 0.0};
#pragma unroll
    for (int i = 0; i < KT; i++) cv[i] = d2{0.0, 0.0};
    // ---- C-phase: the final update of tile t, as k_final ----
    if (has) {
      const long long r = t * TILE + 2LL * threadIdx.x;
      if (r + 1 < n) {
        cs = *reinterpret_cast<const d2 *>(v + r);      // written by the launch before this one; nobody stores it in this launch before this store
#pragma unroll
        for (int i = 0; i < KT; i++) cv[i] = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(V + (long long)i * ld + r));
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
          for (int i = 0; i < KT; i++) { const double c = cc[p][i]; cs.x = fma(c, cv[i].x, cs.x); cs.y = fma(c, cv[i].y, cs.y); }
        cs.x *= alpha; cs.y *= alpha;
        asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(reinterpret_cast<d2 *>(v + r)), "v"(cs) : "memory");
      }
      if ((hooks & 1) && (blockIdx.x & 1)) for (int q = 0; q < 40; q++) __builtin_amdgcn_s_sleep(127);      // about 0.1 ms of lag per round
    }
    // ---- publish ----
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave
    __syncthreads();
    if (has && threadIdx.x == 0) __hip_atomic_store(flags + t, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // ---- A-phase of the tile of the round before ----
    if (pt >= 0 && !dead) {
      if (w == 0) {
        // lane 3 kb + wh polls the wh-th tile that holds rows of base kb's window [r0 + b - d, r0 + 511 + b + d]; lane 63 reads the abort word
        const int kb = lane / 3, wh = lane % 3;
        long long tl = -1;
        int b = 0; bool isb = false;
#pragma unroll
        for (int k = 0; k < NBT; k++) if (k == kb && k < pa.nb) { b = pa.base[k]; isb = true; }
        if (isb) {
          const int d = (int)(pa.dmask >> kb & 1u);         // a wide base also reads the element in front of its first pair and the one behind its last
          long long lo = pt * TILE + b - d, hi = pt * TILE + (TILE - 1) + b + d;
          if (lo < 0) lo = 0;
          if (hi > n - 1) hi = n - 1;
          if (lo <= hi && (lo >> 9) + wh <= (hi >> 9)) tl = (lo >> 9) + wh;
        }
        if (tl == pt) tl = -1;                          // this workgroup's own tile: stored, drained and behind the barrier above
        int res;
        bool first = true;
        const long long tstart = wall_clock64();
        for (;;) {
          unsigned f = epoch, ab = 0;
          if (tl >= 0) f = __hip_atomic_load(flags + tl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (lane == 63) ab = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (__any(lane == 63 && ab == epoch)) { res = 0; break; }
          if (__all(f == epoch)) { res = 1; break; }
          if (first && lane == 0) atomicAdd(ctl + 2, 1u);
          first = false;
          if ((unsigned long long)(wall_clock64() - tstart) >= budget) {
            if (lane == 0) { __hip_atomic_exchange(ctl, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); atomicAdd(ctl + 1, 1u); }
            res = 0; break;
          }
          __builtin_amdgcn_s_sleep(8);
        }
        if (lane == 0) go_sh = res;
      }
      __syncthreads();                                  // the other waves load v only behind this barrier
      if (go_sh) {
        const long long r = pt * TILE + 2LL * threadIdx.x;
        const Lane<true, true> ln(v, n, r, ksp::D2{ps.x, ps.y});
        const unsigned pp = *reinterpret_cast<const unsigned short *>(rowpat + (r < n ? r : 0));
        double y0, y1;
        ksp::dict_pair_walk<NBT>(pa, sc, sm, (int)(pp & 255u), (int)(pp >> 8), r, ln, y0, y1);
        if (r + 1 < n) {
          __builtin_nontemporal_store(d2{y0, y1}, reinterpret_cast<d2 *>(y + r));
#pragma unroll
          for (int i = 0; i < KT; i++) { acc[i] = fma(pv[i].x, y0, acc[i]); acc[i] = fma(pv[i].y, y1, acc[i]); }
          acc[KT] = fma(ps.x, y0, acc[KT]); acc[KT] = fma(ps.y, y1, acc[KT]);
          acc[KT + 1] = fma(y0, y0, acc[KT + 1]); acc[KT + 1] = fma(y1, y1, acc[KT + 1]);
        }
      } else dead = true;
    }
    if (!has) break;
#pragma unroll
    for (int i = 0; i < KT; i++) pv[i] = cv[i];
    ps = cs; pt = t;
  }
  if (dead) return;
  put_partials<KT + 2>(acc, KT + 2, partials);
}

// ---- the pipelined forward launch -------------------------------------------------------------------------------------------------------------
// Same tiles, same hand-off, same sums; the panel loads of tile i + 1 are issued behind publish(i), in front of the A-phase of tile i - 1, so that they are in
// flight through the poll, the barrier, the neighbour loads, the walk and the dots. Three panels are live then and the register file holds two: one is
// parked in LDS (KT columns x 256 lanes x 16 B behind the dictionary tables; lane l writes and reads column i at park[i * BLOCK + l], so the panel itself
// needs no barrier).
//   PARK 0: the panel just computed (tile i) is parked, the loads of tile i + 1 land in its registers, and it comes back to registers behind A(i - 1);
//   PARK 1: the waiting panel (tile i - 1) is parked, the loads land in ITS registers, and the dots of A(i - 1) read it from LDS.
//   POLL_FIRST: wave 0 issues its first flag and abort polls in front of the panel loads (they return first: vector loads return in order), else behind them.
// Progress as k_forward: C(i) waits for nothing but its own loads of V(:,0:k) and of its own rows of v, publish(i) stands in front of A(i - 1), a re-poll
// queues behind panel loads, which wait for nothing.
// The panel loads stand under NO branch: the compiler's wait for wave 0's first polls counts the loads issued behind them (s_waitcnt vmcnt(KT + 1)), and
// where a path around the loads joins, it has to take that path's count, 0 - the whole panel. A lane without a row pair (past n, or no tile left) reads
// rows 0 and 1 of every column instead, one line per column, and nobody uses what it gets.
template <int KT>
__device__ __forceinline__ void load_panel(const double *V, long long ld, int n, const double *v, long long t, bool has, d2 (&xv)[KT], d2 &s)
{
  const long long r = t * TILE + 2LL * threadIdx.x;
  const bool ok = has && r + 1 < n;
  const long long rr = ok ? r : 0;
  s = *reinterpret_cast<const d2 *>(ok ? v + r : V);    // the tile's own rows of v: written by the launch before this one, stored in this launch by this lane only
#pragma unroll
  for (int i = 0; i < KT; i++) xv[i] = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(V + (long long)i * ld + rr));
}
// The barrier between wave 0's matched poll and the other waves' loads of v. __syncthreads() puts s_waitcnt vmcnt(0) behind s_barrier (its workgroup-scope
// acquire), which would hold every wave until its panel loads of the next tile are in: order LDS only (go_sh), and keep the compiler from moving a load over it.
__device__ __forceinline__ void barrier_lds_only()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
  asm volatile("" ::: "memory");
}
template <int KT, int PARK, bool POLL_FIRST>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_forward_pipe(const double *V, long long ld, int n, double *v, double *__restrict__ y, const double *__restrict__ cg, double alpha,
                                                   const unsigned char *__restrict__ rowpat, int npat, ksp::PairArgs pa, const double *__restrict__ pcoef, const unsigned *__restrict__ pmask,
                                                   unsigned *flags, unsigned epoch, unsigned *ctl, double *__restrict__ partials, unsigned long long budget, int hooks)
{
  __shared__ double cc[2][KT];
  __shared__ int go_sh;
  double *sc; unsigned *sm;
  fill_tables(pa, pcoef, pmask, npat, sc, sm);
  d2 *park = reinterpret_cast<d2 *>(reinterpret_cast<char *>(dyn_lds) + park_offset(npat, pa.nb)) + threadIdx.x;
  for (int i = threadIdx.x; i < 2 * KT; i += BLOCK) cc[i / KT][i % KT] = -cg[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long ntiles = ((long long)n + TILE - 1) / TILE;
  double acc[KT + 2];
#pragma unroll
  for (int i = 0; i < KT + 2; i++) acc[i] = 0.0;
  d2 pv[KT]; d2 ps = {0.0, 0.0};                      // the panel (PARK 0) and the new rows of the tile whose A-phase is still to come
#pragma unroll
  for (int i = 0; i < KT; i++) pv[i] = d2{0.0, 0.0};
  long long pt = -1;
  bool dead = false;
  d2 nv[KT]; d2 ns;                                    // the panel and the rows of v of the tile of the next round, in flight
  load_panel<KT>(V, ld, n, v, blockIdx.x, (long long)blockIdx.x < ntiles, nv, ns);
  for (long long t = blockIdx.x;; t += gridDim.x) {
    const bool has = t < ntiles;
    d2 cv[KT]; d2 cs = ns;
#pragma unroll
    for (int i = 0; i < KT; i++) cv[i] = nv[i];
    // ---- C-phase: the final update of tile t, as k_final; its loads went out a round ago ----
    if (has) {
      const long long r = t * TILE + 2LL * threadIdx.x;
      if (r + 1 < n) {
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
          for (int i = 0; i < KT; i++) { const double c = cc[p][i]; cs.x = fma(c, cv[i].x, cs.x); cs.y = fma(c, cv[i].y, cs.y); }
        cs.x *= alpha; cs.y *= alpha;
        asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(reinterpret_cast<d2 *>(v + r)), "v"(cs) : "memory");
      }
      if ((hooks & 1) && (blockIdx.x & 1)) for (int q = 0; q < 40; q++) __builtin_amdgcn_s_sleep(127);
    }
    // ---- publish ----
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave
    __syncthreads();
    if (has && threadIdx.x == 0) __hip_atomic_store(flags + t, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool arun = pt >= 0 && !dead;
    // ---- park ----
    if (PARK == 0) {
#pragma unroll
      for (int i = 0; i < KT; i++) park[i * BLOCK] = cv[i];
    } else if (arun) {
#pragma unroll
      for (int i = 0; i < KT; i++) park[i * BLOCK] = pv[i];
    }
    // ---- wave 0's first polls of A(t - gridDim.x), then every wave's loads of the next round's tile ----
    long long tl = -1;
    unsigned f0 = epoch, ab0 = 0;
    if (arun && w == 0) {
      const int kb = lane / 3, wh = lane % 3;
      int b = 0; bool isb = false;
#pragma unroll
      for (int k = 0; k < NBT; k++) if (k == kb && k < pa.nb) { b = pa.base[k]; isb = true; }
      if (isb) {
        const int d = (int)(pa.dmask >> kb & 1u);
        long long lo = pt * TILE + b - d, hi = pt * TILE + (TILE - 1) + b + d;
        if (lo < 0) lo = 0;
        if (hi > n - 1) hi = n - 1;
        if (lo <= hi && (lo >> 9) + wh <= (hi >> 9)) tl = (lo >> 9) + wh;
      }
      if (tl == pt) tl = -1;
      if (POLL_FIRST) {
        if (tl >= 0) f0 = __hip_atomic_load(flags + tl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 63) ab0 = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    load_panel<KT>(V, ld, n, v, t + gridDim.x, has && t + gridDim.x < ntiles, nv, ns);
    __builtin_amdgcn_sched_barrier(0);
    // ---- A-phase of the tile of the round before ----
    if (arun) {
      if (w == 0) {
        int res;
        bool first = true, fresh = POLL_FIRST;
        const long long tstart = wall_clock64();
        for (;;) {
          unsigned f = f0, ab = ab0;
          if (!fresh) {
            f = epoch; ab = 0;
            if (tl >= 0) f = __hip_atomic_load(flags + tl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (lane == 63) ab = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          fresh = false;
          if (__any(lane == 63 && ab == epoch)) { res = 0; break; }
          if (__all(f == epoch)) { res = 1; break; }
          if (first && lane == 0) atomicAdd(ctl + 2, 1u);
          first = false;
          if ((unsigned long long)(wall_clock64() - tstart) >= budget) {
            if (lane == 0) { __hip_atomic_exchange(ctl, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); atomicAdd(ctl + 1, 1u); }
            res = 0; break;
          }
          __builtin_amdgcn_s_sleep(8);
        }
        if (lane == 0) go_sh = res;
      }
      barrier_lds_only();                               // the other waves load v only behind this barrier
      if (go_sh) {
        const long long r = pt * TILE + 2LL * threadIdx.x;
        const Lane<true, true> ln(v, n, r, ksp::D2{ps.x, ps.y});
        const unsigned pp = *reinterpret_cast<const unsigned short *>(rowpat + (r < n ? r : 0));
        double y0, y1;
        ksp::dict_pair_walk<NBT>(pa, sc, sm, (int)(pp & 255u), (int)(pp >> 8), r, ln, y0, y1);
        if (r + 1 < n) {
          __builtin_nontemporal_store(d2{y0, y1}, reinterpret_cast<d2 *>(y + r));
#pragma unroll
          for (int i = 0; i < KT; i++) { const d2 x = PARK == 1 ? park[i * BLOCK] : pv[i]; acc[i] = fma(x.x, y0, acc[i]); acc[i] = fma(x.y, y1, acc[i]); }
          acc[KT] = fma(ps.x, y0, acc[KT]); acc[KT] = fma(ps.y, y1, acc[KT]);
          acc[KT + 1] = fma(y0, y0, acc[KT + 1]); acc[KT + 1] = fma(y1, y1, acc[KT + 1]);
        }
      } else dead = true;
    }
    if (!has) break;
#pragma unroll
    for (int i = 0; i < KT; i++) pv[i] = PARK == 0 ? park[i * BLOCK] : cv[i];
    ps = cs; pt = t;
  }
  if (dead) return;
  put_partials<KT + 2>(acc, KT + 2, partials);
}

// ---- the round reordered ------------------------------------------------------------------------------------------------------------------------
// k_forward_pipe<KT, 0, true> with the work that needs no vector memory moved into the shadow of the store drain, and the neighbour loads moved into the
// panel stream. The hand-off is untouched: sc1 store, every wave's s_waitcnt vmcnt(0), barrier, one lane's flag, wave 0's sc1 polls, the barrier it joins,
// every load of the column an sc1 load. The A-phase is split into A1 (poll, barrier, neighbour loads, walk, y store) and D (the dots of that tile):
//   DEFER:      A1(i - 1) runs in round i and keeps y0, y1; D(i - 1) runs in round i + 1 between the sc1 store of C(i + 1) and the wave's wait for it, from
//               the panel that stayed in pv; behind it, still in front of the wait, panel i comes back from LDS into pv. The last tile's D runs behind the
//               loop. Each lane's sums receive their tiles in the same order as before: same bits.
//   EARLY_PARK: the panel just computed goes to LDS in front of the wait as well (behind the un-park: a lane reads and then writes its own 16 bytes of a
//               column, in program order) instead of behind the flag.
//   LATE:       the last LATE columns of the next tile's panel are issued behind the ten neighbour loads instead of in front of the poll wait, so the walk
//               waits for KT - LATE columns and the walk, the y store and the next C arithmetic run with loads in flight.
// The neighbour loads and the late columns stand under NO branch (a phi of a loaded value is a copy, and a copy is a wait): in a round without a matched
// poll the neighbour loads ask with the out-of-range offset, which reads nothing, so no load of the column is issued in front of the barrier behind the
// matched poll. The row patterns of A1's tile are asked for in front of the panel, as the library kernel does.
// Between a wave's sc1 store and its s_waitcnt vmcnt(0) stand fmas, ds_read and ds_write only.
template <int KT, int LO, int HI>
__device__ __forceinline__ void load_cols(const double *V, long long ld, int n, long long t, bool has, d2 (&xv)[KT])
{
  const long long r = t * TILE + 2LL * threadIdx.x;
  const long long rr = has && r + 1 < n ? r : 0;
#pragma unroll
  for (int i = LO; i < HI; i++) xv[i] = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(V + (long long)i * ld + rr));
}
template <int KT>
__device__ __forceinline__ void tile_dots(const d2 (&xv)[KT], d2 s, double y0, double y1, double (&acc)[KT + 2])
{
#pragma unroll
  for (int i = 0; i < KT; i++) { acc[i] = fma(xv[i].x, y0, acc[i]); acc[i] = fma(xv[i].y, y1, acc[i]); }
  acc[KT] = fma(s.x, y0, acc[KT]); acc[KT] = fma(s.y, y1, acc[KT]);
  acc[KT + 1] = fma(y0, y0, acc[KT + 1]); acc[KT + 1] = fma(y1, y1, acc[KT + 1]);
}
template <int KT, bool DEFER, bool EARLY_PARK, int LATE>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_forward_round(const double *V, long long ld, int n, double *v, double *__restrict__ y, const double *__restrict__ cg, double alpha,
                                                    const unsigned char *__restrict__ rowpat, int npat, ksp::PairArgs pa, const double *__restrict__ pcoef, const unsigned *__restrict__ pmask,
                                                    unsigned *flags, unsigned epoch, unsigned *ctl, double *__restrict__ partials, unsigned long long budget, int hooks)
{
  static_assert(LATE >= 0 && LATE < KT, "columns issued behind the neighbour loads");
  __shared__ double cc[2][KT];
  __shared__ int go_sh;
  double *sc; unsigned *sm;
  fill_tables(pa, pcoef, pmask, npat, sc, sm);
  d2 *park = reinterpret_cast<d2 *>(reinterpret_cast<char *>(dyn_lds) + park_offset(npat, pa.nb)) + threadIdx.x;
  for (int i = threadIdx.x; i < 2 * KT; i += BLOCK) cc[i / KT][i % KT] = -cg[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long ntiles = ((long long)n + TILE - 1) / TILE;
  double acc[KT + 2];
#pragma unroll
  for (int i = 0; i < KT + 2; i++) acc[i] = 0.0;
  d2 pv[KT]; d2 ps = {0.0, 0.0};                      // the panel and the new rows of the tile whose A1 is still to come (DEFER: the panel is one tile behind)
#pragma unroll
  for (int i = 0; i < KT; i++) pv[i] = d2{0.0, 0.0};
  long long pt = -1;
  d2 ds = {0.0, 0.0}; double dy0 = 0.0, dy1 = 0.0;     // DEFER: new rows and y of the tile whose dots are still to come; its panel is pv
  long long dt = -1;
  bool dead = false;
  d2 nv[KT]; d2 ns;
  load_panel<KT>(V, ld, n, v, blockIdx.x, (long long)blockIdx.x < ntiles, nv, ns);
  for (long long t = blockIdx.x;; t += gridDim.x) {
    const bool has = t < ntiles;
    d2 cv[KT]; d2 cs = ns;
#pragma unroll
    for (int i = 0; i < KT; i++) cv[i] = nv[i];
    // ---- C-phase: the arithmetic under NO branch (a lane without rows, or a round without a tile, computes on rows 0, 1 and stores nothing): on a path
    // around it the panel loads would still be pending at the park behind the join, the compiler would count them there, and since the sc1 store counts
    // in vmcnt too the last ds_write of the park would wait for the store they are meant to shadow ----
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
      for (int i = 0; i < KT; i++) { const double c = cc[p][i]; cs.x = fma(c, cv[i].x, cs.x); cs.y = fma(c, cv[i].y, cs.y); }
    cs.x *= alpha; cs.y *= alpha;
    if (has) {
      const long long r = t * TILE + 2LL * threadIdx.x;
      if (r + 1 < n) asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(reinterpret_cast<d2 *>(v + r)), "v"(cs) : "memory");
      if ((hooks & 1) && (blockIdx.x & 1)) for (int q = 0; q < 40; q++) __builtin_amdgcn_s_sleep(127);
    }
    // ---- in the shadow of the drain: D of the tile two rounds back, its successor's panel back from LDS, this round's panel to LDS ----
    __builtin_amdgcn_sched_barrier(0);
    if (DEFER) {
      if (dt >= 0 && !dead && dt * TILE + 2LL * threadIdx.x + 1 < n) tile_dots<KT>(pv, ds, dy0, dy1, acc);
#pragma unroll
      for (int i = 0; i < KT; i++) pv[i] = park[i * BLOCK];      // (the first round reads what nobody wrote and nobody uses)
    }
    if (EARLY_PARK) {
#pragma unroll
      for (int i = 0; i < KT; i++) park[i * BLOCK] = cv[i];
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- publish ----
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave
    __syncthreads();
    if (has && threadIdx.x == 0) __hip_atomic_store(flags + t, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool arun = pt >= 0 && !dead;
    if (!EARLY_PARK) {
#pragma unroll
      for (int i = 0; i < KT; i++) park[i * BLOCK] = cv[i];
    }
    // ---- wave 0's first polls of A1(t - gridDim.x), the row patterns, then every wave's first KT - LATE columns of the next round's tile ----
    long long tl = -1;
    unsigned f0 = epoch, ab0 = 0;
    if (arun && w == 0) {
      const int kb = lane / 3, wh = lane % 3;
      int b = 0; bool isb = false;
#pragma unroll
      for (int k = 0; k < NBT; k++) if (k == kb && k < pa.nb) { b = pa.base[k]; isb = true; }
      if (isb) {
        const int d = (int)(pa.dmask >> kb & 1u);
        long long lo = pt * TILE + b - d, hi = pt * TILE + (TILE - 1) + b + d;
        if (lo < 0) lo = 0;
        if (hi > n - 1) hi = n - 1;
        if (lo <= hi && (lo >> 9) + wh <= (hi >> 9)) tl = (lo >> 9) + wh;
      }
      if (tl == pt) tl = -1;
      if (tl >= 0) f0 = __hip_atomic_load(flags + tl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (lane == 63) ab0 = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const long long r = (arun ? pt : 0) * TILE + 2LL * threadIdx.x;
    const unsigned pp = *reinterpret_cast<const unsigned short *>(rowpat + (r < n ? r : 0));
    __builtin_amdgcn_sched_barrier(0);
    {
      const long long tn = t + gridDim.x, rn = tn * TILE + 2LL * threadIdx.x;
      const bool hn = has && tn < ntiles;
      ns = *reinterpret_cast<const d2 *>(hn && rn + 1 < n ? v + rn : V);
      load_cols<KT, 0, KT - LATE>(V, ld, n, tn, hn, nv);
    }
    __builtin_amdgcn_sched_barrier(0);
    // ---- A1 of the tile of the round before ----
    bool go = false;
    if (arun) {
      if (w == 0) {
        int res;
        bool first = true, fresh = true;
        const long long tstart = wall_clock64();
        for (;;) {
          unsigned f = f0, ab = ab0;
          if (!fresh) {
            f = epoch; ab = 0;
            if (tl >= 0) f = __hip_atomic_load(flags + tl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (lane == 63) ab = __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          fresh = false;
          if (__any(lane == 63 && ab == epoch)) { res = 0; break; }
          if (__all(f == epoch)) { res = 1; break; }
          if (first && lane == 0) atomicAdd(ctl + 2, 1u);
          first = false;
          if ((unsigned long long)(wall_clock64() - tstart) >= budget) {
            if (lane == 0) { __hip_atomic_exchange(ctl, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); atomicAdd(ctl + 1, 1u); }
            res = 0; break;
          }
          __builtin_amdgcn_s_sleep(8);
        }
        if (lane == 0) go_sh = res;
      }
      barrier_lds_only();                               // the other waves load v only behind this barrier
      go = go_sh != 0;
      if (!go) dead = true;
    }
    // the ten neighbour loads (sc1; out of range, reading nothing, unless the poll matched), then the rest of the panel: one block, no branch
    const Lane<true, true> ln(v, n, r, ksp::D2{ps.x, ps.y});
    ksp::D2 xv[NBT]; double edge[NBT];
#pragma unroll
    for (int q = 0; q < NBT; q++) {
      const bool on = go && q < pa.nb;
      const long long i = r + pa.base[q];
      const auto tq = __builtin_amdgcn_raw_buffer_load_b128(ln.rs, ln.off(i, on && i != r), 0, 16); __builtin_memcpy(&xv[q], &tq, 16);
      edge[q] = ln.one(lane == 0 ? i - 1 : i + 2, on && (pa.dmask >> q & 1u) && (lane == 0 || lane == 63));
    }
    if (LATE) { const long long tn = t + gridDim.x; load_cols<KT, KT - LATE, KT>(V, ld, n, tn, has && tn < ntiles, nv); }
    __builtin_amdgcn_sched_barrier(0);
    double y0 = 0.0, y1 = 0.0;
    if (go) {
#pragma unroll
      for (int q = 0; q < NBT; q++) { const bool own = q < pa.nb && pa.base[q] == 0; xv[q].x = own ? ps.x : xv[q].x; xv[q].y = own ? ps.y : xv[q].y; }
      ksp::dict_pair_sums<NBT>(pa, sc, sm, (int)(pp & 255u), (int)(pp >> 8), r, ln, xv, edge, y0, y1);
      if (r + 1 < n) {
        __builtin_nontemporal_store(d2{y0, y1}, reinterpret_cast<d2 *>(y + r));
        if (!DEFER) tile_dots<KT>(pv, ps, y0, y1, acc);
      }
    }
    if (DEFER) { ds = ps; dy0 = y0; dy1 = y1; dt = go ? pt : -1; }
    if (!has) break;
    if (!DEFER) {
#pragma unroll
      for (int i = 0; i < KT; i++) pv[i] = park[i * BLOCK];
    }
    ps = cs; pt = t;
  }
  if (dead) return;
  if (DEFER && dt >= 0 && dt * TILE + 2LL * threadIdx.x + 1 < n) tile_dots<KT>(pv, ds, dy0, dy1, acc);      // the last tile's dots; its panel came back in the last round
  put_partials<KT + 2>(acc, KT + 2, partials);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------
struct Problem { int nx, n, npat; ksp::PairArgs pa; std::vector<double> coef; std::vector<unsigned> mask; std::vector<unsigned char> rowpat; };
static Problem laplacian(int nx)
{
  Problem P; P.nx = nx; P.n = nx * nx * nx; P.npat = 27;
  const int bases[5] = {-nx * nx, -nx, 0, nx, nx * nx};
  P.pa.nb = 5; P.pa.dmask = 1u << 2;
  for (int k = 0; k < 5; k++) P.pa.base[k] = bases[k];
  P.coef.assign(27 * 15, 0.0); P.mask.assign(27, 0u);
  auto cls = [&](int i) { return i == 0 ? 0 : (i == nx - 1 ? 2 : 1); };
  for (int p = 0; p < 27; p++) {
    const int cx = p % 3, cy = p / 3 % 3, cz = p / 9;
    auto put = [&](int cand, double a) { P.coef[p * 15 + cand] = a; P.mask[p] |= 1u << cand; };
    if (cz != 0) put(3 * 0 + 1, -1.0);
    if (cy != 0) put(3 * 1 + 1, -1.0);
    if (cx != 0) put(3 * 2 + 0, -1.0);
    put(3 * 2 + 1, 6.0);
    if (cx != 2) put(3 * 2 + 2, -1.0);
    if (cy != 2) put(3 * 3 + 1, -1.0);
    if (cz != 2) put(3 * 4 + 1, -1.0);
    P.mask[p] |= 1u << 31;                              // fewer than W = 8 entries: the padding step
  }
  P.rowpat.assign(((size_t)P.n + 511) / 512 * 512, 0);
  for (int z = 0; z < nx; z++) for (int yy = 0; yy < nx; yy++) for (int x = 0; x < nx; x++) P.rowpat[((size_t)z * nx + yy) * nx + x] = (unsigned char)(cls(x) + 3 * cls(yy) + 9 * cls(z));
  return P;
}

using Kern = void (*)(const double *, long long, int, double *, double *, const double *, double, const unsigned char *, int, ksp::PairArgs, const double *, const unsigned *, unsigned *, unsigned, unsigned *, double *, unsigned long long, int);
struct Dev { double *B; const unsigned char *rowpat; const double *coef; const unsigned *mask; double *cg, *p3, *p1; unsigned *flags, *ctl; long long ld; int ncu; size_t lds; };
static unsigned g_epoch = 0;

template <int KT>
static void run_k(const Problem &P, const Dev &D, const std::vector<double> &h0, const std::vector<double> &hy0)
{
  const int n = P.n; const long long ld = D.ld;
  double *v = D.B + (long long)KT * ld, *y = D.B + (long long)(KT + 1) * ld;
  const double alpha = 0.999;
  const int g_upd = D.ncu, g_dot = D.ncu * std::max(1, std::min(4, (30 + KT + 1) / (KT + 2))), g_spmv = D.ncu * 32;
  const long long ntiles = ((long long)n + TILE - 1) / TILE;
  const unsigned long long budget = 100000;            // 1 ms of wall time: some 300 times the guide's loaded hop (L->L 2.9 us, handoff-flag 1.9 x)
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  auto three = [&] {
    hipLaunchKernelGGL(k_final<KT>, dim3(g_upd), dim3(BLOCK), 0, 0, D.B, ld, n, v, D.cg, alpha);
    hipLaunchKernelGGL(k_spmv, dim3(g_spmv), dim3(BLOCK), D.lds, 0, n, D.rowpat, P.npat, v, y, P.pa, D.coef, D.mask);
    hipLaunchKernelGGL((k_dots<KT + 1>), dim3(g_dot), dim3(BLOCK), 0, 0, D.B, ld, n, y, D.p3); };
  // the forward launch and the variants of its pipelined form: same arguments, the parked panel behind the tables in dynamic LDS
  struct Var { const char *name; Kern kern; size_t lds; };
  const size_t lds_pipe = park_offset(P.npat, P.pa.nb) + (size_t)KT * BLOCK * sizeof(d2);
  constexpr int H = KT / 2, Q = KT / 4;                 // columns behind the neighbour loads: a half, a quarter, three quarters
  const std::vector<Var> vars = {{"k_forward                         ", k_forward<KT>, D.lds},
                       {"pipe: computed parked, polls first", k_forward_pipe<KT, 0, true>, lds_pipe}, {"pipe: computed parked, polls last ", k_forward_pipe<KT, 0, false>, lds_pipe},
                       {"pipe: waiting parked, polls first ", k_forward_pipe<KT, 1, true>, lds_pipe}, {"pipe: waiting parked, polls last  ", k_forward_pipe<KT, 1, false>, lds_pipe},
                       {"round: as pipe, loads branch-free ", k_forward_round<KT, false, false, 0>, lds_pipe}, {"round: (c) park before the wait   ", k_forward_round<KT, false, true, 0>, lds_pipe},
                       {"round: (a) dots deferred, park aft", k_forward_round<KT, true, false, 0>, lds_pipe}, {"round: (a)+(c)                    ", k_forward_round<KT, true, true, 0>, lds_pipe},
                       {"round: (b) half the panel late    ", k_forward_round<KT, false, false, H>, lds_pipe}, {"round: (a)+(c)+(b) a quarter late  ", k_forward_round<KT, true, true, Q>, lds_pipe},
                       {"round: (a)+(c)+(b) half late      ", k_forward_round<KT, true, true, H>, lds_pipe}, {"round: (a)+(c)+(b) 3 quarters late ", k_forward_round<KT, true, true, KT - Q>, lds_pipe},
                       {"round: (b) a quarter late         ", k_forward_round<KT, false, false, Q>, lds_pipe}, {"round: (b) 3 quarters late        ", k_forward_round<KT, false, false, KT - Q>, lds_pipe},
                       {"round: (b) all but one late       ", k_forward_round<KT, false, false, KT - 1>, lds_pipe},
                       {"round: (a)+(b) a quarter late     ", k_forward_round<KT, true, false, Q>, lds_pipe}, {"round: (a)+(b) half late          ", k_forward_round<KT, true, false, H>, lds_pipe},
                       {"round: (a)+(b) 3 quarters late    ", k_forward_round<KT, true, false, KT - Q>, lds_pipe}, {"round: (a)+(b) all but one late    ", k_forward_round<KT, true, false, KT - 1>, lds_pipe}};
  const int NV = (int)vars.size();
  for (const Var &q : vars) CK(hipFuncSetAttribute((const void *)q.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)q.lds));
  auto fwd = [&](const Var &q, int hooks, unsigned long long bud) {
    hipLaunchKernelGGL(q.kern, dim3(g_upd), dim3(BLOCK), q.lds, 0, D.B, ld, n, v, y, D.cg, alpha, D.rowpat, P.npat, P.pa, D.coef, D.mask, D.flags, ++g_epoch, D.ctl, D.p1, bud, hooks); };
  auto reset = [&] { CK(hipMemcpy(v, h0.data(), sizeof(double) * n, hipMemcpyHostToDevice)); CK(hipMemcpy(y, hy0.data(), sizeof(double) * n, hipMemcpyHostToDevice)); };
  auto sums = [&](const double *p, int grid, int ncols) { std::vector<double> h((size_t)ncols * grid), s(ncols, 0.0); CK(hipMemcpy(h.data(), p, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    for (int c = 0; c < ncols; c++) for (int b = 0; b < grid; b++) s[c] += h[(size_t)c * grid + b]; return s; };
  // ---- results: same bits of v and y, dots to rounding (the pipelined forms add the same products in k_forward's order: their dots equal its dots) ----
  std::vector<double> va(n), ya(n), vb(n), yb(n);
  reset(); three(); CK(hipDeviceSynchronize());
  CK(hipMemcpy(va.data(), v, sizeof(double) * n, hipMemcpyDeviceToHost)); CK(hipMemcpy(ya.data(), y, sizeof(double) * n, hipMemcpyDeviceToHost));
  const std::vector<double> sa = sums(D.p3, g_dot, KT + 2);
  std::vector<double> s_fwd;
  for (const Var &q : vars) {
    hipFuncAttributes fa; CK(hipFuncGetAttributes(&fa, (const void *)q.kern));
    printf("k %2d %s: %d registers, %zu B scratch, %zu B static + %zu B dynamic LDS\n", KT, q.name, fa.numRegs, (size_t)fa.localSizeBytes, (size_t)fa.sharedSizeBytes, q.lds);
    for (int hooks : {0, 1}) {
      unsigned ctl0[4]; CK(hipMemcpy(ctl0, D.ctl, sizeof(ctl0), hipMemcpyDeviceToHost));
      reset(); fwd(q, hooks, hooks ? 100 * budget : budget); CK(hipDeviceSynchronize());
      CK(hipMemcpy(vb.data(), v, sizeof(double) * n, hipMemcpyDeviceToHost)); CK(hipMemcpy(yb.data(), y, sizeof(double) * n, hipMemcpyDeviceToHost));
      unsigned ctl1[4]; CK(hipMemcpy(ctl1, D.ctl, sizeof(ctl1), hipMemcpyDeviceToHost));
      const std::vector<double> sb = sums(D.p1, g_upd, KT + 2);
      if (&q == &vars[0] && !hooks) s_fwd = sb;
      double worst = 0.0;
      for (int c = 0; c < KT + 2; c++) { const double d = fabs(sa[c] - sb[c]) / (fabs(sa[KT + 1]) + 1e-300); if (!(d <= worst)) worst = d; }      // a NaN shows
      printf("k %2d %s %s: v %s, y %s, dots %s k_forward's, largest dot difference %.2e of y.y, waits out of budget %u, aborted %s, polls that had to wait %u of %lld\n", KT, q.name, hooks ? "odd workgroups lag" : "even load       ",
             memcmp(va.data(), vb.data(), sizeof(double) * n) ? "DIFFERS" : "same bits", memcmp(ya.data(), yb.data(), sizeof(double) * n) ? "DIFFERS" : "same bits",
             memcmp(s_fwd.data(), sb.data(), sizeof(double) * sb.size()) ? "DIFFER from" : "equal", worst, ctl1[1] - ctl0[1], ctl1[0] == g_epoch ? "YES" : "no", ctl1[2] - ctl0[2], ntiles);
    }
  }
  // ---- times: the forms alternating, three rounds; then with odd workgroups lagging (one round) ----
  auto time = [&](auto fn, int reps) { for (int r = 0; r < 3; r++) fn(); CK(hipEventRecord(e0)); for (int r = 0; r < reps; r++) fn(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); float ms; CK(hipEventElapsedTime(&ms, e0, e1)); return 1e3 * ms / reps; };
  const int reps = 30;
  unsigned ctl0[4]; CK(hipMemcpy(ctl0, D.ctl, sizeof(ctl0), hipMemcpyDeviceToHost));
  double t3[3]; std::vector<std::array<double, 3>> t1(NV); std::vector<double> tl(NV);
  for (int rep = 0; rep < 3; rep++) { reset(); t3[rep] = time(three, reps); for (int q = 0; q < NV; q++) { reset(); t1[q][rep] = time([&] { fwd(vars[q], 0, budget); }, reps); } }
  for (int q = 0; q < NV; q++) { reset(); tl[q] = time([&] { fwd(vars[q], 1, 100 * budget); }, 5); }
  unsigned ctl1[4]; CK(hipMemcpy(ctl1, D.ctl, sizeof(ctl1), hipMemcpyDeviceToHost));
  reset();
  const double ta = time([&] { hipLaunchKernelGGL(k_final<KT>, dim3(g_upd), dim3(BLOCK), 0, 0, D.B, ld, n, v, D.cg, alpha); }, reps);
  const double tb = time([&] { hipLaunchKernelGGL(k_spmv, dim3(g_spmv), dim3(BLOCK), D.lds, 0, n, D.rowpat, P.npat, v, y, P.pa, D.coef, D.mask); }, reps);
  const double tc = time([&] { hipLaunchKernelGGL((k_dots<KT + 1>), dim3(g_dot), dim3(BLOCK), 0, 0, D.B, ld, n, y, D.p3); }, reps);
  const double mb3 = 8e-6 * n * ((KT + 2) + 2.2 + (KT + 2)), mb1 = 8e-6 * n * ((KT + 2) + 1.2);
  printf("k %2d: three launches %7.1f %7.1f %7.1f us (final update %6.1f, product %5.1f, dot sweep %6.1f alone; %.0f MB: %.2f TB/s), waits out of budget in the timed launches: %s\n",
         KT, t3[0], t3[1], t3[2], ta, tb, tc, mb3, mb3 / std::min({t3[0], t3[1], t3[2]}), ctl1[1] != ctl0[1] ? "SOME" : "none");
  for (int q = 0; q < NV; q++)
    printf("k %2d %s: %7.1f %7.1f %7.1f us (%.0f MB: %.2f TB/s), odd workgroups lagging %7.1f us\n", KT, vars[q].name, t1[q][0], t1[q][1], t1[q][2], mb1, mb1 / std::min({t1[q][0], t1[q][1], t1[q][2]}), tl[q]);
  fflush(stdout);
}

int main(int argc, char **argv)
{
  const int nx = argc > 1 ? atoi(argv[1]) : 216;
  if (nx < 4 || nx % 2) { printf("side must be even and at least 4\n"); return 1; }
  Problem P = laplacian(nx);
  const int n = P.n, KMAX = 30;
  Dev D; D.ld = n;
  { hipDeviceProp_t pr; CK(hipGetDeviceProperties(&pr, 0)); D.ncu = pr.multiProcessorCount; }
  const long long ntiles = ((long long)n + TILE - 1) / TILE;
  if ((long long)nx * nx / TILE + 2 > D.ncu) { printf("the far neighbours would be more than one round away\n"); return 1; }
  CK(hipMalloc(&D.B, sizeof(double) * D.ld * (KMAX + 2)));
  unsigned char *rp; double *cf; unsigned *mk;
  CK(hipMalloc(&rp, P.rowpat.size())); CK(hipMalloc(&cf, sizeof(double) * P.coef.size())); CK(hipMalloc(&mk, sizeof(unsigned) * P.mask.size()));
  CK(hipMemcpy(rp, P.rowpat.data(), P.rowpat.size(), hipMemcpyHostToDevice)); CK(hipMemcpy(cf, P.coef.data(), sizeof(double) * P.coef.size(), hipMemcpyHostToDevice)); CK(hipMemcpy(mk, P.mask.data(), sizeof(unsigned) * P.mask.size(), hipMemcpyHostToDevice));
  D.rowpat = rp; D.coef = cf; D.mask = mk; D.lds = P.npat * (15 * sizeof(double) + sizeof(unsigned));
  CK(hipMalloc(&D.cg, sizeof(double) * 2 * 64)); CK(hipMalloc(&D.p3, sizeof(double) * 40 * 4096)); CK(hipMalloc(&D.p1, sizeof(double) * 40 * 4096));
  CK(hipMalloc(&D.flags, sizeof(unsigned) * (ntiles + 16))); CK(hipMemset(D.flags, 0, sizeof(unsigned) * (ntiles + 16)));
  CK(hipMalloc(&D.ctl, 64)); CK(hipMemset(D.ctl, 0, 64));
  std::vector<double> h(n), hy(n, NAN);
  for (int c = 0; c < KMAX; c++) { for (int i = 0; i < n; i++) h[i] = 1e-3 * (double)(((size_t)c * n + i) * 2654435761ull % 1000) - 0.5; CK(hipMemcpy(D.B + (long long)c * D.ld, h.data(), sizeof(double) * n, hipMemcpyHostToDevice)); }
  for (int i = 0; i < n; i++) h[i] = 1e-3 * (double)((size_t)i * 40503ull % 1000) - 0.5;
  printf("step_forward: %d^3 Laplacian, n = %d, %lld tiles of 512 rows, %d CUs, one workgroup per CU in the update and the forward launch\n", nx, n, ntiles, D.ncu);
  {
    hipFuncAttributes fa; CK(hipFuncGetAttributes(&fa, (const void *)k_forward<30>)); int occ = 0; CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_forward<30>, BLOCK, D.lds));
    printf("k_forward<30>: %d registers, %zu B scratch, %zu B static LDS, %d workgroups per CU admitted\n", fa.numRegs, (size_t)fa.localSizeBytes, (size_t)fa.sharedSizeBytes, occ);
  }
  auto coefs = [&](int k) { std::vector<double> c(2 * k); for (int i = 0; i < 2 * k; i++) c[i] = (i < k ? 1e-2 : 1e-9) * (double)(i % 7 - 3); CK(hipMemcpy(D.cg, c.data(), sizeof(double) * c.size(), hipMemcpyHostToDevice)); };
  coefs(16); run_k<16>(P, D, h, hy);
  coefs(23); run_k<23>(P, D, h, hy);
  coefs(30); run_k<30>(P, D, h, hy);
  return 0;
}
