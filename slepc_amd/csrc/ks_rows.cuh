// The row walks of the stored layouts: how a kernel finds its rows, brings a row's entries in and decodes them, and the host-side grid of each walk.
// The kernels of ks_spmv.hip (y = A x, and the product inside the dot sweep) and ks_spmm.hip (Y = A X, every column bit for bit the single-vector
// product) take these pieces from here; what stays with a kernel is what is tuned per kernel: how many entries it keeps in flight, its fma chains and
// its stores. ks_mat.hip builds the layouts and shares the storage rules (CW_PAD, sell_pos).
// Pieces that load from memory inside a tuned loop are MACROS, not inline functions: as functions (by value, by reference, returning a struct) they made
// the compiler schedule those loops differently (scripts/isa_diff.py against the kernels they were taken from); the macro is the same text in place.
#pragma once
#include "ks_sweeps.cuh"
#include <algorithm>

namespace ksr {

typedef int ks_i2v __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void ks_lds_void;          // operands of __builtin_amdgcn_global_load_lds (LDS-DMA)
typedef const __attribute__((address_space(1))) void ks_glb_void;
constexpr int ROW_BLOCK = 256;                             // lane = row kernels: rows of a workgroup
constexpr int CW_PAD = 8;                                  // CSR col / val allocations are this much longer than nnz (what a chunk load may read past its end)

template <int BLOCK, typename T>
__device__ __forceinline__ void lds_fill(T *dst, const T *src, int n) { for (int i = threadIdx.x; i < n; i += BLOCK) dst[i] = src[i]; }

// ---- which rows ----------------------------------------------------------------------------------------------------------------------
// lane = row, groups of `block` rows. Workgroups b, b+8, b+16, ... run on the same XCD (round-robin dispatch). With xcd_remap (grid a multiple of 8)
// each XCD walks ONE contiguous eighth of the row groups, so that the x entries its rows share (the +-nx, +-nx*ny neighbours of a stencil) are
// fetched into that XCD's L2 once instead of into all eight: for (g = g0 + lb; g < g1; g += nb).
struct RowGroups { long long g0, g1, lb, nb; };
__device__ __forceinline__ RowGroups row_groups_xcd(int nrows, int block, int xcd_remap)
{
  const long long groups = ((long long)nrows + block - 1) / block;
  RowGroups q = {0, groups, blockIdx.x, gridDim.x};
  if (xcd_remap) {
    const long long gper = (groups + 7) / 8;
    q.g0 = (blockIdx.x % 8) * gper; q.g1 = q.g0 + gper < groups ? q.g0 + gper : groups;
    q.lb = blockIdx.x / 8; q.nb = gridDim.x / 8;
  }
  return q;
}
// a wave per 64 rows, groups of 256 rows: one per workgroup and iteration; with xcd_remap each XCD takes one contiguous eighth of them
// (k_spmv_csr_wave keeps the same lines in place: this function changes its register allocation)
struct WaveGroups { int g, gend, gstep; };
__device__ __forceinline__ WaveGroups wave_groups_xcd(int n, int xcd_remap)
{
  const int NG = (n + 255) / 256;
  int g, gend, gstep;
  if (xcd_remap) {
    const int xcd = blockIdx.x & 7, li = blockIdx.x >> 3, lc = gridDim.x >> 3;
    g = (int)((long long)NG * xcd / 8) + li; gend = (int)((long long)NG * (xcd + 1) / 8); gstep = lc;
  } else { g = blockIdx.x; gend = NG; gstep = gridDim.x; }
  return {g, gend, gstep};
}

// ---- CSR row blocks: the wave's 64 rows and their one contiguous run of entries ------------------------------------------------------------
struct CwRows { int p0, p1, E0, E1; long long r; bool has; };
__device__ __forceinline__ CwRows cw_rows(int n, const int *__restrict__ rp, int g, int w, int lane)
{
  CwRows q; q.p0 = q.p1 = q.E0 = q.E1 = 0; q.has = false;
  const long long r0 = (long long)g * 256 + (long long)w * 64;
  q.r = r0 + lane;
  if (r0 >= n) return q;
  q.has = q.r < n;
  if (q.has) { ks_i2v pp; __builtin_memcpy(&pp, rp + q.r, sizeof(pp)); q.p0 = pp.x; q.p1 = pp.y; }       // rp[r], rp[r + 1]: one 8-byte load (4-byte aligned)
  q.E0 = rp[r0]; q.E1 = rp[r0 + 64 < n ? r0 + 64 : n];                 // the wave's run of entries (uniform: scalar loads)
  return q;
}
// One chunk of CH entries from e0 (a multiple of four: 16-byte aligned in both streams) straight into the wave's pieces of LDS: CH / 128 LDS-DMA
// instructions for the values (lane l of instruction i brings entries 128 i + 2 l, + 1), CH / 256 for the columns (256 i + 4 l .. + 3), into a
// lane-linear image (the DMA's destination is base + lane x 16). Returns with the chunk in LDS.
template <int CH>
__device__ __forceinline__ void cw_dma_chunk(double *sa, int *sc, const int *col, const double *val, int e0, int E1, int lane)
{
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              // the row lanes' reads of the previous chunk are done before this one may land
#pragma unroll
  for (int i = 0; i < CH / 128; i++) {
    const int e = e0 + 128 * i + 2 * lane;
    if (e < E1) __builtin_amdgcn_global_load_lds((ks_glb_void *)(val + e), (ks_lds_void *)(sa + 128 * i), 16, 0, 2);       // aux 2 = nt: the default policy cost 10 % (profiles/r04_csr_lds_dma.txt)      // may take one entry past E1: CW_PAD
  }
#pragma unroll
  for (int i = 0; i < CH / 256; i++) {
    const int e = e0 + 256 * i + 4 * lane;
    if (e < E1) __builtin_amdgcn_global_load_lds((ks_glb_void *)(col + e), (ks_lds_void *)(sc + 256 * i), 16, 0, 2);      // up to three past E1: CW_PAD
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // an LDS-DMA is a pending LDS write on the VM counter
}

// ---- SELL-64: entries in pairs, a slice of odd width keeps its last entry as a column of singles behind its pairs ------------------------------
__device__ __forceinline__ long long sell_pos(long long sbase, int w, int j, int lane)
{
  return (j | 1) < w ? sbase + (long long)(j >> 1) * 128 + lane * 2 + (j & 1) : sbase + (long long)(w >> 1) * 128 + lane;
}
// the workgroup's first group of four slices. Blocks b, b+8, ... share an XCD: with xcd_remap each XCD gets one contiguous range of slice groups
__device__ __forceinline__ long long sell_first_group(long long nblk, int xcd_remap)       // nblk: the grid
{
  long long b = blockIdx.x;
  if (xcd_remap) {
    const long long per = nblk / 8;
    if (b < per * 8) b = (b % 8) * per + b / 8;
  }
  return b;
}
// pairs q .. q + UNR - 1 of the lane's row into c[UNR] (ks_i2v), a[UNR] (ks_d2v); wp pairs in the slice, len entries in the row. Fully predicated: all
// loads of a batch are independent
#define KS_SELL_LOAD_PAIRS(UNR, c, a, col, val, sb, q, wp, len, lane)                                                             \
  _Pragma("unroll") for (int u = 0; u < (UNR); u++) {                                                                              \
    const int j = 2 * ((q) + u);                                                                                                   \
    const bool ok = (q) + u < (wp) && j < (len);                                                                                   \
    const long long p = (sb) + (long long)((q) + u) * 128 + (lane) * 2;                                                            \
    c[u] = ok ? __builtin_nontemporal_load(reinterpret_cast<const ks_i2v *>((col) + p)) : ks_i2v{-1, -1};                          \
    a[u] = ok ? __builtin_nontemporal_load(reinterpret_cast<const ksk::ks_d2v *>((val) + p)) : ksk::ks_d2v{0.0, 0.0};              \
    if (j + 1 >= (len)) { c[u].y = -1; a[u].y = 0.0; }         /* the pair's second slot is padding: never gathered, never multiplied */ \
  }
struct SellEntry { int c; double a; };                     // c < 0: padding (a = 0.0, x is not gathered)
__device__ __forceinline__ SellEntry sell_tail(const int *col, const double *val, long long sb, int w, int len, int lane)
{
  const bool ok = w - 1 < len;                              // the last entry slot of a slice of odd width w: singles
  const long long p = sb + (long long)(w >> 1) * 128 + lane;
  return {ok ? ksk::ldstream(col + p) : -1, ok ? ksk::ldstream(val + p) : 0.0};
}

// ---- dictionary ELL: W 2-byte codes per row (offset code, value code; value code 255 marks padding), or one byte per row into a table of such words --
extern __shared__ __attribute__((aligned(16))) uint4 dict_pat_lds[];          // row-pattern form: npat code words of W / 8 uint4 each
// the preamble of the layout's kernels (k_dot_spmv_dict keeps the same lines in place: through the macro its sweep loop is scheduled differently): values, offsets and (row-pattern form) the table of code words into LDS (sv, so: the kernel's __shared__ arrays)
#define KS_DICT_LDS_FILL(BLOCK, W, sv, so, dval, nval, doff, noff, rowpat, pats, npat)                                            \
  do {                                                                                                                             \
    for (int i = threadIdx.x; i < (nval); i += (BLOCK)) sv[i] = dval[i];                                                           \
    for (int i = threadIdx.x; i < (noff); i += (BLOCK)) so[i] = doff[i];                                                           \
    if (rowpat) for (int i = threadIdx.x; i < (npat) * ((W) / 8); i += (BLOCK)) dict_pat_lds[i] = pats[i];                         \
    __syncthreads();                                                                                                               \
  } while (0)
// entry e < 8 of the four words of a uint4 of codes: offset code, value code; ok = false: padding - its value and its x count as 0.0 and are not loaded,
// the chain still runs fma(0.0, 0.0, acc) there, in every kernel of the layout
struct DictCode { unsigned oc, vc; bool ok; };
__device__ __forceinline__ DictCode dict_code(unsigned word, int e)          // word = wds[e >> 1]
{
  const unsigned code = (word >> ((e & 1) * 16)) & 0xffffu;
  return {code & 0xffu, code >> 8, (code >> 8) != 255u};
}
// offset-dictionary ELL: entry e of the 1-byte codes packed in 32-bit words; word = wds[e >> 2]. Code 255 = padding, as above
__device__ __forceinline__ DictCode odict_code(unsigned word, int e)
{
  const unsigned oc = (word >> ((e & 3) * 8)) & 0xffu;
  return {oc, 0u, oc != 255u};
}
// one row from its code word: decode, gather, fma chain from 0.0 in entry order, padding included - the single-vector kernels of the layout (k_spmv_dict, k_dot_spmv_dict) go through here
template <int W>
__device__ __forceinline__ double dict_word_row(const uint4 (&c)[W / 8], long long r, const double *sv, const int *so, const double *x)
{
  double a[W], xv[W];
#pragma unroll
  for (int q = 0; q < W / 8; q++) {
    const unsigned wds[4] = {c[q].x, c[q].y, c[q].z, c[q].w};
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const DictCode d = dict_code(wds[e >> 1], e);
      a[q * 8 + e] = d.ok ? sv[d.vc] : 0.0;
      xv[q * 8 + e] = d.ok ? x[r + so[d.oc]] : 0.0;
    }
  }
  double acc = 0.0;
#pragma unroll
  for (int e = 0; e < W; e++) acc = fma(a[e], xv[e], acc);
  return acc;
}

// ---- the pair form of the row-pattern form (ks_dict_pairs.h: the walk itself, ksp::dict_pair_walk, and its plan) ------------------------------------
// how a lane of the walk reaches x and its neighbours on the device. Loads go through a buffer descriptor of exactly [x, x + n): an element outside it
// is 0.0 by the hardware's range check (per dword: the pair at n - 1 of an odd n has its first half), no memory access is made for it and no branch stands
// between two loads. An index outside [0, n) is sent to PAIR_OOB_OFFSET, which lies past the end of every descriptor the launch admits (pair_fits32: 8 n <=
// PAIR_OOB_OFFSET), so nothing rests on the 32-bit offset wrapping. The shift is ds_bpermute through __shfl_up / __shfl_down: the wave's first and last lane get their own
// value back and do not use it.
constexpr unsigned PAIR_OOB_OFFSET = 0xfffffff0u;
struct PairLane {
  __amdgpu_buffer_rsrc_t rs; long long n;
  __device__ __forceinline__ PairLane(const double *x, long long n_) : rs(__builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(x), 0, (int)(unsigned)(n_ * 8), 0x00020000)), n(n_) {}
  __device__ __forceinline__ unsigned off(long long i, bool want = true) const { return want && (unsigned long long)i < (unsigned long long)n ? (unsigned)(i * 8) : PAIR_OOB_OFFSET; }
  __device__ __forceinline__ int lane() const { return threadIdx.x & 63; }
  __device__ __forceinline__ ksp::D2 pair(long long i) const { ksp::D2 v; const auto t = __builtin_amdgcn_raw_buffer_load_b128(rs, off(i), 0, 0); __builtin_memcpy(&v, &t, 16); return v; }
  __device__ __forceinline__ double one(long long i, bool want) const { double v; const auto t = __builtin_amdgcn_raw_buffer_load_b64(rs, off(i, want), 0, 0); __builtin_memcpy(&v, &t, 8); return v; }
  __device__ __forceinline__ double up(double v, long long) const { return __shfl_up(v, 1); }
  __device__ __forceinline__ double down(double v, long long) const { return __shfl_down(v, 1); }
};
// the plan's tables into dynamic LDS (in place of the pattern table, which the pair walk does not read): coefficients, then masks
#define KS_PAIR_LDS_FILL(BLOCK, pa, coef, mask, npat, sc, sm)                                                                      \
  double *sc = reinterpret_cast<double *>(dict_pat_lds);                                                                           \
  unsigned *sm = reinterpret_cast<unsigned *>(sc + (npat) * 3 * (pa).nb);                                                          \
  do {                                                                                                                             \
    for (int i = threadIdx.x; i < (npat) * 3 * (pa).nb; i += (BLOCK)) sc[i] = coef[i];                                             \
    for (int i = threadIdx.x; i < (npat); i += (BLOCK)) sm[i] = mask[i];                                                           \
    __syncthreads();                                                                                                               \
  } while (0)
// the two pattern indices of rows r, r + 1 (r even) in one 2-byte load. rowpat is padded to a multiple of 256 rows, so r < n has both bytes; a lane
// past the last row reads the first pair instead (any valid pattern: its results are dropped) - no branch in front of the loads of x
__device__ __forceinline__ void pair_patterns(const unsigned char *__restrict__ rowpat, long long r, long long n, int &p0, int &p1)
{
  const unsigned pp = *reinterpret_cast<const unsigned short *>(rowpat + (r < n ? r : 0));
  p0 = (int)(pp & 255u); p1 = (int)(pp >> 8);
}
// ---- block CSR (KS_MAT_LAYOUT_BSR): the wave's block rows, its one contiguous run of blocks, and the walk both products share -------------------------
// wave_groups_xcd for groups that are not 256 rows: NG groups, with xcd_remap each XCD one contiguous eighth of them
__device__ __forceinline__ WaveGroups group_range_xcd(int NG, int xcd_remap)
{
  if (xcd_remap) {
    const int xcd = blockIdx.x & 7, li = blockIdx.x >> 3, lc = gridDim.x >> 3;
    return {(int)((long long)NG * xcd / 8) + li, (int)((long long)NG * (xcd + 1) / 8), lc};
  }
  return {(int)blockIdx.x, NG, (int)gridDim.x};
}
// wave w of group g owns 64 / BS block rows: lane = scalar row (lanes past 64 / BS * BS idle). p0, p1: the lane's block row in the block stream;
// B0, B1: the wave's run of blocks (uniform)
struct BsrRows { int p0, p1, B0, B1; long long r; bool has; };
template <int BS>
__device__ __forceinline__ BsrRows bsr_rows(int nb, const int *__restrict__ brp, int g, int w, int lane)
{
  constexpr int R = bsr_wave_rows(BS);
  BsrRows q; q.p0 = q.p1 = q.B0 = q.B1 = 0; q.r = 0; q.has = false;
  const long long I0 = (long long)g * (4 * R) + (long long)w * R;
  if (I0 >= nb) return q;
  const long long I = I0 + lane / BS;
  q.has = lane < R * BS && I < nb;
  q.r = I * BS + lane % BS;
  if (q.has) { ks_i2v pp; __builtin_memcpy(&pp, brp + I, sizeof(pp)); q.p0 = pp.x; q.p1 = pp.y; }
  q.B0 = brp[I0]; q.B1 = brp[I0 + R < nb ? I0 + R : nb];
  return q;
}
// a chunk of NBK blocks from block b0 in registers: the values as STEPS 16-byte nontemporal loads per lane from the even scalar at or below the chunk's
// first (lane l of step u: scalars 128 u + 2 l, + 1; may take one scalar past the run: CW_PAD), and the block column of each (block, c) item the lane
// gathers x for (item t = 64 u + l: block t / BS, column t % BS; the BS lanes of a block read one address), -1 where there is none
template <int BS, int NBK> struct BsrRegs {
  static constexpr int STEPS = (NBK * BS * BS + (BS & 1) + 127) / 128, U = (NBK * BS + 63) / 64;
  ksk::ks_d2v a[STEPS]; int c[U];
};
template <int BS, int NBK>
__device__ __forceinline__ void bsr_load(BsrRegs<BS, NBK> &r, const int *__restrict__ bcol, const double *__restrict__ val, int b0, int B1, int lane)
{
  const int e0 = (b0 * BS * BS) & ~1, E1 = B1 * BS * BS;
#pragma unroll
  for (int u = 0; u < BsrRegs<BS, NBK>::STEPS; u++) {
    const int e = e0 + 128 * u + 2 * lane;
    r.a[u] = e < E1 ? __builtin_nontemporal_load(reinterpret_cast<const ksk::ks_d2v *>(val + e)) : ksk::ks_d2v{0.0, 0.0};
  }
#pragma unroll
  for (int u = 0; u < BsrRegs<BS, NBK>::U; u++) {
    const int t = 64 * u + lane, j = t / BS;
    r.c[u] = (t < NBK * BS && b0 + j < B1) ? bcol[b0 + j] : -1;
  }
}
// The walk (k_spmv_bsr: KB = 1; k_spmm_bsr: KB = 4 or 8 accumulators per lane, kb <= KB columns live). k_spmv_csr_wave's software pipeline with blocks
// in place of entries: the chunk in `cur` is parked in the wave's own LDS - values as they came, x gathered once per (block, c) and column of the pass,
// KB values side by side - the NEXT chunk's loads (of the same block rows, or the first chunk of the wave's next block rows) are issued, then lane =
// scalar row i runs acc = fma(blk(i, c), x, acc) over its block row's blocks of the chunk, c ascending: the expansion's entry order, from 0.0. LDS
// operations of one wave execute in order: no workgroup barrier anywhere. sa: 128 STEPS doubles, sx: NBK BS KB doubles, both the wave's own.
template <int BS, int KB, int NBK>
__device__ __forceinline__ void bsr_walk(double *sa, double *sx, int nb, const int *__restrict__ brp, const int *__restrict__ bcol, const double *__restrict__ val,
                                         const double *__restrict__ X, long long ldx, double *__restrict__ Y, long long ldy, int kb, int xcd_remap)
{
  typedef BsrRegs<BS, NBK> Regs;
  constexpr int B2 = BS * BS, GR = bsr_group_rows(BS);
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const WaveGroups wg = group_range_xcd((nb + GR - 1) / GR, xcd_remap);
  int g = wg.g;
  const int gend = wg.gend, gstep = wg.gstep;
  if (g >= gend) return;
  BsrRows cu = bsr_rows<BS>(nb, brp, g, w, lane);
  BsrRows nx = g + gstep < gend ? bsr_rows<BS>(nb, brp, g + gstep, w, lane) : BsrRows{0, 0, 0, 0, 0, false};
  Regs cur, nxt;
  int b0 = cu.B0;
  if (b0 < cu.B1) bsr_load<BS, NBK>(cur, bcol, val, b0, cu.B1, lane);
  bool nxt_loaded = false;                                 // the first chunk of group nx is already in `nxt`
  const int i = lane % BS;
  double acc[KB];
#pragma unroll
  for (int k = 0; k < KB; k++) acc[k] = 0.0;
  for (;;) {
    if (b0 < cu.B1) {
#pragma unroll
      for (int u = 0; u < Regs::STEPS; u++) *reinterpret_cast<ksk::ks_d2v *>(sa + 128 * u + 2 * lane) = cur.a[u];
      double xg[Regs::U][KB];
#pragma unroll
      for (int u = 0; u < Regs::U; u++) {
        const long long xi = (long long)cur.c[u] * BS + (64 * u + lane) % BS;
#pragma unroll
        for (int k = 0; k < KB; k++) xg[u][k] = (cur.c[u] >= 0 && k < kb) ? X[k * ldx + xi] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < Regs::U; u++) {
        const int t = 64 * u + lane;
        if (t < NBK * BS) {
#pragma unroll
          for (int k = 0; k < KB; k++) sx[t * KB + k] = xg[u][k];
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int bn = b0 + NBK;
      if (bn < cu.B1) bsr_load<BS, NBK>(nxt, bcol, val, bn, cu.B1, lane);
      else if (nx.B0 < nx.B1) { bsr_load<BS, NBK>(nxt, bcol, val, nx.B0, nx.B1, lane); nxt_loaded = true; }
      const int lo = max(cu.p0, b0), hi = min(cu.p1, bn);
      const double *av = sa + ((b0 * B2) & 1) + i * BS;
      for (int p = lo; p < hi; p++) {
        const double *ap = av + (p - b0) * B2, *xp = sx + (p - b0) * BS * KB;
#pragma unroll
        for (int c = 0; c < BS; c++) {
          const double a = ap[c];
#pragma unroll
          for (int k = 0; k < KB; k++) acc[k] = fma(a, xp[c * KB + k], acc[k]);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (bn < cu.B1) { cur = nxt; b0 = bn; continue; }
    }
    // this wave's block rows are complete
    if (cu.has) {
#pragma unroll
      for (int k = 0; k < KB; k++) if (k < kb) __builtin_nontemporal_store(acc[k], Y + k * ldy + cu.r);
    }
#pragma unroll
    for (int k = 0; k < KB; k++) acc[k] = 0.0;
    g += gstep;
    if (g >= gend) break;
    cu = nx;
    nx = g + gstep < gend ? bsr_rows<BS>(nb, brp, g + gstep, w, lane) : BsrRows{0, 0, 0, 0, 0, false};
    b0 = cu.B0;
    if (nxt_loaded) cur = nxt;
    else if (b0 < cu.B1) bsr_load<BS, NBK>(cur, bcol, val, b0, cu.B1, lane);
    nxt_loaded = false;
  }
}
#define KS_BSR_SWITCH(bs, F) \
  switch (bs) { case 2: F(2); break; case 3: F(3); break; case 4: F(4); break; case 5: F(5); break; case 6: F(6); break; case 7: F(7); break; default: F(8); break; }

// ---- host side: the grid of each walk, the LDS of the pattern table, the bytes a layout must move ----------------------------------------------------
struct LaunchGrid { unsigned blocks; int remap; };
static inline LaunchGrid dict_launch_grid(ks_mat A, int rows_per_lane = 1)   // dictionary forms: up to 64 workgroups per CU (the pair form, rows_per_lane = 2: groups of 512 rows)
{
  const long long gr = (long long)ROW_BLOCK * rows_per_lane, groups = ((long long)A->n + gr - 1) / gr;
  // the pair form: up to 32 per CU - its tables are 3 KB of LDS to fill per workgroup (216^3 Laplacian: 38.3 us with 64, 34.6 with 32, 41.6 with 16:
  // profiles/r14_dict_pairs.txt)
  long long nblk = std::max<long long>(1, std::min<long long>(groups, (long long)A->ctx->num_cu * (rows_per_lane == 2 ? 32 : 64)));
  const int remap = nblk >= 64 ? 1 : 0;                   // small matrices: nothing to pin
  if (remap) nblk = std::min<long long>((nblk + 7) / 8, (groups + 7) / 8) * 8;
  return {(unsigned)nblk, remap};
}
static inline LaunchGrid sell_launch_grid(ks_mat A)
{
  const long long groups = ((long long)A->nslices + 3) / 4;
  const long long blocks = std::min<long long>(groups, (long long)A->ctx->num_cu * 4096);     // one 256-row group per block measured fastest
  // each XCD one contiguous range of slices (179 -> 172 us on the 216^3 Laplacian), only with one slice group per workgroup (a strided
  // loop would interleave the ranges again)
  return {(unsigned)std::max<long long>(blocks, 1), (blocks == groups && blocks >= 64) ? 1 : 0};
}
static inline LaunchGrid csr_wave_launch_grid(ks_mat A, int per_cu)     // per_cu workgroups of four waves per CU (the kernel's launch bounds); a multiple of 8 so that every XCD gets its eighth of the rows
{
  long long nb = std::min<long long>(((long long)A->n + 255) / 256, (long long)A->ctx->num_cu * per_cu);
  const int remap = nb >= 64 ? 1 : 0;
  if (remap) nb = (nb / 8) * 8;
  return {(unsigned)nb, remap};
}
static inline LaunchGrid window_launch_grid(ks_mat A)              // windowed CSR: a workgroup per block of WIN_ROWS rows (one barrier per block and none between blocks); eight or more blocks per XCD: every XCD one contiguous eighth
{
  const long long nb = std::max<long long>(1, A->wn_blocks);
  const int remap = nb >= 64 ? 1 : 0;
  return {(unsigned)(remap ? (nb + 7) / 8 * 8 : nb), remap};
}
static inline LaunchGrid bsr_launch_grid(ks_mat A, int per_cu)      // block CSR: per_cu workgroups of four waves per CU, a group of bsr_group_rows block rows per step; a multiple of 8 as for the CSR row blocks
{
  const int gr = bsr_group_rows(A->bsr_bs);
  long long nb = std::min<long long>(((long long)A->bsr_nb + gr - 1) / gr, (long long)A->ctx->num_cu * per_cu);
  const int remap = nb >= 64 ? 1 : 0;
  if (remap) nb = (nb / 8) * 8;
  return {(unsigned)nb, remap};
}
static inline size_t dict_pair_lds_bytes(ks_mat A) { return (size_t)A->dict_npat * (3 * A->pr_args.nb * sizeof(double) + sizeof(unsigned)); }   // the pair form's tables instead
static inline bool pair_aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }
static inline bool pair_fits32(long long n) { return n * 8 <= (long long)PAIR_OOB_OFFSET; }        // the descriptor's 32-bit size, and PAIR_OOB_OFFSET stays outside it
static inline size_t dict_pattern_lds_bytes(ks_mat A) { return A->layout == KS_MAT_LAYOUT_DICT && A->dc_rowpat ? (size_t)A->dict_npat * A->dict_w * 2 : 0; }   // dynamic LDS: the pattern table beside the dictionaries
// compulsory bytes of the stored diagonal block per product (the matrix part of a KsProfScope byte model: callers add their x / y traffic)
static inline double layout_own_bytes(ks_mat A)
{
  switch (A->layout) {
  case KS_MAT_LAYOUT_BINNED: return 28.0 * A->bn_entries;
  case KS_MAT_LAYOUT_DICT: return (A->dc_rowpat ? 1.0 : 2.0 * A->dict_w) * A->n;            // one byte per row in the row-pattern form
  case KS_MAT_LAYOUT_ODICT: return 8.0 * A->nnz_d + (double)A->dict_w * A->n;
  case KS_MAT_LAYOUT_SELL: return 12.0 * A->s_entries + 4.0 * A->n;
  case KS_MAT_LAYOUT_WINDOW:                                                                   // values + codes or columns, row pointers, every window filled once, the segment lists and the two per-block tables
    return 10.0 * A->wn_entries + 12.0 * A->wn_direct_entries + 4.0 * (A->n + 1) + 512.0 * A->wn_segments + 4.0 * A->wn_segments + 8.0 * A->wn_blocks;
  case KS_MAT_LAYOUT_BSR: return (8.0 * A->bsr_bs * A->bsr_bs + 4.0) * A->bsr_blocks + 4.0 * (A->bsr_nb + 1);      // values, one column per block, one pointer per block row
  default: return 12.0 * A->nnz_d + 4.0 * (A->n + 1);                                       // the CSR stream
  }
}
#define KS_DICT_W_SWITCH(w, F) do { if ((w) == 8) { F(8); } else if ((w) == 32) { F(32); } else { F(16); } } while (0)

} // namespace ksr
