// MatMult(AIJ): CSR sparse matrix-vector product for gfx950.
//
// Replaces PETSc MatMult_SeqAIJ / MatMult_MPIAIJ as reached from BVMatMultColumn
// (src/sys/classes/bv/interface/bvops.c:862-885) through MatMult_STOperator / STApply_Generic
// (src/sys/classes/st/interface/stsolve.c:16-25,244-259).
//
// Layout in HBM (PETSc MPIAIJ style): the rank's row block is split into a "diagonal" block whose
// columns are owned by this rank (stored with LOCAL column indices) and an "off-diagonal" block
// whose columns live on other ranks (stored with compressed GHOST indices). rowptr int32[n+1],
// col int32[nnz], val f64[nnz]. x, y are columns of the BV (contiguous, stride 1).
//
// Kernel: "CSR-vector with sub-wave row groups". G = 2^g lanes cooperate on one row (G chosen from
// the mean row length: 8 for the 7-point Laplacian, 32 for ~32 nnz/row), so a 64-wide wavefront
// streams 64/G consecutive rows whose val/col entries are contiguous in memory: the val (8 B/lane)
// and col (4 B/lane) loads of a wave are one coalesced segment. Partial products are combined with
// DPP/shuffle butterflies inside the group. Each thread keeps UNROLL independent rows in flight
// so that rowptr -> (col,val) -> x[col] dependent chains of different rows overlap.
// Algorithmic bytes per call: 12*nnz + 4*(n+1) + 16*n.
#include "ks_rows.cuh"
#include "ks_csr.h"

namespace {
using namespace ksr;

constexpr int SPMV_BLOCK = ROW_BLOCK;

template <int G>
__device__ __forceinline__ double group_reduce(double v)
{
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// y[row] (+)= sum_p val[p] * x[col[p]]  over rows handled through an optional compressed row list
template <int G, int UNROLL, bool ACCUM, bool ROWLIST>
__global__ __launch_bounds__(SPMV_BLOCK) void k_spmv_csr(int nrows, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                          const double *__restrict__ val, const double *__restrict__ x,
                                                          double *__restrict__ y, const int *__restrict__ rowlist)
{
  constexpr int GPW = 64 / G;                       // row groups per wavefront
  constexpr int RW = GPW * UNROLL;                  // rows per wavefront per sweep
  const int lane = threadIdx.x & 63;
  const int gi = lane / G, lane_g = lane % G;
  const long long wave = ((long long)blockIdx.x * SPMV_BLOCK + threadIdx.x) >> 6;
  const long long nwaves = ((long long)gridDim.x * SPMV_BLOCK) >> 6;
  // for a fixed u the GPW groups of a wave own GPW CONSECUTIVE rows, so one wave-instruction
  // reads one contiguous run of val/col entries
  for (long long wb = wave * RW; wb < nrows; wb += nwaves * RW) {
    int p0[UNROLL], p1[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      long long r = wb + u * GPW + gi;
      if (r < nrows) { p0[u] = rowptr[r]; p1[u] = rowptr[r + 1]; } else { p0[u] = 0; p1[u] = 0; }
    }
    double s[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      double acc = 0.0;
      for (int p = p0[u] + lane_g; p < p1[u]; p += G) acc = fma(val[p], x[col[p]], acc);
      s[u] = acc;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      double t = group_reduce<G>(s[u]);
      long long r = wb + u * GPW + gi;
      if (lane_g == 0 && r < nrows) {
        long long out = ROWLIST ? rowlist[r] : r;
        if (ACCUM) y[out] += t; else __builtin_nontemporal_store(t, y + out);
      }
    }
  }
}


// ---- CSR, row blocks streamed through LDS, one wave per 64 rows (no workgroup barrier) -------------------------------------------
// The general-matrix kernel: ragged rows, empty rows, rows longer than a chunk; the CSR-vector kernel above keeps the small matrices and
// the compressed off-diagonal block. A wave takes 64 consecutive rows; their entries are ONE contiguous run of col / val, which it
// streams in chunks of 512 with fully coalesced nontemporal loads (lane l of step u loads entry 64 u + l) and parks in a wave-private piece
// of LDS; then lane = row: every lane runs the reference's loop over its own row's segment, acc = fma(val, x, acc) in entry order - the
// bits of the SELL / dictionary kernels. Nothing waits for another wave: LDS operations of one wave execute in order, so the hand-over
// from the loading lanes to the row lanes needs no barrier (the workgroup-per-256-rows form it replaced, since removed, spent four fifths
// of its wave cycles parked at barriers and s_waitcnt, profiles/r03_pmc_csr_kernels.txt), and the col / val loads of the next chunk - of the same rows or of the
// wave's next 64, whose row pointers were loaded one group ahead - are issued before the row sums of this one. Workgroups on one XCD
// (blockIdx % 8) take one contiguous eighth of the rows, so an XCD's L2 holds the part of x its rows gather from.
// ROWSIDE: where x is gathered. false: by the loading lanes (lane = entry), (value, x) pairs go through LDS - every lane has work whatever
// the row lengths. true: by the row lanes (lane = row) - (value, column) go through LDS and the 64 lanes of a gather instruction ask for the
// same entry position of 64 consecutive rows, which for a banded or stencil-like matrix is a few cache lines where the entry-side gather
// touches two to three times as many (216^3 Laplacian: the entry-side gathers cost 35 of 211 us, profiles/r03_csr_wave_variants.txt);
// pays only while a chunk spans most of the wave's rows, i.e. for short rows - which the LDS-DMA form below takes, so the row side of this
// form is reached only through KSGPU_SPMV=csrregs; the entry side is the automatic choice above 16 entries per row on average.
// (16-byte loads of four consecutive entries per lane were tried for the streams: fewer instructions, no faster, and the gathers of such a
// lane assignment touch still more lines.)
// CW_STEPS: 64 entries per step; 8 steps = chunks of 512 (row side with 256-entry chunks: 62 registers, 8 waves per SIMD, and 237 us instead of 199)
__device__ __forceinline__ int cw_slot(int e) { return e + (e >> 5); }     // one slot of skew per 32 entries (rows whose length is a multiple of 32)
// Load width matters more than instruction count here: 4-byte-per-lane streaming loads top out at 0.7 - 2.5 TB/s on this part, 8- and 16-byte
// ones at 7 (scripts/micro/load_width.hip, profiles/r03_micro_load_width.txt). So the 4-byte column indices are loaded two per lane (a chunk
// starts on an even entry: aligned 8-byte loads; lane l of step u holds entries 128 u + 2 l, + 1), the values one per lane (entry 64 u + l),
// and a row's two row pointers come as one 8-byte load.
template <int CW_STEPS> struct CwRegs { ks_i2v c[CW_STEPS / 2]; double a[CW_STEPS]; };
template <int CW_STEPS>
__device__ __forceinline__ void cw_load(CwRegs<CW_STEPS> &r, const int *__restrict__ col, const double *__restrict__ val, int e0, int E1, int lane)
{
#pragma unroll
  for (int u = 0; u < CW_STEPS / 2; u++) {
    const int e = e0 + u * 128 + 2 * lane;
    r.c[u] = e < E1 ? __builtin_nontemporal_load(reinterpret_cast<const ks_i2v *>(col + e)) : ks_i2v{-1, -1};      // may take one entry past E1: CW_PAD
  }
#pragma unroll
  for (int u = 0; u < CW_STEPS; u++) {
    const int e = e0 + u * 64 + lane;
    r.a[u] = e < E1 ? ksk::ldstream(val + e) : 0.0;
  }
}
constexpr int CW_U = 4;                                    // row side: gathers in flight per lane (8: 110 registers, 4 waves per SIMD, 204 us; 2 or 3 at 6 waves per SIMD still spill)
template <bool ROWSIDE, int CW_STEPS>
__global__ __launch_bounds__(256, ROWSIDE ? 5 : 4) void k_spmv_csr_wave(int n, const int *__restrict__ rp, const int *__restrict__ col, const double *__restrict__ val,
                                                       const double *__restrict__ x, double *__restrict__ y, int xcd_remap)
{
  constexpr int CW_CHUNK = 64 * CW_STEPS;
  __shared__ double sa_all[4][CW_CHUNK + CW_CHUNK / 32];
  __shared__ double sb_all[4][ROWSIDE ? (CW_CHUNK + CW_CHUNK / 32) / 2 : CW_CHUNK + CW_CHUNK / 32];       // x values, or the columns (4 bytes each)
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double *sa = sa_all[w], *sx = sb_all[w];
  int *sc = reinterpret_cast<int *>(sb_all[w]);
  const int NG = (n + 255) / 256;                          // groups of 256 rows: as wave_groups_xcd (ks_rows.cuh), in place
  int g, gend, gstep;
  if (xcd_remap) {
    const int xcd = blockIdx.x & 7, li = blockIdx.x >> 3, lc = gridDim.x >> 3;
    g = (int)((long long)NG * xcd / 8) + li; gend = (int)((long long)NG * (xcd + 1) / 8); gstep = lc;
  } else { g = blockIdx.x; gend = NG; gstep = gridDim.x; }
  if (g >= gend) return;
  // Software pipeline over (row group, chunk): while the rows of one chunk are summed, the col / val loads of the NEXT chunk are in
  // flight - the next chunk of the same rows, or the first chunk of the wave's next 64 rows.
  CwRows cu = cw_rows(n, rp, g, w, lane);
  CwRows nx = g + gstep < gend ? cw_rows(n, rp, g + gstep, w, lane) : CwRows{0, 0, 0, 0, 0, false};
  CwRegs<CW_STEPS> cur, nxt;
  int e0 = cu.E0 & ~1;
  if (e0 < cu.E1) cw_load(cur, col, val, e0, cu.E1, lane);
  bool nxt_loaded = false;                                 // the first chunk of group nx is already in `nxt`
  double acc = 0.0;
  for (;;) {
    if (e0 < cu.E1) {
#pragma unroll
      for (int u = 0; u < CW_STEPS; u++) sa[cw_slot(u * 64 + lane)] = cur.a[u];
      if (ROWSIDE) {
#pragma unroll
        for (int u = 0; u < CW_STEPS / 2; u++) { const int sl = cw_slot(u * 128 + 2 * lane); sc[sl] = cur.c[u].x; sc[sl + 1] = cur.c[u].y; }      // 2 l, 2 l + 1 never straddle a skew step
      } else {
        double xg[CW_STEPS];
#pragma unroll
        for (int u = 0; u < CW_STEPS / 2; u++) {
          const int e = e0 + u * 128 + 2 * lane;
          xg[2 * u] = e < cu.E1 ? x[cur.c[u].x] : 0.0; xg[2 * u + 1] = e + 1 < cu.E1 ? x[cur.c[u].y] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < CW_STEPS / 2; u++) { const int sl = cw_slot(u * 128 + 2 * lane); sx[sl] = xg[2 * u]; sx[sl + 1] = xg[2 * u + 1]; }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int en = e0 + CW_CHUNK;
      if (en < cu.E1) cw_load(nxt, col, val, en, cu.E1, lane);
      else if ((nx.E0 & ~1) < nx.E1) { cw_load(nxt, col, val, nx.E0 & ~1, nx.E1, lane); nxt_loaded = true; }
      const int lo = max(cu.p0, e0), hi = min(cu.p1, en);
      if (ROWSIDE) {
        for (int p = lo; __builtin_amdgcn_ballot_w64(p < hi) != 0; p += CW_U) {
          double av[CW_U], xv[CW_U];
#pragma unroll
          for (int j = 0; j < CW_U; j++) {
            const bool ok = p + j < hi;
            const int sl = cw_slot(ok ? p + j - e0 : 0);
            av[j] = sa[sl];
            xv[j] = ok ? x[sc[sl]] : 0.0;
          }
#pragma unroll
          for (int j = 0; j < CW_U; j++) if (p + j < hi) acc = fma(av[j], xv[j], acc);
        }
      } else {
        for (int p = lo; p < hi; p++) { const int sl = cw_slot(p - e0); acc = fma(sa[sl], sx[sl], acc); }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (en < cu.E1) { cur = nxt; e0 = en; continue; }
    }
    // this wave's 64 rows are complete
    if (cu.has) __builtin_nontemporal_store(acc, y + cu.r);
    acc = 0.0;
    g += gstep;
    if (g >= gend) break;
    cu = nx;
    nx = g + gstep < gend ? cw_rows(n, rp, g + gstep, w, lane) : CwRows{0, 0, 0, 0, 0, false};
    e0 = cu.E0 & ~1;
    if (nxt_loaded) cur = nxt;
    else if (e0 < cu.E1) cw_load(cur, col, val, e0, cu.E1, lane);
    nxt_loaded = false;
  }
}

// ---- the same with the col / val streams going STRAIGHT into LDS (global_load_lds_dwordx4: no register staging, no ds_write pass) ----
// Row side only (short rows). A chunk of 512 entries is six LDS-DMA instructions per wave (four for the values: lane l of instruction i brings
// entries 128 i + 2 l, + 1; two for the columns: 256 i + 4 l .. + 3) into a lane-linear image - the DMA's destination is base + lane x 16, so
// the image cannot be skewed; rows whose length is a multiple of 16 meet on one bank (slower, not wrong). Chosen at assembly for up to 16 entries
// per row on average (beyond that the entry-side register form is as fast or faster: profiles/r04_csr_lds_dma.txt); the row-side register form
// measures against it through KSGPU_SPMV=csrregs. The registers the staged form spends on two chunks in flight (48 of its 96) are free here: more waves per
// SIMD take over the latency hiding. A chunk starts on a multiple of four entries (16-byte aligned in both streams; up to three entries of
// the rows before it are fetched and ignored).
template <int CW_STEPS, int WPS, int GU>
__global__ __launch_bounds__(256, WPS) void k_spmv_csr_wave_dma(int n, const int *__restrict__ rp, const int *__restrict__ col, const double *__restrict__ val,
                                                                const double *__restrict__ x, double *__restrict__ y, int xcd_remap)
{
  constexpr int CH = 64 * CW_STEPS;
  __shared__ __attribute__((aligned(16))) double sa_all[4][CH];
  __shared__ __attribute__((aligned(16))) int sc_all[4][CH];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double *sa = sa_all[w];
  int *sc = sc_all[w];
  const WaveGroups wg = wave_groups_xcd(n, xcd_remap);
  int g = wg.g;
  const int gend = wg.gend, gstep = wg.gstep;
  if (g >= gend) return;
  CwRows cu = cw_rows(n, rp, g, w, lane);
  CwRows nx = g + gstep < gend ? cw_rows(n, rp, g + gstep, w, lane) : CwRows{0, 0, 0, 0, 0, false};
  for (;;) {
    double acc = 0.0;
    for (int e0 = cu.E0 & ~3; e0 < cu.E1; e0 += CH) {
      cw_dma_chunk<CH>(sa, sc, col, val, e0, cu.E1, lane);
      const int lo = max(cu.p0, e0), hi = min(cu.p1, e0 + CH);
      for (int p = lo; __builtin_amdgcn_ballot_w64(p < hi) != 0; p += GU) {
        double av[GU], xv[GU];
#pragma unroll
        for (int j = 0; j < GU; j++) {
          const bool ok = p + j < hi;
          const int sl = ok ? p + j - e0 : 0;
          av[j] = sa[sl];
          xv[j] = ok ? x[sc[sl]] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < GU; j++) if (p + j < hi) acc = fma(av[j], xv[j], acc);
      }
    }
    if (cu.has) __builtin_nontemporal_store(acc, y + cu.r);
    g += gstep;
    if (g >= gend) break;
    cu = nx;
    nx = g + gstep < gend ? cw_rows(n, rp, g + gstep, w, lane) : CwRows{0, 0, 0, 0, 0, false};
  }
}

// ---- windowed CSR (KS_MAT_LAYOUT_WINDOW; the plan: ks_csr.h) -------------------------------------------------------------------------------
// For ragged rows of more than 16 entries whose columns are stripe-local (a mesh ordering with several unknowns per node): the entry-side form above
// pulls a 128-byte line of x through L2 and L1 for every 8 bytes it gathers. Here a block of WIN_ROWS rows brings the 64-double segments of x its
// entries reference - at most WIN_SMAX, listed ascending by the builder - into LDS once, by LDS-DMA at 16 bytes per lane (one wave instruction moves two
// segments: lanes 0-31 the even slot, lanes 32-63 the odd one; the image is lane-linear, slot s at win + 64 s), and the entry lanes gather from
// there by ds_read_b64 through a 16-bit code per entry, slot * 64 + (col & 63): 10 bytes per nonzero instead of 12 and no line traffic per entry.
// A segment that reaches past n brings only its lanes below n (x may end where the allocation ends), the last odd element by a plain load; the
// words left unwritten are never referenced, for a code only names a column of the matrix. An x that is not 16-byte aligned fills by plain loads.
// The walk is k_spmv_csr_wave's entry side: a wave per 64 rows streams their one run of entries in chunks of 64 CW_STEPS - values one per lane,
// codes FOUR per lane in one 8-byte load (entries 256 i + 4 l .. + 3 of the chunk; a chunk starts on a multiple of four entries), both
// nontemporal - parks (value, x) in its own piece of LDS and then lane = row sums fma(a, x, acc) from 0.0 in entry order: the bits of every other
// layout. Entries in front of the wave's run that the aligned start takes along are neither gathered nor summed. One workgroup barrier per block,
// between the fill and the first gather, and none per chunk; the grid is a workgroup per block (the second barrier, in front of a refill, is only
// reached by a grid that was capped), XCD by XCD one contiguous eighth of the blocks as in wave_groups_xcd.
// A DIRECT block (more segments than a window holds) is a workgroup-uniform branch into the same walk: four 32-bit columns per lane in one 16-byte
// load from the side array, x gathered from memory; no fill and no barrier.
typedef int ks_i4v __attribute__((ext_vector_type(4)));
typedef unsigned ks_u2v __attribute__((ext_vector_type(2)));
template <int CW_STEPS> struct WinRegs { double a[CW_STEPS]; ks_i4v c[CW_STEPS / 4]; };     // window block: c[i].x, .y hold the four codes
template <int CW_STEPS>
__device__ __forceinline__ void win_load(WinRegs<CW_STEPS> &r, bool direct, const unsigned short *__restrict__ codes, const int *__restrict__ dc,
                                         const double *__restrict__ val, int e0, int E1, int lane)
{
#pragma unroll
  for (int i = 0; i < CW_STEPS / 4; i++) {
    const int e = e0 + 256 * i + 4 * lane;                     // up to three past E1: CW_PAD
    if (direct) r.c[i] = e < E1 ? __builtin_nontemporal_load(reinterpret_cast<const ks_i4v *>(dc + e)) : ks_i4v{0, 0, 0, 0};
    else { const ks_u2v t = e < E1 ? __builtin_nontemporal_load(reinterpret_cast<const ks_u2v *>(codes + e)) : ks_u2v{0u, 0u}; r.c[i] = ks_i4v{(int)t.x, (int)t.y, 0, 0}; }
  }
#pragma unroll
  for (int u = 0; u < CW_STEPS; u++) {
    const int e = e0 + u * 64 + lane;
    r.a[u] = e < E1 ? ksk::ldstream(val + e) : 0.0;
  }
}
template <int CW_STEPS>
__global__ __launch_bounds__(WIN_ROWS, 2) void k_spmv_window(int n, const int *__restrict__ rp, const unsigned short *__restrict__ codes, const int *__restrict__ dcol,
                                                             const double *__restrict__ val, const int *__restrict__ segptr, const int *__restrict__ seg,
                                                             const int *__restrict__ dbase, const double *__restrict__ x, double *__restrict__ y, int xcd_remap)
{
  constexpr int CH = 64 * CW_STEPS, WAVES = WIN_ROWS / 64, NQ = CW_STEPS / 4;
  static_assert(CW_STEPS % 4 == 0, "codes come four per lane: chunks of 256 entries");
  __shared__ __attribute__((aligned(16))) double win[WIN_SMAX * 64];
  __shared__ double sa_all[WAVES][CH + CH / 32];
  __shared__ double sx_all[WAVES][CH + CH / 32];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double *sa = sa_all[w], *sx = sx_all[w];
  const int NG = (n + WIN_ROWS - 1) / WIN_ROWS;              // blocks: as wave_groups_xcd (ks_rows.cuh), with the layout's block in place of 256 rows
  int g, gend, gstep;
  if (xcd_remap) {
    const int xcd = blockIdx.x & 7, li = blockIdx.x >> 3, lc = gridDim.x >> 3;
    g = (int)((long long)NG * xcd / 8) + li; gend = (int)((long long)NG * (xcd + 1) / 8); gstep = lc;
  } else { g = blockIdx.x; gend = NG; gstep = gridDim.x; }
  const bool x16 = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  for (; g < gend; g += gstep) {
    const int db = dbase[g];
    const bool direct = db != ksc::WIN_NOT_DIRECT;          // the same for the whole workgroup
    const int *dc = dcol + (direct ? db : 0);
    const CwRows cu = WIN_ROWS == 256 ? cw_rows(n, rp, g, w, lane) : cw_rows(n, rp, g >> 2, g & 3, lane);
    int e0 = cu.E0 & ~3;
    WinRegs<CW_STEPS> cur, nxt;
    if (e0 < cu.E1) win_load(cur, direct, codes, dc, val, e0, cu.E1, lane);      // the first chunk is on its way while the window fills
    if (!direct) {
      const int s0 = segptr[g], ns = segptr[g + 1] - s0;
      for (int i = w; 2 * i < ns; i += WAVES) {
        const int sl = 2 * i + (lane >> 5);
        if (sl < ns) {
          const long long c = (long long)seg[s0 + sl] * 64 + (lane & 31) * 2;
          if (x16 && c + 1 < n) __builtin_amdgcn_global_load_lds((ks_glb_void *)(x + c), (ks_lds_void *)(win + 128 * i), 16, 0, 0);
          else {
            if (c < n) win[64 * sl + (lane & 31) * 2] = x[c];
            if (c + 1 < n) win[64 * sl + (lane & 31) * 2 + 1] = x[c + 1];
          }
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // an LDS-DMA is a pending LDS write on the VM counter; the barrier then orders the other waves' reads behind it
      __syncthreads();
    }
    double acc = 0.0;
    while (e0 < cu.E1) {
#pragma unroll
      for (int u = 0; u < CW_STEPS; u++) sa[cw_slot(u * 64 + lane)] = cur.a[u];
      double xg[4 * NQ];
#pragma unroll
      for (int i = 0; i < NQ; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int e = e0 + 256 * i + 4 * lane + j;
          const bool ok = e >= cu.E0 && e < cu.E1;
          if (direct) xg[4 * i + j] = ok ? x[cur.c[i][j]] : 0.0;
          else xg[4 * i + j] = ok ? win[((unsigned)cur.c[i][j >> 1] >> (16 * (j & 1))) & 0xffffu] : 0.0;
        }
#pragma unroll
      for (int i = 0; i < NQ; i++) {
        const int sl = cw_slot(256 * i + 4 * lane);            // 4 l .. 4 l + 3 never straddle a skew step
#pragma unroll
        for (int j = 0; j < 4; j++) sx[sl + j] = xg[4 * i + j];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int en = e0 + CH;
      if (en < cu.E1) win_load(nxt, direct, codes, dc, val, en, cu.E1, lane);
      const int lo = max(cu.p0, e0), hi = min(cu.p1, en);
      for (int p = lo; p < hi; p++) { const int sl = cw_slot(p - e0); acc = fma(sa[sl], sx[sl], acc); }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (en < cu.E1) cur = nxt;
      e0 = en;
    }
    if (cu.has) __builtin_nontemporal_store(acc, y + cu.r);
    if (g + gstep < gend) __syncthreads();                    // a capped grid: the next block's fill waits for this block's last gather
  }
}
#ifndef KS_WIN_STEPS
#define KS_WIN_STEPS 4      // chunks of 256 entries: 49.6 KB of LDS per workgroup, three workgroups per CU (8: 66.5 KB, two)
#endif

// ---- block CSR (KS_MAT_LAYOUT_BSR; the plan: ks_csr.h, the walk: bsr_walk, ks_rows.cuh) ----------------------------------------------------------------
// A matrix of dense BS x BS node blocks, one 4-byte column per block: 8 + 4 / BS^2 bytes per stored scalar against the CSR stream's 12, and one gather
// of BS contiguous doubles of x per block where the CSR kernels gather 8 bytes per scalar. The entry side of k_spmv_csr_wave, block by block: a wave
// owns the 64 / BS block rows of at most 64 scalar rows, whose blocks are one contiguous run; it streams that run in chunks of bsr_chunk_blocks(BS)
// whole blocks - at most 512 scalars, four 16-byte nontemporal loads per lane, never a lane-per-row load of the value stream (one 128-byte line per
// block row) - and parks values and x in its own 6 KB of LDS. y is bit for bit the CSR kernels' y on the expansion.
template <int BS>
__global__ __launch_bounds__(256, 4) void k_spmv_bsr(int nb, const int *__restrict__ brp, const int *__restrict__ bcol, const double *__restrict__ val,
                                                     const double *__restrict__ x, double *__restrict__ y, int xcd_remap)
{
  constexpr int NB = bsr_chunk_blocks(BS);
  __shared__ __attribute__((aligned(16))) double sa_all[4][128 * BsrRegs<BS, NB>::STEPS];
  __shared__ double sx_all[4][NB * BS];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  bsr_walk<BS, 1, NB>(sa_all[w], sx_all[w], nb, brp, bcol, val, x, 0, y, 0, 1, xcd_remap);
}
// The same storage for the small matrices (fewer than 2048 local rows), which the CSR layout gives to the CSR-vector kernel k_spmv_csr: 64 rows per wave
// leave most of the machine idle there. G lanes share a scalar row exactly as there - lane g takes entries g, g + G, ... of the row's expansion by fma
// from 0.0, then the butterfly of group_reduce - so y is bit for bit k_spmv_csr<G>'s on the expansion (G = lanes_per_row, picked from the expansion at
// assembly): a block matrix has the bits of its CSR expansion at every size. Entry p of scalar row bs I + i is (block p / bs of block row I, column
// p % bs). The block size is a runtime argument: nothing here is tuned per size.
template <int G>
__global__ __launch_bounds__(SPMV_BLOCK) void k_spmv_bsr_vec(int n, int bs, const int *__restrict__ brp, const int *__restrict__ bcol, const double *__restrict__ val,
                                                             const double *__restrict__ x, double *__restrict__ y)
{
  constexpr int GPW = 64 / G;
  const int lane = threadIdx.x & 63, gi = lane / G, lane_g = lane % G;
  const long long wave = ((long long)blockIdx.x * SPMV_BLOCK + threadIdx.x) >> 6, nwaves = ((long long)gridDim.x * SPMV_BLOCK) >> 6;
  for (long long wb = wave * GPW; wb < n; wb += nwaves * GPW) {
    const long long r = wb + gi;
    double acc = 0.0;
    if (r < n) {
      const int I = (int)(r / bs), i = (int)(r - (long long)I * bs), k0 = brp[I], len = (brp[I + 1] - k0) * bs;
      for (int p = lane_g; p < len; p += G) {
        const int k = p / bs, c = p - k * bs;
        acc = fma(val[((long long)(k0 + k) * bs + i) * bs + c], x[(long long)bcol[k0 + k] * bs + c], acc);
      }
    }
    const double t = group_reduce<G>(acc);
    if (lane_g == 0 && r < n) __builtin_nontemporal_store(t, y + r);
  }
}

// ---- sliced ELL (SELL-64) ---------------------------------------------------------------------------
// lane <-> row: every val/col load of a wavefront is one contiguous run, the x gather of a
// stencil matrix is contiguous too (consecutive rows -> consecutive columns), y is stored 512 B per wave,
// no cross-lane reduction. Row lengths (int32 per row, the same 4n bytes CSR spends on rowptr) mask the
// padding, so padded slots are never multiplied (no 0*NaN pollution, empty rows give exactly 0).
// Round 4: entries are stored in PAIRS - entries 2q and 2q + 1 of a lane's row side by side, 128 entries per pair index q - so that a lane
// fetches two columns with one 8-byte load and two values with one 16-byte load (a wave: 512 B and 1 KB contiguous): 4-byte-per-lane streaming
// loads top out at 0.7 - 2.4 TB/s on this part (profiles/r03_micro_load_width.txt), and a third of this kernel's load instructions were such.
// A slice of odd width keeps its last entry as a column of singles behind its pairs: same storage as before, same entry order, same fma chain
// - the same bits (asserted against the CSR kernels and the dictionary layouts).
template <int UNR>           // pairs in flight per lane
__global__ __launch_bounds__(SPMV_BLOCK) void k_spmv_sell(int nrows, int nslices, const int *__restrict__ sp, const int *__restrict__ rlen,
                                                          const int *__restrict__ col, const double *__restrict__ val,
                                                          const double *__restrict__ x, double *__restrict__ y, int xcd_remap)
{
  const int lane = threadIdx.x & 63;
  const int wpb = SPMV_BLOCK / 64;
  const long long nblk = gridDim.x;
  const long long nsb = ((long long)nslices + wpb - 1) / wpb;     // slice groups
  for (long long g = sell_first_group(nblk, xcd_remap); g < nsb; g += nblk) {
    const long long s = g * wpb + (threadIdx.x >> 6);
    if (s >= nslices) continue;
    const long long r = s * 64 + lane;
    const int w = sp[s + 1] - sp[s], wp = w >> 1;
    const int len = (r < nrows) ? rlen[r] : 0;
    const long long sb = (long long)sp[s] * 64;
    double acc = 0.0;
    for (int q = 0; q < wp; q += UNR) {         // fully predicated batches: all loads of a batch are independent
      ks_i2v c[UNR]; ksk::ks_d2v a[UNR]; double x0[UNR], x1[UNR];
      KS_SELL_LOAD_PAIRS(UNR, c, a, col, val, sb, q, wp, len, lane)
#pragma unroll
      for (int u = 0; u < UNR; u++) { x0[u] = c[u].x >= 0 ? x[c[u].x] : 0.0; x1[u] = c[u].y >= 0 ? x[c[u].y] : 0.0; }
#pragma unroll
      for (int u = 0; u < UNR; u++) { acc = fma(a[u].x, x0[u], acc); acc = fma(a[u].y, x1[u], acc); }
    }
    if (w & 1) { const SellEntry t = sell_tail(col, val, sb, w, len, lane); acc = fma(t.a, t.c >= 0 ? x[t.c] : 0.0, acc); }
    if (r < nrows) __builtin_nontemporal_store(acc, y + r);
  }
}

// ---- dictionary ELL ----------------------------------------------------------------------------------
// Stencil and graph matrices repeat a handful of values at a handful of column offsets (the 7-point Laplacian: 2 values,
// 7 offsets). When a matrix has at most 255 distinct values (compared bit for bit), at most 256 distinct offsets
// col - row and rows of at most 32 entries, every entry is stored as two bytes (offset code, value code; value code 255
// marks padding): 16 or 32 bytes per row instead of 12 per entry, one 16-byte load per lane. The dictionaries sit in
// LDS. Entries keep their CSR order and the products are accumulated in that order with fma, exactly as k_spmv_sell
// does, so y is bit-identical to the SELL / CSR result.
// Row-pattern form: a matrix with constant coefficients has very few distinct rows of codes (the 7-point Dirichlet Laplacian on a box: 27), so
// when there are at most 256 the matrix keeps one byte per row, the index of the row's code word in a table that goes to LDS beside the two
// dictionaries (rowpat != nullptr; codes is then null). A lane takes its row's word from LDS instead of from memory and decodes it as before: the
// product reads n bytes of matrix instead of 2 W n.
// One row per lane and at most 64 workgroups per CU also in the pattern form: two rows per lane with 16-byte stores of y measured the same within
// 2 %, four rows per lane, 16 workgroups per CU and one 256-row group per workgroup slower (profiles/r06_dict_patterns.txt): the walk is bound by
// its per-entry instructions (profiles/r14_dict_pairs.txt), which is what the pair form below cuts (52 -> 37 us on the 216^3 Laplacian)
// Pair form (NBT > 0: the compiled number of bases; ks_dict_pairs.h): a lane owns rows r, r + 1 of a group of 512 and loads x 16 bytes at a time, the
// same XCD-contiguous walk over the row groups. No lane leaves the loop early: a lane past the last row still lends its loads to the lane below it.
template <int W, int NBT = 0>
__global__ __launch_bounds__(SPMV_BLOCK) void k_spmv_dict(int nrows, const uint4 *__restrict__ codes, const unsigned char *__restrict__ rowpat, const uint4 *__restrict__ pats, int npat,
                                                          const double *__restrict__ dval, int nval, const int *__restrict__ doff, int noff,
                                                          const double *__restrict__ x, double *__restrict__ y, int xcd_remap,
                                                          ksp::PairArgs pa = ksp::PairArgs(), const double *__restrict__ pcoef = nullptr, const unsigned *__restrict__ pmask = nullptr,
                                                          unsigned *fctl = nullptr, unsigned fepoch = 0)
{
  if constexpr (NBT > 0) {
    // the fallback behind a forward final update (ks_gs.hip): nothing to do when that launch formed this product itself and no wait of it gave up
    if (fctl) {
      if (fctl[KS_FWD_TAKEN] == fepoch && fctl[KS_FWD_ABORT] != fepoch) return;
      if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(fctl + KS_FWD_NFALLBACK, 1u);
    }
    KS_PAIR_LDS_FILL(SPMV_BLOCK, pa, pcoef, pmask, npat, sc, sm);
    const RowGroups rg = row_groups_xcd(nrows, 2 * SPMV_BLOCK, xcd_remap);
    const PairLane ln(x, nrows);
    for (long long g = rg.g0 + rg.lb; g < rg.g1; g += rg.nb) {
      const long long r = g * (2 * SPMV_BLOCK) + 2 * (long long)threadIdx.x;
      int p0, p1;
      pair_patterns(rowpat, r, nrows, p0, p1);
      double y0, y1;
      ksp::dict_pair_walk<NBT>(pa, sc, sm, p0, p1, r, ln, y0, y1);
      if (r + 1 < nrows) __builtin_nontemporal_store(ksk::ks_d2v{y0, y1}, reinterpret_cast<ksk::ks_d2v *>(y + r));
      else if (r < nrows) __builtin_nontemporal_store(ksp::dict_row_from_tables<W>(rowpat, reinterpret_cast<const unsigned short *>(pats), r, dval, doff, x), y + r);
    }
    return;
  }
  __shared__ double sv[256];
  __shared__ int so[256];
  KS_DICT_LDS_FILL(SPMV_BLOCK, W, sv, so, dval, nval, doff, noff, rowpat, pats, npat);
  const RowGroups rg = row_groups_xcd(nrows, SPMV_BLOCK, xcd_remap);
  for (long long g = rg.g0 + rg.lb; g < rg.g1; g += rg.nb) {
    const long long r = g * SPMV_BLOCK + threadIdx.x;
    if (r >= nrows) break;
    constexpr int Q = W / 8;                                // uint4 (8 entries) per row
    uint4 c[Q];
    if (rowpat) {
      const int p = rowpat[r];
#pragma unroll
      for (int q = 0; q < Q; q++) c[q] = dict_pat_lds[p * Q + q];
    } else {
#pragma unroll
      for (int q = 0; q < Q; q++) c[q] = ksk::ldstream4(codes + r * Q + q);
    }
    // Nontemporal, as in every product kernel below: a plain store leaves the 80 MB of y dirty in the L2s, and their write-back then mixes into the
    // read streams of the dot sweep that follows (15 us of its 303 on the 216^3 workload: profiles/r02_ab_spmv_store_nt.txt)
    __builtin_nontemporal_store(dict_word_row<W>(c, r, sv, so, x), y + r);
  }
}

// ---- dictionary product fused into the dot sweep that follows it --------------------------------------------------------------------
// A Krylov step is y = A x followed by the dot products of y with the basis columns (and itself). While the basis is resident in the
// Infinity Cache (config 1 and 2: a step is five dependent launches of 5 - 30 us each) the product is worth a launch of its own no longer:
// the dictionary layout is row-local (lane = row), so the dot sweep's tile loop computes its two rows of y itself - same entry order and fma
// chain as k_spmv_dict, same bits -, stores them, and uses them from registers as the vector of the dots and as the last "column". One
// launch, one kernel boundary and one read of y less per step. Not for bases that stream from HBM: the sweep's tiles are interleaved over
// the XCDs, so the stencil's far neighbours (+-nx*ny) would miss the tile's L2 where k_spmv_dict, which gives every XCD one contiguous
// range of rows, hits it.
template <int W>
__device__ __forceinline__ double dict_row(const uint4 *__restrict__ codes, const unsigned char *__restrict__ rowpat, long long r, const double *sv, const int *so, const double *__restrict__ x)
{
  constexpr int Q = W / 8;
  uint4 c[Q];
  if (rowpat) {                                              // the row-pattern form: the code word comes from the table in LDS
    const int p = rowpat[r];
#pragma unroll
    for (int q = 0; q < Q; q++) c[q] = dict_pat_lds[p * Q + q];
  } else {
#pragma unroll
    for (int q = 0; q < Q; q++) c[q] = codes[r * Q + q];
  }
  return dict_word_row<W>(c, r, sv, so, x);
}
// Pair form (NBT > 0, ks_dict_pairs.h): the sweep already holds two consecutive rows per lane, so an eligible matrix has them computed by the pair walk -
// same tiles, grid and partials, and y with the one-row walk's bits, so the dots keep theirs. Every lane of a wave enters the walk, also past the last row.
template <int KT, int W, int NBT = 0>
__global__ __launch_bounds__(ksk::SW_BLOCK) void k_dot_spmv_dict(const double *__restrict__ Vb, long long ld, int n, int ncols, const uint4 *__restrict__ codes,
                                                                 const unsigned char *__restrict__ rowpat, const uint4 *__restrict__ pats, int npat,
                                                                 const double *__restrict__ dval, int nval, const int *__restrict__ doff, int noff,
                                                                 const double *__restrict__ x, double *__restrict__ y, double *__restrict__ partials,
                                                                 const KsGsState *__restrict__ gate, int *__restrict__ pgrid, int rev,
                                                                 ksp::PairArgs pa = ksp::PairArgs(), const double *__restrict__ pcoef = nullptr, const unsigned *__restrict__ pmask = nullptr)
{
  using namespace ksk;
  if (gate && !gate->active) return;
  __shared__ double sv[256];
  __shared__ int so[256];
  double *sc = nullptr; unsigned *sm = nullptr;
  if constexpr (NBT > 0) {
    sc = reinterpret_cast<double *>(dict_pat_lds); sm = reinterpret_cast<unsigned *>(sc + npat * 3 * pa.nb);
    for (int i = threadIdx.x; i < npat * 3 * pa.nb; i += SW_BLOCK) sc[i] = pcoef[i];      // as KS_PAIR_LDS_FILL (ks_rows.cuh)
    for (int i = threadIdx.x; i < npat; i += SW_BLOCK) sm[i] = pmask[i];
  } else {
    for (int i = threadIdx.x; i < nval; i += SW_BLOCK) sv[i] = dval[i];               // as KS_DICT_LDS_FILL (ks_rows.cuh), in place
    for (int i = threadIdx.x; i < noff; i += SW_BLOCK) so[i] = doff[i];
    if (rowpat) for (int i = threadIdx.x; i < npat * (W / 8); i += SW_BLOCK) dict_pat_lds[i] = pats[i];
  }
  __syncthreads();
  const ksr::PairLane ln(x, n);
  if (pgrid && blockIdx.x == 0 && threadIdx.x == 0) *pgrid = gridDim.x;
  double acc[KT];
#pragma unroll
  for (int i = 0; i < KT; i++) acc[i] = 0.0;
  const int nprev = ncols - 1;                               // basis columns in memory; the last "column" is y itself
  const long long tile = (long long)SW_BLOCK * 2, ntiles = ((long long)n + tile - 1) / tile;
  for (long long t0 = blockIdx.x; t0 < ntiles; t0 += gridDim.x) {
    const long long t = rev ? ntiles - 1 - t0 : t0;
    const long long r = t * tile + (long long)threadIdx.x * 2;
    double2 yp = {0.0, 0.0};
    if constexpr (NBT > 0) {
      int p0, p1;
      ksr::pair_patterns(rowpat, r, n, p0, p1);
      ksp::dict_pair_walk<NBT>(pa, sc, sm, p0, p1, r, ln, yp.x, yp.y);
    }
    if (r + 1 < n) {
      double2 xv[KT];
#pragma unroll
      for (int i = 0; i < KT; i++) { const int ii = i < nprev ? i : (nprev > 0 ? nprev - 1 : 0); if (nprev > 0) xv[i] = ldplain2(Vb + (long long)ii * ld + r); else xv[i] = double2{0.0, 0.0}; }
      double2 yv = yp;
      if constexpr (NBT == 0) { yv.x = dict_row<W>(codes, rowpat, r, sv, so, x); yv.y = dict_row<W>(codes, rowpat, r + 1, sv, so, x); }
      *reinterpret_cast<double2 *>(y + r) = yv;
#pragma unroll
      for (int i = 0; i < KT; i++) {
        const double2 c = (i == nprev) ? yv : xv[i];
        acc[i] = fma(c.x, yv.x, acc[i]); acc[i] = fma(c.y, yv.y, acc[i]);
      }
    } else if (r < n) {
      double yv;
      if constexpr (NBT > 0) yv = ksp::dict_row_from_tables<W>(rowpat, reinterpret_cast<const unsigned short *>(pats), r, dval, doff, x);      // odd n: the last row on its own
      else yv = dict_row<W>(codes, rowpat, r, sv, so, x);
      y[r] = yv;
#pragma unroll
      for (int i = 0; i < KT; i++) {
        const int ii = i < nprev ? i : (nprev > 0 ? nprev - 1 : 0);
        const double c = (i == nprev) ? yv : (nprev > 0 ? Vb[(long long)ii * ld + r] : 0.0);
        acc[i] = fma(c, yv, acc[i]);
      }
    }
  }
  block_write_partials<KT>(acc, ncols, partials);
}

// Offset-dictionary ELL: the matrix has arbitrary values (variable-coefficient stencils) but still only a few distinct column
// offsets. The index of an entry shrinks from 4 bytes to 1 (code 255 = padding); the values stay full doubles, stored
// slice-column-major like SELL-64 so that a wave reads 512 contiguous bytes per entry slot. 7-point stencil: 80 bytes per row
// instead of 104. Same entry order and fma chain as the other layouts.
template <int W>
__global__ __launch_bounds__(SPMV_BLOCK) void k_spmv_odict(int nrows, const unsigned char *__restrict__ codes, const double *__restrict__ vals, const int *__restrict__ doff, int noff,
                                                           const double *__restrict__ x, double *__restrict__ y, int xcd_remap)
{
  __shared__ int so[256];
  lds_fill<SPMV_BLOCK>(so, doff, noff);
  __syncthreads();
  const RowGroups rg = row_groups_xcd(nrows, SPMV_BLOCK, xcd_remap);
  for (long long g = rg.g0 + rg.lb; g < rg.g1; g += rg.nb) {
    const long long r = g * SPMV_BLOCK + threadIdx.x;
    if (r >= nrows) break;
    unsigned wds[W / 4];
    if (W == 8) { const uint2 c = *reinterpret_cast<const uint2 *>(codes + r * 8); wds[0] = c.x; wds[1] = c.y; }
    else {
#pragma unroll
      for (int q = 0; q < W / 16; q++) {
        const uint4 c = ksk::ldstream4(reinterpret_cast<const uint4 *>(codes + r * W) + q);
        wds[(4 * q) % (W / 4)] = c.x; wds[(4 * q + 1) % (W / 4)] = c.y; wds[(4 * q + 2) % (W / 4)] = c.z; wds[(4 * q + 3) % (W / 4)] = c.w;
      }
    }
    const double *vb = vals + ((r >> 6) * W) * 64 + (r & 63);
    double a[W], xv[W];
#pragma unroll
    for (int e = 0; e < W; e++) {
      const DictCode d = odict_code(wds[e >> 2], e);
      a[e] = d.ok ? ksk::ldstream(vb + (long long)e * 64) : 0.0;
      xv[e] = d.ok ? x[r + so[d.oc]] : 0.0;
    }
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < W; e++) acc = fma(a[e], xv[e], acc);
    __builtin_nontemporal_store(acc, y + r);
  }
}

template <int G, bool ACCUM, bool ROWLIST>
void launch_spmv_g(hipStream_t st, int num_cu, int nrows, const int *rowptr, const int *col, const double *val, const double *x, double *y, const int *rowlist)
{
  constexpr int UNROLL = 4;
  constexpr int RW = (64 / G) * UNROLL;                        // rows per wavefront per sweep
  long long waves = ((long long)nrows + RW - 1) / RW;
  long long blocks = (waves * 64 + SPMV_BLOCK - 1) / SPMV_BLOCK;
  long long maxb = (long long)num_cu * 32;
  if (blocks > maxb) blocks = maxb;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL((k_spmv_csr<G, UNROLL, ACCUM, ROWLIST>), dim3((unsigned)blocks), dim3(SPMV_BLOCK), 0, st, nrows, rowptr, col, val, x, y, rowlist);
}

template <bool ACCUM, bool ROWLIST>
void launch_spmv(hipStream_t st, int num_cu, int lanes, int nrows, const int *rowptr, const int *col, const double *val, const double *x, double *y, const int *rowlist)
{
  switch (lanes) {
    case 2:  launch_spmv_g<2, ACCUM, ROWLIST>(st, num_cu, nrows, rowptr, col, val, x, y, rowlist); break;
    case 4:  launch_spmv_g<4, ACCUM, ROWLIST>(st, num_cu, nrows, rowptr, col, val, x, y, rowlist); break;
    case 8:  launch_spmv_g<8, ACCUM, ROWLIST>(st, num_cu, nrows, rowptr, col, val, x, y, rowlist); break;
    case 16: launch_spmv_g<16, ACCUM, ROWLIST>(st, num_cu, nrows, rowptr, col, val, x, y, rowlist); break;
    case 32: launch_spmv_g<32, ACCUM, ROWLIST>(st, num_cu, nrows, rowptr, col, val, x, y, rowlist); break;
    default: launch_spmv_g<64, ACCUM, ROWLIST>(st, num_cu, nrows, rowptr, col, val, x, y, rowlist); break;
  }
}

__global__ void k_pack(int n, const int *__restrict__ idx, const double *__restrict__ x, double *__restrict__ out)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = x[idx[i]];
}

// Partial y of XCD x = blockIdx % 8 over its slices. A workgroup takes 256 consecutive rows; their entries are one
// contiguous run of the slice's arrays, which the workgroup streams in chunks of 1024 with fully coalesced, nontemporal
// loads (every lane has 4 independent gathers in flight), parks the products in LDS, and then every row (= thread) adds up
// its own segment in entry order.
constexpr int SL_EPT = 4;
__global__ __launch_bounds__(256) void k_spmv_sliced(int n, int nslice, const int *__restrict__ srp, const long long *__restrict__ base,
                                                     const int *__restrict__ col, const double *__restrict__ val, const double *__restrict__ x, double *__restrict__ ypart)
{
  __shared__ double prod[256 * SL_EPT];
  __shared__ int erange[2];
  const int xcd = blockIdx.x & 7, tid = threadIdx.x;
  const long long bx = blockIdx.x >> 3, nbx = gridDim.x >> 3;
  double *yp = ypart + (size_t)xcd * n;
  for (int s = xcd; s < nslice; s += 8) {               // one column range at a time, so that it stays in this XCD's L2
    const int *rp = srp + (size_t)s * (n + 1);
    const int *cs = col + base[s];
    const double *vs = val + base[s];
    for (long long R0 = bx * 256; R0 < n; R0 += nbx * 256) {
      const long long r = R0 + tid;
      const bool has = r < n;
      const int p0 = has ? ksk::ldstream(rp + r) : 0, p1 = has ? ksk::ldstream(rp + r + 1) : 0;
      if (tid == 0) erange[0] = p0;
      if (has && (r == n - 1 || tid == 255)) erange[1] = p1;
      __syncthreads();
      const int E0 = erange[0], E1 = erange[1];
      double acc = (s == xcd || !has) ? 0.0 : yp[r];
      for (int e0 = E0; e0 < E1; e0 += 256 * SL_EPT) {
        int c[SL_EPT]; double a[SL_EPT];
#pragma unroll
        for (int u = 0; u < SL_EPT; u++) { const int e = e0 + u * 256 + tid; const bool ok = e < E1; c[u] = ok ? ksk::ldstream(cs + e) : -1; a[u] = ok ? ksk::ldstream(vs + e) : 0.0; }
#pragma unroll
        for (int u = 0; u < SL_EPT; u++) prod[u * 256 + tid] = c[u] >= 0 ? a[u] * x[c[u]] : 0.0;
        __syncthreads();
        const int lo = max(p0, e0), hi = min(p1, e0 + 256 * SL_EPT);
        for (int p = lo; p < hi; p++) acc += prod[p - e0];
        __syncthreads();
      }
      if (has) __builtin_nontemporal_store(acc, yp + r);
    }
  }
}
__global__ void k_sum_parts(int n, const double *__restrict__ ypart, double *__restrict__ y)
{
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
    double s = ypart[r];
#pragma unroll
    for (int x = 1; x < 8; x++) s += ypart[(size_t)x * n + r];
    __builtin_nontemporal_store(s, y + r);
  }
}


// ---- binned product (ksgpu_internal.h: bn_*) ----------------------------------------------------------------------------------------
// Why: the product of a uniformly random matrix in a row-ordered layout pulls a 128-byte line of x through L2 -> L1 for every nonzero and
// runs at that line rate (1.3 ms for config 5), however x is cut for the L2s. Here no random access leaves the CU: phase 1
// gathers from a piece of x in LDS and streams the gathered values out in the order phase 2 wants them; phase 2 streams them back in with
// the values and adds into rows of y in LDS. 28 bytes per nonzero of pure streams instead of 12 bytes + a line (profiles/r02_micro_binned_spmv*).
// phase 1: grid = slices, 1024 threads; LDS: x piece [cs], off1 row [wb + 1], off2t row [wb], 2 KB per wave for the window's column codes
// Round 4: the window's 1024 column codes come by two global_load_lds_dwordx4 per wave (16 bytes per lane) into a wave-private piece of LDS and the
// lanes read their pairs from there. The register form it replaced loaded a pair per lane and instruction - 4 bytes per lane, and
// 4-byte-per-lane streaming loads top out at 0.7 - 2.4 TB/s on this part (profiles/r03_micro_load_width.txt). Worth 2 - 8 % of this kernel depending on the
// box (334-350 against 363-365 us; 336-341 against 343-351): it stays bound by its store. A second buffer with the next window's codes in flight (counted
// vmcnt behind the window's eight stores) measured no better than the register form: profiles/r04_binned_gather_dma.txt.
// Slices start on multiples of 8 entries (every segment is padded to 8): the 16-byte DMA is aligned.
__global__ __launch_bounds__(1024) void k_binned_gather(int n, int cs, int wb, int nwin, const long long *__restrict__ sbase, const unsigned short *__restrict__ col16,
                                                        const int *__restrict__ off1, const int *__restrict__ off2t, const int *__restrict__ wseg,
                                                        const double *__restrict__ x, double *__restrict__ G)
{
  extern __shared__ double bn_lds[];
  double *xs = bn_lds;
  int *o1 = (int *)(bn_lds + cs);
  int *o2 = o1 + wb + 1;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
  const long long c0 = (long long)s * cs;
  for (int i = tid; i < cs; i += blockDim.x) xs[i] = (c0 + i < n) ? x[c0 + i] : 0.0;
  for (int i = tid; i <= wb; i += blockDim.x) o1[i] = off1[(size_t)s * (wb + 1) + i];
  for (int i = tid; i < wb; i += blockDim.x) o2[i] = off2t[(size_t)s * wb + i];
  __syncthreads();
  const unsigned short *cg = col16 + sbase[s];
  unsigned *cw = reinterpret_cast<unsigned *>(reinterpret_cast<char *>(bn_lds) + ((((size_t)cs * 8 + (size_t)(2 * wb + 1) * 4) + 15) & ~(size_t)15)) + (size_t)w * 512;
  const int total = o1[wb];                                                       // a multiple of 8
  for (int win = w; win * 1024 < total; win += nw) {
    const int base = win * 1024;
    unsigned c[8];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              // the reads of the previous window's codes are done before the next ones may land
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const int e8 = base + 512 * i + 8 * lane;
      if (e8 < total) __builtin_amdgcn_global_load_lds((ks_glb_void *)(cg + e8), (ks_lds_void *)(cw + 256 * i), 16, 0, 2);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int k = 0; k < 8; k++) { const int e = base + k * 128 + 2 * lane; c[k] = e < total ? cw[k * 64 + lane] : 0u; }
    const int lo = wseg[(size_t)s * nwin + win];
    int bnd[BN_MAXSEG], dlt[BN_MAXSEG];
#pragma unroll
    for (int j = 0; j < BN_MAXSEG; j++) { const int sg = min(lo + j, wb - 1); bnd[j] = o1[sg + 1]; dlt[j] = o2[sg] - o1[sg]; }
    const bool fits = bnd[BN_MAXSEG - 1] >= min(base + 1024, total);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int e = base + k * 128 + 2 * lane;
      if (e < total) {
        int d;
        if (fits) {
          d = dlt[0];
#pragma unroll
          for (int j = 1; j < BN_MAXSEG; j++) d = (e >= bnd[j - 1]) ? dlt[j] : d;
        } else { int sg = lo; while (e >= o1[sg + 1]) sg++; d = o2[sg] - o1[sg]; }      // many short segments: look each pair up
        const ksk::ks_d2v g = {xs[c[k] & 0xffffu], xs[c[k] >> 16]};
        __builtin_nontemporal_store(g, reinterpret_cast<ksk::ks_d2v *>(G + ((long long)e + d)));   // pairs never straddle a segment: both orders keep segments even
      }
    }
  }
}
// phase 2: grid = wave-bins / 4, 256 threads: a wave per wave-bin; LDS: 4 x (wr + 1) accumulators (the last one takes the padding entries).
// The wave-bin's entries are ns pieces (one per slice, about 157 entries each, interleaved with the pieces of the workgroup's other three
// waves); the wave takes them in slice order, THREE pieces at a time, each as up to four 64-entry steps (masked beyond the piece's end), so
// that 12 steps of (G, value, row) loads are in flight before the first add. Where a piece is and how long comes from the wave-bin's rows
// of two small tables (wave-uniform: scalar loads) - no per-entry search. (A walk over 512-entry logical windows with a compare chain per
// entry, the mirror of phase 1, cost 70 us more than the contiguous stream it replaced; this form: profiles/r03_ab_binned.txt.)
constexpr int BN_P2 = 3;
__global__ __launch_bounds__(256) void k_binned_reduce(int n, int wr, int ns, const int *__restrict__ log2, const int *__restrict__ off2,
                                                       const double *__restrict__ G, const double *__restrict__ val,
                                                       const unsigned short *__restrict__ row16, double *__restrict__ y, const double *__restrict__ rowscale)
{
  extern __shared__ double bn_lds[];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x * 4 + w;
  double *acc = bn_lds + (size_t)w * (wr + 1);
  for (int i = lane; i <= wr; i += 64) acc[i] = 0.0;
  const int *lg = log2 + (size_t)b * (ns + 1), *ph = off2 + (size_t)b * ns;
  for (int s0 = 0; s0 < ns; s0 += BN_P2) {
    int pb[BN_P2], pl[BN_P2], maxl = 0;
#pragma unroll
    for (int j = 0; j < BN_P2; j++) {
      const int sg = s0 + j < ns ? s0 + j : ns - 1;
      pb[j] = ph[sg]; pl[j] = s0 + j < ns ? lg[sg + 1] - lg[sg] : 0;
      maxl = max(maxl, pl[j]);
    }
    for (int o = 0; o < maxl; o += 256) {                   // one round unless a piece is longer than 256 entries
      double g[BN_P2][4], a[BN_P2][4]; unsigned short r[BN_P2][4];
#pragma unroll
      for (int j = 0; j < BN_P2; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int e = o + k * 64 + lane; const bool ok = e < pl[j];
          const long long p = (long long)pb[j] + e;
          g[j][k] = ok ? __builtin_nontemporal_load(G + p) : 0.0; a[j][k] = ok ? __builtin_nontemporal_load(val + p) : 0.0; r[j][k] = ok ? __builtin_nontemporal_load(row16 + p) : (unsigned short)wr;
        }
      // the adds of one instruction go lane by lane, instructions in program order (piece after piece, entry after entry): a fixed order per
      // row, run after run
#pragma unroll
      for (int j = 0; j < BN_P2; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) if (o + k * 64 + lane < pl[j]) __hip_atomic_fetch_add(acc + r[j][k], a[j][k] * g[j][k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  for (int i = lane; i < wr; i += 64) { const long long row = (long long)b * wr + i; if (row < n) __builtin_nontemporal_store(rowscale ? rowscale[row] * acc[i] : acc[i], y + row); }
}

} // namespace

int ks_binned_prepare(size_t lds1, size_t lds2)      // build_binned declines above 156 KB of either: the casts to int are safe
{
  KS_HIP(hipFuncSetAttribute((const void *)k_binned_gather, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1));
  KS_HIP(hipFuncSetAttribute((const void *)k_binned_reduce, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
  return KS_SUCCESS;
}

// y = A x fused with the dot sweep of y against the ncols - 1 columns in front of it (and itself), where that pays: a single rank, the
// dictionary layout, no B-inner product, a basis that lives in the Infinity Cache, two-row tiles. *done = false: the caller runs the
// product and the dots as separate launches. y must be column jy of bv; the dots are those ksk_dot(bv, col(-nc), ld, nc + jy + 1, y) leaves.
int ks_mat_mult_dot_fused(ks_mat A, ks_bv bv, const double *x, int jy, bool gate, bool *done)
{
  *done = false;
  ks_ctx ctx = A->ctx;
  const int ncols = bv->nc + jy + 1;
  const double *Vb = ks_bv_col(bv, -bv->nc);
  double *y = ks_bv_col(bv, jy);
  // (the other row-local layouts, the windowed CSR among them, keep their own launch: only the dictionary rows are cheap enough to ride in the sweep)
  if (A->layout != KS_MAT_LAYOUT_DICT || A->shell_mult || ks_is_multi(ctx) || A->n_orows > 0 || bv->matrix || A->n != bv->n) return KS_SUCCESS;
  if (ncols < 1 || ncols > KS_MAX_COLS || bv->ld % 2 || (((uintptr_t)Vb) & 15) || (((uintptr_t)y) & 15)) return KS_SUCCESS;
  if (!ksk::ks_basis_is_cache_resident((size_t)(bv->nc + bv->m), (size_t)bv->ld)) return KS_SUCCESS;
  if (ctx->dbg.no_spmv_dot) return KS_SUCCESS;        // test hook: the separate launches, to compare bits
  const int dot_per_cu = std::max(1, std::min(4, (30 + ncols - 1) / ncols));          // the grid ksk_dot would use: the partials, and so the bits, are the same
  const int grid = ks_sweep_grid_for(ctx, bv->n, 2, nullptr, dot_per_cu);
  const int rev = bv->sweep_dir; bv->sweep_dir ^= 1;
  bv->spec.valid = false; bv->last_grid = grid;
  const KsGsState *g = gate ? bv->gs : nullptr;
  KsProfScope ps(ctx, KS_K_SPMVDOT, 8.0 * bv->n * ncols + 12.0 * A->nnz + 4.0 * (A->n + 1) + 16.0 * A->n, ks_kt_for(ncols), 8.0 * bv->n * ncols + layout_own_bytes(A) + 8.0 * A->n);
  if (A->dict_w != 8 && A->dict_w != 16) return KS_SUCCESS;                              // W = 32 is not compiled for the sweep
  // the pair form as in MatMult (read at launch; y is 16-byte aligned here), for matrices of up to five bases: the 5- and 7-point stencils
  const bool pairs = A->pr_ok && A->pr_args.nb <= 5 && !ctx->dbg.no_dict_pairs && pair_aligned16(x) && pair_fits32(A->n);
  if (pairs) A->pr_launches++; else A->dc_row_launches++;
  const size_t lds = pairs ? dict_pair_lds_bytes(A) : dict_pattern_lds_bytes(A);
#define FD_W(W) do { if (pairs) hipLaunchKernelGGL((k_dot_spmv_dict<FD_KT, W, 5>), dim3(grid), dim3(ksk::SW_BLOCK), lds, ctx->stream, Vb, (long long)bv->ld, bv->n, ncols, (const uint4 *)A->dc_codes, A->dc_rowpat, (const uint4 *)A->dc_pats, A->dict_npat, A->dc_val, A->dict_nval, A->dc_off, A->dict_noff, x, y, bv->partials, g, &bv->gs->pgrid, rev, A->pr_args, A->pr_coef, A->pr_mask); \
  else hipLaunchKernelGGL((k_dot_spmv_dict<FD_KT, W>), dim3(grid), dim3(ksk::SW_BLOCK), lds, ctx->stream, Vb, (long long)bv->ld, bv->n, ncols, (const uint4 *)A->dc_codes, A->dc_rowpat, (const uint4 *)A->dc_pats, A->dict_npat, A->dc_val, A->dict_nval, A->dc_off, A->dict_noff, x, y, bv->partials, g, &bv->gs->pgrid, rev); } while (0)
#define LAUNCH_FD(KT) do { constexpr int FD_KT = KT; if (A->dict_w == 8) FD_W(8); else FD_W(16); } while (0)
  KS_KT_DISPATCH(ncols, LAUNCH_FD);
#undef LAUNCH_FD
#undef FD_W
  KS_HIP(hipGetLastError());
  *done = true;
  return KS_SUCCESS;
}

// y = A x.  Multi-rank: pack boundary entries, exchange with the neighbours (RCCL send/recv over xGMI),
// diagonal block product, then the off-diagonal rows add their ghost contributions.
// a row scaling can ride in the product's last pass: the binned layout on a rank without off-diagonal rows (their contribution is added afterwards)
// (nor the transposed view of a row-sharded matrix: the other ranks' contributions are added behind the diagonal block's product)
bool ks_mat_can_rowscale(ks_mat A) { return A && !A->shell_mult && A->layout == KS_MAT_LAYOUT_BINNED && A->n_orows == 0 && !A->sht; }

static int spmv_variant(ks_mat A)
{
  switch (A->layout) {
  case KS_MAT_LAYOUT_BINNED: return KS_SPMV_BINNED;
  case KS_MAT_LAYOUT_DICT: return KS_SPMV_DICT;
  case KS_MAT_LAYOUT_ODICT: return KS_SPMV_ODICT;
  case KS_MAT_LAYOUT_SELL: return KS_SPMV_SELL;
  case KS_MAT_LAYOUT_WINDOW: return KS_SPMV_WINDOW;
  case KS_MAT_LAYOUT_BSR: return KS_SPMV_BSR;
  }
  return KS_SPMV_CSR;
}

// tail (the transposed view of a row-sharded matrix, mult_sharded_transpose): behind the diagonal block's product the main stream waits for the
// reverse exchange (tail_overlap: it ran on the halo stream) and adds what the other ranks sent - where the forward product runs its off-diagonal rows
static int mult_assembled(ks_mat A, const double *x, double *y, const double *rowscale, const ks_mat_s::ShT *tail, bool tail_overlap, const KsFwdGate *gate = nullptr)
{
  ks_ctx ctx = A->ctx;
  const bool multi = ctx->comm.size > 1 && (A->nsend > 0 || A->nghost > 0);
  // Halo under the diagonal-block product (PETSc: VecScatterBegin / local product / VecScatterEnd in MatMult_MPIAIJ): pack and
  // neighbour exchange go to the halo stream once x is complete on the main stream; the main stream runs the diagonal block
  // and only the off-diagonal rows wait for the ghosts. The next product's pack is ordered after this one's off-diagonal rows
  // through ev_x (recorded on the main stream), so send_buf / ghost are never overwritten while still being read.
  const bool overlap = multi && ctx->halo_overlap;
  if (multi) {
    hipStream_t hs = ctx->stream;
    if (overlap) {
      KS_CALL(ks_ctx_halo_stream(ctx));
      hs = ctx->halo_stream;
      KS_HIP(hipEventRecord(ctx->ev_x, ctx->stream));
      KS_HIP(hipStreamWaitEvent(hs, ctx->ev_x, 0));
    }
    KsProfScope ps(ctx, KS_K_HALO, 8.0 * (A->nsend + A->nghost));      // (events on the main stream: with the overlap this times the enqueue only)
    if (A->hp.enabled) KS_CALL(ks_halo_peer_exchange(A, x, hs));      // straight into the neighbours' ghost mailboxes: no library call
    else {
      if (A->nsend) hipLaunchKernelGGL(k_pack, dim3((A->nsend + 255) / 256), dim3(256), 0, hs, A->nsend, A->send_idx, x, A->send_buf);
      KS_CALL(ks_comm_exchange(ctx, (int)A->peers.size(), A->peers.data(), A->send_buf, A->send_off.data(), A->send_cnt.data(),
                               A->ghost, A->recv_off.data(), A->recv_cnt.data(), (int)sizeof(double), hs));
    }
    if (overlap) KS_HIP(hipEventRecord(ctx->ev_halo, hs));
  }
  {
    const double csr_bytes = 12.0 * A->nnz + 4.0 * (A->n + 1) + 16.0 * A->n;                    // what the CSR algorithm moves
    const int variant = spmv_variant(A); double own = layout_own_bytes(A) + 16.0 * A->n + 12.0 * A->nnz_o;      // the layout's own compulsory bytes
    if (A->layout == KS_MAT_LAYOUT_SELL) own = csr_bytes;                                               // filed under the CSR stream's bytes (its padding is at most 12.5 %)
    const bool gated = gate && gate->ctl;            // behind a forward final update: in the common case a launch that returns at once, filed with no bytes
    KsProfScope ps(ctx, KS_K_SPMV, gated ? 0.0 : csr_bytes, variant, gated ? 0.0 : own);
    switch (A->layout) {
    case KS_MAT_LAYOUT_BINNED:
      hipLaunchKernelGGL(k_binned_gather, dim3((unsigned)A->bn_ns), dim3(1024), ks_binned_lds1(A->bn_cs, A->bn_wb), ctx->stream,
                         A->n, A->bn_cs, A->bn_wb, A->bn_nwin, A->bn_sbase, A->bn_col16, A->bn_off1, A->bn_off2t, A->bn_wseg, x, A->bn_g);
      hipLaunchKernelGGL(k_binned_reduce, dim3((unsigned)(A->bn_wb / 4)), dim3(256), ks_binned_lds2(A->bn_wr), ctx->stream, A->n, A->bn_wr, A->bn_ns, A->bn_log2, A->bn_off2,
                         A->bn_g, A->bn_val, A->bn_row16, y, rowscale);
      break;
    case KS_MAT_LAYOUT_SLICED: {
      const int per_xcd = std::max(1, std::min((A->n + 255) / 256, (ctx->num_cu / 8) * 8));       // 8 resident workgroups per CU of the XCD
      hipLaunchKernelGGL(k_spmv_sliced, dim3((unsigned)(8 * per_xcd)), dim3(256), 0, ctx->stream, A->n, A->nslice, A->sl_rowptr, A->sl_base, A->sl_col, A->sl_val, x, A->ypart);
      hipLaunchKernelGGL(k_sum_parts, dim3((unsigned)std::min((A->n + 255) / 256, ctx->num_cu * 8)), dim3(256), 0, ctx->stream, A->n, A->ypart, y);
      break;
    }
    case KS_MAT_LAYOUT_DICT:
    case KS_MAT_LAYOUT_ODICT: {
      // the pair form where the matrix has it (decided at assembly) and both vectors allow 16-byte accesses; read at launch, so a test can run both
      const bool pairs = A->layout == KS_MAT_LAYOUT_DICT && A->pr_ok && !ctx->dbg.no_dict_pairs && pair_aligned16(x) && pair_aligned16(y) && pair_fits32(A->n);
      if (A->layout == KS_MAT_LAYOUT_DICT) { if (pairs) A->pr_launches++; else A->dc_row_launches++; }
      const LaunchGrid lg = dict_launch_grid(A, pairs ? 2 : 1);
      const size_t lds = pairs ? dict_pair_lds_bytes(A) : dict_pattern_lds_bytes(A);
#define SPMV_PAIRS_NB(W, NBT) hipLaunchKernelGGL((k_spmv_dict<W, NBT>), dim3(lg.blocks), dim3(SPMV_BLOCK), lds, ctx->stream, A->n, (const uint4 *)A->dc_codes, A->dc_rowpat, (const uint4 *)A->dc_pats, A->dict_npat, \
                                        A->dc_val, A->dict_nval, A->dc_off, A->dict_noff, x, y, lg.remap, A->pr_args, A->pr_coef, A->pr_mask, gated ? gate->ctl : nullptr, gated ? gate->epoch : 0u)
#define SPMV_PAIRS(W) do { if (A->pr_args.nb <= 5) SPMV_PAIRS_NB(W, 5); else SPMV_PAIRS_NB(W, 9); } while (0)
      if (gated && !pairs) KS_FAIL(KS_ERR_PLIB, "a gated product must take the pair form");
      if (pairs) { KS_DICT_W_SWITCH(A->dict_w, SPMV_PAIRS); break; }             // W is the real one: the last row of an odd n decodes its code word with it
#define SPMV_DICT(W) hipLaunchKernelGGL((k_spmv_dict<W>), dim3(lg.blocks), dim3(SPMV_BLOCK), lds, ctx->stream, A->n, (const uint4 *)A->dc_codes, A->dc_rowpat, (const uint4 *)A->dc_pats, A->dict_npat, \
                                        A->dc_val, A->dict_nval, A->dc_off, A->dict_noff, x, y, lg.remap)
#define SPMV_ODICT(W) hipLaunchKernelGGL((k_spmv_odict<W>), dim3(lg.blocks), dim3(SPMV_BLOCK), 0, ctx->stream, A->n, A->dc_codes8, A->dc_vals, A->dc_off, A->dict_noff, x, y, lg.remap)
      if (A->layout == KS_MAT_LAYOUT_DICT) KS_DICT_W_SWITCH(A->dict_w, SPMV_DICT); else KS_DICT_W_SWITCH(A->dict_w, SPMV_ODICT);
#undef SPMV_DICT
#undef SPMV_ODICT
#undef SPMV_PAIRS
#undef SPMV_PAIRS_NB
      break;
    }
    case KS_MAT_LAYOUT_SELL: {
      const LaunchGrid lg = sell_launch_grid(A);
      hipLaunchKernelGGL((k_spmv_sell<4>), dim3(lg.blocks), dim3(SPMV_BLOCK), 0, ctx->stream, A->n, A->nslices, A->s_ptr, A->s_len, A->s_col, A->s_val, x, y, lg.remap);
      break;
    }
    case KS_MAT_LAYOUT_WINDOW: {
      const LaunchGrid lg = window_launch_grid(A);
      hipLaunchKernelGGL((k_spmv_window<KS_WIN_STEPS>), dim3(lg.blocks), dim3(WIN_ROWS), 0, ctx->stream, A->n, A->d_rowptr, A->wn_codes, A->wn_dcol, A->d_val,
                         A->wn_segptr, A->wn_seg, A->wn_dbase, x, y, lg.remap);
      break;
    }
    case KS_MAT_LAYOUT_BSR: {
      const LaunchGrid lg = bsr_launch_grid(A, 4);
      if (lg.blocks == 0) break;                 // a rank without rows
      if (A->n < 2048) {                         // small matrices: the CSR-vector walk on the blocks, as the CSR layout does below
        const int gpw = 64 / A->lanes_per_row;
        const unsigned nbv = (unsigned)std::max<long long>(1, std::min<long long>(((long long)A->n + 4 * gpw - 1) / (4 * gpw), (long long)ctx->num_cu * 32));
#define SPMV_BSR_VEC(G) hipLaunchKernelGGL((k_spmv_bsr_vec<G>), dim3(nbv), dim3(SPMV_BLOCK), 0, ctx->stream, A->n, A->bsr_bs, A->bsr_rowptr, A->bsr_col, A->bsr_val, x, y)
        switch (A->lanes_per_row) { case 2: SPMV_BSR_VEC(2); break; case 4: SPMV_BSR_VEC(4); break; case 8: SPMV_BSR_VEC(8); break; case 16: SPMV_BSR_VEC(16); break; case 32: SPMV_BSR_VEC(32); break; default: SPMV_BSR_VEC(64); break; }
#undef SPMV_BSR_VEC
        break;
      }
#define SPMV_BSR(BS) hipLaunchKernelGGL((k_spmv_bsr<BS>), dim3(lg.blocks), dim3(256), 0, ctx->stream, A->bsr_nb, A->bsr_rowptr, A->bsr_col, A->bsr_val, x, y, lg.remap)
      KS_BSR_SWITCH(A->bsr_bs, SPMV_BSR);
#undef SPMV_BSR
      break;
    }
    default:                                   // CSR
      if (A->n >= 2048 && A->csr_form != ks_mat_s::CSR_VEC) {
        // 4 or 5 workgroups of 4 waves per CU (registers; forcing 6 spills: 259 us); a multiple of 8 so that every XCD gets its eighth of the rows
        const bool rowside = A->nnz_d <= 12LL * A->n;          // short rows: gather on the row side (register-staged form)
        const bool dma = A->nnz_d <= 16LL * A->n && A->csr_form != ks_mat_s::CSR_REGS;      // the LDS-DMA form gathers on the row side up to 16 entries per row on average
        const LaunchGrid lg = csr_wave_launch_grid(A, rowside ? 5 : 4);
        if (dma) {
          // short rows: the LDS-DMA form (six workgroups of four waves per CU: 144 KB of LDS; 33 registers). 216^3 Laplacian: 191 us against the
          // register-staged form's 207 on the same box (profiles/r04_csr_lds_dma.txt)
          // 64 rows of up to 8 entries fit one 512-entry chunk; up to 12 entries one of 768 (9 KB of LDS per wave: four workgroups per CU), up to 16 one of
          // 1024 (three per CU) - a second chunk per row group is a second serialised DMA wait (rows of 9: 56.6 -> 48.2 us with the wider chunk; beyond
          // 16 entries per row the entry-side register form is as fast or faster: profiles/r04_csr_lds_dma.txt)
          const bool wide = A->nnz_d > 8LL * A->n;
          const bool wider = A->nnz_d > 12LL * A->n;
          const LaunchGrid ld = csr_wave_launch_grid(A, wider ? 3 : wide ? 4 : 6);
          if (wider) hipLaunchKernelGGL((k_spmv_csr_wave_dma<16, 3, 8>), dim3(ld.blocks), dim3(256), 0, ctx->stream, A->n, A->d_rowptr, A->d_col, A->d_val, x, y, ld.remap);
          else if (wide) hipLaunchKernelGGL((k_spmv_csr_wave_dma<12, 4, 8>), dim3(ld.blocks), dim3(256), 0, ctx->stream, A->n, A->d_rowptr, A->d_col, A->d_val, x, y, ld.remap);
          else hipLaunchKernelGGL((k_spmv_csr_wave_dma<8, 6, 8>), dim3(ld.blocks), dim3(256), 0, ctx->stream, A->n, A->d_rowptr, A->d_col, A->d_val, x, y, ld.remap);
        } else if (rowside) hipLaunchKernelGGL((k_spmv_csr_wave<true, 8>), dim3(lg.blocks), dim3(256), 0, ctx->stream, A->n, A->d_rowptr, A->d_col, A->d_val, x, y, lg.remap);
        else hipLaunchKernelGGL((k_spmv_csr_wave<false, 8>), dim3(lg.blocks), dim3(256), 0, ctx->stream, A->n, A->d_rowptr, A->d_col, A->d_val, x, y, lg.remap);
      } else
        launch_spmv<false, false>(ctx->stream, ctx->num_cu, A->lanes_per_row, A->n, A->d_rowptr, A->d_col, A->d_val, x, y, nullptr);
    }
    if (overlap) KS_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_halo, 0));          // also when this rank has no off-diagonal rows: keeps the two streams in step
    if (A->n_orows > 0)
      launch_spmv<true, true>(ctx->stream, ctx->num_cu, 2, A->n_orows, A->o_rowptr, A->o_col, A->o_val, A->ghost, y, A->o_rows);
    if (tail) {
      if (tail_overlap) KS_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_halo, 0));
      KS_CALL(ks_halo_add(ctx->stream, tail->nacc, tail->acc_rows, tail->acc_ptr, tail->acc_pos, tail->rrecv, y));
    }
  }
  KS_HIP(hipGetLastError());
  return KS_SUCCESS;
}

// y = A^T x of a row-sharded A through its view At (MatMultTranspose_MPIAIJ: the transposed off-diagonal block times the local x into a ghost-length
// vector, the transposed diagonal block times x into y, the forward scatter in reverse with ADD). The mirror image of the forward product above:
//   main stream   rsend = Bo^T x   | ev_x |   y = Ad^T x (the view's own layout)   | wait ev_halo |   k_halo_add: y[r] += rrecv[...]
//   halo stream                    | wait ev_x |   exchange rsend -> rrecv (provider)   | ev_halo |
// The ghost rows are short and ragged and x is local: launch_spmv<false, false>, the CSR row walk of the forward path, serves unchanged (two lanes
// per ghost row, as for the forward off-diagonal rows). The exchange is the forward plan with send and receive swapped and ALWAYS the provider's:
// the peer-mapped mailboxes (KS_HALO_PEER) are laid out for the forward direction only, and a matrix with the peer halo active still takes the
// provider here. rsend and rrecv belong to the view, apart from ghost and send_buf: forward and transposed products may alternate freely.
// Back to back: the next product's Bo^T x (main stream) comes behind this one's k_halo_add, which waited for the exchange that read rsend; the next
// exchange (halo stream) waits for the next ev_x, recorded behind this k_halo_add, the last reader of rrecv.
static int mult_sharded_transpose(ks_mat At, const double *x, double *y)
{
  ks_mat A = At->transpose_of;
  ks_ctx ctx = At->ctx;
  const ks_mat_s::ShT *t = At->sht;
  if (A->nsend == 0 && A->nghost == 0) return mult_assembled(At, x, y, nullptr, nullptr, false);      // a rank without peers takes no part in any exchange
  const bool overlap = ctx->halo_overlap;
  if (A->nghost > 0) {
    KsProfScope ps(ctx, KS_K_SPMV, 12.0 * t->nnz_o + 4.0 * (A->nghost + 1) + 8.0 * A->nghost, spmv_variant(At));
    launch_spmv<false, false>(ctx->stream, ctx->num_cu, 2, A->nghost, t->o_rp, t->o_row, t->o_val, x, t->rsend, nullptr);
  }
  hipStream_t hs = ctx->stream;
  if (overlap) {
    KS_CALL(ks_ctx_halo_stream(ctx));
    hs = ctx->halo_stream;
    KS_HIP(hipEventRecord(ctx->ev_x, ctx->stream));
    KS_HIP(hipStreamWaitEvent(hs, ctx->ev_x, 0));
  }
  {
    KsProfScope ps(ctx, KS_K_HALO, 8.0 * (A->nsend + A->nghost));
    KS_CALL(ks_comm_exchange(ctx, (int)A->peers.size(), A->peers.data(), t->rsend, A->recv_off.data(), A->recv_cnt.data(),
                             t->rrecv, A->send_off.data(), A->send_cnt.data(), (int)sizeof(double), hs));
  }
  if (overlap) KS_HIP(hipEventRecord(ctx->ev_halo, hs));
  return mult_assembled(At, x, y, nullptr, t, overlap);
}

int ks_mat_mult_internal(ks_mat A, const double *x, double *y, const double *rowscale, const KsFwdGate *gate)
{
  if (rowscale && !ks_mat_can_rowscale(A)) KS_FAIL(KS_ERR_PLIB, "row scaling asked of a product that cannot fold it in");
  if (gate && gate->ctl) {                           // only the forward form's own eligibility asks for a gate: an assembled one-rank dictionary matrix
    if (A->shell_mult || A->sht || A->layout != KS_MAT_LAYOUT_DICT) KS_FAIL(KS_ERR_PLIB, "a gated product needs the dictionary layout");
    return mult_assembled(A, x, y, nullptr, nullptr, false, gate);
  }
  if (A->shell_mult) return A->shell_mult(A->shell_user, x, y);
  if (A->sht) return mult_sharded_transpose(A, x, y);
  return mult_assembled(A, x, y, rowscale, nullptr, false);
}

extern "C" int ks_mat_mult(ks_mat A, const double *x_dev, double *y_dev)
{
  KS_CHECK(A && x_dev && y_dev, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(x_dev != y_dev, KS_ERR_ARG_WRONG, "x and y must be different vectors");   // MatMult requirement
  KS_HIP(hipSetDevice(A->ctx->device));
  return ks_mat_mult_internal(A, x_dev, y_dev);
}

// MatMultTranspose: through the transposed matrix, built once (MatTranspose on the host, ks_csr.cpp) and multiplied like any other
// The view of a row-sharded matrix created with KS_MAT_SHARDED_TRANSPOSE: the plan (ksc::sharded_transpose_plan, host only, no communication),
// the transposed diagonal block assembled like any matrix - it gets its own layout from the chooser, as the one-rank At does - and the rest of the
// plan with the two exchange buffers on the device
static int upload_ints(const std::vector<int> &h, int **d)
{
  KS_HIP(hipMalloc(d, sizeof(int) * std::max<size_t>(h.size(), 1)));
  if (!h.empty()) KS_HIP(hipMemcpy(*d, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice));
  return KS_SUCCESS;
}
static int build_sharded_transpose(ks_mat A)
{
  ksc::ShardedTransposePlan p;
  try {
    ksc::sharded_transpose_plan(A->n, A->row_start, A->k_rowptr.data(), A->k_col.data(), A->k_val.data(), A->nghost, A->h_ghosts.data(), A->nsend, A->h_send_idx.data(), p);
    for (auto &c : p.d_col) c += A->row_start;                 // the assembly takes global columns
  } catch (const std::exception &e) { KS_FAIL(KS_ERR_MEM, "plan of the transposed product on the host: %s", e.what()); }
  ks_mat At = nullptr;
  KS_CALL(ks_mat_assemble_local(A->ctx, A->n, A->row_start, A->n_global, p.d_rp.data(), p.d_col.data(), p.d_val.data(), &At));
  At->transpose_of = A; A->At = At;                            // from here on A frees it (ks_mat_destroy), half-built or not
  ks_mat_s::ShT *t = At->sht = new ks_mat_s::ShT();
  t->nnz_o = (long long)p.o_row.size(); t->nacc = (int)p.acc_rows.size();
  KS_CALL(upload_ints(p.o_rp, &t->o_rp)); KS_CALL(upload_ints(p.o_row, &t->o_row));
  KS_CALL(upload_ints(p.acc_rows, &t->acc_rows)); KS_CALL(upload_ints(p.acc_ptr, &t->acc_ptr)); KS_CALL(upload_ints(p.acc_pos, &t->acc_pos));
  KS_HIP(hipMalloc(&t->o_val, sizeof(double) * std::max<size_t>(p.o_val.size(), 1)));
  if (!p.o_val.empty()) KS_HIP(hipMemcpy(t->o_val, p.o_val.data(), sizeof(double) * p.o_val.size(), hipMemcpyHostToDevice));
  KS_HIP(hipMalloc(&t->rsend, sizeof(double) * std::max(A->nghost, 1)));
  KS_HIP(hipMalloc(&t->rrecv, sizeof(double) * std::max(A->nsend, 1)));
  return KS_SUCCESS;
}
static int build_transpose(ks_mat A)
{
  if (A->At && (!A->sharded_transpose || (A->At->sht && A->At->sht->rrecv))) return KS_SUCCESS;
  if (A->sharded_transpose && A->keep_csr) {
    KS_CHECK(!A->At, KS_ERR_MEM, "the transposed view of this matrix could not be completed earlier");
    return build_sharded_transpose(A);
  }
  KS_CHECK(A->ctx->comm.size == 1 && A->n == A->n_global, KS_ERR_SUP, "MatMultTranspose of a row-sharded matrix is not built (the transpose is a redistribution)");
  KS_CHECK(A->keep_csr, KS_ERR_ORDER, "MatMultTranspose builds the transpose from the CSR arrays of the matrix: create it with KS_MAT_KEEP_CSR");
  std::vector<int> rp, col; std::vector<double> val;
  try { ksc::csr_transpose(A->n, A->n_global, A->k_rowptr.data(), A->k_col.data(), A->k_val.data(), rp, col, val); }
  catch (const std::exception &e) { KS_FAIL(KS_ERR_MEM, "MatTranspose on the host: %s", e.what()); }
  KS_CALL(ks_mat_create_csr_flags(A->ctx, A->n, 0, A->n_global, rp.data(), col.data(), val.data(), 0u, &A->At));
  A->At->transpose_of = A;
  return KS_SUCCESS;
}
int ks_mat_mult_transpose_internal(ks_mat A, const double *x, double *y)
{
  if (A->shell_mult) {
    KS_CHECK(A->shell_mult_t, KS_ERR_SUP, "the shell matrix has no MATOP_MULT_TRANSPOSE (ks_mat_shell_set_mult_transpose)");
    const int rc = A->shell_mult_t(A->shell_user, x, y);
    KS_CHECK(rc == 0, rc > 0 ? rc : KS_ERR_LIB, "the shell matrix's transposed product returned %d", rc);
    return KS_SUCCESS;
  }
  if (A->transpose_of) return ks_mat_mult_internal(A->transpose_of, x, y);      // a transposed view: its transposed product is the matrix it views
  KS_CALL(build_transpose(A));
  return ks_mat_mult_internal(A->At, x, y);
}
// MatCreateTranspose. Assembled A: the view IS the transposed matrix A keeps for MatMultTranspose (built here if this is its first use), so every
// consumer - ks_mat_mult, the Krylov runs and their product fused into the dot sweep - treats it as the assembled matrix it is. Shell A: a shell
// over the two callbacks swapped.
extern "C" int ks_mat_create_transpose(ks_mat A, ks_mat *At)
{
  KS_CHECK(A && At, KS_ERR_ARG_NULL, "NULL argument");
  KS_HIP(hipSetDevice(A->ctx->device));
  if (A->shell_mult) {
    KS_CHECK(A->shell_mult_t, KS_ERR_SUP, "the shell matrix has no MATOP_MULT_TRANSPOSE (ks_mat_shell_set_mult_transpose)");
    KS_CALL(ks_mat_create_shell(A->ctx, A->n, A->row_start, A->n_global, A->shell_mult_t, A->shell_user, At));
    (*At)->shell_mult_t = A->shell_mult; (*At)->shell_nosync = A->shell_nosync;
    return KS_SUCCESS;
  }
  if (A->transpose_of) { *At = A->transpose_of; return KS_SUCCESS; }                 // the transpose of a view is the matrix itself
  KS_CALL(build_transpose(A));
  *At = A->At;
  return KS_SUCCESS;
}
extern "C" int ks_mat_mult_transpose(ks_mat A, const double *x_dev, double *y_dev)
{
  KS_CHECK(A && x_dev && y_dev, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(x_dev != y_dev, KS_ERR_ARG_WRONG, "x and y must be different vectors");
  KS_HIP(hipSetDevice(A->ctx->device));
  return ks_mat_mult_transpose_internal(A, x_dev, y_dev);
}
extern "C" int ks_mat_shell_set_mult_transpose(ks_mat A, ks_shell_mult_fn mult_transpose)
{
  KS_CHECK(A, KS_ERR_ARG_NULL, "A is NULL");
  KS_CHECK(A->shell_mult, KS_ERR_ARG_WRONG, "not a shell matrix");
  A->shell_mult_t = mult_transpose;
  return KS_SUCCESS;
}

extern "C" int ks_mat_mult_host(ks_mat A, const double *x_host, double *y_host)
{
  KS_CHECK(A && x_host && y_host, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(A->ctx->comm.size == 1, KS_ERR_SUP, "host convenience wrapper is single-rank");
  KS_HIP(hipSetDevice(A->ctx->device));
  double *x = nullptr, *y = nullptr;
  KS_HIP(hipMalloc(&x, sizeof(double) * std::max(A->n_global, 1))); KS_HIP(hipMalloc(&y, sizeof(double) * std::max(A->n, 1)));
  KS_HIP(hipMemcpy(x, x_host, sizeof(double) * A->n_global, hipMemcpyHostToDevice));
  int rc = ks_mat_mult_internal(A, x, y);
  if (!rc) { ks_sync(A->ctx); hipMemcpy(y_host, y, sizeof(double) * A->n, hipMemcpyDeviceToHost); }
  hipFree(x); hipFree(y);
  return rc;
}
