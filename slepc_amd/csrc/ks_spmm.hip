// MatMatMult / MatProductNumeric(AB) with a dense column-major block: Y(:,j) = A X(:,j), j < ncols.
//
// The product behind BVMatMult's MAT method (bvbasic.c:1020-1060, svec.c:210-221): one pass applies the diagonal block to up to
// MM_KB = 8 columns at once, so the matrix is streamed once per pass instead of once per column. Per column a pass moves
// A_bytes / KB + 16 B per row (the x gather and the y store); the column loop moves A_bytes + 16 B per row.
//
// Bit contract: every lane owns one row and runs, for every column of the pass, the single-vector kernel's chain
// acc = fma(a_e, x_e, acc) from 0.0 in entry order - padding entries included exactly where that kernel has them (the dictionary
// forms and SELL-64 fma 0.0 * 0.0, the CSR row blocks skip them). So Y(:,j) is ks_mat_mult(A, X(:,j)) bit for bit, NaN, Inf and the
// +0.0 of an empty row included. Layouts and forms without such a kernel (BINNED, SLICED, shell matrices, the CSR-vector form of small
// matrices, anything with a halo) run the column loop over ks_mat_mult_internal: the same bits by construction.
#include "ks_rows.cuh"
#include <cstdlib>
#include <cstring>

namespace {
using namespace ksr;

constexpr int MM_BLOCK = ROW_BLOCK;
constexpr int MM_KB = 8;                // columns per pass (KB accumulators per lane); every KB from 1 to 8 is compiled for the tail

// ---- dictionary ELL (k_spmv_dict's storage, either form): a row's codes are decoded once, each entry gathers its KB x values ---------------------
template <int W, int KB>
__global__ __launch_bounds__(MM_BLOCK) void k_spmm_dict(int nrows, const uint4 *__restrict__ codes, const unsigned char *__restrict__ rowpat, const uint4 *__restrict__ pats, int npat, const double *__restrict__ dval, int nval, const int *__restrict__ doff, int noff,
                                                        const double *__restrict__ X, long long ldx, double *__restrict__ Y, long long ldy, int xcd_remap)
{
  __shared__ double sv[256];
  __shared__ int so[256];
  KS_DICT_LDS_FILL(MM_BLOCK, W, sv, so, dval, nval, doff, noff, rowpat, pats, npat);
  constexpr int Q = W / 8;
  const RowGroups rg = row_groups_xcd(nrows, MM_BLOCK, xcd_remap);
  for (long long g = rg.g0 + rg.lb; g < rg.g1; g += rg.nb) {
    const long long r = g * MM_BLOCK + threadIdx.x;
    if (r >= nrows) break;
    double acc[KB];
#pragma unroll
    for (int k = 0; k < KB; k++) acc[k] = 0.0;
    const int p = rowpat ? rowpat[r] : 0;
#pragma unroll 1
    for (int q = 0; q < Q; q++) {                           // eight entries at a time: 8 KB gathers in flight, not W KB
      const uint4 c = rowpat ? dict_pat_lds[p * Q + q] : ksk::ldstream4(codes + r * Q + q);
      const unsigned wds[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const DictCode d = dict_code(wds[e >> 1], e);
        const bool ok = d.ok;
        const double a = ok ? sv[d.vc] : 0.0;
        const long long xi = r + (ok ? so[d.oc] : 0);
#pragma unroll
        for (int k = 0; k < KB; k++) acc[k] = fma(a, ok ? X[k * ldx + xi] : 0.0, acc[k]);      // padding: fma(0.0, 0.0, acc) as in k_spmv_dict
      }
    }
#pragma unroll
    for (int k = 0; k < KB; k++) __builtin_nontemporal_store(acc[k], Y + k * ldy + r);
  }
}

// ---- offset-dictionary ELL (k_spmv_odict's storage) ------------------------------------------------------------------------------
template <int W, int KB>
__global__ __launch_bounds__(MM_BLOCK) void k_spmm_odict(int nrows, const unsigned char *__restrict__ codes, const double *__restrict__ vals, const int *__restrict__ doff, int noff,
                                                         const double *__restrict__ X, long long ldx, double *__restrict__ Y, long long ldy, int xcd_remap)
{
  __shared__ int so[256];
  lds_fill<MM_BLOCK>(so, doff, noff);
  __syncthreads();
  const RowGroups rg = row_groups_xcd(nrows, MM_BLOCK, xcd_remap);
  for (long long g = rg.g0 + rg.lb; g < rg.g1; g += rg.nb) {
    const long long r = g * MM_BLOCK + threadIdx.x;
    if (r >= nrows) break;
    const double *vb = vals + ((r >> 6) * W) * 64 + (r & 63);
    double acc[KB];
#pragma unroll
    for (int k = 0; k < KB; k++) acc[k] = 0.0;
#pragma unroll 1
    for (int e8 = 0; e8 < W; e8 += 8) {                     // eight entries at a time (their codes: one 8-byte load)
      const uint2 cw = *reinterpret_cast<const uint2 *>(codes + r * W + e8);
      const unsigned wds[2] = {cw.x, cw.y};
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const DictCode d = odict_code(wds[e >> 2], e);
        const bool ok = d.ok;
        const double a = ok ? ksk::ldstream(vb + (long long)(e8 + e) * 64) : 0.0;
        const long long xi = r + (ok ? so[d.oc] : 0);
#pragma unroll
        for (int k = 0; k < KB; k++) acc[k] = fma(a, ok ? X[k * ldx + xi] : 0.0, acc[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < KB; k++) __builtin_nontemporal_store(acc[k], Y + k * ldy + r);
  }
}

// ---- SELL-64 (k_spmv_sell's entry pairs): batches of MM_UNR pairs, predicated as there, so the padding fmas fall where they fall in
// k_spmv_sell<4> ------------------------------------------------------------------------------------------------------------------
constexpr int MM_UNR = 4;
template <int KB>
__global__ __launch_bounds__(MM_BLOCK) void k_spmm_sell(int nrows, int nslices, const int *__restrict__ sp, const int *__restrict__ rlen,
                                                        const int *__restrict__ col, const double *__restrict__ val,
                                                        const double *__restrict__ X, long long ldx, double *__restrict__ Y, long long ldy, int xcd_remap)
{
  const int lane = threadIdx.x & 63;
  const int wpb = MM_BLOCK / 64;
  const long long nsb = ((long long)nslices + wpb - 1) / wpb;     // slice groups
  const long long nblk = gridDim.x;
  for (long long g = sell_first_group(nblk, xcd_remap); g < nsb; g += nblk) {
    const long long s = g * wpb + (threadIdx.x >> 6);
    if (s >= nslices) continue;
    const long long r = s * 64 + lane;
    const int w = sp[s + 1] - sp[s], wp = w >> 1;
    const int len = (r < nrows) ? rlen[r] : 0;
    const long long sb = (long long)sp[s] * 64;
    double acc[KB];
#pragma unroll
    for (int k = 0; k < KB; k++) acc[k] = 0.0;
    for (int q = 0; q < wp; q += MM_UNR) {
      ks_i2v c[MM_UNR]; ksk::ks_d2v a[MM_UNR];
      KS_SELL_LOAD_PAIRS(MM_UNR, c, a, col, val, sb, q, wp, len, lane)
#pragma unroll
      for (int u = 0; u < MM_UNR; u++) {
#pragma unroll
        for (int k = 0; k < KB; k++) {
          const double x0 = c[u].x >= 0 ? X[k * ldx + c[u].x] : 0.0, x1 = c[u].y >= 0 ? X[k * ldx + c[u].y] : 0.0;
          acc[k] = fma(a[u].x, x0, acc[k]); acc[k] = fma(a[u].y, x1, acc[k]);
        }
      }
    }
    if (w & 1) {
      const SellEntry t = sell_tail(col, val, sb, w, len, lane);
#pragma unroll
      for (int k = 0; k < KB; k++) acc[k] = fma(t.a, t.c >= 0 ? X[k * ldx + t.c] : 0.0, acc[k]);
    }
    if (r < nrows) {
#pragma unroll
      for (int k = 0; k < KB; k++) __builtin_nontemporal_store(acc[k], Y + k * ldy + r);
    }
  }
}

// ---- CSR row blocks: k_spmv_csr_wave_dma's staging (a wave owns 64 rows, their col / val run goes chunk by chunk straight into a
// wave-private piece of LDS), lane = row, KB chains per lane -----------------------------------------------------------------------
// IL: where an entry's KB x values come from. false (direct): the column-major block, KB separate gathers (KB cache lines for a
// scattered column). true (interleaved): a row-major n x KB copy of the pass's columns (k_spmm_pack, owned by the matrix), so one
// entry's KB values are one run of 8 KB bytes.
template <int KB, bool IL>
__device__ __forceinline__ void mm_gather(double (&xv)[KB], const double *__restrict__ X, long long ldx, int c, bool ok)
{
  if (IL && KB % 2 == 0) {
#pragma unroll
    for (int k = 0; k < KB; k += 2) {
      const ksk::ks_d2v t = ok ? *reinterpret_cast<const ksk::ks_d2v *>(X + (long long)c * KB + k) : ksk::ks_d2v{0.0, 0.0};
      xv[k] = t.x; xv[k + 1] = t.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < KB; k++) xv[k] = ok ? (IL ? X[(long long)c * KB + k] : X[k * ldx + c]) : 0.0;
  }
}
constexpr int MM_CH = 512;           // entries per chunk (as k_spmv_csr_wave_dma<8, ...>): 6 KB of LDS per wave
constexpr int MM_GU = 2;             // entries whose KB gathers are in flight per lane
template <int KB, bool IL>
__global__ __launch_bounds__(256, 4) void k_spmm_csr(int n, const int *__restrict__ rp, const int *__restrict__ col, const double *__restrict__ val,
                                                     const double *__restrict__ X, long long ldx, double *__restrict__ Y, long long ldy, int xcd_remap)
{
  __shared__ __attribute__((aligned(16))) double sa_all[4][MM_CH];
  __shared__ __attribute__((aligned(16))) int sc_all[4][MM_CH];
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
    double acc[KB];
#pragma unroll
    for (int k = 0; k < KB; k++) acc[k] = 0.0;
    for (int e0 = cu.E0 & ~3; e0 < cu.E1; e0 += MM_CH) {
      cw_dma_chunk<MM_CH>(sa, sc, col, val, e0, cu.E1, lane);
      const int lo = max(cu.p0, e0), hi = min(cu.p1, e0 + MM_CH);
      for (int p = lo; __builtin_amdgcn_ballot_w64(p < hi) != 0; p += MM_GU) {
        double av[MM_GU], xv[MM_GU][KB];
#pragma unroll
        for (int j = 0; j < MM_GU; j++) {
          const bool ok = p + j < hi;
          const int sl = ok ? p + j - e0 : 0;
          av[j] = sa[sl];
          mm_gather<KB, IL>(xv[j], X, ldx, ok ? sc[sl] : 0, ok);
        }
#pragma unroll
        for (int j = 0; j < MM_GU; j++)
          if (p + j < hi) {
#pragma unroll
            for (int k = 0; k < KB; k++) acc[k] = fma(av[j], xv[j][k], acc[k]);
          }
      }
    }
    if (cu.has) {
#pragma unroll
      for (int k = 0; k < KB; k++) __builtin_nontemporal_store(acc[k], Y + k * ldy + cu.r);
    }
    g += gstep;
    if (g >= gend) break;
    cu = nx;
    nx = g + gstep < gend ? cw_rows(n, rp, g + gstep, w, lane) : CwRows{0, 0, 0, 0, 0, false};
  }
}

// ---- block CSR (k_spmv_bsr's storage and walk, bsr_walk in ks_rows.cuh): KB chains per lane, the x of a (block, c) item gathered for every column of
// the pass and parked side by side, so a row lane reads one value and KB consecutive x per fma set. Chunks of half the single-vector kernel's blocks: with
// 8 columns the parked x of a full chunk would be up to 10.5 KB per wave next to 4 KB of values (58 KB per workgroup: two per CU); halved, a workgroup
// holds at most 29 KB and the 94 registers of the widest form decide: five waves per SIMD. KB = 8 - registers and LDS allow it - or 4 for passes of up
// to four columns (half the parked x, 62-80 registers); the columns past kb are neither gathered nor stored.
template <int BS, int KB>
__global__ __launch_bounds__(256, 3) void k_spmm_bsr(int nb, const int *__restrict__ brp, const int *__restrict__ bcol, const double *__restrict__ val,
                                                     const double *__restrict__ X, long long ldx, double *__restrict__ Y, long long ldy, int kb, int xcd_remap)
{
  constexpr int NBK = bsr_chunk_blocks(BS) / 2;
  __shared__ __attribute__((aligned(16))) double sa_all[4][128 * BsrRegs<BS, NBK>::STEPS];
  __shared__ __attribute__((aligned(16))) double sx_all[4][NBK * BS * KB];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  bsr_walk<BS, KB, NBK>(sa_all[w], sx_all[w], nb, brp, bcol, val, X, ldx, Y, ldy, kb, xcd_remap);
}

// X(:, 0:KB) column-major -> Xi (n x KB, row-major): thread = row; the loads of a column and the stores of a row block are contiguous
template <int KB>
__global__ __launch_bounds__(256) void k_spmm_pack(int n, const double *__restrict__ X, long long ldx, double *__restrict__ Xi)
{
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  double v[KB];
#pragma unroll
  for (int k = 0; k < KB; k++) v[k] = X[k * ldx + r];
#pragma unroll
  for (int k = 0; k < KB; k++) Xi[r * KB + k] = v[k];
}

#define MM_KB_SWITCH(kb, F) \
  switch (kb) { case 1: F(1); break; case 2: F(2); break; case 3: F(3); break; case 4: F(4); break; case 5: F(5); break; case 6: F(6); break; case 7: F(7); break; default: F(8); break; }

// The CSR gather form: interleaved where rows are long enough for the gathers to bind - more than 12 entries per row on average, the
// threshold above which ks_mat_mult_internal gathers on the entry side (profiles/r05_spmm.txt times both forms on both sides of it).
// KSGPU_SPMM=direct|interleaved forces one (A/B legs of scripts/spmm_probe.py; read at every pass).
bool csr_interleaved(ks_mat A)
{
  const char *force = getenv("KSGPU_SPMM");
  if (force && !strcmp(force, "direct")) return false;
  if (force && !strcmp(force, "interleaved")) return true;
  return A->nnz_d > 12LL * A->n;
}

// one pass over kb <= MM_KB columns; the caller has ruled out every layout and form the column loop takes
int spmm_pass(ks_mat A, int kb, const double *X, long long ldx, double *Y, long long ldy)
{
  ks_ctx ctx = A->ctx;
  const bool il = A->layout == KS_MAT_LAYOUT_CSR && csr_interleaved(A);
  if (il && !A->mm_xi) {
    const size_t bytes = sizeof(double) * (size_t)A->n * MM_KB;         // the widest pass: allocated once, freed by ks_mat_destroy
    if (hipMalloc(&A->mm_xi, bytes) != hipSuccess) { A->mm_xi = nullptr; KS_FAIL(KS_ERR_MEM, "hipMalloc of the interleaved block (%zu bytes) failed", bytes); }
  }
  // algorithmic bytes A_bytes + 16 n KB with the CSR stream as A_bytes (as ks_mat_mult_internal counts), the layout's own next to them
  const double xy = 16.0 * A->n * kb;
  const double alg = 12.0 * A->nnz_d + 4.0 * (A->n + 1) + xy;
  int variant = il ? KS_SPMM_CSR_IL : KS_SPMM_CSR;
  switch (A->layout) {
  case KS_MAT_LAYOUT_DICT: variant = KS_SPMM_DICT; break;
  case KS_MAT_LAYOUT_ODICT: variant = KS_SPMM_ODICT; break;
  case KS_MAT_LAYOUT_SELL: variant = KS_SPMM_SELL; break;
  case KS_MAT_LAYOUT_BSR: variant = KS_SPMM_BSR; break;
  }
  KsProfScope ps(ctx, KS_K_SPMV, alg, variant, layout_own_bytes(A) + (il ? 2.0 : 1.0) * xy);      // interleaved: the pack reads the pass's columns and writes them once more
  switch (A->layout) {
  case KS_MAT_LAYOUT_DICT:
  case KS_MAT_LAYOUT_ODICT: {
    const LaunchGrid lg = dict_launch_grid(A);
    const size_t lds = dict_pattern_lds_bytes(A);
#define MM_DICT_W(W) hipLaunchKernelGGL((k_spmm_dict<W, MM_DICT_KB>), dim3(lg.blocks), dim3(MM_BLOCK), lds, ctx->stream, A->n, (const uint4 *)A->dc_codes, A->dc_rowpat, (const uint4 *)A->dc_pats, A->dict_npat, A->dc_val, A->dict_nval, A->dc_off, A->dict_noff, X, ldx, Y, ldy, lg.remap)
#define MM_ODICT_W(W) hipLaunchKernelGGL((k_spmm_odict<W, MM_DICT_KB>), dim3(lg.blocks), dim3(MM_BLOCK), 0, ctx->stream, A->n, A->dc_codes8, A->dc_vals, A->dc_off, A->dict_noff, X, ldx, Y, ldy, lg.remap)
#define MM_DICT(KB) { constexpr int MM_DICT_KB = KB; if (A->layout == KS_MAT_LAYOUT_DICT) KS_DICT_W_SWITCH(A->dict_w, MM_DICT_W); else KS_DICT_W_SWITCH(A->dict_w, MM_ODICT_W); }
    MM_KB_SWITCH(kb, MM_DICT);
#undef MM_DICT
#undef MM_DICT_W
#undef MM_ODICT_W
    break;
  }
  case KS_MAT_LAYOUT_SELL: {
    const LaunchGrid lg = sell_launch_grid(A);
#define MM_SELL(KB) hipLaunchKernelGGL((k_spmm_sell<KB>), dim3(lg.blocks), dim3(MM_BLOCK), 0, ctx->stream, A->n, A->nslices, A->s_ptr, A->s_len, A->s_col, A->s_val, X, ldx, Y, ldy, lg.remap)
    MM_KB_SWITCH(kb, MM_SELL);
#undef MM_SELL
    break;
  }
  case KS_MAT_LAYOUT_BSR: {
    const LaunchGrid lg = bsr_launch_grid(A, 3);
    if (lg.blocks == 0) break;
#define MM_BSR(BS) do { if (kb <= 4) hipLaunchKernelGGL((k_spmm_bsr<BS, 4>), dim3(lg.blocks), dim3(256), 0, ctx->stream, A->bsr_nb, A->bsr_rowptr, A->bsr_col, A->bsr_val, X, ldx, Y, ldy, kb, lg.remap); \
                        else hipLaunchKernelGGL((k_spmm_bsr<BS, 8>), dim3(lg.blocks), dim3(256), 0, ctx->stream, A->bsr_nb, A->bsr_rowptr, A->bsr_col, A->bsr_val, X, ldx, Y, ldy, kb, lg.remap); } while (0)
    KS_BSR_SWITCH(A->bsr_bs, MM_BSR);
#undef MM_BSR
    break;
  }
  default: {                                                                      // CSR row blocks (n >= 2048, not the CSR-vector form)
    const LaunchGrid lg = csr_wave_launch_grid(A, 4);
    const dim3 gr(lg.blocks);
    const int remap = lg.remap;
    const unsigned npk = (unsigned)((A->n + 255) / 256);
#define MM_CSR(KB)                                                                                                                                                    \
  if (il) {                                                                                                                                                           \
    hipLaunchKernelGGL((k_spmm_pack<KB>), dim3(npk), dim3(256), 0, ctx->stream, A->n, X, ldx, A->mm_xi);                                                            \
    hipLaunchKernelGGL((k_spmm_csr<KB, true>), gr, dim3(256), 0, ctx->stream, A->n, A->d_rowptr, A->d_col, A->d_val, (const double *)A->mm_xi, ldx, Y, ldy, remap); \
  } else hipLaunchKernelGGL((k_spmm_csr<KB, false>), gr, dim3(256), 0, ctx->stream, A->n, A->d_rowptr, A->d_col, A->d_val, X, ldx, Y, ldy, remap)
    MM_KB_SWITCH(kb, MM_CSR);
#undef MM_CSR
    break;
  }
  }
  KS_HIP(hipGetLastError());
  return KS_SUCCESS;
}

} // namespace

// The one dispatch of the block product (a switch on A->layout, as in ks_mat_mult_internal): passes of up to MM_KB columns where a
// block kernel exists, the column loop everywhere else - BINNED, SLICED and WINDOW, whose column indices no longer exist as d_col (spmm_pass must
// never see them: its default branch is the CSR block kernel)
int ks_mat_mult_multi_internal(ks_mat A, int ncols, const double *X, int ldx, double *Y, int ldy)
{
  if (ncols <= 0) return KS_SUCCESS;
  ks_ctx ctx = A->ctx;
  const bool halo = ctx->comm.size > 1 && (A->nsend > 0 || A->nghost > 0);       // several columns through the halo at once: not built
  bool loop = ncols == 1 || A->shell_mult || halo || A->n_orows > 0 || A->sht;      // sht: the transposed view of a row-sharded matrix, a reverse exchange per column
  switch (A->layout) {
  case KS_MAT_LAYOUT_DICT: case KS_MAT_LAYOUT_ODICT: case KS_MAT_LAYOUT_SELL: break;
  case KS_MAT_LAYOUT_BSR: if (A->n < 2048) loop = true; break;                                           // small block matrices: the vector form (k_spmv_bsr_vec), as for CSR below
  case KS_MAT_LAYOUT_CSR: if (A->n < 2048 || A->csr_form == ks_mat_s::CSR_VEC) loop = true; break;      // the CSR-vector kernel: its sums are not in entry order
  case KS_MAT_LAYOUT_WINDOW: loop = true; break;                                                          // no block kernel: spmm_pass's default is the CSR block kernel, which would read the released d_col
  default: loop = true; break;                                                                            // BINNED, SLICED
  }
  if (loop) {
    for (int j = 0; j < ncols; j++) KS_CALL(ks_mat_mult_internal(A, X + (size_t)j * ldx, Y + (size_t)j * ldy));
    return KS_SUCCESS;
  }
  for (int j0 = 0; j0 < ncols; j0 += MM_KB) KS_CALL(spmm_pass(A, std::min(MM_KB, ncols - j0), X + (size_t)j0 * ldx, ldx, Y + (size_t)j0 * ldy, ldy));
  return KS_SUCCESS;
}

extern "C" int ks_mat_mult_multi(ks_mat A, int ncols, const double *X_dev, int ldx, double *Y_dev, int ldy)
{
  KS_CHECK(A && X_dev && Y_dev, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(ncols >= 0, KS_ERR_ARG_OUTOFRANGE, "Number of columns %d must be non-negative", ncols);
  KS_CHECK(ldx >= std::max(1, A->n) && ldy >= std::max(1, A->n), KS_ERR_ARG_SIZ, "Leading dimensions ldx %d, ldy %d must be at least %d (local rows)", ldx, ldy, std::max(1, A->n));
  if (ncols == 0) return KS_SUCCESS;
  const uintptr_t x0 = (uintptr_t)X_dev, x1 = x0 + sizeof(double) * ((size_t)(ncols - 1) * ldx + A->n);
  const uintptr_t y0 = (uintptr_t)Y_dev, y1 = y0 + sizeof(double) * ((size_t)(ncols - 1) * ldy + A->n);
  KS_CHECK(X_dev != Y_dev && (x1 <= y0 || y1 <= x0), KS_ERR_ARG_WRONG, "X and Y must be different blocks: they overlap");      // MatMult's x != y, for blocks
  KS_HIP(hipSetDevice(A->ctx->device));
  return ks_mat_mult_multi_internal(A, ncols, X_dev, ldx, Y_dev, ldy);
}
