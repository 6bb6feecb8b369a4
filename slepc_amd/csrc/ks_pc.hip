// Block Jacobi with ILU(0) blocks (KS_PC_BJACOBI_ILU): PCBJACOBI with -sub_pc_type ilu, PETSc's parallel default for AIJ matrices, as the left
// preconditioner of the ST's KSP (ks_st.hip). The factors and their level schedule are made on the host (ksc::csr_ilu0_blocks, ks_csr.cpp: the
// layout is described there); this file uploads them and applies them: y = U^-1 L^-1 x block by block, and - on request, from a second plan of the
// same factors - the transposed preconditioner y = L^-T U^-T x (PCApplyTranspose).
#include "ksgpu_internal.h"
#include "ks_csr.h"
#include <algorithm>

struct KsIlu {
  int n = 0, bs = 0, nblk = 0, longest_row = 0;
  long long levels = 0, entries = 0;
  ksc::IluBlock *blk = nullptr; int2 *lev = nullptr;
  double *val = nullptr, *dinv = nullptr;
  unsigned short *code = nullptr, *rows = nullptr;
  KsIlu *t = nullptr;          // the plan of the transposed triangles (ks_pc_ilu_build with transpose): same factors, owned
};

namespace {
// 256 lanes: four waves, one per SIMD of the CU. What a block can run in parallel is the width of a level, and the levels of stencil blocks in
// natural ordering are tens to a few hundred rows wide, so a wider workgroup would add waves that idle at every barrier and lengthen the barrier
// itself; a single wave (whose barrier is free) strides four times as long over the wide levels and over the copy in and out. With 64 KB of LDS
// at the largest block two workgroups stay resident per CU, two waves per SIMD: one block's barrier waits overlap the other's gathers.
constexpr int ILU_THREADS = 256;

// One workgroup per block, no atomics, nothing shared between workgroups: the block's piece of `in` goes to LDS, the L levels and then the U
// levels update it in place with one barrier between levels, the piece goes out. A lane takes a row of the level: acc = sum v * x[c] by fma
// in slot order, then x[r] -= acc (L, unit diagonal) or x[r] = (x[r] - acc) * dinv (U). Rows of one level read only rows of earlier levels
// (padding reads the row's own x[r]), so the order of the lanes does not matter and the result is the same bits from run to run.
// Memory: the slot-major ELL image makes consecutive lanes read consecutive values (8 B) and codes (2 B); the level descriptors are read one
// level ahead of the barrier that needs them. LDS: x[c] is a gather of 8-byte words (ds_read_b64: 64 banks of 4 bytes, conflicts counted inside
// each half of the wave); lanes p, p + 1 of a level in a stencil block read columns a constant stride apart, conflict-free when that stride
// is odd - the diagonal wavefronts of a grid line of even length - and two-way when it is 2 mod 4. x[r] of the row lists is written in
// ascending row order, near-consecutive words.
// TRANS: the plan of the transposed triangles (ks_csr.h). The walk is the same; the run of levels that carries the pivots is the first one (U^T, lower
// triangular: x[r] = (x[r] - sum_{c<r} u_cr x[c]) / u_rr), the unit triangle (L^T, upper) comes second, and dinv is in the first run's level order.
template <bool TRANS>
__device__ __forceinline__ void ilu_level_walk(int n, int bs, const ksc::IluBlock *__restrict__ blk, const int2 *__restrict__ lev,
                                               const double *__restrict__ val, const unsigned short *__restrict__ code,
                                               const unsigned short *__restrict__ rows, const double *__restrict__ dinv,
                                               const double *__restrict__ in, double *__restrict__ out)
{
  extern __shared__ double xs[];
  const int tid = threadIdx.x;
  const long long b0 = (long long)blockIdx.x * bs;
  const int bl = (int)std::min<long long>(bs, n - b0);
  for (int i = tid; i < bl; i += ILU_THREADS) xs[i] = in[b0 + i];
  const ksc::IluBlock B = blk[blockIdx.x];
  const double *v = val + B.ell; const unsigned short *c = code + B.ell;
  const unsigned short *rw = rows + 2 * b0; const double *dv = dinv + b0;
  const int2 *lv = lev + B.lev;
  const int nlev = B.nL + B.nU;
  int2 d = lv[0];
  __syncthreads();
  for (int l = 0; l < nlev; l++) {
    const int2 next = (l + 1 < nlev) ? lv[l + 1] : make_int2(0, 0);
    const int nl = d.x, w = d.y;
    const bool upper = TRANS ? l < B.nL : l >= B.nL;            // the run of levels with the pivots
    for (int i = tid; i < nl; i += ILU_THREADS) {
      const int r = rw[i];
      double acc = 0.0;
      for (int s = 0; s < w; s++) acc = fma(v[(size_t)s * nl + i], xs[c[(size_t)s * nl + i]], acc);
      const double t = xs[r] - acc;
      xs[r] = upper ? t * dv[i] : t;
    }
    v += (size_t)nl * w; c += (size_t)nl * w; rw += nl; if (upper) dv += nl;
    d = next;
    __syncthreads();
  }
  for (int i = tid; i < bl; i += ILU_THREADS) out[b0 + i] = xs[i];
}
__global__ void __launch_bounds__(ILU_THREADS) k_bjacobi_ilu_apply(int n, int bs, const ksc::IluBlock *__restrict__ blk, const int2 *__restrict__ lev,
                                                                   const double *__restrict__ val, const unsigned short *__restrict__ code,
                                                                   const unsigned short *__restrict__ rows, const double *__restrict__ dinv,
                                                                   const double *__restrict__ in, double *__restrict__ out)
{
  ilu_level_walk<false>(n, bs, blk, lev, val, code, rows, dinv, in, out);
}
// y = L^-T U^-T x from the transposed plan
__global__ void __launch_bounds__(ILU_THREADS) k_bjacobi_ilu_apply_t(int n, int bs, const ksc::IluBlock *__restrict__ blk, const int2 *__restrict__ lev,
                                                                     const double *__restrict__ val, const unsigned short *__restrict__ code,
                                                                     const unsigned short *__restrict__ rows, const double *__restrict__ dinv,
                                                                     const double *__restrict__ in, double *__restrict__ out)
{
  ilu_level_walk<true>(n, bs, blk, lev, val, code, rows, dinv, in, out);
}

// NC right-hand sides of a block at once (ks_st_pc_apply_multi: the preconditioned residuals of a block eigensolver). The walk is ilu_level_walk<false>:
// a lane still owns a row of the level, now with NC accumulators; every factor value and 16-bit code is read ONCE for all columns, each column runs
// the same fma chain in the same slot order - the bits of k_bjacobi_ilu_apply column by column - and a level costs one barrier instead of NC.
// LDS layout: column-major, column j of the block at xs + j * bs. The gather xs[j * bs + c] of one column is then the single-vector kernel's gather
// shifted by a constant, so the bank-conflict argument above holds per instruction unchanged (lanes p, p + 1 a constant stride apart: conflict-free
// for odd strides, two-way for 2 mod 4). Interleaving the columns (xs[c * NC + j]) would multiply every lane stride by NC: with NC = 8 all 8-byte
// words of a column fall on 4 of the 32 bank pairs, an eight-way conflict on every gather; the one thing it would buy, two columns per
// ds_read_b128, costs four LDS cycles where two ds_read_b64 cost the same four.
template <int NC>
__global__ void __launch_bounds__(ILU_THREADS) k_bjacobi_ilu_apply_multi(int n, int bs, const ksc::IluBlock *__restrict__ blk, const int2 *__restrict__ lev,
                                                                         const double *__restrict__ val, const unsigned short *__restrict__ code,
                                                                         const unsigned short *__restrict__ rows, const double *__restrict__ dinv,
                                                                         const double *__restrict__ in, long long ldin, double *__restrict__ out, long long ldout)
{
  extern __shared__ double xs[];
  const int tid = threadIdx.x;
  const long long b0 = (long long)blockIdx.x * bs;
  const int bl = (int)std::min<long long>(bs, n - b0);
#pragma unroll
  for (int j = 0; j < NC; j++) for (int i = tid; i < bl; i += ILU_THREADS) xs[j * bs + i] = in[j * ldin + b0 + i];
  const ksc::IluBlock B = blk[blockIdx.x];
  const double *v = val + B.ell; const unsigned short *c = code + B.ell;
  const unsigned short *rw = rows + 2 * b0; const double *dv = dinv + b0;
  const int2 *lv = lev + B.lev;
  const int nlev = B.nL + B.nU;
  int2 d = lv[0];
  __syncthreads();
  for (int l = 0; l < nlev; l++) {
    const int2 next = (l + 1 < nlev) ? lv[l + 1] : make_int2(0, 0);
    const int nl = d.x, w = d.y;
    const bool upper = l >= B.nL;
    for (int i = tid; i < nl; i += ILU_THREADS) {
      const int r = rw[i];
      double acc[NC];
#pragma unroll
      for (int j = 0; j < NC; j++) acc[j] = 0.0;
      for (int s = 0; s < w; s++) {
        const double vv = v[(size_t)s * nl + i]; const int cc = c[(size_t)s * nl + i];
#pragma unroll
        for (int j = 0; j < NC; j++) acc[j] = fma(vv, xs[j * bs + cc], acc[j]);
      }
      const double dd = upper ? dv[i] : 1.0;
#pragma unroll
      for (int j = 0; j < NC; j++) { const double t = xs[j * bs + r] - acc[j]; xs[j * bs + r] = upper ? t * dd : t; }
    }
    v += (size_t)nl * w; c += (size_t)nl * w; rw += nl; if (upper) dv += nl;
    d = next;
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < NC; j++) for (int i = tid; i < bl; i += ILU_THREADS) out[j * ldout + b0 + i] = xs[j * bs + i];
}

template <class T> int upload(ks_ctx ctx, T **dst, const void *src, size_t count)
{
  KS_HIP(hipMalloc((void **)dst, sizeof(T) * std::max<size_t>(count, 1)));
  if (count) KS_HIP(hipMemcpyAsync(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice, ctx->stream));
  return KS_SUCCESS;
}
} // namespace

void ks_pc_ilu_free(KsIlu *p)
{
  if (!p) return;
  ks_pc_ilu_free(p->t);
  hipFree(p->blk); hipFree(p->lev); hipFree(p->val); hipFree(p->dinv); hipFree(p->code); hipFree(p->rows);
  delete p;
}

namespace {
// one plan on the device; the kernel that walks it may have 64 KB of dynamic LDS (the largest block)
int upload_plan(ks_ctx ctx, int n, int bs, const ksc::IluPlan &plan, const void *kernel, const char *kname, KsIlu **out)
{
  KsIlu *p = new KsIlu();
  p->n = n; p->bs = bs; p->nblk = (int)plan.blk.size(); p->longest_row = plan.longest_row; p->levels = (long long)plan.lev.size() / 2; p->entries = (long long)plan.val.size();
  int rc = upload(ctx, &p->blk, plan.blk.data(), plan.blk.size());
  if (!rc) rc = upload(ctx, &p->lev, plan.lev.data(), plan.lev.size() / 2);
  if (!rc) rc = upload(ctx, &p->val, plan.val.data(), plan.val.size());
  if (!rc) rc = upload(ctx, &p->code, plan.code.data(), plan.code.size());
  if (!rc) rc = upload(ctx, &p->rows, plan.rows.data(), plan.rows.size());
  if (!rc) rc = upload(ctx, &p->dinv, plan.dinv.data(), plan.dinv.size());
  if (!rc) { hipError_t e = ks_sync(ctx); if (e != hipSuccess) { ks_set_error("ILU(0) block set-up: %s", hipGetErrorString(e)); rc = KS_ERR_LIB; } }      // the plan's vectors go out of scope
  if (!rc) { hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(double) * ksc::ILU_BS_MAX);
             if (e != hipSuccess) { ks_set_error("hipFuncSetAttribute(%s) failed: %s", kname, hipGetErrorString(e)); rc = KS_ERR_LIB; } }
  if (rc) { ks_pc_ilu_free(p); return rc; }
  *out = p;
  return KS_SUCCESS;
}
} // namespace

int ks_pc_ilu_build(ks_ctx ctx, int n, int row_start, int bs, const int *rp, const int *col, const double *val, bool transpose, KsIlu **out)
{
  static_assert(sizeof(ksc::IluBlock) == 24, "the kernel reads the host's block records as they are");
  KS_CHECK(bs >= 64 && bs <= ksc::ILU_BS_MAX, KS_ERR_ARG_OUTOFRANGE, "block size %d (64..%d)", bs, ksc::ILU_BS_MAX);
  ksc::IluPlan plan, tplan;
  try { ksc::csr_ilu0_blocks(n, row_start, bs, rp, col, val, false, plan, transpose ? &tplan : nullptr); }
  catch (const std::exception &e) { KS_FAIL(KS_ERR_MEM, "ILU(0) block set-up: %s", e.what()); }
  KS_CHECK(plan.status != ksc::ILU_NO_DIAGONAL, KS_ERR_ARG_WRONGSTATE, "Matrix is missing diagonal entry in local row %d (block %d of the block-Jacobi preconditioner)", plan.bad_row, plan.bad_block);
  KS_CHECK(plan.status != ksc::ILU_ZERO_PIVOT, KS_ERR_MAT_LU_ZRPVT, "Zero pivot in the ILU(0) factorisation of block %d (local rows %d..%d), row %d", plan.bad_block,
           plan.bad_block * bs, std::min(n, (plan.bad_block + 1) * bs) - 1, plan.bad_row);
  KsIlu *p = nullptr;
  KS_CALL(upload_plan(ctx, n, bs, plan, (const void *)k_bjacobi_ilu_apply, "k_bjacobi_ilu_apply", &p));
  if (transpose) { const int rc = upload_plan(ctx, n, bs, tplan, (const void *)k_bjacobi_ilu_apply_t, "k_bjacobi_ilu_apply_t", &p->t); if (rc) { ks_pc_ilu_free(p); return rc; } }
  *out = p;
  return KS_SUCCESS;
}

int ks_pc_ilu_apply(ks_ctx ctx, const KsIlu *p, const double *in, double *out)
{
  if (p->nblk == 0) return KS_SUCCESS;                       // a rank without rows
  hipLaunchKernelGGL(k_bjacobi_ilu_apply, dim3((unsigned)p->nblk), dim3(ILU_THREADS), sizeof(double) * (size_t)p->bs, ctx->stream,
                     p->n, p->bs, p->blk, p->lev, p->val, p->code, p->rows, p->dinv, in, out);
  KS_HIP(hipGetLastError());
  return KS_SUCCESS;
}

int ks_pc_ilu_apply_transpose(ks_ctx ctx, const KsIlu *p, const double *in, double *out)
{
  KS_CHECK(p->t, KS_ERR_PLIB, "the transposed ILU(0) plan was not built");
  const KsIlu *t = p->t;
  if (t->nblk == 0) return KS_SUCCESS;
  hipLaunchKernelGGL(k_bjacobi_ilu_apply_t, dim3((unsigned)t->nblk), dim3(ILU_THREADS), sizeof(double) * (size_t)t->bs, ctx->stream,
                     t->n, t->bs, t->blk, t->lev, t->val, t->code, t->rows, t->dinv, in, out);
  KS_HIP(hipGetLastError());
  return KS_SUCCESS;
}

// Columns of a pass of the block apply, 0 = one at a time through the single-vector kernel. Measured on the MI355X (profiles/r11_lobpcg_probe.txt: 7-point
// Laplacian, 4.1e6 rows, factors past the Infinity Cache, 20 applies per timed window): at block size 512 the multi-column kernel takes 1.45 / 1.60 / 3.26 /
// 6.51 ms for 2 / 4 / 8 / 16 columns where the column loop takes 2.61 / 5.18 / 10.28 / 20.61 ms (1.8 to 3.2 times faster); at 2048 it is level at 2 columns and
// 3 to 14 % slower from 4 on, at 8192 (two columns per pass, 128 KB of LDS, one workgroup per CU) 6 % slower throughout. So: blocks of up to 512 rows, eight
// columns per pass (32 KB of LDS at most); larger blocks - 2048 and 8192 measured, those between not - stay on the loop, which is what the kernel would replace.
constexpr int ILU_MULTI_BS_MAX = 512;
int ks_pc_ilu_multi_columns(ks_ctx, const KsIlu *p) { return p->bs <= ILU_MULTI_BS_MAX ? 8 : 0; }

// Y(:,j) = U^-1 L^-1 X(:,j), j < ncols: passes of up to ks_pc_ilu_multi_columns columns through k_bjacobi_ilu_apply_multi, a last single column
// through the single-vector kernel (the same bits either way). Enqueued; X and Y do not overlap.
int ks_pc_ilu_apply_multi(ks_ctx ctx, const KsIlu *p, int ncols, const double *X, long long ldx, double *Y, long long ldy)
{
  if (p->nblk == 0) return KS_SUCCESS;
  const int cpp = ks_pc_ilu_multi_columns(ctx, p);
  for (int c0 = 0; c0 < ncols;) {
    const int nc = cpp ? std::min(cpp, ncols - c0) : 1;
    const double *in = X + (size_t)c0 * ldx; double *out = Y + (size_t)c0 * ldy;
    if (nc == 1) KS_CALL(ks_pc_ilu_apply(ctx, p, in, out));
    else {
      const size_t lds = sizeof(double) * (size_t)nc * p->bs;
#define KS_ILU_MULTI(NC) case NC: {                                                                                                                     \
        hipLaunchKernelGGL((k_bjacobi_ilu_apply_multi<NC>), dim3((unsigned)p->nblk), dim3(ILU_THREADS), lds, ctx->stream,                                \
                           p->n, p->bs, p->blk, p->lev, p->val, p->code, p->rows, p->dinv, in, ldx, out, ldy); } break;
      switch (nc) { KS_ILU_MULTI(2) KS_ILU_MULTI(3) KS_ILU_MULTI(4) KS_ILU_MULTI(5) KS_ILU_MULTI(6) KS_ILU_MULTI(7) KS_ILU_MULTI(8) }
#undef KS_ILU_MULTI
      KS_HIP(hipGetLastError());
    }
    c0 += nc;
  }
  return KS_SUCCESS;
}
