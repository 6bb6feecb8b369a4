// Sparse LU with fill (KS_PC_LU): PCLU on the ST's KSP, the reference's default exact inner solve (-st_ksp_type preonly -st_pc_type lu, nested
// dissection, no pivoting). The factors Q P Q^T = L U, their level sets and the stage list are made on the host (ksc::csr_lu_plan, ks_csr.cpp: the
// layout is described in ks_csr.h); this file uploads them and applies them: y = Q^T U^-1 L^-1 Q x, and - on request, from a second plan of the same
// factors - y = Q^T L^-T U^-T Q x (PCApplyTranspose).
//
// The work vector is n doubles in device memory in permuted numbering, too long for one workgroup's LDS, so rows of different workgroups meet only
// at kernel boundaries: nothing in a launch waits for another workgroup - no spin, no flag, no cooperative launch, no grid barrier (a CU's L1 is
// never refreshed by another CU's stores; between stages the only ordering is the stream's). The levels of a triangle are cut into stages:
//   wide    levels of at least `wide` rows, one launch per level on a grid over the level's rows (k_lu_level);
//   narrow  a maximal run of levels with fewer rows, ONE launch of ONE workgroup that walks the levels with a barrier between them
//           (k_lu_narrow): its waves share a CU and its L1, where __syncthreads() orders their stores and loads.
// A row is summed by a group of lanes (1, 8 or 64 by the level's mean row length in a wide level, a whole wave in a narrow stage): lane l takes the
// entries l, l + lanes, ... ascending by fma, the partial sums are combined in one fixed order by DPP moves. No atomics: the same bits on every run.
// The gather by Q is the read of the first triangle's rows (in[perm[r]]), the scatter by Q^T the write of the second triangle's rows (out[perm[r]]).
#include "ksgpu_internal.h"
#include "ks_csr.h"
#include "ks_sweeps.cuh"
#include <algorithm>
#include <cstdlib>

struct KsLu {
  int n = 0, wide = 0, first_scaled = 0, longest_row = 0, neg = 0, pos = 0;
  long long nnzL = 0, nnzU = 0;
  int levels[2] = {0, 0}, nstage[2] = {0, 0};
  size_t bytes = 0;
  int *rows = nullptr, *rp = nullptr, *col = nullptr, *lev = nullptr, *perm = nullptr;
  double *val = nullptr, *dinv = nullptr, *work = nullptr;       // work: LU_MULTI_COLUMNS vectors of n
  std::vector<ksc::LuStage> stages;
  std::vector<int> h_lev, h_lanes, h_perm;
  KsLu *t = nullptr;             // the plan of the transposed triangles: same factors, owned
};

namespace {
constexpr int LU_LEVEL_THREADS = 256;
// A narrow stage is latency: every level is a barrier and a dependent round trip to memory. Eight waves: a level of up to eight rows is one pass,
// two waves per SIMD hide each other's gathers; more waves lengthen the barrier that every one-row level of a separator's clique pays.
constexpr int LU_NARROW_THREADS = 512;
constexpr int LU_NARROW_WAVES = LU_NARROW_THREADS / 64;
constexpr int LU_MULTI_COLUMNS = 8;

struct LuDev { const int *rows, *rp, *col, *lev, *perm; const double *val, *dinv; int n, first_scaled; };

using ksk::group_sum;      // the sum over the 1, 8 or 64 lanes of a row (ks_sweeps.cuh)

// what a finished row does with its sum: the first triangle reads its right-hand side through the permutation, the second one writes the result through it
__device__ __forceinline__ void lu_finish_row(const LuDev &d, int pos, int r, double acc, const double *__restrict__ in, double *__restrict__ w, double *__restrict__ out)
{
  const bool second = pos >= d.n;
  const bool scaled = d.first_scaled ? !second : second;
  double t = (second ? w[r] : in[d.perm[r]]) - acc;
  if (scaled) t = t * d.dinv[pos - (second ? d.n : 0)];
  w[r] = t;
  if (second) out[d.perm[r]] = t;
}

// one wide level: rows p0 .. p0 + nrows - 1 of the level order, LANES lanes per row; blockIdx.y: the column of a block of right-hand sides
template <int LANES>
__global__ void __launch_bounds__(LU_LEVEL_THREADS) k_lu_level(LuDev d, int p0, int nrows, const double *__restrict__ in, long long ldin, double *__restrict__ w,
                                                               double *__restrict__ out, long long ldout)
{
  in += blockIdx.y * ldin; out += blockIdx.y * ldout; w += (size_t)blockIdx.y * d.n;
  const long long g = ((long long)blockIdx.x * LU_LEVEL_THREADS + threadIdx.x) / LANES;
  const int l = threadIdx.x % LANES;
  const bool live = g < nrows;                         // a group past the level takes part in the DPP sums with zeros
  const int pos = live ? p0 + (int)g : p0;
  const int e0 = live ? d.rp[pos] : 0, e1 = live ? d.rp[pos + 1] : 0;
  double acc = 0.0;
  for (int p = e0 + l; p < e1; p += LANES) acc = fma(d.val[p], w[d.col[p]], acc);
  acc = group_sum<LANES>(acc);
  if (live && l == 0) lu_finish_row(d, pos, d.rows[pos], acc, in, w, out);
}

// one narrow stage: levels lev0 .. lev0 + nlev - 1, a wave per row, the rows of a level dealt round-robin to the waves, NC right-hand sides per pass
// (every value and column is read once for all of them, one barrier per level; each column runs the fma chain and the sum of the single-column
// kernel). A level is a chain of dependent round trips to memory - the row's record, its entries, the gather of w, the store that the barrier waits
// for - and a stage is hundreds of levels, so what does not depend on w is taken off that chain: while a level is worked on, every wave already
// loads the record and the first 64 entries of its first row of the NEXT level (the level pointers are read two levels ahead for that). Behind
// the barrier a row of up to 64 entries - and most rows of a wave's level - then only gathers, sums and stores.
struct LuRowHead { int r, e0, e1, c; double v; };
__device__ __forceinline__ LuRowHead lu_row_head(const LuDev &d, int pos, int end, int lane)
{
  LuRowHead h{0, 0, 0, 0, 0.0};
  if (pos < end) {
    h.r = d.rows[pos]; h.e0 = d.rp[pos]; h.e1 = d.rp[pos + 1];
    if (h.e0 + lane < h.e1) { h.v = d.val[h.e0 + lane]; h.c = d.col[h.e0 + lane]; }
  }
  return h;
}
template <int NC>
__global__ void __launch_bounds__(LU_NARROW_THREADS) k_lu_narrow(LuDev d, int lev0, int nlev, const double *__restrict__ in, long long ldin, double *__restrict__ w,
                                                                 double *__restrict__ out, long long ldout)
{
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int p0 = d.lev[lev0], p1 = d.lev[lev0 + 1], p2 = nlev > 1 ? d.lev[lev0 + 2] : p1;
  LuRowHead cur = lu_row_head(d, p0 + wave, p1, lane);
  for (int L = 0; L < nlev; L++) {
    const int p3 = (L + 2 < nlev) ? d.lev[lev0 + L + 3] : p2;
    const LuRowHead ahead = (L + 1 < nlev) ? lu_row_head(d, p1 + wave, p2, lane) : LuRowHead{0, 0, 0, 0, 0.0};
    for (int pos = p0 + wave; pos < p1; pos += LU_NARROW_WAVES) {
      const LuRowHead h = (pos == p0 + wave) ? cur : lu_row_head(d, pos, p1, lane);
      double acc[NC];
#pragma unroll
      for (int j = 0; j < NC; j++) acc[j] = 0.0;
      if (h.e0 + lane < h.e1) {
#pragma unroll
        for (int j = 0; j < NC; j++) acc[j] = fma(h.v, w[(size_t)j * d.n + h.c], acc[j]);
      }
      for (int p = h.e0 + 64 + lane; p < h.e1; p += 64) {
        const double v = d.val[p]; const int c = d.col[p];
#pragma unroll
        for (int j = 0; j < NC; j++) acc[j] = fma(v, w[(size_t)j * d.n + c], acc[j]);
      }
#pragma unroll
      for (int j = 0; j < NC; j++) {
        const double s = ksk::wave_sum(acc[j]);
        if (lane == 0) lu_finish_row(d, pos, h.r, s, in + j * ldin, w + (size_t)j * d.n, out + j * ldout);
      }
    }
    cur = ahead; p0 = p1; p1 = p2; p2 = p3;
    __syncthreads();
  }
}

template <class T> int upload(ks_ctx ctx, T **dst, const std::vector<T> &src, size_t *bytes)
{
  const size_t b = sizeof(T) * std::max<size_t>(src.size(), 1);
  if (hipMalloc((void **)dst, b) != hipSuccess) { (void)hipGetLastError(); *dst = nullptr; KS_FAIL(KS_ERR_MEM, "LU set-up: no device memory for %zu bytes of the factors", b); }
  *bytes += b;
  if (!src.empty()) KS_HIP(hipMemcpyAsync(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice, ctx->stream));
  return KS_SUCCESS;
}

int upload_plan(ks_ctx ctx, ksc::LuPlan &plan, KsLu **out)
{
  KsLu *p = new KsLu();
  p->n = plan.n; p->wide = plan.wide; p->first_scaled = plan.first_scaled; p->longest_row = plan.longest_row; p->neg = plan.neg; p->pos = plan.pos;
  p->nnzL = plan.nnzL; p->nnzU = plan.nnzU;
  for (int t = 0; t < 2; t++) { p->levels[t] = plan.levels[t]; p->nstage[t] = plan.nstage[t]; }
  int rc = upload(ctx, &p->rows, plan.rows, &p->bytes);
  if (!rc) rc = upload(ctx, &p->rp, plan.rp, &p->bytes);
  if (!rc) rc = upload(ctx, &p->col, plan.col, &p->bytes);
  if (!rc) rc = upload(ctx, &p->val, plan.val, &p->bytes);
  if (!rc) rc = upload(ctx, &p->lev, plan.lev, &p->bytes);
  if (!rc) rc = upload(ctx, &p->perm, plan.perm, &p->bytes);
  if (!rc) rc = upload(ctx, &p->dinv, plan.dinv, &p->bytes);
  if (!rc) {
    const size_t b = sizeof(double) * (size_t)LU_MULTI_COLUMNS * std::max(plan.n, 1);
    if (hipMalloc((void **)&p->work, b) != hipSuccess) { (void)hipGetLastError(); p->work = nullptr; ks_set_error("LU set-up: no device memory for the work vectors (%zu bytes)", b); rc = KS_ERR_MEM; }
    else p->bytes += b;
  }
  if (!rc) { hipError_t e = ks_sync(ctx); if (e != hipSuccess) { ks_set_error("LU set-up: %s", hipGetErrorString(e)); rc = KS_ERR_LIB; } }      // the plan's vectors go out of scope
  if (rc) { ks_pc_lu_free(p); return rc; }
  p->stages.swap(plan.stages); p->h_lev.swap(plan.lev); p->h_lanes.swap(plan.lanes); p->h_perm.swap(plan.perm);
  *out = p;
  return KS_SUCCESS;
}

// the stages of both triangles in order, ncols (<= LU_MULTI_COLUMNS) right-hand sides at once
int run_plan(ks_ctx ctx, const KsLu *p, int ncols, const double *in, long long ldin, double *out, long long ldout)
{
  if (p->n == 0) return KS_SUCCESS;
  const LuDev d{p->rows, p->rp, p->col, p->lev, p->perm, p->val, p->dinv, p->n, p->first_scaled};
  for (const ksc::LuStage &s : p->stages) {
    if (!s.wide) {
#define KS_LU_NARROW(NC) case NC: hipLaunchKernelGGL((k_lu_narrow<NC>), dim3(1), dim3(LU_NARROW_THREADS), 0, ctx->stream, d, s.lev0, s.nlev, in, ldin, p->work, out, ldout); break;
      switch (ncols) { KS_LU_NARROW(1) KS_LU_NARROW(2) KS_LU_NARROW(3) KS_LU_NARROW(4) KS_LU_NARROW(5) KS_LU_NARROW(6) KS_LU_NARROW(7) KS_LU_NARROW(8) }
#undef KS_LU_NARROW
    } else for (int l = s.lev0; l < s.lev0 + s.nlev; l++) {
      const int p0 = p->h_lev[l], nrows = p->h_lev[l + 1] - p0, lanes = p->h_lanes[l];
      const dim3 grid((unsigned)(((long long)nrows * lanes + LU_LEVEL_THREADS - 1) / LU_LEVEL_THREADS), (unsigned)ncols);
      if (lanes == 1) hipLaunchKernelGGL((k_lu_level<1>), grid, dim3(LU_LEVEL_THREADS), 0, ctx->stream, d, p0, nrows, in, ldin, p->work, out, ldout);
      else if (lanes == 8) hipLaunchKernelGGL((k_lu_level<8>), grid, dim3(LU_LEVEL_THREADS), 0, ctx->stream, d, p0, nrows, in, ldin, p->work, out, ldout);
      else hipLaunchKernelGGL((k_lu_level<64>), grid, dim3(LU_LEVEL_THREADS), 0, ctx->stream, d, p0, nrows, in, ldin, p->work, out, ldout);
    }
  }
  KS_HIP(hipGetLastError());
  return KS_SUCCESS;
}
} // namespace

void ks_pc_lu_free(KsLu *p)
{
  if (!p) return;
  ks_pc_lu_free(p->t);
  hipFree(p->rows); hipFree(p->rp); hipFree(p->col); hipFree(p->lev); hipFree(p->perm); hipFree(p->val); hipFree(p->dinv); hipFree(p->work);
  delete p;
}

int ks_pc_lu_wide_threshold()
{
  const char *e = getenv("KSGPU_LU_WIDE");        // the probe's knob (scripts/lu_probe.py); unset: the constant
  const int w = e ? atoi(e) : 0;
  return w > 0 ? w : KS_LU_WIDE;
}

int ks_pc_lu_build(ks_ctx ctx, int n, const int *rp, const int *col, const double *val, int ordering, bool transpose, KsLu **out)
{
  ksc::LuPlan plan, tplan;
  try { ksc::csr_lu_plan(n, rp, col, val, ordering, ks_pc_lu_wide_threshold(), false, plan, transpose ? &tplan : nullptr); }
  catch (const std::exception &e) { KS_FAIL(KS_ERR_MEM, "LU set-up: %s", e.what()); }
  KS_CHECK(plan.status != ksc::LU_ZERO_PIVOT, KS_ERR_MAT_LU_ZRPVT, "Zero pivot in the LU factorisation, row %d", plan.bad_row);
  KS_CHECK(plan.status != ksc::LU_TOO_LARGE, KS_ERR_MEM, "the LU factors have more than 2^31 - 1 entries (reached at row %d)", plan.bad_row);
  KsLu *p = nullptr;
  KS_CALL(upload_plan(ctx, plan, &p));
  if (transpose) { const int rc = upload_plan(ctx, tplan, &p->t); if (rc) { ks_pc_lu_free(p); return rc; } }
  *out = p;
  return KS_SUCCESS;
}

int ks_pc_lu_apply(ks_ctx ctx, const KsLu *p, const double *in, double *out) { return run_plan(ctx, p, 1, in, 0, out, 0); }
int ks_pc_lu_apply_transpose(ks_ctx ctx, const KsLu *p, const double *in, double *out)
{
  KS_CHECK(p->t, KS_ERR_PLIB, "the transposed LU plan was not built");
  return run_plan(ctx, p->t, 1, in, 0, out, 0);
}
int ks_pc_lu_multi_columns() { return LU_MULTI_COLUMNS; }
// Y(:,j) = Q^T U^-1 L^-1 Q X(:,j): passes of up to eight columns - a narrow stage keeps them in one launch, a wide level puts them on the grid
int ks_pc_lu_apply_multi(ks_ctx ctx, const KsLu *p, int ncols, const double *X, long long ldx, double *Y, long long ldy)
{
  for (int c0 = 0; c0 < ncols; c0 += LU_MULTI_COLUMNS)
    KS_CALL(run_plan(ctx, p, std::min(LU_MULTI_COLUMNS, ncols - c0), X + (size_t)c0 * ldx, ldx, Y + (size_t)c0 * ldy, ldy));
  return KS_SUCCESS;
}

void ks_pc_lu_info(const KsLu *p, KsLuInfo *o)
{
  o->n = p->n; o->nnzL = p->nnzL; o->nnzU = p->nnzU; o->levelsL = p->levels[0]; o->levelsU = p->levels[1]; o->wide = p->wide; o->neg = p->neg; o->pos = p->pos;
  o->wide_launches = o->narrow_launches = 0;
  for (const ksc::LuStage &s : p->stages) { if (s.wide) o->wide_launches += s.nlev; else o->narrow_launches++; }
  o->bytes = (long long)p->bytes + (p->t ? (long long)p->t->bytes : 0);
  o->perm = p->h_perm.data();
}
