// Jacobi-Davidson for symmetric (definite) problems: the outer loop of Generalized Davidson (Gd::solve, ks_gd.hip) with the expansion vector of each pair
// taken from an approximately solved correction equation in place of a preconditioned residual. For users who want eigenvalues near a target and cannot
// afford the accurate inner solves of shift-and-invert: the inner solve here runs to 1e-4 in at most 90 iterations and the method survives it.
//
// Restates, in this project's structure,
//   EPSSetUp_JD / EPSSetDefaultST_JD, the settings         src/eps/impls/davidson/jd/jd.c
//   dvd_improvex_jd_gen (the loop over the block, the fallbacks)   dvdimprovex.c:590-700
//   dvd_improvex_jd_lit_const_0 (the shift pair and the tolerance)  dvdimprovex.c
//   dvd_improvex_jd_proj_uv_KZX / dvd_improvex_apply_proj         dvdimprovex.c:826-929, :220-280
// Scope: GD's (ks_gd.hip): KS_EPS_HEP and KS_EPS_GHEP, B-orthonormal search basis, Ritz extraction, block sizes 1..16, GD's set-up rules and ST choice.
//
// The correction equation of the pair (theta_j, u_j), r_j = A u_j - theta_j B u_j, with Q = [X_locked, U] (k = nconv + nb columns), Zq = B Q (Q itself
// without B), Y = K^-1 Zq, M = Zq^T Y and P = I - Y M^-1 Zq^T:
//     P K^-1 (theta1 A - theta0 B) t = -P K^-1 r_j,      t from a zero start, so every Krylov vector v has Zq^T v = 0 and t is B-orthogonal to Q.
// K is the ST's preconditioner (built on A - sigma B, ks_gd.hip), the solver is the ST's BiCGStab or GMRES on this operator (ks_ksp_*, ks_st.hip). Every
// application of P is ONE call of ks_bv_oblique_project below - the coefficients h = Zq^T w and c = M^-1 h never leave the device.
//
// Where this file departs from the reference:
//   - the projector. The reference projects with the pair of bases (K^-1 Z, X) of its KZX variant (dvdimprovex.c:826-929: u = K^-1 Z, v = X, with
//     Z = the left vectors of the residual); ours is the textbook projector of a B-orthonormal basis, (Y, Zq) = (K^-1 B Q, B Q). Both make the operator
//     map the B-orthogonal complement of Q into itself; the converged eigenvalues do not depend on the choice, the iteration counts do
//   - the inner solver defaults to BiCGStab where EPSSetDefaultST_JD picks KSPBCGSL (BiCGStab(l), l = 2): the ST has GMRES and BiCGStab. rtol 1e-4 and
//     max_it 90 are the reference's. A KSP type, tolerance or iteration limit the caller set on the ST wins; JD resolves all three into its own state and
//     writes nothing into the ST
//   - reaching max_it, or a BiCGStab breakdown, ends the inner solve with the iterate it has (KSPSolve without KSPSetErrorIfNotConverged, as the reference)
//   - the constraints (deflation space) are not part of Q: the expansion vector is orthogonalised against them with the rest of the basis afterwards
//   - the shift pair for a non-target criterion before `fix` applies is (0, 1) for smallest-* and (1, 0) for largest-*, the target pair of
//     dvd_improvex_jd_lit_const_0 with the reference's target (0 resp. infinity)
//   - the fallbacks to the GD correction (dvdimprovex.c:650-655, :683-690), each counted in gd_fallbacks: no B with the pair (1, 0); M numerically
//     singular (ks_dense.cpp: lu_inverse); an inner iterate that is zero or not finite. The GD correction K^-1 r_j is projected once with P where M^-1 exists
//   - blocks are solved one column after another; Krylov start, harmonic extractions and the double expansion are KS_ERR_SUP or absent, as in GD
//   - the oblique projection takes a fourth launch (the fixed-order sum of the workgroups' partial sums of e^T w) when the caller asks for that dot
#include "ksgpu_internal.h"
#include "ks_eps_impl.h"
#include "ks_davidson.h"
#include "ks_dense.h"
#include "ks_sweeps.cuh"
#include <algorithm>

using namespace ksk;

// ---- the oblique projection ---------------------------------------------------------------------------------------------------------------------------
namespace {

bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

// t = s .* (a u + b v) in k_lincomb's rounding (ks_st.hip): a * u, then + b * v as the compiler contracts it there, then the scaling
__device__ __forceinline__ double ob_form(double a, double u, double b, const double *v, long long i, const double *s)
{
  double t = a * u;
  if (v) t += b * v[i];
  return s ? s[i] * t : t;
}

// Launch 1. w = s .* (a u + b v) formed and stored, and the partial sums of Z(:,0:k)^T w of this workgroup, in one pass: the tile walk, the loads of all
// KT columns in flight and the block combine are k_dot_sweep's (ks_sweeps.cuh). u may be w (a thread reads its rows before it writes them).
template <int KT, int VEC, bool PLAIN>
__device__ __forceinline__ void oblique_dot_tiles(const double *__restrict__ Z, long long ldz, int n, int k, double a, const double *u, double b, const double *v,
                                                  const double *s, double *w, double (&acc)[KT])
{
  const long long tile = (long long)SW_BLOCK * VEC;
  const long long ntiles = ((long long)n + tile - 1) / tile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long r = t * tile + (long long)threadIdx.x * VEC;
    if (VEC == 2 && r + 1 < n) {
      double2 zv[KT];
#pragma unroll
      for (int i = 0; i < KT; i++) { const int ii = i < k ? i : k - 1; zv[i] = ldbasis2<PLAIN>(Z + (long long)ii * ldz + r); }
      const double2 uv = *reinterpret_cast<const double2 *>(u + r);
      double2 wv; wv.x = a * uv.x; wv.y = a * uv.y;
      if (v) { const double2 vv = *reinterpret_cast<const double2 *>(v + r); wv.x += b * vv.x; wv.y += b * vv.y; }
      if (s) { const double2 sv = *reinterpret_cast<const double2 *>(s + r); wv.x = sv.x * wv.x; wv.y = sv.y * wv.y; }
      *reinterpret_cast<double2 *>(w + r) = wv;
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < KT; i++) { acc[i] = fma(zv[i].x, wv.x, acc[i]); acc[i] = fma(zv[i].y, wv.y, acc[i]); }
    } else {
      for (int e = 0; e < VEC; e++) {
        const long long rr = r + e;
        if (rr < n) {
          const double wv = ob_form(a, u[rr], b, v, rr, s);
          w[rr] = wv;
#pragma unroll
          for (int i = 0; i < KT; i++) { const int ii = i < k ? i : k - 1; acc[i] = fma(Z[(long long)ii * ldz + rr], wv, acc[i]); }
        }
      }
    }
  }
}

template <int KT, int VEC>
__global__ __launch_bounds__(SW_BLOCK) void k_oblique_dot(const double *__restrict__ Z, long long ldz, int n, int k, double a, const double *u, double b, const double *v,
                                                          const double *s, double *w, double *__restrict__ partials, int plain)
{
  double acc[KT];
#pragma unroll
  for (int i = 0; i < KT; i++) acc[i] = 0.0;
  if (VEC == 2 && plain) oblique_dot_tiles<KT, VEC, true>(Z, ldz, n, k, a, u, b, v, s, w, acc);
  else oblique_dot_tiles<KT, VEC, false>(Z, ldz, n, k, a, u, b, v, s, w, acc);
  block_write_partials<KT>(acc, k, partials);
}

// Launch 2, one workgroup. h(c0 : c0 + nc) = the fixed-order sums of the workgroups' partials (k_reduce_only's), kept in `h`; on the last chunk of columns
// c = Minv h(0:ktot), row i with the columns ascending and one fma each from 0. Minv (Minv h_1 + Minv h_2 = Minv (h_1 + h_2)) is applied BEFORE the sum
// over the ranks, so that sum - ks_allreduce_sum on c - is the only thing between this kernel and the update sweep.
__global__ __launch_bounds__(1024) void k_oblique_reduce(const double *__restrict__ partials, int nblocks, int nc, int c0, int ktot, const double *__restrict__ Minv, int ldm,
                                                         double *h, double *__restrict__ c, int last)
{
  __shared__ double hl[KS_MAX_COLS + 8];
  reduce_partials_to_lds(partials, nblocks, nc, hl);
  if ((int)threadIdx.x < nc) h[c0 + threadIdx.x] = hl[threadIdx.x];
  if (!last) return;
  for (int i = threadIdx.x; i < ktot; i += blockDim.x) {
    double acc = 0.0;
    for (int j = 0; j < ktot; j++) {
      const double hj = (j >= c0 && j < c0 + nc) ? hl[j - c0] : h[j];      // the chunks before this one were written by earlier launches
      acc = fma(Minv[(size_t)i + (size_t)j * ldm], hj, acc);
    }
    c[i] = acc;
  }
}

// Launch 3. w <- w - Y(:,0:k) c with c on the device: per row the columns ascending, one fma each, starting from w (k_multvec's walk with eight
// columns in flight). DOT: the partial sum of e .* w_new of this workgroup into partials (row 0); e may be w itself.
template <int VEC, bool DOT>
__global__ __launch_bounds__(SW_BLOCK) void k_oblique_update(const double *__restrict__ Y, long long ldy, int n, int k, const double *__restrict__ c, double *w, const double *e,
                                                             double *__restrict__ partials)
{
  double acc[1] = {0.0};
  const long long tile = (long long)SW_BLOCK * VEC;
  const long long ntiles = ((long long)n + tile - 1) / tile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long r = t * tile + (long long)threadIdx.x * VEC;
    if (VEC == 2 && r + 1 < n) {
      double2 sv = *reinterpret_cast<const double2 *>(w + r);
      int i = 0;
      for (; i + 8 <= k; i += 8) {
        double2 yv[8];
#pragma unroll
        for (int q = 0; q < 8; q++) yv[q] = *reinterpret_cast<const double2 *>(Y + (long long)(i + q) * ldy + r);
#pragma unroll
        for (int q = 0; q < 8; q++) { const double cq = -c[i + q]; sv.x = fma(yv[q].x, cq, sv.x); sv.y = fma(yv[q].y, cq, sv.y); }
      }
      for (; i < k; i++) { const double2 yv = *reinterpret_cast<const double2 *>(Y + (long long)i * ldy + r); const double cq = -c[i]; sv.x = fma(yv.x, cq, sv.x); sv.y = fma(yv.y, cq, sv.y); }
      if (k > 0) *reinterpret_cast<double2 *>(w + r) = sv;
      if (DOT) {
        double2 ev = sv;
        if (e != w) ev = *reinterpret_cast<const double2 *>(e + r);
        acc[0] = fma(ev.x, sv.x, acc[0]); acc[0] = fma(ev.y, sv.y, acc[0]);
      }
    } else {
      for (int q = 0; q < VEC; q++) {
        const long long rr = r + q;
        if (rr < n) {
          double sv = w[rr];
          for (int i = 0; i < k; i++) sv = fma(Y[(long long)i * ldy + rr], -c[i], sv);
          if (k > 0) w[rr] = sv;
          if (DOT) acc[0] = fma(e != w ? e[rr] : sv, sv, acc[0]);
        }
      }
    }
  }
  if (DOT) block_write_partials<1>(acc, 1, partials);
}

// compiled column counts of the dot sweep: every count up to 8 (a padded column is a full extra read of a streamed basis), then steps that keep the
// padding under a quarter
int oblique_kt_for(int k)
{
  static const int kts[] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 20, 24, 32, 40, 48, 56, 64};
  for (int kt : kts) if (k <= kt) return kt;
  return 64;
}

int launch_oblique_dot(ks_bv Z, const double *Zd, int k, double a, const double *u, double b, const double *v, const double *s, double *w, bool v2)
{
  ks_ctx ctx = Z->ctx;
  const int n = Z->n;
  const int per_cu = std::max(1, std::min(4, (30 + k - 1) / k));                 // ksk_dot's rule: about 120 KiB of loads in flight per CU
  const int plain = ks_basis_loads_plain(ctx, (size_t)(2 * (Z->nc + Z->m)), (size_t)Z->ld);
  const long long ldz = Z->ld;
  Z->spec.valid = false;
  int grid = 1;
  KsProfScope ps(ctx, KS_K_DOT, 8.0 * n * (k + 2 + (v ? 1 : 0) + (s ? 1 : 0)));
#define KSJ_DOT(KT)                                                                                                                                            \
  do {                                                                                                                                                         \
    if (v2) { grid = ks_sweep_grid_for(ctx, n, 2, (const void *)k_oblique_dot<KT, 2>, per_cu);                                                                 \
      hipLaunchKernelGGL((k_oblique_dot<KT, 2>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, Zd, ldz, n, k, a, u, b, v, s, w, Z->partials, plain); }         \
    else { grid = ks_sweep_grid_for(ctx, n, 1, (const void *)k_oblique_dot<KT, 1>, per_cu);                                                                    \
      hipLaunchKernelGGL((k_oblique_dot<KT, 1>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, Zd, ldz, n, k, a, u, b, v, s, w, Z->partials, plain); }         \
  } while (0)
  switch (oblique_kt_for(k)) {
    case 1: KSJ_DOT(1); break; case 2: KSJ_DOT(2); break; case 3: KSJ_DOT(3); break; case 4: KSJ_DOT(4); break; case 5: KSJ_DOT(5); break; case 6: KSJ_DOT(6); break;
    case 7: KSJ_DOT(7); break; case 8: KSJ_DOT(8); break; case 10: KSJ_DOT(10); break; case 12: KSJ_DOT(12); break; case 16: KSJ_DOT(16); break; case 20: KSJ_DOT(20); break;
    case 24: KSJ_DOT(24); break; case 32: KSJ_DOT(32); break; case 40: KSJ_DOT(40); break; case 48: KSJ_DOT(48); break; case 56: KSJ_DOT(56); break; default: KSJ_DOT(64); break;
  }
#undef KSJ_DOT
  Z->last_grid = grid;
  KS_HIP(hipGetLastError());
  return KS_SUCCESS;
}

int launch_oblique_update(ks_bv Y, const double *Yd, int k, const double *c, double *w, const double *e, bool dot, bool v2)
{
  ks_ctx ctx = Y->ctx;
  const int n = Y->n;
  const int grid = ks_sweep_grid(ctx, n, v2 ? 2 : 1);
  const long long ldy = Y->ld;
  Y->spec.valid = false;
  KsProfScope ps(ctx, KS_K_UPD, 8.0 * n * (k + 2 + ((dot && e != w) ? 1 : 0)));
  if (v2) { if (dot) hipLaunchKernelGGL((k_oblique_update<2, true>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, Yd, ldy, n, k, c, w, e, Y->partials);
            else hipLaunchKernelGGL((k_oblique_update<2, false>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, Yd, ldy, n, k, c, w, e, Y->partials); }
  else { if (dot) hipLaunchKernelGGL((k_oblique_update<1, true>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, Yd, ldy, n, k, c, w, e, Y->partials);
         else hipLaunchKernelGGL((k_oblique_update<1, false>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, Yd, ldy, n, k, c, w, e, Y->partials); }
  if (dot) Y->last_grid = grid;
  KS_HIP(hipGetLastError());
  return KS_SUCCESS;
}

bool inside(const double *p, ks_bv bv) { return p >= bv->array && p < bv->array + (size_t)(bv->nc + bv->m) * bv->ld; }

} // namespace

// w <- (I - Y Minv Z^T) (s .* (a u + b v)) over the k active columns of Z and of Y, and *dot = e^T w of the result over all ranks (include/ksgpu.h).
// Three launches with no host wait between them - the dot sweep that forms w, the one-workgroup reduce that multiplies by Minv, the update sweep - and
// the sum over the ranks of c on the device between the last two; a fourth, the fixed-order sum of the update's partial sums, when dot is asked for.
// More than KS_MAX_COLS columns go in chunks: further dot sweeps (ksk_dot) on the stored w, the update chunk after chunk in ascending order.
extern "C" int ks_bv_oblique_project(ks_bv Y, ks_bv Z, const double *Minv_dev, int ldm, double a, const double *u_dev, double b, const double *v_dev,
                                     const double *s_dev, double *w_dev, const double *e_dev, double *dot)
{
  KS_CHECK(Y && Z, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(w_dev && u_dev, KS_ERR_ARG_NULL, "w or u is NULL");
  KS_CALL(ksb_flush(Y)); KS_CALL(ksb_flush(Z));
  const int k = Z->k - Z->l;
  KS_CHECK(Y->n == Z->n, KS_ERR_ARG_INCOMP, "Mismatching local dimensions Y %d, Z %d", Y->n, Z->n);
  KS_CHECK(k >= 0 && Y->k - Y->l == k, KS_ERR_ARG_INCOMP, "Y has %d active columns, Z has %d", Y->k - Y->l, k);
  KS_CHECK(k == 0 || Minv_dev, KS_ERR_ARG_NULL, "Minv is NULL");
  KS_CHECK(k == 0 || ldm >= k, KS_ERR_ARG_SIZ, "Minv has %d rows, should have at least %d", ldm, k);
  KS_CHECK(!dot || e_dev, KS_ERR_ARG_NULL, "a dot is asked for and e is NULL");
  KS_CHECK(!inside(w_dev, Y) && !inside(w_dev, Z), KS_ERR_ARG_WRONG, "w must not be a column of Y or Z");
  ks_ctx ctx = Z->ctx;
  KS_HIP(hipSetDevice(ctx->device));
  const int n = Z->n;
  const double *Zd = ks_bv_col(Z, Z->l), *Yd = ks_bv_col(Y, Y->l);
  const bool want_dot = dot != nullptr;
  double *h = Z->cw, *c = Y->cw;                               // k <= m doubles each: the scratch of the wide Gram-Schmidt, idle here
  if (n > 0) {
    const bool v2 = Z->ld % 2 == 0 && Y->ld % 2 == 0 && aligned16(Zd) && aligned16(Yd) && aligned16(u_dev) && aligned16(w_dev) && (!v_dev || aligned16(v_dev))
                    && (!s_dev || aligned16(s_dev)) && (!want_dot || aligned16(e_dev));
    if (k == 0) {
      if (!(u_dev == w_dev && a == 1.0 && !v_dev && !s_dev)) KS_CALL(ksk_lincomb(ctx, n, s_dev, a, u_dev, b, v_dev, w_dev));
      if (want_dot) KS_CALL(launch_oblique_update(Y, Yd, 0, c, w_dev, e_dev, true, v2));
    } else {
      for (int c0 = 0; c0 < k; c0 += KS_MAX_COLS) {
        const int nc = std::min(KS_MAX_COLS, k - c0);
        if (c0 == 0) KS_CALL(launch_oblique_dot(Z, Zd, nc, a, u_dev, b, v_dev, s_dev, w_dev, v2));
        else KS_CALL(ksk_dot(Z, Zd + (size_t)c0 * Z->ld, Z->ld, nc, w_dev, false));
        hipLaunchKernelGGL(k_oblique_reduce, dim3(1), dim3(1024), 0, ctx->stream, Z->partials, Z->last_grid, nc, c0, k, Minv_dev, ldm, h, c, c0 + nc >= k ? 1 : 0);
        KS_HIP(hipGetLastError());
      }
      KS_CALL(ks_allreduce_sum(ctx, c, k));
      for (int c0 = 0; c0 < k; c0 += KS_MAX_COLS) {
        const int nc = std::min(KS_MAX_COLS, k - c0);
        KS_CALL(launch_oblique_update(Y, Yd + (size_t)c0 * Y->ld, nc, c + c0, w_dev, e_dev, want_dot && c0 + nc >= k, v2));
      }
    }
    if (want_dot) KS_CALL(ksk_reduce_partials(Y, 1, Y->coef));
  } else {
    if (k > 0) { KS_HIP(hipMemsetAsync(c, 0, sizeof(double) * k, ctx->stream)); KS_CALL(ks_allreduce_sum(ctx, c, k)); }     // a rank with no rows still takes part in the sum
    if (want_dot) KS_HIP(hipMemsetAsync(Y->coef, 0, sizeof(double), ctx->stream));
  }
  if (want_dot) {
    KS_CALL(ks_allreduce_sum(ctx, Y->coef, 1));
    KS_HIP(hipMemcpyAsync(dot, Y->coef, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    KS_HIP(ks_sync(ctx));
  }
  return KS_SUCCESS;
}

// ---- the driver -----------------------------------------------------------------------------------------------------------------------------------------
namespace {

struct Jd : Gd {
  ks_bv Zq = nullptr, Yb = nullptr, Wk = nullptr, Kg = nullptr, Kb = nullptr;     // B Q and K^-1 B Q (nev + bs columns), 4 work vectors, the inner solver's vectors
  double *Minv_dev = nullptr;
  int ldM = 0, yvalid = 0;                 // locked columns of Yb (and rows / columns of M) that are up to date
  std::vector<double> M, Minv;
  int ksp_type = KS_KSP_BCGS, max_it = 90, restart = 30; double rtol = 1e-4, dyntol = 0.5;
  long long solves = 0; double last_rnorm = 0.0;
  ~Jd() override { ks_bv_destroy(Zq); ks_bv_destroy(Yb); ks_bv_destroy(Wk); ks_bv_destroy(Kg); ks_bv_destroy(Kb); if (Minv_dev) hipFree(Minv_dev); }

  int prepare()
  {
    ldM = nev + bs;
    KS_CALL(make(ldM, &Zq)); KS_CALL(make(ldM, &Yb)); KS_CALL(make(4, &Wk));
    // EPSSetDefaultST_JD (jd.c) where the caller has not chosen: resolved here, the ST keeps its own values
    ksp_type = st->ksp_type_set ? st->ksp_type : KS_KSP_BCGS;
    rtol = st->rtol_set ? st->rtol : 1e-4; max_it = st->max_it_set ? st->max_it : 90; restart = st->restart;
    KS_CHECK(ksp_type != KS_KSP_CG, KS_ERR_SUP, "Jacobi-Davidson cannot solve its correction equation with KSPCG: the projected operator is not symmetric in the form it is applied here (use BiCGStab or GMRES)");
    KS_CHECK(ksp_type != KS_KSP_MINRES, KS_ERR_SUP, "Jacobi-Davidson cannot solve its correction equation with KSPMINRES: the projected operator is not symmetric in the form it is applied here (use BiCGStab or GMRES)");
    KS_CHECK(ksp_type != KS_KSP_BCGSL, KS_ERR_SUP, "Jacobi-Davidson cannot solve its correction equation with KSPBCGSL: the device-resident solvers run on the ST's own operator, not on the projected one (use BiCGStab or GMRES)");
    if (ksp_type == KS_KSP_BCGS) KS_CALL(make(7, &Kb));
    else if (ksp_type == KS_KSP_PREONLY) {}      // the preconditioned, projected right-hand side is the correction: no vectors
    else { KS_CALL(make(restart + 1, &Kg)); KS_CALL(ks_bv_set_orthogonalization(Kg, KS_BV_ORTHOG_CGS, st->gmres_refine, 0.7071)); }
    M.assign((size_t)ldM * ldM, 0.0); Minv.assign((size_t)ldM * ldM, 0.0);
    KS_HIP(hipMalloc(&Minv_dev, sizeof(double) * (size_t)ldM * ldM));
    if (B) BXo = Zq; else Xo = Zq;           // the sweep leaves B u_j (u_j) of the block in Zq(:, nconv + j)
    return KS_SUCCESS;
  }
  void locked(int) override { dyntol = 0.5; }       // dvdimprovex.c:603-605: the dynamic tolerance starts again when a pair is locked
  int correction(int nb, const double *theta, const double *rnorm, int base) override;
};

// P K^-1 (theta1 A - theta0 B) as the KSPs see it. Pointwise K (none, point Jacobi): the products, then one oblique projection with the linear combination
// and the scaling inside; block K: the combination, the blocks, then the projection with a = 1. Nothing here waits for the device unless a dot is asked for.
struct JdOp : KsKspOp {
  Jd *jd; double th0, th1; bool pointwise; const double *dinv;
  int project(double a, const double *u, double b, const double *v, const double *s, double *w, const double *e, double *dot)
  {
    return ks_bv_oblique_project(jd->Yb, jd->Zq, jd->Minv_dev, jd->ldM, a, u, b, v, s, w, e, dot);
  }
  int pc(const double *in, double *out)
  {
    if (!(jd->st->pc_type == KS_PC_NONE || jd->st->pc_identity)) jd->cfg->pc_columns++;
    return ks_st_pc_apply_multi_internal(jd->st, 1, in, jd->V->ld, out, jd->V->ld);
  }
  int apply_e(const double *x, double *out, const double *e, double *dot)
  {
    double *ta = ks_bv_col(jd->Wk, 0), *tb = ks_bv_col(jd->Wk, 1), *tc = ks_bv_col(jd->Wk, 2);
    double a = th1, b = -th0; const double *u = ta, *v = x;
    if (th1 != 0.0) { KS_CALL(ks_mat_mult_internal(jd->A, x, ta)); jd->cfg->mat_columns++; }
    if (jd->B) { KS_CALL(ks_mat_mult_internal(jd->B, x, tb)); jd->cfg->mat_columns++; v = tb; }
    if (th1 == 0.0) { u = v; a = -th0; b = 0.0; v = nullptr; }        // the pair (1, 0): the operator is -B
    else if (th0 == 0.0) { b = 0.0; v = nullptr; }
    if (pointwise) { if (dinv) jd->cfg->pc_columns++; return project(a, u, b, v, dinv, out, e, dot); }
    KS_CALL(ksk_lincomb(jd->ctx, jd->V->n, nullptr, a, u, b, v, tc));
    KS_CALL(pc(tc, out));
    return project(1.0, out, 0.0, nullptr, nullptr, out, e, dot);
  }
  int apply(const double *x, double *out) override { return apply_e(x, out, nullptr, nullptr); }
  int apply_dot(const double *x, double *out, ks_bv, int, const double *e, double *dot) override { return apply_e(x, out, e, dot); }
  int residual(const double *rhs, const double *y, double *out) override      // rhs is the projected, preconditioned right-hand side already
  {
    if (!y) return ksk_copy(jd->ctx, rhs, out, jd->V->n);
    KS_CALL(apply(y, out));
    return ksk_lincomb(jd->ctx, jd->V->n, nullptr, 1.0, rhs, -1.0, out, out);
  }
};

int Jd::correction(int nb, const double *theta, const double *rnorm, int base)
{
  const int k = nconv + nb, n = V->n;
  const bool nopc = st->pc_type == KS_PC_NONE || st->pc_identity;
  // Y = K^-1 Zq for the columns that are new: the locked ones since the last correction and the block (K does not change during a solve)
  KS_CALL(ks_st_pc_apply_multi_internal(st, k - yvalid, ks_bv_col(Zq, yvalid), Zq->ld, ks_bv_col(Yb, yvalid), Yb->ld));
  if (!nopc) cfg->pc_columns += k - yvalid;
  // the new rows and columns of M = Zq^T Y
  KS_CALL(ksb_dot_range(Yb, yvalid, k, Zq, 0, k, M.data(), ldM));
  if (yvalid > 0) KS_CALL(ksb_dot_range(Yb, 0, yvalid, Zq, yvalid, k, M.data(), ldM));
  KS_CALL(ks_eps_synchronize_values(eps, M.data(), (size_t)ldM * k));
  yvalid = nconv;
  const bool singular = ksd::lu_inverse(k, M.data(), ldM, Minv.data(), ldM) != 0;
  if (!singular) KS_HIP(hipMemcpyAsync(Minv_dev, Minv.data(), sizeof(double) * (size_t)ldM * k, hipMemcpyHostToDevice, ctx->stream));   // M^-1 staged once per outer iteration
  KS_CALL(ks_bv_set_active_columns(Zq, 0, k)); KS_CALL(ks_bv_set_active_columns(Yb, 0, k));

  const int which = eps->cmp_final.which;
  const bool largest = which == KS_EPS_LARGEST_MAGNITUDE || which == KS_EPS_LARGEST_REAL || which == KS_EPS_LARGEST_IMAGINARY;
  const bool tgt = which == KS_EPS_TARGET_MAGNITUDE || which == KS_EPS_TARGET_REAL;
  JdOp op; op.jd = this; op.pointwise = ks_st_pc_pointwise(st, &op.dinv);
  const double tol = eps->jdx.const_tol ? rtol : dyntol;
  bool solved_one = false;
  for (int j = 0; j < nb; j++) {
    double *dst = ks_bv_col(V, base + j), *rj = ks_bv_col(R, j), *rhs = ks_bv_col(Wk, 3);
    // the shift pair (dvd_improvex_jd_lit_const_0): the Ritz value once the residual is small against it, the target before
    if (rnorm[j] < eps->jdx.fix * fabs(theta[j])) { op.th0 = theta[j]; op.th1 = 1.0; }
    else if (tgt) { op.th0 = eps->which.target; op.th1 = 1.0; }
    else if (largest) { op.th0 = 1.0; op.th1 = 0.0; }
    else { op.th0 = 0.0; op.th1 = 1.0; }
    bool fallback = singular || (!B && op.th1 == 0.0);            // no B and the pair (1, 0): the reference's "odd situation" (dvdimprovex.c:650-655)
    if (!fallback) {
      // rhs = -P K^-1 r_j
      if (op.pointwise) KS_CALL(op.project(-1.0, rj, 0.0, nullptr, op.dinv, rhs, nullptr, nullptr));
      else { KS_CALL(op.pc(rj, rhs)); KS_CALL(op.project(-1.0, rhs, 0.0, nullptr, nullptr, rhs, nullptr, nullptr)); }
      if (op.pointwise && op.dinv) cfg->pc_columns++;
      KsKsp ksp{ctx, (long long)n, Kg, Kb, tol, max_it, restart, false, &solves, &eps->jdx.inner_iterations, &last_rnorm};
      KS_CALL(ksp_type == KS_KSP_BCGS ? ks_ksp_bcgs(ksp, op, rhs, dst) : ksp_type == KS_KSP_PREONLY ? ks_ksp_preonly(ksp, op, rhs, dst) : ks_ksp_gmres(ksp, op, rhs, dst));
      eps->jdx.inner_solves++; solved_one = true;
      double nrm = 0.0;
      KS_CALL(ks_bv_normvec(Wk, dst, KS_NORM_2, &nrm));
      KS_CALL(ks_eps_synchronize_values(eps, &nrm, 1));
      fallback = !(nrm > 0.0) || !std::isfinite(nrm);               // an inner iterate that is zero or not finite
    }
    if (fallback) {
      // the GD correction K^-1 r_j, projected once (dvdimprovex.c:683-690)
      KS_CALL(op.pc(rj, dst));
      if (!singular) KS_CALL(op.project(1.0, dst, 0.0, nullptr, nullptr, dst, nullptr, nullptr));
      eps->jdx.gd_fallbacks++;
    }
  }
  // the dynamic rule (dvdimprovex.c:603-605, 630, 698): halved after each outer iteration that solved a correction, floor 10 eps
  if (solved_one) dyntol = std::max(0.5 * dyntol, 10.0 * 2.220446049250313e-16);
  return KS_SUCCESS;
}

int jd_setup(ks_eps eps)
{
  KS_CALL(ks_davidson_setup(eps, eps->jd, "JD"));
  eps->jdx.inner_solves = eps->jdx.inner_iterations = eps->jdx.gd_fallbacks = 0;
  return KS_SUCCESS;
}
int jd_solve(ks_eps eps)
{
  Jd s;
  s.eps = eps; s.ctx = eps->ctx; s.B = eps->ghep ? eps->B : nullptr; s.st = eps->st; s.V = eps->V; s.nev = eps->nev; s.bs = eps->jd.r_bs;
  KS_CALL(s.prepare());
  return ks_davidson_solve(eps, eps->jd, s);
}

} // namespace

const ks_eps_ops *ks_jd_ops()
{
  static const ks_eps_ops ops = {jd_setup, jd_solve, nullptr};
  return &ops;
}

// ---- the settings (EPSJDSet* / EPSJDGet*, src/eps/impls/davidson/jd/jd.c) ----------------------------------------------------------------------------
extern "C" int ks_eps_jd_set_blocksize(ks_eps eps, int bs) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); return ks_davidson_set_blocksize(eps, eps->jd, bs); }            // EPSJDSetBlockSize jd.c
extern "C" int ks_eps_jd_get_blocksize(ks_eps eps, int *bs) { KS_CHECK(eps && bs, KS_ERR_ARG_NULL, "NULL argument"); *bs = eps->jd.bs ? eps->jd.bs : 1; return KS_SUCCESS; }
extern "C" int ks_eps_jd_set_restart(ks_eps eps, int minv, int plusk) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); return ks_davidson_set_restart(eps, eps->jd, minv, plusk); }   // EPSJDSetRestart jd.c
extern "C" int ks_eps_jd_get_restart(ks_eps eps, int *minv, int *plusk) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); ks_davidson_get_restart(eps->jd, minv, plusk); return KS_SUCCESS; }
extern "C" int ks_eps_jd_set_initial_size(ks_eps eps, int initialsize) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); return ks_davidson_set_initial_size(eps, eps->jd, initialsize); }   // EPSJDSetInitialSize jd.c
extern "C" int ks_eps_jd_get_initial_size(ks_eps eps, int *initialsize)
{
  KS_CHECK(eps && initialsize, KS_ERR_ARG_NULL, "NULL argument");
  *initialsize = eps->jd.initv ? eps->jd.initv : eps->jd.r_initv; return KS_SUCCESS;
}
extern "C" int ks_eps_jd_set_borth(ks_eps eps, int borth) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); eps->jd.borth = borth != 0; eps->solved = false; return KS_SUCCESS; }   // EPSJDSetBOrth jd.c
extern "C" int ks_eps_jd_get_borth(ks_eps eps, int *borth) { KS_CHECK(eps && borth, KS_ERR_ARG_NULL, "NULL argument"); *borth = eps->jd.borth ? 1 : 0; return KS_SUCCESS; }
extern "C" int ks_eps_jd_set_fix(ks_eps eps, double fix)                // EPSJDSetFix jd.c
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(fix > 0.0, KS_ERR_ARG_OUTOFRANGE, "Invalid fix value %g, must be > 0", fix);
  eps->jdx.fix = fix; eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_jd_get_fix(ks_eps eps, double *fix) { KS_CHECK(eps && fix, KS_ERR_ARG_NULL, "NULL argument"); *fix = eps->jdx.fix; return KS_SUCCESS; }
extern "C" int ks_eps_jd_set_const_correction_tol(ks_eps eps, int constant) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); eps->jdx.const_tol = constant != 0; eps->solved = false; return KS_SUCCESS; }   // EPSJDSetConstCorrectionTol jd.c
extern "C" int ks_eps_jd_get_const_correction_tol(ks_eps eps, int *constant) { KS_CHECK(eps && constant, KS_ERR_ARG_NULL, "NULL argument"); *constant = eps->jdx.const_tol ? 1 : 0; return KS_SUCCESS; }
extern "C" int ks_eps_jd_get_stats(ks_eps eps, long long *iterations, long long *restarts, long long *locks, long long *mat_columns, long long *pc_columns,
                                   long long *inner_solves, long long *inner_iterations, long long *gd_fallbacks)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  if (iterations) *iterations = eps->jd.iterations; if (restarts) *restarts = eps->jd.restarts; if (locks) *locks = eps->jd.locks;
  if (mat_columns) *mat_columns = eps->jd.mat_columns; if (pc_columns) *pc_columns = eps->jd.pc_columns;
  if (inner_solves) *inner_solves = eps->jdx.inner_solves; if (inner_iterations) *inner_iterations = eps->jdx.inner_iterations; if (gd_fallbacks) *gd_fallbacks = eps->jdx.gd_fallbacks;
  return KS_SUCCESS;
}
