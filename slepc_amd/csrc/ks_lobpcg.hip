// LOBPCG for symmetric (definite) problems: the block eigensolver of the library, for the few smallest (or largest) eigenvalues of A x = k B x
// without inner solves - one preconditioner application per residual, everything else a block operation.
//
// Restates, in this project's structure,
//   EPSSetUp_LOBPCG / EPSSetDimensions_LOBPCG   src/eps/impls/cg/lobpcg/lobpcg.c:40-83
//   EPSSolve_LOBPCG                             lobpcg.c:85-396
// (LOBPCG with soft and hard locking after BLOPEX: Knyazev, SIAM J. Sci. Comput. 23(2) 2001; Knyazev et al., SIAM J. Sci. Comput. 29(5) 2007.)
// The arithmetic is the reference's: A Z and A X are recomputed every iteration (BVMatProject(Z,A,Z), BVMatMult(X,A,AX)) through the block product
// ks_mat_mult_multi. Where this file departs from it:
//   - residuals and their norms are one kernel and one D2H for the block (k_block_residual) instead of a copy, bs axpys and bs norms with a host wait each
//     (lobpcg.c:176-202); r = fma(-theta, bx, ax) where the reference rounds theta * bx first
//   - the preconditioner is applied to the block (ks_st_apply_mat: STApplyMat, lobpcg.c:298)
//   - the preconditioned residuals are made orthogonal to the constraints and the hard-locked vectors as a block, W <- W - Y (Y^T B W) twice, two D2H per
//     iteration, instead of one BVOrthogonalizeVec per column; the reference's scaling of each column to unit norm is left to the BVOrthogonalize that
//     follows (the span is the same), and a column that vanishes shows there or in the projected problem (EPS_DIVERGED_BREAKDOWN either way)
//   - BVOrthogonalize of R, P and X (lobpcg.c:255,330,333) is a block operation: a block Gram-Schmidt step against the leading (soft-locked) columns
//     of the same BV, then a Cholesky factorisation of the Gram matrix scaled to unit diagonal - two D2H with soft-locked columns, one without,
//     none per column. The reference's column-by-column Gram-Schmidt is the fallback of a call whose factorisation fails
//   - block sizes up to 16 (48 columns in the projected problem)
#include "ksgpu_internal.h"
#include "ks_eps_impl.h"
#include "ks_sweeps.cuh"
#include "ks_dense.h"
#include <algorithm>

using namespace ksk;

namespace {

struct KsTheta16 { double v[16]; };

// R(:,j) = AX(:,j) - theta_j BX(:,j), j < KT, and the partial sums of ||R(:,j)||^2 of this block: one pass, two blocks read and one written. The tile walk and
// the block combine are the sweeps' (ks_sweeps.cuh: lane <-> row pair, all 2 KT loads of a tile issued back to back, DPP wave sums, one row of `partials` per
// workgroup: partials[j * gridDim.x + blockIdx.x]). BX may be X itself (a standard problem); R overlaps neither input.
template <int KT, int VEC, bool PLAIN>
__global__ __launch_bounds__(SW_BLOCK) void k_block_residual(const double *__restrict__ AX, long long ldax, const double *__restrict__ BX, long long ldbx,
                                                             double *__restrict__ R, long long ldr, int n, KsTheta16 th, double *__restrict__ partials)
{
  double acc[KT];
#pragma unroll
  for (int i = 0; i < KT; i++) acc[i] = 0.0;
  const long long tile = (long long)SW_BLOCK * VEC;
  const long long ntiles = ((long long)n + tile - 1) / tile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long r = t * tile + (long long)threadIdx.x * VEC;
    if (VEC == 2 && r + 1 < n) {
      double2 a[KT], b[KT];
#pragma unroll
      for (int i = 0; i < KT; i++) { a[i] = ldbasis2<PLAIN>(AX + i * ldax + r); b[i] = ldbasis2<PLAIN>(BX + i * ldbx + r); }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < KT; i++) {
        double2 v; v.x = fma(-th.v[i], b[i].x, a[i].x); v.y = fma(-th.v[i], b[i].y, a[i].y);
        *reinterpret_cast<double2 *>(R + i * ldr + r) = v;
        acc[i] = fma(v.x, v.x, acc[i]); acc[i] = fma(v.y, v.y, acc[i]);
      }
    } else {
      for (int u = 0; u < VEC; u++) {
        const long long rr = r + u;
        if (rr < n) {
#pragma unroll
          for (int i = 0; i < KT; i++) { const double v = fma(-th.v[i], BX[i * ldbx + rr], AX[i * ldax + rr]); R[i * ldr + rr] = v; acc[i] = fma(v, v, acc[i]); }
        }
      }
    }
  }
  block_write_partials<KT>(acc, KT, partials);
}

bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

} // namespace

// The block residual with its norms. The partial sums go the way of ks_bv_dotvec: one row per workgroup, the fixed-order reduction of this rank's rows, the
// communicator's allreduce, and all ncols values in one copy to the host - correct on any number of ranks by construction.
int ksl_block_residual(ks_bv R, int ncols, const double *AX, long long ldax, const double *BX, long long ldbx, double *Rd, long long ldr, const double *theta, double *norms)
{
  ks_ctx ctx = R->ctx;
  KS_CHECK(ncols >= 1 && ncols <= 16, KS_ERR_ARG_OUTOFRANGE, "block residual of %d columns (1..16)", ncols);
  KsTheta16 th; for (int i = 0; i < 16; i++) th.v[i] = i < ncols ? theta[i] : 0.0;
  const int n = R->n;
  R->spec.valid = false;                                        // the partials of this BV are rewritten
  if (n > 0) {
    const bool v2 = ldax % 2 == 0 && ldbx % 2 == 0 && ldr % 2 == 0 && aligned16(AX) && aligned16(BX) && aligned16(Rd);
    const bool plain = ks_basis_loads_plain(ctx, (size_t)3 * ncols, (size_t)R->ld);
    KsProfScope ps(ctx, KS_K_OTHER, 24.0 * n * ncols);
#define KSL_LAUNCH(KT, VEC, PL) do { const int grid = ks_sweep_grid_for(ctx, n, VEC, (const void *)k_block_residual<KT, VEC, PL>, 0); R->last_grid = grid;            \
      hipLaunchKernelGGL((k_block_residual<KT, VEC, PL>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, AX, ldax, BX, ldbx, Rd, ldr, n, th, R->partials); } while (0)
#define KSL_CASE(KT) case KT: if (!v2) KSL_LAUNCH(KT, 1, true); else if (plain) KSL_LAUNCH(KT, 2, true); else KSL_LAUNCH(KT, 2, false); break;
    switch (ncols) {
      KSL_CASE(1) KSL_CASE(2) KSL_CASE(3) KSL_CASE(4) KSL_CASE(5) KSL_CASE(6) KSL_CASE(7) KSL_CASE(8)
      KSL_CASE(9) KSL_CASE(10) KSL_CASE(11) KSL_CASE(12) KSL_CASE(13) KSL_CASE(14) KSL_CASE(15) KSL_CASE(16)
    }
#undef KSL_CASE
#undef KSL_LAUNCH
    KS_HIP(hipGetLastError());
    KS_CALL(ksk_reduce_partials(R, ncols, R->coef));
  } else KS_HIP(hipMemsetAsync(R->coef, 0, sizeof(double) * ncols, ctx->stream));
  KS_CALL(ks_allreduce_sum(ctx, R->coef, ncols));
  KS_HIP(hipMemcpyAsync(norms, R->coef, sizeof(double) * ncols, hipMemcpyDeviceToHost, ctx->stream));
  KS_HIP(ks_sync(ctx));
  for (int i = 0; i < ncols; i++) norms[i] = sqrt(norms[i]);
  return KS_SUCCESS;
}

// R(:,j) = AX(:,j) - theta[j - l] BX(:,j) for the active columns [l, k) of R (at most 16; the same column indices in AX and BX), norms[j - l] = ||R(:,j)||_2
extern "C" int ks_bv_block_residual(ks_bv R, ks_bv AX, ks_bv BX, const double *theta, double *norms)
{
  KS_CHECK(R && AX && BX && theta && norms, KS_ERR_ARG_NULL, "NULL argument");
  KS_CALL(ksb_flush(R)); KS_CALL(ksb_flush(AX)); KS_CALL(ksb_flush(BX));
  KS_CHECK(R != AX && R != BX, KS_ERR_ARG_WRONG, "R must be a different BV from AX and BX");
  KS_CHECK(AX->n == R->n && BX->n == R->n, KS_ERR_ARG_INCOMP, "Mismatching local dimensions R %d, AX %d, BX %d", R->n, AX->n, BX->n);
  const int l = R->l, nc = R->k - R->l;
  if (nc <= 0) return KS_SUCCESS;
  KS_CHECK(nc <= 16, KS_ERR_ARG_OUTOFRANGE, "%d active columns: the block residual takes at most 16", nc);
  KS_CHECK(R->k <= AX->m && R->k <= BX->m, KS_ERR_ARG_SIZ, "AX (%d columns) and BX (%d) must hold the active columns [%d,%d) of R", AX->m, BX->m, l, R->k);
  KS_HIP(hipSetDevice(R->ctx->device));
  return ksl_block_residual(R, nc, ks_bv_col(AX, l), AX->ld, ks_bv_col(BX, l), BX->ld, ks_bv_col(R, l), R->ld, theta, norms);
}

// ---- the driver ----------------------------------------------------------------------------------------------------------------------------------
namespace {

struct Lobpcg {
  ks_eps eps; ks_ctx ctx; ks_mat A, B; ks_st st;
  ks_bv V = nullptr, X = nullptr, R = nullptr, P = nullptr, W = nullptr, AX = nullptr, BX = nullptr, Z = nullptr, Y = nullptr;
  int bs = 0, guard = 0, nc = 0, ld = 0; bool lock = true, flip = false;
  std::vector<double> theta;
  ~Lobpcg() { ks_bv_destroy(X); ks_bv_destroy(R); ks_bv_destroy(P); ks_bv_destroy(W); ks_bv_destroy(AX); ks_bv_destroy(BX); ks_bv_destroy(Z); ks_bv_destroy(Y); }

  // a work BV of m columns in the layout of the solution basis (BVDuplicateResize, lobpcg.c:114-121); ip: it carries the B-inner product
  int make(int m, bool ip, ks_bv *out)
  {
    KS_CALL(ks_bv_create(ctx, V->n, V->N, m, V->ld, out));
    (*out)->row_start = V->row_start;
    (*out)->matmult = KS_BV_MATMULT_MAT;                          // block products through ks_mat_mult_multi
    (*out)->orthog_type = V->orthog_type; (*out)->orthog_ref = V->orthog_ref; (*out)->orthog_eta = V->orthog_eta;
    if (ip && B) KS_CALL(ks_bv_set_matrix(*out, B));
    return KS_SUCCESS;
  }
  // columns [j0, j0 + nc) of S to columns [d0, ...) of D: one strided copy, enqueued
  int copy_block(ks_bv S, int j0, ks_bv D, int d0, int ncols)
  {
    if (ncols <= 0 || !V->n) return KS_SUCCESS;
    KS_HIP(hipMemcpy2DAsync(ks_bv_col(D, d0), sizeof(double) * D->ld, ks_bv_col(S, j0), sizeof(double) * S->ld, sizeof(double) * V->n, (size_t)ncols, hipMemcpyDeviceToDevice, ctx->stream));
    return KS_SUCCESS;
  }
  // BVOrthogonalize of the columns [l, k) of T with the reference's semantics (lobpcg.c:330,333; bvorthog.c:729): first against the columns before l
  // (BVOrthogonalize_BlockGS), then among themselves, as a block: one D2H for the coefficients against the leading columns, one for the Gram matrix.
  // The Gram matrix is scaled to unit diagonal before its Cholesky factorisation - the columns are nearly converged residuals of norm 1e-8 and less,
  // and a factorisation that fails on such a block must fail because of its directions, not its size. When it does fail (a Gram matrix squares
  // the condition of the block) the reference's column-by-column Gram-Schmidt takes over for this call; non-zero: a dependent column there too.
  int orthogonalize(ks_bv T, int l, int k)
  {
    const int na = k - l;
    KS_CALL(ks_bv_set_active_columns(T, l, k));
    std::vector<double> G((size_t)k * k, 0.0), S((size_t)k * k, 0.0);
    if (l) {
      KS_CALL(ksb_dot_range(T, l, k, T, 0, l, G.data(), k));
      KS_CALL(ks_eps_synchronize_values(eps, G.data(), G.size()));
      KS_CALL(ksb_mult_range(T, l, k, -1.0, 1.0, T, 0, l, G.data(), k));
    }
    KS_CALL(ksb_dot_range(T, l, k, T, l, k, G.data(), k));
    KS_CALL(ks_eps_synchronize_values(eps, G.data(), G.size()));
    std::vector<double> U((size_t)na * na, 0.0), d(na);
    bool ok = true;
    for (int i = 0; i < na; i++) { const double g = G[(size_t)(l + i) * k + l + i]; ok = ok && g > 0.0 && std::isfinite(g); d[i] = ok ? 1.0 / sqrt(g) : 0.0; }
    if (ok) {
      for (int j = 0; j < na; j++) for (int i = 0; i <= j; i++) U[(size_t)i + (size_t)j * na] = G[(size_t)(l + i) + (size_t)(l + j) * k] * d[i] * d[j];
      ok = ksd::potrf_upper(na, U.data(), na) == 0;
      if (ok) { for (int j = 0; j < na; j++) for (int i = j + 1; i < na; i++) U[(size_t)i + (size_t)j * na] = 0.0; ok = ksd::trtri_upper(na, U.data(), na) == 0; }
    }
    if (!ok) {
      T->orthog_block = KS_BV_ORTHOG_BLOCK_GS;
      const int rc = ks_bv_orthogonalize(T, nullptr, 0);
      return rc;
    }
    for (int j = 0; j < na; j++) for (int i = 0; i <= j; i++) S[(size_t)(l + i) + (size_t)(l + j) * k] = d[i] * U[(size_t)i + (size_t)j * na];     // T <- T D U^-1
    return ks_bv_multinplace(T, S.data(), k, l, k);
  }
  // DSSolve + DSSort + DSSynchronize of the projected pencil of order nv, then the Ritz values of the block (lobpcg.c:152-155, 360-364); *broke: B-Gram not definite
  int projected(int nv, int locked, bool *broke)
  {
    ksd::DsGhep &ds = eps->dsg;
    ds.n = nv;
    if (flip) for (int j = 0; j < nv; j++) for (int i = 0; i < nv; i++) ds.a(i, j) = -ds.a(i, j);
    const int info = ds.solve(theta.data());
    if (!info) ds.sort(theta.data());
    // rank 0's outcome, values and vectors to every rank (DSSynchronize_GHEP): the control flow that follows is then the same everywhere
    std::vector<double> pack((size_t)1 + ld + (size_t)ld * ld);
    pack[0] = (double)info; std::copy(theta.begin(), theta.end(), pack.begin() + 1); std::copy(ds.Q.begin(), ds.Q.end(), pack.begin() + 1 + ld);
    KS_CALL(ks_eps_synchronize_values(eps, pack.data(), pack.size()));
    std::copy(pack.begin() + 1, pack.begin() + 1 + ld, theta.begin()); std::copy(pack.begin() + 1 + ld, pack.end(), ds.Q.begin());
    *broke = pack[0] != 0.0;
    if (*broke) return KS_SUCCESS;
    for (int j = 0; j < nv; j++) if (locked + j < eps->ncv) eps->eigr[locked + j] = flip ? -theta[j] : theta[j];
    return KS_SUCCESS;
  }
  // Rayleigh-Ritz on the block X alone (lobpcg.c:143-160 and again after a hard lock, :260-278): AX = A X, X^T A X q = theta q, X <- X Q, AX <- AX Q
  int ritz_on_x(int locked, bool *broke)
  {
    ksd::DsGhep &ds = eps->dsg;
    KS_CALL(ks_bv_set_active_columns(X, 0, bs)); KS_CALL(ks_bv_set_active_columns(AX, 0, bs));
    KS_CALL(ks_bv_matmult(X, A, AX)); eps->lob.mat_columns += bs;
    std::fill(ds.A.begin(), ds.A.end(), 0.0); std::fill(ds.B.begin(), ds.B.end(), 0.0);
    KS_CALL(ks_bv_matproject(AX, nullptr, X, ds.A.data(), ld));
    for (int j = 0; j < bs; j++) ds.b(j, j) = 1.0;
    KS_CALL(projected(bs, locked, broke));
    if (*broke) return KS_SUCCESS;
    KS_CALL(ks_bv_multinplace(X, ds.Q.data(), ld, 0, bs));
    return ks_bv_multinplace(AX, ds.Q.data(), ld, 0, bs);
  }
  // W(:, ini:bs) made orthogonal to the ny columns of Y, as a block and twice (classical Gram-Schmidt with one refinement)
  int project_out(int ini, int ny)
  {
    std::vector<double> Cm((size_t)std::max(ny, 1) * bs);
    for (int pass = 0; pass < 2; pass++) {
      KS_CALL(ksb_dot_range(W, ini, bs, Y, 0, ny, Cm.data(), ny));              // Y^T B W (W carries the inner product)
      if (B) eps->lob.mat_columns += bs - ini;
      KS_CALL(ks_eps_synchronize_values(eps, Cm.data(), Cm.size()));
      KS_CALL(ksb_mult_range(W, ini, bs, -1.0, 1.0, Y, 0, ny, Cm.data(), ny));
    }
    return KS_SUCCESS;
  }
  int solve();
};

int Lobpcg::solve()
{
  ksd::DsGhep &ds = eps->dsg;
  const int nev = eps->nev, ncv = eps->ncv;
  theta.assign(ld, 0.0);
  KS_CALL(make(3 * bs, true, &Z)); KS_CALL(make(bs, true, &X)); KS_CALL(make(bs, true, &R)); KS_CALL(make(bs, true, &P)); KS_CALL(make(bs, true, &W));
  KS_CALL(make(bs, false, &AX));
  if (B) KS_CALL(make(bs, false, &BX));
  nc = V->nc;
  const bool haveY = nc > 0 || nev > bs - guard;
  if (haveY) {
    KS_CALL(make(nc + nev, true, &Y));
    for (int j = 0; j < nc; j++) KS_CALL(ks_bv_insert_vec(Y, j, ks_bv_col(V, -nc + j)));
  }
  // initial vectors: the caller's, then random ones, B-orthonormal and orthogonal to the constraints (lobpcg.c:133-141)
  int nini = 0;
  if (eps->ini && eps->nini) {
    nini = std::min(eps->nini, ncv - bs);
    std::vector<const double *> ptr(nini);
    for (int i = 0; i < nini; i++) ptr[i] = ks_bv_col(eps->ini, i);
    KS_CALL(ks_bv_insert_vecs(V, 0, &nini, ptr.data(), 1));
  }
  for (int k = nini; k < ncv - bs; k++) { KS_CALL(ks_bv_set_random_column(V, k, eps->seed)); KS_CALL(ks_bv_orthonormalizecolumn(V, k, 1, nullptr, nullptr)); }
  KS_CALL(copy_block(V, 0, X, 0, bs));
  bool broke = false;
  KS_CALL(ritz_on_x(0, &broke));
  if (broke) { eps->reason = KS_EPS_DIVERGED_BREAKDOWN; return KS_SUCCESS; }

  int locked = 0;     // hard-locked vectors: the leading columns of V, eigenvectors for good
  int nconv = 0;      // converged leading columns of the current block (soft-locked when locking is on)
  int its = 0;        // iterations of the current block
  std::vector<double> norms(bs);
  while (eps->reason == KS_EPS_CONVERGED_ITERATING) {
    eps->lob.iterations++;
    // residuals of the active columns and their norms (lobpcg.c:176-202)
    int ini = lock ? nconv : 0;
    if (B) { KS_CALL(ksb_matmult_block(X, B, ks_bv_col(X, ini), X->ld, ks_bv_col(BX, ini), BX->ld, bs - ini)); eps->lob.mat_columns += bs - ini; }
    ks_bv BXs = B ? BX : X;
    KS_CALL(ksl_block_residual(R, bs - ini, ks_bv_col(AX, ini), AX->ld, ks_bv_col(BXs, ini), BXs->ld, ks_bv_col(R, ini), R->ld, eps->eigr.data() + locked + ini, norms.data()));
    KS_CALL(ks_eps_synchronize_values(eps, norms.data(), (size_t)(bs - ini)));
    int k = ini; bool countc = true;
    for (int j = ini; j < bs; j++) {
      const int i = locked + j;
      eps->errest[i] = ks_eps_converged_estimate(eps, eps->eigr[i], eps->eigi[i], norms[j - ini]);
      if (countc) { if (eps->errest[i] < eps->tol) k++; else countc = false; }
      if (!countc && !eps->trackall) break;
    }
    KS_CHECK(!eps->cb_err, eps->cb_err, "the user's convergence test returned %d", eps->cb_err);
    nconv = k;
    eps->nconv = locked + nconv;
    if (its) KS_CALL(ks_eps_monitor_call(eps, eps->its + its, eps->nconv, locked + bs));
    KS_CALL(ks_eps_stopping_call(eps, eps->its + its, eps->nconv));
    const bool hard = nconv >= bs - guard;
    if (eps->reason != KS_EPS_CONVERGED_ITERATING || hard) KS_CALL(copy_block(X, 0, V, locked, nconv));
    if (eps->reason != KS_EPS_CONVERGED_ITERATING) break;
    if (hard) { eps->its += its - 1; its = 0; } else its++;

    if (hard) {
      // hard locking (lobpcg.c:219-281): the converged vectors join the constraints, the rest of the block moves to the front, fresh vectors from V fill it up
      eps->lob.hard_locks++;
      KS_CALL(copy_block(X, 0, Y, nc + locked, nconv));
      for (int j = nconv; j < bs; j++) {
        KS_CALL(ks_bv_copycolumn(X, j, j - nconv)); KS_CALL(ks_bv_copycolumn(R, j, j - nconv)); KS_CALL(ks_bv_copycolumn(P, j, j - nconv)); KS_CALL(ks_bv_copycolumn(AX, j, j - nconv));
        if (B) KS_CALL(ks_bv_copycolumn(BX, j, j - nconv));
      }
      KS_CALL(ks_bv_set_active_columns(Y, 0, nc + locked + nconv));
      for (int j = bs - nconv; j < bs; j++) {
        KS_CALL(ksk_copy(ctx, ks_bv_col(V, locked + bs + (j - (bs - nconv))), ks_bv_col(X, j), V->n));
        double norm = 0.0; int lindep = 0;
        KS_CALL(ks_bv_orthogonalizevec(Y, ks_bv_col(X, j), nullptr, &norm, &lindep));
        if (!(norm > 0.0) || lindep) { eps->reason = KS_EPS_DIVERGED_BREAKDOWN; break; }      // "Orthogonalization of initial vector failed"
        KS_CALL(ksk_scale(ctx, ks_bv_col(X, j), V->n, 1.0 / norm));
      }
      if (eps->reason != KS_EPS_CONVERGED_ITERATING) break;
      locked += nconv; nconv = 0;
      if (orthogonalize(X, 0, bs)) { eps->reason = KS_EPS_DIVERGED_BREAKDOWN; break; }
      KS_CALL(ritz_on_x(locked, &broke));
      if (broke) { eps->reason = KS_EPS_DIVERGED_BREAKDOWN; break; }
      continue;
    }

    // preconditioned residuals (lobpcg.c:283-327) of the columns that are still active now - the ones that converged in this pass keep the plain
    // residual just computed in R, small and unscaled -, orthogonal to the constraints and the hard-locked vectors, then B-orthonormal
    ini = lock ? nconv : 0;
    KS_CALL(ks_st_apply_mat(st, bs - ini, ks_bv_col(R, ini), R->ld, ks_bv_col(W, ini), W->ld)); eps->lob.pc_columns += st->pc_type == KS_PC_NONE ? 0 : bs - ini;
    if (nc + locked > 0) KS_CALL(project_out(ini, nc + locked));
    KS_CALL(copy_block(W, ini, R, ini, bs - ini));
    if (orthogonalize(R, ini, bs)) { eps->reason = KS_EPS_DIVERGED_BREAKDOWN; break; }
    if (its > 1 && orthogonalize(P, ini, bs)) { eps->reason = KS_EPS_DIVERGED_BREAKDOWN; break; }      // the conjugate directions (lobpcg.c:333)

    // Z = [X, R(:,ini:), P(:,ini:)] and its two Gram matrices (lobpcg.c:335-357)
    const int na = bs - ini, nv = its > 1 ? bs + 2 * na : bs + na;
    KS_CALL(copy_block(X, 0, Z, 0, bs)); KS_CALL(copy_block(R, ini, Z, bs, na));
    if (its > 1) KS_CALL(copy_block(P, ini, Z, bs + na, na));
    KS_CALL(ks_bv_set_active_columns(Z, 0, nv));
    std::fill(ds.A.begin(), ds.A.end(), 0.0); std::fill(ds.B.begin(), ds.B.end(), 0.0);
    KS_CALL(ks_bv_matproject(Z, A, Z, ds.A.data(), ld)); eps->lob.mat_columns += nv;
    KS_CALL(ks_bv_matproject(Z, B, Z, ds.B.data(), ld)); if (B) eps->lob.mat_columns += nv;        // B NULL: Z^T Z
    KS_CALL(projected(nv, locked, &broke));
    if (broke) { eps->reason = KS_EPS_DIVERGED_BREAKDOWN; break; }

    // Ritz vectors (lobpcg.c:367-377): P = [R P] Q(bs:nv, 0:bs), X = P + X Q(0:bs, 0:bs), then A X for the columns that still move
    KS_CALL(ksb_mult_range(P, 0, bs, 1.0, 0.0, Z, bs, nv, ds.Q.data(), ld));
    KS_CALL(copy_block(P, 0, X, 0, bs));
    KS_CALL(ksb_mult_range(X, 0, bs, 1.0, 1.0, Z, 0, bs, ds.Q.data(), ld));
    KS_CALL(ksb_matmult_block(X, A, ks_bv_col(X, ini), X->ld, ks_bv_col(AX, ini), AX->ld, bs - ini)); eps->lob.mat_columns += bs - ini;
  }
  eps->its += its;
  return KS_SUCCESS;
}

} // namespace

// EPSSetUp_LOBPCG (lobpcg.c:55-83) with the parts of EPSSetUp whose rules are this solver's: problem type, sort criterion, dimensions, the ST as a
// preconditioner, B as the inner product; then the common part and the projected problem
static int lobpcg_setup(ks_eps eps)
{
  KS_CHECK(eps->A, KS_ERR_ORDER, "EPSSetOperators must be called first");
  ks_mat A = eps->A;
  KS_HIP(hipSetDevice(eps->ctx->device));
  const int n = A->n_global;
  int ptype = eps->problem_type;
  if (!eps->B && ptype == KS_EPS_GHEP) ptype = KS_EPS_HEP;
  KS_CHECK(ptype == KS_EPS_HEP || ptype == KS_EPS_GHEP, KS_ERR_SUP, "LOBPCG: wrong value of the problem type, only Hermitian (HEP) or generalized Hermitian positive definite (GHEP) problems");   // EPSCheckHermitianDefinite
  KS_CHECK(!eps->B || ptype == KS_EPS_GHEP, KS_ERR_ARG_INCOMP, "Inconsistent EPS state: the problem type does not match the number of matrices");
  KS_CHECK(!eps->twosided, KS_ERR_SUP, "LOBPCG does not compute left eigenvectors (EPSSetTwoSided)");
  KS_CHECK(!eps->arb_fn, KS_ERR_SUP, "LOBPCG does not support arbitrary selection of eigenpairs");
  KS_CHECK(eps->extraction == KS_EPS_RITZ, KS_ERR_SUP, "LOBPCG does not support extraction variants");
  const int which = eps->which.which ? eps->which.which : KS_EPS_SMALLEST_REAL;
  KS_CHECK(which == KS_EPS_SMALLEST_REAL || which == KS_EPS_LARGEST_REAL, KS_ERR_SUP, "This solver supports only smallest real or largest real eigenvalues");
  const int nev = eps->nev;
  const int bs = eps->lob.bs ? eps->lob.bs : std::min(16, nev);
  KS_CHECK(n - eps->nds >= 5 * bs, KS_ERR_SUP, "The problem size is too small relative to the block size");
  const int kmin = std::max(3 * bs, ((nev - 1) / bs + 3) * bs);
  KS_CHECK(!eps->ncv_user || eps->ncv_user >= kmin, KS_ERR_USER_INPUT, "The value of ncv is not sufficiently large");
  KS_CHECK(!eps->mpd_user || eps->mpd_user == 3 * bs, KS_ERR_USER_INPUT, "This solver does not allow a value of mpd different from 3*blocksize");
  eps->mpd = 3 * bs;                                                   // the block size of this solve, for ks_lobpcg_solve
  if (eps->conv == KS_EPS_CONV_NORM) KS_CALL(ks_eps_matrix_norms(eps));
  eps->cmp_final = eps->which; eps->cmp_final.which = which; eps->cmp_ds = eps->cmp_final;
  // the ST only preconditions: K = A - sigma B with sigma the shift, or the target when none was set (precond.c:65)
  ks_st st = nullptr;
  KS_CALL(ks_eps_get_st(eps, &st));
  if (!st->type_set && st->type != KS_ST_PRECOND) { st->type = KS_ST_PRECOND; st->ready = false; }
  if (!st->sigma_set && st->sigma != eps->which.target) { st->sigma = eps->which.target; st->ready = false; }
  KS_CALL(ks_st_set_matrices(st, A, eps->B)); st->ready = false;
  KS_CALL(ks_st_setup_internal(st));
  eps->op = A;
  KS_CALL(eps_setup_common(eps, eps->ncv_user ? eps->ncv_user : kmin, ptype == KS_EPS_GHEP ? eps->B : nullptr));
  eps->ghep = ptype == KS_EPS_GHEP; eps->problem_type_resolved_hermitian = true; eps->left_trivial = true;
  eps->dsg.allocate(3 * bs); eps->dsg.which = ksd::KsCompare(); eps->dsg.which.which = KS_EPS_SMALLEST_REAL;     // the flipped spectrum is sorted like the other (lobpcg.c:103-107)
  return KS_SUCCESS;
}

// EPSSolve_LOBPCG. It leaves the eigenvectors in V(:,0:nconv): nothing for the epilogue to map back, purify or normalise again (no compute_vectors)
int ks_lobpcg_solve(ks_eps eps)
{
  Lobpcg s;
  s.eps = eps; s.ctx = eps->ctx; s.A = eps->A; s.B = eps->ghep ? eps->B : nullptr; s.st = eps->st; s.V = eps->V;
  s.bs = eps->mpd / 3; s.ld = eps->mpd; s.lock = eps->lob.lock; s.flip = eps->cmp_final.which == KS_EPS_LARGEST_REAL;
  const double restart = eps->lob.restart ? eps->lob.restart : 0.9;
  s.guard = s.bs == 1 ? 0 : std::min((int)((1.0 - restart) * s.bs + 0.45), s.bs - 1);
  const int rc = s.solve();
  ks_bv_destroy(eps->ini); eps->ini = nullptr; eps->nini = 0;                                                     // the initial space is consumed like the deflation space
  ks_bv_gs_passes(eps->V, &eps->passes0[0], nullptr);     // the passes stat counts the Gram-Schmidt passes of Krylov expansions: none here, the initial vectors in V are not one
  return rc;
}

const ks_eps_ops *ks_lobpcg_ops()
{
  static const ks_eps_ops ops = {lobpcg_setup, ks_lobpcg_solve, nullptr};
  return &ops;
}
