// Krylov-Schur, one-sided and two-sided: the solver's set-up rules, the two restart loops and what they share, the eigenvectors of the Schur form.
// The dense projected problem of a restart (DS HEP / NHEP / NHEPTS), the eigenvalue comparisons and the ST's eigenvalue map are host-only code in ks_ds.cpp.
// Restates, in plain C++ on host scalars:
//   EPSSetUp_KrylovSchur, EPSSetDimensions_Default      src/eps/impls/krylov/krylovschur/krylovschur.c:93-194, src/eps/interface/epssetup.c:654-678
//   EPSSolve_KrylovSchur_Default, EPSKrylovConvergence  krylovschur.c:227-337, src/eps/impls/krylov/epskrylov.c:207-295
//   EPSSolve_KrylovSchur_TwoSided                       krylovschur/ks-twosided.c:27-241
//   EPSGetStartVector / EPSGetLeftStartVector           src/eps/interface/epssolve.c:841-873, 879-900
//   EPSComputeVectors_Hermitian / _Schur / _Twosided    src/eps/interface/epsdefault.c:27-169
#include "ksgpu_internal.h"
#include "ks_eps_impl.h"
#include "ks_dense.h"
#include <algorithm>
#include <limits>

// DSSynchronize (dsops.c:875 -> DSSynchronize_HEP dshep.c:673-713, DSSynchronize_NHEP dsnhep.c:379): every rank leaves with rank 0's
// projected matrix, vectors and eigenvalues. The scalars the convergence test and the restart sizes are computed from (beta of the
// expansion, its length, the breakdown flag) travel in the same message, so the integer control flow that follows is identical on
// all ranks whatever the allreduce provider returned.
static int ds_synchronize(ks_eps eps, std::vector<double> *M1, std::vector<double> *M2, double *beta, int *nv, int *breakdown)
{
  ks_ctx ctx = eps->ctx;
  if (!ks_is_multi(ctx) || eps->ds_parallel != KS_DS_PARALLEL_SYNCHRONIZED) return KS_SUCCESS;      // (the force_multi test hook issues it on one rank too)
  std::vector<double> *const parts[4] = {M1, M2, &eps->eigr, &eps->eigi};
  std::vector<double> pack;
  for (std::vector<double> *p : parts) pack.insert(pack.end(), p->begin(), p->end());
  pack.push_back(*beta); pack.push_back((double)*nv); pack.push_back((double)*breakdown);
  KS_CALL(ks_comm_bcast0_host(ctx, pack.data(), (int)(pack.size() * sizeof(double))));
  size_t o = 0;
  for (std::vector<double> *p : parts) { std::copy(pack.begin() + o, pack.begin() + o + p->size(), p->begin()); o += p->size(); }
  *beta = pack[o]; *nv = (int)pack[o + 1]; *breakdown = (int)pack[o + 2];
  return KS_SUCCESS;
}

// EPSComputeRitzVector epsdefault.c:313-364: x = V(:,0:nv) Zr (W column 3) and, for a pair, y = V(:,0:nv) Zi (W column 4), purified through the
// operator for a GHEP
static int ritz_vector(ks_eps eps, int nv, const double *Zr, const double *Zi)
{
  ks_bv V = eps->V, W = eps->W;
  int ls = 0, ksv = 0;
  KS_CALL(ks_bv_get_active_columns(V, &ls, &ksv));
  KS_CALL(ks_bv_set_active_columns(V, 0, nv));
  double *x = ks_bv_col(W, 3), *y = ks_bv_col(W, 4);
  KS_CALL(ks_bv_multvec(V, 1.0, 0.0, x, Zr));
  if (eps->ghep && eps->purify) {                                                    // eps->purify (epssetup.c:365-373)
    double norm = 0.0;
    KS_CALL(ks_mat_mult_internal(eps->op, x, y));
    KS_CALL(ksb_norm_b(V, y, &norm));
    KS_CALL(ksk_scale(eps->ctx, y, V->n, 1.0 / norm));
    KS_CALL(ksk_copy(eps->ctx, y, x, V->n));
  }
  if (Zi) KS_CALL(ks_bv_multvec(V, 1.0, 0.0, y, Zi));
  else KS_HIP(hipMemsetAsync(y, 0, sizeof(double) * V->n, eps->ctx->stream));   // VecSet(y,0.0) epsdefault.c:352
  KS_CALL(ks_bv_set_active_columns(V, ls, ksv));
  if (eps->balanced) {                                      // fix and normalise the eigenvector when balancing is used (epsdefault.c:336,349,355-361)
    KS_CALL(ks_eps_pointwise(eps, x, eps->D, x, false));
    if (Zi) KS_CALL(ks_eps_pointwise(eps, y, eps->D, y, false));
    double nx = 0.0, ny = 0.0;
    KS_CALL(ks_bv_normvec(W, x, KS_NORM_2, &nx));
    if (Zi) KS_CALL(ks_bv_normvec(W, y, KS_NORM_2, &ny));
    const double nrm = hypot(nx, ny);
    if (nrm != 0.0) { KS_CALL(ksk_scale(eps->ctx, x, V->n, 1.0 / nrm)); if (Zi) KS_CALL(ksk_scale(eps->ctx, y, V->n, 1.0 / nrm)); }
  }
  return KS_SUCCESS;
}

// EPSGetStartVector epssolve.c:841-873 and EPSGetLeftStartVector :879-900 on column i of bv: the caller's vector (host0, column 0 only), else a random
// one from `seed`, forced into the range of OP where asked (epssolve.c:860-868), orthonormalised in its basis. breakdown NULL: a dependent vector is
// an error, told with msg[0] for column 0 and msg[1] for a later one
static int start_vector(ks_eps eps, ks_bv bv, int i, const double *host0, uint64_t seed, bool in_range_of_op, const char *const msg[2], bool *breakdown)
{
  if (i == 0 && host0) KS_CALL(ks_bv_set_column_host(bv, 0, host0));
  else KS_CALL(ks_bv_set_random_column(bv, i, seed));
  if (in_range_of_op) {
    KS_CALL(ksk_copy(eps->ctx, ks_bv_col(bv, i), ks_bv_col(eps->W, 0), bv->n));
    KS_CALL(ks_mat_mult_internal(eps->op, ks_bv_col(eps->W, 0), ks_bv_col(bv, i)));
  }
  double norm = 0.0; int lindep = 0;
  KS_CALL(ks_bv_orthogonalizecolumn(bv, i, nullptr, &norm, &lindep));
  if (breakdown) *breakdown = lindep != 0;
  else if (lindep || norm == 0.0) {
    if (i == 0) KS_FAIL(KS_ERR_PLIB, "%s", msg[0]);
    KS_FAIL(KS_ERR_CONV_FAILED, "%s", msg[1]);
  }
  KS_CALL(ks_bv_scalecolumn(bv, i, 1.0 / norm));
  return KS_SUCCESS;
}
static int right_start_vector(ks_eps eps, int i, bool *breakdown)
{
  static const char *const msg[2] = {"Initial vector is zero or belongs to the deflation space", "Unable to generate more start vectors"};
  return start_vector(eps, eps->V, i, eps->have_v0 ? eps->v0.data() : nullptr, eps->seed, eps->ghep, msg, breakdown);
}
static int left_start_vector(ks_eps eps, int i, bool *breakdown)      // its own stream of random numbers
{
  static const char *const msg[2] = {"Left initial vector is zero", "Unable to generate more left start vectors"};
  return start_vector(eps, eps->VL, i, eps->have_w0 ? eps->w0.data() : nullptr, eps->seed ^ 0x9E3779B97F4A7C15ULL, false, msg, breakdown);
}

// EPSKrylovConvergence epskrylov.c:207-295 with its conjugate pairs: error estimates of the Ritz pairs nconv.. of ds until the first one that has
// not converged (all of them under trackall); *kout = the number of converged pairs. The estimate of a pair is (resnorm * beta) * corrf - in this
// association: the one-sided loop passes beta * gamma and 1.0, the two-sided one beta and the norm of its corrected residual vector, and an estimate
// that moves by one rounding can move a convergence decision. `left` (the two-sided variant): the same for the left Ritz pairs, the maximum counts.
struct KrylovLeft { ksd::DsNhepTs *ds; double betat, corrft; };
static int krylov_convergence(ks_eps eps, ksd::Ds &ds, int nv, double beta, double corrf, const KrylovLeft *left, int *kout)
{
  const ksd::StMap &map = eps->cmp_ds.map;
  const bool early = map && (map.type == KS_ST_SHIFT || eps->conv == KS_EPS_CONV_NORM);    // epskrylov.c:253: back-transform before the estimate
  int marker = -1;
  for (int k = eps->nconv; k < nv; k++) {
    double re = eps->eigr[k], im = eps->eigi[k];
    if (early) map.backtransform(1, &re, &im);
    double resnorm = 0.0; const double *Zr = nullptr, *Zi = nullptr;
    const int newk = ds.ritz(k, &resnorm, &Zr, &Zi);
    if (eps->trueres) {                                        // epskrylov.c:256-264 (-eps_true_residual): the Ritz vector, then its residual
      if (!early) map.backtransform(1, &re, &im);
      KS_CALL(ritz_vector(eps, nv, Zr, Zi));
      KS_CALL(ks_eps_residual_norm(eps, re, im, ks_bv_col(eps->W, 3), Zi ? ks_bv_col(eps->W, 4) : nullptr, 1.0, &resnorm));
    } else resnorm = (resnorm * beta) * corrf;                 // corrf: harmonic KS (in beta here) and two-sided KS (epskrylov.c:265,269)
    eps->errest[k] = ks_eps_converged_estimate(eps, re, im, resnorm);
    if (marker == -1 && eps->errest[k] >= eps->tol) marker = k;
    if (left) {                                                // epskrylov.c:269-276
      double lresnorm = 0.0;
      left->ds->vectors_side(k, true, true, &lresnorm);
      const double lerrest = ks_eps_converged_estimate(eps, re, im, (lresnorm * left->betat) * left->corrft);
      eps->errest[k] = std::max(eps->errest[k], lerrest);
      if (marker == -1 && lerrest >= eps->tol) marker = k;
    }
    if (newk == k + 1) { eps->errest[k + 1] = eps->errest[k]; k++; }
    if (marker != -1 && !eps->trackall) break;                 // getall: estimates for every Ritz pair (epskrylov.c:240,280)
  }
  *kout = (marker != -1) ? marker : nv;
  KS_CHECK(!eps->cb_err, eps->cb_err, "the user's convergence test returned %d", eps->cb_err);
  return KS_SUCCESS;
}

// "update l" of both loops (krylovschur.c:289-300): the number of Ritz pairs kept by the restart. The non-locking variant keeps the converged ones
// among them and resets their count
static int restart_size(ks_eps eps, ksd::Ds &ds, int *k, int nv, bool breakdown)
{
  int l = 0;
  if (eps->reason == KS_EPS_CONVERGED_ITERATING && !breakdown && *k != nv) {
    l = std::max(1, (int)((nv - *k) * eps->keep));
    l = ds.truncate_size(*k, nv, l);                           // do not split a 2x2 block (krylovschur.c:300)
  }
  if (!eps->lock && l > 0) { l += *k; *k = 0; }                // non-locking variant: reset no. of converged pairs (krylovschur.c:294)
  return l;
}

// EPSSolve_KrylovSchur_Default (krylovschur.c:227-337) over the DS interface. Symmetric variant: BVMatLanczos into T, arbitrary selection. General
// variant: BVMatArnoldi into A, harmonic extraction.
static int restart_loop(ks_eps eps, ksd::Ds &ds)
{
  ks_bv V = eps->V;
  const int nev = eps->nev, ncv = eps->ncv, mpd = eps->mpd;
  const bool hermitian = eps->problem_type_resolved_hermitian, harmonic = eps->extraction == KS_EPS_HARMONIC;   // harmonic: on eps->dsn
  const ksd::StMap &map = eps->cmp_ds.map;
  std::vector<double> g(harmonic ? ncv + 1 : 0);
  KS_CALL(right_start_vector(eps, 0, nullptr));
  int l = 0;
  while (eps->reason == KS_EPS_CONVERGED_ITERATING) {
    eps->its++;
    int nv = std::min(eps->nconv + mpd, ncv);
    if (eps->max_steps && eps->steps + (nv - (eps->nconv + l)) > eps->max_steps) nv = eps->nconv + l + (int)(eps->max_steps - eps->steps);
    ds.set_dimensions(nv, eps->nconv, eps->nconv + l);
    double beta = 0.0; int breakdown = 0;
    const int k0 = eps->nconv + l;
    // the run's last final update may wait for the restart product below (ksb_restart); whatever touches the basis before that flushes it
    const bool defer0 = V->defer.want; V->defer.want = true;
    const int rck = hermitian ? ks_bv_matlanczos(V, eps->op, ds.M().data(), ds.ld, k0, &nv, &beta, &breakdown)
                              : ks_bv_matarnoldi(V, eps->op, ds.M().data(), ds.ld, k0, &nv, &beta, &breakdown);
    V->defer.want = defer0;
    KS_CALL(rck);
    eps->steps += nv - k0;
    ds.set_dimensions(nv, eps->nconv, eps->nconv + l);
    ds.state = l ? ksd::DS_RAW : ksd::DS_INTERMEDIATE;
    KS_CALL(ks_bv_set_active_columns(V, eps->nconv, nv));

    // translation of the Krylov decomposition for harmonic extraction (krylovschur.c:270-271)
    double gamma = 1.0;
    if (harmonic) KS_CHECK(!eps->dsn.translate_harmonic(eps->which.target, beta, false, g.data(), &gamma), KS_ERR_LIB, "harmonic extraction: H - target*I is singular");

    // solve projected problem
    int info = ds.solve(eps->eigr.data(), eps->eigi.data());
    KS_CHECK(info == 0, KS_ERR_LIB, hermitian ? "tridiagonal QL iteration failed to converge (info=%d)" : "Hessenberg QR iteration failed to converge (info=%d)", info);
    std::vector<double> rr, ri;
    if (eps->arb_fn) {                                         // EPSGetArbitraryValues krylovschur.c:30-58, then DSSort on rr/ri
      rr.assign(ncv + 1, 0.0); ri.assign(ncv + 1, 0.0);
      for (int i = ds.l; i < ds.n; i++) {
        double re = eps->eigr[i], im0 = 0.0;
        map.backtransform(1, &re, &im0);
        KS_CALL(ritz_vector(eps, nv, ds.Q.data() + (size_t)i * ds.ld, nullptr));       // DSVectors(X,i) = Q(:,i) for DSHEP
        KS_HIP(ks_sync(eps->ctx));
        const int rc = eps->arb_fn(re, im0, ks_bv_col(eps->W, 3), ks_bv_col(eps->W, 4), &rr[i], &ri[i], eps->arb_ctx);
        KS_CHECK(!rc, rc, "the user's arbitrary selection function returned %d", rc);
      }
    }
    info = ds.sort(eps->eigr.data(), eps->eigi.data(), eps->arb_fn ? rr.data() : nullptr, eps->arb_fn ? ri.data() : nullptr);
    KS_CHECK(info == 0, KS_ERR_LIB, "reordering of the Schur form failed: blocks too close to swap");
    ds.update_extra_row();
    KS_CALL(ds_synchronize(eps, &ds.M(), &ds.Q, &beta, &nv, &breakdown));      // krylovschur.c:281

    // check convergence, then the stopping test and the step cap of the bench harness
    int k = 0;
    KS_CALL(krylov_convergence(eps, ds, nv, beta * gamma, 1.0, nullptr, &k));
    KS_CALL(ks_eps_stopping_call(eps, eps->its, k));
    if (eps->reason == KS_EPS_CONVERGED_ITERATING && eps->max_steps && eps->steps >= eps->max_steps) eps->reason = KS_EPS_CONVERGED_USER;
    const int nconv_mon = k;

    l = restart_size(eps, ds, &k, nv, breakdown);
    if (eps->reason == KS_EPS_CONVERGED_ITERATING) {
      if (breakdown || k == nv) {
        if (k < nev) {
          bool brk = false;
          KS_CALL(right_start_vector(eps, k, &brk));
          if (brk) eps->reason = KS_EPS_DIVERGED_BREAKDOWN;
        }
      } else {
        if (harmonic) {                                        // undo the translation (krylovschur.c:310-320): gamma u^ = u - U g~
          ds.set_dimensions(nv, k, l);
          eps->dsn.translate_harmonic(0.0, beta, true, g.data(), &gamma);
          KS_CALL(ks_bv_set_active_columns(V, 0, nv));
          KS_CALL(ks_bv_multcolumn(V, -1.0, 1.0, nv, g.data()));
          KS_CALL(ks_bv_scalecolumn(V, nv, 1.0 / gamma));
          KS_CALL(ks_bv_set_active_columns(V, eps->nconv, nv));
          ds.set_dimensions(nv, k, nv);
        }
        ds.truncate(k + l, false);
      }
    }
    // V(:,nconv:k+l) = V(:,nconv:nv) * Q(nconv:nv, nconv:k+l)      krylovschur.c:324-327
    if (eps->reason == KS_EPS_CONVERGED_ITERATING && !breakdown) KS_CALL(ksb_restart(V, ds.Q.data(), ds.ld, eps->nconv, k + l, nv, k + l));   // product, then BVCopyColumn(V,nv,k+l)
    else KS_CALL(ks_bv_multinplace(V, ds.Q.data(), ds.ld, eps->nconv, k + l));
    eps->nconv = k;
    KS_CALL(ks_eps_monitor_call(eps, eps->its, nconv_mon, nv));
    eps->restarts++;
  }
  ds.truncate(eps->nconv, true);
  return KS_SUCCESS;
}

// ---- two-sided variant (ks-twosided.c) ----
// BVMatProject(V,NULL,W,M) is L-shaped (BVMatProject_Dot bvglobal.c:1013-1049): with the active columns [k0, nv) of both bases it computes
// W0^T V1 and W1^T [V0 V1], everything but the leading k0 x k0 block, which the caller carries over from the previous restart
static int matproject_lshape(ks_bv V, ks_bv W, int k0, int nv, double *M, int ldm)
{
  KS_CALL(ksb_dot_range(V, k0, nv, W, 0, k0, M, ldm));
  return ksb_dot_range(V, 0, nv, W, k0, nv, M, ldm);
}
// EPSTwoSidedRQUpdate1 ks-twosided.c:27-73: the residual vectors are made orthogonal to the other side's basis, u <- u - V (W^T V)^-1 W^T u and
// its mirror image, and the last columns of the two Rayleigh quotients take the coefficients. One LU of M = W^T V, used as it is and transposed.
static int rq_update1(ks_eps eps, const std::vector<double> &M, int nv, double beta, double betat)
{
  ks_bv V = eps->V, W = eps->VL; ksd::DsNhepTs &ds = eps->dst;
  int l = 0, nnv = 0;
  KS_CALL(ks_bv_get_active_columns(V, &l, &nnv));
  KS_CALL(ks_bv_set_active_columns(V, 0, nv)); KS_CALL(ks_bv_set_active_columns(W, 0, nv));
  std::vector<double> w(nv), LU((size_t)nv * nv); std::vector<int> piv(nv);
  for (int j = 0; j < nv; j++) std::copy(M.begin() + (size_t)j * ds.ld, M.begin() + (size_t)j * ds.ld + nv, LU.begin() + (size_t)j * nv);
  KS_CALL(ks_bv_dotvec(W, ks_bv_col(V, nv), w.data()));
  KS_CALL(ks_eps_synchronize_values(eps, w.data(), w.size()));
  const int info = ksd::lu_factor(nv, LU.data(), nv, piv.data());
  KS_CHECK(info == 0, KS_ERR_LIB, "two-sided Krylov-Schur: W^T V is singular (zero pivot %d of %d): serious breakdown of the two-sided recurrence", info, nv);
  ksd::lu_solve(nv, LU.data(), nv, piv.data(), w.data(), false);
  KS_CALL(ks_bv_multcolumn(V, -1.0, 1.0, nv, w.data()));
  for (int i = 0; i < nv; i++) ds.a(i, nv - 1) += beta * w[i];
  KS_CALL(ks_bv_dotvec(V, ks_bv_col(W, nv), w.data()));
  KS_CALL(ks_eps_synchronize_values(eps, w.data(), w.size()));
  ksd::lu_solve(nv, LU.data(), nv, piv.data(), w.data(), true);
  KS_CALL(ks_bv_multcolumn(W, -1.0, 1.0, nv, w.data()));
  for (int i = 0; i < nv; i++) ds.hb.a(i, nv - 1) += betat * w[i];
  KS_CALL(ks_bv_set_active_columns(V, l, nnv)); KS_CALL(ks_bv_set_active_columns(W, l, nnv));
  return KS_SUCCESS;
}
// EPSTwoSidedRQUpdate2 ks-twosided.c:75-124: column kk of each basis (the residual vector, or a new start vector) is orthonormalised against its own
// basis again and the kept block of the Rayleigh quotient follows, H <- H + (V^T u) b^T from the old nconv on; then M <- Z^T M Q with the full nv x nv Q and Z
static int rq_update2(ks_eps eps, std::vector<double> &M, int kk)
{
  ks_bv V = eps->V, W = eps->VL; ksd::DsNhepTs &ds = eps->dst;
  const int ld = ds.ld;
  int l = 0, nv = 0;
  KS_CALL(ks_bv_get_active_columns(V, &l, &nv));
  KS_CALL(ks_bv_set_active_columns(V, 0, nv)); KS_CALL(ks_bv_set_active_columns(W, 0, nv));
  std::vector<double> c(ld + 1, 0.0);
  for (int side = 0; side < 2; side++) {
    ksd::DsNhep &h = side ? eps->dst.hb : static_cast<ksd::DsNhep &>(eps->dst);
    double norm = 0.0;
    KS_CALL(ks_bv_orthogonalizecolumn(side ? W : V, kk, c.data(), &norm, nullptr));
    KS_CALL(ks_bv_scalecolumn(side ? W : V, kk, 1.0 / norm));
    for (int j = l; j < kk; j++) {
      for (int i = 0; i < kk; i++) h.a(i, j) += c[i] * h.a(kk, j);
      h.a(kk, j) *= norm;
    }
  }
  std::vector<double> T((size_t)nv * nv);
  for (int j = 0; j < nv; j++) for (int i = 0; i < nv; i++) { double s = 0.0; for (int p = 0; p < nv; p++) s += M[(size_t)i + (size_t)p * ld] * ds.q(p, j); T[(size_t)i + (size_t)j * nv] = s; }
  for (int j = 0; j < nv; j++) for (int i = 0; i < nv; i++) { double s = 0.0; for (int p = 0; p < nv; p++) s += ds.hb.q(p, i) * T[(size_t)p + (size_t)j * nv]; M[(size_t)i + (size_t)j * ld] = s; }
  KS_CALL(ks_bv_set_active_columns(V, l, nv)); KS_CALL(ks_bv_set_active_columns(W, l, nv));
  return KS_SUCCESS;
}

// EPSSolve_KrylovSchur_TwoSided ks-twosided.c:126-241: per restart one Arnoldi expansion with Op and one with Op^T, both through ks_bv_matarnoldi
static int restart_loop_twosided(ks_eps eps)
{
  ks_bv V = eps->V, W = eps->VL; ksd::DsNhepTs &ds = eps->dst;
  const int nev = eps->nev, ncv = eps->ncv, mpd = eps->mpd, ld = ds.ld;
  std::vector<double> M((size_t)ld * ld, 0.0);                     // W^T V (the reference's ncv x ncv M)
  KS_CALL(right_start_vector(eps, 0, nullptr));
  KS_CALL(left_start_vector(eps, 0, nullptr));
  int l = 0;
  while (eps->reason == KS_EPS_CONVERGED_ITERATING) {
    eps->its++;
    const int k0 = eps->nconv + l;
    int nv = std::min(eps->nconv + mpd, ncv);
    if (eps->max_steps && eps->steps + 2 * (nv - k0) > eps->max_steps) nv = k0 + std::max(1, (int)((eps->max_steps - eps->steps) / 2));   // (a step of each run per column)
    ds.set_dimensions(nv, eps->nconv, k0);
    double beta = 0.0, betat = 0.0; int breakdown = 0, breakdownt = 0;
    KS_CALL(ks_bv_matarnoldi(V, eps->op, ds.A.data(), ld, k0, &nv, &beta, &breakdown));
    int nvt = nv;
    KS_CALL(ks_bv_matarnoldi(W, eps->opT, ds.hb.A.data(), ld, k0, &nvt, &betat, &breakdownt));
    eps->steps += (nv - k0) + (nvt - k0);
    nv = std::min(nv, nvt);                                    // make sure both factorizations have the same length
    ds.set_dimensions(nv, eps->nconv, k0);
    ds.state = l ? ksd::DS_RAW : ksd::DS_INTERMEDIATE;
    breakdown = breakdown || breakdownt;

    // update M, modify the Rayleigh quotients
    KS_CALL(ks_bv_set_active_columns(V, k0, nv)); KS_CALL(ks_bv_set_active_columns(W, k0, nv));
    KS_CALL(matproject_lshape(V, W, k0, nv, M.data(), ld));
    KS_CALL(ks_eps_synchronize_values(eps, M.data(), M.size()));
    KS_CALL(rq_update1(eps, M, nv, beta, betat));

    // solve projected problem
    int info = ds.solve(eps->eigr.data(), eps->eigi.data());
    KS_CHECK(info == 0, KS_ERR_LIB, "Hessenberg QR iteration failed to converge (info=%d)", info);
    info = ds.sort(eps->eigr.data(), eps->eigi.data());
    KS_CHECK(info != 2, KS_ERR_LIB, "two-sided projected problem: invalid permutation due to a 2x2 block (the two halves do not hold the same eigenvalues)");
    KS_CHECK(info == 0, KS_ERR_LIB, "reordering of the Schur form failed: blocks too close to swap");
    KS_CALL(ds_synchronize(eps, &ds.A, &ds.Q, &beta, &nv, &breakdown));
    KS_CALL(ds_synchronize(eps, &ds.hb.A, &ds.hb.Q, &betat, &nv, &breakdown));
    ds.update_extra_row();

    // check convergence: RQUpdate1 changed the two residual vectors, so their norms belong in the estimates (epskrylov.c:269-276)
    double norm = 0.0, norm2 = 0.0;
    KS_CALL(ks_bv_normcolumn(V, nv, KS_NORM_2, &norm));
    KS_CALL(ks_bv_normcolumn(W, nv, KS_NORM_2, &norm2));
    { double nn[2] = {norm, norm2}; KS_CALL(ks_eps_synchronize_values(eps, nn, 2)); norm = nn[0]; norm2 = nn[1]; }
    int k = 0;
    const KrylovLeft left = {&ds, betat, norm2};
    KS_CALL(krylov_convergence(eps, ds, nv, beta, norm, &left, &k));
    KS_CALL(ks_eps_stopping_call(eps, eps->its, k));
    if (eps->reason == KS_EPS_CONVERGED_ITERATING && eps->max_steps && eps->steps >= eps->max_steps) eps->reason = KS_EPS_CONVERGED_USER;
    const int nconv_mon = k;

    l = restart_size(eps, ds, &k, nv, breakdown);

    // update the corresponding vectors V(:,idx) = V*Q(:,idx), W(:,idx) = W*Z(:,idx)
    KS_CALL(ks_bv_set_active_columns(V, eps->nconv, nv)); KS_CALL(ks_bv_set_active_columns(W, eps->nconv, nv));
    KS_CALL(ks_bv_multinplace(V, ds.Q.data(), ld, eps->nconv, k + l));
    KS_CALL(ks_bv_multinplace(W, ds.hb.Q.data(), ld, eps->nconv, k + l));
    if (eps->reason == KS_EPS_CONVERGED_ITERATING && !breakdown) { KS_CALL(ks_bv_copycolumn(V, nv, k + l)); KS_CALL(ks_bv_copycolumn(W, nv, k + l)); }

    if (eps->reason == KS_EPS_CONVERGED_ITERATING) {
      if (breakdown || k == nv) {                              // start a new Arnoldi factorization
        if (k < nev) {
          bool brk = false, brkl = false;
          KS_CALL(right_start_vector(eps, k, &brk));
          KS_CALL(left_start_vector(eps, k, &brkl));
          if (brk || brkl) eps->reason = KS_EPS_DIVERGED_BREAKDOWN;
        }
      } else {
        ds.set_dimensions(ds.n, k, ds.k);
        ds.truncate(k + l, false);
      }
      KS_CALL(rq_update2(eps, M, k + l));
    }
    eps->nconv = k;
    KS_CALL(ks_eps_monitor_call(eps, eps->its, nconv_mon, nv));
    eps->restarts++;
  }
  ds.truncate(eps->nconv, true);
  eps->twosided_solved = true;                                 // V and VL hold both sides' Schur vectors: the epilogue and the getters take the left branches
  return KS_SUCCESS;
}

// EPSComputeVectors_Schur epsdefault.c:105-169, run on first use (EPSComputeVectors epssolve.c:... state EPS_STATE_EIGENVECTORS):
// X = V*Z with Z the normalised eigenvectors of the trimmed quasi-triangular T. Until then V(:,0:nconv) is the orthonormal
// Schur basis that EPSGetInvariantSubspace hands out.
int ks_eps_schur_vectors(ks_eps eps)
{
  if (eps->vectors_done) return KS_SUCCESS;
  ks_bv V = eps->V; ksd::DsNhep &ds = eps->twosided_solved ? static_cast<ksd::DsNhep &>(eps->dst) : eps->dsn;
  const int nc = eps->nconv;
  KS_CALL(ks_bv_set_active_columns(V, 0, nc));
  if (nc) {
    for (int k = 0; k < nc; k++) k = ds.vectors(k, false, nullptr);
    KS_CALL(ks_bv_multinplace(V, ds.X.data(), ds.ld, 0, nc));
    if (eps->balanced) {                                    // epsdefault.c:130-139: x <- D \ x, then normalise (pairs together)
      for (int i = 0; i < nc; i++) KS_CALL(ks_eps_pointwise(eps, ks_bv_col(V, i), eps->D, ks_bv_col(V, i), false));
      KS_CALL(ks_bv_normalize(V, eps->eigi.data()));
    }
    if (eps->twosided_solved) {                             // left eigenvectors (epsdefault.c:141-167): W <- W Y, normalise, then y = wr - i wi for a pair
      ks_bv W = eps->VL;
      KS_CALL(ks_bv_set_active_columns(W, 0, nc));
      for (int k = 0; k < nc; k++) k = eps->dst.vectors_side(k, true, false, nullptr);
      KS_CALL(ks_bv_multinplace(W, eps->dst.hb.X.data(), ds.ld, 0, nc));
      if (eps->B) {                                         // EPSComputeVectors_Twosided epsdefault.c:79-95: generalized problems, y <- P^-T y (shift: P = B)
        for (int i = 0; i < nc; i++) {
          KS_CALL(ksk_copy(eps->ctx, ks_bv_col(W, i), ks_bv_col(eps->W, 3), W->n));
          KS_CALL(ks_st_matsolve_transpose(eps->st, ks_bv_col(eps->W, 3), ks_bv_col(W, i)));
        }
      }
      KS_CALL(ks_bv_normalize(W, eps->eigi.data()));
      for (int i = 0; i < nc - 1; i++) if (eps->eigi[i] != 0.0) { if (eps->eigi[i] > 0.0) KS_CALL(ks_bv_scalecolumn(W, i + 1, -1.0)); i++; }
    }
  }
  eps->vectors_done = true;
  return KS_SUCCESS;
}

// EPSComputeVectors_Hermitian epsdefault.c:27-49 for a GHEP: the basis already holds the Ritz vectors
static int epilogue_hermitian(ks_eps eps)
{
  ks_bv V = eps->V; ks_st st = eps->st;
  if (eps->ghep && eps->purify) {
    // purification x <- OP x (EPS_Purify epsimpl.h:297-312), then B-normalise
    for (int i = 0; i < eps->nconv; i++) {
      KS_CALL(ksk_copy(eps->ctx, ks_bv_col(V, i), ks_bv_col(eps->W, 0), V->n));
      KS_CALL(ks_mat_mult_internal(eps->op, ks_bv_col(eps->W, 0), ks_bv_col(V, i)));
    }
    KS_CALL(ks_bv_normalize(V, nullptr));
  } else if (eps->ghep && st && st->type == KS_ST_CAYLEY) {
    // without purification the Lanczos vectors are the eigenvectors; under the Cayley transformation they are orthonormal in
    // the A + nu B inner product and still have to be B-normalised (epsdefault.c:38-47)
    KS_CALL(ks_bv_set_matrix(V, eps->B));
    int rc = ks_bv_normalize(V, nullptr);
    KS_CALL(ks_bv_set_matrix(V, st->bil));
    if (rc) return rc;
  }
  return KS_SUCCESS;
}

// The eigenvectors of the general variant are formed on first use (ks_eps_schur_vectors); V(:,0:nconv) stays the Schur basis until then.
// Conjugate pairs come with the positive imaginary part first (epssolve.c:160-175): the inversion of sinvert flips the sign
static int epilogue_schur(ks_eps eps)
{
  eps->vectors_done = false;
  for (int i = 0; i < eps->nconv - 1; i++) {
    if (eps->eigi[i] != 0.0) {
      if (eps->eigi[i] < 0.0) {                                 // "the next correction only works with eigenvectors" (epssolve.c:166-169)
        eps->eigi[i] = -eps->eigi[i]; eps->eigi[i + 1] = -eps->eigi[i + 1];
        KS_CALL(ks_eps_schur_vectors(eps));
        KS_CALL(ks_bv_scalecolumn(eps->V, i + 1, -1.0));
      }
      i++;
    }
  }
  return KS_SUCCESS;
}

// ---- EPSSetUp_KrylovSchur with the parts of EPSSetUp (epssetup.c:286-420) whose rules are this solver's: problem type, ST, sort criteria,
// dimensions, then the common part, balancing and the projected problem ----
static int resolve_problem_type(ks_eps eps, int *out)
{
  KS_CHECK(eps->A, KS_ERR_ORDER, "EPSSetOperators must be called first");
  KS_CHECK(eps->which.which != KS_EPS_WHICH_USER || eps->which.fn, KS_ERR_ORDER, "Must call EPSSetEigenvalueComparison() first");   // epssetup.c:311
  int ptype = eps->problem_type;
  if (!ptype) ptype = eps->B ? KS_EPS_GNHEP : KS_EPS_NHEP;             // default problem type (epssetup.c:318-322)
  if (!eps->B && ptype == KS_EPS_GNHEP) ptype = KS_EPS_NHEP;          // "reverting to a standard eigenproblem" (epssetup.c:324-327)
  if (!eps->B && ptype == KS_EPS_GHEP) ptype = KS_EPS_HEP;
  KS_CHECK(!eps->B || ptype == KS_EPS_GNHEP || ptype == KS_EPS_GHEP, KS_ERR_ARG_INCOMP, "Inconsistent EPS state: the problem type does not match the number of matrices");
  *out = ptype;
  return KS_SUCCESS;
}
static int setup_resolved(ks_eps eps, int ptype)
{
  ks_mat A = eps->A;
  const int n = A->n_global;
  const bool ghep = ptype == KS_EPS_GHEP, symmetric = ptype == KS_EPS_HEP || ghep;
  if (eps->conv == KS_EPS_CONV_NORM) KS_CALL(ks_eps_matrix_norms(eps));
  ks_st st = eps->st;
  KS_CHECK(!st || st->type != KS_ST_PRECOND, KS_ERR_SUP, "STPRECOND only preconditions: a Krylov solver needs a transformation that can be applied (EPSCheckSinvertCayley and friends)");
  const bool cayley = st && st->type == KS_ST_CAYLEY;
  const bool sinvert = (st && st->type == KS_ST_SINVERT) || cayley;   // the set-up rules below are those of EPSCheckSinvertCayley
  if (sinvert && !st->sigma_set) { if (st->sigma != eps->which.target) st->ready = false; st->sigma = eps->which.target; }   // the shift of sinvert defaults to the target (STSetDefaultShift epsbasic.c:386, sinvert.c:64); STSHIFT keeps 0
  KsCompare cmp = eps->which;
  if (!cmp.which) cmp.which = sinvert ? KS_EPS_TARGET_MAGNITUDE : KS_EPS_LARGEST_MAGNITUDE;   // epsdefault.c:209-219
  KS_CHECK(!sinvert || cmp.which == KS_EPS_TARGET_MAGNITUDE || cmp.which == KS_EPS_TARGET_REAL || cmp.which == KS_EPS_WHICH_USER, KS_ERR_USER_INPUT,
           "Shift-and-invert requires a target 'which' (see EPSSetWhichEigenpairs), for instance -st_type sinvert -eps_target 0 -eps_target_magnitude");   // epssetup.c:117-120
  eps->cmp_final = cmp;                                              // EPSSetUpSort_Basic: eps->sc, no map
  eps->cmp_ds = cmp;                                                 // EPSSetUpSort_Default: DS sc with map = SlepcMap_ST
  if (eps->B || !ks_st_is_plain(st)) {
    if (!st) { KS_CALL(ks_eps_get_st(eps, &st)); }
    KS_CALL(ks_st_set_matrices(st, A, eps->B)); st->ready = false;
    KS_CALL(ks_st_setup_internal(st));
    eps->op = st->op; eps->cmp_ds.map = ksd::StMap{st->type, st->sigma, st->nu};   // after the set-up, which resolves nu
  } else eps->op = A;
  int nev = eps->nev, ncv = eps->ncv_user, mpd = eps->mpd_user;
  if (ncv) { KS_CHECK(ncv >= nev + 1 || (ncv == nev && ncv == n), KS_ERR_USER_INPUT, "The value of ncv must be at least nev+1"); }
  else if (mpd) ncv = std::min(n, nev + mpd);
  else { if (nev < 500) ncv = std::min(n, std::max(2 * nev, nev + 15)); else { mpd = 500; ncv = std::min(n, nev + mpd); } }
  if (!mpd) mpd = ncv;
  KS_CHECK(ncv <= nev + mpd, KS_ERR_USER_INPUT, "The value of ncv must not be larger than nev+mpd");
  // ncv + 1 > 64 columns: the basis is wider than the register-tiled fused kernels; Gram-Schmidt then runs its slot program over
  // 64-column chunks (ks_gs.hip, still enqueued as a whole) and the panel products are blocked (ks_bv.hip)
  eps->mpd = mpd;
  // EPS_SetInnerProduct epsimpl.h:280-292: STGetBilinearForm = B, or A + nu B for STCAYLEY (cayley.c:70-77)
  KS_CALL(eps_setup_common(eps, ncv, ghep ? (cayley ? st->bil : eps->B) : nullptr));
  eps->ghep = ghep; eps->left_trivial = symmetric;
  eps->problem_type_resolved_hermitian = symmetric && eps->extraction != KS_EPS_HARMONIC;   // else variant EPS_KS_DEFAULT on the general DS (krylovschur.c:133-151)
  if (!symmetric && eps->balance != KS_EPS_BALANCE_NONE) KS_CALL(ks_eps_setup_balance(eps));   // balancing of non-symmetric problems (epssetup.c:383-391)
  KS_CHECK(eps->extraction == KS_EPS_RITZ || !ghep, KS_ERR_SUP, "harmonic extraction with a B-inner product is not built");
  KS_CHECK(!eps->arb_fn || (symmetric && eps->extraction == KS_EPS_RITZ), KS_ERR_SUP, "arbitrary selection is built for the symmetric (Lanczos) variant only");
  return KS_SUCCESS;
}
static void allocate_ds(ks_eps eps, ksd::Ds &ds) { ds.allocate(eps->ncv + 1); ds.which = eps->cmp_ds; ds.state = ksd::DS_RAW; }   // DSAllocate (krylovschur.c:153-168)
// the projected problem of a one-sided solve: the symmetric or the general variant, as the set-up resolved it
static ksd::Ds &onesided_ds(ks_eps eps) { return eps->problem_type_resolved_hermitian ? static_cast<ksd::Ds &>(eps->dsh) : eps->dsn; }

static int setup_onesided(ks_eps eps)
{
  int ptype = 0;
  KS_CALL(resolve_problem_type(eps, &ptype));
  KS_CALL(setup_resolved(eps, ptype));
  allocate_ds(eps, onesided_ds(eps));
  return KS_SUCCESS;
}
static int solve_onesided(ks_eps eps) { return restart_loop(eps, onesided_ds(eps)); }
static int compute_vectors_onesided(ks_eps eps) { return eps->problem_type_resolved_hermitian ? epilogue_hermitian(eps) : epilogue_schur(eps); }

// what the two-sided variant is built for: each case is listed in ksgpu.h
static int setup_twosided(ks_eps eps)
{
  int ptype = 0;
  KS_CALL(resolve_problem_type(eps, &ptype));
  ks_mat A = eps->A;
  KS_CHECK(ptype != KS_EPS_HEP && ptype != KS_EPS_GHEP, KS_ERR_SUP, "Two-sided methods are not intended for Hermitian problems");   // epssetup.c:309
  const bool tsolves = eps->st && eps->st->tsolves;                  // the ST prepares solves with the transposed matrix (ks_st_set_transpose_solves)
  KS_CHECK(!eps->B || tsolves, KS_ERR_SUP, "two-sided Krylov-Schur is built for standard problems (no B matrix) unless the ST has transposed solves (ks_st_set_transpose_solves)");
  KS_CHECK(!eps->st || eps->st->type == KS_ST_SHIFT || tsolves, KS_ERR_SUP, "two-sided Krylov-Schur is built for STSHIFT (the others need solves with the transposed matrix: ks_st_set_transpose_solves)");
  KS_CHECK(eps->balance == KS_EPS_BALANCE_NONE, KS_ERR_SUP, "two-sided Krylov-Schur with balancing is not built");
  KS_CHECK(eps->extraction == KS_EPS_RITZ, KS_ERR_SUP, "two-sided Krylov-Schur with harmonic extraction is not built");
  KS_CHECK(!eps->trueres, KS_ERR_SUP, "two-sided Krylov-Schur with the true residual is not built");
  KS_CHECK(!eps->nds, KS_ERR_SUP, "two-sided Krylov-Schur with a deflation space is not built");
  // more than one rank: the operator needs a transposed product across ranks - a matrix created with KS_MAT_SHARDED_TRANSPOSE, alone or under the
  // ST's shift operator (STSHIFT, one matrix). Transposed ST solves across ranks are not built (ks_st.hip), so sinvert, Cayley and B stay refused.
  // Decided from what every rank knows alike, before any collective of the set-up.
  KS_CHECK(eps->ctx->comm.size == 1 || (ks_mat_has_transpose_across_ranks(A) && !eps->B && (!eps->st || eps->st->type == KS_ST_SHIFT)), KS_ERR_SUP,
           "two-sided Krylov-Schur on more than one rank needs an operator with a transposed product across ranks: a matrix created with KS_MAT_SHARDED_TRANSPOSE, under STSHIFT and without B (the transpose of a row-sharded matrix is a redistribution otherwise)");
  KS_CALL(setup_resolved(eps, ptype));
  // the left basis (EPSAllocateSolution: BVDuplicate, epssetup.c:733) and Op^T as a matrix (MatCreateHermitianTranspose of STGetOperator, ks-twosided.c:141-142)
  const int ncv = eps->ncv;
  if (eps->VL) { int vm = 0; ks_bv_get_sizes(eps->VL, nullptr, nullptr, &vm, nullptr); if (vm != ncv + 1) { ks_bv_destroy(eps->VL); eps->VL = nullptr; } }
  if (!eps->VL) { KS_CALL(ks_bv_duplicate(eps->V, &eps->VL)); eps->VL->row_start = A->row_start; }
  KS_CALL(ks_bv_set_active_columns(eps->VL, 0, ncv + 1));
  if (eps->opT_owned) ks_mat_destroy(eps->opT);
  eps->opT = nullptr; eps->opT_owned = false;
  KS_CALL(ks_mat_create_transpose(eps->op, &eps->opT));
  eps->opT_owned = eps->op->shell_mult != nullptr;
  // one transposed product now, so that an operator without one fails here and not inside the first restart
  KS_HIP(hipMemsetAsync(ks_bv_col(eps->W, 3), 0, sizeof(double) * std::max(A->n, 1), eps->ctx->stream));
  KS_CALL(ks_mat_mult_internal(eps->opT, ks_bv_col(eps->W, 3), ks_bv_col(eps->W, 4)));
  ks_bv_gs_passes(eps->VL, &eps->passes0[1], nullptr);
  allocate_ds(eps, eps->dst);
  return KS_SUCCESS;
}

const ks_eps_ops *ks_krylovschur_ops(bool twosided)
{
  static const ks_eps_ops onesided = {setup_onesided, solve_onesided, compute_vectors_onesided};
  static const ks_eps_ops both = {setup_twosided, restart_loop_twosided, epilogue_schur};
  return twosided ? &both : &onesided;
}
