// Host side of the path, the part every eigensolver shares: the EPS object with its options and getters, the generic set-up, ks_eps_solve over the
// solver table (ks_eps_impl.h; the solvers are ks_krylovschur.hip, ks_lobpcg.hip and ks_gd.hip), the epilogue of a solve, the results and their errors.
//
// Restates, in plain C++ on host scalars:
//   EPSSetUp (generic part)         src/eps/interface/epssetup.c:286-420
//   EPSConvergedRelative / EPSStoppingBasic   src/eps/interface/epsdefault.c:224,290
//   EPSSolve + SlepcSortEigenvalues  src/eps/interface/epssolve.c:119-208, src/sys/slepcsc.c:89-140
//   EPSGetEigenpair / EPSGetLeftEigenvector   epssolve.c:405,567-613 (BV_GetEigenvector bvimpl.h:423-446)
//   EPSComputeError / EPSComputeResidualNorm_Private  epssolve.c:666-718,742-815
#include "ksgpu_internal.h"
#include "ks_eps_impl.h"
#include <algorithm>
#include <limits>


extern "C" int ks_eps_create(ks_ctx ctx, ks_eps *out)
{
  KS_CHECK(ctx && out, KS_ERR_ARG_NULL, "ctx/out is NULL");
  ks_eps eps = new ks_eps_s(); eps->ctx = ctx; *out = eps;
  return KS_SUCCESS;
}

extern "C" int ks_eps_destroy(ks_eps eps)
{
  if (!eps) return KS_SUCCESS;
  ks_bv_destroy(eps->V); ks_bv_destroy(eps->W); ks_bv_destroy(eps->defl); ks_bv_destroy(eps->VL); ks_bv_destroy(eps->ini);
  if (eps->opT_owned) ks_mat_destroy(eps->opT);
  ks_st_destroy(eps->st);
  if (eps->D) hipFree(eps->D); if (eps->wb) hipFree(eps->wb); if (eps->bal_op) ks_mat_destroy(eps->bal_op);
  delete eps;
  return KS_SUCCESS;
}

extern "C" int ks_eps_set_operators(ks_eps eps, ks_mat A, ks_mat B)   // epssetup.c:450
{
  KS_CHECK(eps && A, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(!B || (B->n == A->n && B->n_global == A->n_global), KS_ERR_ARG_INCOMP, "Mismatching dimensions of A (%d) and B (%d)", A->n, B ? B->n : 0);
  if (eps->A && eps->A->n != A->n) {                                   // EPSReset (epsbasic.c): everything sized by the old operator goes
    ks_bv_destroy(eps->V); ks_bv_destroy(eps->W); ks_bv_destroy(eps->VL); eps->V = eps->W = eps->VL = nullptr;
    eps->have_w0 = false; eps->w0.clear();
    ks_bv_destroy(eps->defl); eps->defl = nullptr; eps->nds = 0;
    eps->have_v0 = false; eps->v0.clear(); ks_bv_destroy(eps->ini); eps->ini = nullptr; eps->nini = 0;
    if (eps->D) { hipFree(eps->D); eps->D = nullptr; } if (eps->wb) { hipFree(eps->wb); eps->wb = nullptr; } eps->D_n = 0;
    if (eps->balance == KS_EPS_BALANCE_USER) eps->balance = KS_EPS_BALANCE_NONE;
  }
  eps->A = A; eps->B = B; eps->solved = false; eps->nrma = eps->nrmb = 0.0;
  if (eps->st) KS_CALL(ks_st_set_matrices(eps->st, A, B));
  return KS_SUCCESS;
}
extern "C" int ks_eps_get_st(ks_eps eps, ks_st *st)                     // EPSGetST epsbasic.c
{
  KS_CHECK(eps && st, KS_ERR_ARG_NULL, "NULL argument");
  if (!eps->st) { KS_CALL(ks_st_create(eps->ctx, &eps->st)); if (eps->A) KS_CALL(ks_st_set_matrices(eps->st, eps->A, eps->B)); }
  *st = eps->st; eps->solved = false;
  return KS_SUCCESS;
}
extern "C" int ks_eps_set_problem_type(ks_eps eps, int type)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(type == KS_EPS_HEP || type == KS_EPS_GHEP || type == KS_EPS_NHEP || type == KS_EPS_GNHEP, KS_ERR_SUP, "EPS_HEP and EPS_GHEP (Lanczos), EPS_NHEP and EPS_GNHEP (Arnoldi) are driven by this build; PGNHEP / GHIEP are not");
  eps->problem_type = type; eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_set_dimensions(ks_eps eps, int nev, int ncv, int mpd)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(nev >= 1, KS_ERR_ARG_OUTOFRANGE, "Illegal value of nev. Must be > 0");
  eps->nev = nev; eps->ncv_user = ncv > 0 ? ncv : 0; eps->mpd_user = mpd > 0 ? mpd : 0; eps->solved = false;
  return KS_SUCCESS;
}
extern "C" int ks_eps_set_tolerances(ks_eps eps, double tol, int max_it)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  eps->tol = tol > 0.0 ? tol : 1e-8;                 // SLEPC_DEFAULT_TOL epssetup.c:378, slepcmath.h:25
  eps->max_it_user = max_it > 0 ? max_it : 0;
  return KS_SUCCESS;
}
extern "C" int ks_eps_set_which_eigenpairs(ks_eps eps, int which)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  switch (which) {                                    // epsopts.c:478-510
    case KS_EPS_LARGEST_MAGNITUDE: case KS_EPS_SMALLEST_MAGNITUDE: case KS_EPS_LARGEST_REAL: case KS_EPS_SMALLEST_REAL:
    case KS_EPS_LARGEST_IMAGINARY: case KS_EPS_SMALLEST_IMAGINARY: case KS_EPS_TARGET_MAGNITUDE: case KS_EPS_TARGET_REAL:
    case KS_EPS_WHICH_USER: break;
    default: KS_FAIL(KS_ERR_ARG_OUTOFRANGE, "Invalid 'which' value");
  }
  eps->which.which = which; eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_set_target(ks_eps eps, double target)                     // EPSSetTarget epsopts.c:604
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  eps->which.target = target; eps->solved = false;
  if (eps->st && !eps->st->sigma_set) { eps->st->sigma = target; eps->st->ready = false; }   // STSetDefaultShift (epsbasic.c:386)
  return KS_SUCCESS;
}
extern "C" int ks_eps_set_eigenvalue_comparison(ks_eps eps, ks_eig_compare_fn fn, void *fctx)   // epsopts.c:563
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  eps->which.fn = fn; eps->which.fn_ctx = fctx; eps->which.which = KS_EPS_WHICH_USER; eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_set_krylovschur_restart(ks_eps eps, double keep)   // krylovschur.c:339-350
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(keep >= 0.1 && keep <= 0.9, KS_ERR_ARG_OUTOFRANGE, "The keep argument %g must be in the range [.1,.9]", keep);
  eps->keep = keep; return KS_SUCCESS;
}
extern "C" int ks_eps_set_convergence_test(ks_eps eps, int conv)            // EPSSetConvergenceTest epsopts.c
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(conv == KS_EPS_CONV_ABS || conv == KS_EPS_CONV_REL || conv == KS_EPS_CONV_NORM || conv == KS_EPS_CONV_USER, KS_ERR_ARG_OUTOFRANGE, "Invalid 'conv' value");
  KS_CHECK(conv != KS_EPS_CONV_USER || eps->conv_fn, KS_ERR_ORDER, "Must call EPSSetConvergenceTestFunction() first");
  eps->conv = conv; eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_set_true_residual(ks_eps eps, int trueres)            // EPSSetTrueResidual epsopts.c
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  eps->trueres = trueres != 0; eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_get_true_residual(ks_eps eps, int *trueres) { KS_CHECK(eps && trueres, KS_ERR_ARG_NULL, "NULL argument"); *trueres = eps->trueres ? 1 : 0; return KS_SUCCESS; }
extern "C" int ks_eps_set_purify(ks_eps eps, int purify)                    // EPSSetPurify epsopts.c (generalized symmetric problems)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  eps->purify = purify != 0; eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_get_purify(ks_eps eps, int *purify) { KS_CHECK(eps && purify, KS_ERR_ARG_NULL, "NULL argument"); *purify = eps->purify ? 1 : 0; return KS_SUCCESS; }
extern "C" int ks_eps_set_track_all(ks_eps eps, int trackall)                // EPSSetTrackAll epsopts.c: residual estimates of all Ritz pairs at every restart
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  eps->trackall = trackall != 0; return KS_SUCCESS;
}
extern "C" int ks_eps_get_krylovschur(ks_eps eps, double *keep, int *lock)   // EPSKrylovSchurGetRestart / GetLocking
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  if (keep) *keep = eps->keep; if (lock) *lock = eps->lock ? 1 : 0;
  return KS_SUCCESS;
}
extern "C" int ks_eps_set_balance(ks_eps eps, int bal, int its, double cutoff)   // EPSSetBalance epsopts.c:1050-1095 (its, cutoff: 0 keeps)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(bal >= KS_EPS_BALANCE_NONE && bal <= KS_EPS_BALANCE_USER, KS_ERR_ARG_OUTOFRANGE, "Invalid value of argument 'bal'");
  KS_CHECK(bal != KS_EPS_BALANCE_USER || eps->D, KS_ERR_ORDER, "EPS_BALANCE_USER: hand the diagonal over first (STSetBalanceMatrix: ks_eps_set_balance_matrix)");
  KS_CHECK(its >= 0, KS_ERR_ARG_OUTOFRANGE, "Illegal value of its. Must be >= 0");
  KS_CHECK(cutoff >= 0.0, KS_ERR_ARG_OUTOFRANGE, "Illegal value of cutoff. Must be >= 0");
  eps->balance = bal; if (its) eps->balance_its = its; if (cutoff > 0.0) eps->balance_cutoff = cutoff;
  eps->solved = false;
  return KS_SUCCESS;
}
// EPS_BALANCE_USER: the diagonal of the balancing matrix comes from the caller (STSetBalanceMatrix stfunc.c on the solver's ST);
// n_local positive doubles on the device, copied. Selects KS_EPS_BALANCE_USER.
extern "C" int ks_eps_set_balance_matrix(ks_eps eps, const double *D_dev)
{
  KS_CHECK(eps && eps->A && D_dev, KS_ERR_ORDER, "set the operators first; D must not be NULL");
  const long long n = eps->A->n;
  KS_HIP(hipSetDevice(eps->ctx->device));
  if (eps->D_n != n || !eps->D) { if (eps->D) hipFree(eps->D); if (eps->wb) hipFree(eps->wb); eps->D = eps->wb = nullptr;
    KS_HIP(hipMalloc(&eps->D, sizeof(double) * std::max<long long>(n, 1))); KS_HIP(hipMalloc(&eps->wb, sizeof(double) * std::max<long long>(n, 1))); eps->D_n = (int)n; }
  KS_HIP(hipMemcpyAsync(eps->D, D_dev, sizeof(double) * n, hipMemcpyDeviceToDevice, eps->ctx->stream));
  KS_HIP(ks_sync(eps->ctx));
  eps->balance = KS_EPS_BALANCE_USER; eps->solved = false;
  return KS_SUCCESS;
}
extern "C" int ks_eps_get_balance(ks_eps eps, int *bal, int *its, double *cutoff)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  if (bal) *bal = eps->balance; if (its) *its = eps->balance_its; if (cutoff) *cutoff = eps->balance_cutoff;
  return KS_SUCCESS;
}
extern "C" int ks_eps_set_extraction(ks_eps eps, int extr)                  // EPSSetExtraction epsopts.c:968-994; krylovschur.c:120 accepts these two
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(extr >= KS_EPS_RITZ && extr <= KS_EPS_REFINED_HARMONIC, KS_ERR_ARG_OUTOFRANGE, "Invalid extraction type");
  KS_CHECK(extr == KS_EPS_RITZ || extr == KS_EPS_HARMONIC, KS_ERR_SUP, "Unsupported extraction type");
  eps->extraction = extr; eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_get_extraction(ks_eps eps, int *extr) { KS_CHECK(eps && extr, KS_ERR_ARG_NULL, "NULL argument"); *extr = eps->extraction; return KS_SUCCESS; }
int ks_eps_matrix_norms(ks_eps eps)                                         // epssetup.c:345-358
{
  if (!eps->nrma) KS_CALL(ks_mat_norm_inf(eps->A, &eps->nrma));
  if (eps->B) { if (!eps->nrmb) KS_CALL(ks_mat_norm_inf(eps->B, &eps->nrmb)); } else eps->nrmb = 1.0;
  return KS_SUCCESS;
}
extern "C" int ks_eps_set_krylovschur_locking(ks_eps eps, int lock)     // EPSKrylovSchurSetLocking krylovschur.c:388-423
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  eps->lock = lock != 0; eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_set_random_seed(ks_eps eps, uint64_t seed) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); eps->seed = seed; return KS_SUCCESS; }
extern "C" int ks_eps_set_initial_vector(ks_eps eps, const double *v)
{
  KS_CHECK(eps && eps->A, KS_ERR_ORDER, "set the operators first");
  if (!v) { eps->have_v0 = false; return KS_SUCCESS; }
  eps->v0.assign(v, v + eps->A->n); eps->have_v0 = true;
  return KS_SUCCESS;
}
// EPSSetDeflationSpace epssetup.c:555-570: the vectors are copied now and become constraints of the basis at the next
// solve (BVInsertConstraints, epssetup.c:397-404), which also forgets them (epssolve.c:201-205): "the deflation space
// should be set every time". They need not be orthonormal; dependent ones are dropped.
extern "C" int ks_eps_set_deflation_space(ks_eps eps, int n, const double *const *v_dev)
{
  KS_CHECK(eps && eps->A, KS_ERR_ORDER, "set the operators first");
  KS_CHECK(n >= 0, KS_ERR_ARG_OUTOFRANGE, "Argument n cannot be negative");
  ks_bv_destroy(eps->defl); eps->defl = nullptr; eps->nds = 0;
  if (!n) return KS_SUCCESS;
  KS_CHECK(v_dev, KS_ERR_ARG_NULL, "NULL argument");
  KS_CALL(ks_bv_create(eps->ctx, eps->A->n, eps->A->n_global, n, 0, &eps->defl));
  for (int i = 0; i < n; i++) { KS_CHECK(v_dev[i], KS_ERR_ARG_NULL, "vector %d is NULL", i); KS_CALL(ks_bv_insert_vec(eps->defl, i, v_dev[i])); }
  eps->nds = n; eps->solved = false;
  return KS_SUCCESS;
}
// EPSSetInitialSpace epssetup.c:590-610 with device vectors. A Krylov solver starts from ONE vector: the first of the
// space (EPSGetStartVector epssolve.c:853 uses column 0 of the inserted, orthonormalised set), the others are not used.
extern "C" int ks_eps_set_initial_space(ks_eps eps, int n, const double *const *v_dev)
{
  KS_CHECK(eps && eps->A, KS_ERR_ORDER, "set the operators first");
  KS_CHECK(n >= 0, KS_ERR_ARG_OUTOFRANGE, "Argument n cannot be negative");
  ks_bv_destroy(eps->ini); eps->ini = nullptr; eps->nini = 0;
  if (!n) { eps->have_v0 = false; return KS_SUCCESS; }
  KS_CHECK(v_dev && v_dev[0], KS_ERR_ARG_NULL, "NULL argument");
  eps->v0.resize(std::max(eps->A->n, 1));
  KS_HIP(hipSetDevice(eps->ctx->device));
  if (eps->type == KS_EPS_LOBPCG || eps->type == KS_EPS_GD || eps->type == KS_EPS_JD) {   // a block solver uses all of them (lobpcg.c:133, dvdinitv.c:45): device copies, made only for those solver types
    KS_CALL(ks_bv_create(eps->ctx, eps->A->n, eps->A->n_global, n, 0, &eps->ini));
    for (int i = 0; i < n; i++) { KS_CHECK(v_dev[i], KS_ERR_ARG_NULL, "vector %d is NULL", i); KS_CALL(ks_bv_insert_vec(eps->ini, i, v_dev[i])); }
    eps->nini = n;
  }
  KS_HIP(hipMemcpyAsync(eps->v0.data(), v_dev[0], sizeof(double) * eps->A->n, hipMemcpyDeviceToHost, eps->ctx->stream));
  KS_HIP(ks_sync(eps->ctx));
  eps->have_v0 = true; eps->solved = false;
  return KS_SUCCESS;
}
// EPSSetTwoSided epsopts.c: also compute left eigenvectors (two-sided Krylov-Schur, non-symmetric problems)
extern "C" int ks_eps_set_two_sided(ks_eps eps, int twosided)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  eps->twosided = twosided != 0; eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_get_two_sided(ks_eps eps, int *twosided) { KS_CHECK(eps && twosided, KS_ERR_ARG_NULL, "NULL argument"); *twosided = eps->twosided ? 1 : 0; return KS_SUCCESS; }
extern "C" int ks_eps_get_two_sided_stats(ks_eps eps, long long *ds_permutations)
{
  KS_CHECK(eps && ds_permutations, KS_ERR_ARG_NULL, "NULL argument");
  *ds_permutations = eps->twosided_solved ? eps->dst.permuted : 0; return KS_SUCCESS;
}
// EPSSetLeftInitialSpace epssetup.c with device vectors: as for the right one, the first vector starts the left recurrence
extern "C" int ks_eps_set_left_initial_space(ks_eps eps, int n, const double *const *w_dev)
{
  KS_CHECK(eps && eps->A, KS_ERR_ORDER, "set the operators first");
  KS_CHECK(n >= 0, KS_ERR_ARG_OUTOFRANGE, "Argument n cannot be negative");
  if (!n) { eps->have_w0 = false; return KS_SUCCESS; }
  KS_CHECK(w_dev && w_dev[0], KS_ERR_ARG_NULL, "NULL argument");
  eps->w0.resize(std::max(eps->A->n, 1));
  KS_HIP(hipSetDevice(eps->ctx->device));
  KS_HIP(hipMemcpyAsync(eps->w0.data(), w_dev[0], sizeof(double) * eps->A->n, hipMemcpyDeviceToHost, eps->ctx->stream));
  KS_HIP(ks_sync(eps->ctx));
  eps->have_w0 = true; eps->solved = false;
  return KS_SUCCESS;
}
extern "C" int ks_eps_set_ds_parallel(ks_eps eps, int pmode)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(pmode == KS_DS_PARALLEL_REDUNDANT || pmode == KS_DS_PARALLEL_SYNCHRONIZED, KS_ERR_ARG_OUTOFRANGE, "unknown DS parallel mode %d", pmode);
  eps->ds_parallel = pmode;
  return KS_SUCCESS;
}
extern "C" int ks_eps_get_ds_parallel(ks_eps eps, int *pmode) { KS_CHECK(eps && pmode, KS_ERR_ARG_NULL, "NULL argument"); *pmode = eps->ds_parallel; return KS_SUCCESS; }

// Values a solver computes with allreduces and then feeds into host arithmetic every rank must repeat bit for bit (Gram matrices, coefficients
// that go through a factorisation, residual norms): rank 0's to every rank under KS_DS_PARALLEL_SYNCHRONIZED, as DSSynchronize does for the DS
int ks_eps_synchronize_values(ks_eps eps, double *v, size_t count)
{
  if (!ks_is_multi(eps->ctx) || eps->ds_parallel != KS_DS_PARALLEL_SYNCHRONIZED) return KS_SUCCESS;
  return ks_comm_bcast0_host(eps->ctx, v, (int)(count * sizeof(double)));
}

extern "C" int ks_eps_set_max_steps(ks_eps eps, long long s) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); eps->max_steps = s > 0 ? s : 0; return KS_SUCCESS; }

// EPSStoppingBasic epsdefault.c:290-307; user functions may call it first, as ex29.c does
extern "C" int ks_eps_stopping_basic(ks_eps eps, int its, int max_it, int nconv, int nev, int *reason, void *ctx)
{
  (void)eps; (void)ctx;
  KS_CHECK(reason, KS_ERR_ARG_NULL, "NULL argument");
  *reason = KS_EPS_CONVERGED_ITERATING;
  if (nconv >= nev) *reason = KS_EPS_CONVERGED_TOL;
  else if (its >= max_it) *reason = KS_EPS_DIVERGED_ITS;
  return KS_SUCCESS;
}
extern "C" int ks_eps_set_stopping_test_function(ks_eps eps, ks_eps_stopping_fn fn, void *ctx)   // EPSSetStoppingTestFunction epsopts.c
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  eps->stop_fn = fn; eps->stop_ctx = ctx; return KS_SUCCESS;
}
extern "C" int ks_eps_set_convergence_test_function(ks_eps eps, ks_eps_converged_fn fn, void *ctx)   // EPSSetConvergenceTestFunction epsopts.c
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  if (fn) { eps->conv_fn = fn; eps->conv_ctx = ctx; eps->conv = KS_EPS_CONV_USER; }
  else { eps->conv_fn = nullptr; eps->conv_ctx = nullptr; if (eps->conv == KS_EPS_CONV_USER) eps->conv = KS_EPS_CONV_REL; }
  eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_set_arbitrary_selection(ks_eps eps, ks_eps_arbitrary_fn fn, void *ctx)      // EPSSetArbitrarySelection epsopts.c:600-615
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  eps->arb_fn = fn; eps->arb_ctx = ctx; eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_monitor_set(ks_eps eps, ks_eps_monitor_fn fn, void *ctx)                   // EPSMonitorSet epsmon.c (one slot); NULL = EPSMonitorCancel
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  eps->mon_fn = fn; eps->mon_ctx = ctx; return KS_SUCCESS;
}
// the stopping test after iteration `its`: the user's function or the basic one, into eps->reason
int ks_eps_stopping_call(ks_eps eps, int its, int nconv)
{
  int reason = KS_EPS_CONVERGED_ITERATING;
  if (eps->stop_fn) { const int rc = eps->stop_fn(eps, its, eps->max_it, nconv, eps->nev, &reason, eps->stop_ctx); KS_CHECK(!rc, rc, "the user's stopping test returned %d", rc); }
  else ks_eps_stopping_basic(eps, its, eps->max_it, nconv, eps->nev, &reason, nullptr);
  eps->reason = reason;
  return KS_SUCCESS;
}
int ks_eps_monitor_call(ks_eps eps, int its, int nconv, int nest)                               // EPSMonitor epsmon.c:21-33
{
  if (!eps->mon_fn) return KS_SUCCESS;
  const int rc = eps->mon_fn(eps, its, nconv, eps->eigr.data(), eps->eigi.data(), eps->errest.data(), nest, eps->mon_ctx);
  KS_CHECK(!rc, rc, "the user's monitor returned %d", rc);
  return KS_SUCCESS;
}

// EPSConvergedRelative / Absolute / Norm epsdefault.c:224-257
double ks_eps_converged_estimate(ks_eps eps, double re, double im, double res)
{
  const double w = hypot(re, im);
  switch (eps->conv) {
    case KS_EPS_CONV_USER: { double e = 0.0; const int rc = eps->conv_fn(eps, re, im, res, &e, eps->conv_ctx); if (rc && !eps->cb_err) eps->cb_err = rc; return e; }
    case KS_EPS_CONV_ABS:  return res;
    case KS_EPS_CONV_NORM: return res / (eps->nrma + w * eps->nrmb);
    default:               return (w != 0.0) ? res / w : std::numeric_limits<double>::max();
  }
}

// EPSComputeResidualNorm_Private epssolve.c:666-718 (STGetMatrix 0/1 = the user's A and B): || A x - k B x ||_2 for a
// real eigenvalue, hypot of the two real-arithmetic residuals for a pair (xi_sign * xi is the imaginary part).
// Work vectors: W columns 0..2.
// trans (the left residual of the two-sided variant): the transposed products and the conjugate eigenvalue, ||A^T y - conj(k) B^T y|| (:676,692,705,711)
int ks_eps_residual_norm(ks_eps eps, double kr, double ki, const double *xr, const double *xi, double xi_sign, double *out, bool trans)
{
  ks_bv W = eps->W; ks_ctx ctx = eps->ctx; ks_mat A = eps->A, B = eps->B;
  const long long n = W->n;
  double *u = ks_bv_col(W, 0);
  double nrm = 0.0;
  auto mult = [&](const double *x, double *y) { return trans ? ks_mat_mult_transpose_internal(A, x, y) : ks_mat_mult_internal(A, x, y); };
  auto multb = [&](const double *x, double *y) { return trans ? ks_mat_mult_transpose_internal(B, x, y) : ks_mat_mult_internal(B, x, y); };   // two matrices: || A^T y - conj(k) B^T y ||
  if (trans) ki = -ki;
  if (ki == 0.0 || fabs(ki) < fabs(kr * std::numeric_limits<double>::epsilon())) {
    KS_CALL(mult(xr, u));                                                            // u = A*x
    if (fabs(kr) > std::numeric_limits<double>::epsilon()) {
      const double *w = xr;
      if (B) { KS_CALL(multb(xr, ks_bv_col(W, 2))); w = ks_bv_col(W, 2); }   // w = B*x
      KS_CALL(ksk_lincomb(ctx, n, nullptr, 1.0, u, -kr, w, u));                      // u = A*x - k*B*x
    }
    KS_CALL(ks_bv_normcolumn(W, 0, KS_NORM_2, &nrm));
  } else {
    const double sg = xi_sign;
    const double *v = xr, *w = xi;                                                   // v = B*xr, w = B*xi (before the sign)
    if (B) { KS_CALL(multb(xr, ks_bv_col(W, 1))); KS_CALL(multb(xi, ks_bv_col(W, 2))); v = ks_bv_col(W, 1); w = ks_bv_col(W, 2); }
    double nr = 0.0, ni = 0.0;
    KS_CALL(mult(xr, u));                                                            // u = A*xr - kr*B*xr + ki*B*xi
    KS_CALL(ksk_lincomb(ctx, n, nullptr, 1.0, u, -kr, v, u));
    KS_CALL(ksk_lincomb(ctx, n, nullptr, 1.0, u, ki * sg, w, u));
    KS_CALL(ks_bv_normcolumn(W, 0, KS_NORM_2, &nr));
    KS_CALL(mult(xi, u));                                                            // u = A*xi - kr*B*xi - ki*B*xr
    KS_CALL(ksk_lincomb(ctx, n, nullptr, sg, u, -kr * sg, w, u));
    KS_CALL(ksk_lincomb(ctx, n, nullptr, 1.0, u, -ki, v, u));
    KS_CALL(ks_bv_normcolumn(W, 0, KS_NORM_2, &ni));
    nrm = hypot(nr, ni);
  }
  *out = nrm;
  return KS_SUCCESS;
}

// The generic part of EPSSetUp (epssetup.c:286-420) and of EPSReset's results, for every solver once its own rules have fixed ncv and the inner
// product: EPSAllocateSolution, the results of the last solve forgotten - every array, counter and flag here and nowhere else -, EPS_SetInnerProduct,
// the deflation space. A solver sets what it resolved (ghep, the variant, left_trivial, balanced) after this returns.
int eps_setup_common(ks_eps eps, int ncv, ks_mat ip)
{
  ks_mat A = eps->A;
  eps->ncv = ncv;
  eps->max_it = eps->max_it_user ? eps->max_it_user : std::max(100, 2 * A->n_global / ncv);
  if (eps->V) { int vm = 0; ks_bv_get_sizes(eps->V, nullptr, nullptr, &vm, nullptr); if (vm != ncv + 1 || eps->V->nc) { ks_bv_destroy(eps->V); eps->V = nullptr; } }
  if (!eps->V) { KS_CALL(ks_bv_create(eps->ctx, A->n, A->n_global, ncv + 1, 0, &eps->V)); eps->V->row_start = A->row_start; }   // EPSAllocateSolution(eps,1)
  if (!eps->W) { KS_CALL(ks_bv_create(eps->ctx, A->n, A->n_global, 5, 0, &eps->W)); }     // work vectors: u, B*xr, B*xi, Ritz vector x, y
  eps->eigr.assign(ncv + 1, 0.0); eps->eigi.assign(ncv + 1, 0.0); eps->errest.assign(ncv + 1, 0.0);
  eps->perm.resize(ncv + 1); for (int i = 0; i <= ncv; i++) eps->perm[i] = i;
  eps->cb_err = 0;
  eps->nconv = 0; eps->its = 0; eps->reason = KS_EPS_CONVERGED_ITERATING; eps->solved = false;
  eps->steps = 0; eps->passes = 0; eps->restarts = 0;
  eps->lob.iterations = eps->lob.hard_locks = eps->lob.mat_columns = eps->lob.pc_columns = 0;
  eps->gd.iterations = eps->gd.restarts = eps->gd.locks = eps->gd.mat_columns = eps->gd.pc_columns = eps->gd.fused_residuals = 0;
  eps->dst.permuted = 0;
  eps->ghep = false; eps->problem_type_resolved_hermitian = false; eps->left_trivial = false; eps->twosided_solved = false; eps->balanced = false;
  eps->vectors_done = true;
  ks_bv V = eps->V;
  ks_bv_gs_passes(V, &eps->passes0[0], nullptr);
  KS_CALL(ks_bv_set_active_columns(V, 0, ncv + 1));
  KS_CALL(ks_bv_set_matrix(V, ip));
  if (eps->nds) {                                                      // process the deflation space (epssetup.c:397-404)
    KS_CHECK(eps->defl && eps->defl->n == A->n, KS_ERR_ARG_INCOMP, "the deflation space was set for an operator of another size");
    std::vector<const double *> cp(eps->nds);
    for (int i = 0; i < eps->nds; i++) cp[i] = ks_bv_col(eps->defl, i);
    int kd = eps->nds;
    int rc = ks_bv_insert_constraints(V, &kd, cp.data());
    ks_bv_destroy(eps->defl); eps->defl = nullptr; eps->nds = 0;
    if (rc) return rc;
  }
  return KS_SUCCESS;
}

// SlepcSortEigenvalues slepcsc.c:89-140 into eps->perm, keeping conjugate pairs together
static void sort_eigenvalues(ks_eps eps)
{
  std::vector<int> &perm = eps->perm;
  const double *eigr = eps->eigr.data(), *eigi = eps->eigi.data();
  const int nc = eps->nconv;
  for (int i = 0; i <= eps->ncv; i++) perm[i] = i;
  for (int i = nc - 1; i >= 0; i--) {
    const double re = eigr[perm[i]]; double im = eigi[perm[i]];
    int j = i + 1;
    if (im != 0.0) { i--; im = eigi[perm[i]]; }                // complex eigenvalue: positive imaginary part first
    while (j < nc) {
      if (ksd::compare_eig(eps->cmp_final, re, im, eigr[perm[j]], eigi[perm[j]]) <= 0) break;
      if (im == 0.0) {
        if (eigi[perm[j]] == 0.0) { std::swap(perm[j - 1], perm[j]); j++; }
        else { const int tmp = perm[j - 1]; perm[j - 1] = perm[j]; perm[j] = perm[j + 1]; perm[j + 1] = tmp; j += 2; }
      } else {
        if (eigi[perm[j]] == 0.0) { const int tmp = perm[j - 2]; perm[j - 2] = perm[j]; perm[j] = perm[j - 1]; perm[j - 1] = tmp; j++; }
        else { std::swap(perm[j - 2], perm[j]); std::swap(perm[j - 1], perm[j + 1]); j += 2; }
      }
    }
  }
}

extern "C" int ks_eps_solve(ks_eps eps)   // EPSSolve epssolve.c:119-208
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  const ks_eps_ops &ops = eps->type == KS_EPS_LOBPCG ? *ks_lobpcg_ops() : eps->type == KS_EPS_GD ? *ks_gd_ops() : eps->type == KS_EPS_JD ? *ks_jd_ops() : *ks_krylovschur_ops(eps->twosided);
  KS_CALL(ops.setup(eps));                                             // takes the pass counters (eps->passes0) and allocates the solver's DS
  KS_CALL(ops.solve(eps));
  // ---- EPSSolve epilogue ----
  const bool left = eps->twosided_solved;                              // the solve filled a left basis
  KS_CALL(ks_bv_set_active_columns(eps->V, 0, eps->nconv));
  if (left) KS_CALL(ks_bv_set_active_columns(eps->VL, 0, eps->nconv));
  eps->cmp_ds.map.backtransform(eps->nconv, eps->eigr.data(), eps->eigi.data());   // EPSComputeValues (epssolve.c:27-41): map the eigenvalues back through the ST (LOBPCG: no map)
  if (ops.compute_vectors) KS_CALL(ops.compute_vectors(eps));
  sort_eigenvalues(eps);
  long long passes1 = 0;
  ks_bv_gs_passes(eps->V, &passes1, nullptr); eps->passes = passes1 - eps->passes0[0];
  if (left) { ks_bv_gs_passes(eps->VL, &passes1, nullptr); eps->passes += passes1 - eps->passes0[1]; }
  KS_CALL(ks_bv_set_num_constraints(eps->V, 0));                       // remove the deflation space (epssolve.c:201-205)
  eps->solved = true;
  return KS_SUCCESS;
}

extern "C" int ks_eps_get_converged(ks_eps eps, int *nconv) { KS_CHECK(eps && nconv, KS_ERR_ARG_NULL, "NULL argument"); KS_CHECK(eps->solved, KS_ERR_ARG_WRONGSTATE, "Must call EPSSolve() first"); *nconv = eps->nconv; return KS_SUCCESS; }
extern "C" int ks_eps_get_iteration_number(ks_eps eps, int *its) { KS_CHECK(eps && its, KS_ERR_ARG_NULL, "NULL argument"); *its = eps->its; return KS_SUCCESS; }
extern "C" int ks_eps_get_converged_reason(ks_eps eps, int *reason) { KS_CHECK(eps && reason, KS_ERR_ARG_NULL, "NULL argument"); KS_CHECK(eps->solved, KS_ERR_ARG_WRONGSTATE, "Must call EPSSolve() first"); *reason = eps->reason; return KS_SUCCESS; }
extern "C" int ks_eps_get_dimensions(ks_eps eps, int *nev, int *ncv, int *mpd)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  if (nev) *nev = eps->nev; if (ncv) *ncv = eps->ncv; if (mpd) *mpd = eps->mpd;
  return KS_SUCCESS;
}
extern "C" int ks_eps_get_eigenvalue(ks_eps eps, int i, double *eigr, double *eigi)   // EPSGetEigenvalue epssolve.c:478: through perm
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(eps->solved, KS_ERR_ARG_WRONGSTATE, "Must call EPSSolve() first");
  KS_CHECK(i >= 0, KS_ERR_ARG_OUTOFRANGE, "The index cannot be negative");
  KS_CHECK(i < eps->nconv, KS_ERR_ARG_OUTOFRANGE, "The index can be nconv-1 at most, see EPSGetConverged()");
  const int k = eps->perm[i];
  if (eigr) *eigr = eps->eigr[k];
  if (eigi) *eigi = eps->eigi[k];
  return KS_SUCCESS;
}
// BV_GetEigenvector bvimpl.h:423-446, the conjugate-pair rule of every eigenvector getter: eigenvalue k of the basis X with imaginary part im has its
// vector in column k (im = 0: the imaginary part is zero), in columns k, k + 1 (im > 0) or in columns k - 1, k with the imaginary part negated (im < 0).
// vr, vi: n_local doubles on the host or on the device, either may be NULL
static int get_eigenvector(ks_bv X, int k, double im, double *vr, double *vi, bool host)
{
  ks_ctx ctx = X->ctx; const size_t nloc = X->n;
  const int kr = im < 0.0 ? k - 1 : k;
  if (host) {
    if (vr) KS_CALL(ks_bv_get_column_host(X, kr, vr));
    if (vi) {
      if (im == 0.0) for (size_t r = 0; r < nloc; r++) vi[r] = 0.0;
      else { KS_CALL(ks_bv_get_column_host(X, kr + 1, vi)); if (im < 0.0) for (size_t r = 0; r < nloc; r++) vi[r] = -vi[r]; }
    }
    return KS_SUCCESS;
  }
  KS_HIP(hipSetDevice(ctx->device));
  if (vr) KS_CALL(ksk_copy(ctx, ks_bv_col(X, kr), vr, nloc));
  if (vi) {
    if (im == 0.0) KS_HIP(hipMemsetAsync(vi, 0, nloc * sizeof(double), ctx->stream));
    else { KS_CALL(ksk_copy(ctx, ks_bv_col(X, kr + 1), vi, nloc)); if (im < 0.0) KS_CALL(ksk_scale(ctx, vi, nloc, -1.0)); }
  }
  KS_HIP(ks_sync(ctx));
  return KS_SUCCESS;
}
// EPSGetEigenpair epssolve.c:405, EPSGetEigenvector: through perm; the vectors on the host, or device vectors of n_local doubles (what EPSGetEigenpair
// fills when the Vecs live on the GPU)
static int get_eigenpair(ks_eps eps, int i, double *eigr, double *eigi, double *xr, double *xi, bool host)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(eps->solved, KS_ERR_ARG_WRONGSTATE, "Must call EPSSolve() first");
  KS_CHECK(i >= 0 && i < eps->nconv, KS_ERR_ARG_OUTOFRANGE, "The index can be nconv-1 at most, see EPSGetConverged()");
  KS_CALL(ks_eps_schur_vectors(eps));
  const int k = eps->perm[i];
  if (eigr) *eigr = eps->eigr[k];
  if (eigi) *eigi = eps->eigi[k];
  return get_eigenvector(eps->V, k, eps->eigi[k], xr, xi, host);
}
extern "C" int ks_eps_get_eigenvector_host(ks_eps eps, int i, double *xr)
{
  KS_CHECK(eps && xr, KS_ERR_ARG_NULL, "NULL argument");
  return get_eigenpair(eps, i, nullptr, nullptr, xr, nullptr, true);
}
extern "C" int ks_eps_get_eigenpair_host(ks_eps eps, int i, double *eigr, double *eigi, double *xr, double *xi) { return get_eigenpair(eps, i, eigr, eigi, xr, xi, true); }
extern "C" int ks_eps_get_eigenpair(ks_eps eps, int i, double *eigr, double *eigi, double *xr_dev, double *xi_dev) { return get_eigenpair(eps, i, eigr, eigi, xr_dev, xi_dev, false); }
// EPSGetLeftEigenvector epssolve.c:567-613: column i of the left basis through the same pair rules; for a symmetric problem the right eigenvector
// (the "trivial" branch); a non-symmetric solve without EPSSetTwoSided has none
static int left_basis(ks_eps eps, int i, ks_bv *bv)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(eps->solved, KS_ERR_ARG_WRONGSTATE, "Must call EPSSolve() first");
  KS_CHECK(i >= 0 && i < eps->nconv, KS_ERR_ARG_OUTOFRANGE, "The index can be nconv-1 at most, see EPSGetConverged()");
  const bool trivial = eps->left_trivial;
  KS_CHECK(trivial || eps->twosided_solved, KS_ERR_ARG_WRONGSTATE, "Must request left vectors with EPSSetTwoSided");
  KS_CALL(ks_eps_schur_vectors(eps));
  *bv = trivial ? eps->V : eps->VL;
  return KS_SUCCESS;
}
extern "C" int ks_eps_get_left_eigenvector(ks_eps eps, int i, double *yr_dev, double *yi_dev)
{
  ks_bv W = nullptr;
  KS_CALL(left_basis(eps, i, &W));
  return get_eigenvector(W, eps->perm[i], eps->eigi[eps->perm[i]], yr_dev, yi_dev, false);
}
extern "C" int ks_eps_get_left_eigenvector_host(ks_eps eps, int i, double *yr, double *yi)
{
  ks_bv W = nullptr;
  KS_CALL(left_basis(eps, i, &W));
  return get_eigenvector(W, eps->perm[i], eps->eigi[eps->perm[i]], yr, yi, true);
}
extern "C" int ks_eps_get_error_estimate(ks_eps eps, int i, double *errest)
{
  KS_CHECK(eps && errest, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(eps->solved, KS_ERR_ARG_WRONGSTATE, "Must call EPSSolve() first");
  KS_CHECK(i >= 0 && i < eps->nconv, KS_ERR_ARG_OUTOFRANGE, "The index can be nconv-1 at most, see EPSGetConverged()");
  *errest = eps->errest[eps->perm[i]];
  return KS_SUCCESS;
}

extern "C" int ks_eps_compute_error(ks_eps eps, int i, int type, double *error)   // epssolve.c:742-815 with :666-718
{
  KS_CHECK(eps && error, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(eps->solved, KS_ERR_ARG_WRONGSTATE, "Must call EPSSolve() first");
  KS_CHECK(i >= 0 && i < eps->nconv, KS_ERR_ARG_OUTOFRANGE, "The index can be nconv-1 at most, see EPSGetConverged()");
  KS_CALL(ks_eps_schur_vectors(eps));
  const int j = eps->perm[i];
  const double kr = eps->eigr[j], ki = eps->eigi[j];
  ks_bv V = eps->V;
  double nrm = 0.0, nrml = 0.0;
  // complex pair in real arithmetic: xr = X(:,jr), xi = sg*X(:,jr+1) (BV_GetEigenvector bvimpl.h:423-446)
  const int jr = ki < 0.0 ? j - 1 : j;
  auto residual = [&](ks_bv X, bool trans, double *out) { return ks_eps_residual_norm(eps, kr, ki, ks_bv_col(X, jr), ki == 0.0 ? nullptr : ks_bv_col(X, jr + 1), ki < 0.0 ? -1.0 : 1.0, out, trans); };
  KS_CALL(residual(V, false, &nrm));
  if (eps->twosided_solved) { KS_CALL(residual(eps->VL, true, &nrml)); nrm = std::max(nrm, nrml); }   // two-sided: the maximum with the left residual (epssolve.c:778-783)
  double vecnorm = 1.0;
  if (eps->ghep) { ks_mat Bsave = V->matrix; V->matrix = nullptr; int rc = ks_bv_normcolumn(V, j, KS_NORM_2, &vecnorm); V->matrix = Bsave; if (rc) return rc; }   // epssolve.c:774: 2-norm of the eigenvector
  if (type == KS_EPS_ERROR_RELATIVE) nrm /= hypot(kr, ki) * vecnorm;
  else if (type == KS_EPS_ERROR_BACKWARD) { KS_CALL(ks_eps_matrix_norms(eps)); nrm /= (eps->nrma + hypot(kr, ki) * eps->nrmb) * vecnorm; }   // epssolve.c:782-800
  else KS_CHECK(type == KS_EPS_ERROR_ABSOLUTE, KS_ERR_ARG_OUTOFRANGE, "Invalid error type");
  *error = nrm;
  return KS_SUCCESS;
}

// ---- getters of the settings (EPSGetTolerances, EPSGetWhichEigenpairs, EPSGetTarget, EPSGetProblemType, EPSIs*, ...) ----
extern "C" int ks_eps_get_tolerances(ks_eps eps, double *tol, int *max_it)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  if (tol) *tol = eps->tol;
  if (max_it) *max_it = eps->solved ? eps->max_it : eps->max_it_user;      // 0 before set-up when left to the default
  return KS_SUCCESS;
}
extern "C" int ks_eps_get_which_eigenpairs(ks_eps eps, int *which) { KS_CHECK(eps && which, KS_ERR_ARG_NULL, "NULL argument"); *which = eps->which.which; return KS_SUCCESS; }
extern "C" int ks_eps_get_target(ks_eps eps, double *target) { KS_CHECK(eps && target, KS_ERR_ARG_NULL, "NULL argument"); *target = eps->which.target; return KS_SUCCESS; }
extern "C" int ks_eps_get_convergence_test(ks_eps eps, int *conv) { KS_CHECK(eps && conv, KS_ERR_ARG_NULL, "NULL argument"); *conv = eps->conv; return KS_SUCCESS; }
extern "C" int ks_eps_get_operators(ks_eps eps, ks_mat *A, ks_mat *B) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); if (A) *A = eps->A; if (B) *B = eps->B; return KS_SUCCESS; }
extern "C" int ks_eps_get_problem_type(ks_eps eps, int *type, int *generalized, int *hermitian, int *positive)   // EPSGetProblemType + EPSIsGeneralized/IsHermitian/IsPositive
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  const int t = eps->problem_type;
  if (type) *type = t;
  if (generalized) *generalized = (t == KS_EPS_GHEP || t == KS_EPS_GNHEP);
  if (hermitian) *hermitian = (t == KS_EPS_HEP || t == KS_EPS_GHEP);
  if (positive) *positive = (t == KS_EPS_GHEP);
  return KS_SUCCESS;
}
// EPSGetInvariantSubspace epssolve.c:247-280: an orthonormal basis of the converged invariant subspace into nconv device
// vectors. Non-symmetric problems: the Schur vectors, which only exist until the eigenvectors are first formed.
extern "C" int ks_eps_get_invariant_subspace(ks_eps eps, double *const *v_dev)
{
  KS_CHECK(eps && v_dev, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(eps->solved, KS_ERR_ARG_WRONGSTATE, "Must call EPSSolve() first");
  KS_CHECK(!eps->vectors_done || eps->problem_type_resolved_hermitian, KS_ERR_ARG_WRONGSTATE,
           "EPSGetInvariantSubspace must be called before EPSGetEigenpair,EPSGetEigenvector or EPSComputeError");
  KS_HIP(hipSetDevice(eps->ctx->device));
  for (int i = 0; i < eps->nconv; i++) KS_CHECK(v_dev[i], KS_ERR_ARG_NULL, "vector %d is NULL", i);
  if (eps->balanced && !eps->vectors_done && eps->nconv) {  // epssolve.c:351-362: Q <- orth(D \ Q)
    ks_bv T = nullptr;
    KS_CALL(ks_bv_create(eps->ctx, eps->V->n, eps->V->N, eps->nconv, 0, &T));
    int rc = KS_SUCCESS;
    for (int i = 0; i < eps->nconv && !rc; i++) rc = ks_eps_pointwise(eps, ks_bv_col(eps->V, i), eps->D, ks_bv_col(T, i), false);
    if (!rc) rc = ks_bv_orthogonalize(T, nullptr, 0);
    for (int i = 0; i < eps->nconv && !rc; i++) rc = ksk_copy(eps->ctx, ks_bv_col(T, i), v_dev[i], eps->V->n);
    ks_sync(eps->ctx);
    ks_bv_destroy(T);
    return rc;
  }
  for (int i = 0; i < eps->nconv; i++) KS_CALL(ksk_copy(eps->ctx, ks_bv_col(eps->V, i), v_dev[i], eps->V->n));
  KS_HIP(ks_sync(eps->ctx));
  return KS_SUCCESS;
}
extern "C" int ks_eps_get_bv(ks_eps eps, ks_bv *V) { KS_CHECK(eps && V, KS_ERR_ARG_NULL, "NULL argument"); *V = eps->V; return KS_SUCCESS; }
extern "C" int ks_eps_get_stats(ks_eps eps, long long *steps, long long *passes, int *restarts)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  if (steps) *steps = eps->steps; if (passes) *passes = eps->passes; if (restarts) *restarts = eps->restarts;
  return KS_SUCCESS;
}

// EPSSetType epsbasic.c: Krylov-Schur (the default), LOBPCG, GD or JD. LOBPCG, GD and JD make STPRECOND the default of the solver's ST (EPSSetDefaultST_Precond
// epsdefault.c) unless the caller chose a type; going back to Krylov-Schur undoes that default. The infinite default shift is GD's and JD's alone (davidson.c:80)
extern "C" int ks_eps_set_type(ks_eps eps, int type)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(type == KS_EPS_KRYLOVSCHUR || type == KS_EPS_LOBPCG || type == KS_EPS_GD || type == KS_EPS_JD, KS_ERR_SUP, "only EPSKRYLOVSCHUR, EPSLOBPCG, EPSGD and EPSJD are built");
  if (type == eps->type) return KS_SUCCESS;
  eps->type = type; eps->solved = false;
  if (eps->st && eps->st->sigma_inf) { eps->st->sigma_inf = false; eps->st->ready = false; }
  if (type == KS_EPS_LOBPCG || type == KS_EPS_GD || type == KS_EPS_JD) {
    ks_st st = nullptr;
    KS_CALL(ks_eps_get_st(eps, &st));
    if (!st->type_set) { st->type = KS_ST_PRECOND; st->ready = false; }
  } else if (eps->st && !eps->st->type_set && eps->st->type == KS_ST_PRECOND) { eps->st->type = KS_ST_SHIFT; eps->st->ready = false; }
  return KS_SUCCESS;
}
extern "C" int ks_eps_get_type(ks_eps eps, int *type) { KS_CHECK(eps && type, KS_ERR_ARG_NULL, "NULL argument"); *type = eps->type; return KS_SUCCESS; }
extern "C" int ks_eps_lobpcg_set_blocksize(ks_eps eps, int bs)         // EPSLOBPCGSetBlockSize lobpcg.c:398-420
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(bs >= 0, KS_ERR_ARG_OUTOFRANGE, "Invalid block size %d", bs);
  KS_CHECK(bs <= 16, KS_ERR_ARG_OUTOFRANGE, "block size %d: this build keeps the blocks of LOBPCG to 16 columns (48 in the projected problem)", bs);
  eps->lob.bs = bs; eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_lobpcg_get_blocksize(ks_eps eps, int *bs) { KS_CHECK(eps && bs, KS_ERR_ARG_NULL, "NULL argument"); *bs = eps->lob.bs; return KS_SUCCESS; }
extern "C" int ks_eps_lobpcg_set_restart(ks_eps eps, double r)          // EPSLOBPCGSetRestart lobpcg.c:472-500
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(r >= 0.1 && r <= 1.0, KS_ERR_ARG_OUTOFRANGE, "The restart argument %g must be in the range [0.1,1.0]", r);
  eps->lob.restart = r; eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_lobpcg_get_restart(ks_eps eps, double *r) { KS_CHECK(eps && r, KS_ERR_ARG_NULL, "NULL argument"); *r = eps->lob.restart ? eps->lob.restart : 0.9; return KS_SUCCESS; }
extern "C" int ks_eps_lobpcg_set_locking(ks_eps eps, int lock) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); eps->lob.lock = lock != 0; eps->solved = false; return KS_SUCCESS; }   // EPSLOBPCGSetLocking
extern "C" int ks_eps_lobpcg_get_locking(ks_eps eps, int *lock) { KS_CHECK(eps && lock, KS_ERR_ARG_NULL, "NULL argument"); *lock = eps->lob.lock ? 1 : 0; return KS_SUCCESS; }
extern "C" int ks_eps_lobpcg_get_stats(ks_eps eps, long long *iterations, long long *hard_locks, long long *mat_columns, long long *pc_columns)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  if (iterations) *iterations = eps->lob.iterations; if (hard_locks) *hard_locks = eps->lob.hard_locks;
  if (mat_columns) *mat_columns = eps->lob.mat_columns; if (pc_columns) *pc_columns = eps->lob.pc_columns;
  return KS_SUCCESS;
}
