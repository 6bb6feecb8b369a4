// Host side of the path: the Krylov-Schur restart driver. The dense projected problem it solves at every restart
// (DS HEP / NHEP), the eigenvalue comparisons and the ST's eigenvalue map are host-only code in ks_ds.cpp.
//
// Restates, in plain C++ on host scalars:
//   EPSSetUp_KrylovSchur            src/eps/impls/krylov/krylovschur/krylovschur.c:93-194
//   EPSSetDimensions_Default        src/eps/interface/epssetup.c:654-678
//   EPSSolve_KrylovSchur_Default    krylovschur.c:227-337
//   EPSKrylovConvergence            src/eps/impls/krylov/epskrylov.c:207-295
//   EPSConvergedRelative / EPSStoppingBasic   src/eps/interface/epsdefault.c:224,290
//   EPSGetStartVector               src/eps/interface/epssolve.c:841-873
//   EPSSolve epilogue + SlepcSortEigenvalues  epssolve.c:119-208, src/sys/slepcsc.c:89-140
//   EPSComputeError / EPSComputeResidualNorm_Private  epssolve.c:666-718,742-815
//   EPSSolve_KrylovSchur_TwoSided   krylovschur/ks-twosided.c:27-241 (with EPSGetLeftStartVector epssolve.c:879-900 and the left
//                                   branches of EPSKrylovConvergence, EPSComputeVectors_Schur, EPSGetLeftEigenvector, EPSComputeError)
#include "ksgpu_internal.h"
#include "ks_eps_impl.h"
#include "ks_dense.h"
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
static int matrix_norms(ks_eps eps)                                         // epssetup.c:345-358
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
  if (eps->type == KS_EPS_LOBPCG) {                    // a block solver uses all of them (lobpcg.c:133): device copies, made only for that solver type
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

// DSSynchronize (dsops.c:875 -> DSSynchronize_HEP dshep.c:673-713, DSSynchronize_NHEP dsnhep.c:379): every rank leaves with rank 0's
// projected matrix, vectors and eigenvalues. The scalars the convergence test and the restart sizes are computed from (beta of the
// expansion, its length, the breakdown flag) travel in the same message, so the integer control flow that follows is identical on
// all ranks whatever the allreduce provider returned.
static int ds_synchronize(ks_eps eps, std::vector<double> *M1, std::vector<double> *M2, double *beta, int *nv, int *breakdown)
{
  ks_ctx ctx = eps->ctx;
  if (!ks_is_multi(ctx) || eps->ds_parallel != KS_DS_PARALLEL_SYNCHRONIZED) return KS_SUCCESS;      // (the force_multi test hook issues it on one rank too)
  std::vector<double> pack;
  pack.reserve(M1->size() + M2->size() + 2 * eps->eigr.size() + 3);
  pack.insert(pack.end(), M1->begin(), M1->end());
  pack.insert(pack.end(), M2->begin(), M2->end());
  pack.insert(pack.end(), eps->eigr.begin(), eps->eigr.end());
  pack.insert(pack.end(), eps->eigi.begin(), eps->eigi.end());
  pack.push_back(*beta); pack.push_back((double)*nv); pack.push_back((double)*breakdown);
  KS_CALL(ks_comm_bcast0_host(ctx, pack.data(), (int)(pack.size() * sizeof(double))));
  size_t o = 0;
  std::copy(pack.begin() + o, pack.begin() + o + M1->size(), M1->begin()); o += M1->size();
  std::copy(pack.begin() + o, pack.begin() + o + M2->size(), M2->begin()); o += M2->size();
  std::copy(pack.begin() + o, pack.begin() + o + eps->eigr.size(), eps->eigr.begin()); o += eps->eigr.size();
  std::copy(pack.begin() + o, pack.begin() + o + eps->eigi.size(), eps->eigi.begin()); o += eps->eigi.size();
  *beta = pack[o]; *nv = (int)pack[o + 1]; *breakdown = (int)pack[o + 2];
  return KS_SUCCESS;
}

// The same for values outside the DS that the two-sided variant computes with allreduces and then feeds into host arithmetic every rank must
// repeat bit for bit (M = W^T V, the coefficients that go through its LU, the two residual norms)
static int ds_synchronize_values(ks_eps eps, double *v, size_t count)
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
// the stopping test of one restart: user function or the basic one, then the step cap of the bench harness
static int stopping_test(ks_eps eps, int k)
{
  int reason = KS_EPS_CONVERGED_ITERATING;
  if (eps->stop_fn) { const int rc = eps->stop_fn(eps, eps->its, eps->max_it, k, eps->nev, &reason, eps->stop_ctx); KS_CHECK(!rc, rc, "the user's stopping test returned %d", rc); }
  else ks_eps_stopping_basic(eps, eps->its, eps->max_it, k, eps->nev, &reason, nullptr);
  eps->reason = reason;
  if (eps->reason == KS_EPS_CONVERGED_ITERATING && eps->max_steps && eps->steps >= eps->max_steps) eps->reason = KS_EPS_CONVERGED_USER;
  return KS_SUCCESS;
}
static int monitor(ks_eps eps, int nconv, int nest)                                            // EPSMonitor epsmon.c:21-33
{
  if (!eps->mon_fn) return KS_SUCCESS;
  const int rc = eps->mon_fn(eps, eps->its, nconv, eps->eigr.data(), eps->eigi.data(), eps->errest.data(), nest, eps->mon_ctx);
  KS_CHECK(!rc, rc, "the user's monitor returned %d", rc);
  return KS_SUCCESS;
}

// EPSConvergedRelative / Absolute / Norm epsdefault.c:224-257
static double converged_estimate(ks_eps eps, double re, double im, double res)
{
  const double w = hypot(re, im);
  switch (eps->conv) {
    case KS_EPS_CONV_USER: { double e = 0.0; const int rc = eps->conv_fn(eps, re, im, res, &e, eps->conv_ctx); if (rc && !eps->cb_err) eps->cb_err = rc; return e; }
    case KS_EPS_CONV_ABS:  return res;
    case KS_EPS_CONV_NORM: return res / (eps->nrma + w * eps->nrmb);
    default:               return (w != 0.0) ? res / w : std::numeric_limits<double>::max();
  }
}

namespace {
__global__ void k_pw(long long n, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ out, int mul)
{
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = mul ? a[i] * b[i] : a[i] / b[i];
}
__global__ void k_sign_half(long long n, double *__restrict__ z)
{
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) z[i] = z[i] < 0.5 ? -1.0 : 1.0;
}
__global__ void k_bal_update(long long n, double *__restrict__ D, const double *__restrict__ p)
{
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) if (p[i] != 0.0) D[i] /= fabs(p[i]);
}
// two-sided form (epsdefault.c:419-421): D_i *= sqrt(|r_i / p_i|) where |p_i| > cutoff * norma and r_i != 0
__global__ void k_bal_update2(long long n, double *__restrict__ D, const double *__restrict__ p, const double *__restrict__ r, double thr)
{
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    if (fabs(p[i]) > thr && r[i] != 0.0) D[i] *= sqrt(fabs(r[i] / p[i]));
}
__global__ void k_fill(long long n, double *__restrict__ x, double v)
{
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) x[i] = v;
}
}
static int pointwise(ks_eps eps, const double *a, const double *b, double *out, bool mul)     // VecPointwiseMult / VecPointwiseDivide
{
  const long long n = eps->V->n;
  if (!n) return KS_SUCCESS;
  const unsigned nb = (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, (long long)eps->ctx->num_cu * 16));
  hipLaunchKernelGGL(k_pw, dim3(nb), dim3(256), 0, eps->ctx->stream, n, a, b, out, mul ? 1 : 0);
  KS_HIP(hipGetLastError());
  return KS_SUCCESS;
}
// the balanced operator D Op D^-1 as a matrix-free operator (STApply with st->D, stsolve.c:252-256)
static int balanced_mult(void *user, const double *x, double *y)
{
  ks_eps eps = (ks_eps)user;
  KS_CALL(pointwise(eps, x, eps->D, eps->wb, false));
  KS_CALL(ks_mat_mult_internal(eps->op_inner, eps->wb, y));
  return pointwise(eps, y, eps->D, y, true);
}
// EPSBuildBalance_Krylov epsdefault.c:370-434 over balance_its random +-1 vectors z. One-sided: D <- D ./ |p|, p = D Op D^-1 z. Two-sided: also
// r = D^-1 Op^T D z (STApplyHermitianTranspose: ks_mat_mult_transpose on the operator), D_i *= sqrt(|r_i / p_i|) where |p_i| exceeds cutoff times the
// infinity norm of the first p
static int build_balance(ks_eps eps)
{
  ks_ctx ctx = eps->ctx; const long long n = eps->V->n;
  const unsigned nb = (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, (long long)ctx->num_cu * 16));
  if (eps->D_n != n) { if (eps->D) hipFree(eps->D); if (eps->wb) hipFree(eps->wb); eps->D = eps->wb = nullptr;
    KS_HIP(hipMalloc(&eps->D, sizeof(double) * std::max<long long>(n, 1))); KS_HIP(hipMalloc(&eps->wb, sizeof(double) * std::max<long long>(n, 1))); eps->D_n = (int)n; }
  if (n) hipLaunchKernelGGL(k_fill, dim3(nb), dim3(256), 0, ctx->stream, n, eps->D, 1.0);
  double *z = ks_bv_col(eps->W, 3), *p = ks_bv_col(eps->W, 4);
  eps->W->row_start = eps->V->row_start;
  double norma = 0.0;
  for (int j = 0; j < eps->balance_its; j++) {
    KS_CALL(ks_bv_set_random_column(eps->W, 3, eps->seed + 7919ULL * (uint64_t)(j + 1)));           // a random vector of +-1's
    if (n) hipLaunchKernelGGL(k_sign_half, dim3(nb), dim3(256), 0, ctx->stream, n, z);
    KS_CALL(balanced_mult(eps, z, p));                                                               // p = D Op (D \ z)
    if (eps->balance == KS_EPS_BALANCE_TWOSIDE) {
      if (j == 0) KS_CALL(ks_bv_normcolumn(eps->W, 4, KS_NORM_INFINITY, &norma));                    // VecAbs + VecMax: the estimate of the matrix infinity norm
      KS_CALL(pointwise(eps, z, eps->D, z, true));                                                    // r = D \ (Op' (D z))
      KS_CALL(ks_mat_mult_transpose_internal(eps->op_inner, z, eps->wb));
      KS_CALL(pointwise(eps, eps->wb, eps->D, eps->wb, false));
      if (n) hipLaunchKernelGGL(k_bal_update2, dim3(nb), dim3(256), 0, ctx->stream, n, eps->D, p, eps->wb, eps->balance_cutoff * norma);
    } else if (n) hipLaunchKernelGGL(k_bal_update, dim3(nb), dim3(256), 0, ctx->stream, n, eps->D, p);
    KS_HIP(hipGetLastError());
  }
  return KS_SUCCESS;
}

// EPSComputeResidualNorm_Private epssolve.c:666-718 (STGetMatrix 0/1 = the user's A and B): || A x - k B x ||_2 for a
// real eigenvalue, hypot of the two real-arithmetic residuals for a pair (xi_sign * xi is the imaginary part).
// Work vectors: W columns 0..2.
// trans (the left residual of the two-sided variant): the transposed products and the conjugate eigenvalue, ||A^T y - conj(k) B^T y|| (:676,692,705,711)
static int residual_norm(ks_eps eps, double kr, double ki, const double *xr, const double *xi, double xi_sign, double *out, bool trans = false)
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

// EPSComputeRitzVector epsdefault.c:313-364 followed by the residual of epskrylov.c:256-264 (-eps_true_residual):
// x = V(:,0:nv) Zr [, y = V(:,0:nv) Zi], purified through the operator for a GHEP, into W columns 3 and 4.
static int ritz_vector(ks_eps eps, int nv, const double *Zr, const double *Zi);
static int true_residual(ks_eps eps, int nv, double re, double im, const double *Zr, const double *Zi, double *resnorm)
{
  KS_CALL(ritz_vector(eps, nv, Zr, Zi));
  return residual_norm(eps, re, im, ks_bv_col(eps->W, 3), Zi ? ks_bv_col(eps->W, 4) : nullptr, 1.0, resnorm);
}
// EPSComputeRitzVector epsdefault.c:313-364: x (W column 3) and, for a pair, y (W column 4)
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
    KS_CALL(pointwise(eps, x, eps->D, x, false));
    if (Zi) KS_CALL(pointwise(eps, y, eps->D, y, false));
    double nx = 0.0, ny = 0.0;
    KS_CALL(ks_bv_normvec(W, x, KS_NORM_2, &nx));
    if (Zi) KS_CALL(ks_bv_normvec(W, y, KS_NORM_2, &ny));
    const double nrm = hypot(nx, ny);
    if (nrm != 0.0) { KS_CALL(ksk_scale(eps->ctx, x, V->n, 1.0 / nrm)); if (Zi) KS_CALL(ksk_scale(eps->ctx, y, V->n, 1.0 / nrm)); }
  }
  return KS_SUCCESS;
}

// EPSGetStartVector epssolve.c:841-873
static int start_vector(ks_eps eps, int i, bool *breakdown)
{
  if (i == 0 && eps->have_v0) KS_CALL(ks_bv_set_column_host(eps->V, 0, eps->v0.data()));
  else KS_CALL(ks_bv_set_random_column(eps->V, i, eps->seed));
  if (eps->ghep) {                                   // force the vector to be in the range of OP (epssolve.c:860-868)
    KS_CALL(ksk_copy(eps->ctx, ks_bv_col(eps->V, i), ks_bv_col(eps->W, 0), eps->V->n));
    KS_CALL(ks_mat_mult_internal(eps->op, ks_bv_col(eps->W, 0), ks_bv_col(eps->V, i)));
  }
  double norm = 0.0; int lindep = 0;
  KS_CALL(ks_bv_orthogonalizecolumn(eps->V, i, nullptr, &norm, &lindep));
  if (breakdown) *breakdown = lindep != 0;
  else if (lindep || norm == 0.0) {
    if (i == 0) KS_FAIL(KS_ERR_PLIB, "Initial vector is zero or belongs to the deflation space");
    KS_FAIL(KS_ERR_CONV_FAILED, "Unable to generate more start vectors");
  }
  KS_CALL(ks_bv_scalecolumn(eps->V, i, 1.0 / norm));
  return KS_SUCCESS;
}

// EPSGetLeftStartVector epssolve.c:879-900: the first left initial vector, else a random one (its own stream of numbers), orthonormalised in the left basis
static int left_start_vector(ks_eps eps, int i, bool *breakdown)
{
  if (i == 0 && eps->have_w0) KS_CALL(ks_bv_set_column_host(eps->VL, 0, eps->w0.data()));
  else KS_CALL(ks_bv_set_random_column(eps->VL, i, eps->seed ^ 0x9E3779B97F4A7C15ULL));
  double norm = 0.0; int lindep = 0;
  KS_CALL(ks_bv_orthogonalizecolumn(eps->VL, i, nullptr, &norm, &lindep));
  if (breakdown) *breakdown = lindep != 0;
  else if (lindep || norm == 0.0) {
    if (i == 0) KS_FAIL(KS_ERR_PLIB, "Left initial vector is zero");
    KS_FAIL(KS_ERR_CONV_FAILED, "Unable to generate more left start vectors");
  }
  KS_CALL(ks_bv_scalecolumn(eps->VL, i, 1.0 / norm));
  return KS_SUCCESS;
}

// EPSComputeVectors_Schur epsdefault.c:105-169, run on first use (EPSComputeVectors epssolve.c:... state EPS_STATE_EIGENVECTORS):
// X = V*Z with Z the normalised eigenvectors of the trimmed quasi-triangular T. Until then V(:,0:nconv) is the orthonormal
// Schur basis that EPSGetInvariantSubspace hands out.
static int compute_vectors(ks_eps eps)
{
  if (eps->vectors_done) return KS_SUCCESS;
  ks_bv V = eps->V; ksd::DsNhep &ds = eps->twosided_solved ? static_cast<ksd::DsNhep &>(eps->dst) : eps->dsn;
  const int nc = eps->nconv;
  KS_CALL(ks_bv_set_active_columns(V, 0, nc));
  if (nc) {
    for (int k = 0; k < nc; k++) k = ds.vectors(k, false, nullptr);
    KS_CALL(ks_bv_multinplace(V, ds.X.data(), ds.ld, 0, nc));
    if (eps->balanced) {                                    // epsdefault.c:130-139: x <- D \ x, then normalise (pairs together)
      for (int i = 0; i < nc; i++) KS_CALL(pointwise(eps, ks_bv_col(V, i), eps->D, ks_bv_col(V, i), false));
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

// ---- EPSSetUp (epssetup.c:286-420): problem type, ST, sort criteria, dimensions, basis, constraints, balancing. passes0: the basis'
// Gram-Schmidt pass count before the solve's own work ----
static int set_up(ks_eps eps, long long *passes0)
{
  KS_CHECK(eps && eps->A, KS_ERR_ORDER, "EPSSetOperators must be called first");
  ks_mat A = eps->A;
  const int n = A->n_global;
  KS_CHECK(eps->which.which != KS_EPS_WHICH_USER || eps->which.fn, KS_ERR_ORDER, "Must call EPSSetEigenvalueComparison() first");   // epssetup.c:311
  int ptype = eps->problem_type;
  if (!ptype) ptype = eps->B ? KS_EPS_GNHEP : KS_EPS_NHEP;             // default problem type (epssetup.c:318-322)
  if (!eps->B && ptype == KS_EPS_GNHEP) ptype = KS_EPS_NHEP;          // "reverting to a standard eigenproblem" (epssetup.c:324-327)
  if (!eps->B && ptype == KS_EPS_GHEP) ptype = KS_EPS_HEP;
  KS_CHECK(!eps->B || ptype == KS_EPS_GNHEP || ptype == KS_EPS_GHEP, KS_ERR_ARG_INCOMP, "Inconsistent EPS state: the problem type does not match the number of matrices");
  const bool ghep = ptype == KS_EPS_GHEP;
  eps->twosided_solved = false; eps->left_trivial = ptype == KS_EPS_HEP || ghep;
  if (eps->twosided) {                                                 // what the two-sided variant is built for: each case is listed in ksgpu.h
    KS_CHECK(ptype != KS_EPS_HEP && !ghep, KS_ERR_SUP, "Two-sided methods are not intended for Hermitian problems");   // epssetup.c:309
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
  }
  if (eps->conv == KS_EPS_CONV_NORM) KS_CALL(matrix_norms(eps));
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
  eps->ncv = ncv; eps->mpd = mpd;
  eps->max_it = eps->max_it_user ? eps->max_it_user : std::max(100, 2 * n / ncv);
  if (eps->V) { int vm = 0; ks_bv_get_sizes(eps->V, nullptr, nullptr, &vm, nullptr); if (vm != ncv + 1 || eps->V->nc) { ks_bv_destroy(eps->V); eps->V = nullptr; } }
  if (!eps->V) { KS_CALL(ks_bv_create(eps->ctx, A->n, A->n_global, ncv + 1, 0, &eps->V)); eps->V->row_start = A->row_start; }   // EPSAllocateSolution(eps,1)
  if (!eps->W) { KS_CALL(ks_bv_create(eps->ctx, A->n, A->n_global, 5, 0, &eps->W)); }     // work vectors: u, B*xr, B*xi, Ritz vector x, y
  eps->eigr.assign(ncv + 1, 0.0); eps->eigi.assign(ncv + 1, 0.0); eps->errest.assign(ncv + 1, 0.0);
  eps->perm.resize(ncv + 1); for (int i = 0; i <= ncv; i++) eps->perm[i] = i;
  eps->cb_err = 0;
  eps->nconv = 0; eps->its = 0; eps->reason = KS_EPS_CONVERGED_ITERATING; eps->steps = 0; eps->restarts = 0; eps->solved = false;
  ks_bv_gs_passes(eps->V, passes0, nullptr);
  ks_bv V = eps->V;
  KS_CALL(ks_bv_set_active_columns(V, 0, ncv + 1));
  KS_CALL(ks_bv_set_matrix(V, ghep ? (cayley ? st->bil : eps->B) : nullptr));   // EPS_SetInnerProduct epsimpl.h:280-292: STGetBilinearForm = B, or A + nu B for STCAYLEY (cayley.c:70-77)
  eps->ghep = ghep;
  eps->problem_type_resolved_hermitian = (ptype == KS_EPS_HEP || ghep) && eps->extraction != KS_EPS_HARMONIC;   // else variant EPS_KS_DEFAULT on the general DS (krylovschur.c:133-151)
  eps->vectors_done = true;
  if (eps->nds) {                                                      // process the deflation space (epssetup.c:397-404)
    KS_CHECK(eps->defl && eps->defl->n == A->n, KS_ERR_ARG_INCOMP, "the deflation space was set for an operator of another size");
    std::vector<const double *> cp(eps->nds);
    for (int i = 0; i < eps->nds; i++) cp[i] = ks_bv_col(eps->defl, i);
    int kd = eps->nds;
    int rc = ks_bv_insert_constraints(V, &kd, cp.data());
    ks_bv_destroy(eps->defl); eps->defl = nullptr; eps->nds = 0;
    if (rc) return rc;
  }

  // balancing of non-symmetric problems (epssetup.c:383-391): build D, then expand with D Op D^-1
  eps->balanced = false;
  if ((ptype == KS_EPS_NHEP || ptype == KS_EPS_GNHEP) && eps->balance != KS_EPS_BALANCE_NONE) {
    eps->op_inner = eps->op;
    if (eps->balance == KS_EPS_BALANCE_ONESIDE || eps->balance == KS_EPS_BALANCE_TWOSIDE) KS_CALL(build_balance(eps));
    else KS_CHECK(eps->D && eps->D_n == A->n, KS_ERR_ORDER, "EPS_BALANCE_USER: the balancing matrix does not match the operator");
    if (!eps->bal_op) KS_CALL(ks_mat_create_shell(eps->ctx, A->n, A->row_start, A->n_global, balanced_mult, eps, &eps->bal_op));
    eps->bal_op->n = A->n; eps->bal_op->row_start = A->row_start; eps->bal_op->n_global = A->n_global;
    eps->bal_op->shell_nosync = !eps->op_inner->shell_mult;         // D A D^-1 on an assembled matrix is three kernel launches: keep the enqueued-ahead run
    eps->op = eps->bal_op; eps->balanced = true;
  }
  if (eps->twosided) {
    // the left basis (EPSAllocateSolution: BVDuplicate, epssetup.c:733) and Op^T as a matrix (MatCreateHermitianTranspose of STGetOperator, ks-twosided.c:141-142)
    if (eps->VL) { int vm = 0; ks_bv_get_sizes(eps->VL, nullptr, nullptr, &vm, nullptr); if (vm != ncv + 1) { ks_bv_destroy(eps->VL); eps->VL = nullptr; } }
    if (!eps->VL) { KS_CALL(ks_bv_duplicate(V, &eps->VL)); eps->VL->row_start = A->row_start; }
    KS_CALL(ks_bv_set_active_columns(eps->VL, 0, ncv + 1));
    if (eps->opT_owned) ks_mat_destroy(eps->opT);
    eps->opT = nullptr; eps->opT_owned = false;
    KS_CALL(ks_mat_create_transpose(eps->op, &eps->opT));
    eps->opT_owned = eps->op->shell_mult != nullptr;
    // one transposed product now, so that an operator without one fails here and not inside the first restart
    KS_HIP(hipMemsetAsync(ks_bv_col(eps->W, 3), 0, sizeof(double) * std::max(A->n, 1), eps->ctx->stream));
    KS_CALL(ks_mat_mult_internal(eps->opT, ks_bv_col(eps->W, 3), ks_bv_col(eps->W, 4)));
  }
  KS_CHECK(eps->extraction == KS_EPS_RITZ || !ghep, KS_ERR_SUP, "harmonic extraction with a B-inner product is not built");
  KS_CHECK(!eps->arb_fn || ((ptype == KS_EPS_HEP || ghep) && eps->extraction == KS_EPS_RITZ), KS_ERR_SUP, "arbitrary selection is built for the symmetric (Lanczos) variant only");
  return KS_SUCCESS;
}

// EPSSolve_KrylovSchur_Default (krylovschur.c:227-337) over the DS interface, with EPSKrylovConvergence (epskrylov.c:207-295) and its
// conjugate pairs. Symmetric variant: BVMatLanczos into T, arbitrary selection. General variant: BVMatArnoldi into A, harmonic extraction.
static int restart_loop(ks_eps eps, ksd::Ds &ds)
{
  ks_bv V = eps->V;
  const int nev = eps->nev, ncv = eps->ncv, mpd = eps->mpd;
  const bool hermitian = eps->problem_type_resolved_hermitian, harmonic = eps->extraction == KS_EPS_HARMONIC;   // harmonic: on eps->dsn
  const ksd::StMap &map = eps->cmp_ds.map;
  const bool early = map && (map.type == KS_ST_SHIFT || eps->conv == KS_EPS_CONV_NORM);    // epskrylov.c:253: back-transform before the estimate
  std::vector<double> g(harmonic ? ncv + 1 : 0);
  KS_CALL(start_vector(eps, 0, nullptr));
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

    // EPSKrylovConvergence(eps,FALSE,nconv,nv-nconv,beta,0.0,1.0,&k)
    int marker = -1, k;
    for (k = eps->nconv; k < nv; k++) {
      double re = eps->eigr[k], im = eps->eigi[k];
      if (early) map.backtransform(1, &re, &im);
      double resnorm = 0.0; const double *Zr = nullptr, *Zi = nullptr;
      const int newk = ds.ritz(k, &resnorm, &Zr, &Zi);
      if (eps->trueres) {                                      // epskrylov.c:256-264
        if (!early) map.backtransform(1, &re, &im);
        KS_CALL(true_residual(eps, nv, re, im, Zr, Zi, &resnorm));
      } else
      resnorm *= beta * gamma;                                 // corrf: only in harmonic KS (epskrylov.c:265)
      eps->errest[k] = converged_estimate(eps, re, im, resnorm);
      if (marker == -1 && eps->errest[k] >= eps->tol) marker = k;
      if (newk == k + 1) { eps->errest[k + 1] = eps->errest[k]; k++; }
      if (marker != -1 && !eps->trackall) break;               // getall: estimates for every Ritz pair (epskrylov.c:240,280)
    }
    k = (marker != -1) ? marker : nv;
    KS_CHECK(!eps->cb_err, eps->cb_err, "the user's convergence test returned %d", eps->cb_err);
    KS_CALL(stopping_test(eps, k));                            // EPSStoppingBasic
    const int nconv_mon = k;

    // update l
    if (eps->reason != KS_EPS_CONVERGED_ITERATING || breakdown || k == nv) l = 0;
    else {
      l = std::max(1, (int)((nv - k) * eps->keep));
      l = ds.truncate_size(k, nv, l);                          // do not split a 2x2 block (krylovschur.c:300)
    }
    if (!eps->lock && l > 0) { l += k; k = 0; }                // non-locking variant: reset no. of converged pairs (krylovschur.c:294)
    if (eps->reason == KS_EPS_CONVERGED_ITERATING) {
      if (breakdown || k == nv) {
        if (k < nev) {
          bool brk = false;
          KS_CALL(start_vector(eps, k, &brk));
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
    KS_CALL(monitor(eps, nconv_mon, nv));
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
  KS_CALL(ds_synchronize_values(eps, w.data(), w.size()));
  const int info = ksd::lu_factor(nv, LU.data(), nv, piv.data());
  KS_CHECK(info == 0, KS_ERR_LIB, "two-sided Krylov-Schur: W^T V is singular (zero pivot %d of %d): serious breakdown of the two-sided recurrence", info, nv);
  ksd::lu_solve(nv, LU.data(), nv, piv.data(), w.data(), false);
  KS_CALL(ks_bv_multcolumn(V, -1.0, 1.0, nv, w.data()));
  for (int i = 0; i < nv; i++) ds.a(i, nv - 1) += beta * w[i];
  KS_CALL(ks_bv_dotvec(V, ks_bv_col(W, nv), w.data()));
  KS_CALL(ds_synchronize_values(eps, w.data(), w.size()));
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
  const ksd::StMap &map = eps->cmp_ds.map;
  const bool early = map && (map.type == KS_ST_SHIFT || eps->conv == KS_EPS_CONV_NORM);
  std::vector<double> M((size_t)ld * ld, 0.0);                     // W^T V (the reference's ncv x ncv M)
  KS_CALL(start_vector(eps, 0, nullptr));
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
    KS_CALL(ds_synchronize_values(eps, M.data(), M.size()));
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
    { double nn[2] = {norm, norm2}; KS_CALL(ds_synchronize_values(eps, nn, 2)); norm = nn[0]; norm2 = nn[1]; }
    int marker = -1, k;
    for (k = eps->nconv; k < nv; k++) {
      double re = eps->eigr[k], im = eps->eigi[k];
      if (early) map.backtransform(1, &re, &im);
      double resnorm = 0.0, lresnorm = 0.0; const double *Zr = nullptr, *Zi = nullptr;
      const int newk = ds.ritz(k, &resnorm, &Zr, &Zi);
      eps->errest[k] = converged_estimate(eps, re, im, resnorm * beta * norm);
      if (marker == -1 && eps->errest[k] >= eps->tol) marker = k;
      ds.vectors_side(k, true, true, &lresnorm);
      const double lerrest = converged_estimate(eps, re, im, lresnorm * betat * norm2);
      eps->errest[k] = std::max(eps->errest[k], lerrest);
      if (marker == -1 && lerrest >= eps->tol) marker = k;
      if (newk == k + 1) { eps->errest[k + 1] = eps->errest[k]; k++; }
      if (marker != -1 && !eps->trackall) break;
    }
    k = (marker != -1) ? marker : nv;
    KS_CHECK(!eps->cb_err, eps->cb_err, "the user's convergence test returned %d", eps->cb_err);
    KS_CALL(stopping_test(eps, k));
    const int nconv_mon = k;

    // update l
    if (eps->reason != KS_EPS_CONVERGED_ITERATING || breakdown || k == nv) l = 0;
    else {
      l = std::max(1, (int)((nv - k) * eps->keep));
      l = ds.truncate_size(k, nv, l);
    }
    if (!eps->lock && l > 0) { l += k; k = 0; }                // non-locking variant: reset no. of converged pairs

    // update the corresponding vectors V(:,idx) = V*Q(:,idx), W(:,idx) = W*Z(:,idx)
    KS_CALL(ks_bv_set_active_columns(V, eps->nconv, nv)); KS_CALL(ks_bv_set_active_columns(W, eps->nconv, nv));
    KS_CALL(ks_bv_multinplace(V, ds.Q.data(), ld, eps->nconv, k + l));
    KS_CALL(ks_bv_multinplace(W, ds.hb.Q.data(), ld, eps->nconv, k + l));
    if (eps->reason == KS_EPS_CONVERGED_ITERATING && !breakdown) { KS_CALL(ks_bv_copycolumn(V, nv, k + l)); KS_CALL(ks_bv_copycolumn(W, nv, k + l)); }

    if (eps->reason == KS_EPS_CONVERGED_ITERATING) {
      if (breakdown || k == nv) {                              // start a new Arnoldi factorization
        if (k < nev) {
          bool brk = false, brkl = false;
          KS_CALL(start_vector(eps, k, &brk));
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
    KS_CALL(monitor(eps, nconv_mon, nv));
    eps->restarts++;
  }
  ds.truncate(eps->nconv, true);
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

// The eigenvectors of the general variant are formed on first use (compute_vectors); V(:,0:nconv) stays the Schur basis until then.
// Conjugate pairs come with the positive imaginary part first (epssolve.c:160-175): the inversion of sinvert flips the sign
static int epilogue_schur(ks_eps eps)
{
  eps->vectors_done = false;
  for (int i = 0; i < eps->nconv - 1; i++) {
    if (eps->eigi[i] != 0.0) {
      if (eps->eigi[i] < 0.0) {                                 // "the next correction only works with eigenvectors" (epssolve.c:166-169)
        eps->eigi[i] = -eps->eigi[i]; eps->eigi[i + 1] = -eps->eigi[i + 1];
        KS_CALL(compute_vectors(eps));
        KS_CALL(ks_bv_scalecolumn(eps->V, i + 1, -1.0));
      }
      i++;
    }
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

extern "C" int ks_eps_solve(ks_eps eps)   // EPSSolve epssolve.c:119 -> EPSSolve_KrylovSchur_Default krylovschur.c:227
{
  long long passes0 = 0;
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  if (eps->type == KS_EPS_LOBPCG) {                                    // EPSSolve_LOBPCG; V(:,0:nconv) holds the eigenvectors, nothing to map back or purify
    KS_CALL(ks_lobpcg_solve(eps));
    KS_CALL(ks_bv_set_active_columns(eps->V, 0, eps->nconv));
    sort_eigenvalues(eps);
    KS_CALL(ks_bv_set_num_constraints(eps->V, 0));
    eps->solved = true;
    return KS_SUCCESS;
  }
  KS_CALL(set_up(eps, &passes0));
  const bool hermitian = eps->problem_type_resolved_hermitian;
  ksd::Ds &ds = hermitian ? static_cast<ksd::Ds &>(eps->dsh) : eps->twosided ? static_cast<ksd::Ds &>(eps->dst) : eps->dsn;
  ds.allocate(eps->ncv + 1); ds.which = eps->cmp_ds; ds.state = ksd::DS_RAW;
  long long passesl0 = 0;
  if (eps->twosided) { eps->dst.permuted = 0; ks_bv_gs_passes(eps->VL, &passesl0, nullptr); KS_CALL(restart_loop_twosided(eps)); eps->twosided_solved = true; }
  else
  KS_CALL(restart_loop(eps, ds));
  // ---- EPSSolve epilogue ----
  KS_CALL(ks_bv_set_active_columns(eps->V, 0, eps->nconv));
  if (eps->twosided) KS_CALL(ks_bv_set_active_columns(eps->VL, 0, eps->nconv));
  eps->cmp_ds.map.backtransform(eps->nconv, eps->eigr.data(), eps->eigi.data());   // EPSComputeValues (epssolve.c:27-41): map the eigenvalues back through the ST
  KS_CALL(hermitian ? epilogue_hermitian(eps) : epilogue_schur(eps));
  sort_eigenvalues(eps);
  long long passes1 = 0; ks_bv_gs_passes(eps->V, &passes1, nullptr);
  eps->passes = passes1 - passes0;
  if (eps->twosided) { long long pl = 0; ks_bv_gs_passes(eps->VL, &pl, nullptr); eps->passes += pl - passesl0; }
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
extern "C" int ks_eps_get_eigenvector_host(ks_eps eps, int i, double *xr)
{
  KS_CHECK(eps && xr, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(eps->solved, KS_ERR_ARG_WRONGSTATE, "Must call EPSSolve() first");
  KS_CHECK(i >= 0 && i < eps->nconv, KS_ERR_ARG_OUTOFRANGE, "The index can be nconv-1 at most, see EPSGetConverged()");
  KS_CALL(compute_vectors(eps));
  const int k = eps->perm[i];
  // EPSComputeVectors_Hermitian: V already holds the Ritz vectors; pairs: BV_GetEigenvector bvimpl.h:423-446
  return ks_bv_get_column_host(eps->V, eps->eigi[k] < 0.0 ? k - 1 : k, xr);
}
extern "C" int ks_eps_get_eigenpair_host(ks_eps eps, int i, double *eigr, double *eigi, double *xr, double *xi)   // EPSGetEigenpair epssolve.c:405
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(eps->solved, KS_ERR_ARG_WRONGSTATE, "Must call EPSSolve() first");
  KS_CHECK(i >= 0 && i < eps->nconv, KS_ERR_ARG_OUTOFRANGE, "The index can be nconv-1 at most, see EPSGetConverged()");
  KS_CALL(compute_vectors(eps));
  const int k = eps->perm[i], nloc = eps->V->n;
  const double im = eps->eigi[k];
  if (eigr) *eigr = eps->eigr[k];
  if (eigi) *eigi = im;
  if (im > 0.0) { if (xr) KS_CALL(ks_bv_get_column_host(eps->V, k, xr)); if (xi) KS_CALL(ks_bv_get_column_host(eps->V, k + 1, xi)); }
  else if (im < 0.0) {
    if (xr) KS_CALL(ks_bv_get_column_host(eps->V, k - 1, xr));
    if (xi) { KS_CALL(ks_bv_get_column_host(eps->V, k, xi)); for (int r = 0; r < nloc; r++) xi[r] = -xi[r]; }
  } else { if (xr) KS_CALL(ks_bv_get_column_host(eps->V, k, xr)); if (xi) for (int r = 0; r < nloc; r++) xi[r] = 0.0; }
  return KS_SUCCESS;
}
// the same with device vectors of n_local doubles (what EPSGetEigenpair fills when the Vecs live on the GPU)
extern "C" int ks_eps_get_eigenpair(ks_eps eps, int i, double *eigr, double *eigi, double *xr_dev, double *xi_dev)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(eps->solved, KS_ERR_ARG_WRONGSTATE, "Must call EPSSolve() first");
  KS_CHECK(i >= 0 && i < eps->nconv, KS_ERR_ARG_OUTOFRANGE, "The index can be nconv-1 at most, see EPSGetConverged()");
  KS_CALL(compute_vectors(eps));
  const int k = eps->perm[i]; const size_t nloc = eps->V->n;
  const double im = eps->eigi[k];
  ks_ctx ctx = eps->ctx; ks_bv V = eps->V;
  KS_HIP(hipSetDevice(ctx->device));
  if (eigr) *eigr = eps->eigr[k];
  if (eigi) *eigi = im;
  const int kr = im < 0.0 ? k - 1 : k;
  if (xr_dev) KS_CALL(ksk_copy(ctx, ks_bv_col(V, kr), xr_dev, nloc));
  if (xi_dev) {
    if (im == 0.0) KS_HIP(hipMemsetAsync(xi_dev, 0, nloc * sizeof(double), ctx->stream));
    else { KS_CALL(ksk_copy(ctx, ks_bv_col(V, kr + 1), xi_dev, nloc)); if (im < 0.0) KS_CALL(ksk_scale(ctx, xi_dev, nloc, -1.0)); }
  }
  KS_HIP(ks_sync(ctx));
  return KS_SUCCESS;
}
// EPSGetLeftEigenvector epssolve.c:567-613: column i of the left basis through the same pair rules; for a symmetric problem the right eigenvector
// (the "trivial" branch); a non-symmetric solve without EPSSetTwoSided has none
static int left_basis(ks_eps eps, int i, ks_bv *bv)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(eps->solved, KS_ERR_ARG_WRONGSTATE, "Must call EPSSolve() first");
  KS_CHECK(i >= 0 && i < eps->nconv, KS_ERR_ARG_OUTOFRANGE, "The index can be nconv-1 at most, see EPSGetConverged()");
  const bool trivial = eps->left_trivial;
  KS_CHECK(trivial || eps->twosided_solved, KS_ERR_ARG_WRONGSTATE, "Must request left vectors with EPSSetTwoSided");
  KS_CALL(compute_vectors(eps));
  *bv = trivial ? eps->V : eps->VL;
  return KS_SUCCESS;
}
extern "C" int ks_eps_get_left_eigenvector(ks_eps eps, int i, double *yr_dev, double *yi_dev)
{
  ks_bv W = nullptr;
  KS_CALL(left_basis(eps, i, &W));
  const int k = eps->perm[i]; const size_t nloc = W->n;
  const double im = eps->eigi[k];
  ks_ctx ctx = eps->ctx;
  KS_HIP(hipSetDevice(ctx->device));
  const int kr = im < 0.0 ? k - 1 : k;
  if (yr_dev) KS_CALL(ksk_copy(ctx, ks_bv_col(W, kr), yr_dev, nloc));
  if (yi_dev) {
    if (im == 0.0) KS_HIP(hipMemsetAsync(yi_dev, 0, nloc * sizeof(double), ctx->stream));
    else { KS_CALL(ksk_copy(ctx, ks_bv_col(W, kr + 1), yi_dev, nloc)); if (im < 0.0) KS_CALL(ksk_scale(ctx, yi_dev, nloc, -1.0)); }
  }
  KS_HIP(ks_sync(ctx));
  return KS_SUCCESS;
}
extern "C" int ks_eps_get_left_eigenvector_host(ks_eps eps, int i, double *yr, double *yi)
{
  ks_bv W = nullptr;
  KS_CALL(left_basis(eps, i, &W));
  const int k = eps->perm[i], nloc = W->n;
  const double im = eps->eigi[k];
  const int kr = im < 0.0 ? k - 1 : k;
  if (yr) KS_CALL(ks_bv_get_column_host(W, kr, yr));
  if (yi) {
    if (im == 0.0) for (int r = 0; r < nloc; r++) yi[r] = 0.0;
    else { KS_CALL(ks_bv_get_column_host(W, kr + 1, yi)); if (im < 0.0) for (int r = 0; r < nloc; r++) yi[r] = -yi[r]; }
  }
  return KS_SUCCESS;
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
  KS_CALL(compute_vectors(eps));
  const int j = eps->perm[i];
  const double kr = eps->eigr[j], ki = eps->eigi[j];
  ks_bv V = eps->V;
  double nrm = 0.0;
  if (ki == 0.0) KS_CALL(residual_norm(eps, kr, ki, ks_bv_col(V, j), nullptr, 1.0, &nrm));
  else {
    // complex pair in real arithmetic: xr = V(:,jr), xi = sg*V(:,jr+1) (BV_GetEigenvector bvimpl.h:423-446)
    const int jr = ki > 0.0 ? j : j - 1;
    KS_CALL(residual_norm(eps, kr, ki, ks_bv_col(V, jr), ks_bv_col(V, jr + 1), ki > 0.0 ? 1.0 : -1.0, &nrm));
  }
  if (eps->twosided_solved) {                                         // two-sided: the maximum with the left residual (epssolve.c:778-783)
    ks_bv W = eps->VL; double nrml = 0.0;
    if (ki == 0.0) KS_CALL(residual_norm(eps, kr, ki, ks_bv_col(W, j), nullptr, 1.0, &nrml, true));
    else { const int jr = ki > 0.0 ? j : j - 1; KS_CALL(residual_norm(eps, kr, ki, ks_bv_col(W, jr), ks_bv_col(W, jr + 1), ki > 0.0 ? 1.0 : -1.0, &nrml, true)); }
    nrm = std::max(nrm, nrml);
  }
  double vecnorm = 1.0;
  if (eps->ghep) { ks_mat Bsave = V->matrix; V->matrix = nullptr; int rc = ks_bv_normcolumn(V, j, KS_NORM_2, &vecnorm); V->matrix = Bsave; if (rc) return rc; }   // epssolve.c:774: 2-norm of the eigenvector
  if (type == KS_EPS_ERROR_RELATIVE) nrm /= hypot(kr, ki) * vecnorm;
  else if (type == KS_EPS_ERROR_BACKWARD) { KS_CALL(matrix_norms(eps)); nrm /= (eps->nrma + hypot(kr, ki) * eps->nrmb) * vecnorm; }   // epssolve.c:782-800
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
    for (int i = 0; i < eps->nconv && !rc; i++) rc = pointwise(eps, ks_bv_col(eps->V, i), eps->D, ks_bv_col(T, i), false);
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

// ---- what the solvers share (ks_eps_impl.h) ----
double ks_eps_converged_estimate(ks_eps eps, double re, double im, double res) { return converged_estimate(eps, re, im, res); }
int ks_eps_synchronize_values(ks_eps eps, double *v, size_t count) { return ds_synchronize_values(eps, v, count); }
int ks_eps_stopping_call(ks_eps eps, int its, int nconv)
{
  int reason = KS_EPS_CONVERGED_ITERATING;
  if (eps->stop_fn) { const int rc = eps->stop_fn(eps, its, eps->max_it, nconv, eps->nev, &reason, eps->stop_ctx); KS_CHECK(!rc, rc, "the user's stopping test returned %d", rc); }
  else ks_eps_stopping_basic(eps, its, eps->max_it, nconv, eps->nev, &reason, nullptr);
  eps->reason = reason;
  return KS_SUCCESS;
}
int ks_eps_monitor_call(ks_eps eps, int its, int nconv, int nest)
{
  if (!eps->mon_fn) return KS_SUCCESS;
  const int rc = eps->mon_fn(eps, its, nconv, eps->eigr.data(), eps->eigi.data(), eps->errest.data(), nest, eps->mon_ctx);
  KS_CHECK(!rc, rc, "the user's monitor returned %d", rc);
  return KS_SUCCESS;
}
int ks_eps_matrix_norms(ks_eps eps) { return matrix_norms(eps); }

// EPSSetType epsbasic.c: Krylov-Schur (the default) or LOBPCG. LOBPCG makes STPRECOND the default of the solver's ST (EPSSetDefaultST_Precond
// epsdefault.c) unless the caller chose a type; going back to Krylov-Schur undoes that default
extern "C" int ks_eps_set_type(ks_eps eps, int type)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  KS_CHECK(type == KS_EPS_KRYLOVSCHUR || type == KS_EPS_LOBPCG, KS_ERR_SUP, "only EPSKRYLOVSCHUR and EPSLOBPCG are built");
  if (type == eps->type) return KS_SUCCESS;
  eps->type = type; eps->solved = false;
  if (type == KS_EPS_LOBPCG) {
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
