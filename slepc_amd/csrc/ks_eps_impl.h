// The EPS object and what crosses the files of its driver: ks_eps.hip (the object, the generic set-up, ks_eps_solve, results), ks_krylovschur.hip
// (both Krylov-Schur variants), ks_lobpcg.hip (LOBPCG), ks_gd.hip (Generalized Davidson), ks_jd.hip (Jacobi-Davidson) and ks_balance.hip (balancing of non-symmetric problems, the driver's only device code).
#pragma once
#include "ksgpu_internal.h"
#include "ks_ds.h"

using ksd::KsCompare;

// the settings of EPS_DAVIDSON that GD and JD share (davidson.h: blocksize, minv, plusk, initialsize, ipB; 0 / -1: the default), what the last set-up
// resolved them to and the counters of the last solve
struct KsDavidson { int bs = 0, minv = 0, plusk = -1, initv = 0; bool borth = true; int r_bs = 0, r_minv = 0, r_plusk = 0, r_initv = 0;
                    long long iterations = 0, restarts = 0, locks = 0, mat_columns = 0, pc_columns = 0, fused_residuals = 0; };

struct ks_eps_s {
  ks_ctx ctx = nullptr;
  ks_mat A = nullptr, B = nullptr;
  ks_mat op = nullptr;                 // operator of the expansion: A itself, or the ST's shell matrix
  // EPSSetBalance (non-symmetric problems): D from EPSBuildBalance_Krylov, the expansion then runs on D Op D^-1 (STApply with st->D, stsolve.c:252-256)
  int balance = KS_EPS_BALANCE_NONE, balance_its = 5; double balance_cutoff = 1e-8;
  double *D = nullptr, *wb = nullptr; int D_n = 0; ks_mat op_inner = nullptr, bal_op = nullptr; bool balanced = false;
  ks_st st = nullptr;                  // owned (EPSGetST)
  ks_bv V = nullptr, W = nullptr;      // basis (ncv+1 columns), work vectors (3 columns)
  int problem_type = 0;               // not set: EPSSetUp picks NHEP (one matrix) or GNHEP (two), epssetup.c:318-322
  int nev = 1, ncv = 0, mpd = 0, ncv_user = 0, mpd_user = 0;
  double tol = 1e-8; int max_it = 0, max_it_user = 0;
  KsCompare which;                     // user settings; cmp_ds / cmp_final are what a solve uses
  KsCompare cmp_ds, cmp_final;
  double keep = 0.5; bool lock = true;   // EPSKrylovSchurSetRestart / SetLocking
  uint64_t seed = 0x12345678ULL;
  std::vector<double> v0; bool have_v0 = false;
  ks_bv defl = nullptr; int nds = 0;       // deflation space handed over by EPSSetDeflationSpace, consumed by the next solve
  long long max_steps = 0;
  int ds_parallel = KS_DS_PARALLEL_SYNCHRONIZED;   // DSSetParallel: broadcast rank 0's projected solve after every restart (krylovschur.c:281)
  // results
  std::vector<double> eigr, eigi, errest; std::vector<int> perm;
  int nconv = 0, its = 0, reason = 0;
  long long steps = 0, passes = 0; int restarts = 0;
  long long passes0[2] = {0, 0};       // Gram-Schmidt pass counts of V and VL where this solve's count starts (eps->passes is the difference at its end)
  bool solved = false, ghep = false;
  ks_eps_converged_fn conv_fn = nullptr; void *conv_ctx = nullptr;     // EPSSetConvergenceTestFunction (conv = KS_EPS_CONV_USER)
  ks_eps_stopping_fn stop_fn = nullptr; void *stop_ctx = nullptr;      // EPSSetStoppingTestFunction; NULL = EPSStoppingBasic
  ks_eps_monitor_fn mon_fn = nullptr; void *mon_ctx = nullptr;         // EPSMonitorSet (one monitor)
  ks_eps_arbitrary_fn arb_fn = nullptr; void *arb_ctx = nullptr;       // EPSSetArbitrarySelection
  bool problem_type_resolved_hermitian = false;                        // the last solve ran the symmetric (Lanczos) variant
  bool vectors_done = true;                                            // non-symmetric variant: V holds Schur vectors until the eigenvectors are first asked for (EPS_STATE_EIGENVECTORS)
  int cb_err = 0;                                                      // first non-zero return of a user callback
  bool purify = true, trackall = false;                               // EPSSetPurify, EPSSetTrackAll
  bool trueres = false;                                          // EPSSetTrueResidual
  int extraction = KS_EPS_RITZ;                                  // EPSSetExtraction: Ritz or harmonic (krylovschur.c:120)
  int conv = KS_EPS_CONV_REL; double nrma = 0.0, nrmb = 0.0;   // EPSSetConvergenceTest; ||A||_inf, ||B||_inf for CONV_NORM / ERROR_BACKWARD
  ksd::DsHep dsh; ksd::DsNhep dsn;                                     // the projected problem of the last solve: the symmetric or the general variant
  // EPSSetTwoSided: the left basis (a duplicate of V), Op^T as a matrix (a view: ks_mat_create_transpose), the left start vector, DS NHEPTS
  bool twosided = false, twosided_solved = false;                      // the flag; the last solve ran the two-sided variant
  ks_bv VL = nullptr; ks_mat opT = nullptr; bool opT_owned = false;   // a shell view is this solver's to destroy; the view of an assembled matrix belongs to that matrix
  bool left_trivial = false;                                           // symmetric problem type: the left eigenvectors are the right ones (epssolve.c:585)
  std::vector<double> w0; bool have_w0 = false;
  ksd::DsNhepTs dst;
  // EPSSetType: KS_EPS_KRYLOVSCHUR or KS_EPS_LOBPCG (ks_lobpcg.hip). The LOBPCG settings (EPS_LOBPCG, lobpcg.c:33-38), its projected problem and counters
  int type = KS_EPS_KRYLOVSCHUR;
  struct { int bs = 0; double restart = 0.0; bool lock = true; long long iterations = 0, hard_locks = 0, mat_columns = 0, pc_columns = 0; } lob;
  ksd::DsGhep dsg;
  ks_bv ini = nullptr; int nini = 0;     // EPSSetInitialSpace: all the vectors (a block solver uses every one; the Krylov solvers use v0, the first)
  // KS_EPS_GD (ks_gd.hip): the settings of EPS_DAVIDSON that GD has (davidson.h: blocksize, minv, plusk, initialsize, ipB; 0 / -1: the default), what the
  // last set-up resolved them to, the counters of the last solve and its projected problem
  KsDavidson gd;
  ksd::DsGd dsd;
  // KS_EPS_JD (ks_jd.hip): its own copy of those settings and counters (jd.c keeps them in the same EPS_DAVIDSON, one solver type at a time; here a
  // change of type leaves the other type's settings alone), then what only JD has (jd.c: fix, const_correction_tol) and the counters of its inner solves
  KsDavidson jd;
  struct { double fix = 0.01; bool const_tol = true; long long inner_solves = 0, inner_iterations = 0, gd_fallbacks = 0; } jdx;
};

// the callbacks of a solve as every solver calls them (ks_eps.hip)
double ks_eps_converged_estimate(ks_eps eps, double re, double im, double res);   // (*eps->converged): EPSConvergedRelative / Absolute / Norm or the user's; a failing callback is kept in eps->cb_err
int ks_eps_stopping_call(ks_eps eps, int its, int nconv);                         // (*eps->stopping) into eps->reason
int ks_eps_monitor_call(ks_eps eps, int its, int nconv, int nest);                // EPSMonitor
int ks_eps_matrix_norms(ks_eps eps);                                              // ||A||_inf, ||B||_inf for KS_EPS_CONV_NORM (epssetup.c:345-358)
int ks_eps_synchronize_values(ks_eps eps, double *v, size_t count);               // rank 0's values to every rank under KS_DS_PARALLEL_SYNCHRONIZED
int ks_lobpcg_solve(ks_eps eps);                                                  // EPSSolve_LOBPCG, the solve of ks_lobpcg_ops (ks_lobpcg.hip)
// R(:,j) = AX(:,j) - theta[j] BX(:,j) for ncols <= 16 columns and their 2-norms over all ranks into norms (host), one kernel and one D2H (ks_lobpcg.hip)
int ksl_block_residual(ks_bv R, int ncols, const double *AX, long long ldax, const double *BX, long long ldbx, double *Rd, long long ldr, const double *theta, double *norms);

#pragma GCC visibility push(hidden)
// eps->ops of the reference, what ks_eps_solve asks of a solver. setup: its checks and dimension rules around eps_setup_common, its projected problem;
// solve: up to eps->nconv converged pairs in the leading columns of V; compute_vectors: what EPSSolve's epilogue does to them (NULL: nothing)
struct ks_eps_ops { int (*setup)(ks_eps); int (*solve)(ks_eps); int (*compute_vectors)(ks_eps); };
const ks_eps_ops *ks_krylovschur_ops(bool twosided);                              // ks_krylovschur.hip: the one-sided or the two-sided variant
const ks_eps_ops *ks_lobpcg_ops();                                                // ks_lobpcg.hip
const ks_eps_ops *ks_gd_ops();                                                    // ks_gd.hip
const ks_eps_ops *ks_jd_ops();                                                    // ks_jd.hip
int eps_setup_common(ks_eps eps, int ncv, ks_mat ip);                             // the generic part of EPSSetUp once a solver knows ncv and its inner product (ks_eps.hip)
int ks_eps_residual_norm(ks_eps eps, double kr, double ki, const double *xr, const double *xi, double xi_sign, double *out, bool trans = false);   // ks_eps.hip
int ks_eps_schur_vectors(ks_eps eps);                                             // EPSComputeVectors_Schur on first use of an eigenvector (ks_krylovschur.hip)
int ks_eps_pointwise(ks_eps eps, const double *a, const double *b, double *out, bool mul);   // ks_balance.hip: out = a .* b or a ./ b on n_local entries
int ks_eps_setup_balance(ks_eps eps);                                             // ks_balance.hip: D built (or the user's checked), eps->op = the shell D Op D^-1
#pragma GCC visibility pop
