// What Generalized Davidson (ks_gd.hip) and Jacobi-Davidson (ks_jd.hip) share, as the reference's two solvers share src/eps/impls/davidson: one outer
// loop (Gd::solve, ks_gd.hip) and one set-up; the solvers differ in the "improve X" step alone (dvdimprovex.c), here Gd::correction.
#pragma once
#include "ksgpu_internal.h"
#include "ks_eps_impl.h"

#pragma GCC visibility push(hidden)
struct Gd {
  ks_eps eps; ks_ctx ctx; ks_mat A, B; ks_st st;
  KsDavidson *cfg = nullptr;            // the settings and counters of the solver type that runs (eps->gd or eps->jd)
  ks_bv V = nullptr, AV = nullptr, BV = nullptr, R = nullptr;
  int bs = 1, mpd = 0, minv = 0, plusk = 0, initv = 0, ncv = 0, nev = 0;
  int nconv = 0, m = 0, mprod = 0;      // locked columns of V; active search columns behind them; how many of those have their images in AV (and BV)
  // JD: the Ritz-residual sweep also stores the Ritz vectors x_j (Xo) and B x_j (BXo) of the block, from column nconv of those BVs (NULL: GD, the
  // sweep of ks_bv_ritz_residual as it is)
  ks_bv Xo = nullptr, BXo = nullptr;
  virtual ~Gd() { ks_bv_destroy(AV); ks_bv_destroy(BV); ks_bv_destroy(R); }

  int make(int cols, ks_bv *out);        // a work BV in the layout of the solution basis; products of its columns as a block (ks_mat_mult_multi)
  int random_column();
  int orthonormalize_new(bool *kept);
  int rotate(const double *Z, int ldz, int cols, int shift);
  int solve();
  // The expansion vectors of the nb best pairs (theta[j], residual R(:,j) of norm rnorm[j]) into V(:, base + j). GD (dvd_improvex_gd2): D = M^-1 R
  virtual int correction(int nb, const double *theta, const double *rnorm, int base);
  virtual void locked(int npre) { (void)npre; }     // npre pairs have just been locked (nconv counts them already)
};

// EPSSetUp_XD with GD's rules on the settings `cfg` of the solver type `name` ("GD", "JD"); ks_gd.hip
int ks_davidson_setup(ks_eps eps, KsDavidson &cfg, const char *name);
int ks_davidson_solve(ks_eps eps, KsDavidson &cfg, Gd &s);       // EPSSolve_XD with the solver object of the type (a Gd, or its JD subclass)
// the rules of the settings both types have, on the type's own copy
int ks_davidson_set_blocksize(ks_eps eps, KsDavidson &cfg, int bs);
int ks_davidson_set_restart(ks_eps eps, KsDavidson &cfg, int minv, int plusk);
void ks_davidson_get_restart(const KsDavidson &cfg, int *minv, int *plusk);
int ks_davidson_set_initial_size(ks_eps eps, KsDavidson &cfg, int initialsize);
// the sweep behind ks_bv_ritz_residual and ks_bv_ritz_residual_vectors on raw column pointers (ks_gd.hip); Xd, BXd NULL: not stored
int ks_ritz_residual(ks_bv R, double *Rd, ks_bv Vs, const double *Vd, long long ldv, const double *AVd, long long ldav, const double *BVd, long long ldbv, int m,
                     const double *S, int lds, int ncols, const double *theta, double *rnorm, double *xnorm, double *Xd = nullptr, long long ldx = 0, double *BXd = nullptr, long long ldbx = 0);
#pragma GCC visibility pop
