// The dense projected eigenproblem of the Krylov-Schur driver (DS HEP and DS NHEP with extra row), the eigenvalue comparisons and
// the ST's back-transformation of eigenvalues: host scalars only, no device code and no HIP headers, so that it is part of the
// host-only library and tested on the CPU (tests/test_ds_host.py). The reference calls LAPACK steqr / lartg / BLAS rot for the
// m x m (m <= 64) symmetric problem; LAPACK is not part of this image's C toolchain, so the tridiagonal eigenproblem is solved by the
// implicit QL/QR iteration written out in ks_ds.cpp (same algorithm family as steqr; eigenvalues returned ascending as steqr does,
// so that the insertion sort of DSSort sees the same input order). The non-symmetric kernels are those of ks_dense.cpp.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>
#include "../../include/ksgpu.h"

namespace ksd {

// Givens rotation with LAPACK-3.10 dlartg conventions: c >= 0, r = sign(f)*hypot(f,g)
void lartg(double f, double g, double *c, double *s, double *r);
// BLAS drot on the first n entries of two columns
void rot(int n, double *x, double *y, double c, double s);
// Symmetric tridiagonal eigenproblem by implicit QL with Wilkinson shifts, accumulating the rotations
// into the columns of Z (Z <- Z * eigvecs), eigenvalues sorted ascending on exit (steqr 'V' contract).
// d[0..n), e[0..n-1) ; Z is ldz x n column-major with n rows used (nz rows updated).
int tridiag_ql(int n, double *d, double *e, double *Z, int ldz, int nz);

// What the eigenvalue map of an ST needs: its type, shift and (resolved) antishift; type < 0 is "no ST"
struct StMap {
  int type = -1; double sigma = 0.0, nu = 0.0;
  explicit operator bool() const { return type >= 0; }
  void backtransform(int n, double *eigr, double *eigi) const;      // STBackTransform stsolve.c:563
};

// SlepcCompare* (src/sys/slepcsc.c:152-300), real scalars; EPS_WHICH_USER calls the function installed with
// ks_eps_set_eigenvalue_comparison (EPSSetEigenvalueComparison epsopts.c:563)
struct KsCompare {
  int which = 0;                      // 0 = not set: resolved at set-up (EPSSetWhichEigenpairs_Default epsdefault.c:209-219)
  double target = 0.0;
  ks_eig_compare_fn fn = nullptr; void *fn_ctx = nullptr;
  StMap map;                          // SlepcMap_ST: compare the back-transformed values (SlepcSCCompare slepcsc.c:41-62)
};
int compare_eig(const KsCompare &cmp, double ar, double ai, double br, double bi);

enum { DS_RAW = 0, DS_INTERMEDIATE = 1, DS_CONDENSED = 2, DS_TRUNCATED = 3 };

// What the restart loop needs of a DS, whichever type it is
struct Ds {
  int ld = 0, n = 0, l = 0, k = 0, t = 0, state = DS_RAW; KsCompare which;
  std::vector<double> Q;              // DS_MAT_Q: the basis is multiplied with it
  virtual ~Ds() {}
  virtual void allocate(int ld_) = 0;
  virtual std::vector<double> &M() = 0;                                                     // DS_MAT_T / DS_MAT_A: filled by the expansion, synchronised together with Q
  void set_dimensions(int n_, int l_, int k_) { n = n_; t = n_; l = l_; k = k_; }           // dsops.c:130-165
  virtual int solve(double *wr, double *wi) = 0;
  // rr/ri: auxiliary values of an arbitrary selection (DSSort with rr: the order comes from them, dshep.c:335-336)
  virtual int sort(double *wr, double *wi, const double *rr = nullptr, const double *ri = nullptr) = 0;
  virtual void update_extra_row() = 0;
  virtual int truncate_size(int, int, int kk) { return kk; }                                // DSGetTruncateSize
  virtual void truncate(int nn, bool trim) = 0;
  // Ritz pair kk: coefficients of the Ritz vector in the basis (Zi for a conjugate pair, else NULL), rnorm = the factor of
  // the residual estimate; returns the index of the last column written (kk, or kk + 1 for a pair)
  virtual int ritz(int kk, double *rnorm, const double **Zr, const double **Zi) = 0;
};

// DS type HEP, compact storage with extra row (krylovschur.c:160-168)
struct DsHep : Ds {
  std::vector<double> T; std::vector<int> perm;
  void allocate(int ld_) override { ld = ld_; T.assign((size_t)3 * ld, 0.0); Q.assign((size_t)ld * ld, 0.0); perm.assign(ld, 0); }
  std::vector<double> &M() override { return T; }
  double *d() { return T.data(); }
  double *e() { return T.data() + ld; }
  void arrow_tridiag(int nn, double *dd, double *ee, double *QQ);                           // dshep.c:221-262
  int solve(double *wr, double *wi) override;                                               // dsops.c:723, dshep.c:383-426 (wi is not touched)
  int sort(double *wr, double *wi, const double *rr = nullptr, const double *ri = nullptr) override;   // dsops.c:329-345, dshep.c:323-347
  void update_extra_row() override { const double beta = e()[n - 1]; for (int i = 0; i < n; i++) e()[i] = beta * Q[(size_t)(n - 1) + (size_t)i * ld]; k = n; }   // dshep.c:349-381 (compact)
  void truncate(int nn, bool trim) override                                                 // dsops.c DSTruncate + dshep.c:643-671
  {
    if (trim) { l = 0; k = 0; n = nn; t = nn; state = DS_RAW; }
    else { k = nn; t = n; n = nn; state = DS_TRUNCATED; }
  }
  int ritz(int kk, double *rnorm, const double **Zr, const double **Zi) override            // DSVectors(X,kk) = Q(:,kk), rnorm = |Q(n-1,kk)| (dshep.c:140-155)
  { *rnorm = fabs(Q[(size_t)(n - 1) + (size_t)kk * ld]); *Zr = Q.data() + (size_t)kk * ld; *Zi = nullptr; return kk; }
};

// DS type NHEP with extra row (krylovschur.c:153-159): A is ld x ld column-major, row n holds the extra row.
struct DsNhep : Ds {
  std::vector<double> A, X;
  void allocate(int ld_) override { ld = ld_; A.assign((size_t)ld * ld, 0.0); Q.assign((size_t)ld * ld, 0.0); X.assign((size_t)ld * ld, 0.0); }
  std::vector<double> &M() override { return A; }
  double &a(int i, int j) { return A[(size_t)i + (size_t)j * ld]; }
  double &q(int i, int j) { return Q[(size_t)i + (size_t)j * ld]; }
  // DSTranslateHarmonic_NHEP dsnhep.c:466-537. g (ld entries) lives in the caller between the two calls. Forward:
  // g = (A - tau I)^{-T} (beta e_n) and A(:,n-1) += beta g. Recover (after solve and sort, with l = converged and
  // k = kept): the rank-one term is removed from the kept block and g is projected out of the kept Schur vectors.
  int translate_harmonic(double tau, double beta, bool recover, double *g, double *gamma_out);
  void eig_from_T(double *wr, double *wi, int j0, int j1);                                  // dsutil.c:65-79,160-170
  int solve(double *wr, double *wi) override;                                               // dsutil.c:21-91
  int sort(double *wr, double *wi, const double *rr = nullptr, const double *ri = nullptr) override;   // dsutil.c:93-175 (rr/ri are not used)
  void update_extra_row() override;                                                         // dsnhep.c:318-341
  // k-th eigenvector of A back-transformed with Q (or not), normalised, into X(:,k[,k+1]); returns the index of the
  // last column written; rnorm = |last component| (dsnhep.c:101-167)
  int vectors(int kk, bool back, double *rnorm);
  int truncate_size(int ll, int nn, int kk) override { if (a(ll + kk, ll + kk - 1) != 0.0) kk = (ll + kk < nn - 1) ? kk + 1 : kk - 1; return kk; }   // do not split a 2x2 block (dsops.c:329-345)
  void truncate(int nn, bool trim) override;                                                // dsnhep.c:385-415
  int ritz(int kk, double *rnorm, const double **Zr, const double **Zi) override
  {
    const int newk = vectors(kk, true, rnorm);
    *Zr = X.data() + (size_t)kk * ld; *Zi = newk == kk + 1 ? X.data() + (size_t)newk * ld : nullptr;
    return newk;
  }
};

// DS type NHEPTS (dsnhepts.c), the projected problem of the two-sided solver: two NHEP halves that are solved, sorted, updated and truncated
// together. This object is the first half (A, Q, X: the Arnoldi relation of Op); `hb` is the second (its A, Q, X are DS_MAT_B, DS_MAT_Z,
// DS_MAT_Y: the relation of Op^T) with its own eigenvalues wr2 / wi2. Dimensions and state live here and are copied to hb before every step.
struct DsNhepTs : DsNhep {
  DsNhep hb;
  std::vector<double> wr2, wi2;
  long long permuted = 0;                                                                   // sorts that had to reorder the second half to match the first
  void allocate(int ld_) override { DsNhep::allocate(ld_); hb.allocate(ld_); wr2.assign(ld_, 0.0); wi2.assign(ld_, 0.0); }
  void dims_to_b() { hb.n = n; hb.l = l; hb.k = k; hb.t = t; hb.state = state; hb.which = which; }
  int solve(double *wr, double *wi) override;                                               // dsnhepts.c:275-286
  // both halves with the same comparison, then the correspondence check and, where the orders differ, the greedy nearest-value permutation
  // applied to the second half (dsnhepts.c:193-242). Returns 0, 1 (a swap was rejected) or 2 (the permutation would split a 2x2 block)
  int sort(double *wr, double *wi, const double *rr = nullptr, const double *ri = nullptr) override;
  int sort_with_permutation(int *perm);                                                     // DSSortWithPermutation_NHEP_Private dsutil.c:177-237 on the second half
  void update_extra_row() override { dims_to_b(); DsNhep::update_extra_row(); hb.update_extra_row(); }   // dsnhepts.c:244-273
  int truncate_size(int ll, int nn, int kk) override                                        // a 2x2 block of either half (dsnhepts.c:353-371)
  { if (a(ll + kk, ll + kk - 1) != 0.0 || hb.a(ll + kk, ll + kk - 1) != 0.0) kk = (ll + kk < nn - 1) ? kk + 1 : kk - 1; return kk; }
  void truncate(int nn, bool trim) override { dims_to_b(); DsNhep::truncate(nn, trim); hb.truncate(nn, trim); }   // dsnhepts.c:373-406
  // DSVectors(DS_MAT_X or DS_MAT_Y, kk): left = the eigenvector of the second half back-transformed with Z, into hb.X (dsnhepts.c:54-119)
  int vectors_side(int kk, bool left, bool back, double *rnorm) { if (!left) return vectors(kk, back, rnorm); dims_to_b(); return hb.vectors(kk, back, rnorm); }
};

// DS type GHEP (src/sys/classes/ds/impls/ghep/dsghep.c): A q = theta B q for symmetric A and symmetric positive definite B of order n <= ld, the
// projected problem of LOBPCG (lobpcg.c:145-158, 350-365). The reference calls LAPACK sygvd (dsghep.c:115-170); here B = U^T U (potrf_upper), the
// reduction C = U^-T A U^-1 by triangular substitution (what sygst does), sym_eig of C and Q = U^-1 Z, so Q^T B Q = I. Not part of the Ds
// hierarchy above: no extra row, no truncation, nothing a restart loop would ask of it.
struct DsGhep {
  int ld = 0, n = 0; KsCompare which;
  std::vector<double> A, B, Q;        // DS_MAT_A, DS_MAT_B (full symmetric matrices; the upper triangle of B and the lower one of the reduced A are read), DS_MAT_Q = DS_MAT_X
  void allocate(int ld_) { ld = ld_; A.assign((size_t)ld * ld, 0.0); B.assign((size_t)ld * ld, 0.0); Q.assign((size_t)ld * ld, 0.0); }
  double &a(int i, int j) { return A[(size_t)i + (size_t)j * ld]; }
  double &b(int i, int j) { return B[(size_t)i + (size_t)j * ld]; }
  // DSSolve_GHEP: w ascending, Q B-orthonormal; A and B are left as they came. Returns 0, k > 0 when the leading minor of order k of B is not
  // positive definite (potrf's info: the caller's breakdown), -1 when the Jacobi iteration of the reduced problem failed
  int solve(double *w);
  void sort(double *w);               // DSSort_GHEP dsghep.c:172-195: eigenvalues and the columns of Q in the order of `which`
};

// The projected problem of Generalized Davidson (ks_gd.hip): H = V^T A V of the active search columns - a standard symmetric problem, the basis being
// B-orthonormal -, its eigenvectors Q in the order of `which`, and the Q of the previous iteration (oldU, dvdupdatev.c:297-307) for the thick restart
// with "+k" vectors. Host only and outside the Ds hierarchy, like DsGhep: the order changes at every step (grow, lock, restart), there is no extra row.
// All three matrices are ld x ld column-major; oldU has order size_oldU and counts as zero-padded to the current order n.
struct DsGd {
  int ld = 0, n = 0, size_oldU = 0; KsCompare which;
  std::vector<double> H, Q, oldU, w;
  void allocate(int ld_) { ld = ld_; n = 0; size_oldU = 0; H.assign((size_t)ld * ld, 0.0); Q.assign((size_t)ld * ld, 0.0); oldU.assign((size_t)ld * ld, 0.0); w.assign(ld, 0.0); }
  double &h(int i, int j) { return H[(size_t)i + (size_t)j * ld]; }
  double &q(int i, int j) { return Q[(size_t)i + (size_t)j * ld]; }
  // nnew new search columns: C (ldc x nnew) holds V^T A v for each, n + nnew rows (the new order); H keeps both triangles (dvdcalcpairs.c:372-418)
  void grow(int nnew, const double *C, int ldc);
  // H = Q diag(w) Q^T with w and the columns of Q in the order of `which` (DSSolve + DSSort, dvdcalcpairs.c:497-521); H is kept. Non-zero: sym_eig failed
  int solve_sort();
  // the leading npre pairs leave (dvd_updateV_conv_gen, dvdupdatev.c:82-149): the basis having been rotated by Q, H is the diagonal of the other Ritz values
  void lock(int npre);
  void save_oldU();                                                                         // oldU <- Q (dvdupdatev.c:297-307)
  // Z = orth([Q(:, 0:size_X), oldU(:, 0:size_plusk)]) (n x kept into Z, ldz >= n): DSOrthogonalize's contract as dvd_updateV_restart_gen uses it
  // (dvdupdatev.c:151-224) - orthonormal columns spanning the block, dependent columns dropped, the kept count returned. Gram-Schmidt with one
  // re-orthogonalisation; a column is dependent when what is left of it is below 64 n eps of its norm (what two passes leave of a column of the span)
  int restart_basis(int size_X, int size_plusk, double *Z, int ldz) const;
  void project(const double *Z, int ldz, int kept);                                         // H <- Z^T H Z of order kept; oldU is forgotten
};

} // namespace ksd
