// The dense projected eigenproblem of the Krylov-Schur driver on host scalars: see ks_ds.h.
#include "ks_ds.h"
#include "ks_dense.h"
#include <algorithm>
#include <cmath>
#include <limits>

namespace ksd {

// ---- small dense kernels ---------------------------------------------------------------------------
void lartg(double f, double g, double *c, double *s, double *r)
{
  if (g == 0.0) { *c = 1.0; *s = 0.0; *r = f; }
  else if (f == 0.0) { *c = 0.0; *s = (g < 0.0) ? -1.0 : 1.0; *r = fabs(g); }
  else { const double d = hypot(f, g); *c = fabs(f) / d; *r = copysign(d, f); *s = g / *r; }
}

void rot(int n, double *x, double *y, double c, double s)
{
  for (int i = 0; i < n; i++) { const double t = c * x[i] + s * y[i]; y[i] = c * y[i] - s * x[i]; x[i] = t; }
}

int tridiag_ql(int n, double *d, double *e, double *Z, int ldz, int nz)
{
  if (n <= 1) return 0;
  std::vector<double> ee(n, 0.0);
  for (int i = 0; i < n - 1; i++) ee[i] = e[i];
  const double eps = std::numeric_limits<double>::epsilon();
  for (int l = 0; l < n; l++) {
    int iter = 0, mm;
    do {
      for (mm = l; mm < n - 1; mm++) {
        const double dd = fabs(d[mm]) + fabs(d[mm + 1]);
        if (fabs(ee[mm]) <= eps * dd) break;
      }
      if (mm != l) {
        if (iter++ == 60 * 4) return l + 1;
        double g = (d[l + 1] - d[l]) / (2.0 * ee[l]);
        double r = hypot(g, 1.0);
        g = d[mm] - d[l] + ee[l] / (g + copysign(r, g));
        double s = 1.0, c = 1.0, p = 0.0;
        int i;
        for (i = mm - 1; i >= l; i--) {
          double f = s * ee[i];
          const double b = c * ee[i];
          r = hypot(f, g);
          ee[i + 1] = r;
          if (r == 0.0) { d[i + 1] -= p; ee[mm] = 0.0; break; }
          s = f / r; c = g / r;
          g = d[i + 1] - p;
          r = (d[i] - g) * s + 2.0 * c * b;
          p = s * r;
          d[i + 1] = g + p;
          g = c * r - b;
          for (int k = 0; k < nz; k++) {
            double *zk = Z + k;
            f = zk[(size_t)(i + 1) * ldz];
            zk[(size_t)(i + 1) * ldz] = s * zk[(size_t)i * ldz] + c * f;
            zk[(size_t)i * ldz] = c * zk[(size_t)i * ldz] - s * f;
          }
        }
        if (r == 0.0 && i >= l) continue;
        d[l] -= p; ee[l] = g; ee[mm] = 0.0;
      }
    } while (mm != l);
  }
  // selection sort, ascending, swapping eigenvector columns (dsteqr epilogue)
  for (int ii = 1; ii < n; ii++) {
    const int i = ii - 1; int k = i; double p = d[i];
    for (int j = ii; j < n; j++) if (d[j] < p) { k = j; p = d[j]; }
    if (k != i) { d[k] = d[i]; d[i] = p; for (int r = 0; r < nz; r++) std::swap(Z[r + (size_t)i * ldz], Z[r + (size_t)k * ldz]); }
  }
  for (int i = 0; i < n - 1; i++) e[i] = 0.0;
  return 0;
}

void StMap::backtransform(int n, double *eigr, double *eigi) const
{
  if (type < 0) return;
  for (int j = 0; j < n; j++) {
    if (type == KS_ST_SHIFT) eigr[j] += sigma;                                           // shift.c:49-56
    else if (type == KS_ST_CAYLEY) {                                                      // cayley.c:79-107
      if (eigi[j] == 0.0) eigr[j] = (nu + eigr[j] * sigma) / (eigr[j] - 1.0);
      else {
        // lambda = (nu + theta sigma) / (theta - 1) for theta = a + b i. Stated deviation: cayley.c:93-99 forms the denominator
        // |theta - 1|^2 = b^2 + a (a - 2) + 1 AFTER it has overwritten a and b with the numerator; here it is taken from theta.
        const double a = eigr[j], b = eigi[j];
        const double t = b * b + a * (a - 2.0) + 1.0;
        eigr[j] = (sigma * (a * a + b * b - a) + nu * (a - 1.0)) / t;
        eigi[j] = (-sigma * b - nu * b) / t;
      }
    }
    else if (eigi[j] == 0.0) eigr[j] = 1.0 / eigr[j] + sigma;                             // sinvert.c:16-40
    else { const double t = eigr[j] * eigr[j] + eigi[j] * eigi[j]; eigr[j] = eigr[j] / t + sigma; eigi[j] = -eigi[j] / t; }
  }
}

int compare_eig(const KsCompare &cmp, double ar, double ai, double br, double bi)
{
  double a, b;
  if (cmp.map) { cmp.map.backtransform(1, &ar, &ai); cmp.map.backtransform(1, &br, &bi); }
  switch (cmp.which) {
    case KS_EPS_LARGEST_MAGNITUDE:  a = hypot(ar, ai); b = hypot(br, bi); return a < b ? 1 : (a > b ? -1 : 0);
    case KS_EPS_SMALLEST_MAGNITUDE: a = hypot(ar, ai); b = hypot(br, bi); return a > b ? 1 : (a < b ? -1 : 0);
    case KS_EPS_LARGEST_REAL:       return ar < br ? 1 : (ar > br ? -1 : 0);
    case KS_EPS_SMALLEST_REAL:      return ar > br ? 1 : (ar < br ? -1 : 0);
    case KS_EPS_LARGEST_IMAGINARY:  a = fabs(ai); b = fabs(bi); return a < b ? 1 : (a > b ? -1 : 0);
    case KS_EPS_SMALLEST_IMAGINARY: a = fabs(ai); b = fabs(bi); return a > b ? 1 : (a < b ? -1 : 0);
    case KS_EPS_TARGET_MAGNITUDE:   a = hypot(ar - cmp.target, ai); b = hypot(br - cmp.target, bi); return a > b ? 1 : (a < b ? -1 : 0);
    case KS_EPS_TARGET_REAL:        a = fabs(ar - cmp.target); b = fabs(br - cmp.target); return a > b ? 1 : (a < b ? -1 : 0);
    case KS_EPS_WHICH_USER: { int r = 0; cmp.fn(ar, ai, br, bi, &r, cmp.fn_ctx); return r; }
  }
  return 0;
}

// ---- DS HEP ----------------------------------------------------------------------------------------
void DsHep::arrow_tridiag(int nn, double *dd, double *ee, double *QQ)
{
  if (nn <= 2) return;
  for (int j = 0; j < nn - 2; j++) {
    double c, s, temp = ee[j + 1];
    lartg(temp, ee[j], &c, &s, &ee[j + 1]);
    s = -s;
    temp = dd[j + 1];
    ee[j] = c * s * (temp - dd[j]);
    dd[j + 1] = s * s * dd[j] + c * c * temp;
    dd[j] = c * c * dd[j] + s * s * temp;
    const int j2 = j + 2;
    rot(j2, QQ + (size_t)j * ld, QQ + (size_t)(j + 1) * ld, c, s);
    for (int i = j - 1; i >= 0; i--) {
      const double off = -s * ee[i];
      ee[i] = c * ee[i];
      temp = ee[i + 1];
      lartg(temp, off, &c, &s, &ee[i + 1]);
      s = -s;
      temp = (dd[i] - dd[i + 1]) * s - 2.0 * c * ee[i];
      const double p = s * temp;
      dd[i + 1] += p;
      dd[i] -= p;
      ee[i] = -ee[i] - c * temp;
      rot(j2, QQ + (size_t)i * ld, QQ + (size_t)(i + 1) * ld, c, s);
    }
  }
}

int DsHep::solve(double *wr, double *)
{
  if (state >= DS_CONDENSED) return 0;
  const int n1 = n - l; const size_t off = (size_t)l + (size_t)l * ld;
  std::fill(Q.begin(), Q.end(), 0.0);
  for (int i = 0; i < ld; i++) Q[(size_t)i + (size_t)i * ld] = 1.0;                       // DSSetIdentity
  if (state < DS_INTERMEDIATE) arrow_tridiag(std::max(0, k - l + 1), d() + l, e() + l, Q.data() + off);   // DSIntermediate_HEP
  for (int i = 0; i < l; i++) wr[i] = d()[i];
  int info = tridiag_ql(n1, d() + l, e() + l, Q.data() + off, ld, n1);
  if (info) return info;
  for (int i = l; i < n; i++) wr[i] = d()[i];
  for (int i = 0; i < n - 1; i++) e()[i] = 0.0;                                           // compact: zero e(0:n-2), keep e(n-1)
  state = DS_CONDENSED;
  return 0;
}

int DsHep::sort(double *wr, double *, const double *rr, const double *ri)
{
  for (int i = 0; i < n; i++) perm[i] = i;
  double *dd = d();
  const double *key = rr ? rr : dd;
  auto im = [&](int i) { return ri ? ri[i] : 0.0; };
  // DSSortEigenvaluesReal_Private dspriv.c:224-243 / DSSortEigenvalues_Private :172-222: insertion sort of the first t values from l
  for (int i = l + 1; i < t; i++) {
    const double re = key[perm[i]], rim = im(perm[i]);
    int j = i - 1;
    int result = compare_eig(which, re, rim, key[perm[j]], im(perm[j]));
    while (result < 0 && j >= l) {
      std::swap(perm[j], perm[j + 1]); j--;
      if (j >= l) result = compare_eig(which, re, rim, key[perm[j]], im(perm[j]));
    }
  }
  for (int i = l; i < n; i++) wr[i] = dd[perm[i]];
  // DSPermuteColumns_Private dspriv.c:248-270
  for (int i = l; i < n; i++) {
    const int p = perm[i];
    if (p != i) {
      int j = i + 1;
      while (perm[j] != i) j++;
      perm[j] = p; perm[i] = i;
      for (int r = 0; r < n; r++) std::swap(Q[(size_t)r + (size_t)p * ld], Q[(size_t)r + (size_t)i * ld]);
    }
  }
  for (int i = l; i < n; i++) dd[i] = wr[i];
  return 0;
}

// ---- DS NHEP, on top of the host kernels of ks_dense.cpp --------------------------------------------
int DsNhep::translate_harmonic(double tau, double beta, bool recover, double *g, double *gamma_out)
{
  if (!recover) {
    std::vector<double> W((size_t)n * n);
    for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) W[i + (size_t)j * n] = a(i, j) - (i == j ? tau : 0.0);
    std::fill(g, g + ld, 0.0); g[n - 1] = beta;
    if (lu_solve_trans(n, W.data(), n, g)) return 1;                                       // getrf + getrs 'C'
    for (int i = 0; i < n; i++) a(i, n - 1) += g[i] * beta;
  } else {
    const int ncol = l + k;
    std::vector<double> ghat(ncol);
    for (int j = 0; j < ncol; j++) { double s2 = 0.0; for (int i = 0; i < n; i++) s2 += q(i, j) * g[i]; ghat[j] = -s2; }   // gemv 'C', alpha = -1
    for (int i = 0; i < ncol; i++) for (int j = l; j < ncol; j++) a(i, j) += ghat[i] * q(n - 1, j) * beta;
    for (int j = 0; j < ncol; j++) { const double t2 = ghat[j]; if (t2 != 0.0) for (int i = 0; i < n; i++) g[i] += t2 * q(i, j); }   // gemv 'N'
  }
  double scale = 0.0, ssq = 1.0;                                                           // dnrm2
  for (int i = 0; i < n; i++) if (g[i] != 0.0) { const double ax = fabs(g[i]); if (scale < ax) { ssq = 1.0 + ssq * (scale / ax) * (scale / ax); scale = ax; } else ssq += (ax / scale) * (ax / scale); }
  const double gamma = hypot(1.0, scale * sqrt(ssq));                                      // SlepcAbs(1.0, nrm2)
  if (gamma_out) *gamma_out = gamma;
  if (recover) for (int j = l; j < l + k; j++) a(n, j) *= gamma;                           // extra row
  return 0;
}

void DsNhep::eig_from_T(double *wr, double *wi, int j0, int j1)
{
  for (int j = j0; j < j1; j++) {
    if (j == n - 1 || a(j + 1, j) == 0.0) { wr[j] = a(j, j); wi[j] = 0.0; }
    else {
      wr[j] = a(j, j); wr[j + 1] = a(j, j);
      wi[j] = sqrt(fabs(a(j + 1, j))) * sqrt(fabs(a(j, j + 1))); wi[j + 1] = -wi[j];
      j++;
    }
  }
}

int DsNhep::solve(double *wr, double *wi)
{
  if (state >= DS_CONDENSED) return 0;
  std::fill(Q.begin(), Q.end(), 0.0);
  for (int i = 0; i < n; i++) q(i, i) = 1.0;
  if (n == 1) { wr[0] = a(0, 0); wi[0] = 0.0; state = DS_CONDENSED; return 0; }
  if (state < DS_INTERMEDIATE) hess_reduce(n, l, A.data(), ld, Q.data());                  // gehrd + orghr
  const int info = real_schur(n, l, A.data(), ld, wr, wi, Q.data());                       // hseqr 'S','V'
  if (info) return info;
  eig_from_T(wr, wi, 0, l);
  state = DS_CONDENSED;
  return 0;
}

int DsNhep::sort(double *wr, double *wi, const double *, const double *)
{
  for (int i = l; i < n - 1; i++) {
    double re = wr[i], im = wi[i];
    int pos = 0;
    for (int j = (im != 0.0) ? i + 2 : i + 1; j < n; j++) {
      if (compare_eig(which, re, im, wr[j], wi[j]) > 0) { re = wr[j]; im = wi[j]; pos = j; }
      if (wi[j] != 0.0) j++;
    }
    if (pos) {
      if (trexc_up(n, A.data(), ld, Q.data(), pos, i)) return 1;                           // trexc 'V', ifst=pos+1, ilst=i+1
      eig_from_T(wr, wi, i, n);
    }
    if (wi[i] != 0.0) i++;
  }
  return 0;
}

void DsNhep::update_extra_row()
{
  std::vector<double> x(n);
  for (int j = 0; j < n; j++) x[j] = a(n, j);
  for (int j = 0; j < n; j++) { double s = 0.0; for (int i = 0; i < n; i++) s += q(i, j) * x[i]; a(n, j) = s; }
  k = n;
}

int DsNhep::vectors(int kk, bool back, double *rnorm)
{
  std::vector<double> xr_(n + 1), xi_(n + 1), zr_(n + 1), zi_(n + 1);
  double *xr = xr_.data(), *xi = xi_.data(), *zr = zr_.data(), *zi = zi_.data();
  const bool cplx = trevc_one(n, A.data(), ld, kk, xr, xi) != 0;
  for (int i = 0; i < n; i++) {
    if (back) { double sr = 0.0, si = 0.0; for (int j = 0; j < n; j++) { sr += q(i, j) * xr[j]; si += q(i, j) * xi[j]; } zr[i] = sr; zi[i] = si; }
    else { zr[i] = xr[i]; zi[i] = xi[i]; }
  }
  double nr = 0.0, ni = 0.0;
  for (int i = 0; i < n; i++) { nr = hypot(nr, zr[i]); ni = hypot(ni, zi[i]); }
  const double norm = cplx ? hypot(nr, ni) : nr;
  for (int i = 0; i < n; i++) { X[(size_t)i + (size_t)kk * ld] = zr[i] / norm; if (cplx) X[(size_t)i + (size_t)(kk + 1) * ld] = zi[i] / norm; }
  if (rnorm) *rnorm = cplx ? hypot(zr[n - 1] / norm, zi[n - 1] / norm) : fabs(zr[n - 1] / norm);
  return cplx ? kk + 1 : kk;
}

void DsNhep::truncate(int nn, bool trim)
{
  if (trim) {
    for (int j = l; j < n; j++) a(n, j) = 0.0;
    l = 0; k = 0; n = nn; t = nn; state = DS_RAW;
  } else {
    if (k == n) { for (int j = l; j < nn; j++) a(nn, j) = a(n, j); for (int j = l; j < n; j++) a(n, j) = 0.0; }
    k = nn; t = n; n = nn; state = DS_TRUNCATED;
  }
}

// ---- DS NHEPTS: two NHEP halves ----------------------------------------------------------------------
int DsNhepTs::solve(double *wr, double *wi)
{
  dims_to_b();                                                                             // with the state the first half starts from
  const int info = DsNhep::solve(wr, wi);
  if (info) return info;
  return hb.solve(wr2.data(), wi2.data());
}

int DsNhepTs::sort_with_permutation(int *perm)
{
  double *T = hb.A.data(), *Z = hb.Q.data();
  auto t = [&](int i, int j) -> double & { return T[(size_t)i + (size_t)j * ld]; };
  for (int i = l; i < n - 1; i++) {
    const int pos = perm[i];
    const int inc = (pos < n - 1 && t(pos + 1, pos) != 0.0) ? 2 : 1;
    if (pos != i) {
      if (pos < i) return 2;                                                               // blocks only move upward
      if (!((t(pos, pos - 1) == 0.0 || perm[i + 1] == pos - 1) && (pos == n - 1 || t(pos + 1, pos) == 0.0 || perm[i + 1] == pos + 1))) return 2;   // "Invalid permutation due to a 2x2 block"
                                                                                           // (stated deviation: dsutil.c:202 also reads T(n,n-1) for pos = n-1, which is the extra row)
      if (trexc_up(n, T, ld, Z, pos, i)) return 1;                                         // trexc 'V', ifst = pos+1, ilst = i+1
      for (int j = i + 1; j < n; j++) if (perm[j] >= i && perm[j] < pos) perm[j] += inc;
      perm[i] = i;
      if (inc == 2) perm[i + 1] = i + 1;
    }
    if (inc == 2) i++;
  }
  hb.n = n; hb.eig_from_T(wr2.data(), wi2.data(), l, n);
  return 0;
}

int DsNhepTs::sort(double *wr, double *wi, const double *, const double *)
{
  int info = DsNhep::sort(wr, wi);
  if (info) return info;
  dims_to_b();
  info = hb.sort(wr2.data(), wi2.data());
  if (info) return info;
  // check correct eigenvalue correspondence
  const double sqeps = sqrt(std::numeric_limits<double>::epsilon());
  std::vector<int> idx(n), idx2(n), p(n, -1);
  int cont = 0;
  for (int i = 0; i < n; i++) if (hypot(wr2[i] - wr[i], wi2[i] - wi[i]) > sqeps) { idx2[cont] = i; idx[cont++] = i; }
  if (!cont) return 0;
  int id = 0;
  for (int i = 0; i < cont; i++) {
    double tmin = std::numeric_limits<double>::max();
    for (int j = 0; j < cont; j++) {
      if (idx2[j] == -1) continue;
      const double s = hypot(wr2[idx[j]] - wr[idx[i]], wi2[idx[j]] - wi[idx[i]]);
      if (s < tmin) { id = j; tmin = s; }
    }
    p[idx[i]] = idx[id];
    idx2[id] = -1;
  }
  for (int i = 0; i < n; i++) if (p[i] == -1) p[i] = i;
  permuted++;
  return sort_with_permutation(p.data());
}

// ---- DS GHEP ---------------------------------------------------------------------------------------
int DsGhep::solve(double *w)
{
  if (n <= 0) return 0;
  std::vector<double> U((size_t)n * n), C((size_t)n * n);
  for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) { U[(size_t)i + (size_t)j * n] = i <= j ? b(i, j) : 0.0; C[(size_t)i + (size_t)j * n] = a(i, j); }
  const int info = potrf_upper(n, U.data(), n);
  if (info) return info;
  auto u = [&](int i, int j) -> double { return U[(size_t)i + (size_t)j * n]; };
  // C <- U^-T C: forward substitution down every column; then C <- C U^-1: the same down every row (sygs2, itype 1, upper)
  for (int j = 0; j < n; j++) { double *c = C.data() + (size_t)j * n; for (int i = 0; i < n; i++) { double t = c[i]; for (int p = 0; p < i; p++) t -= u(p, i) * c[p]; c[i] = t / u(i, i); } }
  for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) { double t = C[(size_t)i + (size_t)j * n]; for (int p = 0; p < j; p++) t -= C[(size_t)i + (size_t)p * n] * u(p, j); C[(size_t)i + (size_t)j * n] = t / u(j, j); }
  for (int j = 0; j < n; j++) for (int i = j + 1; i < n; i++) { const double t = 0.5 * (C[(size_t)i + (size_t)j * n] + C[(size_t)j + (size_t)i * n]); C[(size_t)i + (size_t)j * n] = C[(size_t)j + (size_t)i * n] = t; }
  std::vector<double> C0(C);
  if (sym_eig(n, C.data(), n, w)) return -1;
  // One step of symmetric re-orthogonalisation, Z <- Z (I - (Z^T Z - I) / 2), in extended precision: the rotations leave Z^T Z - I at a few n eps,
  // the step squares that, so the B-orthonormality of Q = U^-1 Z is limited by the back substitution alone
  {
    std::vector<long double> E((size_t)n * n), Zn((size_t)n * n);
    for (int j = 0; j < n; j++) for (int i = 0; i <= j; i++) {
      long double t = 0.0L; for (int q = 0; q < n; q++) t += (long double)C[(size_t)q + (size_t)i * n] * C[(size_t)q + (size_t)j * n];
      if (i == j) t -= 1.0L;
      E[(size_t)i + (size_t)j * n] = E[(size_t)j + (size_t)i * n] = 0.5L * t;
    }
    for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) {
      long double t = C[(size_t)i + (size_t)j * n]; for (int q = 0; q < n; q++) t -= (long double)C[(size_t)i + (size_t)q * n] * E[(size_t)q + (size_t)j * n];
      Zn[(size_t)i + (size_t)j * n] = t;
    }
    for (size_t i = 0; i < Zn.size(); i++) C[i] = (double)Zn[i];
  }
  // Rayleigh quotients of the computed vectors, accumulated in extended precision: an eigenvector good to O(n eps) gives its eigenvalue to
  // O((n eps)^2) ||C||, so what is left is the rounding of this sum - the Jacobi sweeps alone leave a few ulps of ||C||
  for (int j = 0; j < n; j++) {
    const double *z = C.data() + (size_t)j * n;
    long double num = 0.0L, den = 0.0L;
    for (int q = 0; q < n; q++) { long double t = 0.0L; for (int i = 0; i < n; i++) t += (long double)C0[(size_t)i + (size_t)q * n] * z[i]; num += t * z[q]; den += (long double)z[q] * z[q]; }
    if (den > 0.0L) w[j] = (double)(num / den);
  }
  // Q = U^-1 Z: back substitution up every column
  for (int j = 0; j < n; j++) {
    double *z = C.data() + (size_t)j * n;
    for (int i = n - 1; i >= 0; i--) { double t = z[i]; for (int p = i + 1; p < n; p++) t -= u(i, p) * z[p]; z[i] = t / u(i, i); }
    for (int i = 0; i < n; i++) Q[(size_t)i + (size_t)j * ld] = z[i];
  }
  return 0;
}

void DsGhep::sort(double *w)
{
  // insertion sort, as DSSortEigenvalues_Private does it (dsutil.c): stable, so the ascending order of the solve survives among equals
  std::vector<int> perm(n);
  for (int i = 0; i < n; i++) perm[i] = i;
  for (int i = 1; i < n; i++) {
    const int pi = perm[i]; int j = i - 1;
    while (j >= 0 && compare_eig(which, w[perm[j]], 0.0, w[pi], 0.0) > 0) { perm[j + 1] = perm[j]; j--; }
    perm[j + 1] = pi;
  }
  std::vector<double> w2(w, w + n), Q2((size_t)n * n);
  for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) Q2[(size_t)i + (size_t)j * n] = Q[(size_t)i + (size_t)perm[j] * ld];
  for (int j = 0; j < n; j++) { w[j] = w2[perm[j]]; for (int i = 0; i < n; i++) Q[(size_t)i + (size_t)j * ld] = Q2[(size_t)i + (size_t)j * n]; }
}

// ---- the projected problem of Generalized Davidson ---------------------------------------------------
void DsGd::grow(int nnew, const double *C, int ldc)
{
  const int nn = n + nnew;
  for (int j = 0; j < nnew; j++) for (int i = 0; i < nn; i++) { const double v = C[(size_t)i + (size_t)j * ldc]; if (i <= n + j) { h(i, n + j) = v; h(n + j, i) = v; } }
  n = nn;
}

int DsGd::solve_sort()
{
  if (n <= 0) return 0;
  std::vector<double> Z((size_t)n * n), ww(n);
  for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) Z[(size_t)i + (size_t)j * n] = i >= j ? h(i, j) : h(j, i);
  if (sym_eig(n, Z.data(), n, ww.data())) return -1;
  // insertion sort as DSSortEigenvalues_Private does it: stable, the ascending order of the solve survives among equals
  std::vector<int> perm(n);
  for (int i = 0; i < n; i++) perm[i] = i;
  for (int i = 1; i < n; i++) {
    const int pi = perm[i]; int j = i - 1;
    while (j >= 0 && compare_eig(which, ww[perm[j]], 0.0, ww[pi], 0.0) > 0) { perm[j + 1] = perm[j]; j--; }
    perm[j + 1] = pi;
  }
  for (int j = 0; j < n; j++) { w[j] = ww[perm[j]]; for (int i = 0; i < n; i++) q(i, j) = Z[(size_t)i + (size_t)perm[j] * n]; }
  return 0;
}

void DsGd::lock(int npre)
{
  const int nn = n - npre;
  for (int j = 0; j < nn; j++) for (int i = 0; i < nn; i++) h(i, j) = i == j ? w[npre + j] : 0.0;
  for (int j = 0; j < nn; j++) w[j] = w[npre + j];
  n = nn; size_oldU = 0;
}

void DsGd::save_oldU()
{
  std::fill(oldU.begin(), oldU.end(), 0.0);
  for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) oldU[(size_t)i + (size_t)j * ld] = q(i, j);
  size_oldU = n;
}

int DsGd::restart_basis(int size_X, int size_plusk, double *Z, int ldz) const
{
  const double thr = 64.0 * n * std::numeric_limits<double>::epsilon();
  int kept = 0;
  std::vector<double> z(n);
  for (int c = 0; c < size_X + size_plusk; c++) {
    if (c < size_X) for (int i = 0; i < n; i++) z[i] = Q[(size_t)i + (size_t)c * ld];
    else for (int i = 0; i < n; i++) z[i] = (i < size_oldU && c - size_X < size_oldU) ? oldU[(size_t)i + (size_t)(c - size_X) * ld] : 0.0;
    double nrm0 = 0.0; for (int i = 0; i < n; i++) nrm0 += z[i] * z[i];
    nrm0 = sqrt(nrm0);
    for (int pass = 0; pass < 2; pass++)
      for (int k = 0; k < kept; k++) {
        const double *zk = Z + (size_t)k * ldz;
        double d = 0.0; for (int i = 0; i < n; i++) d += zk[i] * z[i];
        for (int i = 0; i < n; i++) z[i] -= d * zk[i];
      }
    double nrm = 0.0; for (int i = 0; i < n; i++) nrm += z[i] * z[i];
    nrm = sqrt(nrm);
    if (!(nrm > thr * nrm0)) continue;
    for (int i = 0; i < n; i++) Z[(size_t)i + (size_t)kept * ldz] = z[i] / nrm;
    kept++;
  }
  return kept;
}

void DsGd::project(const double *Z, int ldz, int kept)
{
  std::vector<double> T((size_t)n * kept), G((size_t)kept * kept);
  for (int j = 0; j < kept; j++) for (int i = 0; i < n; i++) { double t = 0.0; for (int p = 0; p < n; p++) t += H[(size_t)i + (size_t)p * ld] * Z[(size_t)p + (size_t)j * ldz]; T[(size_t)i + (size_t)j * n] = t; }
  for (int j = 0; j < kept; j++) for (int i = 0; i <= j; i++) { double t = 0.0; for (int p = 0; p < n; p++) t += Z[(size_t)p + (size_t)i * ldz] * T[(size_t)p + (size_t)j * n]; G[(size_t)i + (size_t)j * kept] = t; }
  for (int j = 0; j < kept; j++) for (int i = 0; i <= j; i++) { h(i, j) = G[(size_t)i + (size_t)j * kept]; h(j, i) = h(i, j); }
  n = kept; size_oldU = 0;
}

} // namespace ksd

#ifdef KSD_TEST_HOOKS
// C wrappers for tests/test_ds_host.py: one step of a DS on caller-owned arrays. dims = {n, l, k, t, state}, read and written back.
extern "C" {
struct ksd_cmp { int which; double target; ks_eig_compare_fn fn; int st_type; double sigma, nu; };
static void ksd_load(ksd::Ds &ds, int ld, const int *dims, const ksd_cmp *c, const double *M, const double *Q)
{
  ds.allocate(ld); ds.n = dims[0]; ds.l = dims[1]; ds.k = dims[2]; ds.t = dims[3]; ds.state = dims[4];
  ds.which.which = c->which; ds.which.target = c->target; ds.which.fn = c->fn; ds.which.map = ksd::StMap{c->st_type, c->sigma, c->nu};
  std::copy(M, M + ds.M().size(), ds.M().begin()); std::copy(Q, Q + ds.Q.size(), ds.Q.begin());
}
static void ksd_store(ksd::Ds &ds, int *dims, double *M, double *Q)
{
  dims[0] = ds.n; dims[1] = ds.l; dims[2] = ds.k; dims[3] = ds.t; dims[4] = ds.state;
  std::copy(ds.M().begin(), ds.M().end(), M); std::copy(ds.Q.begin(), ds.Q.end(), Q);
}
// the steps both types have: 0 solve, 1 sort (rr / ri may be NULL), 2 update_extra_row, 3 truncate(a0, trim = a1), 4 truncate_size(a0, a1, a2),
// 5 ritz(a0): returns the last column, out = {rnorm, offset of Zr in Q (HEP) or X (NHEP), offset of Zi or -1}
static int ksd_step(ksd::Ds &ds, const double *z0, int op, double *wr, double *wi, const double *rr, const double *ri, int a0, int a1, int a2, double *out)
{
  const double *Zr = nullptr, *Zi = nullptr; int rc = 0;
  switch (op) {
    case 0: return ds.solve(wr, wi);
    case 1: return ds.sort(wr, wi, rr, ri);
    case 2: ds.update_extra_row(); return 0;
    case 3: ds.truncate(a0, a1 != 0); return 0;
    case 4: return ds.truncate_size(a0, a1, a2);
    case 5: rc = ds.ritz(a0, &out[0], &Zr, &Zi); out[1] = (double)(Zr - z0); out[2] = Zi ? (double)(Zi - z0) : -1.0; return rc;
  }
  return -1;
}
int ksd_hep(int op, int ld, int *dims, double *T, double *Q, double *wr, double *wi, const ksd_cmp *c, const double *rr, const double *ri, int a0, int a1, int a2, double *out)
{
  ksd::DsHep ds; ksd_load(ds, ld, dims, c, T, Q);
  const int rc = ksd_step(ds, ds.Q.data(), op, wr, wi, rr, ri, a0, a1, a2, out);
  ksd_store(ds, dims, T, Q);
  return rc;
}
// beside the common steps: 6 vectors(a0, back = a1; out[0] = rnorm), 7 translate_harmonic(tau = x0, beta = x1, recover = a0, g; out[0] = gamma)
int ksd_nhep(int op, int ld, int *dims, double *A, double *Q, double *X, double *wr, double *wi, const ksd_cmp *c, int a0, int a1, int a2, double x0, double x1, double *g, double *out)
{
  ksd::DsNhep ds; ksd_load(ds, ld, dims, c, A, Q); std::copy(X, X + ds.X.size(), ds.X.begin());
  int rc;
  if (op == 6) rc = ds.vectors(a0, a1 != 0, &out[0]);
  else if (op == 7) rc = ds.translate_harmonic(x0, x1, a0 != 0, g, &out[0]);
  else rc = ksd_step(ds, ds.X.data(), op, wr, wi, nullptr, nullptr, a0, a1, a2, out);
  ksd_store(ds, dims, A, Q); std::copy(ds.X.begin(), ds.X.end(), X);
  return rc;
}
// the two-sided DS on caller-owned arrays (B, Z, Y, wr2, wi2: the second half). Steps 0-4 as above; 6 vectors(a0, back = a1, left = a2; out[0] = rnorm);
// out[1] = 1 when a sort had to permute the second half
int ksd_nhepts(int op, int ld, int *dims, double *A, double *Q, double *X, double *B, double *Z, double *Y, double *wr, double *wi, double *wr2, double *wi2,
               const ksd_cmp *c, int a0, int a1, int a2, double *out)
{
  ksd::DsNhepTs ds; ksd_load(ds, ld, dims, c, A, Q); std::copy(X, X + ds.X.size(), ds.X.begin());
  std::copy(B, B + ds.hb.A.size(), ds.hb.A.begin()); std::copy(Z, Z + ds.hb.Q.size(), ds.hb.Q.begin()); std::copy(Y, Y + ds.hb.X.size(), ds.hb.X.begin());
  std::copy(wr2, wr2 + ld, ds.wr2.begin()); std::copy(wi2, wi2 + ld, ds.wi2.begin());
  int rc;
  if (op == 6) rc = ds.vectors_side(a0, a2 != 0, a1 != 0, &out[0]);
  else rc = ksd_step(ds, ds.X.data(), op, wr, wi, nullptr, nullptr, a0, a1, a2, out);
  if (op == 1) out[1] = (double)ds.permuted;
  ksd_store(ds, dims, A, Q); std::copy(ds.X.begin(), ds.X.end(), X);
  std::copy(ds.hb.A.begin(), ds.hb.A.end(), B); std::copy(ds.hb.Q.begin(), ds.hb.Q.end(), Z); std::copy(ds.hb.X.begin(), ds.hb.X.end(), Y);
  std::copy(ds.wr2.begin(), ds.wr2.end(), wr2); std::copy(ds.wi2.begin(), ds.wi2.end(), wi2);
  return rc;
}
// DS GHEP on caller-owned ld x ld arrays (tests/test_ds_ghep_host.py): solve and sort with `which`; returns what DsGhep::solve returns
int ksd_ghep(int n, int ld, const double *A, const double *B, double *Q, double *w, int which)
{
  ksd::DsGhep ds; ds.allocate(ld); ds.n = n; ds.which.which = which;
  std::copy(A, A + ds.A.size(), ds.A.begin()); std::copy(B, B + ds.B.size(), ds.B.begin());
  const int rc = ds.solve(w);
  if (!rc) ds.sort(w);
  std::copy(ds.Q.begin(), ds.Q.end(), Q);
  return rc;
}
// The projected problem of Generalized Davidson on caller-owned ld x ld arrays (tests/test_gd_host.py). dims = {n, size_oldU}, read and written back.
// op 0 grow(a0 columns from Z, ldz), 1 solve_sort (returns its code), 2 lock(a0), 3 restart_basis(a0 = size_X, a1 = size_plusk) into Z (returns the kept
// count), 4 project(Z, ldz, a0 = kept), 5 save_oldU
int ksd_gd(int op, int ld, int *dims, double *H, double *Q, double *oldU, double *w, int which, double target, int a0, int a1, double *Z, int ldz)
{
  ksd::DsGd ds; ds.allocate(ld); ds.n = dims[0]; ds.size_oldU = dims[1]; ds.which.which = which; ds.which.target = target;
  std::copy(H, H + ds.H.size(), ds.H.begin()); std::copy(Q, Q + ds.Q.size(), ds.Q.begin()); std::copy(oldU, oldU + ds.oldU.size(), ds.oldU.begin()); std::copy(w, w + ld, ds.w.begin());
  int rc = 0;
  switch (op) {
    case 0: ds.grow(a0, Z, ldz); break;
    case 1: rc = ds.solve_sort(); break;
    case 2: ds.lock(a0); break;
    case 3: rc = ds.restart_basis(a0, a1, Z, ldz); break;
    case 4: ds.project(Z, ldz, a0); break;
    case 5: ds.save_oldU(); break;
    default: return -1;
  }
  dims[0] = ds.n; dims[1] = ds.size_oldU;
  std::copy(ds.H.begin(), ds.H.end(), H); std::copy(ds.Q.begin(), ds.Q.end(), Q); std::copy(ds.oldU.begin(), ds.oldU.end(), oldU); std::copy(ds.w.begin(), ds.w.end(), w);
  return rc;
}
void ksd_backtransform(int st_type, double sigma, double nu, int n, double *eigr, double *eigi) { ksd::StMap{st_type, sigma, nu}.backtransform(n, eigr, eigi); }
}
#endif
