// Stand-alone replay of two DS NHEPTS cases (slepc_amd/csrc/ks_ds.cpp + ks_dense.cpp, no GPU, no Python): built by
// tests/test_ds_twosided_host.py with -fsanitize=address,undefined and run as a program of its own. Each case makes the two halves from a
// quasi-triangular matrix with known eigenvalues, hidden behind plane rotations, whose orders under "largest magnitude" differ between the
// halves by construction, so that the sort enters the permutation branch; then every step of a restart is taken. Exit status 0 = all checks hold.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../../slepc_amd/csrc/ks_ds.h"
#include "../../slepc_amd/csrc/ks_dense.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("check failed, line %d: %s\n", __LINE__, #c); failures++; } } while (0)

// A <- G^T A G over a fixed sequence of plane rotations (an orthogonal similarity), on the leading n x n block
static void scramble(std::vector<double> &A, int ld, int n, double seed)
{
  for (int s = 0; s < 3 * n; s++) {
    const int i = s % (n - 1), j = i + 1 + (s % (n - 1 - i));
    const double th = seed + 0.37 * s, c = std::cos(th), sn = std::sin(th);
    for (int k = 0; k < n; k++) { double &x = A[(size_t)k + (size_t)i * ld], &y = A[(size_t)k + (size_t)j * ld]; const double t = c * x + sn * y; y = c * y - sn * x; x = t; }
    for (int k = 0; k < n; k++) { double &x = A[(size_t)i + (size_t)k * ld], &y = A[(size_t)j + (size_t)k * ld]; const double t = c * x + sn * y; y = c * y - sn * x; x = t; }
  }
}

// diag entries d, 2x2 block at `blk` (or -1) with eigenvalues re +- i*im, strict upper part filled
static void make_half(std::vector<double> &A, int ld, int n, const double *d, int blk, double re, double im, double seed)
{
  for (int j = 0; j < n; j++) for (int i = 0; i <= j; i++) A[(size_t)i + (size_t)j * ld] = (i == j) ? d[i] : 0.1 * std::sin(seed + i + 3.0 * j);
  if (blk >= 0) { A[(size_t)blk + (size_t)blk * ld] = re; A[(size_t)(blk + 1) + (size_t)(blk + 1) * ld] = re; A[(size_t)blk + (size_t)(blk + 1) * ld] = 2.0 * im; A[(size_t)(blk + 1) + (size_t)blk * ld] = -0.5 * im; }
  scramble(A, ld, n, seed);
  A[(size_t)n + (size_t)(n - 1) * ld] = 0.25;                                                       // the extra row: beta e_n^T
}

static void run_case(bool with_pair)
{
  const int n = 7, ld = 9; const double delta = 1e-6;
  ksd::DsNhepTs ds; ds.allocate(ld); ds.which.which = KS_EPS_LARGEST_MAGNITUDE;
  std::vector<double> wr(ld), wi(ld);
  if (!with_pair) {
    const double da[7] = {0.5, 1.0 + delta, 0.3, -1.0, 0.1, -0.2, 0.7}, db[7] = {-(1.0 + delta), 0.3, 0.7, 0.5, 1.0, 0.1, -0.2};
    make_half(ds.A, ld, n, da, -1, 0, 0, 0.3); make_half(ds.hb.A, ld, n, db, -1, 0, 0, 1.1);
  } else {
    const double r = 1.0 + delta, th = 0.8;                                                          // first half: the pair leads (modulus 1 + delta), then -1
    const double da[7] = {0.5, 0.0, 0.0, -1.0, 0.1, -0.2, 0.7}, db[7] = {0.7, -(1.0 + delta), 0.5, 0.0, 0.0, 0.1, -0.2};   // second half: -(1 + delta), then the pair of modulus 1
    make_half(ds.A, ld, n, da, 1, r * std::cos(th), r * std::sin(th), 0.3); make_half(ds.hb.A, ld, n, db, 3, std::cos(th), std::sin(th), 1.1);
  }
  ds.set_dimensions(n, 0, 0); ds.state = ksd::DS_RAW;
  CHECK(ds.solve(wr.data(), wi.data()) == 0);
  CHECK(ds.sort(wr.data(), wi.data()) == 0);
  CHECK(ds.permuted == 1);
  for (int i = 0; i < n; i++) CHECK(std::hypot(ds.wr2[i] - wr[i], ds.wi2[i] - wi[i]) < 1e-5);       // the halves correspond again (they differ by delta where planted)
  if (with_pair) { CHECK(wi[0] > 0.0 && wi[1] < 0.0 && ds.wi2[0] > 0.0 && std::fabs(wr[2] + 1.0) < 1e-9 && std::fabs(ds.wr2[2] + 1.0 + delta) < 1e-9); }
  else { CHECK(std::fabs(wr[0] - 1.0 - delta) < 1e-9 && std::fabs(wr[1] + 1.0) < 1e-9 && std::fabs(ds.wr2[0] - 1.0) < 1e-9 && std::fabs(ds.wr2[1] + 1.0 + delta) < 1e-9); }
  ds.update_extra_row();
  for (int k = 0; k < n; k++) {
    double rn = 0.0, ln = 0.0;
    const int nk = ds.vectors_side(k, false, true, &rn), lk = ds.vectors_side(k, true, true, &ln);
    CHECK(nk == lk && rn >= 0.0 && ln >= 0.0 && rn <= 1.0 && ln <= 1.0);
    k = nk;
  }
  int kk = ds.truncate_size(0, n, with_pair ? 1 : 3);
  CHECK(kk == (with_pair ? 2 : 3));                                                                  // size 1 would split the leading pair
  ds.truncate(kk, false);
  CHECK(ds.n == kk && ds.hb.n == kk && ds.t == n && ds.state == ksd::DS_TRUNCATED);
  for (int j = 0; j < kk; j++) CHECK(ds.a(kk, j) != 0.0 && ds.hb.a(kk, j) != 0.0 && ds.a(n, j) == 0.0 && ds.hb.a(n, j) == 0.0);
  ds.truncate(kk, true);
  // the LU pair of the solver's RQ update on the same data
  std::vector<double> M((size_t)n * n), b(n, 1.0), c(n, 1.0); std::vector<int> piv(n);
  for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) M[(size_t)i + (size_t)j * n] = (i == j ? 2.0 : 0.0) + 0.3 * std::sin(1.0 + i + 2.0 * j);
  CHECK(ksd::lu_factor(n, M.data(), n, piv.data()) == 0);
  ksd::lu_solve(n, M.data(), n, piv.data(), b.data(), false); ksd::lu_solve(n, M.data(), n, piv.data(), c.data(), true);
  for (int i = 0; i < n; i++) CHECK(std::isfinite(b[i]) && std::isfinite(c[i]));
}

int main()
{
  run_case(false);
  run_case(true);
  std::printf(failures ? "FAILED (%d)\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
