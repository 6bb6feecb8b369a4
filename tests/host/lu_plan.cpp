// Host check of the sparse LU planner of slepc_amd/csrc/ks_csr.cpp (ksc::csr_lu_plan, ksc::lu_apply_host, ksc::lu_apply_transpose_host), built together
// with that file by tests/test_lu_host.py under -fsanitize=address,undefined: the sanitizer is what catches an index outside a plan's arrays. Three small
// matrices are ordered, factored and laid out at several thresholds, with and without the transposed plan; the host applies are checked by a residual
// against the matrix itself, P y = x and P^T y = x, and the plan's arrays by their own invariants.
#include "../../slepc_amd/csrc/ks_csr.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

static uint64_t lcg_state = 0x9E3779B97F4A7C15ULL;
static unsigned lcg(unsigned below) { lcg_state = lcg_state * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)((lcg_state >> 33) % below); }

struct Csr { int n = 0; std::vector<int> rp, col; std::vector<double> val; };
static int fails = 0;
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s line %d: %s\n", name.c_str(), __LINE__, #cond); fails++; return; } } while (0)

static Csr laplacian(int m)
{
  Csr A; A.n = m * m; A.rp.push_back(0);
  for (int y = 0; y < m; y++) for (int x = 0; x < m; x++) {
    const int i = y * m + x;
    if (y) { A.col.push_back(i - m); A.val.push_back(-1.0); }
    if (x) { A.col.push_back(i - 1); A.val.push_back(-1.0); }
    A.col.push_back(i); A.val.push_back(4.0 - 1.3);                  // shifted into the spectrum: indefinite
    if (x < m - 1) { A.col.push_back(i + 1); A.val.push_back(-1.0); }
    if (y < m - 1) { A.col.push_back(i + m); A.val.push_back(-1.0); }
    A.rp.push_back((int)A.col.size());
  }
  return A;
}
// unsorted rows with repeated columns, diagonally dominant
static Csr random_unsymmetric(int n)
{
  Csr A; A.n = n; A.rp.push_back(0);
  for (int r = 0; r < n; r++) {
    const int len = (int)lcg(6);
    double sum = 0.0;
    for (int j = 0; j < len; j++) { const int c = (int)lcg(n); if (c == r) continue; const double v = ((int)lcg(9) - 4) / 4.0; A.col.push_back(c); A.val.push_back(v); sum += std::fabs(v); }
    A.col.push_back(r); A.val.push_back(1.0 + sum);
    if (len > 2) { A.col.push_back(A.col[A.rp.back()]); A.val.push_back(0.25); A.val[A.col.size() - 2] += 0.25; }
    A.rp.push_back((int)A.col.size());
  }
  return A;
}
static Csr arrow(int n)
{
  Csr A; A.n = n; A.rp.push_back(0);
  for (int r = 0; r < n - 1; r++) { A.col.push_back(r); A.val.push_back(2.0 + 0.01 * r); A.rp.push_back((int)A.col.size()); }
  for (int c = 0; c < n - 1; c++) { A.col.push_back(c); A.val.push_back((c % 2 ? -1.0 : 1.0) / n); }
  A.col.push_back(n - 1); A.val.push_back(3.0);
  A.rp.push_back((int)A.col.size());
  return A;
}

static double residual(const Csr &A, const std::vector<double> &y, const std::vector<double> &x, bool transpose)
{
  std::vector<double> r(x);
  for (int i = 0; i < A.n; i++) for (int p = A.rp[i]; p < A.rp[i + 1]; p++) { if (transpose) r[A.col[p]] -= A.val[p] * y[i]; else r[i] -= A.val[p] * y[A.col[p]]; }
  double m = 0.0, s = 0.0;
  for (int i = 0; i < A.n; i++) { m = std::max(m, std::fabs(r[i])); s = std::max(s, std::fabs(y[i])); }
  return m / std::max(s, 1e-300);
}

static void invariants(const std::string &name, const ksc::LuPlan &p, int n)
{
  REQUIRE((int)p.perm.size() == n && (int)p.rows.size() == 2 * n && (int)p.rp.size() == 2 * n + 1 && (int)p.dinv.size() == n);
  REQUIRE((int)p.lev.size() == p.levels[0] + p.levels[1] + 1 && (int)p.lanes.size() == p.levels[0] + p.levels[1]);
  REQUIRE(p.lev.front() == 0 && p.lev.back() == 2 * n && p.rp.back() == (int)p.col.size() && p.col.size() == p.val.size());
  REQUIRE((long long)p.col.size() == p.nnzL + p.nnzU - n);
  std::vector<int> seen((size_t)n, 0);
  for (int v : p.perm) { REQUIRE(v >= 0 && v < n); seen[v]++; }
  for (int v : seen) REQUIRE(v == 1);
  for (int t = 0; t < 2; t++) { std::fill(seen.begin(), seen.end(), 0); for (int i = 0; i < n; i++) { const int r = p.rows[(size_t)t * n + i]; REQUIRE(r >= 0 && r < n); seen[r]++; } for (int v : seen) REQUIRE(v == 1); }
  for (int c : p.col) REQUIRE(c >= 0 && c < n);
  int next = 0;
  REQUIRE((int)p.stages.size() == p.nstage[0] + p.nstage[1]);
  for (const ksc::LuStage &s : p.stages) {
    REQUIRE(s.lev0 == next && s.nlev > 0); next += s.nlev;
    for (int l = s.lev0; l < s.lev0 + s.nlev; l++) REQUIRE(((p.lev[l + 1] - p.lev[l]) >= p.wide) == (s.wide != 0));
  }
  REQUIRE(next == p.levels[0] + p.levels[1]);
}

static void solve(const std::string &name, const Csr &A, int ordering)
{
  std::vector<double> x((size_t)A.n), y((size_t)A.n), z((size_t)A.n);
  for (int i = 0; i < A.n; i++) x[i] = ((int)lcg(2001) - 1000) / 500.0;
  const int wides[] = {1, 3, 64, 1 << 30};
  for (int wide : wides) {
    ksc::LuPlan p, t, alone;
    ksc::csr_lu_plan(A.n, A.rp.data(), A.col.data(), A.val.data(), ordering, wide, true, p, &t);
    ksc::csr_lu_plan(A.n, A.rp.data(), A.col.data(), A.val.data(), ordering, wide, false, alone);
    REQUIRE(p.status == 0 && alone.status == 0);
    invariants(name, p, A.n); invariants(name, t, A.n);
    REQUIRE(t.first_scaled == 1 && p.first_scaled == 0 && alone.val == p.val && alone.col == p.col && alone.rows == p.rows && alone.perm == p.perm);
    REQUIRE(t.levels[0] == p.levels[1] && t.levels[1] == p.levels[0]);         // a transposed triangle has the depth of the triangle it transposes
    ksc::lu_apply_host(p, x.data(), y.data());
    ksc::lu_apply_transpose_host(t, x.data(), z.data());
    const double rf = residual(A, y, x, false), rt = residual(A, z, x, true);
    REQUIRE(rf < 1e-11 && rt < 1e-11);
  }
  std::printf("ok %s\n", name.c_str());
}

static void zero_pivot(const std::string &name)
{
  Csr A = arrow(20);
  A.val[7] = 0.0;                                                     // the diagonal entry of row 7
  ksc::LuPlan p, t;
  ksc::csr_lu_plan(A.n, A.rp.data(), A.col.data(), A.val.data(), ksc::LU_ORDERING_NATURAL, 8, false, p, &t);
  REQUIRE(p.status == ksc::LU_ZERO_PIVOT && p.bad_row == 7);
  std::printf("ok %s\n", name.c_str());
}

static void tiny(const std::string &name)
{
  for (int n = 0; n < 2; n++) {
    Csr A; A.n = n; A.rp.assign((size_t)n + 1, 0);
    if (n) { A.col.push_back(0); A.val.push_back(-4.0); A.rp[1] = 1; }
    ksc::LuPlan p, t;
    ksc::csr_lu_plan(n, A.rp.data(), A.col.data(), A.val.data(), ksc::LU_ORDERING_ND, 64, false, p, &t);
    REQUIRE(p.status == 0);
    invariants(name, p, n); invariants(name, t, n);
    double x = 2.0, y = 0.0;
    ksc::lu_apply_host(p, &x, &y);
    if (n) REQUIRE(y == -0.5 && p.neg == 1 && p.pos == 0);
  }
  std::printf("ok %s\n", name.c_str());
}

int main()
{
  solve("laplacian 9x9, nd", laplacian(9), ksc::LU_ORDERING_ND);
  solve("random unsymmetric 70, nd", random_unsymmetric(70), ksc::LU_ORDERING_ND);
  solve("arrow 130, natural", arrow(130), ksc::LU_ORDERING_NATURAL);
  zero_pivot("zero pivot");
  tiny("n = 0 and n = 1");
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::printf("all ok\n");
  return 0;
}
