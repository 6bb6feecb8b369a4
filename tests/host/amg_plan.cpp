// Host check of the multigrid planner of slepc_amd/csrc/ks_csr.cpp (ksc::amg_plan), built together with that file by tests/test_amg_host.py under
// -fsanitize=address,undefined: the sanitizer is what catches an index outside a level's arrays. Three matrices of the Python tests are planned with
// several options and every level is checked by its own invariants: aggregates, the sizes and column ranges of P and R, R = P^T, and the Galerkin
// operator against a dense R A P.
#include "../../slepc_amd/csrc/ks_csr.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

static uint64_t lcg_state = 0x9E3779B97F4A7C15ULL;
static unsigned lcg(unsigned below) { lcg_state = lcg_state * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)((lcg_state >> 33) % below); }

struct Mat { int n = 0; std::vector<int> rp, col; std::vector<double> val; };
static int fails = 0;
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s line %d: %s\n", name.c_str(), __LINE__, #cond); fails++; return; } } while (0)

static void grid_rows(Mat &A, int nx, int ny, int base)
{
  for (int y = 0; y < ny; y++) for (int x = 0; x < nx; x++) {
    const int i = base + y * nx + x;
    if (y) { A.col.push_back(i - nx); A.val.push_back(-1.0); }
    if (x) { A.col.push_back(i - 1); A.val.push_back(-1.0); }
    A.col.push_back(i); A.val.push_back(4.0);
    if (x < nx - 1) { A.col.push_back(i + 1); A.val.push_back(-1.0); }
    if (y < ny - 1) { A.col.push_back(i + nx); A.val.push_back(-1.0); }
    A.rp.push_back((int)A.col.size());
  }
}
static Mat grid(int nx, int ny) { Mat A; A.n = nx * ny; A.rp.push_back(0); grid_rows(A, nx, ny, 0); return A; }
static Mat two_grids(int nx, int ny, int iso)
{
  Mat A; A.n = 2 * nx * ny + iso; A.rp.push_back(0);
  grid_rows(A, nx, ny, 0);
  for (int i = 0; i < iso; i++) { A.col.push_back(nx * ny + i); A.val.push_back(3.0); A.rp.push_back((int)A.col.size()); }
  grid_rows(A, nx, ny, nx * ny + iso);
  return A;
}
// unsorted rows with repeated columns, some of which cancel to a stored zero
static Mat random_unsymmetric(int n)
{
  Mat A; A.n = n; A.rp.push_back(0);
  for (int r = 0; r < n; r++) {
    const int len = 1 + (int)lcg(5);
    const int first = (int)A.col.size();
    for (int j = 0; j < len; j++) { const int c = (int)lcg(n); if (c == r) continue; A.col.push_back(c); A.val.push_back(-(1 + (int)lcg(4)) / 4.0); }
    A.col.push_back(r); A.val.push_back(5.0);
    if ((int)A.col.size() - first > 2) { A.col.push_back(A.col[first]); A.val.push_back(r % 3 ? -0.25 : -A.val[first]); }
    A.col.push_back(r); A.val.push_back(1.5);
    A.rp.push_back((int)A.col.size());
  }
  return A;
}

static void check(const std::string &name, const Mat &A, const ksc::AmgOptions &opt, int want_levels)
{
  ksc::AmgPlan p;
  ksc::amg_plan(A.n, A.rp.data(), A.col.data(), A.val.data(), opt, p);
  REQUIRE(p.status == 0 && !p.levels.empty() && p.levels[0].n == A.n);
  REQUIRE((int)p.levels.size() <= std::max(1, std::min(opt.max_levels, ksc::AMG_MAX_LEVELS)));
  REQUIRE(want_levels < 0 || (int)p.levels.size() == want_levels);
  for (size_t l = 0; l < p.levels.size(); l++) {
    const ksc::AmgLevel &L = p.levels[l];
    const int n = L.n;
    REQUIRE((int)L.rp.size() == n + 1 && L.rp[0] == 0 && L.rp[n] == (int)L.col.size() && L.col.size() == L.val.size());
    for (int i = 0; i < n; i++) for (int q = L.rp[i]; q < L.rp[i + 1]; q++) REQUIRE(L.col[q] >= 0 && L.col[q] < n && (q == L.rp[i] || L.col[q] > L.col[q - 1]));
    if (l + 1 == p.levels.size()) { REQUIRE(L.agg.empty() && L.pcol.empty() && L.rcol.empty()); continue; }
    const int nc = L.nagg;
    REQUIRE(nc >= 1 && p.levels[l + 1].n == nc && (int)L.agg.size() == n && (int)L.dinv.size() == n && L.rho > 0.0);
    std::vector<int> size((size_t)nc, 0);
    for (int i = 0; i < n; i++) { REQUIRE(L.agg[i] >= -1 && L.agg[i] < nc); if (L.agg[i] >= 0) size[L.agg[i]]++; }
    for (int s : size) REQUIRE(s >= 1);
    REQUIRE((int)L.prp.size() == n + 1 && L.prp[n] == (int)L.pcol.size() && (int)L.rrp.size() == nc + 1 && L.rrp[nc] == (int)L.rcol.size() && L.pcol.size() == L.rcol.size());
    // dense P, R = P^T, and R A P against the next level
    std::vector<double> P((size_t)n * nc, 0.0), AP((size_t)n * nc, 0.0), Ac((size_t)nc * nc, 0.0);
    for (int i = 0; i < n; i++) for (int q = L.prp[i]; q < L.prp[i + 1]; q++) { REQUIRE(L.pcol[q] >= 0 && L.pcol[q] < nc); P[(size_t)i * nc + L.pcol[q]] = L.pval[q]; }
    for (int c = 0; c < nc; c++) for (int q = L.rrp[c]; q < L.rrp[c + 1]; q++) { REQUIRE(L.rcol[q] >= 0 && L.rcol[q] < n); REQUIRE(P[(size_t)L.rcol[q] * nc + c] == L.rval[q]); }
    if (!opt.smooth) for (int i = 0; i < n; i++) REQUIRE(L.prp[i + 1] - L.prp[i] == (L.agg[i] >= 0 ? 1 : 0));
    for (int i = 0; i < n; i++) for (int q = L.rp[i]; q < L.rp[i + 1]; q++) for (int c = 0; c < nc; c++) AP[(size_t)i * nc + c] += L.val[q] * P[(size_t)L.col[q] * nc + c];
    for (int i = 0; i < n; i++) for (int a = 0; a < nc; a++) { const double pa = P[(size_t)i * nc + a]; if (pa != 0.0) for (int c = 0; c < nc; c++) Ac[(size_t)a * nc + c] += pa * AP[(size_t)i * nc + c]; }
    const ksc::AmgLevel &C = p.levels[l + 1];
    double worst = 0.0, scale = 0.0;
    std::vector<double> D((size_t)nc * nc, 0.0);
    for (int a = 0; a < nc; a++) for (int q = C.rp[a]; q < C.rp[a + 1]; q++) D[(size_t)a * nc + C.col[q]] = C.val[q];
    for (size_t k = 0; k < D.size(); k++) { worst = std::max(worst, std::fabs(D[k] - Ac[k])); scale = std::max(scale, std::fabs(Ac[k])); }
    REQUIRE(worst <= 1e-12 * scale);
  }
  std::printf("ok %s (%d levels)\n", name.c_str(), (int)p.levels.size());
}

static void zero_diagonal(const std::string &name)
{
  Mat A = grid(9, 7);
  for (int q = A.rp[20]; q < A.rp[21]; q++) if (A.col[q] == 20) A.val[q] = 0.0;
  ksc::AmgOptions opt; opt.coarse_limit = 8;
  ksc::AmgPlan p;
  ksc::amg_plan(A.n, A.rp.data(), A.col.data(), A.val.data(), opt, p);
  REQUIRE(p.status == ksc::AMG_NO_DIAGONAL && p.bad_level == 0 && p.bad_row == 20);
  std::printf("ok %s\n", name.c_str());
}

static void tiny(const std::string &name)
{
  ksc::AmgOptions opt;
  for (int n = 0; n < 2; n++) {
    Mat A; A.n = n; A.rp.assign((size_t)n + 1, 0);
    if (n) { A.col.push_back(0); A.val.push_back(-4.0); A.rp[1] = 1; }
    ksc::AmgPlan p;
    ksc::amg_plan(n, A.rp.data(), A.col.data(), A.val.data(), opt, p);
    REQUIRE(p.status == 0 && p.levels.size() == 1 && p.levels[0].n == n);
  }
  Mat D; D.n = 300; D.rp.push_back(0);
  for (int i = 0; i < 300; i++) { D.col.push_back(i); D.val.push_back(2.0 + i); D.rp.push_back(i + 1); }
  ksc::AmgPlan p;
  ksc::amg_plan(D.n, D.rp.data(), D.col.data(), D.val.data(), opt, p);
  REQUIRE(p.status == 0 && p.levels.size() == 1);
  std::printf("ok %s\n", name.c_str());
}

int main()
{
  ksc::AmgOptions o8; o8.coarse_limit = 8;
  ksc::AmgOptions plain = o8; plain.smooth = false;
  ksc::AmgOptions strong = o8; strong.theta = 0.2;
  ksc::AmgOptions two = o8; two.max_levels = 2;
  ksc::AmgOptions one; one.coarse_limit = 1 << 30;
  check("grid 45x31", grid(45, 31), o8, 4);
  check("grid 45x31, plain aggregation", grid(45, 31), plain, -1);
  check("grid 45x31, theta 0.2", grid(45, 31), strong, -1);
  check("grid 45x31, two levels", grid(45, 31), two, 2);
  check("grid 45x31, one level", grid(45, 31), one, 1);
  check("two grids and five identity rows", two_grids(17, 9, 5), o8, -1);
  ksc::AmgOptions o4; o4.coarse_limit = 4;
  check("random unsymmetric 60", random_unsymmetric(60), o4, -1);
  zero_diagonal("zero diagonal");
  tiny("n = 0, n = 1 and a diagonal");
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::printf("all ok\n");
  return 0;
}
