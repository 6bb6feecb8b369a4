// Host check of the block CSR planners of slepc_amd/csrc/ks_csr.cpp (bsr_expand, bsr_diag, bsr_plan, bsr_apply_host), built together with that file by
// tests/test_bsr_host.py under -fsanitize=address,undefined: the sanitizer is what catches an index outside a plan's arrays. Block matrices are
// generated from a fixed seed with integer values, so every product is exact: the expansion is checked entry by entry against a brute-force
// restatement, the host walk of the device image against a plain CSR product of the expansion, for every block size 2 .. 8, on one rank and on the
// middle rank of three.
#include "../../slepc_amd/csrc/ks_csr.h"
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <string>

static uint64_t lcg_state = 0x2545F4914F6CDD1DULL;
static unsigned lcg(unsigned below) { lcg_state = lcg_state * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)((lcg_state >> 33) % below); }

static int fails = 0;
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s line %d: %s\n", name.c_str(), __LINE__, #cond); fails++; return; } } while (0)

struct Bsr { int bs = 0, nb = 0, nbg = 0; std::vector<int> rp, col; std::vector<double> val; };      // val: column-major blocks
// block rows of 0 .. maxlen blocks (every 7th empty, row 1 with `longrow` blocks), unsorted block columns with repeats, integers 1 .. 8 of either
// sign and a zero in every fifth block
static Bsr random_blocks(int bs, int nb, int nbg, int maxlen, int longrow)
{
  Bsr A; A.bs = bs; A.nb = nb; A.nbg = nbg; A.rp.push_back(0);
  for (int I = 0; I < nb; I++) {
    int len = I % 7 == 0 ? 0 : (int)lcg(maxlen + 1);
    if (I == 1) len = longrow;
    for (int j = 0; j < len; j++) {
      A.col.push_back((int)lcg(nbg));
      if (j == 2) A.col.back() = A.col[A.col.size() - 3];
      for (int e = 0; e < bs * bs; e++) A.val.push_back((double)(1 + (int)lcg(8)) * (lcg(2) ? 1.0 : -1.0));
      if (A.col.size() % 5 == 0) A.val[A.val.size() - 1 - lcg(bs * bs)] = 0.0;
    }
    A.rp.push_back((int)A.col.size());
  }
  return A;
}

static void expansion(const std::string &name, int bs)
{
  const Bsr A = random_blocks(bs, 23, 31, 6, 9);
  ksc::BsrExpansion e;
  ksc::bsr_expand(bs, A.nb, A.nbg, A.rp.data(), A.col.data(), A.val.data(), e);
  REQUIRE(e.status == 0 && (int)e.rp.size() == A.nb * bs + 1 && e.rp[0] == 0);
  for (int I = 0; I < A.nb; I++)
    for (int i = 0; i < bs; i++) {                            // brute force: block after block in stored order, then c
      int p = e.rp[(size_t)I * bs + i];
      for (int k = A.rp[I]; k < A.rp[I + 1]; k++)
        for (int c = 0; c < bs; c++, p++) REQUIRE(e.col[p] == bs * A.col[k] + c && e.val[p] == A.val[(size_t)k * bs * bs + (size_t)c * bs + i]);
      REQUIRE(p == e.rp[(size_t)I * bs + i + 1]);
    }
  REQUIRE(e.rp.back() == (int)e.col.size() && e.col.size() == A.col.size() * bs * bs && e.val.size() == e.col.size());
  std::printf("ok %s\n", name.c_str());
}

// the rank that owns block rows [bstart, bstart + nb) of nbg: its diagonal block, the image, and the host walk against the CSR product of the
// expansion restricted to the rank's own columns
static void product(const std::string &name, int bs, int nb, int bstart, int nbg)
{
  const int group_rows = 4 * (64 / bs), chunk_blocks = std::min(64, 512 / (bs * bs));
  const Bsr A = random_blocks(bs, nb, nbg, 12, 3 * chunk_blocks + 1);
  ksc::BsrExpansion e;
  ksc::bsr_expand(bs, nb, nbg, A.rp.data(), A.col.data(), A.val.data(), e);
  REQUIRE(e.status == 0);
  ksc::BsrBlocks d; ksc::BsrPlan p;
  ksc::bsr_diag(bs, nb, bstart, A.rp.data(), A.col.data(), A.val.data(), d);
  for (int I = 0; I < nb; I++) {                              // the rank's own blocks, in stored order, local columns
    int q = d.browptr[I];
    for (int k = A.rp[I]; k < A.rp[I + 1]; k++)
      if (A.col[k] >= bstart && A.col[k] < bstart + nb) {
        REQUIRE(q < d.browptr[I + 1] && d.bcol[q] == A.col[k] - bstart);
        for (int t = 0; t < bs * bs; t++) REQUIRE(d.bval[(size_t)q * bs * bs + t] == A.val[(size_t)k * bs * bs + t]);
        q++;
      }
    REQUIRE(q == d.browptr[I + 1]);
  }
  ksc::bsr_plan(bs, nb, d.browptr.data(), d.bcol.data(), d.bval.data(), group_rows, chunk_blocks, 8, p);
  REQUIRE(p.blocks == (long long)d.bcol.size() && p.groups == (nb + group_rows - 1) / group_rows);
  REQUIRE(p.val.size() == d.bval.size() + 8 && p.bcol.size() == d.bcol.size() + 8 && (long long)p.gptr.size() == p.groups + 1);
  for (long long g = 0; g <= p.groups; g++) REQUIRE(p.gptr[(size_t)g] == d.browptr[std::min<long long>(g * group_rows, nb)]);
  for (size_t t = d.bval.size(); t < p.val.size(); t++) REQUIRE(p.val[t] == 0.0);
  const int n = nb * bs;
  std::vector<double> x((size_t)n), y((size_t)n, -1.0);
  for (double &v : x) { const int t = 1 + (int)lcg(8); v = lcg(2) ? t : -t; }
  ksc::bsr_apply_host(p, x.data(), y.data());
  for (int r = 0; r < n; r++) {
    double s = 0.0;
    for (int q = e.rp[r]; q < e.rp[r + 1]; q++) { const int c = e.col[q] - bstart * bs; if (c >= 0 && c < n) s += e.val[q] * x[c]; }
    REQUIRE(y[r] == s);
  }
  std::printf("ok %s: %lld blocks in %lld groups of %d block rows, chunks of %d blocks\n", name.c_str(), p.blocks, p.groups, group_rows, chunk_blocks);
}

static void rejections()
{
  const std::string name = "rejections";
  ksc::BsrExpansion e;
  const int rp_bad[] = {0, 2, 1, 3}, rp[] = {0, 1, 2, 3}, col_bad[] = {0, 1, 3}, col_neg[] = {0, -1, 2}, col[] = {2, 0, 1};
  const std::vector<double> val(3 * 4, 1.0);
  ksc::bsr_expand(2, 3, 3, rp_bad, col_bad, val.data(), e); REQUIRE(e.status == ksc::BSR_ROWPTR && e.bad_row == 1 && e.rp.empty());      // the pointer before any column
  ksc::bsr_expand(2, 3, 3, rp, col_bad, val.data(), e); REQUIRE(e.status == ksc::BSR_COLUMN && e.bad_row == 2 && e.bad_col == 3 && e.col.empty());
  ksc::bsr_expand(2, 3, 3, rp, col_neg, val.data(), e); REQUIRE(e.status == ksc::BSR_COLUMN && e.bad_row == 1 && e.bad_col == -1);
  ksc::bsr_expand(2, 3, 3, rp, col, val.data(), e); REQUIRE(e.status == 0 && e.col.size() == 12);
  const int rp_big[] = {0, 33554432};                                                          // 2^25 blocks of 8 x 8 = 2^31 scalars: refused before bcol is read
  ksc::bsr_expand(8, 1, 1, rp_big, nullptr, nullptr, e); REQUIRE(e.status == ksc::BSR_TOO_LARGE);
  const int rp_fits[] = {0, 0};
  ksc::bsr_expand(8, 1, 1, rp_fits, nullptr, nullptr, e); REQUIRE(e.status == 0 && e.rp.size() == 9 && e.col.empty());
  std::printf("ok %s\n", name.c_str());
}

int main()
{
  for (int bs = 1; bs <= 9; bs++) expansion("expansion bs " + std::to_string(bs), bs);
  for (int bs = 2; bs <= 8; bs++) {
    const int G = 4 * (64 / bs);
    product("product bs " + std::to_string(bs) + " one rank", bs, 2 * G + 5, 0, 2 * G + 5);
    product("product bs " + std::to_string(bs) + " middle rank of three", bs, G + 3, 11, G + 3 + 30);
  }
  rejections();
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
