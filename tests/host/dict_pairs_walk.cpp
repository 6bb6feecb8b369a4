// Host check of the pair form of the dictionary row walk (slepc_amd/csrc/ks_dict_pairs.h), built by tests/test_dict_pairs_host.py under
// -fsanitize=address,undefined. Waves of 64 lanes are emulated with a loop over x and y allocated with exactly n elements: the sanitizer is what catches
// a load outside [x, x + n), the comparison with the one-row walk (entry slots in order, fma from 0.0, padding as fma(0, 0, acc)) is bit for bit.
// The lane shift of the emulation re-reads what the neighbouring lane loads; the wave's first and last lane get a NaN from it, so a walk that used
// the shifted value there instead of its own load would not compare equal.
#include "../../slepc_amd/csrc/ks_dict_pairs.h"
#include <cstdio>
#include <cstdint>
#include <limits>
#include <map>
#include <string>

struct Csr { int n = 0; std::vector<int> rp, col; std::vector<double> val; };

// a stencil on an nx x ny x nz box (x fastest), Dirichlet: the entries of `st` (dx, dy, dz, value) that stay inside the box, columns ascending
struct Pt { int dx, dy, dz; double v; };
static Csr stencil(int nx, int ny, int nz, const std::vector<Pt> &st)
{
  Csr A; A.n = nx * ny * nz; A.rp.push_back(0);
  for (int k = 0; k < nz; k++) for (int j = 0; j < ny; j++) for (int i = 0; i < nx; i++) {
    std::map<int, double> row;
    for (const Pt &p : st) {
      const int a = i + p.dx, b = j + p.dy, c = k + p.dz;
      if (a >= 0 && a < nx && b >= 0 && b < ny && c >= 0 && c < nz) row[a + nx * (b + ny * c)] = p.v;
    }
    for (auto &e : row) { A.col.push_back(e.first); A.val.push_back(e.second); }
    A.rp.push_back((int)A.col.size());
  }
  return A;
}
static std::vector<Pt> lap3() { return {{0, 0, -1, -1.0}, {0, -1, 0, -1.0}, {-1, 0, 0, -1.0}, {0, 0, 0, 6.0}, {1, 0, 0, -1.0}, {0, 1, 0, -1.0}, {0, 0, 1, -1.0}}; }
static std::vector<Pt> lap2() { return {{0, -1, 0, -1.0}, {-1, 0, 0, -1.0}, {0, 0, 0, 4.0}, {1, 0, 0, -1.0}, {0, 1, 0, -1.0}}; }
static std::vector<Pt> box27()
{
  std::vector<Pt> s;
  for (int c = -1; c <= 1; c++) for (int b = -1; b <= 1; b++) for (int a = -1; a <= 1; a++) s.push_back({a, b, c, a == 0 && b == 0 && c == 0 ? 26.0 : -1.0});
  return s;
}
static Csr drop_last_row(const Csr &A)                       // the leading (n - 1) x (n - 1) block
{
  Csr B; B.n = A.n - 1; B.rp.push_back(0);
  for (int r = 0; r < B.n; r++) {
    for (int e = A.rp[r]; e < A.rp[r + 1]; e++) if (A.col[e] < B.n) { B.col.push_back(A.col[e]); B.val.push_back(A.val[e]); }
    B.rp.push_back((int)B.col.size());
  }
  return B;
}

// the dictionary layout as ks_mat.hip builds it: sorted dictionaries of values (bit patterns) and offsets, W 2-byte codes per row, the distinct rows
struct Dict { int W = 0, npat = 0; std::vector<double> vals; std::vector<int> offs; std::vector<unsigned short> pats; std::vector<unsigned char> rowpat; bool patterns = false; };
static Dict build_dict(const Csr &A, bool want_patterns = true)
{
  Dict D;
  int maxlen = 0;
  for (int r = 0; r < A.n; r++) maxlen = std::max(maxlen, A.rp[r + 1] - A.rp[r]);
  D.W = maxlen <= 8 ? 8 : (maxlen <= 16 ? 16 : 32);
  std::vector<int64_t> bits;
  for (double v : A.val) { int64_t b; std::memcpy(&b, &v, 8); bits.push_back(b); }
  std::sort(bits.begin(), bits.end()); bits.erase(std::unique(bits.begin(), bits.end()), bits.end());
  for (int64_t b : bits) { double v; std::memcpy(&v, &b, 8); D.vals.push_back(v); }
  for (int r = 0; r < A.n; r++) for (int e = A.rp[r]; e < A.rp[r + 1]; e++) D.offs.push_back(A.col[e] - r);
  std::sort(D.offs.begin(), D.offs.end()); D.offs.erase(std::unique(D.offs.begin(), D.offs.end()), D.offs.end());
  if (D.vals.size() > 255 || D.offs.size() > 256 || !want_patterns) return D;
  std::vector<std::vector<unsigned short>> rows(A.n, std::vector<unsigned short>(D.W, (unsigned short)(255u << 8)));
  for (int r = 0; r < A.n; r++) for (int e = A.rp[r]; e < A.rp[r + 1]; e++) {
    int64_t b; std::memcpy(&b, &A.val[e], 8);
    const unsigned vc = (unsigned)(std::lower_bound(bits.begin(), bits.end(), b) - bits.begin());
    const unsigned oc = (unsigned)(std::lower_bound(D.offs.begin(), D.offs.end(), A.col[e] - r) - D.offs.begin());
    rows[r][e - A.rp[r]] = (unsigned short)(oc | vc << 8);
  }
  std::vector<std::vector<unsigned short>> table(rows);
  std::sort(table.begin(), table.end()); table.erase(std::unique(table.begin(), table.end()), table.end());
  if (table.size() > 256) return D;
  D.patterns = true; D.npat = (int)table.size();
  for (auto &w : table) D.pats.insert(D.pats.end(), w.begin(), w.end());
  D.rowpat.assign(((size_t)A.n + 255) / 256 * 256, 0);
  for (int r = 0; r < A.n; r++) D.rowpat[r] = (unsigned char)(std::lower_bound(table.begin(), table.end(), rows[r]) - table.begin());
  return D;
}
static ksp::PairPlan plan_of(const Dict &D)
{
  return ksp::dict_pair_plan(D.W, D.npat, D.patterns ? D.pats.data() : nullptr, D.offs.data(), (int)D.offs.size(), D.vals.data(), (int)D.vals.size());
}

// the one-row walk (ksr::dict_word_row): entry slots in order, padding as fma(0, 0, acc)
static double row_walk(const Dict &D, long long r, const double *x)
{
  double acc = 0.0;
  const unsigned short *w = D.pats.data() + (size_t)D.rowpat[r] * D.W;
  for (int e = 0; e < D.W; e++) {
    const unsigned oc = w[e] & 255u, vc = w[e] >> 8;
    const bool ok = vc != 255u;
    acc = std::fma(ok ? D.vals[vc] : 0.0, ok ? x[r + D.offs[oc]] : 0.0, acc);
  }
  return acc;
}

struct HostLane {
  const double *x; long long n; int l;
  int lane() const { return l; }
  ksp::D2 pair(long long i) const { return ksp::pair_ld(x, n, i); }
  double one(long long i, bool want) const { return ksp::one_ld(x, n, i, want); }
  double up(double, long long i) const { return l == 0 ? std::numeric_limits<double>::quiet_NaN() : ksp::pair_ld(x, n, i - 2).y; }
  double down(double, long long i) const { return l == 63 ? std::numeric_limits<double>::quiet_NaN() : ksp::pair_ld(x, n, i + 2).x; }
};

static int failures = 0;
// the last row of an odd n as the pair kernels compute it: with the matrix's own W, which is the stride of the pattern table
static double tail_row(const Dict &D, long long r, const double *x)
{
  if (D.W == 8) return ksp::dict_row_from_tables<8>(D.rowpat.data(), D.pats.data(), r, D.vals.data(), D.offs.data(), x);
  if (D.W == 16) return ksp::dict_row_from_tables<16>(D.rowpat.data(), D.pats.data(), r, D.vals.data(), D.offs.data(), x);
  return ksp::dict_row_from_tables<32>(D.rowpat.data(), D.pats.data(), r, D.vals.data(), D.offs.data(), x);
}

// tiny: x holds +-the smallest denormal and zeros, so that products underflow to -0.0 and +0.0: the sign of a zero result must be the one-row walk's too
static void walk_case(const char *name, const Csr &A, bool tiny = false)
{
  const Dict D = build_dict(A);
  const ksp::PairPlan P = plan_of(D);
  if (!P.ok) { std::printf("FAIL %s: not eligible (%s)\n", name, P.why); failures++; return; }
  const long long n = A.n;
  double *x = new double[n], *y = new double[n];            // exactly n elements each: one element further is the sanitizer's
  uint64_t s = 0x9e3779b97f4a7c15ull;
  for (long long i = 0; i < n; i++) { s = s * 6364136223846793005ull + 1442695040888963407ull; x[i] = (double)(int64_t)(s >> 11) / 9007199254740992.0 - 0.25;
    if (tiny) x[i] = (s >> 40 & 3) == 0 ? 0.0 : ((s >> 42 & 1) ? 1.0 : -1.0) * std::numeric_limits<double>::denorm_min(); }
  const long long waves = (n + 127) / 128;
  for (long long w = 0; w < waves; w++)
    for (int l = 0; l < 64; l++) {
      const long long r = w * 128 + 2 * l;
      const HostLane ln = {x, n, l};
      const int p0 = r + 1 < n ? D.rowpat[r] : 0, p1 = r + 1 < n ? D.rowpat[r + 1] : 0;
      double y0, y1;
      ksp::dict_pair_walk<ksp::PAIR_MAX_BASES>(P.args, P.coef.data(), P.mask.data(), p0, p1, r, ln, y0, y1);   // every lane of the wave, as on the device
      if (r + 1 < n) { y[r] = y0; y[r + 1] = y1; }
      else if (r < n) y[r] = tail_row(D, r, x);               // odd n: the last row on its own
    }
  long long bad = 0, negzero = 0;
  for (long long r = 0; r < n; r++) { const double ref = row_walk(D, r, x); if (std::memcmp(&ref, &y[r], 8) != 0) bad++; if (ref == 0.0 && std::signbit(ref)) negzero++; }
  if (tiny) std::printf("   %s: %lld rows with a result of -0.0\n", name, negzero);
  if (bad) { std::printf("FAIL %s: %lld of %lld rows differ\n", name, bad, n); failures++; }
  else std::printf("ok %s: n %lld, W %d, %d patterns, %d bases, wide mask 0x%x\n", name, n, D.W, D.npat, P.args.nb, P.args.dmask);
  delete[] x; delete[] y;
}
static void refused(const char *name, const Dict &D, const char *expect)
{
  const ksp::PairPlan P = plan_of(D);
  if (P.ok || std::string(P.why).find(expect) == std::string::npos) { std::printf("FAIL %s: %s (%s)\n", name, P.ok ? "accepted" : "refused for another reason", P.why); failures++; }
  else std::printf("ok %s refused: %s\n", name, P.why);
}

int main()
{
  walk_case("lap3d 4x4x4", stencil(4, 4, 4, lap3()));
  walk_case("lap3d 6x6x6", stencil(6, 6, 6, lap3()));
  walk_case("lap3d 4x6x10", stencil(4, 6, 10, lap3()));
  walk_case("lap3d 2x2x2", stencil(2, 2, 2, lap3()));
  walk_case("lap2d 4x4", stencil(4, 4, 1, lap2()));
  walk_case("lap2d 10x12", stencil(10, 12, 1, lap2()));
  walk_case("27-point 4x4x4", stencil(4, 4, 4, box27()));
  walk_case("lap3d 6x6x6 without its last row", drop_last_row(stencil(6, 6, 6, lap3())));
  walk_case("lap2d 10x30 (three waves)", stencil(10, 30, 1, lap2()));
  walk_case("offsets 0, +-1, +-2 (bases 2 apart)", stencil(140, 1, 1, {{-2, 0, 0, -1.0}, {-1, 0, 0, -0.5}, {0, 0, 0, 4.0}, {1, 0, 0, -0.25}, {2, 0, 0, -2.0}}));
  // W = 32 with an odd n (18 offsets, 6 bases): the last row decodes its code word with the table's real stride
  {
    std::vector<Pt> st;
    for (int o : {-9, -8, -7, -5, -4, -3, -1, 0, 1, 3, 4, 5, 7, 8, 9, 11, 12, 13}) st.push_back({o, 0, 0, o == 0 ? 26.0 : -1.0 - 0.125 * (o & 3)});
    walk_case("18 offsets, W 32, n 1001", stencil(1001, 1, 1, st));
  }
  walk_case("W 16 with an odd n", stencil(777, 1, 1, {{-8, 0, 0, -1.0}, {-5, 0, 0, -0.5}, {-4, 0, 0, -1.0}, {-3, 0, 0, -1.0}, {-1, 0, 0, -1.0}, {0, 0, 0, 9.0}, {1, 0, 0, -1.0}, {3, 0, 0, -2.0}, {4, 0, 0, -1.0}, {5, 0, 0, -1.0}, {8, 0, 0, -1.0}}));
  // products that underflow: rows with padding (5 of 8 slots) and rows without (8 of 8) keep the sign of a zero result
  walk_case("underflow, rows with padding", stencil(140, 1, 1, {{-2, 0, 0, -1.0}, {-1, 0, 0, -0.5}, {0, 0, 0, 4.0}, {1, 0, 0, -0.25}, {2, 0, 0, -2.0}}), true);
  walk_case("underflow, full rows", stencil(301, 1, 1, {{-6, 0, 0, -0.5}, {-4, 0, 0, -0.25}, {-1, 0, 0, -0.5}, {0, 0, 0, 0.5}, {1, 0, 0, -0.25}, {4, 0, 0, 0.25}, {6, 0, 0, -0.5}, {10, 0, 0, -0.125}}), true);
  walk_case("underflow, lap3d 6x6x6", stencil(6, 6, 6, {{0, 0, -1, -0.5}, {0, -1, 0, -0.25}, {-1, 0, 0, -0.5}, {0, 0, 0, 0.5}, {1, 0, 0, -0.25}, {0, 1, 0, -0.5}, {0, 0, 1, -0.125}}), true);

  refused("odd stride (lap2d 5x4)", build_dict(stencil(5, 4, 1, lap2())), "not within 1 of an even offset");
  refused("odd stride (lap3d 5x4x4)", build_dict(stencil(5, 4, 4, lap3())), "not within 1 of an even offset");
  // The issue's case "an offset of +-2 refused", as far as the issue's own rule can refuse it: an offset of exactly +-2 is b = +-2 with d = 0 (an even
  // offset is its own base; the 2x2x2 Laplacian, which the issue wants accepted, has such offsets), so the case above with offsets 0, +-1, +-2 is
  // accepted and walked. What is refused is an entry two past the pair the centre loads (offsets 0, +-1, +-3): it would need the pair at +-2, which no
  // row of the matrix reads
  refused("an offset two past a base's pair", build_dict(stencil(12, 1, 1, {{-3, 0, 0, -1.0}, {-1, 0, 0, -1.0}, {0, 0, 0, 4.0}, {1, 0, 0, -1.0}, {3, 0, 0, -1.0}})), "not within 1 of an even offset");
  {
    std::vector<Pt> st;
    for (int k = 0; k < 10; k++) st.push_back({8 * (k - 5), 0, 0, k == 5 ? 9.0 : -1.0});
    refused("10 bases", build_dict(stencil(200, 1, 1, st)), "more than 9 bases");
  }
  {
    Csr A = stencil(6, 6, 6, lap3());
    uint64_t s = 12345;
    for (double &v : A.val) { s = s * 6364136223846793005ull + 1442695040888963407ull; v = (double)(s >> 20); }
    refused("random values (no pattern form)", build_dict(A), "row-pattern form");
  }
  {
    Csr A = stencil(6, 6, 6, lap3());                          // a row with its entries out of ascending order: the candidate chain would reorder it
    std::swap(A.col[A.rp[100]], A.col[A.rp[100] + 1]);
    refused("unsorted row", build_dict(A), "ascending");
  }
  std::printf("%s\n", failures ? "FAILED" : "all ok");
  return failures ? 1 : 0;
}
