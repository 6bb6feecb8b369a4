// Host check of the assembly planners of slepc_amd/csrc/ks_csr.cpp, built together with that file by tests/test_assembly_plans_host.py under
// -fsanitize=address,undefined: the sanitizer is what catches an index outside a plan's arrays. Small worlds are generated from a fixed seed; for
// every rank the split, the receive counts, the peers and the localized send list are made with the product's functions (the two allgathers and the
// exchange of ids are loops here) and checked by brute force. The binned plan is walked on the host against a plain CSR product of integers.
#include "../../slepc_amd/csrc/ks_csr.h"
#include <cstdio>
#include <cstdint>
#include <string>

static uint64_t lcg_state = 0x2545F4914F6CDD1DULL;
static unsigned lcg(unsigned below) { lcg_state = lcg_state * 6364136223846793005ULL + 1442695040888963407ULL; return (unsigned)((lcg_state >> 33) % below); }

struct Csr { int n = 0; std::vector<int> rp, col; std::vector<double> val; };
static int fails = 0;
#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s line %d: %s\n", name.c_str(), __LINE__, #cond); fails++; return; } } while (0)

// rows of 0 ... maxlen entries, unsorted, repeated columns allowed, integer values 1 ... 8 of either sign; a row of a rank listed in `local_only`
// takes its columns from the rank's own range
static Csr random_rows(int nrows, int ncols, int maxlen, const std::vector<int> &starts = {}, int local_only = -1)
{
  Csr A; A.n = nrows; A.rp.push_back(0);
  for (int r = 0; r < nrows; r++) {
    int lo = 0, hi = ncols;
    if (local_only >= 0 && r >= starts[local_only] && r < starts[local_only + 1]) { lo = starts[local_only]; hi = starts[local_only + 1]; }
    const int len = (int)lcg(maxlen + 1);
    for (int j = 0; j < len; j++) { A.col.push_back(lo + (int)lcg(hi - lo)); A.val.push_back((double)(1 + (int)lcg(8)) * (lcg(2) ? 1.0 : -1.0)); }
    A.rp.push_back((int)A.col.size());
  }
  return A;
}

static void world(const std::string &name, const std::vector<int> &counts, int local_only = -1)
{
  const int size = (int)counts.size();
  std::vector<int> starts(size + 1, 0);
  for (int p = 0; p < size; p++) starts[p + 1] = starts[p] + counts[p];
  const int N = starts[size];
  const Csr A = random_rows(N, N, 5, starts, local_only);
  std::vector<ksc::BlockSplit> split(size);
  std::vector<int> all_cnt((size_t)size * size, 0);
  for (int p = 0; p < size; p++) {
    const int r0 = starts[p], n = counts[p], e0 = A.rp[r0];
    std::vector<int> rp(A.rp.begin() + r0, A.rp.begin() + r0 + n + 1);
    for (int &v : rp) v -= e0;
    ksc::csr_split_block(n, r0, N, rp.data(), A.col.data() + e0, A.val.data() + e0, split[p]);
    const ksc::BlockSplit &s = split[p];
    REQUIRE(s.status == 0);
    for (int r = 0; r <= n; r++) REQUIRE(s.rp_d[r] + s.rp_o[r] == rp[r]);
    for (size_t k = 0; k < s.garray.size(); k++) REQUIRE((k == 0 || s.garray[k - 1] < s.garray[k]) && (s.garray[k] < r0 || s.garray[k] >= r0 + n));
    for (int r = 0; r < n; r++) {                              // entry by entry, in stored order
      int d = s.rp_d[r], o = s.rp_o[r];
      for (int e = rp[r]; e < rp[r + 1]; e++) {
        const int c = A.col[e0 + e];
        if (c >= r0 && c < r0 + n) { REQUIRE(s.col_d[d] == c - r0 && s.val_d[d] == A.val[e0 + e]); d++; }
        else { REQUIRE(s.garray[s.col_o[o]] == c && s.val_o[o] == A.val[e0 + e]); o++; }
      }
      REQUIRE(d == s.rp_d[r + 1] && o == s.rp_o[r + 1]);
    }
    std::vector<int> cnt;
    REQUIRE(ksc::halo_recv_counts(s.garray, starts, p, cnt) == 0);
    REQUIRE((int)cnt.size() == size);
    for (int q = 0; q < size; q++) all_cnt[(size_t)p * size + q] = cnt[q];          // the allgather
  }
  if (local_only >= 0) REQUIRE(split[local_only].garray.empty() && counts[local_only] > 0);
  std::vector<ksc::HaloPeers> h(size);
  for (int p = 0; p < size; p++) {
    ksc::halo_peers(p, size, all_cnt.data() + (size_t)p * size, all_cnt.data(), h[p]);
    const ksc::HaloPeers &x = h[p];
    int roff = 0, soff = 0;
    for (size_t i = 0; i < x.peers.size(); i++) {              // offsets: the prefix sums of the counts
      REQUIRE(x.peers[i] != p && (i == 0 || x.peers[i - 1] < x.peers[i]) && (x.recv_cnt[i] > 0 || x.send_cnt[i] > 0));
      REQUIRE(x.recv_off[i] == roff && x.send_off[i] == soff);
      roff += x.recv_cnt[i]; soff += x.send_cnt[i];
    }
    REQUIRE(roff == (int)split[p].garray.size() && soff == x.nsend);
    for (size_t k = 0; k < split[p].garray.size(); k++) {      // every ghost in exactly one peer's segment, and that peer owns it
      int found = 0;
      for (size_t i = 0; i < x.peers.size(); i++)
        if ((int)k >= x.recv_off[i] && (int)k < x.recv_off[i] + x.recv_cnt[i]) { found++; const int q = x.peers[i]; REQUIRE(split[p].garray[k] >= starts[q] && split[p].garray[k] < starts[q + 1]); }
      REQUIRE(found == 1);
    }
  }
  for (int p = 0; p < size; p++) {                             // the exchange of ids, then send_idx of p for q is q's segment for p
    std::vector<int> sidx((size_t)h[p].nsend, -1);
    for (size_t i = 0; i < h[p].peers.size(); i++) {
      const int q = h[p].peers[i];
      int j = -1;
      for (size_t t = 0; t < h[q].peers.size(); t++) if (h[q].peers[t] == p) j = (int)t;
      REQUIRE(j >= 0 && h[q].recv_cnt[j] == h[p].send_cnt[i] && h[q].send_cnt[j] == h[p].recv_cnt[i]);
      for (int t = 0; t < h[p].send_cnt[i]; t++) sidx[(size_t)h[p].send_off[i] + t] = split[q].garray[(size_t)h[q].recv_off[j] + t];
    }
    const std::vector<int> ids = sidx;
    REQUIRE(ksc::halo_localize_send_idx(starts[p], counts[p], h[p].nsend, sidx.data()) == 0);
    for (int e = 0; e < h[p].nsend; e++) REQUIRE(sidx[e] == ids[e] - starts[p] && sidx[e] >= 0 && sidx[e] < counts[p]);
  }
  std::printf("ok %s\n", name.c_str());
}

static void rejections()
{
  const std::string name = "rejections";
  ksc::BlockSplit s;
  const int rp_bad[] = {0, 2, 1, 3}, rp[] = {0, 1, 2, 3}, col[] = {0, 1, 3}; const double val[] = {1.0, 2.0, 3.0};
  ksc::csr_split_block(3, 0, 3, rp_bad, col, val, s); REQUIRE(s.status == ksc::SPLIT_ROWPTR && s.bad_row == 1);
  ksc::csr_split_block(3, 0, 3, rp, col, val, s); REQUIRE(s.status == ksc::SPLIT_COLUMN && s.bad_row == 2 && s.bad_col == 3);
  std::vector<int> cnt;
  REQUIRE(ksc::halo_recv_counts({1}, {0, 5, 3, 10}, 0, cnt) == ksc::HALO_UNORDERED);
  REQUIRE(ksc::halo_recv_counts({1, 4}, {0, 3, 6, 9}, 1, cnt) == ksc::HALO_SELF);
  int ids[] = {3, 6};
  REQUIRE(ksc::halo_localize_send_idx(3, 3, 2, ids) == ksc::HALO_NOT_OWNED);
  ksc::BinnedGeometry g;
  ksc::binned_geometry(300000, 1000000, 1, 1 << 20, 8, g); REQUIRE(g.status == ksc::BINNED_16BIT && g.wr + 1 > 65535);
  std::printf("ok %s\n", name.c_str());
}

static void binned(const std::string &name, int n, int ncu)
{
  const Csr A = random_rows(n, n, 12);
  std::vector<double> x((size_t)n), y((size_t)n, -1.0);
  for (double &v : x) v = (double)((int)lcg(129) - 64);
  ksc::BinnedGeometry g; ksc::BinnedPlan p;
  ksc::binned_geometry(n, A.rp[n], ncu, 9984, 8, g);
  REQUIRE(g.status == 0 && g.ns % ncu == 0 && (long long)g.ns * g.cs >= n && (long long)g.wb * g.wr >= n);
  ksc::binned_plan(n, A.rp.data(), A.col.data(), A.val.data(), g, 8, p);
  REQUIRE(p.status == 0 && p.sbase[g.ns] == p.entries && (long long)p.val2.size() == p.entries);
  ksc::binned_apply_host(p, g, n, x.data(), y.data());
  for (int r = 0; r < n; r++) { double s = 0.0; for (int e = A.rp[r]; e < A.rp[r + 1]; e++) s += A.val[e] * x[A.col[e]]; REQUIRE(y[r] == s); }
  std::printf("ok %s: %d slices of %d columns, %d wave-bins of %d rows, %lld entries for %d\n", name.c_str(), g.ns, g.cs, g.wb, g.wr, p.entries, A.rp[n]);
}

int main()
{
  world("4 ranks, 5 0 3 8 rows", {5, 0, 3, 8});
  world("8 ranks with a 0-row and a 1-row rank", {4, 0, 1, 6, 3, 7, 2, 5});
  world("3 ranks, one without ghosts", {6, 4, 5}, 1);
  rejections();
  binned("binned n 4096 on 4 CUs", 4096, 4);
  binned("binned n 4500 on 256 CUs", 4500, 256);
  if (fails) return 1;
  std::printf("all ok\n");
  return 0;
}
