#include "ks_csr.h"
#include <algorithm>
#include <cmath>
#include <functional>
#include <thread>
#include <sched.h>
#include <system_error>

#pragma clang fp contract(off)      // p_ij = a_ij + (alpha * b_ij): the product is rounded before the sum, as two MatSetValues would

namespace ksc {
namespace {
struct RowB { const int *c; const double *v; int len; int idc; double idv; };      // a row of B, or the one diagonal entry of I
inline bool ascending(const int *c, int len) { for (int i = 1; i < len; i++) if (c[i] <= c[i - 1]) return false; return true; }

// one row; out == nullptr: count only. Returns the row's length.
inline int merge_row(const int *ca, const double *va, int la, const int *cb, const double *vb, int lb, double alpha, int *oc, double *ov)
{
  if (ascending(ca, la) && ascending(cb, lb)) {
    int i = 0, j = 0, k = 0;
    while (i < la || j < lb) {
      if (j >= lb || (i < la && ca[i] < cb[j])) { if (oc) { oc[k] = ca[i]; ov[k] = va[i]; } i++; }
      else if (i >= la || cb[j] < ca[i]) { if (oc) { oc[k] = cb[j]; const double t = alpha * vb[j]; ov[k] = t; } j++; }
      else { if (oc) { oc[k] = ca[i]; const double t = alpha * vb[j]; ov[k] = va[i] + t; } i++; j++; }
      k++;
    }
    return k;
  }
  int k = la;
  if (oc) for (int i = 0; i < la; i++) { oc[i] = ca[i]; ov[i] = va[i]; }
  for (int j = 0; j < lb; j++) {
    int hit = -1;
    for (int i = 0; i < la && hit < 0; i++) if (ca[i] == cb[j]) hit = i;
    if (!oc) { if (hit < 0) k++; continue; }
    const double t = alpha * vb[j];
    if (hit >= 0) ov[hit] = ov[hit] + t; else { oc[k] = cb[j]; ov[k] = t; k++; }
  }
  return k;
}

// helper threads: the CPUs this process may run on (affinity mask: what a cgroup / taskset leaves), at most 16
unsigned helper_threads()
{
  unsigned ncpu = std::thread::hardware_concurrency();
  { cpu_set_t cs; CPU_ZERO(&cs); if (sched_getaffinity(0, sizeof(cs), &cs) == 0 && CPU_COUNT(&cs) > 0) ncpu = (unsigned)CPU_COUNT(&cs); }
  return std::max(1u, std::min(16u, ncpu));
}
// fn(i) for every i in [0, count) on nthr threads, the calling one included: thread t takes i = t, t + nthr, ... A thread that cannot be started
// (pids limit) is simply not used - the calling thread takes every stride that has no thread of its own
template <class F> void parallel_strides(unsigned nthr, int count, const F &fn)
{
  std::vector<std::thread> th;
  unsigned started = 1;                                   // stride 0 belongs to the calling thread
  for (unsigned t = 1; t < nthr; t++) {
    try { th.emplace_back([&fn, t, nthr, count] { for (int i = (int)t; i < count; i += (int)nthr) fn(i); }); started = t + 1; }
    catch (const std::system_error &) { break; }
  }
  for (int i = 0; i < count; i += (int)nthr) fn(i);
  for (unsigned t = started; t < nthr; t++) for (int i = (int)t; i < count; i += (int)nthr) fn(i);      // strides whose thread did not start
  for (auto &x : th) x.join();
}
} // namespace

bool csr_axpy(int n, int row_start, const int *rpa, const int *ca, const double *va, double alpha, const int *rpb, const int *cb, const double *vb,
              std::vector<int> &rp, std::vector<int> &col, std::vector<double> &val)
{
  rp.assign((size_t)n + 1, 0);
  const unsigned nthr = (n < 100000) ? 1u : helper_threads();
  const double one = 1.0;
  auto rows = [&](bool fill, int r0, int r1) {
    for (int r = r0; r < r1; r++) {
      const int id = row_start + r;
      const int *bc = rpb ? cb + rpb[r] : &id; const double *bv = rpb ? vb + rpb[r] : &one; const int lb = rpb ? rpb[r + 1] - rpb[r] : 1;
      if (!fill) rp[r + 1] = merge_row(ca + rpa[r], va + rpa[r], rpa[r + 1] - rpa[r], bc, bv, lb, alpha, nullptr, nullptr);
      else merge_row(ca + rpa[r], va + rpa[r], rpa[r + 1] - rpa[r], bc, bv, lb, alpha, col.data() + rp[r], val.data() + rp[r]);
    }
  };
  const int chunk = (n + (int)nthr - 1) / (int)nthr;         // a chunk of rows per thread
  auto parallel = [&](bool fill) { parallel_strides(nthr, (int)nthr, [&](int t) { rows(fill, std::min(n, t * chunk), std::min(n, (t + 1) * chunk)); }); };
  parallel(false);
  long long total = 0;
  for (int r = 0; r < n; r++) total += rp[r + 1];
  if (total > 2147483647LL) return false;
  for (int r = 0; r < n; r++) rp[r + 1] += rp[r];
  col.resize((size_t)rp[n]); val.resize((size_t)rp[n]);
  parallel(true);
  return true;
}
void csr_transpose(int nrows, int ncols, const int *rp, const int *col, const double *val, std::vector<int> &rpt, std::vector<int> &colt, std::vector<double> &valt)
{
  const size_t nnz = (size_t)rp[nrows];
  rpt.assign((size_t)ncols + 1, 0); colt.resize(nnz); valt.resize(nnz);
  for (size_t p = 0; p < nnz; p++) rpt[(size_t)col[p] + 1]++;
  for (int c = 0; c < ncols; c++) rpt[c + 1] += rpt[c];
  std::vector<int> cur(rpt.begin(), rpt.end() - 1);
  for (int r = 0; r < nrows; r++)
    for (int p = rp[r]; p < rp[r + 1]; p++) { const int q = cur[col[p]]++; colt[q] = r; valt[q] = val[p]; }
}
void sharded_transpose_plan(int n, int row_start, const int *rp, const int *col, const double *val, int nghost, const int *ghosts,
                            int nsend, const int *send_idx, ShardedTransposePlan &out)
{
  out = ShardedTransposePlan();
  // split the rows as the assembly does: local columns to the diagonal block, the others to their position in the sorted ghost list
  std::vector<int> rpd((size_t)n + 1, 0), rpo((size_t)n + 1, 0), cd, co; std::vector<double> vd, vo;
  for (int r = 0; r < n; r++) {
    for (int p = rp[r]; p < rp[r + 1]; p++) {
      const long long c = (long long)col[p] - row_start;
      if (c >= 0 && c < n) { cd.push_back((int)c); vd.push_back(val[p]); }
      else { co.push_back((int)(std::lower_bound(ghosts, ghosts + nghost, col[p]) - ghosts)); vo.push_back(val[p]); }
    }
    rpd[r + 1] = (int)cd.size(); rpo[r + 1] = (int)co.size();
  }
  csr_transpose(n, n, rpd.data(), cd.data(), vd.data(), out.d_rp, out.d_col, out.d_val);
  csr_transpose(n, nghost, rpo.data(), co.data(), vo.data(), out.o_rp, out.o_row, out.o_val);
  // the inverse of send_idx, by the same stable counting sort: positions of a row come out ascending
  std::vector<int> cnt((size_t)n + 1, 0);
  for (int e = 0; e < nsend; e++) cnt[(size_t)send_idx[e] + 1]++;
  out.acc_ptr.assign(1, 0);
  std::vector<int> slot((size_t)n, -1);
  for (int r = 0; r < n; r++) if (cnt[(size_t)r + 1]) { slot[r] = (int)out.acc_rows.size(); out.acc_rows.push_back(r); out.acc_ptr.push_back(out.acc_ptr.back() + cnt[(size_t)r + 1]); }
  out.acc_pos.resize((size_t)nsend);
  std::vector<int> cur(out.acc_ptr.begin(), out.acc_ptr.end() - 1);
  for (int e = 0; e < nsend; e++) out.acc_pos[(size_t)cur[slot[send_idx[e]]]++] = e;
}
void sharded_transpose_local_host(const ShardedTransposePlan &p, int n, int nghost, const double *x, double *rsend, double *y)
{
  for (int g = 0; g < nghost; g++) { double acc = 0.0; for (int q = p.o_rp[g]; q < p.o_rp[g + 1]; q++) acc = __builtin_fma(p.o_val[q], x[p.o_row[q]], acc); rsend[g] = acc; }
  for (int c = 0; c < n; c++) { double acc = 0.0; for (int q = p.d_rp[c]; q < p.d_rp[c + 1]; q++) acc = __builtin_fma(p.d_val[q], x[p.d_col[q]], acc); y[c] = acc; }
}
void sharded_transpose_add_host(const ShardedTransposePlan &p, const double *rrecv, double *y)
{
  for (size_t i = 0; i < p.acc_rows.size(); i++) { double s = y[p.acc_rows[i]]; for (int q = p.acc_ptr[i]; q < p.acc_ptr[i + 1]; q++) s = s + rrecv[p.acc_pos[q]]; y[p.acc_rows[i]] = s; }
}
void csr_split_block(int n_local, int row_start, int n_global, const int *rowptr, const int *col, const double *val, BlockSplit &out)
{
  out = BlockSplit();
  const long long nnz = rowptr[n_local];
  std::vector<int> &cd = out.col_d, &co = out.col_o; std::vector<double> &vd = out.val_d, &vo = out.val_o;
  out.rp_d.assign((size_t)n_local + 1, 0); out.rp_o.assign((size_t)n_local + 1, 0);
  if (nnz > 0) { cd.reserve((size_t)nnz); vd.reserve((size_t)nnz); }
  for (int r = 0; r < n_local; r++) {
    if (rowptr[r + 1] < rowptr[r]) { out.status = SPLIT_ROWPTR; out.bad_row = r; return; }
    for (int p = rowptr[r]; p < rowptr[r + 1]; p++) {
      const int c = col[p];
      if (c < 0 || c >= n_global) { out.status = SPLIT_COLUMN; out.bad_row = r; out.bad_col = c; return; }
      if (c >= row_start && c < row_start + n_local) { cd.push_back(c - row_start); vd.push_back(val[p]); }
      else { co.push_back(c); vo.push_back(val[p]); }
    }
    out.rp_d[r + 1] = (int)cd.size(); out.rp_o[r + 1] = (int)co.size();
  }
  out.garray = co;
  std::sort(out.garray.begin(), out.garray.end()); out.garray.erase(std::unique(out.garray.begin(), out.garray.end()), out.garray.end());
  for (auto &c : co) c = (int)(std::lower_bound(out.garray.begin(), out.garray.end(), c) - out.garray.begin());
}
int halo_recv_counts(const std::vector<int> &garray, const std::vector<int> &starts, int rank, std::vector<int> &recv_cnt)
{
  const int size = (int)starts.size() - 1;
  recv_cnt.assign((size_t)size, 0);
  for (int p = 0; p < size; p++) if (starts[p] > starts[p + 1]) return HALO_UNORDERED;
  int p = 0;
  for (int g : garray) { while (p + 1 < size && g >= starts[p + 1]) p++; if (p == rank) return HALO_SELF; recv_cnt[p]++; }
  return 0;
}
void halo_peers(int rank, int size, const int *recv_cnt, const int *all_cnt, HaloPeers &out)
{
  out = HaloPeers();
  int roff = 0, soff = 0;
  for (int p = 0; p < size; p++) {
    const int send = (p == rank) ? 0 : all_cnt[(size_t)p * size + rank];      // what p receives from this rank
    if (p == rank || (recv_cnt[p] == 0 && send == 0)) continue;
    out.peers.push_back(p); out.recv_cnt.push_back(recv_cnt[p]); out.send_cnt.push_back(send); out.recv_off.push_back(roff); out.send_off.push_back(soff);
    roff += recv_cnt[p]; soff += send;
  }
  out.nsend = soff;
}
int halo_localize_send_idx(int row_start, int n, int nsend, int *sidx)
{
  for (int i = 0; i < nsend; i++) { sidx[i] -= row_start; if (sidx[i] < 0 || sidx[i] >= n) return HALO_NOT_OWNED; }
  return 0;
}

void binned_geometry(int n, long long nnz, int ncu, int cs_max, int seg_pad, BinnedGeometry &out)
{
  out = BinnedGeometry();
  ncu = std::max(ncu, 1);
  const long long per_round = (long long)ncu * cs_max;
  out.ns = (int)(ncu * std::max(1LL, (n + per_round - 1) / per_round));
  out.cs = (n + out.ns - 1) / out.ns;
  out.wb = 4 * out.ns; out.wr = (n + out.wb - 1) / out.wb;
  if (out.cs > 65535 || out.wr + 1 > 65535) out.status = BINNED_16BIT;
  else if (nnz + (long long)out.ns * out.wb * (seg_pad - 1) >= 2147483647LL) out.status = BINNED_32BIT;      // bin-major positions are 32-bit
}
void binned_plan(int n, const int *rp, const int *col, const double *val, const BinnedGeometry &g, int seg_pad, BinnedPlan &out)
{
  out = BinnedPlan();
  const int ns = g.ns, cs = g.cs, wb = g.wb, wr = g.wr;
  const unsigned nthr = helper_threads();                 // the counting sort per wave-bin is cache friendly and runs on a few threads
  // segment lengths (padded to seg_pad entries), bin-major [wb][ns]
  std::vector<int> len((size_t)wb * ns, 0);
  parallel_strides(nthr, wb, [&](int b) {
    int *L = len.data() + (size_t)b * ns;
    const int r0 = std::min((long long)b * wr, (long long)n), r1 = std::min((long long)(b + 1) * wr, (long long)n);
    for (int p = rp[r0]; p < rp[r1]; p++) L[col[p] / cs]++;
    for (int s = 0; s < ns; s++) L[s] = (L[s] + seg_pad - 1) / seg_pad * seg_pad;
  });
  // Bin-major order, GROUPED: `grp` consecutive wave-bins are interleaved slice by slice - [group][slice][wave-bin of the group]
  // - so that the segments a slice's workgroup writes in phase 1 for `grp` consecutive wave-bins are one contiguous run (80 KB instead of 64
  // pieces of 1.26 KB, each 0.6 MB from the next; the gather is store-bound: 436 -> 316-331 us in the stand-alone benchmark with uniform
  // segments, profiles/r03_micro_binned_group.txt).
  // A wave-bin's own entries are then no longer one stream but ns pieces: phase 2 walks them through a LOGICAL position (piece after piece)
  // that a per-wave-bin table log2[wb][ns + 1] maps to the physical one (off2), window by window, the way phase 1 finds its destinations.
  std::vector<int> &off2 = out.off2, &log2 = out.log2, &off1 = out.off1, &off2t = out.off2t, &wseg = out.wseg;
  std::vector<long long> &sbase = out.sbase;
  off2.resize((size_t)wb * ns);                           // physical start of segment (wb, s)
  log2.resize((size_t)wb * (ns + 1));                     // logical start of segment (wb, s) inside wave-bin wb; [ns]: the wave-bin's entry count
  long long run = 0;
  // wave-bins whose segments are adjacent per slice. Measured on config 5's matrix, one box (profiles/r03_ab_binned_groups.txt), phase 1 +
  // phase 2: 1 (the old order): 445 + 488 us; 4: 404 + 507; 16: 390 + 511; 64: 386 + 500; 256: 388 + 511 - the gather gains what its
  // stores gain from longer runs, the reduce pays a little for reading its pieces further apart.
  int grp = 64; while (grp > 1 && wb % grp) grp /= 2;
  for (int gi = 0; gi < wb / grp; gi++)
    for (int s = 0; s < ns; s++)
      for (int wl = 0; wl < grp; wl++) { const int b = grp * gi + wl; off2[(size_t)b * ns + s] = (int)run; run += len[(size_t)b * ns + s]; }
  const long long entries = out.entries = run;
  for (int b = 0; b < wb; b++) {
    int lrun = 0;
    for (int s = 0; s < ns; s++) { log2[(size_t)b * (ns + 1) + s] = lrun; lrun += len[(size_t)b * ns + s]; }
    log2[(size_t)b * (ns + 1) + ns] = lrun;
  }
  off1.resize((size_t)ns * (wb + 1)); off2t.resize((size_t)ns * wb); sbase.resize((size_t)ns + 1);
  long long srun = 0; int nwin = 1;
  for (int s = 0; s < ns; s++) {
    sbase[s] = srun;
    int lrun = 0;
    for (int b = 0; b < wb; b++) { off1[(size_t)s * (wb + 1) + b] = lrun; off2t[(size_t)s * wb + b] = off2[(size_t)b * ns + s]; lrun += len[(size_t)b * ns + s]; }
    off1[(size_t)s * (wb + 1) + wb] = lrun;
    srun += lrun;
    nwin = std::max(nwin, (lrun + 1023) / 1024);
  }
  sbase[ns] = srun; out.nwin = nwin;
  if (srun != entries) { out.status = BINNED_ORDERS; return; }
  wseg.assign((size_t)ns * nwin, 0);
  for (int s = 0; s < ns; s++) {
    const int *o1 = off1.data() + (size_t)s * (wb + 1);
    int sg = 0;
    for (int wdw = 0; wdw < nwin; wdw++) {
      const int base = wdw * 1024;
      while (sg < wb - 1 && o1[sg + 1] <= base) sg++;
      wseg[(size_t)s * nwin + wdw] = sg;
    }
  }
  std::vector<double> &val2 = out.val2; std::vector<unsigned short> &row16 = out.row16, &col16 = out.col16;
  val2.assign((size_t)entries, 0.0);
  row16.assign((size_t)entries, (unsigned short)wr); col16.assign((size_t)entries, 0);      // padding: value 0 into the spare accumulator, column 0 of its slice
  parallel_strides(nthr, wb, [&](int b) {
    std::vector<int> cur(ns, 0);
    const int r0 = std::min((long long)b * wr, (long long)n), r1 = std::min((long long)(b + 1) * wr, (long long)n);
    for (int r = r0; r < r1; r++)
      for (int p = rp[r]; p < rp[r + 1]; p++) {
        const int s = col[p] / cs, i = cur[s]++;
        const long long p2 = (long long)off2[(size_t)b * ns + s] + i;
        val2[p2] = val[p]; row16[p2] = (unsigned short)(r - r0);
        col16[sbase[s] + off1[(size_t)s * (wb + 1) + b] + i] = (unsigned short)(col[p] - s * cs);
      }
  });
}
void binned_apply_host(const BinnedPlan &p, const BinnedGeometry &g, int n, const double *x, double *y)
{
  const int ns = g.ns, cs = g.cs, wb = g.wb, wr = g.wr;
  std::vector<double> G((size_t)p.entries, 0.0), xs((size_t)cs), acc((size_t)wr + 1);
  for (int s = 0; s < ns; s++) {                          // k_binned_gather: a workgroup per slice
    const long long c0 = (long long)s * cs;
    for (int i = 0; i < cs; i++) xs[i] = (c0 + i < n) ? x[c0 + i] : 0.0;
    const int *o1 = p.off1.data() + (size_t)s * (wb + 1), *o2 = p.off2t.data() + (size_t)s * wb;
    const unsigned short *cg = p.col16.data() + p.sbase[s];
    const int total = o1[wb];
    for (int win = 0; win * 1024 < total; win++) {
      int sg = p.wseg[(size_t)s * p.nwin + win];          // the segment of the window's first entry; the others are found from there
      for (int e = win * 1024; e < std::min(total, (win + 1) * 1024); e++) { while (e >= o1[sg + 1]) sg++; G[(size_t)((long long)e + (o2[sg] - o1[sg]))] = xs[cg[e]]; }
    }
  }
  for (int b = 0; b < wb; b++) {                          // k_binned_reduce: a wave per wave-bin
    std::fill(acc.begin(), acc.end(), 0.0);
    const int *lg = p.log2.data() + (size_t)b * (ns + 1), *ph = p.off2.data() + (size_t)b * ns;
    for (int s = 0; s < ns; s++)
      for (long long q = ph[s]; q < (long long)ph[s] + (lg[s + 1] - lg[s]); q++) acc[p.row16[(size_t)q]] += p.val2[(size_t)q] * G[(size_t)q];
    for (int i = 0; i < wr; i++) { const long long row = (long long)b * wr + i; if (row < n) y[row] = acc[i]; }
  }
}

void csr_window_plan(int n, const int *rp, const int *col, int block_rows, int max_segments, int pad, WindowPlan &out)
{
  out = WindowPlan();
  const long long nnz = n > 0 ? rp[n] : 0;
  const long long blocks = ((long long)n + block_rows - 1) / block_rows;
  const int nsegs = (n + 63) / 64;
  out.blocks = blocks;
  out.nseg.assign((size_t)blocks, 0); out.segptr.assign((size_t)blocks + 1, 0); out.dbase.assign((size_t)blocks, WIN_NOT_DIRECT);
  out.codes.assign((size_t)nnz + pad, 0);
  std::vector<long long> stamp((size_t)nsegs, -1);        // the last block that referenced the segment
  std::vector<int> slot((size_t)nsegs, 0), list;
  long long drun = 0;
  for (long long b = 0; b < blocks; b++) {
    const int r0 = (int)(b * block_rows), r1 = (int)std::min<long long>((long long)n, (b + 1) * block_rows);
    const int e0 = rp[r0], e1 = rp[r1];
    list.clear();
    for (int e = e0; e < e1; e++) { const int s = col[e] >> 6; if (stamp[s] != b) { stamp[s] = b; list.push_back(s); } }
    out.nseg[b] = (int)list.size();
    if ((int)list.size() <= max_segments) {
      std::sort(list.begin(), list.end());
      for (size_t i = 0; i < list.size(); i++) slot[list[i]] = (int)i;
      out.seg.insert(out.seg.end(), list.begin(), list.end());
      out.window_entries += e1 - e0;
      for (int e = e0; e < e1; e++) out.codes[e] = (unsigned short)(slot[col[e] >> 6] * 64 + (col[e] & 63));
    } else {
      const long long start = (drun + 3) / 4 * 4 + (e0 & 3);      // start = e0 (mod 4)
      out.dbase[b] = (int)(start - e0);
      drun = start + (e1 - e0);
      out.direct_blocks++; out.direct_entries += e1 - e0;
      out.dcol.resize((size_t)drun, 0); std::copy(col + e0, col + e1, out.dcol.begin() + start);
    }
    out.segptr[b + 1] = (int)out.seg.size();
  }
  out.total_segments = (long long)out.seg.size();
  out.dcol.resize((size_t)drun + pad, 0);
}
namespace {
struct IluLevelScratch { std::vector<int> level, count, start, order, where; };
// Level sets and the ELL image of each level for the two triangular solves of one block, appended to `out`: pass 0 = the entries left of the
// diagonal (levels ascending from row 0), pass 1 = the entries right of it (ascending from the last row). scale_pass: the pass whose rows are
// multiplied by the reciprocal of their diagonal entry (1: the forward solve, U; 0: the transposed solve, U^T); dinv is in that pass's level order.
void ilu_block_levels(int b, int b0, int bl, const std::vector<int> &brp, const std::vector<int> &bcol, const std::vector<double> &bval, const std::vector<int> &diag,
                      int scale_pass, IluPlan &out, IluLevelScratch &sc)
{
  std::vector<int> &level = sc.level, &count = sc.count, &start = sc.start, &order = sc.order, &where = sc.where;
  out.blk[b].ell = (long long)out.val.size(); out.blk[b].lev = (int)(out.lev.size() / 2); out.blk[b].pad = 0;
  level.assign((size_t)bl, 0); order.resize((size_t)bl);
  for (int pass = 0; pass < 2; pass++) {
    int nlev = 0;
    for (int s = 0; s < bl; s++) {
      const int i = pass == 0 ? s : bl - 1 - s;
      const int e0 = pass == 0 ? brp[i] : diag[i] + 1, e1 = pass == 0 ? diag[i] : brp[i + 1];
      int lv = 0;
      for (int p = e0; p < e1; p++) lv = std::max(lv, level[bcol[p]] + 1);
      level[i] = lv; nlev = std::max(nlev, lv + 1);
    }
    count.assign((size_t)nlev, 0); start.assign((size_t)nlev + 1, 0); where.assign((size_t)nlev, 0);
    for (int i = 0; i < bl; i++) count[level[i]]++;
    for (int l = 0; l < nlev; l++) { start[l + 1] = start[l] + count[l]; where[l] = start[l]; }
    for (int i = 0; i < bl; i++) order[where[level[i]]++] = i;
    unsigned short *rows = out.rows.data() + (size_t)2 * b0 + (size_t)pass * bl;
    for (int l = 0; l < nlev; l++) {
      const int nl = count[l];
      int w = 0;
      for (int p = start[l]; p < start[l + 1]; p++) { const int i = order[p]; w = std::max(w, pass == 0 ? diag[i] - brp[i] : brp[i + 1] - diag[i] - 1); }
      const size_t base = out.val.size();
      out.val.resize(base + (size_t)nl * w, 0.0); out.code.resize(base + (size_t)nl * w, 0);
      for (int p = 0; p < nl; p++) {
        const int i = order[start[l] + p];
        rows[start[l] + p] = (unsigned short)i;
        if (pass == scale_pass) out.dinv[(size_t)b0 + start[l] + p] = 1.0 / bval[diag[i]];
        const int e0 = pass == 0 ? brp[i] : diag[i] + 1, e1 = pass == 0 ? diag[i] : brp[i + 1];
        for (int s = 0; s < w; s++) {
          const size_t at = base + (size_t)s * nl + p;
          if (e0 + s < e1) { out.val[at] = bval[e0 + s]; out.code[at] = (unsigned short)bcol[e0 + s]; }
          else out.code[at] = (unsigned short)i;
        }
      }
      out.lev.push_back(nl); out.lev.push_back(w);
    }
    (pass == 0 ? out.blk[b].nL : out.blk[b].nU) = nlev;
  }
}
} // namespace
void csr_ilu0_blocks(int n, int row_start, int bs, const int *rp, const int *col, const double *val, bool keep_factors, IluPlan &out, IluPlan *tr)
{
  out = IluPlan();
  const int nblk = (int)(((long long)n + bs - 1) / bs);
  out.blk.resize((size_t)nblk); out.rows.assign((size_t)2 * n, 0); out.dinv.assign((size_t)n, 0.0);
  if (keep_factors) out.frp.assign(1, 0);
  if (tr) { *tr = IluPlan(); tr->blk.resize((size_t)nblk); tr->rows.assign((size_t)2 * n, 0); tr->dinv.assign((size_t)n, 0.0); }
  std::vector<int> brp, bcol, diag, pos, perm, trp, tcol, tdiag;
  std::vector<double> bval, tval;
  IluLevelScratch sc;
  for (int b = 0; b < nblk; b++) {
    const int b0 = b * bs, bl = std::min(bs, n - b0);
    const long long c0 = (long long)row_start + b0;
    // the block on its sorted pattern
    brp.assign((size_t)bl + 1, 0); bcol.clear(); bval.clear(); diag.assign((size_t)bl, -1);
    for (int r = 0; r < bl; r++) {
      perm.clear();
      for (int p = rp[b0 + r]; p < rp[b0 + r + 1]; p++) { const long long c = (long long)col[p] - c0; if (c >= 0 && c < bl) perm.push_back(p); }
      std::stable_sort(perm.begin(), perm.end(), [&](int x, int y) { return col[x] < col[y]; });
      for (size_t i = 0; i < perm.size(); i++) {
        const int c = (int)((long long)col[perm[i]] - c0);
        if (i > 0 && col[perm[i]] == col[perm[i - 1]]) { bval.back() = bval.back() + val[perm[i]]; continue; }
        if (c == r) diag[r] = (int)bcol.size();
        bcol.push_back(c); bval.push_back(val[perm[i]]);
      }
      brp[r + 1] = (int)bcol.size();
      out.longest_row = std::max(out.longest_row, brp[r + 1] - brp[r]);
      if (diag[r] < 0) { out.status = ILU_NO_DIAGONAL; out.bad_block = b; out.bad_row = b0 + r; return; }
    }
    // ILU(0), IKJ
    pos.assign((size_t)bl, -1);
    for (int i = 0; i < bl; i++) {
      for (int p = brp[i]; p < brp[i + 1]; p++) pos[bcol[p]] = p;
      for (int p = brp[i]; p < diag[i]; p++) {
        const int k = bcol[p];
        const double l = bval[p] / bval[diag[k]];
        bval[p] = l;
        for (int q = diag[k] + 1; q < brp[k + 1]; q++) { const int t = pos[bcol[q]]; if (t >= 0) { const double m = l * bval[q]; bval[t] = bval[t] - m; } }
      }
      for (int p = brp[i]; p < brp[i + 1]; p++) pos[bcol[p]] = -1;
      if (bval[diag[i]] == 0.0) { out.status = ILU_ZERO_PIVOT; out.bad_block = b; out.bad_row = b0 + i; return; }
    }
    if (keep_factors) {
      out.fcol.insert(out.fcol.end(), bcol.begin(), bcol.end()); out.fval.insert(out.fval.end(), bval.begin(), bval.end());
      for (int r = 0; r < bl; r++) out.frp.push_back(out.frp.back() + brp[r + 1] - brp[r]);
    }
    ilu_block_levels(b, b0, bl, brp, bcol, bval, diag, 1, out, sc);
    if (tr) {
      // the transposed triangles from the same factors: row r of the transposed block lists column r of the factors in ascending original row
      // (the counting sort of csr_transpose) - u_cr for c < r, the pivot u_rr, then l_cr for c > r. U^T (lower, with the pivots) is solved
      // first and carries the scaling, L^T (unit upper) second; the levels are those of the transposed triangles
      csr_transpose(bl, bl, brp.data(), bcol.data(), bval.data(), trp, tcol, tval);
      tdiag.assign((size_t)bl, -1);
      for (int r = 0; r < bl; r++) {
        for (int p = trp[r]; p < trp[r + 1]; p++) if (tcol[p] == r) { tdiag[r] = p; break; }
        tr->longest_row = std::max(tr->longest_row, trp[r + 1] - trp[r]);
      }
      ilu_block_levels(b, b0, bl, trp, tcol, tval, tdiag, 0, *tr, sc);
    }
  }
}
namespace {
// the level walk of both kernels: `first_scaled` says which of the block's two runs of levels multiplies by dinv (the second: forward, the first: transposed)
void ilu0_walk_host(const IluPlan &p, int n, int bs, bool first_scaled, const double *in, double *out)
{
  std::vector<double> x;
  for (size_t b = 0; b < p.blk.size(); b++) {
    const int b0 = (int)b * bs, bl = std::min(bs, n - b0);
    x.assign(in + b0, in + b0 + bl);
    const double *v = p.val.data() + p.blk[b].ell; const unsigned short *c = p.code.data() + p.blk[b].ell;
    const unsigned short *rows = p.rows.data() + (size_t)2 * b0; const double *dinv = p.dinv.data() + b0;
    for (int l = 0; l < p.blk[b].nL + p.blk[b].nU; l++) {
      const int nl = p.lev[(size_t)2 * (p.blk[b].lev + l)], w = p.lev[(size_t)2 * (p.blk[b].lev + l) + 1];
      const bool upper = first_scaled ? l < p.blk[b].nL : l >= p.blk[b].nL;        // the run of levels with the pivots
      for (int i = 0; i < nl; i++) {
        const int r = rows[i];
        double acc = 0.0;
        for (int s = 0; s < w; s++) acc = __builtin_fma(v[(size_t)s * nl + i], x[c[(size_t)s * nl + i]], acc);
        x[r] = upper ? (x[r] - acc) * dinv[i] : x[r] - acc;
      }
      v += (size_t)nl * w; c += (size_t)nl * w; rows += nl; if (upper) dinv += nl;
    }
    std::copy(x.begin(), x.end(), out + b0);
  }
}
} // namespace
void ilu0_apply_host(const IluPlan &p, int n, int bs, const double *in, double *out) { ilu0_walk_host(p, n, bs, false, in, out); }
void ilu0_apply_transpose_host(const IluPlan &t, int n, int bs, const double *in, double *out) { ilu0_walk_host(t, n, bs, true, in, out); }

// ---- sparse LU with fill (KS_PC_LU) -------------------------------------------------------------------------------------------------------
namespace {
// the rows of P sorted by column, repeated entries summed in stored order, the diagonal position always there (0.0 when the row stores none)
void lu_sorted_rows(int n, const int *rp, const int *col, const double *val, std::vector<int> &srp, std::vector<int> &scol, std::vector<double> &sval)
{
  srp.assign((size_t)n + 1, 0); scol.clear(); sval.clear();
  std::vector<int> idx;
  for (int r = 0; r < n; r++) {
    idx.clear();
    for (int p = rp[r]; p < rp[r + 1]; p++) if (col[p] >= 0 && col[p] < n) idx.push_back(p);
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return col[x] < col[y]; });
    bool has_diag = false;
    for (size_t i = 0; i < idx.size(); i++) {
      const int c = col[idx[i]];
      if (i > 0 && c == col[idx[i - 1]]) { sval.back() = sval.back() + val[idx[i]]; continue; }
      if (!has_diag && c > r) { scol.push_back(r); sval.push_back(0.0); has_diag = true; }
      if (c == r) has_diag = true;
      scol.push_back(c); sval.push_back(val[idx[i]]);
    }
    if (!has_diag) { scol.push_back(r); sval.push_back(0.0); }
    srp[r + 1] = (int)scol.size();
  }
}

// the rooted level structure of `root` inside the nodes with owner[v] == id: order = the nodes level by level, lstart = where the levels start
struct LevelStructure { std::vector<int> order, lstart; int levels() const { return (int)lstart.size() - 1; } };
void rooted_levels(int root, int id, const std::vector<int> &xadj, const std::vector<int> &adj, const std::vector<int> &owner, std::vector<int> &stamp, int &tick, LevelStructure &out)
{
  out.order.clear(); out.lstart.assign(1, 0);
  tick++;
  out.order.push_back(root); stamp[root] = tick;
  size_t done = 0;
  while (done < out.order.size()) {
    const size_t end = out.order.size();
    out.lstart.push_back((int)end);
    for (; done < end; done++) {
      const int v = out.order[done];
      for (int p = xadj[v]; p < xadj[v + 1]; p++) { const int u = adj[p]; if (owner[u] == id && stamp[u] != tick) { stamp[u] = tick; out.order.push_back(u); } }
    }
  }
}

void nested_dissection(int n, const std::vector<int> &xadj, const std::vector<int> &adj, std::vector<int> &perm)
{
  struct Task { bool emit; int id; std::vector<int> nodes; };
  perm.clear(); perm.reserve((size_t)n);
  std::vector<int> owner((size_t)n, 0), stamp((size_t)n, 0);
  int next_id = 1, tick = 0;
  std::vector<Task> stack, todo;
  { Task all{false, 0, {}}; all.nodes.resize((size_t)n); for (int i = 0; i < n; i++) all.nodes[i] = i; stack.push_back(std::move(all)); }
  LevelStructure cur, cand;
  while (!stack.empty()) {
    Task t = std::move(stack.back()); stack.pop_back();
    if (t.emit) { perm.insert(perm.end(), t.nodes.begin(), t.nodes.end()); continue; }
    todo.clear();
    for (int v0 : t.nodes) {                                   // ascending: the components come in the order of their smallest nodes
      if (owner[v0] != t.id) continue;
      // the component of v0: its level structure from v0, the smallest node, finds it
      rooted_levels(v0, t.id, xadj, adj, owner, stamp, tick, cur);
      const int cid = next_id++;
      std::vector<int> comp(cur.order);
      std::sort(comp.begin(), comp.end());
      for (int v : comp) owner[v] = cid;
      if (comp.size() <= 8) { todo.push_back(Task{true, 0, std::move(comp)}); continue; }
      for (int round = 0; round < 5; round++) {
        int best = -1, best_deg = 0;
        for (int p = cur.lstart[cur.levels() - 1]; p < cur.lstart[cur.levels()]; p++) {
          const int v = cur.order[p];
          int deg = 0;
          for (int q = xadj[v]; q < xadj[v + 1]; q++) deg += owner[adj[q]] == cid;
          if (best < 0 || deg < best_deg || (deg == best_deg && v < best)) { best = v; best_deg = deg; }
        }
        rooted_levels(best, cid, xadj, adj, owner, stamp, tick, cand);
        if (cand.levels() <= cur.levels()) break;
        std::swap(cur, cand);
      }
      if (cur.levels() < 3) { todo.push_back(Task{true, 0, std::move(comp)}); continue; }
      const int mid = cur.levels() / 2;
      std::vector<int> sep(cur.order.begin() + cur.lstart[mid], cur.order.begin() + cur.lstart[mid + 1]), rest;
      std::sort(sep.begin(), sep.end());
      for (int v : sep) owner[v] = -1;
      const int rid = next_id++;
      rest.reserve(comp.size() - sep.size());
      for (int v : comp) if (owner[v] == cid) { owner[v] = rid; rest.push_back(v); }
      todo.push_back(Task{false, rid, std::move(rest)});
      todo.push_back(Task{true, 0, std::move(sep)});
    }
    for (size_t i = todo.size(); i-- > 0;) stack.push_back(std::move(todo[i]));
  }
}

struct Tri { std::vector<int> rp, col; std::vector<double> val; };      // the strict part of a triangle by rows, ascending columns

// level sets, level-ordered rows, stages of one triangle (lower: levels ascending from row 0; upper: from the last row), appended to the plan
void lu_triangle_layout(int n, int t, bool lower, bool scaled, const Tri &T, const std::vector<double> &diag, int wide, LuPlan &out)
{
  std::vector<int> level((size_t)n, 0);
  int nlev = 0;
  for (int s = 0; s < n; s++) {
    const int i = lower ? s : n - 1 - s;
    int lv = 0;
    for (int p = T.rp[i]; p < T.rp[i + 1]; p++) lv = std::max(lv, level[T.col[p]] + 1);
    level[i] = lv; nlev = std::max(nlev, lv + 1);
  }
  std::vector<int> start((size_t)nlev + 1, 0), where((size_t)nlev, 0);
  std::vector<long long> entries((size_t)nlev, 0);
  for (int i = 0; i < n; i++) { start[level[i] + 1]++; entries[level[i]] += T.rp[i + 1] - T.rp[i]; }
  for (int l = 0; l < nlev; l++) { start[l + 1] += start[l]; where[l] = start[l]; }
  int *rows = out.rows.data() + (size_t)t * n;
  for (int i = 0; i < n; i++) rows[where[level[i]]++] = i;
  for (int p = 0; p < n; p++) {
    const int i = rows[p];
    out.col.insert(out.col.end(), T.col.begin() + T.rp[i], T.col.begin() + T.rp[i + 1]);
    out.val.insert(out.val.end(), T.val.begin() + T.rp[i], T.val.begin() + T.rp[i + 1]);
    out.rp[(size_t)t * n + p + 1] = (int)out.col.size();
    if (scaled) out.dinv[p] = 1.0 / diag[i];
  }
  const int lev_base = (int)out.lanes.size();
  for (int l = 0; l < nlev; l++) {
    const int nl = start[l + 1] - start[l];
    const bool is_wide = nl >= wide;
    const double mean = (double)entries[l] / nl;
    out.lev.push_back(t * n + start[l]);
    out.lanes.push_back(!is_wide ? 64 : mean <= 2.0 ? 1 : mean <= 16.0 ? 8 : 64);
    if (out.nstage[t] > 0 && out.stages.back().wide == (int)is_wide) out.stages.back().nlev++;
    else { out.stages.push_back(LuStage{lev_base + l, 1, (int)is_wide}); out.nstage[t]++; }
  }
  out.levels[t] = nlev;
}

void lu_layout(int n, int wide, int first_scaled, const Tri &first, const Tri &second, const std::vector<double> &diag, LuPlan &out)
{
  out.n = n; out.wide = wide; out.first_scaled = first_scaled;
  out.rows.assign((size_t)2 * n, 0); out.rp.assign((size_t)2 * n + 1, 0); out.dinv.assign((size_t)n, 0.0);
  out.col.clear(); out.val.clear(); out.lev.clear(); out.lanes.clear(); out.stages.clear();
  out.col.reserve(first.col.size() + second.col.size()); out.val.reserve(first.col.size() + second.col.size());
  out.levels[0] = out.levels[1] = out.nstage[0] = out.nstage[1] = 0;
  if (n > 0) {
    lu_triangle_layout(n, 0, true, first_scaled != 0, first, diag, wide, out);
    lu_triangle_layout(n, 1, false, first_scaled == 0, second, diag, wide, out);
  }
  out.lev.push_back(2 * n);
}

// the sum one group of lanes forms for a row: partial sums of the lanes, then the order of the DPP sums (wave_sum, ks_sweeps.cuh; 8 lanes: the two
// quad steps and the mirror of the half row)
double lu_row_sum(const double *v, const int *c, int len, int lanes, const double *w)
{
  if (lanes == 1) { double acc = 0.0; for (int p = 0; p < len; p++) acc = __builtin_fma(v[p], w[c[p]], acc); return acc; }
  double part[64];
  for (int l = 0; l < lanes; l++) { double acc = 0.0; for (int p = l; p < len; p += lanes) acc = __builtin_fma(v[p], w[c[p]], acc); part[l] = acc; }
  double Q[16];
  for (int k = 0; k < lanes / 4; k++) { const double a = part[4 * k] + part[4 * k + 1], b = part[4 * k + 2] + part[4 * k + 3]; Q[k] = a + b; }
  if (lanes == 8) return Q[0] + Q[1];
  double R[4];
  for (int j = 0; j < 4; j++) { const double a = Q[4 * j + 3] + Q[4 * j + 2], b = Q[4 * j + 1] + Q[4 * j]; R[j] = a + b; }
  const double a = R[3] + R[2], b = R[1] + R[0];
  return a + b;
}

void lu_walk_host(const LuPlan &p, const double *in, double *out)
{
  const int n = p.n;
  std::vector<double> w((size_t)n, 0.0);
  const int nlev = p.levels[0] + p.levels[1];
  for (int l = 0; l < nlev; l++)
    for (int pos = p.lev[l]; pos < p.lev[l + 1]; pos++) {
      const int r = p.rows[pos], e0 = p.rp[pos], e1 = p.rp[pos + 1];
      const bool second = pos >= n, scaled = p.first_scaled ? !second : second;
      const double acc = lu_row_sum(p.val.data() + e0, p.col.data() + e0, e1 - e0, p.lanes[l], w.data());
      double t = (second ? w[r] : in[p.perm[r]]) - acc;
      if (scaled) t = t * p.dinv[pos - (second ? n : 0)];
      w[r] = t;
      if (second) out[p.perm[r]] = t;
    }
}
} // namespace

void lu_ordering(int n, const int *rp, const int *col, int ordering, std::vector<int> &perm)
{
  if (ordering == LU_ORDERING_NATURAL) { perm.resize((size_t)n); for (int i = 0; i < n; i++) perm[i] = i; return; }
  // the graph of the pattern of P + P^T without the diagonal: both directions of every entry, sorted, repeated edges removed
  std::vector<int> xadj((size_t)n + 1, 0), adj, fill;
  for (int r = 0; r < n; r++) for (int p = rp[r]; p < rp[r + 1]; p++) { const int c = col[p]; if (c >= 0 && c < n && c != r) { xadj[r + 1]++; xadj[c + 1]++; } }
  for (int r = 0; r < n; r++) xadj[r + 1] += xadj[r];
  adj.resize((size_t)xadj[n]); fill.assign(xadj.begin(), xadj.end() - 1);
  for (int r = 0; r < n; r++) for (int p = rp[r]; p < rp[r + 1]; p++) { const int c = col[p]; if (c >= 0 && c < n && c != r) { adj[fill[r]++] = c; adj[fill[c]++] = r; } }
  std::vector<int> xa((size_t)n + 1, 0), ad; ad.reserve(adj.size());
  for (int r = 0; r < n; r++) {
    std::sort(adj.begin() + xadj[r], adj.begin() + xadj[r + 1]);
    for (int p = xadj[r]; p < xadj[r + 1]; p++) if (p == xadj[r] || adj[p] != adj[p - 1]) ad.push_back(adj[p]);
    xa[r + 1] = (int)ad.size();
  }
  nested_dissection(n, xa, ad, perm);
}

void csr_lu_plan(int n, const int *rp, const int *col, const double *val, int ordering, int wide, bool keep_factors, LuPlan &out, LuPlan *tr)
{
  out = LuPlan(); out.n = n;
  if (tr) { *tr = LuPlan(); tr->n = n; }
  std::vector<int> srp, scol; std::vector<double> sval;
  lu_sorted_rows(n, rp, col, val, srp, scol, sval);
  lu_ordering(n, srp.data(), scol.data(), ordering, out.perm);
  std::vector<int> inv((size_t)n, 0);
  for (int i = 0; i < n; i++) inv[out.perm[i]] = i;
  // the factors of Q P Q^T row by row: the row's entries scattered into w, the columns left of the diagonal taken ascending from a heap that fill joins
  Tri L, U;                                                     // U rows start with the pivot here
  L.rp.assign((size_t)n + 1, 0); U.rp.assign((size_t)n + 1, 0);
  std::vector<double> w((size_t)n, 0.0), diag((size_t)n, 0.0);
  std::vector<int> mark((size_t)n, -1), heap, upper;
  const size_t cap = 2147483647u;
  for (int i = 0; i < n; i++) {
    const int orig = out.perm[i];
    heap.clear(); upper.clear();
    for (int p = srp[orig]; p < srp[orig + 1]; p++) {
      const int c = inv[scol[p]];
      w[c] = sval[p]; mark[c] = i;
      if (c < i) heap.push_back(c); else upper.push_back(c);
    }
    std::make_heap(heap.begin(), heap.end(), std::greater<int>());
    while (!heap.empty()) {
      std::pop_heap(heap.begin(), heap.end(), std::greater<int>());
      const int k = heap.back(); heap.pop_back();
      const double l = w[k] / U.val[U.rp[k]];
      L.col.push_back(k); L.val.push_back(l);
      for (int q = U.rp[k] + 1; q < U.rp[k + 1]; q++) {
        const int j = U.col[q];
        const double m = l * U.val[q];
        if (mark[j] != i) {
          mark[j] = i; w[j] = 0.0;
          if (j < i) { heap.push_back(j); std::push_heap(heap.begin(), heap.end(), std::greater<int>()); } else upper.push_back(j);
        }
        w[j] = w[j] - m;
      }
    }
    std::sort(upper.begin(), upper.end());
    for (int j : upper) { U.col.push_back(j); U.val.push_back(w[j]); }
    L.rp[i + 1] = (int)L.col.size(); U.rp[i + 1] = (int)U.col.size();
    if (L.col.size() + U.col.size() > cap) { out.status = LU_TOO_LARGE; out.bad_row = orig; return; }
    out.longest_row = std::max(out.longest_row, (L.rp[i + 1] - L.rp[i]) + (U.rp[i + 1] - U.rp[i]));
    diag[i] = w[i];
    if (diag[i] == 0.0) { out.status = LU_ZERO_PIVOT; out.bad_row = orig; return; }
    if (diag[i] < 0.0) out.neg++; else out.pos++;
  }
  out.nnzL = (long long)L.col.size(); out.nnzU = (long long)U.col.size();
  if (keep_factors) { out.lrp = L.rp; out.lcol = L.col; out.lval = L.val; out.urp = U.rp; out.ucol = U.col; out.uval = U.val; }
  // the strict part of U
  Tri Us; Us.rp.assign((size_t)n + 1, 0); Us.col.reserve(U.col.size()); Us.val.reserve(U.col.size());
  for (int i = 0; i < n; i++) {
    Us.col.insert(Us.col.end(), U.col.begin() + U.rp[i] + 1, U.col.begin() + U.rp[i + 1]);
    Us.val.insert(Us.val.end(), U.val.begin() + U.rp[i] + 1, U.val.begin() + U.rp[i + 1]);
    Us.rp[i + 1] = (int)Us.col.size();
  }
  U = Tri();
  lu_layout(n, wide, 0, L, Us, diag, out);
  if (tr) {
    // the transposed triangles of the same factors (the counting sort of csr_transpose: a row lists a column of the factor by ascending original row):
    // U^T, lower with the pivots, is solved first, L^T, unit upper, second
    Tri Ut, Lt;
    csr_transpose(n, n, Us.rp.data(), Us.col.data(), Us.val.data(), Ut.rp, Ut.col, Ut.val);
    csr_transpose(n, n, L.rp.data(), L.col.data(), L.val.data(), Lt.rp, Lt.col, Lt.val);
    tr->perm = out.perm; tr->nnzL = out.nnzL; tr->nnzU = out.nnzU; tr->neg = out.neg; tr->pos = out.pos; tr->longest_row = out.longest_row;
    lu_layout(n, wide, 1, Ut, Lt, diag, *tr);
  }
}
void lu_apply_host(const LuPlan &p, const double *in, double *out) { lu_walk_host(p, in, out); }
void lu_apply_transpose_host(const LuPlan &t, const double *in, double *out) { lu_walk_host(t, in, out); }

// ---- smoothed-aggregation multigrid (KS_PC_AMG) ---------------------------------------------------------------------------------------------
namespace {
struct Csr { std::vector<int> rp, col; std::vector<double> val; };
constexpr size_t AMG_CAP = 2147483647u;

// the rows sorted by column, repeated entries summed in stored order; nothing is added (a missing diagonal is the set-up's error to report)
void amg_sorted_rows(int n, const int *rp, const int *col, const double *val, Csr &out)
{
  out.rp.assign((size_t)n + 1, 0); out.col.clear(); out.val.clear();
  std::vector<int> idx;
  for (int r = 0; r < n; r++) {
    idx.clear();
    for (int p = rp[r]; p < rp[r + 1]; p++) if (col[p] >= 0 && col[p] < n) idx.push_back(p);
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return col[x] < col[y]; });
    for (size_t i = 0; i < idx.size(); i++) {
      if (i > 0 && col[idx[i]] == col[idx[i - 1]]) { out.val.back() = out.val.back() + val[idx[i]]; continue; }
      out.col.push_back(col[idx[i]]); out.val.push_back(val[idx[i]]);
    }
    out.rp[r + 1] = (int)out.col.size();
  }
}

// C = A B row by row, A with na rows, B with nb columns: the entries of A's row ascending, for each the row of B ascending, one fma per pair; false: too many entries
bool amg_product(int na, int nb, const std::vector<int> &arp, const std::vector<int> &acol, const std::vector<double> &aval,
                 const std::vector<int> &brp, const std::vector<int> &bcol, const std::vector<double> &bval, Csr &C)
{
  C.rp.assign((size_t)na + 1, 0); C.col.clear(); C.val.clear();
  std::vector<int> mark((size_t)nb, -1), cols;
  std::vector<double> acc((size_t)nb, 0.0);
  for (int i = 0; i < na; i++) {
    cols.clear();
    for (int p = arp[i]; p < arp[i + 1]; p++) {
      const int k = acol[p]; const double a = aval[p];
      for (int q = brp[k]; q < brp[k + 1]; q++) {
        const int j = bcol[q];
        if (mark[j] != i) { mark[j] = i; acc[j] = 0.0; cols.push_back(j); }
        acc[j] = __builtin_fma(a, bval[q], acc[j]);
      }
    }
    std::sort(cols.begin(), cols.end());
    if (C.col.size() + cols.size() > AMG_CAP) return false;
    for (int j : cols) { C.col.push_back(j); C.val.push_back(acc[j]); }
    C.rp[i + 1] = (int)C.col.size();
  }
  return true;
}

// the symmetrised strength graph: xadj / adj / w, a row's neighbours ascending, each once with the larger of the two weights
void amg_strength(const AmgLevel &L, const std::vector<double> &d, double theta, std::vector<int> &xadj, std::vector<int> &adj, std::vector<double> &w)
{
  const int n = L.n;
  auto strong = [&](int i, int p) { const int j = L.col[p]; const double a = std::fabs(L.val[p]); return j != i && L.val[p] != 0.0 && a >= theta * std::sqrt(std::fabs(d[i] * d[j])); };
  std::vector<size_t> start((size_t)n + 1, 0);
  for (int i = 0; i < n; i++) for (int p = L.rp[i]; p < L.rp[i + 1]; p++) if (strong(i, p)) { start[i + 1]++; start[L.col[p] + 1]++; }
  for (int i = 0; i < n; i++) start[i + 1] += start[i];
  std::vector<std::pair<int, double>> e(start[n]);
  std::vector<size_t> fill(start.begin(), start.end() - 1);
  for (int i = 0; i < n; i++) for (int p = L.rp[i]; p < L.rp[i + 1]; p++) if (strong(i, p)) {
    const int j = L.col[p]; const double a = std::fabs(L.val[p]);
    e[fill[i]++] = {j, a}; e[fill[j]++] = {i, a};
  }
  xadj.assign((size_t)n + 1, 0); adj.clear(); w.clear();
  for (int i = 0; i < n; i++) {
    std::sort(e.begin() + start[i], e.begin() + start[i + 1]);        // by neighbour, then by weight: the last of a run is the larger
    for (size_t p = start[i]; p < start[i + 1]; p++) {
      if (p + 1 < start[i + 1] && e[p + 1].first == e[p].first) continue;
      adj.push_back(e[p].first); w.push_back(e[p].second);
    }
    xadj[i + 1] = (int)adj.size();
  }
}

int amg_aggregate(int n, const std::vector<int> &xadj, const std::vector<int> &adj, const std::vector<double> &w, std::vector<int> &agg)
{
  agg.assign((size_t)n, -1);
  int nagg = 0;
  for (int i = 0; i < n; i++) {                                       // pass 1
    if (agg[i] >= 0 || xadj[i] == xadj[i + 1]) continue;
    bool free_ = true;
    for (int p = xadj[i]; p < xadj[i + 1] && free_; p++) free_ = agg[adj[p]] < 0;
    if (!free_) continue;
    agg[i] = nagg;
    for (int p = xadj[i]; p < xadj[i + 1]; p++) agg[adj[p]] = nagg;
    nagg++;
  }
  const std::vector<int> after1(agg);
  for (int i = 0; i < n; i++) {                                       // pass 2: against the state pass 1 left
    if (after1[i] >= 0) continue;
    int best = -1;
    for (int p = xadj[i]; p < xadj[i + 1]; p++) if (after1[adj[p]] >= 0 && (best < 0 || w[p] > w[best])) best = p;
    if (best >= 0) agg[i] = after1[adj[best]];
  }
  for (int i = 0; i < n; i++) {                                       // pass 3
    if (agg[i] >= 0 || xadj[i] == xadj[i + 1]) continue;
    agg[i] = nagg;
    for (int p = xadj[i]; p < xadj[i + 1]; p++) if (agg[adj[p]] < 0) agg[adj[p]] = nagg;
    nagg++;
  }
  return nagg;
}
} // namespace

void amg_plan(int n, const int *rp, const int *col, const double *val, const AmgOptions &opt, AmgPlan &out)
{
  out = AmgPlan();
  const int max_levels = std::max(1, std::min(opt.max_levels, AMG_MAX_LEVELS));
  out.levels.reserve((size_t)max_levels);
  out.levels.emplace_back();
  { Csr A0; amg_sorted_rows(n, rp, col, val, A0); AmgLevel &L = out.levels.back(); L.n = n; L.rp.swap(A0.rp); L.col.swap(A0.col); L.val.swap(A0.val); }
  std::vector<int> xadj, adj, size, mark, cols;
  std::vector<double> w, d, t, acc;
  while (out.levels.back().n > opt.coarse_limit && (int)out.levels.size() < max_levels) {
    AmgLevel &L = out.levels.back();
    const int nl = L.n, lev = (int)out.levels.size() - 1;
    d.assign((size_t)nl, 0.0);
    double rho = 0.0;
    for (int i = 0; i < nl; i++) {
      double sum = 0.0; bool stored = false;
      for (int p = L.rp[i]; p < L.rp[i + 1]; p++) { sum = sum + std::fabs(L.val[p]); if (L.col[p] == i) { d[i] = L.val[p]; stored = true; } }
      if (!stored || d[i] == 0.0) { out.status = AMG_NO_DIAGONAL; out.bad_level = lev; out.bad_row = i; return; }
      rho = std::max(rho, sum / std::fabs(d[i]));
    }
    amg_strength(L, d, opt.theta, xadj, adj, w);
    std::vector<int> agg;
    const int nagg = amg_aggregate(nl, xadj, adj, w, agg);
    if (nagg == 0 || (double)nagg > opt.stall * (double)nl) break;
    size.assign((size_t)nagg, 0);
    for (int i = 0; i < nl; i++) if (agg[i] >= 0) size[agg[i]]++;
    t.assign((size_t)nl, 0.0);
    for (int i = 0; i < nl; i++) if (agg[i] >= 0) t[i] = 1.0 / std::sqrt((double)size[agg[i]]);
    L.rho = rho; L.nagg = nagg;
    L.dinv.resize((size_t)nl);
    for (int i = 0; i < nl; i++) L.dinv[i] = 1.0 / d[i];
    L.prp.assign((size_t)nl + 1, 0);
    if (!opt.smooth) {
      for (int i = 0; i < nl; i++) { if (agg[i] >= 0) { L.pcol.push_back(agg[i]); L.pval.push_back(t[i]); } L.prp[i + 1] = (int)L.pcol.size(); }
    } else {
      const double omega = 4.0 / (3.0 * rho);
      mark.assign((size_t)nagg, -1); acc.assign((size_t)nagg, 0.0);
      for (int i = 0; i < nl; i++) {
        cols.clear();
        if (agg[i] >= 0) { mark[agg[i]] = i; acc[agg[i]] = 0.0; cols.push_back(agg[i]); }
        for (int p = L.rp[i]; p < L.rp[i + 1]; p++) {
          const int c = agg[L.col[p]];
          if (c < 0) continue;
          if (mark[c] != i) { mark[c] = i; acc[c] = 0.0; cols.push_back(c); }
          acc[c] = __builtin_fma(L.val[p], t[L.col[p]], acc[c]);
        }
        std::sort(cols.begin(), cols.end());
        if (L.pcol.size() + cols.size() > AMG_CAP) { out.status = AMG_TOO_LARGE; out.bad_level = lev; out.bad_row = i; return; }
        const double s = omega / d[i];
        for (int c : cols) { const double sm = s * acc[c]; L.pcol.push_back(c); L.pval.push_back((c == agg[i] ? t[i] : 0.0) - sm); }
        L.prp[i + 1] = (int)L.pcol.size();
      }
    }
    L.agg.swap(agg);
    csr_transpose(nl, nagg, L.prp.data(), L.pcol.data(), L.pval.data(), L.rrp, L.rcol, L.rval);
    Csr AP, Ac;
    if (!amg_product(nl, nagg, L.rp, L.col, L.val, L.prp, L.pcol, L.pval, AP) || !amg_product(nagg, nagg, L.rrp, L.rcol, L.rval, AP.rp, AP.col, AP.val, Ac)) {
      out.status = AMG_TOO_LARGE; out.bad_level = lev; return;
    }
    out.levels.emplace_back();                                      // (reserved above: L stays valid)
    AmgLevel &Lc = out.levels.back();
    Lc.n = nagg; Lc.rp.swap(Ac.rp); Lc.col.swap(Ac.col); Lc.val.swap(Ac.val);
  }
}

// ---- block CSR (BAIJ) input -------------------------------------------------------------------------------------------------------------------------
void bsr_expand(int bs, int nb, int nb_global, const int *browptr, const int *bcol, const double *bval, BsrExpansion &out)
{
  out = BsrExpansion();
  for (int I = 0; I < nb; I++) if (browptr[I + 1] < browptr[I]) { out.status = BSR_ROWPTR; out.bad_row = I; return; }
  const long long nnzb = browptr[nb], b2 = (long long)bs * bs;
  if (nnzb * b2 > 2147483647LL) { out.status = BSR_TOO_LARGE; return; }
  for (int I = 0; I < nb; I++)
    for (int k = browptr[I]; k < browptr[I + 1]; k++)
      if (bcol[k] < 0 || bcol[k] >= nb_global) { out.status = BSR_COLUMN; out.bad_row = I; out.bad_col = bcol[k]; return; }
  out.rp.assign((size_t)nb * bs + 1, 0); out.col.resize((size_t)(nnzb * b2)); out.val.resize((size_t)(nnzb * b2));
  for (int I = 0; I < nb; I++) {
    const int k0 = browptr[I], len = browptr[I + 1] - k0;
    for (int i = 0; i < bs; i++) {
      size_t e = (size_t)k0 * b2 + (size_t)i * len * bs;             // the rows of a block row have the same length
      out.rp[(size_t)I * bs + i] = (int)e;
      for (int k = k0; k < k0 + len; k++)
        for (int c = 0; c < bs; c++, e++) { out.col[e] = bs * bcol[k] + c; out.val[e] = bval[(size_t)k * b2 + (size_t)c * bs + i]; }
    }
  }
  out.rp[(size_t)nb * bs] = (int)(nnzb * b2);
}
void bsr_diag(int bs, int nb, int bstart, const int *browptr, const int *bcol, const double *bval, BsrBlocks &out)
{
  out = BsrBlocks();
  const size_t b2 = (size_t)bs * bs;
  out.browptr.assign((size_t)nb + 1, 0);
  for (int I = 0; I < nb; I++) {
    for (int k = browptr[I]; k < browptr[I + 1]; k++)
      if (bcol[k] >= bstart && bcol[k] < bstart + nb) { out.bcol.push_back(bcol[k] - bstart); out.bval.insert(out.bval.end(), bval + (size_t)k * b2, bval + (size_t)(k + 1) * b2); }
    out.browptr[(size_t)I + 1] = (int)out.bcol.size();
  }
}
void bsr_plan(int bs, int nb, const int *browptr, const int *bcol, const double *bval, int group_rows, int chunk_blocks, int pad, BsrPlan &out)
{
  out = BsrPlan();
  const long long nnzb = browptr[nb]; const size_t b2 = (size_t)bs * bs;
  out.bs = bs; out.nb = nb; out.group_rows = group_rows; out.chunk_blocks = chunk_blocks; out.blocks = nnzb;
  out.groups = ((long long)nb + group_rows - 1) / group_rows;
  out.browptr.assign(browptr, browptr + nb + 1);
  out.bcol.assign((size_t)nnzb + pad, 0); std::copy(bcol, bcol + nnzb, out.bcol.begin());
  out.val.assign((size_t)nnzb * b2 + pad, 0.0);
  for (long long k = 0; k < nnzb; k++)
    for (int i = 0; i < bs; i++)
      for (int c = 0; c < bs; c++) out.val[(size_t)k * b2 + (size_t)i * bs + c] = bval[(size_t)k * b2 + (size_t)c * bs + i];
  out.gptr.resize((size_t)out.groups + 1);
  for (long long g = 0; g <= out.groups; g++) out.gptr[(size_t)g] = browptr[std::min<long long>(g * group_rows, nb)];
}
void bsr_apply_host(const BsrPlan &p, const double *x, double *y)
{
  const int bs = p.bs, wr = p.group_rows / 4; const size_t b2 = (size_t)bs * bs;
  for (long long g = 0; g < p.groups; g++)
    for (int w = 0; w < 4; w++) {
      const long long I0 = g * p.group_rows + (long long)w * wr, I1 = std::min<long long>(I0 + wr, p.nb);
      if (I0 >= p.nb) continue;
      std::vector<double> acc((size_t)(I1 - I0) * bs, 0.0);
      const int B0 = p.browptr[(size_t)I0], B1 = p.browptr[(size_t)I1];
      for (int b0 = B0; b0 < B1; b0 += p.chunk_blocks)                       // a chunk: every lane sums its row's part of it
        for (long long I = I0; I < I1; I++)
          for (int i = 0; i < bs; i++) {
            double &a = acc[(size_t)(I - I0) * bs + i];
            const int lo = std::max(p.browptr[(size_t)I], b0), hi = std::min(p.browptr[(size_t)I + 1], b0 + p.chunk_blocks);
            for (int k = lo; k < hi; k++)
              for (int c = 0; c < bs; c++) a = std::fma(p.val[(size_t)k * b2 + (size_t)i * bs + c], x[(size_t)bs * p.bcol[(size_t)k] + c], a);
          }
      for (long long I = I0; I < I1; I++) for (int i = 0; i < bs; i++) y[(size_t)I * bs + i] = acc[(size_t)(I - I0) * bs + i];
    }
}
} // namespace ksc

#ifdef KSD_TEST_HOOKS
extern "C" {
// test hook: B = A^T (square blocks of order n); rpt has n + 1 entries, colt / valt nnz
void ksc_csr_transpose(int n, const int *rp, const int *col, const double *val, int *rpt, int *colt, double *valt)
{
  std::vector<int> r, c; std::vector<double> v;
  ksc::csr_transpose(n, n, rp, col, val, r, c, v);
  std::copy(r.begin(), r.end(), rpt); std::copy(c.begin(), c.end(), colt); std::copy(v.begin(), v.end(), valt);
}
// test hook: one rank's plan of the transposed product of a row-sharded matrix. The arrays have room for: d_rp n + 1, d_col / d_val and o_row / o_val
// nnz each, o_rp nghost + 1, acc_rows nsend, acc_ptr nsend + 1, acc_pos nsend. info: entries of the two transposed blocks, listed rows.
void ksc_sharded_transpose_plan(int n, int row_start, const int *rp, const int *col, const double *val, int nghost, const int *ghosts, int nsend, const int *send_idx,
                                int *d_rp, int *d_col, double *d_val, int *o_rp, int *o_row, double *o_val, int *acc_rows, int *acc_ptr, int *acc_pos, long long *info)
{
  ksc::ShardedTransposePlan p;
  ksc::sharded_transpose_plan(n, row_start, rp, col, val, nghost, ghosts, nsend, send_idx, p);
  std::copy(p.d_rp.begin(), p.d_rp.end(), d_rp); std::copy(p.d_col.begin(), p.d_col.end(), d_col); std::copy(p.d_val.begin(), p.d_val.end(), d_val);
  std::copy(p.o_rp.begin(), p.o_rp.end(), o_rp); std::copy(p.o_row.begin(), p.o_row.end(), o_row); std::copy(p.o_val.begin(), p.o_val.end(), o_val);
  std::copy(p.acc_rows.begin(), p.acc_rows.end(), acc_rows); std::copy(p.acc_ptr.begin(), p.acc_ptr.end(), acc_ptr); std::copy(p.acc_pos.begin(), p.acc_pos.end(), acc_pos);
  info[0] = (long long)p.d_col.size(); info[1] = (long long)p.o_row.size(); info[2] = (long long)p.acc_rows.size();
}
// test hooks: the host walk of that plan for one rank (the plan is built again from the same inputs): first the two local products - rsend (nghost) is
// what the rank sends back to the owners of its ghosts, y (n) the transposed diagonal block's part - then, with the receive buffer the reverse
// exchange filled (nsend), the accumulation into y
void ksc_sharded_transpose_local(int n, int row_start, const int *rp, const int *col, const double *val, int nghost, const int *ghosts, const double *x, double *rsend, double *y)
{
  ksc::ShardedTransposePlan p;
  ksc::sharded_transpose_plan(n, row_start, rp, col, val, nghost, ghosts, 0, nullptr, p);
  ksc::sharded_transpose_local_host(p, n, nghost, x, rsend, y);
}
void ksc_sharded_transpose_add(int n, int nsend, const int *send_idx, const double *rrecv, double *y)
{
  ksc::ShardedTransposePlan p;
  std::vector<int> rp((size_t)n + 1, 0);                                                     // an empty matrix: only the accumulate list is needed here
  ksc::sharded_transpose_plan(n, 0, rp.data(), nullptr, nullptr, 0, nullptr, nsend, send_idx, p);
  ksc::sharded_transpose_add_host(p, rrecv, y);
}
// test hook: P = A + alpha B (B arrays NULL: the identity); returns nnz(P), fills rp always and col/val when they are given (capacity cap entries)
long long ksc_csr_axpy(int n, int row_start, const int *rpa, const int *ca, const double *va, double alpha, const int *rpb, const int *cb, const double *vb,
                       int *rp, int *col, double *val, long long cap)
{
  std::vector<int> r, c; std::vector<double> v;
  if (!ksc::csr_axpy(n, row_start, rpa, ca, va, alpha, rpb, cb, vb, r, c, v)) return -1;
  std::copy(r.begin(), r.end(), rp);
  if (col && val && (long long)c.size() <= cap) { std::copy(c.begin(), c.end(), col); std::copy(v.begin(), v.end(), val); }
  return (long long)c.size();
}
// test hook: the diagonal / ghost split of a row block. Room for: rp_d, rp_o n_local + 1; col_d, val_d, col_o, val_o, garray rowptr[n_local] each (none of
// them is written on a rejection). info: status, bad_row, bad_col, entries of the diagonal block, of the ghost block, ghosts. Returns the status.
int ksc_split_block(int n_local, int row_start, int n_global, const int *rowptr, const int *col, const double *val,
                    int *rp_d, int *col_d, double *val_d, int *rp_o, int *col_o, double *val_o, int *garray, long long *info)
{
  ksc::BlockSplit s;
  ksc::csr_split_block(n_local, row_start, n_global, rowptr, col, val, s);
  info[0] = s.status; info[1] = s.bad_row; info[2] = s.bad_col; info[3] = info[4] = info[5] = 0;
  if (s.status) return s.status;
  info[3] = (long long)s.col_d.size(); info[4] = (long long)s.col_o.size(); info[5] = (long long)s.garray.size();
  std::copy(s.rp_d.begin(), s.rp_d.end(), rp_d); std::copy(s.col_d.begin(), s.col_d.end(), col_d); std::copy(s.val_d.begin(), s.val_d.end(), val_d);
  std::copy(s.rp_o.begin(), s.rp_o.end(), rp_o); std::copy(s.col_o.begin(), s.col_o.end(), col_o); std::copy(s.val_o.begin(), s.val_o.end(), val_o);
  std::copy(s.garray.begin(), s.garray.end(), garray);
  return 0;
}
// test hooks: the three host steps of the halo plan. starts: size + 1; recv_cnt: size; all_cnt: size x size, row p = rank p's recv_cnt; the five per-peer
// lists have room for size entries. ksc_halo_peers returns the number of peers; the other two a HALO_* status.
int ksc_halo_recv_counts(int nghost, const int *garray, int size, const int *starts, int rank, int *recv_cnt)
{
  std::vector<int> cnt;
  const int st = ksc::halo_recv_counts(std::vector<int>(garray, garray + nghost), std::vector<int>(starts, starts + size + 1), rank, cnt);
  std::copy(cnt.begin(), cnt.end(), recv_cnt);
  return st;
}
int ksc_halo_peers(int rank, int size, const int *recv_cnt, const int *all_cnt, int *peers, int *rcnt, int *scnt, int *roff, int *soff, int *nsend)
{
  ksc::HaloPeers h;
  ksc::halo_peers(rank, size, recv_cnt, all_cnt, h);
  std::copy(h.peers.begin(), h.peers.end(), peers); std::copy(h.recv_cnt.begin(), h.recv_cnt.end(), rcnt); std::copy(h.send_cnt.begin(), h.send_cnt.end(), scnt);
  std::copy(h.recv_off.begin(), h.recv_off.end(), roff); std::copy(h.send_off.begin(), h.send_off.end(), soff);
  *nsend = h.nsend;
  return (int)h.peers.size();
}
int ksc_halo_localize_send_idx(int row_start, int n, int nsend, int *sidx) { return ksc::halo_localize_send_idx(row_start, n, nsend, sidx); }
// test hook: the geometry of the binned layout alone (no arrays needed). geo: ns, cs, wb, wr. Returns the status.
int ksc_binned_geometry(int n, long long nnz, int ncu, int cs_max, int seg_pad, int *geo)
{
  ksc::BinnedGeometry g;
  ksc::binned_geometry(n, nnz, ncu, cs_max, seg_pad, g);
  geo[0] = g.ns; geo[1] = g.cs; geo[2] = g.wb; geo[3] = g.wr;
  return g.status;
}
// test hook: geometry and plan of the binned layout for ncu compute units, and its host walk. info: geometry status, ns, cs, wb, wr, plan status, nwin,
// entries. Two calls: with col16 NULL only info is filled; then col16, row16, val2 have room for `entries`, off1 ns (wb + 1), off2t, off2 ns wb,
// wseg ns nwin, sbase ns + 1, log2 wb (ns + 1). x, y (n each, may be NULL): y = the host walk of the plan. Returns 0, or the status that ended it.
int ksc_binned_plan(int n, const int *rp, const int *col, const double *val, int ncu, int cs_max, int seg_pad, long long *info,
                    unsigned short *col16, unsigned short *row16, double *val2, int *off1, int *off2t, int *wseg, long long *sbase, int *off2, int *log2,
                    const double *x, double *y)
{
  ksc::BinnedGeometry g; ksc::BinnedPlan p;
  ksc::binned_geometry(n, rp[n], ncu, cs_max, seg_pad, g);
  info[0] = g.status; info[1] = g.ns; info[2] = g.cs; info[3] = g.wb; info[4] = g.wr; info[5] = info[6] = info[7] = 0;
  if (g.status) return g.status;
  ksc::binned_plan(n, rp, col, val, g, seg_pad, p);
  info[5] = p.status; info[6] = p.nwin; info[7] = p.entries;
  if (p.status) return p.status;
  if (col16) {
    std::copy(p.col16.begin(), p.col16.end(), col16); std::copy(p.row16.begin(), p.row16.end(), row16); std::copy(p.val2.begin(), p.val2.end(), val2);
    std::copy(p.off1.begin(), p.off1.end(), off1); std::copy(p.off2t.begin(), p.off2t.end(), off2t); std::copy(p.wseg.begin(), p.wseg.end(), wseg);
    std::copy(p.sbase.begin(), p.sbase.end(), sbase); std::copy(p.off2.begin(), p.off2.end(), off2); std::copy(p.log2.begin(), p.log2.end(), log2);
  }
  if (x && y) ksc::binned_apply_host(p, g, n, x, y);
  return 0;
}
// test hook: the plan of the windowed layout. nseg, dbase: one per block; codes: one per entry; totals: blocks, direct blocks, window entries,
// direct entries, segments listed, length of the direct column array without its padding. seg (the concatenated lists) may be NULL or has room
// for seg_cap segments. Returns the number of segments listed.
long long ksc_window_plan(int n, const int *rp, const int *col, int block_rows, int max_segments, int *nseg, int *dbase, unsigned short *codes,
                          int *seg, long long seg_cap, long long *totals)
{
  ksc::WindowPlan p;
  ksc::csr_window_plan(n, rp, col, block_rows, max_segments, 8, p);
  std::copy(p.nseg.begin(), p.nseg.end(), nseg); std::copy(p.dbase.begin(), p.dbase.end(), dbase);
  std::copy(p.codes.begin(), p.codes.end() - 8, codes);
  if (seg && (long long)p.seg.size() <= seg_cap) std::copy(p.seg.begin(), p.seg.end(), seg);
  totals[0] = p.blocks; totals[1] = p.direct_blocks; totals[2] = p.window_entries; totals[3] = p.direct_entries; totals[4] = p.total_segments;
  totals[5] = (long long)p.dcol.size() - 8;
  return p.total_segments;
}
// test hook: the CSR expansion of block CSR arrays. info: status, bad block row, bad block column, entries. rp (nb bs + 1), col, val (browptr[nb] bs bs
// each) may be NULL (a first call for the status alone). Returns the status.
int ksc_bsr_expand(int bs, int nb, int nb_global, const int *browptr, const int *bcol, const double *bval, int *rp, int *col, double *val, long long *info)
{
  ksc::BsrExpansion e;
  ksc::bsr_expand(bs, nb, nb_global, browptr, bcol, bval, e);
  info[0] = e.status; info[1] = e.bad_row; info[2] = e.bad_col; info[3] = (long long)e.col.size();
  if (e.status) return e.status;
  if (rp) { std::copy(e.rp.begin(), e.rp.end(), rp); std::copy(e.col.begin(), e.col.end(), col); std::copy(e.val.begin(), e.val.end(), val); }
  return 0;
}
// test hook: the diagonal block of a rank's block CSR arrays, its device image and the host walk of that. info: blocks of the diagonal block, groups.
// val (room for browptr[nb] bs bs) receives the row-major image without its padding, x / y (may be NULL): nb bs each.
void ksc_bsr_plan(int bs, int nb, int bstart, const int *browptr, const int *bcol, const double *bval, int group_rows, int chunk_blocks, double *val, const double *x, double *y, long long *info)
{
  ksc::BsrBlocks d; ksc::BsrPlan p;
  ksc::bsr_diag(bs, nb, bstart, browptr, bcol, bval, d);
  ksc::bsr_plan(bs, nb, d.browptr.data(), d.bcol.data(), d.bval.data(), group_rows, chunk_blocks, 8, p);
  info[0] = p.blocks; info[1] = p.groups;
  if (val) std::copy(p.val.begin(), p.val.end() - 8, val);
  if (x && y) ksc::bsr_apply_host(p, x, y);
}
// test hook: ILU(0) of the diagonal blocks (block size bs) and the solve the kernel runs, on the host. frp (n + 1), fcol, fval (cap entries, may be
// NULL): the factors on the blocks' sorted patterns, block-local columns. in / out (may be NULL): out = (LU)^-1 in through the level layout.
// info: status (0, 1 = a row without a diagonal entry, 2 = zero pivot), block, local row, longest row, levels, ELL entries. Returns the number of
// entries of the factors, -1 on a status other than 0.
long long ksc_ilu0_blocks(int n, int row_start, int bs, const int *rp, const int *col, const double *val, int *frp, int *fcol, double *fval, long long cap,
                          const double *in, double *out, long long *info)
{
  ksc::IluPlan p;
  ksc::csr_ilu0_blocks(n, row_start, bs, rp, col, val, true, p);
  info[0] = p.status; info[1] = p.bad_block; info[2] = p.bad_row; info[3] = p.longest_row; info[4] = (long long)p.lev.size() / 2; info[5] = (long long)p.val.size();
  if (p.status) return -1;
  if (frp) std::copy(p.frp.begin(), p.frp.end(), frp);
  if (fcol && fval && (long long)p.fcol.size() <= cap) { std::copy(p.fcol.begin(), p.fcol.end(), fcol); std::copy(p.fval.begin(), p.fval.end(), fval); }
  if (in && out) ksc::ilu0_apply_host(p, n, bs, in, out);
  return (long long)p.fcol.size();
}
// test hook: the transposed level layout of the same factors and the solve k_bjacobi_ilu_apply_t runs, on the host: out_t = (LU)^-T in, out_f = (LU)^-1 in
// (either may be NULL). per_block (six per block): L and U levels of the forward plan, first-phase (U^T) and second-phase (L^T) levels of the
// transposed one, the largest code of the transposed plan, the block's length. info: status, block, local row, longest column, levels and ELL
// entries of the transposed plan, and info[6] = 1 when the forward plan built together with the transposed one equals, array by array, the forward
// plan built alone. Returns the ELL entries of the transposed plan, -1 on a status other than 0.
long long ksc_ilu0_blocks_transpose(int n, int row_start, int bs, const int *rp, const int *col, const double *val, const double *in, double *out_t, double *out_f,
                                    int *per_block, long long *info)
{
  ksc::IluPlan alone, p, t;
  ksc::csr_ilu0_blocks(n, row_start, bs, rp, col, val, false, alone);
  ksc::csr_ilu0_blocks(n, row_start, bs, rp, col, val, false, p, &t);
  info[0] = p.status; info[1] = p.bad_block; info[2] = p.bad_row; info[3] = t.longest_row; info[4] = (long long)t.lev.size() / 2; info[5] = (long long)t.val.size();
  if (p.status) return -1;
  bool same = alone.lev == p.lev && alone.val == p.val && alone.code == p.code && alone.rows == p.rows && alone.dinv == p.dinv && alone.blk.size() == p.blk.size() && alone.longest_row == p.longest_row;
  for (size_t b = 0; same && b < p.blk.size(); b++) same = alone.blk[b].ell == p.blk[b].ell && alone.blk[b].lev == p.blk[b].lev && alone.blk[b].nL == p.blk[b].nL && alone.blk[b].nU == p.blk[b].nU;
  info[6] = same ? 1 : 0;
  for (size_t b = 0; b < t.blk.size(); b++) {
    const size_t e0 = (size_t)t.blk[b].ell, e1 = b + 1 < t.blk.size() ? (size_t)t.blk[b + 1].ell : t.code.size();
    int top = 0;
    for (size_t e = e0; e < e1; e++) top = std::max(top, (int)t.code[e]);
    for (int i = 0; i < 2 * std::min(bs, n - (int)b * bs); i++) top = std::max(top, (int)t.rows[(size_t)2 * b * bs + i]);
    int *o = per_block + 6 * b;
    o[0] = p.blk[b].nL; o[1] = p.blk[b].nU; o[2] = t.blk[b].nL; o[3] = t.blk[b].nU; o[4] = top; o[5] = std::min(bs, n - (int)b * bs);
  }
  if (in && out_t) ksc::ilu0_apply_transpose_host(t, n, bs, in, out_t);
  if (in && out_f) ksc::ilu0_apply_host(p, n, bs, in, out_f);
  return (long long)t.val.size();
}
// test hooks: the ordering alone; and the LU plan. ksc_lu_plan fills info first: status, bad row, entries of L, of U, levels and stages of the two
// triangles (forward plan: 4..7), pivots < 0 and > 0, longest row, entries of the layout, levels and stages of the transposed plan (12..15); every
// array may be NULL, else it has room for what a first call reported: perm n; lrp / urp n + 1 with lcol, lval / ucol, uval (the factors by rows, U rows
// starting with the pivot); rows 2n, prp 2n + 1, pcol / pval, lev levels + 1, lanes levels, dinv n, stages 3 per stage (the forward plan's layout);
// in -> out_f = the forward host apply, out_t = the transposed one. Returns the status.
void ksc_lu_ordering(int n, const int *rp, const int *col, int ordering, int *perm)
{
  std::vector<int> p;
  ksc::lu_ordering(n, rp, col, ordering, p);
  std::copy(p.begin(), p.end(), perm);
}
int ksc_lu_plan(int n, const int *rp, const int *col, const double *val, int ordering, int wide, long long *info, int *perm, int *lrp, int *lcol, double *lval,
                int *urp, int *ucol, double *uval, int *rows, int *prp, int *pcol, double *pval, int *lev, int *lanes, double *dinv, int *stages,
                const double *in, double *out_f, double *out_t)
{
  ksc::LuPlan p, t;
  ksc::csr_lu_plan(n, rp, col, val, ordering, wide, true, p, &t);
  for (int i = 0; i < 16; i++) info[i] = 0;
  info[0] = p.status; info[1] = p.bad_row;
  if (p.status) return p.status;
  info[2] = p.nnzL; info[3] = p.nnzU; info[4] = p.levels[0]; info[5] = p.levels[1]; info[6] = p.nstage[0]; info[7] = p.nstage[1];
  info[8] = p.neg; info[9] = p.pos; info[10] = p.longest_row; info[11] = (long long)p.col.size();
  info[12] = t.levels[0]; info[13] = t.levels[1]; info[14] = t.nstage[0]; info[15] = t.nstage[1];
  if (perm) std::copy(p.perm.begin(), p.perm.end(), perm);
  if (lrp) { std::copy(p.lrp.begin(), p.lrp.end(), lrp); std::copy(p.lcol.begin(), p.lcol.end(), lcol); std::copy(p.lval.begin(), p.lval.end(), lval); }
  if (urp) { std::copy(p.urp.begin(), p.urp.end(), urp); std::copy(p.ucol.begin(), p.ucol.end(), ucol); std::copy(p.uval.begin(), p.uval.end(), uval); }
  if (rows) {
    std::copy(p.rows.begin(), p.rows.end(), rows); std::copy(p.rp.begin(), p.rp.end(), prp); std::copy(p.col.begin(), p.col.end(), pcol); std::copy(p.val.begin(), p.val.end(), pval);
    std::copy(p.lev.begin(), p.lev.end(), lev); std::copy(p.lanes.begin(), p.lanes.end(), lanes); std::copy(p.dinv.begin(), p.dinv.end(), dinv);
    for (size_t s = 0; s < p.stages.size(); s++) { stages[3 * s] = p.stages[s].lev0; stages[3 * s + 1] = p.stages[s].nlev; stages[3 * s + 2] = p.stages[s].wide; }
  }
  if (in && out_f) ksc::lu_apply_host(p, in, out_f);
  if (in && out_t) ksc::lu_apply_transpose_host(t, in, out_t);
  return 0;
}
// test hook: the AMG hierarchy. info: status, bad row, bad level, levels, then four per level: rows, entries of the operator, entries of P, aggregates
// (room for 4 + 4 * 16); rho: one per level (16). level >= 0: that level's operator (arp rows + 1, acol / aval), and - every level but the last - its
// P (prp rows + 1, pcol / pval) and aggregate index (agg rows; the last level: -1 everywhere) into arrays sized by a first call. Returns the status.
int ksc_amg_plan(int n, const int *rp, const int *col, const double *val, double theta, int coarse_limit, int max_levels, int smooth, double stall, long long *info,
                 double *rho, int level, int *arp, int *acol, double *aval, int *prp, int *pcol, double *pval, int *agg)
{
  ksc::AmgOptions opt; opt.theta = theta; opt.coarse_limit = coarse_limit; opt.max_levels = max_levels; opt.smooth = smooth != 0; opt.stall = stall;
  ksc::AmgPlan p;
  ksc::amg_plan(n, rp, col, val, opt, p);
  for (int i = 0; i < 4 + 4 * ksc::AMG_MAX_LEVELS; i++) info[i] = 0;
  info[0] = p.status; info[1] = p.bad_row; info[2] = p.bad_level;
  if (p.status) return p.status;
  info[3] = (long long)p.levels.size();
  for (size_t l = 0; l < p.levels.size(); l++) {
    const ksc::AmgLevel &L = p.levels[l];
    info[4 + 4 * l] = L.n; info[5 + 4 * l] = (long long)L.col.size(); info[6 + 4 * l] = (long long)L.pcol.size(); info[7 + 4 * l] = L.nagg;
    rho[l] = L.rho;
  }
  if (level >= 0 && level < (int)p.levels.size()) {
    const ksc::AmgLevel &L = p.levels[level];
    std::copy(L.rp.begin(), L.rp.end(), arp); std::copy(L.col.begin(), L.col.end(), acol); std::copy(L.val.begin(), L.val.end(), aval);
    if (L.agg.empty()) { std::fill(prp, prp + L.n + 1, 0); std::fill(agg, agg + L.n, -1); }
    else { std::copy(L.prp.begin(), L.prp.end(), prp); std::copy(L.pcol.begin(), L.pcol.end(), pcol); std::copy(L.pval.begin(), L.pval.end(), pval); std::copy(L.agg.begin(), L.agg.end(), agg); }
  }
  return 0;
}
}
#endif
