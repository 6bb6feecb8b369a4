#include "ks_csr.h"
#include <algorithm>
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
} // namespace

bool csr_axpy(int n, int row_start, const int *rpa, const int *ca, const double *va, double alpha, const int *rpb, const int *cb, const double *vb,
              std::vector<int> &rp, std::vector<int> &col, std::vector<double> &val)
{
  rp.assign((size_t)n + 1, 0);
  unsigned ncpu = std::thread::hardware_concurrency();
  { cpu_set_t cs; CPU_ZERO(&cs); if (sched_getaffinity(0, sizeof(cs), &cs) == 0 && CPU_COUNT(&cs) > 0) ncpu = (unsigned)CPU_COUNT(&cs); }
  const unsigned nthr = (n < 100000) ? 1u : std::max(1u, std::min(16u, ncpu));
  const double one = 1.0;
  auto rows = [&](bool fill, int r0, int r1) {
    for (int r = r0; r < r1; r++) {
      const int id = row_start + r;
      const int *bc = rpb ? cb + rpb[r] : &id; const double *bv = rpb ? vb + rpb[r] : &one; const int lb = rpb ? rpb[r + 1] - rpb[r] : 1;
      if (!fill) rp[r + 1] = merge_row(ca + rpa[r], va + rpa[r], rpa[r + 1] - rpa[r], bc, bv, lb, alpha, nullptr, nullptr);
      else merge_row(ca + rpa[r], va + rpa[r], rpa[r + 1] - rpa[r], bc, bv, lb, alpha, col.data() + rp[r], val.data() + rp[r]);
    }
  };
  auto parallel = [&](bool fill) {
    std::vector<std::thread> th;
    const int chunk = (n + (int)nthr - 1) / (int)nthr;
    unsigned started = 1;
    for (unsigned t = 1; t < nthr; t++) {
      try { th.emplace_back([&, t] { rows(fill, std::min(n, (int)t * chunk), std::min(n, (int)(t + 1) * chunk)); }); started = t + 1; }
      catch (const std::system_error &) { break; }
    }
    rows(fill, 0, std::min(n, chunk));
    for (unsigned t = started; t < nthr; t++) rows(fill, std::min(n, (int)t * chunk), std::min(n, (int)(t + 1) * chunk));     // chunks whose thread did not start
    for (auto &x : th) x.join();
  };
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
}
#endif
