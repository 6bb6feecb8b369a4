// Smoothed-aggregation algebraic multigrid (KS_PC_AMG): PCGAMG's smoothed aggregation on the ST's KSP, written from the algorithm's description. The
// hierarchy - aggregates, prolongators P, restrictions R = P^T, Galerkin operators R A P - is made on the host (ksc::amg_plan, ks_csr.cpp: described in
// ks_csr.h); this file uploads it and applies one V(nu, nu) cycle per application, zero initial guess on every level:
//   pre-smooth from zero, r_c = R (b - A x), the cycle on the next level, x += P e_c, post-smooth; the last level is the sparse LU of ks_pc_lu.hip.
// A level's operator is an assembled matrix of its own (ks_mat_assemble_local): the products of the cycle run on whatever layout the chooser gives it
// and, for a block of right-hand sides, on the eight-column product. The smoother is nu steps of Chebyshev on D^-1 A over [0.1 rho, rho], rho the
// Gershgorin bound of the plan: with theta = (a + b) / 2, delta = (b - a) / 2, sigma = theta / delta, rho_0 = 1 / sigma
//   step 0:  d = D^-1 r / theta,  x += d          step k:  rho_k = 1 / (2 sigma - rho_k-1),  d = rho_k rho_k-1 d + (2 rho_k / delta) D^-1 r,  x += d
// with r = b - A x (step 0 from zero: r = b, no product). Equal pre- and post-smoothing makes the cycle symmetric for a symmetric matrix (LOBPCG).
//
// Three kernels: the Chebyshev update (one streaming pass over the product, b, 1/d, d and x), the restriction (a CSR product over R whose gather forms
// b - A x: the fine residual is never stored) and the prolongation (a CSR product over P that adds into x). A row of R or P is summed like a row of
// the LU levels: 1, 8 or 64 lanes by the mean row length, lane l takes the entries l, l + lanes, ... ascending by fma, the partial sums are combined in
// the fixed order of ksk::group_sum. No atomics: the same bits on every run. Nothing in a launch waits for another workgroup; data crosses compute
// units at kernel boundaries only. A block of right-hand sides goes eight columns per pass, the column on the grid's second dimension of the same
// kernels: every column has the bits of the single-column application.
#include "ksgpu_internal.h"
#include "ks_csr.h"
#include "ks_sweeps.cuh"
#include <algorithm>

namespace {
constexpr int AMG_THREADS = 256;
constexpr int AMG_MULTI_COLUMNS = 8;

struct AmgCsr { int *rp = nullptr, *col = nullptr; double *val = nullptr; int nrows = 0, lanes = 1; long long nnz = 0; };
struct AmgLevelDev {
  int n = 0; double rho = 0.0;
  ks_mat A = nullptr;                    // the level's operator (every level but the last)
  double *dinv = nullptr;                // 1 / a_ii
  AmgCsr P, R;                           // n x n_coarse, n_coarse x n
  double *b = nullptr, *x = nullptr;     // right-hand side and iterate, AMG_MULTI_COLUMNS columns of n (level 0 works on the caller's)
  double *t = nullptr, *d = nullptr;     // the product A x and the Chebyshev direction, AMG_MULTI_COLUMNS columns of n
};
} // namespace

struct KsAmg {
  int degree = 2;
  std::vector<AmgLevelDev> lev;
  KsLu *lu = nullptr;                    // the factors of the last level's operator
  size_t bytes = 0;
  ksc::AmgPlan plan;                     // the host arrays behind ks_pc_amg_level (operators, prolongators, aggregates; the restrictions are released)
};

namespace {
// d = c1 d + c2 D^-1 (b - t), x += d. first: step 0, d is not read; from_zero: x is not read either; t NULL: r = b
__global__ void __launch_bounds__(AMG_THREADS) k_amg_cheby(int n, const double *__restrict__ t, const double *__restrict__ b, long long ldb, const double *__restrict__ dinv,
                                                           double *__restrict__ d, double *__restrict__ x, long long ldx, double c1, double c2, int first, int from_zero)
{
  b += blockIdx.y * ldb; x += blockIdx.y * ldx; d += (size_t)blockIdx.y * n;
  if (t) t += (size_t)blockIdx.y * n;
  for (long long i = (long long)blockIdx.x * AMG_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * AMG_THREADS) {
    const double r = t ? b[i] - t[i] : b[i];
    const double z = c2 * (dinv[i] * r);
    const double dn = first ? z : fma(c1, d[i], z);
    d[i] = dn;
    x[i] = from_zero ? dn : x[i] + dn;
  }
}

// a CSR product with LANES lanes per row. RESTRICT: out = M (u - v), the subtraction in the gather (u = b, v = A x); else: out += M u
template <int LANES, bool RESTRICT>
__global__ void __launch_bounds__(AMG_THREADS) k_amg_transfer(int nrows, const int *__restrict__ rp, const int *__restrict__ col, const double *__restrict__ val,
                                                              const double *__restrict__ u, long long ldu, const double *__restrict__ v, long long ldv, double *__restrict__ out, long long ldo)
{
  u += blockIdx.y * ldu; out += blockIdx.y * ldo;
  if (RESTRICT) v += blockIdx.y * ldv;
  const long long g = ((long long)blockIdx.x * AMG_THREADS + threadIdx.x) / LANES;
  const int l = threadIdx.x % LANES;
  const bool live = g < nrows;                         // a group past the last row takes part in the DPP sums with zeros
  const int r = live ? (int)g : 0;
  const int e0 = live ? rp[r] : 0, e1 = live ? rp[r + 1] : 0;
  double acc = 0.0;
  for (int p = e0 + l; p < e1; p += LANES) {
    const int c = col[p];
    acc = fma(val[p], RESTRICT ? u[c] - v[c] : u[c], acc);
  }
  acc = ksk::group_sum<LANES>(acc);
  if (live && l == 0) out[r] = RESTRICT ? acc : out[r] + acc;
}

inline int lanes_for(long long nnz, int nrows)        // the cut points of the LU levels (ksc::csr_lu_plan)
{
  const double mean = nrows > 0 ? (double)nnz / nrows : 0.0;
  return mean <= 2.0 ? 1 : mean <= 16.0 ? 8 : 64;
}

template <bool RESTRICT>
int transfer(ks_ctx ctx, const AmgCsr &M, int nc, const double *u, long long ldu, const double *v, long long ldv, double *out, long long ldo)
{
  if (M.nrows == 0 || nc == 0) return KS_SUCCESS;
  const dim3 grid((unsigned)(((long long)M.nrows * M.lanes + AMG_THREADS - 1) / AMG_THREADS), (unsigned)nc);
  if (M.lanes == 1) hipLaunchKernelGGL((k_amg_transfer<1, RESTRICT>), grid, dim3(AMG_THREADS), 0, ctx->stream, M.nrows, M.rp, M.col, M.val, u, ldu, v, ldv, out, ldo);
  else if (M.lanes == 8) hipLaunchKernelGGL((k_amg_transfer<8, RESTRICT>), grid, dim3(AMG_THREADS), 0, ctx->stream, M.nrows, M.rp, M.col, M.val, u, ldu, v, ldv, out, ldo);
  else hipLaunchKernelGGL((k_amg_transfer<64, RESTRICT>), grid, dim3(AMG_THREADS), 0, ctx->stream, M.nrows, M.rp, M.col, M.val, u, ldu, v, ldv, out, ldo);
  KS_HIP(hipGetLastError());
  return KS_SUCCESS;
}

// `degree` Chebyshev steps on level L for nc columns; from_zero: x holds nothing yet
int smooth(ks_ctx ctx, const AmgLevelDev &L, int degree, int nc, const double *b, long long ldb, double *x, long long ldx, bool from_zero)
{
  const double lo = 0.1 * L.rho, hi = L.rho, theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo), sigma = theta / delta;
  double rk = 1.0 / sigma;
  const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>(((long long)L.n + AMG_THREADS - 1) / AMG_THREADS, (long long)ctx->num_cu * 16)), (unsigned)nc);
  for (int k = 0; k < degree; k++) {
    const bool no_product = from_zero && k == 0;
    if (!no_product) KS_CALL(ks_mat_mult_multi_internal(L.A, nc, x, (int)ldx, L.t, L.n));
    double c1 = 0.0, c2 = 1.0 / theta;
    if (k > 0) { const double rn = 1.0 / (2.0 * sigma - rk); c1 = rn * rk; c2 = 2.0 * rn / delta; rk = rn; }
    hipLaunchKernelGGL(k_amg_cheby, grid, dim3(AMG_THREADS), 0, ctx->stream, L.n, no_product ? (const double *)nullptr : L.t, b, ldb, L.dinv, L.d, x, ldx, c1, c2, k == 0 ? 1 : 0, no_product ? 1 : 0);
    KS_HIP(hipGetLastError());
  }
  return KS_SUCCESS;
}

// x = the V-cycle of level l on b, nc (<= AMG_MULTI_COLUMNS) columns
int cycle(ks_ctx ctx, const KsAmg *p, int l, int nc, const double *b, long long ldb, double *x, long long ldx)
{
  if (l + 1 == (int)p->lev.size()) return nc == 1 ? ks_pc_lu_apply(ctx, p->lu, b, x) : ks_pc_lu_apply_multi(ctx, p->lu, nc, b, ldb, x, ldx);
  const AmgLevelDev &L = p->lev[l], &C = p->lev[l + 1];
  KS_CALL(smooth(ctx, L, p->degree, nc, b, ldb, x, ldx, true));
  KS_CALL(ks_mat_mult_multi_internal(L.A, nc, x, (int)ldx, L.t, L.n));
  KS_CALL(transfer<true>(ctx, L.R, nc, b, ldb, L.t, L.n, C.b, C.n));
  KS_CALL(cycle(ctx, p, l + 1, nc, C.b, C.n, C.x, C.n));
  KS_CALL(transfer<false>(ctx, L.P, nc, C.x, C.n, nullptr, 0, x, ldx));
  return smooth(ctx, L, p->degree, nc, b, ldb, x, ldx, false);
}

template <class T> int upload(ks_ctx ctx, T **dst, const T *src, size_t count, size_t *bytes)
{
  const size_t b = sizeof(T) * std::max<size_t>(count, 1);
  if (hipMalloc((void **)dst, b) != hipSuccess) { (void)hipGetLastError(); *dst = nullptr; KS_FAIL(KS_ERR_MEM, "AMG set-up: no device memory for %zu bytes of the hierarchy", b); }
  *bytes += b;
  if (src && count) KS_HIP(hipMemcpyAsync(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice, ctx->stream));
  return KS_SUCCESS;
}
int upload_csr(ks_ctx ctx, AmgCsr &M, int nrows, const std::vector<int> &rp, const std::vector<int> &col, const std::vector<double> &val, size_t *bytes)
{
  M.nrows = nrows; M.nnz = (long long)col.size(); M.lanes = lanes_for(M.nnz, nrows);
  KS_CALL(upload(ctx, &M.rp, rp.data(), rp.size(), bytes));
  KS_CALL(upload(ctx, &M.col, col.data(), col.size(), bytes));
  return upload(ctx, &M.val, val.data(), val.size(), bytes);
}
int work(ks_ctx ctx, double **dst, int n, size_t *bytes) { return upload<double>(ctx, dst, nullptr, (size_t)AMG_MULTI_COLUMNS * std::max(n, 1), bytes); }
void free_csr(AmgCsr &M) { hipFree(M.rp); hipFree(M.col); hipFree(M.val); M = AmgCsr(); }

int upload_hierarchy(ks_ctx ctx, KsAmg *p)
{
  const int nlev = (int)p->plan.levels.size();
  p->lev.resize((size_t)nlev);
  for (int l = 0; l < nlev; l++) {
    ksc::AmgLevel &H = p->plan.levels[l];
    AmgLevelDev &L = p->lev[l];
    L.n = H.n; L.rho = H.rho;
    if (l > 0) { KS_CALL(work(ctx, &L.b, L.n, &p->bytes)); KS_CALL(work(ctx, &L.x, L.n, &p->bytes)); }
    if (l + 1 == nlev) {
      KS_CALL(ks_pc_lu_build(ctx, H.n, H.rp.data(), H.col.data(), H.val.data(), KS_ORDERING_ND, false, &p->lu));
      continue;
    }
    KS_CALL(ks_mat_assemble_local(ctx, H.n, 0, H.n, H.rp.data(), H.col.data(), H.val.data(), &L.A));
    p->bytes += (size_t)12 * H.col.size() + (size_t)4 * (H.n + 1);      // the operator as CSR would hold it (the layout the chooser took may be smaller)
    KS_CALL(upload(ctx, &L.dinv, H.dinv.data(), H.dinv.size(), &p->bytes));
    KS_CALL(upload_csr(ctx, L.P, H.n, H.prp, H.pcol, H.pval, &p->bytes));
    KS_CALL(upload_csr(ctx, L.R, H.nagg, H.rrp, H.rcol, H.rval, &p->bytes));
    KS_CALL(work(ctx, &L.t, L.n, &p->bytes)); KS_CALL(work(ctx, &L.d, L.n, &p->bytes));
  }
  const hipError_t e = ks_sync(ctx);                                    // the uploads have left the plan's vectors
  if (e != hipSuccess) KS_FAIL(KS_ERR_LIB, "AMG set-up: %s", hipGetErrorString(e));
  for (ksc::AmgLevel &H : p->plan.levels) { std::vector<int>().swap(H.rrp); std::vector<int>().swap(H.rcol); std::vector<double>().swap(H.rval); std::vector<double>().swap(H.dinv); }
  return KS_SUCCESS;
}
} // namespace

void ks_pc_amg_free(KsAmg *p)
{
  if (!p) return;
  for (AmgLevelDev &L : p->lev) {
    if (L.A) ks_mat_destroy(L.A);
    hipFree(L.dinv); hipFree(L.b); hipFree(L.x); hipFree(L.t); hipFree(L.d);
    free_csr(L.P); free_csr(L.R);
  }
  ks_pc_lu_free(p->lu);
  delete p;
}

int ks_pc_amg_build(ks_ctx ctx, int n, const int *rp, const int *col, const double *val, const KsAmgOptions &opt, KsAmg **out)
{
  KsAmg *p = nullptr;
  try {
    p = new KsAmg();
    ksc::AmgOptions o; o.theta = opt.theta; o.coarse_limit = opt.coarse_limit; o.max_levels = opt.max_levels; o.smooth = opt.smooth;
    ksc::amg_plan(n, rp, col, val, o, p->plan);
  } catch (const std::exception &e) { delete p; KS_FAIL(KS_ERR_MEM, "AMG set-up: %s", e.what()); }
  const ksc::AmgPlan &plan = p->plan;
  int rc = KS_SUCCESS;
  if (plan.status == ksc::AMG_NO_DIAGONAL) { ks_set_error("Matrix is missing diagonal entry, or stores a zero there, in row %d of level %d of the multigrid hierarchy", plan.bad_row, plan.bad_level); rc = KS_ERR_ARG_WRONGSTATE; }
  else if (plan.status == ksc::AMG_TOO_LARGE) { ks_set_error("a product of the multigrid set-up on level %d has more than 2^31 - 1 entries", plan.bad_level); rc = KS_ERR_ARG_OUTOFRANGE; }
  p->degree = opt.degree;
  if (!rc) {
    try { rc = upload_hierarchy(ctx, p); }
    catch (const std::exception &e) { ks_set_error("AMG set-up: %s", e.what()); rc = KS_ERR_MEM; }
  }
  if (rc) { (void)hipStreamSynchronize(ctx->stream); ks_pc_amg_free(p); return rc; }      // (no upload may still be reading the plan)
  *out = p;
  return KS_SUCCESS;
}

int ks_pc_amg_apply(ks_ctx ctx, const KsAmg *p, const double *in, double *out) { return cycle(ctx, p, 0, 1, in, 0, out, 0); }
int ks_pc_amg_multi_columns() { return AMG_MULTI_COLUMNS; }
int ks_pc_amg_apply_multi(ks_ctx ctx, const KsAmg *p, int ncols, const double *X, long long ldx, double *Y, long long ldy)
{
  for (int c0 = 0; c0 < ncols; c0 += AMG_MULTI_COLUMNS)
    KS_CALL(cycle(ctx, p, 0, std::min(AMG_MULTI_COLUMNS, ncols - c0), X + (size_t)c0 * ldx, ldx, Y + (size_t)c0 * ldy, ldy));
  return KS_SUCCESS;
}

void ks_pc_amg_info(const KsAmg *p, KsAmgInfo *o)
{
  *o = KsAmgInfo();
  o->levels = (int)p->lev.size();
  long long total = 0;
  for (int l = 0; l < o->levels; l++) {
    const ksc::AmgLevel &H = p->plan.levels[l];
    o->rows[l] = H.n; o->nnz[l] = (long long)H.col.size(); o->rho[l] = H.rho;
    total += o->nnz[l];
  }
  o->complexity = o->nnz[0] > 0 ? (double)total / (double)o->nnz[0] : 1.0;
  KsLuInfo lu; ks_pc_lu_info(p->lu, &lu);
  o->bytes = (long long)p->bytes + lu.bytes;
  // one application of one column: per smoothed level 2 nu Chebyshev updates, 2 nu products (a product counted as one), the restriction and the
  // prolongation; the last level's triangular solves as PCLUGetInfo counts them
  o->launches = (o->levels - 1) * (4 * p->degree + 2) + lu.wide_launches + lu.narrow_launches;
}

int ks_pc_amg_level(const KsAmg *p, int level, int *n, int *nagg, const int **arp, const int **acol, const double **aval, const int **prp, const int **pcol, const double **pval, const int **agg)
{
  KS_CHECK(level >= 0 && level < (int)p->plan.levels.size(), KS_ERR_ARG_OUTOFRANGE, "level %d of a hierarchy of %d", level, (int)p->plan.levels.size());
  const ksc::AmgLevel &H = p->plan.levels[level];
  const bool last = level + 1 == (int)p->plan.levels.size();
  *n = H.n; *nagg = last ? 0 : H.nagg;
  *arp = H.rp.data(); *acol = H.col.data(); *aval = H.val.data();
  *prp = last ? nullptr : H.prp.data(); *pcol = last ? nullptr : H.pcol.data(); *pval = last ? nullptr : H.pval.data(); *agg = last ? nullptr : H.agg.data();
  return KS_SUCCESS;
}

#ifdef KSD_TEST_HOOKS
// test hook: one transfer kernel on a rectangular CSR of the caller's (host arrays), nvec columns. restriction != 0: out = M (u - v), u and v being
// ncols x nvec; else out = w + M u, u being ncols x nvec and v = w nrows x nvec. out: nrows x nvec. lanes: 1, 8, 64, or 0 for the library's choice.
extern "C" int ks_pc_amg_test_transfer(ks_ctx ctx, int restriction, int lanes, int nrows, int ncols, const int *rp, const int *col, const double *val,
                                       int nvec, const double *u_host, const double *v_host, double *out_host)
{
  KS_CHECK(ctx && rp && u_host && v_host && out_host, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(nrows >= 1 && ncols >= 1 && nvec >= 1, KS_ERR_ARG_OUTOFRANGE, "rows %d, columns %d, vectors %d must be positive", nrows, ncols, nvec);
  KS_CHECK(lanes == 0 || lanes == 1 || lanes == 8 || lanes == 64, KS_ERR_ARG_OUTOFRANGE, "lanes per row %d (0, 1, 8, 64)", lanes);
  KS_CHECK(rp[0] == 0, KS_ERR_ARG_OUTOFRANGE, "row pointers must start at 0");
  for (int r = 0; r < nrows; r++) KS_CHECK(rp[r + 1] >= rp[r], KS_ERR_ARG_OUTOFRANGE, "row pointers must not descend (row %d)", r);
  KS_CHECK(rp[nrows] == 0 || (col && val), KS_ERR_ARG_NULL, "NULL argument");
  for (int e = 0; e < rp[nrows]; e++) KS_CHECK(col[e] >= 0 && col[e] < ncols, KS_ERR_ARG_OUTOFRANGE, "column %d of entry %d is outside [0, %d)", col[e], e, ncols);
  KS_HIP(hipSetDevice(ctx->device));
  AmgCsr M; double *u = nullptr, *v = nullptr, *out = nullptr; size_t bytes = 0;
  const std::vector<int> vrp(rp, rp + nrows + 1), vcol(col, col + rp[nrows]); const std::vector<double> vval(val, val + rp[nrows]);
  const size_t nu = (size_t)ncols * nvec, no = (size_t)nrows * nvec;
  int rc = upload_csr(ctx, M, nrows, vrp, vcol, vval, &bytes);
  if (lanes) M.lanes = lanes;
  if (!rc) rc = upload(ctx, &u, u_host, nu, &bytes);
  if (!rc && restriction) rc = upload(ctx, &v, v_host, nu, &bytes);
  if (!rc) rc = upload(ctx, &out, restriction ? (const double *)nullptr : v_host, no, &bytes);
  for (int c0 = 0; !rc && c0 < nvec; c0 += AMG_MULTI_COLUMNS) {
    const int nc = std::min(AMG_MULTI_COLUMNS, nvec - c0);
    rc = restriction ? transfer<true>(ctx, M, nc, u + (size_t)c0 * ncols, ncols, v + (size_t)c0 * ncols, ncols, out + (size_t)c0 * nrows, nrows)
                     : transfer<false>(ctx, M, nc, u + (size_t)c0 * ncols, ncols, nullptr, 0, out + (size_t)c0 * nrows, nrows);
  }
  if (!rc && hipMemcpyAsync(out_host, out, sizeof(double) * no, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) { ks_set_error("the copy of the result failed"); rc = KS_ERR_LIB; }
  if (ks_sync(ctx) != hipSuccess && !rc) { ks_set_error("the transfer kernel failed"); rc = KS_ERR_LIB; }
  free_csr(M); hipFree(u); hipFree(v); hipFree(out);
  return rc;
}
#endif
