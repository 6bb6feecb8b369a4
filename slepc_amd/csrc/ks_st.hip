// Spectral transformation: the operator the Krylov expansion multiplies by (the caller side of MatMult on the path).
//
// Restates STSHIFT and STSINVERT (src/sys/classes/st/impls/shift/shift.c:16-97, sinvert/sinvert.c:16-77) with
// STApply_Generic (src/sys/classes/st/interface/stsolve.c:16-25):  y = P^-1 M x,
//     shift:    nmat=1  M = A - sigma I, P none          nmat=2  M = A - sigma B, P = B
//     sinvert:  nmat=1  M none,          P = A - sigma I nmat=2  M = B,           P = A - sigma B
//     cayley:   nmat=1  M = A + nu I,    P = A - sigma I nmat=2  M = A + nu B,    P = A - sigma B   (cayley/cayley.c:138-165)
// in the reference's ST_MATMODE_SHELL form: A - sigma B is never assembled, it is applied as two SpMVs and an
// axpy (stshellmat.c), and its diagonal is diag(A) - sigma diag(B). The linear solves are the KSP that mode
// defaults to (stsles.c:51-53): GMRES(30) with a Jacobi preconditioner on the left, relative tolerance
// SLEPC_DEFAULT_TOL on the preconditioned residual (stsles.c:407), zero initial guess, failure to converge is an
// error (KSPSetErrorIfNotConverged, stsles.c:58). PETSc's KSP itself is external to the reference; this GMRES runs on
// the same device kernels as the outer iteration: the Krylov basis is a BV, its Gram-Schmidt is the fused CGS of
// ks_gs.hip, the update x += K y is BVMultVec.
//
// Transposed solves (ks_st_set_transpose_solves; STMatSolveTranspose stsolve.c, KSPSolveTranspose, PCApplyTranspose): P^T is applied through the
// transposed views of A and B (shell mode) or of the assembled P (copy mode), the preconditioner through its own transpose - point Jacobi is its own,
// the dense blocks are walked by columns, the ILU(0) blocks have a second plan of the same factors (ks_pc.hip). The KSPs are the same code with a
// side: left-preconditioned on M^-T P^T y = M^-T b (PCApplyBAorABTranspose, PC_LEFT). STApplyTranspose_Generic (stsolve.c:107-116) sits on top.
#include "ksgpu_internal.h"
#include "ks_csr.h"
#include "ks_ds.h"
#include <algorithm>

namespace {

// out = s .* (a*u + b*v)   (s, v may be NULL: s = 1, v ignored)
__global__ void k_lincomb(long long n, const double *__restrict__ s, double a, const double *__restrict__ u, double b, const double *__restrict__ v, double *__restrict__ out)
{
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    double t = a * u[i];
    if (v) t += b * v[i];
    out[i] = s ? s[i] * t : t;
  }
}
// d = 1 / (a*da + b*db), db NULL = identity; a zero diagonal entry leaves the row unscaled (PCJacobi does the same); use_abs: 1 / |a*da + b*db| (PCJacobiSetUseAbs)
__global__ void k_jacobi_setup(long long n, double a, const double *__restrict__ da, double b, const double *__restrict__ db, double *__restrict__ d, int use_abs)
{
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    double t = (da ? a * da[i] : 0.0) + b * (db ? db[i] : 1.0);
    if (use_abs) t = fabs(t);
    d[i] = (t != 0.0) ? 1.0 / t : 1.0;
  }
}

// out = M^-1 in for the block-Jacobi M: row i of out is row i of its block's inverse times the block's piece of in (binv: n x bs, row-major)
// (blockIdx.y: the column of a block of vectors, ks_st_pc_apply_multi; a single vector is the launch with gridDim.y = 1)
__global__ void k_bjacobi_apply(long long n, int bs, const double *__restrict__ binv, const double *__restrict__ in, long long ldin, double *__restrict__ out, long long ldout)
{
  in += blockIdx.y * ldin; out += blockIdx.y * ldout;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long b0 = i / bs * bs;
    const double *row = binv + i * bs;
    double acc = 0.0;
    for (int c = 0; c < bs && b0 + c < n; c++) acc = fma(row[c], in[b0 + c], acc);
    out[i] = acc;
  }
}

// out(:,j) = s .* in(:,j) for the columns j = blockIdx.y of a block (s NULL: a copy): point Jacobi and PCNONE applied to a block of vectors. The product
// is the one k_lincomb forms for a single vector (1.0 * u is exact), so every column has the bits of ks_st_pc_apply.
__global__ void k_diag_apply_multi(long long n, const double *__restrict__ s, const double *__restrict__ in, long long ldin, double *__restrict__ out, long long ldout)
{
  in += blockIdx.y * ldin; out += blockIdx.y * ldout;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = s ? s[i] * in[i] : in[i];
}

// out = M^-T in: row i of out is COLUMN i of its block's inverse times the block's piece of in - the same array, walked with stride bs
__global__ void k_bjacobi_apply_t(long long n, int bs, const double *__restrict__ binv, const double *__restrict__ in, double *__restrict__ out)
{
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long b0 = i / bs * bs;
    const double *colm = binv + b0 * bs + (i - b0);
    double acc = 0.0;
    for (int c = 0; c < bs && b0 + c < n; c++) acc = fma(colm[(long long)c * bs], in[b0 + c], acc);
    out[i] = acc;
  }
}

} // namespace
int ksk_lincomb(ks_ctx ctx, long long n, const double *s, double a, const double *u, double b, const double *v, double *out)
{
  if (n == 0) return KS_SUCCESS;
  const unsigned nb = (unsigned)std::min<long long>((n + 255) / 256, (long long)ctx->num_cu * 16);
  hipLaunchKernelGGL(k_lincomb, dim3(nb), dim3(256), 0, ctx->stream, n, s, a, u, b, v, out);
  KS_HIP(hipGetLastError());
  return KS_SUCCESS;
}
namespace {
inline int lincomb(ks_ctx ctx, long long n, const double *s, double a, const double *u, double b, const double *v, double *out) { return ksk_lincomb(ctx, n, s, a, u, b, v, out); }
inline bool pc_none(ks_st st) { return st->pc_type == KS_PC_NONE || st->pc_identity; }      // no preconditioner: the caller's choice, or STPRECOND's infinite default shift on one matrix

// out = s .* (a*A*x + b*(B*x | x)); tmp is scratch of n doubles (used when both terms are present)
int linop_apply(ks_st st, double a, ks_mat A, double b, ks_mat B, bool identity_term, const double *s, const double *x, double *out, double *tmp)
{
  ks_ctx ctx = st->ctx;
  const long long n = st->n;
  if (A) {
    if (s && a == 1.0 && (b == 0.0 || (!B && !identity_term)) && ks_mat_can_rowscale(A)) return ks_mat_mult_internal(A, x, out, s);   // out = s .* (A x) in the product's own launches
    KS_CALL(ks_mat_mult_internal(A, x, out));
    if (b != 0.0) {                                         // a zero shift leaves A alone (MatMult_Shell, stshellmat.c:52: "if (ctx->alpha!=0.0)")
      if (B) { KS_CALL(ks_mat_mult_internal(B, x, tmp)); return lincomb(ctx, n, s, a, out, b, tmp, out); }
      if (identity_term) return lincomb(ctx, n, s, a, out, b, x, out);
    }
    if (s || a != 1.0) return lincomb(ctx, n, s, a, out, 0.0, nullptr, out);
    return KS_SUCCESS;
  }
  if (B) { KS_CALL(ks_mat_mult_internal(B, x, out)); if (s || b != 1.0) return lincomb(ctx, n, s, b, out, 0.0, nullptr, out); return KS_SUCCESS; }
  return lincomb(ctx, n, s, b, x, 0.0, nullptr, out);
}

// the matrix P of the table above, y = s .* P x; tr: y = s .* P^T x through the transposed views (assembled matrices like the ones they view)
int apply_P(ks_st st, const double *s, const double *x, double *out, double *tmp, bool tr = false)
{
  ks_mat Pm = tr ? st->PmatT : st->Pmat, A = tr ? st->At : st->A, B = tr ? st->Bt : st->B;
  if (Pm) {                                                  // ST_MATMODE_COPY: the assembled A - sigma B, one product
    if (s && ks_mat_can_rowscale(Pm)) return ks_mat_mult_internal(Pm, x, out, s);
    KS_CALL(ks_mat_mult_internal(Pm, x, out));
    return s ? lincomb(st->ctx, st->n, s, 1.0, out, 0.0, nullptr, out) : KS_SUCCESS;
  }
  if (st->type != KS_ST_SHIFT) return linop_apply(st, 1.0, A, -st->sigma, B, !B, s, x, out, tmp);     // sinvert, cayley (and the K of STPRECOND)
  return linop_apply(st, 0.0, nullptr, 1.0, B, false, s, x, out, tmp);               // shift, nmat=2: P = B
}

int bjacobi_apply(ks_st st, const double *in, double *out, bool tr = false)
{
  if (st->n == 0) return KS_SUCCESS;
  const unsigned nb = (unsigned)std::min<long long>(((long long)st->n + 255) / 256, (long long)st->ctx->num_cu * 16);
  if (tr) hipLaunchKernelGGL(k_bjacobi_apply_t, dim3(nb), dim3(256), 0, st->ctx->stream, (long long)st->n, st->pc_bs, st->binv, in, out);
  else hipLaunchKernelGGL(k_bjacobi_apply, dim3(nb), dim3(256), 0, st->ctx->stream, (long long)st->n, st->pc_bs, st->binv, in, 0LL, out, 0LL);
  KS_HIP(hipGetLastError());
  return KS_SUCCESS;
}
// out = M^-1 in for the preconditioners that are not pointwise: the dense inverses, the ILU(0) factors (k_bjacobi_ilu_apply, ks_pc.hip), or the LU
// factors of the whole P (ks_pc_lu.hip), or the multigrid cycle on P (ks_pc_amg.hip)
int blocks_apply(ks_st st, const double *in, double *out, bool tr = false)
{
  if (st->pc_type == KS_PC_LU) return tr ? ks_pc_lu_apply_transpose(st->ctx, st->lu, in, out) : ks_pc_lu_apply(st->ctx, st->lu, in, out);
  if (st->pc_type == KS_PC_AMG) {
    KS_CHECK(!tr, KS_ERR_SUP, "KS_PC_AMG has no transposed cycle");
    return ks_pc_amg_apply(st->ctx, st->amg, in, out);
  }
  if (st->pc_type == KS_PC_BJACOBI_ILU) return tr ? ks_pc_ilu_apply_transpose(st->ctx, st->ilu, in, out) : ks_pc_ilu_apply(st->ctx, st->ilu, in, out);
  return bjacobi_apply(st, in, out, tr);
}
// out = M^-1 (a u + b v) with the left preconditioner M of the KSP: diag(P) (one fused kernel) or the diagonal blocks of P; tr: M^-T (point Jacobi is its own)
int pc_lincomb(ks_st st, double a, const double *u, double b, const double *v, double *out, bool tr = false)
{
  if (st->pc_type == KS_PC_JACOBI || pc_none(st)) return lincomb(st->ctx, st->n, pc_none(st) ? nullptr : st->dinv, a, u, b, v, out);
  if ((st->pc_type == KS_PC_LU || st->pc_type == KS_PC_AMG) && a == 1.0 && (b == 0.0 || !v) && u != out) return blocks_apply(st, u, out, tr);      // the factors read u through their permutation, the cycle only reads it: no copy
  KS_CALL(lincomb(st->ctx, st->n, nullptr, a, u, b, v, st->pcwork));
  return blocks_apply(st, st->pcwork, out, tr);
}
// out = M^-1 P x; tr: out = M^-T P^T x (PCApplyBAorABTranspose, PC_LEFT)
int apply_MP(ks_st st, const double *x, double *out, double *tmp, bool tr = false)
{
  if (st->pc_type == KS_PC_JACOBI || st->pc_type == KS_PC_NONE) return apply_P(st, st->pc_type == KS_PC_NONE ? nullptr : st->dinv, x, out, tmp, tr);
  KS_CALL(apply_P(st, nullptr, x, st->pcwork, tmp, tr));
  return blocks_apply(st, st->pcwork, out, tr);
}

// The ST's own linear system as the KSPs below see it (KsKspOp, ksgpu_internal.h): M^-1 P with the left preconditioner M of the table above; tr: the
// transposed side of both. The calls and their order are the ones the two solvers made before they took an operator.
struct StKspOp : KsKspOp {
  ks_st st; bool tr; double *t1, *t2;
  StKspOp(ks_st s, bool t) : st(s), tr(t), t1(ks_bv_col(s->W, 1)), t2(ks_bv_col(s->W, 2)) {}
  int apply(const double *x, double *out) override { return apply_MP(st, x, out, t1, tr); }
  int residual(const double *rhs, const double *y, double *out) override
  {
    if (!y) return pc_lincomb(st, 1.0, rhs, 0.0, nullptr, out, tr);
    KS_CALL(apply_P(st, nullptr, y, t1, t2, tr));
    return pc_lincomb(st, 1.0, rhs, -1.0, t1, out, tr);
  }
};
KsKsp st_ksp(ks_st st) { return KsKsp{st->ctx, (long long)st->n, st->K, st->Kb, st->rtol, st->max_it, st->restart, true, &st->solves, &st->its, &st->last_rnorm}; }

} // namespace

// out = M^-1 P x into column jout of K, then *dot = (e, out): the operator application, then the BVDotVec of that one column (one host wait)
int KsKspOp::apply_dot(const double *x, double *out, ks_bv K, int jout, const double *e, double *dot)
{
  KS_CALL(apply(x, out));
  KS_CALL(ks_bv_set_active_columns(K, jout, jout + 1));
  return ks_bv_dotvec(K, e, dot);
}

// Left-preconditioned restarted GMRES for P y = rhs (KSPGMRES defaults: restart 30, classical Gram-Schmidt) on the operator M^-1 P and the residual
// M^-1 (rhs - P y) of `op`; the ST's transposed solves (KSPSolveTranspose) are the same iteration with an operator on the transposed side. k.strict:
// failure to converge is an error (the ST); otherwise the iterate reached after max_it iterations is the answer (the Jacobi-Davidson correction).
int ks_ksp_gmres(const KsKsp &k, KsKspOp &op, const double *rhs, double *y)
{
  ks_ctx ctx = k.ctx; ks_bv K = k.K;
  const int m = k.restart;
  const long long n = k.n;
  std::vector<double> H((size_t)(m + 1) * m, 0.0), g(m + 1, 0.0), cs(m, 0.0), sn(m, 0.0), h(m + 1, 0.0), yc(m, 0.0);
  (*k.solves)++;
  KS_HIP(hipMemsetAsync(y, 0, sizeof(double) * std::max<long long>(n, 1), ctx->stream));
  KS_CALL(op.residual(rhs, nullptr, ks_bv_col(K, 0)));
  double beta = 0.0;
  const bool split = ks_bv_orthonormalize_can_split(K);
  bool k0_normalised = false, applied0 = false;
  if (split) {
    // norm and scaling of the first basis vector as one enqueued program (BVOrthonormalizeColumn of column 0), the first operator application behind it:
    // the host learns beta while the product runs
    int lin0 = 0, late0 = 0;
    KS_CALL(ks_bv_orthonormalize_enqueue(K, 0));
    KS_CALL(op.apply(ks_bv_col(K, 0), ks_bv_col(K, 1)));
    KS_CALL(ks_bv_orthonormalize_collect(K, 0, nullptr, &beta, &lin0, &late0));
    k0_normalised = true; applied0 = !late0;
  } else KS_CALL(ks_bv_normcolumn(K, 0, KS_NORM_2, &beta));
  *k.last_rnorm = beta;
  if (beta == 0.0 || (!k.strict && !std::isfinite(beta))) return KS_SUCCESS;
  const double tol = std::max(k.rtol * beta, 1e-50);
  int its = 0;
  for (;;) {
    if (!k0_normalised) KS_CALL(ks_bv_scalecolumn(K, 0, 1.0 / beta));
    k0_normalised = false;
    std::fill(g.begin(), g.end(), 0.0); g[0] = beta;
    int jj = 0; double res = beta, res_before = beta;
    bool applied = applied0;                        // K(:, j+1) = P K(:, j) already enqueued (speculatively, during the previous iteration)
    applied0 = false;
    for (int j = 0; j < m; j++) {
      if (!applied) KS_CALL(op.apply(ks_bv_col(K, j), ks_bv_col(K, j + 1)));
      applied = false;
      double hn = 0.0; int lindep = 0;
      if (split) {
        // The next operator application goes in behind the orthogonalisation BEFORE the host waits for this column's coefficients, so the device
        // is not idle while the host rotates and tests (30 us per iteration in the trace, profiles/r02_config5_kernel_trace_gaps.txt) - but only
        // when the residual history says another iteration is coming: a product wasted on the last iteration costs more than the gaps of a solve.
        const double predicted = (j == 0) ? res : res * std::min(1.0, res / res_before);
        const bool spec = (j + 1 < m) && (its + 1 < k.max_it) && predicted > 3.0 * tol;
        int late = 0;
        KS_CALL(ks_bv_orthonormalize_enqueue(K, j + 1));
        if (spec) KS_CALL(op.apply(ks_bv_col(K, j + 1), ks_bv_col(K, j + 2)));
        KS_CALL(ks_bv_orthonormalize_collect(K, j + 1, h.data(), &hn, &lindep, &late));
        applied = spec && !late;                    // a column completed late was multiplied unfinished: apply again
      } else KS_CALL(ks_bv_orthonormalize_coefs(K, j + 1, h.data(), &hn, &lindep));       // the 1/hn scaling rides in the final update; h, hn and the flag arrive in one host wait
      its++; (*k.its)++;
      h[j + 1] = hn;
      for (int i = 0; i < j; i++) { const double t = cs[i] * h[i] + sn[i] * h[i + 1]; h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1]; h[i] = t; }
      const double r = hypot(h[j], h[j + 1]);
      if (r == 0.0) { cs[j] = 1.0; sn[j] = 0.0; } else { cs[j] = h[j] / r; sn[j] = h[j + 1] / r; }
      h[j] = r; h[j + 1] = 0.0;
      g[j + 1] = -sn[j] * g[j]; g[j] = cs[j] * g[j];
      for (int i = 0; i <= j; i++) H[(size_t)i + (size_t)j * (m + 1)] = h[i];
      res_before = res; res = fabs(g[j + 1]); jj = j + 1;
      if (res <= tol || its >= k.max_it || lindep || hn == 0.0) break;
    }
    for (int i = jj - 1; i >= 0; i--) {                     // back substitution R yc = g
      double t = g[i];
      for (int c = i + 1; c < jj; c++) t -= H[(size_t)i + (size_t)c * (m + 1)] * yc[c];
      const double d = H[(size_t)i + (size_t)i * (m + 1)];
      yc[i] = (d != 0.0) ? t / d : 0.0;
    }
    KS_CALL(ks_bv_set_active_columns(K, 0, jj));
    KS_CALL(ks_bv_multvec(K, 1.0, 1.0, y, yc.data()));
    *k.last_rnorm = res;
    if (res <= tol) break;
    if (!k.strict && its >= k.max_it) break;
    KS_CHECK(its < k.max_it, KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: GMRES reached %d iterations, preconditioned residual %g > %g", its, res, tol);
    // restart from the true preconditioned residual
    KS_CALL(op.residual(rhs, y, ks_bv_col(K, 0)));
    KS_CALL(ks_bv_normcolumn(K, 0, KS_NORM_2, &beta));
    *k.last_rnorm = beta;
    if (beta <= tol || (!k.strict && !std::isfinite(beta))) break;
  }
  return KS_SUCCESS;
}

// Left-preconditioned BiCGStab for P y = rhs (KSPBCGS with PC_LEFT: the iteration runs on D^-1 P, the residual that is tested
// is the preconditioned one, as for the GMRES above). Two operator applications per iteration, no growing basis: the
// memory is 7 vectors whatever the iteration count. The dot products of one phase travel in one BVDotVec (one allreduce).
// Not strict: a breakdown or the iteration limit ends the solve with the iterate it has.
int ks_ksp_bcgs(const KsKsp &k, KsKspOp &op, const double *rhs, double *y)
{
  ks_ctx ctx = k.ctx; ks_bv K = k.Kb;
  const long long n = k.n;
  double *r = ks_bv_col(K, 0), *rh = ks_bv_col(K, 1), *p = ks_bv_col(K, 2), *v = ks_bv_col(K, 3), *s = ks_bv_col(K, 4), *t = ks_bv_col(K, 5);
  (*k.solves)++;
  KS_HIP(hipMemsetAsync(y, 0, sizeof(double) * std::max<long long>(n, 1), ctx->stream));
  KS_CALL(op.residual(rhs, nullptr, r));                                    // r = D^-1 b (zero initial guess)
  double beta0 = 0.0;
  KS_CALL(ks_bv_normcolumn(K, 0, KS_NORM_2, &beta0));
  *k.last_rnorm = beta0;
  if (beta0 == 0.0 || (!k.strict && !std::isfinite(beta0))) return KS_SUCCESS;
  const double tol = std::max(k.rtol * beta0, 1e-50);
  KS_CALL(ksk_copy(ctx, r, rh, n));
  KS_HIP(hipMemsetAsync(p, 0, sizeof(double) * n, ctx->stream));
  KS_HIP(hipMemsetAsync(v, 0, sizeof(double) * n, ctx->stream));
  double rho = 1.0, alpha = 1.0, omega = 1.0, d[2];
  for (int its = 0; ; its++) {
    if (!k.strict && its >= k.max_it) break;
    KS_CHECK(its < k.max_it, KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: BiCGStab reached %d iterations, preconditioned residual %g > %g", its, *k.last_rnorm, tol);
    KS_CALL(ks_bv_set_active_columns(K, 0, 1));
    KS_CALL(ks_bv_dotvec(K, rh, d));                                                 // rho' = (rhat, r)
    const double rho_new = d[0];
    if (!k.strict && (rho_new == 0.0 || omega == 0.0 || !std::isfinite(rho_new))) break;
    KS_CHECK(rho_new != 0.0 && omega != 0.0, KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: BiCGStab breakdown (rho = %g, omega = %g)", rho_new, omega);
    const double bt = (rho_new / rho) * (alpha / omega);
    KS_CALL(lincomb(ctx, n, nullptr, 1.0, p, -omega, v, p));                         // p = r + beta (p - omega v)
    KS_CALL(lincomb(ctx, n, nullptr, bt, p, 1.0, r, p));
    KS_CALL(op.apply_dot(p, v, K, 3, rh, d));                                        // v = D^-1 P p, (rhat, v)
    if (!k.strict && (d[0] == 0.0 || !std::isfinite(d[0]))) break;
    KS_CHECK(d[0] != 0.0, KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: BiCGStab breakdown ((rhat,v) = 0)");
    alpha = rho_new / d[0];
    KS_CALL(lincomb(ctx, n, nullptr, 1.0, r, -alpha, v, s));                         // s = r - alpha v
    KS_CALL(op.apply(s, t));                                                         // t = D^-1 P s
    KS_CALL(ks_bv_set_active_columns(K, 4, 6));
    KS_CALL(ks_bv_dotvec(K, t, d));                                                  // (s,t), (t,t) in one reduction
    omega = d[1] != 0.0 ? d[0] / d[1] : 0.0;
    KS_CALL(lincomb(ctx, n, nullptr, 1.0, y, alpha, p, y));                          // y += alpha p + omega s
    KS_CALL(lincomb(ctx, n, nullptr, 1.0, y, omega, s, y));
    KS_CALL(lincomb(ctx, n, nullptr, 1.0, s, -omega, t, r));                         // r = s - omega t
    rho = rho_new;
    (*k.its)++;
    double rn = 0.0;
    KS_CALL(ks_bv_normcolumn(K, 0, KS_NORM_2, &rn));
    *k.last_rnorm = rn;
    if (rn <= tol) break;
  }
  return KS_SUCCESS;
}

// KSPPREONLY: y = M^-1 rhs - one application of the preconditioner (the operator's residual with a zero iterate), no residual norm, no convergence
// test. One solve and one iteration are counted; last_rnorm is left alone.
int ks_ksp_preonly(const KsKsp &k, KsKspOp &op, const double *rhs, double *y)
{
  (*k.solves)++; (*k.its)++;
  return op.residual(rhs, nullptr, y);
}

// the product of a CG or MINRES iteration: the calls of apply_P without the combining sweep of a P with two terms, which the solver's next sweep does
int ks_st_product_one_term_left(ks_st st, bool tr, const double *p, double *w, const double **v, double *b)
{
  ks_mat Pm = tr ? st->PmatT : st->Pmat, A = tr ? st->At : st->A, B = tr ? st->Bt : st->B;
  *v = nullptr; *b = 0.0;
  if (Pm) return ks_mat_mult_internal(Pm, p, w);
  if (st->type == KS_ST_SHIFT) return ks_mat_mult_internal(B, p, w);                // shift, nmat = 2: P = B
  KS_CALL(ks_mat_mult_internal(A, p, w));
  if (st->sigma == 0.0) return KS_SUCCESS;                                          // a zero shift leaves A alone, as in linop_apply
  *b = -st->sigma; *v = p;
  if (B) { double *tmp = ks_bv_col(st->W, 1); KS_CALL(ks_mat_mult_internal(B, p, tmp)); *v = tmp; }
  return KS_SUCCESS;
}
int ks_st_blocks_apply(ks_st st, const double *in, double *out, bool tr) { return blocks_apply(st, in, out, tr); }
int ks_resident_alloc(KsResident *r, size_t head_bytes, int part_cols)               // a KsResident belongs to one solver: the same sizes at every call
{
  if (r->dev && r->host) return KS_SUCCESS;
  ks_resident_free(r);                                                              // an earlier call that got only the device half: begin again
  KS_HIP(hipMalloc(&r->dev, head_bytes + sizeof(double) * part_cols * (size_t)KS_MAX_BLOCKS));
  KS_HIP(hipHostMalloc(&r->host, head_bytes, hipHostMallocDefault));
  return KS_SUCCESS;
}
void ks_resident_free(KsResident *r)
{
  if (r->dev) hipFree(r->dev);
  if (r->host) hipHostFree(r->host);
  r->dev = nullptr; r->host = nullptr;
}

namespace {
int gmres_solve(ks_st st, const double *rhs, double *y, bool tr) { StKspOp op(st, tr); return ks_ksp_gmres(st_ksp(st), op, rhs, y); }
int bcgs_solve(ks_st st, const double *rhs, double *y, bool tr) { StKspOp op(st, tr); return ks_ksp_bcgs(st_ksp(st), op, rhs, y); }
int preonly_solve(ks_st st, const double *rhs, double *y, bool tr) { StKspOp op(st, tr); return ks_ksp_preonly(st_ksp(st), op, rhs, y); }
int inner_solve(ks_st st, const double *rhs, double *y, bool tr = false)
{
  if (st->ksp_type == KS_KSP_PREONLY) return preonly_solve(st, rhs, y, tr);
  if (st->ksp_type == KS_KSP_CG) return ks_ksp_cg(st_ksp(st), st, tr, rhs, y);
  if (st->ksp_type == KS_KSP_MINRES) return ks_ksp_minres(st_ksp(st), st, tr, rhs, y);
  if (st->ksp_type == KS_KSP_BCGSL) return ks_ksp_bcgsl(st_ksp(st), st, tr, rhs, y);
  return st->ksp_type == KS_KSP_BCGS ? bcgs_solve(st, rhs, y, tr) : gmres_solve(st, rhs, y, tr);
}

int st_shell_mult(void *user, const double *x, double *y) { return ks_st_apply_internal((ks_st)user, x, y); }
int st_shell_mult_transpose(void *user, const double *x, double *y) { return ks_st_apply_transpose_internal((ks_st)user, x, y); }
// y = (A + nu B) x, MatMult_Cayley cayley.c:21-44
int st_bilinear_mult(void *user, const double *x, double *y)
{
  ks_st st = (ks_st)user;
  return linop_apply(st, 1.0, st->A, st->nu, st->B, !st->B, nullptr, x, y, ks_bv_col(st->W, 2));
}

} // namespace

// The CSR arrays of P the block preconditioners take their blocks from: entry by entry a_ij + (-sigma b_ij) of the arrays the matrices keep
// (ks_csr.cpp, as the assembled P of ST_MATMODE_COPY has them) for sinvert and cayley, B's own for a shift with two matrices. Global columns;
// the same arrays in both matrix modes. rp / col / val hold the sum where one is formed.
static int pc_block_source(ks_st st, std::vector<int> &rp, std::vector<int> &col, std::vector<double> &val, const int **prp, const int **pcol, const double **pval)
{
  ks_mat A = st->A, B = st->B;
  const bool p_is_b = (st->type == KS_ST_SHIFT) || st->pc_on_b;    // shift, nmat = 2: P = B; STPRECOND with the infinite default shift: M from B alone
  ks_mat M0 = p_is_b ? B : A;
  KS_CHECK(M0 && M0->keep_csr && (p_is_b || !B || B->keep_csr), KS_ERR_ORDER, "the block-Jacobi preconditioner takes its blocks from the CSR arrays of the matrices: create them with KS_MAT_KEEP_CSR");
  if (p_is_b) { *prp = B->k_rowptr.data(); *pcol = B->k_col.data(); *pval = B->k_val.data(); }
  else {
    bool fits = false;
    try { fits = ksc::csr_axpy(st->n, A->row_start, A->k_rowptr.data(), A->k_col.data(), A->k_val.data(), -st->sigma, B ? B->k_rowptr.data() : nullptr, B ? B->k_col.data() : nullptr, B ? B->k_val.data() : nullptr, rp, col, val); }
    catch (const std::exception &e) { KS_FAIL(KS_ERR_MEM, "block Jacobi set-up: %s", e.what()); }
    KS_CHECK(fits, KS_ERR_ARG_OUTOFRANGE, "A - sigma B exceeds 32-bit PetscInt indices");
    *prp = rp.data(); *pcol = col.data(); *pval = val.data();
  }
  return KS_SUCCESS;
}

// Block Jacobi set-up (PCSetUp_BJacobi with LU sub-solves, PETSc): the dense diagonal blocks of P - pc_bs consecutive local rows each - from the
// CSR arrays the matrices keep, inverted on the host by Gauss-Jordan elimination with partial pivoting, uploaded row by row.
static int bjacobi_setup(ks_st st)
{
  ks_ctx ctx = st->ctx;
  const int n = st->n, bs = st->pc_bs;
  ks_mat M0 = (st->type == KS_ST_SHIFT || st->pc_on_b) ? st->B : st->A;
  std::vector<int> rp, col; std::vector<double> val;
  const int *prp; const int *pcol; const double *pval;
  KS_CALL(pc_block_source(st, rp, col, val, &prp, &pcol, &pval));
  std::vector<double> inv;
  try { inv.assign((size_t)n * bs, 0.0); } catch (const std::exception &e) { KS_FAIL(KS_ERR_MEM, "block Jacobi set-up: %s", e.what()); }
  std::vector<double> Mb((size_t)bs * 2 * bs);
  const long long base = M0->row_start;
  for (int b0 = 0; b0 < n; b0 += bs) {
    const int bl = std::min(bs, n - b0), w = 2 * bl;
    std::fill(Mb.begin(), Mb.end(), 0.0);
    for (int r = 0; r < bl; r++) {                                 // [block | I]
      for (int p = prp[b0 + r]; p < prp[b0 + r + 1]; p++) { const long long c = (long long)pcol[p] - base - b0; if (c >= 0 && c < bl) Mb[(size_t)r * w + c] += pval[p]; }
      Mb[(size_t)r * w + bl + r] = 1.0;
    }
    for (int k = 0; k < bl; k++) {
      int piv = k; double big = fabs(Mb[(size_t)k * w + k]);
      for (int r = k + 1; r < bl; r++) if (fabs(Mb[(size_t)r * w + k]) > big) { big = fabs(Mb[(size_t)r * w + k]); piv = r; }
      KS_CHECK(big != 0.0, KS_ERR_MAT_LU_ZRPVT, "Zero pivot in the block of local rows %d..%d (column %d)", b0, b0 + bl - 1, b0 + k);
      if (piv != k) for (int c = 0; c < w; c++) std::swap(Mb[(size_t)k * w + c], Mb[(size_t)piv * w + c]);
      const double d = 1.0 / Mb[(size_t)k * w + k];
      for (int c = 0; c < w; c++) Mb[(size_t)k * w + c] *= d;
      for (int r = 0; r < bl; r++) if (r != k) { const double f = Mb[(size_t)r * w + k]; if (f != 0.0) for (int c = 0; c < w; c++) Mb[(size_t)r * w + c] -= f * Mb[(size_t)k * w + c]; }
    }
    for (int r = 0; r < bl; r++) for (int c = 0; c < bl; c++) inv[(size_t)(b0 + r) * bs + c] = Mb[(size_t)r * w + bl + c];
  }
  if (st->binv) { hipFree(st->binv); st->binv = nullptr; }
  if (st->pcwork) { hipFree(st->pcwork); st->pcwork = nullptr; }
  KS_HIP(hipMalloc(&st->binv, sizeof(double) * std::max<size_t>(inv.size(), 1)));
  KS_HIP(hipMalloc(&st->pcwork, sizeof(double) * std::max(n, 1)));
  KS_HIP(hipMemcpyAsync(st->binv, inv.data(), sizeof(double) * inv.size(), hipMemcpyHostToDevice, ctx->stream));
  KS_HIP(ks_sync(ctx));
  return KS_SUCCESS;
}

// Block Jacobi with ILU(0) blocks (PCSetUp_BJacobi with -sub_pc_type ilu): the same blocks, factored on their own pattern and laid out by levels
// on the host (ksc::csr_ilu0_blocks), uploaded once per set-up (ks_pc.hip)
static int bjacobi_ilu_setup(ks_st st)
{
  ks_mat M0 = (st->type == KS_ST_SHIFT || st->pc_on_b) ? st->B : st->A;
  std::vector<int> rp, col; std::vector<double> val;
  const int *prp; const int *pcol; const double *pval;
  KS_CALL(pc_block_source(st, rp, col, val, &prp, &pcol, &pval));
  KS_CALL(ks_pc_ilu_build(st->ctx, st->n, M0->row_start, st->pc_bs, prp, pcol, pval, st->tsolves, &st->ilu));
  if (st->pcwork) { hipFree(st->pcwork); st->pcwork = nullptr; }
  KS_HIP(hipMalloc(&st->pcwork, sizeof(double) * std::max(st->n, 1)));
  return KS_SUCCESS;
}

// PCLU (PCSetUp_LU: MatGetOrdering, MatLUFactorSymbolic / Numeric): the whole P from the same arrays the blocks come from, ordered and factored with fill on
// the host (ksc::csr_lu_plan), uploaded once per set-up (ks_pc_lu.hip)
static int lu_setup(ks_st st)
{
  KS_CHECK(st->ctx->comm.size == 1, KS_ERR_SUP, "KS_PC_LU runs on one rank (PETSc's built-in LU is sequential as well)");
  std::vector<int> rp, col; std::vector<double> val;
  const int *prp; const int *pcol; const double *pval;
  KS_CALL(pc_block_source(st, rp, col, val, &prp, &pcol, &pval));
  KS_CALL(ks_pc_lu_build(st->ctx, st->n, prp, pcol, pval, st->lu_ordering, st->tsolves, &st->lu));
  if (st->pcwork) { hipFree(st->pcwork); st->pcwork = nullptr; }
  if (hipMalloc(&st->pcwork, sizeof(double) * std::max(st->n, 1)) != hipSuccess) {
    (void)hipGetLastError(); st->pcwork = nullptr; ks_pc_lu_free(st->lu); st->lu = nullptr;
    KS_FAIL(KS_ERR_MEM, "LU set-up: no device memory for a work vector of %d rows", st->n);
  }
  return KS_SUCCESS;
}

// PCGAMG with smoothed aggregation: the hierarchy of the whole P from the same arrays, made on the host (ksc::amg_plan), uploaded once per set-up (ks_pc_amg.hip)
static int amg_setup(ks_st st)
{
  KS_CHECK(st->ctx->comm.size == 1, KS_ERR_SUP, "KS_PC_AMG runs on one rank (the aggregation of a row-sharded matrix is not built)");
  KS_CHECK(!st->tsolves, KS_ERR_SUP, "KS_PC_AMG has no transposed cycle: ks_st_set_transpose_solves cannot be on with it");
  std::vector<int> rp, col; std::vector<double> val;
  const int *prp; const int *pcol; const double *pval;
  KS_CALL(pc_block_source(st, rp, col, val, &prp, &pcol, &pval));
  KS_CALL(ks_pc_amg_build(st->ctx, st->n, prp, pcol, pval, st->amg_opt, &st->amg));
  if (st->pcwork) { hipFree(st->pcwork); st->pcwork = nullptr; }
  if (hipMalloc(&st->pcwork, sizeof(double) * std::max(st->n, 1)) != hipSuccess) {
    (void)hipGetLastError(); st->pcwork = nullptr; ks_pc_amg_free(st->amg); st->amg = nullptr;
    KS_FAIL(KS_ERR_MEM, "AMG set-up: no device memory for a work vector of %d rows", st->n);
  }
  return KS_SUCCESS;
}

bool ks_st_is_plain(ks_st st) { return !st || (st->type == KS_ST_SHIFT && st->sigma == 0.0 && !st->B); }

int ks_st_setup_internal(ks_st st)
{
  KS_CHECK(st && st->A, KS_ERR_ORDER, "STSetMatrices must be called first");
  if (st->ready) return KS_SUCCESS;
  ks_ctx ctx = st->ctx; ks_mat A = st->A, B = st->B;
  KS_CHECK(!B || (B->n == A->n && B->n_global == A->n_global), KS_ERR_ARG_INCOMP, "Mismatching dimensions of A (%d) and B (%d)", A->n, B ? B->n : 0);
  KS_HIP(hipSetDevice(ctx->device));
  st->n = A->n;
  if (st->type == KS_ST_CAYLEY) {                                      // STComputeOperator_Cayley cayley.c:138-147
    if (!st->nu_set) st->nu = st->sigma;
    KS_CHECK(st->nu != 0.0 || st->sigma != 0.0, KS_ERR_USER_INPUT, "Values of shift and antishift cannot be zero simultaneously");
    KS_CHECK(st->nu != -st->sigma, KS_ERR_USER_INPUT, "It is not allowed to set the antishift equal to minus the shift (the target)");
  }
  if (st->Pmat) { ks_mat_destroy(st->Pmat); st->Pmat = nullptr; }           // the assembled P of an earlier shift / type / mode
  if (st->ilu) { ks_pc_ilu_free(st->ilu); st->ilu = nullptr; }              // and its ILU(0) blocks
  if (st->lu) { ks_pc_lu_free(st->lu); st->lu = nullptr; }                  // or its LU factors
  if (st->amg) { ks_pc_amg_free(st->amg); st->amg = nullptr; }              // or its multigrid hierarchy
  const bool need_solve = (st->type == KS_ST_SINVERT) || (st->type == KS_ST_CAYLEY) || (st->type == KS_ST_SHIFT && B);
  // STPRECOND (precond.c:36-110): K = A - sigma B is only preconditioned, the KSP is preonly - the preconditioner is built, no Krylov basis
  const bool precond = st->type == KS_ST_PRECOND;
  // the infinite default shift (precond.c:70-74: K = -B, or no K at all with one matrix): only a solver asks for it (GD, davidson.c:80), a shift the caller set wins
  const bool inf = precond && st->sigma_inf && !st->sigma_set;
  st->pc_on_b = inf && B; st->pc_identity = inf && !B;
  st->At = st->Bt = st->PmatT = nullptr;                                      // views: freed with the matrices they view
  if (need_solve && st->tsolves) {
    // the transposed side of P and of the operator's other factor (B^T, (A + nu B)^T): MatTranspose of the kept arrays, one rank
    KS_CHECK(ctx->comm.size == 1, KS_ERR_SUP, "transposed ST solves (ks_st_set_transpose_solves) run on one rank: the transpose of a row-sharded matrix is a redistribution");
    KS_CALL(ks_mat_create_transpose(A, &st->At));
    if (B) KS_CALL(ks_mat_create_transpose(B, &st->Bt));
  }
  if (st->W) { int wn = 0; ks_bv_get_sizes(st->W, &wn, nullptr, nullptr, nullptr); if (wn != A->n) { ks_bv_destroy(st->W); ks_bv_destroy(st->K); ks_bv_destroy(st->Kb); ks_bv_destroy(st->Kl); st->W = st->K = st->Kb = st->Kl = nullptr; if (st->dinv) hipFree(st->dinv); st->dinv = nullptr; } }
  if (!st->W) KS_CALL(ks_bv_create(ctx, A->n, A->n_global, 3, 0, &st->W));
  if (need_solve || precond) {
    if (st->K && !need_solve) { ks_bv_destroy(st->K); st->K = nullptr; }
    if (st->K) { int km = 0; ks_bv_get_sizes(st->K, nullptr, nullptr, &km, nullptr); if (km != st->restart + 1) { ks_bv_destroy(st->K); st->K = nullptr; } }
    const bool resident_sym = st->ksp_type == KS_KSP_CG || st->ksp_type == KS_KSP_MINRES;
    const bool short_rec = resident_sym || st->ksp_type == KS_KSP_BCGSL;
    if (st->K && (st->ksp_type == KS_KSP_PREONLY || short_rec)) { ks_bv_destroy(st->K); st->K = nullptr; }      // KSPPREONLY, KSPCG, KSPMINRES and KSPBCGSL keep no basis
    if (need_solve && !st->K && st->ksp_type != KS_KSP_PREONLY && !short_rec) { KS_CALL(ks_bv_create(ctx, A->n, A->n_global, st->restart + 1, 0, &st->K)); st->K->row_start = A->row_start; }
    if (need_solve && st->K) KS_CALL(ks_bv_set_orthogonalization(st->K, KS_BV_ORTHOG_CGS, st->gmres_refine, 0.7071));      // KSPGMRESClassicalGramSchmidtOrthogonalization + refinement type
    if (need_solve && st->ksp_type == KS_KSP_CG) KS_CALL(ks_resident_alloc(&st->cg));
    if (need_solve && st->ksp_type == KS_KSP_MINRES) KS_CALL(ks_resident_alloc(&st->mr));
    if (need_solve && st->ksp_type == KS_KSP_BCGSL) {                      // r_0..r_l, u_0..u_l, rt, one scratch column: 2 l + 4 columns, made anew when l changed
      KS_CALL(ks_resident_alloc(&st->bl, KS_BCGSL_HEAD_BYTES, KS_BCGSL_PART_COLS));
      const int cols = 2 * st->bcgsl_ell + 4;
      if (st->Kl) { int km = 0; ks_bv_get_sizes(st->Kl, nullptr, nullptr, &km, nullptr); if (km != cols) { ks_bv_destroy(st->Kl); st->Kl = nullptr; } }
      if (!st->Kl) { KS_CALL(ks_bv_create(ctx, A->n, A->n_global, cols, 0, &st->Kl)); st->Kl->row_start = A->row_start; }
    }
    if (need_solve && (st->ksp_type == KS_KSP_BCGS || resident_sym) && !st->Kb) { KS_CALL(ks_bv_create(ctx, A->n, A->n_global, 7, 0, &st->Kb)); st->Kb->row_start = A->row_start; }
    if (!st->dinv) KS_HIP(hipMalloc(&st->dinv, sizeof(double) * std::max(A->n, 1)));
    // Jacobi: diag(P)
    double *da = ks_bv_col(st->W, 1), *db = ks_bv_col(st->W, 2);
    const unsigned nb = (unsigned)std::max<long long>(1, std::min<long long>(((long long)A->n + 255) / 256, (long long)ctx->num_cu * 16));
    const int use_abs = st->jacobi_abs ? 1 : 0;
    if (st->matmode == KS_ST_MATMODE_COPY && (st->type == KS_ST_SINVERT || st->type == KS_ST_CAYLEY)) {
      // STMatMAXPY_Private, ST_MATMODE_COPY (stsolve.c:603-631): P = A - sigma B assembled (nmat = 1: MatShift); a zero shift takes A itself
      // there (:611-614) - here a copy of it, so that the ST owns what it destroys
      KS_CALL(ks_mat_create_axpy(A, -st->sigma, B, st->tsolves ? (unsigned)KS_MAT_KEEP_CSR : 0u, &st->Pmat));     // its transposed view needs its arrays
      if (st->tsolves) KS_CALL(ks_mat_create_transpose(st->Pmat, &st->PmatT));
      KS_CALL(ks_mat_get_diagonal_internal(st->Pmat, da));
      hipLaunchKernelGGL(k_jacobi_setup, dim3(nb), dim3(256), 0, ctx->stream, (long long)A->n, 1.0, da, 0.0, (const double *)nullptr, st->dinv, use_abs);
    } else if (st->type != KS_ST_SHIFT && !inf) {
      KS_CALL(ks_mat_get_diagonal_internal(A, da));
      if (B) KS_CALL(ks_mat_get_diagonal_internal(B, db));
      hipLaunchKernelGGL(k_jacobi_setup, dim3(nb), dim3(256), 0, ctx->stream, (long long)A->n, 1.0, da, -st->sigma, B ? db : nullptr, st->dinv, use_abs);
    } else if (B) {                                                    // shift with two matrices, or the infinite default shift: diag(B); one matrix there: nothing to build
      KS_CALL(ks_mat_get_diagonal_internal(B, db));
      hipLaunchKernelGGL(k_jacobi_setup, dim3(nb), dim3(256), 0, ctx->stream, (long long)A->n, 0.0, (const double *)nullptr, 1.0, db, st->dinv, use_abs);
    }
    KS_HIP(hipGetLastError());
    if (st->pc_type == KS_PC_BJACOBI && !st->pc_identity) KS_CALL(bjacobi_setup(st));
    if (st->pc_type == KS_PC_BJACOBI_ILU && !st->pc_identity) KS_CALL(bjacobi_ilu_setup(st));
    if (st->pc_type == KS_PC_LU && !st->pc_identity) KS_CALL(lu_setup(st));
    if (st->pc_type == KS_PC_AMG && !st->pc_identity) KS_CALL(amg_setup(st));
  }
  if (!st->op) KS_CALL(ks_mat_create_shell(ctx, A->n, A->row_start, A->n_global, st_shell_mult, st, &st->op));
  st->op->n = A->n; st->op->row_start = A->row_start; st->op->n_global = A->n_global;
  st->op->shell_mult_t = st_shell_mult_transpose;
  st->op->shell_nosync = !need_solve;                         // a plain shift is two kernel launches: Krylov runs stay enqueued ahead
  if (st->type == KS_ST_CAYLEY) {
    if (!st->bil) KS_CALL(ks_mat_create_shell(ctx, A->n, A->row_start, A->n_global, st_bilinear_mult, st, &st->bil));
    st->bil->n = A->n; st->bil->row_start = A->row_start; st->bil->n_global = A->n_global;
  }
  st->ready = true;
  return KS_SUCCESS;
}

int ks_st_apply_internal(ks_st st, const double *x, double *y)     // STApply_Generic stsolve.c:16-25
{
  if (!st->ready) KS_CALL(ks_st_setup_internal(st));
  double *w = ks_bv_col(st->W, 0), *t1 = ks_bv_col(st->W, 1);
  if (st->type == KS_ST_SINVERT) {
    if (st->B) { KS_CALL(ks_mat_mult_internal(st->B, x, w)); return inner_solve(st, w, y); }
    return inner_solve(st, x, y);
  }
  if (st->type == KS_ST_CAYLEY) {                                      // y = (A - sigma B)^-1 (A + nu B) x
    KS_CALL(linop_apply(st, 1.0, st->A, st->nu, st->B, !st->B, nullptr, x, w, t1));
    return inner_solve(st, w, y);
  }
  if (st->type == KS_ST_PRECOND) return pc_lincomb(st, 1.0, x, 0.0, nullptr, y);      // y = M^-1 x, KSPPREONLY (precond.c:93)
  // shift
  if (st->B) { KS_CALL(linop_apply(st, 1.0, st->A, -st->sigma, st->B, false, nullptr, x, w, t1)); return inner_solve(st, w, y); }
  return linop_apply(st, 1.0, st->A, -st->sigma, nullptr, st->sigma != 0.0, nullptr, x, y, t1);
}

void ks_st_backtransform_internal(ks_st st, int n, double *eigr, double *eigi) { if (st) ksd::StMap{st->type, st->sigma, st->nu}.backtransform(n, eigr, eigi); }

extern "C" int ks_st_create(ks_ctx ctx, ks_st *out)
{
  KS_CHECK(ctx && out, KS_ERR_ARG_NULL, "ctx/out is NULL");
  ks_st st = new ks_st_s(); st->ctx = ctx; *out = st;
  return KS_SUCCESS;
}
extern "C" int ks_st_destroy(ks_st st)
{
  if (!st) return KS_SUCCESS;
  ks_bv_destroy(st->K); ks_bv_destroy(st->W); ks_bv_destroy(st->Kb); ks_bv_destroy(st->Kl);
  if (st->dinv) hipFree(st->dinv);
  if (st->op) ks_mat_destroy(st->op);
  if (st->bil) ks_mat_destroy(st->bil);
  if (st->Pmat) ks_mat_destroy(st->Pmat);
  if (st->binv) hipFree(st->binv);
  if (st->pcwork) hipFree(st->pcwork);
  ks_resident_free(&st->cg);
  ks_resident_free(&st->mr);
  ks_resident_free(&st->bl);
  ks_pc_ilu_free(st->ilu);
  ks_pc_lu_free(st->lu);
  ks_pc_amg_free(st->amg);
  delete st;
  return KS_SUCCESS;
}
extern "C" int ks_st_set_type(ks_st st, int type)                    // STSetType
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  KS_CHECK(type == KS_ST_SHIFT || type == KS_ST_SINVERT || type == KS_ST_CAYLEY || type == KS_ST_PRECOND, KS_ERR_SUP, "only STSHIFT, STSINVERT, STCAYLEY and STPRECOND are built");
  if (st->type != type) { st->type = type; st->ready = false; }
  st->type_set = true;
  return KS_SUCCESS;
}
extern "C" int ks_st_set_shift(ks_st st, double sigma)               // STSetShift stfunc.c
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  if (st->sigma != sigma || !st->sigma_set) { st->sigma = sigma; st->ready = false; }
  st->sigma_set = true;
  return KS_SUCCESS;
}
extern "C" int ks_st_cayley_set_antishift(ks_st st, double nu)       // STCayleySetAntishift cayley.c:236
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  if (st->nu != nu || !st->nu_set) { st->nu = nu; st->ready = false; }
  st->nu_set = true;
  return KS_SUCCESS;
}
extern "C" int ks_st_cayley_get_antishift(ks_st st, double *nu) { KS_CHECK(st && nu, KS_ERR_ARG_NULL, "NULL argument"); *nu = st->nu; return KS_SUCCESS; }
extern "C" int ks_st_get_shift(ks_st st, double *sigma) { KS_CHECK(st && sigma, KS_ERR_ARG_NULL, "NULL argument"); *sigma = st->sigma; return KS_SUCCESS; }
extern "C" int ks_st_set_matrices(ks_st st, ks_mat A, ks_mat B)      // STSetMatrices (n = 1 or 2)
{
  KS_CHECK(st && A, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(!A->shell_mult && (!B || !B->shell_mult), KS_ERR_SUP, "ST needs assembled matrices (their diagonals feed the Jacobi preconditioner)");
  st->A = A; st->B = B; st->ready = false;
  return KS_SUCCESS;
}
extern "C" int ks_st_set_matmode(ks_st st, int mode)                 // STSetMatMode
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  KS_CHECK(mode == KS_ST_MATMODE_COPY || mode == KS_ST_MATMODE_SHELL, KS_ERR_SUP, "only ST_MATMODE_COPY and ST_MATMODE_SHELL are built");
  if (st->matmode != mode) { st->matmode = mode; st->ready = false; }
  return KS_SUCCESS;
}
extern "C" int ks_st_get_matmode(ks_st st, int *mode) { KS_CHECK(st && mode, KS_ERR_ARG_NULL, "NULL argument"); *mode = st->matmode; return KS_SUCCESS; }
extern "C" int ks_st_set_ksp(ks_st st, double rtol, int max_it, int restart)   // KSPSetTolerances / KSPGMRESSetRestart on STGetKSP
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  if (rtol > 0.0) { st->rtol = rtol; st->rtol_set = true; }
  if (max_it > 0) { st->max_it = max_it; st->max_it_set = true; }
  if (restart > 0 && restart != st->restart) { st->restart = restart; st->ready = false; }   // a basis wider than 64 columns orthogonalises through the host-driven loop
  return KS_SUCCESS;
}
extern "C" int ks_st_set_ksp_type(ks_st st, int type)              // KSPSetType on STGetKSP: KSPGMRES (default), KSPBCGS, KSPPREONLY, KSPCG, KSPMINRES or KSPBCGSL
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  KS_CHECK(type == KS_KSP_GMRES || type == KS_KSP_BCGS || type == KS_KSP_PREONLY || type == KS_KSP_CG || type == KS_KSP_MINRES || type == KS_KSP_BCGSL, KS_ERR_SUP,
           "only KSPGMRES, KSPBCGS, KSPPREONLY, KSPCG, KSPMINRES and KSPBCGSL are built");
  if (st->ksp_type != type) { st->ksp_type = type; st->ready = false; }
  st->ksp_type_set = true;
  return KS_SUCCESS;
}
// the check interval and the statistics of the device-resident solvers: which: the ST's cg, mr or bl
static int resident_set_check(ks_st st, KsResident ks_st_s::*which, int c)
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  KS_CHECK(c >= 1 && c <= 1024, KS_ERR_ARG_OUTOFRANGE, "check interval %d (1..1024)", c);
  (st->*which).check = c;
  return KS_SUCCESS;
}
static int resident_get_check(ks_st st, KsResident ks_st_s::*which, int *c) { KS_CHECK(st && c, KS_ERR_ARG_NULL, "NULL argument"); *c = (st->*which).check; return KS_SUCCESS; }
static int resident_get_stats(ks_st st, KsResident ks_st_s::*which, long long *sweeps, long long *host_waits, long long *gated_iterations)
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  const KsResident &r = st->*which;
  if (sweeps) *sweeps = r.sweeps; if (host_waits) *host_waits = r.waits; if (gated_iterations) *gated_iterations = r.gated;
  return KS_SUCCESS;
}
extern "C" int ks_st_cg_set_check_interval(ks_st st, int c) { return resident_set_check(st, &ks_st_s::cg, c); }
extern "C" int ks_st_cg_get_check_interval(ks_st st, int *c) { return resident_get_check(st, &ks_st_s::cg, c); }
extern "C" int ks_st_cg_get_stats(ks_st st, long long *sweeps, long long *waits, long long *gated) { return resident_get_stats(st, &ks_st_s::cg, sweeps, waits, gated); }
extern "C" int ks_st_minres_set_check_interval(ks_st st, int c) { return resident_set_check(st, &ks_st_s::mr, c); }
extern "C" int ks_st_minres_get_check_interval(ks_st st, int *c) { return resident_get_check(st, &ks_st_s::mr, c); }
extern "C" int ks_st_minres_get_stats(ks_st st, long long *sweeps, long long *waits, long long *gated) { return resident_get_stats(st, &ks_st_s::mr, sweeps, waits, gated); }
extern "C" int ks_st_bcgsl_set_check_interval(ks_st st, int c) { return resident_set_check(st, &ks_st_s::bl, c); }
extern "C" int ks_st_bcgsl_get_check_interval(ks_st st, int *c) { return resident_get_check(st, &ks_st_s::bl, c); }
extern "C" int ks_st_bcgsl_get_stats(ks_st st, long long *sweeps, long long *waits, long long *gated) { return resident_get_stats(st, &ks_st_s::bl, sweeps, waits, gated); }
extern "C" int ks_st_bcgsl_set_ell(ks_st st, int ell)                 // KSPBCGSLSetEll on STGetKSP; the work vectors depend on it: the set-up is cleared
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  KS_CHECK(ell >= 1 && ell <= KS_BCGSL_MAX_ELL, KS_ERR_ARG_OUTOFRANGE, "BiCGStab(l): l = %d (1..%d)", ell, KS_BCGSL_MAX_ELL);
  st->bcgsl_ell = ell; st->ready = false;
  return KS_SUCCESS;
}
extern "C" int ks_st_bcgsl_get_ell(ks_st st, int *ell) { KS_CHECK(st && ell, KS_ERR_ARG_NULL, "NULL argument"); *ell = st->bcgsl_ell; return KS_SUCCESS; }
extern "C" int ks_st_pc_jacobi_set_use_abs(ks_st st, int flag)        // PCJacobiSetUseAbs on the KSP's PC; the diagonal is rebuilt at the next set-up
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  st->jacobi_abs = flag != 0; st->ready = false;
  return KS_SUCCESS;
}
extern "C" int ks_st_pc_jacobi_get_use_abs(ks_st st, int *flag) { KS_CHECK(st && flag, KS_ERR_ARG_NULL, "NULL argument"); *flag = st->jacobi_abs ? 1 : 0; return KS_SUCCESS; }
extern "C" int ks_st_set_pc(ks_st st, int type, int block_size)      // PCSetType (+ PCBJacobiSetLocalBlocks, -sub_pc_type lu | ilu) on the KSP's PC
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  KS_CHECK(type == KS_PC_JACOBI || type == KS_PC_BJACOBI || type == KS_PC_BJACOBI_ILU || type == KS_PC_NONE || type == KS_PC_LU || type == KS_PC_AMG, KS_ERR_SUP, "only PCNONE, PCJACOBI, PCBJACOBI (sub-solves: LU on dense blocks, or ILU(0)), PCLU and PCGAMG are built");
  KS_CHECK(type != KS_PC_AMG || block_size == 0, KS_ERR_SUP, "PCGAMG works on the whole matrix: a block size (%d) with it names no preconditioner this build has", block_size);
  KS_CHECK(type != KS_PC_LU || block_size == 0, KS_ERR_SUP, "PCLU factors the whole matrix: a block size (%d) with it names no preconditioner this build has", block_size);
  KS_CHECK(type != KS_PC_NONE || block_size == 0, KS_ERR_SUP, "PCNONE has no blocks: a block size (%d) with it names no preconditioner this build has", block_size);
  KS_CHECK(type != KS_PC_BJACOBI || (block_size >= 2 && block_size <= 32), KS_ERR_ARG_OUTOFRANGE, "block size %d (2..32)", block_size);
  KS_CHECK(type != KS_PC_BJACOBI_ILU || (block_size >= 64 && block_size <= ksc::ILU_BS_MAX), KS_ERR_ARG_OUTOFRANGE, "block size %d (64..%d)", block_size, ksc::ILU_BS_MAX);
  if (type == KS_PC_JACOBI || type == KS_PC_NONE) block_size = 0;
  if (st->pc_type != type || st->pc_bs != block_size) { st->pc_type = type; st->pc_bs = block_size; st->ready = false; }
  return KS_SUCCESS;
}
extern "C" int ks_st_pc_lu_set_ordering(ks_st st, int which)          // PCFactorSetMatOrderingType on the PCLU
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  KS_CHECK(which == KS_ORDERING_ND || which == KS_ORDERING_NATURAL, KS_ERR_ARG_OUTOFRANGE, "unknown ordering %d (KS_ORDERING_ND, KS_ORDERING_NATURAL)", which);
  if (st->lu_ordering != which) { st->lu_ordering = which; st->ready = false; }
  return KS_SUCCESS;
}
extern "C" int ks_st_pc_lu_get_ordering_type(ks_st st, int *which) { KS_CHECK(st && which, KS_ERR_ARG_NULL, "NULL argument"); *which = st->lu_ordering; return KS_SUCCESS; }
// the set-up behind the three queries of the factors
static int lu_query(ks_st st, KsLuInfo *info)
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  KS_CHECK(st->A, KS_ERR_ORDER, "STSetMatrices must be called first");
  KS_CHECK(st->pc_type == KS_PC_LU, KS_ERR_ORDER, "the preconditioner is not KS_PC_LU");
  KS_HIP(hipSetDevice(st->ctx->device));
  if (!st->ready) KS_CALL(ks_st_setup_internal(st));
  KS_CHECK(st->lu, KS_ERR_ORDER, "this transformation has no linear solve, so no factors (STSHIFT with one matrix, or STPRECOND without a matrix to precondition)");
  ks_pc_lu_info(st->lu, info);
  return KS_SUCCESS;
}
extern "C" int ks_st_pc_lu_get_permutation(ks_st st, int *perm_host)
{
  KS_CHECK(perm_host, KS_ERR_ARG_NULL, "NULL argument");
  KsLuInfo i; KS_CALL(lu_query(st, &i));
  std::copy(i.perm, i.perm + i.n, perm_host);
  return KS_SUCCESS;
}
extern "C" int ks_st_pc_lu_get_info(ks_st st, int *n, long long *nnz_l, long long *nnz_u, int *levels_l, int *levels_u, int *wide, int *wide_launches, int *narrow_launches, long long *device_bytes)
{
  KsLuInfo i; KS_CALL(lu_query(st, &i));
  if (n) *n = i.n; if (nnz_l) *nnz_l = i.nnzL; if (nnz_u) *nnz_u = i.nnzU; if (levels_l) *levels_l = i.levelsL; if (levels_u) *levels_u = i.levelsU;
  if (wide) *wide = i.wide; if (wide_launches) *wide_launches = i.wide_launches; if (narrow_launches) *narrow_launches = i.narrow_launches;
  if (device_bytes) *device_bytes = i.bytes + (long long)sizeof(double) * std::max(i.n, 1);      // the ST's own work vector with it
  return KS_SUCCESS;
}
extern "C" int ks_st_pc_lu_get_inertia(ks_st st, int *neg, int *zero, int *pos)      // MatGetInertia on the factor
{
  KsLuInfo i; KS_CALL(lu_query(st, &i));
  if (neg) *neg = i.neg; if (zero) *zero = 0; if (pos) *pos = i.pos;
  return KS_SUCCESS;
}
// KS_PC_AMG: its options (each clears the set-up) and the two queries of the hierarchy
extern "C" int ks_st_pc_amg_set_threshold(ks_st st, double theta)           // -pc_gamg_threshold
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  KS_CHECK(theta >= 0.0 && theta < 1.0, KS_ERR_ARG_OUTOFRANGE, "strength threshold %g (0 <= theta < 1)", theta);
  if (st->amg_opt.theta != theta) { st->amg_opt.theta = theta; st->ready = false; }
  return KS_SUCCESS;
}
extern "C" int ks_st_pc_amg_get_threshold(ks_st st, double *theta) { KS_CHECK(st && theta, KS_ERR_ARG_NULL, "NULL argument"); *theta = st->amg_opt.theta; return KS_SUCCESS; }
extern "C" int ks_st_pc_amg_set_smoother(ks_st st, int degree)
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  KS_CHECK(degree >= 1 && degree <= 4, KS_ERR_ARG_OUTOFRANGE, "Chebyshev degree %d (1..4)", degree);
  if (st->amg_opt.degree != degree) { st->amg_opt.degree = degree; st->ready = false; }
  return KS_SUCCESS;
}
extern "C" int ks_st_pc_amg_get_smoother(ks_st st, int *degree) { KS_CHECK(st && degree, KS_ERR_ARG_NULL, "NULL argument"); *degree = st->amg_opt.degree; return KS_SUCCESS; }
extern "C" int ks_st_pc_amg_set_coarse(ks_st st, int coarse_limit, int max_levels)
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  KS_CHECK(coarse_limit >= 1, KS_ERR_ARG_OUTOFRANGE, "coarse limit %d (at least 1 row)", coarse_limit);
  KS_CHECK(max_levels >= 1 && max_levels <= KS_AMG_MAX_LEVELS, KS_ERR_ARG_OUTOFRANGE, "levels %d (1..%d)", max_levels, KS_AMG_MAX_LEVELS);
  if (st->amg_opt.coarse_limit != coarse_limit || st->amg_opt.max_levels != max_levels) { st->amg_opt.coarse_limit = coarse_limit; st->amg_opt.max_levels = max_levels; st->ready = false; }
  return KS_SUCCESS;
}
extern "C" int ks_st_pc_amg_get_coarse(ks_st st, int *coarse_limit, int *max_levels)
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  if (coarse_limit) *coarse_limit = st->amg_opt.coarse_limit; if (max_levels) *max_levels = st->amg_opt.max_levels;
  return KS_SUCCESS;
}
extern "C" int ks_st_pc_amg_set_prolongator_smoothing(ks_st st, int on)
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  if (st->amg_opt.smooth != (on != 0)) { st->amg_opt.smooth = on != 0; st->ready = false; }
  return KS_SUCCESS;
}
extern "C" int ks_st_pc_amg_get_prolongator_smoothing(ks_st st, int *on) { KS_CHECK(st && on, KS_ERR_ARG_NULL, "NULL argument"); *on = st->amg_opt.smooth ? 1 : 0; return KS_SUCCESS; }
static int amg_query(ks_st st)
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  KS_CHECK(st->A, KS_ERR_ORDER, "STSetMatrices must be called first");
  KS_CHECK(st->pc_type == KS_PC_AMG, KS_ERR_ORDER, "the preconditioner is not KS_PC_AMG");
  KS_HIP(hipSetDevice(st->ctx->device));
  if (!st->ready) KS_CALL(ks_st_setup_internal(st));
  KS_CHECK(st->amg, KS_ERR_ORDER, "this transformation has no linear solve, so no hierarchy (STSHIFT with one matrix, or STPRECOND without a matrix to precondition)");
  return KS_SUCCESS;
}
extern "C" int ks_st_pc_amg_get_info(ks_st st, int *levels, int *rows, long long *nnz, double *rho, double *complexity, long long *device_bytes, int *launches)
{
  KS_CALL(amg_query(st));
  KsAmgInfo i; ks_pc_amg_info(st->amg, &i);
  if (levels) *levels = i.levels;
  for (int l = 0; l < KS_AMG_MAX_LEVELS; l++) { if (rows) rows[l] = i.rows[l]; if (nnz) nnz[l] = i.nnz[l]; if (rho) rho[l] = i.rho[l]; }
  if (complexity) *complexity = i.complexity; if (launches) *launches = i.launches;
  if (device_bytes) *device_bytes = i.bytes + (long long)sizeof(double) * std::max(st->n, 1);      // the ST's own work vector with it
  return KS_SUCCESS;
}
extern "C" int ks_st_pc_amg_get_level(ks_st st, int level, int *n, int *n_coarse, long long *nnz_a, long long *nnz_p, int *arp, int *acol, double *aval,
                                      int *prp, int *pcol, double *pval, int *agg)
{
  KS_CALL(amg_query(st));
  int nl = 0, nc = 0; const int *hrp, *hcol, *hprp, *hpcol, *hagg; const double *hval, *hpval;
  KS_CALL(ks_pc_amg_level(st->amg, level, &nl, &nc, &hrp, &hcol, &hval, &hprp, &hpcol, &hpval, &hagg));
  const long long za = hrp[nl], zp = hprp ? hprp[nl] : 0;
  if (n) *n = nl; if (n_coarse) *n_coarse = nc; if (nnz_a) *nnz_a = za; if (nnz_p) *nnz_p = zp;
  if (arp && acol && aval) { std::copy(hrp, hrp + nl + 1, arp); std::copy(hcol, hcol + za, acol); std::copy(hval, hval + za, aval); }
  if (prp && pcol && pval) { if (hprp) { std::copy(hprp, hprp + nl + 1, prp); std::copy(hpcol, hpcol + zp, pcol); std::copy(hpval, hpval + zp, pval); } else std::fill(prp, prp + nl + 1, 0); }
  if (agg) { if (hagg) std::copy(hagg, hagg + nl, agg); else std::fill(agg, agg + nl, -1); }
  return KS_SUCCESS;
}
extern "C" int ks_st_set_gmres_cgs_refinement(ks_st st, int refine)   // KSPGMRESSetCGSRefinementType on STGetKSP
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  KS_CHECK(refine == KS_BV_ORTHOG_REFINE_NEVER || refine == KS_BV_ORTHOG_REFINE_IFNEEDED || refine == KS_BV_ORTHOG_REFINE_ALWAYS, KS_ERR_ARG_OUTOFRANGE, "unknown refinement type %d", refine);
  if (st->gmres_refine != refine) { st->gmres_refine = refine; st->ready = false; }
  return KS_SUCCESS;
}
extern "C" int ks_st_setup(ks_st st) { KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL"); return ks_st_setup_internal(st); }
extern "C" int ks_st_apply(ks_st st, const double *x_dev, double *y_dev)        // STApply stsolve.c:44
{
  KS_CHECK(st && x_dev && y_dev, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(x_dev != y_dev, KS_ERR_ARG_IDN, "x and y must be different vectors");
  KS_CHECK(st->A, KS_ERR_ORDER, "STSetMatrices must be called first");
  KS_HIP(hipSetDevice(st->ctx->device));
  return ks_st_apply_internal(st, x_dev, y_dev);
}
extern "C" int ks_st_pc_apply(ks_st st, const double *x_dev, double *y_dev)     // PCApply on KSPGetPC(STGetKSP)
{
  KS_CHECK(st && x_dev && y_dev, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(x_dev != y_dev, KS_ERR_ARG_IDN, "x and y must be different vectors");
  KS_CHECK(st->A, KS_ERR_ORDER, "STSetMatrices must be called first");
  KS_HIP(hipSetDevice(st->ctx->device));
  if (!st->ready) KS_CALL(ks_st_setup_internal(st));
  KS_CHECK(st->type != KS_ST_SHIFT || st->B, KS_ERR_ORDER, "this transformation has no linear solve, so no preconditioner (STSHIFT with one matrix)");
  if (pc_none(st)) return ksk_copy(st->ctx, x_dev, y_dev, st->n);
  if (st->pc_type == KS_PC_JACOBI) return lincomb(st->ctx, st->n, st->dinv, 1.0, x_dev, 0.0, nullptr, y_dev);
  return blocks_apply(st, x_dev, y_dev);
}
// the argument checks a block entry shares with ks_mat_mult_multi; *empty: nothing to do
static int block_entry(ks_st st, int ncols, const double *X_dev, int ldx, double *Y_dev, int ldy, bool *empty)
{
  KS_CHECK(st && X_dev && Y_dev, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(st->A, KS_ERR_ORDER, "STSetMatrices must be called first");
  KS_CHECK(ncols >= 0, KS_ERR_ARG_OUTOFRANGE, "Number of columns %d must be non-negative", ncols);
  const int n = st->A->n;
  KS_CHECK(ldx >= std::max(1, n) && ldy >= std::max(1, n), KS_ERR_ARG_SIZ, "Leading dimensions ldx %d, ldy %d must be at least %d (local rows)", ldx, ldy, std::max(1, n));
  *empty = ncols == 0;
  if (*empty) return KS_SUCCESS;
  const uintptr_t x0 = (uintptr_t)X_dev, x1 = x0 + sizeof(double) * ((size_t)(ncols - 1) * ldx + n);
  const uintptr_t y0 = (uintptr_t)Y_dev, y1 = y0 + sizeof(double) * ((size_t)(ncols - 1) * ldy + n);
  KS_CHECK(X_dev != Y_dev && (x1 <= y0 || y1 <= x0), KS_ERR_ARG_WRONG, "X and Y must be different blocks: they overlap");
  KS_HIP(hipSetDevice(st->ctx->device));
  if (!st->ready) KS_CALL(ks_st_setup_internal(st));
  return KS_SUCCESS;
}
// PCMatApply on KSPGetPC(STGetKSP): Y(:,j) = M^-1 X(:,j). The pointwise preconditioners and the dense blocks are their single-vector kernels with the
// column on the grid's second dimension; the ILU(0) blocks keep several columns of a block in LDS at once (ks_pc.hip). One column IS ks_st_pc_apply.
int ks_st_pc_apply_multi_internal(ks_st st, int ncols, const double *X, int ldx, double *Y, int ldy)
{
  if (ncols <= 0 || st->n == 0) return KS_SUCCESS;
  if (st->pc_type == KS_PC_BJACOBI_ILU && !st->pc_identity) return ks_pc_ilu_apply_multi(st->ctx, st->ilu, ncols, X, ldx, Y, ldy);
  if (st->pc_type == KS_PC_LU && !st->pc_identity) return ks_pc_lu_apply_multi(st->ctx, st->lu, ncols, X, ldx, Y, ldy);
  if (st->pc_type == KS_PC_AMG && !st->pc_identity) return ks_pc_amg_apply_multi(st->ctx, st->amg, ncols, X, ldx, Y, ldy);
  const unsigned nb = (unsigned)std::min<long long>(((long long)st->n + 255) / 256, (long long)st->ctx->num_cu * 16);
  if (st->pc_type == KS_PC_BJACOBI && !st->pc_identity) hipLaunchKernelGGL(k_bjacobi_apply, dim3(nb, (unsigned)ncols), dim3(256), 0, st->ctx->stream, (long long)st->n, st->pc_bs, st->binv, X, (long long)ldx, Y, (long long)ldy);
  else hipLaunchKernelGGL(k_diag_apply_multi, dim3(nb, (unsigned)ncols), dim3(256), 0, st->ctx->stream, (long long)st->n, pc_none(st) ? (const double *)nullptr : st->dinv, X, (long long)ldx, Y, (long long)ldy);
  KS_HIP(hipGetLastError());
  return KS_SUCCESS;
}
bool ks_st_pc_pointwise(ks_st st, const double **dinv)
{
  *dinv = (!pc_none(st) && st->pc_type == KS_PC_JACOBI) ? st->dinv : nullptr;
  return pc_none(st) || st->pc_type == KS_PC_JACOBI;
}
extern "C" int ks_st_pc_apply_multi(ks_st st, int ncols, const double *X_dev, int ldx, double *Y_dev, int ldy)
{
  bool empty = false;
  KS_CALL(block_entry(st, ncols, X_dev, ldx, Y_dev, ldy, &empty));
  if (empty) return KS_SUCCESS;
  KS_CHECK(st->type != KS_ST_SHIFT || st->B, KS_ERR_ORDER, "this transformation has no linear solve, so no preconditioner (STSHIFT with one matrix)");
  return ks_st_pc_apply_multi_internal(st, ncols, X_dev, ldx, Y_dev, ldy);
}
extern "C" int ks_st_pc_multi_columns(ks_st st, int *columns)      // instrumentation: columns ks_st_pc_apply_multi handles per pass with the PC that is set up
{
  KS_CHECK(st && columns, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(st->A, KS_ERR_ORDER, "STSetMatrices must be called first");
  KS_HIP(hipSetDevice(st->ctx->device));
  if (!st->ready) KS_CALL(ks_st_setup_internal(st));
  if (st->pc_type == KS_PC_LU && st->lu) { *columns = ks_pc_lu_multi_columns(); return KS_SUCCESS; }
  if (st->pc_type == KS_PC_AMG && st->amg) { *columns = ks_pc_amg_multi_columns(); return KS_SUCCESS; }
  *columns = (st->pc_type == KS_PC_BJACOBI_ILU && st->ilu) ? std::max(1, ks_pc_ilu_multi_columns(st->ctx, st->ilu)) : 65535;      // the other types take the whole block in one launch (grid.y)
  return KS_SUCCESS;
}
// STApplyMat (stsolve.c:62-80): Y = Op X for a block of vectors. STPRECOND applies its preconditioner to the block; the transformations with a
// Krylov solve inside go column by column through STApply
extern "C" int ks_st_apply_mat(ks_st st, int ncols, const double *X_dev, int ldx, double *Y_dev, int ldy)
{
  bool empty = false;
  KS_CALL(block_entry(st, ncols, X_dev, ldx, Y_dev, ldy, &empty));
  if (empty) return KS_SUCCESS;
  if (st->type == KS_ST_PRECOND) return ks_st_pc_apply_multi_internal(st, ncols, X_dev, ldx, Y_dev, ldy);
  for (int j = 0; j < ncols; j++) KS_CALL(ks_st_apply_internal(st, X_dev + (size_t)j * ldx, Y_dev + (size_t)j * ldy));
  return KS_SUCCESS;
}
extern "C" int ks_st_set_transpose_solves(ks_st st, int enable)
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  if (st->tsolves != (enable != 0)) { st->tsolves = enable != 0; st->ready = false; }
  return KS_SUCCESS;
}
extern "C" int ks_st_get_transpose_solves(ks_st st, int *enable) { KS_CHECK(st && enable, KS_ERR_ARG_NULL, "NULL argument"); *enable = st->tsolves ? 1 : 0; return KS_SUCCESS; }
// the checks the two transposed entries share; `what` names the caller
static int transpose_entry(ks_st st, const double *x_dev, double *y_dev, const char *what)
{
  KS_CHECK(st && x_dev && y_dev, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(x_dev != y_dev, KS_ERR_ARG_IDN, "x and y must be different vectors");
  KS_CHECK(st->A, KS_ERR_ORDER, "STSetMatrices must be called first");
  KS_CHECK(st->type != KS_ST_SHIFT || st->B, KS_ERR_ORDER, "this transformation has no linear solve, so no %s (STSHIFT with one matrix)", what);
  KS_CHECK(st->tsolves, KS_ERR_SUP, "%s needs the transposed side of the solves: ks_st_set_transpose_solves(st, 1) before the set-up", what);
  KS_HIP(hipSetDevice(st->ctx->device));
  if (!st->ready) KS_CALL(ks_st_setup_internal(st));
  return KS_SUCCESS;
}
extern "C" int ks_st_matsolve_transpose(ks_st st, const double *b_dev, double *y_dev)      // STMatSolveTranspose stsolve.c (KSPSolveTranspose on STGetKSP)
{
  KS_CALL(transpose_entry(st, b_dev, y_dev, "STMatSolveTranspose"));
  return inner_solve(st, b_dev, y_dev, true);
}
extern "C" int ks_st_pc_apply_transpose(ks_st st, const double *x_dev, double *y_dev)      // PCApplyTranspose on KSPGetPC(STGetKSP)
{
  KS_CALL(transpose_entry(st, x_dev, y_dev, "PCApplyTranspose"));
  if (st->pc_type == KS_PC_JACOBI) return lincomb(st->ctx, st->n, st->dinv, 1.0, x_dev, 0.0, nullptr, y_dev);
  return blocks_apply(st, x_dev, y_dev, true);
}
// STApplyTranspose_Generic (stsolve.c:107-116; the Hermitian form :153-162 with real scalars): y = M^T P^-T x. The branch without a solve (st->M alone:
// shift with one matrix) always; the ones with a solve when the ST prepares transposed solves (ks_st_set_transpose_solves)
int ks_st_apply_transpose_internal(ks_st st, const double *x, double *y)
{
  KS_CALL(ks_st_setup_internal(st));
  KS_CHECK((st->type == KS_ST_SHIFT && !st->B) || st->tsolves, KS_ERR_SUP, "STApplyHermitianTranspose is built for STSHIFT with one matrix (the others need a solve with the transposed matrix: ks_st_set_transpose_solves)");
  if (st->type != KS_ST_SHIFT || st->B) {
    double *w = ks_bv_col(st->W, 0), *t1 = ks_bv_col(st->W, 1);
    if (st->type == KS_ST_SINVERT && !st->B) return inner_solve(st, x, y, true);                       // y = P^-T x
    KS_CALL(inner_solve(st, x, w, true));                                                              // w = P^-T x
    if (st->type == KS_ST_SINVERT) return ks_mat_mult_internal(st->Bt, w, y);                          // y = B^T w
    if (st->type == KS_ST_CAYLEY) return linop_apply(st, 1.0, st->At, st->nu, st->Bt, !st->Bt, nullptr, w, y, t1);      // y = (A + nu B)^T w
    return linop_apply(st, 1.0, st->At, -st->sigma, st->Bt, false, nullptr, w, y, t1);                 // shift, two matrices: P = B, y = (A - sigma B)^T w
  }
  KS_CALL(ks_mat_mult_transpose_internal(st->A, x, y));
  if (st->sigma != 0.0) KS_CALL(ksk_lincomb(st->ctx, st->n, nullptr, 1.0, y, -st->sigma, x, y));      // (A - sigma I)^T x
  return KS_SUCCESS;
}
extern "C" int ks_st_apply_transpose(ks_st st, const double *x_dev, double *y_dev)
{
  KS_CHECK(st && x_dev && y_dev, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(x_dev != y_dev, KS_ERR_ARG_IDN, "x and y must be different vectors");
  KS_CHECK(st->A, KS_ERR_ORDER, "STSetMatrices must be called first");
  KS_HIP(hipSetDevice(st->ctx->device));
  return ks_st_apply_transpose_internal(st, x_dev, y_dev);
}
extern "C" int ks_st_backtransform(ks_st st, int n, double *eigr, double *eigi) // STBackTransform stsolve.c:563
{
  KS_CHECK(st && (n == 0 || (eigr && eigi)), KS_ERR_ARG_NULL, "NULL argument");
  ks_st_backtransform_internal(st, n, eigr, eigi);
  return KS_SUCCESS;
}
extern "C" int ks_st_get_ksp_stats(ks_st st, long long *solves, long long *iterations, double *last_rnorm)
{
  KS_CHECK(st, KS_ERR_ARG_NULL, "ST is NULL");
  if (solves) *solves = st->solves; if (iterations) *iterations = st->its; if (last_rnorm) *last_rnorm = st->last_rnorm;
  return KS_SUCCESS;
}
