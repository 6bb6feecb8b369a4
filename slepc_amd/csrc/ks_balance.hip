// Balancing of non-symmetric problems (EPSSetBalance): the diagonal D of EPSBuildBalance_Krylov (epsdefault.c:370-434) and the balanced operator
// D Op D^-1 the expansion then runs on (epssetup.c:383-391, STApply with st->D). The only device code of the EPS driver: five element-wise kernels.
#include "ksgpu_internal.h"
#include "ks_eps_impl.h"
#include <algorithm>

namespace {
__global__ void k_pw(long long n, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ out, int mul)
{
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = mul ? a[i] * b[i] : a[i] / b[i];
}
__global__ void k_sign_half(long long n, double *__restrict__ z)
{
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) z[i] = z[i] < 0.5 ? -1.0 : 1.0;
}
__global__ void k_bal_update(long long n, double *__restrict__ D, const double *__restrict__ p)
{
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) if (p[i] != 0.0) D[i] /= fabs(p[i]);
}
// two-sided form (epsdefault.c:419-421): D_i *= sqrt(|r_i / p_i|) where |p_i| > cutoff * norma and r_i != 0
__global__ void k_bal_update2(long long n, double *__restrict__ D, const double *__restrict__ p, const double *__restrict__ r, double thr)
{
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    if (fabs(p[i]) > thr && r[i] != 0.0) D[i] *= sqrt(fabs(r[i] / p[i]));
}
__global__ void k_fill(long long n, double *__restrict__ x, double v)
{
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) x[i] = v;
}
}
int ks_eps_pointwise(ks_eps eps, const double *a, const double *b, double *out, bool mul)     // VecPointwiseMult / VecPointwiseDivide
{
  const long long n = eps->V->n;
  if (!n) return KS_SUCCESS;
  const unsigned nb = (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, (long long)eps->ctx->num_cu * 16));
  hipLaunchKernelGGL(k_pw, dim3(nb), dim3(256), 0, eps->ctx->stream, n, a, b, out, mul ? 1 : 0);
  KS_HIP(hipGetLastError());
  return KS_SUCCESS;
}
// the balanced operator D Op D^-1 as a matrix-free operator (STApply with st->D, stsolve.c:252-256)
static int balanced_mult(void *user, const double *x, double *y)
{
  ks_eps eps = (ks_eps)user;
  KS_CALL(ks_eps_pointwise(eps, x, eps->D, eps->wb, false));
  KS_CALL(ks_mat_mult_internal(eps->op_inner, eps->wb, y));
  return ks_eps_pointwise(eps, y, eps->D, y, true);
}
// EPSBuildBalance_Krylov epsdefault.c:370-434 over balance_its random +-1 vectors z. One-sided: D <- D ./ |p|, p = D Op D^-1 z. Two-sided: also
// r = D^-1 Op^T D z (STApplyHermitianTranspose: ks_mat_mult_transpose on the operator), D_i *= sqrt(|r_i / p_i|) where |p_i| exceeds cutoff times the
// infinity norm of the first p
static int build_balance(ks_eps eps)
{
  ks_ctx ctx = eps->ctx; const long long n = eps->V->n;
  const unsigned nb = (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, (long long)ctx->num_cu * 16));
  if (eps->D_n != n) { if (eps->D) hipFree(eps->D); if (eps->wb) hipFree(eps->wb); eps->D = eps->wb = nullptr;
    KS_HIP(hipMalloc(&eps->D, sizeof(double) * std::max<long long>(n, 1))); KS_HIP(hipMalloc(&eps->wb, sizeof(double) * std::max<long long>(n, 1))); eps->D_n = (int)n; }
  if (n) hipLaunchKernelGGL(k_fill, dim3(nb), dim3(256), 0, ctx->stream, n, eps->D, 1.0);
  double *z = ks_bv_col(eps->W, 3), *p = ks_bv_col(eps->W, 4);
  eps->W->row_start = eps->V->row_start;
  double norma = 0.0;
  for (int j = 0; j < eps->balance_its; j++) {
    KS_CALL(ks_bv_set_random_column(eps->W, 3, eps->seed + 7919ULL * (uint64_t)(j + 1)));           // a random vector of +-1's
    if (n) hipLaunchKernelGGL(k_sign_half, dim3(nb), dim3(256), 0, ctx->stream, n, z);
    KS_CALL(balanced_mult(eps, z, p));                                                               // p = D Op (D \ z)
    if (eps->balance == KS_EPS_BALANCE_TWOSIDE) {
      if (j == 0) KS_CALL(ks_bv_normcolumn(eps->W, 4, KS_NORM_INFINITY, &norma));                    // VecAbs + VecMax: the estimate of the matrix infinity norm
      KS_CALL(ks_eps_pointwise(eps, z, eps->D, z, true));                                             // r = D \ (Op' (D z))
      KS_CALL(ks_mat_mult_transpose_internal(eps->op_inner, z, eps->wb));
      KS_CALL(ks_eps_pointwise(eps, eps->wb, eps->D, eps->wb, false));
      if (n) hipLaunchKernelGGL(k_bal_update2, dim3(nb), dim3(256), 0, ctx->stream, n, eps->D, p, eps->wb, eps->balance_cutoff * norma);
    } else if (n) hipLaunchKernelGGL(k_bal_update, dim3(nb), dim3(256), 0, ctx->stream, n, eps->D, p);
    KS_HIP(hipGetLastError());
  }
  return KS_SUCCESS;
}

// balancing in EPSSetUp (epssetup.c:383-391): build D, then expand with D Op D^-1
int ks_eps_setup_balance(ks_eps eps)
{
  ks_mat A = eps->A;
  eps->op_inner = eps->op;
  if (eps->balance == KS_EPS_BALANCE_ONESIDE || eps->balance == KS_EPS_BALANCE_TWOSIDE) KS_CALL(build_balance(eps));
  else KS_CHECK(eps->D && eps->D_n == A->n, KS_ERR_ORDER, "EPS_BALANCE_USER: the balancing matrix does not match the operator");
  if (!eps->bal_op) KS_CALL(ks_mat_create_shell(eps->ctx, A->n, A->row_start, A->n_global, balanced_mult, eps, &eps->bal_op));
  eps->bal_op->n = A->n; eps->bal_op->row_start = A->row_start; eps->bal_op->n_global = A->n_global;
  eps->bal_op->shell_nosync = !eps->op_inner->shell_mult;         // D A D^-1 on an assembled matrix is three kernel launches: keep the enqueued-ahead run
  eps->op = eps->bal_op; eps->balanced = true;
  return KS_SUCCESS;
}
