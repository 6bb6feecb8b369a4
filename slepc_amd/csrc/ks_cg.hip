// Conjugate gradients for the ST's inner solves (KS_KSP_CG): KSPCG with a left preconditioner and its default norm, the preconditioned residual,
// written from the algorithm (PETSc's KSP is external to the reference):
//     y = 0, r = b, z = M^-1 r, dp0 = ||z||, tol = max(rtol dp0, 1e-50)
//     iteration i:  gamma = (r,z);  p = z (i = 0) or z + (gamma / gamma_old) p;  w = P p;  delta = (p,w);  alpha = gamma / delta
//                   y += alpha p;  r -= alpha w;  z = M^-1 r;  dp = ||z||;  converged when dp <= tol
// The scalars never leave the device. A state block (KsCgState) holds them; an iteration is three row sweeps of this file around the existing
// product (and, for the preconditioners that are not pointwise, the existing application and a fourth sweep):
//     direction   sums the partials of (r,z) and (z,z) the sweep before it left, decides whether the solve has ended, p = z + beta p
//     (p,w)       partials of (p,w); with a P applied term by term, w = A p - sigma (B p | p) is formed in the same sweep
//     update      sums the partials of (p,w), y += alpha p, r -= alpha w, z = dinv .* r, partials of (r,z) and (z,z)
// The host enqueues `check` iterations, then reads the state once. Every sweep of an iteration that starts with `done` set returns without touching
// a vector, so the iterations enqueued past the end of the solve change nothing: count, iterate and residual norm are the same bits for every `check`.
//
// Who may write what: only thread 0 of workgroup 0 writes the state, and no field it writes in a launch is read by the other workgroups of that launch
// to decide what they compute - they all sum the same partials in the same order (reduce_partials_to_lds: a fixed order, no floating-point atomics) and so
// arrive at the same gamma, beta, alpha and the same verdict. The one word read and written inside one launch is `done`, read once per workgroup: one that starts after
// workgroup 0 has set it returns at the gate, one that started before returns when it reaches the same verdict itself - without a store either way.
// Kernel boundaries order everything else: a sweep's partials and the state are complete when the next launch begins.
// On more than one rank the partials are summed by a one-workgroup kernel into `red`, ks_allreduce_sum runs on it in stream order, and the consumer reads
// the sums there instead of the partials; a rank without rows writes zero partials and takes part in every collective.
#include "ks_sweeps.cuh"
#include <algorithm>

using namespace ksk;

namespace {

// The gate, the same for every wave of a workgroup: thread 0 reads `done` once and hands it out through LDS. Were every wave to read it for itself,
// workgroup 0 could set it in between, and the waves left would sum partials without the wave that owns a column of them (reduce_partials_to_lds).
__device__ __forceinline__ int cg_done(const KsCgState *st)
{
  __shared__ int gate;
  if (threadIdx.x == 0) gate = __atomic_load_n(&st->done, __ATOMIC_RELAXED);
  __syncthreads();
  return gate;
}
__device__ __forceinline__ void cg_end(KsCgState *st, int reason) { st->reason = reason; __atomic_store_n(&st->done, 1, __ATOMIC_RELAXED); }

// ncols <= 2 sums of this rank and its peers (red) or of this rank's workgroups (part, nblocks of them per column), the same values in every workgroup
__device__ __forceinline__ void cg_sums(const double *__restrict__ red, const double *__restrict__ part, int nblocks, int ncols, double *c_lds)
{
  if (red) { if ((int)threadIdx.x < ncols) c_lds[threadIdx.x] = red[threadIdx.x]; __syncthreads(); }
  else reduce_partials_to_lds(part, nblocks, ncols, c_lds);
}

// direction: the verdict on the iterate the last update left, then p = z + beta p (p = z in the first iteration)
template <int VEC>
__global__ __launch_bounds__(SW_BLOCK) void k_cg_direction(KsCgState *__restrict__ st, const double *__restrict__ red, const double *__restrict__ part, int nblocks,
                                                           double rtol, int max_it, int n, const double *__restrict__ z, double *__restrict__ p)
{
  const bool book = blockIdx.x == 0 && threadIdx.x == 0;
  if (cg_done(st)) { if (book) st->gated++; return; }
  __shared__ double c[2];
  cg_sums(red, part, nblocks, 2, c);
  const double gamma = c[0], dp = sqrt(c[1]);
  const int its = st->its;
  const bool first = its == 0;
  const double tol = first ? fmax(rtol * dp, 1e-50) : st->tol;
  int reason = 0;
  if (!isfinite(dp) || !isfinite(gamma)) reason = KS_CG_NAN;
  else if (dp <= tol) reason = KS_CG_CONVERGED;                      // a zero right-hand side ends here, before the first iteration
  else if (its >= max_it) reason = KS_CG_ITS;
  else if (gamma < 0.0) reason = KS_CG_INDEFINITE_PC;
  if (book) {
    st->dp = dp; st->gamma = gamma;
    if (first) st->tol = tol;
    if (reason) cg_end(st, reason);
  }
  if (reason) return;
  const double beta = first ? 0.0 : gamma / st->gamma_old;
  const long long tile = (long long)SW_BLOCK * VEC;
  const long long ntiles = ((long long)n + tile - 1) / tile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long r = t * tile + (long long)threadIdx.x * VEC;
    if (VEC == 2 && r + 1 < n) {
      double2 zv = *reinterpret_cast<const double2 *>(z + r);
      if (!first) { const double2 pv = *reinterpret_cast<const double2 *>(p + r); zv.x = fma(beta, pv.x, zv.x); zv.y = fma(beta, pv.y, zv.y); }
      *reinterpret_cast<double2 *>(p + r) = zv;
    } else {
      for (int v = 0; v < VEC; v++) if (r + v < n) p[r + v] = first ? z[r + v] : fma(beta, p[r + v], z[r + v]);
    }
  }
}

// partials of (p, w); COMBINE: w += b v first (the second term of a P that is applied term by term: v = B p, or p itself for the identity)
template <int VEC, bool COMBINE>
__global__ __launch_bounds__(SW_BLOCK) void k_cg_pw(const KsCgState *__restrict__ st, int n, const double *__restrict__ p, double *__restrict__ w, double b,
                                                    const double *__restrict__ v, double *__restrict__ part)
{
  if (cg_done(st)) return;
  double acc[1] = {0.0};
  const long long tile = (long long)SW_BLOCK * VEC;
  const long long ntiles = ((long long)n + tile - 1) / tile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long r = t * tile + (long long)threadIdx.x * VEC;
    if (VEC == 2 && r + 1 < n) {
      const double2 pv = *reinterpret_cast<const double2 *>(p + r);
      double2 wv = *reinterpret_cast<const double2 *>(w + r);
      if (COMBINE) {
        const double2 vv = *reinterpret_cast<const double2 *>(v + r);
        wv.x = fma(b, vv.x, wv.x); wv.y = fma(b, vv.y, wv.y);
        *reinterpret_cast<double2 *>(w + r) = wv;
      }
      acc[0] = fma(pv.x, wv.x, acc[0]); acc[0] = fma(pv.y, wv.y, acc[0]);
    } else {
      for (int u = 0; u < VEC; u++) if (r + u < n) {
        double wv = w[r + u];
        if (COMBINE) { wv = fma(b, v[r + u], wv); w[r + u] = wv; }
        acc[0] = fma(p[r + u], wv, acc[0]);
      }
    }
  }
  block_write_partials<1>(acc, 1, part);
}

// update: alpha from the partials of (p,w), y += alpha p, r -= alpha w; PC 0: z is r itself (no preconditioner), 1: z = dinv .* r, both with the partials
// of (r,z) and (z,z); 2: the sweep ends after r (the preconditioner's own kernels make z, k_cg_dots the partials)
template <int VEC, int PC>
__global__ __launch_bounds__(SW_BLOCK) void k_cg_update(KsCgState *__restrict__ st, const double *__restrict__ red, const double *__restrict__ part_d, int nblocks, int n,
                                                        const double *__restrict__ p, const double *__restrict__ w, const double *__restrict__ dinv,
                                                        double *__restrict__ y, double *__restrict__ r, double *__restrict__ z, double *__restrict__ part)
{
  if (cg_done(st)) return;
  __shared__ double c[1];
  cg_sums(red, part_d, nblocks, 1, c);
  const double delta = c[0], gamma = st->gamma;
  const int reason = !isfinite(delta) ? KS_CG_NAN : (delta <= 0.0 ? KS_CG_INDEFINITE_MAT : 0);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->delta = delta;
    if (reason) cg_end(st, reason);
    else { st->gamma_old = gamma; st->its++; }
  }
  if (reason) return;
  const double alpha = gamma / delta;
  double acc[2] = {0.0, 0.0};
  const long long tile = (long long)SW_BLOCK * VEC;
  const long long ntiles = ((long long)n + tile - 1) / tile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * tile + (long long)threadIdx.x * VEC;
    if (VEC == 2 && i + 1 < n) {
      const double2 pv = *reinterpret_cast<const double2 *>(p + i), wv = *reinterpret_cast<const double2 *>(w + i);
      double2 yv = *reinterpret_cast<const double2 *>(y + i), rv = *reinterpret_cast<const double2 *>(r + i);
      double2 dv; dv.x = dv.y = 1.0;
      if (PC == 1) dv = *reinterpret_cast<const double2 *>(dinv + i);
      yv.x = fma(alpha, pv.x, yv.x); yv.y = fma(alpha, pv.y, yv.y);
      rv.x = fma(-alpha, wv.x, rv.x); rv.y = fma(-alpha, wv.y, rv.y);
      *reinterpret_cast<double2 *>(y + i) = yv;
      *reinterpret_cast<double2 *>(r + i) = rv;
      if (PC != 2) {
        double2 zv = rv;
        if (PC == 1) { zv.x = dv.x * rv.x; zv.y = dv.y * rv.y; *reinterpret_cast<double2 *>(z + i) = zv; }
        acc[0] = fma(rv.x, zv.x, acc[0]); acc[0] = fma(rv.y, zv.y, acc[0]);
        acc[1] = fma(zv.x, zv.x, acc[1]); acc[1] = fma(zv.y, zv.y, acc[1]);
      }
    } else {
      for (int u = 0; u < VEC; u++) if (i + u < n) {
        const long long j = i + u;
        y[j] = fma(alpha, p[j], y[j]);
        const double rv = fma(-alpha, w[j], r[j]);
        r[j] = rv;
        if (PC != 2) {
          double zv = rv;
          if (PC == 1) { zv = dinv[j] * rv; z[j] = zv; }
          acc[0] = fma(rv, zv, acc[0]); acc[1] = fma(zv, zv, acc[1]);
        }
      }
    }
  }
  if (PC != 2) block_write_partials<2>(acc, 2, part);
}

// partials of (r,z) and (z,z): the start of a solve, and every iteration of a preconditioner with kernels of its own
template <int VEC>
__global__ __launch_bounds__(SW_BLOCK) void k_cg_dots(const KsCgState *__restrict__ st, int n, const double *__restrict__ r, const double *__restrict__ z, double *__restrict__ part)
{
  if (cg_done(st)) return;
  double acc[2] = {0.0, 0.0};
  const long long tile = (long long)SW_BLOCK * VEC;
  const long long ntiles = ((long long)n + tile - 1) / tile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * tile + (long long)threadIdx.x * VEC;
    if (VEC == 2 && i + 1 < n) {
      const double2 rv = *reinterpret_cast<const double2 *>(r + i), zv = *reinterpret_cast<const double2 *>(z + i);
      acc[0] = fma(rv.x, zv.x, acc[0]); acc[0] = fma(rv.y, zv.y, acc[0]);
      acc[1] = fma(zv.x, zv.x, acc[1]); acc[1] = fma(zv.y, zv.y, acc[1]);
    } else {
      for (int u = 0; u < VEC; u++) if (i + u < n) { acc[0] = fma(r[i + u], z[i + u], acc[0]); acc[1] = fma(z[i + u], z[i + u], acc[1]); }
    }
  }
  block_write_partials<2>(acc, 2, part);
}

// more than one rank: red[i] = this rank's sum of column i of the partials, for the allreduce behind it. Not gated: its inputs are left alone once the
// solve has ended, and every rank keeps issuing the same collectives
__global__ __launch_bounds__(SW_BLOCK) void k_cg_finish(const double *__restrict__ part, int nblocks, int ncols, double *__restrict__ red)
{
  __shared__ double c[2];
  reduce_partials_to_lds(part, nblocks, ncols, c);
  if ((int)threadIdx.x < ncols) red[threadIdx.x] = c[threadIdx.x];
}

inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

// one solve's device arrays and launch shape
struct Cg {
  ks_st st; ks_ctx ctx; int n, grid; bool multi, v2, tr;
  KsCgState *state; double *red, *part_gz, *part_d;
  double *r, *z, *p, *w, *y; const double *dinv; int pc;      // pc: the PC argument of k_cg_update

  // the sums of a sweep's partials across the ranks, stream-ordered: no host wait
  int collect(double *part, int ncols, double *out)
  {
    if (!multi) return KS_SUCCESS;
    hipLaunchKernelGGL(k_cg_finish, dim3(1), dim3(SW_BLOCK), 0, ctx->stream, part, grid, ncols, out);
    KS_HIP(hipGetLastError());
    st->cg_sweeps++;
    return ks_allreduce_sum(ctx, out, ncols);
  }
  int dots()
  {
    {
      KsProfScope ps(ctx, KS_K_OTHER, 16.0 * n);
      if (v2) hipLaunchKernelGGL(k_cg_dots<2>, dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, n, r, z, part_gz);
      else hipLaunchKernelGGL(k_cg_dots<1>, dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, n, r, z, part_gz);
      KS_HIP(hipGetLastError());
      st->cg_sweeps++;
    }
    return collect(part_gz, 2, red);
  }
  int direction(double rtol, int max_it)
  {
    KsProfScope ps(ctx, KS_K_OTHER, 24.0 * n);
    const double *rd = multi ? red : nullptr;
    if (v2) hipLaunchKernelGGL(k_cg_direction<2>, dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, rd, part_gz, grid, rtol, max_it, n, z, p);
    else hipLaunchKernelGGL(k_cg_direction<1>, dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, rd, part_gz, grid, rtol, max_it, n, z, p);
    KS_HIP(hipGetLastError());
    st->cg_sweeps++;
    return KS_SUCCESS;
  }
  // v: the term of P still to be added to w, w += b v (NULL: w is complete)
  int pw(const double *v, double b)
  {
    {
      KsProfScope ps(ctx, KS_K_OTHER, (v ? (v == p ? 24.0 : 32.0) : 16.0) * n);
      if (v) {
        if (v2 && aligned16(v)) hipLaunchKernelGGL((k_cg_pw<2, true>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, n, p, w, b, v, part_d);
        else hipLaunchKernelGGL((k_cg_pw<1, true>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, n, p, w, b, v, part_d);
      } else {
        if (v2) hipLaunchKernelGGL((k_cg_pw<2, false>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, n, p, w, b, v, part_d);
        else hipLaunchKernelGGL((k_cg_pw<1, false>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, n, p, w, b, v, part_d);
      }
      KS_HIP(hipGetLastError());
      st->cg_sweeps++;
    }
    return collect(part_d, 1, red + 2);
  }
  int update()
  {
    {
      KsProfScope ps(ctx, KS_K_OTHER, (pc == 0 ? 48.0 : pc == 1 ? 64.0 : 48.0) * n);
      const double *rd = multi ? red + 2 : nullptr;
#define KS_CG_UPDATE(VEC, PC) hipLaunchKernelGGL((k_cg_update<VEC, PC>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, rd, part_d, grid, n, p, w, dinv, y, r, z, part_gz)
      if (v2) { if (pc == 0) KS_CG_UPDATE(2, 0); else if (pc == 1) KS_CG_UPDATE(2, 1); else KS_CG_UPDATE(2, 2); }
      else { if (pc == 0) KS_CG_UPDATE(1, 0); else if (pc == 1) KS_CG_UPDATE(1, 1); else KS_CG_UPDATE(1, 2); }
#undef KS_CG_UPDATE
      KS_HIP(hipGetLastError());
      st->cg_sweeps++;
    }
    if (pc == 2) { KS_CALL(ks_st_blocks_apply(st, r, z, tr)); return dots(); }
    return collect(part_gz, 2, red);
  }
};

} // namespace

// the device scratch of the solver (state, the ranks' sums, the two partials arrays) and the pinned copy of the state the host reads
int ks_st_cg_alloc(ks_st st)
{
  if (st->cg_dev) return KS_SUCCESS;
  KS_HIP(hipMalloc(&st->cg_dev, KS_CG_STATE_BYTES + sizeof(double) * 3 * (size_t)KS_MAX_BLOCKS));
  KS_HIP(hipHostMalloc((void **)&st->cg_host, sizeof(KsCgState), hipHostMallocDefault));
  return KS_SUCCESS;
}
void ks_st_cg_free(ks_st st)
{
  if (st->cg_dev) hipFree(st->cg_dev);
  if (st->cg_host) hipHostFree(st->cg_host);
  st->cg_dev = nullptr; st->cg_host = nullptr;
}

int ks_ksp_cg(const KsKsp &k, ks_st st, bool tr, const double *rhs, double *y)
{
  ks_ctx ctx = k.ctx;
  static_assert(sizeof(KsCgState) + 4 * sizeof(double) <= KS_CG_STATE_BYTES, "state and the ranks' sums share the head of the scratch");
  KS_CALL(ks_st_cg_alloc(st));
  Cg s;
  s.st = st; s.ctx = ctx; s.n = (int)k.n; s.tr = tr; s.multi = ks_is_multi(ctx);
  s.grid = ks_sweep_grid(ctx, s.n, 2);        // one grid for every sweep, so that the partials line up: at most 4 workgroups per CU, KS_MAX_BLOCKS at the most (what the
                                              // partials arrays hold); the one-row-per-lane forms of a misaligned vector keep it and walk twice the tiles per workgroup
  s.state = (KsCgState *)st->cg_dev; s.red = (double *)(st->cg_dev + sizeof(KsCgState));
  s.part_gz = (double *)(st->cg_dev + KS_CG_STATE_BYTES); s.part_d = s.part_gz + 2 * (size_t)KS_MAX_BLOCKS;
  const double *dinv = nullptr;
  const bool pointwise = ks_st_pc_pointwise(st, &dinv);
  s.pc = !pointwise ? 2 : (dinv ? 1 : 0); s.dinv = dinv;
  s.r = ks_bv_col(k.Kb, 0); s.z = s.pc == 0 ? s.r : ks_bv_col(k.Kb, 1); s.p = ks_bv_col(k.Kb, 2); s.w = ks_bv_col(k.Kb, 3); s.y = y;
  s.v2 = aligned16(s.r) && aligned16(s.z) && aligned16(s.p) && aligned16(s.w) && aligned16(y);
  (*k.solves)++;
  KS_HIP(hipMemsetAsync(s.state, 0, KS_CG_STATE_BYTES, ctx->stream));
  KS_HIP(hipMemsetAsync(y, 0, sizeof(double) * std::max<long long>(k.n, 1), ctx->stream));
  KS_CALL(ksk_copy(ctx, rhs, s.r, (size_t)k.n));
  if (s.pc == 1) KS_CALL(ksk_lincomb(ctx, k.n, dinv, 1.0, s.r, 0.0, nullptr, s.z));
  else if (s.pc == 2) KS_CALL(ks_st_blocks_apply(st, s.r, s.z, tr));
  KS_CALL(s.dots());
  KsCgState *hs = st->cg_host;
  for (;;) {
    for (int j = 0; j < st->cg_check; j++) {
      KS_CALL(s.direction(k.rtol, k.max_it));
      const double *v = nullptr; double b = 0.0;
      KS_CALL(ks_st_cg_product(st, tr, s.p, s.w, &v, &b));
      KS_CALL(s.pw(v, b));
      KS_CALL(s.update());
    }
    KS_HIP(hipMemcpyAsync(hs, s.state, sizeof(KsCgState), hipMemcpyDeviceToHost, ctx->stream));
    KS_HIP(ks_sync(ctx));
    st->cg_waits++;
    KS_CALL(ks_oneshot_error(ctx));
    if (hs->done) break;
  }
  *k.its += hs->its; *k.last_rnorm = hs->dp; st->cg_gated += hs->gated;
  if (hs->reason == KS_CG_CONVERGED || !k.strict) return KS_SUCCESS;
  switch (hs->reason) {
    case KS_CG_ITS: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: CG reached %d iterations, preconditioned residual %g > %g", hs->its, hs->dp, hs->tol);
    case KS_CG_INDEFINITE_MAT: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: CG met an indefinite matrix, (p, P p) = %g in iteration %d", hs->delta, hs->its);
    case KS_CG_INDEFINITE_PC: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: CG met an indefinite preconditioner, (r, M^-1 r) = %g in iteration %d", hs->gamma, hs->its);
    default: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: CG met not a number in iteration %d ((r, M^-1 r) = %g, (p, P p) = %g, residual %g)", hs->its, hs->gamma, hs->delta, hs->dp);
  }
}
