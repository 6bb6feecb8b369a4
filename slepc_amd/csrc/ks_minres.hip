// MINRES for the ST's inner solves (KS_KSP_MINRES): the minimum residual method of Paige and Saunders for a symmetric, possibly indefinite P, with a
// symmetric positive definite preconditioner M applied symmetrically, written from the algorithm (PETSc's KSP is external to the reference). The norm
// it minimises and reports is phibar = ||b - P y|| in the M^-1 inner product:
//     y = 0; r1 = r2 = b; z = M^-1 b; beta1 = sqrt((b,z)); tol = max(rtol beta1, 1e-50)          (beta1 == 0: y = 0, no iteration)
//     oldb = 0; beta = beta1; dbar = 0; epsln = 0; phibar = beta1; cs = -1; sn = 0; w = w2 = 0
//     iteration i:  v = z / beta;  u = P v;  if i > 0: u -= (beta / oldb) r1;  alfa = (v,u);  u -= (alfa / beta) r2
//                   r1 = r2; r2 = u;  z = M^-1 r2;  oldb = beta;  beta = sqrt((r2,z))
//                   oldeps = epsln;  delta = cs dbar + sn alfa;  gbar = sn dbar - cs alfa;  epsln = sn beta;  dbar = -cs beta
//                   gamma = max(hypot(gbar, beta), DBL_EPSILON);  cs = gbar / gamma;  sn = beta / gamma;  phi = cs phibar;  phibar = sn phibar
//                   w1 = w2; w2 = w;  w = (v - oldeps w1 - delta w2) / gamma;  y += phi w;  converged when phibar <= tol
// The scalars never leave the device. A state block (KsMinresState) holds them; an iteration is three row sweeps of this file around the existing
// product (and, for the preconditioners that are not pointwise, the existing application and a dot sweep):
//     alfa      partials of (v, t), t = u - (beta / oldb) r1 formed in registers and not stored; with a P applied term by term, u = A v - sigma (B v | v)
//               is formed and stored in the same sweep                                                                    3 passes (v, u, r1)
//     lanczos   sums those partials; r_new = t - (alfa / beta) r2, the same t, into r1's buffer; z = dinv .* r_new; partials of (r_new, z)
//                                                                                                                         5 passes (u, r1, r2, r_new, z) + dinv
//     update    sums (r_new, z), the rotation, w_new = (v - oldeps w1 - delta w2) / gamma into w1's buffer, y += phi w_new, v = z / beta for the
//               next product; decides whether the solve has ended                                                          8 passes (v, w1, w2, w_new, y, y, z, v)
// The residuals live in two buffers and the directions in two, both rotated by the parity of the iteration index, which the host knows when it
// enqueues: an iteration either runs as the one it was enqueued as or not at all. Seven work vectors: v, u, two residuals, z, two directions.
// The (v,u) dot takes u after the r1 term, as the algorithm states it; that costs the alfa sweep a read of r1 (16 passes, not 15) and keeps
// tests/minres_cases.py the same operations in the same order.
// The host enqueues `check` iterations, then reads the state once. Every sweep of an iteration that starts after the solve has ended returns
// without touching a vector: count, iterate and residual norm are the same bits for every `check`.
//
// Who may write what: only thread 0 of workgroup 0 writes the state, and no field written in a launch is read by the other workgroups of that
// launch to decide what they compute. Every workgroup sums the same partials in the same order (reduce_partials_to_lds, no floating-point atomics)
// and runs the same instructions on them, so all arrive at the same alfa, beta, rotation and verdict.
//   rot[2]   cs, sn, dbar, epsln, phibar and beta are read AND rewritten by the update sweep. They are double-buffered by the iteration's parity:
//            iteration i reads rot[i & 1] and its update writes rot[(i + 1) & 1], which no workgroup of that launch reads. beta of rot[(i + 1) & 1]
//            is oldb to iteration i + 1 until that iteration's update overwrites it - the last launch of the iteration, which does not read oldb.
//   alfa     written by the lanczos sweep, read by the update sweep behind it. tol, beta1: written by the start sweep, read by the updates.
//   done     set where a sweep ends the solve WITHOUT doing its vector work (not a number, indefinite preconditioner, a zero right-hand side): a
//            workgroup that starts after workgroup 0 has set it returns at the gate, one that started before reaches the same verdict itself -
//            no store either way, as in ks_cg.hip.
//   conv     set by the update sweep that ends the solve AFTER its vector work (converged, max_it). No gate of that launch reads it - a workgroup
//            that saw it would skip work the iterate needs. The first sweep of the next iteration (alfa) gates on done | conv and its bookkeeping
//            thread turns conv into done, so the sweeps behind it, the update included, gate on done alone, set by an earlier launch.
// Kernel boundaries order everything else: a sweep's partials and the state are complete when the next launch begins. The product and the block
// preconditioners between the sweeps are not gated: they write u and z, which nobody reads once the solve has ended.
// On more than one rank a sweep's partials are summed by a one-workgroup kernel into `red`, ks_allreduce_sum runs on it in stream order, and the
// consumer reads the sum there: two collectives per iteration. A rank without rows writes zero partials and takes part in every collective.
#include "ks_sweeps.cuh"
#include <algorithm>
#include <cfloat>

using namespace ksk;

namespace {

// The gate, the same for every wave of a workgroup (see cg_done, ks_cg.hip): thread 0 reads once, LDS hands it out. WITH_CONV: the first sweep of an iteration
template <bool WITH_CONV>
__device__ __forceinline__ int mr_done(const KsMinresState *st)
{
  __shared__ int gate;
  if (threadIdx.x == 0) {
    int g = __atomic_load_n(&st->done, __ATOMIC_RELAXED);
    if (WITH_CONV) g |= __atomic_load_n(&st->conv, __ATOMIC_RELAXED);
    gate = g;
  }
  __syncthreads();
  return gate;
}
__device__ __forceinline__ void mr_end(KsMinresState *st, int reason) { st->reason = reason; __atomic_store_n(&st->done, 1, __ATOMIC_RELAXED); }

// one sum of this rank and its peers (red) or of this rank's workgroups (part), the same value in every workgroup
__device__ __forceinline__ double mr_sum(const double *__restrict__ red, const double *__restrict__ part, int nblocks)
{
  __shared__ double c[1];
  if (red) { if (threadIdx.x == 0) c[0] = red[0]; __syncthreads(); }
  else reduce_partials_to_lds(part, nblocks, 1, c);
  return c[0];
}

// start: beta1 from the partials of (b, z), the verdict on the right-hand side, the scalars of iteration 0, v = z / beta1
template <int VEC>
__global__ __launch_bounds__(SW_BLOCK) void k_minres_start(KsMinresState *__restrict__ st, const double *__restrict__ red, const double *__restrict__ part, int nblocks,
                                                           double rtol, int n, const double *__restrict__ z, double *__restrict__ v)
{
  const double bz = mr_sum(red, part, nblocks);
  const double beta1 = sqrt(bz);
  int reason = 0;
  if (!isfinite(bz)) reason = KS_MINRES_NAN;
  else if (bz < 0.0) reason = KS_MINRES_INDEFINITE_PC;
  else if (beta1 == 0.0) reason = KS_MINRES_CONVERGED;                 // a zero right-hand side: y = 0 and no iteration
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    KsMinresRot r; r.cs = -1.0; r.sn = 0.0; r.dbar = 0.0; r.epsln = 0.0; r.phibar = reason ? 0.0 : beta1; r.beta = beta1;
    st->rot[0] = r; st->bz = bz; st->beta1 = beta1; st->tol = fmax(rtol * beta1, 1e-50);
    if (reason) mr_end(st, reason);
  }
  if (reason) return;
  const long long tile = (long long)SW_BLOCK * VEC;
  const long long ntiles = ((long long)n + tile - 1) / tile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * tile + (long long)threadIdx.x * VEC;
    if (VEC == 2 && i + 1 < n) {
      double2 zv = *reinterpret_cast<const double2 *>(z + i);
      zv.x /= beta1; zv.y /= beta1;
      *reinterpret_cast<double2 *>(v + i) = zv;
    } else {
      for (int k = 0; k < VEC; k++) if (i + k < n) v[i + k] = z[i + k] / beta1;
    }
  }
}

// alfa: partials of (v, t), t = u - (beta / oldb) r1 (FIRST: t = u); COMBINE: u += b x first (the second term of a P that is applied term by term:
// x = B v, or v itself for the identity). par: the parity of the iteration
template <int VEC, bool COMBINE, bool FIRST>
__global__ __launch_bounds__(SW_BLOCK) void k_minres_alfa(KsMinresState *__restrict__ st, int par, int n, const double *__restrict__ v, double *__restrict__ u, double b,
                                                          const double *__restrict__ x, const double *__restrict__ r1, double *__restrict__ part)
{
  if (mr_done<true>(st)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { st->gated++; __atomic_store_n(&st->done, 1, __ATOMIC_RELAXED); }
    return;
  }
  const double c = FIRST ? 0.0 : st->rot[par].beta / st->rot[par ^ 1].beta;
  double acc[1] = {0.0};
  const long long tile = (long long)SW_BLOCK * VEC;
  const long long ntiles = ((long long)n + tile - 1) / tile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * tile + (long long)threadIdx.x * VEC;
    if (VEC == 2 && i + 1 < n) {
      const double2 vv = *reinterpret_cast<const double2 *>(v + i);
      double2 uv = *reinterpret_cast<const double2 *>(u + i);
      if (COMBINE) {
        const double2 xv = *reinterpret_cast<const double2 *>(x + i);
        uv.x = fma(b, xv.x, uv.x); uv.y = fma(b, xv.y, uv.y);
        *reinterpret_cast<double2 *>(u + i) = uv;
      }
      if (!FIRST) { const double2 rv = *reinterpret_cast<const double2 *>(r1 + i); uv.x = fma(-c, rv.x, uv.x); uv.y = fma(-c, rv.y, uv.y); }
      acc[0] = fma(vv.x, uv.x, acc[0]); acc[0] = fma(vv.y, uv.y, acc[0]);
    } else {
      for (int k = 0; k < VEC; k++) if (i + k < n) {
        const long long j = i + k;
        double uv = u[j];
        if (COMBINE) { uv = fma(b, x[j], uv); u[j] = uv; }
        if (!FIRST) uv = fma(-c, r1[j], uv);
        acc[0] = fma(v[j], uv, acc[0]);
      }
    }
  }
  block_write_partials<1>(acc, 1, part);
}

// lanczos: alfa from the partials, r_new = (u - (beta / oldb) r1) - (alfa / beta) r2 into r1's buffer; PC 0: z is r_new itself (no preconditioner), 1: z = dinv .* r_new,
// both with the partials of (r_new, z); 2: the sweep ends after r_new (the preconditioner's own kernels make z, k_minres_dot the partials)
template <int VEC, int PC, bool FIRST>
__global__ __launch_bounds__(SW_BLOCK) void k_minres_lanczos(KsMinresState *__restrict__ st, int par, const double *__restrict__ red, const double *__restrict__ part_a, int nblocks, int n,
                                                             const double *__restrict__ u, const double *__restrict__ r2, double *__restrict__ r1, const double *__restrict__ dinv,
                                                             double *__restrict__ z, double *__restrict__ part)
{
  if (mr_done<false>(st)) return;
  const double alfa = mr_sum(red, part_a, nblocks);
  const double beta = st->rot[par].beta;
  const int reason = !isfinite(alfa) ? KS_MINRES_NAN : 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->alfa = alfa;
    if (reason) mr_end(st, reason);
  }
  if (reason) return;
  const double c = FIRST ? 0.0 : beta / st->rot[par ^ 1].beta, a = alfa / beta;
  double acc[1] = {0.0};
  const long long tile = (long long)SW_BLOCK * VEC;
  const long long ntiles = ((long long)n + tile - 1) / tile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * tile + (long long)threadIdx.x * VEC;
    if (VEC == 2 && i + 1 < n) {
      double2 rn = *reinterpret_cast<const double2 *>(u + i);
      const double2 r2v = *reinterpret_cast<const double2 *>(r2 + i);
      if (!FIRST) { const double2 r1v = *reinterpret_cast<const double2 *>(r1 + i); rn.x = fma(-c, r1v.x, rn.x); rn.y = fma(-c, r1v.y, rn.y); }
      rn.x = fma(-a, r2v.x, rn.x); rn.y = fma(-a, r2v.y, rn.y);
      *reinterpret_cast<double2 *>(r1 + i) = rn;
      if (PC != 2) {
        double2 zv = rn;
        if (PC == 1) { const double2 dv = *reinterpret_cast<const double2 *>(dinv + i); zv.x = dv.x * rn.x; zv.y = dv.y * rn.y; *reinterpret_cast<double2 *>(z + i) = zv; }
        acc[0] = fma(rn.x, zv.x, acc[0]); acc[0] = fma(rn.y, zv.y, acc[0]);
      }
    } else {
      for (int k = 0; k < VEC; k++) if (i + k < n) {
        const long long j = i + k;
        double rn = u[j];
        if (!FIRST) rn = fma(-c, r1[j], rn);
        rn = fma(-a, r2[j], rn);
        r1[j] = rn;
        if (PC != 2) {
          double zv = rn;
          if (PC == 1) { zv = dinv[j] * rn; z[j] = zv; }
          acc[0] = fma(rn, zv, acc[0]);
        }
      }
    }
  }
  if (PC != 2) block_write_partials<1>(acc, 1, part);
}

// update: beta from the partials of (r_new, z), the rotation, w_new = (v - oldeps w1 - delta w2) / gamma into w1's buffer, y += phi w_new, v = z / beta; the end of the solve
template <int VEC>
__global__ __launch_bounds__(SW_BLOCK) void k_minres_update(KsMinresState *__restrict__ st, int par, const double *__restrict__ red, const double *__restrict__ part_b, int nblocks,
                                                            int max_it, int n, const double *__restrict__ z, double *__restrict__ v, const double *__restrict__ w2,
                                                            double *__restrict__ w1, double *__restrict__ y)
{
  if (mr_done<false>(st)) return;
  const double bz = mr_sum(red, part_b, nblocks);
  const int reason = !isfinite(bz) ? KS_MINRES_NAN : (bz < 0.0 ? KS_MINRES_INDEFINITE_PC : 0);
  const bool book = blockIdx.x == 0 && threadIdx.x == 0;
  if (reason) {
    if (book) { st->bz = bz; mr_end(st, reason); }
    return;
  }
  const KsMinresRot o = st->rot[par];
  const double alfa = st->alfa, beta = sqrt(bz);
  const double oldeps = o.epsln;
  const double delta = fma(o.cs, o.dbar, o.sn * alfa), gbar = fma(o.sn, o.dbar, -(o.cs * alfa));
  KsMinresRot r;
  r.epsln = o.sn * beta; r.dbar = -o.cs * beta;
  const double gamma = fmax(hypot(gbar, beta), DBL_EPSILON);
  r.cs = gbar / gamma; r.sn = beta / gamma; r.beta = beta;
  const double phi = r.cs * o.phibar;
  r.phibar = r.sn * o.phibar;
  if (book) {
    const int its = st->its + 1;
    st->rot[par ^ 1] = r; st->bz = bz; st->its = its;
    const int end = r.phibar <= st->tol ? KS_MINRES_CONVERGED : (its >= max_it ? KS_MINRES_ITS : 0);
    if (end) { st->reason = end; __atomic_store_n(&st->conv, 1, __ATOMIC_RELAXED); }      // after this sweep's work: read by the next launches only
  }
  const bool next = beta > 0.0;                 // beta == 0: the lucky breakdown, phibar = 0 and the solve has converged; there is no next v
  const long long tile = (long long)SW_BLOCK * VEC;
  const long long ntiles = ((long long)n + tile - 1) / tile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * tile + (long long)threadIdx.x * VEC;
    if (VEC == 2 && i + 1 < n) {
      const double2 vv = *reinterpret_cast<const double2 *>(v + i), w1v = *reinterpret_cast<const double2 *>(w1 + i), w2v = *reinterpret_cast<const double2 *>(w2 + i);
      const double2 zv = *reinterpret_cast<const double2 *>(z + i);
      double2 yv = *reinterpret_cast<const double2 *>(y + i), wn;
      wn.x = fma(-delta, w2v.x, fma(-oldeps, w1v.x, vv.x)) / gamma; wn.y = fma(-delta, w2v.y, fma(-oldeps, w1v.y, vv.y)) / gamma;
      yv.x = fma(phi, wn.x, yv.x); yv.y = fma(phi, wn.y, yv.y);
      *reinterpret_cast<double2 *>(w1 + i) = wn;
      *reinterpret_cast<double2 *>(y + i) = yv;
      if (next) { double2 nv; nv.x = zv.x / beta; nv.y = zv.y / beta; *reinterpret_cast<double2 *>(v + i) = nv; }
    } else {
      for (int k = 0; k < VEC; k++) if (i + k < n) {
        const long long j = i + k;
        const double wn = fma(-delta, w2[j], fma(-oldeps, w1[j], v[j])) / gamma;
        w1[j] = wn;
        y[j] = fma(phi, wn, y[j]);
        if (next) v[j] = z[j] / beta;
      }
    }
  }
}

// partials of (r, z): the start of a solve, and every iteration of a preconditioner with kernels of its own
template <int VEC>
__global__ __launch_bounds__(SW_BLOCK) void k_minres_dot(const KsMinresState *__restrict__ st, int n, const double *__restrict__ r, const double *__restrict__ z, double *__restrict__ part)
{
  if (mr_done<false>(st)) return;
  double acc[1] = {0.0};
  const long long tile = (long long)SW_BLOCK * VEC;
  const long long ntiles = ((long long)n + tile - 1) / tile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * tile + (long long)threadIdx.x * VEC;
    if (VEC == 2 && i + 1 < n) {
      const double2 rv = *reinterpret_cast<const double2 *>(r + i), zv = *reinterpret_cast<const double2 *>(z + i);
      acc[0] = fma(rv.x, zv.x, acc[0]); acc[0] = fma(rv.y, zv.y, acc[0]);
    } else {
      for (int k = 0; k < VEC; k++) if (i + k < n) acc[0] = fma(r[i + k], z[i + k], acc[0]);
    }
  }
  block_write_partials<1>(acc, 1, part);
}

// more than one rank: red[0] = this rank's sum of the partials, for the allreduce behind it. Not gated: its input is left alone once the solve has
// ended, and every rank keeps issuing the same collectives
__global__ __launch_bounds__(SW_BLOCK) void k_minres_finish(const double *__restrict__ part, int nblocks, double *__restrict__ red)
{
  __shared__ double c[1];
  reduce_partials_to_lds(part, nblocks, 1, c);
  if (threadIdx.x == 0) red[0] = c[0];
}

inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

// one solve's device arrays and launch shape
struct Minres {
  ks_st st; ks_ctx ctx; int n, grid; bool multi, v2, tr;
  KsMinresState *state; double *red, *part_a, *part_b;
  double *v, *u, *R[2], *z, *W[2], *y; const double *dinv; int pc;      // pc: the PC argument of k_minres_lanczos; pc 0: z is the newest residual, no buffer of its own

  int collect(double *part, double *out)
  {
    if (!multi) return KS_SUCCESS;
    hipLaunchKernelGGL(k_minres_finish, dim3(1), dim3(SW_BLOCK), 0, ctx->stream, part, grid, out);
    KS_HIP(hipGetLastError());
    st->mr_sweeps++;
    return ks_allreduce_sum(ctx, out, 1);
  }
  int dot(const double *r, const double *zz)
  {
    {
      KsProfScope ps(ctx, KS_K_OTHER, (r == zz ? 8.0 : 16.0) * n);
      if (v2) hipLaunchKernelGGL(k_minres_dot<2>, dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, n, r, zz, part_b);
      else hipLaunchKernelGGL(k_minres_dot<1>, dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, n, r, zz, part_b);
      KS_HIP(hipGetLastError());
      st->mr_sweeps++;
    }
    return collect(part_b, red + 1);
  }
  int start(double rtol, const double *zz)
  {
    KsProfScope ps(ctx, KS_K_OTHER, 16.0 * n);
    const double *rd = multi ? red + 1 : nullptr;
    if (v2) hipLaunchKernelGGL(k_minres_start<2>, dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, rd, part_b, grid, rtol, n, zz, v);
    else hipLaunchKernelGGL(k_minres_start<1>, dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, rd, part_b, grid, rtol, n, zz, v);
    KS_HIP(hipGetLastError());
    st->mr_sweeps++;
    return KS_SUCCESS;
  }
  // x: the term of P still to be added to u, u += b x (NULL: u is complete)
  int alfa(int it, const double *x, double b)
  {
    {
      const bool first = it == 0; const int par = it & 1;
      KsProfScope ps(ctx, KS_K_OTHER, ((first ? 16.0 : 24.0) + (x ? (x == v ? 8.0 : 16.0) : 0.0)) * n);
      const bool two = v2 && (!x || aligned16(x));
#define KS_MR_ALFA(VEC, COMBINE, FIRST) hipLaunchKernelGGL((k_minres_alfa<VEC, COMBINE, FIRST>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, par, n, v, u, b, x, R[par], part_a)
      if (two) { if (x) { if (first) KS_MR_ALFA(2, true, true); else KS_MR_ALFA(2, true, false); } else { if (first) KS_MR_ALFA(2, false, true); else KS_MR_ALFA(2, false, false); } }
      else { if (x) { if (first) KS_MR_ALFA(1, true, true); else KS_MR_ALFA(1, true, false); } else { if (first) KS_MR_ALFA(1, false, true); else KS_MR_ALFA(1, false, false); } }
#undef KS_MR_ALFA
      KS_HIP(hipGetLastError());
      st->mr_sweeps++;
    }
    return collect(part_a, red);
  }
  int lanczos(int it)
  {
    const bool first = it == 0; const int par = it & 1;
    double *rn = R[par];                        // r1's buffer takes the new residual
    {
      KsProfScope ps(ctx, KS_K_OTHER, ((first ? 24.0 : 32.0) + (pc == 1 ? 16.0 : 0.0)) * n);
      const double *rd = multi ? red : nullptr;
#define KS_MR_LANCZOS(VEC, PC, FIRST) hipLaunchKernelGGL((k_minres_lanczos<VEC, PC, FIRST>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, par, rd, part_a, grid, n, u, R[par ^ 1], rn, dinv, z, part_b)
#define KS_MR_LANCZOS_PC(VEC, FIRST) do { if (pc == 0) KS_MR_LANCZOS(VEC, 0, FIRST); else if (pc == 1) KS_MR_LANCZOS(VEC, 1, FIRST); else KS_MR_LANCZOS(VEC, 2, FIRST); } while (0)
      if (v2) { if (first) KS_MR_LANCZOS_PC(2, true); else KS_MR_LANCZOS_PC(2, false); }
      else { if (first) KS_MR_LANCZOS_PC(1, true); else KS_MR_LANCZOS_PC(1, false); }
#undef KS_MR_LANCZOS_PC
#undef KS_MR_LANCZOS
      KS_HIP(hipGetLastError());
      st->mr_sweeps++;
    }
    if (pc == 2) { KS_CALL(ks_st_blocks_apply(st, rn, z, tr)); return dot(rn, z); }
    return collect(part_b, red + 1);
  }
  int update(int it, int max_it)
  {
    const int par = it & 1;
    const double *zz = pc == 0 ? R[par] : z;
    KsProfScope ps(ctx, KS_K_OTHER, 64.0 * n);
    const double *rd = multi ? red + 1 : nullptr;
    // w2 (the last direction) is in W[par ^ 1], w1 (the one before) in W[par], which takes the new one
    if (v2) hipLaunchKernelGGL(k_minres_update<2>, dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, par, rd, part_b, grid, max_it, n, zz, v, W[par ^ 1], W[par], y);
    else hipLaunchKernelGGL(k_minres_update<1>, dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, state, par, rd, part_b, grid, max_it, n, zz, v, W[par ^ 1], W[par], y);
    KS_HIP(hipGetLastError());
    st->mr_sweeps++;
    return KS_SUCCESS;
  }
};

} // namespace

// the device scratch of the solver (state, the ranks' sums, the two partials arrays) and the pinned copy of the state the host reads
int ks_st_minres_alloc(ks_st st)
{
  if (st->mr_dev) return KS_SUCCESS;
  KS_HIP(hipMalloc(&st->mr_dev, KS_MINRES_STATE_BYTES + sizeof(double) * 2 * (size_t)KS_MAX_BLOCKS));
  KS_HIP(hipHostMalloc((void **)&st->mr_host, sizeof(KsMinresState), hipHostMallocDefault));
  return KS_SUCCESS;
}
void ks_st_minres_free(ks_st st)
{
  if (st->mr_dev) hipFree(st->mr_dev);
  if (st->mr_host) hipHostFree(st->mr_host);
  st->mr_dev = nullptr; st->mr_host = nullptr;
}

int ks_ksp_minres(const KsKsp &k, ks_st st, bool tr, const double *rhs, double *y)
{
  ks_ctx ctx = k.ctx;
  static_assert(sizeof(KsMinresState) + 2 * sizeof(double) <= KS_MINRES_STATE_BYTES, "state and the ranks' sums share the head of the scratch");
  KS_CALL(ks_st_minres_alloc(st));
  Minres s;
  s.st = st; s.ctx = ctx; s.n = (int)k.n; s.tr = tr; s.multi = ks_is_multi(ctx);
  s.grid = ks_sweep_grid(ctx, s.n, 2);        // one grid for every sweep, so that the partials line up (see ks_ksp_cg)
  s.state = (KsMinresState *)st->mr_dev; s.red = (double *)(st->mr_dev + sizeof(KsMinresState));
  s.part_a = (double *)(st->mr_dev + KS_MINRES_STATE_BYTES); s.part_b = s.part_a + (size_t)KS_MAX_BLOCKS;
  const double *dinv = nullptr;
  const bool pointwise = ks_st_pc_pointwise(st, &dinv);
  s.pc = !pointwise ? 2 : (dinv ? 1 : 0); s.dinv = dinv;
  s.v = ks_bv_col(k.Kb, 0); s.u = ks_bv_col(k.Kb, 1); s.R[0] = ks_bv_col(k.Kb, 2); s.R[1] = ks_bv_col(k.Kb, 3); s.z = ks_bv_col(k.Kb, 4);
  s.W[0] = ks_bv_col(k.Kb, 5); s.W[1] = ks_bv_col(k.Kb, 6); s.y = y;
  s.v2 = aligned16(s.v) && aligned16(s.u) && aligned16(s.R[0]) && aligned16(s.R[1]) && aligned16(s.z) && aligned16(s.W[0]) && aligned16(s.W[1]) && aligned16(y) &&
         (!dinv || aligned16(dinv));
  (*k.solves)++;
  const size_t bytes = sizeof(double) * (size_t)std::max<long long>(k.n, 1);
  KS_HIP(hipMemsetAsync(s.state, 0, KS_MINRES_STATE_BYTES, ctx->stream));
  KS_HIP(hipMemsetAsync(y, 0, bytes, ctx->stream));
  if (k.n > 0) {                                                       // w = w2 = 0
    KS_HIP(hipMemsetAsync(s.W[0], 0, bytes, ctx->stream));
    KS_HIP(hipMemsetAsync(s.W[1], 0, bytes, ctx->stream));
  }
  KS_CALL(ksk_copy(ctx, rhs, s.R[1], (size_t)k.n));                    // r2 of iteration 0; r1 is not read there
  const double *z0 = s.R[1];
  if (s.pc == 1) { KS_CALL(ksk_lincomb(ctx, k.n, dinv, 1.0, s.R[1], 0.0, nullptr, s.z)); z0 = s.z; }
  else if (s.pc == 2) { KS_CALL(ks_st_blocks_apply(st, s.R[1], s.z, tr)); z0 = s.z; }
  KS_CALL(s.dot(s.R[1], z0));
  KS_CALL(s.start(k.rtol, z0));
  KsMinresState *hs = st->mr_host;
  for (int it = 0;;) {
    for (int j = 0; j < st->mr_check; j++, it++) {
      const double *x = nullptr; double b = 0.0;
      KS_CALL(ks_st_cg_product(st, tr, s.v, s.u, &x, &b));
      KS_CALL(s.alfa(it, x, b));
      KS_CALL(s.lanczos(it));
      KS_CALL(s.update(it, k.max_it));
    }
    KS_HIP(hipMemcpyAsync(hs, s.state, sizeof(KsMinresState), hipMemcpyDeviceToHost, ctx->stream));
    KS_HIP(ks_sync(ctx));
    st->mr_waits++;
    KS_CALL(ks_oneshot_error(ctx));
    if (hs->done || hs->conv) break;
  }
  const double phibar = hs->rot[hs->its & 1].phibar;                   // the rotation the last completed iteration left
  *k.its += hs->its; *k.last_rnorm = phibar; st->mr_gated += hs->gated;
  if (hs->reason == KS_MINRES_CONVERGED || !k.strict) return KS_SUCCESS;
  switch (hs->reason) {
    case KS_MINRES_ITS: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: MINRES reached %d iterations, residual %g > %g", hs->its, phibar, hs->tol);
    case KS_MINRES_INDEFINITE_PC: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: MINRES met an indefinite preconditioner, (r, M^-1 r) = %g in iteration %d (point Jacobi of an indefinite matrix: ks_st_pc_jacobi_set_use_abs)", hs->bz, hs->its);
    default: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: MINRES met not a number in iteration %d ((v, P v) = %g, (r, M^-1 r) = %g, residual %g)", hs->its, hs->alfa, hs->bz, phibar);
  }
}
