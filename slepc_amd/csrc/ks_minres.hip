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
// The scalars never leave the device (ks_ksp_resident.cuh: the state block, its gate, who may write what, the ranks, the host's batches). An iteration is
// three row sweeps of this file around the existing product (and, for the preconditioners that are not pointwise, the existing application and the dot sweep):
//     alfa      partials of (v, t), t = u - (beta / oldb) r1 formed in registers and not stored; with a P applied term by term, u = A v - sigma (B v | v)
//               is formed and stored in the same sweep                                                                    3 passes (v, u, r1)
//     lanczos   sums those partials; r_new = t - (alfa / beta) r2, the same t, into r1's buffer; z = dinv .* r_new; partials of (r_new, z)
//                                                                                                                         5 passes (u, r1, r2, r_new, z) + dinv
//     update    sums (r_new, z), the rotation, w_new = (v - oldeps w1 - delta w2) / gamma into w1's buffer, y += phi w_new, v = z / beta for the
//               next product; decides whether the solve has ended                                                          8 passes (v, w1, w2, w_new, y, y, z, v)
// The residuals live in two buffers and the directions in two, both rotated by the parity of the iteration index, which the host knows when it
// enqueues: an iteration either runs as the one it was enqueued as or not at all. Seven work vectors: v, u, two residuals, z, two directions.
// The (v,u) dot takes u after the r1 term, as the algorithm states it; that costs the alfa sweep a read of r1 (16 passes, not 15) and keeps
// tests/minres_cases.py the same operations in the same order. Two collectives per iteration on more than one rank.
//
// What the state adds to the shared rules:
//   rot[2]   cs, sn, dbar, epsln, phibar and beta are read AND rewritten by the update sweep. They are double-buffered by the iteration's parity:
//            iteration i reads rot[i & 1] and its update writes rot[(i + 1) & 1], which no workgroup of that launch reads. beta of rot[(i + 1) & 1]
//            is oldb to iteration i + 1 until that iteration's update overwrites it - the last launch of the iteration, which does not read oldb.
//   alfa     written by the lanczos sweep, read by the update sweep behind it. tol, beta1: written by the start sweep, read by the updates.
//   conv     the update sweep ends the solve (converged, max_it) after its vector work; the alfa sweep is the first of the next iteration.
#include "ks_ksp_resident.cuh"
#include <cfloat>

using namespace ksk;

enum { KS_MINRES_CONVERGED = 1, KS_MINRES_ITS = 2, KS_MINRES_INDEFINITE_PC = 3, KS_MINRES_NAN = 4 };
struct KsMinresRot { double cs, sn, dbar, epsln, phibar, beta; };
struct KsMinresState { KsKspHead h; KsMinresRot rot[2]; double alfa, bz, beta1, tol; };

namespace {

// start: beta1 from the partials of (b, z), the verdict on the right-hand side, the scalars of iteration 0, v = z / beta1
template <int VEC>
__global__ __launch_bounds__(SW_BLOCK) void k_minres_start(KsMinresState *__restrict__ st, const double *__restrict__ red, const double *__restrict__ part, int nblocks,
                                                           double rtol, int n, const double *__restrict__ z, double *__restrict__ v)
{
  __shared__ double c[1];
  ksp_sums(red, part, nblocks, 1, c);
  const double bz = c[0];
  const double beta1 = sqrt(bz);
  int reason = 0;
  if (!isfinite(bz)) reason = KS_MINRES_NAN;
  else if (bz < 0.0) reason = KS_MINRES_INDEFINITE_PC;
  else if (beta1 == 0.0) reason = KS_MINRES_CONVERGED;                 // a zero right-hand side: y = 0 and no iteration
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    KsMinresRot r; r.cs = -1.0; r.sn = 0.0; r.dbar = 0.0; r.epsln = 0.0; r.phibar = reason ? 0.0 : beta1; r.beta = beta1;
    st->rot[0] = r; st->bz = bz; st->beta1 = beta1; st->tol = fmax(rtol * beta1, 1e-50);
    if (reason) ksp_end(&st->h, reason);
  }
  if (reason) return;
  ksp_rows<VEC>(n, [&](long long i, auto width) {
    constexpr int W = decltype(width)::value;
    row_store(v + i, row_div(row_load<W>(z + i), beta1));
  });
}

// alfa: partials of (v, t), t = u - (beta / oldb) r1 (FIRST: t = u); COMBINE: u += b x first (the second term of a P that is applied term by term:
// x = B v, or v itself for the identity). par: the parity of the iteration
template <int VEC, bool COMBINE, bool FIRST>
__global__ __launch_bounds__(SW_BLOCK) void k_minres_alfa(KsMinresState *__restrict__ st, int par, int n, const double *__restrict__ v, double *__restrict__ u, double b,
                                                          const double *__restrict__ x, const double *__restrict__ r1, double *__restrict__ part)
{
  if (ksp_gate<true>(&st->h)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { st->h.gated++; __atomic_store_n(&st->h.done, 1, __ATOMIC_RELAXED); }
    return;
  }
  const double c = FIRST ? 0.0 : st->rot[par].beta / st->rot[par ^ 1].beta;
  double acc[1] = {0.0};
  ksp_rows<VEC>(n, [&](long long i, auto width) {
    constexpr int W = decltype(width)::value;
    const Rows<W> vv = row_load<W>(v + i);
    Rows<W> uv = row_load<W>(u + i);
    if (COMBINE) { uv = row_fma(b, row_load<W>(x + i), uv); row_store(u + i, uv); }
    if (!FIRST) uv = row_fma(-c, row_load<W>(r1 + i), uv);
    row_dot(vv, uv, acc[0]);
  });
  block_write_partials<1>(acc, 1, part);
}

// lanczos: alfa from the partials, r_new = (u - (beta / oldb) r1) - (alfa / beta) r2 into r1's buffer; PC 0: z is r_new itself (no preconditioner), 1: z = dinv .* r_new,
// both with the partials of (r_new, z); 2: the sweep ends after r_new (the preconditioner's own kernels make z, the dot sweep the partials)
template <int VEC, int PC, bool FIRST>
__global__ __launch_bounds__(SW_BLOCK) void k_minres_lanczos(KsMinresState *__restrict__ st, int par, const double *__restrict__ red, const double *__restrict__ part_a, int nblocks, int n,
                                                             const double *__restrict__ u, const double *__restrict__ r2, double *__restrict__ r1, const double *__restrict__ dinv,
                                                             double *__restrict__ z, double *__restrict__ part)
{
  if (ksp_gate<false>(&st->h)) return;
  __shared__ double s[1];
  ksp_sums(red, part_a, nblocks, 1, s);
  const double alfa = s[0];
  const double beta = st->rot[par].beta;
  const int reason = !isfinite(alfa) ? KS_MINRES_NAN : 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->alfa = alfa;
    if (reason) ksp_end(&st->h, reason);
  }
  if (reason) return;
  const double c = FIRST ? 0.0 : beta / st->rot[par ^ 1].beta, a = alfa / beta;
  double acc[1] = {0.0};
  ksp_rows<VEC>(n, [&](long long i, auto width) {
    constexpr int W = decltype(width)::value;
    Rows<W> rn = row_load<W>(u + i);
    const Rows<W> r2v = row_load<W>(r2 + i);
    if (!FIRST) rn = row_fma(-c, row_load<W>(r1 + i), rn);
    rn = row_fma(-a, r2v, rn);
    row_store(r1 + i, rn);
    if (PC != 2) {
      Rows<W> zv = rn;
      if (PC == 1) { zv = row_mul(row_load<W>(dinv + i), rn); row_store(z + i, zv); }
      row_dot(rn, zv, acc[0]);
    }
  });
  if (PC != 2) block_write_partials<1>(acc, 1, part);
}

// update: beta from the partials of (r_new, z), the rotation, w_new = (v - oldeps w1 - delta w2) / gamma into w1's buffer, y += phi w_new, v = z / beta; the end of the solve
template <int VEC>
__global__ __launch_bounds__(SW_BLOCK) void k_minres_update(KsMinresState *__restrict__ st, int par, const double *__restrict__ red, const double *__restrict__ part_b, int nblocks,
                                                            int max_it, int n, const double *__restrict__ z, double *__restrict__ v, const double *__restrict__ w2,
                                                            double *__restrict__ w1, double *__restrict__ y)
{
  if (ksp_gate<false>(&st->h)) return;
  __shared__ double s[1];
  ksp_sums(red, part_b, nblocks, 1, s);
  const double bz = s[0];
  const int reason = !isfinite(bz) ? KS_MINRES_NAN : (bz < 0.0 ? KS_MINRES_INDEFINITE_PC : 0);
  const bool book = blockIdx.x == 0 && threadIdx.x == 0;
  if (reason) {
    if (book) { st->bz = bz; ksp_end(&st->h, reason); }
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
    const int its = st->h.its + 1;
    st->rot[par ^ 1] = r; st->bz = bz; st->h.its = its;
    const int end = r.phibar <= st->tol ? KS_MINRES_CONVERGED : (its >= max_it ? KS_MINRES_ITS : 0);
    if (end) { st->h.reason = end; __atomic_store_n(&st->h.conv, 1, __ATOMIC_RELAXED); }      // after this sweep's work: read by the next launches only
  }
  const bool next = beta > 0.0;                 // beta == 0: the lucky breakdown, phibar = 0 and the solve has converged; there is no next v
  ksp_rows<VEC>(n, [&](long long i, auto width) {
    constexpr int W = decltype(width)::value;
    const Rows<W> vv = row_load<W>(v + i), w1v = row_load<W>(w1 + i), w2v = row_load<W>(w2 + i), zv = row_load<W>(z + i);
    const Rows<W> wn = row_div(row_fma(-delta, w2v, row_fma(-oldeps, w1v, vv)), gamma);
    const Rows<W> yv = row_fma(phi, wn, row_load<W>(y + i));
    row_store(w1 + i, wn);
    row_store(y + i, yv);
    if (next) row_store(v + i, row_div(zv, beta));
  });
}

// one solve's device arrays
struct Minres : KspResident<KsMinresState> {
  double *part_a, *part_b, *v, *u, *R[2], *z, *W[2], *y;      // pc 0: z is the newest residual, no buffer of its own

  int dot(const double *r, const double *zz) { return dots<1>((r == zz ? 8.0 : 16.0) * n, r, zz, part_b, red + 1); }
  int start(double rtol, const double *zz)
  {
    KsProfScope ps(ctx, KS_K_OTHER, 16.0 * n);
    const double *rd = multi ? red + 1 : nullptr;
    return width(v2, [&](auto VEC) { return launch(k_minres_start<decltype(VEC)::value>, grid, state, rd, part_b, grid, rtol, n, zz, v); });
  }
  // x: the term of P still to be added to u, u += b x (NULL: u is complete)
  int alfa(int it, const double *x, double b)
  {
    {
      const bool first = it == 0; const int par = it & 1;
      KsProfScope ps(ctx, KS_K_OTHER, ((first ? 16.0 : 24.0) + (x ? (x == v ? 8.0 : 16.0) : 0.0)) * n);
      KS_CALL(width(v2 && (!x || aligned16(x)), [&](auto VEC) {
        return ksp_flag(x != nullptr, [&](auto COMBINE) {
          return ksp_flag(first, [&](auto FIRST) {
            return launch(k_minres_alfa<decltype(VEC)::value, decltype(COMBINE)::value, decltype(FIRST)::value>, grid, state, par, n, v, u, b, x, R[par], part_a);
          });
        });
      }));
    }
    return collect<1>(part_a, red);
  }
  int lanczos(int it)
  {
    const bool first = it == 0; const int par = it & 1;
    double *rn = R[par];                        // r1's buffer takes the new residual
    {
      KsProfScope ps(ctx, KS_K_OTHER, ((first ? 24.0 : 32.0) + (pc == 1 ? 16.0 : 0.0)) * n);
      const double *rd = multi ? red : nullptr;
      KS_CALL(width(v2, [&](auto VEC) {
        return ksp_pick<0, 1, 2>(pc, [&](auto PC) {
          return ksp_flag(first, [&](auto FIRST) {
            return launch(k_minres_lanczos<decltype(VEC)::value, decltype(PC)::value, decltype(FIRST)::value>, grid, state, par, rd, part_a, grid, n, u, R[par ^ 1], rn, dinv, z, part_b);
          });
        });
      }));
    }
    if (pc == 2) { KS_CALL(ks_st_blocks_apply(st, rn, z, tr)); return dot(rn, z); }
    return collect<1>(part_b, red + 1);
  }
  int update(int it, int max_it)
  {
    const int par = it & 1;
    const double *zz = pc == 0 ? R[par] : z;
    KsProfScope ps(ctx, KS_K_OTHER, 64.0 * n);
    const double *rd = multi ? red + 1 : nullptr;
    // w2 (the last direction) is in W[par ^ 1], w1 (the one before) in W[par], which takes the new one
    return width(v2, [&](auto VEC) { return launch(k_minres_update<decltype(VEC)::value>, grid, state, par, rd, part_b, grid, max_it, n, zz, v, W[par ^ 1], W[par], y); });
  }
};

} // namespace

int ks_ksp_minres(const KsKsp &k, ks_st st, bool tr, const double *rhs, double *y)
{
  ks_ctx ctx = k.ctx;
  Minres s;
  KS_CALL(s.init(k, st, &st->mr, tr));
  s.part_a = s.part; s.part_b = s.part + (size_t)KS_MAX_BLOCKS;
  s.v = ks_bv_col(k.Kb, 0); s.u = ks_bv_col(k.Kb, 1); s.R[0] = ks_bv_col(k.Kb, 2); s.R[1] = ks_bv_col(k.Kb, 3); s.z = ks_bv_col(k.Kb, 4);
  s.W[0] = ks_bv_col(k.Kb, 5); s.W[1] = ks_bv_col(k.Kb, 6); s.y = y;
  s.v2 = s.v2 && aligned16(s.v) && aligned16(s.u) && aligned16(s.R[0]) && aligned16(s.R[1]) && aligned16(s.z) && aligned16(s.W[0]) && aligned16(s.W[1]) && aligned16(y);
  (*k.solves)++;
  KS_CALL(s.zero(y));
  if (k.n > 0) {                                                       // w = w2 = 0
    KS_HIP(hipMemsetAsync(s.W[0], 0, sizeof(double) * (size_t)k.n, ctx->stream));
    KS_HIP(hipMemsetAsync(s.W[1], 0, sizeof(double) * (size_t)k.n, ctx->stream));
  }
  KS_CALL(ksk_copy(ctx, rhs, s.R[1], (size_t)k.n));                    // r2 of iteration 0; r1 is not read there
  const double *z0 = s.R[1];
  if (s.pc == 1) { KS_CALL(ksk_lincomb(ctx, k.n, s.dinv, 1.0, s.R[1], 0.0, nullptr, s.z)); z0 = s.z; }
  else if (s.pc == 2) { KS_CALL(ks_st_blocks_apply(st, s.R[1], s.z, tr)); z0 = s.z; }
  KS_CALL(s.dot(s.R[1], z0));
  KS_CALL(s.start(k.rtol, z0));
  const KsMinresState *hs = nullptr;
  int it = 0;
  KS_CALL(s.run([&]() {
    const double *x = nullptr; double b = 0.0;
    KS_CALL(ks_st_product_one_term_left(st, tr, s.v, s.u, &x, &b));
    KS_CALL(s.alfa(it, x, b));
    KS_CALL(s.lanczos(it));
    return s.update(it++, k.max_it);
  }, &hs));
  const int its = hs->h.its;
  const double phibar = hs->rot[its & 1].phibar;                       // the rotation the last completed iteration left
  *k.its += its; *k.last_rnorm = phibar;
  if (hs->h.reason == KS_MINRES_CONVERGED || !k.strict) return KS_SUCCESS;
  switch (hs->h.reason) {
    case KS_MINRES_ITS: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: MINRES reached %d iterations, residual %g > %g", its, phibar, hs->tol);
    case KS_MINRES_INDEFINITE_PC: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: MINRES met an indefinite preconditioner, (r, M^-1 r) = %g in iteration %d (point Jacobi of an indefinite matrix: ks_st_pc_jacobi_set_use_abs)", hs->bz, its);
    default: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: MINRES met not a number in iteration %d ((v, P v) = %g, (r, M^-1 r) = %g, residual %g)", its, hs->alfa, hs->bz, phibar);
  }
}
