// Conjugate gradients for the ST's inner solves (KS_KSP_CG): KSPCG with a left preconditioner and its default norm, the preconditioned residual,
// written from the algorithm (PETSc's KSP is external to the reference):
//     y = 0, r = b, z = M^-1 r, dp0 = ||z||, tol = max(rtol dp0, 1e-50)
//     iteration i:  gamma = (r,z);  p = z (i = 0) or z + (gamma / gamma_old) p;  w = P p;  delta = (p,w);  alpha = gamma / delta
//                   y += alpha p;  r -= alpha w;  z = M^-1 r;  dp = ||z||;  converged when dp <= tol
// The scalars never leave the device (ks_ksp_resident.cuh: the state block, its gate, who may write what, the ranks, the host's batches). An iteration is
// three row sweeps of this file around the existing product (and, for the preconditioners that are not pointwise, the existing application and the dot sweep):
//     direction   sums the partials of (r,z) and (z,z) the sweep before it left, decides whether the solve has ended, p = z + beta p
//     (p,w)       partials of (p,w); with a P applied term by term, w = A p - sigma (B p | p) is formed in the same sweep
//     update      sums the partials of (p,w), y += alpha p, r -= alpha w, z = dinv .* r, partials of (r,z) and (z,z)
// Every verdict comes before the vector work of its sweep: the state's `conv` stays zero.
#include "ks_ksp_resident.cuh"

using namespace ksk;

enum { KS_CG_CONVERGED = 1, KS_CG_ITS = 2, KS_CG_INDEFINITE_MAT = 3, KS_CG_INDEFINITE_PC = 4, KS_CG_NAN = 5 };
// written by thread 0 of workgroup 0 of the direction and update sweeps, read by every workgroup of the sweeps behind them and, once per batch, by the host
struct KsCgState { KsKspHead h; double gamma, gamma_old, delta, dp, tol; };

namespace {

// direction: the verdict on the iterate the last update left, then p = z + beta p (p = z in the first iteration)
template <int VEC>
__global__ __launch_bounds__(SW_BLOCK) void k_cg_direction(KsCgState *__restrict__ st, const double *__restrict__ red, const double *__restrict__ part, int nblocks,
                                                           double rtol, int max_it, int n, const double *__restrict__ z, double *__restrict__ p)
{
  const bool book = blockIdx.x == 0 && threadIdx.x == 0;
  if (ksp_gate<false>(&st->h)) { if (book) st->h.gated++; return; }
  __shared__ double c[2];
  ksp_sums(red, part, nblocks, 2, c);
  const double gamma = c[0], dp = sqrt(c[1]);
  const int its = st->h.its;
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
    if (reason) ksp_end(&st->h, reason);
  }
  if (reason) return;
  const double beta = first ? 0.0 : gamma / st->gamma_old;
  ksp_rows<VEC>(n, [&](long long i, auto width) {
    constexpr int W = decltype(width)::value;
    Rows<W> zv = row_load<W>(z + i);
    if (!first) zv = row_fma(beta, row_load<W>(p + i), zv);
    row_store(p + i, zv);
  });
}

// partials of (p, w); COMBINE: w += b v first (the second term of a P that is applied term by term: v = B p, or p itself for the identity)
template <int VEC, bool COMBINE>
__global__ __launch_bounds__(SW_BLOCK) void k_cg_pw(const KsCgState *__restrict__ st, int n, const double *__restrict__ p, double *__restrict__ w, double b,
                                                    const double *__restrict__ v, double *__restrict__ part)
{
  if (ksp_gate<false>(&st->h)) return;
  double acc[1] = {0.0};
  ksp_rows<VEC>(n, [&](long long i, auto width) {
    constexpr int W = decltype(width)::value;
    const Rows<W> pv = row_load<W>(p + i);
    Rows<W> wv = row_load<W>(w + i);
    if (COMBINE) { wv = row_fma(b, row_load<W>(v + i), wv); row_store(w + i, wv); }
    row_dot(pv, wv, acc[0]);
  });
  block_write_partials<1>(acc, 1, part);
}

// update: alpha from the partials of (p,w), y += alpha p, r -= alpha w; PC 0: z is r itself (no preconditioner), 1: z = dinv .* r, both with the partials
// of (r,z) and (z,z); 2: the sweep ends after r (the preconditioner's own kernels make z, the dot sweep the partials)
template <int VEC, int PC>
__global__ __launch_bounds__(SW_BLOCK) void k_cg_update(KsCgState *__restrict__ st, const double *__restrict__ red, const double *__restrict__ part_d, int nblocks, int n,
                                                        const double *__restrict__ p, const double *__restrict__ w, const double *__restrict__ dinv,
                                                        double *__restrict__ y, double *__restrict__ r, double *__restrict__ z, double *__restrict__ part)
{
  if (ksp_gate<false>(&st->h)) return;
  __shared__ double c[1];
  ksp_sums(red, part_d, nblocks, 1, c);
  const double delta = c[0], gamma = st->gamma;
  const int reason = !isfinite(delta) ? KS_CG_NAN : (delta <= 0.0 ? KS_CG_INDEFINITE_MAT : 0);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->delta = delta;
    if (reason) ksp_end(&st->h, reason);
    else { st->gamma_old = gamma; st->h.its++; }
  }
  if (reason) return;
  const double alpha = gamma / delta;
  double acc[2] = {0.0, 0.0};
  ksp_rows<VEC>(n, [&](long long i, auto width) {
    constexpr int W = decltype(width)::value;
    const Rows<W> pv = row_load<W>(p + i), wv = row_load<W>(w + i);
    Rows<W> yv = row_load<W>(y + i), rv = row_load<W>(r + i), dv;
    if (PC == 1) dv = row_load<W>(dinv + i);
    yv = row_fma(alpha, pv, yv);
    rv = row_fma(-alpha, wv, rv);
    row_store(y + i, yv);
    row_store(r + i, rv);
    if (PC != 2) {
      Rows<W> zv = rv;
      if (PC == 1) { zv = row_mul(dv, rv); row_store(z + i, zv); }
      row_dot(rv, zv, acc[0]);
      row_dot(zv, zv, acc[1]);
    }
  });
  if (PC != 2) block_write_partials<2>(acc, 2, part);
}

// one solve's device arrays
struct Cg : KspResident<KsCgState> {
  double *part_gz, *part_d, *r, *z, *p, *w, *y;

  int dots() { return KspResident::dots<2>(16.0 * n, r, z, part_gz, red); }
  int direction(double rtol, int max_it)
  {
    KsProfScope ps(ctx, KS_K_OTHER, 24.0 * n);
    const double *rd = multi ? red : nullptr;
    return width(v2, [&](auto VEC) { return launch(k_cg_direction<decltype(VEC)::value>, grid, state, rd, part_gz, grid, rtol, max_it, n, z, p); });
  }
  // v: the term of P still to be added to w, w += b v (NULL: w is complete)
  int pw(const double *v, double b)
  {
    {
      KsProfScope ps(ctx, KS_K_OTHER, (v ? (v == p ? 24.0 : 32.0) : 16.0) * n);
      KS_CALL(width(v2 && (!v || aligned16(v)), [&](auto VEC) {
        return ksp_flag(v != nullptr, [&](auto COMBINE) { return launch(k_cg_pw<decltype(VEC)::value, decltype(COMBINE)::value>, grid, state, n, p, w, b, v, part_d); });
      }));
    }
    return collect<1>(part_d, red + 2);
  }
  int update()
  {
    {
      KsProfScope ps(ctx, KS_K_OTHER, (pc == 0 ? 48.0 : pc == 1 ? 64.0 : 48.0) * n);
      const double *rd = multi ? red + 2 : nullptr;
      KS_CALL(width(v2, [&](auto VEC) {
        return ksp_pick<0, 1, 2>(pc, [&](auto PC) {
          return launch(k_cg_update<decltype(VEC)::value, decltype(PC)::value>, grid, state, rd, part_d, grid, n, p, w, dinv, y, r, z, part_gz);
        });
      }));
    }
    if (pc == 2) { KS_CALL(ks_st_blocks_apply(st, r, z, tr)); return dots(); }
    return collect<2>(part_gz, red);
  }
};

} // namespace

int ks_ksp_cg(const KsKsp &k, ks_st st, bool tr, const double *rhs, double *y)
{
  ks_ctx ctx = k.ctx;
  Cg s;
  KS_CALL(s.init(k, st, &st->cg, tr));
  s.part_gz = s.part; s.part_d = s.part + 2 * (size_t)KS_MAX_BLOCKS;
  s.r = ks_bv_col(k.Kb, 0); s.z = s.pc == 0 ? s.r : ks_bv_col(k.Kb, 1); s.p = ks_bv_col(k.Kb, 2); s.w = ks_bv_col(k.Kb, 3); s.y = y;
  s.v2 = s.v2 && aligned16(s.r) && aligned16(s.z) && aligned16(s.p) && aligned16(s.w) && aligned16(y);
  (*k.solves)++;
  KS_CALL(s.zero(y));
  KS_CALL(ksk_copy(ctx, rhs, s.r, (size_t)k.n));
  if (s.pc == 1) KS_CALL(ksk_lincomb(ctx, k.n, s.dinv, 1.0, s.r, 0.0, nullptr, s.z));
  else if (s.pc == 2) KS_CALL(ks_st_blocks_apply(st, s.r, s.z, tr));
  KS_CALL(s.dots());
  const KsCgState *hs = nullptr;
  KS_CALL(s.run([&]() {
    KS_CALL(s.direction(k.rtol, k.max_it));
    const double *v = nullptr; double b = 0.0;
    KS_CALL(ks_st_product_one_term_left(st, tr, s.p, s.w, &v, &b));
    KS_CALL(s.pw(v, b));
    return s.update();
  }, &hs));
  const int its = hs->h.its;
  *k.its += its; *k.last_rnorm = hs->dp;
  if (hs->h.reason == KS_CG_CONVERGED || !k.strict) return KS_SUCCESS;
  switch (hs->h.reason) {
    case KS_CG_ITS: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: CG reached %d iterations, preconditioned residual %g > %g", its, hs->dp, hs->tol);
    case KS_CG_INDEFINITE_MAT: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: CG met an indefinite matrix, (p, P p) = %g in iteration %d", hs->delta, its);
    case KS_CG_INDEFINITE_PC: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: CG met an indefinite preconditioner, (r, M^-1 r) = %g in iteration %d", hs->gamma, its);
    default: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: CG met not a number in iteration %d ((r, M^-1 r) = %g, (p, P p) = %g, residual %g)", its, hs->gamma, hs->delta, hs->dp);
  }
}
