// BiCGStab(l) for the ST's inner solves (KS_KSP_BCGSL): the method of Sleijpen and Fokkema (BiCGstab(l) for linear equations involving unsymmetric
// matrices with complex spectrum, ETNA 1, 1993) with the preconditioner on the left, A^ = M^-1 P, and the preconditioned residual as the norm that is
// tested, written from the paper (PETSc's KSPBCGSL is external to the reference). l BiCG steps, then one minimum-residual polynomial of degree l:
//     y = 0; r_0 = M^-1 b; rt = r_0; u_0 = 0; rho0 = 1; alpha = 0; omega = 1; dp0 = ||r_0||; tol = max(rtol dp0, 1e-50)      (dp0 == 0: y = 0, no iteration)
//     cycle:  converged when ||r_0|| <= tol; "reached %d iterations" when its >= max_it                            (both tested at the start of a cycle only)
//             rho0 = -omega rho0
//             for j = 0 .. l-1:  rho1 = (r_j, rt); beta = alpha (rho1 / rho0); rho0 = rho1;  u_i = r_i - beta u_i (i <= j);  u_{j+1} = A^ u_j
//                                sigma = (u_{j+1}, rt); alpha = rho1 / sigma;  y += alpha u_0;  r_i -= alpha u_{i+1} (i <= j);  r_{j+1} = A^ r_j;  its++
//             G = [r_0 .. r_l]^T [r_0 .. r_l];  gamma = argmin ||r_0 - sum_j gamma_j r_j||  (Cholesky of G(1:l,1:l), right-hand side G(1:l,0))
//             y += sum gamma_j r_{j-1};  r_0 -= sum gamma_j r_j;  u_0 -= sum gamma_j u_j;  omega = gamma_l
// Not built: PETSc's convex polynomial, its `delta` residual replacement and the pseudo-inverse of a singular minimum-residual step.
// The scalars never leave the device (ks_ksp_resident.cuh: the state block, its gate, who may write what, the ranks, the host's batches; the host enqueues
// whole cycles). A BiCG step j is four row sweeps of this file around two products, a cycle ends with two more (n: rows, passes of 8 n bytes):
//     dir<j>     sums (r_j, rt) - j = 0: and (r_0, r_0), the verdict on the iterate -, u_i = r_i - beta u_i, i <= j                     3 (j + 1) passes
//     apply      behind a product: w += b x (a P applied term by term), w = dinv .* w (point Jacobi), partials of (w, rt)            2 to 5 passes
//                a block preconditioner: the product goes to the scratch column, its own kernels make w, the dot sweep the partials
//     step<j>    sums (u_{j+1}, rt), alpha, y += alpha u_0, r_i -= alpha u_{i+1}, i <= j                                            3 j + 6 passes
//     apply      r_{j+1} = A^ r_j and the partials of (r_{j+1}, rt), the rho1 of step j + 1
//     gram<l>    one read of r_0..r_l, (l + 1)(l + 2) / 2 partials                                                                   l + 1 passes
//     mr<l>      sums them, the Cholesky factorisation and the two triangular solves in registers, the three updates, partials of (r_0, rt) and
//                (r_0, r_0) for the next cycle                                                                                       2 l + 7 passes
// Every verdict comes before the vector work of its sweep: the state's `conv` stays zero.
//
// What the state adds to the shared rules:
//   rho0[2]   read AND rewritten by the dir sweep. Double-buffered by the parity of the global step index g = l cycle + j, which the host knows when it
//             enqueues: dir reads rho0[g & 1] and writes rho1 to rho0[(g + 1) & 1], where the step sweep behind it reads it.
//   alpha     written by the step sweep, read by the dir sweep of the next step; omega: written by mr, read by dir<0> of the next cycle; tol: written by
//             dir<0> of cycle 0 and read by the later ones; h.its: written by step, read by dir<0>. None is read in the launch that writes it.
#include "ks_ksp_resident.cuh"

using namespace ksk;

enum { KS_BCGSL_CONVERGED = 1, KS_BCGSL_ITS = 2, KS_BCGSL_BREAKDOWN = 3, KS_BCGSL_SINGULAR = 4, KS_BCGSL_NAN = 5 };
// written by thread 0 of workgroup 0 of the dir, step and mr sweeps; rho1, sigma, pivot: what the sweep that ended the solve saw, for the message
struct KsBcgslState { KsKspHead h; double rho0[2]; double alpha, omega, tol, dp, rho0_used, rho1, sigma, pivot; };
constexpr int BL_MAX = KS_BCGSL_MAX_ELL;
constexpr int BL_NRED = 3 + (BL_MAX + 1) * (BL_MAX + 2) / 2;
static_assert(BL_NRED == KS_BCGSL_PART_COLS, "one partials column and one sum of the ranks per dot of a cycle's widest sweeps");
struct BcgslVecs { double *r[BL_MAX + 1], *u[BL_MAX + 1]; };

namespace {

// dir: rho1 from the partials the sweep before it left, beta, u_i = r_i - beta u_i for i <= J. J = 0 begins a cycle: the verdict on the iterate the
// last minimum-residual step left, tol in cycle 0, rho0 = -omega rho0. par: the parity of the global step index
template <int VEC, int J>
__global__ __launch_bounds__(SW_BLOCK) void k_bcgsl_dir(KsBcgslState *__restrict__ st, int par, const double *__restrict__ red, const double *__restrict__ part, int nblocks,
                                                        double rtol, int max_it, int n, BcgslVecs v)
{
  const bool book = blockIdx.x == 0 && threadIdx.x == 0;
  if (ksp_gate<false>(&st->h)) { if (J == 0 && book) st->h.gated++; return; }
  constexpr int NS = J == 0 ? 2 : 1;
  __shared__ double c[NS];
  ksp_sums<NS>(red, part, nblocks, c);
  const double rho1 = c[0];
  const int its = st->h.its;
  const bool first = J == 0 && its == 0;
  const double alpha = first ? 0.0 : st->alpha;
  const double rho0 = first ? -1.0 : (J == 0 ? -st->omega * st->rho0[par] : st->rho0[par]);
  double dp = 0.0, tol = 0.0;
  int reason = 0;
  if (J == 0) {
    dp = sqrt(c[NS - 1]);
    tol = first ? fmax(rtol * dp, 1e-50) : st->tol;
    if (!isfinite(dp) || !isfinite(rho1) || !isfinite(rho0)) reason = KS_BCGSL_NAN;
    else if (dp <= tol) reason = KS_BCGSL_CONVERGED;                   // a zero right-hand side ends here, before the first step
    else if (its >= max_it) reason = KS_BCGSL_ITS;
    else if (rho0 == 0.0) reason = KS_BCGSL_BREAKDOWN;
  } else {
    if (!isfinite(rho1)) reason = KS_BCGSL_NAN;
    else if (rho0 == 0.0) reason = KS_BCGSL_BREAKDOWN;
  }
  if (book) {
    st->rho1 = rho1; st->rho0_used = rho0;
    if (J == 0) { st->dp = dp; if (first) st->tol = tol; }
    if (reason) ksp_end(&st->h, reason);
    else st->rho0[par ^ 1] = rho1;
  }
  if (reason) return;
  const double beta = alpha * (rho1 / rho0);
  ksp_rows<VEC>(n, [&](long long i, auto width) {
    constexpr int W = decltype(width)::value;
#pragma unroll
    for (int k = 0; k <= J; k++) row_store(v.u[k] + i, row_fma(-beta, row_load<W>(v.u[k] + i), row_load<W>(v.r[k] + i)));
  });
}

// behind a product w = P x but for one term: COMBINE: w += b x2 first (x2 = B x, or x itself for the identity); PC 1: w = dinv .* w; partials of (w, rt).
// PC 2: the combining alone, on the scratch column (the preconditioner's own kernels make the vector, the dot sweep the partials)
template <int VEC, bool COMBINE, int PC>
__global__ __launch_bounds__(SW_BLOCK) void k_bcgsl_apply(const KsBcgslState *__restrict__ st, int n, double *__restrict__ w, double b, const double *__restrict__ x2,
                                                          const double *__restrict__ dinv, const double *__restrict__ rt, double *__restrict__ part)
{
  if (ksp_gate<false>(&st->h)) return;
  double acc[1] = {0.0};
  ksp_rows<VEC>(n, [&](long long i, auto width) {
    constexpr int W = decltype(width)::value;
    Rows<W> wv = row_load<W>(w + i);
    if (COMBINE) wv = row_fma(b, row_load<W>(x2 + i), wv);
    if (PC == 1) wv = row_mul(row_load<W>(dinv + i), wv);
    if (COMBINE || PC == 1) row_store(w + i, wv);
    if (PC != 2) row_dot(wv, row_load<W>(rt + i), acc[0]);
  });
  if (PC != 2) block_write_partials<1>(acc, 1, part);
}

// step: sigma from the partials of (u_{J+1}, rt), alpha = rho1 / sigma, y += alpha u_0, r_i -= alpha u_{i+1} for i <= J
template <int VEC, int J>
__global__ __launch_bounds__(SW_BLOCK) void k_bcgsl_step(KsBcgslState *__restrict__ st, int par, const double *__restrict__ red, const double *__restrict__ part, int nblocks,
                                                         int n, BcgslVecs v, double *__restrict__ y)
{
  if (ksp_gate<false>(&st->h)) return;
  __shared__ double c[1];
  ksp_sums<1>(red, part, nblocks, c);
  const double sigma = c[0], rho1 = st->rho0[par ^ 1];
  const int reason = !isfinite(sigma) ? KS_BCGSL_NAN : (sigma == 0.0 ? KS_BCGSL_BREAKDOWN : 0);
  const double alpha = rho1 / sigma;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->sigma = sigma;
    if (reason) ksp_end(&st->h, reason);
    else { st->alpha = alpha; st->h.its++; }
  }
  if (reason) return;
  ksp_rows<VEC>(n, [&](long long i, auto width) {
    constexpr int W = decltype(width)::value;
    Rows<W> un = row_load<W>(v.u[0] + i);
    row_store(y + i, row_fma(alpha, un, row_load<W>(y + i)));
#pragma unroll
    for (int k = 0; k <= J; k++) {
      un = row_load<W>(v.u[k + 1] + i);
      row_store(v.r[k] + i, row_fma(-alpha, un, row_load<W>(v.r[k] + i)));
    }
  });
}

// gram: partials of (r_a, r_b), a <= b <= L, row by row of the upper triangle
template <int VEC, int L>
__global__ __launch_bounds__(SW_BLOCK) void k_bcgsl_gram(const KsBcgslState *__restrict__ st, int n, BcgslVecs v, double *__restrict__ part)
{
  if (ksp_gate<false>(&st->h)) return;
  constexpr int NG = (L + 1) * (L + 2) / 2;
  double acc[NG];
#pragma unroll
  for (int k = 0; k < NG; k++) acc[k] = 0.0;
  ksp_rows<VEC>(n, [&](long long i, auto width) {
    constexpr int W = decltype(width)::value;
    Rows<W> rv[L + 1];
#pragma unroll
    for (int a = 0; a <= L; a++) rv[a] = row_load<W>(v.r[a] + i);
    int k = 0;
#pragma unroll
    for (int a = 0; a <= L; a++)
#pragma unroll
      for (int b = a; b <= L; b++) row_dot(rv[a], rv[b], acc[k++]);
  });
  block_write_partials<NG>(acc, NG, part);
}

// mr: every workgroup sums the Gram partials and solves the normal equations of min ||r_0 - sum_j gamma_j r_j|| in registers (Cholesky of G(1:L,1:L),
// explicit fma, the same instructions on the same sums: the same gamma everywhere); then y += sum gamma_j r_{j-1}, r_0 -= sum gamma_j r_j,
// u_0 -= sum gamma_j u_j and the partials of (r_0, rt) and (r_0, r_0) for the dir<0> of the next cycle
template <int VEC, int L>
__global__ __launch_bounds__(SW_BLOCK) void k_bcgsl_mr(KsBcgslState *__restrict__ st, const double *__restrict__ red, const double *__restrict__ part_g, int nblocks, int n,
                                                       BcgslVecs v, const double *__restrict__ rt, double *__restrict__ y, double *__restrict__ part)
{
  if (ksp_gate<false>(&st->h)) return;
  constexpr int NG = (L + 1) * (L + 2) / 2;
  __shared__ double c[NG];
  ksp_sums<NG>(red, part_g, nblocks, c);
  double G[L + 1][L + 1];
  {
    int k = 0;
#pragma unroll
    for (int a = 0; a <= L; a++)
#pragma unroll
      for (int b = a; b <= L; b++) { G[a][b] = c[k]; G[b][a] = c[k]; k++; }
  }
  double C[L][L], gamma[L], pivot = 0.0;
  int reason = 0;
#pragma unroll
  for (int j = 0; j < L; j++) {
#pragma unroll
    for (int i = j; i < L; i++) {
      double s = G[i + 1][j + 1];
#pragma unroll
      for (int k = 0; k < j; k++) s = fma(-C[i][k], C[j][k], s);
      if (i == j) {
        if (!reason) { pivot = s; reason = !isfinite(s) ? KS_BCGSL_NAN : (s <= 0.0 ? KS_BCGSL_SINGULAR : 0); }
        C[j][j] = sqrt(s);
      } else C[i][j] = s / C[j][j];
    }
  }
#pragma unroll
  for (int i = 0; i < L; i++) {                                          // C w = G(1:L,0)
    double s = G[i + 1][0];
#pragma unroll
    for (int k = 0; k < i; k++) s = fma(-C[i][k], gamma[k], s);
    gamma[i] = s / C[i][i];
  }
#pragma unroll
  for (int i = L - 1; i >= 0; i--) {                                     // C^T gamma = w
    double s = gamma[i];
#pragma unroll
    for (int k = i + 1; k < L; k++) s = fma(-C[k][i], gamma[k], s);
    gamma[i] = s / C[i][i];
  }
  if (!reason) {
#pragma unroll
    for (int i = 0; i < L; i++) if (!isfinite(gamma[i])) reason = KS_BCGSL_NAN;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->pivot = pivot;
    if (reason) ksp_end(&st->h, reason);
    else st->omega = gamma[L - 1];
  }
  if (reason) return;
  double acc[2] = {0.0, 0.0};
  ksp_rows<VEC>(n, [&](long long i, auto width) {
    constexpr int W = decltype(width)::value;
    Rows<W> yv = row_load<W>(y + i), r0 = row_load<W>(v.r[0] + i), prev = r0;
#pragma unroll
    for (int j = 1; j <= L; j++) {
      const Rows<W> rj = row_load<W>(v.r[j] + i);
      yv = row_fma(gamma[j - 1], prev, yv);
      r0 = row_fma(-gamma[j - 1], rj, r0);
      prev = rj;
    }
    row_store(y + i, yv);
    row_store(v.r[0] + i, r0);
    Rows<W> u0 = row_load<W>(v.u[0] + i);
#pragma unroll
    for (int j = 1; j <= L; j++) u0 = row_fma(-gamma[j - 1], row_load<W>(v.u[j] + i), u0);
    row_store(v.u[0] + i, u0);
    row_dot(row_load<W>(rt + i), r0, acc[0]);
    row_dot(r0, r0, acc[1]);
  });
  block_write_partials<2>(acc, 2, part);
}

// one solve's device arrays. Partials columns and the ranks' sums alike: 0, 1: (r_0, rt) and (r_0, r_0); 2: the dot an apply leaves; 3..: the Gram matrix
struct Bcgsl : KspResident<KsBcgslState, KS_BCGSL_HEAD_BYTES, KS_BCGSL_PART_COLS, BL_NRED> {
  double *part_rr, *part_d, *part_g, *rt, *scr, *y; BcgslVecs v; int L; long long g;

  const double *sums(int at) const { return multi ? red + at : nullptr; }
  int dots_rr() { return KspResident::dots<2>(16.0 * n, rt, v.r[0], part_rr, red); }
  int dir(int j, double rtol, int max_it)
  {
    KsProfScope ps(ctx, KS_K_OTHER, 24.0 * (j + 1) * n);
    return width(v2, [&](auto VEC) {
      return ksp_pick<0, 1, 2, 3>(j, [&](auto J) {
        constexpr int JJ = decltype(J)::value;
        return launch(k_bcgsl_dir<decltype(VEC)::value, JJ>, grid, state, (int)(g & 1), sums(JJ == 0 ? 0 : 2), JJ == 0 ? part_rr : part_d, grid, rtol, max_it, n, v);
      });
    });
  }
  // out = M^-1 P x and the partials of (out, rt)
  int apply(const double *x, double *out)
  {
    double *w = pc == 2 ? scr : out;
    const double *x2 = nullptr; double b = 0.0;
    KS_CALL(ks_st_product_one_term_left(st, tr, x, w, &x2, &b));
    if (pc != 2 || x2) {
      const double passes = (pc == 2 ? 2.0 : (x2 || pc == 1 ? 3.0 : 2.0)) + (x2 ? 1.0 : 0.0) + (pc == 1 ? 1.0 : 0.0);
      KsProfScope ps(ctx, KS_K_OTHER, 8.0 * passes * n);
      KS_CALL(width(v2 && (!x2 || aligned16(x2)), [&](auto VEC) {
        return ksp_flag(x2 != nullptr, [&](auto COMBINE) {
          return ksp_pick<0, 1, 2>(pc, [&](auto PC) {
            return launch(k_bcgsl_apply<decltype(VEC)::value, decltype(COMBINE)::value, decltype(PC)::value>, grid, state, n, w, b, x2, dinv, rt, part_d);
          });
        });
      }));
    }
    if (pc == 2) { KS_CALL(ks_st_blocks_apply(st, w, out, tr)); return KspResident::dots<1>(16.0 * n, rt, out, part_d, red + 2); }
    return collect<1>(part_d, red + 2);
  }
  int step(int j)
  {
    KsProfScope ps(ctx, KS_K_OTHER, 8.0 * (3 * j + 6) * n);
    return width(v2, [&](auto VEC) {
      return ksp_pick<0, 1, 2, 3>(j, [&](auto J) { return launch(k_bcgsl_step<decltype(VEC)::value, decltype(J)::value>, grid, state, (int)(g & 1), sums(2), part_d, grid, n, v, y); });
    });
  }
  int gram()
  {
    return ksp_pick<1, 2, 3, 4>(L, [&](auto LL) {
      constexpr int NG = (decltype(LL)::value + 1) * (decltype(LL)::value + 2) / 2;
      {
        KsProfScope ps(ctx, KS_K_OTHER, 8.0 * (L + 1) * n);
        KS_CALL(width(v2, [&](auto VEC) { return launch(k_bcgsl_gram<decltype(VEC)::value, decltype(LL)::value>, grid, state, n, v, part_g); }));
      }
      return collect<NG>(part_g, red + 3);
    });
  }
  int mr()
  {
    {
      KsProfScope ps(ctx, KS_K_OTHER, 8.0 * (2 * L + 7) * n);
      KS_CALL(width(v2, [&](auto VEC) {
        return ksp_pick<1, 2, 3, 4>(L, [&](auto LL) { return launch(k_bcgsl_mr<decltype(VEC)::value, decltype(LL)::value>, grid, state, sums(3), part_g, grid, n, v, rt, y, part_rr); });
      }));
    }
    return collect<2>(part_rr, red);
  }
};

} // namespace

int ks_ksp_bcgsl(const KsKsp &k, ks_st st, bool tr, const double *rhs, double *y)
{
  ks_ctx ctx = k.ctx;
  Bcgsl s;
  KS_CALL(s.init(k, st, &st->bl, tr));
  const int L = st->bcgsl_ell;
  s.L = L; s.g = 0; s.y = y;
  s.part_rr = s.part; s.part_d = s.part + 2 * (size_t)KS_MAX_BLOCKS; s.part_g = s.part + 3 * (size_t)KS_MAX_BLOCKS;
  for (int j = 0; j <= BL_MAX; j++) { s.v.r[j] = ks_bv_col(st->Kl, std::min(j, L)); s.v.u[j] = ks_bv_col(st->Kl, L + 1 + std::min(j, L)); }
  s.rt = ks_bv_col(st->Kl, 2 * L + 2); s.scr = ks_bv_col(st->Kl, 2 * L + 3);
  s.v2 = s.v2 && aligned16(y) && aligned16(s.rt) && aligned16(s.scr);
  for (int j = 0; j <= L; j++) s.v2 = s.v2 && aligned16(s.v.r[j]) && aligned16(s.v.u[j]);
  (*k.solves)++;
  KS_CALL(s.zero(y));
  double *r0 = s.v.r[0];
  if (s.pc == 0) KS_CALL(ksk_copy(ctx, rhs, r0, (size_t)k.n));                                  // r_0 = M^-1 b
  else if (s.pc == 1) KS_CALL(ksk_lincomb(ctx, k.n, s.dinv, 1.0, rhs, 0.0, nullptr, r0));
  else KS_CALL(ks_st_blocks_apply(st, rhs, r0, tr));
  KS_CALL(ksk_copy(ctx, r0, s.rt, (size_t)k.n));
  if (k.n > 0) { KS_HIP(hipMemsetAsync(s.v.u[0], 0, sizeof(double) * (size_t)k.n, ctx->stream)); }  // u_0 = 0
  KS_CALL(s.dots_rr());
  const KsBcgslState *hs = nullptr;
  KS_CALL(s.run([&]() {                                                                         // one cycle
    for (int j = 0; j < L; j++, s.g++) {
      KS_CALL(s.dir(j, k.rtol, k.max_it));
      KS_CALL(s.apply(s.v.u[j], s.v.u[j + 1]));
      KS_CALL(s.step(j));
      KS_CALL(s.apply(s.v.r[j], s.v.r[j + 1]));
    }
    KS_CALL(s.gram());
    return s.mr();
  }, &hs));
  const int its = hs->h.its;
  *k.its += its; *k.last_rnorm = hs->dp;
  if (hs->h.reason == KS_BCGSL_CONVERGED || !k.strict) return KS_SUCCESS;
  switch (hs->h.reason) {
    case KS_BCGSL_ITS: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: BiCGStab(%d) reached %d iterations, preconditioned residual %g > %g", L, its, hs->dp, hs->tol);
    case KS_BCGSL_BREAKDOWN: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: BiCGStab(%d) breakdown in iteration %d (rho0 = %g, rho1 = %g, last sigma = %g)", L, its, hs->rho0_used, hs->rho1, hs->sigma);
    case KS_BCGSL_SINGULAR: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: BiCGStab(%d) met a singular minimum-residual step after iteration %d (Cholesky pivot %g)", L, its, hs->pivot);
    default: KS_FAIL(KS_ERR_NOT_CONVERGED, "KSPSolve has not converged: BiCGStab(%d) met not a number in iteration %d (rho1 = %g, sigma = %g, pivot %g, residual %g)", L, its, hs->rho1, hs->sigma, hs->pivot, hs->dp);
  }
}
