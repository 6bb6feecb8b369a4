// Generalized Davidson for symmetric (definite) problems: a search basis that grows by a block of preconditioned residuals per iteration, Rayleigh-Ritz
// on it, locking of converged pairs and a thick restart with "+k" vectors of the previous iteration. For users that have a preconditioner but no
// accurate inner solve, want either end of the spectrum or a target with block size 1, or cannot afford the three panels of LOBPCG.
//
// Restates, in this project's structure,
//   EPSSetUp_XD / EPSSolve_XD                   src/eps/impls/davidson/davidson.c:35-189, 191-228
//   dvd_initV_classic_0                         dvdinitv.c:38-62          (the caller's vectors, then random ones, orthonormalised)
//   dvd_calcpairs_proj / _updateproj / _projeig dvdcalcpairs.c:372-521    (A V, B V, the new columns of H, DSSolve + DSSort)
//   dvd_calcpairs_res_0 / _selectPairs          dvdcalcpairs.c:523-600    (Ritz vectors and residuals of the best bs pairs)
//   dvd_improvex_gd2 / GD branch                dvdimprovex.c             (D = M^-1 R)
//   dvd_updateV_extrapol, _conv_gen, _restart_gen, _update_gen, _testConv   dvdupdatev.c:82-356
//   dvd_testconv_slepc_0                        dvdtestconv.c:24-36       (the EPS's convergence test on ||r|| / ||x||)
// Scope: KS_EPS_HEP and KS_EPS_GHEP with a B-orthonormal search basis and Ritz extraction, the reference's defaults for these problem types. The
// projected problem is then a standard symmetric one (DsGd, ks_ds.h). Where this file departs from the reference:
//   - Ritz vectors, A x, B x, the residuals and both norms of the best bs pairs are ONE sweep over V, AV (and BV) and one D2H (k_ritz_residual below)
//     where dvd_calcpairs_res_0 makes two or three BVMult, bs BVMultVec / VecNorm pairs and a host wait each; r = fma(-theta, bx, ax)
//   - one step per iteration: lock, or restart, or expand. The reference expands first and locks in the same call when a pair converged
//     (dvdupdatev.c:334-351); here the converged pairs are locked at once and the expansion follows in the next iteration from the rotated basis
//   - the basis is full when m + bs > mpd or when the locked and active columns plus a block no longer fit in ncv (the reference: k + 2 > ncv,
//     dvdupdatev.c:57, with mpd bounding the restart size only)
//   - non-symmetric problem types, B-orthogonalisation switched off with a B matrix, harmonic extractions, Krylov start, double expansion, the
//     dynamic and fix options are KS_ERR_SUP or absent; block sizes 1..16
//   - D is orthonormalised column by column against the constraints, the locked vectors and V (BVOrthonormalizeColumn); a dependent column is dropped
#include "ksgpu_internal.h"
#include "ks_eps_impl.h"
#include "ks_davidson.h"
#include "ks_sweeps.cuh"
#include <algorithm>

using namespace ksk;

namespace {

struct KsTheta16 { double v[16]; };

// Result columns of one pass, from the register budget. A lane carries x, ax (and bx) of JT columns for two rows, 4 JT (6 JT) doubles, beside the 2 JT
// sums of squares and the loads in flight: in the generalized form JT = 8 is 64 doubles of data, 16 would be 128 - 256 VGPRs before a single
// load or address, past what a wave has with two workgroups per CU - so more than 8 result columns run as a second pass over the three panels
// inside the call; the standard form holds 16 columns (96 doubles) and always makes one pass.
constexpr int GD_JT_GEN = 8, GD_JT_STD = 16;
// basis columns whose loads are issued back to back (2 or 3 KiB per column and wave): four, two in the 16-column form whose 2 x 16 coefficients
// of S per group of columns already fill the scalar registers
template <int JT> struct GdGroup { static constexpr int CU = JT > 8 ? 2 : 4; };

// One sweep over the m active columns of V, AV (and BV, GEN): for j < nc, x_j = V S(:,j), ax_j = AV S(:,j), bx_j = BV S(:,j) (x_j itself without
// BV), R(:,j) = ax_j - theta_j bx_j, and the partial sums of ||R(:,j)||^2 (row j0 + j of `partials`) and ||x_j||^2 (row ncols + j0 + j) of this
// workgroup. Every sum starts at 0 and takes the columns in ascending order with one fma each, so an entry of R depends on its own row alone.
// The tile walk and the block combine are the sweeps' (ks_sweeps.cuh); S is m x nc on the device, column-major with lds = m - its entries are the
// same in every lane, the compiler reads them with scalar loads. JT >= nc is compile-time; the columns past nc repeat the last one and are discarded.
// OUT (ks_bv_ritz_residual_vectors): x_j and B x_j, which the sweep holds in registers, are also stored into X(:,j) and BX(:,j) where those are given
// (B x_j = x_j without BV); the arithmetic of R and of the sums is the same code either way.
template <int JT, int VEC, bool PLAIN, bool GEN, bool OUT>
__global__ __launch_bounds__(SW_BLOCK) void k_ritz_residual(const double *__restrict__ V, long long ldv, const double *__restrict__ AV, long long ldav,
                                                            const double *__restrict__ BV, long long ldbv, int m, const double *__restrict__ S, int lds, int nc,
                                                            KsTheta16 th, double *__restrict__ R, long long ldr, int n, double *__restrict__ partials, int j0, int ncols,
                                                            double *__restrict__ X, long long ldx, double *__restrict__ BX, long long ldbx)
{
  constexpr int JB = GEN ? JT : 1, GD_CU = GdGroup<JT>::CU;
  double accr[JT], accx[JT];
#pragma unroll
  for (int j = 0; j < JT; j++) { accr[j] = 0.0; accx[j] = 0.0; }
  const long long tile = (long long)SW_BLOCK * VEC;
  const long long ntiles = ((long long)n + tile - 1) / tile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long r = t * tile + (long long)threadIdx.x * VEC;
    if (VEC == 2 && r + 1 < n) {
      double2 x[JT], ax[JT], bx[JB];
#pragma unroll
      for (int j = 0; j < JT; j++) { x[j].x = x[j].y = 0.0; ax[j].x = ax[j].y = 0.0; }
#pragma unroll
      for (int j = 0; j < JB; j++) { bx[j].x = bx[j].y = 0.0; }
      int c = 0;
      for (; c + GD_CU <= m; c += GD_CU) {
        double2 v[GD_CU], a[GD_CU], b[GEN ? GD_CU : 1];
#pragma unroll
        for (int u = 0; u < GD_CU; u++) {
          v[u] = ldbasis2<PLAIN>(V + (long long)(c + u) * ldv + r); a[u] = ldbasis2<PLAIN>(AV + (long long)(c + u) * ldav + r);
          if (GEN) b[u] = ldbasis2<PLAIN>(BV + (long long)(c + u) * ldbv + r);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < GD_CU; u++) {
#pragma unroll
          for (int j = 0; j < JT; j++) {
            const double s = S[(size_t)(j < nc ? j : nc - 1) * lds + c + u];
            x[j].x = fma(v[u].x, s, x[j].x); x[j].y = fma(v[u].y, s, x[j].y);
            ax[j].x = fma(a[u].x, s, ax[j].x); ax[j].y = fma(a[u].y, s, ax[j].y);
            if (GEN) { bx[j % JB].x = fma(b[u].x, s, bx[j % JB].x); bx[j % JB].y = fma(b[u].y, s, bx[j % JB].y); }
          }
        }
      }
      for (; c < m; c++) {
        const double2 v = ldbasis2<PLAIN>(V + (long long)c * ldv + r), a = ldbasis2<PLAIN>(AV + (long long)c * ldav + r);
        double2 b; b.x = b.y = 0.0;
        if (GEN) b = ldbasis2<PLAIN>(BV + (long long)c * ldbv + r);
#pragma unroll
        for (int j = 0; j < JT; j++) {
          const double s = S[(size_t)(j < nc ? j : nc - 1) * lds + c];
          x[j].x = fma(v.x, s, x[j].x); x[j].y = fma(v.y, s, x[j].y);
          ax[j].x = fma(a.x, s, ax[j].x); ax[j].y = fma(a.y, s, ax[j].y);
          if (GEN) { bx[j % JB].x = fma(b.x, s, bx[j % JB].x); bx[j % JB].y = fma(b.y, s, bx[j % JB].y); }
        }
      }
#pragma unroll
      for (int j = 0; j < JT; j++) {
        if (j < nc) {
          const double2 bj = GEN ? bx[j % JB] : x[j];
          double2 rv; rv.x = fma(-th.v[j], bj.x, ax[j].x); rv.y = fma(-th.v[j], bj.y, ax[j].y);
          *reinterpret_cast<double2 *>(R + (long long)j * ldr + r) = rv;
          if (OUT) {
            if (X) *reinterpret_cast<double2 *>(X + (long long)j * ldx + r) = x[j];
            if (BX) *reinterpret_cast<double2 *>(BX + (long long)j * ldbx + r) = bj;
          }
          accr[j] = fma(rv.x, rv.x, accr[j]); accr[j] = fma(rv.y, rv.y, accr[j]);
          accx[j] = fma(x[j].x, x[j].x, accx[j]); accx[j] = fma(x[j].y, x[j].y, accx[j]);
        }
      }
    } else {
      for (int u = 0; u < VEC; u++) {
        const long long rr = r + u;
        if (rr < n) {
          double x[JT], ax[JT], bx[JB];
#pragma unroll
          for (int j = 0; j < JT; j++) { x[j] = 0.0; ax[j] = 0.0; }
#pragma unroll
          for (int j = 0; j < JB; j++) bx[j] = 0.0;
          for (int c = 0; c < m; c++) {
            const double v = V[(long long)c * ldv + rr], a = AV[(long long)c * ldav + rr], b = GEN ? BV[(long long)c * ldbv + rr] : 0.0;
#pragma unroll
            for (int j = 0; j < JT; j++) {
              const double s = S[(size_t)(j < nc ? j : nc - 1) * lds + c];
              x[j] = fma(v, s, x[j]); ax[j] = fma(a, s, ax[j]);
              if (GEN) bx[j % JB] = fma(b, s, bx[j % JB]);
            }
          }
#pragma unroll
          for (int j = 0; j < JT; j++) {
            if (j < nc) {
              const double rv = fma(-th.v[j], GEN ? bx[j % JB] : x[j], ax[j]);
              R[(long long)j * ldr + rr] = rv;
              if (OUT) {
                if (X) X[(long long)j * ldx + rr] = x[j];
                if (BX) BX[(long long)j * ldbx + rr] = GEN ? bx[j % JB] : x[j];
              }
              accr[j] = fma(rv, rv, accr[j]); accx[j] = fma(x[j], x[j], accx[j]);
            }
          }
        }
      }
    }
  }
  // one row of `partials` per workgroup and quantity, as block_write_partials lays them out: partials[row * gridDim.x + blockIdx.x]
  __shared__ double red[SW_WAVES][2 * JT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < JT; j++) {
    const double sr = wave_sum(accr[j]), sx = wave_sum(accx[j]);
    if (lane == 0) { red[w][j] = sr; red[w][JT + j] = sx; }
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * JT) {
    const int j = (int)threadIdx.x % JT; const bool isx = (int)threadIdx.x >= JT;
    if (j < nc) {
      double s = red[0][threadIdx.x];
#pragma unroll
      for (int ww = 1; ww < SW_WAVES; ww++) s += red[ww][threadIdx.x];
      partials[(size_t)((isx ? ncols : 0) + j0 + j) * gridDim.x + blockIdx.x] = s;
    }
  }
}

bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

// The sweep with its norms on raw column pointers (the solver's AV and BV start at column 0 where V starts at its first unlocked column). S: host,
// m x ncols with lds >= m, staged compactly in Vs's coefficient scratch. The partial sums go the way of ksl_block_residual: one row per workgroup,
// the fixed-order reduction of this rank's rows, the communicator's allreduce, all 2 ncols values in one copy and one host wait.
} // namespace
int ks_ritz_residual(ks_bv R, double *Rd, ks_bv Vs, const double *Vd, long long ldv, const double *AVd, long long ldav, const double *BVd, long long ldbv, int m,
                     const double *S, int lds, int ncols, const double *theta, double *rnorm, double *xnorm, double *Xd, long long ldx, double *BXd, long long ldbx)
{
  ks_ctx ctx = R->ctx;
  const int n = R->n; const long long ldr = R->ld;
  R->spec.valid = false;                                        // the partials of this BV are rewritten
  double nrm[32];
  if (n > 0) {
    std::vector<double> Sc((size_t)m * ncols);
    for (int j = 0; j < ncols; j++) for (int c = 0; c < m; c++) Sc[(size_t)c + (size_t)j * m] = S[(size_t)c + (size_t)j * lds];
    double *Sdev = nullptr;
    KS_CALL(ksb_stage_coefs(Vs, Sc.data(), Sc.size(), &Sdev));
    const bool gen = BVd != nullptr;
    const bool out = Xd || BXd;
    const bool v2 = ldv % 2 == 0 && ldav % 2 == 0 && (!gen || ldbv % 2 == 0) && ldr % 2 == 0 && aligned16(Vd) && aligned16(AVd) && (!gen || aligned16(BVd)) && aligned16(Rd)
                    && (!Xd || (ldx % 2 == 0 && aligned16(Xd))) && (!BXd || (ldbx % 2 == 0 && aligned16(BXd)));
    const bool plain = ks_basis_loads_plain(ctx, (size_t)(gen ? 3 : 2) * m + ncols, (size_t)R->ld);
    const int grid = ks_sweep_grid_for(ctx, n, v2 ? 2 : 1, nullptr, 2);      // two workgroups per CU: what the registers of the widest form leave room for; the same grid for every pass
    R->last_grid = grid;
    const int jt = gen ? GD_JT_GEN : GD_JT_STD;
    KsProfScope ps(ctx, KS_K_OTHER, 8.0 * n * ((gen ? 3.0 : 2.0) * m * ((ncols + jt - 1) / jt) + ncols));
    for (int j0 = 0; j0 < ncols; j0 += jt) {
      const int nc = std::min(jt, ncols - j0);
      KsTheta16 th; for (int i = 0; i < 16; i++) th.v[i] = i < nc ? theta[j0 + i] : 0.0;
      const double *Sp = Sdev + (size_t)j0 * m; double *Rp = Rd + (size_t)j0 * ldr;
      double *Xp = Xd ? Xd + (size_t)j0 * ldx : nullptr, *BXp = BXd ? BXd + (size_t)j0 * ldbx : nullptr;
#define KSG_LAUNCH_O(JT, VEC, PL, GEN, OUT) hipLaunchKernelGGL((k_ritz_residual<JT, VEC, PL, GEN, OUT>), dim3(grid), dim3(SW_BLOCK), 0, ctx->stream, Vd, ldv, AVd, ldav, BVd, ldbv, m, Sp, m, nc, th, Rp, ldr, n, R->partials, j0, ncols, Xp, ldx, BXp, ldbx)
#define KSG_LAUNCH(JT, VEC, PL, GEN) do { if (out) KSG_LAUNCH_O(JT, VEC, PL, GEN, true); else KSG_LAUNCH_O(JT, VEC, PL, GEN, false); } while (0)
#define KSG_FORM(JT, GEN) do { if (!v2) KSG_LAUNCH(JT, 1, true, GEN); else if (plain) KSG_LAUNCH(JT, 2, true, GEN); else KSG_LAUNCH(JT, 2, false, GEN); } while (0)
#define KSG_JT(JT) do { if (gen) KSG_FORM(JT, true); else KSG_FORM(JT, false); } while (0)
      if (nc <= 1) KSG_JT(1); else if (nc <= 2) KSG_JT(2); else if (nc <= 4) KSG_JT(4); else if (nc <= 8) KSG_JT(8); else KSG_FORM(16, false);
#undef KSG_JT
#undef KSG_FORM
#undef KSG_LAUNCH
#undef KSG_LAUNCH_O
      KS_HIP(hipGetLastError());
    }
    KS_CALL(ksk_reduce_partials(R, 2 * ncols, R->coef));
  } else KS_HIP(hipMemsetAsync(R->coef, 0, sizeof(double) * 2 * ncols, ctx->stream));
  KS_CALL(ks_allreduce_sum(ctx, R->coef, 2 * ncols));
  KS_HIP(hipMemcpyAsync(nrm, R->coef, sizeof(double) * 2 * ncols, hipMemcpyDeviceToHost, ctx->stream));
  KS_HIP(ks_sync(ctx));
  for (int i = 0; i < ncols; i++) { rnorm[i] = sqrt(nrm[i]); if (xnorm) xnorm[i] = sqrt(nrm[ncols + i]); }
  return KS_SUCCESS;
}

static_assert(GD_JT_GEN == 8 && GD_JT_STD == 16, "the dispatch of ritz_residual compiles the pass widths 1, 2, 4, 8 and, for the standard form, 16");

// the checks of the two entries; X, BX NULL: ks_bv_ritz_residual
static int ritz_residual_entry(ks_bv R, ks_bv V, ks_bv AV, ks_bv BV, const double *S, int lds, int ncols, const double *theta, double *rnorm, double *xnorm, ks_bv X, ks_bv BX)
{
  KS_CHECK(R && V && AV && S && theta && rnorm, KS_ERR_ARG_NULL, "NULL argument");
  KS_CALL(ksb_flush(R)); KS_CALL(ksb_flush(V)); KS_CALL(ksb_flush(AV)); KS_CALL(ksb_flush(BV));
  KS_CHECK(R != V && R != AV && R != BV, KS_ERR_ARG_WRONG, "R must be a different BV from V, AV and BV");
  KS_CHECK(V->n == R->n && AV->n == R->n && (!BV || BV->n == R->n), KS_ERR_ARG_INCOMP, "Mismatching local dimensions R %d, V %d, AV %d, BV %d", R->n, V->n, AV->n, BV ? BV->n : R->n);
  KS_CHECK(ncols >= 1 && ncols <= 16, KS_ERR_ARG_OUTOFRANGE, "%d result columns: the Ritz residual takes 1..16", ncols);
  const int l = V->l, m = V->k - V->l;
  KS_CHECK(m >= 1, KS_ERR_ARG_OUTOFRANGE, "V has no active columns");
  KS_CHECK(lds >= m, KS_ERR_ARG_SIZ, "S has %d rows, should have at least %d", lds, m);
  KS_CHECK(V->k <= AV->m && (!BV || V->k <= BV->m), KS_ERR_ARG_SIZ, "AV (%d columns) and BV (%d) must hold the active columns [%d,%d) of V", AV->m, BV ? BV->m : V->k, l, V->k);
  KS_CHECK(R->l >= 0 && R->l + ncols <= R->m, KS_ERR_ARG_SIZ, "R (%d columns) must hold %d columns from its first active column %d", R->m, ncols, R->l);
  for (ks_bv O : {X, BX}) {
    if (!O) continue;
    KS_CALL(ksb_flush(O));
    KS_CHECK(O != R && O != V && O != AV && O != BV && (X != BX), KS_ERR_ARG_WRONG, "X and BX must be BVs of their own");
    KS_CHECK(O->n == R->n, KS_ERR_ARG_INCOMP, "Mismatching local dimensions R %d, output %d", R->n, O->n);
    KS_CHECK(O->l >= 0 && O->l + ncols <= O->m, KS_ERR_ARG_SIZ, "An output BV (%d columns) must hold %d columns from its first active column %d", O->m, ncols, O->l);
    O->spec.valid = false;
  }
  KS_HIP(hipSetDevice(R->ctx->device));
  return ks_ritz_residual(R, ks_bv_col(R, R->l), V, ks_bv_col(V, l), V->ld, ks_bv_col(AV, l), AV->ld, BV ? ks_bv_col(BV, l) : nullptr, BV ? BV->ld : 0, m, S, lds, ncols, theta, rnorm, xnorm,
                          X ? ks_bv_col(X, X->l) : nullptr, X ? X->ld : 0, BX ? ks_bv_col(BX, BX->l) : nullptr, BX ? BX->ld : 0);
}
extern "C" int ks_bv_ritz_residual(ks_bv R, ks_bv V, ks_bv AV, ks_bv BV, const double *S, int lds, int ncols, const double *theta, double *rnorm, double *xnorm)
{
  return ritz_residual_entry(R, V, AV, BV, S, lds, ncols, theta, rnorm, xnorm, nullptr, nullptr);
}
// the same sweep, which also stores the Ritz vectors x_j = V S(:,j) into X and B x_j = BV S(:,j) (x_j itself without BV) into BX, each from the first
// active column of its BV and each optional: what the Jacobi-Davidson projector is made of (dvd_improvex_jd_start, dvdimprovex.c)
extern "C" int ks_bv_ritz_residual_vectors(ks_bv R, ks_bv V, ks_bv AV, ks_bv BV, const double *S, int lds, int ncols, const double *theta, double *rnorm, double *xnorm, ks_bv X, ks_bv BX)
{
  return ritz_residual_entry(R, V, AV, BV, S, lds, ncols, theta, rnorm, xnorm, X, BX);
}

// ---- the driver (struct Gd: ks_davidson.h) ----------------------------------------------------------------------------------------------------------
// a work BV in the layout of the solution basis; products of its columns as a block (ks_mat_mult_multi)
int Gd::make(int cols, ks_bv *out)
{
  KS_CALL(ks_bv_create(ctx, V->n, V->N, cols, V->ld, out));
  (*out)->row_start = V->row_start;
  (*out)->matmult = KS_BV_MATMULT_MAT;
  return KS_SUCCESS;
}
// column nconv + m of V <- a random vector orthonormal to the constraints, the locked vectors and the search basis (dvdinitv.c:52-58)
int Gd::random_column()
{
  const int j = nconv + m;
  KS_CALL(ks_bv_set_random_column(V, j, eps->seed));
  double nrm = 0.0; int lin = 0;
  KS_CALL(ks_bv_orthonormalizecolumn(V, j, 1, &nrm, &lin));
  KS_CHECK(nrm > 0.0 && !lin, KS_ERR_PLIB, "GD: no random vector independent of the basis could be found");
  m++;
  return KS_SUCCESS;
}
// V(:, nconv + m) orthonormalised against everything before it; *kept = false: dependent, the column is free again
int Gd::orthonormalize_new(bool *kept)
{
  double nrm = 0.0; int lin = 0;
  KS_CALL(ks_bv_orthonormalizecolumn(V, nconv + m, 0, &nrm, &lin));
  *kept = nrm > 0.0 && std::isfinite(nrm) && !lin;
  if (*kept) m++;
  return KS_SUCCESS;
}
// the m x cols host matrix Z (ldz) applied to the active columns: V <- V Z, AV <- AV Z, BV <- BV Z; `shift` leading columns of the product leave the
// work BVs (they are locked), so AV and BV take the columns [shift, cols) of Z into their columns [0, cols - shift)
int Gd::rotate(const double *Z, int ldz, int cols, int shift)
{
  const int kq = nconv + m;
  std::vector<double> Qv((size_t)kq * kq, 0.0), Qw((size_t)m * m, 0.0);
  for (int j = 0; j < cols; j++) for (int i = 0; i < m; i++) Qv[(size_t)(nconv + i) + (size_t)(nconv + j) * kq] = Z[(size_t)i + (size_t)j * ldz];
  for (int j = shift; j < cols; j++) for (int i = 0; i < m; i++) Qw[(size_t)i + (size_t)(j - shift) * m] = Z[(size_t)i + (size_t)j * ldz];
  KS_CALL(ks_bv_set_active_columns(V, nconv, kq));
  KS_CALL(ks_bv_multinplace(V, Qv.data(), kq, nconv, nconv + cols));
  KS_CALL(ks_bv_set_active_columns(AV, 0, m));
  if (cols > shift) KS_CALL(ks_bv_multinplace(AV, Qw.data(), m, 0, cols - shift));
  if (BV) { KS_CALL(ks_bv_set_active_columns(BV, 0, m)); if (cols > shift) KS_CALL(ks_bv_multinplace(BV, Qw.data(), m, 0, cols - shift)); }
  return KS_SUCCESS;
}
// the GD correction D = M^-1 R (dvd_improvex_gd2), one block application of the ST's preconditioner
int Gd::correction(int nb, const double *, const double *, int base)
{
  KS_CALL(ks_st_apply_mat(st, nb, ks_bv_col(R, 0), R->ld, ks_bv_col(V, base), V->ld));
  if (!(st->pc_type == KS_PC_NONE || st->pc_identity)) cfg->pc_columns += nb;
  return KS_SUCCESS;
}

int Gd::solve()
{
  ksd::DsGd &ds = eps->dsd;
  KS_CALL(make(mpd, &AV));
  if (B) KS_CALL(make(mpd, &BV));
  KS_CALL(make(bs, &R));
  const int ldg = ncv + 1;
  std::vector<double> G((size_t)ldg * ldg), C((size_t)ds.ld * ds.ld), Z((size_t)ds.ld * ds.ld), S((size_t)ds.ld * 16), theta(16), rnorm(16), xnorm(16);

  // the initial basis (dvd_initV_classic_0): the caller's initial space, all its vectors up to the initial size, then random ones
  const int ninit = std::min(initv, std::min(mpd, ncv));
  const int nuser = (eps->ini && eps->nini) ? std::min(eps->nini, ninit) : 0;
  for (int i = 0; i < nuser; i++) {
    KS_CALL(ksk_copy(ctx, ks_bv_col(eps->ini, i), ks_bv_col(V, m), V->n));
    bool kept = false;
    KS_CALL(orthonormalize_new(&kept));
  }
  while (m < ninit) KS_CALL(random_column());

  while (eps->reason == KS_EPS_CONVERGED_ITERATING) {
    cfg->iterations++;
    if (m == 0) KS_CALL(random_column());                                 // everything was locked: start again (davidson.c:205-206)
    // images of the new columns and the new columns of H (dvd_calcpairs_proj)
    if (mprod < m) {
      const int nn = m - mprod;
      KS_CALL(ksb_matmult_block(AV, A, ks_bv_col(V, nconv + mprod), V->ld, ks_bv_col(AV, mprod), AV->ld, nn)); cfg->mat_columns += nn;
      if (B) { KS_CALL(ksb_matmult_block(BV, B, ks_bv_col(V, nconv + mprod), V->ld, ks_bv_col(BV, mprod), BV->ld, nn)); cfg->mat_columns += nn; }
      std::fill(G.begin(), G.end(), 0.0);
      KS_CALL(ksb_dot_range(AV, mprod, m, V, nconv, nconv + m, G.data(), ldg));               // G(nconv + i, j) = V(:, nconv + i)^T AV(:, j)
      for (int j = 0; j < nn; j++) for (int i = 0; i < m; i++) C[(size_t)i + (size_t)j * ds.ld] = G[(size_t)(nconv + i) + (size_t)(mprod + j) * ldg];
      KS_CALL(ks_eps_synchronize_values(eps, C.data(), (size_t)ds.ld * nn));
      ds.grow(nn, C.data(), ds.ld);
      mprod = m;
    }
    // Rayleigh-Ritz (dvd_calcpairs_projeig): rank 0's values and vectors to every rank, the control flow that follows is then the same everywhere
    {
      std::vector<double> pack((size_t)1 + ds.ld + ds.Q.size());
      pack[0] = (double)ds.solve_sort();
      std::copy(ds.w.begin(), ds.w.end(), pack.begin() + 1); std::copy(ds.Q.begin(), ds.Q.end(), pack.begin() + 1 + ds.ld);
      KS_CALL(ks_eps_synchronize_values(eps, pack.data(), pack.size()));
      std::copy(pack.begin() + 1, pack.begin() + 1 + ds.ld, ds.w.begin()); std::copy(pack.begin() + 1 + ds.ld, pack.end(), ds.Q.begin());
      if (pack[0] != 0.0) { eps->reason = KS_EPS_DIVERGED_BREAKDOWN; break; }
    }
    for (int j = 0; j < m && nconv + j <= ncv; j++) { eps->eigr[nconv + j] = ds.w[j]; eps->eigi[nconv + j] = 0.0; }
    // Ritz vectors and residuals of the best pairs, one sweep (dvd_calcpairs_res_0), then the convergence test in order (dvd_updateV_testConv)
    const int nb = std::min(bs, m);
    for (int j = 0; j < nb; j++) { theta[j] = ds.w[j]; for (int i = 0; i < m; i++) S[(size_t)i + (size_t)j * ds.ld] = ds.q(i, j); }
    KS_CALL(ks_ritz_residual(R, ks_bv_col(R, 0), V, ks_bv_col(V, nconv), V->ld, ks_bv_col(AV, 0), AV->ld, BV ? ks_bv_col(BV, 0) : nullptr, BV ? BV->ld : 0, m,
                             S.data(), ds.ld, nb, theta.data(), rnorm.data(), xnorm.data(), Xo ? ks_bv_col(Xo, nconv) : nullptr, Xo ? Xo->ld : 0,
                             BXo ? ks_bv_col(BXo, nconv) : nullptr, BXo ? BXo->ld : 0));
    cfg->fused_residuals++;
    KS_CALL(ks_eps_synchronize_values(eps, rnorm.data(), 16)); KS_CALL(ks_eps_synchronize_values(eps, xnorm.data(), 16));
    int npre = 0; bool conv = true;
    for (int j = 0; j < nb; j++) {
      const int i = nconv + j;
      eps->errest[i] = ks_eps_converged_estimate(eps, eps->eigr[i], 0.0, xnorm[j] > 0.0 ? rnorm[j] / xnorm[j] : rnorm[j]);
      if (conv && eps->errest[i] < eps->tol) npre++; else conv = false;
      if (!conv && !eps->trackall) break;
    }
    KS_CHECK(!eps->cb_err, eps->cb_err, "the user's convergence test returned %d", eps->cb_err);
    npre = std::max(std::min(npre, nev - nconv), 0);                      // dvdupdatev.c:100
    eps->nconv = nconv;
    KS_CALL(ks_eps_stopping_call(eps, eps->its, eps->nconv));
    if (eps->reason != KS_EPS_CONVERGED_ITERATING) break;

    if (npre > 0) {
      // lock (dvd_updateV_conv_gen): the basis and its images rotated by Q, the converged Ritz vectors lead and leave the active range
      KS_CALL(rotate(ds.Q.data(), ds.ld, m, npre));
      nconv += npre; m -= npre; mprod = m;
      ds.lock(npre);
      cfg->locks++;
      locked(npre);
    } else if (m + bs > mpd || nconv + m + bs > ncv) {
      // thick restart (dvd_updateV_restart_gen, dvdupdatev.c:166-170): size_X Ritz vectors and size_plusk vectors of the previous iteration
      const int mrs = std::max(0, std::min(mpd - 1, ncv - nconv - 2));
      const int size_X = std::max(1, std::min(std::min(minv, mrs - ((mrs > 1 && plusk > 0 && ds.size_oldU > 0) ? 1 : 0)), m));
      const int size_plusk = std::max(0, std::min(std::min(std::min(plusk, ds.size_oldU), mrs - size_X), m - size_X));
      const int kept = ds.restart_basis(size_X, size_plusk, Z.data(), ds.ld);
      KS_CALL(rotate(Z.data(), ds.ld, kept, 0));
      ds.project(Z.data(), ds.ld, kept);
      m = kept; mprod = m;
      cfg->restarts++; eps->restarts++;
    } else {
      // expand (dvd_updateV_update_gen with the solver's correction: GD's D = M^-1 R, or JD's correction equation), the Q of this iteration kept for the next restart
      const int mold = m, base = nconv + m;
      KS_CALL(correction(nb, theta.data(), rnorm.data(), base));
      for (int j = 0; j < nb; j++) {
        if (base + j != nconv + m) KS_CALL(ks_bv_copycolumn(V, base + j, nconv + m));      // a dropped column's place is taken by the next
        bool kept = false;
        KS_CALL(orthonormalize_new(&kept));
      }
      if (m == mold) KS_CALL(random_column());
      if (plusk > 0) ds.save_oldU();
    }
    KS_CALL(ks_bv_set_active_columns(V, nconv, nconv + m));
    eps->nconv = nconv;
    eps->its++;
    KS_CALL(ks_eps_monitor_call(eps, eps->its, eps->nconv, std::min(nconv + m, nev)));
  }
  eps->nconv = nconv;
  return KS_SUCCESS;
}

// EPSSetUp_XD (davidson.c:51-77) with the parts of EPSSetUp whose rules are this solver's: every violated rule is KS_ERR_SUP, as there
int ks_davidson_setup(ks_eps eps, KsDavidson &cfg, const char *name)
{
  KS_CHECK(eps->A, KS_ERR_ORDER, "EPSSetOperators must be called first");
  ks_mat A = eps->A;
  KS_HIP(hipSetDevice(eps->ctx->device));
  const int n = A->n_global, nev = eps->nev;
  int ptype = eps->problem_type;
  if (!eps->B && ptype == KS_EPS_GHEP) ptype = KS_EPS_HEP;
  KS_CHECK(ptype == KS_EPS_HEP || ptype == KS_EPS_GHEP, KS_ERR_SUP, "%s: only Hermitian (HEP) or generalized Hermitian positive definite (GHEP) problems are built (the reference also solves non-symmetric ones)", name);
  KS_CHECK(!eps->B || ptype == KS_EPS_GHEP, KS_ERR_ARG_INCOMP, "Inconsistent EPS state: the problem type does not match the number of matrices");
  KS_CHECK(!eps->B || cfg.borth, KS_ERR_SUP, "%s: a generalized problem needs the B-orthonormal search basis (EPS%sSetBOrth); the other variant is not built", name, name);
  const int bs = cfg.bs > 0 ? cfg.bs : 1;
  int ncv;
  if (eps->ncv_user) { KS_CHECK(eps->ncv_user >= nev, KS_ERR_SUP, "The value of ncv must be at least nev"); ncv = eps->ncv_user; }
  else if (eps->mpd_user) ncv = eps->mpd_user + nev + bs;
  else if (n < 10) ncv = n + nev + bs;
  else ncv = std::max(nev, std::min(n - bs, std::max(2 * nev, nev + 15)) + bs);
  const int mpd = eps->mpd_user ? eps->mpd_user : std::min(n, ncv);
  KS_CHECK(mpd <= ncv, KS_ERR_SUP, "The mpd parameter has to be less than or equal to ncv");
  KS_CHECK(mpd >= 2, KS_ERR_SUP, "The mpd parameter has to be greater than 2");
  const int which = eps->which.which ? eps->which.which : KS_EPS_LARGEST_MAGNITUDE;
  KS_CHECK(nev + bs <= ncv, KS_ERR_SUP, "The value of ncv has to be greater than nev plus blocksize");
  KS_CHECK(!eps->trueres, KS_ERR_SUP, "The true residual is disabled in this solver");
  KS_CHECK(!eps->twosided, KS_ERR_SUP, "%s does not compute left eigenvectors (EPSSetTwoSided)", name);
  KS_CHECK(eps->extraction == KS_EPS_RITZ, KS_ERR_SUP, "%s: only the Ritz extraction is built", name);
  KS_CHECK(!eps->arb_fn, KS_ERR_SUP, "%s does not support arbitrary selection of eigenpairs", name);
  const int minv = cfg.minv > 0 ? cfg.minv : (n < 10 ? 1 : std::min(std::max(bs, 6), mpd / 2));
  KS_CHECK(minv + bs <= mpd, KS_ERR_SUP, "The value of minv must be less than mpd minus blocksize");
  const int plusk = cfg.plusk >= 0 ? cfg.plusk : 1;
  const int initv = cfg.initv > 0 ? cfg.initv : (n < 10 ? 1 : 6);
  KS_CHECK(mpd >= initv, KS_ERR_SUP, "The initv parameter has to be less than or equal to mpd");
  eps->mpd = mpd;
  cfg.r_bs = bs; cfg.r_minv = minv; cfg.r_plusk = plusk; cfg.r_initv = initv;
  if (eps->conv == KS_EPS_CONV_NORM) KS_CALL(ks_eps_matrix_norms(eps));
  eps->cmp_final = eps->which; eps->cmp_final.which = which; eps->cmp_ds = eps->cmp_final;
  // the ST only preconditions: K = A - sigma B with sigma the shift, else the target for the target criteria, else 0; for the largest-* criteria the
  // default shift is infinite (davidson.c:80, precond.c:70-74): M from B alone, or no preconditioning for a standard problem
  ks_st st = nullptr;
  KS_CALL(ks_eps_get_st(eps, &st));
  if (!st->type_set && st->type != KS_ST_PRECOND) { st->type = KS_ST_PRECOND; st->ready = false; }
  const bool inf = which == KS_EPS_LARGEST_MAGNITUDE || which == KS_EPS_LARGEST_REAL || which == KS_EPS_LARGEST_IMAGINARY;
  const bool tgt = which == KS_EPS_TARGET_MAGNITUDE || which == KS_EPS_TARGET_REAL;
  if (!st->sigma_set) { const double sg = tgt ? eps->which.target : 0.0; if (st->sigma != sg || st->sigma_inf != inf) { st->sigma = sg; st->sigma_inf = inf; st->ready = false; } }
  KS_CALL(ks_st_set_matrices(st, A, eps->B)); st->ready = false;
  KS_CALL(ks_st_setup_internal(st));
  eps->op = A;
  KS_CALL(eps_setup_common(eps, ncv, ptype == KS_EPS_GHEP ? eps->B : nullptr));
  if (!eps->max_it_user) eps->max_it = std::max(100 * ncv, 2 * n);
  cfg.iterations = cfg.restarts = cfg.locks = cfg.mat_columns = cfg.pc_columns = cfg.fused_residuals = 0;
  eps->ghep = ptype == KS_EPS_GHEP; eps->problem_type_resolved_hermitian = true; eps->left_trivial = true;
  eps->dsd.allocate(ncv + 1); eps->dsd.which = eps->cmp_final;
  return KS_SUCCESS;
}

static int gd_setup(ks_eps eps) { return ks_davidson_setup(eps, eps->gd, "GD"); }

// EPSSolve_XD. It leaves the eigenvectors in V(:,0:nconv), B-orthonormal: nothing for the epilogue to map back, purify or normalise (no compute_vectors)
int ks_davidson_solve(ks_eps eps, KsDavidson &cfg, Gd &s)
{
  s.eps = eps; s.ctx = eps->ctx; s.A = eps->A; s.B = eps->ghep ? eps->B : nullptr; s.st = eps->st; s.V = eps->V; s.cfg = &cfg;
  s.bs = cfg.r_bs; s.mpd = eps->mpd; s.minv = cfg.r_minv; s.plusk = cfg.r_plusk; s.initv = cfg.r_initv; s.ncv = eps->ncv; s.nev = eps->nev;
  const int rc = s.solve();
  ks_bv_destroy(eps->ini); eps->ini = nullptr; eps->nini = 0;                                                     // the initial space is consumed like the deflation space
  ks_bv_gs_passes(eps->V, &eps->passes0[0], nullptr);     // the passes stat counts the Gram-Schmidt passes of Krylov expansions: none here
  return rc;
}
static int gd_solve(ks_eps eps) { Gd s; return ks_davidson_solve(eps, eps->gd, s); }

const ks_eps_ops *ks_gd_ops()
{
  static const ks_eps_ops ops = {gd_setup, gd_solve, nullptr};
  return &ops;
}

// ---- the settings (EPSGDSet* / EPSGDGet*, src/eps/impls/davidson/gd/gd.c; EPSJDSet* / EPSJDGet*, jd/jd.c: the same rules on the type's own copy) ----
int ks_davidson_set_blocksize(ks_eps eps, KsDavidson &cfg, int bs)
{
  KS_CHECK(bs >= 0 && bs <= 16, KS_ERR_ARG_OUTOFRANGE, "block size %d: this build keeps the blocks of GD to 1..16 columns (0: the default, 1)", bs);
  cfg.bs = bs; eps->solved = false; return KS_SUCCESS;
}
int ks_davidson_set_restart(ks_eps eps, KsDavidson &cfg, int minv, int plusk)
{
  KS_CHECK(minv >= -1, KS_ERR_ARG_OUTOFRANGE, "Invalid minv value %d", minv);
  KS_CHECK(plusk >= -1, KS_ERR_ARG_OUTOFRANGE, "Invalid plusk value %d", plusk);
  cfg.minv = minv > 0 ? minv : 0; cfg.plusk = plusk; eps->solved = false; return KS_SUCCESS;
}
void ks_davidson_get_restart(const KsDavidson &cfg, int *minv, int *plusk)
{
  if (minv) *minv = cfg.minv ? cfg.minv : cfg.r_minv;
  if (plusk) *plusk = cfg.plusk >= 0 ? cfg.plusk : 1;
}
int ks_davidson_set_initial_size(ks_eps eps, KsDavidson &cfg, int initialsize)
{
  KS_CHECK(initialsize >= -1, KS_ERR_ARG_OUTOFRANGE, "Invalid initial size %d", initialsize);
  cfg.initv = initialsize > 0 ? initialsize : 0; eps->solved = false; return KS_SUCCESS;
}
extern "C" int ks_eps_gd_set_blocksize(ks_eps eps, int bs) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); return ks_davidson_set_blocksize(eps, eps->gd, bs); }            // EPSGDSetBlockSize gd.c
extern "C" int ks_eps_gd_get_blocksize(ks_eps eps, int *bs) { KS_CHECK(eps && bs, KS_ERR_ARG_NULL, "NULL argument"); *bs = eps->gd.bs ? eps->gd.bs : 1; return KS_SUCCESS; }
extern "C" int ks_eps_gd_set_restart(ks_eps eps, int minv, int plusk) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); return ks_davidson_set_restart(eps, eps->gd, minv, plusk); }   // EPSGDSetRestart gd.c
extern "C" int ks_eps_gd_get_restart(ks_eps eps, int *minv, int *plusk) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); ks_davidson_get_restart(eps->gd, minv, plusk); return KS_SUCCESS; }
extern "C" int ks_eps_gd_set_initial_size(ks_eps eps, int initialsize) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); return ks_davidson_set_initial_size(eps, eps->gd, initialsize); }   // EPSGDSetInitialSize gd.c
extern "C" int ks_eps_gd_get_initial_size(ks_eps eps, int *initialsize)
{
  KS_CHECK(eps && initialsize, KS_ERR_ARG_NULL, "NULL argument");
  *initialsize = eps->gd.initv ? eps->gd.initv : eps->gd.r_initv; return KS_SUCCESS;
}
extern "C" int ks_eps_gd_set_borth(ks_eps eps, int borth) { KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL"); eps->gd.borth = borth != 0; eps->solved = false; return KS_SUCCESS; }   // EPSGDSetBOrth gd.c
extern "C" int ks_eps_gd_get_borth(ks_eps eps, int *borth) { KS_CHECK(eps && borth, KS_ERR_ARG_NULL, "NULL argument"); *borth = eps->gd.borth ? 1 : 0; return KS_SUCCESS; }
extern "C" int ks_eps_gd_get_stats(ks_eps eps, long long *iterations, long long *restarts, long long *locks, long long *mat_columns, long long *pc_columns, long long *fused_residuals)
{
  KS_CHECK(eps, KS_ERR_ARG_NULL, "EPS is NULL");
  if (iterations) *iterations = eps->gd.iterations; if (restarts) *restarts = eps->gd.restarts; if (locks) *locks = eps->gd.locks;
  if (mat_columns) *mat_columns = eps->gd.mat_columns; if (pc_columns) *pc_columns = eps->gd.pc_columns; if (fused_residuals) *fused_residuals = eps->gd.fused_residuals;
  return KS_SUCCESS;
}
