// The device-resident shell of the ST's Krylov solvers whose scalars never leave the device (KS_KSP_CG: ks_cg.hip, KS_KSP_MINRES: ks_minres.hip). A solver
// keeps its scalars in a state block that begins with a KsKspHead and runs an iteration as a few row sweeps of its own around the existing product. The
// host enqueues `check` iterations (KsResident), then reads the state once. Every sweep of an iteration that starts after the solve has ended returns
// at its gate without touching a vector, so the iterations enqueued past the end change nothing: count, iterate and residual norm are the same bits for
// every `check`. What is here: the head's gate and end, the sums a sweep consumes, the kernel that prepares them for the ranks, the dot sweep, the row
// walk with its width-W values, and the host side of a solve (scratch, launches, the batch loop). What a solver file holds is its algorithm.
//
// Who may write what: only thread 0 of workgroup 0 writes the state, and no field written in a launch is read by the other workgroups of that launch to
// decide what they compute. Every workgroup sums the same partials in the same order (reduce_partials_to_lds: a fixed order, no floating-point atomics)
// and runs the same instructions on them, so all arrive at the same scalars and the same verdict. A field that a sweep both reads and rewrites is
// double-buffered by its solver (KsMinresState::rot). The words read and written inside one launch are the head's two flags:
//   done   set where a sweep ends the solve WITHOUT doing its vector work (ksp_end). It is read once per workgroup: one that starts after workgroup 0
//          has set it returns at the gate, one that started before reaches the same verdict itself - without a store either way.
//   conv   set by a sweep that ends the solve AFTER its vector work. No gate of that launch reads it - a workgroup that saw it would skip work the
//          iterate needs. The first sweep of the next iteration gates on done | conv (ksp_gate<true>) and its bookkeeping thread turns conv into done,
//          so the sweeps behind it gate on done alone, set by an earlier launch. A solver whose verdicts all come before the vector work leaves it zero.
// Kernel boundaries order everything else: a sweep's partials and the state are complete when the next launch begins. The product and the block
// preconditioners between the sweeps are not gated: what they write nobody reads once the solve has ended.
// More than one rank: a sweep's partials are summed by a one-workgroup kernel into `red`, ks_allreduce_sum runs on it in stream order, and the consumer
// reads the sums there instead of the partials (KspResident::collect). A rank without rows writes zero partials and takes part in every collective.
#pragma once
#include "ks_sweeps.cuh"
#include <algorithm>
#include <type_traits>

namespace ksk {

// ---- the head -------------------------------------------------------------------------------------------------------------------------------------
// The gate, the same for every wave of a workgroup: thread 0 reads once and hands it out through LDS. Were every wave to read it for itself, workgroup 0
// could set it in between, and the waves left would sum partials without the wave that owns a column of them (reduce_partials_to_lds).
template <bool WITH_CONV>
__device__ __forceinline__ int ksp_gate(const KsKspHead *h)
{
  __shared__ int gate;
  if (threadIdx.x == 0) {
    int g = __atomic_load_n(&h->done, __ATOMIC_RELAXED);
    if (WITH_CONV) g |= __atomic_load_n(&h->conv, __ATOMIC_RELAXED);
    gate = g;
  }
  __syncthreads();
  return gate;
}
__device__ __forceinline__ void ksp_end(KsKspHead *h, int reason) { h->reason = reason; __atomic_store_n(&h->done, 1, __ATOMIC_RELAXED); }

// ncols <= 2 sums of this rank and its peers (red) or of this rank's workgroups (part, nblocks of them per column), the same values in every workgroup
__device__ __forceinline__ void ksp_sums(const double *__restrict__ red, const double *__restrict__ part, int nblocks, int ncols, double *c_lds)
{
  if (red) { if ((int)threadIdx.x < ncols) c_lds[threadIdx.x] = red[threadIdx.x]; __syncthreads(); }
  else reduce_partials_to_lds(part, nblocks, ncols, c_lds);
}
// the same for a solver with more sums per sweep (BiCGStab(l): the 15 of a Gram matrix): their number is a template argument, and the sweeps of CG and
// MINRES keep the form above and the instructions they had
template <int NCOLS>
__device__ __forceinline__ void ksp_sums(const double *__restrict__ red, const double *__restrict__ part, int nblocks, double *c_lds)
{
  if (red) { if ((int)threadIdx.x < NCOLS) c_lds[threadIdx.x] = red[threadIdx.x]; __syncthreads(); }
  else reduce_partials_to_lds(part, nblocks, NCOLS, c_lds);
}
// more than one rank: red[i] = this rank's sum of column i < NCOLS of the partials, for the allreduce behind it. Not gated: its inputs are left
// alone once the solve has ended, and every rank keeps issuing the same collectives. NCOLS is a template argument for the sake of the sweeps beside it:
// with a run-time count here the compiler stops specialising reduce_partials_to_lds in a file whose every other caller sums one column (MINRES: 56
// VGPRs and some 90 instructions more in each of start, lanczos and update: scripts/isa_diff.py)
template <int NCOLS>
__global__ __launch_bounds__(SW_BLOCK) void k_ksp_finish(const double *__restrict__ part, int nblocks, double *__restrict__ red)
{
  __shared__ double c[NCOLS];
  reduce_partials_to_lds(part, nblocks, NCOLS, c);
  if ((int)threadIdx.x < NCOLS) red[threadIdx.x] = c[threadIdx.x];
}

// ---- the row walk ---------------------------------------------------------------------------------------------------------------------------------
// W consecutive rows of one vector in a lane's registers: a sweep states its arithmetic once, on these, for the pair form (one 16-byte access) and the
// one-row form. Element by element, with the fma, multiply or divide the caller names; row_dot takes the pair's first row into the sum before its second.
template <int W> struct Rows { double e[W]; };
template <int W> __device__ __forceinline__ Rows<W> row_load(const double *p)
{
  Rows<W> v;
  if (W == 2) { const double2 t = *reinterpret_cast<const double2 *>(p); v.e[0] = t.x; v.e[W - 1] = t.y; }
  else v.e[0] = p[0];
  return v;
}
template <int W> __device__ __forceinline__ void row_store(double *p, const Rows<W> &v)
{
  if (W == 2) { double2 t; t.x = v.e[0]; t.y = v.e[W - 1]; *reinterpret_cast<double2 *>(p) = t; }
  else p[0] = v.e[0];
}
template <int W> __device__ __forceinline__ Rows<W> row_fma(double a, const Rows<W> &x, Rows<W> y) { for (int k = 0; k < W; k++) y.e[k] = fma(a, x.e[k], y.e[k]); return y; }
template <int W> __device__ __forceinline__ Rows<W> row_mul(const Rows<W> &a, Rows<W> x) { for (int k = 0; k < W; k++) x.e[k] = a.e[k] * x.e[k]; return x; }
template <int W> __device__ __forceinline__ Rows<W> row_div(Rows<W> x, double d) { for (int k = 0; k < W; k++) x.e[k] /= d; return x; }
template <int W> __device__ __forceinline__ void row_dot(const Rows<W> &a, const Rows<W> &b, double &acc) { for (int k = 0; k < W; k++) acc = fma(a.e[k], b.e[k], acc); }

// Tiles of SW_BLOCK x VEC rows dealt to the workgroups grid-stride; body(i, width) runs once per lane with width 2 for a full pair of rows from i (VEC = 2,
// every vector 16-byte aligned), else once per row with width 1: every row of a misaligned vector, and the last row of an odd n. width is a
// std::integral_constant, so that the body's W is a compile-time value
template <int VEC, typename F>
__device__ __forceinline__ void ksp_rows(int n, F body)
{
  const long long tile = (long long)SW_BLOCK * VEC;
  const long long ntiles = ((long long)n + tile - 1) / tile;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * tile + (long long)threadIdx.x * VEC;
    if (VEC == 2 && i + 1 < n) body(i, std::integral_constant<int, 2>());
    else for (int u = 0; u < VEC; u++) if (i + u < n) body(i + u, std::integral_constant<int, 1>());
  }
}

// partials of (r, z) and, K = 2, of (z, z): the start of a solve, and every iteration of a preconditioner with kernels of its own
template <int VEC, int K>
__global__ __launch_bounds__(SW_BLOCK) void k_ksp_dots(const KsKspHead *__restrict__ h, int n, const double *__restrict__ r, const double *__restrict__ z, double *__restrict__ part)
{
  if (ksp_gate<false>(h)) return;
  double acc[K] = {};
  ksp_rows<VEC>(n, [&](long long i, auto width) {
    constexpr int W = decltype(width)::value;
    const Rows<W> rv = row_load<W>(r + i), zv = row_load<W>(z + i);
    row_dot(rv, zv, acc[0]);
    if (K == 2) row_dot(zv, zv, acc[K - 1]);
  });
  block_write_partials<K>(acc, K, part);
}

// ---- the host side --------------------------------------------------------------------------------------------------------------------------------
// run-time flags to template arguments: f is called with the std::integral_constant of v, one of V..., or of the flag
template <int... V, typename F> int ksp_pick(int v, F f)
{
  int rc = KS_ERR_ARG_OUTOFRANGE;
  (void)((v == V && ((rc = f(std::integral_constant<int, V>())), true)) || ...);
  return rc;
}
template <typename F> int ksp_flag(bool b, F f) { return b ? f(std::true_type()) : f(std::false_type()); }
inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

// One solve: the launch shape, the scratch carved behind its head (the state, then the ranks' sums; the partials arrays follow the head, KS_MAX_BLOCKS
// doubles per column) and what every resident solver does with them. State begins with a KsKspHead `h`. The scratch has a size per solver: HEAD bytes
// for the state and NRED sums of the ranks, then COLS partials columns (CG and MINRES: 256 bytes, 4 sums, 3 columns)
template <typename State, size_t HEAD = KS_RESIDENT_HEAD_BYTES, int COLS = KS_RESIDENT_PART_COLS, int NRED = 4>
struct KspResident {
  ks_st st; ks_ctx ctx; KsResident *res; int n, grid; bool multi, v2, tr;
  State *state; double *red, *part;
  const double *dinv; int pc;                   // 0: no preconditioner, 1: point Jacobi (dinv), 2: blocks with kernels of their own (ks_st_blocks_apply)

  int init(const KsKsp &k, ks_st st_, KsResident *res_, bool tr_)
  {
    static_assert(sizeof(State) + NRED * sizeof(double) <= HEAD, "state and the ranks' sums share the head of the scratch");
    st = st_; ctx = k.ctx; res = res_; n = (int)k.n; tr = tr_; multi = ks_is_multi(ctx);
    KS_CALL(ks_resident_alloc(res, HEAD, COLS));
    // one grid for every sweep, so that the partials line up: at most 4 workgroups per CU, KS_MAX_BLOCKS at the most (what a partials array holds); the
    // one-row-per-lane forms of a misaligned vector keep it and walk twice the tiles per workgroup
    grid = ks_sweep_grid(ctx, n, 2);
    state = (State *)res->dev; red = (double *)(res->dev + sizeof(State)); part = (double *)(res->dev + HEAD);
    dinv = nullptr;
    const bool pointwise = ks_st_pc_pointwise(st, &dinv);
    pc = !pointwise ? 2 : (dinv ? 1 : 0);
    v2 = !dinv || aligned16(dinv);              // and every vector of the solver: it adds them
    return KS_SUCCESS;
  }
  // state = 0, y = 0
  int zero(double *y)
  {
    KS_HIP(hipMemsetAsync(state, 0, HEAD, ctx->stream));
    KS_HIP(hipMemsetAsync(y, 0, sizeof(double) * std::max<long long>(n, 1), ctx->stream));
    return KS_SUCCESS;
  }
  // one of the solver's own kernels on `blocks` workgroups, counted
  template <typename... P, typename... A> int launch(void (*kern)(P...), int blocks, A... a)
  {
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(SW_BLOCK), 0, ctx->stream, a...);
    KS_HIP(hipGetLastError());
    res->sweeps++;
    return KS_SUCCESS;
  }
  template <typename F> int width(bool two, F f) { return ksp_pick<1, 2>(two ? 2 : 1, f); }
  // the NCOLS sums of a sweep's partials across the ranks, stream-ordered: no host wait
  template <int NCOLS> int collect(double *p, double *out)
  {
    if (!multi) return KS_SUCCESS;
    KS_CALL(launch(k_ksp_finish<NCOLS>, 1, p, grid, out));
    return ks_allreduce_sum(ctx, out, NCOLS);
  }
  // the dot sweep of K sums into p, and their collection into out
  template <int K> int dots(double bytes, const double *r, const double *z, double *p, double *out)
  {
    {
      KsProfScope ps(ctx, KS_K_OTHER, bytes);
      KS_CALL(width(v2, [&](auto VEC) { return launch(k_ksp_dots<decltype(VEC)::value, K>, grid, &state->h, n, r, z, p); }));
    }
    return collect<K>(p, out);
  }
  // batches of `check` iterations, each enqueued by one call of `iteration`, until a read of the state finds the solve ended: *out is the host's copy
  template <typename F> int run(F iteration, const State **out)
  {
    const State *hs = (const State *)res->host;
    do {
      for (int j = 0; j < res->check; j++) KS_CALL(iteration());
      KS_HIP(hipMemcpyAsync(res->host, state, sizeof(State), hipMemcpyDeviceToHost, ctx->stream));
      KS_HIP(ks_sync(ctx));
      res->waits++;
      KS_CALL(ks_oneshot_error(ctx));
    } while (!hs->h.done && !hs->h.conv);
    res->gated += hs->h.gated;
    *out = hs;
    return KS_SUCCESS;
  }
};

} // namespace ksk
