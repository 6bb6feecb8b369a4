// Mat: assembly of a matrix - creation from CSR arrays, the Laplacian generators and the PETSc binary loader, the halo plan, the device layouts of the
// diagonal block and their chooser (the product kernels that walk them: ks_spmv.hip, ks_spmm.hip; the storage rules both sides share: ks_rows.cuh),
// MatGetDiagonal, MatNorm, shell matrices, destruction.
// What is decided on the host with index arithmetic alone - the diagonal / ghost split of ks_mat_create_csr, the peers, counts and offsets of the halo
// plan, the binned and the windowed layout - is planned in ks_csr.cpp (ks_csr.h), which has no device code and is tested on the CPU: here those are
// "call the planner, upload what it filled". The layouts built by kernels (dictionary, SELL-64, XCD-sliced) and the generators are all here.
#include "ks_rows.cuh"
#include "ks_csr.h"
#include <algorithm>
#include <numeric>
#include <new>

namespace {
using namespace ksr;

// a host vector's copy in device memory (never an empty allocation); what a failure means is the caller's to say
template <class T> hipError_t upload(T **dev, const std::vector<T> &host)
{
  const hipError_t e = hipMalloc((void **)dev, sizeof(T) * std::max<size_t>(host.size(), 1));
  return e != hipSuccess ? e : hipMemcpy(*dev, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice);
}

// one thread per row: encode the row's entries against the sorted candidate dictionaries (binary search); entries that
// are not covered are counted and the first `cap` of them recorded so that the host can extend the dictionaries
__global__ void k_dict_encode(int n, int W, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val,
                              const long long *__restrict__ dbits, int nv, const int *__restrict__ doffs, int no,
                              unsigned short *__restrict__ codes, int *miss, long long *miss_bits, int *miss_off, int cap,
                              unsigned char *__restrict__ codes8, double *__restrict__ vals_out)
{
  // nv < 0: offsets-only mode (values kept in full): 1-byte codes into codes8, values into vals_out in slice-column-major order
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int p0 = rowptr[r], len = rowptr[r + 1] - p0;
  for (int j = 0; j < W; j++) {
    unsigned short code = 0xff00u;                                       // padding
    if (nv < 0) {
      unsigned char c8 = 255; double v = 0.0;
      if (j < len) {
        const int off = col[p0 + j] - (int)r;
        int lo = 0, hi = no; while (lo < hi) { const int m = (lo + hi) >> 1; if (doffs[m] < off) lo = m + 1; else hi = m; }
        if (lo < no && doffs[lo] == off) c8 = (unsigned char)lo;
        else { if (*(volatile int *)miss < cap) { const int idx = atomicAdd(miss, 1); if (idx < cap) { miss_bits[idx] = 0; miss_off[idx] = off; } } else atomicAdd(miss + 1, 1); c8 = 0; }
        v = val[p0 + j];
      }
      codes8[r * W + j] = c8;
      vals_out[((r >> 6) * W + j) * 64 + (r & 63)] = v;
      continue;
    }
    if (j < len) {
      const long long bits = __double_as_longlong(val[p0 + j]);
      const int off = col[p0 + j] - (int)r;
      int lo = 0, hi = nv; while (lo < hi) { const int m = (lo + hi) >> 1; if (dbits[m] < bits) lo = m + 1; else hi = m; }
      const int vi = (lo < nv && dbits[lo] == bits) ? lo : -1;
      lo = 0; hi = no; while (lo < hi) { const int m = (lo + hi) >> 1; if (doffs[m] < off) lo = m + 1; else hi = m; }
      const int oi = (lo < no && doffs[lo] == off) ? lo : -1;
      if (vi < 0 || oi < 0) {
        if (*(volatile int *)miss < cap) { const int idx = atomicAdd(miss, 1); if (idx < cap) { miss_bits[idx] = bits; miss_off[idx] = off; } }
        else atomicAdd(miss + 1, 1);
        code = 0;
      } else code = (unsigned short)((vi << 8) | oi);
    }
    codes[r * W + j] = code;
  }
}
// one thread per row: find the row's code word (wpr 32-bit words) in the sorted candidate table (binary search, words compared in order) and write its
// index; rows that are not covered are counted and the code words of the first `cap` of them recorded so that the host can extend the table
__global__ void k_dict_match(int n, int wpr, const unsigned *__restrict__ codes, const unsigned *__restrict__ pats, int npat, unsigned char *__restrict__ rowpat,
                             int *miss, unsigned *__restrict__ miss_words, int cap)
{
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const unsigned *c = codes + r * wpr;
  auto cmp = [&](int m) { for (int i = 0; i < wpr; i++) { const unsigned a = pats[(long long)m * wpr + i], b = c[i]; if (a != b) return a < b ? -1 : 1; } return 0; };
  int lo = 0, hi = npat;
  while (lo < hi) { const int m = (lo + hi) >> 1; if (cmp(m) < 0) lo = m + 1; else hi = m; }
  if (lo < npat && cmp(lo) == 0) { rowpat[r] = (unsigned char)lo; return; }
  if (*(volatile int *)miss < cap) { const int idx = atomicAdd(miss, 1); if (idx < cap) for (int i = 0; i < wpr; i++) miss_words[(long long)idx * wpr + i] = c[i]; }
  else atomicAdd(miss + 1, 1);
}
__global__ void k_max_rowlen(int n, const int *__restrict__ rowptr, int *out)
{
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  int len = (r < n) ? rowptr[r + 1] - rowptr[r] : 0;
  for (int off = 32; off > 0; off >>= 1) len = max(len, __shfl_xor(len, off, 64));
  if ((threadIdx.x & 63) == 0 && len > 0) atomicMax(out, len);
}

__global__ void k_sell_widths(int n, int nslices, const int *__restrict__ rowptr, int *__restrict__ width, int *__restrict__ rlen)
{
  const long long s = (long long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (s >= nslices) return;
  const int lane = threadIdx.x & 63;
  const long long r = s * 64 + lane;
  int len = (r < n) ? rowptr[r + 1] - rowptr[r] : 0;
  if (r < n) rlen[r] = len;
  for (int off = 32; off > 0; off >>= 1) len = max(len, __shfl_xor(len, off, 64));
  if (lane == 0) width[s] = len;
}
__global__ void k_sell_fill(int n, int nslices, const int *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val,
                            const int *__restrict__ sp, int *__restrict__ scol, double *__restrict__ sval)
{
  const long long s = (long long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (s >= nslices) return;
  const int lane = threadIdx.x & 63;
  const long long r = s * 64 + lane;
  const int w = sp[s + 1] - sp[s];
  const int p0 = (r < n) ? rowptr[r] : 0, len = (r < n) ? rowptr[r + 1] - p0 : 0;
  const long long sb = (long long)sp[s] * 64;
  for (int j = 0; j < w; j++) {
    const long long p = sell_pos(sb, w, j, lane);
    scol[p] = (j < len) ? col[p0 + j] : 0;
    sval[p] = (j < len) ? val[p0 + j] : 0.0;
  }
}

int pick_lanes(long long nnz, int n)
{
  double mean = n > 0 ? (double)nnz / n : 1.0;
  int g = 2;
  while (g < 64 && g < mean) g <<= 1;      // smallest power of two >= mean row length
  return g;
}

// ---- synthetic generators, built directly in device memory -------------------------------------
// 3-D 7-point Laplacian, ex19.c:47-78: diag 6, off -1, natural ordering (x fastest), Dirichlet.
// Local rows = planes [z0,z0+nzl). Entries whose column is owned by another slab go to the
// off-diagonal block with ghost index: lower plane -> [0,plane), upper plane -> [nlow, nlow+plane).
__global__ void k_lap3d_count(int nx, int ny, int nz, int z0, int nzl, int *cnt_d, int *cnt_o)
{
  long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long n = (long long)nx * ny * nzl;
  if (r >= n) return;
  int i = (int)(r % nx); long long t = r / nx; int j = (int)(t % ny); int kl = (int)(t / ny); int k = z0 + kl;
  int cd = 1, co = 0;
  if (k > 0) { if (kl > 0) cd++; else co++; }
  if (j > 0) cd++;
  if (i > 0) cd++;
  if (i < nx - 1) cd++;
  if (j < ny - 1) cd++;
  if (k < nz - 1) { if (kl < nzl - 1) cd++; else co++; }
  cnt_d[r] = cd; cnt_o[r] = co;
}

__global__ void k_lap3d_fill(int nx, int ny, int nz, int z0, int nzl, const int *rp_d, int *col_d, double *val_d,
                             const int *rp_o, int *col_o, double *val_o)
{
  long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long plane = (long long)nx * ny, n = plane * nzl;
  if (r >= n) return;
  int i = (int)(r % nx); long long t = r / nx; int j = (int)(t % ny); int kl = (int)(t / ny); int k = z0 + kl;
  int p = rp_d[r], q = rp_o[r];
  const int nlow = (z0 > 0) ? (int)plane : 0;
  if (k > 0) { if (kl > 0) { col_d[p] = (int)(r - plane); val_d[p++] = -1.0; } else { col_o[q] = (int)(r); val_o[q++] = -1.0; } }
  if (j > 0) { col_d[p] = (int)(r - nx); val_d[p++] = -1.0; }
  if (i > 0) { col_d[p] = (int)(r - 1); val_d[p++] = -1.0; }
  col_d[p] = (int)r; val_d[p++] = 6.0;
  if (i < nx - 1) { col_d[p] = (int)(r + 1); val_d[p++] = -1.0; }
  if (j < ny - 1) { col_d[p] = (int)(r + nx); val_d[p++] = -1.0; }
  if (k < nz - 1) { if (kl < nzl - 1) { col_d[p] = (int)(r + plane); val_d[p++] = -1.0; } else { col_o[q] = nlow + (int)(r - (n - plane)); val_o[q++] = -1.0; } }
}

// 2-D 5-point Laplacian, ex2.c:44-51 (single slab): diag 4, off -1, II=i*n+j
__global__ void k_lap2d_count(int n, int m, int *cnt)
{
  long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= (long long)n * m) return;
  int i = (int)(r / n), j = (int)(r % n);
  cnt[r] = 1 + (i > 0) + (i < m - 1) + (j > 0) + (j < n - 1);
}
__global__ void k_lap2d_fill(int n, int m, const int *rp, int *col, double *val)
{
  long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= (long long)n * m) return;
  int i = (int)(r / n), j = (int)(r % n);
  int p = rp[r];
  if (i > 0) { col[p] = (int)(r - n); val[p++] = -1.0; }
  if (j > 0) { col[p] = (int)(r - 1); val[p++] = -1.0; }
  col[p] = (int)r; val[p++] = 4.0;
  if (j < n - 1) { col[p] = (int)(r + 1); val[p++] = -1.0; }
  if (i < m - 1) { col[p] = (int)(r + n); val[p++] = -1.0; }
}

__global__ void k_rows_with_entries(int n, const int *rp, int *flag)
{
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) flag[r] = (rp[r + 1] > rp[r]) ? 1 : 0;
}
__global__ void k_compact_rows(int n, const int *rp, const int *pos, int *rows, int *rp_c)
{
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n && rp[r + 1] > rp[r]) { rows[pos[r]] = r; rp_c[pos[r]] = rp[r]; }
}

// Exclusive prefix sum of ints (assembly only: row pointers from row counts). Three launches: sums of 2048-item tiles, an exclusive scan
// of the tile sums by one workgroup, then every tile scans itself (wave shuffles, 8 items per thread) starting from its offset.
constexpr int SCAN_TILE = 2048;
__device__ __forceinline__ int scan_wave_incl(int v)
{
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d, 64); if ((int)(threadIdx.x & 63) >= d) v += t; }
  return v;
}
__global__ __launch_bounds__(256) void k_scan_tile_sums(const int *__restrict__ in, long long n, int *__restrict__ sums)
{
  __shared__ int ws[4];
  const long long base = (long long)blockIdx.x * SCAN_TILE;
  int s = 0;
  for (int i = threadIdx.x; i < SCAN_TILE; i += 256) { const long long g = base + i; if (g < n) s += in[g]; }
  for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
__global__ __launch_bounds__(1024) void k_scan_sums(int *__restrict__ sums, int ntiles)
{
  __shared__ int ws[16];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int b0 = 0; b0 < ntiles; b0 += 1024) {
    const int i = b0 + threadIdx.x;
    const int v = i < ntiles ? sums[i] : 0;
    int inc = scan_wave_incl(v);
    if ((threadIdx.x & 63) == 63) ws[threadIdx.x >> 6] = inc;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < (int)(threadIdx.x >> 6); w++) woff += ws[w];
    const int c = carry;
    if (i < ntiles) sums[i] = c + woff + inc - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = c + woff + inc;
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void k_scan_tiles(const int *__restrict__ in, int *__restrict__ out, long long n, const int *__restrict__ offs)
{
  __shared__ int ws[4];
  const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * 8;
  int v[8], t = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) { const long long g = base + j; v[j] = g < n ? in[g] : 0; t += v[j]; }
  const int inc = scan_wave_incl(t);
  if ((threadIdx.x & 63) == 63) ws[threadIdx.x >> 6] = inc;
  __syncthreads();
  int run = offs[blockIdx.x] + inc - t;
  for (int w = 0; w < (int)(threadIdx.x >> 6); w++) run += ws[w];
#pragma unroll
  for (int j = 0; j < 8; j++) { const long long g = base + j; if (g < n) out[g] = run; run += v[j]; }
}
int exclusive_scan_int(hipStream_t st, const int *in, int *out, long long nitems)
{
  if (nitems <= 0) return KS_SUCCESS;
  const int ntiles = (int)((nitems + SCAN_TILE - 1) / SCAN_TILE);
  int *sums = nullptr;
  KS_HIP(hipMalloc(&sums, sizeof(int) * (size_t)ntiles));
  hipLaunchKernelGGL(k_scan_tile_sums, dim3(ntiles), dim3(256), 0, st, in, nitems, sums);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, st, sums, ntiles);
  hipLaunchKernelGGL(k_scan_tiles, dim3(ntiles), dim3(256), 0, st, in, out, nitems, sums);
  hipError_t e = hipGetLastError();
  hipStreamSynchronize(st);
  hipFree(sums);
  KS_HIP(e);
  return KS_SUCCESS;
}

// Build the halo plan from the sorted list of needed global columns (garray, host).
// Owners are found from the allgathered row_start array; every rank tells its owners which rows it needs. The collectives and the device
// buffers are here; what is computed between them is ks_csr.cpp's (halo_recv_counts, halo_peers, halo_localize_send_idx).
int build_halo_plan(ks_mat A, const std::vector<int> &garray)
{
  ks_ctx ctx = A->ctx;
  const int size = ctx->comm.size, rank = ctx->comm.rank;
  A->nghost = (int)garray.size();
  if (size == 1) { KS_CHECK(garray.empty(), KS_ERR_ARG_OUTOFRANGE, "column index outside [0,n) on a single rank"); return KS_SUCCESS; }
  // 1. ownership ranges
  std::vector<int> starts(size + 1);
  KS_CALL(ks_comm_allgather_host(ctx, &A->row_start, sizeof(int), starts.data()));
  starts[size] = A->n_global;
  // 2. how many entries I need from every owner; 3. everybody learns everybody's needs
  std::vector<int> recv_cnt, all_cnt((size_t)size * size, 0);
  const int owners = ksc::halo_recv_counts(garray, starts, rank, recv_cnt);
  KS_CHECK(owners != ksc::HALO_UNORDERED, KS_ERR_ARG_WRONG, "row blocks must be contiguous and ordered by rank");
  KS_CHECK(owners != ksc::HALO_SELF, KS_ERR_PLIB, "ghost column owned by self");
  KS_CALL(ks_comm_allgather_host(ctx, recv_cnt.data(), (int)(sizeof(int) * size), all_cnt.data()));
  ksc::HaloPeers h;
  ksc::halo_peers(rank, size, recv_cnt.data(), all_cnt.data(), h);
  // 4. exchange index lists: I send my garray segments (global ids) to their owners and receive the ids I must serve
  const int nsend = h.nsend;
  int *d_g = nullptr, *d_sidx = nullptr;
  KS_HIP(hipMalloc(&d_g, sizeof(int) * std::max<size_t>(garray.size(), 1)));
  KS_HIP(hipMalloc(&d_sidx, sizeof(int) * std::max(nsend, 1)));
  KS_HIP(hipMemcpyAsync(d_g, garray.data(), sizeof(int) * garray.size(), hipMemcpyHostToDevice, ctx->stream));
  A->peers.swap(h.peers); A->send_cnt.swap(h.send_cnt); A->recv_cnt.swap(h.recv_cnt); A->send_off.swap(h.send_off); A->recv_off.swap(h.recv_off);
  // in this exchange the roles are swapped: what I will RECEIVE during SpMV (ghost segments) is what I SEND now (their ids)
  KS_CALL(ks_comm_exchange(ctx, (int)A->peers.size(), A->peers.data(), d_g, A->recv_off.data(), A->recv_cnt.data(),
                           d_sidx, A->send_off.data(), A->send_cnt.data(), (int)sizeof(int)));
  std::vector<int> sidx(std::max(nsend, 1));
  KS_HIP(hipMemcpyAsync(sidx.data(), d_sidx, sizeof(int) * nsend, hipMemcpyDeviceToHost, ctx->stream));
  KS_HIP(ks_sync(ctx));
  KS_CHECK(ksc::halo_localize_send_idx(A->row_start, A->n, nsend, sidx.data()) == 0, KS_ERR_PLIB, "peer requested a row this rank does not own");
  KS_HIP(hipMemcpy(d_sidx, sidx.data(), sizeof(int) * nsend, hipMemcpyHostToDevice));
  A->send_idx = d_sidx; A->nsend = nsend;
  if (A->sharded_transpose) { try { A->h_send_idx.assign(sidx.begin(), sidx.begin() + nsend); } catch (const std::exception &e) { KS_FAIL(KS_ERR_MEM, "KS_MAT_SHARDED_TRANSPOSE: %s", e.what()); } }
  KS_HIP(hipMalloc(&A->send_buf, sizeof(double) * std::max(nsend, 1)));
  KS_HIP(hipMalloc(&A->ghost, sizeof(double) * std::max(A->nghost, 1)));
  hipFree(d_g);
  return KS_SUCCESS;
}

int compact_offdiag_rows(ks_mat A)
{
  // rows with off-diagonal entries -> compressed row list + compressed rowptr (PETSc "compressed row" AIJ)
  ks_ctx ctx = A->ctx;
  if (A->nnz_o == 0) { A->n_orows = 0; return KS_SUCCESS; }
  int *flag = nullptr, *pos = nullptr;
  KS_HIP(hipMalloc(&flag, sizeof(int) * (A->n + 1))); KS_HIP(hipMalloc(&pos, sizeof(int) * (A->n + 1)));
  KS_HIP(hipMemsetAsync(flag, 0, sizeof(int) * (A->n + 1), ctx->stream));
  hipLaunchKernelGGL(k_rows_with_entries, dim3((A->n + 255) / 256), dim3(256), 0, ctx->stream, A->n, A->o_rowptr, flag);
  KS_CALL(exclusive_scan_int(ctx->stream, flag, pos, A->n + 1));
  int norows = 0; KS_HIP(hipMemcpy(&norows, pos + A->n, sizeof(int), hipMemcpyDeviceToHost));
  int *rows = nullptr, *rp_c = nullptr;
  KS_HIP(hipMalloc(&rows, sizeof(int) * std::max(norows, 1))); KS_HIP(hipMalloc(&rp_c, sizeof(int) * (norows + 1)));
  hipLaunchKernelGGL(k_compact_rows, dim3((A->n + 255) / 256), dim3(256), 0, ctx->stream, A->n, A->o_rowptr, pos, rows, rp_c);
  int last = (int)A->nnz_o; KS_HIP(hipMemcpyAsync(rp_c + norows, &last, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  KS_HIP(ks_sync(ctx));
  hipFree(flag); hipFree(pos); hipFree(A->o_rowptr);
  A->o_rowptr = rp_c; A->o_rows = rows; A->n_orows = norows;
  return KS_SUCCESS;
}

// ---- XCD-sliced layout ---------------------------------------------------------------------------------------------
// Measured on MI355X (scripts/micro/gather_xcd.hip): 1.6e8 random 8-byte gathers from a 40 MB vector take 2.83 ms when
// every XCD gathers from all of it (each one a 128-B line from the Infinity Cache) and 1.23 ms when the workgroups of
// XCD i (blockIdx % 8 == i) only touch the i-th eighth (L2 hits).
__global__ void k_slice_count(int n, int nslice, int slice_cols, const int *__restrict__ rp, const int *__restrict__ col, int *__restrict__ cnt)
{
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > n) return;
  for (int s = 0; s < nslice; s++) cnt[(size_t)s * (n + 1) + r] = 0;
  if (r == n) return;
  for (int p = rp[r]; p < rp[r + 1]; p++) cnt[(size_t)(col[p] / slice_cols) * (n + 1) + r]++;
}
__global__ void k_slice_fill(int n, int nslice, int slice_cols, const int *__restrict__ rp, const int *__restrict__ col, const double *__restrict__ val,
                             const int *__restrict__ srp, const long long *__restrict__ base, int *__restrict__ scol, double *__restrict__ sval)
{
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  for (int s = 0; s < nslice; s++) {                    // stable: entries keep their order inside (row, slice)
    long long pos = base[s] + srp[(size_t)s * (n + 1) + r];
    for (int p = rp[r]; p < rp[r + 1]; p++) if (col[p] / slice_cols == s) { scol[pos] = col[p]; sval[pos] = val[p]; pos++; }
  }
}
__global__ void k_far_entries(int n, int far, const int *__restrict__ rp, const int *__restrict__ col, unsigned long long *__restrict__ count)
{
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long c = 0;
  if (r < n) for (int p = rp[r]; p < rp[r + 1]; p++) { const long long d = (long long)col[p] - r; if (d > far || d < -far) c++; }
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

// The matrices the binned and XCD-sliced layouts are for: x well beyond an L2 and most entries far from the diagonal (nothing a row-ordered
// sweep could reuse). Measured, 33 nnz/row uniformly random: x = 4 MB CSR 0.118 ms / sliced 0.128 ms; 8 MB 0.379 / 0.247; 16 MB 1.97 / 0.49;
// 40 MB 2.90 / 1.37.
int wide_scatter(ks_mat A, bool *wide)
{
  ks_ctx ctx = A->ctx;
  const int n = A->n;
  *wide = false;
  if (n < 4096 || A->nnz_d == 0 || (double)n * 8.0 < 6.0 * 1048576.0 || A->nnz_d < 8LL * n) return KS_SUCCESS;
  unsigned long long *cnt = nullptr, h = 0;
  KS_HIP(hipMalloc(&cnt, sizeof(unsigned long long))); KS_HIP(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_far_entries, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, n / 16, A->d_rowptr, A->d_col, cnt);
  KS_HIP(hipMemcpyAsync(&h, cnt, sizeof(h), hipMemcpyDeviceToHost, ctx->stream)); KS_HIP(ks_sync(ctx)); hipFree(cnt);
  *wide = (double)h >= 0.5 * (double)A->nnz_d;
  return KS_SUCCESS;
}

// The binned, XCD-sliced and dictionary layouts are the only copy of the diagonal block kept: its diagonal and infinity norm are taken from
// the CSR arrays before those are released (local rows only: no collective inside the per-rank layout choice).
int release_csr(ks_mat A, bool keep_val = false)            // keep_val: the windowed layout walks d_val as it is
{
  double *d = nullptr, nrm = 0.0;
  KS_HIP(hipMalloc(&d, sizeof(double) * A->n));
  int rc = ks_mat_get_diagonal_internal(A, d);
  if (!rc) rc = ks_mat_norm_inf_local(A, &nrm);            // waits for the stream: the diagonal is complete too
  if (rc) { hipFree(d); return rc; }
  A->diag_cache = d; A->norm_inf_cache = nrm;
  hipFree(A->d_col); A->d_col = nullptr;
  if (!keep_val) { hipFree(A->d_val); A->d_val = nullptr; }
  return KS_SUCCESS;
}

// The windowed CSR layout: the plan is made on the host (ks_csr.cpp) from the row pointers and columns of the diagonal block, copied back once;
// the values stay where they are. Out of host or device memory: the matrix stays CSR.
int build_window(ks_mat A)
{
  ks_ctx ctx = A->ctx;
  const int n = A->n;
  const long long nnz = A->nnz_d;
  auto drop = [&]() {
    hipFree(A->wn_codes); hipFree(A->wn_dcol); hipFree(A->wn_segptr); hipFree(A->wn_seg); hipFree(A->wn_dbase);
    A->wn_codes = nullptr; A->wn_dcol = A->wn_segptr = A->wn_seg = A->wn_dbase = nullptr;
    (void)hipGetLastError();
    return KS_SUCCESS;
  };
  try {
  std::vector<int> rp(n + 1), col(nnz);
  KS_HIP(hipMemcpyAsync(rp.data(), A->d_rowptr, sizeof(int) * (n + 1), hipMemcpyDeviceToHost, ctx->stream));
  KS_HIP(hipMemcpyAsync(col.data(), A->d_col, sizeof(int) * nnz, hipMemcpyDeviceToHost, ctx->stream));
  KS_HIP(ks_sync(ctx));
  ksc::WindowPlan p;
  ksc::csr_window_plan(n, rp.data(), col.data(), WIN_ROWS, WIN_SMAX, CW_PAD, p);
  if (p.dcol.size() >= 2147483647u) return KS_SUCCESS;   // positions in the direct column array are 32-bit
  const bool ok = upload(&A->wn_codes, p.codes) == hipSuccess && upload(&A->wn_dcol, p.dcol) == hipSuccess && upload(&A->wn_segptr, p.segptr) == hipSuccess &&
                  upload(&A->wn_seg, p.seg) == hipSuccess && upload(&A->wn_dbase, p.dbase) == hipSuccess;
  if (!ok) return drop();
  KS_CALL(release_csr(A, true));
  A->layout = KS_MAT_LAYOUT_WINDOW;
  A->wn_blocks = p.blocks; A->wn_direct_blocks = p.direct_blocks; A->wn_entries = p.window_entries; A->wn_direct_entries = p.direct_entries; A->wn_segments = p.total_segments;
  } catch (const std::exception &) { return drop(); }
  return KS_SUCCESS;
}

// The binned layout: geometry and plan are made on the host (ks_csr.cpp) from the CSR arrays of the diagonal block, copied back once. A size the
// layout does not take, or no host or device memory for the build: the matrix stays CSR and the other layouts take it.
int build_binned(ks_mat A)
{
  ks_ctx ctx = A->ctx;
  const int n = A->n;
  const long long nnz = A->nnz_d;
  ksc::BinnedGeometry g;
  ksc::binned_geometry(n, nnz, ctx->num_cu, BN_CS_MAX, BN_SEG_PAD, g);
  if (g.status) return KS_SUCCESS;
  if (ks_binned_lds1(g.cs, g.wb) > 156 * 1024 || ks_binned_lds2(g.wr) > 156 * 1024) return KS_SUCCESS;   // the offset rows of more than ~20 M local rows no longer fit LDS next to the piece of x: the XCD-sliced layout takes those
  try {                                               // the build holds about 25 bytes per nonzero in host memory: without it the sliced layout takes the matrix
  std::vector<int> rp(n + 1), col(nnz); std::vector<double> val(nnz);
  KS_HIP(hipMemcpyAsync(rp.data(), A->d_rowptr, sizeof(int) * (n + 1), hipMemcpyDeviceToHost, ctx->stream));
  KS_HIP(hipMemcpyAsync(col.data(), A->d_col, sizeof(int) * nnz, hipMemcpyDeviceToHost, ctx->stream));
  KS_HIP(hipMemcpyAsync(val.data(), A->d_val, sizeof(double) * nnz, hipMemcpyDeviceToHost, ctx->stream));
  KS_HIP(ks_sync(ctx));
  ksc::BinnedPlan p;
  ksc::binned_plan(n, rp.data(), col.data(), val.data(), g, BN_SEG_PAD, p);
  KS_CHECK(p.status != ksc::BINNED_ORDERS, KS_ERR_PLIB, "binned layout: the two orders disagree (%lld vs %lld entries)", p.sbase[g.ns], p.entries);
  std::vector<int>().swap(col); std::vector<double>().swap(val);
  KS_HIP(upload(&A->bn_col16, p.col16)); KS_HIP(upload(&A->bn_row16, p.row16)); KS_HIP(upload(&A->bn_val, p.val2));
  KS_HIP(upload(&A->bn_off1, p.off1)); KS_HIP(upload(&A->bn_off2t, p.off2t)); KS_HIP(upload(&A->bn_wseg, p.wseg));
  KS_HIP(upload(&A->bn_sbase, p.sbase)); KS_HIP(upload(&A->bn_off2, p.off2)); KS_HIP(upload(&A->bn_log2, p.log2));
  KS_HIP(hipMalloc(&A->bn_g, sizeof(double) * std::max<long long>(p.entries, 1)));
  KS_HIP(hipMemset(A->bn_g, 0, sizeof(double) * std::max<long long>(p.entries, 1)));
  KS_CALL(ks_binned_prepare(ks_binned_lds1(g.cs, g.wb), ks_binned_lds2(g.wr)));
  KS_CALL(release_csr(A));
  A->layout = KS_MAT_LAYOUT_BINNED; A->bn_ns = g.ns; A->bn_cs = g.cs; A->bn_wb = g.wb; A->bn_wr = g.wr; A->bn_nwin = p.nwin; A->bn_entries = p.entries;
  } catch (const std::exception &) {                    // out of host memory (or anything else the build throws): the other layouts take the matrix
    hipFree(A->bn_col16); hipFree(A->bn_row16); hipFree(A->bn_val); hipFree(A->bn_g); hipFree(A->bn_off1); hipFree(A->bn_off2t); hipFree(A->bn_wseg); hipFree(A->bn_sbase); hipFree(A->bn_off2); hipFree(A->bn_log2);
    A->bn_col16 = A->bn_row16 = nullptr; A->bn_val = A->bn_g = nullptr; A->bn_off1 = A->bn_off2t = A->bn_wseg = nullptr; A->bn_sbase = nullptr; A->bn_off2 = A->bn_log2 = nullptr;
    (void)hipGetLastError();
  }
  return KS_SUCCESS;
}

int build_sliced(ks_mat A)
{
  ks_ctx ctx = A->ctx;
  const int n = A->n;
  const int max_slice_rows = 786432;   // 6 MiB of x per slice: the 5 MiB slices of the 40 MB probe ran at the L2 rate
  int P = (int)(((long long)n + 8LL * max_slice_rows - 1) / (8LL * max_slice_rows)); if (P < 1) P = 1;
  KS_CHECK(P <= 8, KS_ERR_SUP, "sliced SpMV layout supports up to %d local rows", 64 * max_slice_rows);
  const int S = 8 * P, sc = (n + S - 1) / S;
  int *cnt = nullptr;
  KS_HIP(hipMalloc(&cnt, sizeof(int) * (size_t)S * (n + 1)));
  KS_HIP(hipMalloc(&A->sl_rowptr, sizeof(int) * (size_t)S * (n + 1)));
  hipLaunchKernelGGL(k_slice_count, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, ctx->stream, n, S, sc, A->d_rowptr, A->d_col, cnt);
  std::vector<long long> base(S + 1, 0);
  for (int s = 0; s < S; s++) {
    KS_CALL(exclusive_scan_int(ctx->stream, cnt + (size_t)s * (n + 1), A->sl_rowptr + (size_t)s * (n + 1), n + 1));
    int tot = 0;
    KS_HIP(hipMemcpyAsync(&tot, A->sl_rowptr + (size_t)s * (n + 1) + n, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    KS_HIP(ks_sync(ctx));
    base[s + 1] = base[s] + tot;
  }
  hipFree(cnt);
  KS_CHECK(base[S] == A->nnz_d, KS_ERR_PLIB, "slice counts do not add up (%lld vs %lld)", base[S], A->nnz_d);
  KS_HIP(hipMalloc(&A->sl_base, sizeof(long long) * (S + 1)));
  KS_HIP(hipMemcpyAsync(A->sl_base, base.data(), sizeof(long long) * (S + 1), hipMemcpyHostToDevice, ctx->stream));
  KS_HIP(ks_sync(ctx));
  KS_HIP(hipMalloc(&A->sl_col, sizeof(int) * A->nnz_d)); KS_HIP(hipMalloc(&A->sl_val, sizeof(double) * A->nnz_d));
  hipLaunchKernelGGL(k_slice_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, S, sc, A->d_rowptr, A->d_col, A->d_val, A->sl_rowptr, A->sl_base, A->sl_col, A->sl_val);
  KS_HIP(hipMalloc(&A->ypart, sizeof(double) * 8 * (size_t)n));
  KS_HIP(hipGetLastError());
  KS_CALL(release_csr(A));
  A->layout = KS_MAT_LAYOUT_SLICED; A->nslice = S; A->slice_cols = sc;
  return KS_SUCCESS;
}

// The row-pattern form of the dictionary layout (see k_spmv_dict): the distinct rows of codes are found the way build_dict finds its dictionaries -
// match every row against the sorted table, extend the table by the rows that missed, repeat; every round with a miss adds at least one word, so the
// loop ends with every row matched or with more than 256 words, and then the matrix keeps its codes as they are.
// The pair form of the row-pattern form (ks_dict_pairs.h): whether the matrix qualifies is decided here, once, from the host copies of the dictionaries
// and the pattern table (pats: dict_npat words of dict_w codes); a matrix that does not keeps the one-row walk alone.
static int build_dict_pairs(ks_mat A, const unsigned short *pats)
{
  std::vector<double> dv(256); std::vector<int> dof(256);
  KS_HIP(hipMemcpy(dv.data(), A->dc_val, sizeof(double) * 256, hipMemcpyDeviceToHost));
  KS_HIP(hipMemcpy(dof.data(), A->dc_off, sizeof(int) * 256, hipMemcpyDeviceToHost));
  const ksp::PairPlan P = ksp::dict_pair_plan(A->dict_w, A->dict_npat, pats, dof.data(), A->dict_noff, dv.data(), A->dict_nval);
  if (!P.ok) return KS_SUCCESS;
  KS_HIP(hipMalloc(&A->pr_coef, sizeof(double) * P.coef.size())); KS_HIP(hipMalloc(&A->pr_mask, sizeof(unsigned) * P.mask.size()));
  KS_HIP(hipMemcpy(A->pr_coef, P.coef.data(), sizeof(double) * P.coef.size(), hipMemcpyHostToDevice));
  KS_HIP(hipMemcpy(A->pr_mask, P.mask.data(), sizeof(unsigned) * P.mask.size(), hipMemcpyHostToDevice));
  A->pr_args = P.args; A->pr_ok = true;
  return KS_SUCCESS;
}

int build_dict_patterns(ks_mat A)
{
  ks_ctx ctx = A->ctx;
  const int n = A->n, wpr = A->dict_w / 2, cap = 4096;
  const size_t nidx = ((size_t)n + 255) / 256 * 256;
  using Word = std::vector<unsigned>;
  std::vector<Word> table;                                                 // sorted
  unsigned char *rowpat = nullptr; unsigned *d_pats = nullptr, *m_words = nullptr; int *d_miss = nullptr;
  auto cleanup = [&]() { hipFree(rowpat); hipFree(d_pats); hipFree(m_words); hipFree(d_miss); };
  KS_HIP(hipMalloc(&rowpat, nidx)); KS_HIP(hipMalloc(&d_pats, sizeof(unsigned) * 256 * wpr));
  KS_HIP(hipMalloc(&m_words, sizeof(unsigned) * (size_t)cap * wpr)); KS_HIP(hipMalloc(&d_miss, sizeof(int) * 2));
  KS_HIP(hipMemsetAsync(rowpat, 0, nidx, ctx->stream));
  std::vector<unsigned> flat, got;
  bool done = false;
  while (!done) {
    flat.clear();
    for (const Word &w : table) flat.insert(flat.end(), w.begin(), w.end());
    KS_HIP(hipMemsetAsync(d_miss, 0, sizeof(int) * 2, ctx->stream));
    if (!flat.empty()) KS_HIP(hipMemcpyAsync(d_pats, flat.data(), sizeof(unsigned) * flat.size(), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_dict_match, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, wpr, (const unsigned *)A->dc_codes, d_pats, (int)table.size(),
                       rowpat, d_miss, m_words, cap);
    int miss[2] = {0, 0};
    KS_HIP(hipMemcpyAsync(miss, d_miss, sizeof(int) * 2, hipMemcpyDeviceToHost, ctx->stream));
    KS_HIP(ks_sync(ctx));
    if (miss[0] == 0) { done = true; break; }
    const int m = std::min(miss[0], cap);
    got.resize((size_t)m * wpr);
    KS_HIP(hipMemcpy(got.data(), m_words, sizeof(unsigned) * got.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < m; i++) table.emplace_back(got.begin() + (size_t)i * wpr, got.begin() + (size_t)(i + 1) * wpr);
    std::sort(table.begin(), table.end()); table.erase(std::unique(table.begin(), table.end()), table.end());
    if (table.size() > 256) break;                                         // too many distinct rows: the 2-byte codes stay
  }
  if (!done) { cleanup(); return KS_SUCCESS; }
  A->dc_rowpat = rowpat; rowpat = nullptr; A->dc_pats = (unsigned short *)d_pats; d_pats = nullptr; A->dict_npat = (int)table.size();
  hipFree(A->dc_codes); A->dc_codes = nullptr;
  cleanup();
  flat.clear();
  for (const Word &w : table) flat.insert(flat.end(), w.begin(), w.end());
  return build_dict_pairs(A, (const unsigned short *)flat.data());
}

// Try the dictionary layout (see k_spmv_dict); offsets_only: the offset-dictionary form at once. Needs the CSR arrays of the diagonal block on the device.
int build_dict(ks_mat A, bool offsets_only)
{
  ks_ctx ctx = A->ctx;
  bool value_mode = !offsets_only;
  const int n = A->n;
  int *d_int = nullptr;
  KS_HIP(hipMalloc(&d_int, sizeof(int) * 4));
  KS_HIP(hipMemsetAsync(d_int, 0, sizeof(int) * 4, ctx->stream));
  hipLaunchKernelGGL(k_max_rowlen, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, A->d_rowptr, d_int + 2);
  int maxlen = 0;
  KS_HIP(hipMemcpyAsync(&maxlen, d_int + 2, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  KS_HIP(ks_sync(ctx));
  if (maxlen > 32 || maxlen == 0) { hipFree(d_int); return KS_SUCCESS; }
  const int W = maxlen <= 8 ? 8 : (maxlen <= 16 ? 16 : 32);                // 32: 27-point stencils
  if ((double)W * n > 4.0 * (double)A->nnz_d + 4096.0) { hipFree(d_int); return KS_SUCCESS; }   // mostly padding: nothing to gain
  const int cap = 4096;
  unsigned short *codes = nullptr; long long *d_bits = nullptr, *m_bits = nullptr; int *d_offs = nullptr, *m_off = nullptr;
  KS_HIP(hipMalloc(&codes, sizeof(unsigned short) * (size_t)n * W));
  KS_HIP(hipMalloc(&d_bits, sizeof(long long) * 256)); KS_HIP(hipMalloc(&d_offs, sizeof(int) * 256));
  KS_HIP(hipMalloc(&m_bits, sizeof(long long) * cap)); KS_HIP(hipMalloc(&m_off, sizeof(int) * cap));
  unsigned char *codes8 = nullptr; double *vals_out = nullptr;
  auto cleanup = [&]() { hipFree(d_int); hipFree(codes); hipFree(d_bits); hipFree(d_offs); hipFree(m_bits); hipFree(m_off); hipFree(codes8); hipFree(vals_out); };
  const size_t nslot = (size_t)((n + 63) / 64) * 64 * W;
  std::vector<long long> vals; std::vector<int> offs;                   // sorted candidate dictionaries
  bool done = false;
  while (!done) {                                                          // every round with a miss adds a value or an offset: ends coded, or with a dictionary full
    KS_HIP(hipMemsetAsync(d_int, 0, sizeof(int) * 2, ctx->stream));
    if (!vals.empty()) KS_HIP(hipMemcpyAsync(d_bits, vals.data(), sizeof(long long) * vals.size(), hipMemcpyHostToDevice, ctx->stream));
    if (!offs.empty()) KS_HIP(hipMemcpyAsync(d_offs, offs.data(), sizeof(int) * offs.size(), hipMemcpyHostToDevice, ctx->stream));
    if (!value_mode && !codes8) {
      KS_HIP(hipMalloc(&codes8, nslot)); KS_HIP(hipMalloc(&vals_out, sizeof(double) * nslot));
      KS_HIP(hipMemsetAsync(vals_out, 0, sizeof(double) * nslot, ctx->stream));
    }
    hipLaunchKernelGGL(k_dict_encode, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, W, A->d_rowptr, A->d_col, A->d_val,
                       d_bits, value_mode ? (int)vals.size() : -1, d_offs, (int)offs.size(), codes, d_int, m_bits, m_off, cap, codes8, vals_out);
    int miss[2] = {0, 0};
    KS_HIP(hipMemcpyAsync(miss, d_int, sizeof(int) * 2, hipMemcpyDeviceToHost, ctx->stream));
    KS_HIP(ks_sync(ctx));
    if (miss[0] == 0) { done = true; break; }
    const int got = std::min(miss[0], cap);
    std::vector<long long> mb(got); std::vector<int> mo(got);
    KS_HIP(hipMemcpy(mb.data(), m_bits, sizeof(long long) * got, hipMemcpyDeviceToHost));
    KS_HIP(hipMemcpy(mo.data(), m_off, sizeof(int) * got, hipMemcpyDeviceToHost));
    if (value_mode) { vals.insert(vals.end(), mb.begin(), mb.end()); std::sort(vals.begin(), vals.end()); vals.erase(std::unique(vals.begin(), vals.end()), vals.end()); }
    offs.insert(offs.end(), mo.begin(), mo.end()); std::sort(offs.begin(), offs.end()); offs.erase(std::unique(offs.begin(), offs.end()), offs.end());
    if (value_mode && vals.size() > 255) { value_mode = false; vals.clear(); }        // too many values: keep them in full, compress the indices only
    if (offs.size() > (value_mode ? 256u : 255u)) break;                 // not a dictionary matrix
  }
  if (!done) { cleanup(); return KS_SUCCESS; }
  if (!value_mode) {
    std::vector<int> dof(256, 0);
    for (size_t i = 0; i < offs.size(); i++) dof[i] = offs[i];
    KS_HIP(hipMalloc(&A->dc_off, sizeof(int) * 256));
    KS_HIP(hipMemcpy(A->dc_off, dof.data(), sizeof(int) * 256, hipMemcpyHostToDevice));
    A->dc_codes8 = codes8; codes8 = nullptr; A->dc_vals = vals_out; vals_out = nullptr;
    A->layout = KS_MAT_LAYOUT_ODICT; A->dict_w = W; A->dict_nval = 0; A->dict_noff = (int)offs.size();
    cleanup();
    return KS_SUCCESS;
  }
  std::vector<double> dv(256, 0.0); std::vector<int> dof(256, 0);
  for (size_t i = 0; i < vals.size(); i++) memcpy(&dv[i], &vals[i], sizeof(double));
  for (size_t i = 0; i < offs.size(); i++) dof[i] = offs[i];
  KS_HIP(hipMalloc(&A->dc_val, sizeof(double) * 256)); KS_HIP(hipMalloc(&A->dc_off, sizeof(int) * 256));
  KS_HIP(hipMemcpy(A->dc_val, dv.data(), sizeof(double) * 256, hipMemcpyHostToDevice));
  KS_HIP(hipMemcpy(A->dc_off, dof.data(), sizeof(int) * 256, hipMemcpyHostToDevice));
  A->dc_codes = codes; codes = nullptr;
  A->layout = KS_MAT_LAYOUT_DICT; A->dict_w = W; A->dict_nval = (int)vals.size(); A->dict_noff = (int)offs.size();
  cleanup();
  return ctx->dbg.no_dict_patterns ? KS_SUCCESS : build_dict_patterns(A);
}

// Build the SELL-64 copy of the diagonal block when its padding is small (<= 12.5 % extra entries) or it is forced.
int build_sell(ks_mat A, bool forced)
{
  ks_ctx ctx = A->ctx;
  const int ns = (A->n + 63) / 64;
  int *width = nullptr;
  KS_HIP(hipMalloc(&width, sizeof(int) * (ns + 1)));
  KS_HIP(hipMalloc(&A->s_len, sizeof(int) * A->n));
  KS_HIP(hipMalloc(&A->s_ptr, sizeof(int) * (ns + 1)));
  KS_HIP(hipMemsetAsync(width + ns, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL(k_sell_widths, dim3((ns + 3) / 4), dim3(256), 0, ctx->stream, A->n, ns, A->d_rowptr, width, A->s_len);
  KS_CALL(exclusive_scan_int(ctx->stream, width, A->s_ptr, ns + 1));
  int total = 0;
  KS_HIP(hipMemcpy(&total, A->s_ptr + ns, sizeof(int), hipMemcpyDeviceToHost));
  hipFree(width);
  const long long entries = (long long)total * 64;
  const bool ok = forced || (double)entries <= 1.125 * (double)A->nnz_d + 64.0 * 64.0;
  if (!ok || entries <= 0) { hipFree(A->s_len); hipFree(A->s_ptr); A->s_len = A->s_ptr = nullptr; return KS_SUCCESS; }
  KS_HIP(hipMalloc(&A->s_col, sizeof(int) * entries));
  KS_HIP(hipMalloc(&A->s_val, sizeof(double) * entries));
  hipLaunchKernelGGL(k_sell_fill, dim3((ns + 3) / 4), dim3(256), 0, ctx->stream, A->n, ns, A->d_rowptr, A->d_col, A->d_val, A->s_ptr, A->s_col, A->s_val);
  KS_HIP(ks_sync(ctx));
  KS_HIP(hipGetLastError());
  A->layout = KS_MAT_LAYOUT_SELL; A->nslices = ns; A->s_entries = entries;
  // the CSR copy of the diagonal block is no longer needed on the device
  hipFree(A->d_col); hipFree(A->d_val); A->d_col = nullptr; A->d_val = nullptr;
  return KS_SUCCESS;
}

// The device layout of the diagonal block, chosen at assembly by every creation path: wide-scatter matrices get the binned layout, or the
// XCD-sliced one where the binned build declines; the others a dictionary form, SELL-64 when its padding is small, or CSR. KSGPU_SPMV=<name>
// forces one (tests and A/B legs); a forced layout that cannot be built falls through to SELL-64 under the padding rule, or CSR. window (the windowed
// CSR layout) is built only when forced: for any matrix with rows and entries, without the dictionary and SELL attempts (all its blocks may be
// direct). No automatic rule picks it: the product has not been timed against the CSR kernel it would replace.
int choose_layout(ks_mat A)
{
  enum { AUTO, CSR, CSRVEC, CSRREGS, SELL, DICT, ODICT, BINNED, SLICED, WINDOW };
  static const char *const names[] = {"", "csr", "csrvec", "csrregs", "sell", "dict", "odict", "binned", "sliced", "window"};
  const char *force = getenv("KSGPU_SPMV");
  int want = AUTO;
  if (force) {
    want = -1;
    for (int i = CSR; i <= WINDOW; i++) if (!strcmp(force, names[i])) want = i;
    KS_CHECK(want >= 0, KS_ERR_ARG_WRONG, "KSGPU_SPMV=%s: not one of csr, csrvec, csrregs, sell, dict, odict, binned, sliced, window", force);
  }
  bool wide = false;
  if (want == AUTO) KS_CALL(wide_scatter(A, &wide));
  const bool big = A->n >= 4096 && A->nnz_d > 0;
  if (wide || (want == BINNED && big)) KS_CALL(build_binned(A));
  if ((wide || (want == SLICED && big)) && A->layout == KS_MAT_LAYOUT_CSR) KS_CALL(build_sliced(A));
  if (A->layout != KS_MAT_LAYOUT_CSR) return KS_SUCCESS;
  if (want == CSR || want == CSRVEC || want == CSRREGS) {
    A->csr_form = want == CSRVEC ? ks_mat_s::CSR_VEC : want == CSRREGS ? ks_mat_s::CSR_REGS : ks_mat_s::CSR_AUTO;
    return KS_SUCCESS;
  }
  if (A->n == 0 || A->nnz_d == 0) return KS_SUCCESS;
  if (want == WINDOW) return build_window(A);
  if (want == AUTO || want == DICT || want == ODICT) {
    KS_CALL(build_dict(A, want == ODICT));
    if (A->layout != KS_MAT_LAYOUT_CSR) return release_csr(A);
  }
  return build_sell(A, want == SELL);
}

// The block CSR layout of a matrix that came as block CSR (ks_mat_create_bsr): the rank's own block columns of the arrays it was given, planned on
// the host (ks_csr.cpp) and uploaded; the CSR arrays of the diagonal block, which the assembly has on the device by now, give the diagonal and the
// norm and are released. A failed allocation is KS_ERR_MEM (the caller destroys the matrix).
struct BsrInput { int bs; const int *browptr, *bcol; const double *bval; };
int build_bsr(ks_mat A, const BsrInput &in)
{
  const int bs = in.bs, nb = A->n / bs;
  try {
    ksc::BsrBlocks d; ksc::BsrPlan p;
    ksc::bsr_diag(bs, nb, A->row_start / bs, in.browptr, in.bcol, in.bval, d);
    ksc::bsr_plan(bs, nb, d.browptr.data(), d.bcol.data(), d.bval.data(), bsr_group_rows(bs), bsr_chunk_blocks(bs), CW_PAD, p);
    KS_CHECK(p.blocks * bs * bs == A->nnz_d, KS_ERR_PLIB, "block CSR: %lld blocks of %d x %d against %lld entries of the diagonal block", p.blocks, bs, bs, A->nnz_d);
    const bool ok = upload(&A->bsr_rowptr, p.browptr) == hipSuccess && upload(&A->bsr_col, p.bcol) == hipSuccess && upload(&A->bsr_val, p.val) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); KS_FAIL(KS_ERR_MEM, "block CSR: no device memory for %lld blocks of %d x %d", p.blocks, bs, bs); }
    if (A->n > 0) KS_CALL(release_csr(A));
    A->bsr_bs = bs; A->bsr_nb = nb; A->bsr_blocks = p.blocks;
    A->layout = KS_MAT_LAYOUT_BSR;
  } catch (const std::exception &e) { KS_FAIL(KS_ERR_MEM, "block CSR plan on the host: %s", e.what()); }
  return KS_SUCCESS;
}

} // namespace

extern "C" int ks_mat_create_csr(ks_ctx ctx, int n_local, int row_start, int n_global, const int *rowptr, const int *col, const double *val, ks_mat *out)
{
  return ks_mat_create_csr_flags(ctx, n_local, row_start, n_global, rowptr, col, val, 0u, out);
}

// the one assembly path. local_only: the block is assembled as a matrix of its own whatever the communicator - no halo plan, so no collective
// (every column must then be the rank's own): the transposed diagonal block of a row-sharded matrix
// bsr: the block CSR arrays the CSR arrays are the expansion of (ks_mat_create_bsr) - the diagonal block then gets the block CSR layout, not the chooser's
static int mat_assemble(ks_ctx ctx, int n_local, int row_start, int n_global, const int *rowptr, const int *col, const double *val, unsigned flags, bool local_only, ks_mat *out, const BsrInput *bsr = nullptr)
{
  KS_CHECK(ctx && out, KS_ERR_ARG_NULL, "ctx/out is NULL");
  KS_CHECK((flags & ~(KS_MAT_KEEP_CSR | KS_MAT_SHARDED_TRANSPOSE)) == 0, KS_ERR_ARG_OUTOFRANGE, "unknown matrix creation flags 0x%x", flags);
  KS_CHECK(!(flags & KS_MAT_SHARDED_TRANSPOSE) || (flags & KS_MAT_KEEP_CSR), KS_ERR_ARG_INCOMP, "KS_MAT_SHARDED_TRANSPOSE builds its plan from the CSR arrays of the matrix: it needs KS_MAT_KEEP_CSR");
  KS_CHECK(n_local >= 0 && row_start >= 0 && row_start + n_local <= n_global, KS_ERR_ARG_OUTOFRANGE, "bad row range [%d,%d) of %d", row_start, row_start + n_local, n_global);
  KS_CHECK(rowptr && (rowptr[n_local] == 0 || (col && val)), KS_ERR_ARG_NULL, "CSR arrays are NULL");
  KS_CHECK(rowptr[0] == 0, KS_ERR_ARG_WRONG, "rowptr[0] must be 0");
  KS_HIP(hipSetDevice(ctx->device));
  const long long nnz = rowptr[n_local];
  // split diag / off-diag on the host (setup path; ks_csr.cpp), before anything is allocated
  ksc::BlockSplit s;
  ksc::csr_split_block(n_local, row_start, n_global, rowptr, col, val, s);
  KS_CHECK(s.status != ksc::SPLIT_ROWPTR, KS_ERR_ARG_WRONG, "rowptr not monotone at row %d", s.bad_row);
  KS_CHECK(s.status != ksc::SPLIT_COLUMN, KS_ERR_ARG_OUTOFRANGE, "column %d out of range at row %d", s.bad_col, s.bad_row);
  const std::vector<int> &garray = s.garray;
  ks_mat A = new ks_mat_s(); A->ctx = ctx; A->n = n_local; A->row_start = row_start; A->n_global = n_global; A->nnz = nnz;
  A->nnz_d = (long long)s.col_d.size(); A->nnz_o = (long long)s.col_o.size();
  KS_HIP(upload(&A->d_rowptr, s.rp_d));
  KS_HIP(hipMalloc(&A->d_col, sizeof(int) * (s.col_d.size() + CW_PAD)));
  KS_HIP(hipMalloc(&A->d_val, sizeof(double) * (s.val_d.size() + CW_PAD)));
  KS_HIP(hipMemcpy(A->d_col, s.col_d.data(), sizeof(int) * s.col_d.size(), hipMemcpyHostToDevice));
  KS_HIP(hipMemcpy(A->d_val, s.val_d.data(), sizeof(double) * s.val_d.size(), hipMemcpyHostToDevice));
  A->lanes_per_row = pick_lanes(A->nnz_d, n_local);
  if (A->nnz_o) { KS_HIP(upload(&A->o_rowptr, s.rp_o)); KS_HIP(upload(&A->o_col, s.col_o)); KS_HIP(upload(&A->o_val, s.val_o)); }
  A->sharded_transpose = (flags & KS_MAT_SHARDED_TRANSPOSE) && ctx->comm.size > 1 && !local_only;      // (one rank: the flag changes nothing)
  int rc = KS_SUCCESS;
  if (local_only) { if (!garray.empty()) { ks_set_error("a block assembled on its own has a column outside its rows"); rc = KS_ERR_PLIB; } }
  else rc = build_halo_plan(A, garray);
  if (!rc && A->sharded_transpose) {
    try { A->h_ghosts = garray; } catch (const std::exception &e) { ks_set_error("KS_MAT_SHARDED_TRANSPOSE: %s", e.what()); rc = KS_ERR_MEM; }
  }
  if (!rc) rc = compact_offdiag_rows(A);
  if (!rc) rc = bsr ? build_bsr(A, *bsr) : choose_layout(A);
  if (rc) { ks_mat_destroy(A); return rc; }
  if (flags & KS_MAT_KEEP_CSR) {
    try { A->k_rowptr.assign(rowptr, rowptr + n_local + 1); A->k_col.assign(col, col + nnz); A->k_val.assign(val, val + nnz); }
    catch (const std::exception &e) { ks_mat_destroy(A); KS_FAIL(KS_ERR_MEM, "KS_MAT_KEEP_CSR: %s", e.what()); }
    A->keep_csr = true;
  }
  *out = A;
  return KS_SUCCESS;
}
extern "C" int ks_mat_create_csr_flags(ks_ctx ctx, int n_local, int row_start, int n_global, const int *rowptr, const int *col, const double *val, unsigned flags, ks_mat *out)
{
  return mat_assemble(ctx, n_local, row_start, n_global, rowptr, col, val, flags, false, out);
}
int ks_mat_assemble_local(ks_ctx ctx, int n_local, int row_start, int n_global, const int *rowptr, const int *col, const double *val, ks_mat *out)
{
  return mat_assemble(ctx, n_local, row_start, n_global, rowptr, col, val, 0u, true, out);
}
// MatCreateSeqBAIJWithArrays / MatCreateMPIBAIJWithArrays: the matrix IS ks_mat_create_csr_flags of the expansion (ksc::bsr_expand), apart from the device
// layout of its diagonal block: block CSR for 2 <= bs <= 8 unless KSGPU_SPMV forces one of the chooser's on the expansion
extern "C" int ks_mat_create_bsr(ks_ctx ctx, int bs, int n_local, int row_start, int n_global, const int *browptr, const int *bcol, const double *bval, unsigned flags, ks_mat *out)
{
  KS_CHECK(ctx && out, KS_ERR_ARG_NULL, "ctx/out is NULL");
  KS_CHECK(bs >= 1, KS_ERR_ARG_OUTOFRANGE, "block size %d must be at least 1", bs);
  KS_CHECK(n_local >= 0 && row_start >= 0 && n_global >= 0 && n_local % bs == 0 && row_start % bs == 0 && n_global % bs == 0, KS_ERR_ARG_SIZ,
           "local rows %d, first row %d and global size %d must be multiples of the block size %d", n_local, row_start, n_global, bs);
  KS_CHECK(row_start + (long long)n_local <= n_global, KS_ERR_ARG_OUTOFRANGE, "bad row range [%d,%lld) of %d", row_start, row_start + (long long)n_local, n_global);
  const int nb = n_local / bs;
  KS_CHECK(browptr && (browptr[nb] == 0 || (bcol && bval)), KS_ERR_ARG_NULL, "block CSR arrays are NULL");
  KS_CHECK(browptr[0] == 0, KS_ERR_ARG_WRONG, "rowptr[0] must be 0");
  ksc::BsrExpansion e;
  try { ksc::bsr_expand(bs, nb, n_global / bs, browptr, bcol, bval, e); }
  catch (const std::exception &x) { KS_FAIL(KS_ERR_MEM, "expansion of the block CSR arrays: %s", x.what()); }
  KS_CHECK(e.status != ksc::BSR_ROWPTR, KS_ERR_ARG_WRONG, "rowptr not monotone at block row %d", e.bad_row);
  KS_CHECK(e.status != ksc::BSR_TOO_LARGE, KS_ERR_ARG_OUTOFRANGE, "%d blocks of %d x %d exceed 32-bit PetscInt indices", browptr[nb], bs, bs);
  KS_CHECK(e.status != ksc::BSR_COLUMN, KS_ERR_ARG_OUTOFRANGE, "block column %d out of range at block row %d", e.bad_col, e.bad_row);
  const BsrInput in = {bs, browptr, bcol, bval};
  const bool blocked = bs >= BSR_BS_MIN && bs <= BSR_BS_MAX && !getenv("KSGPU_SPMV");
  return mat_assemble(ctx, n_local, row_start, n_global, e.rp.data(), e.col.data(), e.val.data(), flags, false, out, blocked ? &in : nullptr);
}
extern "C" int ks_mat_get_bsr_info(ks_mat A, int *bs, int *group_block_rows, int *chunk_entries, long long *block_rows, long long *blocks, long long *index_bytes)
{
  KS_CHECK(A && bs && group_block_rows && chunk_entries && block_rows && blocks && index_bytes, KS_ERR_ARG_NULL, "NULL argument");
  *bs = *group_block_rows = *chunk_entries = 0; *block_rows = *blocks = *index_bytes = 0;
  if (A->shell_mult || A->layout != KS_MAT_LAYOUT_BSR) return KS_SUCCESS;
  *bs = A->bsr_bs; *group_block_rows = bsr_group_rows(A->bsr_bs); *chunk_entries = bsr_chunk_blocks(A->bsr_bs) * A->bsr_bs * A->bsr_bs;
  *block_rows = A->bsr_nb; *blocks = A->bsr_blocks; *index_bytes = 4 * A->bsr_blocks + 4 * ((long long)A->bsr_nb + 1);
  return KS_SUCCESS;
}
bool ks_mat_has_transpose_across_ranks(ks_mat A)
{
  if (!A || A->shell_mult) return false;
  if (A->transpose_of) A = A->transpose_of;
  return A->sharded_transpose && A->keep_csr;
}

// MatDuplicate + MatAXPY / MatShift on the kept CSR arrays (ks_csr.cpp), then the ordinary assembly of the result
extern "C" int ks_mat_create_axpy(ks_mat A, double alpha, ks_mat B, unsigned flags, ks_mat *out)
{
  KS_CHECK(A && out, KS_ERR_ARG_NULL, "A/out is NULL");
  KS_CHECK(!A->shell_mult && (!B || !B->shell_mult), KS_ERR_SUP, "MatAXPY of a shell matrix");
  KS_CHECK(A->keep_csr && (!B || B->keep_csr), KS_ERR_ORDER, "MatAXPY needs the CSR arrays of its operands: create them with KS_MAT_KEEP_CSR");
  KS_CHECK(!B || (B->n == A->n && B->row_start == A->row_start && B->n_global == A->n_global && B->ctx == A->ctx), KS_ERR_ARG_INCOMP, "Mismatching row blocks of A (%d rows from %d) and B (%d rows from %d)", A->n, A->row_start, B ? B->n : 0, B ? B->row_start : 0);
  std::vector<int> rp, col; std::vector<double> val;
  bool fits = false;
  try { fits = ksc::csr_axpy(A->n, A->row_start, A->k_rowptr.data(), A->k_col.data(), A->k_val.data(), alpha, B ? B->k_rowptr.data() : nullptr, B ? B->k_col.data() : nullptr, B ? B->k_val.data() : nullptr, rp, col, val); }
  catch (const std::exception &e) { KS_FAIL(KS_ERR_MEM, "MatAXPY on the host: %s", e.what()); }
  KS_CHECK(fits, KS_ERR_ARG_OUTOFRANGE, "the sum exceeds 32-bit PetscInt indices");
  // P of two matrices with a transposed product across ranks has one too (then it keeps its arrays as well: the plan is made from them)
  if (A->sharded_transpose && (!B || B->sharded_transpose)) flags |= KS_MAT_SHARDED_TRANSPOSE | KS_MAT_KEEP_CSR;
  return ks_mat_create_csr_flags(A->ctx, A->n, A->row_start, A->n_global, rp.data(), col.data(), val.data(), flags, out);
}

extern "C" int ks_mat_create_laplacian3d(ks_ctx ctx, int nx, int ny, int nz, int z0, int nzl, ks_mat *out)
{
  KS_CHECK(ctx && out, KS_ERR_ARG_NULL, "ctx/out is NULL");
  KS_CHECK(nx > 0 && ny > 0 && nz > 0 && z0 >= 0 && nzl > 0 && z0 + nzl <= nz, KS_ERR_ARG_OUTOFRANGE, "bad grid %dx%dx%d planes [%d,%d)", nx, ny, nz, z0, z0 + nzl);
  const long long plane = (long long)nx * ny, n = plane * nzl, N = plane * nz;
  KS_CHECK(N * 7 < 2147483647LL && n < 2147483647LL, KS_ERR_ARG_OUTOFRANGE, "problem exceeds 32-bit PetscInt indices");
  KS_HIP(hipSetDevice(ctx->device));
  ks_mat A = new ks_mat_s(); A->ctx = ctx; A->n = (int)n; A->row_start = (int)(plane * z0); A->n_global = (int)N;
  int *cnt_d = nullptr, *cnt_o = nullptr;
  KS_HIP(hipMalloc(&cnt_d, sizeof(int) * (n + 1))); KS_HIP(hipMalloc(&cnt_o, sizeof(int) * (n + 1)));
  KS_HIP(hipMemsetAsync(cnt_d + n, 0, sizeof(int), ctx->stream)); KS_HIP(hipMemsetAsync(cnt_o + n, 0, sizeof(int), ctx->stream));
  const unsigned nb = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_lap3d_count, dim3(nb), dim3(256), 0, ctx->stream, nx, ny, nz, z0, nzl, cnt_d, cnt_o);
  KS_HIP(hipMalloc(&A->d_rowptr, sizeof(int) * (n + 1))); KS_HIP(hipMalloc(&A->o_rowptr, sizeof(int) * (n + 1)));
  KS_CALL(exclusive_scan_int(ctx->stream, cnt_d, A->d_rowptr, n + 1));
  KS_CALL(exclusive_scan_int(ctx->stream, cnt_o, A->o_rowptr, n + 1));
  int nnzd = 0, nnzo = 0;
  KS_HIP(hipMemcpy(&nnzd, A->d_rowptr + n, sizeof(int), hipMemcpyDeviceToHost));
  KS_HIP(hipMemcpy(&nnzo, A->o_rowptr + n, sizeof(int), hipMemcpyDeviceToHost));
  hipFree(cnt_d); hipFree(cnt_o);
  A->nnz_d = nnzd; A->nnz_o = nnzo; A->nnz = (long long)nnzd + nnzo;
  KS_HIP(hipMalloc(&A->d_col, sizeof(int) * (nnzd + CW_PAD))); KS_HIP(hipMalloc(&A->d_val, sizeof(double) * (nnzd + CW_PAD)));
  KS_HIP(hipMalloc(&A->o_col, sizeof(int) * std::max(nnzo, 1))); KS_HIP(hipMalloc(&A->o_val, sizeof(double) * std::max(nnzo, 1)));
  hipLaunchKernelGGL(k_lap3d_fill, dim3(nb), dim3(256), 0, ctx->stream, nx, ny, nz, z0, nzl, A->d_rowptr, A->d_col, A->d_val, A->o_rowptr, A->o_col, A->o_val);
  KS_HIP(ks_sync(ctx));
  A->lanes_per_row = pick_lanes(A->nnz_d, A->n);
  // ghost columns: the plane below (owned by the previous slab) then the plane above
  std::vector<int> garray;
  if (z0 > 0) for (long long c = 0; c < plane; c++) garray.push_back((int)(plane * (z0 - 1) + c));
  if (z0 + nzl < nz) for (long long c = 0; c < plane; c++) garray.push_back((int)(plane * (z0 + nzl) + c));
  int rc = KS_SUCCESS;
  if (ctx->comm.size == 1 && !garray.empty()) { ks_mat_destroy(A); KS_FAIL(KS_ERR_ARG_INCOMP, "a partial slab needs a multi-rank communicator"); }
  rc = build_halo_plan(A, garray);
  if (!rc) rc = compact_offdiag_rows(A);
  if (!rc) rc = choose_layout(A);
  if (rc) { ks_mat_destroy(A); return rc; }
  *out = A;
  return KS_SUCCESS;
}

extern "C" int ks_mat_create_laplacian2d(ks_ctx ctx, int n, int m, ks_mat *out)
{
  KS_CHECK(ctx && out, KS_ERR_ARG_NULL, "ctx/out is NULL");
  KS_CHECK(n > 0 && m > 0 && (long long)n * m * 5 < 2147483647LL, KS_ERR_ARG_OUTOFRANGE, "bad grid %dx%d", n, m);
  KS_CHECK(ctx->comm.size == 1, KS_ERR_SUP, "2-D generator is single-rank");
  KS_HIP(hipSetDevice(ctx->device));
  const long long N = (long long)n * m;
  ks_mat A = new ks_mat_s(); A->ctx = ctx; A->n = (int)N; A->row_start = 0; A->n_global = (int)N;
  int *cnt = nullptr; KS_HIP(hipMalloc(&cnt, sizeof(int) * (N + 1)));
  KS_HIP(hipMemsetAsync(cnt + N, 0, sizeof(int), ctx->stream));
  const unsigned nb = (unsigned)((N + 255) / 256);
  hipLaunchKernelGGL(k_lap2d_count, dim3(nb), dim3(256), 0, ctx->stream, n, m, cnt);
  KS_HIP(hipMalloc(&A->d_rowptr, sizeof(int) * (N + 1)));
  KS_CALL(exclusive_scan_int(ctx->stream, cnt, A->d_rowptr, N + 1));
  int nnz = 0; KS_HIP(hipMemcpy(&nnz, A->d_rowptr + N, sizeof(int), hipMemcpyDeviceToHost));
  hipFree(cnt);
  A->nnz = A->nnz_d = nnz;
  KS_HIP(hipMalloc(&A->d_col, sizeof(int) * (nnz + CW_PAD))); KS_HIP(hipMalloc(&A->d_val, sizeof(double) * (nnz + CW_PAD)));
  hipLaunchKernelGGL(k_lap2d_fill, dim3(nb), dim3(256), 0, ctx->stream, n, m, A->d_rowptr, A->d_col, A->d_val);
  KS_HIP(ks_sync(ctx));
  A->lanes_per_row = pick_lanes(A->nnz_d, A->n);
  { int rc = choose_layout(A); if (rc) { ks_mat_destroy(A); return rc; } }
  *out = A;
  return KS_SUCCESS;
}

extern "C" int ks_mat_destroy(ks_mat A)
{
  if (!A) return KS_SUCCESS;
  if (A->transpose_of) return KS_SUCCESS;     // a transposed view (ks_mat_create_transpose) of an assembled matrix: freed with the matrix it views
  if (A->At) { A->At->transpose_of = nullptr; ks_mat_destroy(A->At); A->At = nullptr; }
  hipSetDevice(A->ctx->device);
  ks_sync(A->ctx);
  hipFree(A->d_rowptr); hipFree(A->d_col); hipFree(A->d_val);
  hipFree(A->o_rowptr); hipFree(A->o_col); hipFree(A->o_val); hipFree(A->o_rows);
  if (A->ctx->halo_stream) hipStreamSynchronize(A->ctx->halo_stream);
  ks_halo_release(A);                 // not collective: waits for the neighbours' last acknowledgements (ks_halo.hip); ks_mat_set_halo(A, KS_HALO_PROVIDER) first is the collective way
  hipFree(A->ghost); hipFree(A->send_idx); hipFree(A->send_buf);
  if (A->sht) {
    hipFree(A->sht->o_rp); hipFree(A->sht->o_row); hipFree(A->sht->o_val); hipFree(A->sht->acc_rows); hipFree(A->sht->acc_ptr); hipFree(A->sht->acc_pos);
    hipFree(A->sht->rsend); hipFree(A->sht->rrecv);
    delete A->sht; A->sht = nullptr;
  }
  hipFree(A->s_ptr); hipFree(A->s_len); hipFree(A->s_col); hipFree(A->s_val);
  hipFree(A->dc_codes); hipFree(A->dc_rowpat); hipFree(A->dc_pats); hipFree(A->dc_val); hipFree(A->dc_off); hipFree(A->dc_codes8); hipFree(A->dc_vals); hipFree(A->pr_coef); hipFree(A->pr_mask);
  hipFree(A->sl_rowptr); hipFree(A->sl_col); hipFree(A->sl_val); hipFree(A->sl_base); hipFree(A->ypart); hipFree(A->diag_cache); hipFree(A->mm_xi);
  hipFree(A->bn_col16); hipFree(A->bn_row16); hipFree(A->bn_val); hipFree(A->bn_g); hipFree(A->bn_off1); hipFree(A->bn_off2t); hipFree(A->bn_wseg); hipFree(A->bn_sbase); hipFree(A->bn_off2); hipFree(A->bn_log2);
  hipFree(A->wn_codes); hipFree(A->wn_dcol); hipFree(A->wn_segptr); hipFree(A->wn_seg); hipFree(A->wn_dbase);
  hipFree(A->bsr_rowptr); hipFree(A->bsr_col); hipFree(A->bsr_val);
  delete A;
  return KS_SUCCESS;
}

// A matrix-free operator whose callback only enqueues work on the context's stream (no host synchronisation, no host reads of
// device results) lets BVMatLanczos / BVMatArnoldi enqueue the whole run ahead, as they do for assembled matrices.
extern "C" int ks_mat_shell_set_enqueue_only(ks_mat A, int flag)
{
  KS_CHECK(A, KS_ERR_ARG_NULL, "Mat is NULL");
  KS_CHECK(A->shell_mult, KS_ERR_ARG_WRONGSTATE, "not a matrix-free operator");
  A->shell_nosync = flag != 0;
  return KS_SUCCESS;
}
extern "C" int ks_mat_get_layout(ks_mat A, int *layout)     // storage of the diagonal block: KS_MAT_LAYOUT_*
{
  KS_CHECK(A && layout, KS_ERR_ARG_NULL, "NULL argument");
  *layout = A->shell_mult ? KS_MAT_LAYOUT_SHELL : A->layout;
  return KS_SUCCESS;
}
extern "C" int ks_mat_get_dict_info(ks_mat A, int *patterns, int *npatterns, int *w, long long *index_bytes)
{
  KS_CHECK(A && patterns && npatterns && w && index_bytes, KS_ERR_ARG_NULL, "NULL argument");
  *patterns = *npatterns = *w = 0; *index_bytes = 0;
  if (A->shell_mult || A->layout != KS_MAT_LAYOUT_DICT) return KS_SUCCESS;
  *w = A->dict_w;
  if (A->dc_rowpat) { *patterns = 1; *npatterns = A->dict_npat; *index_bytes = ((long long)A->n + 255) / 256 * 256; }
  else *index_bytes = 2LL * A->dict_w * A->n;
  return KS_SUCCESS;
}
extern "C" int ks_mat_get_dict_pairs_info(ks_mat A, int *eligible, int *nbases, long long *pair_launches, long long *row_launches)
{
  KS_CHECK(A && eligible && nbases && pair_launches && row_launches, KS_ERR_ARG_NULL, "NULL argument");
  *eligible = *nbases = 0; *pair_launches = *row_launches = 0;
  if (A->shell_mult || A->layout != KS_MAT_LAYOUT_DICT) return KS_SUCCESS;
  *eligible = A->pr_ok ? 1 : 0; *nbases = A->pr_args.nb; *pair_launches = A->pr_launches; *row_launches = A->dc_row_launches;
  return KS_SUCCESS;
}
extern "C" int ks_mat_get_window_info(ks_mat A, int *block_rows, int *max_segments, long long *blocks, long long *direct_blocks, long long *window_entries, long long *index_bytes)
{
  KS_CHECK(A && block_rows && max_segments && blocks && direct_blocks && window_entries && index_bytes, KS_ERR_ARG_NULL, "NULL argument");
  *block_rows = WIN_ROWS; *max_segments = WIN_SMAX;
  *blocks = *direct_blocks = *window_entries = *index_bytes = 0;
  if (A->shell_mult || A->layout != KS_MAT_LAYOUT_WINDOW) return KS_SUCCESS;
  *blocks = A->wn_blocks; *direct_blocks = A->wn_direct_blocks; *window_entries = A->wn_entries;
  *index_bytes = 2 * A->wn_entries + 4 * A->wn_direct_entries + 4 * A->wn_segments;
  return KS_SUCCESS;
}
extern "C" int ks_mat_get_sizes(ks_mat A, int *n_local, int *n_global, long long *nnz_local)
{
  KS_CHECK(A, KS_ERR_ARG_NULL, "Mat is NULL");
  if (n_local) *n_local = A->n;
  if (n_global) *n_global = A->n_global;
  if (nnz_local) *nnz_local = A->nnz;
  return KS_SUCCESS;
}

// MatGetDiagonal: entries (i,i) of the diagonal block, 0 where the pattern has none
__global__ void k_diag_csr(int n, const int *__restrict__ rp, const int *__restrict__ col, const double *__restrict__ val, double *__restrict__ d)
{
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  double v = 0.0;
  for (int p = rp[r]; p < rp[r + 1]; p++) if (col[p] == r) v += val[p];
  d[r] = v;
}
__global__ void k_diag_sell(int n, const int *__restrict__ sp, const int *__restrict__ rlen, const int *__restrict__ col, const double *__restrict__ val, double *__restrict__ d)
{
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const long long s = r >> 6, sb = (long long)sp[s] * 64;
  const int w = sp[s + 1] - sp[s], lane = (int)(r & 63);
  double v = 0.0;
  for (int j = 0; j < rlen[r]; j++) { const long long p = sell_pos(sb, w, j, lane); if (col[p] == r) v += val[p]; }
  d[r] = v;
}
int ks_mat_get_diagonal_internal(ks_mat A, double *d)
{
  ks_ctx ctx = A->ctx;
  KS_CHECK(!A->shell_mult, KS_ERR_SUP, "a matrix-free operator has no stored diagonal");
  if (A->sht) A = A->transpose_of;            // the transposed view of a row-sharded matrix: the diagonal of the matrix it views
  if (A->n == 0) return KS_SUCCESS;
  if (A->diag_cache) { KS_HIP(hipMemcpyAsync(d, A->diag_cache, sizeof(double) * A->n, hipMemcpyDeviceToDevice, ctx->stream)); return KS_SUCCESS; }
  const unsigned nb = (unsigned)((A->n + 255) / 256);
  if (A->layout == KS_MAT_LAYOUT_SELL) hipLaunchKernelGGL(k_diag_sell, dim3(nb), dim3(256), 0, ctx->stream, A->n, A->s_ptr, A->s_len, A->s_col, A->s_val, d);
  else hipLaunchKernelGGL(k_diag_csr, dim3(nb), dim3(256), 0, ctx->stream, A->n, A->d_rowptr, A->d_col, A->d_val, d);
  KS_HIP(hipGetLastError());
  return KS_SUCCESS;
}
// MatNorm(A,NORM_INFINITY): max over rows of the sum of |a_ij| (diagonal and off-diagonal blocks)
__global__ void k_rowabs_csr(int n, const int *__restrict__ rp, const double *__restrict__ val, double *__restrict__ out, int accumulate)
{
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  double v = 0.0;
  for (int p = rp[r]; p < rp[r + 1]; p++) v += fabs(val[p]);
  out[r] = accumulate ? out[r] + v : v;
}
__global__ void k_rowabs_sell(int n, const int *__restrict__ sp, const int *__restrict__ rlen, const double *__restrict__ val, double *__restrict__ out)
{
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const long long s = r >> 6, sb = (long long)sp[s] * 64;
  const int w = sp[s + 1] - sp[s], lane = (int)(r & 63);
  double v = 0.0;
  for (int j = 0; j < rlen[r]; j++) v += fabs(val[sell_pos(sb, w, j, lane)]);
  out[r] = v;
}
__global__ void k_rowabs_rows(int nrows, const int *__restrict__ rows, const int *__restrict__ rp, const double *__restrict__ val, double *__restrict__ out)
{
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nrows) return;
  double v = 0.0;
  for (int p = rp[i]; p < rp[i + 1]; p++) v += fabs(val[p]);
  out[rows[i]] += v;
}
int ks_mat_norm_inf_local(ks_mat A, double *val)          // this rank's rows only
{
  ks_ctx ctx = A->ctx;
  if (A->diag_cache) { *val = A->norm_inf_cache; return KS_SUCCESS; }     // taken before the CSR arrays were released
  double local = 0.0;
  if (A->n > 0) {
    double *w = nullptr;
    KS_HIP(hipMalloc(&w, sizeof(double) * A->n));
    const unsigned nb = (unsigned)((A->n + 255) / 256);
    if (A->layout == KS_MAT_LAYOUT_SELL) hipLaunchKernelGGL(k_rowabs_sell, dim3(nb), dim3(256), 0, ctx->stream, A->n, A->s_ptr, A->s_len, A->s_val, w);
    else hipLaunchKernelGGL(k_rowabs_csr, dim3(nb), dim3(256), 0, ctx->stream, A->n, A->d_rowptr, A->d_val, w, 0);
    if (A->n_orows > 0) hipLaunchKernelGGL(k_rowabs_rows, dim3((unsigned)((A->n_orows + 255) / 256)), dim3(256), 0, ctx->stream, A->n_orows, A->o_rows, A->o_rowptr, A->o_val, w);
    std::vector<double> h(A->n);
    int rc = hipGetLastError() == hipSuccess && hipMemcpyAsync(h.data(), w, sizeof(double) * A->n, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess && ks_sync(ctx) == hipSuccess ? 0 : 1;
    hipFree(w);
    KS_CHECK(!rc, KS_ERR_LIB, "row-sum kernel failed");
    for (double v : h) local = std::max(local, v);
  }
  *val = local;
  return KS_SUCCESS;
}
extern "C" int ks_mat_norm_inf(ks_mat A, double *val)
{
  KS_CHECK(A && val, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(!A->shell_mult, KS_ERR_SUP, "a matrix-free operator has no norm operation");      // MatHasOperation(A,MATOP_NORM) epssolve.c:786
  KS_CHECK(!A->sht, KS_ERR_SUP, "the infinity norm of the transposed view of a row-sharded matrix is not built (it is a 1-norm of the matrix across ranks)");
  ks_ctx ctx = A->ctx;
  KS_HIP(hipSetDevice(ctx->device));
  double local = 0.0;
  KS_CALL(ks_mat_norm_inf_local(A, &local));
  if (ctx->comm.size > 1) {
    std::vector<double> all(ctx->comm.size);
    KS_CALL(ks_comm_allgather_host(ctx, &local, (int)sizeof(double), all.data()));
    for (double v : all) local = std::max(local, v);
  }
  *val = local;
  return KS_SUCCESS;
}

extern "C" int ks_mat_get_diagonal(ks_mat A, double *d_dev)
{
  KS_CHECK(A && d_dev, KS_ERR_ARG_NULL, "NULL argument");
  KS_HIP(hipSetDevice(A->ctx->device));
  return ks_mat_get_diagonal_internal(A, d_dev);
}

// MatLoad of a PETSc binary viewer file (the format of share/slepc/datafiles/matrices/*.petsc): big-endian int32
// header {MAT_FILE_CLASSID = 1211216, rows, cols, nnz}, int32 row lengths, int32 column indices, float64 values.
// Each rank keeps the row block PETSC_DECIDE would give it (n/size rows, the first n%size ranks one more).
namespace {
inline uint32_t be32(const unsigned char *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }
inline double be64f(const unsigned char *p) { uint64_t v = 0; for (int i = 0; i < 8; i++) v = (v << 8) | p[i]; double d; memcpy(&d, &v, 8); return d; }
}
extern "C" int ks_mat_load_petsc_binary(ks_ctx ctx, const char *path, ks_mat *out)
{
  KS_CHECK(ctx && path && out, KS_ERR_ARG_NULL, "NULL argument");
  FILE *f = fopen(path, "rb");
  KS_CHECK(f, KS_ERR_FILE_OPEN, "Cannot open file %s", path);
  std::vector<unsigned char> buf;
  fseek(f, 0, SEEK_END); const long sz = ftell(f); fseek(f, 0, SEEK_SET);
  buf.resize(sz > 0 ? (size_t)sz : 0);
  const size_t got = buf.empty() ? 0 : fread(buf.data(), 1, buf.size(), f);
  fclose(f);
  KS_CHECK(got == buf.size() && buf.size() >= 16, KS_ERR_FILE_UNEXPECTED, "Short read on %s", path);
  KS_CHECK(be32(buf.data()) == 1211216u, KS_ERR_FILE_UNEXPECTED, "Not a Mat object in %s (classid %u)", path, be32(buf.data()));
  const long long rows = (int32_t)be32(buf.data() + 4), cols = (int32_t)be32(buf.data() + 8), nnz = (int32_t)be32(buf.data() + 12);
  KS_CHECK(rows >= 0 && cols == rows && nnz >= 0, KS_ERR_FILE_UNEXPECTED, "Unsupported matrix shape %lld x %lld (nnz %lld) in %s: square sparse matrices only", rows, cols, nnz, path);
  KS_CHECK((long long)buf.size() >= 16 + 4 * rows + 12 * nnz, KS_ERR_FILE_UNEXPECTED, "File %s is truncated", path);
  const unsigned char *pl = buf.data() + 16, *pc = pl + 4 * rows, *pv = pc + 4 * nnz;
  std::vector<long long> start(rows + 1, 0);
  for (long long i = 0; i < rows; i++) {
    const long long len = (int32_t)be32(pl + 4 * i);
    KS_CHECK(len >= 0 && len <= cols, KS_ERR_FILE_UNEXPECTED, "Row %lld of %s has length %lld", i, path, len);
    start[i + 1] = start[i] + len;
  }
  KS_CHECK(start[rows] == nnz, KS_ERR_FILE_UNEXPECTED, "Row lengths of %s do not add up to its nnz", path);
  const int size = ctx->comm.size, rank = ctx->comm.rank;
  const long long base = rows / size, rem = rows % size;
  const long long r0 = rank * base + std::min<long long>(rank, rem), nloc = base + (rank < rem ? 1 : 0);
  std::vector<int> rp(nloc + 1), ci((size_t)(start[r0 + nloc] - start[r0]));
  std::vector<double> va(ci.size());
  for (long long i = 0; i <= nloc; i++) rp[i] = (int)(start[r0 + i] - start[r0]);
  for (size_t e = 0; e < ci.size(); e++) { ci[e] = (int32_t)be32(pc + 4 * (start[r0] + e)); va[e] = be64f(pv + 8 * (start[r0] + e)); }
  return ks_mat_create_csr_flags(ctx, (int)nloc, (int)r0, (int)rows, rp.data(), ci.data(), va.data(), KS_MAT_KEEP_CSR, out);
}

// MatCreateShell + MatShellSetOperation(MATOP_MULT) (the matrix-free route of src/eps/tutorials/ex3.c)
extern "C" int ks_mat_create_shell(ks_ctx ctx, int n_local, int row_start, int n_global, ks_shell_mult_fn mult, void *user, ks_mat *out)
{
  KS_CHECK(ctx && out && mult, KS_ERR_ARG_NULL, "NULL argument");
  KS_CHECK(n_local >= 0 && n_global >= n_local && row_start >= 0, KS_ERR_ARG_OUTOFRANGE, "bad sizes n_local=%d n_global=%d row_start=%d", n_local, n_global, row_start);
  ks_mat A = new ks_mat_s(); A->ctx = ctx; A->n = n_local; A->row_start = row_start; A->n_global = n_global;
  A->shell_mult = mult; A->shell_user = user;
  *out = A;
  return KS_SUCCESS;
}
