// Micro-benchmark: where the one-row walk of the dictionary product (k_spmv_dict, row-pattern form) spends its time on the 216^3 7-point Laplacian -
// the gathers of x or the store of y. The walk of ks_spmv.hip / ks_rows.cuh is repeated here on a matrix built on the host (one byte per row, 27 code
// words, two values, seven offsets; the same XCD-contiguous walk over groups of 256 rows and the same grid) and timed in four forms:
//   (a) as it is;
//   (b) the store made conditional on a value that never occurs: the loads stay, the 80 MB write stream goes;
//   (c) only the centre gather (the other entries multiply a constant): the write stream stays, six of seven gathers go;
//   (d) seven gathers, but each the aligned 16-byte pair that holds the entry (both halves used, the result is not the product): the request width alone.
// Prints us per product for each. Build: hipcc -O3 --offload-arch=gfx950 dict_gather_split.hip -o dict_gather_split
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

constexpr int BLOCK = 256, W = 8;
typedef double d2v __attribute__((ext_vector_type(2)));

template <int MODE>
__global__ __launch_bounds__(BLOCK) void k_walk(int nrows, const unsigned char *__restrict__ rowpat, const uint4 *__restrict__ pats, int npat, const double *__restrict__ dval, int nval,
                                                const int *__restrict__ doff, int noff, const double *__restrict__ x, double *__restrict__ y)
{
  __shared__ double sv[256];
  __shared__ int so[256];
  __shared__ uint4 sp[256];
  for (int i = threadIdx.x; i < nval; i += BLOCK) sv[i] = dval[i];
  for (int i = threadIdx.x; i < noff; i += BLOCK) so[i] = doff[i];
  for (int i = threadIdx.x; i < npat; i += BLOCK) sp[i] = pats[i];
  __syncthreads();
  const long long groups = ((long long)nrows + BLOCK - 1) / BLOCK, gper = (groups + 7) / 8;
  const long long g0 = (blockIdx.x % 8) * gper, g1 = g0 + gper < groups ? g0 + gper : groups;
  for (long long g = g0 + blockIdx.x / 8; g < g1; g += gridDim.x / 8) {
    const long long r = g * BLOCK + threadIdx.x;
    if (r >= nrows) break;
    const uint4 c = sp[rowpat[r]];
    const unsigned wds[4] = {c.x, c.y, c.z, c.w};
    double a[W], xv[W];
#pragma unroll
    for (int e = 0; e < W; e++) {
      const unsigned code = (wds[e >> 1] >> ((e & 1) * 16)) & 0xffffu, oc = code & 0xffu, vc = code >> 8;
      const bool ok = vc != 255u;
      a[e] = ok ? sv[vc] : 0.0;
      if (MODE == 2) xv[e] = ok ? (so[oc] == 0 ? x[r] : 1.0) : 0.0;
      else if (MODE == 3) {
        d2v t = {0.0, 0.0};
        if (ok) t = *reinterpret_cast<const d2v *>(x + ((r + so[oc]) & ~1LL));
        xv[e] = t.x + t.y;
      } else xv[e] = ok ? x[r + so[oc]] : 0.0;
    }
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < W; e++) acc = fma(a[e], xv[e], acc);
    if (MODE == 1) { if (acc == 1.2345e300) __builtin_nontemporal_store(acc, y + r); }
    else __builtin_nontemporal_store(acc, y + r);
  }
}

int main()
{
  const int N = 216; const long long n = (long long)N * N * N;
  const int offs[7] = {-N * N, -N, -1, 0, 1, N, N * N};
  const double vals[2] = {-1.0, 6.0};
  // a row's word: its entries in ascending columns, padding (value code 255) behind them; the 27 distinct words by the boundary flags of the row
  std::vector<unsigned char> rowpat(((size_t)n + 255) / 256 * 256, 0);
  std::vector<std::vector<unsigned short>> table;
  for (int k = 0; k < N; k++) for (int j = 0; j < N; j++) for (int i = 0; i < N; i++) {
    const bool have[7] = {k > 0, j > 0, i > 0, true, i < N - 1, j < N - 1, k < N - 1};
    std::vector<unsigned short> w;
    for (int e = 0; e < 7; e++) if (have[e]) w.push_back((unsigned short)(e | (e == 3 ? 1 : 0) << 8));
    while ((int)w.size() < W) w.push_back((unsigned short)(255u << 8));
    size_t p = std::find(table.begin(), table.end(), w) - table.begin();
    if (p == table.size()) table.push_back(w);
    rowpat[i + (size_t)N * (j + (size_t)N * k)] = (unsigned char)p;
  }
  std::vector<unsigned short> flat;
  for (auto &w : table) flat.insert(flat.end(), w.begin(), w.end());
  const int npat = (int)table.size();
  unsigned char *d_rp; uint4 *d_pats; double *d_val, *d_x, *d_y; int *d_off;
  CK(hipMalloc(&d_rp, rowpat.size())); CK(hipMalloc(&d_pats, flat.size() * 2)); CK(hipMalloc(&d_val, sizeof(vals))); CK(hipMalloc(&d_off, sizeof(offs)));
  CK(hipMalloc(&d_x, n * 8)); CK(hipMalloc(&d_y, n * 8));
  CK(hipMemcpy(d_rp, rowpat.data(), rowpat.size(), hipMemcpyHostToDevice)); CK(hipMemcpy(d_pats, flat.data(), flat.size() * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_val, vals, sizeof(vals), hipMemcpyHostToDevice)); CK(hipMemcpy(d_off, offs, sizeof(offs), hipMemcpyHostToDevice));
  std::vector<double> hx(n);
  for (long long i = 0; i < n; i++) hx[i] = 1.0 + (double)(i % 1009) / 1009.0;
  CK(hipMemcpy(d_x, hx.data(), n * 8, hipMemcpyHostToDevice)); CK(hipMemset(d_y, 0, n * 8));
  hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
  const long long groups = (n + BLOCK - 1) / BLOCK;
  long long nblk = std::min<long long>(groups, (long long)prop.multiProcessorCount * 64);
  nblk = std::min<long long>((nblk + 7) / 8, (groups + 7) / 8) * 8;                 // the grid of ksr::dict_launch_grid
  printf("216^3 Laplacian, row-pattern form: n %lld, %d patterns, grid %lld x %d\n", n, npat, nblk, BLOCK);
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const char *names[4] = {"(a) as it is", "(b) no store (loads stay)", "(c) centre gather only", "(d) seven 16-byte gathers"};
  for (int round = 0; round < 2; round++)
    for (int mode = 0; mode < 4; mode++) {
#define RUN(M) hipLaunchKernelGGL((k_walk<M>), dim3((unsigned)nblk), dim3(BLOCK), 0, 0, (int)n, d_rp, d_pats, npat, d_val, 2, d_off, 7, d_x, d_y)
#define RUN_MODE() do { if (mode == 0) RUN(0); else if (mode == 1) RUN(1); else if (mode == 2) RUN(2); else RUN(3); } while (0)
      for (int w = 0; w < 5; w++) RUN_MODE();
      CK(hipEventRecord(e0));
      for (int r = 0; r < 50; r++) RUN_MODE();
      CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      printf("round %d %-28s %7.1f us per product\n", round, names[mode], ms * 1000.0 / 50);
    }
  return 0;
}
