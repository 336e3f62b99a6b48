// CSR rows against a dense transposed table T[n][kp], shared by the sparse KMeans search
// (csr_kmeans.hip) and the sparse silhouette (csr_silhouette.hip).
//
// CSR layout as in csr_knn.hip: int64 row offsets, int32 column indices, ABSOLUTE offsets (a row
// block is a pointer into the row offsets of the whole matrix). Column indices are in [0, n),
// validated by the caller before any launch; the kernels do not check again.
//
// The table scheme: one wave per row, CSR_ROWS waves per block, kp a multiple of 64. A non-zero
// (col, val) of the row is wave-uniform; lane l accumulates table columns tile + l + 64 s,
// s < CSR_KS, so one non-zero costs CSR_KS reads of 64 consecutive values of T row `col` and CSR_KS
// fused multiply-adds per lane: one accumulator chain per (lane, s), products added in column
// order, no cross-lane sum and no atomics (csr_accumulate). kp > CSR_TK loops over tiles; the row's
// first CSR_STAGE (col, val) pairs are staged once in LDS and re-used by every tile, a longer row
// re-reads its tail from global memory. The stage and the per-tile loop are written out in the two
// kernels (csr_nearest_kernel, csr_sil_wide_kernel): wrapped in a shared function they compile to
// different code on gfx950, and the kernels must stay instruction for instruction what they were.
//
// The label sums: sums[label][col] += f value over the non-zeros, G lanes per row, fp64 atomics or
// exact i64 fixed-point atomics.
#pragma once
#include "common.h"

namespace {
constexpr int CSR_ROWS = 4;             // rows (waves) per block
constexpr int CSR_T = 64 * CSR_ROWS;    // threads per block
constexpr int CSR_KS = 4;               // accumulators per lane
constexpr int CSR_TK = 64 * CSR_KS;     // table columns per pass
constexpr int CSR_STAGE = 512;          // non-zeros of a row staged in LDS

template <typename T>
__device__ __forceinline__ T csr_fma(T a, T b, T c);
template <>
__device__ __forceinline__ float csr_fma<float>(float a, float b, float c) { return fmaf(a, b, c); }
template <>
__device__ __forceinline__ double csr_fma<double>(double a, double b, double c) { return fma(a, b, c); }

__device__ __forceinline__ float csr_shfl_xor(float v, int o) { return __shfl_xor(v, o, 64); }
__device__ __forceinline__ double csr_shfl_xor(double v, int o) { return __shfl_xor(v, o, 64); }

// blocks of a one-wave-per-row launch over m rows, -1 where the grid cannot hold them
static inline long csr_row_blocks(long m) {
  const long blocks = (m + CSR_ROWS - 1) / CSR_ROWS;
  return blocks > srml_max_blocks(CSR_T) ? -1 : blocks;
}

template <typename T>
__device__ __forceinline__ void csr_accumulate(const T* __restrict__ ct, T v, int tile, int kp, T (&acc)[CSR_KS]) {
#pragma unroll
  for (int s = 0; s < CSR_KS; ++s)
    if (tile + 64 * s < kp) acc[s] = csr_fma<T>(v, ct[64 * s], acc[s]);  // wave-uniform condition
}

// A group of G lanes owns one row and strides its non-zeros: sums[label][col] += f value, f the
// per-row factor (null: 1; a row with f = 0 is skipped). FIXED: the value is scaled by the power of
// two `scale`, rounded to an integer and added with 64-bit integer atomics, exact in any order
// (wrap-around two's complement: the caller's scale keeps every true sum inside i64).
template <typename T, int G, bool FIXED>
__global__ __launch_bounds__(256) void csr_label_sums_kernel(const long* __restrict__ indptr,
                                                             const int* __restrict__ indices,
                                                             const T* __restrict__ data, long m, int n,
                                                             const int* __restrict__ labels, int k,
                                                             const double* __restrict__ f, double scale,
                                                             double* __restrict__ sums) {
  constexpr int GPB = 256 / G;
  const int g = threadIdx.x / G, l = threadIdx.x % G;
  for (long r = (long)blockIdx.x * GPB + g; r < m; r += (long)gridDim.x * GPB) {
    const int lab = labels[r];
    if ((unsigned)lab >= (unsigned)k) continue;  // never outside the buffer
    const double fi = f ? f[r] : 1.0;
    if (fi == 0.0) continue;
    double* row = sums + (long)lab * n;
    const long p1 = indptr[r + 1];
    for (long p = indptr[r] + l; p < p1; p += G) {
      const double v = f ? fi * (double)data[p] : (double)data[p];
      if constexpr (FIXED)
        atomicAdd(reinterpret_cast<unsigned long long*>(row + indices[p]), (unsigned long long)__double2ll_rn(v * scale));
      else
        atomicAdd(row + indices[p], v);
    }
  }
}

template <typename T, int G>
int csr_label_sums_g(const long* indptr, const int* indices, const T* data, long m, int n, const int* labels, int k,
                     const double* f, double scale, double* sums, hipStream_t stream) {
  constexpr int GPB = 256 / G;
  long blocks = (m + GPB - 1) / GPB;
  if (blocks > 256L * 64) blocks = 256L * 64;  // grid-stride beyond 64 blocks per CU
  if (scale != 0.0)
    hipLaunchKernelGGL((csr_label_sums_kernel<T, G, true>), dim3((unsigned)blocks), dim3(256), 0, stream, indptr,
                       indices, data, m, n, labels, k, f, scale, sums);
  else
    hipLaunchKernelGGL((csr_label_sums_kernel<T, G, false>), dim3((unsigned)blocks), dim3(256), 0, stream, indptr,
                       indices, data, m, n, labels, k, f, scale, sums);
  return srml_status();
}

// sums (k x n, zeroed by the caller) += f_r x_r grouped by label; the mean nnz picks the lanes per
// row. scale = 0: fp64 atomics. scale = 2^s: sums holds i64 integers of rint(f value 2^s)
// afterwards (srml_csr_cluster_sums_finish converts). -2: k or n not positive.
template <typename T>
int csr_label_sums(const long* indptr, const int* indices, const T* data, long m, int n, long nnz, const int* labels,
                   int k, const double* f, double scale, double* sums, hipStream_t stream) {
  if (m <= 0) return 0;
  if (k <= 0 || n <= 0) return -2;
  const long mean = nnz / m;
  if (mean <= 12) return csr_label_sums_g<T, 8>(indptr, indices, data, m, n, labels, k, f, scale, sums, stream);
  if (mean <= 24) return csr_label_sums_g<T, 16>(indptr, indices, data, m, n, labels, k, f, scale, sums, stream);
  if (mean <= 48) return csr_label_sums_g<T, 32>(indptr, indices, data, m, n, labels, k, f, scale, sums, stream);
  return csr_label_sums_g<T, 64>(indptr, indices, data, m, n, labels, k, f, scale, sums, stream);
}
}  // namespace
