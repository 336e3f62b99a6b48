// KMeans on CSR rows (sparse vector columns) against DENSE centres:
//
//  * srml_csr_nearest_{f32,f64}      — label (i32) and squared distance of every CSR row to its
//    nearest centre, expanded form key_j = |x|^2 + |c_j|^2 - 2 x.c_j clamped at 0, the lowest centre
//    index winning bit-equal keys;
//  * srml_csr_centres_transpose_{f32,f64} — the transposed, 64-padded centre table the search reads;
//  * srml_csr_cluster_sums_{f32,f64} — sums[label][col] += value over the non-zeros (fp64), either
//    fp64 atomics or, for bit-reproducible results, exact i64 fixed-point integer atomics that
//    srml_csr_cluster_sums_finish converts to fp64 in place.
//
// CSR layout as in csr_knn.hip: int64 row offsets, int32 column indices, ABSOLUTE offsets (a row
// block is a pointer into the row offsets of the whole matrix). Column indices are in [0, n),
// validated by the caller before any launch; the kernels do not check again.
//
// srml_csr_nearest: one wave per row, KM_ROWS waves per block. The centres come TRANSPOSED and
// padded, CT[n][kp] with kp a multiple of 64 (padding columns zero, their |c|^2 = +inf). A non-zero
// (col, val) of the row is wave-uniform; lane l accumulates centres tile + l + 64 s, s < KM_KS, so
// one non-zero costs KM_KS reads of 64 consecutive values of CT row `col` (256 B each in fp32) and
// KM_KS fused multiply-adds per lane: one accumulator chain per (lane, s), products added in column
// order, no cross-lane sum and no atomics. k > KM_TK = 64 KM_KS loops over centre tiles; the row's
// first KM_STAGE (col, val) pairs are staged once in LDS and re-used by every tile, a longer row
// re-reads its tail from global memory. |x|^2 is summed in fp64 from the same values (lane-strided
// partials, DPP reduction) and rounded once. Per tile each lane folds its KM_KS keys into a running
// (min, arg-min) in ascending index order with a strict compare; a 6-step butterfly on (key, index)
// picks the wave's minimum, the lower index on equal keys.
#include "common.h"

namespace {
constexpr int KM_ROWS = 4;             // rows (waves) per block
constexpr int KM_T = 64 * KM_ROWS;     // threads per block
constexpr int KM_KS = 4;               // accumulators per lane
constexpr int KM_TK = 64 * KM_KS;      // centres per pass
constexpr int KM_STAGE = 512;          // non-zeros of a row staged in LDS

template <typename T>
__device__ __forceinline__ T km_fma(T a, T b, T c);
template <>
__device__ __forceinline__ float km_fma<float>(float a, float b, float c) { return fmaf(a, b, c); }
template <>
__device__ __forceinline__ double km_fma<double>(double a, double b, double c) { return fma(a, b, c); }

__device__ __forceinline__ float km_shfl_xor(float v, int o) { return __shfl_xor(v, o, 64); }
__device__ __forceinline__ double km_shfl_xor(double v, int o) { return __shfl_xor(v, o, 64); }

template <typename T>
__device__ __forceinline__ void km_accumulate(const T* __restrict__ ct, T v, int tile, int kp, T (&acc)[KM_KS]) {
#pragma unroll
  for (int s = 0; s < KM_KS; ++s)
    if (tile + 64 * s < kp) acc[s] = km_fma<T>(v, ct[64 * s], acc[s]);  // wave-uniform condition
}

template <typename T>
__global__ __launch_bounds__(KM_T) void csr_nearest_kernel(const long* __restrict__ indptr,
                                                           const int* __restrict__ indices,
                                                           const T* __restrict__ data, long m,
                                                           const T* __restrict__ CT, const T* __restrict__ cnorm,
                                                           int k, int kp, int* __restrict__ labels,
                                                           T* __restrict__ dist) {
  __shared__ int sI[KM_ROWS][KM_STAGE];
  __shared__ T sV[KM_ROWS][KM_STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long r = (long)blockIdx.x * KM_ROWS + wave;
  long p0 = 0, nnz = 0;
  if (r < m) {
    p0 = indptr[r];
    nnz = indptr[r + 1] - p0;
  }
  const int ns = nnz < KM_STAGE ? (int)nnz : KM_STAGE;
  double sq = 0.0;
  for (long p = lane; p < nnz; p += 64) {
    const T v = data[p0 + p];
    sq = fma((double)v, (double)v, sq);
    if (p < KM_STAGE) {
      sI[wave][p] = indices[p0 + p];
      sV[wave][p] = v;
    }
  }
  const T xn = (T)wave_sum(sq);
  __syncthreads();  // every wave reaches this: rows past m have nnz = 0
  if (r >= m) return;
  T best = (T)__builtin_inff();
  int bi = 0x7fffffff;
  for (int tile = 0; tile < kp; tile += KM_TK) {
    T acc[KM_KS];
#pragma unroll
    for (int s = 0; s < KM_KS; ++s) acc[s] = (T)0;
    const T* ct = CT + tile + lane;
#pragma unroll 4
    for (int p = 0; p < ns; ++p) km_accumulate<T>(ct + (long)sI[wave][p] * kp, sV[wave][p], tile, kp, acc);
    for (long p = KM_STAGE; p < nnz; ++p) km_accumulate<T>(ct + (long)indices[p0 + p] * kp, data[p0 + p], tile, kp, acc);
#pragma unroll
    for (int s = 0; s < KM_KS; ++s) {
      const int j = tile + 64 * s + lane;
      if (j < k) {  // j < k <= kp: the padding never competes
        const T key = km_fma<T>((T)-2, acc[s], xn + cnorm[j]);
        const T d = key > (T)0 ? key : (T)0;
        if (d < best) {  // ascending j per lane: strict keeps the lower index
          best = d;
          bi = j;
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T ob = km_shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob < best || (ob == best && oi < bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (lane == 0) {
    labels[r] = bi;
    dist[r] = best;
  }
}

// A group of G lanes owns one row and strides its non-zeros. FIXED: the value is scaled by the
// power of two `scale`, rounded to an integer and added with 64-bit integer atomics (wrap-around
// two's complement: the caller's scale keeps every true sum inside i64).
template <typename T, int G, bool FIXED>
__global__ __launch_bounds__(256) void csr_cluster_sums_kernel(const long* __restrict__ indptr,
                                                               const int* __restrict__ indices,
                                                               const T* __restrict__ data, long m, int n,
                                                               const int* __restrict__ labels, int k, double scale,
                                                               double* __restrict__ sums) {
  constexpr int GPB = 256 / G;
  const int g = threadIdx.x / G, l = threadIdx.x % G;
  for (long r = (long)blockIdx.x * GPB + g; r < m; r += (long)gridDim.x * GPB) {
    const int lab = labels[r];
    if ((unsigned)lab >= (unsigned)k) continue;  // never outside the buffer
    double* row = sums + (long)lab * n;
    const long p1 = indptr[r + 1];
    for (long p = indptr[r] + l; p < p1; p += G) {
      const double v = (double)data[p];
      if constexpr (FIXED)
        atomicAdd(reinterpret_cast<unsigned long long*>(row + indices[p]), (unsigned long long)__double2ll_rn(v * scale));
      else
        atomicAdd(row + indices[p], v);
    }
  }
}

__global__ __launch_bounds__(256) void csr_cluster_sums_finish_kernel(double* __restrict__ buf, long count,
                                                                      double inv_scale) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256)
    buf[i] = (double)reinterpret_cast<const long long*>(buf)[i] * inv_scale;  // one rounding, exact scaling
}

// CT[d][j] = C[j][d] for j < k, 0 for k <= j < kp: 64 x 64 tiles through LDS, reads coalesced
// along the columns of C, writes along the (padded) centres of CT. Every cell of CT is written,
// so the table can live in a buffer kept across the iterations of a fit.
template <typename T>
__global__ __launch_bounds__(256) void csr_centres_transpose_kernel(const T* __restrict__ C, int k, int n, int kp,
                                                                    T* __restrict__ CT) {
  __shared__ T tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long d0 = (long)blockIdx.x * 64;
  const int j0 = blockIdx.y * 64;
  for (int r = ty; r < 64; r += 4) {
    const int j = j0 + r;
    const long d = d0 + tx;
    tile[r][tx] = (j < k && d < n) ? C[(long)j * n + d] : (T)0;
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const long d = d0 + r;
    if (d < n) CT[d * kp + j0 + tx] = tile[tx][r];  // j0 + tx < kp: kp is a multiple of 64
  }
}

template <typename T>
int km_transpose(const T* C, int k, int n, int kp, T* CT, hipStream_t stream) {
  if (n <= 0) return 0;
  if (k <= 0 || kp < k || kp % 64 != 0) return -2;
  const long bx = ((long)n + 63) / 64;
  if (kp / 64 > 65535 || bx * (kp / 64) > srml_max_blocks(256)) return -1;
  hipLaunchKernelGGL((csr_centres_transpose_kernel<T>), dim3((unsigned)bx, (unsigned)(kp / 64)), dim3(256), 0, stream, C,
                     k, n, kp, CT);
  return srml_status();
}

template <typename T>
int km_nearest(const long* indptr, const int* indices, const T* data, long m, const T* CT, const T* cnorm, int k,
               int kp, int* labels, T* dist, hipStream_t stream) {
  if (m <= 0) return 0;
  if (k <= 0 || kp < k || kp % 64 != 0) return -2;
  const long blocks = (m + KM_ROWS - 1) / KM_ROWS;
  if (blocks > srml_max_blocks(KM_T)) return -1;
  hipLaunchKernelGGL((csr_nearest_kernel<T>), dim3((unsigned)blocks), dim3(KM_T), 0, stream, indptr, indices, data, m,
                     CT, cnorm, k, kp, labels, dist);
  return srml_status();
}

template <typename T, int G>
int km_sums_g(const long* indptr, const int* indices, const T* data, long m, int n, const int* labels, int k,
              double scale, double* sums, hipStream_t stream) {
  constexpr int GPB = 256 / G;
  long blocks = (m + GPB - 1) / GPB;
  if (blocks > 256L * 64) blocks = 256L * 64;  // grid-stride beyond 64 blocks per CU
  if (scale != 0.0)
    hipLaunchKernelGGL((csr_cluster_sums_kernel<T, G, true>), dim3((unsigned)blocks), dim3(256), 0, stream, indptr,
                       indices, data, m, n, labels, k, scale, sums);
  else
    hipLaunchKernelGGL((csr_cluster_sums_kernel<T, G, false>), dim3((unsigned)blocks), dim3(256), 0, stream, indptr,
                       indices, data, m, n, labels, k, scale, sums);
  return srml_status();
}

template <typename T>
int km_sums(const long* indptr, const int* indices, const T* data, long m, int n, long nnz, const int* labels, int k,
            double scale, double* sums, hipStream_t stream) {
  if (m <= 0) return 0;
  if (k <= 0 || n <= 0) return -2;
  const long mean = nnz / m;
  if (mean <= 12) return km_sums_g<T, 8>(indptr, indices, data, m, n, labels, k, scale, sums, stream);
  if (mean <= 24) return km_sums_g<T, 16>(indptr, indices, data, m, n, labels, k, scale, sums, stream);
  if (mean <= 48) return km_sums_g<T, 32>(indptr, indices, data, m, n, labels, k, scale, sums, stream);
  return km_sums_g<T, 64>(indptr, indices, data, m, n, labels, k, scale, sums, stream);
}
}  // namespace

// The dispatch constants of this file, for the Python layer's checks: 0 centres per pass, 1 staged
// non-zeros per row, 2 rows per block.
SRML_API int srml_csr_kmeans_config(int which) {
  switch (which) {
    case 0: return KM_TK;
    case 1: return KM_STAGE;
    case 2: return KM_ROWS;
    default: return -1;
  }
}

// labels[r], dist[r] for the m rows whose offsets start at indptr (m + 1 absolute offsets). CT is
// n x kp, cnorm kp values (+inf past k). -1: the grid overflows, -2: k, kp inconsistent.
SRML_API int srml_csr_nearest_f32(const long* indptr, const int* indices, const float* data, long m, const float* CT,
                                  const float* cnorm, int k, int kp, int* labels, float* dist, hipStream_t stream) {
  return km_nearest<float>(indptr, indices, data, m, CT, cnorm, k, kp, labels, dist, stream);
}

SRML_API int srml_csr_nearest_f64(const long* indptr, const int* indices, const double* data, long m, const double* CT,
                                  const double* cnorm, int k, int kp, int* labels, double* dist, hipStream_t stream) {
  return km_nearest<double>(indptr, indices, data, m, CT, cnorm, k, kp, labels, dist, stream);
}

// CT (n x kp) = the transposed centres C (k x n), zero in the padding columns k .. kp. -1: the grid
// overflows, -2: k, kp inconsistent.
SRML_API int srml_csr_centres_transpose_f32(const float* C, int k, int n, int kp, float* CT, hipStream_t stream) {
  return km_transpose<float>(C, k, n, kp, CT, stream);
}

SRML_API int srml_csr_centres_transpose_f64(const double* C, int k, int n, int kp, double* CT, hipStream_t stream) {
  return km_transpose<double>(C, k, n, kp, CT, stream);
}

// sums (k x n, zeroed by the caller) += the rows grouped by label; nnz picks the lanes per row.
// scale = 0: fp64 atomics. scale = 2^s: sums holds i64 integers of rint(value * 2^s) afterwards
// (srml_csr_cluster_sums_finish converts). Rows with a label outside [0, k) are skipped.
SRML_API int srml_csr_cluster_sums_f32(const long* indptr, const int* indices, const float* data, long m, int n,
                                       long nnz, const int* labels, int k, double scale, double* sums,
                                       hipStream_t stream) {
  return km_sums<float>(indptr, indices, data, m, n, nnz, labels, k, scale, sums, stream);
}

SRML_API int srml_csr_cluster_sums_f64(const long* indptr, const int* indices, const double* data, long m, int n,
                                       long nnz, const int* labels, int k, double scale, double* sums,
                                       hipStream_t stream) {
  return km_sums<double>(indptr, indices, data, m, n, nnz, labels, k, scale, sums, stream);
}

// buf[i] = (double)(i64 at buf[i]) * inv_scale, in place, i < count
SRML_API int srml_csr_cluster_sums_finish(double* buf, long count, double inv_scale, hipStream_t stream) {
  if (count <= 0) return 0;
  long blocks = (count + 255) / 256;
  if (blocks > 256L * 64) blocks = 256L * 64;
  hipLaunchKernelGGL(csr_cluster_sums_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, buf, count,
                     inv_scale);
  return srml_status();
}
