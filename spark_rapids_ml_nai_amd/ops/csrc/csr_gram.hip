// Gram matrix and X^T y of CSR rows (sparse vector columns), the first pass of the Gram-based fits
// (LinearRegression, PCA; models/stats.py):
//
//  * srml_csr_gram_{f32,f64} — out (n x n fp64, UPPER triangle) += X^T X; the caller completes the
//    matrix with srml_mirror_upper_f64;
//  * srml_csr_gram_finish    — deterministic mode: out += (i64 buffer) * 2^-s, upper triangle;
//  * srml_csr_xty_{f32,f64}  — out (n fp64) += X^T y for y in fp32 or fp64.
//
// CSR layout as in csr_knn.hip / csr_kmeans.hip: int64 row offsets, int32 column indices, ABSOLUTE
// offsets (a row block is a pointer into the row offsets of the whole matrix). Column indices are
// in [0, n) and ASCENDING within a row, validated by the caller before any launch.
//
// Why no matrix instructions. Densifying row tiles in LDS and running MFMA costs m n^2
// multiply-adds whatever the density; the products that are not zero number sum_r nnz_r^2, which
// is 10^4 times fewer at 1 % density. The kernel below does only those. This was an argument from
// the operation count alone: nobody had measured either side when the design was fixed, and a
// kernel that densifies CSR tiles in LDS for MFMA has still not been written or measured. What has
// been measured since (docs/performance.md, 1M x 3000): the dense SYRK on rows already resident
// and dense on the device is faster than this kernel from about 1 % density; it is the host
// densification and the copy that make the dense route slower for a sparse column.
//
// Window table. The columns are cut into W = ceil(n / T) windows of T. csr_gram_windows_kernel
// writes, for every row r and w = 0 .. W, the offset within the row of its first index >= w T
// (a lower bound by bisection; int32; entry W is the row's length). The table is stored
// window-major, win[w * rows + r], so that 64 lanes reading one window of 64 consecutive rows
// read 256 contiguous bytes.
//
// Tile kernel. One 256-thread workgroup owns one output tile (I, J), I <= J, for one slab of rows:
// the grid is (tile pairs) x (slabs), the slab count chosen so that the grid holds GR_TARGET_WG
// workgroups (a few per CU), by the same arithmetic when there is a single tile pair. The T x T
// accumulators of the workgroup live in LDS as fp64, leading dimension T + 1. A product of two
// fp32 values is exact in fp64, so a cell carries only the roundings of its fp64 additions; the
// scatter is later formed as G - m mu mu^T (sparse rows cannot be centred first), which is why
// the sum is not taken in fp32.
//
// The four waves take the slab's rows round-robin in groups of GR_R = 64: lane l reads the four
// table entries that bound row l's segments in windows I and J (coalesced, see above) and the
// row's offset. A ballot keeps the rows whose two segments are both non-empty: this is where
// sparsity pays, a row without a non-zero in either window costs 16 bytes of table and nothing
// else. For a kept row each lane holds one element of the J segment (chunks of GR_C = 64 for
// longer segments) and one of the I segment; the I elements are broadcast one at a time with
// v_readlane, and every lane adds x_a x_b into acc[a - I T][b - J T] with an LDS fp64 atomic
// add: one instruction touches up to 64 distinct cells of one accumulator row, the atomic only
// resolves collisions between waves. A diagonal tile computes both halves and flushes the upper
// one. After the slab each thread adds its non-zero cells into `out` with fp64 global atomics, so
// a cell that no row touches with both columns stays exactly 0.0.
//
// Deterministic mode (scale = 2^s != 0): the same template with u64 accumulators. Each product is
// rounded to the grid 2^-s (rint(x_a x_b 2^s)); the adds in LDS and in the n x n i64 buffer are
// integer adds, exact in any order, so the result repeats bit for bit. The caller sizes s from
// m max|x|^2 so that no sum leaves i64, and converts once with srml_csr_gram_finish.
#include "common.h"

namespace {
constexpr int GR_THREADS = 256;
constexpr int GR_WAVES = GR_THREADS / 64;
constexpr int GR_R = 64;            // rows a wave takes at once = the slab unit
constexpr int GR_C = 64;            // elements of a segment held by the wave at once
constexpr int GR_T_DEFAULT = 64;    // tile width of srml_csr_gram_* when the caller passes 0
constexpr long GR_TARGET_WG = 2048; // workgroups of one launch: 8 per CU on 256 CUs

__device__ __forceinline__ int gr_bcast(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float gr_bcast(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ long gr_bcast(long v, int l) {
  const int lo = __builtin_amdgcn_readlane((int)(v & 0xffffffffL), l);
  const int hi = __builtin_amdgcn_readlane((int)(v >> 32), l);
  return ((long)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ double gr_bcast(double v, int l) {
  return __longlong_as_double(gr_bcast((long)__double_as_longlong(v), l));
}

// win[w * rows + r] = offset within row r of its first index >= w T, w = 0 .. W (W included)
__global__ __launch_bounds__(256) void csr_gram_windows_kernel(const long* __restrict__ indptr,
                                                               const int* __restrict__ indices, long rows, int W, int T,
                                                               int* __restrict__ win) {
  const long total = rows * (long)(W + 1);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i % rows;
    const long key = (i / rows) * (long)T;
    const long p0 = indptr[r];
    long lo = 0, hi = indptr[r + 1] - p0;
    while (lo < hi) {  // lower bound of key in the ascending indices of the row
      const long mid = (lo + hi) >> 1;
      if ((long)indices[p0 + mid] < key) lo = mid + 1;
      else hi = mid;
    }
    win[i] = (int)lo;
  }
}

template <bool FIXED>
struct GrAcc {
  using type = double;
};
template <>
struct GrAcc<true> {
  using type = unsigned long long;
};

template <typename V, int T, bool FIXED>
__global__ __launch_bounds__(GR_THREADS) void csr_gram_tile_kernel(const long* __restrict__ indptr,
                                                                    const int* __restrict__ indices,
                                                                    const V* __restrict__ data, long rows, int n, int W,
                                                                    const int* __restrict__ win, long slab_rows,
                                                                    double scale, double* __restrict__ out) {
  using A = typename GrAcc<FIXED>::type;
  constexpr int LD = T + 1;  // odd in 8-byte units: the rows of the tile start in different banks
  __shared__ A acc[T * LD];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // tile pair blockIdx.x -> (I, J), I <= J, row-major over the upper triangle of W x W
  int I = 0, rem = (int)blockIdx.x;
  while (rem >= W - I) {
    rem -= W - I;
    ++I;
  }
  const int J = I + rem;
  for (int c = threadIdx.x; c < T * LD; c += GR_THREADS) acc[c] = (A)0;
  __syncthreads();
  const long s0 = (long)blockIdx.y * slab_rows;
  const long s1 = s0 + slab_rows < rows ? s0 + slab_rows : rows;
  const int* wI = win + (long)I * rows;
  const int* wJ = win + (long)J * rows;
  for (long g = s0 + (long)wave * GR_R; g < s1; g += (long)GR_WAVES * GR_R) {
    const long r = g + lane;
    int a0 = 0, a1 = 0, b0 = 0, b1 = 0;
    long p0 = 0;
    if (r < s1) {
      a0 = wI[r];
      a1 = wI[rows + r];
      b0 = wJ[r];
      b1 = wJ[rows + r];
      p0 = indptr[r];
    }
    unsigned long long keep = __ballot(a1 > a0 && b1 > b0);
    while (keep) {
      const int l = __ffsll((long long)keep) - 1;  // wave-uniform
      keep &= keep - 1;
      const long base = gr_bcast(p0, l);
      const int ra0 = gr_bcast(a0, l), na = gr_bcast(a1, l) - ra0;
      const int rb0 = gr_bcast(b0, l), nb = gr_bcast(b1, l) - rb0;
      for (int cb = 0; cb < nb; cb += GR_C) {
        int jb = -1;  // column within tile J held by this lane, -1: none
        V xb = (V)0;
        if (cb + lane < nb) {
          const long p = base + rb0 + cb + lane;
          jb = indices[p] - J * T;
          xb = data[p];
        }
        const bool lane_ok = (unsigned)jb < (unsigned)T;
        for (int ca = 0; ca < na; ca += GR_C) {
          int ia = -1;
          V xa = (V)0;
          if (ca + lane < na) {
            const long p = base + ra0 + ca + lane;
            ia = indices[p] - I * T;
            xa = data[p];
          }
          const int cnt = na - ca < GR_C ? na - ca : GR_C;
          for (int i = 0; i < cnt; ++i) {
            const int ri = gr_bcast(ia, i);
            const double prod = (double)gr_bcast(xa, i) * (double)xb;
            if (lane_ok && (unsigned)ri < (unsigned)T) {  // always true for ascending, in-range indices
              if constexpr (FIXED) atomicAdd(&acc[ri * LD + jb], (unsigned long long)__double2ll_rn(prod * scale));
              else atomicAdd(&acc[ri * LD + jb], prod);
            }
          }
        }
      }
    }
  }
  __syncthreads();
  A* o = reinterpret_cast<A*>(out);
  for (int c = threadIdx.x; c < T * T; c += GR_THREADS) {
    const int i = c / T, j = c % T;
    const long gi = (long)I * T + i, gj = (long)J * T + j;
    const A v = acc[i * LD + j];
    if (gi < n && gj < n && gj >= gi && v != (A)0) atomicAdd(o + gi * n + gj, v);
  }
}

__global__ __launch_bounds__(256) void csr_gram_finish_kernel(const long long* __restrict__ buf, int n,
                                                              double inv_scale, double* __restrict__ out) {
  const long count = (long)n * n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256)
    if (i % n >= i / n && buf[i] != 0) out[i] += (double)buf[i] * inv_scale;  // one rounding, exact scaling
}

// One wave per row: lanes stride the row's non-zeros, out[col] += x * y[r] in fp64.
template <typename V, typename Y>
__global__ __launch_bounds__(256) void csr_xty_kernel(const long* __restrict__ indptr, const int* __restrict__ indices,
                                                      const V* __restrict__ data, long rows, const Y* __restrict__ y,
                                                      double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long w = ((long)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((long)gridDim.x * 256) >> 6;
  for (long r = w; r < rows; r += nw) {
    const double yr = (double)y[r];
    const long p1 = indptr[r + 1];
    for (long p = indptr[r] + lane; p < p1; p += 64) atomicAdd(out + indices[p], (double)data[p] * yr);
  }
}

template <typename V, int T>
int gr_launch(const long* indptr, const int* indices, const V* data, long rows, int n, int* win, double scale,
              double* out, hipStream_t stream) {
  const int W = (n + T - 1) / T;
  const long npairs = (long)W * (W + 1) / 2;
  long wb = (rows * (long)(W + 1) + 255) / 256;
  if (wb > 256L * 64) wb = 256L * 64;  // grid-stride beyond 64 blocks per CU
  hipLaunchKernelGGL(csr_gram_windows_kernel, dim3((unsigned)wb), dim3(256), 0, stream, indptr, indices, rows, W, T, win);
  // slabs: enough workgroups for a few per CU, each slab a multiple of the GR_R rows a wave takes
  long slabs = (GR_TARGET_WG + npairs - 1) / npairs;
  const long units = (rows + GR_R - 1) / GR_R;
  if (slabs > units) slabs = units;
  if (slabs > 65535) slabs = 65535;
  const long slab_rows = (units + slabs - 1) / slabs * GR_R;
  slabs = (rows + slab_rows - 1) / slab_rows;
  if (npairs > 0x7fffffffL || npairs * slabs > srml_max_blocks(GR_THREADS)) return -1;
  const dim3 grid((unsigned)npairs, (unsigned)slabs);
  if (scale != 0.0)
    hipLaunchKernelGGL((csr_gram_tile_kernel<V, T, true>), grid, dim3(GR_THREADS), 0, stream, indptr, indices, data, rows,
                       n, W, win, slab_rows, scale, out);
  else
    hipLaunchKernelGGL((csr_gram_tile_kernel<V, T, false>), grid, dim3(GR_THREADS), 0, stream, indptr, indices, data,
                       rows, n, W, win, slab_rows, scale, out);
  return srml_status();
}

template <typename V>
int gr_gram(const long* indptr, const int* indices, const V* data, long rows, int n, int tile, int* win, double scale,
            double* out, hipStream_t stream) {
  if (rows <= 0 || n <= 0) return 0;
  if (tile == 0) tile = GR_T_DEFAULT;
  if (tile == 64) return gr_launch<V, 64>(indptr, indices, data, rows, n, win, scale, out, stream);
  if (tile == 128) return gr_launch<V, 128>(indptr, indices, data, rows, n, win, scale, out, stream);
  return -2;
}

template <typename V>
int gr_xty(const long* indptr, const int* indices, const V* data, long rows, const void* y, int y_f64, double* out,
           hipStream_t stream) {
  if (rows <= 0) return 0;
  long blocks = (rows + 3) / 4;
  if (blocks > 256L * 64) blocks = 256L * 64;
  if (y_f64)
    hipLaunchKernelGGL((csr_xty_kernel<V, double>), dim3((unsigned)blocks), dim3(256), 0, stream, indptr, indices, data,
                       rows, static_cast<const double*>(y), out);
  else
    hipLaunchKernelGGL((csr_xty_kernel<V, float>), dim3((unsigned)blocks), dim3(256), 0, stream, indptr, indices, data,
                       rows, static_cast<const float*>(y), out);
  return srml_status();
}
}  // namespace

// The dispatch constants of this file, for the Python layer and the tests: 0 the default tile
// width T, 1 the rows a wave takes at once (the slab unit R), 2 the segment chunk C, 3 the
// workgroups one launch aims at.
SRML_API int srml_csr_gram_config(int which) {
  switch (which) {
    case 0: return GR_T_DEFAULT;
    case 1: return GR_R;
    case 2: return GR_C;
    case 3: return (int)GR_TARGET_WG;
    default: return -1;
  }
}

// out (n x n, upper triangle) += X^T X for the `rows` rows whose offsets start at indptr (rows + 1
// absolute offsets). tile: 64, 128 or 0 (the default). win: workspace of (ceil(n / tile) + 1) * rows
// int32. scale = 0: out holds fp64 sums; scale = 2^s: out is an n x n i64 buffer of
// sum rint(x_a x_b 2^s) (srml_csr_gram_finish converts). -1: the grid overflows, -2: tile.
SRML_API int srml_csr_gram_f32(const long* indptr, const int* indices, const float* data, long rows, int n, int tile,
                               int* win, double scale, double* out, hipStream_t stream) {
  return gr_gram<float>(indptr, indices, data, rows, n, tile, win, scale, out, stream);
}

SRML_API int srml_csr_gram_f64(const long* indptr, const int* indices, const double* data, long rows, int n, int tile,
                               int* win, double scale, double* out, hipStream_t stream) {
  return gr_gram<double>(indptr, indices, data, rows, n, tile, win, scale, out, stream);
}

// out[i] += (double)buf[i] * inv_scale over the upper triangle of the n x n i64 buffer
SRML_API int srml_csr_gram_finish(const long long* buf, int n, double inv_scale, double* out, hipStream_t stream) {
  if (n <= 0) return 0;
  long blocks = ((long)n * n + 255) / 256;
  if (blocks > 256L * 64) blocks = 256L * 64;
  hipLaunchKernelGGL(csr_gram_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, buf, n, inv_scale, out);
  return srml_status();
}

// out (n fp64) += X^T y; y has `rows` values, fp64 when y_f64 != 0 and fp32 otherwise
SRML_API int srml_csr_xty_f32(const long* indptr, const int* indices, const float* data, long rows, const void* y,
                              int y_f64, double* out, hipStream_t stream) {
  return gr_xty<float>(indptr, indices, data, rows, y, y_f64, out, stream);
}

SRML_API int srml_csr_xty_f64(const long* indptr, const int* indices, const double* data, long rows, const void* y,
                              int y_f64, double* out, hipStream_t stream) {
  return gr_xty<double>(indptr, indices, data, rows, y, y_f64, out, stream);
}
