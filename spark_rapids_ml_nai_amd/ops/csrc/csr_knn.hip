// Exact nearest neighbours between two CSR row sets (UMAP on sparse features):
//
//  * srml_csr_pairdist_f32 — D[q][i] = key(Q[q0 + q, :], I[i0 + i, :]) for one (query chunk x item
//    chunk), from the sparse dot S = sum_j x_j y_j and a per-metric finaliser;
//  * srml_csr_refine_f32   — direct-form squared Euclidean distances of selected (query, item)
//    pairs: every (x_j - y_j)^2 over the union of the two supports, no difference of sums.
//
// Both CSRs are (int64 row offsets, int32 column indices, fp32 values) with ABSOLUTE offsets: a
// row block of a larger CSR is a pointer into its row offsets, the index / value pointers stay
// those of the whole matrix. Column indices are in [0, n) and strictly increasing within a row
// (ops.csr_prepare checks it once); the kernels rely on it for the window search and only clamp
// the LDS offsets.
//
// srml_csr_pairdist_f32: a 512-thread block owns CK_TQ = 16 query rows x CK_TI = 512 item rows,
// one item row per thread. Columns are processed in windows of CK_W = 1024:
//
//  * the block keeps a dense image of its queries' window in LDS, sX[CK_W][CK_TQ] (query-minor:
//    the 16 query values of one column are 64 contiguous bytes, four ds_read_b128). It is zeroed
//    once; per window the queries' non-zeros are scattered in (32 threads stride one query row)
//    and the same cells are zeroed again afterwards, so a window costs O(non-zeros), not O(W);
//  * rows are sorted, so every thread keeps a cursor into its row: the window's end is one binary
//    search from the cursor, O(log nnz) per (row, window), all 64 rows of a wave searching at once;
//  * a thread walks its row's non-zeros of the window and accumulates the 16 dots in registers
//    (products added in column order); the accumulators live across the windows, so nothing is
//    accumulated through memory and no atomics are needed. A row with >= CK_COOP non-zeros in the
//    window is taken by its whole wave instead (lanes stride the non-zeros, DPP reduction), so one
//    long row does not serialise 63 idle lanes behind it;
//  * after the last window the finaliser is applied and, per query, the 64 lanes of a wave store
//    64 consecutive floats of a D row.
//
// Keys (metric code):
//   0 sqeuclidean  max(0, |x|^2 + |y|^2 - 2 S)             aux = row squared norms
//   1 hellinger    sqrt(max(0, 1 - S)) on values that hold sqrt(x) (cuML's un-normalised form)
//   2 jaccard      (u - S) / u, u = nnz_x + nnz_y - S, 0 when u = 0, on indicator values (S is an
//                  exact integer in fp32)                   aux = row non-zero counts
// Cosine is the sqeuclidean key of unit rows (the caller scales the values).
#include "common.h"
#include "csr_pair.h"  // ck_lower_bound, rf_pair

namespace {
enum : int { CK_SQEUCLIDEAN = 0, CK_HELLINGER = 1, CK_JACCARD = 2 };

constexpr int CK_T = 512;      // threads per block
constexpr int CK_TQ = 16;      // query rows per block
constexpr int CK_TI = CK_T;    // item rows per block: one per thread
constexpr int CK_W = 1024;     // columns per window
constexpr int CK_COOP = 64;    // non-zeros of one (row, window) from which the wave shares the row
constexpr int CK_QG = CK_T / CK_TQ;  // threads striding one query row's non-zeros
constexpr int CK_LDS = CK_W * CK_TQ * (int)sizeof(float);
constexpr int CK_LDS_MAX = 160 * 1024;

constexpr int RF_T = 256;      // refine: 4 waves per query
constexpr int RF_CAP = 2048;   // query non-zeros staged in LDS (index + value: 16 KiB)

__device__ __forceinline__ long ck_shfl(long v, int src) {
  const int lo = __shfl((int)(v & 0xffffffffL), src, 64);
  const int hi = __shfl((int)(v >> 32), src, 64);
  return ((long)hi << 32) | (unsigned)lo;
}

// acc[0 .. 15] += v * sX[c][0 .. 15]
__device__ __forceinline__ void ck_gather(const float* __restrict__ sX, int c, float v, float (&acc)[CK_TQ]) {
  const floatx4* col = reinterpret_cast<const floatx4*>(sX + (long)c * CK_TQ);
#pragma unroll
  for (int g = 0; g < CK_TQ / 4; ++g) {
    const floatx4 x = col[g];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[4 * g + j] = fmaf(v, x[j], acc[4 * g + j]);
  }
}

template <int M>
__device__ __forceinline__ float ck_final(float S, float qa, float ia) {
  if constexpr (M == CK_SQEUCLIDEAN) return fmaxf(0.f, qa + ia - 2.f * S);
  if constexpr (M == CK_HELLINGER) return sqrtf(fmaxf(0.f, 1.f - S));
  const float uni = qa + ia - S;  // JACCARD
  return uni > 0.f ? (uni - S) / uni : 0.f;
}

template <int M>
__global__ __launch_bounds__(CK_T) void csr_pairdist_kernel(
    const long* __restrict__ qptr, const int* __restrict__ qidx, const float* __restrict__ qval,
    const float* __restrict__ qaux, long r, const long* __restrict__ iptr, const int* __restrict__ iidx,
    const float* __restrict__ ival, const float* __restrict__ iaux, long L, int n, float* __restrict__ D, long ldd,
    int n_iblocks) {
  extern __shared__ __attribute__((aligned(16))) float sX[];  // [CK_W][CK_TQ]
  const int t = threadIdx.x, lane = t & 63;
  const long qb = blockIdx.x / n_iblocks, ib = blockIdx.x % n_iblocks;
  // this thread's item row and its cursor
  const long irow = ib * CK_TI + t;
  long ipos = 0, iend = 0;
  if (irow < L) {
    ipos = iptr[irow];
    iend = iptr[irow + 1];
  }
  // the query row this thread helps to scatter
  const int qg = t / CK_QG, qs = t % CK_QG;
  const long qrow = qb * CK_TQ + qg;
  long qpos = 0, qend = 0;
  if (qrow < r) {
    qpos = qptr[qrow];
    qend = qptr[qrow + 1];
  }
  for (int i = t; i < CK_W * CK_TQ / 4; i += CK_T) reinterpret_cast<floatx4*>(sX)[i] = floatx4{0.f, 0.f, 0.f, 0.f};
  float acc[CK_TQ];
#pragma unroll
  for (int q = 0; q < CK_TQ; ++q) acc[q] = 0.f;
  for (long w0 = 0; w0 < n; w0 += CK_W) {
    const bool last = w0 + CK_W >= n;
    const int w1 = last ? n : (int)(w0 + CK_W);
    const long qe = last ? qend : ck_lower_bound(qidx, qpos, qend, w1);
    __syncthreads();  // the image is all zero again
    for (long p = qpos + qs; p < qe; p += CK_QG) {
      const unsigned c = (unsigned)(qidx[p] - (int)w0);
      if (c < (unsigned)CK_W) sX[c * CK_TQ + qg] = qval[p];
    }
    __syncthreads();
    const long ie = last ? iend : ck_lower_bound(iidx, ipos, iend, w1);
    const bool shared_row = ie - ipos >= CK_COOP;
    if (!shared_row) {
      for (long p = ipos; p < ie; ++p) {
        const unsigned c = (unsigned)(iidx[p] - (int)w0);
        if (c < (unsigned)CK_W) ck_gather(sX, (int)c, ival[p], acc);
      }
    }
    unsigned long long big = __ballot(shared_row);
    while (big) {  // wave-uniform
      const int j = __ffsll((long long)big) - 1;
      big &= big - 1;
      const long s = ck_shfl(ipos, j), e = ck_shfl(ie, j);
      float part[CK_TQ];
#pragma unroll
      for (int q = 0; q < CK_TQ; ++q) part[q] = 0.f;
      for (long p = s + lane; p < e; p += 64) {
        const unsigned c = (unsigned)(iidx[p] - (int)w0);
        if (c < (unsigned)CK_W) ck_gather(sX, (int)c, ival[p], part);
      }
#pragma unroll
      for (int q = 0; q < CK_TQ; ++q) {
        const float tot = wave_sum(part[q]);
        if (lane == j) acc[q] += tot;
      }
    }
    ipos = ie;
    __syncthreads();  // every gather of this window is done
    for (long p = qpos + qs; p < qe; p += CK_QG) {
      const unsigned c = (unsigned)(qidx[p] - (int)w0);
      if (c < (unsigned)CK_W) sX[c * CK_TQ + qg] = 0.f;
    }
    qpos = qe;
  }
  if (irow >= L) return;
  float ia = 0.f;
  if constexpr (M != CK_HELLINGER) ia = iaux[irow];
#pragma unroll
  for (int q = 0; q < CK_TQ; ++q) {
    const long row = qb * CK_TQ + q;
    if (row < r) {
      float qa = 0.f;
      if constexpr (M != CK_HELLINGER) qa = qaux[row];
      D[row * ldd + irow] = ck_final<M>(acc[q], qa, ia);
    }
  }
}

template <int M>
int ck_launch(const long* qptr, const int* qidx, const float* qval, const float* qaux, long r, const long* iptr,
              const int* iidx, const float* ival, const float* iaux, long L, int n, float* D, long ldd,
              hipStream_t stream) {
  const long nq = (r + CK_TQ - 1) / CK_TQ, ni = (L + CK_TI - 1) / CK_TI;
  if (ni > 0x7fffffffL || nq * ni > srml_max_blocks(CK_T)) return -1;
  if (CK_LDS > 48 * 1024)
    (void)hipFuncSetAttribute((const void*)csr_pairdist_kernel<M>, hipFuncAttributeMaxDynamicSharedMemorySize, CK_LDS);
  hipLaunchKernelGGL((csr_pairdist_kernel<M>), dim3((unsigned)(nq * ni)), dim3(CK_T), CK_LDS, stream, qptr, qidx, qval,
                     qaux, r, iptr, iidx, ival, iaux, L, n, D, ldd, (int)ni);
  return srml_status();
}

__global__ __launch_bounds__(RF_T) void csr_refine_kernel(const long* __restrict__ qptr, const int* __restrict__ qidx,
                                                          const float* __restrict__ qval, const long* __restrict__ iptr,
                                                          const int* __restrict__ iidx, const float* __restrict__ ival,
                                                          long mi, const long long* __restrict__ ids, int k, long ldi,
                                                          float* __restrict__ out, long ldo) {
  __shared__ int sI[RF_CAP];
  __shared__ float sV[RF_CAP];
  const long q = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long x0 = qptr[q], nx = qptr[q + 1] - x0;
  const bool staged = nx <= RF_CAP;
  if (staged) {
    for (long p = threadIdx.x; p < nx; p += RF_T) {
      sI[p] = qidx[x0 + p];
      sV[p] = qval[x0 + p];
    }
  }
  __syncthreads();
  for (int j = wave; j < k; j += RF_T / 64) {
    const long long id = ids[q * ldi + j];
    float d = __int_as_float(0x7f800000);  // +inf: no candidate
    if (id >= 0 && id < mi) {
      const long y0 = iptr[id], ny = iptr[id + 1] - y0;
      d = staged ? rf_pair((const int*)sI, (const float*)sV, nx, iidx + y0, ival + y0, ny, lane)
                 : rf_pair(qidx + x0, qval + x0, nx, iidx + y0, ival + y0, ny, lane);
    }
    if (lane == 0) out[q * ldo + j] = d;
  }
}
}  // namespace

// The dispatch constants of this file, for the Python layer's checks: 0 window width, 1 query rows
// per block, 2 item rows per block, 3 non-zeros from which a wave shares a row, 4 refine LDS cap.
SRML_API int srml_csr_knn_config(int which) {
  switch (which) {
    case 0: return CK_W;
    case 1: return CK_TQ;
    case 2: return CK_TI;
    case 3: return CK_COOP;
    case 4: return RF_CAP;
    default: return -1;
  }
}

// D (r x L, leading dim ldd) = key(Q rows, I rows) for one (query chunk, item chunk); qptr / iptr
// point at the chunk's first row offset (r + 1 / L + 1 absolute offsets), qaux / iaux at its first
// auxiliary (unused for hellinger). -1: the grid overflows, -2: unknown metric or n <= 0, -9: the
// window image does not fit the LDS.
SRML_API int srml_csr_pairdist_f32(const long* qptr, const int* qidx, const float* qval, const float* qaux, long r,
                                   const long* iptr, const int* iidx, const float* ival, const float* iaux, long L,
                                   int n, int metric, float* D, long ldd, hipStream_t stream) {
  if (r <= 0 || L <= 0) return 0;
  if (n <= 0) return -2;
  if (CK_LDS > CK_LDS_MAX) return -9;
  switch (metric) {
    case CK_SQEUCLIDEAN:
      return ck_launch<CK_SQEUCLIDEAN>(qptr, qidx, qval, qaux, r, iptr, iidx, ival, iaux, L, n, D, ldd, stream);
    case CK_HELLINGER:
      return ck_launch<CK_HELLINGER>(qptr, qidx, qval, qaux, r, iptr, iidx, ival, iaux, L, n, D, ldd, stream);
    case CK_JACCARD:
      return ck_launch<CK_JACCARD>(qptr, qidx, qval, qaux, r, iptr, iidx, ival, iaux, L, n, D, ldd, stream);
    default: return -2;
  }
}

// out[q][j] = |Q[q] - I[ids[q][j]]|^2 in direct form for q < mq, j < k; ids < 0 (or >= mi) give +inf.
// iptr is the row-offset array of the whole item matrix (ids index it). -1: the grid overflows.
SRML_API int srml_csr_refine_f32(const long* qptr, const int* qidx, const float* qval, long mq, const long* iptr,
                                 const int* iidx, const float* ival, long mi, const long long* ids, int k, long ldi,
                                 float* out, long ldo, hipStream_t stream) {
  if (mq <= 0 || k <= 0) return 0;
  if (mq > srml_max_blocks(RF_T)) return -1;
  hipLaunchKernelGGL(csr_refine_kernel, dim3((unsigned)mq), dim3(RF_T), 0, stream, qptr, qidx, qval, iptr, iidx, ival,
                     mi, ids, k, ldi, out, ldo);
  return srml_status();
}
