// NN-descent join on CSR rows in the sparse route's own metrics (UMAP's approximate sparse graph):
//
//  * srml_csr_nnd_join_f32 — for every query row i of a row block, the k nearest rows among
//      its own list                 pos[i, :kw]
//      its neighbours' neighbours   pos[pos[i, :a], :b]
//      its reverse neighbours       perm[off[i] .. off[i] + R) / kw   (edges grouped by target)
//    re-ranked by the distance of the CSR rows themselves.
//
// One 256-thread workgroup (four 64-lane waves) owns one graph row:
//
//  1. the row's non-zeros are staged in LDS when there are at most NJ_CAP of them; a longer row is
//     read from global memory (as csr_refine_kernel does);
//  2. the kw + a b + R candidate slots are gathered into LDS, one slot per thread; -1 entries, ids
//     outside [0, N) and the slots past a short reverse list become NJ_NONE;
//  3. the slots are sorted (bitonic, in LDS), so duplicates are neighbours: a slot equal to the one
//     before it is dropped BEFORE any distance is computed;
//  4. each wave takes live slots in turn, its lanes stride the item's non-zeros and look the
//     columns up in the query row (csr_pair.h); the metric is a template parameter:
//       0 sqeuclidean  sum (x_j - y_j)^2 over the union of the supports (direct form)
//       1 hellinger    sqrt(max(0, 1 - S)) on values that hold sqrt(x)
//       2 jaccard      (u - S) / u, u = nnz_x + nnz_y - S, 0 when u = 0 (S an exact integer in fp32)
//  5. (orderable fp32 bits << 32 | id) keys are sorted in LDS and the first k written: ascending by
//     (key, id), equal keys to the lower id, missing places +inf / -1.
//
// A row that lists itself is a candidate like any other and keeps itself at its true distance. No
// atomics, no cross-block state: the output is a pure function of the inputs. Both CSRs carry
// ABSOLUTE row offsets (see csr_knn.hip); ids index the item matrix.
#include "common.h"
#include "csr_pair.h"  // ck_lower_bound, rf_pair, rf_dot

namespace {
enum : int { NJ_SQEUCLIDEAN = 0, NJ_HELLINGER = 1, NJ_JACCARD = 2 };

constexpr int NJ_T = 256;        // threads per block
constexpr int NJ_WAVES = NJ_T / 64;
constexpr int NJ_CAND = 512;     // candidate slots (kw + a b + R) per row; a power of two
constexpr int NJ_CAP = 2048;     // query non-zeros staged in LDS (index + value: 16 KiB)
constexpr int NJ_KMAX = 64;      // output width
constexpr int NJ_NONE = 0x7fffffff;  // an empty slot: sorts after every id
constexpr unsigned long long NJ_EMPTY = ~0ull;  // an empty key: no id has all 32 low bits set
constexpr int NJ_LDS = NJ_CAP * 8 + NJ_CAND * 12;
constexpr int NJ_LDS_MAX = 64 * 1024;  // static LDS of one workgroup

// ascending bitonic sort of s[0 .. P), P a power of two >= 2, by the whole block
template <typename T>
__device__ __forceinline__ void nj_sort(T* s, int P, int t) {
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int p = t; p < (P >> 1); p += NJ_T) {
        const int i = 2 * p - (p & (stride - 1));  // the pair's lower index: bit `stride` clear
        const int j = i + stride;
        const bool up = (i & size) == 0;
        const T x = s[i], y = s[j];
        if ((x > y) == up) {
          s[i] = y;
          s[j] = x;
        }
      }
    }
  }
  __syncthreads();
}

// fp32 bits whose unsigned order is the order of the floats (-0 < +0, NaNs at the ends)
__device__ __forceinline__ unsigned nj_orderable(float d) {
  const unsigned b = (unsigned)__float_as_int(d);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float nj_float(unsigned o) {
  return __int_as_float((int)((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o));
}

template <int M, typename PI, typename PV>
__device__ __forceinline__ float nj_key(PI xi, PV xv, long nx, float qa, const int* __restrict__ yi,
                                        const float* __restrict__ yv, long ny, float ia, int lane) {
  if constexpr (M == NJ_SQEUCLIDEAN) return rf_pair(xi, xv, nx, yi, yv, ny, lane);
  const float S = rf_dot(xi, xv, nx, yi, yv, ny, lane);
  if constexpr (M == NJ_HELLINGER) return sqrtf(fmaxf(0.f, 1.f - S));
  const float uni = qa + ia - S;  // JACCARD
  return uni > 0.f ? (uni - S) / uni : 0.f;
}

template <int M>
__global__ __launch_bounds__(NJ_T) void csr_nnd_join_kernel(
    const long* __restrict__ qptr, const int* __restrict__ qidx, const float* __restrict__ qval,
    const float* __restrict__ qaux, long row0, const long* __restrict__ iptr, const int* __restrict__ iidx,
    const float* __restrict__ ival, const float* __restrict__ iaux, long N, const long long* __restrict__ pos, int kw,
    const long long* __restrict__ perm, const long long* __restrict__ off, int k, int a, int b, int R, int P,
    float* __restrict__ outk, long long* __restrict__ outi) {
  __shared__ int sI[NJ_CAP];
  __shared__ float sV[NJ_CAP];
  __shared__ int sC[NJ_CAND];
  __shared__ unsigned long long sK[NJ_CAND];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long q = blockIdx.x, i = row0 + q;  // the block's row and its row in the graph
  const long x0 = qptr[q], nx = qptr[q + 1] - x0;
  const bool staged = nx <= NJ_CAP;
  if (staged) {
    for (long p = t; p < nx; p += NJ_T) {
      sI[p] = qidx[x0 + p];
      sV[p] = qval[x0 + p];
    }
  }
  // candidate slots: own list, neighbours' neighbours, reverse neighbours; P - total empty ones
  const int ab = a * b, total = kw + ab + R;
  const long long nperm = (long long)N * kw;
  for (int s = t; s < P; s += NJ_T) {
    long long id = -1;
    if (s < kw) {
      id = pos[i * kw + s];
    } else if (s < kw + ab) {
      const int e = s - kw;
      const long long nb = pos[i * kw + e / b];
      if (nb >= 0 && nb < N) id = pos[nb * kw + e % b];
    } else if (s < total) {
      const long long p = off[i] + (s - kw - ab);
      if (p >= 0 && p < off[i + 1] && p < nperm) {
        const long long e = perm[p];
        if (e >= 0 && e < nperm) id = e / kw;
      }
    }
    sC[s] = (id >= 0 && id < N) ? (int)id : NJ_NONE;
  }
  nj_sort(sC, P, t);  // its first barrier also orders the staging and the gather before the sort
  float qa = 0.f;
  if constexpr (M == NJ_JACCARD) qa = qaux[q];
  for (int s = wave; s < P; s += NJ_WAVES) {  // wave-uniform throughout
    const int id = sC[s];
    unsigned long long key = NJ_EMPTY;
    if (id != NJ_NONE && (s == 0 || sC[s - 1] != id)) {
      const long y0 = iptr[id], ny = iptr[id + 1] - y0;
      float ia = 0.f;
      if constexpr (M == NJ_JACCARD) ia = iaux[id];
      const float d = staged ? nj_key<M>((const int*)sI, (const float*)sV, nx, qa, iidx + y0, ival + y0, ny, ia, lane)
                             : nj_key<M>(qidx + x0, qval + x0, nx, qa, iidx + y0, ival + y0, ny, ia, lane);
      key = ((unsigned long long)nj_orderable(d) << 32) | (unsigned)id;
    }
    if (lane == 0) sK[s] = key;
  }
  nj_sort(sK, P, t);
  for (int j = t; j < k; j += NJ_T) {
    const unsigned long long key = j < P ? sK[j] : NJ_EMPTY;
    const bool none = key == NJ_EMPTY;
    outk[q * k + j] = none ? __int_as_float(0x7f800000) : nj_float((unsigned)(key >> 32));
    outi[q * k + j] = none ? -1LL : (long long)(key & 0xffffffffull);
  }
}

template <int M>
int nj_launch(const long* qptr, const int* qidx, const float* qval, const float* qaux, long rows, long row0,
              const long* iptr, const int* iidx, const float* ival, const float* iaux, long N, const long long* pos,
              int kw, const long long* perm, const long long* off, int k, int a, int b, int R, int P, float* outk,
              long long* outi, hipStream_t stream) {
  hipLaunchKernelGGL((csr_nnd_join_kernel<M>), dim3((unsigned)rows), dim3(NJ_T), 0, stream, qptr, qidx, qval, qaux,
                     row0, iptr, iidx, ival, iaux, N, pos, kw, perm, off, k, a, b, R, P, outk, outi);
  return srml_status();
}
}  // namespace

// The dispatch constants of this file, for the Python layer's checks: 0 candidate slots per row,
// 1 query non-zeros staged in LDS, 2 largest output width.
SRML_API int srml_csr_nnd_config(int which) {
  switch (which) {
    case 0: return NJ_CAND;
    case 1: return NJ_CAP;
    case 2: return NJ_KMAX;
    default: return -1;
  }
}

// (outk fp32, outi int64) [rows, k] = the k nearest candidates of graph rows row0 .. row0 + rows.
// qptr points at the block's first row offset (rows + 1 absolute offsets into qidx / qval), qaux
// at its first auxiliary; iptr / iaux are those of the whole item matrix of N rows (aux: jaccard
// non-zero counts, unused otherwise). pos is the N x kw graph, perm (N kw edge numbers grouped by
// target) and off (N + 1 group starts) its reverse lists; a, b <= kw.
// -1: the grid overflows, -2: bad metric or arguments, -3: kw + a b + R exceeds the candidate
// slots, -9: the block's LDS does not fit.
SRML_API int srml_csr_nnd_join_f32(const long* qptr, const int* qidx, const float* qval, const float* qaux, long rows,
                                   long row0, const long* iptr, const int* iidx, const float* ival, const float* iaux,
                                   long N, const long long* pos, int kw, const long long* perm, const long long* off,
                                   int k, int a, int b, int R, int metric, float* outk, long long* outi,
                                   hipStream_t stream) {
  if (rows <= 0) return 0;
  if (k < 1 || k > NJ_KMAX || kw < 1 || a < 0 || b < 0 || R < 0 || a > kw || b > kw) return -2;
  if (row0 < 0 || row0 + rows > N || N >= (long)NJ_NONE) return -2;
  if (R > NJ_CAND || (long)kw + (long)a * b + R > NJ_CAND) return -3;
  if (NJ_LDS > NJ_LDS_MAX) return -9;
  if (rows > srml_max_blocks(NJ_T)) return -1;
  int P = 2;
  while (P < kw + a * b + R) P <<= 1;
  switch (metric) {
    case NJ_SQEUCLIDEAN:
      return nj_launch<NJ_SQEUCLIDEAN>(qptr, qidx, qval, qaux, rows, row0, iptr, iidx, ival, iaux, N, pos, kw, perm, off,
                                       k, a, b, R, P, outk, outi, stream);
    case NJ_HELLINGER:
      return nj_launch<NJ_HELLINGER>(qptr, qidx, qval, qaux, rows, row0, iptr, iidx, ival, iaux, N, pos, kw, perm, off,
                                     k, a, b, R, P, outk, outi, stream);
    case NJ_JACCARD:
      return nj_launch<NJ_JACCARD>(qptr, qidx, qval, qaux, rows, row0, iptr, iidx, ival, iaux, N, pos, kw, perm, off, k,
                                   a, b, R, P, outk, outi, stream);
    default: return -2;
  }
}
