// Pairwise distances for the metrics that are no Euclidean distance of transformed rows
// (UMAP's l1 / chebyshev / minkowski / canberra / hamming / jaccard / hellinger graphs):
//
//  * srml_pairdist_f32 — D[q][i] = d(Q[q,:], I[i,:]) for one (query chunk x item chunk).
//
// These cannot ride the MFMA ||q||^2 + ||i||^2 - 2 q.i tiles (`srml_knn_f32`, `srml_knn_dist_f32`):
// every (q, i, feature) term is its own VALU expression. One tiled kernel, the per-term op and
// the finaliser chosen by a template parameter (no switch in the inner loop):
//
//  * a 256-thread block owns a 64-query x 128-item tile of D; thread (ty = t / 32, tx = t % 32)
//    holds the 8 x 4 accumulators of queries 8 ty .. 8 ty + 7 and items 4 tx .. 4 tx + 3;
//  * the feature dimension streams through LDS in chunks of 32, both tiles stored feature-major
//    (sQ[k][64], sI[k][128]): per feature a thread reads its 8 query values as two 16-byte reads
//    (one address per 32 lanes: a broadcast) and its 4 item values as one 16-byte read (lanes
//    16 B apart; the sixteen lanes of every ds_read_b128 group cover all 16 slots of the 256-B
//    bank row: conflict-free). The staging writes are 4-byte, consecutive lanes on consecutive
//    rows of one feature: conflict-free;
//  * the next chunk's global loads (16-byte per lane where the strides, n and base pointers
//    allow, element loads otherwise) are issued before the current chunk's arithmetic;
//  * out-of-range rows and features are staged as 0, the identity of every op here (|0 - 0|,
//    0 != 0, a 0/0 Canberra term and a zero product all add nothing; HAMMING divides by the true
//    n); out-of-range rows and columns are never stored.
//
// JACCARD and HELLINGER are products: JACCARD stages the indicators x != 0, so the accumulator is
// the intersection count and the row non-zero counts (kept per thread for its 8 + 4 rows) give the
// union; HELLINGER expects the square roots of the rows and accumulates their product.
// Reference: the metrics of cuML UMAP (umap.py:169-179 of the reference), scipy's definitions.
#include "common.h"

namespace {
enum : int { PD_L1 = 0, PD_LINF = 1, PD_MINKOWSKI = 2, PD_CANBERRA = 3, PD_HAMMING = 4, PD_JACCARD = 5,
             PD_HELLINGER = 6, PD_MINK3 = 7, PD_MINK4 = 8 };  // 7, 8: MINKOWSKI with p = 3 / 4 on multiplies

constexpr int PD_TQ = 64, PD_TI = 128, PD_KC = 32, PD_T = 256;

template <int M>
__device__ __forceinline__ float pd_pre(float x) {
  if constexpr (M == PD_JACCARD) return x != 0.f ? 1.f : 0.f;
  return x;
}

template <int M>
__device__ __forceinline__ void pd_term(float& acc, float a, float b, float p) {
  if constexpr (M == PD_L1) {
    acc += fabsf(a - b);
  } else if constexpr (M == PD_LINF) {
    acc = fmaxf(acc, fabsf(a - b));
  } else if constexpr (M == PD_MINKOWSKI) {
    acc += powf(fabsf(a - b), p);
  } else if constexpr (M == PD_MINK3) {
    const float t = fabsf(a - b);
    acc += t * t * t;
  } else if constexpr (M == PD_MINK4) {
    const float t = (a - b) * (a - b);
    acc += t * t;
  } else if constexpr (M == PD_CANBERRA) {
    const float s = fabsf(a) + fabsf(b);
    acc += s > 0.f ? fabsf(a - b) / s : 0.f;
  } else if constexpr (M == PD_HAMMING) {
    acc += a != b ? 1.f : 0.f;
  } else {  // JACCARD (indicators), HELLINGER (square roots)
    acc = fmaf(a, b, acc);
  }
}

template <int M>
__device__ __forceinline__ float pd_final(float acc, float qnz, float inz, int n, float p) {
  if constexpr (M == PD_MINKOWSKI) return powf(acc, 1.f / p);
  if constexpr (M == PD_MINK3) return cbrtf(acc);
  if constexpr (M == PD_MINK4) return sqrtf(sqrtf(acc));
  if constexpr (M == PD_HAMMING) return acc / (float)n;
  if constexpr (M == PD_JACCARD) {
    const float uni = qnz + inz - acc;
    return uni > 0.f ? (uni - acc) / uni : 0.f;
  }
  if constexpr (M == PD_HELLINGER) return sqrtf(fmaxf(0.f, 1.f - acc));
  return acc;
}

// global -> registers: the ROWS x 32 block at (row0, k0) of a row-major matrix; element e of the
// thread is (row f % ROWS, feature f / ROWS [VEC: 4 features from 4 (f / ROWS)]) of
// f = t + 256 (e [VEC: e / 4])
template <int ROWS, int M, bool VEC>
__device__ __forceinline__ void pd_load(const float* __restrict__ X, long ld, long m, long row0, int k0, int n,
                                        float (&r)[ROWS * PD_KC / PD_T]) {
  constexpr int NE = ROWS * PD_KC / PD_T;
  const int t = threadIdx.x;
  if constexpr (VEC) {
#pragma unroll
    for (int e = 0; e < NE / 4; ++e) {
      const int f = t + PD_T * e;
      const long row = row0 + f % ROWS;
      const int k = k0 + 4 * (f / ROWS);
      floatx4 v = {0.f, 0.f, 0.f, 0.f};
      if (row < m && k < n) v = *reinterpret_cast<const floatx4*>(X + row * ld + k);  // n % 4 == 0: whole quad in range
#pragma unroll
      for (int j = 0; j < 4; ++j) r[4 * e + j] = pd_pre<M>(v[j]);
    }
  } else {
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int f = t + PD_T * e;
      const long row = row0 + f % ROWS;
      const int k = k0 + f / ROWS;
      r[e] = (row < m && k < n) ? pd_pre<M>(X[row * ld + k]) : 0.f;
    }
  }
}

// registers -> the feature-major LDS image s[k][ROWS]
template <int ROWS, bool VEC>
__device__ __forceinline__ void pd_stage(const float (&r)[ROWS * PD_KC / PD_T], float* __restrict__ s) {
  constexpr int NE = ROWS * PD_KC / PD_T;
  const int t = threadIdx.x;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const int f = t + PD_T * (VEC ? e / 4 : e);
    const int k = VEC ? 4 * (f / ROWS) + (e & 3) : f / ROWS;
    s[k * ROWS + f % ROWS] = r[e];
  }
}

template <int M, bool VEC>
__global__ __launch_bounds__(PD_T, 2) void pairdist_kernel(const float* __restrict__ Q, long mq, int n, long ldq,
                                                           const float* __restrict__ I, long mi, long ldi, float p,
                                                           float* __restrict__ D, long ldd, int n_itiles, int vec_st) {
  __shared__ __attribute__((aligned(16))) float sQ[PD_KC * PD_TQ];
  __shared__ __attribute__((aligned(16))) float sI[PD_KC * PD_TI];
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const long q0 = (long)(bid / n_itiles) * PD_TQ;
  const long i0 = (long)(bid % n_itiles) * PD_TI;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  float acc[8][4];
  float qnz[8], inz[4];  // JACCARD: non-zero counts of the thread's rows
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    qnz[u] = 0.f;
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) inz[v] = 0.f;
  float rq[PD_TQ * PD_KC / PD_T], ri[PD_TI * PD_KC / PD_T];
  pd_load<PD_TQ, M, VEC>(Q, ldq, mq, q0, 0, n, rq);
  pd_load<PD_TI, M, VEC>(I, ldi, mi, i0, 0, n, ri);
  for (int k0 = 0; k0 < n; k0 += PD_KC) {
    __syncthreads();  // the previous chunk's reads are done
    pd_stage<PD_TQ, VEC>(rq, sQ);
    pd_stage<PD_TI, VEC>(ri, sI);
    __syncthreads();
    if (k0 + PD_KC < n) {
      pd_load<PD_TQ, M, VEC>(Q, ldq, mq, q0, k0 + PD_KC, n, rq);
      pd_load<PD_TI, M, VEC>(I, ldi, mi, i0, k0 + PD_KC, n, ri);
    }
    const int kend = min(PD_KC, (n - k0 + 3) & ~3);  // features past n inside the last quad are staged 0
    for (int kk = 0; kk < kend; kk += 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = kk + j;
        const floatx4 a0 = *reinterpret_cast<const floatx4*>(&sQ[k * PD_TQ + 8 * ty]);
        const floatx4 a1 = *reinterpret_cast<const floatx4*>(&sQ[k * PD_TQ + 8 * ty + 4]);
        const floatx4 b = *reinterpret_cast<const floatx4*>(&sI[k * PD_TI + 4 * tx]);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float a = u < 4 ? a0[u & 3] : a1[u & 3];
          if constexpr (M == PD_JACCARD) qnz[u] += a;
#pragma unroll
          for (int v = 0; v < 4; ++v) pd_term<M>(acc[u][v], a, b[v], p);
        }
        if constexpr (M == PD_JACCARD) {
#pragma unroll
          for (int v = 0; v < 4; ++v) inz[v] += b[v];
        }
      }
    }
  }
  const long i = i0 + 4 * tx;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const long q = q0 + 8 * ty + u;
    if (q >= mq) continue;
    floatx4 d;
#pragma unroll
    for (int v = 0; v < 4; ++v) d[v] = pd_final<M>(acc[u][v], qnz[u], inz[v], n, p);
    if (vec_st && i + 3 < mi) {
      *reinterpret_cast<floatx4*>(D + q * ldd + i) = d;
    } else {
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (i + v < mi) D[q * ldd + i + v] = d[v];
    }
  }
}

template <int M>
int pd_launch(const float* Q, long mq, int n, long ldq, const float* I, long mi, long ldi, float p, float* D, long ldd,
              hipStream_t stream) {
  const long nq = (mq + PD_TQ - 1) / PD_TQ, ni = (mi + PD_TI - 1) / PD_TI;
  if (ni > 0x7fffffffL || nq * ni > srml_max_blocks(PD_T)) return -1;
  const bool vec = ((ldq & 3) == 0) && ((ldi & 3) == 0) && ((n & 3) == 0) &&
                   ((reinterpret_cast<uintptr_t>(Q) & 15) == 0) && ((reinterpret_cast<uintptr_t>(I) & 15) == 0);
  const int vec_st = ((ldd & 3) == 0) && ((reinterpret_cast<uintptr_t>(D) & 15) == 0);
  if (vec)
    hipLaunchKernelGGL((pairdist_kernel<M, true>), dim3((unsigned)(nq * ni)), dim3(PD_T), 0, stream, Q, mq, n, ldq, I,
                       mi, ldi, p, D, ldd, (int)ni, vec_st);
  else
    hipLaunchKernelGGL((pairdist_kernel<M, false>), dim3((unsigned)(nq * ni)), dim3(PD_T), 0, stream, Q, mq, n, ldq,
                       I, mi, ldi, p, D, ldd, (int)ni, vec_st);
  return srml_status();
}
}  // namespace

// D (mq x mi, leading dim ldd) = d(Q[q,:], I[i,:]) for one (query chunk, item chunk). metric:
// 0 L1, 1 LINF, 2 MINKOWSKI (exponent p >= 1), 3 CANBERRA, 4 HAMMING, 5 JACCARD (non-zero
// patterns), 6 HELLINGER (Q and I hold the square roots of the rows). -1: the grid overflows,
// -2: unknown metric or a bad p.
SRML_API int srml_pairdist_f32(const float* Q, long mq, int n, long ldq, const float* I, long mi, long ldi,
                               int metric, float p, float* D, long ldd, hipStream_t stream) {
  if (mq <= 0 || mi <= 0) return 0;
  if (n <= 0) return -2;
  switch (metric) {
    case PD_L1: return pd_launch<PD_L1>(Q, mq, n, ldq, I, mi, ldi, p, D, ldd, stream);
    case PD_LINF: return pd_launch<PD_LINF>(Q, mq, n, ldq, I, mi, ldi, p, D, ldd, stream);
    case PD_MINKOWSKI:
      if (!(p >= 1.f) || !(p < 3.0e38f)) return -2;
      if (p == 1.f) return pd_launch<PD_L1>(Q, mq, n, ldq, I, mi, ldi, p, D, ldd, stream);
      if (p == 3.f) return pd_launch<PD_MINK3>(Q, mq, n, ldq, I, mi, ldi, p, D, ldd, stream);
      if (p == 4.f) return pd_launch<PD_MINK4>(Q, mq, n, ldq, I, mi, ldi, p, D, ldd, stream);
      return pd_launch<PD_MINKOWSKI>(Q, mq, n, ldq, I, mi, ldi, p, D, ldd, stream);
    case PD_CANBERRA: return pd_launch<PD_CANBERRA>(Q, mq, n, ldq, I, mi, ldi, p, D, ldd, stream);
    case PD_HAMMING: return pd_launch<PD_HAMMING>(Q, mq, n, ldq, I, mi, ldi, p, D, ldd, stream);
    case PD_JACCARD: return pd_launch<PD_JACCARD>(Q, mq, n, ldq, I, mi, ldi, p, D, ldd, stream);
    case PD_HELLINGER: return pd_launch<PD_HELLINGER>(Q, mq, n, ldq, I, mi, ldi, p, D, ldd, stream);
    default: return -2;
  }
}
