// The per-term ops of the metrics that are no Euclidean distance of transformed rows, shared by the
// tiled all-pairs kernel (pairdist.hip) and the dense NN-descent join (nnd.hip). A distance is
//   pd_final<M>( fold over features of pd_term<M>(acc, pd_pre<M>(x_j), pd_pre<M>(y_j)) )
// with acc starting at 0 (every term is >= 0, LINF folds with max). The metric is a template
// parameter: no switch in an inner loop. scipy's definitions; HELLINGER rows hold square roots.
#pragma once

enum : int { PD_L1 = 0, PD_LINF = 1, PD_MINKOWSKI = 2, PD_CANBERRA = 3, PD_HAMMING = 4, PD_JACCARD = 5,
             PD_HELLINGER = 6, PD_MINK3 = 7, PD_MINK4 = 8,  // 7, 8: MINKOWSKI with p = 3 / 4 on multiplies
             PD_SQEUCLIDEAN = 9 };  // sum (x - y)^2 in direct form (nnd.hip only)

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
  } else if constexpr (M == PD_SQEUCLIDEAN) {
    const float t = a - b;
    acc = fmaf(t, t, acc);
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
