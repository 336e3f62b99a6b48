// The product-quantiser lookup table in LDS and an item's sum over it, shared by the IVF-PQ scans
// (ivfpq.hip) and the code-scoring CAGRA search (cagra.hip). Both run 256-thread workgroups.
#pragma once
#include "common.h"

namespace srml_pq {
constexpr int PQ_T = 256;

// Table of one (query, list): qr holds q - c_l (L2) or q (inner product).
__device__ __forceinline__ void pq_build_lut(const float* qr, const float* __restrict__ cbT, int M, int ksub, int dsub,
                                             int ip, float* lut) {
  for (int e = threadIdx.x; e < M * ksub; e += PQ_T) {
    const int m = e / ksub, j = e - m * ksub;
    const float* col = cbT + (long)m * dsub * ksub + j;
    const float* r = qr + m * dsub;
    float acc = 0.f;
    if (ip) {
      for (int d = 0; d < dsub; ++d) acc = fmaf(r[d], col[(long)d * ksub], acc);
    } else {
      for (int d = 0; d < dsub; ++d) {
        const float diff = r[d] - col[(long)d * ksub];
        acc = fmaf(diff, diff, acc);
      }
    }
    lut[e] = acc;
  }
}

// Sum of one item's M table entries. A code past the codebook (foreign data) reads the last entry.
__device__ __forceinline__ float pq_item_sum(const unsigned char* __restrict__ row, const float* lut, int M, int ksub,
                                             bool vec) {
  const unsigned top = (unsigned)ksub - 1u;
  float acc = 0.f;
  if (vec) {
    const unsigned* w = reinterpret_cast<const unsigned*>(row);
    for (int m4 = 0; m4 < (M >> 2); ++m4) {
      const unsigned c = w[m4];
      const float* L = lut + (m4 * 4) * ksub;
      acc += L[min(c & 255u, top)];
      acc += L[ksub + min((c >> 8) & 255u, top)];
      acc += L[2 * ksub + min((c >> 16) & 255u, top)];
      acc += L[3 * ksub + min(c >> 24, top)];
    }
  } else {
    for (int m = 0; m < M; ++m) acc += lut[m * ksub + min((unsigned)row[m], top)];
  }
  return acc;
}
}  // namespace srml_pq
