// Pair arithmetic of two sorted sparse rows, shared by the CSR nearest-neighbour kernels
// (csr_knn.hip, csr_nnd.hip). A row is (column indices strictly increasing, fp32 values); either
// pointer may be an LDS or a global one.
#pragma once
#include "common.h"

namespace {
// first position in [lo, hi) of the sorted idx with idx[pos] >= key
template <typename P>
__device__ __forceinline__ long ck_lower_bound(P idx, long lo, long hi, int key) {
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (idx[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// squared distance of x (nx non-zeros at xi / xv, an LDS or a global pointer) and y, summed by
// one wave: the lanes stride y and look each column up in x, then stride x for the columns y lacks
template <typename PI, typename PV>
__device__ __forceinline__ float rf_pair(PI xi, PV xv, long nx, const int* __restrict__ yi,
                                         const float* __restrict__ yv, long ny, int lane) {
  float sum = 0.f;
  for (long p = lane; p < ny; p += 64) {
    const int c = yi[p];
    const float y = yv[p];
    const long pos = ck_lower_bound(xi, 0, nx, c);
    const float x = (pos < nx && xi[pos] == c) ? xv[pos] : 0.f;
    const float d = x - y;
    sum = fmaf(d, d, sum);
  }
  for (long p = lane; p < nx; p += 64) {
    const int c = xi[p];
    const long pos = ck_lower_bound(yi, 0, ny, c);
    if (!(pos < ny && yi[pos] == c)) {
      const float x = xv[p];
      sum = fmaf(x, x, sum);
    }
  }
  return wave_sum(sum);
}

// sparse dot S = sum over the common columns of x_j y_j, summed by one wave: the lanes stride y
// and look each column up in x (products added in the lane's column order, then the wave tree)
template <typename PI, typename PV>
__device__ __forceinline__ float rf_dot(PI xi, PV xv, long nx, const int* __restrict__ yi,
                                        const float* __restrict__ yv, long ny, int lane) {
  float sum = 0.f;
  for (long p = lane; p < ny; p += 64) {
    const int c = yi[p];
    const long pos = ck_lower_bound(xi, 0, nx, c);
    if (pos < nx && xi[pos] == c) sum = fmaf(xv[pos], yv[p], sum);
  }
  return wave_sum(sum);
}
}  // namespace
