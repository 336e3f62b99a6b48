// The in-LDS pieces the NN-descent join kernels share (csr_nnd.hip, nnd.hip): the block-wide bitonic
// sort of the candidate slots / packed keys and the order-preserving fp32 <-> unsigned map.
#pragma once

constexpr int NJ_T = 256;            // threads per join block
constexpr int NJ_NONE = 0x7fffffff;  // an empty slot: sorts after every id
constexpr unsigned long long NJ_EMPTY = ~0ull;  // an empty key: no id has all 32 low bits set

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
