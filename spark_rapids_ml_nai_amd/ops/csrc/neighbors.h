// Selection pieces shared by the nearest-neighbour kernels (knn.hip, knn_graph.hip, ivf.hip,
// ivfpq.hip): the list-length limit, the four wave-private sorted lists of the per-query scans,
// and the fill of a large-k candidate matrix.
#pragma once
#include "common.h"

#include "tile.h"

namespace srml_nn {
using namespace srml_tile;

// longest sorted insertion list kept in LDS; larger k goes through a candidate matrix + topk_rows
constexpr int NN_KMAX = 64;

// ------------------------------------------------------------------------------------------
// Wave lists of the per-query scans (one block of 4 waves per query): every wave keeps a sorted
// list of its k best (key, id) pairs in LDS; candidates are offered wave-uniformly in item order,
// so ties keep the earlier item; one thread merges the four lists at the end.
// ------------------------------------------------------------------------------------------
typedef float WaveD[4][NN_KMAX];
typedef long long WaveI[4][NN_KMAX];

__device__ __forceinline__ void wave_lists_init(WaveD& wd, WaveI& wi) {
  for (int j = threadIdx.x; j < 4 * NN_KMAX; j += 256) {
    (&wd[0][0])[j] = __builtin_huge_valf();
    (&wi[0][0])[j] = -1;
  }
}

// Wave-uniform dg < thr: lane 0 inserts (dg, id) into this wave's list; thr becomes its k-th key.
__device__ __forceinline__ void wave_list_offer(WaveD& wd, WaveI& wi, int k, float dg, long long id, float& thr) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    int pos = k - 1;
    while (pos > 0 && wd[wid][pos - 1] > dg) {
      wd[wid][pos] = wd[wid][pos - 1];
      wi[wid][pos] = wi[wid][pos - 1];
      --pos;
    }
    wd[wid][pos] = dg;
    wi[wid][pos] = id;
  }
  __builtin_amdgcn_wave_barrier();
  thr = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(wd[wid][k - 1])));
}

// One thread, after a __syncthreads(): the k smallest of the four lists, ascending (+inf / -1 padded).
__device__ __forceinline__ void wave_lists_merge_write(WaveD& wd, const WaveI& wi, int k, float* out_d,
                                                       long long* out_i) {
  int h[4] = {0, 0, 0, 0};
  for (int j = 0; j < k; ++j) {
    int bw = 0;
    float bd = wd[0][h[0]];
    for (int w = 1; w < 4; ++w)
      if (wd[w][h[w]] < bd) { bd = wd[w][h[w]]; bw = w; }
    out_d[j] = bd;
    out_i[j] = bd < __builtin_huge_valf() ? wi[bw][h[bw]] : -1;
    if (h[bw] < k - 1) ++h[bw]; else wd[bw][h[bw]] = __builtin_huge_valf();
  }
}

// D[i] = +inf, DI[i] = -1 for i < total: an empty large-k candidate matrix (defined in ivf.hip).
__attribute__((visibility("hidden"))) void fill_candidates(float* D, long long* DI, long total, hipStream_t stream);

}  // namespace srml_nn
