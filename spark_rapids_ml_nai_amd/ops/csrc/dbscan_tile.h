// Per-tile bodies of the DBSCAN sweeps, shared by the triangle sweeps (dbscan.hip) and the list-driven
// sweeps over permuted rows (dbscan_rbc.hip).
//
// A tile pair (bi, bj), bj <= bi, is rows r0 = 128 bi and columns c0 = 128 bj of the matrix the
// distances are taken on: *positions*. What the results live in (counts, core, parent, best) is
// indexed by *ids*: an id map turns slot s of the tile pair (rows 0..127, columns 128..255) into
// the id of the row at that position. The triangle sweeps use the identity (id = position); the
// list sweeps read the 256 ids from LDS. The self pair is a matter of positions, the union-find
// roots and the border keys of ids.
#pragma once
#include "common.h"
#include "tile.h"

namespace srml_dbscan {
using namespace srml_tile;

__device__ __forceinline__ void tri_decode(long t, long& bi, long& bj) {
  double d = sqrt(8.0 * (double)t + 1.0);
  long i = (long)((d - 1.0) * 0.5);
  while (i > 0 && i * (i + 1) / 2 > t) --i;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  bi = i;
  bj = t - i * (i + 1) / 2;
}

union DbSmem {
  Stage128 st;
  float D[128][129];
};

template <bool VEC>
__device__ __forceinline__ void distance_tile(const float* __restrict__ X, long N, int n, long ld,
                                              const float* __restrict__ xnorm, float eps2, long r0, long c0,
                                              DbSmem& sm) {
  floatx16 acc[2][2];
  gemm_tile_128<VEC>(X, ld, N, r0, X, ld, N, c0, n, sm.st, acc);
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int cl = acc_col(nt);
    const long gc = c0 + cl;
    const float cn = gc < N ? xnorm[gc] : 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = acc_row(mt, r);
        const long gr = r0 + rl;
        const float rn = gr < N ? xnorm[gr] : 0.f;
        // a point is its own neighbour at every eps >= 0: the expanded form of D(i, i) is rounding noise
        const float d = gr == gc ? 0.f : fmaxf(fmaf(-2.f, acc[mt][nt][r], rn + cn), 0.f);
        sm.D[rl][cl] = (gr < N && gc < N && d <= eps2) ? d : __builtin_huge_valf();
      }
  }
  __syncthreads();
}

// id maps: id of slot s (valid where the slot's position is below N)
struct IdentityIds {
  long r0, c0;
  __device__ __forceinline__ long operator()(int s) const { return s < 128 ? r0 + s : c0 + (s - 128); }
};
struct LdsIds {
  const int* ids;  // 256 ids in LDS, written by thread s for slot s before the tile body runs
  __device__ __forceinline__ long operator()(int s) const { return ids[s]; }
};

template <bool VEC, class Ids>
__device__ __forceinline__ void degree_tile(const float* __restrict__ X, long N, int n, long ld,
                                            const float* __restrict__ xnorm, float eps2, long bi, long bj,
                                            const Ids& ids, int* __restrict__ counts, DbSmem& sm) {
  const int t = threadIdx.x;
  distance_tile<VEC>(X, N, n, ld, xnorm, eps2, bi * 128, bj * 128, sm);
  if (t < 128) {
    int cnt = 0;
    for (int c = 0; c < 128; ++c) cnt += sm.D[t][c] != __builtin_huge_valf();
    if (cnt) atomicAdd(&counts[ids(t)], cnt);
  } else if (bi != bj) {
    const int c = t - 128;
    int cnt = 0;
    for (int r = 0; r < 128; ++r) cnt += sm.D[r][c] != __builtin_huge_valf();
    if (cnt) atomicAdd(&counts[ids(t)], cnt);
  }
  __syncthreads();
}

// ---- union-find -------------------------------------------------------------------------------
__device__ __forceinline__ int uf_find(volatile int* p, int x) {
  int y = p[x];
  while (y != x) {
    const int z = p[y];
    if (z != y) p[x] = z;  // path halving; parents only ever point to smaller indices
    x = y;
    y = z;
  }
  return x;
}

__device__ __forceinline__ void uf_unite(int* p, int a, int b) {
  volatile int* vp = p;
  a = uf_find(vp, a);
  b = uf_find(vp, b);
  while (a != b) {
    if (a < b) {
      const int s = a;
      a = b;
      b = s;
    }
    const int old = atomicCAS(&p[a], a, b);  // hook the larger root under the smaller
    if (old == a) return;
    a = uf_find(vp, old);
    b = uf_find(vp, b);
  }
}

__device__ __forceinline__ unsigned long long nn_key(float d, long idx) {
  return ((unsigned long long)orderable(d) << 32) | (unsigned long long)(unsigned)idx;
}

struct LinkSmem {
  int lp[256];
  unsigned char lcore[256];
  unsigned long long cbest[128];
};

template <bool VEC, class Ids>
__device__ __forceinline__ void link_tile(const float* __restrict__ X, long N, int n, long ld,
                                          const float* __restrict__ xnorm, float eps2, long bi, long bj,
                                          const Ids& ids, const unsigned char* __restrict__ core,
                                          int* __restrict__ parent, unsigned long long* __restrict__ best,
                                          DbSmem& sm, LinkSmem& ls) {
  const int t = threadIdx.x;
  const long r0 = bi * 128, c0 = bj * 128;
  const long pos = t < 128 ? r0 + t : c0 + (t - 128);
  ls.lcore[t] = pos < N ? core[ids(t)] : 0;
  ls.lp[t] = (bi == bj && t >= 128) ? t - 128 : t;  // diagonal tile: column slot c is row slot c
  if (t < 128) ls.cbest[t] = ~0ull;
  distance_tile<VEC>(X, N, n, ld, xnorm, eps2, r0, c0, sm);  // ends with __syncthreads
  if (t < 128 && r0 + t < N) {
    const bool rc = ls.lcore[t];
    unsigned long long rb = ~0ull;
    for (int c = 0; c < 128; ++c) {
      const float d = sm.D[t][c];
      if (d == __builtin_huge_valf()) continue;
      const bool cc = ls.lcore[128 + c];
      if (rc && cc) {
        // local union in LDS (same CAS scheme on slot indices)
        volatile int* vp = ls.lp;
        int a = uf_find(vp, t), b = uf_find(vp, 128 + c);
        while (a != b) {
          if (a < b) {
            const int s = a;
            a = b;
            b = s;
          }
          const int old = atomicCAS(&ls.lp[a], a, b);
          if (old == a) break;
          a = uf_find(vp, old);
          b = uf_find(vp, b);
        }
      } else if (!rc && cc) {
        const unsigned long long key = nn_key(d, ids(128 + c));
        rb = key < rb ? key : rb;
      } else if (rc && !cc) {
        atomicMin(&ls.cbest[c], nn_key(d, ids(t)));
      }
    }
    if (rb != ~0ull) atomicMin(&best[ids(t)], rb);
  }
  __syncthreads();
  if (t < 128 && ls.cbest[t] != ~0ull) atomicMin(&best[ids(128 + t)], ls.cbest[t]);
  if (pos < N && ls.lcore[t]) {
    const int r = uf_find((volatile int*)ls.lp, t);
    if (r != t) {
      const long p2 = r < 128 ? r0 + r : c0 + (r - 128);
      if (p2 != pos) uf_unite(parent, (int)ids(t), (int)ids(r));
    }
  }
  __syncthreads();
}

inline bool vec_ok(const float* X, long ld, int n) {
  return ((ld & 3) == 0) && ((n & 3) == 0) && ((reinterpret_cast<uintptr_t>(X) & 15) == 0);
}

inline unsigned grid_for(long tiles) {
  long g = tiles < 8192 ? tiles : 8192;
  return (unsigned)(g < 1 ? 1 : g);
}
}  // namespace srml_dbscan
