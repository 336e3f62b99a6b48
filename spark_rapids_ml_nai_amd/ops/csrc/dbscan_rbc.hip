// DBSCAN algorithm="rbc": ball-cover pruning of the tile sweeps (models/dbscan.py orders the rows by
// nearest landmark, so a 128-row tile of the permuted matrix Xp is a compact ball).
//
//   srml_dbscan_tile_balls_f32: one workgroup per tile -> centre c_t (column means), an upper bound
//     r_t of max_i ||x_i - c_t|| and ||c_t||^2. Each element is read once: lane l of wave w keeps
//     column k0 + l of rows 4 p + w (p = 0..31) in registers, so a column sum is a per-lane sum and
//     LDS only carries the four waves' partials; the row sums of (x - c)^2 are per-lane partials
//     over the 64-column chunks, reduced across the wave once at the end.
//   srml_dbscan_tile_pairs: the T x n centre matrix through the same gemm_tile_128 core: a
//     workgroup holds 128 x 128 centre-to-centre distances, applies the keep rule (below) and
//     leaves the flags in LDS. Count pass: kept pairs per (tile a, column block); the caller scans
//     them; fill pass: recompute, write the tri_decode index a (a + 1) / 2 + b at offset + rank in
//     the row. Rows ascend, column blocks ascend within a row, columns within a block: the list is
//     ascending and the same on every run; no T x T array is ever in global memory.
//   srml_dbscan_degree_list_f32 / srml_dbscan_link_list_f32: the sweeps of dbscan.hip over the
//     listed tile pairs only. Distances are taken at permuted positions, results written at
//     original ids (perm[position], 256 of them in LDS per tile pair): dbscan_tile.h.
#include "dbscan_tile.h"

namespace {
using namespace srml_dbscan;

constexpr float U24 = 5.9604644775390625e-8f;  // 2^-24
constexpr int KC = 64;                         // columns per chunk of the ball kernel: one per lane

__global__ __launch_bounds__(256) void tile_balls_kernel(const float* __restrict__ X, long N, int n, long ld,
                                                         long T, float* __restrict__ centres,
                                                         float* __restrict__ radii, float* __restrict__ cnorm) {
  __shared__ float part[2][4][KC];
  __shared__ float wmax[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (long tile = blockIdx.x; tile < T; tile += gridDim.x) {
    const long r0 = tile * 128;
    const int rows = (int)(N - r0 < 128 ? N - r0 : 128);  // >= 1
    const float frows = (float)rows;
    float acc[32];
#pragma unroll
    for (int p = 0; p < 32; ++p) acc[p] = 0.f;
    float c2 = 0.f;
    int buf = 0;
    for (int k0 = 0; k0 < n; k0 += KC, buf ^= 1) {
      const int col = k0 + lane;
      const bool okc = col < n;
      float v[32];
      float s = 0.f;
#pragma unroll
      for (int p = 0; p < 32; ++p) {
        const int row = 4 * p + wid;
        const bool ok = okc && row < rows;
        const float x = X[(ok ? r0 + row : r0) * ld + (okc ? col : 0)];
        v[p] = ok ? x : 0.f;
        s += v[p];
      }
      part[buf][wid][lane] = s;
      __syncthreads();  // the other buffer is rewritten only after every wave has passed this barrier again
      // the same four terms in the same order in every wave: one centre for the whole workgroup
      const float c = (((part[buf][0][lane] + part[buf][1][lane]) + part[buf][2][lane]) + part[buf][3][lane]) / frows;
      if (wid == 0 && okc) {
        centres[tile * (long)n + col] = c;
        c2 = fmaf(c, c, c2);
      }
#pragma unroll
      for (int p = 0; p < 32; ++p) {
        const float d = v[p] - c;  // an invalid column has v = c = 0; invalid rows are dropped below
        acc[p] = fmaf(d, d, acc[p]);
      }
    }
    float m = 0.f;
#pragma unroll
    for (int p = 0; p < 32; ++p) {
      const float s = wave_sum(acc[p]);
      if (4 * p + wid < rows) m = fmaxf(m, s);
    }
    if (wid == 0) c2 = wave_sum(c2);
    if (lane == 0) wmax[wid] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float mm = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
      // Upper bound: the fp32 sum of n squared differences is low by at most (n + 2) u relative (one
      // rounding per difference, one per fused term), its root by half that plus the root's own u:
      // (n / 2 + 2) u. The factor (n + 4) u covers it twice over, the product's rounding included.
      radii[tile] = sqrtf(mm) * (1.f + (float)(n + 4) * U24);
      cnorm[tile] = c2;
    }
    __syncthreads();
  }
}

// Keep rule. The brute sweep counts a pair (i, j) when its *computed* distance is <= eps2, and that
// differs from the exact squared distance D_ij of the rows it runs on by at most
// c(n) u (||x_i|| + ||x_j||)^2 <= band = c(n) u (2 R)^2, c(n) = 3 n / 2 + 8, R = max_i ||x_i||
// (docs/coverage.md, the bound of distance_tile). So a counted pair has D_ij <= eps2 + band. With
// x_i in the ball (c_a, r_a) and x_j in (c_b, r_b) the triangle inequality gives
//   ||c_a - c_b|| <= r_a + r_b + ||x_i - x_j|| <= r_a + r_b + sqrt(eps2 + band).
// The centre distance itself comes from the same expanded form, d2 = ||c_a||^2 + ||c_b||^2 - 2 c_a.c_b in
// fp32, off by at most e_ab = (3 n / 2 + 5) u (||c_a|| + ||c_b||)^2. Hence a tile pair that holds any pair
// the brute sweep could count satisfies
//   d2_ab - e_ab <= (r_a + r_b + sqrt(eps2 + band))^2,
// and every tile pair that fails it can be skipped without changing a count, an edge or a key. Both
// sides are evaluated in fp64 from the fp32 inputs; thr = sqrt(eps2 + band) comes from the host.
// The diagonal is always kept. A zero row under cosine sits in its ball as the zero vector while
// the sweep holds it at distance 2 >= its geometric 1 from a unit row: the bound stays a lower bound.
template <bool VEC, bool FILL>
__global__ __launch_bounds__(256, 2) void tile_pairs_kernel(const float* __restrict__ C, long T, int n, long ld,
                                                            const float* __restrict__ radii,
                                                            const float* __restrict__ cnorm, double thr,
                                                            double ecoef, long TB, long nblk,
                                                            int* __restrict__ counts,
                                                            const long long* __restrict__ offs,
                                                            long long* __restrict__ out) {
  __shared__ DbSmem sm;
  const int t = threadIdx.x;
  for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    long Bi, Bj;
    tri_decode(blk, Bi, Bj);
    const long a0 = Bi * 128, b0 = Bj * 128;
    floatx16 acc[2][2];
    gemm_tile_128<VEC>(C, ld, T, a0, C, ld, T, b0, n, sm.st, acc);  // ends with __syncthreads
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int cl = acc_col(nt);
      const long b = b0 + cl;
      const float cnb = b < T ? cnorm[b] : 0.f;
      const double rb = b < T ? (double)radii[b] : 0.0;
      const double sb = sqrt((double)cnb);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rl = acc_row(mt, r);
          const long a = a0 + rl;
          const float cna = a < T ? cnorm[a] : 0.f;
          const double ra = a < T ? (double)radii[a] : 0.0;
          const double sc = sqrt((double)cna) + sb;
          const double d2 = (double)fmaf(-2.f, acc[mt][nt][r], cna + cnb) - ecoef * sc * sc;
          const double reach = ra + rb + thr;
          const bool keep = a < T && b <= a && (a == b || d2 <= reach * reach);
          sm.D[rl][cl] = keep ? 1.f : 0.f;
        }
    }
    __syncthreads();
    const long a = a0 + t;
    if (t < 128 && a < T) {
      if (FILL) {
        long long o = offs[a * TB + Bj];
        const long long base = (long long)a * (a + 1) / 2 + b0;
        for (int c = 0; c < 128; ++c)
          if (sm.D[t][c] != 0.f) out[o++] = base + c;
      } else {
        int cnt = 0;
        for (int c = 0; c < 128; ++c) cnt += sm.D[t][c] != 0.f;
        counts[a * TB + Bj] = cnt;
      }
    }
    __syncthreads();
  }
}

// id of this thread's slot of a tile pair (the host entry points' callers check the map and the list)
__device__ __forceinline__ int slot_id(const int* __restrict__ perm, long N, long bi, long bj) {
  const int t = threadIdx.x;
  const long pos = t < 128 ? bi * 128 + t : bj * 128 + (t - 128);
  return pos < N ? perm[pos] : 0;
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void dbscan_degree_list_kernel(const float* __restrict__ X, long N, int n, long ld,
                                                                    const float* __restrict__ xnorm, float eps2,
                                                                    const long long* __restrict__ pairs, long l0,
                                                                    long l1, const int* __restrict__ perm,
                                                                    int* __restrict__ counts) {
  __shared__ DbSmem sm;
  __shared__ int sid[256];
  for (long l = l0 + blockIdx.x; l < l1; l += gridDim.x) {
    long bi, bj;
    tri_decode(pairs[l], bi, bj);
    sid[threadIdx.x] = slot_id(perm, N, bi, bj);  // read back by this thread only: no barrier needed
    degree_tile<VEC>(X, N, n, ld, xnorm, eps2, bi, bj, LdsIds{sid}, counts, sm);
  }
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void dbscan_link_list_kernel(const float* __restrict__ X, long N, int n, long ld,
                                                                  const float* __restrict__ xnorm, float eps2,
                                                                  const long long* __restrict__ pairs, long l0, long l1,
                                                                  const int* __restrict__ perm,
                                                                  const unsigned char* __restrict__ core,
                                                                  int* __restrict__ parent,
                                                                  unsigned long long* __restrict__ best) {
  __shared__ DbSmem sm;
  __shared__ LinkSmem ls;
  __shared__ int sid[256];
  for (long l = l0 + blockIdx.x; l < l1; l += gridDim.x) {
    long bi, bj;
    tri_decode(pairs[l], bi, bj);
    // slot s is written by thread s; other threads' slots are read after the barriers of the distance tile
    sid[threadIdx.x] = slot_id(perm, N, bi, bj);
    link_tile<VEC>(X, N, n, ld, xnorm, eps2, bi, bj, LdsIds{sid}, core, parent, best, sm, ls);
  }
}

inline long tri_count(long T) { return T * (T + 1) / 2; }
}  // namespace

// centres (T x n, dense), radii (T), cnorm (T) of the T = ceil(N / 128) row tiles of X
SRML_API int srml_dbscan_tile_balls_f32(const float* X, long N, int n, long ld, float* centres, float* radii,
                                        float* cnorm, hipStream_t stream) {
  if (N <= 0 || n <= 0) return 0;
  const long T = (N + 127) / 128;
  hipLaunchKernelGGL(tile_balls_kernel, dim3(grid_for(T)), dim3(256), 0, stream, X, N, n, ld, T, centres, radii,
                     cnorm);
  return srml_status();
}

// fill == 0: counts[a * TB + Bj] (TB = ceil(T / 128), zeroed by the caller) = kept pairs of tile a in
// column block Bj. fill != 0: offs = their exclusive scan; out receives the ascending list.
SRML_API int srml_dbscan_tile_pairs(const float* C, long T, int n, long ld, const float* radii, const float* cnorm,
                                    double thr, int* counts, const long long* offs, long long* out, int fill,
                                    hipStream_t stream) {
  if (T <= 0) return 0;
  const long TB = (T + 127) / 128, nblk = tri_count(TB);
  const double ecoef = (1.5 * n + 5.0) * (double)U24;
  const dim3 g(grid_for(nblk)), b(256);
  const bool vec = vec_ok(C, ld, n);
  if (fill) {
    if (vec)
      hipLaunchKernelGGL((tile_pairs_kernel<true, true>), g, b, 0, stream, C, T, n, ld, radii, cnorm, thr, ecoef, TB,
                         nblk, counts, offs, out);
    else
      hipLaunchKernelGGL((tile_pairs_kernel<false, true>), g, b, 0, stream, C, T, n, ld, radii, cnorm, thr, ecoef, TB,
                         nblk, counts, offs, out);
  } else {
    if (vec)
      hipLaunchKernelGGL((tile_pairs_kernel<true, false>), g, b, 0, stream, C, T, n, ld, radii, cnorm, thr, ecoef, TB,
                         nblk, counts, offs, out);
    else
      hipLaunchKernelGGL((tile_pairs_kernel<false, false>), g, b, 0, stream, C, T, n, ld, radii, cnorm, thr, ecoef, TB,
                         nblk, counts, offs, out);
  }
  return srml_status();
}

SRML_API int srml_dbscan_degree_list_f32(const float* X, long N, int n, long ld, const float* xnorm, float eps2,
                                         const long long* pairs, long l0, long l1, const int* perm, int* counts,
                                         hipStream_t stream) {
  if (N <= 0 || l1 <= l0) return 0;
  if (N > 0x7fffffffL) return -3;
  if (vec_ok(X, ld, n))
    hipLaunchKernelGGL(dbscan_degree_list_kernel<true>, dim3(grid_for(l1 - l0)), dim3(256), 0, stream, X, N, n, ld,
                       xnorm, eps2, pairs, l0, l1, perm, counts);
  else
    hipLaunchKernelGGL(dbscan_degree_list_kernel<false>, dim3(grid_for(l1 - l0)), dim3(256), 0, stream, X, N, n, ld,
                       xnorm, eps2, pairs, l0, l1, perm, counts);
  return srml_status();
}

SRML_API int srml_dbscan_link_list_f32(const float* X, long N, int n, long ld, const float* xnorm, float eps2,
                                       const long long* pairs, long l0, long l1, const int* perm,
                                       const unsigned char* core, int* parent, unsigned long long* best,
                                       hipStream_t stream) {
  if (N <= 0 || l1 <= l0) return 0;
  if (N > 0x7fffffffL) return -3;
  if (vec_ok(X, ld, n))
    hipLaunchKernelGGL(dbscan_link_list_kernel<true>, dim3(grid_for(l1 - l0)), dim3(256), 0, stream, X, N, n, ld, xnorm,
                       eps2, pairs, l0, l1, perm, core, parent, best);
  else
    hipLaunchKernelGGL(dbscan_link_list_kernel<false>, dim3(grid_for(l1 - l0)), dim3(256), 0, stream, X, N, n, ld,
                       xnorm, eps2, pairs, l0, l1, perm, core, parent, best);
  return srml_status();
}
