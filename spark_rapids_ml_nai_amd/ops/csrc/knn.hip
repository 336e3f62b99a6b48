// ------------------------------------------------------------------------------------------
// Exact k-nearest-neighbours: fused MFMA distance tiles + per-query top-k in LDS.
// Block = 128 queries x one slice of the item range; the query tile's top-k list lives in LDS
// for the whole item sweep, so the q x items distance matrix is never materialised (reference:
// cuML NearestNeighborsMG brute force, knn.py:638-749). After each 128x128 MFMA tile the
// partial distances (||i||^2 - 2 q.i) go through the (reused) staging LDS and 128 threads each
// merge one query row with a threshold test + insertion into a sorted list (most candidates are
// rejected by the threshold after the first tiles). Item-range slices (grid.y) keep >= 512
// blocks in flight for small query sets; slices are merged by the caller.
// ------------------------------------------------------------------------------------------
#include "common.h"

#include "neighbors.h"

namespace {
using namespace srml_nn;

template <bool VEC>
__global__ __launch_bounds__(256, 1) void knn_kernel(const float* __restrict__ Q, long mq, int n, long ldq,
                                                     const float* __restrict__ I, long mi, long ldi,
                                                     const float* __restrict__ inorm, int k, long items_per_slice,
                                                     float* __restrict__ out_d, long long* __restrict__ out_i,
                                                     long long id_offset) {
  constexpr int BM = 128, BN = 128, MT = 2, NT = 2;
  union Smem {
    struct {
      float Xs[2][BM][PADK];
      float Cs[2][BN][PADK];
    } st;
    float D[BM][BN + 1];
  };
  __shared__ Smem sm;
  // +1 pad: thread t walks row t, so an unpadded 64-word stride would put every thread on one bank
  __shared__ float topd[BM][NN_KMAX + 1];
  __shared__ int topi[BM][NN_KMAX + 1];
  const long q0 = (long)blockIdx.x * BM;
  const long slice = blockIdx.y;
  const long ibeg = slice * items_per_slice;
  const long iend = min(mi, ibeg + items_per_slice);
  const int t = threadIdx.x;
  const int lane = t & 63, wid = t >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int li = lane & 31, lk = lane >> 5;
  for (int i = t; i < BM * (NN_KMAX + 1); i += 256) {
    (&topd[0][0])[i] = __builtin_huge_valf();
    (&topi[0][0])[i] = -1;
  }
  const int nk = (n + BK - 1) / BK;
  for (long c0 = ibeg; c0 < iend; c0 += BN) {
    floatx16 acc[MT][NT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
      for (int b = 0; b < NT; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    RowTile<BM, VEC> xt;
    RowTile<BN, VEC> ct;
    xt.load(Q, ldq, mq, n, q0, 0);
    ct.load(I, ldi, iend, n, c0, 0);
    __syncthreads();  // previous tile's top-k scan has finished with sm.D
    xt.store(sm.st.Xs[0]);
    ct.store(sm.st.Cs[0]);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
      const bool more = kt + 1 < nk;
      if (more) {
        xt.load(Q, ldq, mq, n, q0, (kt + 1) * BK);
        ct.load(I, ldi, iend, n, c0, (kt + 1) * BK);
      }
#pragma unroll
      for (int kk = 0; kk < BK / 2; ++kk) {
        const int kx = 2 * kk + lk;
        float a[MT], b[NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = sm.st.Xs[cur][wm * MT * 32 + mt * 32 + li][kx];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b[nt] = sm.st.Cs[cur][wn * NT * 32 + nt * 32 + li][kx];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
      }
      if (more) {
        xt.store(sm.st.Xs[cur ^ 1]);
        ct.store(sm.st.Cs[cur ^ 1]);
      }
      __syncthreads();
      cur ^= 1;
    }
    // partial distances -> LDS tile (staging buffers are dead now)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int cl = wn * NT * 32 + nt * 32 + li;
      const long cg = c0 + cl;
      const float in = cg < iend ? inorm[cg] : 0.f;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rl = wm * MT * 32 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
          sm.D[rl][cl] = cg < iend ? fmaf(-2.f, acc[mt][nt][r], in) : __builtin_huge_valf();
        }
    }
    __syncthreads();
    if (t < BM) {
      float thr = topd[t][k - 1];
      const int ncol = (int)min((long)BN, iend - c0);
      for (int c = 0; c < ncol; ++c) {
        const float d = sm.D[t][c];
        if (d < thr) {
          int p = k - 1;
          while (p > 0 && topd[t][p - 1] > d) {
            topd[t][p] = topd[t][p - 1];
            topi[t][p] = topi[t][p - 1];
            --p;
          }
          topd[t][p] = d;
          topi[t][p] = (int)(c0 + c - ibeg);
          thr = topd[t][k - 1];
        }
      }
    }
  }
  __syncthreads();
  if (t < BM && q0 + t < mq) {
    const long base = ((q0 + t) * gridDim.y + slice) * (long)k;
    for (int j = 0; j < k; ++j) {
      out_d[base + j] = topd[t][j];
      out_i[base + j] = topi[t][j] >= 0 ? (long long)topi[t][j] + ibeg + id_offset : -1;
    }
  }
}

}  // namespace

// out_d / out_i: (mq, slices, k) partial top-k (distance WITHOUT the ||q||^2 term)
SRML_API int srml_knn_f32(const float* Q, long mq, int n, long ldq, const float* I, long mi, long ldi,
                          const float* inorm, int k, int slices, float* out_d, long long* out_i, long long id_offset,
                          hipStream_t stream) {
  if (mq <= 0) return 0;
  if (k < 1 || k > NN_KMAX) return -8;
  const bool vec = ((ldq & 3) == 0) && ((ldi & 3) == 0) && ((n & 3) == 0) &&
                   ((reinterpret_cast<uintptr_t>(Q) & 15) == 0) && ((reinterpret_cast<uintptr_t>(I) & 15) == 0);
  if (slices < 1) slices = 1;
  long per = (mi + slices - 1) / slices;
  per = ((per + 127) / 128) * 128;
  if (per < 128) per = 128;
  dim3 grid(ceil_div(mq, 128), (unsigned)slices);
  if (vec)
    hipLaunchKernelGGL(knn_kernel<true>, grid, dim3(256), 0, stream, Q, mq, n, ldq, I, mi, ldi, inorm, k, per, out_d,
                       out_i, id_offset);
  else
    hipLaunchKernelGGL(knn_kernel<false>, grid, dim3(256), 0, stream, Q, mq, n, ldq, I, mi, ldi, inorm, k, per,
                       out_d, out_i, id_offset);
  return srml_status();
}
