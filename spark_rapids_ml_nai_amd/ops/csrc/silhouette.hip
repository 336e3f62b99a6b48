// Silhouette of a clustering (Spark's closed form) on the 128 x 128 fp32 MFMA tile core.
//
// srml_silhouette_f32: for every row i and cluster c the tile computes v_i . m_c, with
//   v_i = (x_i - mu) * scale_i formed in the register-to-LDS store of the X tile (no centred or
//   normalised copy of X exists) and m_c the centred cluster means (k x n fp32). The epilogue forms
//   e(i, c) = t_c - alpha v_i . m_c and routes it by label[i] == c into the row's own-cluster slot
//   or its running minimum over the other non-empty clusters. ONE 256-thread workgroup owns a
//   128-row tile and walks all ceil(k / 128) column tiles itself, so both slots stay in registers
//   from the first column tile to the last and a row is finished inside its workgroup: no atomics,
//   the m x k matrix is never written, and the result is bit-identical run to run. After the last
//   column tile the 32 lanes that share a row and the two column waves are reduced, one thread per
//   row applies d = max(0, r_i + e), N / (N - w), the singleton rule and the three-way formula, and
//   a fixed-order fp64 sum of w_i s_i goes to the block's slot; a second kernel adds the slots in
//   block order.
//     squaredEuclidean: mu = global mean, scale = 1, r_i = ||v_i||^2, t_c = Psi'_c / N_c, alpha = 2
//     cosine:           mu = 0, scale_i = 1 / ||x_i||, r_i = 1, t_c = 0, alpha = 1
// srml_silhouette_sums_f32: per-cluster fp64 sums of w_i scale_i x_i over label-sorted segments, in
//   a fixed order (one block per cluster, 256-column chunk and split; the splits are folded in order).
// srml_silhouette_seg_scalars: per-cluster fp64 sum of w_i and of w_i r_i, fixed order.
#include "common.h"

#include "tile.h"

namespace {
using namespace srml_tile;

// The X operand of the silhouette tile: RowTile's branch-free loads, and a store that subtracts
// the column means and multiplies by the row's scale on the way into the padded LDS image.
template <bool VEC>
struct CentredTile {
  RowTile<128, VEC> t;
  float mu4[4];

  __device__ __forceinline__ void load(const float* __restrict__ X, long ldx, long m, int n, long row0, int k0,
                                       const float* __restrict__ mu) {
    t.load(X, ldx, m, n, row0, k0);
    const int c = k0 + (threadIdx.x & 7) * 4;  // the thread's four columns are the same for every p
#pragma unroll
    for (int q = 0; q < 4; ++q) mu4[q] = (mu && c + q < n) ? mu[c + q] : 0.f;
  }

  // sc[p]: scale of row (threadIdx.x >> 3) + 32 p of the tile
  __device__ __forceinline__ void store(float (*dst)[PADK], const float (&sc)[4]) const {
    const int rr = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        dst[rr + 32 * p][c4 + q] = ((t.okmask >> (4 * p + q)) & 1u) ? (t.v[p][q] - mu4[q]) * sc[p] : 0.f;
  }
};

template <bool VEC>
__global__ __launch_bounds__(256, 2) void silhouette_kernel(
    const float* __restrict__ X, long m, int n, long ldx, const float* __restrict__ mu,
    const float* __restrict__ scale, const float* __restrict__ rvec, const float* __restrict__ M, int k, long ldm,
    const float* __restrict__ tc, const double* __restrict__ Nc, const int* __restrict__ labels,
    const double* __restrict__ w, float alpha, float* __restrict__ s_out, double* __restrict__ part) {
  __shared__ Stage128 st;
  __shared__ int lab_s[128];
  __shared__ float red[2][2][128];  // [own | min other][column wave][row]
  __shared__ double ws_s[128];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int li = lane & 31, lk = lane >> 5;
  const long row0 = (long)blockIdx.x * 128;
  const float inf = __builtin_huge_valf();

  if (tid < 128) lab_s[tid] = row0 + tid < m ? labels[row0 + tid] : -1;
  float sc[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const long r = row0 + (tid >> 3) + 32 * p;
    sc[p] = (scale && r < m) ? scale[r] : 1.f;
  }
  float own[2][16], mn[2][16];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) own[a][r] = mn[a][r] = inf;

  floatx16 acc[2][2];
  const int nk = (n + BK - 1) / BK;
  const int nct = (k + 127) / 128;
  const long total = (long)nct * nk;
  CentredTile<VEC> xt;
  RowTile<128, VEC> ct;
  xt.load(X, ldx, m, n, row0, 0, mu);
  ct.load(M, ldm, k, n, 0, 0);
  xt.store(st.Xs[0], sc);
  ct.store(st.Cs[0]);
  __syncthreads();
  int cur = 0, kt = 0, cti = 0;
  for (long it = 0; it < total; ++it) {
    const bool more = it + 1 < total;
    const bool last_k = kt + 1 == nk;
    const int nkt = last_k ? 0 : kt + 1;
    const int ncti = last_k ? cti + 1 : cti;
    if (more) {  // the next (column tile, k step) loads stay in flight under this step's MFMAs
      xt.load(X, ldx, m, n, row0, nkt * BK, mu);
      ct.load(M, ldm, k, n, (long)ncti * 128, nkt * BK);
    }
    if (kt == 0) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    }
    const int colw = cti * 128 + wn * 64;
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      const int kx = 2 * kk + lk;
      float a[2], b[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) a[mt] = st.Xs[cur][wm * 64 + mt * 32 + li][kx];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) b[nt] = st.Cs[cur][wn * 64 + nt * 32 + li][kx];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          if (colw + nt * 32 < k)  // wave-uniform: a 32-column tile of padding is skipped
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
    }
    if (more) {
      xt.store(st.Xs[cur ^ 1], sc);
      ct.store(st.Cs[cur ^ 1]);
    }
    if (last_k) {  // epilogue of this column tile: registers and lab_s only
      int cj[2];
      bool ok[2];
      float tcv[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        cj[nt] = colw + nt * 32 + li;
        ok[nt] = cj[nt] < k && Nc[cj[nt] < k ? cj[nt] : 0] > 0.0;  // empty clusters never enter
        tcv[nt] = (ok[nt] && tc) ? tc[cj[nt]] : 0.f;
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int lab = lab_s[wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk];
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            const float e = fmaf(-alpha, acc[mt][nt][r], tcv[nt]);
            if (ok[nt]) {
              if (cj[nt] == lab) own[mt][r] = e;
              else mn[mt][r] = fminf(mn[mt][r], e);
            }
          }
        }
    }
    __syncthreads();
    cur ^= 1;
    kt = nkt;
    cti = ncti;
  }

  // the 32 lanes that share a row, then the two column waves through LDS
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float o = own[mt][r], b = mn[mt][r];
#pragma unroll
      for (int s = 1; s < 32; s <<= 1) {
        o = fminf(o, __shfl_xor(o, s, 64));
        b = fminf(b, __shfl_xor(b, s, 64));
      }
      if (li == 0) {
        const int row = wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        red[0][wn][row] = o;
        red[1][wn][row] = b;
      }
    }
  __syncthreads();
  if (tid < 128) {
    const long row = row0 + tid;
    double wsv = 0.0;
    if (row < m) {
      const int lab = lab_s[tid];
      const double wi = w ? w[row] : 1.0;
      const double Nl = (lab >= 0 && lab < k) ? Nc[lab] : 0.0;
      float s = 0.f;
      if (wi > 0.0 && Nl > wi) {  // a weightless row and a row alone in its cluster score 0
        const float ri = rvec ? rvec[row] : 1.f;
        const float d_own = fmaxf(ri + fminf(red[0][0][tid], red[0][1][tid]), 0.f);
        const float b = fmaxf(ri + fminf(red[1][0][tid], red[1][1][tid]), 0.f);
        const float a = d_own * (float)(Nl / (Nl - wi));
        if (a < b) s = 1.f - a / b;
        else if (a > b) s = b / a - 1.f;
      }
      if (s_out) s_out[row] = s;
      wsv = wi * (double)s;
    }
    ws_s[tid] = wsv;
  }
  __syncthreads();
#pragma unroll
  for (int s = 64; s > 0; s >>= 1) {  // fixed-order tree
    if (tid < s) ws_s[tid] += ws_s[tid + s];
    __syncthreads();
  }
  if (tid == 0) part[blockIdx.x] = ws_s[0];
}

// out[0] = sum of the block slots: thread t adds slots t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void silhouette_fold_kernel(const double* __restrict__ part, long nb,
                                                              double* __restrict__ out) {
  __shared__ double s_s[256];
  double a = 0.0;
  for (long i = threadIdx.x; i < nb; i += 256) a += part[i];
  s_s[threadIdx.x] = a;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) s_s[threadIdx.x] += s_s[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = s_s[0];
}

// ws[split][l][c] = sum over the split's rows of cluster l (label-sorted: perm, off) of f_i x_i[c],
// f_i = w_i scale_i, in fp64 and in row order
__global__ __launch_bounds__(256) void seg_wsums_kernel(const float* __restrict__ X, int n, long ld,
                                                        const int* __restrict__ perm, const long* __restrict__ off,
                                                        int k, const float* __restrict__ scale,
                                                        const double* __restrict__ w, double* __restrict__ ws) {
  const int l = blockIdx.x;
  const int c = blockIdx.y * 256 + threadIdx.x;
  const int sp = blockIdx.z, S = gridDim.z;
  if (c >= n) return;
  const long a = off[l], len = off[l + 1] - a;
  const long s0 = a + len * sp / S, s1 = a + len * (sp + 1) / S;
  constexpr int U = 4;
  double acc = 0.0;
  long i = s0;
  for (; i + U <= s1; i += U) {
    float v[U];
    double f[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long row = perm[i + u];
      v[u] = X[row * ld + c];
      f[u] = (w ? w[row] : 1.0) * (scale ? (double)scale[row] : 1.0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc += f[u] * (double)v[u];
  }
  for (; i < s1; ++i) {
    const long row = perm[i];
    acc += (w ? w[row] : 1.0) * (scale ? (double)scale[row] : 1.0) * (double)X[row * ld + c];
  }
  ws[((long)sp * k + l) * n + c] = acc;
}

__global__ __launch_bounds__(256) void seg_fold_kernel(const double* __restrict__ ws, int S, long kn,
                                                       double* __restrict__ sums) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= kn) return;
  double s = 0.0;
  for (int z = 0; z < S; ++z) s += ws[z * kn + i];
  sums[i] = s;
}

// Nout[l] = sum of w_i, Pout[l] = sum of w_i r_i over cluster l's segment: thread t takes rows
// t, t + 256, ... of the segment in order, then a fixed tree
__global__ __launch_bounds__(256) void seg_scalars_kernel(const int* __restrict__ perm, const long* __restrict__ off,
                                                          const double* __restrict__ w, const float* __restrict__ r,
                                                          double* __restrict__ Nout, double* __restrict__ Pout) {
  __shared__ double sn[256], sq[256];
  const int l = blockIdx.x;
  const long a = off[l], b = off[l + 1];
  double an = 0.0, ap = 0.0;
  for (long i = a + threadIdx.x; i < b; i += 256) {
    const long row = perm[i];
    const double wi = w ? w[row] : 1.0;
    an += wi;
    if (r) ap += wi * (double)r[row];
  }
  sn[threadIdx.x] = an;
  sq[threadIdx.x] = ap;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sn[threadIdx.x] += sn[threadIdx.x + s];
      sq[threadIdx.x] += sq[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (Nout) Nout[l] = sn[0];
    if (Pout) Pout[l] = sq[0];
  }
}

}  // namespace

// part: ceil(m / 128) fp64 block slots; out[0] = sum_i w_i s_i; s_out (m fp32) may be null, as may mu,
// scale (1), rvec (1), tc (0) and w (1). Labels are dense ids in [0, k); Nc[c] = 0 marks an empty id.
SRML_API int srml_silhouette_f32(const float* X, long m, int n, long ldx, const float* mu, const float* scale,
                                 const float* rvec, const float* M, int k, long ldm, const float* tc,
                                 const double* Nc, const int* labels, const double* w, float alpha, float* s_out,
                                 double* part, double* out, hipStream_t stream) {
  if (m <= 0 || k <= 0 || n <= 0) return 0;
  const long nb = (m + 127) / 128;
  if (nb > srml_max_blocks(256)) return -3;
  const bool vec = ((ldx & 3) == 0) && ((ldm & 3) == 0) && ((n & 3) == 0) &&
                   ((reinterpret_cast<uintptr_t>(X) & 15) == 0) && ((reinterpret_cast<uintptr_t>(M) & 15) == 0);
  if (vec)
    hipLaunchKernelGGL(silhouette_kernel<true>, dim3((unsigned)nb), dim3(256), 0, stream, X, m, n, ldx, mu, scale, rvec,
                       M, k, ldm, tc, Nc, labels, w, alpha, s_out, part);
  else
    hipLaunchKernelGGL(silhouette_kernel<false>, dim3((unsigned)nb), dim3(256), 0, stream, X, m, n, ldx, mu, scale,
                       rvec, M, k, ldm, tc, Nc, labels, w, alpha, s_out, part);
  int st = srml_status();
  if (st) return st;
  hipLaunchKernelGGL(silhouette_fold_kernel, dim3(1), dim3(256), 0, stream, part, nb, out);
  return srml_status();
}

// sums (k * n fp64, fully written); ws: splits * k * n fp64 (null / splits = 1: direct)
SRML_API int srml_silhouette_sums_f32(const float* X, long m, int n, long ld, const int* perm, const long* off, int k,
                                      const float* scale, const double* w, double* sums, int splits, double* ws,
                                      hipStream_t stream) {
  if (k <= 0 || n <= 0) return 0;
  (void)m;
  if (splits < 1 || !ws) { splits = 1; ws = sums; }
  dim3 grid((unsigned)k, ceil_div(n, 256), (unsigned)splits);
  hipLaunchKernelGGL(seg_wsums_kernel, grid, dim3(256), 0, stream, X, n, ld, perm, off, k, scale, w, ws);
  int st = srml_status();
  if (st || ws == sums) return st;
  const long kn = (long)k * n;
  hipLaunchKernelGGL(seg_fold_kernel, dim3(ceil_div(kn, 256)), dim3(256), 0, stream, ws, splits, kn, sums);
  return srml_status();
}

SRML_API int srml_silhouette_seg_scalars(const int* perm, const long* off, int k, const double* w, const float* r,
                                         double* Nout, double* Pout, hipStream_t stream) {
  if (k <= 0) return 0;
  hipLaunchKernelGGL(seg_scalars_kernel, dim3((unsigned)k), dim3(256), 0, stream, perm, off, w, r, Nout, Pout);
  return srml_status();
}
