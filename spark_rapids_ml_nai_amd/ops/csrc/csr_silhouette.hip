// Silhouette of a clustering (Spark's closed form) on CSR rows: the sparse sibling of silhouette.hip.
//
// Everything is taken about the global weighted mean mu without ever forming x - mu: with
// M_c = m_c - mu (fp32, stored transposed), g_c = mu . M_c and r_i = ||x_i - mu||^2,
//   squaredEuclidean: d(i, c) = r_i + t_c - 2 (sum_{j in nz(i)} x_ij M_cj - g_c),  t_c = Psi'_c / N_c
//   cosine:           d(i, c) = 1 - (sum_{j in nz(i)} x_ij m_cj) / ||x_i||          (mu = 0, t = g = 0)
// so the only work per non-zero is a sparse dot against the table. The CSR layout (int64 ABSOLUTE
// row offsets, int32 column indices in [0, n), validated by the caller), the table scheme of the
// kp > 64 kernel and the label-sums kernel are in csr_table.h, shared with csr_kmeans.hip.
//
//  * srml_csr_silhouette_rows_f32 — one wave per row: r_i = sum_nz (x - mu_j)^2 + (||mu||^2 - sum_nz
//    mu_j^2), or ||x_i||^2 without mu, lane-strided fp64 partials folded in a fixed order.
//  * srml_csr_silhouette_sums_f32 — Y[label][col] += f_i value (f_i = w_i, times 1 / ||x_i|| under
//    cosine): csr_table.h's label sums with the per-row factor.
//  * srml_csr_silhouette_f32 — the scoring kernel. One wave owns a row, CSR_ROWS waves a block. The
//    table is MT[n][kp] fp32, kp = k rounded up to 8, 16, 32 or a multiple of 64, padding zero and
//    t = +inf there (as for an empty cluster).
//    kp <= 64 (KP = kp): lane = (e, c), c = lane % KP, e = lane / KP. The wave keeps E = 64 / KP
//      non-zeros in flight: the KP lanes of group e read ONE (col, val) pair (same address) and the
//      KP consecutive floats of MT[col] (32 .. 256 B contiguous), one FMA per lane, CS_U such reads
//      outstanding per lane. After the row the E partial dots of a cluster are folded with log2(E)
//      xor steps at strides KP, 2 KP, ...: a fixed order.
//    kp > 64: tiles of CSR_TK clusters on the row staged in LDS, the table scheme of csr_table.h.
//    Epilogue in registers, fp64: lane c forms d_c and routes it by label == c into the own-cluster
//    value or the running minimum over the other non-empty clusters (across tiles); a butterfly
//    takes the minimum; N / (N - w), the singleton rule and the three-way formula give s (fp32).
//    w s goes to a fixed-order fp64 block slot, a second kernel adds the slots in block order: no
//    atomics, bit-identical run to run for given summaries.
#include "csr_table.h"

namespace {
constexpr int CS_U = 4;  // table reads in flight per lane (kp <= 64)

__global__ __launch_bounds__(CSR_T) void csr_sil_rows_kernel(const long* __restrict__ indptr,
                                                             const int* __restrict__ indices,
                                                             const float* __restrict__ data, long m,
                                                             const double* __restrict__ mu, double mu2,
                                                             double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * CSR_ROWS + (threadIdx.x >> 6);
  if (r >= m) return;  // wave-uniform
  const long p1 = indptr[r + 1];
  double a = 0.0, b = 0.0;
  for (long p = indptr[r] + lane; p < p1; p += 64) {
    const double v = (double)data[p];
    if (mu) {
      const double u = mu[indices[p]], d = v - u;
      a = fma(d, d, a);
      b = fma(u, u, b);
    } else {
      a = fma(v, v, a);
    }
  }
  a = wave_sum(a);
  if (mu) a += mu2 - wave_sum(b);  // the columns the row does not touch: ||mu||^2 less the touched ones
  if (lane == 0) out[r] = a;
}

// What the epilogue needs besides the dot: per cluster g, t (+inf: empty or padding) and N, per row
// r_i (cosine: ||x_i||^2), label and weight.
struct SilEpi {
  const double* g;
  const double* tc;
  const double* Nc;
  const double* rv;
  const int* labels;
  const double* w;
  int k;
  int cosine;
};

struct SilRow {
  double base, sc, alpha;
  int lab;
};

__device__ __forceinline__ SilRow sil_row(const SilEpi& ep, long row) {
  SilRow s;
  const double rv = ep.rv[row];
  s.base = ep.cosine ? 1.0 : rv;
  s.sc = ep.cosine ? (rv > 0.0 ? 1.0 / sqrt(rv) : 0.0) : 1.0;
  s.alpha = ep.cosine ? 1.0 : 2.0;
  s.lab = ep.labels[row];
  return s;
}

// d(i, j) from the fp32 dot, routed into the row's own-cluster value or its minimum over the others
__device__ __forceinline__ void sil_route(const SilEpi& ep, const SilRow& sr, float dot, int j, double& own,
                                          double& oth) {
  const double d = sr.base + (ep.tc[j] - sr.alpha * ((double)dot * sr.sc - ep.g[j]));
  if (j == sr.lab) own = d;
  else oth = fmin(oth, d);
}

// wave minimum of both values, then the row's s; returns w_i s_i (every lane)
__device__ __forceinline__ double sil_finish(const SilEpi& ep, const SilRow& sr, double own, double oth, long row,
                                             float* __restrict__ s_out) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    own = fmin(own, __shfl_xor(own, o, 64));
    oth = fmin(oth, __shfl_xor(oth, o, 64));
  }
  const double wi = ep.w ? ep.w[row] : 1.0;
  const double Nl = (unsigned)sr.lab < (unsigned)ep.k ? ep.Nc[sr.lab] : 0.0;
  float s = 0.f;
  if (wi > 0.0 && Nl > wi) {  // a weightless row and a row alone in its cluster score 0
    const double a = fmax(own, 0.0) * (Nl / (Nl - wi));
    const double b = fmax(oth, 0.0);
    if (a < b) s = (float)(1.0 - a / b);
    else if (a > b) s = (float)(b / a - 1.0);
  }
  if (s_out && (threadIdx.x & 63) == 0) s_out[row] = s;
  return wi * (double)s;
}

// the block's slot: its CSR_ROWS rows in wave order
__device__ __forceinline__ void sil_block_slot(double wsv, double* __restrict__ part) {
  __shared__ double ws_s[CSR_ROWS];
  if ((threadIdx.x & 63) == 0) ws_s[threadIdx.x >> 6] = wsv;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = ws_s[0];
#pragma unroll
    for (int i = 1; i < CSR_ROWS; ++i) t += ws_s[i];
    part[blockIdx.x] = t;
  }
}

template <int KP>
__global__ __launch_bounds__(CSR_T) void csr_sil_small_kernel(const long* __restrict__ indptr,
                                                              const int* __restrict__ indices,
                                                              const float* __restrict__ data, long m,
                                                              const float* __restrict__ MT, SilEpi ep,
                                                              float* __restrict__ s_out, double* __restrict__ part) {
  constexpr int E = 64 / KP;
  const int lane = threadIdx.x & 63;
  const int c = lane % KP, e = lane / KP;
  const long row = (long)blockIdx.x * CSR_ROWS + (threadIdx.x >> 6);
  const double inf = (double)__builtin_inff();
  double wsv = 0.0;
  if (row < m) {  // wave-uniform
    const long p0 = indptr[row], nnz = indptr[row + 1] - p0;
    const float* mt = MT + c;
    float acc = 0.f;
    for (long q = 0; q < nnz; q += E * CS_U) {
      float v[CS_U], t[CS_U];
#pragma unroll
      for (int u = 0; u < CS_U; ++u) {  // past the row's end: value 0 against table row 0
        const long p = q + u * E + e;
        const bool ok = p < nnz;
        const int col = ok ? indices[p0 + p] : 0;
        v[u] = ok ? data[p0 + p] : 0.f;
        t[u] = mt[(long)col * KP];
      }
#pragma unroll
      for (int u = 0; u < CS_U; ++u) acc = fmaf(v[u], t[u], acc);
    }
#pragma unroll
    for (int s = KP; s < 64; s <<= 1) acc += __shfl_xor(acc, s, 64);  // the E groups, fixed order
    const SilRow sr = sil_row(ep, row);
    double own = inf, oth = inf;
    sil_route(ep, sr, acc, c, own, oth);
    wsv = sil_finish(ep, sr, own, oth, row, s_out);
  }
  sil_block_slot(wsv, part);
}

__global__ __launch_bounds__(CSR_T) void csr_sil_wide_kernel(const long* __restrict__ indptr,
                                                             const int* __restrict__ indices,
                                                             const float* __restrict__ data, long m,
                                                             const float* __restrict__ MT, int kp, SilEpi ep,
                                                             float* __restrict__ s_out, double* __restrict__ part) {
  __shared__ int sI[CSR_ROWS][CSR_STAGE];
  __shared__ float sV[CSR_ROWS][CSR_STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * CSR_ROWS + wave;
  const double inf = (double)__builtin_inff();
  long p0 = 0, nnz = 0;
  if (row < m) {
    p0 = indptr[row];
    nnz = indptr[row + 1] - p0;
  }
  const int ns = nnz < CSR_STAGE ? (int)nnz : CSR_STAGE;
  for (int p = lane; p < ns; p += 64) {
    sI[wave][p] = indices[p0 + p];
    sV[wave][p] = data[p0 + p];
  }
  __syncthreads();  // every wave reaches this: rows past m have nnz = 0
  double wsv = 0.0;
  if (row < m) {
    const SilRow sr = sil_row(ep, row);
    double own = inf, oth = inf;
    for (int tile = 0; tile < kp; tile += CSR_TK) {
      float acc[CSR_KS];
#pragma unroll
      for (int s = 0; s < CSR_KS; ++s) acc[s] = 0.f;
      const float* ct = MT + tile + lane;
#pragma unroll 4
      for (int p = 0; p < ns; ++p) csr_accumulate<float>(ct + (long)sI[wave][p] * kp, sV[wave][p], tile, kp, acc);
      for (long p = CSR_STAGE; p < nnz; ++p)
        csr_accumulate<float>(ct + (long)indices[p0 + p] * kp, data[p0 + p], tile, kp, acc);
#pragma unroll
      for (int s = 0; s < CSR_KS; ++s)
        if (tile + 64 * s < kp) sil_route(ep, sr, acc[s], tile + 64 * s + lane, own, oth);
    }
    wsv = sil_finish(ep, sr, own, oth, row, s_out);
  }
  sil_block_slot(wsv, part);
}

// out[0] = sum of the block slots: thread t adds slots t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void csr_sil_fold_kernel(const double* __restrict__ part, long nb,
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

template <int KP>
void sil_small(unsigned blocks, const long* indptr, const int* indices, const float* data, long m, const float* MT,
               const SilEpi& ep, float* s_out, double* part, hipStream_t stream) {
  hipLaunchKernelGGL((csr_sil_small_kernel<KP>), dim3(blocks), dim3(CSR_T), 0, stream, indptr, indices, data, m, MT, ep,
                     s_out, part);
}
}  // namespace

// The dispatch constants of this file, for the Python layer and the tests: 0 clusters per tile
// (kp > 64), 1 staged non-zeros per row, 2 rows per block (csr_table.h's, as srml_csr_kmeans_config
// returns them), 3 table reads in flight per lane.
SRML_API int srml_csr_silhouette_config(int which) {
  switch (which) {
    case 0: return CSR_TK;
    case 1: return CSR_STAGE;
    case 2: return CSR_ROWS;
    case 3: return CS_U;
    default: return -1;
  }
}

// out[r] = ||x_r - mu||^2 (mu: n fp64, mu2 = ||mu||^2), or ||x_r||^2 when mu is null, for the m rows
// whose offsets start at indptr (m + 1 absolute offsets). -1: the grid overflows.
SRML_API int srml_csr_silhouette_rows_f32(const long* indptr, const int* indices, const float* data, long m,
                                          const double* mu, double mu2, double* out, hipStream_t stream) {
  if (m <= 0) return 0;
  const long blocks = csr_row_blocks(m);
  if (blocks < 0) return -1;
  hipLaunchKernelGGL(csr_sil_rows_kernel, dim3((unsigned)blocks), dim3(CSR_T), 0, stream, indptr, indices, data, m, mu,
                     mu2, out);
  return srml_status();
}

// sums (k x n, zeroed by the caller) += f_r x_r grouped by label (f null: 1); nnz picks the lanes per
// row. scale = 0: fp64 atomics. scale = 2^s: sums holds i64 integers of rint(f value 2^s) afterwards
// (srml_csr_cluster_sums_finish converts). Rows with a label outside [0, k) are skipped.
SRML_API int srml_csr_silhouette_sums_f32(const long* indptr, const int* indices, const float* data, long m, int n,
                                          long nnz, const int* labels, int k, const double* f, double scale,
                                          double* sums, hipStream_t stream) {
  return csr_label_sums<float>(indptr, indices, data, m, n, nnz, labels, k, f, scale, sums, stream);
}

// out[0] = sum_r w_r s_r over the m rows whose offsets start at indptr. MT: n x kp fp32; g, tc: kp
// fp64 (tc = +inf for an empty cluster and for the padding); Nc: k fp64; rv, labels, w (null: 1),
// s_out (null: not stored): m values; part: ceil(m / CSR_ROWS) fp64 block slots.
// -1: the grid overflows, -2: k, kp inconsistent.
SRML_API int srml_csr_silhouette_f32(const long* indptr, const int* indices, const float* data, long m, const float* MT,
                                     int k, int kp, const double* g, const double* tc, const double* Nc,
                                     const double* rv, const int* labels, const double* w, int cosine, float* s_out,
                                     double* part, double* out, hipStream_t stream) {
  if (m <= 0) return 0;
  if (k <= 0 || kp < k || !(kp == 8 || kp == 16 || kp == 32 || kp % 64 == 0)) return -2;
  const long nb = csr_row_blocks(m);
  if (nb < 0) return -1;
  const SilEpi ep{g, tc, Nc, rv, labels, w, k, cosine};
  const unsigned blocks = (unsigned)nb;
  switch (kp) {
    case 8: sil_small<8>(blocks, indptr, indices, data, m, MT, ep, s_out, part, stream); break;
    case 16: sil_small<16>(blocks, indptr, indices, data, m, MT, ep, s_out, part, stream); break;
    case 32: sil_small<32>(blocks, indptr, indices, data, m, MT, ep, s_out, part, stream); break;
    case 64: sil_small<64>(blocks, indptr, indices, data, m, MT, ep, s_out, part, stream); break;
    default:
      hipLaunchKernelGGL(csr_sil_wide_kernel, dim3(blocks), dim3(CSR_T), 0, stream, indptr, indices, data, m, MT, kp, ep,
                         s_out, part);
  }
  int st = srml_status();
  if (st) return st;
  hipLaunchKernelGGL(csr_sil_fold_kernel, dim3(1), dim3(256), 0, stream, part, nb, out);
  return srml_status();
}
