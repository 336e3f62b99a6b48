// IVF-PQ: product-quantised inverted lists (cuVS / FAISS "IVF-PQ"; beyond the reference version,
// whose docstring announces it, knn.py:895-914).
//
// An item is stored as M one-byte codes: code m names one of ksub codewords of dsub = n / M
// dimensions that approximates sub-vector m of the item's residual to its list centre. The scan
// of one (query, list) pair first builds an fp32 lookup table LUT[m][j] in LDS
//   L2:            LUT[m][j] = ||(q - c_l)_m - cb[m][j]||^2        key = sum_m LUT[m][code_m]
//   inner product: LUT[m][j] = q_m . cb[m][j]  (list-independent)  key = -(q . c_l + sum_m ...)
// and then streams the list's code rows: one item per lane, M data-dependent LDS lookups each.
// Codebooks arrive transposed, cbT[m][d][j], so that the table build reads them coalesced over j.
// Code rows are row-major u8 [N, M] in list order; with M % 4 == 0 a lane fetches four codes per
// 32-bit load. The table lookups hit random banks: a 32-lane ds_read_b32 group with uniformly
// random codes sees about 3.5 distinct addresses on its busiest bank.
#include "common.h"

#include "neighbors.h"

namespace {
using namespace srml_nn;
constexpr int PQ_T = 256;
constexpr int PQ_MMAX = 128;
constexpr int PQ_KSUBMAX = 256;
// static LDS of the search kernel: 4 wave lists of (fp32 key, int64 position)
constexpr size_t PQ_STATIC_LDS = sizeof(WaveD) + sizeof(WaveI);
constexpr size_t PQ_LDS_TOTAL = 160 * 1024;  // per CU on gfx950; one workgroup may take all of it

// The one place the dynamic LDS bytes of both scan kernels are computed: table | query residual.
inline size_t pq_lds_bytes(int n, int M, int ksub) {
  return ((size_t)M * ksub + (size_t)((n + 3) / 4) * 4) * sizeof(float);
}

inline bool pq_shape_ok(int n, int M, int ksub) {
  return n >= 1 && M >= 1 && M <= PQ_MMAX && n % M == 0 && ksub >= 1 && ksub <= PQ_KSUBMAX;
}

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

// q . c over the wave (every wave of the block gets the same value: same order of additions)
__device__ __forceinline__ float pq_wave_dot(const float* qs, const float* __restrict__ c, int n) {
  float a = 0.f;
  for (int d = threadIdx.x & 63; d < n; d += 64) a = fmaf(qs[d], c[d], a);
  return wave_sum(a);
}

// One block per query, as ivf_search_kernel: the probed lists are swept by the 4 waves, 64 items
// per wave step, and a wave-private sorted list in LDS takes what beats its threshold.
__global__ __launch_bounds__(PQ_T) void ivfpq_search_kernel(const float* __restrict__ Q, int n, long ldq,
                                                            const int* __restrict__ probes, int nprobe,
                                                            const long long* __restrict__ list_off, int nlist, long N,
                                                            const float* __restrict__ C,
                                                            const float* __restrict__ cbT,
                                                            const unsigned char* __restrict__ codes, int M, int ksub,
                                                            int ip, int vec, int k, float* __restrict__ out_d,
                                                            long long* __restrict__ out_i) {
  extern __shared__ __attribute__((aligned(16))) float pq_s[];  // lut [M * ksub] | qr [n]
  __shared__ WaveD wd;
  __shared__ WaveI wi;
  float* lut = pq_s;
  float* qr = pq_s + M * ksub;
  const long q = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int dsub = n / M;
  wave_lists_init(wd, wi);
  float thr = __builtin_huge_valf();
  bool have_lut = false;
  for (int p = 0; p < nprobe; ++p) {  // everything that steers this loop is block-uniform
    const int l = probes[q * nprobe + p];
    if (l < 0 || l >= nlist) continue;
    const long s = list_off[l], e = min((long)list_off[l + 1], N);
    if (s < 0 || e <= s) continue;
    const float* c = C + (long)l * n;
    float bias = 0.f;
    if (!ip || !have_lut) {
      __syncthreads();  // the previous list's scan is done with lut / qr
      for (int d = t; d < n; d += PQ_T) qr[d] = ip ? Q[q * ldq + d] : Q[q * ldq + d] - c[d];
      __syncthreads();
      pq_build_lut(qr, cbT, M, ksub, dsub, ip, lut);
      __syncthreads();
      have_lut = true;
    }
    if (ip) bias = pq_wave_dot(qr, c, n);
    for (long j0 = s + (long)wid * 64; j0 < e; j0 += 4 * 64) {
      const long j = j0 + lane;
      float key = __builtin_huge_valf();
      if (j < e) {
        const float a = pq_item_sum(codes + j * M, lut, M, ksub, vec != 0);
        key = ip ? -(bias + a) : a;
      }
      unsigned long long mask = __ballot(key < thr);
      while (mask) {  // wave-uniform
        const int g = __builtin_amdgcn_readfirstlane(__builtin_ctzll(mask));
        mask &= mask - 1;
        const float dg = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(key), g));
        if (dg < thr) wave_list_offer(wd, wi, k, dg, j0 + g, thr);
      }
    }
  }
  __syncthreads();
  if (t == 0) wave_lists_merge_write(wd, wi, k, out_d + q * k, out_i + q * k);
}

// One block per (query, probe), as ivf_candidates_kernel: the list's keys and positions go into
// the query's candidate row at the prefix offset of its earlier probes.
__global__ __launch_bounds__(PQ_T) void ivfpq_candidates_kernel(const float* __restrict__ Q, long q0, int n, long ldq,
                                                                const int* __restrict__ probes, int nprobe,
                                                                const long long* __restrict__ list_off, int nlist,
                                                                long N, const float* __restrict__ C,
                                                                const float* __restrict__ cbT,
                                                                const unsigned char* __restrict__ codes, int M,
                                                                int ksub, int ip, int vec, float* __restrict__ D,
                                                                long long* __restrict__ DI, long ldd) {
  extern __shared__ __attribute__((aligned(16))) float pq_s[];  // lut [M * ksub] | qr [n]
  float* lut = pq_s;
  float* qr = pq_s + M * ksub;
  const long qi = q0 + blockIdx.x;
  const int p = blockIdx.y;
  const int* pr = probes + qi * nprobe;
  const int l = pr[p];
  if (l < 0 || l >= nlist) return;
  const long b0 = list_off[l], b1 = min((long)list_off[l + 1], N);
  if (b0 < 0 || b1 <= b0) return;
  long off = 0;  // as srml_ivf_candidate_max counts: every non-negative earlier probe
  for (int j = 0; j < p; ++j)
    if (pr[j] >= 0 && pr[j] < nlist) off += list_off[pr[j] + 1] - list_off[pr[j]];
  if (off < 0 || off + (b1 - b0) > ldd) return;
  const float* c = C + (long)l * n;
  for (int d = threadIdx.x; d < n; d += PQ_T) qr[d] = ip ? Q[qi * ldq + d] : Q[qi * ldq + d] - c[d];
  __syncthreads();
  pq_build_lut(qr, cbT, M, ksub, n / M, ip, lut);
  __syncthreads();
  const float bias = ip ? pq_wave_dot(qr, c, n) : 0.f;
  float* drow = D + (long)blockIdx.x * ldd + off;
  long long* irow = DI + (long)blockIdx.x * ldd + off;
  for (long j = b0 + threadIdx.x; j < b1; j += PQ_T) {
    const float a = pq_item_sum(codes + j * M, lut, M, ksub, vec != 0);
    drow[j - b0] = ip ? -(bias + a) : a;
    irow[j - b0] = j;
  }
}

// One wave per row: the row's residual sits in LDS, lanes split the codewords of one sub-space
// (coalesced reads of cbT), and a wave arg-min (ties -> lower codeword) gives the code.
__global__ __launch_bounds__(PQ_T) void pq_encode_kernel(const float* __restrict__ X, long N, int n, long ldx,
                                                         const int* __restrict__ labels, int nlist,
                                                         const float* __restrict__ C, const float* __restrict__ cbT,
                                                         int M, int ksub, unsigned char* __restrict__ codes) {
  extern __shared__ __attribute__((aligned(16))) float pe_s[];  // 4 rows x n
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wid;
  float* r = pe_s + (long)wid * n;
  if (row < N) {
    const float* c = nullptr;
    if (labels) {
      const int l = labels[row];
      if (l >= 0 && l < nlist) c = C + (long)l * n;
    }
    for (int d = lane; d < n; d += 64) r[d] = c ? X[row * ldx + d] - c[d] : X[row * ldx + d];
  }
  __syncthreads();
  if (row >= N) return;
  const int dsub = n / M;
  for (int m = 0; m < M; ++m) {
    const float* rm = r + m * dsub;
    const float* cm = cbT + (long)m * dsub * ksub;
    float best = __builtin_huge_valf();
    int bj = 0;
    for (int j = lane; j < ksub; j += 64) {
      float acc = 0.f;
      for (int d = 0; d < dsub; ++d) {
        const float diff = rm[d] - cm[(long)d * ksub + j];
        acc = fmaf(diff, diff, acc);
      }
      if (acc < best) { best = acc; bj = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oj = __shfl_xor(bj, o, 64);
      if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
    }
    if (lane == 0) codes[row * M + m] = (unsigned char)bj;
  }
}
}  // namespace

// Status -9: the lookup table does not fit the LDS (or the shape is outside the kernel's limits).

// codes[r][m] = arg-min_j ||(x_r - C[labels[r]])_m - cb[m][j]||^2 (labels == NULL: x_r itself).
SRML_API int srml_pq_encode_f32(const float* X, long N, int n, long ldx, const int* labels, int nlist, const float* C,
                                const float* cbT, int M, int ksub, unsigned char* codes, hipStream_t stream) {
  if (N <= 0) return 0;
  if (!pq_shape_ok(n, M, ksub) || ldx < n) return -9;
  const size_t lds = (size_t)4 * n * sizeof(float);
  if (lds > 64 * 1024) return -9;
  const long blocks = (N + 3) / 4;
  if (blocks > srml_max_blocks(PQ_T)) return -1;
  hipLaunchKernelGGL(pq_encode_kernel, dim3((unsigned)blocks), dim3(PQ_T), lds, stream, X, N, n, ldx, labels, nlist, C,
                     cbT, M, ksub, codes);
  return srml_status();
}

// Ascending keys and list-order positions of the k best items of each query's probed lists
// (k <= 64; empty slots +inf / -1).
SRML_API int srml_ivfpq_search_f32(const float* Q, long nq, int n, long ldq, const int* probes, int nprobe,
                                   const long long* list_off, int nlist, long N, const float* C, const float* cbT,
                                   const unsigned char* codes, int M, int ksub, int ip, int k, float* out_d,
                                   long long* out_i, hipStream_t stream) {
  if (nq <= 0) return 0;
  if (k < 1 || k > NN_KMAX || nprobe < 0 || nq > 0x7fffffffL) return -8;
  if (!pq_shape_ok(n, M, ksub)) return -9;
  const size_t lds = pq_lds_bytes(n, M, ksub);
  if (lds + PQ_STATIC_LDS > PQ_LDS_TOTAL) return -9;
  if (lds > 64 * 1024 - PQ_STATIC_LDS)
    (void)hipFuncSetAttribute((const void*)ivfpq_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const int vec = (M % 4 == 0) && (((uintptr_t)codes & 3) == 0);
  hipLaunchKernelGGL(ivfpq_search_kernel, dim3((unsigned)nq), dim3(PQ_T), lds, stream, Q, n, ldq, probes, nprobe,
                     list_off, nlist, N, C, cbT, codes, M, ksub, ip, vec, k, out_d, out_i);
  return srml_status();
}

// Candidate rows for queries [q0, q0 + nq): row r of D / DI (ldd columns, ldd >= the largest
// candidate count of these queries, as srml_ivf_candidate_max reports) = query q0 + r.
SRML_API int srml_ivfpq_candidates_f32(const float* Q, long q0, long nq, int n, long ldq, const int* probes, int nprobe,
                                       const long long* list_off, int nlist, long N, const float* C, const float* cbT,
                                       const unsigned char* codes, int M, int ksub, int ip, float* D, long long* DI,
                                       long ldd, hipStream_t stream) {
  if (nq <= 0) return 0;
  if (nprobe <= 0 || nprobe > 65535 || nq > 0x7fffffffL || ldd <= 0) return -1;
  if (!pq_shape_ok(n, M, ksub)) return -9;
  const size_t lds = pq_lds_bytes(n, M, ksub);
  if (lds > PQ_LDS_TOTAL) return -9;
  srml_nn::fill_candidates(D, DI, nq * ldd, stream);
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)ivfpq_candidates_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
  const int vec = (M % 4 == 0) && (((uintptr_t)codes & 3) == 0);
  hipLaunchKernelGGL(ivfpq_candidates_kernel, dim3((unsigned)nq, (unsigned)nprobe), dim3(PQ_T), lds, stream, Q, q0, n,
                     ldq, probes, nprobe, list_off, nlist, N, C, cbT, codes, M, ksub, ip, vec, D, DI, ldd);
  return srml_status();
}
