// IVF-Flat search kernels: the per-query scan (k <= 64) and the large-k candidate matrix.
#include "common.h"

#include "neighbors.h"

// ------------------------------------------------------------------------------------------
// IVF-Flat search: one block per query; the query's nprobe inverted lists (items pre-sorted by
// list, contiguous) are swept by the 4 waves, one item per wave step: lanes split the feature
// dimension (16-B loads), the dot product is a DPP wave reduction, and a wave-private sorted
// top-k list in LDS takes the candidate when it beats the list's threshold. The four lists are
// merged at the end (reference: cuML NearestNeighbors(algorithm="ivfflat"), knn.py:1295-1380).
// ------------------------------------------------------------------------------------------
namespace {
using namespace srml_nn;

// G lanes per item (G = pow2 >= n/4, <= 64): a wave scores 64/G items per step, each group
// reduces its dot product with in-group shuffles; candidates are inserted in item order with
// wave-uniform threshold tests (a 128-wide item used only 32 lanes of a 64-lane wave per step).
template <int G>
__global__ __launch_bounds__(256) void ivf_search_kernel(const float* __restrict__ Q, long nq, int n, long ldq,
                                                         const int* __restrict__ probes, int nprobe,
                                                         const long long* __restrict__ list_off,
                                                         const float* __restrict__ items, long ldi,
                                                         const float* __restrict__ inorm,
                                                         const long long* __restrict__ ids, int k,
                                                         float* __restrict__ out_d, long long* __restrict__ out_i) {
  constexpr int IPW = 64 / G;  // items per wave step
  extern __shared__ __attribute__((aligned(16))) float qs[];  // n floats (padded to 4)
  __shared__ WaveD wd;
  __shared__ WaveI wi;
  const long q = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int gi = lane / G, gl = lane % G;
  for (int d = t; d < n; d += 256) qs[d] = Q[q * ldq + d];
  wave_lists_init(wd, wi);
  __syncthreads();
  float thr = __builtin_huge_valf();
  const bool vec = ((n & 3) == 0) && ((ldi & 3) == 0);
  for (int p = 0; p < nprobe; ++p) {
    const int l = probes[q * nprobe + p];
    if (l < 0) continue;
    const long s = list_off[l], e = list_off[l + 1];
    for (long j0 = s + (long)wid * IPW; j0 < e; j0 += 4 * IPW) {
      const long j = j0 + gi;
      float acc = 0.f;
      if (j < e) {
        const float* row = items + j * ldi;
        if (vec) {
          for (int d = gl * 4; d < n; d += 4 * G) {
            const floatx4 x = *reinterpret_cast<const floatx4*>(row + d);
            acc = fmaf(x[0], qs[d], fmaf(x[1], qs[d + 1], fmaf(x[2], qs[d + 2], fmaf(x[3], qs[d + 3], acc))));
          }
        } else {
          for (int d = gl; d < n; d += G) acc = fmaf(row[d], qs[d], acc);
        }
      }
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
      const float dist = j < e ? fmaf(-2.f, acc, inorm[j]) : __builtin_huge_valf();
#pragma unroll
      for (int g = 0; g < IPW; ++g) {
        const float dg = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dist), g * G));
        if (dg < thr) wave_list_offer(wd, wi, k, dg, ids[j0 + g], thr);  // wave-uniform
      }
    }
  }
  __syncthreads();
  if (t == 0) wave_lists_merge_write(wd, wi, k, out_d + q * k, out_i + q * k);
}
}  // namespace

SRML_API int srml_ivf_search_f32(const float* Q, long nq, int n, long ldq, const int* probes, int nprobe,
                                 const long long* list_off, const float* items, long ldi, const float* inorm,
                                 const long long* ids, int k, float* out_d, long long* out_i, hipStream_t stream) {
  if (nq <= 0) return 0;
  if (k < 1 || k > NN_KMAX) return -8;
  const size_t lds = (size_t)((n + 3) / 4) * 4 * sizeof(float);
  const int need = (n + 3) / 4;  // lanes that a 16-B-per-lane pass over one item occupies
#define SRML_IVF(GG)                                                                                        \
  hipLaunchKernelGGL((ivf_search_kernel<GG>), dim3((unsigned)nq), dim3(256), lds, stream, Q, nq, n, ldq, probes, \
                     nprobe, list_off, items, ldi, inorm, ids, k, out_d, out_i)
  if (need <= 8) SRML_IVF(8);
  else if (need <= 16) SRML_IVF(16);
  else if (need <= 32) SRML_IVF(32);
  else SRML_IVF(64);
#undef SRML_IVF
  return srml_status();
}

// ------------------------------------------------------------------------------------------
// IVF large-k candidates (64 < k <= 1024; the k <= 64 paths keep LDS insertion lists): for every
// (query, probe) the distances ||i||^2 - 2 q.i to each item of the probed list are written, with
// the item's id (or list position), into the query's row of a candidate matrix at the prefix
// offset of its earlier probes; columns past the query's candidate count are +inf / -1. One block
// per (query, probe): the query vector is staged in LDS once, the list's items stream through
// 64-row LDS tiles (coalesced 16-B row loads, row stride n + 1 words: conflict-free column reads)
// and each thread forms one item's dot product. srml_topk_rows_f32 (with ids) then selects k per
// query. qlist: optional query -> list map (all-points kNN over IVF lists: a row probes the lists
// of its own list's probe set); without it probes are per query.
// ------------------------------------------------------------------------------------------
constexpr int IVC_T = 256;
constexpr int IVC_ROWS = 64;
constexpr int IVC_NC = 512;  // feature chunk staged in LDS (133 KiB with the 64-row tile)

__global__ __launch_bounds__(IVC_T) void ivf_candidates_kernel(const float* __restrict__ Q, long q0, int n, long ldq,
                                                               const int* __restrict__ probes, int nprobe,
                                                               const int* __restrict__ qlist,
                                                               const long long* __restrict__ list_off,
                                                               const float* __restrict__ items, long ldi,
                                                               const float* __restrict__ inorm,
                                                               const long long* __restrict__ ids, float* __restrict__ D,
                                                               long long* __restrict__ DI, long ldd, int nc) {
  // features are staged in chunks of nc (= min(n, IVC_NC)) columns, so any width fits the LDS:
  // each row's dot product accumulates in its thread's register across the chunks
  extern __shared__ float ivc_s[];  // q chunk [nc] | tile[IVC_ROWS][nc + 1]
  float* qs = ivc_s;
  float* tile = ivc_s + nc;
  const int tn = nc + 1;
  const long qi = q0 + blockIdx.x;  // global query (row) index
  const int p = blockIdx.y;
  const int* pr = probes + (long)(qlist ? qlist[qi] : qi) * nprobe;
  const int l = pr[p];
  // this probe's offset in the query's candidate row
  long off = 0;
  for (int j = 0; j < p; ++j)
    if (pr[j] >= 0) off += list_off[pr[j] + 1] - list_off[pr[j]];
  if (l < 0) return;
  const long b0 = list_off[l], b1 = list_off[l + 1];
  float* drow = D + (long)blockIdx.x * ldd + off;
  long long* irow = DI + (long)blockIdx.x * ldd + off;
  for (long r0 = b0; r0 < b1; r0 += IVC_ROWS) {
    const int rows = (int)min((long)IVC_ROWS, b1 - r0);
    float acc = 0.f;
    for (int c0 = 0; c0 < n; c0 += nc) {
      const int w = min(nc, n - c0);
      __syncthreads();  // previous chunk / tile consumed
      for (int c = threadIdx.x; c < w; c += IVC_T) qs[c] = Q[qi * ldq + c0 + c];
      for (int e = threadIdx.x; e < rows * w; e += IVC_T) {
        const int rr = e / w, cc = e - rr * w;
        tile[rr * tn + cc] = items[(r0 + rr) * ldi + c0 + cc];
      }
      __syncthreads();
      if (threadIdx.x < rows) {
        const float* row = tile + threadIdx.x * tn;
        for (int c = 0; c < w; ++c) acc = fmaf(qs[c], row[c], acc);
      }
    }
    if (threadIdx.x < rows) {
      const long it = r0 + threadIdx.x;
      drow[it - b0] = inorm[it] - 2.f * acc;
      irow[it - b0] = ids ? ids[it] : it;
    }
  }
}

__global__ void ivf_count_kernel(const int* __restrict__ probes, int nprobe, const int* __restrict__ qlist, long nq,
                                 const long long* __restrict__ list_off, unsigned long long* __restrict__ cmax) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const int* pr = probes + (long)(qlist ? qlist[q] : q) * nprobe;
  unsigned long long c = 0;
  for (int j = 0; j < nprobe; ++j)
    if (pr[j] >= 0) c += (unsigned long long)(list_off[pr[j] + 1] - list_off[pr[j]]);
  atomicMax(cmax, c);
}

// Largest candidate count over nq queries (-> *cmax, which the caller zeroes): sizes the matrix.
SRML_API int srml_ivf_candidate_max(const int* probes, int nprobe, const int* qlist, long nq, const long long* list_off,
                                    unsigned long long* cmax, hipStream_t stream) {
  if (nq <= 0) return 0;
  hipLaunchKernelGGL(ivf_count_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, probes, nprobe, qlist,
                     nq, list_off, cmax);
  return srml_status();
}

__global__ void row_list_kernel(const long long* __restrict__ list_off, int nlist, long N, int* __restrict__ qlist) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  int lo = 0, hi = nlist - 1;  // largest l with list_off[l] <= r
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (list_off[mid] <= r) lo = mid; else hi = mid - 1;
  }
  qlist[r] = lo;
}

// List of every row of a list-sorted matrix (list_off: nlist + 1 offsets covering the N rows).
SRML_API int srml_row_list(const long long* list_off, int nlist, long N, int* qlist, hipStream_t stream) {
  if (N <= 0 || nlist <= 0) return 0;
  hipLaunchKernelGGL(row_list_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, list_off, nlist, N, qlist);
  return srml_status();
}

__global__ void ivf_fill_kernel(float* __restrict__ D, long long* __restrict__ DI, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  D[i] = __builtin_huge_valf();
  DI[i] = -1;
}

void srml_nn::fill_candidates(float* D, long long* DI, long total, hipStream_t stream) {
  hipLaunchKernelGGL(ivf_fill_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, D, DI, total);
}

// Candidate matrix rows for queries [q0, q0 + nq) (row r of D / DI = query q0 + r, ldd columns,
// ldd >= the largest candidate count of these queries; the caller sizes it).
SRML_API int srml_ivf_candidates_f32(const float* Q, long q0, long nq, int n, long ldq, const int* probes, int nprobe,
                                     const int* qlist, const long long* list_off, const float* items, long ldi,
                                     const float* inorm, const long long* ids, float* D, long long* DI, long ldd,
                                     hipStream_t stream) {
  if (nq <= 0) return 0;
  if (n <= 0 || nprobe <= 0 || nprobe > 65535 || nq > 0x7fffffffL || ldd <= 0) return -1;
  const int nc = n < IVC_NC ? n : IVC_NC;
  const size_t shm = (size_t)(nc + IVC_ROWS * (nc + 1)) * sizeof(float);
  srml_nn::fill_candidates(D, DI, nq * ldd, stream);
  if (shm > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)ivf_candidates_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  hipLaunchKernelGGL(ivf_candidates_kernel, dim3((unsigned)nq, (unsigned)nprobe), dim3(IVC_T), shm, stream, Q, q0, n,
                     ldq, probes, nprobe, qlist, list_off, items, ldi, inorm, ids, D, DI, ldd, nc);
  return srml_status();
}
