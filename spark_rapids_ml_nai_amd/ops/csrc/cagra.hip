// CAGRA: a fixed-degree proximity graph walked greedily on the device (cuVS "CAGRA"; beyond the
// reference version, whose later releases ship it).
//
// Build: the all-points kNN graph (models/knn_graph.py) is cut from d to gd edges per node by
// rank-based detour pruning (srml_cagra_prune_i32), then half of every row is given to reverse
// edges (srml_cagra_merge_i32; the edges are grouped by the project's radix sort, so the rows do
// not depend on atomic arrival order).
// Search (srml_cagra_search_f32): one 256-thread workgroup per query keeps the whole beam state in
// LDS: the query row, the sorted list of itopk packed keys, the candidate buffer and the visited
// hash. Per iteration the first `width` unexpanded list entries hand in their graph rows, the new
// ones are scored from gathered rows (teams of 8 lanes, 16-byte loads, 8 rows in flight per wave,
// all four waves), bitonic-sorted and bitonic-merged into the list. No atomics leave the block and
// the list order is total ((d2, id); a node is scored once), so the result is a pure function of
// the inputs.
//
// A packed key is d2's fp32 bit pattern (non-negative, so it orders as an unsigned integer) in the
// high word and (id << 1 | expanded) in the low word; all ones is the empty slot.
#include "common.h"

namespace {
constexpr int CG_T = 256;
constexpr int CG_DMAX = 128;       // intermediate and final graph degree
constexpr int CG_ITOPK_MAX = 512;
constexpr int CG_CAND_MAX = 512;   // width * gd
constexpr int CG_SEED_MAX = 1024;
constexpr int CG_TEAM = 8;         // lanes per gathered row
static_assert(CG_TEAM == 8, "cg_score folds a team with the DPP steps of an 8-lane half row");
constexpr size_t CG_STATIC_LDS = 64;
constexpr size_t CG_LDS_TOTAL = 160 * 1024;  // per CU on gfx950; one workgroup may take all of it
constexpr unsigned long long CG_EMPTY = ~0ull;
typedef unsigned long long u64;

__host__ __device__ inline int cg_pow2(long v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

__host__ __device__ inline unsigned cg_mix(unsigned h) {  // murmur3's finaliser
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// The one place the dynamic LDS of the search kernel is laid out (host: the budget; device: the
// pointers): query row | keys (list + candidates) | candidate ids | parents | visited table.
struct CgLayout {
  int c_init, c_iter, p_init, p_iter, lg_slots;
  size_t q, buf, cand, par, vis, total;
};

__host__ __device__ inline CgLayout cg_layout(int n, int itopk, int width, int gd, int S, int max_iter) {
  CgLayout L;
  L.c_init = cg_pow2(S);
  L.c_iter = cg_pow2((long)width * gd);
  L.p_init = cg_pow2((long)itopk + L.c_init);
  L.p_iter = cg_pow2((long)itopk + L.c_iter);
  const long inserts = (long)S + (long)max_iter * width * gd;
  L.lg_slots = 1;
  while ((1L << L.lg_slots) < 2 * inserts) ++L.lg_slots;
  const int pmax = L.p_init > L.p_iter ? L.p_init : L.p_iter;
  const int cmax = L.c_init > L.c_iter ? L.c_init : L.c_iter;
  L.q = 0;
  L.buf = L.q + (size_t)((n + 3) / 4) * 16;
  L.cand = L.buf + (size_t)pmax * 8;
  L.par = L.cand + (size_t)cmax * 4;
  L.vis = L.par + (size_t)((width + 3) / 4) * 16;
  L.total = L.vis + ((size_t)4 << L.lg_slots);
  return L;
}

inline bool cg_search_shape_ok(int n, long N, int gd, int S, int k, int itopk, int width, int max_iter, int min_iter) {
  return n >= 1 && N >= 1 && N <= 0x7fffffffL && gd >= 1 && gd <= CG_DMAX && itopk >= 32 && itopk <= CG_ITOPK_MAX &&
         itopk % 32 == 0 && width >= 1 && (long)width * gd <= CG_CAND_MAX && k >= 1 && k <= itopk && S >= 1 &&
         S <= CG_SEED_MAX && max_iter >= 0 && max_iter <= 65536 && min_iter >= 0;
}

// ------------------------------------------------------------------------------------- seeds
// out[q][s] = mix(rowhash(q) ^ mix(seed, s)) mod N, rowhash = sum_d mix(bits(Q[q][d]) ^ (d + 1) g)
// (a wrapping sum, so lanes may take the features in any order).
__global__ __launch_bounds__(64) void cagra_seeds_kernel(const float* __restrict__ Q, int n, long ldq, unsigned N,
                                                         int S, unsigned seed, int* __restrict__ out) {
  const long q = blockIdx.x;
  const int lane = threadIdx.x;
  unsigned h = 0;
  for (int d = lane; d < n; d += 64) h += cg_mix(__float_as_uint(Q[q * ldq + d]) ^ ((unsigned)(d + 1) * 0x9E3779B9u));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) h += (unsigned)__shfl_xor((int)h, o, 64);
  for (int s = lane; s < S; s += 64)
    out[q * S + s] = (int)(cg_mix(h ^ cg_mix(seed * 0x9E3779B9u + (unsigned)s * 0x85EBCA6Bu + 1u)) % N);
}

// ------------------------------------------------------------------------------------- prune
// One block per node a. detour(a, i) = #{j < i : G[G[a][j]] holds G[a][i] at a slot l < i}; the
// neighbours' rows are read coalesced (consecutive threads, consecutive slots) and looked up in a
// sorted copy of the node's own list. Entries of a row are distinct (a kNN list).
__global__ __launch_bounds__(CG_T) void cagra_prune_kernel(const int* __restrict__ G, long N, int d, int gd,
                                                           int* __restrict__ P) {
  __shared__ int lst[CG_DMAX], sval[CG_DMAX], srank[CG_DMAX], cnt[CG_DMAX];
  const long a = blockIdx.x;
  const int t = threadIdx.x;
  if (t < d) {
    const int v = G[a * d + t];
    lst[t] = (v >= 0 && v < N) ? v : -1;
    cnt[t] = 0;
  }
  const int nv = __syncthreads_count(t < d && lst[t] >= 0);
  if (t < d) {  // rank sort by (value, rank): invalid entries go last
    const u64 mine = ((u64)(lst[t] < 0 ? 0x7fffffffu : (unsigned)lst[t]) << 8) | (unsigned)t;
    int pos = 0;
    for (int i = 0; i < d; ++i) pos += ((((u64)(lst[i] < 0 ? 0x7fffffffu : (unsigned)lst[i])) << 8) | (unsigned)i) < mine;
    sval[pos] = lst[t];
    srank[pos] = t;
  }
  __syncthreads();
  for (int e = t; e < d * d; e += CG_T) {
    const int j = e / d, l = e - j * d;
    const int c = lst[j];
    if (c < 0) continue;
    const int v = G[(long)c * d + l];
    if (v < 0) continue;
    int lo = 0, hi = nv;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sval[mid] < v) lo = mid + 1; else hi = mid;
    }
    if (lo < nv && sval[lo] == v) {
      const int i = srank[lo];
      if (i > j && i > l) atomicAdd(&cnt[i], 1);  // LDS integer add: order-free
    }
  }
  __syncthreads();
  if (t < d) {  // position by (detour, rank); invalid entries after every valid one
    const int mine = (lst[t] >= 0 ? cnt[t] : CG_DMAX) * CG_DMAX + t;
    int pos = 0;
    for (int i = 0; i < d; ++i) pos += ((lst[i] >= 0 ? cnt[i] : CG_DMAX) * CG_DMAX + i) < mine;
    if (pos < gd) P[a * gd + pos] = lst[t];
  }
  for (int i = d + t; i < gd; i += CG_T) P[a * gd + i] = -1;
}

// ------------------------------------------------------------------------------------- merge
// One wave per node v. src holds the edge numbers e = p * N + u of every edge P[u][p] = v, grouped
// by v in (p, u) order (a stable sort of the slot-major edge list by v); off[v] .. off[v + 1] is
// v's group. F[v] = first gd of: P[v][:h] | rev[v] not in P[v][:h] | P[v][h:] not in rev[v].
__global__ __launch_bounds__(CG_T) void cagra_merge_kernel(const int* __restrict__ P, long N, int gd,
                                                           const long long* __restrict__ off,
                                                           const int* __restrict__ src, long nedges,
                                                           int* __restrict__ F) {
  __shared__ int prow[4][CG_DMAX], rrow[4][CG_DMAX];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long v = (long)blockIdx.x * 4 + wid;
  const bool live = v < N;
  const int h = gd / 2;
  int nr = 0;
  if (live) {
    long b0 = off[v], b1 = off[v + 1];
    if (b0 < 0) b0 = 0;
    if (b1 > nedges) b1 = nedges;
    nr = (int)(b1 - b0 < 0 ? 0 : (b1 - b0 > gd ? gd : b1 - b0));
    for (int i = lane; i < gd; i += 64) {
      const int w = P[v * gd + i];
      prow[wid][i] = (w >= 0 && w < N) ? w : -1;
      rrow[wid][i] = i < nr ? (int)((long)src[b0 + i] % N) : -1;
    }
  }
  __syncthreads();
  if (!live) return;
  int outn = 0;
  for (int c0 = 0; c0 < 2 * gd && outn < gd; c0 += 64) {  // wave-uniform
    const int c = c0 + lane;
    int val = -1;
    if (c < h) {
      val = prow[wid][c];
    } else if (c < h + gd) {
      val = rrow[wid][c - h];
      for (int i = 0; i < h && val >= 0; ++i)
        if (prow[wid][i] == val) val = -1;
    } else if (c < 2 * gd) {
      val = prow[wid][c - gd];
      for (int i = 0; i < nr && val >= 0; ++i)
        if (rrow[wid][i] == val) val = -1;
    }
    const u64 mask = __ballot(val >= 0);
    const int pos = outn + __popcll(mask & ((1ull << lane) - 1ull));
    if (val >= 0 && pos < gd) F[v * gd + pos] = val;
    outn += __popcll(mask);
  }
  for (int i = (outn < gd ? outn : gd) + lane; i < gd; i += 64) F[v * gd + i] = -1;
}

// ------------------------------------------------------------------------------------ search
__device__ __forceinline__ void cg_cmpx(u64* a, int lo, int hi, bool up) {
  const u64 x = a[lo], y = a[hi];
  if ((x > y) == up) {
    a[lo] = y;
    a[hi] = x;
  }
}

// Bitonic sort of a[0, C), C a power of two, descending. Ends behind a barrier.
__device__ void cg_sort_desc(u64* a, int C) {
  for (int k2 = 2; k2 <= C; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < (C >> 1); i += CG_T) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
        cg_cmpx(a, lo, lo + j, (lo & k2) != 0);
      }
      __syncthreads();
    }
}

// Bitonic merge of the bitonic a[0, P), P a power of two, ascending. Ends behind a barrier.
__device__ void cg_merge_asc(u64* a, int P) {
  for (int j = P >> 1; j > 0; j >>= 1) {
    for (int i = threadIdx.x; i < (P >> 1); i += CG_T) {
      const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
      cg_cmpx(a, lo, lo + j, true);
    }
    __syncthreads();
  }
}

// First visit of id? Open addressing, linear probing; the table has twice the slots of all the
// inserts a search can make, so a free slot always turns up.
__device__ __forceinline__ bool cg_visit(int* vis, int lg, int id) {
  const unsigned mask = (1u << lg) - 1u;
  unsigned s = ((unsigned)id * 0x9E3779B1u) >> (32 - lg);
  for (unsigned it = 0; it <= mask; ++it) {
    const int old = atomicCAS(&vis[s], -1, id);
    if (old == -1) return true;
    if (old == id) return false;
    s = (s + 1) & mask;
  }
  return false;
}

// Keys of the candidates cand[0, C) (-1: none) into dst[0, C). A team of 8 lanes takes one row:
// 16-byte loads when the rows allow it (vec), 8 rows in flight per wave, all four waves.
__device__ void cg_score(const float* qs, const float* __restrict__ X, long ldx, int n, int vec, const int* cand,
                         int C, u64* dst) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int g = lane / CG_TEAM, sub = lane % CG_TEAM;
  const int n4 = vec ? (n >> 2) : 0;
  for (int c0 = wid * (64 / CG_TEAM); c0 < C; c0 += 4 * (64 / CG_TEAM)) {  // wave-uniform
    const int ci = c0 + g;
    const int id = ci < C ? cand[ci] : -1;
    float acc = 0.f;
    if (id >= 0) {
      const float* row = X + (long)id * ldx;
      const floatx4* r4 = reinterpret_cast<const floatx4*>(row);
      const floatx4* q4 = reinterpret_cast<const floatx4*>(qs);
#pragma unroll 4
      for (int c = sub; c < n4; c += CG_TEAM) {
        const floatx4 x = r4[c], y = q4[c];
        const float d0 = y.x - x.x, d1 = y.y - x.y, d2 = y.z - x.z, d3 = y.w - x.w;
        acc = fmaf(d0, d0, acc);
        acc = fmaf(d1, d1, acc);
        acc = fmaf(d2, d2, acc);
        acc = fmaf(d3, d3, acc);
      }
      for (int d = (n4 << 2) + sub; d < n; d += CG_TEAM) {
        const float df = qs[d] - row[d];
        acc = fmaf(df, df, acc);
      }
    }
    acc += dpp_f<0xb1>(acc);   // quad_perm [1,0,3,2]
    acc += dpp_f<0x4e>(acc);   // quad_perm [2,3,0,1]
    acc += dpp_f<0x141>(acc);  // row_half_mirror: every lane of the team holds its 8-lane sum
    if (sub == 0 && ci < C)
      dst[ci] = id >= 0 ? (((u64)__float_as_uint(acc) << 32) | ((unsigned)id << 1)) : CG_EMPTY;
  }
}

// Score cand[0, C), sort the keys (descending, at the end of buf[0, P)) and merge them into the
// ascending list buf[0, itopk); the slots between stay empty, so buf[0, P) is bitonic.
__device__ void cg_round(const float* qs, const float* __restrict__ X, long ldx, int n, int vec, const int* cand,
                         int C, u64* buf, int P, int itopk) {
  for (int i = itopk + threadIdx.x; i < P - C; i += CG_T) buf[i] = CG_EMPTY;
  cg_score(qs, X, ldx, n, vec, cand, C, buf + (P - C));
  __syncthreads();
  cg_sort_desc(buf + (P - C), C);
  cg_merge_asc(buf, P);
}

__global__ __launch_bounds__(CG_T) void cagra_search_kernel(const float* __restrict__ Q, int n, long ldq,
                                                            const float* __restrict__ X, long N, long ldx,
                                                            const int* __restrict__ F, int gd,
                                                            const int* __restrict__ seeds, int S, int k, int itopk,
                                                            int width, int max_iter, int min_iter, int vec,
                                                            float* __restrict__ out_d, long long* __restrict__ out_i) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cg_s[];
  __shared__ int np_s;
  const CgLayout L = cg_layout(n, itopk, width, gd, S, max_iter);
  float* qs = reinterpret_cast<float*>(cg_s + L.q);
  u64* buf = reinterpret_cast<u64*>(cg_s + L.buf);
  int* cand = reinterpret_cast<int*>(cg_s + L.cand);
  int* par = reinterpret_cast<int*>(cg_s + L.par);
  int* vis = reinterpret_cast<int*>(cg_s + L.vis);
  const long q = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  for (int d = t; d < ((n + 3) & ~3); d += CG_T) qs[d] = d < n ? Q[q * ldq + d] : 0.f;
  for (int i = t; i < (1 << L.lg_slots); i += CG_T) vis[i] = -1;
  for (int i = t; i < itopk; i += CG_T) buf[i] = CG_EMPTY;
  __syncthreads();
  for (int i = t; i < L.c_init; i += CG_T) {  // the seeds, duplicates dropped through the table
    int id = -1;
    if (i < S) {
      const int s = seeds[q * S + i];
      if (s >= 0 && s < N && cg_visit(vis, L.lg_slots, s)) id = s;
    }
    cand[i] = id;
  }
  __syncthreads();
  cg_round(qs, X, ldx, n, vec, cand, L.c_init, buf, L.p_init, itopk);
  for (int it = 0; it < max_iter; ++it) {  // everything that steers this loop is block-uniform
    if (wid == 0) {  // the first `width` unexpanded entries, in list order
      int found = 0;
      for (int b = 0; b < itopk && found < width; b += 64) {
        const int i = b + lane;
        const u64 key = i < itopk ? buf[i] : CG_EMPTY;
        const bool un = key != CG_EMPTY && !(key & 1ull);
        const u64 mask = __ballot(un);
        const int r = found + __popcll(mask & ((1ull << lane) - 1ull));
        if (un && r < width) {
          par[r] = (int)((unsigned)(key & 0xffffffffull) >> 1);
          buf[i] = key | 1ull;
        }
        found += __popcll(mask);
      }
      if (lane == 0) np_s = found < width ? found : width;
    }
    __syncthreads();
    const int np = np_s;
    __syncthreads();  // np_s is free for the next iteration
    if (np == 0) {
      if (it >= min_iter) break;
      continue;
    }
    for (int i = t; i < L.c_iter; i += CG_T) {
      int id = -1;
      if (i < np * gd) {
        const int p = i / gd, s = i - p * gd;
        const int v = F[(long)par[p] * gd + s];
        if (v >= 0 && v < N && cg_visit(vis, L.lg_slots, v)) id = v;
      }
      cand[i] = id;
    }
    __syncthreads();
    cg_round(qs, X, ldx, n, vec, cand, L.c_iter, buf, L.p_iter, itopk);
  }
  for (int j = t; j < k; j += CG_T) {
    const u64 key = buf[j];
    const bool ok = key != CG_EMPTY;
    out_d[q * k + j] = ok ? __uint_as_float((unsigned)(key >> 32)) : __builtin_huge_valf();
    out_i[q * k + j] = ok ? (long long)((unsigned)(key & 0xffffffffull) >> 1) : -1;
  }
}
}  // namespace

// Status -8: an argument outside the kernels' limits; -9: the search state does not fit the LDS.

SRML_API int srml_cagra_seeds_i32(const float* Q, long nq, int n, long ldq, long N, int S, unsigned seed, int* out,
                                  hipStream_t stream) {
  if (nq <= 0 || S <= 0) return 0;
  if (n < 1 || ldq < n || N < 1 || N > 0x7fffffffL || nq > srml_max_blocks(64)) return -8;
  hipLaunchKernelGGL(cagra_seeds_kernel, dim3((unsigned)nq), dim3(64), 0, stream, Q, n, ldq, (unsigned)N, S, seed, out);
  return srml_status();
}

// P[a] = the gd ranks of G[a] (int32 [N, d], ascending distance, -1 tail) with the smallest (detour, rank).
SRML_API int srml_cagra_prune_i32(const int* G, long N, int d, int gd, int* P, hipStream_t stream) {
  if (N <= 0) return 0;
  if (d < 1 || d > CG_DMAX || gd < 1 || gd > CG_DMAX || N > 0x7fffffffL || N > srml_max_blocks(CG_T)) return -8;
  hipLaunchKernelGGL(cagra_prune_kernel, dim3((unsigned)N), dim3(CG_T), 0, stream, G, N, d, gd, P);
  return srml_status();
}

// F from P (int32 [N, gd]) and its edges grouped by target (see cagra_merge_kernel).
SRML_API int srml_cagra_merge_i32(const int* P, long N, int gd, const long long* off, const int* src, long nedges,
                                  int* F, hipStream_t stream) {
  if (N <= 0) return 0;
  if (gd < 1 || gd > CG_DMAX || N * gd > 0x7fffffffL || nedges < 0 || nedges > N * gd) return -8;
  hipLaunchKernelGGL(cagra_merge_kernel, dim3((unsigned)((N + 3) / 4)), dim3(CG_T), 0, stream, P, N, gd, off, src,
                     nedges, F);
  return srml_status();
}

// Dynamic + static LDS bytes of one search workgroup (what -9 is decided on).
SRML_API long srml_cagra_lds_bytes(int n, int itopk, int width, int gd, int S, int max_iter) {
  if (n < 1 || itopk < 1 || width < 1 || gd < 1 || S < 1 || max_iter < 0 || max_iter > 65536) return -1;
  return (long)(cg_layout(n, itopk, width, gd, S, max_iter).total + CG_STATIC_LDS);
}

// Ascending (d2, id) of the k best list entries per query after the beam search (empty: +inf / -1).
SRML_API int srml_cagra_search_f32(const float* Q, long nq, int n, long ldq, const float* X, long N, long ldx,
                                   const int* F, int gd, const int* seeds, int S, int k, int itopk, int width,
                                   int max_iter, int min_iter, float* out_d, long long* out_i, hipStream_t stream) {
  if (nq <= 0) return 0;
  if (!cg_search_shape_ok(n, N, gd, S, k, itopk, width, max_iter, min_iter) || ldq < n || ldx < n ||
      nq > srml_max_blocks(CG_T))
    return -8;
  const CgLayout L = cg_layout(n, itopk, width, gd, S, max_iter);
  if (L.total + CG_STATIC_LDS > CG_LDS_TOTAL) return -9;
  if (L.total > 32 * 1024)
    (void)hipFuncSetAttribute((const void*)cagra_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)L.total);
  const int vec = (ldx % 4 == 0) && (((uintptr_t)X & 15) == 0);
  hipLaunchKernelGGL(cagra_search_kernel, dim3((unsigned)nq), dim3(CG_T), L.total, stream, Q, n, ldq, X, N, ldx, F, gd,
                     seeds, S, k, itopk, width, max_iter, min_iter, vec, out_d, out_i);
  return srml_status();
}
