// NN-descent join on dense rows in the metrics that are no Euclidean distance of transformed rows
// (UMAP's approximate l1 / chebyshev / minkowski / canberra / hamming / jaccard / hellinger graphs):
//
//  * srml_nnd_join_f32 — for every query row i of a row block, the k nearest rows among
//      its own list                 pos[i, :kw]
//      its neighbours' neighbours   pos[pos[i, :a], :b]
//      its reverse neighbours       perm[off[i] .. off[i] + R) / kw   (edges grouped by target)
//    re-ranked by the distance of the rows themselves. The dense twin of srml_csr_nnd_join_f32
//    (csr_nnd.hip), same contract; the metric is a template parameter (pair_metric.h).
//
// One 256-thread workgroup owns one graph row:
//
//  1. the query row is staged in LDS with the metric's pre-map applied (JACCARD: indicators) when
//     it has at most ND_STAGE features; a longer row is read from global memory. JACCARD counts
//     the row's non-zeros here, once per block;
//  2. the kw + a b + R candidate slots are gathered into LDS, one slot per thread; -1 entries, ids
//     outside [0, N) and the slots past a short reverse list become NJ_NONE; the slots are sorted
//     (bitonic, in LDS), so duplicates are neighbours;
//  3. the live slots that differ from their left neighbour are compacted (wave ballots + an
//     8-entry prefix): L unique ids, BEFORE any distance is computed, so no team idles on a
//     duplicate;
//  4. distances by sub-wave teams of TW = 8 / 16 / 32 / 64 lanes (the host picks the narrowest
//     whose one pass of quads covers the row: a 32-feature row keeps all 32 teams of the block
//     busy instead of 8 lanes of each wave). A team owns TWO candidates per step: both rows'
//     16-byte global loads (consecutive lanes on consecutive quads: one 64 .. 1024-byte run per
//     team) are in flight before the first term is computed; the query quad comes from LDS as
//     one 16-byte read (teams of a wave read the same address: a broadcast). Every lane folds
//     its terms, the team reduces by xor-shuffles (a sum; a max for LINF) and the finaliser
//     follows. JACCARD folds the candidate's non-zero count in the same loop. Every step is
//     block-uniform: a team past the last candidate re-computes candidate 0 and writes nothing;
//  5. (orderable fp32 bits << 32 | id) keys are sorted in LDS (only the power of two that holds L)
//     and the first k written: ascending by (key, id), equal keys to the lower id, missing places
//     +inf / -1.
//
// VEC = false serves an unaligned base pointer, ld % 4 != 0 or n % 4 != 0 with element loads (lanes
// stride the features), as pairdist_kernel<M, false> does. A row that lists itself is a candidate
// like any other and keeps itself at its true distance. No atomics, no cross-block state: the
// output is a pure function of the inputs.
#include "common.h"
#include "nnd_lds.h"      // NJ_T, NJ_NONE, NJ_EMPTY, nj_sort, nj_orderable, nj_float
#include "pair_metric.h"  // PD_* codes, pd_pre, pd_term, pd_final

namespace {
constexpr int ND_WAVES = NJ_T / 64;
constexpr int ND_CAND = 512;     // candidate slots (kw + a b + R) per row; a power of two, 2 per thread
constexpr int ND_STAGE = 8192;   // query features staged in LDS (32 KiB)
constexpr int ND_KMAX = 64;      // output width
constexpr int ND_LDS = ND_STAGE * 4 + ND_CAND * 16 + (3 * ND_WAVES + 1) * 4;
constexpr int ND_LDS_MAX = 64 * 1024;  // static LDS of one workgroup
static_assert(ND_LDS <= ND_LDS_MAX && ND_CAND == 2 * NJ_T, "nnd.hip: LDS layout");

struct NdArgs {
  const float* Q;  // the block's first query row
  long ldq, row0;
  const float* I;
  long ldi, N;
  int n;
  float p;
  const long long* pos;
  int kw;
  const long long* perm;
  const long long* off;
  int k, a, b, R, P;
  float* outk;
  long long* outi;
};

template <int M, int TW>
__device__ __forceinline__ float nd_team_fold(float v) {
#pragma unroll
  for (int o = TW >> 1; o > 0; o >>= 1) {
    const float w = __shfl_xor(v, o);
    v = M == PD_LINF ? fmaxf(v, w) : v + w;
  }
  return v;
}

// d(x, y0), d(x, y1) by one team; x is the query row (LDS image or global row; the pre-map is
// idempotent), lane l of the team. Every lane of the team returns both distances.
template <int M, int TW, bool VEC, typename PX>
__device__ __forceinline__ void nd_pair2(PX x, const float* __restrict__ y0, const float* __restrict__ y1, int n,
                                         float p, float qnz, int l, float& d0, float& d1) {
  float acc0 = 0.f, acc1 = 0.f, nz0 = 0.f, nz1 = 0.f;
  if constexpr (VEC) {
    for (int e = 4 * l; e < n; e += 4 * TW) {  // n % 4 == 0: whole quads
      const floatx4 v0 = *reinterpret_cast<const floatx4*>(y0 + e);
      const floatx4 v1 = *reinterpret_cast<const floatx4*>(y1 + e);
      const floatx4 xv = *reinterpret_cast<const floatx4*>(x + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float xa = pd_pre<M>(xv[j]), b0 = pd_pre<M>(v0[j]), b1 = pd_pre<M>(v1[j]);
        pd_term<M>(acc0, xa, b0, p);
        pd_term<M>(acc1, xa, b1, p);
        if constexpr (M == PD_JACCARD) {
          nz0 += b0;
          nz1 += b1;
        }
      }
    }
  } else {
    for (int e = l; e < n; e += TW) {
      const float xa = pd_pre<M>(x[e]), b0 = pd_pre<M>(y0[e]), b1 = pd_pre<M>(y1[e]);
      pd_term<M>(acc0, xa, b0, p);
      pd_term<M>(acc1, xa, b1, p);
      if constexpr (M == PD_JACCARD) {
        nz0 += b0;
        nz1 += b1;
      }
    }
  }
  acc0 = nd_team_fold<M, TW>(acc0);
  acc1 = nd_team_fold<M, TW>(acc1);
  if constexpr (M == PD_JACCARD) {
    nz0 = nd_team_fold<M, TW>(nz0);
    nz1 = nd_team_fold<M, TW>(nz1);
  }
  d0 = pd_final<M>(acc0, qnz, nz0, n, p);
  d1 = pd_final<M>(acc1, qnz, nz1, n, p);
}

template <int M, int TW, bool VEC>
__global__ __launch_bounds__(NJ_T) void nnd_join_kernel(const NdArgs A) {
  __shared__ __attribute__((aligned(16))) float sQ[ND_STAGE];
  __shared__ int sC[ND_CAND];                 // the sorted slots
  __shared__ int sL[ND_CAND];                 // the live unique ids, compacted
  __shared__ unsigned long long sK[ND_CAND];  // the packed keys
  __shared__ float sNz[ND_WAVES];
  __shared__ int sCnt[2 * ND_WAVES + 1];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long q = blockIdx.x, i = A.row0 + q;  // the block's row and its row in the graph
  const int n = A.n, kw = A.kw;
  const long N = A.N;
  const float* __restrict__ qrow = A.Q + q * A.ldq;
  const bool staged = n <= ND_STAGE;
  // 1. the query row -> LDS (pre-mapped); JACCARD: its non-zero count
  if (staged || M == PD_JACCARD) {
    float cnt = 0.f;
    if constexpr (VEC) {
      for (int e = 4 * t; e < n; e += 4 * NJ_T) {
        floatx4 v = *reinterpret_cast<const floatx4*>(qrow + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = pd_pre<M>(v[j]);
          cnt += v[j];
        }
        if (staged) *reinterpret_cast<floatx4*>(&sQ[e]) = v;
      }
    } else {
      for (int e = t; e < n; e += NJ_T) {
        const float v = pd_pre<M>(qrow[e]);
        cnt += v;
        if (staged) sQ[e] = v;
      }
    }
    if constexpr (M == PD_JACCARD) {  // exact integers in fp32: the order of the sum is immaterial
      cnt = nd_team_fold<M, 64>(cnt);
      if (lane == 0) sNz[wave] = cnt;
    }
  }
  // 2. candidate slots: own list, neighbours' neighbours, reverse neighbours; P - total empty ones
  const int ab = A.a * A.b, total = kw + ab + A.R, P = A.P;
  const long long nperm = (long long)N * kw;
  for (int s = t; s < P; s += NJ_T) {
    long long id = -1;
    if (s < kw) {
      id = A.pos[i * kw + s];
    } else if (s < kw + ab) {
      const int e = s - kw;
      const long long nb = A.pos[i * kw + e / A.b];
      if (nb >= 0 && nb < N) id = A.pos[nb * kw + e % A.b];
    } else if (s < total) {
      const long long pp = A.off[i] + (s - kw - ab);
      if (pp >= 0 && pp < A.off[i + 1] && pp < nperm) {
        const long long e = A.perm[pp];
        if (e >= 0 && e < nperm) id = e / kw;
      }
    }
    sC[s] = (id >= 0 && id < N) ? (int)id : NJ_NONE;
  }
  nj_sort(sC, P, t);  // its first barrier also orders the staging and the gather before the sort
  // 3. compaction of the live slots that differ from their left neighbour (slot t and t + 256)
  int cid[2], within[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int s = t + h * NJ_T;
    cid[h] = s < P ? sC[s] : NJ_NONE;
    if (cid[h] != NJ_NONE && s > 0 && sC[s - 1] == cid[h]) cid[h] = NJ_NONE;
    const unsigned long long m = __ballot(cid[h] != NJ_NONE);
    within[h] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) sCnt[h * ND_WAVES + wave] = __popcll(m);
  }
  __syncthreads();
  int L = 0;
  int base[2] = {0, 0};
#pragma unroll
  for (int g = 0; g < 2 * ND_WAVES; ++g) {
    if (g == wave) base[0] = L;
    if (g == ND_WAVES + wave) base[1] = L;
    L += sCnt[g];
  }
#pragma unroll
  for (int h = 0; h < 2; ++h)
    if (cid[h] != NJ_NONE) sL[base[h] + within[h]] = cid[h];
  float qnz = 0.f;
  if constexpr (M == PD_JACCARD) qnz = sNz[0] + sNz[1] + sNz[2] + sNz[3];
  int P2 = 2;
  while (P2 < L) P2 <<= 1;
  for (int s = L + t; s < P2; s += NJ_T) sK[s] = NJ_EMPTY;
  __syncthreads();
  // 4. distances: team g takes candidates step + g and step + NT + g (block-uniform trip count)
  constexpr int NT = NJ_T / TW;
  const int team = t / TW, l = t % TW;
  for (int step = 0; step < L; step += 2 * NT) {
    const int c0 = step + team, c1 = c0 + NT;
    const int id0 = sL[c0 < L ? c0 : 0], id1 = sL[c1 < L ? c1 : 0];
    const float* __restrict__ y0 = A.I + (long)id0 * A.ldi;
    const float* __restrict__ y1 = A.I + (long)id1 * A.ldi;
    float d0, d1;
    if (staged)
      nd_pair2<M, TW, VEC>((const float*)sQ, y0, y1, n, A.p, qnz, l, d0, d1);
    else
      nd_pair2<M, TW, VEC>(qrow, y0, y1, n, A.p, qnz, l, d0, d1);
    if (l == 0) {
      if (c0 < L) sK[c0] = ((unsigned long long)nj_orderable(d0) << 32) | (unsigned)id0;
      if (c1 < L) sK[c1] = ((unsigned long long)nj_orderable(d1) << 32) | (unsigned)id1;
    }
  }
  // 5. the k smallest (key, id)
  nj_sort(sK, P2, t);
  for (int j = t; j < A.k; j += NJ_T) {
    const unsigned long long key = j < P2 ? sK[j] : NJ_EMPTY;
    const bool none = key == NJ_EMPTY;
    A.outk[q * A.k + j] = none ? __int_as_float(0x7f800000) : nj_float((unsigned)(key >> 32));
    A.outi[q * A.k + j] = none ? -1LL : (long long)(key & 0xffffffffull);
  }
}

template <int M, int TW>
int nd_launch_tw(const NdArgs& A, long rows, bool vec, hipStream_t stream) {
  if (vec)
    hipLaunchKernelGGL((nnd_join_kernel<M, TW, true>), dim3((unsigned)rows), dim3(NJ_T), 0, stream, A);
  else
    hipLaunchKernelGGL((nnd_join_kernel<M, TW, false>), dim3((unsigned)rows), dim3(NJ_T), 0, stream, A);
  return srml_status();
}

// the narrowest team whose one pass of quads covers the row
inline int nd_team_width(int n) { return n <= 32 ? 8 : n <= 64 ? 16 : n <= 128 ? 32 : 64; }

template <int M>
int nd_launch(const NdArgs& A, long rows, hipStream_t stream) {
  const bool vec = ((A.ldq & 3) == 0) && ((A.ldi & 3) == 0) && ((A.n & 3) == 0) &&
                   ((reinterpret_cast<uintptr_t>(A.Q) & 15) == 0) && ((reinterpret_cast<uintptr_t>(A.I) & 15) == 0);
  switch (nd_team_width(A.n)) {
    case 8: return nd_launch_tw<M, 8>(A, rows, vec, stream);
    case 16: return nd_launch_tw<M, 16>(A, rows, vec, stream);
    case 32: return nd_launch_tw<M, 32>(A, rows, vec, stream);
    default: return nd_launch_tw<M, 64>(A, rows, vec, stream);
  }
}
}  // namespace

// The dispatch constants of this file, for the Python layer's checks: 0 candidate slots per row,
// 1 query features staged in LDS, 2 largest output width.
SRML_API int srml_nnd_config(int which) {
  switch (which) {
    case 0: return ND_CAND;
    case 1: return ND_STAGE;
    case 2: return ND_KMAX;
    default: return -1;
  }
}

// (outk fp32, outi int64) [rows, k] = the k nearest candidates of graph rows row0 .. row0 + rows.
// Q points at the block's first row (rows x n, leading dim ldq), I at the N x n item matrix (leading
// dim ldi); both hold the rows as srml_pairdist_f32 reads them (HELLINGER: square roots). pos is the
// N x kw graph, perm (N kw edge numbers grouped by target) and off (N + 1 group starts) its reverse
// lists; a, b <= kw. metric: the codes of srml_pairdist_f32 (0 .. 6, MINKOWSKI with exponent p >= 1)
// and 9 SQEUCLIDEAN (direct form).
// -1: the grid overflows, -2: bad metric, arguments or p, -3: kw + a b + R exceeds the candidate
// slots or k the output width.
SRML_API int srml_nnd_join_f32(const float* Q, long rows, long row0, long ldq, const float* I, long N, int n, long ldi,
                               const long long* pos, int kw, const long long* perm, const long long* off, int k, int a,
                               int b, int R, int metric, float p, float* outk, long long* outi, hipStream_t stream) {
  if (rows <= 0) return 0;
  if (k < 1 || kw < 1 || a < 0 || b < 0 || R < 0 || a > kw || b > kw || n < 1 || ldq < n || ldi < n) return -2;
  if (row0 < 0 || row0 + rows > N || N >= (long)NJ_NONE) return -2;
  if (k > ND_KMAX || R > ND_CAND || (long)kw + (long)a * b + R > ND_CAND) return -3;
  if (rows > srml_max_blocks(NJ_T)) return -1;
  int P = 2;
  while (P < kw + a * b + R) P <<= 1;
  const NdArgs A = {Q, ldq, row0, I, ldi, N, n, p, pos, kw, perm, off, k, a, b, R, P, outk, outi};
  switch (metric) {
    case PD_L1: return nd_launch<PD_L1>(A, rows, stream);
    case PD_LINF: return nd_launch<PD_LINF>(A, rows, stream);
    case PD_MINKOWSKI:
      if (!(p >= 1.f) || !(p < 3.0e38f)) return -2;
      if (p == 1.f) return nd_launch<PD_L1>(A, rows, stream);
      if (p == 3.f) return nd_launch<PD_MINK3>(A, rows, stream);
      if (p == 4.f) return nd_launch<PD_MINK4>(A, rows, stream);
      return nd_launch<PD_MINKOWSKI>(A, rows, stream);
    case PD_CANBERRA: return nd_launch<PD_CANBERRA>(A, rows, stream);
    case PD_HAMMING: return nd_launch<PD_HAMMING>(A, rows, stream);
    case PD_JACCARD: return nd_launch<PD_JACCARD>(A, rows, stream);
    case PD_HELLINGER: return nd_launch<PD_HELLINGER>(A, rows, stream);
    case PD_SQEUCLIDEAN: return nd_launch<PD_SQEUCLIDEAN>(A, rows, stream);
    default: return -2;
  }
}
