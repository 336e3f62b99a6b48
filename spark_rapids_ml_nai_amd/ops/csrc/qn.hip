// On-device quasi-Newton driver (L-BFGS, and OWL-QN for L1 / elastic-net) for the GLM solvers.
//
// Reference: cuML's QN solver behind LogisticRegressionMG (classification.py:957-1151,
// lbfgs_memory=10, penalty_normalized=False): it runs its L-BFGS / OWL-QN iteration on the host
// and pays a device round trip per function evaluation. Here the whole optimiser state lives in
// device memory and an on-device step advances it after every (all-reduced) loss+gradient
// evaluation, so a fit is a stream of   [fused loss/grad pass] -> [RCCL all-reduce] -> [qn step]
// launches with no host synchronisation; the host only polls a `done` flag every few evaluations
// (and the evaluation kernels early-exit once it is set). The step has two forms built from the
// same pieces (the first part of this file): four multi-block launches (N <= 16384, the default)
// and one single-block kernel (larger N, the batch of independent problems, the probe).
//
// State machine per step (one evaluation at the trial point xt has just been summed into `out`):
//   pass 0  smooth gradient at xt in the optimiser's (standardised) coordinates, penalty terms,
//           directional derivatives; `out` is re-zeroed for the next evaluation.
//   line search (backtracking Armijo — cuML's default LBFGS_LS_BT_ARMIJO — with a safeguarded quadratic
//           interpolation step in [0.1, 0.5] instead of plain halving; optional weak
//           Wolfe with inc = 2.1 until bracketed; OWL-QN: Armijo on the projected step).
//   accept  pass 1 computes, in ONE fused multi-value block reduction, every dot product the
//           compact L-BFGS representation needs (Byrd-Nocedal-Schnabel: H = gI + [S gY] M [S gY]^T)
//           — new-pair products with the history and S^T pg, Y^T pg — instead of the 2m dependent
//           reductions of the two-loop recursion; thread 0 solves the small triangular systems;
//           pass 2 stores the pair, forms the direction (orthant-constrained for OWL-QN) and
//           moves x; pass 3 writes the next trial point (orthant-projected) and the evaluation
//           parameters w = xt[:Kn] * inv_sigma, b = xt[Kn:].
// Convergence (cuML qn semantics): max|pg| <= tol * max(|f|, tol); |f_{k-past} - f_k| <= delta *
// max(|f|, tol); k >= max_iter; or a failed line search (the last accepted point is kept).
#include "common.h"

namespace {

constexpr int QN_T = 512;      // one block, 8 waves: the passes are latency-bound (143 VGPRs, no spills)
constexpr int QN_NW = QN_T / 64;
constexpr int QN_MMAX = 12;    // history capacity (runtime M <= 12; the reference uses 10)
constexpr int QN_NV = 6 + 5 * QN_MMAX;

// F_ZC .. F_NCHEAP / SC_ALPHA1, SC_BETA: the line-search margin cache of the multi-block step
// (binary LogisticRegression, Armijo, no L1; glm.hip logreg_binary_pf_kernel reads F_ZMODE /
// F_ZSEL / SC_BETA): F_ZMODE is the mode of the NEXT evaluation — 0 full, 1 margins-only (a
// backtracking trial: loss from z0 + beta (z1 - z0)), 2 full at a point a margins-only trial
// already accepted; F_ZSEL selects which of the two margin buffers holds z0 (the accepted point).
// F_SKIPX: 1 while the next evaluation must not read X (margins-only, or the fit is done) — the
// skip word of the multinomial margin pass / X^T R pass (two-pass GLM)
enum { F_DONE = 0, F_STATUS, F_ITER, F_NEVAL, F_LS, F_COUNT, F_HEAD, F_STARTED, F_BRACKET, F_ZMODE, F_ZSEL,
       F_NCHEAP, F_ZC, F_SKIPX };
enum { ST_RUNNING = 0, ST_CONV_GRAD = 1, ST_CONV_F = 2, ST_MAXITER = 3, ST_LS_FAIL = 4 };
enum { SC_F = 0, SC_ALPHA, SC_DGINIT, SC_GAMMA, SC_GINF, SC_ALPHA1, SC_BETA };

}  // namespace

// Host-visible argument block (mirrored by a ctypes.Structure in ops/__init__.py)
struct QnArgs {
  long N;        // parameters: Kn + (K if fit_intercept else 0)
  long Kn;       // coefficients K * n
  int n, K, M, past, max_iter, max_ls, l1, wolfe;
  double tol, delta, inv_m, c1, c2;
  double *x, *g, *pg, *d, *xt, *gt;  // [N] each
  double *S, *Y;                     // [M][N]
  double *SY, *YY;                   // [M][M] slot-indexed s_i.y_j, y_i.y_j
  double *fh;                        // [past] objective history
  double *sc;                        // scalars
  const double *l2, *l1c;            // [N] penalty coefficients in optimiser coordinates
  const double *isg;                 // [n] 1 / sigma (0 for constant columns)
  int *fl;                           // int flags
  double *wb;                        // evaluation parameters [Kn | K] in the original space
  double *out;                       // summed evaluation [grad_w (Kn) | grad_b (K) | loss]
  long long *probe;                  // optional: wall-clock stamps of the kernel's sections (tuning)
};

// ------------------------------------------------------------------------------------------
// The pieces both forms of the step are built from. Each is the step's arithmetic or its
// decision, written once; where the operands come from (batched loads, registers loaded at kernel
// entry) and where a result is committed (the flags at once, or a record for a later launch) stay
// with the caller.
// ------------------------------------------------------------------------------------------

// Block-wide sums of NV per-thread values over NW waves: `red` takes the NV * NW wave partials,
// `tot` (LDS) the NV totals, valid for every thread on return (the totals are folded by NV threads,
// so no thread holds NV * NW LDS loads in registers).
template <int NW, int NV>
__device__ __forceinline__ void qn_block_sum(const double (&v)[NV], double* red, double* tot) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const double t = wave_sum(v[i]);
    if (lane == 0) red[i * NW + wid] = t;
    __builtin_amdgcn_sched_barrier(0);  // one reduction at a time: no NV-wide live DPP temporaries
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[threadIdx.x * NW + w];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
}

// OWL-QN pseudo-gradient of f + sum c_i |x_i|
__device__ __forceinline__ double pseudo_grad(double x, double g, double c) {
  if (c <= 0.0) return g;
  if (x > 0.0) return g + c;
  if (x < 0.0) return g - c;
  if (g + c < 0.0) return g + c;
  if (g - c > 0.0) return g - c;
  return 0.0;
}

// trial point of one element: t = x + alpha d, projected onto x's orthant where c > 0 (the L1
// coordinates; the caller passes c = 0 without L1)
__device__ __forceinline__ double qn_trial_value(double xv, double dv, double pv, double cv, double alpha) {
  double t = xv + alpha * dv;
  if (cv > 0.0) {
    const double orth = xv != 0.0 ? (xv > 0.0 ? 1.0 : -1.0) : (pv < 0.0 ? 1.0 : (pv > 0.0 ? -1.0 : 0.0));
    if (t * orth <= 0.0) t = 0.0;
  }
  return t;
}

// pass 0 of one element: returns its smooth gradient (summed evaluation value `ov`, optimiser
// coordinates) and leaves its terms of the L2 / L1 penalties, gt.d and pg.(xt - x) in `t`
__device__ __forceinline__ double qn_p0_terms(const QnArgs& A, double ov, double isg, double l2v, double l1v,
                                              double xv, double dv, double pv, double xo, double (&t)[4]) {
  const double gi = ov * A.inv_m * isg + l2v * xv;
  t[0] = l2v * xv * xv;
  t[1] = l1v * fabs(xv);
  t[2] = gi * dv;
  t[3] = pv * (xv - xo);
  return gi;
}

// pass 1 of one element: its pseudo-gradient and new pair s = xt - x, y = gt - g, and its terms of
// s.y, y.y, s.pg, y.pg, pg.pg and |pg| in `t`
struct QnPair {
  double sx, yx, pgi;
};

__device__ __forceinline__ QnPair qn_p1_terms(bool started, double xv, double gv, double xo, double go, double cv,
                                              double (&t)[6]) {
  const double sx = started ? xv - xo : 0.0;
  const double yx = started ? gv - go : 0.0;
  const double pgi = pseudo_grad(xv, gv, cv);
  t[0] = sx * yx;
  t[1] = yx * yx;
  t[2] = sx * pgi;
  t[3] = yx * pgi;
  t[4] = pgi * pgi;
  t[5] = fabs(pgi);
  return {sx, yx, pgi};
}

// ... and its terms of the products with one stored pair (S_j, Y_j): s.Y_j, S_j.y, y.Y_j, S_j.pg, Y_j.pg
__device__ __forceinline__ void qn_p1_slot_terms(double sx, double yx, double pgi, double Sj, double Yj,
                                                 double (&t)[5]) {
  t[0] = sx * Yj;
  t[1] = Sj * yx;
  t[2] = yx * Yj;
  t[3] = Sj * pgi;
  t[4] = Yj * pgi;
}

// Line-search decision on the objective `ft` at the trial point of step `alpha` (p02 = gt.d,
// p03 = pg.(xt - x) of pass 0; zc / zmode: the margin cache and the mode of this evaluation):
// accept, or the factor the step length takes for the next trial
struct QnLs {
  bool accept;
  double width;
};

__device__ __forceinline__ QnLs qn_ls_decide(const QnArgs& A, double ft, double f, double alpha, double dginit,
                                             double p02, double p03, bool bracket, bool zc, int zmode) {
  bool accept = true;
  double width = 1.0;
  if (zc && zmode == 2 && isfinite(ft)) {
    // a margins-only trial passed the test at this point: this full evaluation supplies its
    // gradient (and the exact loss), nothing is re-tested
  } else if (!isfinite(ft)) {
    accept = false;
    width = 0.5;
  } else {
    const double dgtest = A.l1 ? p03 : alpha * dginit;
    if (ft > f + A.c1 * dgtest) {
      // safeguarded quadratic interpolation through phi(0), phi'(0) alpha, phi(alpha)
      accept = false;
      const double den = 2.0 * (ft - f - dgtest);
      width = den > 0.0 ? -dgtest / den : 0.5;
      width = isfinite(width) ? fmin(0.5, fmax(0.1, width)) : 0.5;
    } else if (A.wolfe && !A.l1 && !bracket && p02 < A.c2 * dginit) {
      accept = false;
      width = 2.1;
    }
  }
  return {accept, width};
}

// The one-thread commits of the line search.
// the fit ends with `status`: the evaluations that may still be queued must not read X
__device__ __forceinline__ void qn_commit_done(int* fl, int status) {
  fl[F_STATUS] = status;
  fl[F_DONE] = 1;
  fl[F_SKIPX] = 1;
}

// margin cache: the mode of the next evaluation (margins-only evaluations do not read X)
__device__ __forceinline__ void qn_commit_zmode(int* fl, int zmode) {
  fl[F_ZMODE] = zmode;
  fl[F_SKIPX] = zmode == 1 ? 1 : 0;
}

// a rejected trial (its `ls`-th of this search, step alpha_tried): the search has failed, or the
// next trial runs at step `alpha`
__device__ __forceinline__ void qn_commit_reject(const QnArgs& A, int ls, int neval, double width, double alpha_tried,
                                                 double alpha, double ft, bool zc, int zmode, double alpha1) {
  int* fl = A.fl;
  fl[F_LS] = ls;
  fl[F_NEVAL] = neval;
  if (ls >= A.max_ls) {
    qn_commit_done(fl, ST_LS_FAIL);
    return;
  }
  if (width < 1.0) fl[F_BRACKET] = 1;
  A.sc[SC_ALPHA] = alpha;
  if (zc && isfinite(ft)) {
    // the rejected full evaluation's margins (at step alpha_tried) become z1; later trials of this
    // search are margins-only evaluations at beta = alpha / alpha1
    const double a1 = zmode == 0 ? alpha_tried : alpha1;
    A.sc[SC_ALPHA1] = a1;
    A.sc[SC_BETA] = alpha / a1;
    qn_commit_zmode(fl, 1);
  } else if (zc) {
    qn_commit_zmode(fl, 0);  // a non-finite loss: no trusted margins, the next trial runs in full
  }
}

// a trial accepted on margins only: the same point is evaluated in full next
__device__ __forceinline__ void qn_commit_margins_accept(int* fl, int neval) {
  fl[F_NEVAL] = neval;
  qn_commit_zmode(fl, 2);
}

// an accepted full evaluation: its margins (the other buffer) are the new accepted point's
__device__ __forceinline__ void qn_commit_margins_point(int* fl) {
  fl[F_ZSEL] ^= 1;
  qn_commit_zmode(fl, 0);
}

// The history in LDS: the Gram blocks s_i.y_j / y_i.y_j (slot-indexed), S^T pg / Y^T pg, the
// compact-form coefficients and the chronological slot list
struct QnHist {
  double sy[QN_MMAX * QN_MMAX], yy[QN_MMAX * QN_MMAX];
  double p1[QN_MMAX], p2[QN_MMAX];
  double cf_a[QN_MMAX], cf_t[QN_MMAX];
  int sl[QN_MMAX];
};

// what an accepted step decides; the caller commits it
struct QnUpd {
  int status, newp, cnt, hd, iter;
  double gamma;
};

// One thread: history bookkeeping and the convergence test of an accepted point with objective
// `fn` and max |pg| `ginf`. `tot`: the pass-1 totals [6 | 5 x QN_MMAX]; count / head / pre_iter /
// pre_gamma / fh_next: the pre-step state (fh_next = the objective `past` iterations back). Inserts
// the new pair's products into H.sy / H.yy (which hold the current blocks), fills H.p1 / H.p2 / H.sl.
__device__ __forceinline__ QnUpd qn_history_update(const QnArgs& A, QnHist& H, const double* tot, double ginf,
                                                   double fn, bool started, int count, int head, int pre_iter,
                                                   double pre_gamma, double fh_next) {
  const int M = A.M;
  int cnt = count, hd = head, status = ST_RUNNING;
  double gamma = started ? pre_gamma : 1.0;
  for (int j = 0; j < M; ++j) {
    H.p1[j] = tot[6 + 3 * QN_MMAX + j];
    H.p2[j] = tot[6 + 4 * QN_MMAX + j];
  }
  const double ys = tot[0], yy = tot[1];
  const bool newp = started && yy > 0.0 && ys > 1e-10 * yy;
  if (newp) {
    const int h = hd;
    for (int j = 0; j < M; ++j) {
      if (j == h) continue;
      H.sy[h * M + j] = tot[6 + j];
      H.sy[j * M + h] = tot[6 + QN_MMAX + j];
      H.yy[h * M + j] = tot[6 + 2 * QN_MMAX + j];
      H.yy[j * M + h] = tot[6 + 2 * QN_MMAX + j];
    }
    H.sy[h * M + h] = ys;
    H.yy[h * M + h] = yy;
    H.p1[h] = tot[2];
    H.p2[h] = tot[3];
    hd = (h + 1) % M;
    cnt = cnt < M ? cnt + 1 : M;
    gamma = ys / yy;
  }
  const int iter = pre_iter + (started ? 1 : 0);
  const double fmag = fmax(fabs(fn), A.tol);
  if (ginf <= A.tol * fmag) status = ST_CONV_GRAD;
  if (A.past > 0 && status == ST_RUNNING && started && iter >= A.past && fabs(fh_next - fn) <= A.delta * fmag)
    status = ST_CONV_F;
  if (status == ST_RUNNING && iter >= A.max_iter) status = ST_MAXITER;
  for (int c = 0; c < cnt; ++c) H.sl[c] = (hd - cnt + c + 2 * M) % M;
  return {status, newp ? 1 : 0, cnt, hd, iter, gamma};
}

// Wave 0: compact-form coefficients into H.cf_a / H.cf_t (slot-indexed, zero for unused slots),
// lane c = chronological pair c:
//      t = R^-1 p1 (back substitution), a = R^-T ((D + gamma YtY) t - gamma p2) (forward),
//      R_ce = s_c.y_e (c <= e); one broadcast + one FMA per lane per step
__device__ __forceinline__ void qn_compact_solve(QnHist& H, int M, int cnt, double gamma) {
  const int c = threadIdx.x;
  const bool act = c < cnt;
  const int slc = act ? H.sl[c] : 0;
  double Rrow[QN_MMAX], Rcol[QN_MMAX], Yrow[QN_MMAX], tv[QN_MMAX];
#pragma unroll
  for (int e = 0; e < QN_MMAX; ++e) {
    const bool ok = act && e < cnt;
    const int sle = ok ? H.sl[e] : 0;
    Rrow[e] = ok ? H.sy[slc * M + sle] : 0.0;
    Rcol[e] = ok ? H.sy[sle * M + slc] : 0.0;
    Yrow[e] = ok ? H.yy[slc * M + sle] : 0.0;
    tv[e] = 0.0;
  }
  const double diag = act ? H.sy[slc * M + slc] : 1.0;
  double acc = act ? H.p1[slc] : 0.0;
  double tmine = 0.0;
#pragma unroll
  for (int e = QN_MMAX - 1; e >= 0; --e) {
    if (e < cnt) {
      const double te = __shfl(acc / diag, e, 64);
      tv[e] = te;
      if (c == e) tmine = te;
      if (c < e) acc -= Rrow[e] * te;
    }
  }
  acc = diag * tmine - gamma * (act ? H.p2[slc] : 0.0);
#pragma unroll
  for (int e = 0; e < QN_MMAX; ++e) acc += gamma * Yrow[e] * tv[e];
  double amine = 0.0;
#pragma unroll
  for (int e = 0; e < QN_MMAX; ++e) {
    if (e < cnt) {
      const double ae = __shfl(acc / diag, e, 64);
      if (c == e) amine = ae;
      if (c > e) acc -= Rcol[e] * ae;
    }
  }
  if (c < QN_MMAX) {
    H.cf_a[c] = 0.0;
    H.cf_t[c] = 0.0;
  }
  __builtin_amdgcn_wave_barrier();
  if (act) {
    H.cf_a[slc] = amine;
    H.cf_t[slc] = gamma * tmine;
  }
}

// ------------------------------------------------------------------------------------------
// Single-block step: one block of QN_T threads walks the whole state.
// ------------------------------------------------------------------------------------------

// every thread takes the totals back into `v`; `red` holds NV * (QN_NW + 1) doubles
template <int NV>
__device__ __forceinline__ void qn_sum_all(double (&v)[NV], double* red) {
  qn_block_sum<QN_NW>(v, red, red + NV * QN_NW);
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = red[NV * QN_NW + i];
}

__device__ __forceinline__ double qn_max_all(double v, double* red) {
  v = wave_max(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = v;
  __syncthreads();
  double r = red[0];
#pragma unroll
  for (int w = 1; w < QN_NW; ++w) r = fmax(r, red[w]);
  __syncthreads();
  return r;
}

// Element loops: every thread owns i = tid + k * QN_T and handles QN_U of its elements per batch,
// issuing all of a batch's loads before any store (the state vectors are separate allocations, but
// the compiler cannot prove it, so without batching each element's loads would wait for the
// previous element's stores: one full memory latency per element).
constexpr int QN_U = 4;
#define QN_BATCH(i0) for (long i0 = threadIdx.x; i0 < A.N; i0 += (long)QN_T * QN_U)
#define QN_LANE(u, i0) const long i_##u = (i0) + (long)(u) * QN_T

// next trial point xt = x + alpha d (orthant-projected on L1 coordinates) and its evaluation params
__device__ void qn_set_trial(const QnArgs& A, double alpha) {
  QN_BATCH(i0) {
    double xv[QN_U], dv[QN_U], pv[QN_U], cv[QN_U], sv[QN_U];
#pragma unroll
    for (int u = 0; u < QN_U; ++u) {
      const long i = i0 + (long)u * QN_T;
      const bool ok = i < A.N;
      xv[u] = ok ? A.x[i] : 0.0;
      dv[u] = ok ? A.d[i] : 0.0;
      pv[u] = (ok && A.l1) ? A.pg[i] : 0.0;
      cv[u] = (ok && A.l1) ? A.l1c[i] : 0.0;
      sv[u] = (ok && i < A.Kn) ? A.isg[i % A.n] : 1.0;
    }
#pragma unroll
    for (int u = 0; u < QN_U; ++u) {
      const long i = i0 + (long)u * QN_T;
      if (i < A.N) {
        const double t = qn_trial_value(xv[u], dv[u], pv[u], cv[u], alpha);
        A.xt[i] = t;
        A.wb[i] = t * sv[u];
      }
    }
  }
}

#define QN_PROBE(k) \
  do { if (A.probe && threadIdx.x == 0) A.probe[k] = wall_clock64(); } while (0)

__device__ __forceinline__ void qn_step_body(const QnArgs& A) {
  __shared__ double red[QN_NV * (QN_NW + 1)];
  __shared__ QnHist H;
  __shared__ QnUpd s_u;
  __shared__ double s_v[QN_NV];
  int* fl = A.fl;
  if (fl[F_DONE]) return;
  QN_PROBE(0);
  const int tid = threadIdx.x;
  const long N = A.N, Kn = A.Kn;
  const int M = A.M;
  const double lossv = A.out[Kn + A.K];
  // optimiser scalars, loaded up front so their latency hides under pass 0
  const bool started = fl[F_STARTED] != 0;
  const int pre_iter = fl[F_ITER];
  const int count = fl[F_COUNT];
  const int head = fl[F_HEAD];
  const int pre_ls = fl[F_LS];
  const int pre_neval = fl[F_NEVAL];
  const bool bracket = fl[F_BRACKET] != 0;
  const double f = A.sc[SC_F];
  double alpha = A.sc[SC_ALPHA];
  const double dginit = A.sc[SC_DGINIT];
  const double pre_gamma = A.sc[SC_GAMMA];
  const double pre_fh_next = (A.past > 0 && started) ? A.fh[(pre_iter + 1) % A.past] : 0.0;
  // line-search margin cache (see the multi-block step K2): the mode of the evaluation just summed
  const bool zc = fl[F_ZC] != 0;
  const int zmode = zc ? fl[F_ZMODE] : 0;
  const double alpha1 = A.sc[SC_ALPHA1];

  // ---- pass 0: smooth gradient at xt (optimiser coordinates), penalties, directional terms
  double p0[4] = {0.0, 0.0, 0.0, 0.0};
  QN_BATCH(i0) {
    double xv[QN_U], ov[QN_U], sv[QN_U], l2v[QN_U], l1v[QN_U], dv[QN_U], pv[QN_U], xo[QN_U];
#pragma unroll
    for (int u = 0; u < QN_U; ++u) {
      const long i = i0 + (long)u * QN_T;
      const bool ok = i < N;
      xv[u] = ok ? A.xt[i] : 0.0;
      ov[u] = ok ? A.out[i] : 0.0;
      sv[u] = (ok && i < Kn) ? A.isg[i % A.n] : 1.0;
      l2v[u] = ok ? A.l2[i] : 0.0;
      l1v[u] = ok ? A.l1c[i] : 0.0;
      dv[u] = ok ? A.d[i] : 0.0;
      pv[u] = ok ? A.pg[i] : 0.0;
      xo[u] = ok ? A.x[i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < QN_U; ++u) {
      const long i = i0 + (long)u * QN_T;
      if (i < N) {
        double t[4];
        A.gt[i] = qn_p0_terms(A, ov[u], sv[u], l2v[u], l1v[u], xv[u], dv[u], pv[u], xo[u], t);
#pragma unroll
        for (int k = 0; k < 4; ++k) p0[k] += t[k];
      }
    }
  }
  qn_sum_all(p0, red);  // every read of `out` precedes this barrier
  QN_PROBE(1);
  for (long i = tid; i < Kn + A.K + 1; i += QN_T) A.out[i] = 0.0;
  const double ft = lossv * A.inv_m + 0.5 * p0[0] + p0[1];

  // ---- line search decision (uniform: every thread sees the same reduced values)
  if (tid == 0 && zc && zmode == 1) fl[F_NCHEAP] += 1;
  if (started) {
    const QnLs d = qn_ls_decide(A, ft, f, alpha, dginit, p0[2], p0[3], bracket, zc, zmode);
    if (!d.accept) {
      const int ls = pre_ls + 1;
      __syncthreads();
      const double alpha_tried = alpha;
      alpha *= d.width;
      if (ls < A.max_ls) qn_set_trial(A, alpha);
      if (tid == 0) qn_commit_reject(A, ls, pre_neval + 1, d.width, alpha_tried, alpha, ft, zc, zmode, alpha1);
      return;
    }
    if (zc && zmode == 1) {
      if (tid == 0) qn_commit_margins_accept(fl, pre_neval + 1);
      return;
    }
  }
  if (tid == 0 && zc) qn_commit_margins_point(fl);

  // ---- accepted: pass 1 — pseudo-gradient at xt and every dot product of the compact form
  // 1a: pseudo-gradient at xt, new pair s = xt - x, y = gt - g (kept in the free d / wb buffers for
  //     the next passes), and s.y, y.y, s.pg, y.pg, pg.pg, max |pg|
  double v5[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double ginf = 0.0;
  QN_BATCH(i0) {
    double xv[QN_U], gv[QN_U], xo[QN_U], go[QN_U], cv[QN_U];
#pragma unroll
    for (int u = 0; u < QN_U; ++u) {
      const long i = i0 + (long)u * QN_T;
      const bool ok = i < N;
      xv[u] = ok ? A.xt[i] : 0.0;
      gv[u] = ok ? A.gt[i] : 0.0;
      xo[u] = ok ? A.x[i] : 0.0;
      go[u] = ok ? A.g[i] : 0.0;
      cv[u] = (ok && A.l1) ? A.l1c[i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < QN_U; ++u) {
      const long i = i0 + (long)u * QN_T;
      if (i < N) {
        double t[6];
        const QnPair e = qn_p1_terms(started, xv[u], gv[u], xo[u], go[u], cv[u], t);
        A.pg[i] = e.pgi;
        A.d[i] = e.sx;
        A.wb[i] = e.yx;
        ginf = fmax(ginf, t[5]);
#pragma unroll
        for (int k = 0; k < 5; ++k) v5[k] += t[k];
      }
    }
  }
  // stage the history Gram blocks in LDS: the serial small solve below must not chase global loads
  for (int i = tid; i < M * M; i += QN_T) {
    H.sy[i] = A.SY[i];
    H.yy[i] = A.YY[i];
  }
  qn_sum_all(v5, red);
  QN_PROBE(2);
  ginf = qn_max_all(ginf, red);
  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < 6; ++j) s_v[j] = v5[j];
  }
  // 1b: products with the stored pairs, QN_JB history slots per sweep (bounded register set)
  constexpr int QN_JB = 5;
  constexpr int QN_UB = 2;
  for (int j0 = 0; j0 < M; j0 += QN_JB) {
    double w[5 * QN_JB];
#pragma unroll
    for (int q = 0; q < 5 * QN_JB; ++q) w[q] = 0.0;
    for (long i0 = tid; i0 < N; i0 += (long)QN_T * QN_UB) {
      double sv[QN_UB], yv[QN_UB], pv[QN_UB], Sv[QN_UB][QN_JB], Yv[QN_UB][QN_JB];
#pragma unroll
      for (int u = 0; u < QN_UB; ++u) {
        const long i = i0 + (long)u * QN_T;
        const bool ok = i < N;
        sv[u] = ok ? A.d[i] : 0.0;
        yv[u] = ok ? A.wb[i] : 0.0;
        pv[u] = ok ? A.pg[i] : 0.0;
#pragma unroll
        for (int jj = 0; jj < QN_JB; ++jj) {
          const bool okj = ok && (j0 + jj < M);
          Sv[u][jj] = okj ? A.S[(long)(j0 + jj) * N + i] : 0.0;
          Yv[u][jj] = okj ? A.Y[(long)(j0 + jj) * N + i] : 0.0;
        }
      }
#pragma unroll
      for (int u = 0; u < QN_UB; ++u)
#pragma unroll
        for (int jj = 0; jj < QN_JB; ++jj) {
          double t[5];
          qn_p1_slot_terms(sv[u], yv[u], pv[u], Sv[u][jj], Yv[u][jj], t);
#pragma unroll
          for (int k = 0; k < 5; ++k) w[5 * jj + k] += t[k];
        }
    }
    qn_sum_all(w, red);
    if (tid == 0) {
#pragma unroll
      for (int jj = 0; jj < QN_JB; ++jj) {
        const int j = j0 + jj;
        if (j < M) {
          s_v[6 + j] = w[5 * jj + 0];
          s_v[6 + QN_MMAX + j] = w[5 * jj + 1];
          s_v[6 + 2 * QN_MMAX + j] = w[5 * jj + 2];
          s_v[6 + 3 * QN_MMAX + j] = w[5 * jj + 3];
          s_v[6 + 4 * QN_MMAX + j] = w[5 * jj + 4];
        }
      }
    }
  }

  QN_PROBE(3);
  // ---- lane 0: history bookkeeping and convergence (LDS + prefetched scalars only), committed at once
  if (tid == 0) {
    const QnUpd u = qn_history_update(A, H, s_v, ginf, ft, started, count, head, pre_iter, pre_gamma, pre_fh_next);
    s_u = u;
    if (A.past > 0) A.fh[u.iter % A.past] = ft;
    fl[F_ITER] = u.iter;
    fl[F_HEAD] = u.hd;
    fl[F_COUNT] = u.cnt;
    fl[F_NEVAL] = pre_neval + 1;
    fl[F_LS] = 0;
    fl[F_BRACKET] = 0;
    fl[F_STARTED] = 1;
    A.sc[SC_F] = ft;
    A.sc[SC_GAMMA] = u.gamma;
    A.sc[SC_GINF] = ginf;
  }
  __syncthreads();
  if (tid < 64) qn_compact_solve(H, M, s_u.cnt, s_u.gamma);
  __syncthreads();
  if (s_u.newp) {
    for (int i = tid; i < M * M; i += QN_T) {
      A.SY[i] = H.sy[i];
      A.YY[i] = H.yy[i];
    }
  }
  __syncthreads();
  const int status = s_u.status;
  const bool newp = s_u.newp != 0;
  const int cnt = s_u.cnt;
  const double gamma = s_u.gamma;
  QN_PROBE(4);

  // ---- pass 2: store the pair, x <- xt, g <- gt, direction d = -H pg
  double p2v[2] = {0.0, 0.0};
  QN_BATCH(i0) {
    double xv[QN_U], gv[QN_U], sv[QN_U], yv[QN_U], pv[QN_U], cv[QN_U];
#pragma unroll
    for (int u = 0; u < QN_U; ++u) {
      const long i = i0 + (long)u * QN_T;
      const bool ok = i < N;
      xv[u] = ok ? A.xt[i] : 0.0;
      gv[u] = ok ? A.gt[i] : 0.0;
      sv[u] = ok ? A.d[i] : 0.0;
      yv[u] = ok ? A.wb[i] : 0.0;
      pv[u] = ok ? A.pg[i] : 0.0;
      cv[u] = (ok && A.l1) ? A.l1c[i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < QN_U; ++u) {
      const long i = i0 + (long)u * QN_T;
      if (i < N) {
        if (newp) {
          A.S[(long)head * N + i] = sv[u];
          A.Y[(long)head * N + i] = yv[u];
        }
        A.x[i] = xv[u];
        A.g[i] = gv[u];
      }
    }
    if (status == ST_RUNNING) {
      double hg[QN_U];
#pragma unroll
      for (int u = 0; u < QN_U; ++u) hg[u] = gamma * pv[u];
      constexpr int QN_G = 4;  // history slots whose loads are in flight together
      for (int c0 = 0; c0 < cnt; c0 += QN_G) {
        double Sv[QN_G][QN_U], Yv[QN_G][QN_U], ca[QN_G], ct[QN_G];
#pragma unroll
        for (int q = 0; q < QN_G; ++q) {
          const bool okq = c0 + q < cnt;
          const int j = okq ? H.sl[c0 + q] : 0;
          ca[q] = okq ? H.cf_a[j] : 0.0;
          ct[q] = okq ? H.cf_t[j] : 0.0;
#pragma unroll
          for (int u = 0; u < QN_U; ++u) {
            const long i = i0 + (long)u * QN_T;
            const bool ok = okq && i < N;
            Sv[q][u] = ok ? A.S[(long)j * N + i] : 0.0;
            Yv[q][u] = ok ? A.Y[(long)j * N + i] : 0.0;
          }
        }
#pragma unroll
        for (int q = 0; q < QN_G; ++q)
#pragma unroll
          for (int u = 0; u < QN_U; ++u) hg[u] += ca[q] * Sv[q][u] - ct[q] * Yv[q][u];
      }
#pragma unroll
      for (int u = 0; u < QN_U; ++u) {
        const long i = i0 + (long)u * QN_T;
        if (i < N) {
          double di = -hg[u];
          if (cv[u] > 0.0 && di * pv[u] >= 0.0) di = 0.0;
          A.d[i] = di;
          p2v[0] += pv[u] * di;
          p2v[1] += di * di;
        }
      }
    }
  }
  if (status != ST_RUNNING) {
    if (tid == 0) qn_commit_done(fl, status);
    return;
  }
  QN_PROBE(5);
  qn_sum_all(p2v, red);
  double dg = p2v[0], dd = p2v[1];
  int cnt2 = cnt;
  if (!(dg < 0.0)) {  // not a descent direction: drop the history, steepest descent
    for (long i = tid; i < N; i += QN_T) A.d[i] = -A.pg[i];  // rare
    dg = -s_v[4];
    dd = s_v[4];
    cnt2 = 0;
    __syncthreads();
  }
  // ---- pass 3: next trial point (first iteration / after a reset: alpha = 1 / ||d||)
  alpha = cnt2 == 0 ? 1.0 / fmax(sqrt(dd), 1e-300) : 1.0;
  QN_PROBE(6);
  qn_set_trial(A, alpha);
  QN_PROBE(7);
  if (tid == 0) {
    if (cnt2 == 0) {
      fl[F_COUNT] = 0;
      A.sc[SC_GAMMA] = 1.0;
    }
    A.sc[SC_ALPHA] = alpha;
    A.sc[SC_DGINIT] = dg;
  }
}

__global__ __launch_bounds__(QN_T) void qn_step_kernel(QnArgs A) { qn_step_body(A); }

// hyper-parameter batching: one block per independent problem, args array in device memory
__global__ __launch_bounds__(QN_T) void qn_step_batch_kernel(const QnArgs* __restrict__ args) {
  const QnArgs A = args[blockIdx.x];
  qn_step_body(A);
}

SRML_API int srml_qn_step_batch(const QnArgs* args_dev, int count, hipStream_t stream) {
  if (count <= 0) return 0;
  hipLaunchKernelGGL(qn_step_batch_kernel, dim3((unsigned)count), dim3(QN_T), 0, stream, args_dev);
  return srml_status();
}

SRML_API int srml_qn_step(const QnArgs* a, hipStream_t stream) {
  if (a->M < 1 || a->M > QN_MMAX || a->N <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(qn_step_kernel, dim3(1), dim3(QN_T), 0, stream, *a);
  return srml_status();
}

SRML_API int srml_qn_max_history() { return QN_MMAX; }
SRML_API long srml_qn_args_size() { return (long)sizeof(QnArgs); }

// ------------------------------------------------------------------------------------------
// Multi-block step (one problem): the single-block step above spends ~40 us walking ~1.7 MB of
// optimiser state (x, g, pg, d, xt, gt and the S / Y history) through ONE CU. Here the same state
// machine runs as four launches over G blocks of 256 threads (element i belongs to one thread of
// one block), the kernel boundaries standing in for grid barriers:
//   K1  pass 0 (gt, penalty / directional partials); pre-step scalars snapshotted to scratch;
//   K2  every block reduces K1's partials (block order: all blocks see the same bits) and takes the
//       same line-search decision; reject -> its share of the next trial point (block 0 updates
//       the flags); accept -> pass 1 (pg, s, y and every compact-form dot product) partials;
//   K3  every block reduces them, repeats the bookkeeping / convergence test / compact-form solve
//       redundantly (identical inputs, identical results), stores its share of the new pair,
//       x <- xt, g <- gt and the direction, and leaves the p.d / d.d partials;
//   K4  reduce, descent check, its share of the next trial point; block 0 commits the optimiser
//       scalars, flags and history Gram blocks (deferred so no block of K3 reads state another
//       block of K3 already advanced).
// Same arithmetic as the single-block step except the summation order of the reductions.
// ------------------------------------------------------------------------------------------
namespace {

constexpr int MB_T = 256;
constexpr int MB_NW = MB_T / 64;
constexpr int MB_GMAX = 64;
constexpr int MBF_E = 32;      // elements per block of the folding K1 (qn_mb1f_kernel)
constexpr int MB_GAMAX = 512;  // K1 partial rows: the folding K1 runs ceil(N / MBF_E) blocks
constexpr int MB_PW = 6 + 5 * QN_MMAX + 1;  // pass-1 partials: 6 dots, 5 history products per slot, max |pg|
enum {
  S_STARTED = 0, S_ITER, S_COUNT, S_HEAD, S_LS, S_NEVAL, S_BRACKET, S_F, S_ALPHA, S_DGINIT, S_GAMMA, S_FHN, S_LOSS,
  S_ZMODE, S_ZC, S_ALPHA1,
  S_PHASE = 16, S_STATUS, S_NEWP, S_CNT, S_HD, S_GAM, S_FT, S_GINF, S_ITERN, S_FN,
  S_CF = 32,                              // cf_a[QN_MMAX] | cf_t[QN_MMAX]
  S_SL = S_CF + 2 * QN_MMAX,              // chronological slots [QN_MMAX]
  S_SY = S_SL + QN_MMAX,                  // updated SY [QN_MMAX^2] | YY [QN_MMAX^2] (committed by K4)
  S_PA = S_SY + 2 * QN_MMAX * QN_MMAX,    // K1 partials [G1][4]
  S_PB = S_PA + 4 * MB_GAMAX,             // K2 partials [G][MB_PW]
  S_PC = S_PB + MB_PW * MB_GMAX,          // K3 partials [G][2]
  S_END = S_PC + 2 * MB_GMAX
};

// grid totals of a [G][width] partial table (width <= MB_T) into LDS `tot` (all threads). Every
// thread of the block loads: slice s = tid / width of the blocks, eight independent loads in flight
// per thread, then an LDS combine of the slices in fixed order — the partials come from other CUs
// (L2 / fabric latency ~1 us each), so a one-thread-per-column serial loop over G blocks costs
// ~G us; this costs ~ceil(G / (8 * slices)) round trips.
__device__ __forceinline__ void mb_grid_sum(const double* part, int G, int width, double* tot, bool max_last) {
  __shared__ double gs[MB_T];
  const int t = threadIdx.x, S = MB_T / width;
  const int j = t % width, sl = t / width;
  const bool mx = max_last && j == width - 1;
  double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (sl < S) {
    int b = sl;
    for (; b + 7 * S < G; b += 8 * S) {
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = part[(long)(b + k * S) * width + j];
#pragma unroll
      for (int k = 0; k < 8; ++k) a[k] = mx ? fmax(a[k], v[k]) : a[k] + v[k];
    }
    for (; b < G; b += S) {
      const double v = part[(long)b * width + j];
      a[0] = mx ? fmax(a[0], v) : a[0] + v;
    }
  }
  gs[t] = mx ? fmax(fmax(fmax(a[0], a[1]), fmax(a[2], a[3])), fmax(fmax(a[4], a[5]), fmax(a[6], a[7])))
             : ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  if (t < width) {
    double x = gs[t];
    for (int q = 1; q < S; ++q) x = mx ? fmax(x, gs[q * width + t]) : x + gs[q * width + t];
    tot[t] = x;
  }
  __syncthreads();
}

}  // namespace

// Each kernel issues EVERY load it may need at entry (element data, history columns, grid
// partials, snapshot scalars), before its early exits and decisions: what the previous launch wrote
// comes from beyond this CU's caches (~1 us per round trip), so the kernel's time is its count of
// DEPENDENT round trips — one here, plus the boundary.

// pre-step snapshot of the flags / scalars (block 0, thread 0 of K1): later kernels read these,
// K2 / K4 rewrite the flags
struct MbSnap {
  int started, iter, count, head, ls, neval, bracket, zmode, zc;
  double f, alpha, dginit, gamma, alpha1;
};

__device__ __forceinline__ MbSnap mb_snap_load(const QnArgs& A) {
  const int* fl = A.fl;
  MbSnap q;
  q.started = fl[F_STARTED];
  q.iter = fl[F_ITER];
  q.count = fl[F_COUNT];
  q.head = fl[F_HEAD];
  q.ls = fl[F_LS];
  q.neval = fl[F_NEVAL];
  q.bracket = fl[F_BRACKET];
  q.f = A.sc[SC_F];
  q.alpha = A.sc[SC_ALPHA];
  q.dginit = A.sc[SC_DGINIT];
  q.gamma = A.sc[SC_GAMMA];
  q.zc = fl[F_ZC];
  q.zmode = q.zc ? fl[F_ZMODE] : 0;
  q.alpha1 = A.sc[SC_ALPHA1];
  return q;
}

__device__ __forceinline__ void mb_snap_store(const QnArgs& A, const MbSnap& q, double* scr) {
  scr[S_STARTED] = q.started ? 1.0 : 0.0;
  scr[S_ITER] = q.iter;
  scr[S_COUNT] = q.count;
  scr[S_HEAD] = q.head;
  scr[S_LS] = q.ls;
  scr[S_NEVAL] = q.neval;
  scr[S_BRACKET] = q.bracket;
  scr[S_F] = q.f;
  scr[S_ALPHA] = q.alpha;
  scr[S_DGINIT] = q.dginit;
  scr[S_GAMMA] = q.gamma;
  scr[S_FHN] = (A.past > 0 && q.started) ? A.fh[(q.iter + 1) % A.past] : 0.0;
  scr[S_ZMODE] = q.zmode;
  scr[S_ZC] = q.zc;
  scr[S_ALPHA1] = q.alpha1;
  scr[S_PHASE] = 0.0;
}

// pass 0 of element i from its summed evaluation value `ov`
struct MbP0In {
  double xv, l2v, l1v, dv, pgv, xo, isg;
};

__device__ __forceinline__ MbP0In mb_p0_load(const QnArgs& A, long i, bool own) {
  MbP0In e{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  if (own) {
    e.xv = A.xt[i];
    e.l2v = A.l2[i];
    e.l1v = A.l1c[i];
    e.dv = A.d[i];
    e.pgv = A.pg[i];
    e.xo = A.x[i];
    if (i < A.Kn) e.isg = A.isg[i % A.n];
  }
  return e;
}

__device__ __forceinline__ void mb_p0(const QnArgs& A, long i, bool own, const MbP0In& e, double ov, double (&p0)[4]) {
  if (own) A.gt[i] = qn_p0_terms(A, ov, e.isg, e.l2v, e.l1v, e.xv, e.dv, e.pgv, e.xo, p0);
}

__global__ __launch_bounds__(MB_T) void qn_mb1_kernel(QnArgs A, double* __restrict__ scr) {
  __shared__ double red[4 * MB_NW], tot[4];
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  const long i = (long)blockIdx.x * MB_T + threadIdx.x;
  const bool own = i < A.N;
  const int done = A.fl[F_DONE];
  MbSnap q{};
  double loss = 0.0;
  if (first) {
    q = mb_snap_load(A);
    loss = A.out[A.Kn + A.K];
  }
  const MbP0In e = mb_p0_load(A, i, own);
  const double ov = own ? A.out[i] : 0.0;
  if (done) {
    if (first) scr[S_PHASE] = 0.0;  // K3 / K4 must not act on a stale phase
    return;
  }
  if (first) {
    mb_snap_store(A, q, scr);
    scr[S_LOSS] = loss;
  }
  double p0[4] = {0.0, 0.0, 0.0, 0.0};
  mb_p0(A, i, own, e, ov, p0);
  if (own && i < A.Kn + A.K) A.out[i] = 0.0;  // this element's evaluation sum is consumed
  qn_block_sum<MB_NW>(p0, red, tot);
  if (threadIdx.x < 4) scr[S_PA + blockIdx.x * 4 + threadIdx.x] = tot[threadIdx.x];
}

// trial point of element i and its evaluation parameter
__device__ __forceinline__ void mb_trial(const QnArgs& A, long i, double xv, double dv, double pv, double cv,
                                         double isg, double alpha) {
  const double t = qn_trial_value(xv, dv, pv, A.l1 ? cv : 0.0, alpha);
  A.xt[i] = t;
  A.wb[i] = t * isg;
}

__global__ __launch_bounds__(MB_T) void qn_mb2_kernel(QnArgs A, double* __restrict__ scr, int ga) {
  __shared__ double red[MB_PW * MB_NW], p0[4];
  int* fl = A.fl;
  const int M = A.M;
  const long N = A.N;
  const long i = (long)blockIdx.x * MB_T + threadIdx.x;
  const bool own = i < N;
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  // ---- every load up front
  const int done = fl[F_DONE];
  const bool started = scr[S_STARTED] != 0.0;
  const double f = scr[S_F], dginit = scr[S_DGINIT], alpha0 = scr[S_ALPHA], loss = scr[S_LOSS];
  const bool bracket = scr[S_BRACKET] != 0.0;
  const int pre_ls = (int)scr[S_LS], pre_neval = (int)scr[S_NEVAL];
  const bool zc = scr[S_ZC] != 0.0;
  const int zmode = (int)scr[S_ZMODE];
  const double alpha1 = scr[S_ALPHA1];
  double xt = 0.0, gt = 0.0, xo = 0.0, go = 0.0, cv = 0.0, dv = 0.0, pv = 0.0, isg = 1.0;
  double Sv[QN_MMAX], Yv[QN_MMAX];
  if (own) {
    xt = A.xt[i];
    gt = A.gt[i];
    xo = A.x[i];
    go = A.g[i];
    cv = A.l1c[i];
    dv = A.d[i];
    pv = A.pg[i];
    if (i < A.Kn) isg = A.isg[i % A.n];
  }
#pragma unroll
  for (int j = 0; j < QN_MMAX; ++j) {
    Sv[j] = (own && j < M) ? A.S[(long)j * N + i] : 0.0;
    Yv[j] = (own && j < M) ? A.Y[(long)j * N + i] : 0.0;
  }
  if (done) return;
  mb_grid_sum(scr + S_PA, ga, 4, p0, false);  // ga: K1's block count
  double alpha = alpha0;
  const double ft = loss * A.inv_m + 0.5 * p0[0] + p0[1];
  if (first)  // the loss sum (read from the snapshot) and bias sums without a parameter (no intercept)
    for (long j = N; j < A.Kn + A.K + 1; ++j) A.out[j] = 0.0;
  if (first && zc && zmode == 1) fl[F_NCHEAP] += 1;
  if (started) {
    const QnLs d = qn_ls_decide(A, ft, f, alpha, dginit, p0[2], p0[3], bracket, zc, zmode);
    if (!d.accept) {
      const int ls = pre_ls + 1;
      alpha *= d.width;
      if (ls < A.max_ls && own) mb_trial(A, i, xo, dv, pv, cv, isg, alpha);
      if (first) qn_commit_reject(A, ls, pre_neval + 1, d.width, alpha0, alpha, ft, zc, zmode, alpha1);
      return;
    }
    if (zc && zmode == 1) {
      if (first) qn_commit_margins_accept(fl, pre_neval + 1);
      return;
    }
  }
  if (first) {
    scr[S_PHASE] = 1.0;
    scr[S_FT] = ft;
    if (zc) qn_commit_margins_point(fl);
  }
  // accepted: pass 1 partials of this block's elements
  double v[MB_PW];
#pragma unroll
  for (int j = 0; j < MB_PW; ++j) v[j] = 0.0;
  if (own) {
    double t[6];
    const QnPair e = qn_p1_terms(started, xt, gt, xo, go, A.l1 ? cv : 0.0, t);
    A.pg[i] = e.pgi;
    A.d[i] = e.sx;
    A.wb[i] = e.yx;
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = t[k];
    v[MB_PW - 1] = t[5];
#pragma unroll
    for (int j = 0; j < QN_MMAX; ++j) {
      double h[5];
      qn_p1_slot_terms(e.sx, e.yx, e.pgi, Sv[j], Yv[j], h);
#pragma unroll
      for (int k = 0; k < 5; ++k) v[6 + k * QN_MMAX + j] = h[k];
    }
  }
  // block sums (the last entry is a max); history slots >= M are zero and skipped
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < MB_PW - 1; ++j) {
    const bool live = j < 6 || ((j - 6) % QN_MMAX) < M;
    const double t = live ? wave_sum(v[j]) : 0.0;
    if (lane == 0) red[j * MB_NW + wid] = t;
    __builtin_amdgcn_sched_barrier(0);
  }
  {
    const double mx = wave_max(v[MB_PW - 1]);
    if (lane == 0) red[(MB_PW - 1) * MB_NW + wid] = mx;
  }
  __syncthreads();
  if (threadIdx.x < MB_PW) {
    const int j = threadIdx.x;
    double s = 0.0;
    for (int w = 0; w < MB_NW; ++w)
      s = j == MB_PW - 1 ? fmax(s, red[j * MB_NW + w]) : s + red[j * MB_NW + w];
    scr[S_PB + (long)blockIdx.x * MB_PW + j] = s;
  }
}

__global__ __launch_bounds__(MB_T) void qn_mb3_kernel(QnArgs A, double* __restrict__ scr) {
  __shared__ double tot[MB_PW], red[2 * MB_NW], t2[2];
  __shared__ QnHist H;
  __shared__ QnUpd s_u;
  const int G = gridDim.x, M = A.M, tid = threadIdx.x;
  const long N = A.N;
  const long i = (long)blockIdx.x * MB_T + tid;
  const bool own = i < N;
  // ---- every load up front
  const double phase = scr[S_PHASE];
  const bool started = scr[S_STARTED] != 0.0;
  const int pre_count = (int)scr[S_COUNT], head = (int)scr[S_HEAD], pre_iter = (int)scr[S_ITER];
  const double pre_gamma = scr[S_GAMMA], fn = scr[S_FT], fhn = scr[S_FHN];
  // K4's block 0 commits the updated blocks: every block reads the old ones here
  const double sy0 = tid < M * M ? A.SY[tid] : 0.0, yy0 = tid < M * M ? A.YY[tid] : 0.0;
  double xt = 0.0, gt = 0.0, sv = 0.0, yv = 0.0, pv = 0.0, cv = 0.0;
  double Sv[QN_MMAX], Yv[QN_MMAX];
  if (own) {
    xt = A.xt[i];
    gt = A.gt[i];
    sv = A.d[i];
    yv = A.wb[i];
    pv = A.pg[i];
    cv = A.l1c[i];
  }
#pragma unroll
  for (int j = 0; j < QN_MMAX; ++j) {
    Sv[j] = (own && j < M) ? A.S[(long)j * N + i] : 0.0;
    Yv[j] = (own && j < M) ? A.Y[(long)j * N + i] : 0.0;
  }
  if (phase != 1.0) return;
  if (tid < M * M) {
    H.sy[tid] = sy0;
    H.yy[tid] = yy0;
  }
  mb_grid_sum(scr + S_PB, G, MB_PW, tot, true);  // (its barriers also publish H.sy / H.yy)
  if (tid == 0) {
    const double ginf = tot[MB_PW - 1];
    const QnUpd u = qn_history_update(A, H, tot, ginf, fn, started, pre_count, head, pre_iter, pre_gamma, fhn);
    s_u = u;
    if (blockIdx.x == 0) {  // the commit record for K4
      scr[S_STATUS] = u.status;
      scr[S_NEWP] = u.newp ? 1.0 : 0.0;
      scr[S_CNT] = u.cnt;
      scr[S_HD] = u.hd;
      scr[S_GAM] = u.gamma;
      scr[S_GINF] = ginf;
      scr[S_ITERN] = u.iter;
      scr[S_FN] = fn;
    }
  }
  __syncthreads();
  if (tid < 64) qn_compact_solve(H, M, s_u.cnt, s_u.gamma);  // wave 0, as the single-block step
  __syncthreads();
  const int status = s_u.status;
  const bool newp = s_u.newp != 0;
  const double gamma = s_u.gamma;
  if (blockIdx.x == 0 && newp)  // staged for K4 (other blocks of this launch still read A.SY / A.YY)
    for (int k = tid; k < M * M; k += MB_T) {
      scr[S_SY + k] = H.sy[k];
      scr[S_SY + QN_MMAX * QN_MMAX + k] = H.yy[k];
    }
  // pass 2: store the pair, x <- xt, g <- gt, direction (inactive slots have zero coefficients)
  double p2v[2] = {0.0, 0.0};
  if (own) {
    if (newp) {
      A.S[(long)head * N + i] = sv;
      A.Y[(long)head * N + i] = yv;
    }
    A.x[i] = xt;
    A.g[i] = gt;
    if (status == ST_RUNNING) {
      double hg = gamma * pv;
#pragma unroll
      for (int j = 0; j < QN_MMAX; ++j) {
        if (j < M) {
          const bool fresh = newp && j == head;  // the pair stored just above
          hg += H.cf_a[j] * (fresh ? sv : Sv[j]) - H.cf_t[j] * (fresh ? yv : Yv[j]);
        }
      }
      double di = -hg;
      if (A.l1 && cv > 0.0 && di * pv >= 0.0) di = 0.0;
      A.d[i] = di;
      p2v[0] = pv * di;
      p2v[1] = di * di;
    }
  }
  qn_block_sum<MB_NW>(p2v, red, t2);
  if (tid < 2) scr[S_PC + blockIdx.x * 2 + tid] = t2[tid];
}

__global__ __launch_bounds__(MB_T) void qn_mb4_kernel(QnArgs A, double* __restrict__ scr) {
  __shared__ double p2[2], pbt[MB_PW];
  const int G = gridDim.x, M = A.M, tid = threadIdx.x;
  const bool first = blockIdx.x == 0 && tid == 0;
  const long i = (long)blockIdx.x * MB_T + tid;
  const bool own = i < A.N;
  int* fl = A.fl;
  // ---- every load up front
  const double phase = scr[S_PHASE];
  const int status = (int)scr[S_STATUS];
  const bool newp = scr[S_NEWP] != 0.0;
  const int cnt0 = (int)scr[S_CNT];
  double sy = 0.0, yy = 0.0;
  if (blockIdx.x == 0 && tid < M * M) {
    sy = scr[S_SY + tid];
    yy = scr[S_SY + QN_MMAX * QN_MMAX + tid];
  }
  double xv = 0.0, dv = 0.0, pv = 0.0, cv = 0.0, isg = 1.0;
  if (own) {
    xv = A.x[i];
    dv = A.d[i];
    pv = A.pg[i];
    cv = A.l1c[i];
    if (i < A.Kn) isg = A.isg[i % A.n];
  }
  if (phase != 1.0) return;
  if (blockIdx.x == 0) {  // commit the step's history blocks and scalars
    if (newp && tid < M * M) {
      A.SY[tid] = sy;
      A.YY[tid] = yy;
    }
    if (tid == 0) {
      const int iter = (int)scr[S_ITERN];
      if (A.past > 0) A.fh[iter % A.past] = scr[S_FN];
      fl[F_ITER] = iter;
      fl[F_HEAD] = (int)scr[S_HD];
      fl[F_COUNT] = cnt0;
      fl[F_NEVAL] = (int)scr[S_NEVAL] + 1;
      fl[F_LS] = 0;
      fl[F_BRACKET] = 0;
      fl[F_STARTED] = 1;
      A.sc[SC_F] = scr[S_FN];
      A.sc[SC_GAMMA] = scr[S_GAM];
      A.sc[SC_GINF] = scr[S_GINF];
    }
  }
  if (status != ST_RUNNING) {
    if (first) qn_commit_done(fl, status);
    return;
  }
  mb_grid_sum(scr + S_PC, G, 2, p2, false);
  double dg = p2[0], dd = p2[1];
  int cnt2 = cnt0;
  if (!(dg < 0.0)) {  // not a descent direction: drop the history, steepest descent (rare)
    mb_grid_sum(scr + S_PB, G, MB_PW, pbt, true);  // pg.pg is in the K2 partials
    const double pp = pbt[4];
    dv = -pv;
    if (own) A.d[i] = dv;
    dg = -pp;
    dd = pp;
    cnt2 = 0;
  }
  const double alpha = cnt2 == 0 ? 1.0 / fmax(sqrt(dd), 1e-300) : 1.0;
  if (own) mb_trial(A, i, xv, dv, pv, cv, isg, alpha);
  if (first) {
    if (cnt2 == 0) {
      fl[F_COUNT] = 0;
      A.sc[SC_GAMMA] = 1.0;
    }
    A.sc[SC_ALPHA] = alpha;
    A.sc[SC_DGINIT] = dg;
  }
}

// doubles of scratch the multi-block step needs (independent of N)
SRML_API long srml_qn_mb_scratch() { return (long)S_END; }

// One optimiser step as four G-block launches (G = ceil(N / 256) <= 64; larger problems use the
// single-block step). `scratch`: srml_qn_mb_scratch() doubles owned by this problem.
SRML_API int srml_qn_step_mb(const QnArgs* a, double* scratch, hipStream_t stream) {
  if (a->M < 1 || a->M > QN_MMAX || a->N <= 0 || !scratch) return (int)hipErrorInvalidValue;
  const long G = (a->N + MB_T - 1) / MB_T;
  if (G > MB_GMAX) return srml_qn_step(a, stream);
  const dim3 grid((unsigned)G), blk(MB_T);
  hipLaunchKernelGGL(qn_mb1_kernel, grid, blk, 0, stream, *a, scratch);
  hipLaunchKernelGGL(qn_mb2_kernel, grid, blk, 0, stream, *a, scratch, (int)G);
  hipLaunchKernelGGL(qn_mb3_kernel, grid, blk, 0, stream, *a, scratch);
  hipLaunchKernelGGL(qn_mb4_kernel, grid, blk, 0, stream, *a, scratch);
  return srml_status();
}

// Fold of the binary evaluation's fp32 partial gradient rows for this block's MBF_E elements
// (columns blockIdx.x * MBF_E ...): 8 lanes x float4 per row, 32 row groups, 8 rows in flight per
// thread; the bias element and the loss are the trailing doubles of every row (summed by the
// block owning element Kn / the last block). Returns the element's sum in `oval` and the block's
// loss contribution in `lpart`.
__device__ __forceinline__ void mbf_fold_block(const QnArgs& A, const float* __restrict__ fws, int parts, long wst,
                                              double (*fold)[33], double* red, bool own, long i, unsigned G,
                                              double& oval, double& lpart) {
  const int tid = threadIdx.x;
  const int q = tid & 7, rg = tid >> 3;  // 8 lanes x float4 = 32 columns, 32 row groups
  const long c = (long)blockIdx.x * MBF_E + 4 * q;
  // the bias gradient (element Kn, owned by one block) and the loss (block G - 1): trailing
  // doubles of every row, summed over the block's 256 threads; issued first, all in flight
  const bool has_bias = A.K == 1 && A.Kn < A.N && (long)blockIdx.x == A.Kn / MBF_E;
  const bool has_loss = blockIdx.x == G - 1;
  double gb = 0.0, ls = 0.0;
  if (has_bias || has_loss)
    for (int p = tid; p < parts; p += 4 * MB_T) {
      double t0[4], t1[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int pk = p + k * MB_T;
        const double* pd = reinterpret_cast<const double*>(fws + (long)(pk < parts ? pk : 0) * wst + wst - 4);
        t0[k] = pk < parts ? pd[0] : 0.0;
        t1[k] = pk < parts ? pd[1] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        gb += t0[k];
        ls += t1[k];
      }
    }
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (c < A.Kn) {
    int p = rg;
    for (; p + 32 * 11 < parts; p += 32 * 12) {  // 12 rows in flight per thread
      floatx4 v[12];
#pragma unroll
      for (int j = 0; j < 12; ++j)
        v[j] = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(fws + (long)(p + 32 * j) * wst + c));
#pragma unroll
      for (int j = 0; j < 12; ++j) { a0 += v[j][0]; a1 += v[j][1]; a2 += v[j][2]; a3 += v[j][3]; }
    }
    for (; p < parts; p += 32) {
      const floatx4 v = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(fws + (long)p * wst + c));
      a0 += v[0]; a1 += v[1]; a2 += v[2]; a3 += v[3];
    }
  }
  fold[rg][4 * q] = a0;
  fold[rg][4 * q + 1] = a1;
  fold[rg][4 * q + 2] = a2;
  fold[rg][4 * q + 3] = a3;
  const double sums[2] = {has_bias ? gb : 0.0, has_loss ? ls : 0.0};
  double tv2[2];
  {
    const int lane = tid & 63, wid = tid >> 6;
    for (int k = 0; k < 2; ++k) {
      const double t = wave_sum(sums[k]);
      if (lane == 0) red[k * MB_NW + wid] = t;
    }
  }
  __syncthreads();
  tv2[0] = (red[0] + red[1]) + (red[2] + red[3]);
  tv2[1] = (red[MB_NW] + red[MB_NW + 1]) + (red[MB_NW + 2] + red[MB_NW + 3]);
  if (own) {
    if (i < A.Kn) {
      double s = 0.0;
#pragma unroll
      for (int g2 = 0; g2 < 32; ++g2) s += fold[g2][tid];
      oval = s;
    } else {
      oval = tv2[0];  // the bias element
    }
  }
  lpart = tv2[1];
  __syncthreads();
}

// K1 of the multi-block step with the fold of the binary evaluation's partial rows in front
// (one-rank fits): ceil(N / 32) blocks, each folds its 32 elements' columns (mbf_fold_block) and
// writes the pass-0 partials; K2..K4 as in srml_qn_step_mb. Replaces fold_rows_kernel + K1.
__global__ __launch_bounds__(MB_T) void qn_mb1f_kernel(QnArgs A, double* __restrict__ scr,
                                                       const float* __restrict__ fws, int parts, long wst) {
  __shared__ double red[4 * MB_NW], tot[4], fold[32][33];
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  const unsigned G = gridDim.x;
  const long i = (long)blockIdx.x * MBF_E + threadIdx.x;
  const bool own = threadIdx.x < MBF_E && i < A.N;
  // every load up front (the fold's rows are read even when the fit is done: a finished fit's
  // remaining graph replays cost one wasted read each, against a round trip on every step)
  const int done = A.fl[F_DONE];
  MbSnap q{};
  if (first) q = mb_snap_load(A);
  const MbP0In e = mb_p0_load(A, i, own);
  double oval = 0.0, lpart = 0.0;
  mbf_fold_block(A, fws, parts, wst, fold, red, own, i, G, oval, lpart);
  if (done) {
    if (first) scr[S_PHASE] = 0.0;
    return;
  }
  if (first) mb_snap_store(A, q, scr);
  if (blockIdx.x == G - 1 && threadIdx.x == 0) scr[S_LOSS] = lpart;
  double p0[4] = {0.0, 0.0, 0.0, 0.0};
  mb_p0(A, i, own, e, oval, p0);
  qn_block_sum<MB_NW>(p0, red, tot);
  if (threadIdx.x < 4) scr[S_PA + blockIdx.x * 4 + threadIdx.x] = tot[threadIdx.x];
}

// One optimiser step of a one-rank binary fit as four launches with the evaluation's fold in K1:
// fws = srml_logreg_binary_f32's workspace left unfolded (leave = 1), parts rows of wst floats.
SRML_API int srml_qn_step_mbf(const QnArgs* a, double* scratch, const float* fws, int parts, long wst,
                              hipStream_t stream) {
  if (a->M < 1 || a->M > QN_MMAX || a->N <= 0 || !scratch || !fws) return (int)hipErrorInvalidValue;
  if (a->K != 1 || (wst & 3) || parts <= 0) return (int)hipErrorInvalidValue;
  const long G = (a->N + MB_T - 1) / MB_T, G1 = (a->N + MBF_E - 1) / MBF_E;
  if (G > MB_GMAX || G1 > MB_GAMAX) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)G), blk(MB_T);
  hipLaunchKernelGGL(qn_mb1f_kernel, dim3((unsigned)G1), blk, 0, stream, *a, scratch, fws, parts, wst);
  hipLaunchKernelGGL(qn_mb2_kernel, grid, blk, 0, stream, *a, scratch, (int)G1);
  hipLaunchKernelGGL(qn_mb3_kernel, grid, blk, 0, stream, *a, scratch);
  hipLaunchKernelGGL(qn_mb4_kernel, grid, blk, 0, stream, *a, scratch);
  return srml_status();
}
