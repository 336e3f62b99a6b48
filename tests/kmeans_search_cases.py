"""Shared oracle, error bounds and case builders of the KMeans nearest-centre search tests
(``test_kmeans_search_edges.py``: the checker on the CPU paths, every kernel on the GPU).

Oracle. Every search works on the fp32 operands V = fp32(X - mu) and W = fp32(C - mu) (fp64 centres
are centred in fp64 and rounded once, as ``srml_f16_centre_prep`` does). The oracle evaluates
D[i, j] = sum_d (v_id - w_jd)^2 of exactly those operands in fp64 by the DIRECT form, row-chunked:
bit-identical centres then give bit-identical distances whatever the row, and nothing cancels (the
expanded form ||v||^2 - 2 v.w + ||w||^2 does neither). Each term is one fp64 subtraction, square and
add, so |D~ - D| <= (n + 2) 2^-53 D <= (n + 2) 2^-53 (||v|| + ||w||)^2; two such distances are compared
and a kernel that claims exactness in fp64 makes the same error again, hence the per-row bound

    beta_i = 4 (n + 2) 2^-53 (||v_i|| + max_j ||w_j||)^2.

Contracts (``check_labels``):

* ``exact``: D[i, lab_i] <= Dmin_i + beta_i for every row; lab_i == arg-min wherever the oracle's
  top-2 gap exceeds beta_i; where the two best oracle distances are bit-equal (duplicated centres)
  the LOWER index. Rows with 0 < gap <= beta_i would be undecidable: the checker asserts there are
  none instead of excluding them.
* ``within`` eps: D[i, lab_i] <= Dmin_i + 2 eps_i + beta_i, lab_i == arg-min where the oracle's
  gap exceeds 2 eps_i, and |dist_i - Dmin_i| <= the distance bound (eps_i unless a path documents another).
  eps_i is derived (u = 2^-24), never tuned:
    - ``eps_fp32``: 6-product split search and fp32 MFMA search: 2 (n + 4) u ||v_i|| wmax + (n + 2) u wmax^2
      (gamma_n accumulation with Cauchy-Schwarz as ``ops.certify_tau`` argues, the three dropped plane
      products, the fp32 sum of ||w||^2);
    - ``eps_split3``: + 2 CERTIFY_TAU ||v_i|| wmax (3-product pass);
    - ``eps_f16``: the fp16 filter's radius 2 tau16 (||v_i|| + xadd) wmax + z ||v_i|| + z2
      (``ops.certify_tau16`` / ``ops.f16_radius_terms``).

Inputs are finite throughout; NaN / inf rows are out of scope of these tests.

numpy / torch on the CPU in fp64 only, so the CPU and GPU tests share every case; cases are cached
and their arrays read-only (one oracle per case, shared by every test that needs it)."""
import functools
import json
import math
import os

import numpy as np

from spark_rapids_ml_nai_amd import ops

U32 = 2.0 ** -24
U64 = 2.0 ** -53
KINDS = ("generic", "ties", "crowd", "offset", "wide_range", "far_centre")


class Case:
    """One search problem and its oracle. X fp32 [m, n], C fp32 or fp64 [k, n], mu fp32 [n];
    V, W the fp32 centred operands; D fp64 [m, k] direct-form distances of V, W; arg / dmin / gap
    the oracle's lowest-index arg-min, its distance and the top-2 gap (+inf for k = 1); vnorm
    ||v_i||, wmax max_j ||w_j||, beta the oracle's own rounding bound; tie_rows / dup_rows the
    engineered bisector rows and the rows whose nearest is the duplicated pair."""

    def __init__(self, X, C, mu, kind, tie_rows=(), dup_rows=()):
        self.kind = kind
        self.X = np.ascontiguousarray(X, dtype=np.float32)
        self.C = np.ascontiguousarray(C)
        self.mu = np.ascontiguousarray(mu, dtype=np.float32)
        self.m, self.n = self.X.shape
        self.k = self.C.shape[0]
        self.V = self.X - self.mu[None, :]  # fp32 subtraction, as every kernel does it
        self.W = (self.C.astype(np.float64) - self.mu.astype(np.float64)[None, :]).astype(np.float32)
        self.tie_rows = np.asarray(tie_rows, dtype=np.int64)
        self.dup_rows = np.asarray(dup_rows, dtype=np.int64)
        V64, W64 = self.V.astype(np.float64), self.W.astype(np.float64)
        self.D = direct_distances(V64, W64)
        self.arg = self.D.argmin(1)  # numpy: the first (lowest-index) minimum
        self.dmin = self.D[np.arange(self.m), self.arg]
        if self.k > 1:
            rest = self.D.copy()
            rest[np.arange(self.m), self.arg] = np.inf
            self.gap = rest.min(1) - self.dmin
        else:
            self.gap = np.full(self.m, np.inf)
        self.vnorm = np.sqrt((V64 * V64).sum(1))
        self.wnorm = np.sqrt((W64 * W64).sum(1))
        self.wmax = float(self.wnorm.max())
        self.beta = 4.0 * (self.n + 2) * U64 * (self.vnorm + self.wmax) ** 2
        for a in (self.X, self.C, self.mu, self.V, self.W, self.D, self.arg, self.dmin, self.gap, self.vnorm,
                  self.wnorm, self.beta, self.tie_rows, self.dup_rows):
            a.setflags(write=False)

    @property
    def shape(self):
        return "%dx%dx%d %s" % (self.m, self.n, self.k, self.kind)


def direct_distances(V64, W64):
    """D[i, j] = sum_d (v_id - w_jd)^2 in fp64, rows chunked to ~2^23 differences at a time."""
    m, n = V64.shape
    k = W64.shape[0]
    D = np.empty((m, k), np.float64)
    step = max(1, (1 << 23) // max(1, k * n))
    for r0 in range(0, m, step):
        diff = V64[r0: r0 + step, None, :] - W64[None, :, :]
        D[r0: r0 + step] = np.einsum("ijd,ijd->ij", diff, diff)
    return D


# ------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def make_case(m, n, k, kind, seed=0, near=None, shuffle=False, c64=False):
    """The case (m rows, n columns, k centres) of ``kind``:

    generic     Gaussian rows and centres.
    ties        (k >= 4) C[1] = C[0] bit for bit, C[3] = C[2] + 1e-6 noise; the first quarter of the
                rows are 0.5 (C[0] + C[2]) + 1e-7 noise (bisector rows: ``tie_rows``), the second
                quarter C[0] + 1e-3 noise (their exact nearest is the duplicated pair: ``dup_rows``).
                ``shuffle``: the rows are permuted, so both groups spread over every row tile.
    crowd       ``near`` centres (default all k) are c + 1e-6 noise around one point c, the other
                k - near sit at c +- 0.9 per coordinate (far outside any filter radius, inside the
                plane's range); rows are c + 0.3 Gaussian.
    offset      generic + 1e4 on X and C.
    wide_range  (n >= 4) generic with three columns x 1e7 and the rest x 1e-3.
    far_centre  generic with the last centre at mu + 8 max|X - mu| in coordinate 0 (mu elsewhere).

    mu is the fp32 column mean of X; for m = 1 it is 0 and the row's first element 4, so that the
    planes exist (mu != the row) and every centre stays inside their range. ``c64``: the centres
    stay fp64 (not representable in fp32)."""
    assert kind in KINDS
    g = np.random.default_rng(1000003 * seed + 7919 * m + 104729 * n + k + 17 * KINDS.index(kind))
    X = g.standard_normal((m, n))
    C = g.standard_normal((k, n))
    if m == 1:
        X[0, 0] = 4.0
    tie_rows, dup_rows = [], []
    if kind == "ties":
        assert k >= 4
        C[1] = C[0]
        C[3] = C[2] + 1e-6 * g.standard_normal(n)
        q = m // 4
        X[:q] = 0.5 * (C[0] + C[2]) + 1e-7 * g.standard_normal((q, n))
        X[q: 2 * q] = C[0] + 1e-3 * g.standard_normal((q, n))
        pos = g.permutation(m) if shuffle else np.arange(m)
        inv = np.empty(m, np.int64)
        inv[pos] = np.arange(m)
        X = X[pos]  # row i of the result is the old row pos[i]
        tie_rows, dup_rows = np.sort(inv[:q]), np.sort(inv[q: 2 * q])
    elif kind == "crowd":
        near = k if near is None else near
        c = g.standard_normal(n)
        X = c + 0.3 * X
        C[:near] = c + 1e-6 * C[:near]
        C[near:] = c + 0.9 * np.sign(C[near:])
        C = C[g.permutation(k)]
    elif kind == "offset":
        X += 1e4
        C += 1e4
    elif kind == "wide_range":
        assert n >= 4
        X[:, :3] *= 1e7
        C[:, :3] *= 1e7
        X[:, 3:] *= 1e-3
        C[:, 3:] *= 1e-3
    X = X.astype(np.float32)
    if not c64:
        C = C.astype(np.float32)
    if kind == "ties":
        C[1] = C[0]
    mu = X.astype(np.float64).mean(0).astype(np.float32)
    if m == 1:
        mu = np.zeros(n, np.float32)
    if kind == "far_centre":
        amax = float(np.abs(X - mu[None, :]).max())
        C[k - 1] = mu
        C[k - 1, 0] = mu[0] + np.float32(8.0 * amax)
    return Case(X, C, mu, kind, tie_rows, dup_rows)


# ------------------------------------------------------------------------------------ bounds
def eps_fp32(case):
    """6-product split search / fp32 MFMA search (per row)."""
    n = case.n
    return 2.0 * (n + 4) * U32 * case.vnorm * case.wmax + (n + 2) * U32 * case.wmax ** 2


def eps_split3(case):
    """3-product split search (``approx=True`` on tiled planes)."""
    return eps_fp32(case) + 2.0 * ops.CERTIFY_TAU * case.vnorm * case.wmax


def f16_scale(case):
    """The power-of-two plane scale ``ops.F16Planes`` picks: max |v| lands in [2^13, 2^14)."""
    a = float(np.abs(case.V).max())
    return 2.0 ** (13 - (math.frexp(a)[1] - 1))


def eps_f16(case):
    """The fp16 filter's certified radius against the worst centre (per row)."""
    tau = ops.certify_tau16(case.n)
    xadd, z, z2 = ops.f16_radius_terms(case.n, f16_scale(case), tau)
    return 2.0 * tau * (case.vnorm + xadd) * case.wmax + z * case.vnorm + z2


def _f16_emulate(case):
    """The fp16 filter's distances with exact accumulation (fp64 products of the fp16-rounded scaled
    operands, as ``test_f16_certificate`` emulates them), and the share of the radius that is NOT
    spent on the kernel's own fp32 accumulation: r_lo[i, j] = 2 (tau16 - 1.01^2 n 2^-24) ||v_i|| ||w_j||."""
    n, s = case.n, f16_scale(case)
    Vh = (case.V.astype(np.float64) * s).astype(np.float16).astype(np.float64) / s
    Wh = (np.clip(case.W.astype(np.float64) * s, -32768.0, 32768.0)).astype(np.float16).astype(np.float64) / s
    d_f = (case.wnorm ** 2)[None, :] - 2.0 * Vh @ Wh.T
    tau_round = ops.certify_tau16(n) - 1.01 * 1.01 * n * U32
    return d_f, 2.0 * tau_round * case.vnorm[:, None] * case.wnorm[None, :]


def _top2_within(d, r):
    """Rows whose two smallest d differ by at most the sum of their r."""
    if d.shape[1] < 2:
        return np.zeros(d.shape[0], bool)
    idx = np.argsort(d, axis=1, kind="stable")[:, :2]
    rows = np.arange(d.shape[0])
    return d[rows, idx[:, 1]] - d[rows, idx[:, 0]] <= r[rows, idx[:, 1]] + r[rows, idx[:, 0]]


def f16_must_flag(case):
    """Rows the fp16 filter cannot certify, whatever its accumulation order: certifying needs the
    kernel's two best filtered distances more than both full radii apart; they differ from the
    emulated ones by the accumulation share only, so an emulated gap within the remaining share
    stays uncertified. (A bisector row of ``ties`` is NOT such a row when a third centre happens to
    be nearer to the midpoint than C[0] and C[2]: common at n <= 17.)"""
    return _top2_within(*_f16_emulate(case))


def bf16_must_flag(case):
    """The same for the 3-product bf16 filter: its distances emulated from the two leading bf16 planes
    with exact accumulation; the kernel's differ by the 2 n 2^-24 share of ``ops.certify_tau``, so an
    emulated gap within 2 CERTIFY_TAU ||v|| (||w_j|| + ||w_b||) is never certified."""
    import torch

    def planes(A):
        a = torch.from_numpy(np.array(A, dtype=np.float32))
        h = a.to(torch.bfloat16).float()
        m_ = (a - h).to(torch.bfloat16).float()
        return h.double().numpy(), m_.double().numpy()

    Vh, Vm = planes(case.V)
    Wh, Wm = planes(case.W)
    d3 = (case.wnorm ** 2)[None, :] - 2.0 * (Vh @ Wh.T + Vh @ Wm.T + Vm @ Wh.T)
    return _top2_within(d3, 2.0 * ops.CERTIFY_TAU * case.vnorm[:, None] * case.wnorm[None, :])


def f16_listed(case):
    """(lo, hi) per row: how many centres the fp16 candidate pass SURELY lists and how many it
    MAY list. The filter's distances are emulated as ``test_f16_certificate`` does (fp64 products of
    the fp16-rounded scaled operands: d_f); the kernel's own d~ differs from d_f only by its fp32
    accumulation and norm rounding, which is the 1.01 n 2^-24 share of ``certify_tau16``. A centre is
    surely listed when d_f_j - min d_f is within the remaining (fp16 rounding) share of its radius,
    and surely not listed when it exceeds twice the full radii of both plus the absolute terms."""
    n, s = case.n, f16_scale(case)
    tau = ops.certify_tau16(n)
    xadd, z, z2 = ops.f16_radius_terms(n, s, tau)
    d_f, r_lo = _f16_emulate(case)
    rel = d_f - d_f.min(1, keepdims=True)
    r_hi = 2.0 * tau * (case.vnorm[:, None] + xadd) * case.wnorm[None, :] + z * case.vnorm[:, None] + z2
    lo = (rel <= r_lo).sum(1)
    hi = (rel <= 2.0 * (r_hi + r_hi.max(1, keepdims=True))).sum(1)
    return lo, hi


# ------------------------------------------------------------------------------------ checker
def check_labels(case, labels, dist=None, contract="exact", eps=None, dist_eps=None):
    """Assert ``labels`` (and ``dist`` when given) against ``case`` under ``contract`` ("exact" or
    "within" with the per-row ``eps``); ``dist_eps``: the per-row bound on |dist - Dmin| (default:
    eps for "within", beta + one fp32 rounding of the distance for "exact"). Returns the worst
    error / bound ratios {"label": ..., "dist": ...} (dist None without distances)."""
    m, k = case.m, case.k
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    assert lab.shape == (m,), "labels have shape %s, want (%d,)" % (lab.shape, m)
    bad = np.nonzero((lab < 0) | (lab >= k))[0]
    assert bad.size == 0, "%s: %d labels outside [0, %d), first at row %d: %d" % (
        case.shape, bad.size, k, bad[0], lab[bad[0]])
    got = case.D[np.arange(m), lab]
    excess = got - case.dmin
    if contract == "exact":
        bound = case.beta
        ambiguous = int(((case.gap > 0) & (case.gap <= case.beta)).sum())
        assert ambiguous == 0, "%s: %d rows have an oracle gap inside its own rounding bound" % (case.shape, ambiguous)
        decided = (case.gap > case.beta) | (case.gap == 0)  # clear winner, or a bit-equal pair: lowest index
        wrong = np.nonzero(decided & (lab != case.arg))[0]
        assert wrong.size == 0, "%s: %d rows miss the exact arg-min, first row %d: got %d want %d (gap %.3g)" % (
            case.shape, wrong.size, wrong[0], lab[wrong[0]], case.arg[wrong[0]], case.gap[wrong[0]])
        if dist_eps is None:
            dist_eps = case.beta + U32 * case.dmin
    elif contract == "within":
        assert eps is not None
        eps = np.broadcast_to(np.asarray(eps, dtype=np.float64), (m,))
        bound = 2.0 * eps + case.beta
        if dist_eps is None:
            dist_eps = eps
    else:
        raise ValueError(contract)
    worse = np.nonzero(excess > bound)[0]
    assert worse.size == 0, "%s: %d rows chose a centre farther than the bound, first row %d: excess %.3g > %.3g" % (
        case.shape, worse.size, worse[0], excess[worse[0]], np.broadcast_to(bound, (m,))[worse[0]])
    clear = case.gap > (bound if contract == "exact" else 2.0 * eps)
    wrong = np.nonzero(clear & (lab != case.arg))[0]
    assert wrong.size == 0, "%s: %d clear rows miss the arg-min" % (case.shape, wrong.size)
    out = {"label": float((excess / bound).max()), "dist": None}
    if dist is not None:
        d = np.asarray(dist).astype(np.float64).reshape(-1)
        assert d.shape == (m,)
        assert np.isfinite(d).all(), "%s: non-finite distances" % case.shape
        dist_eps = np.broadcast_to(np.asarray(dist_eps, dtype=np.float64), (m,))
        err = np.abs(d - case.dmin)
        off = np.nonzero(err > dist_eps)[0]
        assert off.size == 0, "%s: %d distances off, first row %d: |%.9g - %.9g| = %.3g > %.3g" % (
            case.shape, off.size, off[0], d[off[0]], case.dmin[off[0]], err[off[0]], dist_eps[off[0]])
        out["dist"] = float((err / dist_eps).max())
    return out


# ------------------------------------------------------------------------------------ records
RATIOS = {}  # path -> {"label": (ratio, shape), "dist": (ratio, shape)}: the worst seen in this process


def record(path, case, ratios):
    """Keep the worst error / bound ratios of ``path`` (measurements for docs/coverage.md, not
    thresholds); with ``SRML_KMEANS_SEARCH_RATIOS=<file>`` the table is rewritten there as JSON."""
    slot = RATIOS.setdefault(path, {})
    for key, r in ratios.items():
        if r is not None and (key not in slot or r > slot[key][0]):
            slot[key] = (r, case.shape)
    out = os.environ.get("SRML_KMEANS_SEARCH_RATIOS")
    if out:
        with open(out, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)
