"""Oracle, bounds, case builders and the contract checkers of the sparse (CSR rows x dense centres)
KMeans tests: the nearest-centre search, the cluster sums and the planted fit-level data.

Search oracle: the CSR values and the centres (both already in the kernel's precision, fp32 or
fp64) densified to fp64, D[i, j] = sum_d (x_id - c_jd)^2 in DIRECT form, so bit-identical centres
give bit-identical distances and nothing cancels. Its own rounding is
beta_i = 4 (n + 2) 2^-53 (|x_i| + max_j |c_j|)^2 (``kmeans_search_cases``).

Band of the fp32 search, derived from the kernel's arithmetic (u = 2^-24, t_i = nnz of row i):

* the dot product is ONE chain of t_i fused multiply-adds per (row, centre), in column order, no
  cross-lane sum: |S^ - S| <= t_i u |x| |c| (any order gives the same bound); doubled, with
  |x| |c| <= (|x| + |c|)^2 / 4: (t_i / 2) u (|x| + |c|)^2;
* |x|^2 and |c|^2 are fp32 roundings of fp64 sums (the fp64 sums' own error is 2^-29 of that), their
  fp32 sum and the final fused -2 S + (|x|^2 + |c|^2) are two more roundings, each of a value no
  larger than (|x| + |c|)^2: 4 u (|x| + |c|)^2; the clamp at 0 only moves a key towards D >= 0;
* eps_ij = (t_i / 2 + 4) u (|x_i| + |c_j|)^2.

Contract ``within``: D[i, lab] <= Dmin + eps[i, lab] + eps[i, arg] + beta (both keys are off by at
most their own eps: never wider than the 2 eps of the row's worst centre); the label is the oracle's
arg-min where the top-2 gap exceeds 2 max_j eps_ij + beta, and the LOWER index where the two best
are bit-equal; the distance is within eps[i, lab] + beta of D[i, lab]. Every builder asserts that
none of its rows has 0 < gap <= 2 max_j eps_ij + beta, so every label is pinned. Contract ``exact``
(fp64 instantiation): the same with eps = 0 (its own error (t / 2 + 4) 2^-53 (|x| + |c|)^2 is inside
beta). Contract ``bit`` (lattice cases: small integers, 4 n max^2 < 2^24, every product and partial
sum an exact integer): labels and distances equal the oracle's bit for bit.

Cluster sums: the fp64 ``np.add.at`` oracle; a cell with c terms lies within gamma_c(2^-53) sum|x|
(fp64 atomics add in any order); lattice cases are bit-equal; counts are exact. The fixed-point
(deterministic) sums add rint(x 2^s) exactly and round once: c / 2 quanta 2^-s plus 2^-53 |sum| off the
true sum, and the oracle's own fp64 chain is gamma_c(2^-53) sum|x| off it.
"""
import functools

import numpy as np
import torch

from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.core.base import CSR

U24 = 2.0 ** -24
U53 = 2.0 ** -53
TK, STAGE, ROWS = ops.CSR_KM_TK, ops.CSR_KM_STAGE, ops.CSR_KM_ROWS


def csr_from_rows(rows, n, dtype=np.float32):
    """``core.base.CSR`` on the CPU (int64 / int32 / dtype) from a list of (sorted columns, values)."""
    counts = np.array([len(c) for c, _ in rows], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    idx = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows] + [np.zeros(0, np.int32)])
    val = np.concatenate([np.asarray(v, dtype=dtype) for _, v in rows] + [np.zeros(0, dtype)])
    return CSR(indptr=torch.from_numpy(indptr), indices=torch.from_numpy(idx.astype(np.int32)),
               data=torch.from_numpy(val.astype(dtype)), shape=(len(rows), int(n)))


def to(A, device):
    return CSR(indptr=A.indptr.to(device), indices=A.indices.to(device), data=A.data.to(device), shape=A.shape)


def row_block(A, lo, hi):
    """Rows lo .. hi with ABSOLUTE offsets: the indptr slice is not re-based."""
    return CSR(indptr=A.indptr[lo: hi + 1], indices=A.indices, data=A.data, shape=(hi - lo, A.shape[1]))


def take_rows(A, order):
    """The CSR whose row i is row order[i] of ``A``."""
    ip, ix, v = A.indptr.numpy(), A.indices.numpy(), A.data.numpy()
    return csr_from_rows([(ix[ip[r]: ip[r + 1]], v[ip[r]: ip[r + 1]]) for r in order], A.shape[1], v.dtype)


def dense64(A):
    m, n = A.shape
    out = np.zeros((m, n), np.float64)
    ip = A.indptr.cpu().numpy()
    rows = np.repeat(np.arange(m), np.diff(ip))
    out[rows, A.indices.cpu().numpy()[ip[0]: ip[-1]]] = A.data.cpu().numpy()[ip[0]: ip[-1]].astype(np.float64)
    return out


def direct_distances(X64, C64):
    m, n = X64.shape
    k = C64.shape[0]
    D = np.empty((m, k), np.float64)
    step = max(1, (1 << 23) // max(1, k * n))
    for r0 in range(0, m, step):
        diff = X64[r0: r0 + step, None, :] - C64[None, :, :]
        D[r0: r0 + step] = np.einsum("ijd,ijd->ij", diff, diff)
    return D


class SearchCase:
    """One search problem and its oracle: A (CPU CSR), C (k, n) in the values' dtype, D, arg (lowest
    index), dmin, gap (+inf for k = 1), eps [m, k], beta [m]; ``contract`` within / exact / bit."""

    def __init__(self, name, A, C, contract):
        self.name, self.A, self.contract = name, A, contract
        self.C = np.ascontiguousarray(C)
        assert self.C.dtype == A.data.numpy().dtype
        self.m, self.n = A.shape
        self.k = self.C.shape[0]
        assert self.m * self.k * max(1, self.n) <= 1 << 28, "the direct-form oracle of %s is too large" % name
        X64, C64 = dense64(A), self.C.astype(np.float64)
        self.D = direct_distances(X64, C64)
        rows = np.arange(self.m)
        self.arg = self.D.argmin(1)
        self.dmin = self.D[rows, self.arg]
        if self.k > 1:
            rest = self.D.copy()
            rest[rows, self.arg] = np.inf
            self.gap = rest.min(1) - self.dmin
        else:
            self.gap = np.full(self.m, np.inf)
        self.t = np.diff(A.indptr.numpy()).astype(np.float64)
        xn, cn = np.sqrt((X64 * X64).sum(1)), np.sqrt((C64 * C64).sum(1))
        s2 = (xn[:, None] + cn[None, :]) ** 2
        self.beta = 4.0 * (self.n + 2) * U53 * (xn + cn.max()) ** 2
        self.eps = (self.t[:, None] / 2 + 4) * U24 * s2 if contract == "within" else np.zeros_like(s2)
        self.clear = 2.0 * self.eps.max(1) + self.beta
        # no undecidable row: a clear winner, or a bit-equal pair (the lower index is pinned)
        amb = np.nonzero((self.gap > 0) & (self.gap <= self.clear))[0]
        assert amb.size == 0, "%s: rows %s have a gap inside the band (gap %s, band %s)" % (
            name, amb[:5], self.gap[amb[:5]], self.clear[amb[:5]])
        if contract == "bit":
            big = max(float(np.abs(X64).max()) if X64.size else 0.0, float(np.abs(C64).max()))
            assert 4 * max(1, self.n) * big * big < 2 ** 24 and (X64 == np.rint(X64)).all() and (C64 == np.rint(C64)).all()
        for a in (self.C, self.D, self.arg, self.dmin, self.gap, self.eps, self.beta, self.clear):
            a.setflags(write=False)

    def centres(self, device="cpu"):
        return torch.from_numpy(self.C.copy()).to(device)


def check_nearest(case, labels, dist):
    """The case's contract on every row, none skipped; AssertionError names the first violation.
    Returns the worst error / bound ratios {"label", "dist"} (0 for bit cases)."""
    m, k = case.m, case.k
    lab = np.asarray(labels.detach().cpu() if torch.is_tensor(labels) else labels).astype(np.int64).reshape(-1)
    d = np.asarray(dist.detach().cpu() if torch.is_tensor(dist) else dist).astype(np.float64).reshape(-1)
    assert lab.shape == (m,) and d.shape == (m,), (lab.shape, d.shape)
    bad = np.nonzero((lab < 0) | (lab >= k))[0]
    assert bad.size == 0, "%s: label outside [0, %d) at row %d: %d" % (case.name, k, bad[0], lab[bad[0]])
    assert np.isfinite(d).all() and (d >= 0).all(), "%s: distances not finite and non-negative" % case.name
    rows = np.arange(m)
    got = case.D[rows, lab]
    if case.contract == "bit":
        wrong = np.nonzero(lab != case.arg)[0]
        assert wrong.size == 0, "%s: row %d label %d, the oracle's lowest arg-min is %d" % (
            case.name, wrong[0], lab[wrong[0]], case.arg[wrong[0]])
        off = np.nonzero(d != case.dmin)[0]
        assert off.size == 0, "%s: row %d distance %r is not the oracle's %r" % (case.name, off[0], d[off[0]],
                                                                                 case.dmin[off[0]])
        return {"label": 0.0, "dist": 0.0}
    bound = case.eps[rows, lab] + case.eps[rows, case.arg] + case.beta
    excess = got - case.dmin
    worse = np.nonzero(excess > bound)[0]
    assert worse.size == 0, "%s: row %d chose centre %d, farther than the band: excess %.3g > %.3g" % (
        case.name, worse[0], lab[worse[0]], excess[worse[0]], bound[worse[0]])
    pinned = (case.gap > case.clear) | (case.gap == 0)
    wrong = np.nonzero(pinned & (lab != case.arg))[0]
    assert wrong.size == 0, "%s: row %d label %d, want %d (gap %.3g%s)" % (
        case.name, wrong[0], lab[wrong[0]], case.arg[wrong[0]], case.gap[wrong[0]],
        ": bit-equal centres, the lower index wins" if case.gap[wrong[0]] == 0 else "")
    dbound = case.eps[rows, lab] + case.beta + (U53 * got if case.contract == "exact" else 0.0)
    err = np.abs(d - got)
    off = np.nonzero(err > dbound)[0]
    assert off.size == 0, "%s: row %d distance %.9g, oracle %.9g: off by %.3g > %.3g" % (
        case.name, off[0], d[off[0]], got[off[0]], err[off[0]], dbound[off[0]])
    return {"label": float((excess / bound).max()), "dist": float((err / np.maximum(dbound, 1e-300)).max())}


# ------------------------------------------------------------------------------------ search cases
def _values(rng, count, kind):
    if kind == "lattice":
        v = rng.integers(1, 4, count) * rng.choice([-1, 1], count)
        return v.astype(np.float64)
    v = rng.standard_normal(count)
    v[v == 0] = 1.0
    return v


def make_rows(rng, m, n, mean_nnz, kind="normal", lengths=None):
    """Poisson row lengths; row 0 always holds column n - 1, row 1 is empty and row 2 long (50 x the
    mean, at most n) when there are that many rows; ``lengths`` {row: nnz} overrides."""
    counts = np.clip(rng.poisson(mean_nnz, m), 1, n)
    if m > 1:
        counts[1] = 0
    if m > 2:
        counts[2] = min(n, 50 * mean_nnz)
    for r, c in (lengths or {}).items():
        counts[r] = c
    rows = []
    for r, c in enumerate(counts):
        cols = np.sort(rng.choice(n, int(c), replace=False)) if c else np.zeros(0, np.int64)
        if r == 0 and len(cols) and cols[-1] != n - 1:
            cols[-1] = n - 1
        rows.append((cols, _values(rng, len(cols), kind)))
    return rows


def build_search(name, m, n, k, mean_nnz, seed, dtype=np.float32, kind="normal", lengths=None, dups=True,
                 cscale=None):
    """Rows as ``make_rows``; Gaussian centres of about the rows' norm (lattice: integers in [-3, 3]).
    ``dups`` (k >= 3, a row 3 exists): centre 0 is row 3 densified and centre k - 1 its bit-identical
    copy, so row 3's two best are bit-equal, first and last tile apart."""
    rng = np.random.default_rng(seed)
    rows = make_rows(rng, m, n, mean_nnz, kind, lengths)
    A = csr_from_rows(rows, n, dtype)
    if kind == "lattice":
        C = rng.integers(-3, 4, (k, n)).astype(dtype)
    else:
        cscale = np.sqrt(max(1.0, mean_nnz) / n) if cscale is None else cscale
        C = (cscale * rng.standard_normal((k, n))).astype(dtype)
    if dups and k >= 3 and m > 3:
        C[0] = dense64(A)[3].astype(dtype)
        C[k - 1] = C[0]
    contract = "bit" if kind == "lattice" else ("within" if dtype == np.float32 else "exact")
    return SearchCase(name, A, C, contract)


K_EDGES = (1, 2, 63, 64, 65, TK - 1, TK, TK + 1, 2 * TK + 1)
M_EDGES = (1, ROWS - 1, ROWS, ROWS + 1)
STAGE_EDGES = (STAGE - 1, STAGE, STAGE + 1)

# name -> build_search arguments; the seeds were chosen on the CPU so that the oracle alone decides every
# row (SearchCase asserts it)
_SEARCH = {}
for _k in K_EDGES:
    _SEARCH["k%d" % _k] = dict(m=3 * ROWS + 1, n=257, k=_k, mean_nnz=9, seed=10 + _k)
for _m in M_EDGES:
    _SEARCH["m%d" % _m] = dict(m=_m, n=50, k=5, mean_nnz=6, seed=40 + _m)
_SEARCH["n1"] = dict(m=6, n=1, k=3, mean_nnz=1, seed=3, dups=False, cscale=2.0)
_SEARCH["full_row"] = dict(m=7, n=40, k=TK + 1, mean_nnz=5, seed=5, lengths={4: 40})
for _s in STAGE_EDGES:  # k > TK: the staged row is re-used across centre tiles
    _SEARCH["stage%d" % _s] = dict(m=6, n=STAGE + 37, k=TK + 3, mean_nnz=8, seed=70 + (_s - STAGE),
                                   lengths={2: 8, 4: _s}, cscale=0.5)
_SEARCH["long_row"] = dict(m=9, n=3 * STAGE, k=TK + 1, mean_nnz=7, seed=81, lengths={2: 7, 5: 2 * STAGE + 5},
                           cscale=0.5)
_SEARCH["all_empty"] = dict(m=ROWS + 2, n=33, k=7, mean_nnz=4, seed=9,
                            lengths={r: 0 for r in range(ROWS + 2)}, dups=False)
_SEARCH["generic"] = dict(m=301, n=5000, k=70, mean_nnz=12, seed=1, dups=False)
_SEARCH["generic_wide"] = dict(m=97, n=70001, k=9, mean_nnz=30, seed=3, dups=False)
for _name in ("k2", "k65", "k%d" % (2 * TK + 1), "stage%d" % (STAGE + 1), "all_empty", "generic"):
    _SEARCH[_name + "_f64"] = dict(_SEARCH[_name], dtype=np.float64)
for _name in ("k%d" % (TK + 1), "m%d" % (ROWS + 1), "full_row", "stage%d" % STAGE):
    _SEARCH[_name + "_lattice"] = dict(_SEARCH[_name], kind="lattice")
SEARCH_NAMES = tuple(_SEARCH)


@functools.lru_cache(maxsize=None)
def search_case(name):
    return build_search(name, **_SEARCH[name])


# ------------------------------------------------------------------------------------ cluster sums
class SumsCase:
    def __init__(self, name, A, labels, k, lattice=False):
        self.name, self.A, self.k, self.lattice = name, A, int(k), lattice
        self.labels = np.asarray(labels, dtype=np.int32)
        m, n = A.shape
        ip = A.indptr.numpy()
        rows = np.repeat(np.arange(m), np.diff(ip))
        cols = A.indices.numpy()[ip[0]: ip[-1]].astype(np.int64)
        v = A.data.numpy()[ip[0]: ip[-1]].astype(np.float64)
        self.sums = np.zeros((k, n), np.float64)
        self.abs = np.zeros((k, n), np.float64)
        self.terms = np.zeros((k, n), np.float64)
        np.add.at(self.sums, (self.labels[rows], cols), v)
        np.add.at(self.abs, (self.labels[rows], cols), np.abs(v))
        np.add.at(self.terms, (self.labels[rows], cols), 1.0)
        self.counts = np.bincount(self.labels, minlength=k).astype(np.int64)
        self.bound = self.terms * U53 / (1 - self.terms * U53) * self.abs
        self.vmax = float(np.abs(v).max()) if v.size else 0.0
        if lattice:
            assert (v == np.rint(v)).all()

    def labels_t(self, device="cpu"):
        return torch.from_numpy(self.labels.copy()).to(device)


def check_sums(case, sums, counts, fixed_scale=None):
    """Counts exact; every cell within its bound (bit-equal for lattice cases). ``fixed_scale``: the
    deterministic sums' 2^s — c / 2 quanta of 2^-s and one rounding of the sum off the true sum, plus
    the oracle's own gamma_c chain."""
    s = np.asarray(sums.detach().cpu()).astype(np.float64)
    c = np.asarray(counts.detach().cpu()).astype(np.int64)
    assert s.shape == case.sums.shape and c.shape == (case.k,), (s.shape, c.shape)
    assert np.array_equal(c, case.counts), "%s: counts %s, want %s" % (case.name, c[:8], case.counts[:8])
    if case.lattice:
        bad = np.argwhere(s != case.sums)
        assert bad.size == 0, "%s: cell %s is %r, want %r" % (case.name, tuple(bad[0]), s[tuple(bad[0])],
                                                              case.sums[tuple(bad[0])])
        return 0.0
    bound = case.bound if fixed_scale is None else (case.terms * 0.5 / fixed_scale + U53 * np.abs(case.sums)
                                                            + case.bound)
    err = np.abs(s - case.sums)
    bad = np.argwhere(err > bound)
    assert bad.size == 0, "%s: cell %s off by %.3g > %.3g (%d terms)" % (
        case.name, tuple(bad[0]), err[tuple(bad[0])], bound[tuple(bad[0])], case.terms[tuple(bad[0])])
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


_SUMS = {
    "generic": dict(m=700, n=300, k=9, mean_nnz=12, seed=1),          # few cells: many terms per cell
    "wide": dict(m=203, n=40000, k=TK + 1, mean_nnz=30, seed=2),
    "k1": dict(m=ROWS + 1, n=20, k=1, mean_nnz=5, seed=3),
    "m1": dict(m=1, n=20, k=3, mean_nnz=5, seed=4),
    "all_empty": dict(m=9, n=11, k=4, mean_nnz=3, seed=5, lengths={r: 0 for r in range(9)}),
    "long_row": dict(m=12, n=2 * STAGE, k=3, mean_nnz=4, seed=6, lengths={5: STAGE + 9}),
    "lattice": dict(m=400, n=64, k=5, mean_nnz=20, seed=7, kind="lattice"),
    "generic_f64": dict(m=300, n=200, k=6, mean_nnz=10, seed=8, dtype=np.float64),
}
SUMS_NAMES = tuple(_SUMS)


@functools.lru_cache(maxsize=None)
def sums_case(name):
    """Random labels in [0, k) with cluster k - 2 left empty (k >= 3): its sums stay 0, its count 0."""
    p = dict(_SUMS[name])
    k, seed, dtype, kind = p.pop("k"), p.pop("seed"), p.pop("dtype", np.float32), p.pop("kind", "normal")
    rng = np.random.default_rng(1000 + seed)
    A = csr_from_rows(make_rows(rng, p["m"], p["n"], p["mean_nnz"], kind, p.get("lengths")), p["n"], dtype)
    labels = rng.integers(0, k, p["m"])
    if k >= 3:
        labels[labels == k - 2] = k - 1
    return SumsCase(name, A, labels, k, lattice=kind == "lattice")


# ------------------------------------------------------------------------------------ planted fit data
PLANT_K, PLANT_N, PLANT_M = 6, 4096, 1200


class Planted:
    """k = 6 clusters, each on 22 columns of its own block of n / k columns: a row keeps 19 to 21 of
    its cluster's 22 columns, values template (in [1, 2]) x (1 +- 5 %), all non-negative. Rows of two
    clusters share no column, so cross-cluster squared distances (|x|^2 + |y|^2 ~ 90) exceed the
    within-cluster ones (~ 10) several times over: asserted."""

    def __init__(self, seed=0):
        import scipy.sparse as sp

        rng = np.random.default_rng(seed)
        k, n, m = PLANT_K, PLANT_N, PLANT_M
        block = n // k
        self.truth = rng.integers(0, k, m)
        self.truth[:k] = np.arange(k)
        support = [c * block + np.sort(rng.choice(block, 22, replace=False)) for c in range(k)]
        template = [1.0 + rng.random(22) for _ in range(k)]
        ind, val, ptr = [], [], [0]
        for c in self.truth:
            keep = np.sort(rng.choice(22, int(rng.integers(19, 22)), replace=False))
            ind.append(support[c][keep])
            val.append(template[c][keep] * (1.0 + 0.05 * rng.uniform(-1, 1, len(keep))))
            ptr.append(ptr[-1] + len(keep))
        self.M = sp.csr_matrix((np.concatenate(val).astype(np.float32), np.concatenate(ind).astype(np.int32),
                                np.array(ptr, np.int64)), shape=(m, n))
        self.M.sort_indices()
        X = self.M.toarray().astype(np.float64)
        sub = X[:240]
        G = sub @ sub.T
        sq = np.diag(G)
        D = sq[:, None] + sq[None, :] - 2 * G
        same = self.truth[:240, None] == self.truth[None, :240]
        self.within, self.cross = float(D[same].max()), float(D[~same].min())
        assert self.cross > 3 * self.within, (self.within, self.cross)
        self.X64 = X
        self.means = np.stack([X[self.truth == c].mean(0) for c in range(k)])

    def recovers(self, labels):
        """Whether ``labels`` is the planted partition up to a renaming of the clusters."""
        labels = np.asarray(labels).astype(np.int64)
        pairs = set(zip(self.truth.tolist(), labels.tolist()))
        return len(pairs) == PLANT_K and len({a for a, _ in pairs}) == PLANT_K and len({b for _, b in pairs}) == PLANT_K

    def oracle_lloyd(self, C0, iters=20):
        """fp64 dense Lloyd from the centres ``C0``: the labels it ends on."""
        C = np.asarray(C0, np.float64).copy()
        lab = None
        for _ in range(iters):
            D = (self.X64 * self.X64).sum(1)[:, None] + (C * C).sum(1)[None, :] - 2 * self.X64 @ C.T
            new = D.argmin(1)
            if lab is not None and np.array_equal(new, lab):
                break
            lab = new
            for c in range(C.shape[0]):
                if (lab == c).any():
                    C[c] = self.X64[lab == c].mean(0)
        return lab

    def centre_bound(self, labels):
        """Per-cell bound of a fitted centre against the fp64 mean of its rows: the cluster-sum bound
        divided by the count, plus the division's rounding."""
        labels = np.asarray(labels).astype(np.int64)
        k = PLANT_K
        cnt = np.bincount(labels, minlength=k).astype(np.float64)
        absum = np.stack([np.abs(self.X64[labels == c]).sum(0) for c in range(k)])
        terms = np.stack([(self.X64[labels == c] != 0).sum(0) for c in range(k)]).astype(np.float64)
        mean = np.stack([self.X64[labels == c].mean(0) for c in range(k)])
        return mean, (terms * U53 / (1 - terms * U53) * absum) / cnt[:, None] + 2 * U53 * np.abs(mean)


PLANT_SEED = 3  # the KMeans seed of the fit tests: planted() asserts the oracle Lloyd recovers from its seeding


@functools.lru_cache(maxsize=None)
def planted():
    """The planted data, with the assertion that an fp64 Lloyd from the SAME k-means|| seeding (the
    estimator's seeding code on the CPU, seed PLANT_SEED) recovers the partition."""
    from spark_rapids_ml_nai_amd.core.base import to_device
    from spark_rapids_ml_nai_amd.models.kmeans import init_kmeans_parallel
    from spark_rapids_ml_nai_amd.parallel.context import PartitionDescriptor, WorkerContext

    P = Planted(0)
    ctx = WorkerContext.single(torch.device("cpu"))
    A = to_device(P.M, torch.device("cpu"), torch.float32)
    desc = PartitionDescriptor.build(ctx, PLANT_M, PLANT_N)
    C0 = init_kmeans_parallel(A, None, desc, ctx, PLANT_K, PLANT_SEED, 2.0, 2).numpy()
    assert P.recovers(P.oracle_lloyd(C0)), "seed %d: the oracle Lloyd does not recover the planted partition" % PLANT_SEED
    return P


def planted_decided(P, C):
    """Rows of the planted data whose nearest of the centres ``C`` the oracle decides for BOTH fp32
    searches: top-2 gap above twice the wider band — the CSR search's (t / 2 + 4) u (|x| + |c|)^2 and
    the dense fp32 search's 2 (n + 4) u |x| cmax + (n + 2) u cmax^2 (``kmeans_search_cases.eps_fp32``)."""
    C64 = np.asarray(C, np.float64)
    n = P.X64.shape[1]
    D = np.sort(direct_distances(P.X64, C64), axis=1)
    xn, cmax = np.sqrt((P.X64 * P.X64).sum(1)), float(np.sqrt((C64 * C64).sum(1)).max())
    t = (P.X64 != 0).sum(1)
    eps_csr = (t / 2 + 4) * U24 * (xn + cmax) ** 2
    eps_dense = 2.0 * (n + 4) * U24 * xn * cmax + (n + 2) * U24 * cmax ** 2
    return (D[:, 1] - D[:, 0]) > 2 * np.maximum(eps_csr, eps_dense)


def fit_with_an_empty_cluster(device, monkeypatch):
    """``kmeans_fit_csr`` of the planted rows from chosen centres: the five first planted means and a
    sixth centre (100 in every column) that no row is nearest to. Returns (initial centres fp64
    [6, n], the fit's result dict)."""
    from spark_rapids_ml_nai_amd.core.base import to_device
    from spark_rapids_ml_nai_amd.models import kmeans as M
    from spark_rapids_ml_nai_amd.parallel.context import PartitionDescriptor, WorkerContext

    P = planted()
    C0 = np.concatenate([P.means[:5] + 0.01, np.full((1, PLANT_N), 100.0)])
    ctx = WorkerContext.single(torch.device(device))
    A = to_device(P.M, ctx.device, torch.float32)
    desc = PartitionDescriptor.build(ctx, PLANT_M, PLANT_N)
    monkeypatch.setattr(M, "init_random", lambda *a, **kw: torch.from_numpy(C0.copy()).to(ctx.device))
    return C0, M.kmeans_fit_csr(A, desc, ctx, PLANT_K, 5, 1e-4, 1, init="random")


def million_column_fit():
    """Run in a fresh process (its peak resident size is the measurement): a sparse fit and transform
    at n = 2^20, m = 2000, k = 8 on the CPU; prints one JSON line with the growth of the peak resident
    size over the state just before the fit (modules imported, the frame built)."""
    import json
    import resource

    import scipy.sparse as sp

    from spark_rapids_ml_nai_amd.clustering import KMeans
    from spark_rapids_ml_nai_amd.core.dataframe import DataFrame

    n, m, k = 1 << 20, 2000, 8
    rng = np.random.default_rng(0)
    blocks = rng.integers(0, k, m)
    ind = blocks[:, None] * (n // k) + rng.integers(0, 64, (m, 24))
    rows = [np.unique(r) for r in ind]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    M = sp.csr_matrix((1.0 + rng.random(ptr[-1]).astype(np.float32), np.concatenate(rows).astype(np.int32), ptr),
                      shape=(m, n))
    frame = DataFrame.from_numpy(M)
    KMeans(k=2, seed=2, enable_sparse_data_optim=True, maxIter=1, initMode="random").fit(
        DataFrame.from_numpy(M[:50, :]))  # first-use allocations of the libraries, at a small k
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    model = KMeans(k=k, seed=2, enable_sparse_data_optim=True, maxIter=3, initMode="random").fit(frame)
    lab = np.asarray(model.transform(frame).to_numpy("prediction"))
    grown = (resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before) * 1024
    print(json.dumps({"grown": int(grown), "knb": k * n * 8, "centres": list(np.asarray(model.cluster_centers_).shape),
                      "labels": int(lab.shape[0]), "clusters": int(len(set(lab.tolist())))}), flush=True)
