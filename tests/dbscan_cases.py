"""DBSCAN oracle, error bound, case builders and checker (plain numpy / scipy; nothing from the
package's kernels is imported here).

Oracle: D[i, j] = sum_d (x_id - x_jd)^2 in fp64 on the fp32 rows a call receives, components from
``scipy.sparse.csgraph.connected_components``. Cosine: D = ||a/|a| - b/|b|||^2 = 2 (1 - cos) in fp64,
an all-zero row at D = 2 (cosine distance 1) from every row but itself (sklearn's rule).

Two kinds of input.

Lattice (exact): small-integer coordinates with 4 n max|x|^2 < 2^24 (four times stricter than the
n max|x|^2 < 2^24 that makes the products and partial sums exact: it also covers ||a||^2 + ||b||^2
and the fused 2 a.b subtraction). Every fp32 value of the expanded form is then an integer below
2^24 in any summation order, so the kernels must equal the oracle bit for bit.

Generic (banded): eps_ij = c(n) u (||a - mu|| + ||b - mu||)^2, u = 2^-24, mu the fp64 column mean,
c(n) = 3 n / 2 + 8. Derivation, for the model's path (rows centred on c = fp32(mu), then the
expanded form ||a'||^2 + ||b'||^2 - 2 a'.b' in fp32), with A = ||a'||, B = ||b'||,
S_c = ||a - c|| + ||b - c||, in units of u S_c^2:
  * centring a' = fl(a - c): |a'_d - (a_d - c_d)| <= u |a_d - c_d|, so a' - b' differs from a - b
    by a vector of norm <= u S_c, and D by <= 2 ||a - b|| u S_c + u^2 S_c^2 <= 2 (||a - b|| <= S_c);
  * row norms: n products and additions of non-negative terms, at most n roundings on any path
    of any summation order (the device kernel: ceil(n / 64) fused terms per lane and a 6-level
    wave tree; the CPU fall-back: a vectorised sum): n u (A^2 + B^2) <= n;
  * their sum rn + cn: 1;
  * the dot product, n fused terms (``mfma_f32_32x32x2f32`` over the k-tiles, one rounding per
    term; any order): n u A B, doubled, A B <= S_c^2 / 4: n / 2;
  * the finaliser ``fmaf(-2, acc, rn + cn)``: one rounding of a value <= S_c^2: 1;
  * the threshold eps^2 rounded to fp32: u eps^2, and a pair that close to eps^2 has
    S_c^2 >= D >= eps^2 (1 - u): 1.
  Sum 3 n / 2 + 5. The remaining 3 pay for S_c against the S = ||a - mu|| + ||b - mu|| of the bound
  (the centre the rows are taken about is fp32(mu), not mu): the builder asserts
  (1 + rho)^2 (3 n / 2 + 5) (1 + 2^-10) <= c(n), rho = ||mu - fp32(mu)|| / min_i ||x_i - mu||, the 2^-10 for
  the second-order terms dropped above.
Cosine: unit rows, S = 2. Normalising x / ||x|| carries (n / 2 + 1) u from the fp32 norm (n roundings
under a square root, one for the root) as a common factor and u per element from the division: the
unit row moves by <= (n / 2 + 2) u, a' - b' by <= (n + 4) u, D by <= 2 . 2 (n + 4) u = (n + 4) u S^2. With the
expanded form's 3 n / 2 + 3 (no centring) c_cos(n) = 5 n / 2 + 8, band c_cos(n) u 4.

A pair is *in* if D <= eps^2 - band, *out* if D > eps^2 + band, undecided otherwise; the self pair is
always in. ``generic_case`` drops one row of every undecided pair and asserts that at least 95 % of
the rows remain and that none is left; ``make_oracle`` asserts the latter again, so the checker
never skips a pair.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

U = 2.0 ** -24
# constants of the kernels; tests/test_dbscan_edges.py compares TILE with ``ops.DB_TILE``
TILE = 128          # ops.DB_TILE, the 128 x 128 tile pairs of csrc/dbscan.hip
BK = 32             # srml_tile::BK of csrc/tile.h, the k-tile of gemm_tile_128
LABEL_BLOCK = 1024  # DL_T of csrc/dbscan.hip, the block of the root-flag prefix scan
GRID_CAP = 8192     # grid_for() of csrc/dbscan.hip, the largest grid of the sweeps


def c_of_n(n: int) -> float:
    return 1.5 * n + 8.0


def c_cos(n: int) -> float:
    return 2.5 * n + 8.0


def num_tiles(N: int) -> int:
    nt = (N + TILE - 1) // TILE
    return nt * (nt + 1) // 2


def orderable(d32: np.ndarray) -> np.ndarray:
    """The kernels' order-preserving uint32 image of a non-negative fp32."""
    return (np.asarray(d32, np.float32).view(np.uint32) | np.uint32(0x80000000)).astype(np.int64)


def key_dist(best: np.ndarray) -> np.ndarray:
    """fp32 distance held in the high half of a packed key (non-negative distances)."""
    hi = ((np.asarray(best, np.int64) >> 32) & 0x7FFFFFFF).astype(np.uint32)
    return hi.view(np.float32).astype(np.float64)


def pack_key(D: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """int64 view of (orderable(fp32(D)) << 32 | idx)."""
    hi = orderable(np.asarray(D, np.float64).astype(np.float32))
    return ((hi - (1 << 32)) << 32) | (np.asarray(idx, np.int64) & 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------ oracle
def sqdist64(X: np.ndarray, I=None, J=None) -> np.ndarray:
    """Direct-form squared distances in fp64: the full matrix, or of the index pairs (I, J)."""
    X64 = np.asarray(X, np.float64)
    if I is not None:
        t = X64[np.asarray(I)] - X64[np.asarray(J)]
        return (t * t).sum(-1)
    D = np.zeros((X64.shape[0], X64.shape[0]))
    for d in range(X64.shape[1]):
        t = X64[:, d, None] - X64[None, :, d]
        D += t * t
    return D


def _unit64(X: np.ndarray):
    X64 = np.asarray(X, np.float64)
    nr = np.sqrt((X64 * X64).sum(1))
    return X64 / np.where(nr == 0, 1.0, nr)[:, None], nr == 0


@dataclass
class Oracle:
    X: np.ndarray            # fp32 rows as the call receives them
    eps2: float              # threshold on D (cosine: 2 eps)
    min_samples: int
    metric: str
    lattice: bool            # exact contract (no band)
    deg: np.ndarray          # eps-degree, self included
    core: np.ndarray
    root: np.ndarray         # smallest core index of the component (core), i (non-core)
    has_core_nb: np.ndarray  # non-core with a core neighbour (border)
    dmin_core: np.ndarray    # min D over core neighbours (inf: none)
    nearest: np.ndarray      # lowest index among the exactly nearest core neighbours (-1: none)
    adj: Optional[np.ndarray] = None  # dense *in* matrix where the case is small enough

    @property
    def N(self) -> int:
        return self.X.shape[0]

    @property
    def noise(self) -> np.ndarray:
        return ~self.core & ~self.has_core_nb

    def dist(self, I, J) -> np.ndarray:
        I, J = np.asarray(I), np.asarray(J)
        if self.metric == "cosine":
            Xh, zero = _unit64(self.X)
            D = sqdist64(Xh, I, J)
            D = np.where(zero[I] | zero[J], 2.0, D)
        else:
            D = sqdist64(self.X, I, J)
        return np.where(I == J, 0.0, D)

    def band(self, I, J) -> np.ndarray:
        I, J = np.asarray(I), np.asarray(J)
        if self.lattice:
            return np.zeros(I.shape)
        n = self.X.shape[1]
        if self.metric == "cosine":
            return np.full(I.shape, c_cos(n) * U * 4.0)
        r = centred_norms(self.X)
        return c_of_n(n) * U * (r[I] + r[J]) ** 2

    def is_in(self, I, J) -> np.ndarray:
        I, J = np.asarray(I), np.asarray(J)
        D, E = self.dist(I, J), self.band(I, J)
        inn, out = (D <= self.eps2 - E) | (I == J), D > self.eps2 + E
        assert (inn | out).all(), "undecided pair"
        return inn

    def cluster_ids(self) -> np.ndarray:
        """sklearn's numbering: clusters by ascending first core point; -1 where not core."""
        roots = np.unique(self.root[self.core])
        ids = np.searchsorted(roots, self.root)
        return np.where(self.core, ids, -1)


def centred_norms(X: np.ndarray) -> np.ndarray:
    X64 = np.asarray(X, np.float64)
    t = X64 - X64.mean(0)
    return np.sqrt((t * t).sum(1))


def dense_matrices(X: np.ndarray, metric: str, lattice: bool):
    """(D, band) as dense fp64 matrices."""
    N, n = X.shape
    if metric == "cosine":
        Xh, zero = _unit64(X)
        D = sqdist64(Xh)
        D[zero, :] = 2.0
        D[:, zero] = 2.0
        E = np.full((N, N), 0.0 if lattice else c_cos(n) * U * 4.0)
    else:
        D = sqdist64(X)
        r = centred_norms(X)
        E = np.zeros((N, N)) if lattice else c_of_n(n) * U * (r[:, None] + r[None, :]) ** 2
    np.fill_diagonal(D, 0.0)
    return D, E


def undecided(D: np.ndarray, E: np.ndarray, eps2: float) -> np.ndarray:
    und = ~(D <= eps2 - E) & ~(D > eps2 + E)
    np.fill_diagonal(und, False)  # D_ii = 0 is a neighbour for every eps >= 0
    return und


def _components(inn: np.ndarray, core: np.ndarray) -> np.ndarray:
    N = core.shape[0]
    root = np.arange(N)
    cidx = np.nonzero(core)[0]
    if cidx.size:
        ncomp, comp = connected_components(csr_matrix(inn[np.ix_(cidx, cidx)]), directed=False)
        mins = np.full(ncomp, N)
        np.minimum.at(mins, comp, cidx)
        root[cidx] = mins[comp]
    return root


def make_oracle(X: np.ndarray, eps2: float, min_samples: int, metric: str = "euclidean",
                lattice: bool = False) -> Oracle:
    X = np.ascontiguousarray(X, np.float32)
    if lattice:
        assert_lattice(X)
    D, E = dense_matrices(X, metric, lattice)
    assert not undecided(D, E, eps2).any(), "undecided pair left in the case"
    inn = D <= eps2 - E
    np.fill_diagonal(inn, True)
    deg = inn.sum(1)
    core = deg >= min_samples
    Dc = np.where(inn & core[None, :], D, np.inf)
    dmin = Dc.min(1)
    has = np.isfinite(dmin) & ~core
    nearest = np.where(has, Dc.argmin(1), -1)  # argmin: the first, i.e. lowest, index of the minimum
    return Oracle(X, float(eps2), int(min_samples), metric, lattice, deg, core, _components(inn, core), has,
                  np.where(has, dmin, np.inf), nearest, inn)


def make_oracle_1d(X: np.ndarray, e: int, min_samples: int) -> Oracle:
    """Lattice oracle of integer positions on a line (n = 1), eps = e, by sorting: no N x N matrix
    (the grid-cap case has 16385 rows). On a line the core-core graph links two cores exactly when
    every gap between consecutive cores from one to the other is <= e."""
    X = np.ascontiguousarray(X, np.float32)
    assert X.shape[1] == 1
    assert_lattice(X)
    x = X[:, 0].astype(np.int64)
    N = x.size
    xs = np.sort(x)
    deg = np.searchsorted(xs, x + e, "right") - np.searchsorted(xs, x - e, "left")
    core = deg >= min_samples
    root = np.arange(N)
    has = np.zeros(N, bool)
    dmin = np.full(N, np.inf)
    nearest = np.full(N, -1)
    cidx = np.nonzero(core)[0]
    if cidx.size:
        o = cidx[np.argsort(x[cidx], kind="stable")]
        cx = x[o]
        start = np.concatenate([[True], np.diff(cx) > e])
        seg = np.cumsum(start) - 1
        mins = np.minimum.reduceat(o, np.nonzero(start)[0])
        root[o] = mins[seg]
        # lowest core index at every occupied core position
        pstart = np.concatenate([[True], np.diff(cx) != 0])
        ppos = cx[pstart]
        pmin = np.minimum.reduceat(o, np.nonzero(pstart)[0])
        nb = np.nonzero(~core)[0]
        k = np.searchsorted(ppos, x[nb])
        left = np.clip(k - 1, 0, ppos.size - 1)
        right = np.clip(k, 0, ppos.size - 1)
        dl, dr = np.abs(x[nb] - ppos[left]), np.abs(x[nb] - ppos[right])
        d = np.minimum(dl, dr)
        cand = np.where(dl < dr, pmin[left], np.where(dr < dl, pmin[right], np.minimum(pmin[left], pmin[right])))
        ok = d <= e
        has[nb] = ok
        dmin[nb[ok]] = (d[ok] ** 2).astype(np.float64)
        nearest[nb[ok]] = cand[ok]
    return Oracle(X, float(e * e), int(min_samples), "euclidean", True, deg, core, root, has, dmin, nearest, None)


# --------------------------------------------------------------------------------------- the checker
def check_sweeps(orc: Oracle, counts, parent, best, keys: bool = False) -> dict:
    """counts / compressed parent / best of ``ops.dbscan_degree`` + ``dbscan_link`` + ``uf_compress``
    against the oracle. ``keys``: also hold the fp32 distance in every key to the band (valid where
    the rows the sweeps ran on are the oracle's rows about their mean). Returns the worst
    key error / band ratio seen (generic cases)."""
    N = orc.N
    counts, parent, best = (np.asarray(a).astype(np.int64) for a in (counts, parent, best))
    bad = np.nonzero(counts != orc.deg)[0]
    assert bad.size == 0, "degrees differ at %d rows, e.g. row %d: %d, oracle %d" % (
        bad.size, bad[0], counts[bad[0]], orc.deg[bad[0]])
    idx = np.arange(N)
    bad = np.nonzero(parent != orc.root)[0]
    assert bad.size == 0, "roots differ at %d rows, e.g. row %d (core %d): %d, oracle %d" % (
        bad.size, bad[0], orc.core[bad[0]], parent[bad[0]], orc.root[bad[0]])
    assert (parent[~orc.core] == idx[~orc.core]).all()
    none = best == -1
    bad = np.nonzero(none != ~orc.has_core_nb)[0]
    assert bad.size == 0, "best == -1 differs from 'no core neighbour' at %d rows, e.g. %d" % (bad.size, bad[0])
    b = np.nonzero(~none)[0]
    ratio = 0.0
    if b.size:
        j = best[b] & 0xFFFFFFFF
        assert (j < N).all(), "key names a row past N"
        assert orc.core[j].all(), "key names a non-core point"
        assert orc.is_in(b, j).all(), "key names a point that is not a neighbour"
        Dj = orc.dist(b, j)
        ns = orc.nearest[b]
        assert (Dj <= orc.dmin_core[b] + orc.band(b, j) + orc.band(b, ns)).all(), "key is not the nearest core"
        if orc.lattice:
            assert np.array_equal(j, ns), "ties go to the lowest index among the nearest cores"
            assert np.array_equal((best[b] >> 32) & 0xFFFFFFFF, orderable(Dj.astype(np.float32)))
        elif keys:
            r = np.abs(key_dist(best[b]) - Dj) / orc.band(b, j)
            ratio = float(r.max())
            assert ratio <= 1.0, "key distance off by %.3g bands at row %d" % (ratio, b[r.argmax()])
    return {"key_ratio": ratio, "borders": int(b.size)}


def check_labels(orc: Oracle, labels, chosen=None, core_idx=None) -> None:
    """Labels against the oracle: -1 exactly on its noise, clusters numbered by ascending first core
    point, every border point in the cluster of a core point that is *in* (of ``chosen`` where the
    oracle has no dense matrix)."""
    labels = np.asarray(labels).astype(np.int64)
    assert labels.shape == (orc.N,)
    if core_idx is not None:
        assert np.array_equal(np.asarray(core_idx), np.nonzero(orc.core)[0]), "core_sample_indices_ differ"
    bad = np.nonzero((labels == -1) != orc.noise)[0]
    assert bad.size == 0, "noise differs at %d rows, e.g. %d" % (bad.size, bad[0])
    ids = orc.cluster_ids()
    bad = np.nonzero(orc.core & (labels != ids))[0]
    assert bad.size == 0, "core labels differ at %d rows, e.g. row %d: %d, oracle %d" % (
        bad.size, bad[0], labels[bad[0]], ids[bad[0]])
    b = np.nonzero(orc.has_core_nb)[0]
    if not b.size:
        return
    if orc.adj is not None:
        ok = (orc.adj[b] & orc.core[None, :] & (labels[None, :] == labels[b, None])).any(1)
        assert ok.all(), "border row %d carries the label of no adjacent core point" % b[np.argmin(ok)]
    else:
        assert chosen is not None
        j = np.asarray(chosen).astype(np.int64)[b] & 0xFFFFFFFF
        assert orc.core[j].all() and orc.is_in(b, j).all() and np.array_equal(labels[b], ids[j])


def oracle_result(orc: Oracle):
    """(counts, parent, best, labels) a correct implementation returns on a lattice case."""
    b = np.nonzero(orc.has_core_nb)[0]
    best = np.full(orc.N, -1, np.int64)
    best[b] = pack_key(orc.dmin_core[b], orc.nearest[b])
    ids = orc.cluster_ids()
    labels = ids.copy()
    labels[b] = ids[orc.nearest[b]]
    return orc.deg.copy(), orc.root.copy(), best, labels


# ------------------------------------------------------------------------------------- case builders
def assert_lattice(X: np.ndarray) -> None:
    X = np.asarray(X)
    assert np.array_equal(X, np.round(X)), "lattice rows are integers"
    assert 4.0 * X.shape[1] * float(np.abs(X).max(initial=0.0)) ** 2 < 2.0 ** 24, "fp32 exactness condition"


def lattice_sweep_case(N: int, n: int, seed: int = 0):
    """(X, eps2 = 25, min_samples): random small-integer rows whose squared distances straddle 25, with
    3-4-5 pairs at exactly eps^2 and pairs at eps^2 + 1. Every column carries signal, the last one
    of a k-tile included. min_samples is the degree nearest the median whose predecessor occurs too, so
    degree == min_samples and degree == min_samples - 1 both occur (asserted from N = 127 on)."""
    rng = np.random.default_rng(1000 * N + n + seed)
    if n == 1:
        X = rng.integers(0, max(2, 3 * N), (N, 1))
    elif n == 2:
        X = rng.integers(0, max(2, int(np.sqrt(13.0 * N))), (N, 2))
    else:
        m = max(2, int(round(np.sqrt(1.0 + 240.0 / n))))  # E[D] = n (m^2 - 1) / 6 ~ 40
        X = rng.integers(0, m, (N, n))
    X = X - X.max() // 2
    if N >= 4:  # the gadget: b, b + 5 e_0 (D 25), and for n >= 2 b + (3, .., 4) (D 25), b + (5, .., 1) (D 26)
        g = rng.choice(N, 4, replace=False)
        X[g[1:]] = X[g[0]]
        X[g[1], 0] += 5
        if n >= 2:
            X[g[2], 0] += 3
            X[g[2], n - 1] += 4
            X[g[3], 0] += 5
            X[g[3], n - 1] += 1
        else:
            X[g[2], 0] -= 5
            X[g[3], 0] += 6
    X = X.astype(np.float32)
    assert_lattice(X)
    D = sqdist64(X)
    deg = (D <= 25.0).sum(1)
    vals = np.unique(deg)
    cand = vals[np.isin(vals - 1, vals)]  # degrees whose predecessor occurs too
    med = float(np.median(deg))
    ms = int(cand[np.abs(cand - med).argmin()]) if cand.size else max(1, int(med))
    if N >= 4:
        assert (D == 25.0).any() and (n == 1 or (D == 26.0).any())
    if N >= 127:
        assert (deg == ms).any() and (deg == ms - 1).any()
    return X, 25.0, ms


def blobs(N: int, n: int, centers: int, shift: float, seed: int = 0, std: float = 1.0) -> np.ndarray:
    """Gaussian blobs about centres uniform in [-10, 10]^n, translated by ``shift``, as fp32."""
    rng = np.random.default_rng(seed)
    C = rng.uniform(-10.0, 10.0, (centers, n))
    X = C[rng.integers(0, centers, N)] + std * rng.standard_normal((N, n))
    return (X + shift).astype(np.float32)


def generic_case(X: np.ndarray, eps: float, metric: str = "euclidean") -> np.ndarray:
    """The rows of X (fp32) that leave no undecided pair: one row of every undecided pair is dropped,
    the band recomputed about the new mean, until none is left. Asserts that >= 95 % of the rows
    remain and that the band's centre condition holds (module docstring)."""
    X = np.ascontiguousarray(X, np.float32)
    N0 = X.shape[0]
    eps2 = 2.0 * eps if metric == "cosine" else eps * eps
    keep = np.arange(N0)
    while True:
        D, E = dense_matrices(X[keep], metric, False)
        I, J = np.nonzero(np.triu(undecided(D, E, eps2), 1))
        if not I.size:
            break
        drop = set()
        for a, b in zip(I.tolist(), J.tolist()):
            if a not in drop and b not in drop:
                drop.add(b)
        keep = np.delete(keep, sorted(drop))
    assert keep.size >= 0.95 * N0, "only %d of %d rows remain" % (keep.size, N0)
    Xk = X[keep]
    assert not undecided(*dense_matrices(Xk, metric, False), eps2).any()
    if metric != "cosine":
        n = Xk.shape[1]
        mu = Xk.astype(np.float64).mean(0)
        rho = np.linalg.norm(mu - mu.astype(np.float32)) / centred_norms(Xk).min()
        assert (1.0 + rho) ** 2 * (1.5 * n + 5.0) * (1.0 + 2.0 ** -10) <= c_of_n(n), "centre too coarse for the band"
    return Xk


def place(N: int, items, spacing: int = 6):
    """N lattice rows in the plane: ``items`` [(index, (x, y))] at their indices, every other index an
    isolated filler (a grid of pitch ``spacing`` > eps = 5 far below the items)."""
    X = np.zeros((N, 2), np.int64)
    used = np.zeros(N, bool)
    for i, (x, y) in items:
        assert not used[i]
        X[i] = (x, y)
        used[i] = True
    free = np.nonzero(~used)[0]
    side = int(np.ceil(np.sqrt(max(1, free.size))))
    k = np.arange(free.size)
    X[free, 0] = spacing * (k % side) - spacing * side // 2
    X[free, 1] = -200 - spacing * (k // side)
    assert all(y > -150 for _, (_, y) in items)
    X = X.astype(np.float32)
    assert_lattice(X)
    return X
