"""Oracle, bounds, case builders and checker for the RandomForest level kernels (csrc/forest.hip:
``ops.rf_hist`` on every layout / kernel, ``ops.rf_best_split``, ``ops.rf_node_split``,
``ops.rf_left_totals``). Independent of ``ops``: plain numpy / Python integers and ``Fraction``.

Histogram contract
  counts are integers and exact on every path. Regression sums:
  * lattice cases (integer weights 0..255, y a multiple of 2^-10 with |y| <= 4, yscale =
    packed_scale = 2^20, every |cell sum| * 2^20 < 2^53): every rint is the identity and every
    conversion / fp64 add is exact, so all paths equal the oracle bit for bit;
  * generic cases: |got - sum w y| <= ``sum_bound`` (derivation in its docstring).

Split contract (``check_split``): validity, totals, n_left / n_right and the left totals exact; the
reported gain within ``band`` of the oracle's gain at the reported (slot, bin), which is within
``band`` of the oracle's maximum; where the oracle's gap to the best non-tied runner-up exceeds
2 band the reported split is one of the oracle's maximisers; among candidates whose left statistics
equal the winner's (bit-identical gain computations) the winner is the lowest (slot, bin)."""
import functools
import math
from fractions import Fraction

import numpy as np

FB = 8              # csrc/forest.hip FB (ops.RF_HIST_FB_MAX)
ITEM_T = 256        # rf_hist_kernel threads; two rows per thread and step
WIDE_T = 1024       # RHW_T
NS_T, NS_W, NS_U, NS_FL = 512, 8, 4, 4   # rf_node_split_kernel
PACK_SHIFT, PACK_BIAS = 44, 1 << 22      # RF_PACK_SHIFT, RF_PACK_BIAS
PACK_MAX_WEIGHT = (1 << 20) - 1          # sum of weights of one packed item (20 count bits)
EXCL = 1 << 30                           # RF_ITEM_EXCLUSIVE flag of item.w
U64 = 2.0 ** -53
ULD = float(np.finfo(np.longdouble).eps) / 2
LATTICE_SCALE = 2.0 ** 20
Y_UNIT = 1024                            # lattice y = k / 1024
POISON = 0xA5


# ============================================================================== histogram cases
class HistCase:
    """Feature-major ``bins`` (n, m) uint8, ``idx`` (P,) row ids, per-position ``w`` (integers as
    fp32) and ``y`` (class ids or regression labels, fp32), ``node_feats`` (nodes, nf), ``chunks``:
    per node the list of its (row_begin, row_end) chunks (empty for a node without rows)."""

    def __init__(self, name, bins, idx, w, y_row, node_feats, chunks, B, S, regression, lattice):
        # labels belong to rows (``y_row``, as ``ops`` takes them); ``y`` is the per-position stream
        self.name, self.bins, self.idx, self.w, self.y_row = name, bins, idx, w, y_row
        self.y = y_row[idx.astype(np.int64)]
        self.node_feats, self.chunks, self.B, self.S = node_feats, chunks, B, S
        self.regression, self.lattice = regression, lattice
        self.n, self.m = bins.shape
        self.nodes, self.nf = node_feats.shape
        if regression and lattice:
            self.yscale = self.packed_scale = LATTICE_SCALE
        else:
            self.yscale = self.packed_scale = None  # ops.rf_yscale / ops.rf_pack_scale in the test
        self.oracle = hist_oracle(self)
        if regression and lattice:
            # every cell's fixed-point sum below 2^53: conversions and fp64 folds are exact
            assert int(np.abs(self.oracle["sum_int"]).max(initial=0)) * (int(LATTICE_SCALE) // Y_UNIT) < 2 ** 53

    def node_range(self, node):
        ch = self.chunks[node]
        return (ch[0][0], ch[-1][1]) if ch else (0, 0)

    def items(self, fb, exclusive=False, chunks=None):
        """(node, row_begin, row_end, feature chunk [| EXCL for single-chunk nodes]) int32 rows."""
        out = []
        for node, ch in enumerate(self.chunks if chunks is None else chunks):
            flag = EXCL if (exclusive and len(ch) == 1) else 0
            for rb, re in ch:
                for fc in range((self.nf + fb - 1) // fb):
                    out.append((node, rb, re, fc | flag))
        return np.array(out, dtype=np.int32).reshape(-1, 4)

    def multi_nodes(self):
        return np.array([i for i, ch in enumerate(self.chunks) if len(ch) != 1], dtype=np.int64)


def hist_oracle(case):
    """Counts (int64) and regression sums straight from bins / idx / (w, y) / node_feats / ranges.
    Lattice sums are exact integers in units of 2^-10; generic sums are longdouble, with the
    per-cell row count, sum |w y| and sum w that the bound needs."""
    B, S, nodes, nf = case.B, case.S, case.nodes, case.nf
    wi = case.w.astype(np.int64)
    assert np.array_equal(wi.astype(np.float32), case.w) and wi.min(initial=0) >= 0
    if not case.regression:
        cls = case.y.astype(np.int64)
        assert cls.min(initial=0) >= 0 and cls.max(initial=0) < S
        cnt = np.zeros((nodes, nf, B, S), dtype=np.int64)
    else:
        cnt = np.zeros((nodes, nf, B), dtype=np.int64)
        rows = np.zeros((nodes, nf, B), dtype=np.int64)
        if case.lattice:
            yi = np.rint(case.y.astype(np.float64) * Y_UNIT).astype(np.int64)
            assert np.array_equal(yi / Y_UNIT, case.y.astype(np.float64)) and np.abs(yi).max(initial=0) <= 4 * Y_UNIT
            sum_int = np.zeros((nodes, nf, B), dtype=np.int64)
        else:
            wy = case.w.astype(np.longdouble) * case.y.astype(np.longdouble)
            sums = np.zeros((nodes, nf, B), dtype=np.longdouble)
            sabs = np.zeros((nodes, nf, B), dtype=np.float64)
    for node in range(nodes):
        rb, re = case.node_range(node)
        if re <= rb:
            continue
        r = case.idx[rb:re].astype(np.int64)
        for j in range(nf):
            b = case.bins[int(case.node_feats[node, j]), r].astype(np.int64)
            if not case.regression:
                np.add.at(cnt[node, j], (b, cls[rb:re]), wi[rb:re])
                continue
            np.add.at(cnt[node, j], b, wi[rb:re])
            np.add.at(rows[node, j], b, 1)
            if case.lattice:
                np.add.at(sum_int[node, j], b, wi[rb:re] * yi[rb:re])
            else:
                np.add.at(sums[node, j], b, wy[rb:re])
                np.add.at(sabs[node, j], b, np.abs(wy[rb:re]).astype(np.float64))
    out = {"cnt": cnt}
    if case.regression:
        out["rows"] = rows
        if case.lattice:
            out["sum_int"] = sum_int
        else:
            out["sum"], out["sabs"] = sums, sabs
    return out


def expected_hist(case):
    """The histogram as the device returns it where the contract is exact: int32 counts
    (classification) or fp64 (count, sum) (lattice regression)."""
    o = case.oracle
    if not case.regression:
        return o["cnt"].astype(np.int32)
    assert case.lattice
    return np.stack([o["cnt"].astype(np.float64), o["sum_int"].astype(np.float64) / Y_UNIT], -1)


def sum_bound(case, path, yscale, packed_scale, nchunks):
    """Per-cell bound on |got - sum w y| of a generic regression case, from the design alone
    (kernel comments, ``rf_yscale``). u = 2^-53, A = sum |w y| of the cell, r its rows, W its weight.
      * w y is exact in fp64 (8 x 24 bits); (w y) * yscale rounds once (u A in all) and rint moves
        each row by <= 0.5 steps: r * 0.5 / yscale. Packed cells round y * scale before the integer
        multiply by w: W * 0.5 / packed_scale, and u A for the scale multiply.
      * the i64 cell sum is exact; i64 -> fp64, fl(1 / scale) and the multiply by it: 3 u |sum|,
        |sum| <= A + the terms above: 4 u A covers them with the scale multiply, 5 u A with the
        second-order terms.
      * a node folded from k row chunks with fp64 atomics: (k - 1) u * sum |chunk values|
        <= (k - 1) u (A + the terms above). The fixed-point fold is exact (k = 1).
      * the longdouble oracle adds r terms in sequence: r * 2^-64 * A."""
    o = case.oracle
    A, r, W = o["sabs"], o["rows"].astype(np.float64), o["cnt"].astype(np.float64)
    if path.endswith("packed"):
        q = 0.5 * W / packed_scale
    else:
        q = 0.5 * r / yscale
    base = q + 5 * U64 * A
    k = np.array([1 if "fixed" in path else max(1, nc) for nc in nchunks], dtype=np.float64)
    fold = (k - 1)[:, None, None] * U64 * (A + base)
    return (base + fold + r * ULD * A) * (1 + 1e-9)


def check_hist(case, got, path="fm", yscale=None, packed_scale=None, nchunks=None, touched=None):
    """``got``: the (nodes, nf, B, S) histogram of ``path``. ``touched`` (poisoned-buffer runs): the
    nodes that must hold their histogram; every other node must still hold the poison bytes.
    Returns the worst error / bound ratio of the sum plane (0 where the contract is exact)."""
    got = np.asarray(got)
    nodes = case.nodes
    assert got.shape == (nodes, case.nf, case.B, case.S), (got.shape, case.name)
    keep = np.ones(nodes, dtype=bool) if touched is None else np.isin(np.arange(nodes), touched)
    raw = got.reshape(nodes, -1).view(np.uint8)
    assert (raw[~keep] == POISON).all(), "%s/%s: a node without items was written" % (case.name, path)
    if not case.regression or case.lattice:
        exp = expected_hist(case)
        assert got.dtype == exp.dtype
        a, b = got[keep].view(np.int32 if not case.regression else np.int64), \
            exp[keep].view(np.int32 if not case.regression else np.int64)
        if not np.array_equal(a, b):
            bad = np.argwhere(got[keep] != exp[keep])
            k = tuple(bad[0]) if len(bad) else tuple(np.argwhere(a != b)[0])
            raise AssertionError("%s/%s: cell %s (node, slot, bin, stat) got %r, oracle %r (%d cells differ)"
                                 % (case.name, path, k, got[keep][k], exp[keep][k], len(bad)))
        return 0.0
    o = case.oracle
    assert got.dtype == np.float64
    cnt = got[..., 0][keep]
    assert np.array_equal(cnt, o["cnt"][keep].astype(np.float64)), "%s/%s: counts differ" % (case.name, path)
    nchunks = [len(c) for c in case.chunks] if nchunks is None else nchunks
    bound = sum_bound(case, path, yscale, packed_scale, nchunks)[keep]
    err = np.abs(got[..., 1][keep].astype(np.longdouble) - o["sum"][keep]).astype(np.float64)
    assert np.isfinite(got[..., 1][keep]).all()
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max(initial=0.0))
    assert worst <= 1.0, "%s/%s: sum error / bound = %.3g at %s" % (
        case.name, path, worst, np.unravel_index(int(ratio.argmax()), ratio.shape))
    return worst


def _cut(rb, re, k):
    """[rb, re) in up to k chunks of unequal length (20 / 30 / 50 %, 40 / 60 %)."""
    n = re - rb
    k = min(k, n)
    if k <= 1:
        return [(rb, re)] if n > 0 else []
    fr = {2: (0.4,), 3: (0.2, 0.5)}[k]
    cuts = sorted({min(n - 1, max(1, int(f * n))) for f in fr})
    pts = [0] + cuts + [n]
    return [(rb + a, rb + b) for a, b in zip(pts[:-1], pts[1:]) if b > a]


@functools.lru_cache(maxsize=None)
def hist_case(name, m, n, B, S, regression, lattice, node_rows, node_chunks, nf, feats=None, seed=0,
              yshift=0.0, wmode="mixed", ymode="random"):
    """``node_rows``: rows per node (0: a node without items); ``node_chunks``: row chunks per node;
    ``feats``: explicit slot -> feature ids (every node) or None for an ascending sample per node.
    Edges planted: row ids 0 and m - 1, duplicated row ids, bins 0 and B - 1, class S - 1, weights 0
    in the first and the second row slot of a thread (item and wide kernel) and weights 255."""
    rng = np.random.default_rng(seed)
    bins = rng.integers(0, B, size=(n, m)).astype(np.uint8)
    bins[:, 0] = B - 1
    bins[:, m - 1] = 0 if m > 1 else B - 1
    P = int(sum(node_rows))
    idx = rng.integers(0, m, size=P).astype(np.int32)
    if P >= 2:
        idx[0], idx[-1] = 0, m - 1
    if P >= 4:
        idx[2] = idx[1]
    if wmode == "mixed":
        w = rng.integers(0, 256, size=P)
        w[rng.random(P) < 0.1] = 0
        w[rng.random(P) < 0.1] = 255
        for p in (0, ITEM_T, WIDE_T):  # first slot / second slot of thread 0
            if p < P:
                w[p] = 0
        if P > 1:
            w[1] = 255
    else:
        w = np.full(P, int(wmode))
    w = w.astype(np.float32)
    if not regression:
        y = rng.integers(0, S, size=m)
        if P > 1:
            y[idx[1]] = S - 1
        y = y.astype(np.float32)
    elif lattice:
        if ymode == "random":
            y = rng.integers(-4 * Y_UNIT, 4 * Y_UNIT + 1, size=m) / Y_UNIT
        else:
            y = np.full(m, float(ymode))
        y = y.astype(np.float32)
    else:
        y = (rng.standard_normal(m) + yshift).astype(np.float32)
    chunks, p = [], 0
    for rows, k in zip(node_rows, node_chunks):
        chunks.append(_cut(p, p + rows, k))
        p += rows
    nodes = len(node_rows)
    if feats is not None:
        nfeat = np.tile(np.array(feats, dtype=np.int32), (nodes, 1))
    elif nf <= n:
        nfeat = np.stack([np.sort(rng.choice(n, size=nf, replace=False)) for _ in range(nodes)]).astype(np.int32)
    else:
        nfeat = np.stack([np.sort(rng.integers(0, n, size=nf)) for _ in range(nodes)]).astype(np.int32)
    assert nfeat.shape == (nodes, nf) and nfeat.max() < n
    return HistCase(name, bins, idx, w, y, nfeat, chunks, B, S, regression, lattice)


# ------------------------------------------------------------------ faulty kernels (self-tests)
def simulate_hist(case, fb, threads=ITEM_T, rec_bytes=32, exclusive=False, packed=False, fault=None,
                  chunks=None):
    """numpy model of one launch on a poisoned buffer (multi-chunk nodes zeroed): items in order,
    first / second row slot of a thread as in the kernels, exclusive stores. ``fault`` injects one
    defect of the list in test_rf_hist_edges."""
    B, S, nf = case.B, case.S, case.nf
    reg = case.regression
    chs = case.chunks if chunks is None else chunks
    dt = np.float64 if reg else np.int32
    hist = np.frombuffer(bytes([POISON]) * (case.nodes * nf * B * S * np.dtype(dt).itemsize), dtype=dt).copy()
    hist = hist.reshape(case.nodes, nf, B, S)
    for node, ch in enumerate(chs):
        if len(ch) > 1 or not exclusive:  # an exclusive launch zeroes the multi-chunk nodes only
            hist[node] = 0
    scale = case.packed_scale if packed else case.yscale
    first = True
    for node, rb, re, fcw in case.items(fb, exclusive, chunks):
        excl, fc = bool(fcw & EXCL), int(fcw) & (EXCL - 1)
        pos = np.arange(rb, re)
        second = ((pos - rb) % (2 * threads)) >= threads
        if fault == "drop_second_slot":
            pos = pos[~second]
        if fault == "drop_row" and first:
            pos = np.delete(pos, 1)  # position 1 carries weight 255
        first = False
        r = case.idx[pos].astype(np.int64)
        w = case.w[pos].astype(np.int64)
        for j in range(fc * fb, min(nf, (fc + 1) * fb)):
            f = int(case.node_feats[node, j])
            prev = int(case.node_feats[node, j - 1])
            if fault == "prev_group_byte" and j > fc * fb and f // rec_bytes != prev // rec_bytes:
                f -= rec_bytes  # the byte of the record still held from the previous group
                f = f if f >= 0 else 0
            b = case.bins[f, r].astype(np.int64)
            if reg:
                local = np.zeros((B, 2), dtype=np.float64)
                yv = case.y[pos].astype(np.float64)
                if packed:
                    q = np.rint(yv * scale).astype(np.int64)
                    s = w * (q + (PACK_BIAS if fault == "packed_no_bias" else 0))
                else:
                    s = np.rint(w * yv * scale).astype(np.int64)
                si = np.zeros(B, dtype=np.int64)
                ci = np.zeros(B, dtype=np.int64)
                np.add.at(ci, b, w)
                np.add.at(si, b, s + (w if fault == "count_in_sum" else 0))
                local[:, 0], local[:, 1] = ci, si.astype(np.float64) * (1.0 / scale)
            else:
                local = np.zeros((B, S), dtype=np.int64)
                c = case.y[pos].astype(np.int64)
                if fault == "swap_bin_class":
                    ok = (c < B) & (b < S)
                    np.add.at(local, (c[ok], b[ok]), w[ok])
                else:
                    np.add.at(local, (b, c), w)
            local = local.astype(dt)
            if excl:
                if fault == "excl_zero_not_stored":
                    hist[node, j][local != 0] = local[local != 0]
                else:
                    hist[node, j] = local
            elif fault == "multi_stored":
                hist[node, j] = local
            else:
                hist[node, j] += local
    return hist


# ================================================================================= split oracle
class SplitOracle:
    """Exact gains of every valid (slot, bin) of one node. ``cnt``: (nf, B, S) integers
    (classification) or (nf, B) with ``sums`` (nf, B) integers over ``unit`` (regression: fp64
    histogram cells are dyadic rationals, so any fp64 histogram has such integers)."""

    def __init__(self, cnt, crit, min_leaf, min_gain, sums=None, unit=1, sabs=None, B_u=0.0):
        self.crit, self.min_leaf, self.min_gain = crit, min_leaf, min_gain
        self.reg = crit == 2
        cnt = np.asarray(cnt, dtype=np.int64)
        self.nf, self.B = cnt.shape[:2]
        self.S = 2 if self.reg else cnt.shape[2]
        self.left = np.cumsum(cnt, axis=1)                    # prefix up to and including bin b
        if self.reg:
            self.sl = np.cumsum(np.asarray(sums, dtype=object), axis=1)
            self.unit = unit
            self.tot = (int(self.left[0, -1]), self.sl[0, -1])
            self.ntot = self.tot[0]
            self.nl = self.left
        else:
            self.tot = [int(v) for v in self.left[0, -1]]
            self.ntot = sum(self.tot)
            self.nl = self.left.sum(-1)
        self.prefix_u = B_u                                   # fp64 prefix-sum error of the sums (generic)
        nl, n = self.nl, self.ntot
        self.valid = (nl >= min_leaf) & (n - nl >= min_leaf) & (nl > 0) & (n - nl > 0)
        self.valid[:, self.B - 1] = False
        self.keys = [(int(f), int(b)) for f, b in np.argwhere(self.valid)]
        self.gain = {k: self._gain(*k) for k in self.keys}
        self.thr = max(min_gain, 1e-15)
        self._rank()

    # ---- exact / longdouble gains
    def _gain(self, f, b):
        n, nl = self.ntot, int(self.nl[f, b])
        nr = n - nl
        if self.reg:
            sl, s = self.sl[f, b], self.tot[1]
            sr = s - sl
            return (Fraction(sl * sl, nl) + Fraction(sr * sr, nr) - Fraction(s * s, n)) / n / (self.unit * self.unit)
        l = [int(v) for v in self.left[f, b]]
        r = [t - v for t, v in zip(self.tot, l)]
        if self.crit == 0:
            return (Fraction(sum(v * v for v in l), nl) + Fraction(sum(v * v for v in r), nr)
                    - Fraction(sum(v * v for v in self.tot), n)) / n
        return _entropy(self.tot, n) - np.longdouble(nl) / n * _entropy(l, nl) - np.longdouble(nr) / n * _entropy(r, nr)

    def impurity(self):
        if self.reg or self.ntot <= 0:
            return 0.0
        if self.crit == 0:
            return float(1 - Fraction(sum(v * v for v in self.tot), self.ntot * self.ntot))
        return float(_entropy(self.tot, self.ntot))

    def band(self, key=None):
        """c * u64 * scale (docs/coverage.md derives c). Classification: every term of pimp -
        nl/n imp_l - nr/n imp_r is at most scale = max(1, log2 S); S + 2 roundings per impurity
        (entropy: log2 to 2 ulp and a multiply more), 3 impurities, 5 for the combination.
        Regression: 9 roundings on terms of at most scale = (sl^2/nl + sr^2/nr + s^2/n) / n, plus
        the fp64 prefix sums of a generic histogram (prefix_u = B u * sum |cells|) through
        d gain / d s."""
        if not self.reg:
            scale = 1.0 if self.crit == 0 else max(1.0, math.log2(self.S))
            c = 3 * (self.S + 2) * (1 if self.crit == 0 else 3) + 5
            return c * U64 * scale
        n, u2 = self.ntot, self.unit * self.unit

        def one(f, b):
            nl = int(self.nl[f, b])
            nr = n - nl
            sl, s = self.sl[f, b], self.tot[1]
            sr = s - sl
            scale = float((Fraction(sl * sl, nl) + Fraction(sr * sr, nr) + Fraction(s * s, n)) / n / u2)
            d = self.prefix_u
            lin = 2 * d * (abs(float(Fraction(sl, self.unit))) / nl + abs(float(Fraction(sr, self.unit))) / nr * 2
                           + abs(float(Fraction(s, self.unit))) / n) / n + 4 * d * d / n
            return 12 * U64 * scale + lin
        if key is not None:
            return one(*key)
        return max((one(*k) for k in self.keys), default=0.0)

    def _rank(self):
        self.bnd = self.band()
        if not self.keys:
            self.max, self.maximisers, self.gap = None, [], math.inf
            return
        self.max = max(self.gain.values())
        tol = 0 if not isinstance(self.max, np.longdouble) else np.longdouble(64 * self.S) * np.longdouble(ULD)
        self.maximisers = [k for k in self.keys if self.max - self.gain[k] <= tol]
        rest = [self.gain[k] for k in self.keys if self.max - self.gain[k] > tol]
        self.gap = float(self.max - max(rest)) if rest else math.inf

    def stats(self, key):
        f, b = key
        return (int(self.nl[f, b]), self.sl[f, b]) if self.reg else tuple(int(v) for v in self.left[f, b])

    def splits(self):
        """True / False where the oracle alone decides validity, None inside the band of the threshold."""
        if self.max is None or float(self.max) < self.thr - self.bnd:
            return False
        if float(self.max) > self.thr + self.bnd:
            return True
        return None

    def decided(self):
        sp = self.splits()
        return sp is False or (sp is True and self.gap > 2 * self.bnd)


def _entropy(counts, n):
    acc = np.longdouble(0)
    for v in counts:
        if v > 0:
            p = np.longdouble(v) / np.longdouble(n)
            acc -= p * np.log2(p)
    return acc


def dyadic_ints(a):
    """fp64 array -> (Python-int object array, unit) with a == ints / unit exactly."""
    a = np.asarray(a, dtype=np.float64)
    e = 0
    for v in a.ravel():
        d = float(v).as_integer_ratio()[1]
        e = max(e, d.bit_length() - 1)
    unit = 1 << e
    ints = np.array([int(Fraction(float(v)) * unit) for v in a.ravel()], dtype=object).reshape(a.shape)
    return ints, unit


def split_oracles(hist, regression, crit, min_leaf, min_gain, sabs_u=None):
    """One ``SplitOracle`` per node of a (nodes, nf, B, S) histogram (int counts, or fp64 (count,
    sum) whose cells are taken as the exact rationals they are)."""
    hist = np.asarray(hist)
    out = []
    for node in range(hist.shape[0]):
        if regression:
            ints, unit = dyadic_ints(hist[node, :, :, 1])
            cnt = hist[node, :, :, 0]
            assert np.array_equal(cnt, np.rint(cnt))
            bu = 0.0 if sabs_u is None else float(sabs_u[node])
            out.append(SplitOracle(cnt.astype(np.int64), 2, min_leaf, min_gain, sums=ints, unit=unit, B_u=bu))
        else:
            out.append(SplitOracle(hist[node], crit, min_leaf, min_gain))
    return out


def check_split(orcs, out, totals=None, left=None, hist=None, exact_sums=True):
    """``out``: (nodes, 6) records; ``totals`` (nodes, S); ``left``: the left totals (nodes, S).
    Every node is classified; returns (decided nodes, worst gain error / band)."""
    out = np.asarray(out, dtype=np.float64)
    decided, worst = 0, 0.0
    for node, o in enumerate(orcs):
        rec = out[node]
        tag = "node %d" % node
        sp = o.splits()
        got_split = rec[1] >= 0
        if sp is not None:
            assert got_split == sp, "%s: split %s, oracle %s (max gain %s)" % (tag, got_split, sp, o.max)
        decided += o.decided()
        if totals is not None:
            t = np.asarray(totals[node], dtype=np.float64)
            if o.reg:
                assert t[0] == o.tot[0], tag
                ts = float(Fraction(o.tot[1], o.unit))
                assert t[1] == ts if exact_sums else abs(t[1] - ts) <= o.prefix_u + U64 * abs(ts), (tag, t[1], ts)
            else:
                assert np.array_equal(t, np.array(o.tot, dtype=np.float64)), (tag, t, o.tot)
        assert abs(rec[5] - o.impurity()) <= o.bnd + 4 * U64, (tag, rec[5], o.impurity())
        if not got_split:
            assert np.array_equal(rec[:5], [-1, -1, -1, 0, 0]), (tag, rec)
            if left is not None:
                assert not np.asarray(left[node]).any(), "%s: left totals of a node without a split" % tag
            continue
        key = (int(rec[1]), int(rec[2]))
        assert rec[1] == key[0] and rec[2] == key[1] and 0 <= key[0] < o.nf and 0 <= key[1] <= o.B - 2, \
            "%s: (slot, bin) %s outside the thresholds" % (tag, (rec[1], rec[2]))
        assert key in o.gain, "%s: %s is no valid threshold (min_leaf %s, n_left %s of %s)" % (
            tag, key, o.min_leaf, int(o.nl[key]), o.ntot)
        nl = int(o.nl[key])
        assert rec[3] == nl and rec[4] == o.ntot - nl, (tag, rec[3], rec[4], nl, o.ntot - nl)
        g = o.gain[key]
        b = o.bnd
        err = abs(float(np.longdouble(rec[0]) - np.longdouble(float(g)))) if not isinstance(g, np.longdouble) \
            else abs(float(np.longdouble(rec[0]) - g))
        # float(Fraction) rounds once more: u |g|
        assert err <= b + U64 * abs(float(g)), "%s: gain %r, oracle %r at %s, band %.3g" % (tag, rec[0], float(g), key, b)
        worst = max(worst, err / b if b > 0 else 0.0)
        assert float(o.max - g) <= 2 * b, "%s: %s has gain %r, the maximum is %r" % (tag, key, float(g), float(o.max))
        if o.gap > 2 * b:
            assert key in o.maximisers, "%s: %s is not among the maximisers %s" % (tag, key, o.maximisers[:4])
        st = o.stats(key)
        twin = min(k for k in o.keys if o.stats(k) == st)
        assert key == twin, "%s: tie of identical computations went to %s, not the lowest %s" % (tag, key, twin)
        if left is not None:
            lt = np.asarray(left[node], dtype=np.float64)
            if o.reg:
                assert lt[0] == st[0], tag
                ls = float(Fraction(st[1], o.unit))
                assert lt[1] == ls if exact_sums else abs(lt[1] - ls) <= o.prefix_u + U64 * abs(ls), (tag, lt, ls)
            else:
                assert np.array_equal(lt, np.array(st, dtype=np.float64)), "%s: left totals %s, oracle %s" % (tag, lt, st)
    return decided, worst


def emulate_best_split(hist, regression, crit, min_leaf, min_gain, fault=None):
    """fp64 model of the split kernels (same formulas, same order of preference) with one injected
    fault: "min_leaf_strict", "tie_high_slot", "last_bin", "left_short". Returns (out, totals, left)."""
    hist = np.asarray(hist)
    nodes, nf, B, S = hist.shape
    out = np.zeros((nodes, 6))
    totals = np.zeros((nodes, S))
    left_out = np.zeros((nodes, S))

    def imp(s, n):
        if n <= 0:
            return 0.0
        p = s / n
        if crit == 0:
            return 1.0 - float((p * p).sum())
        return float(-(p[p > 0] * np.log2(p[p > 0])).sum())

    for node in range(nodes):
        h = hist[node].astype(np.float64)
        tot = h[0].sum(0)
        ntot = tot[0] if regression else tot.sum()
        pimp = 0.0 if regression else imp(tot, ntot)
        best, bkey = -1.0, None
        for f in range(nf):
            pre = np.cumsum(h[f], axis=0)
            for b in range(B if fault == "last_bin" else B - 1):
                l = pre[b]
                nl = l[0] if regression else l.sum()
                nr = ntot - nl
                if fault == "last_bin" and b == B - 1:
                    if nl >= min_leaf and nl > 0 and best <= 1e-15:
                        best, bkey = 1.0, (f, b)  # the unguarded 0 / 0 of an empty right child
                    continue
                bad = (nl <= min_leaf or nr <= min_leaf) if fault == "min_leaf_strict" else (nl < min_leaf or nr < min_leaf)
                if bad or nl <= 0 or nr <= 0:
                    continue
                if regression:
                    sl, sr = l[1], tot[1] - l[1]
                    g = (sl * sl / nl + sr * sr / nr - tot[1] * tot[1] / ntot) / ntot
                else:
                    g = pimp - nl / ntot * imp(l, nl) - nr / ntot * imp(tot - l, nr)
                if g > best or (fault == "tie_high_slot" and g == best and bkey is not None and f > bkey[0]):
                    best, bkey = g, (f, b)
        ok = bkey is not None and best > 1e-15 and (best > min_gain)
        totals[node] = tot
        if not ok:
            out[node] = [-1, -1, -1, 0, 0, pimp]
            continue
        f, b = bkey
        l = h[f, : b + 1].sum(0)
        nl = l[0] if regression else l.sum()
        out[node] = [best, f, b, nl, ntot - nl, pimp]
        left_out[node] = h[f, :b].sum(0) if fault == "left_short" else l
    return out, totals, left_out


# ================================================================================== split cases
@functools.lru_cache(maxsize=None)
def class_hist(nodes, nf, B, S, seed, mass=200, dup=True, wmax=3):
    """Random class-count histograms (every slot of a node sums to the node's totals, as a real
    histogram does): ``mass`` rows per node thrown into the bins of each slot independently. With
    ``dup`` slot nf - 1 repeats slot 0 (a duplicated column: an exact tie whenever slot 0 wins)."""
    rng = np.random.default_rng(seed)
    hist = np.zeros((nodes, nf, B, S), dtype=np.int32)
    for node in range(nodes):
        rows = int(rng.integers(max(2, mass // 2), mass + 1))
        c = rng.integers(0, S, size=rows)
        w = rng.integers(1, wmax + 1, size=rows)
        sig = rng.integers(0, nf)  # one informative slot: class-dependent bins
        for f in range(nf):
            b = rng.integers(0, B, size=rows)
            if f == sig:
                b = np.clip((c * B) // S + rng.integers(-1, 2, size=rows), 0, B - 1)
            np.add.at(hist[node, f], (b, c), w)
        if dup and nf > 1:
            hist[node, nf - 1] = hist[node, 0]
    return hist


@functools.lru_cache(maxsize=None)
def reg_hist(nodes, nf, B, seed, lattice=True, mass=200, yshift=0.0, dup=True):
    """Regression (count, sum) fp64 histograms: lattice sums are multiples of 2^-10, generic ones the
    fp64 sums of fp32 labels. Returns (hist, sum |cells| per node for the prefix term of the band)."""
    rng = np.random.default_rng(seed)
    hist = np.zeros((nodes, nf, B, 2), dtype=np.float64)
    for node in range(nodes):
        rows = int(rng.integers(max(2, mass // 2), mass + 1))
        w = rng.integers(1, 4, size=rows).astype(np.float64)
        sig = rng.integers(0, nf)
        if lattice:
            y = rng.integers(-4 * Y_UNIT, 4 * Y_UNIT + 1, size=rows) / Y_UNIT
        else:
            y = (rng.standard_normal(rows) + yshift).astype(np.float32).astype(np.float64)
        order = np.argsort(y)
        for f in range(nf):
            b = rng.integers(0, B, size=rows)
            if f == sig:
                b[order] = np.clip((np.arange(rows) * B) // rows + rng.integers(-1, 2, size=rows), 0, B - 1)
            np.add.at(hist[node, f, :, 0], b, w)
            np.add.at(hist[node, f, :, 1], b, w * y)
        if dup and nf > 1:
            hist[node, nf - 1] = hist[node, 0]
    sabs = np.abs(hist[..., 1]).sum(-1).max(-1)
    return hist, sabs


def assert_decided(orcs, frac=0.9):
    d = sum(o.decided() for o in orcs)
    assert d >= frac * len(orcs), "only %d of %d nodes are decided by the oracle alone" % (d, len(orcs))
    return d
