"""Oracles, bounds, case builders and contract checkers of the top-k selection and exact kNN tests.

Selection (``ops.topk_rows``): per row the k smallest by (value, column), values compared
numerically (signed zeros tie, NaN is excluded from every case), ascending, id = ``ids[r, c]`` or
``id_base + c``, ``+inf`` / ``-1`` past L. The operation is exact, no tolerance is used.

kNN (``ops.knn``, ``ops.knn_refine_sort``): fp64 direct-form D = sum_j (q_j - x_j)^2 on the fp32
operands, or -2 q.x for the inner-product form. With u = 2^-24 the bounds are derived from the
arithmetic, never fitted to a kernel's output:

* selection keys (expanded form ||q||^2 + ||x||^2 - 2 q.x): |key - D| <= eps = c(n) u (||q|| + ||x||)^2,
  c(n) = 3 n / 2 + 3, in units of u S^2 with S = ||q|| + ||x||:
    - the dot product, n fused terms on ``mfma_f32_32x32x2f32`` over the k-tiles (one rounding per
      term, any order; the zero padding of the last k-tile adds exact zeros): n u ||q|| ||x||,
      doubled, with ||q|| ||x|| <= S^2 / 4: n / 2;
    - ``row_sqnorm`` of both rows: n squares added in some order, at most n roundings on any path:
      n u (||q||^2 + ||x||^2) <= n;
    - the finaliser ``fmaf(-2, acc, inorm)``: one rounding of a value <= S^2: 1;
    - ``+ qnorm``: one rounding of a value <= S^2: 1; the clamp at 0 moves a key towards D >= 0;
    - second-order terms: (3 n / 2 + 2)^2 u < 1 for n <= 2048: 1.
* inner-product keys (``inorm = qnorm = 0``: the finaliser and the add are exact):
  |key + 2 q.x| <= 2 n u sum_j |q_j x_j|.
* refined squared distances (direct form, all terms non-negative): |d - D| <= (n + 4) u D. Each term
  (q - x)^2 carries 2 u from the subtraction and u from the fused square-add; the sum of n terms
  adds at most n - 1 roundings on any path of the lane-strided + tree reduction (lanes past n hold
  exact zeros), one u of second-order slack.
* refined inner products: |d + 2 q.x| <= 2 (n + 2) u sum_j |q_j x_j|: n fused terms (or n rounded
  products and n - 1 additions on the host), the factor -2 exact, 2 u of slack.

Lattice cases hold small integers with 4 n max|x|^2 < 2^24 (asserted): every product, every partial
sum, the norms and both additions of the finaliser are integers below 2^24 in any order, so keys,
ids and tie order must equal the oracle exactly.
"""
import functools

import numpy as np
import torch

U24 = 2.0 ** -24
TK_T = 256                      # threads of topk_rows_kernel = columns of one collection block
TK_SHIFTS = (21, 10, 0)         # digit shifts of the three radix passes (11 / 11 / 10 bits)
TK_BUCKETS = (2048, 2048, 1024)
TK_SHARE = 8                    # buckets scanned by one thread
KEY_ONE = 0xBF800000            # orderable(1.0f)


# ------------------------------------------------------------------------------------------
# selection
# ------------------------------------------------------------------------------------------
def orderable(v):
    """The kernel's monotone fp32 -> uint32 key map (``csrc/tile.h``), in numpy."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def from_keys(keys):
    """fp32 values whose ``orderable`` keys are ``keys``."""
    k = np.asarray(keys, dtype=np.uint32)
    bits = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32)
    v = bits.view(np.float32)
    assert not np.isnan(v).any(), "a key that maps to NaN"
    return v


def select_oracle(vals, k, ids=None, id_base=0):
    """(values fp32 [rows, k], ids int64 [rows, k], columns int64 [rows, k], -1 past L)."""
    vals = np.asarray(vals, dtype=np.float32)
    assert not np.isnan(vals).any(), "NaN is excluded from every case"
    rows, L = vals.shape
    kk = min(k, L)
    # + 0.0 makes -0.0 a +0.0: signed zeros tie; the stable sort keeps the lower column
    order = np.argsort(vals.astype(np.float64) + 0.0, axis=1, kind="stable")[:, :kk]
    ov = np.full((rows, k), np.inf, dtype=np.float32)
    oi = np.full((rows, k), -1, dtype=np.int64)
    oc = np.full((rows, k), -1, dtype=np.int64)
    ov[:, :kk] = np.take_along_axis(vals, order, 1)
    oc[:, :kk] = order
    oi[:, :kk] = np.take_along_axis(np.asarray(ids, dtype=np.int64), order, 1) if ids is not None \
        else order + np.int64(id_base)
    return ov, oi, oc


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def check_select(vals, k, out_v, out_i, ids=None, id_base=0):
    """The selection contract on every row; raises AssertionError naming the first violation."""
    vals = np.asarray(vals, dtype=np.float32)
    out_v, out_i = _np(out_v), _np(out_i)
    rows, L = vals.shape
    assert out_v.shape == (rows, k) and out_i.shape == (rows, k), (out_v.shape, out_i.shape)
    assert out_v.dtype == np.float32 and out_i.dtype == np.int64, (out_v.dtype, out_i.dtype)
    kk = min(k, L)
    ev, ei, ec = select_oracle(vals, k, ids, id_base)
    assert (out_i[:, kk:] == -1).all(), "padding id is not -1"
    assert np.array_equal(out_v[:, kk:].view(np.uint32), ev[:, kk:].view(np.uint32)), "padding value is not +inf"
    assert not np.isnan(out_v).any(), "NaN returned"
    assert (out_v[:, 1:] >= out_v[:, :-1]).all(), "row not ascending"
    bad = out_i != ei
    assert not bad.any(), "ids differ from the oracle's at (row, rank) %s: got %d, want %d" % (
        tuple(np.argwhere(bad)[0]), out_i[bad][0], ei[bad][0])
    # the ids are the oracle's, so its columns are the returned ones
    src = np.take_along_axis(vals, ec[:, :kk], 1)
    got = out_v[:, :kk]
    assert (got == src).all(), "a value is not the input value of its id"
    nz = src != 0
    assert np.array_equal(got.view(np.uint32)[nz], src.view(np.uint32)[nz]), "a non-zero value is not bit-equal"


def bits_equal(a, b):
    """Bit-for-bit equality of two results (fp32 or int64 tensors / arrays)."""
    a, b = _np(a), _np(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


def model_select(vals, k, ids=None, id_base=0, slice_len=None, fault=None):
    """numpy model of the sliced select (per-slice lists merged with their ids), with the injected
    faults of the checker tests."""
    vals = np.array(vals, dtype=np.float32)
    rows, L = vals.shape
    if fault == "dropped_column":  # one that belongs to row 0's result
        vals[0, np.argmin(vals[0])] = np.inf
    if fault == "next_value":  # the (k + 1)-th value where the k-th belongs
        v, i, _ = select_oracle(vals, k + 1, ids, id_base)
        v, i = np.delete(v, k - 1, 1), np.delete(i, k - 1, 1)
        return v, i
    S = max(int(slice_len or L), k)
    pv, pi = [], []
    for c0 in range(0, L, S):
        sl = slice(c0, min(L, c0 + S))
        base = 0 if fault == "ignored_id_base" else id_base
        off = 0 if fault == "lost_c0" else c0
        v, i, _ = select_oracle(vals[:, sl], k, ids[:, sl] if ids is not None else None, base + off)
        pv.append(v)
        pi.append(i)
    v, i, _ = select_oracle(np.concatenate(pv, 1), k, np.concatenate(pi, 1))
    kk = min(k, L)
    if fault == "swapped_ties":
        r, j = np.argwhere(v[:, 1:kk] == v[:, :kk - 1])[0]
        i[r, [j, j + 1]] = i[r, [j + 1, j]]
    if fault == "padding_id":
        i[:, kk:] = 0
    if fault == "foreign_value":
        v[0, 0] = np.nextafter(v[0, 0], np.float32(-np.inf))
    if fault == "unsorted":
        v[0, [0, kk - 1]] = v[0, [kk - 1, 0]]
        i[0, [0, kk - 1]] = i[0, [kk - 1, 0]]
    return v, i


def kth_digit_row(p, digit, rng, below=150, inside=100, above=350, rank=50):
    """(row fp32, k): the k-th smallest key of the row has ``digit`` in radix pass ``p``; all keys
    share the digits of the earlier passes with 1.0f, so pass p is the first to split them. Bucket 3
    of pass 0 holds -inf only and bucket 2044 +inf only (the other keys there, and every key of
    buckets 0 .. 2 and 2045 .. 2047, are NaN): the first and last buckets a NaN-free row reaches."""
    shift, nb = TK_SHIFTS[p], TK_BUCKETS[p]
    lo_ok, hi_ok = (4, 2043) if p == 0 else (0, nb - 1)   # digits whose every key is a finite number
    prefix = KEY_ONE & ~((1 << (32 - 11 * p)) - 1) if p else 0   # the 11 p leading bits of 1.0f's key
    low = lambda c: rng.integers(0, 1 << shift, c, dtype=np.uint64) if shift else np.zeros(c, np.uint64)  # noqa: E731

    def keys(digits):
        return (np.uint64(prefix) | (digits.astype(np.uint64) << np.uint64(shift)) | low(len(digits))).astype(np.uint32)

    parts = []
    nlow = below if digit > lo_ok else 0
    if nlow:
        parts.append(keys(rng.integers(max(lo_ok, digit - 5), digit, nlow)))
    if p == 0 and digit in (3, 2044):
        parts.append(np.full(inside, 0x007FFFFF if digit == 3 else 0xFF800000, dtype=np.uint32))
    else:
        parts.append(keys(np.full(inside, digit)))
    if digit < hi_ok:
        parts.append(keys(rng.integers(digit + 1, min(hi_ok, digit + 5) + 1, above)))
    k = nlow + rank
    allk = rng.permutation(np.concatenate(parts))
    kth = np.sort(allk)[k - 1]
    assert (int(kth) >> shift) & (nb - 1) == digit, "the k-th key is not in the bucket asked for"
    return from_keys(allk), k


# ------------------------------------------------------------------------------------------
# kNN
# ------------------------------------------------------------------------------------------
def c_keys(n):
    return 1.5 * n + 3.0


def lattice(m, n, amp, seed):
    """m x n small integers in [-amp, amp] as fp32; 4 n amp^2 < 2^24 keeps every partial sum exact."""
    assert 4 * n * amp * amp < 2 ** 24, "lattice (n=%d, amp=%d) leaves the exact range" % (n, amp)
    return np.random.default_rng(seed).integers(-amp, amp + 1, (m, n)).astype(np.float32)


class KnnOracle:
    """fp64 distances and bounds of one (queries, items) pair, computed once and left unchanged."""

    def __init__(self, Q, I, inner_product=False):
        Q = np.asarray(Q, dtype=np.float32).astype(np.float64)
        I = np.asarray(I, dtype=np.float32).astype(np.float64)
        mq, n = Q.shape
        self.n, self.ip = n, inner_product
        absdot = np.abs(Q) @ np.abs(I).T
        if inner_product:
            self.D = -2.0 * (Q @ I.T)
            self.eps_key = 2.0 * n * U24 * absdot
            self.eps = 2.0 * (n + 2) * U24 * absdot
        else:
            self.D = np.empty((mq, I.shape[0]))
            step = max(1, (1 << 24) // max(1, I.shape[0] * n))
            for s in range(0, mq, step):
                self.D[s: s + step] = ((Q[s: s + step, None, :] - I[None, :, :]) ** 2).sum(-1)
            S = np.linalg.norm(Q, axis=1)[:, None] + np.linalg.norm(I, axis=1)[None, :]
            self.eps_key = c_keys(n) * U24 * S * S
            self.eps = (n + 4) * U24 * self.D
        self.order = np.argsort(self.D, axis=1, kind="stable")  # by (D, id)

    def sub(self, mq, mi):
        """The oracle of the first mq queries against the first mi items."""
        o = object.__new__(KnnOracle)
        o.n, o.ip = self.n, self.ip
        o.D, o.eps_key, o.eps = self.D[:mq, :mi], self.eps_key[:mq, :mi], self.eps[:mq, :mi]
        o.order = np.argsort(o.D, axis=1, kind="stable")
        return o

    def decided(self, k):
        """Rows whose top-k set the key bounds pin: max_topk(D + eps) < min_rest(D - eps)."""
        mi = self.D.shape[1]
        if k >= mi:
            return np.ones(self.D.shape[0], dtype=bool)
        hi = np.take_along_axis(self.D + self.eps_key, self.order[:, :k], 1).max(1)
        lo = np.take_along_axis(self.D - self.eps_key, self.order[:, k:], 1).min(1)
        return hi < lo


def check_knn(orc, dist, ids, k, which="keys", id_offset=0, exact=False, padded=False):
    """The kNN contract on every row, none skipped; raises AssertionError naming the first
    violation. ``which``: "keys" (expanded-form distances as ``ops.knn`` returns them) or "refined"
    (direct form). ``exact`` (lattice cases): distances and ids equal the oracle's bit for bit, ties
    in id order. ``padded``: k columns with +inf / -1 past the items, else min(k, items) columns.
    Returns the worst error / bound ratio seen."""
    D = orc.D
    mq, mi = D.shape
    dist, ids = _np(dist).astype(np.float64), _np(ids).astype(np.int64)
    kk = min(k, mi)
    cols = k if padded else kk
    assert dist.shape == (mq, cols) and ids.shape == (mq, cols), (dist.shape, ids.shape, (mq, cols))
    assert np.isposinf(dist[:, kk:]).all() and (ids[:, kk:] == -1).all(), "padding"
    dist, ids = dist[:, :kk], ids[:, :kk] - id_offset
    assert ((ids >= 0) & (ids < mi)).all(), "id out of range"
    srt = np.sort(ids, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "an id returned twice"
    assert np.isfinite(dist).all() and (dist[:, 1:] >= dist[:, :-1]).all(), "distances not ascending"
    if exact:
        want = orc.order[:, :kk]
        bad = ids != want
        assert not bad.any(), "ids differ from the oracle's (D, id) order at %s: got %d, want %d" % (
            tuple(np.argwhere(bad)[0]), ids[bad][0], want[bad][0])
        Dw = np.take_along_axis(D, want, 1)
        # ops.knn clamps at 0: in the inner-product form (keys -2 q.x) only the order carries information
        assert np.array_equal(dist, np.maximum(Dw, 0)), "lattice distances are not exact"
        return 0.0
    Dg = np.take_along_axis(D, ids, 1)
    bound = np.take_along_axis(orc.eps_key if which == "keys" else orc.eps, ids, 1)
    err = np.abs(dist - Dg)
    bad = err > bound
    assert not bad.any(), "distance off its bound at %s: err %.3e, bound %.3e" % (
        tuple(np.argwhere(bad)[0]), err[bad][0], bound[bad][0])
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    # the set: no omitted item is decidedly nearer than a returned one
    ek = orc.eps_key
    ret = np.zeros(D.shape, dtype=bool)
    np.put_along_axis(ret, ids, True, 1)
    hi = np.where(ret, D - ek, -np.inf).max(1)
    lo = np.where(ret, np.inf, D + ek).min(1)
    bad = hi > lo
    assert not bad.any(), "row %d returns an item decidedly farther than one it omits" % int(np.argwhere(bad)[0, 0])
    dec = orc.decided(kk)
    assert np.array_equal(srt[dec], np.sort(orc.order[dec, :kk], axis=1)), "a decided row's set is not the oracle's"
    return ratio


@functools.lru_cache(maxsize=None)
def lattice_case(mq, mi, n, amp=3, seed=0, inner_product=False, dups=()):
    """(Q, I, KnnOracle) of a lattice case; ``dups``: item ids overwritten with query row 0, so they
    are bit-identical rows at D = 0 from it and must come back in id order."""
    Q = lattice(mq, n, amp, 1000 + seed + n)
    I = lattice(mi, n, amp, 2000 + seed + n)
    for j in dups:
        I[j] = Q[0]
    return Q, I, KnnOracle(Q, I, inner_product)


@functools.lru_cache(maxsize=None)
def generic_case(mq, mi, n, k, seed=0, inner_product=False):
    """(Q, I, KnnOracle) of standard-normal rows; the oracle alone decides the returned set on at
    least 90 % of the rows (asserted), and the contract pins the set there."""
    rng = np.random.default_rng(3000 + seed + mq + mi + n)
    Q = rng.standard_normal((mq, n)).astype(np.float32)
    I = rng.standard_normal((mi, n)).astype(np.float32)
    orc = KnnOracle(Q, I, inner_product)
    share = float(orc.decided(min(k, mi)).mean())
    assert share >= 0.9, "generic case (%d, %d, %d, %d) decided on %.3f of its rows only" % (mq, mi, n, k, share)
    return Q, I, orc


def near_duplicates(n=40, pairs=8, seed=3):
    """Rows x and x + 2^-10 e_j at ||x|| = 30 (D = 2^-20 while u (||x|| + ||y||)^2 ~ 2e-4: the expanded
    form says nothing about D), plus unrelated rows."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(pairs):
        v = rng.standard_normal(n).astype(np.float32)
        v *= np.float32(30.0 / np.linalg.norm(v))
        v2 = v.copy()
        v2[n // 2] = np.float32(v2[n // 2] + np.float32(2.0 ** -10))
        assert v2[n // 2] != v[n // 2]
        rows += [v, v2]
    return np.concatenate([np.stack(rows), rng.standard_normal((20, n)).astype(np.float32)])


def expanded_f32(Q, I):
    """The expanded form ||q||^2 + ||x||^2 - 2 q.x evaluated in fp32 (what a selection key holds)."""
    Q, I = np.asarray(Q, np.float32), np.asarray(I, np.float32)
    qn, xn = (Q * Q).sum(1, dtype=np.float32), (I * I).sum(1, dtype=np.float32)
    return np.maximum(qn[:, None] + (xn[None, :] - np.float32(2) * (Q @ I.T)), 0).astype(np.float32)


def model_knn(orc, k, dist_matrix=None, drop=None):
    """numpy model of a search: the k smallest of ``dist_matrix`` (default: the oracle's D rounded
    to fp32) by (distance, id), with the item columns ``drop`` never offered."""
    Dm = np.array(orc.D if dist_matrix is None else dist_matrix, dtype=np.float32)
    if drop is not None:
        Dm[:, drop] = np.inf
    v, i, _ = select_oracle(Dm, min(k, Dm.shape[1]))
    return v, i


def check_refine(Q, X, pos, d, p, inner_product=False, exact=False):
    """``ops.knn_refine_sort`` contract: the output positions are the input's, re-ordered by
    (distance, candidate order), missing candidates last at +inf; each distance within the refine
    bound of the oracle distance of its position (bit-equal on lattice cases). Returns the worst
    error / bound ratio."""
    Q64, X64 = np.asarray(Q, np.float32).astype(np.float64), np.asarray(X, np.float32).astype(np.float64)
    pos, d, p = _np(pos).astype(np.int64), _np(d), _np(p).astype(np.int64)
    mq, k = pos.shape
    n = Q64.shape[1]
    assert d.shape == (mq, k) and p.shape == (mq, k) and d.dtype == np.float32, (d.shape, p.shape, d.dtype)
    assert np.array_equal(np.sort(p, 1), np.sort(pos, 1)), "the output positions are not the input's"
    assert not np.isnan(d).any() and (d[:, 1:] >= d[:, :-1]).all(), "distances not ascending"
    assert (np.isposinf(d) == (p < 0)).all(), "+inf and -1 do not go together"

    def score(pp):
        rows = X64[np.maximum(pp, 0)]
        if inner_product:
            D = -2.0 * (rows * Q64[:, None, :]).sum(-1)
            b = 2.0 * (n + 2) * U24 * (np.abs(rows) * np.abs(Q64[:, None, :])).sum(-1)
        else:
            D = ((rows - Q64[:, None, :]) ** 2).sum(-1)
            b = (n + 4) * U24 * D
        return np.where(pp < 0, np.inf, D), np.where(pp < 0, 0.0, b)

    if exact:  # candidate order among ties
        Din, _ = score(pos)
        order = np.argsort(Din, axis=1, kind="stable")
        want = np.take_along_axis(pos, order, 1)
        bad = p != want
        assert not bad.any(), "positions differ from the (distance, candidate order) sort at %s" % (
            tuple(np.argwhere(bad)[0]),)
        assert np.array_equal(d.astype(np.float64), np.take_along_axis(Din, order, 1)), "lattice distances not exact"
        return 0.0
    Dg, b = score(p)
    fin = p >= 0
    err = np.abs(d.astype(np.float64)[fin] - Dg[fin])
    bad = err > b[fin]
    assert not bad.any(), "refined distance off its bound: err %.3e, bound %.3e" % (err[bad][0], b[fin][bad][0])
    pos_b = b[fin] > 0
    return float((err[pos_b] / b[fin][pos_b]).max()) if pos_b.any() else 0.0
