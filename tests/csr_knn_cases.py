"""Oracle, bounds, case builders and the contract checker of the sparse (CSR x CSR) kNN tests.

Oracle: the fp32 CSR densified to fp64, distances in direct form. With u = 2^-24 and
t = nnz_x + nnz_y the bounds are derived from the arithmetic, not measured:

* selection keys (sqeuclidean, expanded form |x|^2 + |y|^2 - 2 S):
      |key - D| <= eps = (t + 4) u (|x| + |y|)^2
  The dot S has at most min(nnz_x, nnz_y) <= t / 2 products, fused into the sum (one rounding per
  term, any order): |S^ - S| <= (t / 2) u |x| |y|, so 2 S carries t u |x| |y| <= (t / 4) u (|x| + |y|)^2.
  The row norms are fp32 roundings of an fp64 sum of fp32 squares (2 u each), the two additions
  of the finaliser round intermediates no larger than (|x| + |y|)^2 (2 u): 4 u (|x| + |y|)^2 together.
* refined squared distances (direct form, all terms non-negative): |d2 - D| <= (t + 4) u D. Each
  term (x - y)^2 carries 2 u from the subtraction and 1 u from the fused square-add, the sum of at
  most t terms at most t - 1 roundings along any path of the lane-strided + tree reduction.
* hellinger: |d^2 - (1 - S)| <= (t + 4) u: two fp32 square roots per product (2 u S), t / 2 fused
  products, the subtraction from 1 (u) and the fp32 square root squared again (2 u); S <= 1.
* jaccard: bit-equal to (u - S) / u in fp32 from the exact integer counts, ids included.
"""
import functools

import numpy as np
import torch

from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.core.base import CSR

U24 = 2.0 ** -24


def csr_from_rows(rows, n, device="cpu"):
    """``core.base.CSR`` (int64 / int32 / fp32) from a list of (sorted column array, value array)."""
    counts = np.array([len(c) for c, _ in rows], dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    idx = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows]) if rows else np.zeros(0, np.int32)
    val = np.concatenate([np.asarray(v, dtype=np.float32) for _, v in rows]) if rows else np.zeros(0, np.float32)
    return CSR(indptr=torch.from_numpy(indptr).to(device), indices=torch.from_numpy(idx.astype(np.int32)).to(device),
               data=torch.from_numpy(val.astype(np.float32)).to(device), shape=(len(rows), int(n)))


def csr_from_dense(X, device="cpu"):
    X = np.asarray(X, dtype=np.float32)
    return csr_from_rows([(np.nonzero(r)[0], r[np.nonzero(r)[0]]) for r in X], X.shape[1], device)


def to(A, device):
    return CSR(indptr=A.indptr.to(device), indices=A.indices.to(device), data=A.data.to(device), shape=A.shape)


def row_block(A, lo, hi):
    """Rows lo .. hi with ABSOLUTE offsets: the indptr slice is not re-based."""
    return CSR(indptr=A.indptr[lo: hi + 1], indices=A.indices, data=A.data, shape=(hi - lo, A.shape[1]))


def dense64(A):
    A = to(A, "cpu")
    m, n = A.shape
    out = torch.zeros((m, n), dtype=torch.float64)
    a = int(A.indptr[0])
    rows = torch.repeat_interleave(torch.arange(m), A.indptr[1:] - A.indptr[:-1])
    out[rows, A.indices[a: a + rows.numel()].long()] = A.data[a: a + rows.numel()].double()
    return out


def nnz_rows(A):
    return (A.indptr[1:] - A.indptr[:-1]).cpu().double()


def oracle_sq(Q, I):
    """fp64 direct-form squared distances [mq, mi] of two fp64 dense row sets. The expanded form in
    fp64 is exact to ~1e-15 (|x|^2 + |y|^2); where that is not far below u D the pair is recomputed
    term by term."""
    qn, inn = (Q * Q).sum(1), (I * I).sum(1)
    scale = qn.view(-1, 1) + inn.view(1, -1)
    D = (scale - 2.0 * (Q @ I.T)).clamp_min(0)
    close = torch.nonzero(D <= 1e-4 * scale)
    for s in range(0, close.shape[0], 4096):
        q, i = close[s: s + 4096, 0], close[s: s + 4096, 1]
        D[q, i] = ((Q[q] - I[i]) ** 2).sum(1)
    return D


class Oracle:
    """Everything the checker needs about one (queries, items) pair, computed once."""

    def __init__(self, Q, I, metric="sqeuclidean"):
        self.metric = metric
        Qd, Id = dense64(Q), dense64(I)
        self.t = nnz_rows(Q).view(-1, 1) + nnz_rows(I).view(1, -1)
        if metric == "sqeuclidean":
            self.D = oracle_sq(Qd, Id)
            s = Qd.norm(dim=1).view(-1, 1) + Id.norm(dim=1).view(1, -1)
            self.eps_key = (self.t + 4) * U24 * s * s
            self.eps = (self.t + 4) * U24 * self.D  # refined distances
        elif metric == "hellinger":
            self.D = (1.0 - Qd.sqrt() @ Id.sqrt().T).clamp_min(0)  # d^2
            self.eps = self.eps_key = (self.t + 4) * U24 * torch.ones_like(self.D)
        else:  # jaccard: the fp32 expression on exact integer counts
            qa, ia = (Qd != 0).float(), (Id != 0).float()
            S = qa @ ia.T
            uni = qa.sum(1).view(-1, 1) + ia.sum(1).view(1, -1) - S
            self.D = torch.where(uni > 0, (uni - S) / uni.clamp_min(1), torch.zeros_like(uni)).double()
            self.eps = self.eps_key = torch.zeros_like(self.D)
        # items that are bit-identical rows: first id of each group
        _, inv = np.unique(Id.numpy(), axis=0, return_inverse=True)
        first = {}
        self.dup_first = np.array([first.setdefault(int(g), i) for i, g in enumerate(inv.reshape(-1))])

    def decided(self, k):
        """Rows whose exact top-k set the bounds pin: max_topk(D + eps) < min_rest(D - eps)."""
        mi = self.D.shape[1]
        if k >= mi:
            return torch.ones(self.D.shape[0], dtype=torch.bool)
        order = torch.argsort(self.D, dim=1, stable=True)
        hi = (self.D + self.eps_key).gather(1, order[:, :k]).max(1).values
        lo = (self.D - self.eps_key).gather(1, order[:, k:]).min(1).values
        return hi < lo

    def topk_ids(self, k):
        return torch.argsort(self.D, dim=1, stable=True)[:, :k]


def check_knn(orc, dist, ids, k, which="refined", id_offset=0):
    """The contract on every row, none skipped; raises AssertionError naming the first violation.
    ``which``: "refined" (direct-form squared distances, hellinger d^2, jaccard), or "keys"
    (expanded-form selection keys: the wider per-pair bound). ``dist`` holds SQUARED distances for
    sqeuclidean / hellinger. Returns the worst error / bound ratio seen."""
    D, mi = orc.D, orc.D.shape[1]
    dist, ids = dist.detach().cpu().double(), ids.detach().cpu().long()
    mq = D.shape[0]
    assert dist.shape == (mq, k) and ids.shape == (mq, k), (dist.shape, ids.shape)
    kk = min(k, mi)
    assert torch.isinf(dist[:, kk:]).all() and (dist[:, kk:] > 0).all() and (ids[:, kk:] == -1).all(), "padding"
    dist, ids = dist[:, :kk], ids[:, :kk] - id_offset
    assert ((ids >= 0) & (ids < mi)).all(), "id out of range"
    srt = torch.sort(ids, dim=1).values
    assert (srt[:, 1:] != srt[:, :-1]).all(), "an id returned twice"
    assert torch.isfinite(dist).all() and (dist[:, 1:] >= dist[:, :-1]).all(), "distances not ascending"
    Dg = D.gather(1, ids)
    bound = (orc.eps_key if which == "keys" else orc.eps).gather(1, ids)
    err = (dist - Dg).abs()
    bad = err > bound
    assert not bad.any(), "distance off its bound at %s: err %.3e, bound %.3e" % (
        tuple(torch.nonzero(bad)[0].tolist()), float(err[bad][0]), float(bound[bad][0]))
    ratio = float((err / bound.clamp_min(1e-300))[bound > 0].max()) if (bound > 0).any() else 0.0
    if orc.metric == "jaccard":
        assert torch.equal(ids, orc.topk_ids(kk)), "jaccard ids differ from the fp32 expression's order"
    # the set: no omitted item is decidedly nearer than a returned one
    ek = orc.eps_key
    ret = torch.zeros(D.shape, dtype=torch.bool)
    ret.scatter_(1, ids, True)
    hi = torch.where(ret, D - ek, torch.full_like(D, -float("inf"))).max(1).values
    lo = torch.where(ret, torch.full_like(D, float("inf")), D + ek).min(1).values
    bad = hi > lo
    assert not bad.any(), "row %d returns an item decidedly farther than one it omits" % int(torch.nonzero(bad)[0])
    # bit-identical item rows: the lower id first
    idn = ids.numpy()
    for q in range(mq):
        pos = {int(j): p for p, j in enumerate(idn[q])}
        for j, p in pos.items():
            f = int(orc.dup_first[j])
            if f != j:
                for j2 in range(f, j):
                    if orc.dup_first[j2] == f:
                        assert j2 in pos and pos[j2] < p, "row %d: duplicate item %d before lower id %d" % (q, j, j2)
    return ratio


def random_rows(m, n, mean_nnz, seed, values="normal"):
    """Per-row non-zero counts drawn Poisson, standard-normal values; row 1 is empty and row 2 long."""
    rng = np.random.default_rng(seed)
    counts = np.minimum(rng.poisson(mean_nnz, m), n)
    if m > 2:
        counts[1] = 0
        counts[2] = min(n, 50 * mean_nnz)
    rows = []
    for c in counts:
        cols = np.sort(rng.choice(n, int(c), replace=False)) if c else np.zeros(0, np.int64)
        if values == "normal":
            v = rng.standard_normal(len(cols))
            v[v == 0] = 1.0
        elif values == "ones":
            v = np.ones(len(cols))
        else:  # "prob": non-negative rows of sum 1 (hellinger)
            v = rng.random(len(cols)) + 1e-3
            v = v / v.sum() if len(cols) else v
        rows.append((cols, v.astype(np.float32)))
    return rows


GENERIC = [(300, 5000, 12, 15), (257, 9000, 40, 33), (130, 70000, 6, 5), (513, 4097, 100, 64)]


@functools.lru_cache(maxsize=None)
def generic_case(m, n, mean_nnz, k, metric="sqeuclidean"):
    """(CSR on the CPU, Oracle) of one generic self-kNN case; at least 90 % of its rows are decided
    by the oracle alone, so the contract pins the exact neighbour set there."""
    values = {"sqeuclidean": "normal", "hellinger": "prob", "jaccard": "ones"}[metric]
    A = csr_from_rows(random_rows(m, n, mean_nnz, seed=m + n + k, values=values), n)
    orc = Oracle(A, A, metric)
    if metric == "sqeuclidean":
        share = float(orc.decided(k).double().mean())
        assert share >= 0.9, "case (%d, %d, %d, %d) decided on %.3f of its rows only" % (m, n, mean_nnz, k, share)
    return A, orc


def near_duplicates(n=3000, pairs=8, nnz=40, seed=3):
    """Rows x and x + 2^-10 e_j at |x| ~ 30: D = 2^-20 while (|x| + |y|)^2 u ~ 2e-4, the expanded form
    says nothing about D; plus unrelated rows."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(pairs):
        cols = np.sort(rng.choice(n, nnz, replace=False))
        v = rng.standard_normal(nnz).astype(np.float32)
        v *= np.float32(30.0 / np.linalg.norm(v))
        v2 = v.copy()
        v2[nnz // 2] = np.float32(v2[nnz // 2] + np.float32(2.0 ** -10))
        assert v2[nnz // 2] != v[nnz // 2]
        rows += [(cols, v), (cols, v2)]
    rows += random_rows(20, n, nnz, seed + 1)
    return csr_from_rows(rows, n)


def knn_refined(Q, I, k):
    """(squared distances, ids) as the graph builder computes them: select on keys, refine."""
    _, ids = ops.csr_knn(Q, I, k, "sqeuclidean")
    return ops.csr_refine_sort(Q, I, ids)


def check_pairdist(orc, Dm):
    """A full key matrix against the oracle; returns the worst error / bound ratio."""
    Dm = Dm.detach().cpu().double()
    assert Dm.shape == orc.D.shape and torch.isfinite(Dm).all()
    if orc.metric == "jaccard":
        assert torch.equal(Dm, orc.D), "jaccard keys are not bit-equal to the fp32 expression"
        return 0.0
    got = Dm * Dm if orc.metric == "hellinger" else Dm
    err = (got - orc.D).abs()
    bad = err > orc.eps_key
    assert not bad.any(), "key off its bound at %s: err %.3e, bound %.3e" % (
        tuple(torch.nonzero(bad)[0].tolist()), float(err[bad][0]), float(orc.eps_key[bad][0]))
    return float((err / orc.eps_key.clamp_min(1e-300))[orc.eps_key > 0].max()) if (orc.eps_key > 0).any() else 0.0


def edge_rows(m, n, seed, values="normal", full_row=True):
    """Rows that sit on the window edges of the distance kernel (window width ``ops.CSR_KNN_W``):
    an empty row, non-zeros exactly at columns W - 1 and W, a row whose non-zeros all lie in the
    last window, a row with none in the first window and one that skips a middle window, a row with
    nnz = n, rows with W-window counts around the wave-sharing threshold, a bit-identical copy of a
    row and random rows."""
    W, coop = ops.CSR_KNN_W, ops.CSR_KNN_COOP
    rng = np.random.default_rng(seed)
    base = min(n, 9)

    def pick(lo, hi, c):
        c = min(c, hi - lo)
        return lo + np.sort(rng.choice(hi - lo, c, replace=False)) if c > 0 else np.zeros(0, np.int64)

    last = ((n - 1) // W) * W
    cols = []
    for r in range(m):
        kind = r % 9
        if kind == 1:
            c = np.zeros(0, np.int64)
        elif kind == 2 and n > W:
            c = np.array([W - 1, W])
        elif kind == 3:
            c = pick(last, n, base)
        elif kind == 4 and n > W:
            c = pick(W, n, base)
        elif kind == 5 and n > 2 * W:
            c = np.concatenate([pick(0, W, 3), pick(2 * W, n, 3)])
        elif kind == 6 and full_row and n <= 2 * W + 1:
            c = np.arange(n)
        elif kind == 7:
            c = pick(0, min(n, W), coop - 1 + (r // 9) % 3)  # coop - 1, coop, coop + 1 in one window
        else:
            c = pick(0, n, base)
        cols.append(np.asarray(c, dtype=np.int64))
    rows = []
    for c in cols:
        if values == "normal":
            v = rng.standard_normal(len(c))
            v[v == 0] = 1.0
        elif values == "ones":
            v = np.ones(len(c))
        else:
            v = rng.random(len(c)) + 1e-3
            v = v / v.sum() if len(c) else v
        rows.append((c, v.astype(np.float32)))
    if m > 10:
        rows[m - 1] = (rows[0][0].copy(), rows[0][1].copy())  # a bit-identical pair: ids 0 and m - 1
    return rows


VALUES = {"sqeuclidean": "normal", "hellinger": "prob", "jaccard": "ones"}


@functools.lru_cache(maxsize=None)
def edge_case(mq, mi, n, metric="sqeuclidean", seed=0):
    """(queries, items, Oracle) on the CPU for one edge shape."""
    Q = csr_from_rows(edge_rows(mq, n, 100 + seed + mq, VALUES[metric]), n)
    I = csr_from_rows(edge_rows(mi, n, 200 + seed + mi, VALUES[metric]), n)
    return Q, I, Oracle(Q, I, metric)
