"""The fused silhouette kernel against the direct O(m^2) definition, held to the derived bound
(docs/coverage.md, "Silhouette: contract and measured error"):

  eps(i, c) = (n + 8) u (||v_i|| + ||m_c|| + sqrt t_c)^2,  u = 2^-24  (cosine: ||v|| = 1, t = 0)
  |s^_i - s_i| <= (eps(i, own) N / (N - w) + max_c eps(i, c)) / max(a_i, b_i) + 6 u
  |score^ - score| <= weighted mean of the row bounds + m 2^-53
"""
import numpy as np
import pytest
import torch

from spark_rapids_ml_nai_amd import ops
from test_silhouette import oracle

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def make_case(m, k, n, measure="squaredEuclidean", weighted=False, shift=0.0, seed=0):
    """Unit-variance blobs on ids {0, 1, k-2, k-1} whose centres alternate between the first and the
    last column tile (a row's own cluster and its best other one sit in different tiles), one
    singleton id in between when k > 4, every other id empty."""
    rng = np.random.default_rng(seed)
    used = [0, k - 1, 1, k - 2][: min(4, k)] if k > 2 else [0, 1]
    lab = np.array(used)[np.arange(m) % len(used)]
    if k > 4:
        lab[m // 2] = k // 2
    elif k == 3 and m > 6:
        lab[lab == 2] = 0  # id 2 keeps one row
        lab[m // 2] = 2
    pos = {c: j for j, c in enumerate(used + [k // 2])}
    if measure == "cosine":
        C = 10.0 * np.random.default_rng(99).standard_normal((5, n))
    else:
        C = np.zeros((5, n))
        C[:, 0] = 10.0 * np.arange(5)
    X = (rng.standard_normal((m, n)) + C[[pos[c] for c in lab]] + shift).astype(np.float32)
    w = None
    if weighted:
        w = rng.uniform(0.5, 2.0, m)
        w[m // 3] = 0.0
    return X, lab, w


def check(X, lab, w, k, measure, Xd=None, exact=False):
    """Run the kernel on ``Xd`` (default: X on the device) and hold rows and sums to the bound."""
    m, n = X.shape
    Xd = torch.from_numpy(X).cuda() if Xd is None else Xd
    wd = None if w is None else torch.from_numpy(w).cuda()
    sws, sw, rows = ops.silhouette(Xd, torch.from_numpy(lab).cuda(), k, wd, measure, rows_out=True)
    torch.cuda.synchronize()
    s, a, b = oracle(X, lab, w, measure)
    w = np.ones(m) if w is None else w
    live = w > 0
    V = X.astype(np.float64)
    V = V / np.linalg.norm(V, axis=1, keepdims=True) if measure == "cosine" else V - (w @ V) / w.sum()
    ids = np.unique(lab[live])
    W = np.stack([w * (lab == c) for c in ids], 1)
    N, own = W.sum(0), np.searchsorted(ids, lab).clip(max=len(ids) - 1)
    Mc = (W.T @ V) / N[:, None]
    r = (V * V).sum(1)
    t = np.zeros(len(ids)) if measure == "cosine" else (W.T @ r) / N
    eps = (n + 8) * U * (np.sqrt(r)[:, None] + np.linalg.norm(Mc, axis=1)[None, :] + np.sqrt(t)[None, :]) ** 2
    scored = live & (N[own] > w)
    da = np.where(scored, eps[np.arange(m), own] * N[own] / np.where(scored, N[own] - w, 1.0), 0.0)
    db = np.where(scored, eps.max(1), 0.0)
    if exact:  # lattice: every d is exact in fp32, only the epilogue rounds
        bound = np.where(scored, 6 * U, 0.0)
    else:
        assert (np.maximum(a, b)[scored] > (da + db)[scored]).all(), "case is not generic"
        bound = np.where(scored, (da + db) / np.where(scored, np.maximum(a, b), 1.0) + 6 * U, 0.0)
    err = np.abs(rows.cpu().numpy().astype(np.float64) - s)
    score, got = (w * s).sum() / w.sum(), float(sws) / float(sw)
    sbound = (w * bound).sum() / w.sum() + m * 2.0 ** -53
    print("worst row err/bound %.3f  score err/bound %.3f" % ((err[scored] / bound[scored]).max(initial=0.0),
                                                              abs(got - score) / sbound))
    assert (err <= bound).all(), (err - bound).max()
    assert abs(float(sw) - w.sum()) <= 1e-12 * w.sum()
    assert abs(got - score) <= sbound
    return rows


BASE = (257, 129, 33)
SHAPES = sorted({(2, 2, 33)} | {(m, BASE[1], BASE[2]) for m in (127, 129, 257)}
                | {(BASE[0], k, BASE[2]) for k in (2, 3, 128, 129, 257)}
                | {(BASE[0], BASE[1], n) for n in (1, 3, 32, 33, 100)})


@pytest.mark.parametrize("m,k,n", SHAPES)
def test_shapes(m, k, n):
    X, lab, w = make_case(m, k, n)
    check(X, lab, w, k, "squaredEuclidean")


@pytest.mark.parametrize("measure", ("squaredEuclidean", "cosine"))
@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("n", (32, 33))
def test_measures_and_weights(measure, weighted, n):
    X, lab, w = make_case(BASE[0], BASE[1], n, measure, weighted)
    check(X, lab, w, BASE[1], measure)


@pytest.mark.parametrize("view", ("strided", "unaligned"))
@pytest.mark.parametrize("measure", ("squaredEuclidean", "cosine"))
def test_views(view, measure):
    X, lab, w = make_case(BASE[0], BASE[1], 32, measure, True)
    big = torch.zeros((BASE[0], 36), dtype=torch.float32, device="cuda")
    Xd = big[:, :32] if view == "strided" else big[:, 1:33]  # ld = 36 > n; base 4 bytes off 16-byte alignment
    Xd.copy_(torch.from_numpy(X))
    check(X, lab, w, BASE[1], measure, Xd=Xd)


def test_far_from_origin():
    X, lab, w = make_case(*BASE, shift=1024.0)  # the bound is in centred norms: an uncentred kernel fails it
    check(X, lab, w, BASE[1], "squaredEuclidean")


def test_lattice_is_exact():
    X = np.array([[0, 0], [2, 0], [0, 2], [0, -2], [8, 8], [8, 8], [8, 8], [8, 8]], np.float32)
    lab = np.array([0, 0, 130, 130, 1, 1, 259, 259])  # cluster sizes 2: means and every d exact in fp32
    rows = check(X, lab, None, 260, "squaredEuclidean", exact=True)
    assert (rows.cpu()[[0, 4, 5, 6, 7]] == 0).all()  # a == b tie and the a = b = 0 duplicates


def test_bit_identical_runs():
    X, lab, w = make_case(*BASE, weighted=True)
    args = (torch.from_numpy(X).cuda(), torch.from_numpy(lab).cuda(), BASE[1], torch.from_numpy(w).cuda())
    one, two = ops.silhouette(*args, rows_out=True), ops.silhouette(*args, rows_out=True)
    assert all(torch.equal(x, y) for x, y in zip(one, two))
