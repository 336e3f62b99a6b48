"""``ops.nnd_join`` (the NN-descent join on dense rows, ``csrc/nnd.hip``) and the route built on it
(``build_algo="metric_nn_descent"``) against a literal numpy oracle: the candidate set built from the
docstring, distances in fp64 from the fp32 prepared rows by scipy's definitions. Every case runs on
the torch form (CPU) and, marked ``gpu``, on the kernel.

Bounds (u = 2^-24, derived, never fitted): l1 (n + 2) u D; chebyshev 2 u D; canberra and sqeuclidean
(n + 4) u D; hamming and jaccard bit-equal to the fp32 quotient of the exact counts; hellinger (n + 4) u
on d^2; minkowski: the power sum carries (n + 6) u for p = 3 / 4 and (n + p + 2 E) u for a general p
(the subtraction's u grows p-fold, powf is assumed within E = 2 ulp, n - 1 additions), the root divides
that by p and adds its own roundings (2 ulp for cbrtf / sqrtf o sqrtf, E ulp for powf)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.core.dataframe import DataFrame
from spark_rapids_ml_nai_amd.models.knn_graph import build_knn_graph, knn_graph_metric_approx, reverse_lists
from spark_rapids_ml_nai_amd.umap import UMAP

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
U, E_POW = 2.0 ** -24, 2
CAP, STAGE = ops.NND_CAND_CAP, ops.NND_STAGE_CAP
METRICS = [("l1", 2.0), ("chebyshev", 2.0), ("canberra", 2.0), ("hamming", 2.0), ("jaccard", 2.0), ("hellinger", 2.0),
           ("sqeuclidean", 2.0), ("minkowski", 1.0), ("minkowski", 1.5), ("minkowski", 3.0), ("minkowski", 4.0)]


def rows(metric, N, n, seed=0, dup=False):
    """fp32 PREPARED rows: small integers for hamming, ~30 % non-zeros for jaccard / canberra, square roots
    of sub-unit-mass rows for hellinger; rows 3 and 5 all zero; ``dup``: the second half repeats the first."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, n))
    if metric == "hamming":
        X = rng.integers(0, 3, (N, n)).astype(np.float64)
    if metric in ("jaccard", "canberra"):
        X = X * (rng.random((N, n)) < 0.3)
    if metric == "hellinger":
        X = np.abs(X) / (np.abs(X).sum(1, keepdims=True) * 1.001)
    X[[3, 5]] = 0.0
    if dup:
        X[N // 2:] = X[: N - N // 2]
    return ops._pairdist_prepare(torch.from_numpy(X.astype(np.float32)), ops.PAIRDIST_ALIASES.get(metric, metric)).numpy()


def oracle(metric, p, x, Y):
    """(D, eps) of fp32 row x against the fp32 rows Y, on the scale the bound is stated on (hellinger: d^2)."""
    n = x.shape[0]
    x, Y = x.astype(np.float64), Y.astype(np.float64)
    t = np.abs(x - Y)
    if metric in ("hamming", "jaccard"):  # exact counts, one fp32 division
        inter, uni = ((x != 0) & (Y != 0)).sum(1), ((x != 0) | (Y != 0)).sum(1)
        num, den = ((x != Y).sum(1), np.full(len(Y), n)) if metric == "hamming" else (uni - inter, np.maximum(uni, 1))
        return (num.astype(np.float32) / den.astype(np.float32)).astype(np.float64), np.zeros(len(Y))
    if metric == "hellinger":
        return np.maximum(0.0, 1.0 - (x * Y).sum(1)), np.full(len(Y), (n + 4) * U)
    if metric == "minkowski" and p != 1.0:
        D = (t ** p).sum(1) ** (1.0 / p)
        dlt, root = ((n + 6) * U, 4 * U) if p in (3.0, 4.0) else ((n + p + 2 * E_POW) * U, 2 * E_POW * U)
        return D, (dlt * (1 + dlt) / p + root) * D
    s = np.abs(x) + np.abs(Y)
    D, c = {"l1": (t.sum(1), n + 2), "minkowski": (t.sum(1), n + 2), "chebyshev": (t.max(1), 2),
            "sqeuclidean": ((t * t).sum(1), n + 4),
            "canberra": (np.where(s > 0, t / np.where(s > 0, s, 1), 0.0).sum(1), n + 4)}[metric]
    return D, c * U * D


def graph(kind, N, kw, seed=1):
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, N, (N, kw))
    if kind == "star":    # every row lists row 0: its reverse list is longer than any R, the others' shorter
        pos[:, 0] = 0
    if kind == "same":    # all neighbours the same id
        pos[:] = pos[:, :1]
    if kind == "ragged":  # -1 padding and ids >= N
        pos = np.where(rng.random((N, kw)) < 0.3, -1, pos)
        pos[::5, -1], pos[1::5, 0] = N + 3, 2 ** 40
    return pos.astype(np.int64)


# name: (N, n, metric, p, graph, kw, k, (a, b, R), layout, (r0, r1) or None, dup rows)
CASES = {"n%d" % n: (70, n, *METRICS[j % len(METRICS)], "star", 8, 8, (3, 3, 4), "c", None, False)
         for j, n in enumerate((1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257))}
CASES.update({"m_%s_%g" % m: (90, 40, *m, "star", 10, 10, (4, 4, 8), "c", None, False) for m in METRICS})
CASES.update({
    "stage_cap": (40, STAGE, "l1", 2.0, "star", 6, 6, (2, 2, 3), "c", None, False),
    "stage_cap_1": (40, STAGE + 1, "jaccard", 2.0, "star", 6, 6, (2, 2, 3), "c", None, False),
    "stage_cap_4": (40, STAGE + 4, "jaccard", 2.0, "star", 6, 6, (2, 2, 3), "c", None, False),
    "ld_n_plus_1": (70, 64, "canberra", 2.0, "star", 8, 8, (3, 3, 4), "ld1", None, False),
    "base_off_1": (70, 64, "jaccard", 2.0, "star", 8, 8, (3, 3, 4), "off1", None, False),
    "kw1": (70, 20, "l1", 2.0, "star", 1, 1, (1, 1, 2), "c", None, False),
    "slots_511": (600, 12, "l1", 2.0, "star", 15, 15, (15, 15, CAP - 241), "c", (0, 40), False),
    "slots_512": (600, 12, "chebyshev", 2.0, "star", 15, 15, (15, 15, CAP - 240), "c", (0, 40), False),
    "slots_513_torch": (600, 12, "l1", 2.0, "star", 15, 15, (15, 15, CAP - 239), "c", (0, 8), False),
    "same_id_short_of_k": (70, 20, "jaccard", 2.0, "same", 6, 5, (3, 3, 2), "c", None, False),
    "ragged": (70, 20, "canberra", 2.0, "ragged", 8, 8, (3, 3, 4), "c", None, False),
    "no_join": (70, 20, "hellinger", 2.0, "ragged", 8, 5, (0, 0, 0), "c", None, False),
    "k1": (70, 20, "hamming", 2.0, "star", 8, 1, (3, 3, 4), "c", None, False),
    "k64": (600, 20, "sqeuclidean", 2.0, "star", 15, 64, (8, 8, 16), "c", (0, 64), False),
    "k65_torch": (600, 20, "l1", 2.0, "star", 15, 65, (8, 8, 16), "c", (0, 16), False),
    "row_block": (70, 33, "minkowski", 3.0, "star", 8, 8, (9, 9, 4), "c", (7, 65), False),
    "dup_rows": (70, 20, "l1", 2.0, "star", 8, 12, (3, 3, 4), "c", None, True),
})


def check(metric, p, X, pos, perm, off, abR, r0, keys, ids):
    """The contract of ``ops.nnd_join``'s docstring on graph rows r0 .. r0 + len(keys)."""
    N, kw = pos.shape
    a, b, R = min(abR[0], kw), min(abR[1], kw), abR[2]
    k = keys.shape[1]
    for q in range(len(keys)):
        i = r0 + q
        c = list(pos[i])
        for nb in pos[i, :a]:
            if 0 <= nb < N:
                c += list(pos[nb, :b])
        if R:
            c += [perm[e] // kw for e in range(off[i], min(off[i + 1], off[i] + R))]
        cand = np.array(sorted({int(x) for x in c if 0 <= x < N}), dtype=np.int64)
        m = min(k, len(cand))
        got, d = ids[q, :m], keys[q, :m].astype(np.float64)
        assert (ids[q, m:] == -1).all() and np.isposinf(keys[q, m:]).all(), "row %d: padding" % i
        assert len(set(got)) == m and set(got) <= set(cand), "row %d: ids %s" % (i, got)
        assert (np.diff(d) >= 0).all() and (np.diff(got)[np.diff(d) == 0] > 0).all(), "row %d: not ascending" % i
        D, eps = oracle(metric, p, X[i], X[cand])
        at = np.searchsorted(cand, got)
        err = np.abs((d * d if metric == "hellinger" else d) - D[at])
        assert (err <= eps[at]).all(), "row %d: off its bound by %g x" % (i, (err / np.maximum(eps[at], 1e-300)).max())
        out = np.setdiff1d(np.arange(len(cand)), at)
        if len(out) and m:
            assert (D[at] - eps[at]).max() <= (D[out] + eps[out]).min(), "row %d: a nearer candidate was left out" % i


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_join_matches_the_oracle(dev, name):
    N, n, metric, p, kind, kw, k, abR, layout, block, dup = CASES[name]
    X, pos = rows(metric, N, n, dup=dup), graph(kind, N, kw)
    perm, off = reverse_lists(torch.from_numpy(pos))
    r0, r1 = block or (0, N)
    buf = torch.zeros(N * (n + 1) + 1, device=dev)
    Xd = {"c": buf[: N * n].view(N, n), "ld1": buf[: N * (n + 1)].view(N, n + 1)[:, :n],
          "off1": buf[1: N * n + 1].view(N, n)}[layout]
    Xd.copy_(torch.from_numpy(X))
    args = (torch.from_numpy(pos).to(dev), perm.to(dev), off.to(dev), k, *abR, metric, p)
    keys, ids = ops.nnd_join(Xd[r0:r1], Xd, *args, row0=r0)
    assert keys.device.type == dev and keys.dtype == torch.float32 and ids.dtype == torch.int64
    check(metric, p, X, pos, perm.numpy(), off.numpy(), abR, r0, keys.cpu().numpy(), ids.cpu().numpy())
    again = ops.nnd_join(Xd[r0:r1], Xd, *args, row0=r0)  # a second call repeats bit for bit
    assert torch.equal(keys.view(torch.int32), again[0].view(torch.int32)) and torch.equal(ids, again[1])


def test_constants_and_refusals():
    lib = ops.native.lib()
    assert tuple(int(lib.srml_nnd_config(j)) for j in range(4)) == (CAP, STAGE, ops.NND_KMAX, -1) == (512, 8192, 64, -1)

    def raw(k, R):  # refused before any pointer is read
        return ops.native.call_status("srml_nnd_join_f32", None, 1, 0, 4, None, 10, 4, 4, None, 15, None, None, k, 15, 15,
                                      R, 0, 2.0, None, None, None)
    assert (raw(15, CAP - 239), raw(65, 0), raw(0, 0)) == (-3, -3, -2)
    X, pos = torch.from_numpy(rows("l1", 50, 8)), torch.from_numpy(graph("star", 50, 5))
    with pytest.raises(ValueError, match="graph must be"):
        ops.nnd_join(X, X, pos[:10], None, None, 5, 2, 2, 0, "l1")
    with pytest.raises(ValueError, match="outside the graph"):
        ops.nnd_join(X[:10], X, pos, None, None, 5, 2, 2, 0, "l1", row0=45)
    with pytest.raises(ValueError, match="needs perm"):
        ops.nnd_join(X, X, pos, None, None, 5, 2, 2, 4, "l1")
    with pytest.raises(ValueError, match="'nn_descent'"):
        build_knn_graph(X, 5, "metric_nn_descent", None, 0, None, metric="euclidean")
    with pytest.raises(ValueError, match="'rp_nn_descent'"):
        build_knn_graph(sp.csr_matrix(X.numpy()), 5, "metric_nn_descent", None, 0, None, metric="jaccard")
    with pytest.raises(ValueError, match="exact search"):
        build_knn_graph(X, 5, "nn_descent", None, 0, None, metric="l1")


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("metric,p", [("manhattan", 2.0), ("jaccard", 2.0), ("hellinger", 2.0), ("minkowski", 3.0)])
def test_round0_on_every_row_is_the_exact_graph(dev, metric, p):
    """Candidate lists of N - 1 rows and no later round: the exact graph, up to the band of the bound."""
    N, k = 60, 10
    name = ops.pairdist_metric(metric, p)[0]
    Xp = rows(name, N, 24, seed=2)
    X = torch.from_numpy(Xp * Xp if name == "hellinger" else Xp).to(dev)
    d, j = build_knn_graph(X, k, "metric_nn_descent", {"cand_k": N - 1, "nnd_iters": 0}, 0, None, metric=metric, p=p)
    de, je = ops.knn_metric(X, X, k, metric, p)
    Xp = ops._pairdist_prepare(X, name).cpu().numpy()
    for i in range(N):
        D, eps = oracle(name, p, Xp[i], Xp)
        o = np.argsort(D, kind="stable")
        got, dd = j[i].cpu().numpy(), d[i].double().cpu().numpy()
        assert len(set(got)) == k and (D[got] - eps[got] <= D[o[k - 1]] + eps[o[k - 1]]).all()
        assert (np.abs((dd * dd if name == "hellinger" else dd) - D[got]) <= eps[got]).all()
        if D[o[k]] - eps[o[k]] > D[o[k - 1]] + eps[o[k - 1]]:  # the row's k-set is decided
            assert set(got) == set(je[i].tolist()) == set(o[:k])


@pytest.mark.parametrize("dev", DEVICES)
def test_rounds_never_raise_a_kth_distance(dev):
    N, k = 600, 10
    Xp = rows("l1", N, 24, seed=3)
    rounds, phases = [], {}
    d, j = knn_graph_metric_approx(torch.from_numpy(Xp).to(dev), k, "manhattan", nnd_iters=2, rounds=rounds, phases=phases)
    assert [r[0] for r in rounds] == ["candidates", "round0", "round1", "round2"] and rounds[0][1] is None
    assert {"metric_candidates", "metric_nn_descent"} <= set(phases)
    assert torch.equal(j, rounds[-1][2]) and torch.equal(d, rounds[-1][1]) and bool((j >= 0).all())
    for prev, cur in zip(rounds[1:], rounds[2:]):
        assert bool((cur[1][:, -1] <= prev[1][:, -1]).all()), "%s raised a k-th distance" % cur[0]
    d, j = d.double().cpu().numpy(), j.cpu().numpy()
    for i in range(N):
        D, eps = oracle("l1", 2.0, Xp[i], Xp[j[i]])
        assert (np.abs(d[i] - D) <= eps).all()


def _public_fit():
    X = np.random.default_rng(0).standard_normal((300, 16)).astype(np.float32)
    est = UMAP(metric="manhattan", build_algo="metric_nn_descent", random_state=0, n_epochs=20)
    model = est.fit(DataFrame.from_numpy(X))
    assert model.embedding_.shape == (300, 2) and np.isfinite(model.embedding_).all()


def test_public_fit():
    _public_fit()


@pytest.mark.gpu
def test_public_fit_on_the_device(gpu_device):
    _public_fit()


@pytest.mark.dist
def test_two_gloo_ranks_build_the_one_rank_graph():
    from spark_rapids_ml_nai_amd.parallel.launcher import run_barrier_job

    def job(ctx, _):
        from spark_rapids_ml_nai_amd.models.knn_graph import build_knn_graph as build

        X = torch.from_numpy(np.random.default_rng(4).standard_normal((201, 12)).astype(np.float32))
        return build(X, 10, "metric_nn_descent", {"nnd_iters": 1}, 0, ctx, metric="canberra")

    one = job(None, None)
    for d, j in run_barrier_job(job, [None, None], use_gpu=False):
        assert torch.equal(j, one[1]) and torch.equal(d, one[0])
