"""The approximate kNN graph of sparse rows (``build_algo="rp_nn_descent"``): exhaustive equivalence
with the exact CSR search, the monotone properties of its NN-descent rounds, repeatability, the
UMAP fit / transform / persistence route, the two-worker fit and the refusals. The device twins
are marked ``gpu``. No recall floor is asserted anywhere: the properties hold exactly."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import csr_knn_cases as C
from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.core.base import to_device
from spark_rapids_ml_nai_amd.core.dataframe import DataFrame
from spark_rapids_ml_nai_amd.models import umap as U
from spark_rapids_ml_nai_amd.models.knn_graph import build_knn_graph, knn_graph_csr, knn_graph_csr_approx
from spark_rapids_ml_nai_amd.umap import UMAP, UMAPModel
from spark_rapids_ml_nai_amd.utils.determinism import set_deterministic

CPU = torch.device("cpu")
DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
ALGO = "rp_nn_descent"
K = 10


def _device(dev):
    return torch.device(dev, 0) if dev == "cuda" else CPU


def _small_rows(metric):
    """60 x 400 rows at ~8 % density in the values the metric reads."""
    rng = np.random.default_rng(5)
    M = sp.random(60, 400, density=0.08, format="csr", random_state=rng, dtype=np.float32,
                  data_rvs=(lambda s: rng.standard_normal(s).astype(np.float32)) if metric not in ("hellinger", "jaccard")
                  else None)
    M.sort_indices()
    if metric == "jaccard":
        M.data[:] = 1.0
    if metric == "hellinger":
        M = sp.csr_matrix(sp.diags(1.0 / np.maximum(np.asarray(M.sum(1)).ravel(), 1e-30)) @ M, dtype=np.float32)
        M.sort_indices()
    return C.csr_from_rows([(M.indices[M.indptr[r]: M.indptr[r + 1]], M.data[M.indptr[r]: M.indptr[r + 1]])
                            for r in range(M.shape[0])], M.shape[1])


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("metric", ["euclidean", "l2", "sqeuclidean", "cosine", "hellinger", "jaccard"])
def test_every_row_a_candidate_gives_the_exact_graph(dev, metric):
    """Candidate lists as wide as the row count: round 0 scores every row, so the graph is the exact
    one: the oracle's contract on every row, the exact builder's ids on the decided rows."""
    dev = _device(dev)
    A = _small_rows(metric)
    kind, pre, _, _ = U.resolve_metric(metric)
    As = U._sparse_metric_rows(C.to(A, dev), metric, kind, pre)
    d, j = build_knn_graph(As, K, ALGO, {"cand_k": 64, "nnd_iters": 1}, 3, None, metric=kind)
    de, je = knn_graph_csr(As, As, K, kind)
    assert d.shape == (60, K) and j.dtype == torch.int64 and d.dtype == torch.float32
    okind = kind if kind in ("hellinger", "jaccard") else "sqeuclidean"
    orc = C.Oracle(C.to(As, "cpu"), C.to(As, "cpu"), okind)
    d, j, de, je = d.cpu(), j.cpu(), de.cpu(), je.cpu()
    C.check_knn(orc, d if okind == "jaccard" else d.double() ** 2, j, K)
    if okind == "jaccard":
        assert torch.equal(j, je) and torch.equal(d, de)
        return
    decided = orc.decided(K)
    assert float(decided.double().mean()) >= 0.9
    assert torch.equal(torch.sort(j[decided], dim=1).values, torch.sort(je[decided], dim=1).values)


def _clustered(seed=0, N=600, n=5000, clusters=12, nnz=30):
    """Sparse rows around ``clusters`` sparse centres: a row keeps ~80 % of its centre's columns
    (values centre + noise) and adds a few columns of its own."""
    rng = np.random.default_rng(seed)
    centres = [(np.sort(rng.choice(n, nnz, replace=False)), rng.standard_normal(nnz) * 2.0) for _ in range(clusters)]
    rows = []
    for r in range(N):
        cols, vals = centres[r % clusters]
        keep = rng.random(nnz) < 0.8
        own = np.setdiff1d(rng.choice(n, 6, replace=False), cols)
        c = np.concatenate([cols[keep], own])
        v = np.concatenate([vals[keep] + 0.3 * rng.standard_normal(int(keep.sum())), rng.standard_normal(len(own))])
        o = np.argsort(c)
        rows.append((c[o], v[o].astype(np.float32)))
    return C.csr_from_rows(rows, n)


@pytest.fixture(scope="module")
def clustered():
    A = _clustered()
    orc = C.Oracle(A, A, "sqeuclidean")
    return A, orc


@pytest.mark.parametrize("dev", DEVICES)
def test_rounds_never_lose_ground(dev, clustered):
    """Across round 0 and every later round each row's k-th key never increases — exactly: the same
    pair is always computed the same way and a row's own list is among its candidates — and on the
    rows the oracle decides a true neighbour once listed stays listed, so recall never decreases.
    A second seeded build repeats the first bit for bit."""
    dev = _device(dev)
    A, orc = clustered
    Ad = C.to(A, dev)
    rounds, phases = [], {}
    d, j = knn_graph_csr_approx(Ad, K, "euclidean", seed=4, nnd_iters=3, rounds=rounds, phases=phases)
    assert [r[0] for r in rounds] == ["candidates", "round0", "round1", "round2", "round3"] and rounds[0][1] is None
    rounds = [r[1:] for r in rounds[1:]]
    assert {"rp_projection", "rp_candidates", "csr_nn_descent"} <= set(phases)
    assert torch.equal(j, rounds[-1][1]) and torch.equal(d, torch.sqrt(rounds[-1][0]))
    decided = orc.decided(K)
    assert float(decided.double().mean()) >= 0.9
    true = torch.zeros(orc.D.shape, dtype=torch.bool)
    true.scatter_(1, orc.topk_ids(K), True)
    listed, kth = [], []
    for keys, ids in rounds:
        keys, ids = keys.cpu(), ids.cpu()
        assert bool((ids >= 0).all()) and bool(torch.isfinite(keys).all())
        err = (keys.double() - orc.D.gather(1, ids)).abs()
        assert bool((err <= orc.eps.gather(1, ids)).all())  # every distance is the CSR rows' own
        kth.append(keys[:, -1])
        listed.append(torch.zeros_like(true).scatter_(1, ids, True))
    for r in range(1, len(rounds)):
        assert bool((kth[r] <= kth[r - 1]).all()), "round %d raised a k-th key" % r
        lost = true & listed[r - 1] & ~listed[r]
        assert not bool(lost[decided].any()), "round %d dropped a true neighbour of a decided row" % r
        assert int((true & listed[r])[decided].sum()) >= int((true & listed[r - 1])[decided].sum())
    d2, j2 = knn_graph_csr_approx(Ad, K, "euclidean", seed=4, nnd_iters=3)
    assert torch.equal(j, j2) and torch.equal(d.view(torch.int32), d2.view(torch.int32))


def _scipy_rows(m, n, density, seed):
    rng = np.random.default_rng(seed)
    M = sp.random(m, n, density=density, format="csr", random_state=rng, dtype=np.float32,
                  data_rvs=lambda s: rng.standard_normal(s).astype(np.float32))
    M.sort_indices()
    return M


def _emb(out):
    return np.asarray(out.to_numpy("embedding"), dtype=np.float32)


@pytest.mark.parametrize("dev", DEVICES)
def test_seeded_fit_equals_the_fit_on_its_own_graph(dev):
    dev = _device(dev)
    Ad = to_device(_scipy_rows(400, 3000, 0.01, 7), dev, torch.float32)
    kw = {"proj_dim": 32, "nnd_iters": 1}
    params = {"n_neighbors": K, "random_state": 11, "n_epochs": 20, "init": "random", "metric": "euclidean",
              "build_algo": ALGO, "build_kwds": kw}
    set_deterministic(True)
    try:
        e1 = U.umap_fit(Ad, params)
        dist, idx = build_knn_graph(Ad, K, ALGO, kw, 11, None)
        e2 = U.umap_fit(Ad, dict(params, precomputed_knn=(idx.cpu().numpy(), dist.cpu().numpy())))
    finally:
        set_deterministic(None)
    assert e1.shape == (400, 2) and np.isfinite(e1).all() and float(np.ptp(e1, axis=0).min()) > 1.0
    assert np.array_equal(e1, e2)


def _fit_transform_save_load(tmp_path):
    M = _scipy_rows(300, 2000, 0.01, 3)
    df = DataFrame.from_numpy(M)
    est = UMAP(enable_sparse_data_optim=True, build_algo=ALGO, build_kwds={"nnd_iters": 1}, random_state=2, n_epochs=20,
               n_neighbors=K)
    model = est.fit(df)
    assert model.embedding_.shape == (300, 2) and np.isfinite(model.embedding_).all() and sp.issparse(model.raw_data_)
    e = _emb(model.transform(df))
    assert e.shape == (300, 2) and np.isfinite(e).all()
    path = str(tmp_path / "model")
    model.write().overwrite().save(path)
    loaded = UMAPModel.load(path)
    assert sp.issparse(loaded.raw_data_) and np.array_equal(loaded.embedding_, model.embedding_)
    assert loaded.getOrDefault("build_algo") == ALGO and loaded.getOrDefault("build_kwds") == {"nnd_iters": 1}
    set_deterministic(True)
    try:
        assert np.array_equal(_emb(model.transform(df)), _emb(loaded.transform(df)))
    finally:
        set_deterministic(None)


def test_fit_transform_save_load(tmp_path):
    _fit_transform_save_load(tmp_path)


@pytest.mark.gpu
def test_fit_transform_save_load_on_the_device(tmp_path, gpu_device):
    _fit_transform_save_load(tmp_path)


@pytest.mark.dist
def test_two_worker_fit(monkeypatch):
    monkeypatch.setenv("SRML_FORCE_CPU", "1")
    M = _scipy_rows(300, 500, 0.03, 8)
    model = UMAP(enable_sparse_data_optim=True, build_algo=ALGO, random_state=5, num_workers=2, n_epochs=30,
                 n_neighbors=K).fit(DataFrame.from_numpy(M, num_partitions=2))
    assert model.embedding_.shape == (300, 2) and np.isfinite(model.embedding_).all()
    got = sp.csr_matrix(model.raw_data_)
    assert np.array_equal(got.indptr, M.indptr) and np.array_equal(got.indices, M.indices)  # rows in input order
    assert np.array_equal(got.data, M.data)


def test_refusals():
    A = _small_rows("euclidean")
    X = torch.from_numpy(np.random.default_rng(0).standard_normal((50, 8)).astype(np.float32))
    with pytest.raises(ValueError, match="sparse \\(CSR\\) rows only"):
        build_knn_graph(X, 5, ALGO, None, 0, None)
    for algo in ("ivf", "nn_descent"):
        with pytest.raises(ValueError, match="exact search"):
            build_knn_graph(A, 5, algo, None, 0, None)
    with pytest.raises(ValueError, match="proj_dim"):
        build_knn_graph(A, 5, ALGO, {"proj_dim": 129}, 0, None)
    with pytest.raises(ValueError, match="no sparse kNN graph"):
        build_knn_graph(A, 5, ALGO, None, 0, None, metric="l1")
    d, j, order = build_knn_graph(A, 5, ALGO, None, 0, None, list_order=True)
    assert order is None and d.shape == j.shape == (60, 5)
    da, ja = build_knn_graph(A, 5, "auto", None, 0, None)  # auto stays the exact search
    de, je = knn_graph_csr(ops.csr_prepare(A, "sqeuclidean"), ops.csr_prepare(A, "sqeuclidean"), 5)
    assert torch.equal(ja, je) and torch.equal(da, de)
