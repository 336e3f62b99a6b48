"""IVF-PQ on the CPU path: ``ops.pq_encode`` / ``ops.ivfpq_search`` against fp64 oracles with the
derived rounding bound (``ivfpq_cases.py``), and ``ApproximateNearestNeighbors(algorithm="ivfpq")``
end to end. ``test_ivfpq_gpu.py`` repeats the same checks on the kernels."""
import warnings

import numpy as np
import pytest
import torch

import ivfpq_cases as cases
from spark_rapids_ml_nai_amd import DataFrame, ops
from spark_rapids_ml_nai_amd.knn import ApproximateNearestNeighbors, NearestNeighbors

warnings.filterwarnings("ignore")

METRICS = ["euclidean", "sqeuclidean", "l2", "inner_product"]


@pytest.fixture(autouse=True)
def _cpu(monkeypatch):
    monkeypatch.setenv("SRML_FORCE_CPU", "1")


# ------------------------------------------------------------------------------------------ ops
@pytest.mark.parametrize("ip", [0, 1])
@pytest.mark.parametrize("name", sorted(cases.SCAN_CASES))
def test_scan_matches_fp64_oracle(name, ip):
    cases.run_scan_case(ops, name, ip, "cpu")


@pytest.mark.parametrize("ip", [0, 1])
@pytest.mark.parametrize("kc", [10, 64, 65])
def test_scan_identical_rows_give_distinct_positions(kc, ip):
    index = cases.make_index(8, 2, 16, 70, 1, identical=40)
    Q, probes = cases.make_queries(index, 9, 1)
    keys, pos = cases.scan(ops, index, Q, probes, kc, ip, "cpu")
    cases.check_scan(index, Q, probes, kc, ip, keys, pos)


@pytest.mark.parametrize("ip", [0, 1])
@pytest.mark.parametrize("nq", [0, 1, 257])
def test_scan_query_counts(nq, ip):
    n, M, ksub, N, nlist, nprobe, _, _ = cases.SCAN_CASES["n32"]
    index = cases.make_index(n, M, ksub, N, nlist)
    Q, probes = cases.make_queries(index, nq, nprobe)
    for kc in (40, 65):
        keys, pos = cases.scan(ops, index, Q, probes, kc, ip, "cpu")
        cases.check_scan(index, Q, probes, kc, ip, keys, pos)


@pytest.mark.parametrize("N", cases.ENCODE_ROWS)
@pytest.mark.parametrize("shape", cases.ENCODE_SHAPES, ids=lambda s: "n%d_M%d_k%d" % s)
def test_encode_within_bound_and_repeatable(shape, N):
    cases.run_encode_case(ops, *shape, N, "cpu")


def test_ops_refuse_bad_shapes():
    index = cases.make_index(8, 2, 16, 20, 2)
    Q, probes = cases.make_queries(index, 3, 2)
    with pytest.raises(ValueError):
        ops.ivfpq_search(Q[:, :7], probes, index["list_off"], index["C"][:, :7], index["cb"], index["codes"], 5)
    with pytest.raises(ValueError):
        ops.ivfpq_search(Q, probes, index["list_off"], index["C"], index["cb"], index["codes"], ops.TOPK_KMAX + 1)
    with pytest.raises(ValueError):
        ops.pq_encode(Q, torch.zeros((129, 16, 1)))


# ---------------------------------------------------------------------------------------- model
def _ann(k=10, **kw):
    ap = {"nlist": 16, "nprobe": 4, "M": 8, "n_bits": 6}
    ap.update(kw.pop("algoParams", {}))
    return ApproximateNearestNeighbors(k=k, algorithm="ivfpq", algoParams=ap, inputCol="features", **kw)


@pytest.mark.parametrize("ap", [{"M": 5}, {"M": 129}, {"M": 256}, {"n_bits": 3}, {"n_bits": 9}, {"refine_ratio": 0},
                                {"refine_ratio": 2000}], ids=str)
def test_bad_arguments_raise(ap):
    X, Q = cases.blobs()
    with pytest.raises(ValueError):
        _ann(algoParams=ap).fit(DataFrame.from_numpy(X[:200])).kneighbors(DataFrame.from_numpy(Q[:5]))


def test_default_m_and_ignored_precomputed_tables():
    from spark_rapids_ml_nai_amd.models.knn import default_pq_m

    assert [default_pq_m(n) for n in (1, 3, 16, 35, 128, 1024)] == [1, 1, 4, 7, 32, 128]
    X, Q = cases.blobs()
    ann = ApproximateNearestNeighbors(k=5, algorithm="ivfpq", inputCol="features",
                                      algoParams={"n_lists": 8, "n_probes": 8, "usePrecomputedTables": True})
    _, _, knn_df = ann.fit(DataFrame.from_numpy(X[:300])).kneighbors(DataFrame.from_numpy(Q[:20]))
    _, ind, _ = cases.knn_arrays(knn_df)
    assert ind.shape == (20, 5)


def _exhaustive(metric, workers):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((200, 16)).astype(np.float32)
    Q = rng.standard_normal((40, 16)).astype(np.float32)
    ann = _ann(metric=metric, num_workers=workers, algoParams={"nlist": 4, "nprobe": 4, "M": 4, "refine_ratio": 20})
    _, _, knn_df = ann.fit(DataFrame.from_numpy(X, num_partitions=workers)) \
        .kneighbors(DataFrame.from_numpy(Q, num_partitions=workers))
    return X, Q, cases.knn_arrays(knn_df)


def _check_exhaustive(X, Q, got, metric):
    _, ind, dist = got
    ref_d = cases.direct_distance(X, Q, cases.exact_ids(X, Q, 10, metric), metric)
    np.testing.assert_allclose(dist, ref_d, rtol=1e-5, atol=1e-6)
    if metric == "inner_product":  # NearestNeighbors is euclidean only: the exact search of this metric
        ref = ApproximateNearestNeighbors(k=10, algorithm="brute", metric=metric, inputCol="features")
    else:  # the same neighbour order for the three L2 forms
        ref = NearestNeighbors(k=10, inputCol="features")
    _, _, ref_df = ref.fit(DataFrame.from_numpy(X)).kneighbors(DataFrame.from_numpy(Q))
    _, ref_i, _ = cases.knn_arrays(ref_df)
    every = np.tile(np.arange(X.shape[0]), (Q.shape[0], 1))
    full = cases.direct_distance(X, Q, every, "inner_product" if metric == "inner_product" else "sqeuclidean")
    full = np.sort(-full if metric == "inner_product" else full, axis=1)[:, :11]
    gap = np.diff(full, axis=1) > 1e-6 * np.abs(full[:, 1:])  # neighbour j and j + 1 not tied
    clear = np.concatenate([np.ones((Q.shape[0], 1), bool), gap[:, :-1]], 1) & gap
    assert clear.mean() > 0.9
    assert np.array_equal(ind[clear], ref_i[clear])


@pytest.mark.parametrize("metric", METRICS)
def test_exhaustive_search_is_exact(metric):
    """nprobe = nlist and kc = 200 >= N: the candidates path sees every item."""
    X, Q, got = _exhaustive(metric, 1)
    _check_exhaustive(X, Q, got, metric)


@pytest.mark.dist
@pytest.mark.parametrize("metric", METRICS)
def test_exhaustive_search_two_workers(metric):
    X, Q, one = _exhaustive(metric, 1)
    _, _, two = _exhaustive(metric, 2)
    _check_exhaustive(X, Q, two, metric)
    o1, o2 = np.argsort(one[0]), np.argsort(two[0])
    assert np.array_equal(one[0][o1], two[0][o2])
    assert np.array_equal(one[1][o1], two[1][o2])
    np.testing.assert_allclose(one[2][o1], two[2][o2], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("refine_ratio", [1, 4])
@pytest.mark.parametrize("metric", METRICS)
def test_distances_are_exact_for_returned_ids(metric, refine_ratio):
    X, Q = cases.blobs()
    _, _, knn_df = _ann(metric=metric, algoParams={"refine_ratio": refine_ratio}).fit(DataFrame.from_numpy(X)) \
        .kneighbors(DataFrame.from_numpy(Q[:60]))
    _, ind, dist = cases.knn_arrays(knn_df)
    np.testing.assert_allclose(dist, cases.direct_distance(X, Q[:60], ind, metric), rtol=1e-5, atol=1e-5)


def test_refine_raises_recall():
    X, Q = cases.blobs()
    exact = cases.exact_ids(X, Q, 10, "euclidean")
    rec = {}
    for rr in (1, 4):
        _, _, knn_df = _ann(algoParams={"refine_ratio": rr}).fit(DataFrame.from_numpy(X)) \
            .kneighbors(DataFrame.from_numpy(Q))
        rec[rr] = cases.recall(cases.knn_arrays(knn_df)[1], exact)
    print("ivfpq recall@10 (cpu path): refine_ratio 1 -> %.3f, 4 -> %.3f" % (rec[1], rec[4]))
    assert rec[4] > rec[1], rec


def test_index_cache_is_keyed_by_algorithm_and_parameters(monkeypatch):
    from spark_rapids_ml_nai_amd.models import knn as mk

    built = []
    real_pq, real_flat = mk.build_ivfpq, mk.build_ivf
    monkeypatch.setattr(mk, "build_ivfpq", lambda *a, **k: built.append("pq") or real_pq(*a, **k))
    X, Q = cases.blobs()
    model = _ann().fit(DataFrame.from_numpy(X[:500]))
    q = DataFrame.from_numpy(Q[:10])
    model.kneighbors(q)
    model.kneighbors(q)
    assert built == ["pq"]  # the second call reused the index
    model.setAlgoParams({"nlist": 16, "nprobe": 4, "M": 4, "n_bits": 6})
    model.kneighbors(q)
    assert built == ["pq", "pq"]  # other parameters, other index
    monkeypatch.setattr(mk, "build_ivf", lambda *a, **k: built.append("flat") or real_flat(*a, **k))
    monkeypatch.setattr(ops, "ivfpq_search", lambda *a, **k: pytest.fail("the PQ index was used for ivfflat"))
    model.setAlgorithm("ivfflat")
    _, _, knn_df = model.kneighbors(q)
    assert built[2:] == ["flat"]
    _, ind, dist = cases.knn_arrays(knn_df)
    np.testing.assert_allclose(dist, cases.direct_distance(X[:500], Q[:10], ind, "euclidean"), rtol=1e-5, atol=1e-5)


def test_spark_task_carries_pq_parameters(monkeypatch):
    """The barrier-job task hands (M, n_bits, refine_ratio) to the worker behind the empty cache slot."""
    from spark_rapids_ml_nai_amd import knn as pk
    from spark_rapids_ml_nai_amd.models import knn as mk
    from spark_rapids_ml_nai_amd.parallel.context import WorkerContext

    seen = []
    real = mk.build_ivfpq
    monkeypatch.setattr(mk, "build_ivfpq", lambda X, ids, nl, M, nb, seed: seen.append((nl, M, nb, seed))
                        or real(X, ids, nl, M, nb, seed))
    X, Q = cases.blobs()
    both = np.concatenate([X[:400], Q[:20]])
    tag = np.concatenate([np.zeros(400), np.ones(20)]).astype(np.int32)
    df = DataFrame.from_numpy(both, extra={"id": np.arange(420), pk._TAG: tag})
    model = _ann(k=5, algoParams={"refine_ratio": 3, "seed": 7}).fit(DataFrame.from_numpy(X[:400]))
    assert model._ivf_args() == ("ivfpq", 16, 4, 7, (8, 6, 3))
    extra = ("features", None, "id", "query_id", 5, "euclidean", model._ivf_args())
    batch = next(pk._spark_knn_task(WorkerContext.single(), df._concat(), extra))
    assert seen == [(16, 8, 6, 7)]
    ind = np.stack([np.asarray(v) for v in batch.column("indices").to_pylist()])
    dist = np.stack([np.asarray(v) for v in batch.column("distances").to_pylist()])
    assert ind.shape == (20, 5) and ind.max() < 400
    np.testing.assert_allclose(dist, cases.direct_distance(X[:400], Q[:20], ind, "euclidean"), rtol=1e-5, atol=1e-5)
    # the other algorithms' arguments are what they were
    model.setAlgorithm("ivfflat")
    assert model._ivf_args() == ("ivfflat", 16, 4, 7)
    assert len(model._payload_extra()) == 5


def test_approx_similarity_join():
    X, Q = cases.blobs()
    model = _ann(k=4).fit(DataFrame.from_numpy(X[:400]))
    join = model.approxSimilarityJoin(DataFrame.from_numpy(Q[:25]), distCol="dist")
    assert join.columns == ["item_df", "query_df", "dist"]
    assert join.count() == 100
    r = join.collect()[0]
    d = np.linalg.norm(np.asarray(r["query_df"]["features"]) - np.asarray(r["item_df"]["features"]))
    assert np.isclose(d, r["dist"], rtol=1e-5)
