"""CAGRA on the CPU path: ``ops.cagra_prune`` / ``cagra_merge`` / ``cagra_seeds`` / ``cagra_search``
against the numpy oracles of ``cagra_cases.py`` (bit for bit on lattice data), and
``ApproximateNearestNeighbors(algorithm="cagra")`` end to end. ``test_cagra_gpu.py`` repeats the
same checks on the kernels."""
import warnings

import numpy as np
import pytest

import cagra_cases as cases
import ivfpq_cases
from spark_rapids_ml_nai_amd import DataFrame, ops
from spark_rapids_ml_nai_amd.knn import ApproximateNearestNeighbors

warnings.filterwarnings("ignore")

METRICS = ["euclidean", "sqeuclidean", "l2"]
DEV = "cpu"


@pytest.fixture(autouse=True)
def _cpu(monkeypatch):
    monkeypatch.setenv("SRML_FORCE_CPU", "1")


# ------------------------------------------------------------------------------------------ ops
@pytest.mark.parametrize("name", sorted(cases.GRAPH_CASES))
def test_prune_and_merge_match_oracle(name):
    N, d, gd = cases.GRAPH_CASES[name]
    G = cases.knn_rows(N, d)
    if name == "tail":
        assert ((G >= 0).sum(1) == 19).all()
    cases.run_graph_case(ops, G, gd, DEV)


def test_prune_and_merge_identical_rows():
    cases.run_graph_case(ops, cases.knn_rows(200, 33, identical=40), 16, DEV)


@pytest.mark.parametrize("N", [1, 2])
def test_prune_and_merge_tiny_graphs(N):
    """N = 1: the only row has no edge at all."""
    P, F = cases.run_graph_case(ops, cases.knn_rows(N, 4), 2, DEV)
    assert (P >= 0).sum() == (N - 1) * N and (F >= 0).sum() == (N - 1) * N


def test_seeds_match_oracle_and_follow_the_row():
    cases.run_seed_case(ops, DEV)
    cases.run_seed_case(ops, DEV, n=4, nq=5, N=3, S=40)  # S > N


@pytest.mark.parametrize("name", sorted(cases.SEARCH_CASES))
def test_search_matches_oracle_on_lattice(name):
    cases.run_search_case(ops, name, DEV)


@pytest.mark.parametrize("n,pad,shift", [(35, 1, 1), (128, 4, 1), (128, 4, 4), (35, 5, 0)])
def test_search_strided_and_misaligned_rows(n, pad, shift):
    cases.run_layout_case(ops, DEV, n, pad, shift)


def test_search_edge_cases():
    cases.run_edge_cases(ops, DEV)


def test_exhaustive_regime_is_exact():
    cases.run_exhaustive_case(ops, DEV)


@pytest.mark.parametrize("name", sorted(cases.LIMITS))
def test_limits_are_refused(name, monkeypatch):
    cases.run_limit_case(ops, name, DEV, monkeypatch)


def test_auto_iterations_fit_the_lds():
    assert ops.cagra_auto_iters(128, 64, 1, 64, 64) == 64 + 16
    assert ops.cagra_auto_iters(128, 64, 4, 64, 64) == 16 + 16
    it = ops.cagra_auto_iters(128, 512, 1, 64, 512)  # 528 iterations would need a 512 KiB table
    assert 1 <= it < 528
    assert ops.cagra_lds_bytes(128, 512, 1, 64, 512, it) <= ops.CAGRA_LDS_TOTAL
    assert ops.cagra_lds_bytes(128, 512, 1, 64, 512, it + 1) > ops.CAGRA_LDS_TOTAL


# ---------------------------------------------------------------------------------------- model
AP = {"intermediate_graph_degree": 32, "graph_degree": 16, "itopk_size": 64, "build_algo": "brute_force"}


def _ann(k=10, **kw):
    ap = dict(AP)
    ap.update(kw.pop("algoParams", {}))
    return ApproximateNearestNeighbors(k=k, algorithm="cagra", algoParams=ap, inputCol="features", **kw)


BAD = [{"intermediate_graph_degree": 129}, {"intermediate_graph_degree": 0}, {"graph_degree": 33}, {"graph_degree": 0},
       {"build_algo": "hnsw"}, {"itopk_size": 513}, {"itopk_size": 0}, {"itopk_size": 8}, {"search_width": 0},
       {"search_width": 40}, {"max_iterations": -1}, {"min_iterations": -1}, {"num_random_samplings": 0},
       {"compression": "vpq"}, {"graph_degree": 2.5}, {"metric": "inner_product"}]


@pytest.mark.parametrize("ap", BAD, ids=str)
def test_bad_arguments_raise(ap):
    """itopk_size 8 rounds up to 32, below k = 40."""
    X, Q = ivfpq_cases.blobs()
    ap = dict(ap)
    kw = {"metric": ap.pop("metric")} if "metric" in ap else {}
    with pytest.raises(ValueError):
        _ann(k=40 if ap.get("itopk_size") == 8 else 10, algoParams=ap, **kw).fit(DataFrame.from_numpy(X[:200])) \
            .kneighbors(DataFrame.from_numpy(Q[:5]))


@pytest.mark.parametrize("metric", METRICS)
def test_distances_are_exact_for_returned_ids(metric):
    X, Q = ivfpq_cases.blobs()
    _, _, knn_df = _ann(metric=metric).fit(DataFrame.from_numpy(X)).kneighbors(DataFrame.from_numpy(Q[:60]))
    _, ind, dist = ivfpq_cases.knn_arrays(knn_df)
    assert all(len(set(r.tolist())) == r.size for r in ind)
    np.testing.assert_allclose(dist, ivfpq_cases.direct_distance(X, Q[:60], ind, metric), rtol=1e-5, atol=1e-5)


def test_k_above_item_count_pads():
    X, Q = ivfpq_cases.blobs()
    _, _, knn_df = _ann(k=12).fit(DataFrame.from_numpy(X[:7])).kneighbors(DataFrame.from_numpy(Q[:4]))
    _, ind, dist = ivfpq_cases.knn_arrays(knn_df)
    for r in ind:  # the -1 padding is dropped from the rows of the frame
        assert sorted(r.tolist()) == list(range(7))


def _recalls():
    X, Q = ivfpq_cases.blobs()
    exact = ivfpq_cases.exact_ids(X, Q, 10, "euclidean")
    out = {}
    model = _ann().fit(DataFrame.from_numpy(X))
    for itopk in (32, 64, 128):
        model.setAlgoParams(dict(AP, itopk_size=itopk))
        _, _, knn_df = model.kneighbors(DataFrame.from_numpy(Q))
        out[itopk] = ivfpq_cases.recall(ivfpq_cases.knn_arrays(knn_df)[1], exact)
    return out


def test_recall():
    """graph_degree 16 (from 32) and itopk_size 64 on the 2000 x 32 blobs: recall@10 is 0.953 on the CPU
    path (0.810 at itopk_size 32, 0.993 at 128). The 20 blobs are separate components of the kNN graph, so
    a query is answered when one of its itopk_size seeds falls into its blob: 1 - 0.95^64 = 0.96. The
    seeds are integer hashes, so the figure does not move with the rounding of a distance."""
    rec = _recalls()
    print("cagra recall@10 (cpu path): itopk 32 -> %.3f, 64 -> %.3f, 128 -> %.3f" % (rec[32], rec[64], rec[128]))
    assert rec[64] >= 0.95, rec
    assert rec[128] >= rec[32], rec


def test_index_cache_is_keyed_by_algorithm_and_build_parameters(monkeypatch):
    from spark_rapids_ml_nai_amd.models import knn as mk

    built = []
    real = mk.build_cagra
    monkeypatch.setattr(mk, "build_cagra", lambda *a, **k: built.append("cagra") or real(*a, **k))
    X, Q = ivfpq_cases.blobs()
    model = _ann().fit(DataFrame.from_numpy(X[:500]))
    q = DataFrame.from_numpy(Q[:10])
    model.kneighbors(q)
    model.kneighbors(q)
    assert built == ["cagra"]  # the second call reused the graph
    model.setAlgoParams(dict(AP, itopk_size=128, search_width=2, max_iterations=20))
    model.kneighbors(q)
    assert built == ["cagra"]  # search-only parameters: no rebuild
    model.setAlgoParams(dict(AP, graph_degree=8))
    model.kneighbors(q)
    assert built == ["cagra", "cagra"]  # another graph degree, another index
    for name in ("cagra_search", "cagra_prune", "cagra_merge"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the graph was used for ivfflat"))
    model.setAlgorithm("ivfflat")
    model.setAlgoParams({"nlist": 8, "nprobe": 8})
    _, _, knn_df = model.kneighbors(q)
    assert built == ["cagra", "cagra"]
    assert sorted(k[0] if isinstance(k, tuple) else k for k in model._index_cache) == ["cagra", "cagra", "index"]
    _, ind, dist = ivfpq_cases.knn_arrays(knn_df)
    np.testing.assert_allclose(dist, ivfpq_cases.direct_distance(X[:500], Q[:10], ind, "euclidean"), rtol=1e-5,
                               atol=1e-5)


def test_spark_task_carries_cagra_parameters(monkeypatch):
    """The barrier-job task hands the graph and search parameters to the worker behind the empty cache slot."""
    from spark_rapids_ml_nai_amd import knn as pk
    from spark_rapids_ml_nai_amd.models import knn as mk
    from spark_rapids_ml_nai_amd.parallel.context import WorkerContext

    seen = []
    real_b, real_s = mk.build_cagra, mk.cagra_knn
    monkeypatch.setattr(mk, "build_cagra", lambda X, ids, igd, gd, algo, seed: seen.append((igd, gd, algo, seed))
                        or real_b(X, ids, igd, gd, algo, seed))
    monkeypatch.setattr(mk, "cagra_knn", lambda index, Q, k, params, ctx, metric: seen.append(params)
                        or real_s(index, Q, k, params, ctx, metric))
    X, Q = ivfpq_cases.blobs()
    both = np.concatenate([X[:400], Q[:20]])
    tag = np.concatenate([np.zeros(400), np.ones(20)]).astype(np.int32)
    df = DataFrame.from_numpy(both, extra={"id": np.arange(420), pk._TAG: tag})
    model = _ann(k=5, algoParams={"itopk_size": 40, "search_width": 2, "seed": 7}).fit(DataFrame.from_numpy(X[:400]))
    assert model._ivf_args() == ("cagra", None, None, 7, (32, 16, "brute_force_knn", 64, 2, 0, 0, 1))
    extra = ("features", None, "id", "query_id", 5, "euclidean", model._ivf_args())
    batch = next(pk._spark_knn_task(WorkerContext.single(), df._concat(), extra))
    assert seen == [(32, 16, "brute_force_knn", 7), (64, 2, 0, 0, 1, 7)]
    ind = np.stack([np.asarray(v) for v in batch.column("indices").to_pylist()])
    dist = np.stack([np.asarray(v) for v in batch.column("distances").to_pylist()])
    assert ind.shape == (20, 5) and ind.max() < 400
    np.testing.assert_allclose(dist, ivfpq_cases.direct_distance(X[:400], Q[:20], ind, "euclidean"), rtol=1e-5,
                               atol=1e-5)
    # the other algorithms' arguments are what they were
    model.setAlgorithm("ivfflat")
    assert model._ivf_args() == ("ivfflat", None, None, 7)
    assert len(model._payload_extra()) == 5


def test_approx_similarity_join():
    X, Q = ivfpq_cases.blobs()
    model = _ann(k=4).fit(DataFrame.from_numpy(X[:400]))
    join = model.approxSimilarityJoin(DataFrame.from_numpy(Q[:25]), distCol="dist")
    assert join.columns == ["item_df", "query_df", "dist"]
    assert join.count() == 100
    r = join.collect()[0]
    d = np.linalg.norm(np.asarray(r["query_df"]["features"]) - np.asarray(r["item_df"]["features"]))
    assert np.isclose(d, r["dist"], rtol=1e-5)


def _exhaustive(workers):
    """itopk_size 256 >= N and max_iterations = N: every rank's search expands all it can reach."""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((200, 16)).astype(np.float32)
    Q = rng.standard_normal((40, 16)).astype(np.float32)
    ann = _ann(num_workers=workers, algoParams={"itopk_size": 256, "max_iterations": 200})
    _, _, knn_df = ann.fit(DataFrame.from_numpy(X, num_partitions=workers)) \
        .kneighbors(DataFrame.from_numpy(Q, num_partitions=workers))
    return X, Q, ivfpq_cases.knn_arrays(knn_df)


@pytest.mark.dist
def test_exhaustive_search_two_workers():
    X, Q, one = _exhaustive(1)
    _, _, two = _exhaustive(2)
    o1, o2 = np.argsort(one[0]), np.argsort(two[0])
    assert np.array_equal(one[0][o1], two[0][o2])
    ref_d = ivfpq_cases.direct_distance(X, Q, ivfpq_cases.exact_ids(X, Q, 10, "euclidean"), "euclidean")
    np.testing.assert_allclose(one[2][o1], ref_d, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(two[2][o2], ref_d, rtol=1e-5, atol=1e-6)
    every = ivfpq_cases.direct_distance(X, Q, np.tile(np.arange(200), (40, 1)), "sqeuclidean")
    full = np.sort(every, axis=1)[:, :11]
    gap = np.diff(full, axis=1) > 1e-6 * np.abs(full[:, 1:])
    clear = np.concatenate([np.ones((40, 1), bool), gap[:, :-1]], 1) & gap
    assert clear.mean() > 0.9
    assert np.array_equal(one[1][o1][clear], two[1][o2][clear])
