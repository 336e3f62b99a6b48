"""CAGRA on the device: ``srml_cagra_prune_i32``, ``srml_cagra_merge_i32``, ``srml_cagra_seeds_i32`` and
``srml_cagra_search_f32`` against the numpy oracles of ``cagra_cases.py`` (bit for bit on lattice
data), and ``ApproximateNearestNeighbors(algorithm="cagra")`` end to end on the GPU. The CPU path
gets the same assertions in ``test_cagra.py``."""
import warnings

import numpy as np
import pytest

import cagra_cases as cases
import ivfpq_cases
from spark_rapids_ml_nai_amd import DataFrame, ops
from spark_rapids_ml_nai_amd.knn import ApproximateNearestNeighbors

warnings.filterwarnings("ignore")
pytestmark = pytest.mark.gpu

METRICS = ["euclidean", "sqeuclidean", "l2"]
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------ ops
@pytest.mark.parametrize("name", sorted(cases.GRAPH_CASES))
def test_prune_and_merge_match_oracle(name):
    N, d, gd = cases.GRAPH_CASES[name]
    cases.run_graph_case(ops, cases.knn_rows(N, d), gd, DEV)


def test_prune_and_merge_identical_rows():
    cases.run_graph_case(ops, cases.knn_rows(200, 33, identical=40), 16, DEV)


@pytest.mark.parametrize("N", [1, 2])
def test_prune_and_merge_tiny_graphs(N):
    P, F = cases.run_graph_case(ops, cases.knn_rows(N, 4), 2, DEV)
    assert (P >= 0).sum() == (N - 1) * N and (F >= 0).sum() == (N - 1) * N


def test_seeds_match_oracle_and_follow_the_row():
    cases.run_seed_case(ops, DEV)
    cases.run_seed_case(ops, DEV, n=4, nq=5, N=3, S=40)  # S > N


@pytest.mark.parametrize("name", sorted(cases.SEARCH_CASES))
def test_search_matches_oracle_on_lattice(name):
    """gd 4 / 32 / 64, (itopk, width) (32, 1) (64, 1) (64, 4) (512, 1), k 1 / 10 / itopk, max_iter
    1 / 5 / auto (lowered to the LDS at itopk 512), nq 0 / 1 / 257, up to 1024 seeds."""
    cases.run_search_case(ops, name, DEV)


@pytest.mark.parametrize("n,pad,shift", [(35, 1, 1), (128, 4, 1), (128, 4, 4), (35, 5, 0)])
def test_search_strided_and_misaligned_rows(n, pad, shift):
    """(128, 4, 4) keeps the 16-byte loads at a row stride above n; the others take the scalar loads."""
    cases.run_layout_case(ops, DEV, n, pad, shift)


def test_search_edge_cases():
    cases.run_edge_cases(ops, DEV)


def test_exhaustive_regime_is_exact():
    cases.run_exhaustive_case(ops, DEV)


@pytest.mark.parametrize("name", sorted(cases.LIMITS))
def test_limits_are_refused(name, monkeypatch):
    cases.run_limit_case(ops, name, DEV, monkeypatch)


def test_lds_budget_matches_the_kernel_library():
    """``ops.cagra_lds_bytes`` mirrors the host function the launch is decided on."""
    from spark_rapids_ml_nai_amd.ops import native

    for args in [(4, 32, 1, 4, 32, 1), (35, 64, 1, 32, 64, 80), (128, 64, 4, 64, 64, 32), (260, 512, 1, 32, 1024, 400),
                 (128, 512, 8, 64, 512, 10), (1, 32, 1, 1, 1, 0)]:
        assert int(native.lib().srml_cagra_lds_bytes(*args)) == ops.cagra_lds_bytes(*args), args


# ---------------------------------------------------------------------------------------- model
AP = {"intermediate_graph_degree": 32, "graph_degree": 16, "itopk_size": 64, "build_algo": "brute_force"}


def _ann(k=10, **kw):
    ap = dict(AP)
    ap.update(kw.pop("algoParams", {}))
    return ApproximateNearestNeighbors(k=k, algorithm="cagra", algoParams=ap, inputCol="features", **kw)


@pytest.mark.parametrize("ap", [{"intermediate_graph_degree": 129}, {"graph_degree": 33}, {"build_algo": "hnsw"},
                                {"itopk_size": 513}, {"search_width": 40}, {"compression": "vpq"},
                                {"metric": "inner_product"}], ids=str)
def test_bad_arguments_raise(ap):
    X, Q = ivfpq_cases.blobs()
    ap = dict(ap)
    kw = {"metric": ap.pop("metric")} if "metric" in ap else {}
    with pytest.raises(ValueError):
        _ann(algoParams=ap, **kw).fit(DataFrame.from_numpy(X[:200])).kneighbors(DataFrame.from_numpy(Q[:5]))


@pytest.mark.parametrize("build_algo", ["brute_force", "ivf_pq", "nn_descent"])
@pytest.mark.parametrize("metric", METRICS)
def test_distances_are_exact_for_returned_ids(metric, build_algo):
    X, Q = ivfpq_cases.blobs()
    _, _, knn_df = _ann(metric=metric, algoParams={"build_algo": build_algo}).fit(DataFrame.from_numpy(X)) \
        .kneighbors(DataFrame.from_numpy(Q[:60]))
    _, ind, dist = ivfpq_cases.knn_arrays(knn_df)
    assert all(len(set(r.tolist())) == r.size for r in ind)
    np.testing.assert_allclose(dist, ivfpq_cases.direct_distance(X, Q[:60], ind, metric), rtol=1e-5, atol=1e-5)


def test_k_above_item_count_pads():
    X, Q = ivfpq_cases.blobs()
    _, _, knn_df = _ann(k=12).fit(DataFrame.from_numpy(X[:7])).kneighbors(DataFrame.from_numpy(Q[:4]))
    _, ind, _ = ivfpq_cases.knn_arrays(knn_df)
    for r in ind:
        assert sorted(r.tolist()) == list(range(7))


def _recalls(monkeypatch, cpu):
    if cpu:
        monkeypatch.setenv("SRML_FORCE_CPU", "1")
    else:
        monkeypatch.delenv("SRML_FORCE_CPU", raising=False)
    X, Q = ivfpq_cases.blobs()
    exact = ivfpq_cases.exact_ids(X, Q, 10, "euclidean")
    out = {}
    model = _ann().fit(DataFrame.from_numpy(X))
    for itopk in (32, 64, 128):
        model.setAlgoParams(dict(AP, itopk_size=itopk))
        _, _, knn_df = model.kneighbors(DataFrame.from_numpy(Q))
        out[itopk] = ivfpq_cases.recall(ivfpq_cases.knn_arrays(knn_df)[1], exact)
    return out


def test_recall_matches_cpu_path(monkeypatch):
    """graph_degree 16 (from 32), itopk_size 64 on the 2000 x 32 blobs: the CPU path reaches 0.953
    (``test_cagra.py::test_recall``). Near-ties in the build may order differently on the device, so
    its recall may trail the CPU path's by 0.02 at most."""
    dev = _recalls(monkeypatch, cpu=False)
    cpu = _recalls(monkeypatch, cpu=True)
    print("cagra recall@10: device itopk 32 %.3f 64 %.3f 128 %.3f | cpu path 32 %.3f 64 %.3f 128 %.3f"
          % (dev[32], dev[64], dev[128], cpu[32], cpu[64], cpu[128]))
    assert cpu[64] >= 0.95, cpu
    assert dev[128] >= dev[32], dev
    for itopk in (32, 64, 128):
        assert dev[itopk] >= cpu[itopk] - 0.02, (itopk, dev, cpu)


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
    assert built == ["cagra"]
    assert next(iter(model._index_cache.values())).graph.is_cuda
    model.setAlgoParams(dict(AP, itopk_size=128, search_width=2, max_iterations=20))
    model.kneighbors(q)
    assert built == ["cagra"]  # search-only parameters: no rebuild
    for name in ("cagra_search", "cagra_prune", "cagra_merge"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the graph was used for ivfflat"))
    model.setAlgorithm("ivfflat")
    model.setAlgoParams({"nlist": 8, "nprobe": 8})
    _, _, knn_df = model.kneighbors(q)
    assert built == ["cagra"]
    _, ind, dist = ivfpq_cases.knn_arrays(knn_df)
    np.testing.assert_allclose(dist, ivfpq_cases.direct_distance(X[:500], Q[:10], ind, "euclidean"), rtol=1e-5,
                               atol=1e-5)


def test_approx_similarity_join():
    X, Q = ivfpq_cases.blobs()
    model = _ann(k=4).fit(DataFrame.from_numpy(X[:400]))
    join = model.approxSimilarityJoin(DataFrame.from_numpy(Q[:25]), distCol="dist")
    assert join.count() == 100
    r = join.collect()[0]
    d = np.linalg.norm(np.asarray(r["query_df"]["features"]) - np.asarray(r["item_df"]["features"]))
    assert np.isclose(d, r["dist"], rtol=1e-5)
