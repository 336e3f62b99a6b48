"""IVF-PQ on the device: ``srml_pq_encode_f32``, ``srml_ivfpq_search_f32`` (kc <= 64) and
``srml_ivfpq_candidates_f32`` + radix select (kc > 64) against the fp64 oracles and the derived
rounding bound of ``ivfpq_cases.py``, and ``ApproximateNearestNeighbors(algorithm="ivfpq")`` end
to end on the GPU. The CPU path gets the same assertions in ``test_ivfpq.py``."""
import warnings

import numpy as np
import pytest
import torch

import ivfpq_cases as cases
from spark_rapids_ml_nai_amd import DataFrame, ops
from spark_rapids_ml_nai_amd.knn import ApproximateNearestNeighbors, NearestNeighbors

warnings.filterwarnings("ignore")
pytestmark = pytest.mark.gpu

METRICS = ["euclidean", "sqeuclidean", "l2", "inner_product"]
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------ ops
@pytest.mark.parametrize("ip", [0, 1])
@pytest.mark.parametrize("name", sorted(cases.SCAN_CASES))
def test_scan_matches_fp64_oracle(name, ip):
    """n35 runs kc = 64 (fused kernel) and 65 (candidates + select) under the same rule;
    table128k is the 128 KiB lookup table."""
    cases.run_scan_case(ops, name, ip, DEV)


@pytest.mark.parametrize("ip", [0, 1])
@pytest.mark.parametrize("kc", [10, 64, 65])
def test_scan_identical_rows_give_distinct_positions(kc, ip):
    index = cases.make_index(8, 2, 16, 70, 1, identical=40)
    Q, probes = cases.make_queries(index, 9, 1)
    keys, pos = cases.scan(ops, index, Q, probes, kc, ip, DEV)
    cases.check_scan(index, Q, probes, kc, ip, keys, pos)


@pytest.mark.parametrize("ip", [0, 1])
@pytest.mark.parametrize("nq", [0, 1, 257])
def test_scan_query_counts(nq, ip):
    n, M, ksub, N, nlist, nprobe, _, _ = cases.SCAN_CASES["n32"]
    index = cases.make_index(n, M, ksub, N, nlist)
    Q, probes = cases.make_queries(index, nq, nprobe)
    for kc in (40, 65):
        keys, pos = cases.scan(ops, index, Q, probes, kc, ip, DEV)
        cases.check_scan(index, Q, probes, kc, ip, keys, pos)


@pytest.mark.parametrize("N", cases.ENCODE_ROWS)
@pytest.mark.parametrize("shape", cases.ENCODE_SHAPES, ids=lambda s: "n%d_M%d_k%d" % s)
def test_encode_within_bound_and_repeatable(shape, N):
    cases.run_encode_case(ops, *shape, N, DEV)


def test_table_that_does_not_fit_is_refused():
    """M * ksub * 4 + n * 4 bytes of LDS: 128 x 256 with 8320 features is past the 160 KiB."""
    n, M, ksub = 8320, 128, 256
    d = torch.device(DEV)
    Q = torch.zeros((2, n), device=d)
    probes = torch.zeros((2, 1), dtype=torch.int32, device=d)
    off = torch.tensor([0, 3], device=d)
    C = torch.zeros((1, n), device=d)
    cb = torch.zeros((M, ksub, n // M), device=d)
    codes = torch.zeros((3, M), dtype=torch.uint8, device=d)
    for kc in (10, 65):
        with pytest.raises(ValueError):
            ops.ivfpq_search(Q, probes, off, C, cb, codes, kc)


# ---------------------------------------------------------------------------------------- model
def _ann(k=10, **kw):
    ap = {"nlist": 16, "nprobe": 4, "M": 8, "n_bits": 6}
    ap.update(kw.pop("algoParams", {}))
    return ApproximateNearestNeighbors(k=k, algorithm="ivfpq", algoParams=ap, inputCol="features", **kw)


@pytest.mark.parametrize("ap", [{"M": 5}, {"M": 129}, {"n_bits": 3}, {"n_bits": 9}, {"refine_ratio": 0},
                                {"refine_ratio": 2000}], ids=str)
def test_bad_arguments_raise(ap):
    X, Q = cases.blobs()
    with pytest.raises(ValueError):
        _ann(algoParams=ap).fit(DataFrame.from_numpy(X[:200])).kneighbors(DataFrame.from_numpy(Q[:5]))


@pytest.mark.parametrize("metric", METRICS)
def test_exhaustive_search_is_exact(metric):
    """nprobe = nlist and kc = 200 >= N: the candidates path sees every item."""
    rng = np.random.default_rng(3)
    X = rng.standard_normal((200, 16)).astype(np.float32)
    Q = rng.standard_normal((40, 16)).astype(np.float32)
    ann = _ann(metric=metric, algoParams={"nlist": 4, "nprobe": 4, "M": 4, "refine_ratio": 20})
    _, _, knn_df = ann.fit(DataFrame.from_numpy(X)).kneighbors(DataFrame.from_numpy(Q))
    _, ind, dist = cases.knn_arrays(knn_df)
    ref_d = cases.direct_distance(X, Q, cases.exact_ids(X, Q, 10, metric), metric)
    np.testing.assert_allclose(dist, ref_d, rtol=1e-5, atol=1e-6)
    if metric == "inner_product":  # NearestNeighbors is euclidean only: the exact search of this metric
        ref = ApproximateNearestNeighbors(k=10, algorithm="brute", metric=metric, inputCol="features")
    else:
        ref = NearestNeighbors(k=10, inputCol="features")
    _, _, ref_df = ref.fit(DataFrame.from_numpy(X)).kneighbors(DataFrame.from_numpy(Q))
    _, ref_i, _ = cases.knn_arrays(ref_df)
    every = np.tile(np.arange(200), (40, 1))
    full = cases.direct_distance(X, Q, every, "inner_product" if metric == "inner_product" else "sqeuclidean")
    full = np.sort(-full if metric == "inner_product" else full, axis=1)[:, :11]
    gap = np.diff(full, axis=1) > 1e-6 * np.abs(full[:, 1:])
    clear = np.concatenate([np.ones((40, 1), bool), gap[:, :-1]], 1) & gap
    assert clear.mean() > 0.9
    assert np.array_equal(ind[clear], ref_i[clear])


@pytest.mark.parametrize("refine_ratio", [1, 4])
@pytest.mark.parametrize("metric", METRICS)
def test_distances_are_exact_for_returned_ids(metric, refine_ratio):
    X, Q = cases.blobs()
    _, _, knn_df = _ann(metric=metric, algoParams={"refine_ratio": refine_ratio}).fit(DataFrame.from_numpy(X)) \
        .kneighbors(DataFrame.from_numpy(Q[:60]))
    _, ind, dist = cases.knn_arrays(knn_df)
    np.testing.assert_allclose(dist, cases.direct_distance(X, Q[:60], ind, metric), rtol=1e-5, atol=1e-5)


def _recalls(monkeypatch, cpu):
    if cpu:
        monkeypatch.setenv("SRML_FORCE_CPU", "1")
    else:
        monkeypatch.delenv("SRML_FORCE_CPU", raising=False)
    X, Q = cases.blobs()
    exact = cases.exact_ids(X, Q, 10, "euclidean")
    out = {}
    for rr in (1, 4):
        _, _, knn_df = _ann(algoParams={"refine_ratio": rr}).fit(DataFrame.from_numpy(X)) \
            .kneighbors(DataFrame.from_numpy(Q))
        out[rr] = cases.recall(cases.knn_arrays(knn_df)[1], exact)
    return out


def test_refine_raises_recall_and_matches_cpu_path(monkeypatch):
    """The device trainer may land in another Lloyd optimum than the CPU path's (both start from the
    same seeded rows; the sums differ in their last bits): its recall may trail the CPU path's by 0.02
    at most. Measured on an MI355X: 0.519 / 0.915 at refine_ratio 1 / 4 on both paths, a gap of 0."""
    dev = _recalls(monkeypatch, cpu=False)
    cpu = _recalls(monkeypatch, cpu=True)
    print("ivfpq recall@10: device rr1 %.3f rr4 %.3f | cpu path rr1 %.3f rr4 %.3f"
          % (dev[1], dev[4], cpu[1], cpu[4]))
    assert dev[4] > dev[1], dev
    for rr in (1, 4):
        assert dev[rr] >= cpu[rr] - 0.02, (rr, dev, cpu)


def test_index_cache_is_keyed_by_algorithm_and_parameters(monkeypatch):
    from spark_rapids_ml_nai_amd.models import knn as mk

    built = []
    real_pq = mk.build_ivfpq
    monkeypatch.setattr(mk, "build_ivfpq", lambda *a, **k: built.append("pq") or real_pq(*a, **k))
    X, Q = cases.blobs()
    model = _ann().fit(DataFrame.from_numpy(X[:500]))
    q = DataFrame.from_numpy(Q[:10])
    model.kneighbors(q)
    model.kneighbors(q)
    assert built == ["pq"]
    assert next(iter(model._index_cache.values())).codes.is_cuda
    monkeypatch.setattr(ops, "ivfpq_search", lambda *a, **k: pytest.fail("the PQ index was used for ivfflat"))
    model.setAlgorithm("ivfflat")
    _, _, knn_df = model.kneighbors(q)
    _, ind, dist = cases.knn_arrays(knn_df)
    np.testing.assert_allclose(dist, cases.direct_distance(X[:500], Q[:10], ind, "euclidean"), rtol=1e-5, atol=1e-5)


def test_approx_similarity_join():
    X, Q = cases.blobs()
    model = _ann(k=4).fit(DataFrame.from_numpy(X[:400]))
    join = model.approxSimilarityJoin(DataFrame.from_numpy(Q[:25]), distCol="dist")
    assert join.count() == 100
    r = join.collect()[0]
    d = np.linalg.norm(np.asarray(r["query_df"]["features"]) - np.asarray(r["item_df"]["features"]))
    assert np.isclose(d, r["dist"], rtol=1e-5)
