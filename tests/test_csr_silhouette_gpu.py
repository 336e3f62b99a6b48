"""The CSR silhouette kernels (csrc/csr_silhouette.hip) against the direct O(m^2) definition, held to
the derived bound of test_csr_silhouette.py (builder, bound and checker are imported from there)."""
import numpy as np
import pytest
import torch

from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.core.dataframe import DataFrame
from spark_rapids_ml_nai_amd.evaluation import ClusteringEvaluator
from spark_rapids_ml_nai_amd.utils.determinism import set_deterministic
from test_csr_silhouette import bounds, check, lattice, make_case, sums_pair, to_csr

pytestmark = pytest.mark.gpu
M = 129  # not a multiple of the rows per block


def edge_lengths(k):
    """Row lengths around every step of the kernel that serves k: the E = 64 / kp non-zeros a wave
    keeps in flight, its unrolled loop, and the LDS stage of the tiled kernel."""
    _, stage, _, unroll = ops.csr_silhouette_config()
    e = max(1, 64 // ops.csr_silhouette_kp(k))
    return sorted({0, 1, max(e - 1, 0), e, e + 1, unroll * e - 1, unroll * e + 1, stage - 1, stage + 1}) + [2, 3]


SHAPES = [(M, k, 1000) for k in (2, 3, 8, 9, 16, 17, 33, 64, 65, 129)] + [(M, 3, 1), (M, 9, 100), (M, 8, 2 ** 20),
                                                                          (M, 65, 2 ** 20)]


@pytest.mark.parametrize("m,k,n", SHAPES)
def test_shapes(m, k, n):
    A, lab, w = make_case(m, k, n, edge_lengths(k))
    check(A, lab, w, k, "squaredEuclidean", "cuda")


@pytest.mark.parametrize("head", (1, 2))
@pytest.mark.parametrize("k", (8, 129))
def test_short_block_of_a_partitioned_set(head, k):
    A, lab, w = make_case(M, k, 1000, edge_lengths(k)[1:])
    check(A, lab, w, k, "squaredEuclidean", "cuda", head=head)


@pytest.mark.parametrize("measure", ("squaredEuclidean", "cosine"))
@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("k", (9, 129))
def test_measures_and_weights(measure, weighted, k):
    # ids 2 .. k-3 but one are empty, k // 2 holds a single row, row m // 3 is weightless when weighted
    A, lab, w = make_case(M, k, 100, None if measure == "cosine" else [0, 1, 5, 100, 7], measure, weighted)
    rows = check(A, lab, w, k, measure, "cuda")
    assert rows[M // 2] == 0 and (not weighted or rows[M // 3] == 0)


@pytest.mark.parametrize("k", (4, 260))
def test_lattice_is_exact(k):
    A, lab = lattice(k)
    rows = check(A, lab, None, k, "squaredEuclidean", "cuda", exact=True)
    assert (rows[[0, 4, 5, 6, 7]] == 0).all()  # a == b tie and the a = b = 0 duplicates


@pytest.mark.parametrize("measure", ("squaredEuclidean", "cosine"))
def test_bit_identical_runs(measure):
    A, lab, w = make_case(M, 9, 100, measure=measure, weighted=True)
    Ad, labd, wd = to_csr(A, "cuda"), torch.from_numpy(lab).cuda(), torch.from_numpy(w).cuda()
    N, Y = ops.silhouette_sums(Ad, labd, 9, wd, measure)
    stats = (N, Y, None if measure == "cosine" else ops.silhouette_psi(Ad, labd, 9, ops.silhouette_centre(N, Y), wd))
    one, two = (ops.silhouette(Ad, labd, 9, wd, measure, stats=stats, rows_out=True) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(one, two))
    set_deterministic(True)  # the sums pass on exact i64 atomics: end to end
    try:
        one, two = (ops.silhouette(Ad, labd, 9, wd, measure, rows_out=True) for _ in range(2))
    finally:
        set_deterministic(None)
    assert all(torch.equal(x, y) for x, y in zip(one, two))
    s, _, bound = bounds(A, lab, w, measure)
    assert (np.abs(one[2].cpu().numpy() - s) <= bound).all()


def test_evaluator_and_errors(monkeypatch):
    A, lab, w = make_case(M, 9, 100, weighted=True)
    s, ww, bound = bounds(A, lab, w, "squaredEuclidean")
    df = DataFrame.from_numpy(A, extra={"prediction": 3.0 * lab, "w": w}, num_partitions=3)
    got = ClusteringEvaluator(weightCol="w", enable_sparse_data_optim=True).evaluate(df)
    assert abs(got - (ww * s).sum() / ww.sum()) <= (ww * bound).sum() / ww.sum() + M * 2.0 ** -53
    Ad, labd = to_csr(A, "cuda"), torch.from_numpy(lab).cuda()
    stats = ops.silhouette_sums(Ad, labd, 9) + (torch.ones(9, dtype=torch.float64),)
    bad = to_csr(A, "cuda")
    bad.indices[0] = 100
    with pytest.raises(ValueError, match="CSR column"):
        ops.silhouette(bad, labd, 9, stats=stats)
    monkeypatch.setattr(ops, "_CSR_KM_CT_BYTES", 1024)
    with pytest.raises(ValueError, match="cluster table"):
        ops.silhouette(Ad, labd, 9, stats=stats)


def test_config_is_the_shared_table_config():
    km = ops.native.lib().srml_csr_kmeans_config
    assert ops.csr_silhouette_config()[:3] == tuple(int(km(i)) for i in range(3))


def test_sums_share_the_label_sums_kernel():
    Y, sums = sums_pair("cuda")
    assert torch.equal(Y, sums)  # no factor: the cluster sums, exact integer sums on one scale
    assert torch.equal(sums_pair("cuda", weighted=True)[0].cpu(), sums_pair("cpu", weighted=True)[0])  # a factor
