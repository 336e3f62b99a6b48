"""Sparse (CSR x CSR) kNN on the CPU: the torch reference of ``ops.csr_knn`` / ``ops.csr_refine_sort``
is held to the contract of ``csr_knn_cases``, and the contract checker itself is tested against
injected faults (a checker that accepts a broken search proves nothing on the device)."""
import numpy as np
import pytest
import torch

import csr_knn_cases as C
from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.core.base import CSR

W, TQ, TI = ops.CSR_KNN_W, ops.CSR_KNN_TQ, ops.CSR_KNN_TI


def test_exported_constants_are_the_kernels():
    """The edge shapes of the device tests are derived from these: they must be the kernels' own."""
    lib = ops.native.lib()
    got = tuple(int(lib.srml_csr_knn_config(i)) for i in range(5))
    assert got == (W, TQ, TI, ops.CSR_KNN_COOP, ops.CSR_REFINE_LDS_CAP)
    assert W * TQ * 4 <= 160 * 1024  # the window image fits the LDS


@pytest.mark.parametrize("m,n,nnz,k", C.GENERIC)
def test_reference_generic_cases(m, n, nnz, k):
    A, orc = C.generic_case(m, n, nnz, k)
    keys, ids = ops.csr_knn(A, A, k, "sqeuclidean")
    assert keys.dtype == torch.float32 and ids.dtype == torch.int64
    C.check_knn(orc, keys, ids, k, which="keys")
    d2, ids2 = ops.csr_refine_sort(A, A, ids)
    C.check_knn(orc, d2, ids2, k)
    dec = orc.decided(k)
    assert torch.equal(torch.sort(ids2[dec], dim=1).values, torch.sort(orc.topk_ids(k)[dec], dim=1).values)


@pytest.mark.parametrize("metric", ["hellinger", "jaccard"])
def test_reference_hellinger_jaccard(metric):
    m, n, nnz, k = C.GENERIC[0]
    A, orc = C.generic_case(m, n, nnz, k, metric)
    d, ids = ops.csr_knn(A, A, k, metric)
    C.check_knn(orc, d * d if metric == "hellinger" else d, ids, k)
    C.check_pairdist(orc, ops.csr_pairwise_dist(A, A, metric))


@pytest.mark.parametrize("metric", ["sqeuclidean", "hellinger", "jaccard"])
def test_reference_edge_shapes_and_row_blocks(metric):
    Q, I, orc = C.edge_case(TQ + 1, 40, 2 * W + 1, metric)
    C.check_pairdist(orc, ops.csr_pairwise_dist(Q, I, metric))
    # row blocks with absolute offsets, for both operands (held to the oracle of the block: a BLAS
    # product of another shape need not repeat the full product's bits; the device test asks for that)
    D = ops.csr_pairwise_dist(C.row_block(Q, 3, 11), C.row_block(I, 7, 33), metric)
    C.check_pairdist(C.Oracle(C.row_block(Q, 3, 11), C.row_block(I, 7, 33), metric), D)
    v, i = ops.csr_knn(ops.csr_prepare(Q, metric).rows(2, 9), ops.csr_prepare(I, metric), 5, metric, id_offset=100)
    C.check_knn(C.Oracle(C.row_block(Q, 2, 9), I, metric), v * v if metric == "hellinger" else v, i, 5, which="keys",
                id_offset=100)


def test_reference_padding_and_k1():
    Q, I, orc = C.edge_case(TQ - 1, 12, W + 1)
    for k in (1, 12, 20):
        d2, ids = C.knn_refined(Q, I, k)
        C.check_knn(orc, d2, ids, k)


def test_duplicates_and_near_duplicates_reference():
    A = C.near_duplicates()
    orc = C.Oracle(A, A)
    d2, ids = C.knn_refined(A, A, 4)
    C.check_knn(orc, d2, ids, 4)
    assert (d2[:, 0] == 0).all() and torch.equal(ids[:, 0], torch.arange(A.shape[0]))
    assert torch.allclose(d2[:16, 1].double(), torch.full((16,), 2.0 ** -20, dtype=torch.float64), rtol=1e-3)


# --- the checker against injected faults ---------------------------------------------------------
def _case():
    A, orc = C.generic_case(*C.GENERIC[0])
    return A, orc, C.GENERIC[0][3]


def test_checker_accepts_the_reference_and_rejects_a_dropped_nonzero():
    A, orc, k = _case()
    C.check_knn(orc, *C.knn_refined(A, A, k), k)
    # the largest value of row 0 dropped from the matrix that is searched
    a, b = int(A.indptr[0]), int(A.indptr[1])
    data = A.data.clone()
    data[a + int(A.data[a:b].abs().argmax())] = 0.0
    B = CSR(indptr=A.indptr, indices=A.indices, data=data, shape=A.shape)
    with pytest.raises(AssertionError):
        C.check_knn(orc, *C.knn_refined(B, B, k), k)


def test_checker_rejects_an_omitted_window():
    Q, I, orc = C.edge_case(TQ + 1, 40, 2 * W + 1)
    keep = I.indices < W  # the second and third windows contribute nothing
    data = torch.where(keep, I.data, torch.zeros_like(I.data))
    I2 = CSR(indptr=I.indptr, indices=I.indices, data=data, shape=I.shape)
    with pytest.raises(AssertionError):
        C.check_pairdist(orc, ops.csr_pairwise_dist(Q, I2, "sqeuclidean"))
    with pytest.raises(AssertionError):
        C.check_knn(orc, *C.knn_refined(Q, I2, 5), 5)


def test_checker_rejects_swapped_ids():
    A, orc, k = _case()
    d2, ids = C.knn_refined(A, A, k)
    ids = ids.clone()
    ids[7, [2, 9]] = ids[7, [9, 2]]
    with pytest.raises(AssertionError):
        C.check_knn(orc, d2, ids, k)


def test_checker_rejects_a_rebased_indptr():
    A, orc, k = _case()
    blk = C.row_block(A, 100, 200)
    sub = C.Oracle(blk, A)
    C.check_knn(sub, *C.knn_refined(blk, A, k), k)
    # validation would refuse most re-based blocks (their rows are cut at the wrong places); the fault
    # is injected behind it, as a search that re-bases internally would
    P = ops.csr_prepare(blk, "sqeuclidean")
    rebased = ops.CSRRows(P.indptr - P.indptr[0], P.indices, P.data, P.shape, P.aux, P.metric)
    with pytest.raises(AssertionError):
        C.check_knn(sub, *C.knn_refined(rebased, A, k), k)


def test_checker_rejects_expanded_form_distances_of_near_duplicates():
    A = C.near_duplicates()
    orc = C.Oracle(A, A)
    keys, ids = ops.csr_knn(A, A, 4, "sqeuclidean")
    C.check_knn(orc, keys, ids, 4, which="keys")  # fine as selection keys
    with pytest.raises(AssertionError):
        C.check_knn(orc, keys, ids, 4)  # useless as distances


# --- validation ------------------------------------------------------------------------------------
def _small():
    return C.csr_from_rows([(np.array([0, 3, 5]), np.array([1.0, 2.0, 3.0])), (np.array([1, 2]), np.array([1.0, 1.0]))], 6)


def test_prepare_rejects_bad_input(monkeypatch):
    launched = []
    monkeypatch.setattr(ops, "_csr_pairdist_launch", lambda *a: launched.append(a))
    A = _small()
    bad = CSR(indptr=A.indptr, indices=torch.tensor([0, 5, 3, 1, 2], dtype=torch.int32), data=A.data, shape=A.shape)
    with pytest.raises(ValueError, match="strictly increasing"):
        ops.csr_knn(bad, A, 1, "euclidean")
    dup = CSR(indptr=A.indptr, indices=torch.tensor([0, 3, 3, 1, 2], dtype=torch.int32), data=A.data, shape=A.shape)
    with pytest.raises(ValueError, match="strictly increasing"):
        ops.csr_prepare(dup, "jaccard")
    for ix in ([0, 3, 6, 1, 2], [-1, 3, 5, 1, 2]):
        oob = CSR(indptr=A.indptr, indices=torch.tensor(ix, dtype=torch.int32), data=A.data, shape=A.shape)
        with pytest.raises(ValueError, match="out of range"):
            ops.csr_knn(A, oob, 1, "euclidean")
    neg = CSR(indptr=A.indptr, indices=A.indices, data=-A.data, shape=A.shape)
    with pytest.raises(ValueError, match="non-negative"):
        ops.csr_knn(neg, A, 1, "hellinger")
    with pytest.raises(ValueError, match="Unsupported sparse kNN metric"):
        ops.csr_knn(A, A, 1, "manhattan")
    assert launched == []
    # a row's first index may be lower than the previous row's last
    ops.csr_prepare(A, "euclidean")


def test_prepare_auxiliaries():
    A = _small()
    P = ops.csr_prepare(A, "l2")
    assert torch.equal(P.aux, torch.tensor([14.0, 2.0]))
    J = ops.csr_prepare(A, "jaccard")
    assert torch.equal(J.aux, torch.tensor([3.0, 2.0])) and (J.data == 1).all()
    H = ops.csr_prepare(A, "hellinger")
    assert H.aux is None and torch.equal(H.data, torch.sqrt(A.data))
    assert ops.csr_prepare(P, "euclidean") is P
    with pytest.raises(ValueError):
        ops.csr_prepare(P, "jaccard")
