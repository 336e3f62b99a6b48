"""The CSR x CSR distance and refine kernels (``srml_csr_pairdist_f32`` / ``srml_csr_refine_f32``)
on the device against the fp64 oracle of ``csr_knn_cases`` (never against the CPU path), at the
kernels' edges. Every edge shape is derived from the constants ``ops`` exports: window width W,
query rows per block TQ, item rows per block TI, the wave-sharing threshold and the refine
kernel's LDS cap."""
import numpy as np
import pytest
import torch

import csr_knn_cases as C
from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.core.base import CSR

pytestmark = pytest.mark.gpu

W, TQ, TI, CAP = ops.CSR_KNN_W, ops.CSR_KNN_TQ, ops.CSR_KNN_TI, ops.CSR_REFINE_LDS_CAP
METRICS = ["sqeuclidean", "hellinger", "jaccard"]


def _sq(d, metric):
    return d * d if metric == "hellinger" else d


@pytest.mark.parametrize("m,n,nnz,k", C.GENERIC)
def test_device_generic_cases(gpu_device, m, n, nnz, k):
    A, orc = C.generic_case(m, n, nnz, k)
    Ad = C.to(A, gpu_device)
    keys, ids = ops.csr_knn(Ad, Ad, k, "sqeuclidean")
    assert keys.is_cuda and keys.dtype == torch.float32 and ids.dtype == torch.int64
    rk = C.check_knn(orc, keys, ids, k, which="keys")
    d2, ids2 = ops.csr_refine_sort(Ad, Ad, ids)
    rr = C.check_knn(orc, d2, ids2, k)
    dec = orc.decided(k)
    assert torch.equal(torch.sort(ids2.cpu()[dec], dim=1).values, torch.sort(orc.topk_ids(k)[dec], dim=1).values)
    print("sqeuclidean (%d, %d, %d, %d): keys err/bound %.3f, refined err/bound %.3f" % (m, n, nnz, k, rk, rr))


@pytest.mark.parametrize("metric", ["hellinger", "jaccard"])
def test_device_hellinger_jaccard(gpu_device, metric):
    m, n, nnz, k = C.GENERIC[0]
    A, orc = C.generic_case(m, n, nnz, k, metric)
    Ad = C.to(A, gpu_device)
    d, ids = ops.csr_knn(Ad, Ad, k, metric)
    r = C.check_knn(orc, _sq(d, metric), ids, k)
    r2 = C.check_pairdist(orc, ops.csr_pairwise_dist(Ad, Ad, metric))
    print("%s: knn err/bound %.3f, pairwise err/bound %.3f" % (metric, r, r2))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, W - 1, W, W + 1, 2 * W + 1])
def test_device_window_edges(gpu_device, metric, n):
    """Column counts around the window width: non-zeros at columns W - 1 and W, rows living in the
    last window only, rows with an empty window, empty rows, a row with nnz = n (which also crosses
    the wave-sharing threshold) on both sides."""
    Q, I, orc = C.edge_case(TQ + 1, 40, n, metric)
    Qd, Id = C.to(Q, gpu_device), C.to(I, gpu_device)
    r = C.check_pairdist(orc, ops.csr_pairwise_dist(Qd, Id, metric))
    k = 7
    d, ids = ops.csr_knn(Qd, Id, k, metric)
    C.check_knn(orc, _sq(d, metric), ids, k, which="keys")
    if metric == "sqeuclidean":
        C.check_knn(orc, *ops.csr_refine_sort(Qd, Id, ids), k)
    print("%s n=%d: pairwise err/bound %.3f" % (metric, n, r))


@pytest.mark.parametrize("mq", [1, TQ - 1, TQ, TQ + 1])
@pytest.mark.parametrize("mi", [1, TI - 1, TI, TI + 1])
def test_device_tile_edges(gpu_device, mq, mi):
    """Query counts around the query tile, item counts 1 and either side of a block's item rows."""
    Q, I, orc = C.edge_case(mq, mi, W + 1)
    Qd, Id = C.to(Q, gpu_device), C.to(I, gpu_device)
    C.check_pairdist(orc, ops.csr_pairwise_dist(Qd, Id, "sqeuclidean"))
    for k in (1, min(mi, 5), mi + 3):  # k = 1, a few, and past the items (padding)
        C.check_knn(orc, *C.knn_refined(Qd, Id, k), k)


@pytest.mark.parametrize("k", [1, 64, 65])
def test_device_k_edges(gpu_device, k):
    Q, I, orc = C.edge_case(TQ + 1, TI + 1, W + 1)
    C.check_knn(orc, *C.knn_refined(C.to(Q, gpu_device), C.to(I, gpu_device), k), k)


def test_device_refine_lds_cap(gpu_device):
    """Query rows with CAP - 1, CAP and CAP + 1 non-zeros: staged in LDS up to the cap, read from
    global memory past it; candidates include short rows, long rows and a missing one (-1)."""
    n = CAP + 40
    rng = np.random.default_rng(5)
    rows = []
    for c in (CAP - 1, CAP, CAP + 1, 3, 0):
        cols = np.sort(rng.choice(n, c, replace=False))
        rows.append((cols, rng.standard_normal(c).astype(np.float32)))
    rows += C.random_rows(12, n, 30, 6)
    A = C.csr_from_rows(rows, n)
    orc = C.Oracle(A, A)
    Ad = C.to(A, gpu_device)
    m = A.shape[0]
    ids = torch.arange(m).repeat(m, 1)
    ids[:, 5] = -1
    d2, out = ops.csr_refine_sort(Ad, Ad, ids.to(gpu_device))
    d2, out = d2.cpu().double(), out.cpu()
    assert (out[:, -1] == -1).all() and torch.isinf(d2[:, -1]).all()
    got, j = d2[:, :-1], out[:, :-1]
    want, bound = orc.D.gather(1, j), orc.eps.gather(1, j)
    assert ((got - want).abs() <= bound).all(), float(((got - want).abs() - bound).max())
    assert (got[:, 1:] >= got[:, :-1]).all()


@pytest.mark.parametrize("metric", METRICS)
def test_device_row_blocks_with_absolute_offsets(gpu_device, metric):
    Q, I, orc = C.edge_case(2 * TQ + 3, 60, W + 1, metric)
    Qd, Id = C.to(Q, gpu_device), C.to(I, gpu_device)
    full = ops.csr_pairwise_dist(Qd, Id, metric)
    C.check_pairdist(orc, full)
    blk = ops.csr_pairwise_dist(C.row_block(Qd, 5, TQ + 9), C.row_block(Id, 7, 51), metric)
    assert torch.equal(blk, full[5: TQ + 9, 7:51])
    P = ops.csr_prepare(Id, metric)
    v0, i0 = ops.csr_knn(Qd, P, 6, metric)
    v1, i1 = ops.csr_knn(ops.csr_prepare(Qd, metric).rows(3, TQ + 5), P.rows(7, 51), 6, metric, id_offset=7)
    sub = C.Oracle(C.row_block(Q, 3, TQ + 5), C.row_block(I, 7, 51), metric)
    C.check_knn(sub, _sq(v1, metric), i1, 6, which="keys", id_offset=7)
    if metric == "sqeuclidean":
        d2, i2 = ops.csr_refine_sort(C.row_block(Qd, 3, TQ + 5), Id, i1)  # ids of the whole item matrix
        C.check_knn(sub, d2, i2, 6, id_offset=7)


def test_device_duplicates_and_near_duplicates(gpu_device):
    A = C.near_duplicates()
    orc = C.Oracle(A, A)
    Ad = C.to(A, gpu_device)
    keys, ids = ops.csr_knn(Ad, Ad, 4, "sqeuclidean")
    C.check_knn(orc, keys, ids, 4, which="keys")
    d2, ids2 = ops.csr_refine_sort(Ad, Ad, ids)
    r = C.check_knn(orc, d2, ids2, 4)
    assert (d2[:, 0] == 0).all() and torch.equal(ids2[:, 0].cpu(), torch.arange(A.shape[0]))
    # bit-identical rows at distance 0: the lower id first
    Q, I, orc2 = C.edge_case(TQ + 1, 40, W + 1)
    d2, ids2 = C.knn_refined(C.to(I, gpu_device), C.to(I, gpu_device), 3)
    C.check_knn(C.Oracle(I, I), d2, ids2, 3)
    assert ids2[39, 0] == 0 and ids2[39, 1] == 39 and (d2[39, :2] == 0).all()
    print("near duplicates: refined err/bound %.3f" % r)


@pytest.mark.parametrize("metric", METRICS)
def test_device_chunked_equals_single(gpu_device, monkeypatch, metric):
    mq, mi, k = 3 * TQ + 5, 2 * TI + 40, 15
    Q, I, _ = C.edge_case(mq, mi, W + 1, metric)
    Qd, Id = C.to(Q, gpu_device), C.to(I, gpu_device)
    d0, i0 = ops.csr_knn(Qd, Id, k, metric)
    monkeypatch.setattr(ops, "_KNN_DIST_BYTES", TQ * TI * 4)  # TI-item chunks (3), TQ-query chunks (4)
    launches = []
    orig = ops._csr_pairdist_launch
    monkeypatch.setattr(ops, "_csr_pairdist_launch", lambda *a: (launches.append((a[1], a[2], a[4], a[5])), orig(*a))[1])
    d1, i1 = ops.csr_knn(Qd, Id, k, metric)
    assert len(launches) == 12 and {a[1] for a in launches} == {TQ, 5} and {a[3] for a in launches} == {TI, 40}
    assert torch.equal(d0, d1) and torch.equal(i0, i1)


def test_device_bad_input_raises_and_launches_nothing(gpu_device, monkeypatch):
    launched = []
    monkeypatch.setattr(ops, "_csr_pairdist_launch", lambda *a: launched.append(a))
    A = C.to(C.csr_from_rows([(np.array([0, 3, 5]), np.ones(3)), (np.array([1, 2]), np.ones(2))], 6), gpu_device)

    def with_indices(ix):
        return CSR(indptr=A.indptr, indices=torch.tensor(ix, dtype=torch.int32, device=gpu_device), data=A.data,
                   shape=A.shape)

    for bad in (with_indices([0, 5, 3, 1, 2]), with_indices([0, 3, 6, 1, 2]), with_indices([0, 3, 3, 1, 2])):
        with pytest.raises(ValueError):
            ops.csr_knn(bad, A, 1, "euclidean")
        with pytest.raises(ValueError):
            ops.csr_pairwise_dist(A, bad, "jaccard")
    neg = CSR(indptr=A.indptr, indices=A.indices, data=-A.data, shape=A.shape)
    with pytest.raises(ValueError):
        ops.csr_knn(neg, A, 1, "hellinger")
    assert launched == []
