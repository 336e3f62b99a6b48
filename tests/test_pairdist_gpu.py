"""The tiled distance kernel ``srml_pairdist_f32`` (``ops.pairwise_dist`` / ``ops.knn_metric``) on the
device against an fp64 torch evaluation of the metric table, at the kernel's edges: its tile is
64 queries x 128 items, features stream in chunks of 32, 16-byte loads need n % 4 == 0."""
import numpy as np
import pytest
import torch

from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.models import umap as U
from spark_rapids_ml_nai_amd.models.knn_graph import knn_graph_metric

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
FLOOR = 1e-7
SHAPES = [(1, 1, 1), (3, 130, 3), (65, 63, 31), (129, 257, 33), (130, 70, 70), (64, 128, 128)]
CODES = [("l1", 2.0), ("linf", 2.0), ("minkowski", 1.5), ("minkowski", 3.0), ("minkowski", 4.0), ("canberra", 2.0),
         ("hamming", 2.0), ("jaccard", 2.0), ("hellinger", 2.0)]


def _data(name, mq, mi, n, seed):
    """fp32 rows fit for the metric: continuous with planted zeros, 0/1 with all-zero rows, or
    non-negative rows of sum 1."""
    g = torch.Generator().manual_seed(seed)
    if name in ("hamming", "jaccard"):
        A, B = (torch.rand((mq, n), generator=g) < 0.3).float(), (torch.rand((mi, n), generator=g) < 0.3).float()
        A[0], B[mi // 2] = 0.0, 0.0
        return A, B
    if name == "hellinger":
        A, B = torch.rand((mq, n), generator=g), torch.rand((mi, n), generator=g)
        A[:, 0] += 1e-3  # no all-zero row after the planted zeros
        B[:, 0] += 1e-3
        A[::2, (n + 1) // 2:] = 0.0
        A, B = A / A.sum(1, keepdim=True), B / B.sum(1, keepdim=True)
        B[0] = A[0]  # a pair at distance ~0: 1 - sum cancels
        return A, B
    A, B = torch.randn((mq, n), generator=g), torch.randn((mi, n), generator=g)
    A[::3, 0], B[::2, 0] = 0.0, 0.0  # 0 / 0 canberra terms
    return A, B


def _oracle(A, B, name, p):
    """fp64 evaluation of the metric table on the fp32 inputs (hellinger: returns d^2 = max(0, 1 - S))."""
    a, b = A.double().unsqueeze(1), B.double().unsqueeze(0)
    n = A.shape[1]
    if name == "l1":
        return (a - b).abs().sum(-1)
    if name == "linf":
        return (a - b).abs().amax(-1)
    if name == "minkowski":
        return (a - b).abs().pow(p).sum(-1).pow(1.0 / p)
    if name == "canberra":
        num, den = (a - b).abs(), a.abs() + b.abs()
        return torch.where(den > 0, num / den.clamp_min(1e-300), torch.zeros_like(num)).sum(-1)
    if name == "hamming":
        return (a != b).double().sum(-1) / n
    if name == "jaccard":
        inter = ((a != 0) & (b != 0)).double().sum(-1)
        uni = ((a != 0) | (b != 0)).double().sum(-1)
        return torch.where(uni > 0, 1.0 - inter / uni.clamp_min(1), torch.zeros_like(uni))
    assert name == "hellinger"
    return (1.0 - (a.sqrt() * b.sqrt()).sum(-1)).clamp_min(0)


def _minkowski_rtol(A, B, p, n):
    """8 x the deviation of a plain fp32 CPU evaluation from the fp64 oracle, at least the l1 bound:
    the device powf's error is not derivable from the code; host and device powf each carry a few
    ulp per term and need not agree in sign."""
    ref = _oracle(A, B, "minkowski", p)
    cpu32 = (A.unsqueeze(1) - B.unsqueeze(0)).abs().pow(p).sum(-1).pow(1.0 / p).double()
    dev = ((cpu32 - ref).abs() / ref.clamp_min(1e-30))[ref > 0]
    cpu_dev = float(dev.max()) if dev.numel() else 0.0
    return max(8.0 * cpu_dev, 4 * (n + 4) * U24)


def _check(D, A, B, name, p):
    """Device distances D against the oracle under the bound of the metric."""
    n = A.shape[1]
    ref = _oracle(A, B, name, p)
    got = D.double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    if name == "hellinger":
        # the bound applies to S = sum sqrt(x) sqrt(y) (non-negative terms); d^2 = 1 - S inherits it as
        # an absolute error rtol * S <= rtol * 1 (+ the rounding of 1 - S and of the fp32 square roots)
        S = 1.0 - ref
        tol2 = 4 * (n + 4) * U24 * S + 4 * U24 + FLOOR
        err2 = (got * got - ref).abs()
        assert (err2 <= tol2).all(), (name, float((err2 - tol2).max()))
        far = ref > 1e-3  # d itself only where 1 - S is well away from the cancellation
        d = ref.sqrt()
        tol = tol2 / (2 * d.clamp_min(1e-30)) + 2 * U24 * d + FLOOR
        assert ((got - d).abs()[far] <= tol[far]).all(), (name, float(((got - d).abs() - tol)[far].max()))
        return None
    if name == "linf":
        rtol = 4 * U24
    elif name == "minkowski":
        rtol = _minkowski_rtol(A, B, p, n)
    else:
        rtol = 4 * (n + 4) * U24
    err = (got - ref).abs()
    tol = rtol * ref.abs() + FLOOR
    observed = float((err / ref.abs().clamp_min(1e-30))[ref > 1e-3].max()) if (ref > 1e-3).any() else 0.0
    assert (err <= tol).all(), "%s p=%s: device relative deviation %.3e, allowed %.3e" % (name, p, observed, rtol)
    return observed


@pytest.mark.parametrize("name,p", CODES)
@pytest.mark.parametrize("mq,mi,n", SHAPES)
def test_pairwise_dist_device_matches_fp64(gpu_device, name, p, mq, mi, n):
    A, B = _data(name, mq, mi, n, seed=mq * 1000 + mi + n)
    D = ops.pairwise_dist(A.to(gpu_device), B.to(gpu_device), name, p)
    assert D.is_cuda and D.dtype == torch.float32
    obs = _check(D, A, B, name, p)
    if name == "minkowski":
        print("minkowski p=%s (%d, %d, %d): device relative deviation %.3e" % (p, mq, mi, n, obs))


@pytest.mark.parametrize("name,p", CODES)
def test_pairwise_dist_device_strided_unaligned(gpu_device, name, p):
    """Rows are a column slice of a wider tensor (row stride > n) starting at an odd column: the
    base pointer is 4-byte aligned only, so the kernel takes its element-load path."""
    mq, mi, n = 70, 131, 37
    A, B = _data(name, mq, mi, n, seed=11)
    wa = torch.full((mq, n + 9), 7.0, device=gpu_device)
    wb = torch.full((mi, n + 6), 7.0, device=gpu_device)
    wa[:, 1: 1 + n], wb[:, 3: 3 + n] = A.to(gpu_device), B.to(gpu_device)
    Av, Bv = wa[:, 1: 1 + n], wb[:, 3: 3 + n]
    assert Av.data_ptr() % 16 != 0 and Av.stride(0) > n
    _check(ops.pairwise_dist(Av, Bv, name, p), A, B, name, p)


def _separated(name, p, mq, mi, n, k, seed0):
    """Continuous data whose oracle k-th and (k+1)-th distances (and every pair before them: the
    ids are compared in order) differ by more than 10 x the tolerance on every row; another seed
    until that holds. Returns the data, the oracle's sorted (distances, ids) and the tolerance."""
    for seed in range(seed0, seed0 + 2000):
        g = torch.Generator().manual_seed(seed)
        A, B = torch.randn((mq, n), generator=g), torch.randn((mi, n), generator=g)
        rtol = {"linf": 4 * U24, "minkowski": _minkowski_rtol(A, B, p, n)}.get(name, 4 * (n + 4) * U24)
        sv, sj = torch.sort(_oracle(A, B, name, p), dim=1, stable=True)
        if (sv[:, 1: k + 1] - sv[:, :k] > 10 * (rtol * sv[:, 1: k + 1] + FLOOR)).all():
            return A, B, sv, sj, rtol
    raise AssertionError("no separated data found")


@pytest.mark.parametrize("name,p", [("l1", 2.0), ("canberra", 2.0), ("minkowski", 3.0), ("linf", 2.0)])
@pytest.mark.parametrize("k", [1, 15, 64, 65])
@pytest.mark.parametrize("mi", [70, 300])
def test_knn_metric_device_ids_and_distances(gpu_device, name, p, k, mi):
    mq, n = 12, 5  # few rows and features: 12 k gaps must all clear the bound
    A, B, sv, sj, rtol = _separated(name, p, mq, mi, n, k, seed0=1000 * k + mi)
    assert (sv[:, 1: k + 1] - sv[:, :k] > 10 * (rtol * sv[:, 1: k + 1] + FLOOR)).all()
    d, i = ops.knn_metric(A.to(gpu_device), B.to(gpu_device), k, name, p)
    assert d.dtype == torch.float32 and i.dtype == torch.int64 and d.shape == (mq, k)
    assert torch.equal(i.cpu(), sj[:, :k])
    assert ((d.double().cpu() - sv[:, :k]).abs() <= rtol * sv[:, :k] + FLOOR).all()


@pytest.mark.parametrize("name", ["hamming", "jaccard"])
@pytest.mark.parametrize("k", [1, 15, 65])
def test_knn_metric_device_heavy_ties(gpu_device, name, k):
    mq, mi, n = 67, 300, 12
    A, B = _data(name, mq, mi, n, seed=5)
    ref = _oracle(A, B, name, 2.0)
    d, i = ops.knn_metric(A.to(gpu_device), B.to(gpu_device), k, name)
    d, i = d.double().cpu(), i.cpu()
    tol = 4 * (n + 4) * U24
    want = torch.sort(ref, dim=1).values[:, :k]
    assert ((d - want).abs() <= tol * want + FLOOR).all()  # the k smallest, as a sorted list
    assert ((ref.gather(1, i) - d).abs() <= tol * d + FLOOR).all()  # each id carries its distance
    si = torch.sort(i, dim=1).values
    assert (si[:, 1:] != si[:, :-1]).all() and (i >= 0).all() and (i < mi).all()


def test_knn_metric_device_pads_past_the_items(gpu_device):
    A, B = _data("l1", 5, 9, 6, seed=2)
    d, i = ops.knn_metric(A.to(gpu_device), B.to(gpu_device), 12, "manhattan", id_offset=1000)
    assert torch.isinf(d[:, 9:]).all() and (i[:, 9:] == -1).all()
    ref = torch.sort(_oracle(A, B, "l1", 2.0), dim=1, stable=True)
    assert torch.equal(i[:, :9].cpu(), ref.indices + 1000)
    assert ((d[:, :9].double().cpu() - ref.values).abs() <= 40 * U24 * ref.values + FLOOR).all()


@pytest.mark.parametrize("name,p", [("l1", 2.0), ("hamming", 2.0), ("minkowski", 2.5)])
def test_knn_metric_device_chunked_equals_single(gpu_device, monkeypatch, name, p):
    mq, mi, n, k = 150, 300, 20, 15
    A, B = _data(name, mq, mi, n, seed=9)
    Ad, Bd = A.to(gpu_device), B.to(gpu_device)
    d0, i0 = ops.knn_metric(Ad, Bd, k, name, p)
    monkeypatch.setattr(ops, "_KNN_DIST_BYTES", 64 * 128 * 4)  # 128-item chunks (3), 64-query chunks (3)
    launches = []
    orig = ops._pairdist_launch
    monkeypatch.setattr(ops, "_pairdist_launch", lambda *a: (launches.append((a[1], a[3])), orig(*a))[1])
    d1, i1 = ops.knn_metric(Ad, Bd, k, name, p)
    assert len({r for r, _ in launches}) >= 2 and len(launches) == 9, launches
    assert torch.equal(d0, d1) and torch.equal(i0, i1)


def test_knn_graph_metric_self_graph(gpu_device):
    g = torch.Generator().manual_seed(4)
    X = torch.randn((333, 24), generator=g).to(gpu_device)
    for name, p in (("manhattan", 2.0), ("chebyshev", 2.0), ("canberra", 2.0), ("minkowski", 3.0)):
        d, i = knn_graph_metric(X, X, 10, name, p)
        assert torch.equal(i[:, 0].cpu(), torch.arange(333)) and (d[:, 0] == 0).all(), name
    Xb = (torch.rand((200, 40), generator=g) < 0.5).float()
    assert torch.unique(Xb, dim=0).shape[0] == 200
    for name in ("hamming", "jaccard"):
        d, i = knn_graph_metric(Xb.to(gpu_device), Xb.to(gpu_device), 10, name)
        assert torch.equal(i[:, 0].cpu(), torch.arange(200)) and (d[:, 0] == 0).all(), name


@pytest.mark.parametrize("metric", ["manhattan", "jaccard"])
def test_umap_device_fit_per_metric(gpu_device, metric):
    from sklearn.datasets import load_digits
    from sklearn.manifold import trustworthiness

    X = load_digits(return_X_y=True)[0].astype(np.float32)
    if metric == "jaccard":
        X = (X > 7).astype(np.float32)
    Xd = torch.from_numpy(X).to(gpu_device)
    params = {"n_neighbors": 15, "random_state": 1, "n_epochs": 200, "metric": metric}
    emb = U.umap_fit(Xd, params)
    assert emb.shape == (1797, 2) and np.isfinite(emb).all()
    Xs = X.astype(bool) if metric == "jaccard" else X
    assert trustworthiness(Xs, emb, n_neighbors=15, metric=metric) > 0.9
    e2 = U.umap_transform(Xd, Xd, torch.from_numpy(emb).to(gpu_device), params)
    assert e2.shape == (1797, 2) and np.isfinite(e2).all()
