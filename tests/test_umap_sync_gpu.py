"""Synchronous UMAP epoch on the device: ``ops.umap_epoch_sync`` against its CPU oracle on every
head (runs inside a wave, across waves and blocks, around an idle wave), bit-equal repeats, and
seeded fits / transforms that repeat bit for bit in deterministic mode."""
import numpy as np
import pytest
import torch

from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.models import umap as U
from spark_rapids_ml_nai_amd.utils.determinism import set_deterministic

pytestmark = pytest.mark.gpu

KW = dict(a=1.577, b=0.895, gamma=1.0, alpha=0.7, seed=3)
LONG = 201  # index of the head with 700 edges


def _graph(dim, same):
    """test_umap_epoch_head_runs' graph (400 heads of degree 1..150, every 7th of degree 1) plus a
    head of degree 700 (more than two 256-edge blocks) with 200 consecutive edges that are never
    due (a whole idle wave in the middle of a crossing run), 30 vertex ids without edges, and
    schedules that draw 5 and 10 negatives at the first epoch (below and above the 8-draw prefetch
    group of the dim <= 4 kernels). eps / eps_neg are small dyadic numbers, so the schedule
    arithmetic is exact whether or not the compiler contracts it into an fma."""
    g = torch.Generator().manual_seed(11 + dim)
    nh, nv, nt = 400, 430, 700
    deg = torch.randint(1, 151, (nh,), generator=g)
    deg[::7] = 1
    deg[LONG] = 700
    if int(deg.sum()) % 64 == 0:
        deg[-1] += 1
    ids = torch.sort(torch.randperm(nv, generator=g)[:nh]).values
    head = torch.repeat_interleave(ids, deg).int()
    E = head.numel()
    assert E % 64 != 0
    n_tail = nv if same else nt
    tail = torch.randint(0, n_tail, (E,), generator=g).int()
    eps = torch.where(torch.rand(E, generator=g) < 0.8, torch.ones(E), torch.full((E,), 3.0))
    next_sample = eps.clone()
    s = int(deg[:LONG].sum())
    next_sample[s + 250: s + 450] = 100.0
    eps_neg = torch.where(torch.rand(E, generator=g) < 0.5, torch.full((E,), 0.375), torch.full((E,), 0.1875))
    emb = torch.rand(nv, dim, generator=g) * 10
    embt = emb if same else torch.rand(nt, dim, generator=g) * 10
    return dict(head=head, tail=tail, eps=eps, next_sample=next_sample, next_neg=torch.zeros(E), eps_neg=eps_neg,
                emb=emb, embt=embt, deg=deg, ids=ids, n_tail=n_tail, seed_gen=g)


class _Side:
    """One replica of the epoch state (CPU oracle or device)."""

    def __init__(self, G, dev, same):
        to = lambda t: t.clone().to(dev)
        self.head, self.tail, self.eps, self.eps_neg = to(G["head"]), to(G["tail"]), to(G["eps"]), to(G["eps_neg"])
        self.ns, self.nn = to(G["next_sample"]), to(G["next_neg"])
        self.emb = to(G["emb"])
        self.embt = self.emb if same else to(G["embt"])

    def epoch(self, n, pull, move_other, line_ids=None, apply=True):
        neg = None
        if line_ids is not None:
            ids = line_ids.to(self.emb.device)
            neg = (ops.umap_neg_table(self.embt, ids, torch.empty(ids.shape[0], self.emb.shape[1],
                                                                   device=self.emb.device)), ids)
        kw = dict(KW, epoch=n, move_other=move_other, pull=pull, neg_table=neg, apply=apply)
        return ops.umap_epoch_sync(self.head, self.tail, self.eps, self.ns, self.nn, self.eps_neg, self.emb, self.embt,
                                   **kw).clone()


@pytest.mark.parametrize("lines", [False, True])
@pytest.mark.parametrize("same", [True, False])
@pytest.mark.parametrize("dim", [2, 5, 16])
def test_sync_epoch_matches_cpu_oracle(gpu_device, dim, same, lines):
    """``same``: pull on one shared table (the fit; Hogwild cannot be pinned there); otherwise
    heads move against a fixed tail table (the transform). Tolerance: test_umap_epoch_head_runs'
    rtol = atol = 1e-4 (hardware log2 / exp2 against torch.pow). Measured: every case inside it,
    the largest |emb - oracle| 8.4e-4, within the rtol term (the 700-edge head moves by up to
    56); the Hogwild kernel's one-wave runs with the same negatives differ from the same
    oracle by at most 3.4e-5."""
    G = _graph(dim, same)
    pull, move_other = same, same
    line_ids = None
    if lines:
        line_ids = torch.randperm(G["n_tail"], generator=G["seed_gen"])[: (G["n_tail"] // 8) * 8].int()
    cpu, gpu, gpu2 = _Side(G, "cpu", same), _Side(G, gpu_device, same), _Side(G, gpu_device, same)
    no_edges = torch.ones(G["emb"].shape[0], dtype=torch.bool)
    no_edges[G["ids"]] = False
    assert int(no_edges.sum()) == 30
    # Three consecutive epochs on the device's carried state: a stale workspace would show in the
    # later ones. An epoch is a pure function of its input, and
    # the repulsion near a negative is steep (up to 2 b / 0.001 per unit of distance), so the
    # oracle starts every epoch from the layout the device holds (measured: the 1e-4 of the first
    # epoch became 2e-3 after the second when each side carried its own layout); the schedules
    # are carried by each side and must stay equal bit for bit.
    for n in (2, 3, 4):
        n_neg = torch.trunc((n - cpu.nn) / cpu.eps_neg)[(cpu.ns <= n)]
        cpu.emb.copy_(gpu.emb.cpu())
        before = cpu.emb.clone()
        D_ref = cpu.epoch(n, pull, move_other, line_ids)
        D = gpu.epoch(n, pull, move_other, line_ids)
        D2 = gpu2.epoch(n, pull, move_other, line_ids)
        if n == 2:
            assert sorted(set(n_neg.tolist())) == [5.0, 10.0]
        assert float(D_ref[G["ids"][LONG]].abs().max()) > 0
        err = (gpu.emb.cpu() - cpu.emb).abs().max()
        print("dim %d same %s lines %s epoch %d: max |emb - oracle| = %.3g, max |D| = %.3g"
              % (dim, same, lines, n, float(err), float(D_ref.abs().max())))
        torch.testing.assert_close(D.cpu(), D_ref, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(gpu.emb.cpu(), cpu.emb, rtol=1e-4, atol=1e-4)  # every head
        assert torch.equal(cpu.emb, before + D_ref)
        assert torch.equal(D.cpu()[no_edges], torch.zeros(30, dim))
        assert torch.equal(gpu.ns.cpu(), cpu.ns) and torch.equal(gpu.nn.cpu(), cpu.nn)
        # identical inputs, identical bits
        assert torch.equal(D, D2) and torch.equal(gpu.emb, gpu2.emb)
        assert torch.equal(gpu.ns, gpu2.ns) and torch.equal(gpu.nn, gpu2.nn)
        if not same:
            assert torch.equal(gpu.embt.cpu(), G["embt"])
    assert float(cpu.ns[cpu.ns < 100].max()) > 3.0 and float(cpu.ns.max()) == 100.0


def test_sync_epoch_returns_moves_without_applying(gpu_device):
    G = _graph(3, False)
    gpu, ref = _Side(G, gpu_device, False), _Side(G, gpu_device, False)
    D = gpu.epoch(2, False, False, apply=False)
    assert torch.equal(gpu.emb.cpu(), G["emb"])
    ref.epoch(2, False, False)
    assert torch.equal(ref.emb, gpu.emb + D)


def test_sync_epoch_refuses_tail_moves(gpu_device):
    G = _graph(2, True)
    gpu = _Side(G, gpu_device, True)
    with pytest.raises(ValueError):
        gpu.epoch(2, False, True)
    assert torch.equal(gpu.emb.cpu(), G["emb"])
    # the native entry refuses on its own as well
    from spark_rapids_ml_nai_amd.ops import native

    with pytest.raises(Exception):
        native.call("srml_umap_epoch_sync", None, None, 0, None, None, None, None, None, None, None, 1, 1, 2, 1.0, 1.0,
                    1.0, 1.0, 1.0, 1, 0, 0, None, None, 0, None, 0, native.stream(gpu_device))


# ------------------------------------------------------------------------------------------
def _blobs(n):
    from sklearn.datasets import make_blobs

    return make_blobs(n, 16, centers=8, random_state=0)


FIT = {"n_neighbors": 15, "random_state": 3, "n_epochs": 50}


def _fit_twice(X, params, dev, y=None):
    Xt = torch.from_numpy(X).float().to(dev)
    yt = torch.from_numpy(y).to(dev) if y is not None else None
    set_deterministic(True)
    try:
        return U.umap_fit(Xt, params, y=yt), U.umap_fit(Xt, params, y=yt)
    finally:
        set_deterministic(None)


@pytest.mark.parametrize("case", ["dense_spectral", "csr_spectral", "random_init", "supervised", "precomputed_knn",
                                  "ivf", "nn_descent"])
def test_deterministic_fit_repeats_bit_for_bit(gpu_device, case):
    """Brute-force and precomputed graphs are reproducible by construction. The ivf / nn_descent
    builders hand out candidate slots in arrival order but select an order-independent top k: their
    graphs were bit-equal in every repeated build that was tried (12k and 200k rows)."""
    n = {"csr_spectral": 3000, "ivf": 12000, "nn_descent": 12000}.get(case, 1500)
    assert (n <= U.SPECTRAL_DENSE_N) == (case not in ("csr_spectral", "ivf", "nn_descent"))
    X, y = _blobs(n)
    params = dict(FIT)
    if case in ("ivf", "nn_descent"):
        params.update(build_algo=case, build_kwds={"nlist": 24, "nprobe": 8})
    if case == "random_init":
        params["init"] = "random"
    if case == "precomputed_knn":
        from sklearn.neighbors import NearestNeighbors

        dist, idx = NearestNeighbors(n_neighbors=15).fit(X).kneighbors(X)
        params["precomputed_knn"] = (idx, dist.astype(np.float32))
    e1, e2 = _fit_twice(X, params, gpu_device, y if case == "supervised" else None)
    assert e1.shape == (n, 2) and np.isfinite(e1).all()
    assert float(np.ptp(e1, axis=0).min()) > 1.0
    assert np.array_equal(e1, e2)


def test_deterministic_transform_repeats_bit_for_bit(gpu_device):
    X, _ = _blobs(2000)
    tr = torch.from_numpy(X[:1500]).float().to(gpu_device)
    new = torch.from_numpy(X[1500:]).float().to(gpu_device)
    set_deterministic(True)
    try:
        emb = torch.from_numpy(U.umap_fit(tr, FIT)).to(gpu_device)
        t1 = U.umap_transform(new, tr, emb, FIT)
        t2 = U.umap_transform(new, tr, emb, FIT)
    finally:
        set_deterministic(None)
    assert t1.shape == (500, 2) and np.isfinite(t1).all()
    assert np.array_equal(t1, t2)


@pytest.mark.parametrize("n", [1797, 6000])
def test_deterministic_fit_trustworthiness(gpu_device, n):
    """The margins of tests/test_umap_gpu.py: above 0.9, and within 0.01 of the Hogwild fit."""
    from sklearn.datasets import load_digits, make_blobs
    from sklearn.manifold import trustworthiness

    if n == 1797:
        X, _ = load_digits(return_X_y=True)
    else:
        X, _ = make_blobs(n, 20, centers=10, cluster_std=3.0, random_state=4)
    Xt = torch.from_numpy(X).float().to(gpu_device)
    params = {"n_neighbors": 15, "random_state": 1}
    hog = trustworthiness(X, U.umap_fit(Xt, params), n_neighbors=15)
    set_deterministic(True)
    try:
        emb = U.umap_fit(Xt, params)
    finally:
        set_deterministic(None)
    tw = trustworthiness(X, emb, n_neighbors=15)
    print("n %d: trustworthiness synchronous %.4f, Hogwild %.4f" % (n, tw, hog))
    assert tw > 0.9
    assert tw >= hog - 0.01
