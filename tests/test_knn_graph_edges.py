"""The kNN-graph builders (models/knn_graph.py; knn_graph.hip, knn.hip, ivf.hip, topk.hip,
group.hip, the fp16 bucketing of splitmm.hip) at their edges: k below the NN-descent fan-out, rows
with fewer than k reachable candidates (padded with -1), centres outside the range an fp16 plane was scaled for, and
padded graphs through the fuzzy-set kernels that consume them.

Every oracle is plain numpy / torch in fp64, written here, and calls none of the code under test.

Re-rank tolerance (``_rerank_tol``): the re-rank sums (q - i)^2 in fp32, a relative error of at
most (n + 4) 2^-24 against fp64 in any summation order; no absolute term (identical rows give
exact zeros). The builders return sqrt of that (half the relative error plus one rounding), which
the same bound covers.

Measured on an MI355X: section C, N = 3000, n = 16, nlist = nprobe = 12: recall of the fp16
candidate path 1.0000 (list and query probing), of the fp32 ranking 1.0000; N = 4000, nlist =
nprobe = 64, list probing: fp16 1.0000, fp32 1.0000; the fp32 keys' largest excess over the exact
j-th distance 5.1e-6 of a 3.6e-3 band. Largest re-rank error of the module: 0.42 x (n + 4) 2^-24.
Section D: with the centre plane's overflow flag unread the row loop mislabels 10 (n = 116) and 2
(n = 128) of the 16 rows whose nearest centre is out of range (excess 0.091 / 0.075 against the
5e-3 allowed); reading it, none. Section A on the device with padding edges counted as edges into
row 0: every padded case fails. The device tests of the module take 7 s.
"""
import functools

import numpy as np
import pytest
import torch

from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.models import umap as U
from spark_rapids_ml_nai_amd.models.knn_graph import build_knn_graph, nn_descent_refine

DEVICES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture(params=DEVICES)
def dev(request, monkeypatch):
    if request.param == "cpu":
        monkeypatch.setenv("SRML_FORCE_CPU", "1")
        return torch.device("cpu")
    monkeypatch.delenv("SRML_FORCE_CPU", raising=False)
    return torch.device("cuda", 0)


def _rerank_tol(n):
    return (n + 4) * 2.0 ** -24


def _assert_rerank(got, exact, n, what):
    """|got - exact| <= (n + 4) 2^-24 exact, elementwise (fp64 arrays); prints the largest error as
    a multiple of the bound."""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    err = np.abs(got - exact)
    bound = _rerank_tol(n) * exact
    ratio = float(np.max(np.where(exact > 0, err / np.where(exact > 0, bound, 1.0), 0.0))) if err.size else 0.0
    print("%s: largest re-rank error = %.3f x (n + 4) 2^-24" % (what, ratio))
    assert np.all(err <= bound), (what, ratio)
    return ratio


def _blobs(N, n, seed, centres=8, std=1.0):
    rng = np.random.default_rng(seed)
    C = rng.uniform(-10.0, 10.0, (centres, n))
    return (C[rng.integers(0, centres, N)] + std * rng.standard_normal((N, n))).astype(np.float32)


def _pair_d2(X64, idx):
    """fp64 squared distances of (row i, idx[i, j]); idx < 0 -> +inf."""
    nb = X64[np.clip(idx, 0, None)]
    d2 = ((nb - X64[:, None, :]) ** 2).sum(-1)
    return np.where(idx >= 0, d2, np.inf)


# ------------------------------------------------------------------------------------------
# A. one NN-descent round against an oracle
# ------------------------------------------------------------------------------------------
def _nnd_oracle(X64, pos, k, a=8, b=8, R=16):
    """nn_descent_refine's docstring, literally: row i re-ranks the union of its neighbours, its
    first a neighbours' first b neighbours and the first R rows (ascending) that list it; -1 is an
    edge to nobody; the k smallest fp64 distances, padded with +inf. Returns (D [N, k], sets)."""
    N = pos.shape[0]
    a, b = min(a, k), min(b, k)
    rev = [[] for _ in range(N)]
    for s in range(N):
        for t in pos[s]:
            if t >= 0 and len(rev[t]) < R:
                rev[t].append(s)
    D = np.full((N, k), np.inf)
    sets = []
    for i in range(N):
        own = [int(t) for t in pos[i] if t >= 0]
        c = set(own)
        for t in own[:a]:
            c.update([int(u) for u in pos[t] if u >= 0][:b])
        c.update(rev[i])
        ids = np.array(sorted(c), dtype=np.int64)
        d = np.sort(((X64[ids] - X64[i]) ** 2).sum(1))[:k]
        D[i, : d.shape[0]] = d
        sets.append(c)
    return D, sets


def _start_graph(N, n, k, variant):
    """Self plus k - 1 random neighbours, sorted by exact distance. ``half``: every third row is
    padded from column k / 2 on and row 7 keeps only itself; ``early``: every fourth row (1, 5, ..)
    is padded from column 2 on (inside the first a columns). In the padded variants the first two
    padded rows other than row 0 lie next to row 0 but are strangers to it: nobody lists them and
    they do not list row 0, so they are in none of row 0's candidate sets, and a builder that takes
    padding edges for edges into row 0 returns them as row 0's nearest."""
    rng = np.random.default_rng(1000 * N + 10 * n + k)
    X = rng.standard_normal((N, n)).astype(np.float32)
    if variant == "half":
        padded = {i: max(1, k // 2) for i in range(0, N, 3)}
        padded[7] = 1
    elif variant == "early":
        padded = {i: min(2, k - 1) for i in range(1, N, 4)}
    else:
        padded = {}
    strangers = [i for i in sorted(padded) if i != 0 and padded[i] < k][:2]
    for s in strangers:
        X[s] = X[0] + np.float32(1e-3) * rng.standard_normal(n).astype(np.float32)
    X64 = X.astype(np.float64)
    pos = np.full((N, k), -1, dtype=np.int64)
    for i in range(N):
        banned = set(strangers) | {i} | ({0} if i in strangers else set())
        pool = np.array([j for j in range(N) if j not in banned])
        row = np.concatenate([[i], rng.choice(pool, k - 1, replace=False)]) if k > 1 else np.array([i])
        d = ((X64[row] - X64[i]) ** 2).sum(1)
        pos[i] = row[np.argsort(d, kind="stable")]
    for i, c in padded.items():
        pos[i, c:] = -1
    return X, pos, strangers


@pytest.mark.parametrize("variant", ["full", "half", "early"])
@pytest.mark.parametrize("k", [3, 5, 8, 12])
@pytest.mark.parametrize("N,n", [(257, 5), (257, 8), (300, 5), (300, 8)])
def test_nn_descent_round_matches_oracle(dev, N, n, k, variant):
    X, pos, strangers = _start_graph(N, n, k, variant)
    X64 = X.astype(np.float64)
    D, sets = _nnd_oracle(X64, pos, k)
    if variant != "full":
        assert strangers and not (set(strangers) & sets[0])
        assert (pos < 0).any() and (pos[:, : min(8, k)] < 0).any()
    if variant == "half":
        assert (pos[7] >= 0).sum() == 1
    if dev.type == "cuda":
        # the device groups the edges with srml_label_sort (the torch.sort path is the CPU's)
        assert N <= int(ops.native.lib().srml_label_sort_kmax())
    Xt = torch.from_numpy(X).to(dev)
    d2_0 = torch.from_numpy(_pair_d2(X64, pos)).float().to(dev)
    dd, pp = nn_descent_refine(Xt, d2_0, torch.from_numpy(pos).to(dev), k, iters=1)
    assert dd.shape == (N, k) and pp.shape == (N, k)
    dd, pp = dd.cpu().numpy().astype(np.float64), pp.cpu().numpy()
    # the +inf / -1 pattern
    assert np.array_equal(np.isinf(dd), np.isinf(D))
    assert np.array_equal(pp < 0, np.isinf(D))
    assert pp.max() < N and pp.min() >= -1
    real = pp >= 0
    # the k smallest distances of the candidate set
    _assert_rerank(dd[real], D[real], n, "nn_descent N=%d n=%d k=%d %s (k smallest)" % (N, n, k, variant))
    # every id is a candidate of its row, appears once, and carries its exact distance
    for i in range(N):
        ids = pp[i][pp[i] >= 0].tolist()
        assert len(set(ids)) == len(ids), (i, ids)
        assert set(ids) <= sets[i], (i, sorted(set(ids) - sets[i]))
    _assert_rerank(dd[real], _pair_d2(X64, pp)[real], n, "nn_descent N=%d n=%d k=%d %s (pairs)" % (N, n, k, variant))
    # row 0 on its own: padding edges are edges to nobody, not edges into row 0
    ids0 = [int(t) for t in pp[0] if t >= 0]
    assert set(ids0) <= sets[0], sorted(set(ids0) - sets[0])
    assert not (set(ids0) & set(strangers))
    r0 = np.isfinite(D[0])
    assert np.all(np.abs(dd[0][r0] - D[0][r0]) <= _rerank_tol(n) * D[0][r0])


# ------------------------------------------------------------------------------------------
# B. builder contract on edge inputs
# ------------------------------------------------------------------------------------------
ALGOS = {
    "brute": ("brute_force_knn", {}),
    "ivf_list": ("ivf", {"probe": "list"}),
    "ivf_query": ("ivf", {"probe": "query"}),
    "nn_descent": ("nn_descent", {}),
}


@functools.lru_cache(maxsize=None)
def _edge_input(name):
    """(X fp32 [N, n], k, build_kwds) of a named edge input."""
    if name == "tiny_lists":
        return _blobs(40, 8, 3, centres=4), 10, {"nlist": 8, "nprobe": 1}
    if name == "duplicates":
        return np.tile(_blobs(200, 8, 4), (3, 1)), 10, {"nlist": 6, "nprobe": 3}
    if name == "nlist64":
        return _blobs(4000, 16, 5, centres=20), 10, {"nlist": 64}
    if name.startswith("nlist300_n"):
        return _blobs(4000, int(name[10:]), 6, centres=20), 10, {"nlist": 300}
    if name.startswith("k"):
        return _blobs(600, 16, 1), int(name[1:]), {"nlist": 6, "nprobe": 3}
    if name.startswith("n"):
        return _blobs(600, int(name[1:]), 2), 10, {"nlist": 6, "nprobe": 3}
    raise KeyError(name)


EDGE_INPUTS = (["k1", "k3", "k5", "k32", "k33", "n4", "n6", "n116", "n128", "n132", "tiny_lists", "duplicates",
                "nlist64", "nlist300_n116", "nlist300_n128"])
# tiny lists under list probing leave rows short of candidates: also through the NN-descent rounds
EDGE_CASES = [(i, a) for i in EDGE_INPUTS for a in ALGOS] + [("tiny_lists", "nn_descent_list")]
PADDED_CASES = {("tiny_lists", "ivf_list"), ("tiny_lists", "nn_descent_list")}


def _check_graph(X, dist, idx, k, what):
    """The builders' contract; returns the number of padded entries."""
    N, n = X.shape
    assert dist.shape == (N, k) and idx.shape == (N, k)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64
    d, ix = dist.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    assert np.all(np.isfinite(d))
    assert np.all(d[:, 1:] >= d[:, :-1]), "distances ascend per row"
    assert ix.min() >= -1 and ix.max() < N
    pad = ix < 0
    assert not pad[:, 0].any()
    assert np.all(pad[:, 1:] >= pad[:, :-1]), "-1 only as a suffix"
    s = np.sort(ix, axis=1)
    assert not np.any((s[:, 1:] == s[:, :-1]) & (s[:, 1:] >= 0)), "an id repeats within a row"
    rowmax = np.where(pad, -np.inf, d).max(1, keepdims=True)
    assert np.array_equal(d[pad], np.broadcast_to(rowmax, d.shape)[pad]), "padding carries the row's largest distance"
    ex = np.sqrt(_pair_d2(X.astype(np.float64), ix))
    _assert_rerank(d[~pad], ex[~pad], n, what)
    return int(pad.sum())


def _build(Xt, k, case_algo, kw, **extra):
    if case_algo == "nn_descent_list":
        algo, akw = "nn_descent", {"probe": "list"}
    else:
        algo, akw = ALGOS[case_algo]
    return build_knn_graph(Xt, k, algo, dict(kw, **akw), **extra)


@pytest.mark.parametrize("inp,algo", EDGE_CASES)
def test_builder_contract(dev, inp, algo):
    X, k, kw = _edge_input(inp)
    if algo in ("nn_descent", "nn_descent_list"):
        kw = dict(kw, nnd_iters=1)
    Xt = torch.from_numpy(X).to(dev)
    dist, idx = _build(Xt, k, algo, kw)
    npad = _check_graph(X, dist, idx, k, "%s %s %s" % (inp, algo, dev.type))
    print("%s %s %s: %d padded entries" % (inp, algo, dev.type, npad))
    if (inp, algo) in PADDED_CASES:
        # 40 rows in 8 lists of which each row scans one: no row reaches 10 candidates, so the
        # padding checks above (here and in section E) did check something
        assert npad > 0
    # list order: the same graph once positions are mapped through ``order``
    dl, il, order = _build(Xt, k, algo, kw, list_order=True)
    if order is None:
        assert algo == "brute"
        assert torch.equal(dl, dist) and torch.equal(il, idx)
        return
    assert torch.equal(torch.sort(order).values, torch.arange(X.shape[0], device=order.device))
    d_back = torch.empty_like(dl)
    d_back[order] = dl
    i_back = torch.empty_like(il)
    i_back[order] = torch.where(il >= 0, order[il.clamp_min(0)], torch.full_like(il, -1))
    assert torch.equal(d_back, dist) and torch.equal(i_back, idx)


# ------------------------------------------------------------------------------------------
# C. exhaustive probing must be exact
# ------------------------------------------------------------------------------------------
EXHAUSTIVE = [(3000, 6, 12, "list"), (3000, 6, 12, "query"), (3000, 16, 12, "list"), (3000, 16, 12, "query"),
              (4000, 16, 64, "list")]
K_EXH = 10


@functools.lru_cache(maxsize=None)
def _exact_graph(N, n):
    """(X fp32, exact fp64 squared distances ascending [N, K_EXH], their ids)."""
    X = _blobs(N, n, 7 + n, centres=12)
    X64 = torch.from_numpy(X).double()
    d2 = torch.cdist(X64, X64, compute_mode="donot_use_mm_for_euclid_dist") ** 2
    v, i = torch.topk(d2, K_EXH, dim=1, largest=False)
    return X, v.numpy(), i.numpy()


def _recall(idx, exact_ids):
    hit = (idx[:, :, None] == exact_ids[:, None, :]).any(2)
    return float(hit.mean())


def _exhaustive(X, dev, nlist, probe):
    d, i = build_knn_graph(torch.from_numpy(X).to(dev), K_EXH, "ivf", {"nlist": nlist, "nprobe": nlist, "probe": probe})
    return d.cpu().numpy().astype(np.float64), i.cpu().numpy()


@pytest.mark.parametrize("N,n,nlist,probe", EXHAUSTIVE)
def test_exhaustive_probe_fp32_ranking_band(dev, monkeypatch, N, n, nlist, probe):
    """nprobe = nlist scans every list, so only the ranking keys ||i||^2 - 2 q.i (fp32) stand
    between the graph and the exact one: two compared keys cancel to within
    2 (n + 2) 2^-23 max ||x||^2, and the j-th returned neighbour is at most that much farther than
    the j-th exact one."""
    monkeypatch.setattr(ops, "KNN_LISTS_F16", False)
    X, ex_d2, ex_i = _exact_graph(N, n)
    X64 = X.astype(np.float64)
    d, i = _exhaustive(X, dev, nlist, probe)
    assert (i >= 0).all()
    band = 2.0 * (n + 2) * 2.0 ** -23 * float((X64 ** 2).sum(1).max())
    print("exhaustive N=%d n=%d nlist=%d %s %s: fp32 ranking recall %.4f, band %.3g, largest excess %.3g"
          % (N, n, nlist, probe, dev.type, _recall(i, ex_i), band, float((d * d - ex_d2).max())))
    assert np.all(d * d <= ex_d2 + band)
    assert np.all(np.sort(_pair_d2(X64, i), axis=1) <= ex_d2 + band)
    _assert_rerank(d, np.sqrt(_pair_d2(X64, i)), n, "exhaustive N=%d n=%d %s %s" % (N, n, probe, dev.type))


@pytest.mark.gpu
@pytest.mark.parametrize("N,n,nlist,probe", [c for c in EXHAUSTIVE if c[1] % 4 == 0])
def test_exhaustive_probe_f16_recall(gpu_device, monkeypatch, N, n, nlist, probe):
    """The fp16 candidate keys round relative to centred norms, not to the distance: no band of
    the fp32 kind is derivable, so the path is held to the fp32 ranking's recall in the same run
    (the margin of test_knn_graph_ivf_f16_recall)."""
    X, ex_d2, ex_i = _exact_graph(N, n)
    Xt = torch.from_numpy(X).to(gpu_device)
    assert ops.KNN_LISTS_F16 and ops.knn_lists_f16_ok(Xt, K_EXH, Xt[:nlist].contiguous())
    _, i16 = _exhaustive(X, gpu_device, nlist, probe)
    monkeypatch.setattr(ops, "KNN_LISTS_F16", False)
    assert not ops.knn_lists_f16_ok(Xt, K_EXH, Xt[:nlist].contiguous())
    _, i32 = _exhaustive(X, gpu_device, nlist, probe)
    r16, r32 = _recall(i16, ex_i), _recall(i32, ex_i)
    print("exhaustive N=%d n=%d nlist=%d %s: recall f16 %.4f, fp32 %.4f" % (N, n, nlist, probe, r16, r32))
    assert r16 >= r32 - 0.005


# ------------------------------------------------------------------------------------------
# D. bucketing with centres outside the plane's range (device)
# ------------------------------------------------------------------------------------------
def _stray_centres(X, rows, rng):
    """256 centres drawn like the rows plus copies of ``rows`` of X with each copy's two
    largest-magnitude coordinates set to +-6: six times the range the plane of X is scaled for."""
    S = X[rows].copy()
    for r in range(S.shape[0]):
        j = np.argsort(-np.abs(S[r]))[:2]
        S[r, j] = np.where(S[r, j] >= 0, 6.0, -6.0)
    return np.concatenate([rng.uniform(-1.0, 1.0, (256, X.shape[1])).astype(np.float32), S]).astype(np.float32)


def _check_bucketing(X, C, F, what):
    k = C.shape[0]
    d = torch.cdist(torch.from_numpy(X).double(), torch.from_numpy(C).double(),
                    compute_mode="donot_use_mm_for_euclid_dist") ** 2
    stray = d.argmin(1) >= 256
    assert int(stray.sum()) >= 8
    assert F is not None
    dev = F.X.device
    lab = ops.nearest_list(F.X, torch.from_numpy(C).to(dev), F).cpu().long()
    assert lab.shape == (X.shape[0],) and bool((lab >= 0).all()) and bool((lab < k).all())
    got = d.gather(1, lab.view(-1, 1)).view(-1)
    excess = (got - d.min(1).values) / d.mean(1)
    print("%s: %d rows nearest to an out-of-range centre, %d of them mislabelled, largest excess %.3g"
          % (what, int(stray.sum()), int((lab != d.argmin(1))[stray].sum()), float(excess.max())))
    assert float(excess.max()) < 5e-3


@pytest.mark.gpu
@pytest.mark.parametrize("n", [116, 128])
def test_bucketing_centres_outside_plane_range(gpu_device, n):
    """The centre plane clamps |scale (c - mu)| >= 2^15; the row-loop arg-min must not rank by the
    clamped values (the criterion of test_nearest_f16_rowloop_matches_filter_argmin)."""
    rng = np.random.default_rng(0)
    X = rng.uniform(-1.0, 1.0, (512, n)).astype(np.float32)
    C = _stray_centres(X, np.arange(16), rng)
    assert C.shape == (272, n)
    _check_bucketing(X, C, ops.quantizer_planes(torch.from_numpy(X).to(gpu_device)), "bucketing n=%d" % n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [116, 128])
def test_bucketing_block_planes_global_centres(gpu_device, n):
    """knn_graph_ivf on rank 0 of 4: the planes (mean, scale) come from the rank's row block — the
    first quarter of rows sorted by coordinate 0 — the centres from the whole array."""
    rng = np.random.default_rng(1)
    X = rng.uniform(-1.0, 1.0, (2048, n)).astype(np.float32)
    X = X[np.argsort(X[:, 0], kind="stable")]
    Xb = np.ascontiguousarray(X[:512])
    C = _stray_centres(Xb, np.arange(16), rng)
    C[:256] = X[rng.choice(2048, 256, replace=False)]
    _check_bucketing(Xb, C, ops.quantizer_planes(torch.from_numpy(Xb).to(gpu_device)), "block bucketing n=%d" % n)


# ------------------------------------------------------------------------------------------
# E. a padded graph through the fuzzy-set kernels (device)
# ------------------------------------------------------------------------------------------
def _padded_graph(name, gpu_device):
    if name == "tiny_lists":
        X, k, kw = _edge_input("tiny_lists")
        dist, idx = _build(torch.from_numpy(X).to(gpu_device), k, "ivf_list", kw)
        return dist.cpu(), idx.cpu(), k
    X = _blobs(2000, 15, 8)
    X64 = torch.from_numpy(X).double()
    d2, idx = torch.topk(torch.cdist(X64, X64, compute_mode="donot_use_mm_for_euclid_dist") ** 2, 15, dim=1,
                         largest=False)
    dist = d2.sqrt().float()
    dist[::5, 6:] = dist[::5, 5:6]
    idx[::5, 6:] = -1
    dist[3, 1:] = dist[3, 0]
    idx[3, 1:] = -1
    return dist, idx, 15


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_lists", "synthetic"])
def test_padded_graph_through_fuzzy_set_kernels(gpu_device, name):
    dist, idx, k = _padded_graph(name, gpu_device)
    N = dist.shape[0]
    assert int((idx < 0).sum()) > 0
    sig_ref, rho_ref = U.smooth_knn_dist(dist, float(k))
    w_ref = U.membership_strengths(idx, dist, sig_ref, rho_ref, torch.arange(N))
    sig, rho, w = ops.umap_smooth_knn(dist.to(gpu_device), idx.to(gpu_device), float(k), self_rows=True)
    torch.testing.assert_close(rho.cpu(), rho_ref, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(sig.cpu(), sig_ref, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(w.cpu(), w_ref, rtol=1e-5, atol=1e-6)
    assert bool((w.cpu()[idx < 0] == 0).all())
    rows = torch.arange(N).view(-1, 1).expand_as(idx).reshape(-1)
    r_ref, c_ref, v_ref = U.fuzzy_union(rows, idx.reshape(-1).clamp_min(0), w_ref.reshape(-1), N)
    r, c, v = ops.umap_fuzzy_union_knn(idx.to(gpu_device), w_ref.to(gpu_device), 1.0)
    r, c, v = r.cpu(), c.cpu(), v.cpu()
    assert bool((r >= 0).all()) and bool((r < N).all()) and bool((c >= 0).all()) and bool((c < N).all())
    keep, keep_ref = v > 0, v_ref > 0
    kg = (r[keep] * N + c[keep]).numpy()
    kr = (r_ref[keep_ref] * N + c_ref[keep_ref]).numpy()
    order = np.argsort(kr)
    assert np.array_equal(kg, kr[order])
    np.testing.assert_allclose(v[keep].numpy(), v_ref[keep_ref].numpy()[order], rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------------------------------
# F. UMAP end to end at small k
# ------------------------------------------------------------------------------------------
def _umap_small_k():
    from spark_rapids_ml_nai_amd import DataFrame
    from spark_rapids_ml_nai_amd.umap import UMAP

    df = DataFrame.from_numpy(_blobs(1500, 16, 9))
    return UMAP(n_neighbors=5, build_algo="nn_descent", build_kwds={"nlist": 12, "nprobe": 4, "nnd_iters": 1},
                random_state=1).fit(df).embedding_


def test_umap_small_k_nn_descent_fits(dev):
    emb = _umap_small_k()
    assert emb.shape == (1500, 2) and np.isfinite(emb).all()


@pytest.mark.gpu
def test_umap_small_k_deterministic_repeats(gpu_device, monkeypatch):
    """test_umap_sync_gpu.py's guarantee (k = 15), at k = 5 below the NN-descent fan-out."""
    monkeypatch.delenv("SRML_FORCE_CPU", raising=False)
    monkeypatch.setenv("SRML_DETERMINISTIC", "1")
    e1, e2 = _umap_small_k(), _umap_small_k()
    assert np.isfinite(e1).all() and np.array_equal(e1, e2)
