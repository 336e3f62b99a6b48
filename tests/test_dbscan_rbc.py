"""DBSCAN ``algorithm="rbc"`` (csrc/dbscan_rbc.hip): the sweeps over a tile-pair list of permuted rows, the
tile balls, the surviving pair list and the model, against the fp64 oracle of ``dbscan_cases``. Every case
runs through ``ops.*`` on CPU tensors and, marked ``gpu``, on the device."""
import numpy as np
import pytest
import torch

import dbscan_cases as cases
from dbscan_cases import U, check_labels, check_sweeps, make_oracle
from spark_rapids_ml_nai_amd import DataFrame, ops
from spark_rapids_ml_nai_amd.clustering import DBSCAN
from spark_rapids_ml_nai_amd.models.dbscan import _prepare, _rbc_pairs


@pytest.fixture(params=["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def dev(request, monkeypatch):
    if request.param == "cpu":
        monkeypatch.setenv("SRML_FORCE_CPU", "1")
    return torch.device(request.param)


def _np(t):
    return t.detach().cpu().numpy()


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)


def _tri(a, b):
    return a * (a + 1) // 2 + b


def _list_sweeps(X, xn, eps2, ms, perm, pairs):
    """degree -> core -> link -> compress -> labels over ``pairs``, on the rows in ``perm`` order."""
    N = X.shape[0]
    Xp, xnp = X[perm.long()].contiguous(), xn[perm.long()].contiguous()
    counts = ops.dbscan_degree_list(Xp, xnp, eps2, pairs, 0, pairs.shape[0], perm)
    core = (counts >= ms).to(torch.uint8)
    parent = torch.arange(N, dtype=torch.int32, device=X.device)
    best = torch.full((N,), -1, dtype=torch.int64, device=X.device)
    ops.dbscan_link_list(Xp, xnp, eps2, pairs, 0, pairs.shape[0], perm, core, parent, best)
    ops.uf_compress(parent)
    return [_np(a) for a in (counts, parent, best, ops.dbscan_labels(parent, core, best))]


def _all_pairs(N, dev):
    return torch.arange(ops.dbscan_num_tiles(N), dtype=torch.int64, device=dev)


LATTICE = [(1, 3), (127, 2), (129, 4), (300, 5), (513, 33)]


@pytest.mark.parametrize("N,n", LATTICE)
def test_list_sweeps_lattice_under_a_permutation(dev, N, n):
    """Bit for bit the oracle's result in original ids: roots are the smallest original core index, border
    ties go to the lowest original index, whatever order the rows are swept in."""
    Xn, eps2, ms = cases.lattice_sweep_case(N, n)
    orc = make_oracle(Xn, eps2, ms, lattice=True)
    perm = _t(np.random.default_rng(N).permutation(N).astype(np.int32), dev)
    X = _t(Xn, dev)
    counts, parent, best, labels = _list_sweeps(X, ops.row_sqnorm(X), eps2, ms, perm, _all_pairs(N, dev))
    check_sweeps(orc, counts, parent, best)
    check_labels(orc, labels, chosen=best)
    for got, want in zip((counts, parent, best, labels), cases.oracle_result(orc)):
        assert np.array_equal(got, want)


_generic_cache = {}


def _generic(shift):
    if shift not in _generic_cache:
        Xn = cases.generic_case(cases.blobs(600, 8, 10, shift), 2.0)
        ms = int(np.median(make_oracle(Xn, 4.0, 1).deg))  # about half the rows are not core: many border keys
        _generic_cache[shift] = (Xn, make_oracle(Xn, 4.0, ms))
    return _generic_cache[shift]


@pytest.mark.parametrize("shift", [0.0, 4096.0])
def test_list_sweeps_generic_under_a_permutation(dev, shift):
    Xn, orc = _generic(shift)
    N = Xn.shape[0]
    X, xn, eps2 = _prepare(_t(Xn, dev), 2.0, "euclidean")
    perm = _t(np.random.default_rng(7).permutation(N).astype(np.int32), dev)
    counts, parent, best, labels = _list_sweeps(X, xn, eps2, orc.min_samples, perm, _all_pairs(N, dev))
    check_sweeps(orc, counts, parent, best, keys=True)
    check_labels(orc, labels)


# ---------------------------------------------------------------------------------- the pair list
def _boxes(centres, seed=3):
    """128 lattice rows inside a 10 x 10 box about each centre; the centres lie on a grid of pitch 300."""
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.integers(-5, 6, (128, 2)) + np.asarray(c) for c in centres]).astype(np.float32)
    cases.assert_lattice(X)
    return X


# no third box within 320 of box 0 or box 1: the two balls that a swapped row inflates to a radius of
# about 300 reach each other and nothing else
FIVE = [(-300, -300), (0, -300), (-300, 300), (0, 300), (300, 300)]


def _pairs_of(X, eps2):
    n = X.shape[1]
    band = cases.c_of_n(n) * U * 4.0 * float(ops.row_sqnorm(X).max())
    C, r, cn = ops.dbscan_tile_balls(X)
    return _np(ops.dbscan_tile_pairs(C, r, cn, eps2, band)), band


@pytest.mark.parametrize("swap", [False, True])
def test_pair_list_exact_on_separated_boxes(dev, swap):
    Xn = _boxes(FIVE)
    want = [_tri(a, a) for a in range(5)]
    if swap:
        Xn[[5, 128 + 7]] = Xn[[128 + 7, 5]]
        want = sorted(want + [_tri(1, 0)])
    pairs, band = _pairs_of(_t(Xn, dev), 25.0)
    # provable from the data: every pruned pair's centres are further apart than the rule's reach, with room for
    # the radii's inflation (2 n + 8) u and the centre distance's error e_ab
    T64 = Xn.astype(np.float64).reshape(5, 128, 2)
    c = T64.mean(1)
    r = np.sqrt(((T64 - c[:, None]) ** 2).sum(2)).max(1) * (1.0 + 12 * U)
    for a in range(5):
        for b in range(a):
            if _tri(a, b) not in want:
                e_ab = 8.0 * U * (np.linalg.norm(c[a]) + np.linalg.norm(c[b])) ** 2
                assert np.linalg.norm(c[a] - c[b]) ** 2 - 2.0 * e_ab > (r[a] + r[b] + np.sqrt(25.0 + band)) ** 2 + 1.0
    assert not swap or r[0] + r[1] > 300.0  # and the pair (1, 0) does hold neighbours: the swapped rows' own boxes
    assert pairs.tolist() == want


@pytest.mark.parametrize("case", ["generic"] + [c for c in LATTICE if c[0] > 128])
def test_pair_list_never_too_small(dev, case):
    """With the model's own row order, every tile pair that holds an oracle neighbour pair is listed."""
    if case == "generic":
        Xn, orc = _generic(0.0)
        X, xn, eps2 = _prepare(_t(Xn, dev), 2.0, "euclidean")
    else:
        Xn, eps2, ms = cases.lattice_sweep_case(*case)
        orc = make_oracle(Xn, eps2, ms, lattice=True)
        X = _t(Xn, dev)
        xn = ops.row_sqnorm(X)
    _, _, perm, pairs = _rbc_pairs(X, xn, eps2)
    perm = _np(perm).astype(np.int64)
    assert np.array_equal(np.sort(perm), np.arange(orc.N))
    pos = np.empty(orc.N, np.int64)
    pos[perm] = np.arange(orc.N)
    I, J = np.nonzero(orc.adj)
    ti, tj = pos[I] // cases.TILE, pos[J] // cases.TILE
    need = np.unique(_tri(np.maximum(ti, tj), np.minimum(ti, tj)))
    got = _np(pairs)
    assert (np.diff(got) > 0).all() and got[-1] < cases.num_tiles(orc.N)
    assert np.isin(need, got).all()


@pytest.mark.parametrize("n", [1, 3, 33])
@pytest.mark.parametrize("N", [1, 127, 128, 129, 300])
def test_tile_balls(dev, N, n):
    rng = np.random.default_rng(100 * N + n)
    Xn = (10.0 * rng.standard_normal((N, n)) + rng.uniform(-50, 50, n)).astype(np.float32)
    C, r, cn = (_np(a).astype(np.float64) for a in ops.dbscan_tile_balls(_t(Xn, dev)))
    T = (N + cases.TILE - 1) // cases.TILE
    assert C.shape == (T, n) and r.shape == cn.shape == (T,)
    for t in range(T):
        rows = Xn[t * cases.TILE: (t + 1) * cases.TILE].astype(np.float64)
        far = np.sqrt(((rows - C[t]) ** 2).sum(1)).max()
        assert far <= r[t] <= (1.0 + (2 * n + 8) * U) * far
        # the centre is the fp32 column mean (<= 128 roundings of a sum, one of the division), cnorm its fp32 norm
        assert np.abs(C[t] - rows.mean(0)).max() <= 129 * U * np.abs(rows).max()
        assert abs(cn[t] - (C[t] ** 2).sum()) <= (n + 8) * U * (C[t] ** 2).sum()


# ------------------------------------------------------------------------------------------ the model
def _fit(Xn, eps, ms, algorithm, workers=1, metric="euclidean"):
    df = DataFrame.from_numpy(np.array(Xn), num_partitions=workers)
    model = DBSCAN(eps=eps, min_samples=ms, algorithm=algorithm, metric=metric, num_workers=workers).fit(df)
    return model.transform(df).to_numpy("prediction"), model.core_sample_indices_, model._tile_pairs_


def _interleaved_boxes():
    """Eight boxes of 128 rows, four and their mirror images: the column means are exactly 0, so the model's
    centred rows are the rows and the lattice contract holds for it. Row j comes from box (j + j // 128) % 8: every
    run of eight rows visits every box, and the eight landmarks (rows 0, 128, ..) fall one into each box, the
    regime the ordering is made for (real data has many landmarks per cluster). Every landmark group is then one
    box and a tile of the ordered rows is one box: no shuffle seed is chosen."""
    P = _boxes([(150, 150), (450, 150), (150, 450), (450, 450)])
    Xn = np.concatenate([P, -P])
    assert not Xn.astype(np.float64).mean(0).any()
    j = np.arange(1024)
    out = np.empty_like(Xn)
    out[np.argsort((j + j // 128) % 8, kind="stable")] = Xn
    return out


def _cosine_rows():
    """Four directions in 12 columns, norms spread over 1e-3 .. 1e3, three all-zero rows."""
    rng = np.random.default_rng(6)
    X = rng.standard_normal((4, 12))[rng.integers(0, 4, 400)] + 0.35 * rng.standard_normal((400, 12))
    X = (X * 10.0 ** rng.uniform(-3, 3, (400, 1))).astype(np.float32)
    X[[5, 140, 399]] = 0.0
    return cases.generic_case(X, 0.6, "cosine")


@pytest.mark.parametrize("name", ["boxes", "blobs", "cosine"])
def test_model_rbc_equals_brute(dev, name):
    """Identical, not close: a pair's distance depends on its two rows only (the k order of the MFMA does
    not depend on the tile position, the products and rn + cn commute), counts are integers, roots and keys
    are minima, and no pair the brute sweep could count is pruned."""
    metric = "euclidean"
    if name == "boxes":
        Xn, eps, ms = _interleaved_boxes(), 5.0, 5
        orc = make_oracle(Xn, 25.0, ms, lattice=True)
    elif name == "blobs":
        (Xn, _), eps, ms = _generic(0.0), 2.0, 5
        orc = make_oracle(Xn, 4.0, ms)
    else:
        Xn, eps, ms, metric = _cosine_rows(), 0.6, 5, "cosine"
        orc = make_oracle(Xn, 1.2, ms, "cosine")
        assert orc.N > 2 * cases.TILE and (~Xn.any(1)).sum() == 3
    lab_b, core_b, tp_b = _fit(Xn, eps, ms, "brute", metric=metric)
    lab_r, core_r, tp_r = _fit(Xn, eps, ms, "rbc", metric=metric)
    assert np.array_equal(lab_r, lab_b) and np.array_equal(core_r, core_b)
    check_labels(orc, lab_r, core_idx=core_r)
    total = cases.num_tiles(orc.N)
    assert tp_b == (total, total) and tp_r[1] == total and 0 < tp_r[0] <= total
    if name == "boxes":
        assert tp_r[0] <= total // 2, tp_r


@pytest.mark.dist
def test_model_rbc_two_ranks(monkeypatch):
    monkeypatch.setenv("SRML_FORCE_CPU", "1")
    Xn = _interleaved_boxes()
    a = _fit(Xn, 5.0, 5, "rbc", 1)
    b = _fit(Xn, 5.0, 5, "rbc", 2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
