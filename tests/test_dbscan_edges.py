"""DBSCAN sweeps (``ops.dbscan_degree`` / ``dbscan_link``: csrc/dbscan.hip), the union-find and label
kernels and the model at the tile, k-tile, eps, union-find, scan-chunk and grid-cap edges, against the
fp64 oracle of ``dbscan_cases``: bit for bit on lattice cases, and on generic cases with every pair
decided by a derived band (contract and derivation there). No comparison uses a fraction of rows.
Inputs are finite; NaN / inf rows are out of scope.

Every case runs through ``ops.*`` on CPU tensors (the fall-back evaluates the same formula) and,
marked ``gpu``, on the device; the checker's own tests are CPU only."""
import itertools

import numpy as np
import pytest
import torch

import dbscan_cases as cases
from dbscan_cases import check_labels, check_sweeps, make_oracle
from spark_rapids_ml_nai_amd import DataFrame, ops
from spark_rapids_ml_nai_amd.clustering import DBSCAN
from spark_rapids_ml_nai_amd.models.dbscan import _prepare


@pytest.fixture(params=["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def dev(request, monkeypatch):
    if request.param == "cpu":
        monkeypatch.setenv("SRML_FORCE_CPU", "1")
    return torch.device(request.param)


def _np(t):
    return t.detach().cpu().numpy()


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)


def _fresh(N, dev):
    return (torch.arange(N, dtype=torch.int32, device=dev), torch.full((N,), -1, dtype=torch.int64, device=dev))


def _sweeps(X, xn, eps2, ms, ranges=None):
    """degree -> core -> link -> compress -> labels over the tile ranges (default: [0, T) at once)."""
    N = X.shape[0]
    ranges = ranges or [(0, ops.dbscan_num_tiles(N))]
    counts = torch.zeros(N, dtype=torch.int32, device=X.device)
    for t0, t1 in ranges:
        ops.dbscan_degree(X, xn, eps2, t0, t1, counts)
    core = (counts >= ms).to(torch.uint8)
    parent, best = _fresh(N, X.device)
    for t0, t1 in ranges:
        ops.dbscan_link(X, xn, eps2, t0, t1, core, parent, best)
    ops.uf_compress(parent)
    labels = ops.dbscan_labels(parent, core, best)
    return counts, core, parent, best, labels


def _run_lattice(Xn, eps2, ms, dev, orc=None, ranges=None):
    orc = orc or make_oracle(Xn, eps2, ms, lattice=True)
    X = _t(Xn, dev)
    out = _sweeps(X, ops.row_sqnorm(X), eps2, ms, ranges)
    counts, _, parent, best, labels = (_np(a) for a in out)
    check_sweeps(orc, counts, parent, best)
    check_labels(orc, labels, chosen=best)
    return orc, out


def test_constants():
    assert cases.TILE == ops.DB_TILE
    assert cases.num_tiles(385) == ops.dbscan_num_tiles(385) == 10
    assert ops.dbscan_num_tiles(128 * 128 + 1) == 8385 > cases.GRID_CAP


# ================================================================================= sweeps, lattice
_NS = (1, 2, 127, 128, 129, 255, 256, 257, 385)
_DIMS = (1, 2, 3, 4, 5, 31, 32, 33, 64, 65)
# every N at n = 4 (VEC, one partial k-tile) and 33 (one column into the second k-tile); every n at
# N = 129 and 257 (one row into the second / third tile)
SWEEP_SHAPES = sorted({(N, n) for N in _NS for n in (4, 33)} | {(N, n) for N in (129, 257) for n in _DIMS})


@pytest.mark.parametrize("N,n", SWEEP_SHAPES)
def test_sweeps_lattice(dev, N, n):
    Xn, eps2, ms = cases.lattice_sweep_case(N, n)
    orc, out = _run_lattice(Xn, eps2, ms, dev)
    if n % 4 == 0:
        # the same rows at a base pointer that is not 16-byte aligned: the non-VEC kernels
        buf = torch.empty(N * n + 1, dtype=torch.float32, device=dev)
        X = buf[1:].view(N, n)
        X.copy_(_t(Xn, dev))
        assert X.is_contiguous() and X.data_ptr() % 16 == 4
        out2 = _sweeps(X, ops.row_sqnorm(_t(Xn, dev)), eps2, ms)
        for a, b in zip(out, out2):
            assert torch.equal(a, b)


# ===================================================================================== tile ranges
def _split(T, k):
    b = np.linspace(0, T, k + 1).astype(int)
    return [(int(b[i]), int(b[i + 1])) for i in range(k)]


@pytest.mark.parametrize("N,n", [(385, 5), (700, 3)])
def test_tile_ranges(dev, N, n):
    """One call, single tiles in shuffled order into the same buffers, and two / three ranges with
    their own forests merged in both orders: bit-identical after ``uf_compress``."""
    Xn, eps2, ms = cases.lattice_sweep_case(N, n, seed=1)
    T = ops.dbscan_num_tiles(N)
    assert T == cases.num_tiles(N) and (N != 385 or T == 10)
    orc, (counts, core, parent, best, _) = _run_lattice(Xn, eps2, ms, dev)
    X = _t(Xn, dev)
    xn = ops.row_sqnorm(X)
    order = np.random.default_rng(N).permutation(T)
    out = _sweeps(X, xn, eps2, ms, [(int(t), int(t) + 1) for t in order])
    for a, b in zip((counts, core, parent, best), out):
        assert torch.equal(a, b)
    for k in (2, 3):
        forests = []
        for t0, t1 in _split(T, k):
            p, b = _fresh(N, dev)
            ops.dbscan_link(X, xn, eps2, t0, t1, core, p, b)
            forests.append((p, b))
        for perm in (list(range(k)), list(range(k))[::-1]):
            p = forests[perm[0]][0].clone()
            b = forests[perm[0]][1].clone()
            for r in perm[1:]:
                ops.uf_unite_pairs(p, forests[r][0])
                b = torch.minimum(b, forests[r][1])
            ops.uf_compress(p)
            assert torch.equal(p, parent) and torch.equal(b, best)
    # an empty range leaves the buffers untouched
    c2, p2, b2 = counts.clone(), parent.clone(), best.clone()
    for t in (0, 3, T):
        ops.dbscan_degree(X, xn, eps2, t, t, c2)
        ops.dbscan_link(X, xn, eps2, t, t, core, p2, b2)
    assert torch.equal(c2, counts) and torch.equal(p2, parent) and torch.equal(b2, best)


# ====================================================================================== duplicates
@pytest.mark.parametrize("ms,kind", [(300, "one"), (301, "noise"), (1, "one")])
def test_duplicate_rows(dev, ms, kind):
    Xn = np.tile(np.array([[3, -2, 7, 0, -5]], np.float32), (300, 1))
    orc, out = _run_lattice(Xn, 25.0, ms, dev)
    labels = _np(out[4])
    assert (orc.deg == 300).all() and orc.core.all() == (kind == "one")
    assert (labels == (0 if kind == "one" else -1)).all()


def test_isolated_points_number_in_index_order(dev):
    rng = np.random.default_rng(5)
    P = np.stack(np.meshgrid(np.arange(15), np.arange(14)), -1).reshape(-1, 2)[:200] * 10 - 70
    Xn = np.concatenate([P[rng.permutation(200)], np.zeros((200, 1), int)], 1).astype(np.float32)
    orc, out = _run_lattice(Xn, 25.0, 1, dev)
    assert (orc.deg == 1).all()
    assert np.array_equal(_np(out[4]), np.arange(200))


# ====================================================================================== union-find
def _chain(cuts=()):
    """1000 integer positions on a line, one apart, two apart after the indices in ``cuts``."""
    x = np.arange(1000) + np.searchsorted(np.asarray(cuts, int), np.arange(1000), "left")
    return (x - 500).astype(np.float32).reshape(-1, 1)


def test_uf_chain_spans_every_tile(dev):
    Xn = _chain()[np.random.default_rng(0).permutation(1000)]
    Xn[[0, int(np.argmin(Xn[:, 0]))]] = Xn[[int(np.argmin(Xn[:, 0])), 0]]  # an end of the chain at row 0
    orc = make_oracle(Xn, 1.0, 2, lattice=True)
    assert np.sort(orc.deg).tolist() == [2, 2] + [3] * 998 and orc.core.all() and (orc.root == 0).all()
    _run_lattice(Xn, 1.0, 2, dev, orc)
    orc1 = cases.make_oracle_1d(Xn, 1, 2)  # the sorting oracle of the grid-cap case agrees with the dense one
    for f in ("deg", "core", "root", "has_core_nb", "dmin_core", "nearest"):
        assert np.array_equal(getattr(orc, f), getattr(orc1, f)), f


def test_uf_chain_cut_into_seven(dev):
    Xn = _chain(cuts=(100, 250, 400, 520, 640, 900))[np.random.default_rng(1).permutation(1000)]
    orc = make_oracle(Xn, 1.0, 2, lattice=True)
    assert np.unique(orc.root[orc.core]).size == 7 and orc.core.all()
    orc, out = _run_lattice(Xn, 1.0, 2, dev, orc)
    assert _np(out[4]).max() == 6
    orc1 = cases.make_oracle_1d(Xn, 1, 2)
    assert np.array_equal(orc.root, orc1.root) and np.array_equal(orc.deg, orc1.deg)


def test_uf_interleaved_chains_do_not_merge(dev):
    """Chain A at (5 i, 0), chain B at (5 i + 1, 5): links of exactly eps^2 = 25 inside a chain, the
    closest A-B pairs at 26. Rows alternate A, B, then are permuted."""
    i = np.arange(300)
    A = np.stack([5 * i - 750, 0 * i], 1)
    B = np.stack([5 * i - 749, 0 * i + 5], 1)
    Xn = np.stack([A, B], 1).reshape(-1, 2)[np.random.default_rng(2).permutation(600)].astype(np.float32)
    D = cases.sqdist64(Xn)
    assert (D == 26.0).sum() == 600 and (D == 25.0).sum() == 2 * 2 * 299
    orc = make_oracle(Xn, 25.0, 2, lattice=True)
    assert orc.core.all() and np.unique(orc.root).size == 2
    _run_lattice(Xn, 25.0, 2, dev, orc)


def test_uf_many_roots(dev):
    """1500 two-point components (a 3-4-5 pair each) on a grid of pitch 10, rows permuted."""
    k = np.arange(1500)
    a = np.stack([10 * (k % 40) - 200, 10 * (k // 40) - 190], 1)
    Xn = np.concatenate([a, a + (3, 4)])[np.random.default_rng(3).permutation(3000)].astype(np.float32)
    orc = make_oracle(Xn, 25.0, 2, lattice=True)
    assert (orc.deg == 2).all() and np.unique(orc.root).size == 1500
    orc, out = _run_lattice(Xn, 25.0, 2, dev, orc)
    assert _np(out[4]).max() == 1499


def test_uf_root_in_last_and_first_tile_row(dev):
    """N = 300 (tile rows 0-127, 128-255, 256-299). Component A lives in the last tile row only
    (rows 270-289); component B has its smallest index in the first (row 5) and its other rows in
    the later two, so the root is reached only through off-diagonal tiles."""
    items = [(270 + k, (k, 0)) for k in range(20)]
    rows_b = [5] + list(range(140, 150)) + list(range(257, 266))
    items += [(r, (k, 40)) for k, r in enumerate(rows_b)]
    Xn = cases.place(300, items)
    orc = make_oracle(Xn, 25.0, 6, lattice=True)
    assert orc.core.sum() == 40 and set(orc.root[orc.core]) == {5, 270}
    assert (orc.root[270:290] == 270).all() and (orc.root[rows_b] == 5).all()
    _run_lattice(Xn, 25.0, 6, dev, orc)


# ==================================================================================== border paths
def _line(rows, y, x0=0):
    return [(r, (x0 + k, y)) for k, r in enumerate(rows)]


def test_border_exact_tie_between_two_clusters(dev):
    """Cores on x = 0..9 and x = 15..24 (min_samples 6, eps 5); the border at (12, 4) is at exactly 25
    from (9, 0) and from (15, 0), which are 36 apart. The lower index wins, whichever cluster holds it."""
    for lo_first in (True, False):
        a, b = (range(10, 20), range(30, 40)) if lo_first else (range(30, 40), range(10, 20))
        Xn = cases.place(200, _line(a, 0) + _line(b, 0, 15) + [(150, (12, 4))])
        orc = make_oracle(Xn, 25.0, 6, lattice=True)
        e9, e15 = list(a)[9], list(b)[0]
        assert orc.core.sum() == 20 and not orc.core[150] and orc.deg[150] == 3 and orc.dmin_core[150] == 25.0
        assert orc.nearest[150] == min(e9, e15) and orc.root[e9] != orc.root[e15]
        orc, out = _run_lattice(Xn, 25.0, 6, dev, orc)
        assert _np(out[3])[150] & 0xFFFFFFFF == min(e9, e15)
        # the winner is the left line's end in the first layout, the right line's in the second
        assert Xn[min(e9, e15), 0] == (9 if lo_first else 15)
        assert _np(out[4])[150] == orc.cluster_ids()[min(e9, e15)] == 0


def test_border_routes(dev):
    """The three ways a border key is written, chosen by index: ``rb`` (the border's tile row comes
    after the core's: it is a row of an off-diagonal tile), ``cbest`` (the border's tile comes first:
    it is a column) and a diagonal tile (both). Each border sees one core, at exactly eps^2."""
    items = _line(range(0, 10), 0) + [(200, (12, 4))]          # cores in tile 0, border in tile 1: row
    items += _line(range(260, 270), 40) + [(20, (12, 44))]     # cores in tile 2, border in tile 0: column
    items += _line(range(130, 140), 80) + [(150, (12, 84))]    # all in tile 1: diagonal
    Xn = cases.place(300, items)
    orc = make_oracle(Xn, 25.0, 6, lattice=True)
    T = cases.TILE
    assert np.nonzero(orc.has_core_nb)[0].tolist() == [20, 150, 200]
    assert orc.nearest[[20, 150, 200]].tolist() == [269, 139, 9]
    assert 200 // T > 9 // T and 20 // T < 269 // T and 150 // T == 139 // T
    orc, out = _run_lattice(Xn, 25.0, 6, dev, orc)
    assert _np(out[4])[[200, 150, 20]].tolist() == [0, 1, 2]


def test_border_nearest_core_in_another_tile_pair(dev):
    """The border (10, 3) in tile 1 sees the cores at x = 9 (D 10, tile 0) and x = 8, 7, 6 (D 13, 18,
    25, tile 2): the keys of two tile pairs meet in one atomicMin, in either order."""
    rows = [260, 261, 262, 263, 264, 265, 266, 267, 268, 3]
    Xn = cases.place(300, _line(rows, 0) + [(140, (10, 3))])
    orc = make_oracle(Xn, 25.0, 6, lattice=True)
    assert orc.deg[140] == 5 and orc.nearest[140] == 3 and orc.dmin_core[140] == 10.0 and orc.core.sum() == 10
    _run_lattice(Xn, 25.0, 6, dev, orc)
    Xn = cases.place(300, _line(rows[::-1], 0) + [(140, (10, 3))])  # the nearest in tile 2, the farthest in tile 0
    orc = make_oracle(Xn, 25.0, 6, lattice=True)
    assert orc.nearest[140] == 260
    _run_lattice(Xn, 25.0, 6, dev, orc)


def test_noncore_point_with_only_noncore_neighbours(dev):
    """Three points within eps of each other, min_samples 4: each has neighbours, none is core."""
    Xn = cases.place(150, [(10, (0, 0)), (140, (3, 4)), (141, (0, 5))])
    orc = make_oracle(Xn, 25.0, 4, lattice=True)
    assert orc.deg[[10, 140, 141]].tolist() == [3, 3, 3] and not orc.core.any() and orc.noise.all()
    orc, out = _run_lattice(Xn, 25.0, 4, dev, orc)
    assert (_np(out[3]) == -1).all() and (_np(out[4]) == -1).all()


# ======================================================================================== grid cap
@pytest.mark.gpu
def test_grid_cap_second_tile_per_block(gpu_device):
    """The grid is a property of the device launch, so this case has no CPU twin. N = 128 * 128 + 1 rows
    on a line: 8385 tile pairs > the 8192-block grid cap, so 193 blocks run a second tile. About ten
    rows share each occupied integer site of [-2000, 2000] (eps 1), at random indices, so every tile pair
    holds neighbours. The oracle is computed by sorting (``make_oracle_1d``), not from an N x N matrix."""
    dev = gpu_device
    N = cases.TILE * cases.TILE + 1
    assert ops.dbscan_num_tiles(N) > cases.GRID_CAP
    rng = np.random.default_rng(7)
    sites = np.nonzero(rng.random(4001) < 0.4)[0] - 2000
    Xn = sites[rng.integers(0, sites.size, N)].astype(np.float32).reshape(-1, 1)
    deg = cases.make_oracle_1d(Xn, 1, 1).deg
    ms = int(np.median(deg))
    orc = cases.make_oracle_1d(Xn, 1, ms)
    assert 0.2 < orc.core.mean() < 0.8 and orc.has_core_nb.sum() > 100 and orc.noise.sum() > 100
    _run_lattice(Xn, 1.0, ms, dev, orc)


# ======================================================================= labels on synthetic forests
def _forest(N, seed, p_core=0.5, p_root=0.3):
    rng = np.random.default_rng(seed)
    core = rng.random(N) < p_core
    is_root = core & (rng.random(N) < p_root)
    cidx = np.nonzero(core)[0]
    if cidx.size:
        is_root[cidx[0]] = True
    idx = np.arange(N)
    last_root = np.maximum.accumulate(np.where(is_root, idx, -1))
    parent = np.where(core, last_root, idx)
    best = np.full(N, -1, np.int64)
    if cidx.size:
        nb = np.nonzero(~core & (rng.random(N) < 0.5))[0]
        best[nb] = cases.pack_key(rng.random(nb.size), cidx[rng.integers(0, cidx.size, nb.size)])
    return parent.astype(np.int32), core, best


def _labels_ref(parent, core, best):
    roots = np.unique(parent[core])
    tgt = np.where(core, parent, np.where(best != -1, parent[np.clip(best & 0xFFFFFFFF, 0, parent.size - 1)], -1))
    return np.where(tgt >= 0, np.searchsorted(roots, tgt), -1)


def _check_labels_op(parent, core, best, dev):
    lab = ops.dbscan_labels(_t(parent, dev), _t(core.astype(np.uint8), dev), _t(best, dev))
    assert lab.dtype == torch.int64
    assert np.array_equal(_np(lab), _labels_ref(parent, core, best))


@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 1024 * 1024 + 1025])
def test_labels_scan_blocks(dev, N):
    """N around the 1024-element scan block; 1024 * 1024 + 1025 needs 1026 block totals, i.e. the second
    chunk of the single-block scan over them."""
    assert cases.LABEL_BLOCK == 1024
    parent, core, best = _forest(N, N)
    assert N < 1024 or (core & (parent == np.arange(N)))[-1000:].any()
    _check_labels_op(parent, core, best, dev)


def test_labels_corner_forests(dev):
    N = 2500
    idx = np.arange(N, dtype=np.int32)
    none = np.full(N, -1, np.int64)
    _check_labels_op(idx, np.zeros(N, bool), none, dev)  # no core point at all
    _check_labels_op(idx, np.ones(N, bool), none, dev)   # every point its own root
    core = np.zeros(N, bool)
    core[[0, N - 1]] = True                             # borders pointing at index 0 and at N - 1
    best = none.copy()
    best[1:N - 1:2] = cases.pack_key(np.ones(len(best[1:N - 1:2])), 0)
    best[2:N - 1:2] = cases.pack_key(np.ones(len(best[2:N - 1:2])), N - 1)
    _check_labels_op(idx, core, best, dev)
    ref = _labels_ref(idx, core, best)
    assert ref[1] == 0 and ref[2] == 1 and ref[0] == 0 and ref[N - 1] == 1


# ================================================================================== uf_unite_pairs
def _component_minima(N, edges):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    s = np.concatenate([e[0] for e in edges])
    d = np.concatenate([e[1] for e in edges])
    _, comp = connected_components(coo_matrix((np.ones(s.size, np.int8), (s, d)), shape=(N, N)), directed=False)
    mins = np.full(comp.max() + 1, N)
    np.minimum.at(mins, comp, np.arange(N))
    return mins[comp]


def test_unite_path_forest(dev):
    N = 20000
    other = np.maximum(np.arange(N) - 1, 0).astype(np.int32)
    p = torch.arange(N, dtype=torch.int32, device=dev)
    ops.uf_unite_pairs(p, _t(other, dev))
    ops.uf_compress(p)
    assert not _np(p).any()


def test_unite_three_forests_in_every_order(dev):
    N = 5000
    rng = np.random.default_rng(11)
    idx = np.arange(N)
    forests = []
    for _ in range(3):  # parents point to smaller indices; a third of the nodes are hooked
        o = np.where(rng.random(N) < 0.33, (rng.random(N) * (idx + 1)).astype(int), idx)
        forests.append(np.minimum(o, idx).astype(np.int32))
    ref = _component_minima(N, [(idx, f.astype(np.int64)) for f in forests])
    assert 10 < np.unique(ref).size < N // 2
    for perm in itertools.permutations(range(3)):
        p = _t(forests[perm[0]], dev)
        for r in perm[1:]:
            ops.uf_unite_pairs(p, _t(forests[r], dev))
        ops.uf_compress(p)
        assert np.array_equal(_np(p), ref), perm


# ===================================================================== generic cases, sweeps and model
GENERIC = {  # name: (rows, n, centres, shift, eps, std of a blob)
    "blobs8": (600, 8, 6, 0.0, 2.0, 1.0),
    "blobs8_4096": (600, 8, 6, 4096.0, 2.0, 1.0),
    "blobs8_65536": (600, 8, 6, 65536.0, 2.0, 1.0),
    "blobs33_4096": (700, 33, 6, 4096.0, 4.0, 1.0),  # every row isolated at eps 4: no neighbour may appear
    # tighter blobs, eps near the typical distance inside one: median degree 57 (n = 8) and 4 (n = 33)
    "tight8": (600, 8, 6, 0.0, 2.0, 0.5),
    "tight8_4096": (600, 8, 6, 4096.0, 2.0, 0.5),
    "tight8_65536": (600, 8, 6, 65536.0, 2.0, 0.5),
    "tight33_4096": (700, 33, 12, 4096.0, 4.0, 0.6),
}
TIGHT = [k for k in GENERIC if k.startswith("tight")]
_generic_cache = {}


def _generic(name):
    if name not in _generic_cache:
        N, n, k, shift, eps, std = GENERIC[name]
        X = cases.generic_case(cases.blobs(N, n, k, shift, seed=0, std=std), eps)
        X.setflags(write=False)
        _generic_cache[name] = (X, eps)
    return _generic_cache[name]


@pytest.mark.parametrize("name", TIGHT)
def test_generic_sweeps_on_prepared_rows(dev, name):
    """The model's preparation (``_prepare``: rows about their column mean) and the sweeps, against the
    oracle on the raw rows. min_samples is the median degree, so about half the rows are not core and
    the border keys are many; the fp32 distance in each key is held to the band."""
    Xn, eps = _generic(name)
    ms = int(np.median(make_oracle(Xn, eps * eps, 1).deg))
    orc = make_oracle(Xn, eps * eps, ms)
    assert ms >= 4 and (orc.deg == ms).any()
    X, xn, eps2 = _prepare(_t(Xn, dev), eps, "euclidean")
    counts, _, parent, best, labels = (_np(a) for a in _sweeps(X, xn, eps2, ms))
    r = check_sweeps(orc, counts, parent, best, keys=True)
    check_labels(orc, labels)
    assert r["borders"] > 20
    print("dbscan key error / band %s %s: %.3f over %d borders" % (dev.type, name, r["key_ratio"], r["borders"]))


def _fit(Xn, eps, ms, metric, parts):
    df = DataFrame.from_numpy(np.array(Xn), num_partitions=parts)
    model = DBSCAN(eps=eps, min_samples=ms, metric=metric).fit(df)
    lab = model.transform(df).to_numpy("prediction")
    return lab, model.core_sample_indices_


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("name", list(GENERIC))
def test_model_generic(dev, name, parts):
    """Far from the origin the clustering is the one at the origin (fails on raw rows: at shift 4096 the
    fp32 expanded form decides hundreds of pairs by rounding noise)."""
    Xn, eps = _generic(name)
    orc = make_oracle(Xn, eps * eps, 5)
    lab, core_idx = _fit(Xn, eps, 5, "euclidean", parts)
    check_labels(orc, lab, core_idx=core_idx)


def _small_eps_case():
    rng = np.random.default_rng(4)
    X = (30.0 * rng.standard_normal((400, 16))).astype(np.float32)
    X[[77, 333]] = X[[12, 200]]  # two duplicated rows
    return X


@pytest.mark.parametrize("ms", [1, 3])
def test_model_small_eps_self_neighbour(dev, ms):
    """400 x 16 rows of norm ~ 120 at eps 1e-3: every row is its own and only neighbour. The
    expanded form of D(i, i) is rounding noise of the order of 1e-5 * 120^2 >> eps^2, so the self pair
    is a neighbour by rule, not by arithmetic. The band (~ 0.1) cannot tell a duplicate (D = 0) from
    eps^2 = 1e-6 either, so the builder drops one row of each of the two duplicated pairs, as it must."""
    Xn = cases.generic_case(_small_eps_case(), 1e-3)
    assert Xn.shape[0] == 398
    orc = make_oracle(Xn, 1e-6, ms)
    assert (orc.deg == 1).all()
    for parts in (1, 3):
        lab, core_idx = _fit(Xn, 1e-3, ms, "euclidean", parts)
        check_labels(orc, lab, core_idx=core_idx)
        assert np.array_equal(lab, np.arange(398) if ms == 1 else np.full(398, -1))


def test_sweeps_self_neighbour_on_raw_rows(dev):
    """The same rows straight into the sweeps (no centring): every degree is exactly 1."""
    Xn = cases.generic_case(_small_eps_case(), 1e-3)
    X = _t(Xn, dev)
    for eps in (1e-3, 0.0):
        counts = ops.dbscan_degree(X, ops.row_sqnorm(X), eps * eps, 0, ops.dbscan_num_tiles(X.shape[0]))
        assert (_np(counts) == 1).all()


def test_model_eps_zero_with_duplicates(dev):
    """eps = 0: the neighbours of a row are its bit-identical copies. Integer rows in +- pairs, so the
    column mean is exactly 0 and the centred rows are the rows: the lattice contract holds for the
    model."""
    rng = np.random.default_rng(9)
    base = rng.integers(-20, 21, (40, 6))
    base = base[np.unique(base, axis=0, return_index=True)[1]]
    rows = np.concatenate([np.repeat(base[:10], 3, 0), base[10:]])  # ten rows three times, the rest once
    Xn = np.concatenate([rows, -rows])
    Xn = Xn[rng.permutation(Xn.shape[0])].astype(np.float32)
    assert not Xn.astype(np.float64).mean(0).any()
    for ms in (1, 3):
        orc = make_oracle(Xn, 0.0, ms, lattice=True)
        assert sorted(np.unique(orc.deg)) == [1, 3] and (orc.deg == 3).sum() == 60
        for parts in (1, 3):
            lab, core_idx = _fit(Xn, 0.0, ms, "euclidean", parts)
            check_labels(orc, lab, core_idx=core_idx)
            assert (lab >= 0).sum() == (Xn.shape[0] if ms == 1 else 60)


def _cosine_rows(zero_rows):
    rng = np.random.default_rng(6)
    C = rng.standard_normal((4, 12))
    X = C[rng.integers(0, 4, 300)] + 0.35 * rng.standard_normal((300, 12))
    X *= 10.0 ** rng.uniform(-3, 3, (300, 1))  # norms spread over 1e-3 .. 1e3
    X = X.astype(np.float32)
    if zero_rows:
        X[[5, 140, 299]] = 0.0
    return X


@pytest.mark.parametrize("eps,zero_rows", [(0.2, False), (0.6, True), (0.4, True)])
def test_model_cosine(dev, eps, zero_rows):
    """sklearn's contract: cosine distance on the rows' directions whatever their norms; an all-zero
    row is at distance 1 from every row but itself, so below eps = 1 it is noise (min_samples 5)."""
    Xn = cases.generic_case(_cosine_rows(zero_rows), eps, "cosine")
    orc = make_oracle(Xn, 2.0 * eps, 5, "cosine")
    zero = np.nonzero(~Xn.any(1))[0]
    assert zero.size == (3 if zero_rows else 0) and (orc.deg[zero] == 1).all() and orc.noise[zero].all()
    assert orc.core.sum() > 100
    for parts in (1, 3):
        lab, core_idx = _fit(Xn, eps, 5, "cosine", parts)
        check_labels(orc, lab, core_idx=core_idx)
    X, xn, eps2 = _prepare(_t(Xn, dev), eps, "cosine")
    ms = int(np.median(orc.deg))
    orc = make_oracle(Xn, 2.0 * eps, ms, "cosine")
    counts, _, parent, best, labels = (_np(a) for a in _sweeps(X, xn, eps2, ms))
    r = check_sweeps(orc, counts, parent, best, keys=True)
    check_labels(orc, labels)
    print("dbscan key error / band %s cosine eps %.1f: %.3f over %d borders" % (
        dev.type, eps, r["key_ratio"], r["borders"]))


# =============================================================================== the checker itself
def _checker_case():
    Xn, eps2, ms = cases.lattice_sweep_case(385, 2, seed=1)
    orc = make_oracle(Xn, eps2, ms, lattice=True)
    assert orc.noise.any() and orc.has_core_nb.sum() > 5 and np.unique(orc.root[orc.core]).size >= 2
    return orc, cases.oracle_result(orc), cases.sqdist64(Xn)


def test_checker_accepts_the_oracle_result():
    orc, (counts, parent, best, labels), _ = _checker_case()
    check_sweeps(orc, counts, parent, best)
    check_labels(orc, labels, chosen=best, core_idx=np.nonzero(orc.core)[0])


def test_checker_rejects_injected_faults():
    orc, (counts, parent, best, labels), D = _checker_case()
    T = cases.TILE
    adj = orc.adj.astype(np.int64)

    def sweeps_fail(c=counts, p=parent, b=best):
        with pytest.raises(AssertionError):
            check_sweeps(orc, c, p, b)

    def labels_fail(lab):
        with pytest.raises(AssertionError):
            check_labels(orc, lab, chosen=best)

    # one tile pair skipped: rows 256.., columns 128..255, and the columns' half with it
    blk = adj[256:384, 128:256]
    assert blk.any()
    c = counts.copy()
    c[256:384] -= blk.sum(1)
    c[128:256] -= blk.sum(0)
    sweeps_fail(c=c)
    # the column half of that off-diagonal tile not added
    c = counts.copy()
    c[128:256] -= blk.sum(0)
    sweeps_fail(c=c)
    # '<' for '<=' at eps^2
    assert (D == 25.0).any()
    sweeps_fail(c=(D < 25.0).sum(1))
    # the self pair not counted
    sweeps_fail(c=counts - 1)
    # a root that is not the component's smallest core index
    roots, sizes = np.unique(orc.root[orc.core], return_counts=True)
    big = roots[sizes.argmax()]
    members = np.nonzero(orc.core & (orc.root == big))[0]
    assert members.size >= 2
    p = parent.copy()
    p[members] = members[1]
    sweeps_fail(p=p)
    # two components merged
    other = roots[roots != big][0]
    p = parent.copy()
    p[orc.root == max(big, other)] = min(big, other)
    sweeps_fail(p=p)
    lab = labels.copy()
    lab[orc.core & (orc.root == max(big, other))] = lab[min(big, other)]
    labels_fail(lab)
    # a border point given a cluster it is not adjacent to
    ids = orc.cluster_ids()
    for i in np.nonzero(orc.has_core_nb)[0]:
        adjacent = set(ids[np.nonzero(orc.adj[i] & orc.core)[0]])
        free = sorted(set(range(roots.size)) - adjacent)
        if free:
            lab = labels.copy()
            lab[i] = free[0]
            labels_fail(lab)
            break
    else:
        raise AssertionError("no border point with a non-adjacent cluster in the case")
    # cluster numbers permuted
    lab = labels.copy()
    lab[labels == 0], lab[labels == 1] = 1, 0
    labels_fail(lab)
    # a border marked noise, a noise point given a cluster, a key naming a farther core
    lab = labels.copy()
    lab[np.nonzero(orc.has_core_nb)[0][0]] = -1
    labels_fail(lab)
    if orc.noise.any():
        lab = labels.copy()
        lab[np.nonzero(orc.noise)[0][0]] = 0
        labels_fail(lab)
    for i in np.nonzero(orc.has_core_nb)[0]:
        far = np.nonzero(orc.adj[i] & orc.core & (D[i] > orc.dmin_core[i]))[0]
        if far.size:
            b = best.copy()
            b[i] = cases.pack_key(D[i, far[0]], far[0])
            sweeps_fail(b=b)
            break
    else:
        raise AssertionError("no border point with a second, farther core in the case")


def test_oracle_agrees_with_sklearn():
    """On cases with every pair decided the oracle's core points, noise and core labels are sklearn's
    (its euclidean distances of fp32 rows are computed in fp64; its cosine rule for all-zero rows is
    the contract)."""
    from sklearn.cluster import DBSCAN as SkDBSCAN

    Xn, eps = _generic("blobs8_65536")
    Xc = cases.generic_case(_cosine_rows(True), 0.6, "cosine")
    for X, e, metric, eps2 in ((Xn, eps, "euclidean", eps * eps), (Xc, 0.6, "cosine", 1.2)):
        ref = SkDBSCAN(eps=e, min_samples=5, metric=metric, algorithm="brute").fit(np.array(X))
        orc = make_oracle(X, eps2, 5, metric)
        assert np.array_equal(ref.core_sample_indices_, np.nonzero(orc.core)[0])
        assert np.array_equal(ref.labels_ == -1, orc.noise)
        assert np.array_equal(ref.labels_[orc.core], orc.cluster_ids()[orc.core])
        check_labels(orc, ref.labels_, core_idx=ref.core_sample_indices_)
    assert (ref.labels_[~Xc.any(1)] == -1).all()


def test_builder_asserts():
    """The builders refuse what the contracts exclude."""
    with pytest.raises(AssertionError):
        cases.assert_lattice(np.full((4, 4), 1100.0, np.float32))  # 4 n max^2 >= 2^24
    with pytest.raises(AssertionError):
        cases.assert_lattice(np.array([[0.5, 1.0]], np.float32))
    X = cases.blobs(300, 8, 3, 0.0, seed=2)
    r = cases.centred_norms(X)
    D = cases.sqdist64(X)
    i, j = np.unravel_index(np.argsort(D, axis=None)[400], D.shape)
    with pytest.raises(AssertionError):  # a pair exactly at eps^2 is undecided under any band
        make_oracle(X, float(D[i, j]), 5)
    Xk = cases.generic_case(X, float(np.sqrt(D[i, j])))
    assert Xk.shape[0] < 300 and r.min() > 0
