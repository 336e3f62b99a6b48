"""RandomForest level kernels (csrc/forest.hip) against the exact oracle of ``rf_hist_cases``:
``ops.rf_hist`` on every layout and kernel (feature-major, 32-byte records, row-major, fixed-point,
the 1024-thread wide kernel on 32 / 64-byte records with class, regression, fixed and packed cells)
at the row-slot, feature-chunk, record-group, bin / class and store edges, and ``ops.rf_best_split``
/ ``rf_node_split`` / ``rf_left_totals`` with ties held to the kernels' promise (highest gain, lowest
slot, lowest bin). Lattice cases are bit for bit, generic ones within the derived bound (contract in
``rf_hist_cases``, derivation in docs/coverage.md). The checker's own tests need no GPU.
Out of scope: NaN / inf labels, more than 2^31 positions, the SRML_RF_* switches of models/forest.py."""
import numpy as np
import pytest
import torch

import rf_hist_cases as cases
from rf_hist_cases import check_hist, check_split, hist_case, split_oracles
from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.ops import native
from spark_rapids_ml_nai_amd.utils.determinism import set_deterministic

gpu = pytest.mark.gpu
ITEM_PATHS = ("fm", "il", "rm", "fixed", "fixed_il")
WIDE_PATHS = tuple("wide%d%s" % (rb, k) for rb in (32, 64) for k in ("", "_fixed", "_packed"))
ALL_PATHS = ITEM_PATHS + WIDE_PATHS
RATIOS = {}  # path -> (worst sum error / bound, case): printed by test_zz_report


def _note(key, ratio, where):
    if ratio > RATIOS.get(key, (-1.0, ""))[0]:
        RATIOS[key] = (ratio, where)


def _paths(case, paths=ALL_PATHS):
    return [p for p in paths if case.regression or not ("fixed" in p or "packed" in p)]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_DEV = {}


def _dev_case(case, dev):
    """Device copies of a case and its three bin layouts (built once)."""
    key = (id(case), str(dev))
    if key not in _DEV:
        d = {k: _t(getattr(case, k), dev) for k in ("bins", "idx", "w", "y", "y_row", "node_feats")}
        d["case"] = case  # keeps id(case) from being reused
        d["wy"] = _t(np.stack([case.w, case.y], 1), dev)
        d["il32"] = ops.rf_interleave(d["bins"], 32)
        d["il64"] = ops.rf_interleave(d["bins"], 64)
        d["rm"] = ops.rf_row_major(d["bins"])
        if case.regression and not case.lattice:
            d["yscale"] = ops.rf_yscale(d["y"], float(case.w.sum()))
            d["pscale"] = ops.rf_pack_scale(d["y"])
        else:
            d["yscale"], d["pscale"] = case.yscale, case.packed_scale
        _DEV[key] = d
    return _DEV[key]


def _fb(case, path, fb=None):
    if path.startswith("wide"):
        cap = ops.rf_hist_fb_wide(case.B, case.S, case.regression, packed=path.endswith("packed"))
    else:
        cap = ops.rf_hist_fb(case.B, case.S, case.regression)
    return cap if fb is None else min(int(fb), cap)


def _kw(case, d, path):
    kw = dict(yscale=d["yscale"])
    if path in ("il", "fixed_il"):
        kw["bins_il"] = d["il32"]
    if path == "rm":
        kw["bins_rm"] = d["rm"]
    if path.startswith("wide"):
        rb = int(path[4:6])
        kw.update(wide=True, rec_bytes=rb, bins_il=d["il%d" % rb])
        if path.endswith("packed"):
            kw["packed_scale"] = d["pscale"]
    return kw


def run_hist(case, path, dev, fb=None, exclusive=False, chunks=None, out=None):
    d = _dev_case(case, dev)
    fb = _fb(case, path, fb)
    items = _t(case.items(fb, exclusive, chunks), dev)
    excl = {"multi_nodes": _t(case.multi_nodes(), dev)} if exclusive else None
    set_deterministic("fixed" in path)
    try:
        h = ops.rf_hist(d["bins"], d["idx"], d["y_row"], None, items, d["node_feats"], case.nodes, case.B, case.S,
                        case.regression, pos_weight=d["w"], fb=fb, exclusive=excl, out=out, wy=d["wy"],
                        **_kw(case, d, path))
    finally:
        set_deterministic(None)
    if exclusive:  # nodes without items are neither stored nor zeroed
        empty = [i for i, ch in enumerate(case.chunks) if not ch]
        if empty:
            h[_t(np.array(empty), dev)] = 0
    return h


def _check(case, h, path, dev, nchunks=None):
    d = _dev_case(case, dev)
    r = check_hist(case, h.cpu().numpy(), path, d["yscale"], d["pscale"], nchunks)
    _note(path, r, case.name)
    if "+1000" in case.name:
        _note(path + " (y + 1000)", r, case.name)
    return r


def run_poisoned(case, path, dev, fb=None):
    """The launch of ``ops.rf_hist(exclusive=...)`` on a buffer of 0xA5 bytes with only the
    multi-chunk nodes zeroed (``native.call`` on a pre-filled tensor)."""
    d = _dev_case(case, dev)
    fb = _fb(case, path, fb)
    items = _t(case.items(fb, True), dev)
    hdt = torch.float64 if case.regression else torch.int32
    hist = torch.full((case.nodes, case.nf, case.B, case.S, 8 if case.regression else 4), cases.POISON,
                      dtype=torch.uint8, device=dev).view(hdt).squeeze(-1)
    multi = [i for i, ch in enumerate(case.chunks) if len(ch) > 1]
    if multi:
        hist[_t(np.array(multi), dev)] = 0
    wy = d["wy"]
    st = native.stream(dev)
    hu, hd = (None, hist.data_ptr()) if case.regression else (hist.data_ptr(), None)
    if path.startswith("wide"):
        rb = int(path[4:6])
        packed = path.endswith("packed")
        native.call("srml_rf_hist_wide", d["il%d" % rb].data_ptr(), case.m, d["idx"].data_ptr(), wy.data_ptr(),
                    items.data_ptr(), int(items.shape[0]), d["node_feats"].data_ptr(), case.nf, case.B, case.S,
                    int(case.regression), float(d["pscale"] if packed else d["yscale"] or 1.0), fb,
                    2 if packed else 0, rb, hu, hd, st)
    else:
        mode = {"fm": 0, "il": 1, "rm": 2}[path]
        src = {"fm": d["bins"], "il": d["il32"], "rm": d["rm"]}[path]
        native.call("srml_rf_hist", src.data_ptr(), case.m if mode != 2 else case.n, d["idx"].data_ptr(),
                    wy.data_ptr(), items.data_ptr(), int(items.shape[0]), d["node_feats"].data_ptr(), case.nf,
                    case.B, case.S, int(case.regression), float(d["yscale"] or 1.0), fb, hu, hd, mode, st)
    return hist


# ------------------------------------------------------------------------------- the case list
def _mk(name, regression, lattice=True, m=300, n=40, B=16, S=3, rows=(700, 0, 513, 90), chunks=(3, 1, 1, 2),
        nf=9, **kw):
    return hist_case(name, m, n, B, 2 if regression else S, regression, lattice, tuple(rows), tuple(chunks), nf, **kw)


def _kinds(name, **kw):
    """A shape as classification, lattice regression and generic regression."""
    return [_mk(name + "/class", False, **kw), _mk(name + "/reg", True, **kw),
            _mk(name + "/generic", True, lattice=False, **kw)]


def base_cases():
    out = _kinds("base")
    out.append(_mk("base/generic+1000", True, lattice=False, yshift=1000.0, seed=3))
    return out


ROW_EDGES_ITEM = (1, 255, 256, 257, 511, 512, 513)
ROW_EDGES_WIDE = (1, 1023, 1024, 1025, 2047, 2048, 2049)


def row_case(rows, regression):
    # every edge length as a node of its own (one chunk), then one node of three chunks and an empty one
    return _mk("rows%s/%s" % (rows[0:2], "reg" if regression else "class"), regression, m=257,
               rows=tuple(rows) + (0, 600), chunks=(1,) * len(rows) + (1, 3), nf=3, n=5, seed=7)


NF_EDGES = (1, cases.FB - 1, cases.FB, cases.FB + 1, 2 * cases.FB + 1)
N_EDGES = (1, 31, 32, 33, 64, 65, 129, 200)
GROUP_FEATS = {
    "31|32": (31, 32), "63|64": (63, 64), "127|128": (127, 128), "one-group": (33, 35, 40, 62),
    "own-groups": (5, 40, 70, 100, 130, 170), "skip": (3, 170, 171), "unsorted": (40, 3, 70),
    "unsorted-back": (130, 129, 2, 64, 63, 1), "repeat": (7, 7, 64, 7),
}
BS_EDGES = ((2, 2), (16, 3), (33, 5), (255, 2), (256, 3), (256, 32), (16, 32))


# ========================================================================= CPU: oracle, checker
def test_constants():
    assert cases.FB == ops.RF_HIST_FB_MAX
    assert cases.PACK_BIAS == 1 << ops.RF_PACK_BITS
    assert cases.PACK_MAX_WEIGHT == ops.RF_PACK_MAX_WEIGHT == (1 << (64 - cases.PACK_SHIFT)) - 1
    assert ops.rf_hist_fb(256, 32, False) == 2 and (2 * 256 * 32 + 1) * 4 == 65540  # the > 64 KiB LDS shape
    assert ops.rf_hist_fb_wide(16, 2, True) > 74 > ops.rf_hist_fb(16, 2, True)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_oracle_agrees_with_cpu_twin(kind):
    """Two independent derivations (numpy integers here, torch index_add in ``ops``) agree."""
    case = base_cases()[kind]
    fb = ops.rf_hist_fb(case.B, case.S, case.regression)
    t = torch.from_numpy
    h = ops.rf_hist(t(case.bins), t(case.idx), t(case.y_row), None, t(case.items(fb)), t(case.node_feats), case.nodes,
                    case.B, case.S, case.regression, pos_weight=t(case.w), fb=fb)
    # the twin adds fp64 products in sequence: the fold term of the bound with k = rows covers it
    rows = [max(1, re - rb) for rb, re in map(case.node_range, range(case.nodes))]
    check_hist(case, h.numpy(), "fm", float("inf"), None, rows)  # no fixed-point step on this path


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("threads,rec", [(cases.ITEM_T, 32), (cases.WIDE_T, 64)])
def test_checker_accepts_model(kind, threads, rec):
    case = base_cases()[kind]
    excl = [i for i, ch in enumerate(case.chunks) if ch]
    for packed in ((False, True) if case.regression else (False,)):
        h = cases.simulate_hist(case, 4, threads, rec, exclusive=True, packed=packed)
        check_hist(case, h, touched=excl)


HIST_FAULTS = ("drop_row", "drop_second_slot", "prev_group_byte", "swap_bin_class", "count_in_sum",
               "packed_no_bias", "excl_zero_not_stored", "multi_stored")


@pytest.mark.parametrize("fault", HIST_FAULTS)
def test_checker_rejects_hist_fault(fault):
    reg = fault in ("count_in_sum", "packed_no_bias")
    # node 2: an exclusive node of 20 rows (most of its cells are zeros); node 0 has a chunk of 350 rows
    case = _mk("fault", reg, feats=(3, 31, 32, 33, 39), nf=5, rows=(700, 0, 20, 90))
    touched = [i for i, ch in enumerate(case.chunks) if ch]
    h = cases.simulate_hist(case, 4, exclusive=True, packed=fault == "packed_no_bias", fault=fault)
    with pytest.raises(AssertionError):
        check_hist(case, h, touched=touched)


def test_checker_rejects_write_to_untouched_node():
    case = base_cases()[0]
    h = cases.simulate_hist(case, 4, exclusive=True)
    h[1] = 0  # the node without rows was zeroed: somebody wrote it
    with pytest.raises(AssertionError):
        check_hist(case, h, touched=[0, 2, 3])


def _split_sets():
    return [("gini", cases.class_hist(6, 5, 8, 3, 1), False, 0), ("entropy", cases.class_hist(6, 5, 8, 3, 2), False, 1),
            ("var", cases.reg_hist(6, 5, 8, 3)[0], True, 2)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_split_checker_accepts_cpu_twin_and_model(which):
    _, hist, reg, crit = _split_sets()[which]
    S = hist.shape[-1]
    orcs = split_oracles(hist, reg, crit, 2.0, 0.0)
    cases.assert_decided(orcs)
    out, tot = ops.rf_best_split(torch.from_numpy(hist), hist.shape[2], S, reg, crit, 2.0, 0.0)
    left = ops.rf_left_totals(torch.from_numpy(hist), out)
    d, _ = check_split(orcs, out.numpy(), tot.numpy(), left.numpy())
    assert d >= 5
    check_split(orcs, *cases.emulate_best_split(hist, reg, crit, 2.0, 0.0))


@pytest.mark.parametrize("fault", ["min_leaf_strict", "tie_high_slot", "last_bin", "left_short"])
def test_split_checker_rejects_fault(fault):
    # two classes split cleanly at bin 1 by slots 0 and 2 (a duplicated column); min_leaf == n_left
    hist = np.zeros((1, 3, 4, 2), dtype=np.int32)
    hist[0, 0, 0] = hist[0, 2, 0] = (2, 0)
    hist[0, 0, 1] = hist[0, 2, 1] = (2, 0)
    hist[0, 0, 3] = hist[0, 2, 3] = (0, 5)
    hist[0, 1, 0], hist[0, 1, 3] = (2, 2), (2, 3)
    if fault == "last_bin":
        hist[0, :, :3] = 0
        hist[0, :, 3] = (4, 5)  # all mass in bin B - 1: no threshold at all
    orcs = split_oracles(hist, False, 0, 4.0, 0.0)
    check_split(orcs, *cases.emulate_best_split(hist, False, 0, 4.0, 0.0))
    with pytest.raises(AssertionError):
        check_split(orcs, *cases.emulate_best_split(hist, False, 0, 4.0, 0.0, fault=fault))


def test_out_with_exclusive_or_deterministic_raises():
    case = base_cases()[1]
    t = torch.from_numpy
    args = (t(case.bins), t(case.idx), t(case.y_row), None, t(case.items(4)), t(case.node_feats), case.nodes, case.B,
            case.S, True)
    out = torch.zeros((case.nodes, case.nf, case.B, 2), dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.rf_hist(*args, pos_weight=t(case.w), fb=4, out=out, exclusive={"multi_nodes": torch.zeros(0).long()})
    set_deterministic(True)
    try:
        with pytest.raises(ValueError):
            ops.rf_hist(*args, pos_weight=t(case.w), fb=4, out=out)
    finally:
        set_deterministic(None)


def test_generic_split_cases_are_decided():
    for yshift, nodes in ((0.0, 20), (1000.0, 10)):
        hist, sabs = cases.reg_hist(nodes, 6, 16, 11, lattice=False, yshift=yshift)
        orcs = split_oracles(hist, True, 2, 1.0, 0.0, sabs_u=16 * cases.U64 * sabs)
        cases.assert_decided(orcs)


# =================================================================================== GPU: histograms
@gpu
def test_native_constants(gpu_device):
    lib = native.lib()
    assert lib.srml_rf_hist_fb_max() == cases.FB
    for B, S, reg in ((16, 3, 0), (256, 32, 0), (33, 2, 1), (256, 2, 2)):
        assert lib.srml_rf_hist_wide_fb(B, S, reg) == ops.rf_hist_fb_wide(B, S, bool(reg), packed=reg == 2)
        assert lib.srml_rf_hist_fb(B, S, min(reg, 1)) == ops.rf_hist_fb(B, S, bool(reg))


def _all_paths_equal(case, dev, paths=ALL_PATHS, fb_item=None, fb_wide=None, exclusive=False):
    got = {}
    for p in _paths(case, paths):
        h = run_hist(case, p, dev, fb_wide if p.startswith("wide") else fb_item, exclusive)
        _check(case, h, p, dev)
        got[p] = h
    if not case.regression or case.lattice:  # exact contract: the paths agree bit for bit
        ref = next(iter(got.values()))
        for p, h in got.items():
            assert torch.equal(h, ref), p
    for p in ("fixed", "wide32_fixed"):  # deterministic mode: a second call is bit-identical
        if p in got:
            assert torch.equal(run_hist(case, p, dev, fb_wide if p.startswith("wide") else fb_item, exclusive), got[p])
    return got


@gpu
@pytest.mark.parametrize("k", range(4))
@pytest.mark.parametrize("exclusive", [False, True])
def test_hist_every_path(gpu_device, k, exclusive):
    _all_paths_equal(base_cases()[k], gpu_device, exclusive=exclusive)


@gpu
@pytest.mark.parametrize("kind", ["class", "reg", "generic"])
def test_hist_level_sized(gpu_device, kind):
    """A level of 60 nodes (50 .. 620 rows in 1, 2, 3 chunks), 200 of 256 features sampled: 25 chunks of
    the item kernel, ONE chunk of the wide kernel at its default ``rf_hist_fb_wide`` (four or eight
    record groups walked per row)."""
    rows = tuple(int(v) for v in np.random.default_rng(0).integers(50, 620, size=60))
    case = hist_case("level/" + kind, 5000, 256, 16, 2 if kind != "class" else 3, kind != "class", kind != "generic",
                     rows, (1, 2, 3) * 20, 200, seed=9)
    assert ops.rf_hist_fb_wide(16, case.S, case.regression) >= 200
    _all_paths_equal(case, gpu_device, exclusive=True)


@gpu
@pytest.mark.parametrize("regression", [False, True])
def test_hist_rows_per_item(gpu_device, regression):
    _all_paths_equal(row_case(ROW_EDGES_ITEM, regression), gpu_device, ITEM_PATHS, exclusive=True)
    _all_paths_equal(row_case(ROW_EDGES_WIDE, regression), gpu_device, WIDE_PATHS, exclusive=True)


@gpu
@pytest.mark.parametrize("nf", NF_EDGES)
def test_hist_feature_chunks(gpu_device, nf):
    for case in _kinds("nf%d" % nf, nf=nf, rows=(300, 40), chunks=(2, 1), seed=nf):
        _all_paths_equal(case, gpu_device, ITEM_PATHS)
        for fbw in (3, 5, 74, None):
            _all_paths_equal(case, gpu_device, WIDE_PATHS, fb_wide=fbw)


@gpu
@pytest.mark.parametrize("name", sorted(GROUP_FEATS))
def test_hist_record_groups(gpu_device, name):
    feats = GROUP_FEATS[name]
    for case in _kinds("grp-" + name, n=200, m=131, feats=feats, nf=len(feats), rows=(140, 30), chunks=(1, 2))[:2]:
        for fbw in (3, 5, 74):
            _all_paths_equal(case, gpu_device, fb_wide=fbw, fb_item=3 if fbw == 3 else None)


@gpu
@pytest.mark.parametrize("n", N_EDGES)
@pytest.mark.parametrize("m", [64, 67])  # m % 4 == 0: rf_interleave4_kernel, else rf_interleave_kernel
def test_hist_layout_sizes(gpu_device, n, m):
    nf = min(n, 11)
    feats = tuple(sorted({0, n - 1} | set(range(max(0, n - nf + 1), n))))
    for case in _kinds("n%d-m%d" % (n, m), n=n, m=m, feats=feats, nf=len(feats), rows=(100, 1), chunks=(2, 1))[:2]:
        _all_paths_equal(case, gpu_device, fb_wide=5)
        d = _dev_case(case, gpu_device)
        assert torch.equal(d["rm"].cpu(), torch.from_numpy(case.bins).t())


@gpu
@pytest.mark.parametrize("B,S", BS_EDGES)
def test_hist_bins_and_stats(gpu_device, B, S):
    ks = _kinds("B%d-S%d" % (B, S), B=B, S=S, nf=7, rows=(600, 10), chunks=(2, 1), seed=B + S)
    for case in (ks[:1] if S != 2 else ks):
        for fb in (None, 3):  # odd fb x odd B: the u64 plane behind an odd number of count words
            _all_paths_equal(case, gpu_device, fb_item=fb, fb_wide=fb, exclusive=fb is None)


@gpu
@pytest.mark.parametrize("k", [0, 1, 2])
def test_hist_poisoned_stores(gpu_device, k):
    case = base_cases()[k]
    touched = [i for i, ch in enumerate(case.chunks) if ch]
    for p in _paths(case, ("fm", "il", "rm", "wide32", "wide64", "wide32_packed", "wide64_packed")):
        for fb in (None, 3):
            h = run_poisoned(case, p, gpu_device, fb)
            d = _dev_case(case, gpu_device)
            check_hist(case, h.cpu().numpy(), p, d["yscale"], d["pscale"], touched=touched)


@gpu
@pytest.mark.parametrize("k", [0, 1, 2])
def test_hist_out_accumulates(gpu_device, k):
    case = base_cases()[k]
    first = [ch[:1] for ch in case.chunks]
    rest = [ch[1:] for ch in case.chunks]
    for p in _paths(case, ("fm", "il", "rm", "wide64", "wide64_packed")):
        one = run_hist(case, p, gpu_device)
        two = torch.zeros_like(one)
        run_hist(case, p, gpu_device, chunks=first, out=two)
        run_hist(case, p, gpu_device, chunks=rest, out=two)
        _check(case, two, p, gpu_device)
        if case.lattice or not case.regression:
            assert torch.equal(one, two)


@gpu
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_hist_fixed_point_limits(gpu_device, sign):
    """Every row of the tree at y = +-max|y| and weight 255 in one cell: the i64 sum sits at the
    ``rf_yscale`` bound 2^62; and the packed cell at the largest item weight the 20 count bits hold."""
    rows = 4096  # x weight 128 x |y| 4: W max|y| = 2^21, yscale = 2^41, still a lattice (every rint exact)
    case = hist_case("limit%+d" % sign, 50, 1, 2, 2, True, True, (rows,), (3,), 1, wmode="128", ymode=str(4.0 * sign))
    case = cases.HistCase(case.name, np.ones_like(case.bins), case.idx, case.w, case.y_row, case.node_feats,
                          case.chunks, 2, 2, True, True)
    d = _dev_case(case, gpu_device)
    d["yscale"] = ops.rf_yscale(d["y"], float(case.w.sum()))  # 2^62 / (W max|y|): the cell sum is +-2^62
    assert d["yscale"] == 2.0 ** 41 and rows * 128 * 4.0 * d["yscale"] == 2.0 ** 62
    for p in ITEM_PATHS + ("wide32", "wide64", "wide32_fixed", "wide64_fixed"):
        for excl in (False, True):
            h = run_hist(case, p, gpu_device, exclusive=excl)
            _check(case, h, p, gpu_device)
            assert h[0, 0, 1, 0].item() == rows * 128 and h[0, 0, 1, 1].item() == sign * rows * 128 * 4.0, p


@gpu
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("total", [cases.PACK_MAX_WEIGHT])
def test_hist_packed_weight_limit(gpu_device, sign, total):
    """65536 rows of weight 16 less one unit: sum w = 2^20 - 1 fills the packed cell's count field
    (bits 44..63) and, at |y| = max|y|, its sum field. (At 2^20 the count wraps to 0: the limit of
    ``ops.RF_PACK_MAX_WEIGHT`` is therefore 2^20 - 1.)"""
    rows = 65536
    case = hist_case("packed%+d" % sign, 64, 1, 2, 2, True, True, (rows,), (1,), 1, wmode="16", ymode=str(4.0 * sign))
    w = case.w.copy()
    w[5] = 15
    bins = np.ones_like(case.bins)
    case = cases.HistCase(case.name, bins, case.idx, w, case.y_row, case.node_feats, case.chunks, 2, 2, True, True)
    assert int(w.sum()) == total
    for p in ("wide32_packed", "wide64_packed"):
        h = run_hist(case, p, gpu_device, exclusive=True)
        _check(case, h, p, gpu_device)
        assert h[0, 0, 1, 0].item() == total and h[0, 0, 1, 1].item() == sign * 4.0 * total


# ================================================================================ GPU: split search
def _best(hist, reg, crit, min_leaf, min_gain, dev):
    h = torch.from_numpy(hist).to(dev)
    out, tot = ops.rf_best_split(h, hist.shape[2], hist.shape[3], reg, crit, float(min_leaf), float(min_gain))
    left = ops.rf_left_totals(h, out)
    return out.cpu().numpy(), tot.cpu().numpy(), left.cpu().numpy()


SPLIT_S = (2, 3, 4, 5, 8, 9, 16, 17, 32)


@gpu
@pytest.mark.parametrize("crit", [0, 1])
@pytest.mark.parametrize("S", SPLIT_S)
def test_best_split_classes(gpu_device, S, crit):
    hist = cases.class_hist(6, 5, 9, S, 100 + S)
    for min_leaf, min_gain in ((1.0, 0.0), (20.0, -1.0)):
        orcs = split_oracles(hist, False, crit, min_leaf, min_gain)
        cases.assert_decided(orcs)
        _, worst = check_split(orcs, *_best(hist, False, crit, min_leaf, min_gain, gpu_device))
        _note("best_split %s" % ("gini", "entropy")[crit], worst, "S = %d" % S)


@gpu
@pytest.mark.parametrize("nf", [1, 255, 256, 257, 600])
def test_best_split_feature_stride(gpu_device, nf):
    hist = cases.class_hist(3, nf, 4, 3, nf, mass=60)
    orcs = split_oracles(hist, False, 0, 1.0, 0.0)
    check_split(orcs, *_best(hist, False, 0, 1.0, 0.0, gpu_device))
    rh, _ = cases.reg_hist(3, nf, 4, nf, mass=60)
    check_split(split_oracles(rh, True, 2, 1.0, 0.0), *_best(rh, True, 2, 1.0, 0.0, gpu_device))


@gpu
@pytest.mark.parametrize("B", [2, 63, 64, 65, 128, 256])
def test_best_split_bins(gpu_device, B):
    hist = cases.class_hist(4, 3, B, 3, B, mass=150)
    check_split(split_oracles(hist, False, 0, 1.0, 0.0), *_best(hist, False, 0, 1.0, 0.0, gpu_device))
    rh, _ = cases.reg_hist(4, 3, B, B, mass=150)
    orcs = split_oracles(rh, True, 2, 3.0, 0.0)
    cases.assert_decided(orcs)
    _, worst = check_split(orcs, *_best(rh, True, 2, 3.0, 0.0, gpu_device))
    _note("best_split variance, lattice", worst, "B = %d" % B)


@gpu
@pytest.mark.parametrize("yshift,nodes", [(0.0, 20), (1000.0, 10)])
def test_best_split_generic_regression(gpu_device, yshift, nodes):
    hist, sabs = cases.reg_hist(nodes, 6, 16, 11, lattice=False, yshift=yshift)
    orcs = split_oracles(hist, True, 2, 1.0, 0.0, sabs_u=16 * cases.U64 * sabs)
    cases.assert_decided(orcs)
    out, tot, left = _best(hist, True, 2, 1.0, 0.0, gpu_device)
    d, worst = check_split(orcs, out, tot, left, exact_sums=False)
    RATIOS["best_split var y%+d" % yshift] = (worst, "%d of %d nodes decided" % (d, nodes))


def _edge_hist():
    """Nodes: 0 clean two-class split (gain exactly 0.5); 1 pure; 2 zero weight; 3 one row; 4 all mass
    in bin 0; 5 all mass in bin B - 1; 6 a left / right mirror (equal only mathematically); 7 a clean
    split 3 | 6; 8 a clean split 6 | 3."""
    h = np.zeros((9, 2, 6, 2), dtype=np.int32)
    h[7, :, 1], h[7, :, 4] = (3, 0), (0, 6)
    h[8, :, 1], h[8, :, 4] = (6, 0), (0, 3)
    h[0, :, 1], h[0, :, 4] = (4, 0), (0, 4)
    h[1, :, 0], h[1, :, 3] = (3, 0), (2, 0)
    h[3, :, 2] = (0, 1)
    h[4, :, 0] = (3, 2)
    h[5, :, 5] = (3, 2)
    h[6, :, 0], h[6, :, 2], h[6, :, 4] = (3, 1), (2, 2), (1, 3)
    return h


@gpu
@pytest.mark.parametrize("crit", [0, 1])
def test_best_split_edges(gpu_device, crit):
    h = _edge_hist()
    for min_leaf, min_gain in ((1.0, 0.0), (1.0, -1.0), (3.0, 0.0), (4.0, 0.0), (5.0, 0.0),
                               (1.0, 0.5 if crit == 0 else 1.0)):
        orcs = split_oracles(h, False, crit, min_leaf, min_gain)
        out, tot, left = _best(h, False, crit, min_leaf, min_gain, gpu_device)
        check_split(orcs, out, tot, left)
        assert (out[1:6, 1] == -1).all()  # pure, empty, one row, one-sided: never a split
        # node 0: n_left = n_right = 4, and its gain (0.5 gini, 1 bit) is computed exactly
        assert (out[0, 1] >= 0) == (min_leaf <= 4.0 and min_gain < 0.5), (min_leaf, min_gain, out[0])
        # nodes 7 / 8: min_leaf = n_left (n_right) = 3 is valid, one more is not; gains 4/9 and 0.918 bit
        assert ((out[7:9, 1] >= 0) == (min_leaf <= 3.0 and min_gain < 0.4)).all(), (min_leaf, min_gain, out[7:9])
    rh = np.zeros((3, 2, 6, 2))
    rh[0, :, 1], rh[0, :, 4] = (4, -8.0), (4, -24.0)     # negative sums
    rh[1, :, 1], rh[1, :, 4] = (4, -8.0), (4, 8.0)
    rh[2, :, 2] = (5, -3.0)
    for min_leaf in (4.0, 5.0):
        out, tot, left = _best(rh, True, 2, min_leaf, 0.0, gpu_device)
        check_split(split_oracles(rh, True, 2, min_leaf, 0.0), out, tot, left)
        assert (out[:2, 1] >= 0).all() == (min_leaf == 4.0) and out[2, 1] == -1


def _node_split_both(case, crit, min_leaf, min_gain, dev):
    """rf_node_split on the rows and rf_hist + rf_best_split + rf_left_totals on the same rows."""
    d = _dev_case(case, dev)
    se = _t(np.array([case.node_range(i) for i in range(case.nodes)], dtype=np.int32), dev)
    out, left = ops.rf_node_split(d["rm"], d["idx"], d["wy"], se, d["node_feats"], case.B, case.S, crit, float(min_leaf),
                                  float(min_gain))
    h = run_hist(case, "fm", dev)
    _check(case, h, "fm", dev)
    o2, tot = ops.rf_best_split(h, case.B, case.S, False, crit, float(min_leaf), float(min_gain))
    l2 = ops.rf_left_totals(h, o2)
    orcs = split_oracles(case.oracle["cnt"], False, crit, min_leaf, min_gain)
    _, worst = check_split(orcs, out.cpu().numpy(), None, left.cpu().numpy())
    _note("node_split %s" % ("gini", "entropy")[crit], worst, case.name)
    check_split(orcs, o2.cpu().numpy(), tot.cpu().numpy(), l2.cpu().numpy())
    assert torch.equal(out, o2) and torch.equal(left, l2), "rf_node_split and rf_hist + rf_best_split differ"


def _ns_rows(nf):
    lpr = 1
    while lpr < nf and lpr < 64:
        lpr *= 2
    step = cases.NS_U * 64 // lpr  # rows per wave step
    return (0, 1, step - 1, step, step + 1, 8 * step - 1, 8 * step, 8 * step + 1, 3 * 8 * step + 5)


@gpu
@pytest.mark.parametrize("nf", [1, 2, 3, 32, 33, 64, 65, 255, 256])
def test_node_split_features_and_rows(gpu_device, nf):
    rows = _ns_rows(nf)
    B = 8 if nf > 64 else 16
    case = hist_case("ns-nf%d" % nf, 300, 70, B, 3, False, True, rows, (1,) * len(rows), nf, seed=nf)
    assert ops.rf_node_split_ok(nf, B, 3)
    for crit in (0, 1):
        _node_split_both(case, crit, 1.0, 0.0, gpu_device)


@gpu
@pytest.mark.parametrize("S", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("B", [2, 63, 64, 65, 128, 256])
def test_node_split_classes_and_bins(gpu_device, S, B):
    # slots 0 and 3 read the same column, slot 2 repeats slot 1's feature id: exact ties every node
    case = hist_case("ns-S%d-B%d" % (S, B), 200, 6, B, S, False, True, (0, 1, 40, 333, 700), (1,) * 5, 4,
                     feats=(2, 5, 5, 2), seed=S * 1000 + B)
    for crit, min_leaf, min_gain in ((0, 1.0, 0.0), (1, 30.0, -1.0)):
        _node_split_both(case, crit, min_leaf, min_gain, gpu_device)


@gpu
@pytest.mark.parametrize("kind", ["bin0", "binlast", "pure"])
def test_node_split_degenerate(gpu_device, kind):
    """All mass in bin 0 or in bin B - 1 (no valid threshold) and a pure node: no split, zero left totals."""
    c = hist_case("ns-" + kind, 120, 5, 16, 3, False, True, (70, 300), (1, 1), 3, seed=5)
    bins = c.bins.copy() if kind == "pure" else np.full_like(c.bins, 0 if kind == "bin0" else 15)
    y_row = np.full_like(c.y_row, 2.0) if kind == "pure" else c.y_row
    case = cases.HistCase(c.name, bins, c.idx, c.w, y_row, c.node_feats, c.chunks, 16, 3, False, True)
    for crit in (0, 1):
        _node_split_both(case, crit, 1.0, -1.0, gpu_device)
    d = _dev_case(case, gpu_device)
    se = _t(np.array([case.node_range(i) for i in range(2)], dtype=np.int32), gpu_device)
    out, left = ops.rf_node_split(d["rm"], d["idx"], d["wy"], se, d["node_feats"], 16, 3, 0, 1.0, -1.0)
    assert (out[:, 1] == -1).all() and not left.any()


@gpu
def test_left_totals_records(gpu_device):
    """int32 and fp64 histograms; records without a split give zeros."""
    hist = cases.class_hist(5, 4, 16, 3, 77)
    out, tot, left = _best(hist, False, 0, 1e9, 0.0, gpu_device)
    assert (out[:, 1] == -1).all() and not left.any()
    rh, _ = cases.reg_hist(5, 4, 16, 78)
    out, tot, left = _best(rh, True, 2, 1e9, 0.0, gpu_device)
    assert (out[:, 1] == -1).all() and not left.any()


@gpu
def test_zz_report(gpu_device):
    """Prints the worst measured error / bound of every path (the table of docs/coverage.md)."""
    for k in sorted(RATIOS):
        print("rf-ratio %-22s %.4f  %s" % (k, RATIOS[k][0], RATIOS[k][1]))
