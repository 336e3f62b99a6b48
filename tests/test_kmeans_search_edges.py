"""KMeans nearest-centre searches (``ops.nearest_centroid*``: splitmm.hip, kmeans.hip, fp64.hip) at
the k-step, tile, dispatch and list edges, every kernel against the fp64 direct-form oracle of
``kmeans_search_cases`` under a derived per-row bound (contracts ``exact`` / ``within`` there).
No comparison uses a fraction of rows. Inputs are finite; NaN / inf rows are out of scope.

CPU part: the checker itself (it passes the CPU paths and catches each injected fault) and the
properties the case kinds claim. GPU part, scenarios A .. I of the module's sections."""
import numpy as np
import pytest
import torch

import kmeans_search_cases as cases
from kmeans_search_cases import check_labels, make_case
from spark_rapids_ml_nai_amd import ops


def _t(a, dev=None):
    t = torch.from_numpy(np.array(a, order="C"))  # a writable copy: the cases are read-only
    return t.to(dev) if dev is not None else t


def _np(t):
    return t.detach().cpu().numpy()


# =============================================================================== CPU: the checker
CPU_CASES = [(300, 33, 65, "ties"), (257, 17, 257, "generic"), (300, 48, 4, "ties")]


@pytest.mark.parametrize("m,n,k,kind", CPU_CASES)
def test_checker_passes_cpu_paths(m, n, k, kind):
    """The CPU branch of ``nearest_centroid_split`` (six plane products in fp32) and the torch
    fall-back of ``nearest_centroid`` hold the fp32-class contract; the oracle's own labels the
    exact one."""
    case = make_case(m, n, k, kind)
    V, W = _t(case.V), _t(case.W)
    xn = (V * V).sum(1)
    lab, d = ops.nearest_centroid_split(ops.split_bf16x3(V), m, W, xn)
    check_labels(case, _np(lab), _np(d), "within", cases.eps_fp32(case))
    lab, d = ops.nearest_centroid(V, W)
    check_labels(case, _np(lab), _np(d), "within", cases.eps_fp32(case))
    r = check_labels(case, case.arg, case.dmin, "exact")
    assert r["label"] == 0.0 and r["dist"] == 0.0


def test_checker_catches_injected_faults():
    case = make_case(300, 33, 65, "ties")
    eps = cases.eps_fp32(case)
    good, dist = case.arg.copy(), case.dmin.copy()
    second = np.where(np.arange(case.k)[None, :] == case.arg[:, None], np.inf, case.D).argmin(1)
    clear = np.nonzero(case.gap > 2.0 * eps.max() + case.beta.max())[0]
    assert clear.size > 100 and case.dup_rows.size == 75 and case.tie_rows.size == 75

    def fails(lab, d=dist, contracts=("exact", "within")):
        for c in contracts:
            with pytest.raises(AssertionError):
                check_labels(case, lab, d, c, eps)

    lab = good.copy()  # one label replaced by the second-nearest centre
    lab[clear[7]] = second[clear[7]]
    fails(lab)
    lab = good.copy()  # the duplicated pair answered with the higher index
    r = case.dup_rows[3]
    assert good[r] == 0 and case.gap[r] == 0.0
    lab[r] = 1
    fails(lab, contracts=("exact",))
    check_labels(case, lab, dist, "within", eps)  # the fp32-class contract does not promise the tie rule
    lab = good.copy()  # labels of the rows past the first 256-row tile shifted by one
    lab[256:] = np.roll(good[256:], 1)
    fails(lab)
    lab = good.copy()  # a centre index past k (a padded tile column)
    lab[11] = case.k
    fails(lab)
    lab[11] = -1
    fails(lab)
    d = dist.copy()  # the distances of one row tile zeroed
    d[:256] = 0.0
    fails(good, d)
    d = dist.copy()
    d[299] = np.nan
    fails(good, d)


def test_case_kinds_have_their_properties():
    c = make_case(300, 33, 65, "ties", shuffle=True)
    assert np.array_equal(c.C[0], c.C[1]) and not np.array_equal(c.C[2], c.C[3])
    assert (c.gap[c.dup_rows] == 0.0).all() and (c.arg[c.dup_rows] == 0).all()
    assert (c.gap[c.tie_rows] < 1e-4).all() and np.isin(c.arg[c.tie_rows], (0, 2, 3)).all()
    assert c.tie_rows.max() > 256 and c.tie_rows.min() < 256  # spread over the row tiles
    # far_centre: the scaled centre element leaves the fp16 plane's range
    for m, n, k in ((300, 33, 70), (300, 129, 257), (300, 128, 257)):
        c = make_case(m, n, k, "far_centre")
        assert cases.f16_scale(c) * np.abs(c.W).max() >= 2.0 ** 15
        assert 2.0 ** 13 <= cases.f16_scale(c) * np.abs(c.V).max() < 2.0 ** 14
    # crowd: more than F16_CAND_CAP centres inside every row's radius; the two variants sit on the cap
    for k in (130, 257):
        lo, _ = cases.f16_listed(make_case(300, 33, k, "crowd"))
        assert lo.min() > ops.F16_CAND_CAP
    lo, hi = cases.f16_listed(make_case(300, 33, 130, "crowd", near=64))
    assert lo.min() == 64 and hi.max() == 64 == ops.F16_CAND_CAP
    lo, hi = cases.f16_listed(make_case(300, 33, 130, "crowd", near=65))
    assert lo.min() == 65 and hi.max() == 65
    # wide_range: most plane elements fall below fp16's normal range (2^-14 after scaling)
    c = make_case(300, 40, 20, "wide_range")
    assert (np.abs(c.V) * cases.f16_scale(c) < 2.0 ** -14).mean() > 0.5
    c = make_case(300, 40, 20, "offset")
    assert abs(float(c.mu.mean()) - 1e4) < 1.0
    c = make_case(1, 17, 3, "generic")
    assert c.V[0, 0] == 4.0 and not c.mu.any()  # m = 1: mu is off the row
    # the filters cannot certify an engineered tie row (where the pair it bisects is its nearest)
    for a in ((300, 33, 65), (300, 64, 40), (257, 112, 65)):
        c = make_case(*a, "ties")
        q2 = 2 * (a[0] // 4)
        assert cases.f16_must_flag(c)[:q2].all() and cases.bf16_must_flag(c)[:q2].all()


# =============================================================================== GPU: the paths
def _device_case(case, dev):
    return {"X": _t(case.X, dev), "C": _t(case.C, dev), "mu": _t(case.mu, dev), "V": _t(case.V, dev),
            "W": _t(case.W, dev)}


def _count_calls(monkeypatch):
    from spark_rapids_ml_nai_amd.ops import native

    launches = {}
    real = native.call

    def counting(name, *args):
        launches[name] = launches.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(native, "call", counting)
    return launches


def _planes(case, t):
    F = ops.F16Planes(t["X"], t["mu"])
    assert F.ok and F.ovf is not None and int(F.ovf.item()) == 0
    assert F.scale == cases.f16_scale(case)
    return F


def _f16_dist_eps(case):
    # certified rows report the filter's distance: its radius plus the fp32 ||x - mu||^2 rounding
    # test_nearest_centroid_f16_certified_matches_exact allows
    return cases.eps_f16(case) + 1e-4 * float((case.vnorm ** 2).max())


def _run_f16(case, t, record=True, C=None):
    """Both modes of ``nearest_centroid_f16``; returns (labels exact, labels approx, refined exact)."""
    F = _planes(case, t)
    C = t["C"] if C is None else C
    st = dict(ops._CERTIFY_STATS)
    lab, d = ops.nearest_centroid_f16(F, C)
    rows = ops._CERTIFY_STATS["rows"] - st["rows"]
    refined = ops._CERTIFY_STATS["refined"] - st["refined"]
    assert rows == case.m
    # every row the filter cannot certify was re-searched: the engineered tie rows, unless a third
    # centre is nearer to a bisector row than the pair it bisects (f16_must_flag)
    assert refined >= cases.f16_must_flag(case).sum() >= case.dup_rows.size
    if case.kind != "far_centre":  # the centre plane stays in range: the filter, not the overflow path, ran
        assert cases.f16_scale(case) * np.abs(case.W).max() < 2.0 ** 15
    r = check_labels(case, _np(lab), _np(d), "exact", dist_eps=_f16_dist_eps(case))
    if record:
        cases.record("nearest_centroid_f16 exact", case, r)
    lab_a, d_a = ops.nearest_centroid_f16(F, C, approx=True)
    r = check_labels(case, _np(lab_a), _np(d_a), "within", cases.eps_f16(case))
    if record:
        cases.record("nearest_centroid_f16 approx", case, r)
    return lab, lab_a, refined


def _run_all_paths(case, dev, monkeypatch):
    t = _device_case(case, dev)
    m = case.m
    e32, e3 = cases.eps_fp32(case), cases.eps_split3(case)
    ties = cases.bf16_must_flag(case).sum()  # rows the 3-product filter cannot certify
    assert ties >= case.dup_rows.size
    _run_f16(case, t)
    # ---- split-bf16 on tiled, centred planes
    XP = ops.split_bf16x3(t["X"], tiled=True, mu=t["mu"])
    xn = ops.row_sqnorm(t["X"], t["mu"])
    lab6, d6 = ops.nearest_centroid_split(XP, m, t["C"], xn, mu=t["mu"])
    cases.record("split 6-product tiled", case, check_labels(case, _np(lab6), _np(d6), "within", e32))
    lab3, d3 = ops.nearest_centroid_split(XP, m, t["C"], xn, approx=True, mu=t["mu"])
    cases.record("split 3-product tiled", case, check_labels(case, _np(lab3), _np(d3), "within", e3))
    st = dict(ops._CERTIFY_STATS)
    labc, dc = ops.nearest_centroid_split(XP, m, t["C"], xn, X=t["X"], mu=t["mu"])
    assert ops._CERTIFY_STATS["rows"] - st["rows"] == m
    assert ops._CERTIFY_STATS["refined"] - st["refined"] >= ties
    assert torch.equal(labc, lab6)  # documented: the certified search gives the 6-product search's labels
    cases.record("split certified (mu)", case, check_labels(case, _np(labc), _np(dc), "within", e32, dist_eps=e3))
    # ---- the same on planes of V itself (mu = None: xnorm = ||v||^2, centres W)
    XPv = ops.split_bf16x3(t["V"], tiled=True)
    xnv = ops.row_sqnorm(t["V"])
    lab6v, d6v = ops.nearest_centroid_split(XPv, m, t["W"], xnv)
    check_labels(case, _np(lab6v), _np(d6v), "within", e32)
    st = dict(ops._CERTIFY_STATS)
    labcv, dcv = ops.nearest_centroid_split(XPv, m, t["W"], xnv, X=t["V"])
    assert ops._CERTIFY_STATS["refined"] - st["refined"] >= ties
    assert torch.equal(labcv, lab6v)
    cases.record("split certified (no mu)", case,
                 check_labels(case, _np(labcv), _np(dcv), "within", e32, dist_eps=e3))
    # ---- plain plane layout: 128-row tiles for k <= 256, 256-row tiles above
    XPn = ops.split_bf16x3(t["V"], tiled=False)
    assert XPn.dim() == 3
    labn, dn = ops.nearest_centroid_split(XPn, m, t["W"], xnv)
    cases.record("split 6-product plain", case, check_labels(case, _np(labn), _np(dn), "within", e32))
    # ---- fp32: the MFMA kernel, then the default dispatch (lloyd-small where it applies)
    monkeypatch.setenv("SRML_KMEANS_SMALL", "0")
    assert not ops.lloyd_small_ok(t["V"], case.k, search_only=True)
    lab, d = ops.nearest_centroid(t["V"], t["W"])
    cases.record("fp32 MFMA", case, check_labels(case, _np(lab), _np(d), "within", e32))
    monkeypatch.delenv("SRML_KMEANS_SMALL")
    small = ops.lloyd_small_ok(t["V"], case.k, search_only=True)
    assert small == (case.k <= 32 and case.n <= 64 and case.n % 4 == 0)
    lab, d = ops.nearest_centroid(t["V"], t["W"])
    cases.record("fp32 lloyd-small" if small else "fp32 MFMA", case,
                 check_labels(case, _np(lab), _np(d), "within", e32))
    # ---- fp64 operands: exact
    lab, d = ops.nearest_centroid(t["V"].double(), t["W"].double())
    cases.record("fp64 MFMA", case, check_labels(case, _np(lab), _np(d), "exact"))


# ---- A. k-step sweep: nk = 1 .. 7 with full and partial last k steps, every pipeline
A_N = [1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 64, 80, 81, 96, 97, 112]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["generic", "ties"])
@pytest.mark.parametrize("m,k", [(257, 65), (300, 257)])
@pytest.mark.parametrize("n", A_N)
def test_kstep_sweep(gpu_device, monkeypatch, n, m, k, kind):
    """nk = ceil(n / 16) = 1 .. 7 k steps: the fp16 filter (3 steps per barrier, 3 groups) runs its
    prologue guard ``j < nk`` and the vmcnt(0) branch at every nk < 6 and a partial first group at
    nk % 3 != 0; the 3-product pass (2 per barrier) an odd tail; the 6-product ring nk = 1, 2."""
    _run_all_paths(make_case(m, n, k, kind), gpu_device, monkeypatch)


# ---- B. tile-edge sweep
@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 48])
@pytest.mark.parametrize("k", [1, 2, 3, 63, 64, 65, 255, 256, 257, 513])
@pytest.mark.parametrize("m", [1, 7, 255, 256, 257, 513])
def test_tile_edge_sweep(gpu_device, monkeypatch, m, k, n):
    """Half-empty row tiles (m < 256), one row, one centre (no second best), two; the last centre
    tile 1, 63, 64, 65, 255 and 256 wide. The j < k masks of the epilogues are all that keep the
    padded centres (norms left unset past k) out of the arg-min: every label is checked to lie in
    [0, k) before anything else."""
    case = make_case(m, n, k, "ties" if k >= 4 else "generic")
    _run_all_paths(case, gpu_device, monkeypatch)


# ---- C. srml_kmeans_cand_exact dispatch
def _cand_exact_variant(n, ld, x_ptr, ldw, w_ptr=0, mu_ptr=0):
    """The kernel ``srml_kmeans_cand_exact`` picks (its dispatch condition, copied)."""
    vec = n % 4 == 0 and ld % 4 == 0 and ldw % 4 == 0 and x_ptr % 16 == 0 and w_ptr % 16 == 0 and mu_ptr % 16 == 0
    nv = (n // 4 + 63) // 64
    for width in (4, 8, 12, 16):
        if vec and nv <= width:
            return "vec%d" % width
    return "scalar"


def _check_planes(case, F, X):
    """``F.xnorm`` against the fp64 norms (fp32 accumulation: (n + 2) u ||v||^2) and a few rows of
    the tiled, swizzled fp16 plane against fp16(scale * v), first and last k step."""
    err = np.abs(_np(F.xnorm).astype(np.float64) - case.vnorm ** 2)
    assert (err <= (case.n + 2) * cases.U32 * case.vnorm ** 2).all()
    P = _np(F.P.float())  # [tiles][ks][256][16]
    want = (case.V.astype(np.float64) * F.scale).astype(np.float16).astype(np.float32)
    for r in (0, 7, 8, 255, 256, case.m - 1):
        for ks in (0, F.kp // 16 - 1):
            phys = P[r // 256, ks, r % 256]
            sw = (r % 256 >> 3) & 1
            logical = np.concatenate([phys[8 * sw: 8 * sw + 8], phys[8 * (sw ^ 1): 8 * (sw ^ 1) + 8]])
            w = np.zeros(16, np.float32)
            cols = want[r, 16 * ks: 16 * ks + 16]
            w[: cols.size] = cols
            assert np.array_equal(logical, w), (r, ks)
    assert not P[(case.m - 1) // 256, :, (case.m - 1) % 256 + 1:].any()  # padding rows are zero


# seed 1: with seed 0 one bisector row at n = 4096 has an oracle gap inside beta (the checker refuses
# such a case instead of skipping the row); none of the widths below has one with this seed
C_SEED = 1
C_CASES = [(1024, "vec4"), (1028, "vec8"), (2048, "vec8"), (2052, "vec12"), (3072, "vec12"), (3076, "vec16"),
           (4096, "vec16"), (4100, "scalar"), (4099, "scalar")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,variant", C_CASES)
def test_cand_exact_dispatch_by_width(gpu_device, n, variant):
    """NV = 4 | 8 | 12 | 16 by ceil(n / 4 / 64), the scalar kernel past n = 4096 and at n % 4 != 0.
    The branch is known from the dispatch condition (copied above) on the very pointers the call
    passes, and from ``refined``: every engineered tie row went through the kernel."""
    case = make_case(300, n, 40, "ties", seed=C_SEED)
    t = _device_case(case, gpu_device)
    assert _cand_exact_variant(n, t["X"].stride(0), t["X"].data_ptr(), n) == variant
    _, _, refined = _run_f16(case, t)
    assert refined >= 150


@pytest.mark.gpu
@pytest.mark.parametrize("width,gather", [(66, "plane"), (68, "plane"), (64, "rows"), (66, "rows")])
def test_cand_exact_dispatch_by_alignment(gpu_device, monkeypatch, width, gather):
    """X a view buf[:, 1:65]: the base is 4 B off a 16-B boundary with ld = 66 (even, not a multiple
    of 4) or ld = 68 (a multiple of 4): both take the scalar ``cand_exact`` kernel and the scalar
    branch of ``split_tiled_f16_kernel``. ``SRML_F16_GATHER=rows`` re-converts the flagged rows from
    X (``srml_split_f16_tiled_centered_rows``) instead of gathering them from the plane."""
    case = make_case(300, 64, 40, "ties")
    t = _device_case(case, gpu_device)
    if width == 64:
        X = t["X"]
    else:
        buf = torch.full((case.m, width), 7.0, device=gpu_device)
        buf[:, 1:65] = t["X"]
        X = buf[:, 1:65]
        assert X.data_ptr() % 16 == 4 and X.stride(0) == width and X.stride(1) == 1
    want = "vec4" if width == 64 else "scalar"
    assert _cand_exact_variant(64, X.stride(0), X.data_ptr(), 64) == want
    monkeypatch.setenv("SRML_F16_GATHER", gather)
    t["X"] = X
    F = _planes(case, t)
    _check_planes(case, F, X)
    _, _, refined = _run_f16(case, t, record=False)
    assert refined >= 150


# ---- D. candidate-list overflow
@pytest.mark.gpu
@pytest.mark.parametrize("k,near", [(130, None), (257, None), (130, 64), (130, 65)])
def test_candidate_list_overflow(gpu_device, k, near):
    """``crowd``: every row has more than F16_CAND_CAP = 64 centres inside its radius, so no row is
    certified (``refined == m``) and every list overflows: the exact pass scans every centre
    (``cnt > cap``). near = 64 / 65: exactly 64 (the list is full, not overflowed) and exactly 65
    (overflowed by one) listed centres; the counts are proven on the CPU by ``f16_listed``
    (test_case_kinds_have_their_properties)."""
    case = make_case(300, 33, k, "crowd", near=near)
    lo, hi = cases.f16_listed(case)
    if near == 64:
        assert lo.min() == hi.max() == ops.F16_CAND_CAP
    else:
        assert lo.min() > ops.F16_CAND_CAP
    t = _device_case(case, gpu_device)
    _, _, refined = _run_f16(case, t)
    assert refined == case.m


# ---- E. centre-plane overflow
@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(300, 33, 70), (300, 129, 257)])
def test_centre_plane_overflow(gpu_device, m, n, k):
    """``far_centre``: one centre element reaches 2^15 after scaling, the centre plane's flag is
    raised, nothing is certified (``refined == m``: thr = +inf, every centre listed, k > cap: full
    scan) and BOTH modes return the exact arg-min, as the docstring promises on overflow."""
    case = make_case(m, n, k, "far_centre")
    t = _device_case(case, gpu_device)
    F = _planes(case, t)
    flag = ops._f16_centre_planes(F, t["C"], False)[3]
    assert int(flag[0].item()) == 1  # the centre plane's overflow flag
    assert int(ops._f16_centre_planes(F, _t(make_case(m, n, k, "generic").C, gpu_device), False)[3][0].item()) == 0
    for approx in (False, True):
        st = dict(ops._CERTIFY_STATS)
        lab, d = ops.nearest_centroid_f16(F, t["C"], approx=approx)
        assert ops._CERTIFY_STATS["refined"] - st["refined"] == m
        r = check_labels(case, _np(lab), _np(d), "exact")  # every distance is the fp64 one
        cases.record("nearest_centroid_f16 overflow", case, r)


@pytest.mark.gpu
def test_rowloop_refuses_overflowed_centres(gpu_device):
    case = make_case(300, 128, 257, "far_centre")
    t = _device_case(case, gpu_device)
    F = _planes(case, t)
    assert F.kp == 128
    assert ops.nearest_f16_labels(F, t["C"]) is None
    assert ops.nearest_f16_labels(F, _t(make_case(300, 128, 257, "generic").C, gpu_device)) is not None


# ---- F. row-chunked launches
@pytest.mark.gpu
@pytest.mark.parametrize("k", [65, 300])
def test_row_chunks_bit_identical(gpu_device, monkeypatch, k):
    """256 rows per launch: three filter launches with r0 = 0, 256, 512 (``flagged[c0:nc] += r0``,
    ``labels[r0:]``) and, with 350 tie rows spread over all of them, two candidate chunks
    (``thr[q0:]``, ``ccount[q0:]``, ``cand[q0 * cap:]``). Labels and distances equal the one-launch
    call's bit for bit."""
    case = make_case(700, 33, k, "ties", shuffle=True)
    ties = np.concatenate([case.tie_rows, case.dup_rows])
    assert ties.size == 350 and all(((ties >= lo) & (ties < lo + 256)).sum() > 50 for lo in (0, 256, 512))
    t = _device_case(case, gpu_device)
    F = _planes(case, t)
    lab0, d0 = ops.nearest_centroid_f16(F, t["C"])
    a0, da0 = ops.nearest_centroid_f16(F, t["C"], approx=True)
    launches = _count_calls(monkeypatch)
    monkeypatch.setattr(ops, "split_rows_per_launch", lambda k: 256)
    st = dict(ops._CERTIFY_STATS)
    lab1, d1 = ops.nearest_centroid_f16(F, t["C"])
    refined = ops._CERTIFY_STATS["refined"] - st["refined"]
    assert ops._CERTIFY_STATS["rows"] - st["rows"] == 700 and refined >= 350
    assert launches["srml_nearest_centroid_f16_top2"] == 3
    assert launches["srml_nearest_centroid_f16_cand"] == (refined + 255) // 256 >= 2
    assert launches["srml_kmeans_cand_exact"] == 1
    a1, da1 = ops.nearest_centroid_f16(F, t["C"], approx=True)
    assert torch.equal(lab1, lab0) and torch.equal(d1.view(torch.int32), d0.view(torch.int32))
    assert torch.equal(a1, a0) and torch.equal(da1.view(torch.int32), da0.view(torch.int32))
    check_labels(case, _np(lab1), _np(d1), "exact", dist_eps=_f16_dist_eps(case))


# ---- G. fp64 centres, sub-normal plane elements
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["generic", "offset"])
@pytest.mark.parametrize("m,n,k", [(300, 40, 20), (300, 257, 300)])
def test_fp64_centres(gpu_device, m, n, k, kind):
    """The ``c_f64`` branch of ``srml_f16_centre_prep``: W = fp32(C - mu) with one rounding of the
    fp64 difference. The oracle is built from exactly that W; the fp32-rounded centres have their
    own, and where the two oracles agree so must the labels."""
    c64 = make_case(m, n, k, kind, c64=True)
    assert c64.C.dtype == np.float64 and not np.array_equal(c64.C.astype(np.float32).astype(np.float64), c64.C)
    t = _device_case(c64, gpu_device)
    lab64, _, _ = _run_f16(c64, t, record=False)
    c32 = cases.Case(c64.X, c64.C.astype(np.float32), c64.mu, kind)
    lab32, _, _ = _run_f16(c32, t, record=False, C=_t(c32.C, gpu_device))
    agree = c64.arg == c32.arg
    assert agree.mean() > 0.9 and np.array_equal(_np(lab64)[agree], _np(lab32)[agree])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["wide_range", "offset"])
@pytest.mark.parametrize("m,n,k", [(300, 40, 20), (300, 257, 300)])
def test_subnormal_and_offset_planes(gpu_device, m, n, k, kind):
    """Plane elements below fp16's normal range (``wide_range``: the absolute F16_A term of the
    radius carries the certificate) and a common offset of 1e4 (centring in fp32)."""
    case = make_case(m, n, k, kind)
    _run_f16(case, _device_case(case, gpu_device))


# ---- H. degenerate planes and the model-level fall-back
@pytest.mark.gpu
def test_degenerate_planes_fall_back(gpu_device, monkeypatch):
    """``F16Planes.ok`` is False for constant X and for m = 1 with mu = the row (no non-zero
    range); ``kmeans_predict`` then takes the bf16 certified path and returns the oracle's labels,
    and ``kmeans_fit`` keeps the bf16 planes."""
    from spark_rapids_ml_nai_amd.models.kmeans import kmeans_fit, kmeans_predict
    from spark_rapids_ml_nai_amd.parallel.context import PartitionDescriptor, WorkerContext

    g = np.random.default_rng(5)
    m, n, k = 65536, 17, 257
    row = g.standard_normal(n).astype(np.float32)
    X = _t(np.tile(row, (m, 1)), gpu_device)
    assert ops.F16Planes(X, X[0]).ok is False
    assert ops.F16Planes(X[:1], X[0]).ok is False
    C = (row.astype(np.float64) + 0.1 * g.standard_normal((k, n))).astype(np.float32)
    monkeypatch.setenv("SRML_KMEANS_SPLIT", "1")
    launches = _count_calls(monkeypatch)
    st = dict(ops._CERTIFY_STATS)
    lab = kmeans_predict(X, _t(C, gpu_device))
    assert ops._CERTIFY_STATS["rows"] - st["rows"] == m  # a certified path ran ...
    assert launches.get("srml_nearest_centroid_split_top2", 0) == 1  # ... the bf16 one
    assert "srml_nearest_centroid_f16_top2" not in launches
    mu = _np(ops.col_moments(X, need_sq=False)[0].div_(m).float())
    case = cases.Case(np.tile(row, (300, 1)), C, mu, "generic")  # every row is this row
    lab = _np(lab)
    assert (lab == lab[0]).all()
    check_labels(case, lab[:300], None, "within", cases.eps_fp32(case))
    # a fit on the same data: every centre is the row itself, every row ties at the lowest index
    ctx = WorkerContext.single(gpu_device)
    Xs = X[:600].contiguous()
    out = kmeans_fit(Xs, PartitionDescriptor.build(ctx, 600, n), ctx, k=k, max_iter=3, tol=0.0, seed=1, init="random")
    assert out["refined_frac"] is not None
    # (cluster 0's mean of 600 copies of the row: fp32 partial sums, 600 u relative)
    np.testing.assert_allclose(out["cluster_centers_"], np.tile(row.astype(np.float64), (k, 1)),
                               rtol=600 * cases.U32, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_small_fit_matches_fp64_lloyd(gpu_device, monkeypatch, mode):
    """Three Lloyd steps of a k > 256 fit on either certified filter against a plain fp64 Lloyd loop
    from the same start, at the KMeans tolerance of tests/test_oracles.py (rtol = atol = 1e-4)."""
    from spark_rapids_ml_nai_amd.models.kmeans import init_random, kmeans_fit
    from spark_rapids_ml_nai_amd.parallel.context import PartitionDescriptor, WorkerContext

    m, n, k = 600, 17, 257
    case = make_case(m, n, k, "generic", seed=3)
    X = _t(case.X, gpu_device)
    ctx = WorkerContext.single(gpu_device)
    desc = PartitionDescriptor.build(ctx, m, n)
    monkeypatch.setenv("SRML_KMEANS_SPLIT", "1")
    monkeypatch.setenv("SRML_KMEANS_FILTER", mode)
    launches = _count_calls(monkeypatch)
    out = kmeans_fit(X, desc, ctx, k=k, max_iter=3, tol=0.0, seed=3, init="random")
    assert 1 <= out["n_iter"] <= 3 and out["refined_frac"] is not None
    name = "srml_nearest_centroid_f16_top2" if mode == "f16" else "srml_nearest_centroid_split_top2"
    assert launches.get(name, 0) == out["n_iter"]  # every Lloyd step searched on the chosen filter
    C = _np(init_random(X, desc, ctx, k, 3).double())
    X64 = case.X.astype(np.float64)
    for _ in range(3):
        lab = cases.direct_distances(X64, C).argmin(1)
        for j in range(k):
            if (lab == j).any():
                C[j] = X64[lab == j].mean(0)
    np.testing.assert_allclose(out["cluster_centers_"], C, rtol=1e-4, atol=1e-4)


# ---- I. srml_nearest_f16_rowloop (kp = 128)
@pytest.mark.gpu
@pytest.mark.parametrize("n", [113, 128])
@pytest.mark.parametrize("k", [257, 300, 513])
@pytest.mark.parametrize("m", [1, 255, 257])
def test_rowloop_small_shapes(gpu_device, m, k, n):
    """The one-pass-per-row-tile fp16 arg-min at one row, a half-empty and a second row tile, and a
    last centre tile 1, 44 and 1 wide: within the fp16 filter's radius of the oracle, and the top-2
    filter's approximate arg-min wherever the oracle's gap exceeds twice that radius."""
    case = make_case(m, n, k, "generic")
    t = _device_case(case, gpu_device)
    F = _planes(case, t)
    assert F.kp == 128
    lab = ops.nearest_f16_labels(F, t["C"])
    assert lab is not None and lab.dtype == torch.int32 and lab.shape == (m,)
    eps = cases.eps_f16(case)
    cases.record("nearest_f16_rowloop", case, check_labels(case, _np(lab), None, "within", eps))
    ref = _np(ops.nearest_centroid_f16(F, t["C"], approx=True)[0])
    clear = case.gap > 2.0 * eps
    assert np.array_equal(_np(lab)[clear], ref[clear])
