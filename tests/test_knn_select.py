"""``ops.topk_rows``, ``ops.knn``, ``ops.knn_refine_sort`` and the exact ``NearestNeighbors`` at the
digit, tile, slice, chunk and k edges of ``csrc/topk.hip`` and ``csrc/knn.hip``, against the exact
selection oracle and the fp64 kNN oracle of ``tests/knn_select_cases.py``. Every case runs on the
host form and, marked ``gpu``, on the device; the checkers are tested against injected faults."""
import warnings

import numpy as np
import pytest
import torch

import knn_select_cases as cases
from spark_rapids_ml_nai_amd import DataFrame, ops
from spark_rapids_ml_nai_amd.knn import NearestNeighbors
from spark_rapids_ml_nai_amd.models import knn as mknn
from spark_rapids_ml_nai_amd.ops import native

warnings.filterwarnings("ignore")

BK = 32          # k-tile of csrc/tile.h
CPU = torch.device("cpu")
DEVICES = [pytest.param("cpu", id="host"), pytest.param("cuda", id="device", marks=pytest.mark.gpu)]
RATIOS = {}      # path -> worst error / bound seen in this run (printed by the last test)


def _dev(name):
    return torch.device("cuda", 0) if name == "cuda" else CPU


def _note(path, ratio):
    RATIOS[path] = max(RATIOS.get(path, 0.0), ratio)
    print("ratio %-40s %.3f" % (path, ratio))


# ------------------------------------------------------------------------------------------
# the checkers against injected faults (CPU)
# ------------------------------------------------------------------------------------------
def _select_fault_input():
    rng = np.random.default_rng(5)
    v = rng.integers(0, 40, (3, 700)).astype(np.float32)  # many ties
    return v, 90, dict(id_base=(1 << 31) + 5, slice_len=300)


def test_checker_accepts_the_model():
    v, k, kw = _select_fault_input()
    ov, oi = cases.model_select(v, k, **kw)
    cases.check_select(v, k, ov, oi, id_base=kw["id_base"])
    ov, oi = cases.model_select(v[:, :50], k, **kw)  # padded
    cases.check_select(v[:, :50], k, ov, oi, id_base=kw["id_base"])


@pytest.mark.parametrize("fault", ["dropped_column", "lost_c0", "ignored_id_base", "swapped_ties", "next_value",
                                   "foreign_value", "unsorted"])
def test_checker_rejects_select_fault(fault):
    v, k, kw = _select_fault_input()
    ov, oi = cases.model_select(v, k, fault=fault, **kw)
    with pytest.raises(AssertionError):
        cases.check_select(v, k, ov, oi, id_base=kw["id_base"])


def test_checker_rejects_padding_id():
    v, k, kw = _select_fault_input()
    ov, oi = cases.model_select(v[:, :50], k, fault="padding_id", **kw)
    with pytest.raises(AssertionError, match="padding id"):
        cases.check_select(v[:, :50], k, ov, oi, id_base=kw["id_base"])


def test_checker_rejects_a_dropped_item_tile():
    for exact in (True, False):
        _, _, orc = cases.lattice_case(5, 300, 8) if exact else cases.generic_case(40, 300, 16, 10)
        d, i = cases.model_knn(orc, 10)
        cases.check_knn(orc, d, i, 10, exact=exact)
        d, i = cases.model_knn(orc, 10, drop=slice(128, 256))
        with pytest.raises(AssertionError):
            cases.check_knn(orc, d, i, 10, exact=exact)


def test_checker_rejects_swapped_tied_items():
    _, _, orc = cases.lattice_case(5, 300, 4, amp=1)
    d, i = cases.model_knn(orc, 10)
    r, j = np.argwhere(d[:, 1:] == d[:, :-1])[0]
    i[r, [j, j + 1]] = i[r, [j + 1, j]]
    with pytest.raises(AssertionError, match="order"):
        cases.check_knn(orc, d, i, 10, exact=True)


def test_checker_rejects_expanded_form_as_refined():
    X = cases.near_duplicates()
    orc = cases.KnnOracle(X, X)
    d, i = cases.model_knn(orc, 2)
    assert cases.check_knn(orc, d, i, 2, which="refined") <= 1.0  # the direct form in fp32 meets the bound
    d, i = cases.model_knn(orc, 2, dist_matrix=cases.expanded_f32(X, X))
    cases.check_knn(orc, d, i, 2, which="keys")
    with pytest.raises(AssertionError, match="off its bound"):
        cases.check_knn(orc, d, i, 2, which="refined")


def test_checker_rejects_refine_faults():
    Q, X = cases.lattice(4, 9, 3, 1), cases.lattice(50, 9, 1, 2)
    pos = np.random.default_rng(0).integers(0, 50, (4, 20))
    Din = ((X[pos].astype(np.float64) - Q[:, None, :]) ** 2).sum(-1)
    order = np.argsort(Din, 1, kind="stable")
    d, p = np.take_along_axis(Din, order, 1).astype(np.float32), np.take_along_axis(pos, order, 1)
    cases.check_refine(Q, X, pos, d, p, exact=True)
    r, j = np.argwhere((d[:, 1:] == d[:, :-1]) & (p[:, 1:] != p[:, :-1]))[0]
    p2 = p.copy()
    p2[r, [j, j + 1]] = p2[r, [j + 1, j]]
    with pytest.raises(AssertionError):
        cases.check_refine(Q, X, pos, d, p2, exact=True)
    p3 = p.copy()
    p3[0, 0] = (p3[0, 0] + 1) % 50
    with pytest.raises(AssertionError):
        cases.check_refine(Q, X, pos, d, p3)


# ------------------------------------------------------------------------------------------
# ops.topk_rows
# ------------------------------------------------------------------------------------------
def _topk(dev, vals, k, ids=None, id_base=0, slice_len=None, strided=False):
    """Run ``ops.topk_rows`` on ``dev``, check the contract and that a second call repeats bit for
    bit; ``strided``: the values are the view ``D[:rows, :L]`` of a wider, taller buffer."""
    v = torch.from_numpy(np.ascontiguousarray(vals))
    if strided:
        buf = torch.full((vals.shape[0] + 2, vals.shape[1] + 5), -7.0)  # a read past the view would win
        buf[:vals.shape[0], :vals.shape[1]] = v
        v = buf.to(dev)[:vals.shape[0], :vals.shape[1]]
        assert v.stride(0) == vals.shape[1] + 5
    else:
        v = v.to(dev)
    it = torch.from_numpy(np.ascontiguousarray(ids)).to(dev) if ids is not None else None
    ov, oi = ops.topk_rows(v, k, ids=it, id_base=id_base, slice_len=slice_len)
    cases.check_select(vals, k, ov, oi, ids, id_base)
    ov2, oi2 = ops.topk_rows(v, k, ids=it, id_base=id_base, slice_len=slice_len)
    assert cases.bits_equal(ov, ov2) and cases.bits_equal(oi, oi2), "a second call differs"
    return ov, oi


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("p,digit", [(0, 3), (0, 2044), (0, 480), (0, 487), (0, 1040), (0, 1047),
                                     (1, 0), (1, 2047), (1, 1040), (1, 1047),
                                     (2, 0), (2, 1023), (2, 520), (2, 527)])
def test_topk_kth_key_digit(dev, p, digit):
    """The k-th key in the first / last bucket of a pass and on both ends of a thread's 8-bucket
    share; the rows of p = 1 share the top 11 bits, those of p = 2 the top 22 (only pass 3 decides).
    The builder asserts the digit of the k-th key."""
    rng = np.random.default_rng(100 * p + digit)
    assert digit % cases.TK_SHARE in (0, 3, 4, 7)
    rows = [cases.kth_digit_row(p, digit, rng) for _ in range(2)]
    assert rows[0][1] == rows[1][1]
    _topk(_dev(dev), np.stack([r for r, _ in rows]), rows[0][1])


@pytest.mark.parametrize("dev", DEVICES)
def test_topk_pass3_only_and_all_equal(dev):
    rng = np.random.default_rng(1)
    v = (1.0 + rng.integers(0, 1024, (5, 1500)) * 2.0 ** -23).astype(np.float32)  # 1 + j 2^-23: top 22 bits shared
    assert len(np.unique(cases.orderable(v) >> 10)) == 1
    for k in (1, 700, 1499):
        _topk(_dev(dev), v, k)
    for val in (0.25, -3.0, 0.0, np.inf, -np.inf):
        _topk(_dev(dev), np.full((2, 600), val, dtype=np.float32), 300)


@pytest.mark.parametrize("dev", DEVICES)
def test_topk_values(dev):
    rng = np.random.default_rng(2)
    d = _dev(dev)
    _topk(d, -np.abs(rng.standard_normal((3, 900))).astype(np.float32), 100)          # negative
    _topk(d, (rng.standard_normal((3, 900)) * 1e3).astype(np.float32), 450)           # mixed sign
    sub = (rng.integers(1, 1 << 23, (3, 900)).astype(np.uint32)
           | (rng.integers(0, 2, (3, 900)).astype(np.uint32) << np.uint32(31))).view(np.float32)
    assert (np.abs(sub) < np.finfo(np.float32).tiny).all() and (sub != 0).all()
    _topk(d, sub, 450)                                                                # subnormals
    _topk(d, np.concatenate([sub, np.zeros((3, 50), np.float32), -np.zeros((3, 50), np.float32)], 1), 500)
    inf = rng.standard_normal((3, 400)).astype(np.float32)
    inf[:, ::3] = np.inf
    inf[:, 1::17] = -np.inf
    for k in (10, 300, 400, 420):  # genuine +inf entries keep their ids; -1 only past L
        ov, oi = _topk(d, inf, k, id_base=7)
        assert (cases._np(oi)[:, :min(k, 400)] >= 7).all()


@pytest.mark.parametrize("dev", DEVICES)
def test_topk_signed_zeros_tie(dev):
    """-0.0 and +0.0 tie: the lower column first, whichever sign it carries."""
    rng = np.random.default_rng(3)
    v = rng.choice(np.array([-0.0, 0.0, -0.0, 0.0, -1.0, 1.0, 1e-40, -1e-40], dtype=np.float32), (4, 700))
    v[0, :300] = np.where(np.arange(300) % 2 == 0, np.float32(0.0), np.float32(-0.0))  # +0 before -0 ...
    v[1, :300] = np.where(np.arange(300) % 2 == 0, np.float32(-0.0), np.float32(0.0))  # ... and after
    nneg = int((v < 0).sum(1).max())
    for k in (1, nneg + 5, nneg + 150, 600):
        _topk(_dev(dev), v, k)


@pytest.mark.parametrize("dev", DEVICES)
def test_topk_tie_run_across_collection_blocks(dev):
    """The threshold value ~700 times from column 250 on: 6 of them in the first 256-column
    collection block, 256 in the second; the cut falls in the second, then the third block. 100
    values below the threshold, themselves tied."""
    rng = np.random.default_rng(4)
    L, T = 1200, cases.TK_T
    v = (2.0 + rng.random((3, L))).astype(np.float32)
    v[:, 250:950] = 0.5
    low = np.concatenate([np.arange(10, 60), np.arange(1000, 1050)])
    v[:, low] = np.where(np.arange(100) % 2 == 0, np.float32(0.25), np.float32(-4.0))
    first, second = T - 250, 2 * T - 250
    for need in (1, first, first + 1, first + 150, second, second + 1, second + 138, 700):
        _topk(_dev(dev), v, 100 + need)


@pytest.mark.parametrize("dev", DEVICES)
def test_topk_sizes(dev):
    rng = np.random.default_rng(6)
    for L in (1, 255, 256, 257, 513):
        v = rng.integers(-20, 20, (5, L)).astype(np.float32)
        for k in sorted({1, max(1, L - 1), L, L + 1, L + 40}):
            _topk(_dev(dev), v, k, id_base=3)
    v = rng.standard_normal((2, 1300)).astype(np.float32)
    v[:, ::5] = 0.125
    for k in (63, 64, 65, 1023, 1024, 1025):
        _topk(_dev(dev), v, k)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("L,k", [(9000, 8192), (9000, 8193), (16385, 16384), (16384, 16384)])
def test_topk_large_k(dev, L, k):
    """k = 8192 is the last k whose pair buffer fits 64 KiB of dynamic LDS, 8193 the first that
    needs the opt-in; ``TOPK_KMAX`` on L = k + 1 (selected) and L = k (take-all)."""
    assert ops.TOPK_KMAX == 16384
    v = np.random.default_rng(L + k).integers(0, 3000, (1, L)).astype(np.float32)
    _topk(_dev(dev), v, k, id_base=1 << 31)


@pytest.mark.gpu
def test_topk_k_above_kmax_refused(gpu_device):
    v = torch.zeros((1, 17000), device=gpu_device)
    with pytest.raises(ValueError):
        ops.topk_rows(v, ops.TOPK_KMAX + 1)
    ov = torch.empty((1, ops.TOPK_KMAX + 1), device=gpu_device)
    oi = torch.empty((1, ops.TOPK_KMAX + 1), dtype=torch.int64, device=gpu_device)
    rc = native.call_status("srml_topk_rows_f32", v.data_ptr(), 1, v.stride(0), 17000, 17000, None, 0, 0,
                            ops.TOPK_KMAX + 1, ov.data_ptr(), oi.data_ptr(), ops.TOPK_KMAX + 1, 0,
                            native.stream(gpu_device))
    assert rc == -1


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("rows", [1, 5])
def test_topk_slices(dev, rows):
    """L on each side of a slice edge, a last slice shorter than k, ``slice_len`` < k, ids and an
    ``id_base`` above 2^31, a strided row view; the sliced result is bit-identical to one slice."""
    rng = np.random.default_rng(7 + rows)
    s, k = 300, 7
    d = _dev(dev)
    for L in (s - 1, s, s + 1, 2 * s + 1):
        v = rng.integers(0, 25, (rows, L)).astype(np.float32)
        ids = (rng.permutation(rows * L).reshape(rows, L) + (1 << 33)).astype(np.int64)
        for kw in (dict(id_base=(1 << 31) + 11), dict(ids=ids)):
            for strided in (False, True):
                one = _topk(d, v, k, strided=strided, **kw)
                for sl in (s, 4):  # 4 < k: raised to k
                    got = _topk(d, v, k, slice_len=sl, strided=strided, **kw)
                    assert cases.bits_equal(one[0], got[0]) and cases.bits_equal(one[1], got[1])
    v = rng.integers(0, 25, (rows, 2 * s + 40)).astype(np.float32)  # last slice of 40 < k = 65
    _topk(d, v, 65, slice_len=s, id_base=5)


# ------------------------------------------------------------------------------------------
# ops.knn
# ------------------------------------------------------------------------------------------
def _knn_vec(qptr, ldq, iptr, ldi, n):
    """``srml_knn_f32``'s alignment condition (csrc/knn.hip), copied: true -> ``knn_kernel<true>``."""
    return ldq % 4 == 0 and ldi % 4 == 0 and n % 4 == 0 and qptr % 16 == 0 and iptr % 16 == 0


def _offset_rows(X, dev, pad=0):
    """X on ``dev`` as a view one float past a 16-byte boundary, row stride n + pad."""
    m, n = X.shape
    buf = torch.zeros(1 + m * (n + pad), dtype=torch.float32, device=dev)
    v = buf[1:].view(m, n + pad)[:, :n]
    v.copy_(torch.from_numpy(X))
    return v


def _raw_knn(Q, I, k, slices, id_offset=0):
    """``srml_knn_f32`` on the views as they are (no contiguous copy), merged as ``ops.knn`` does."""
    mq, n = Q.shape
    inorm, qnorm = ops.row_sqnorm(I), ops.row_sqnorm(Q)
    od = torch.empty((mq, slices, k), dtype=torch.float32, device=Q.device)
    oi = torch.empty((mq, slices, k), dtype=torch.int64, device=Q.device)
    native.call("srml_knn_f32", Q.data_ptr(), mq, n, Q.stride(0), I.data_ptr(), I.shape[0], I.stride(0),
                inorm.data_ptr(), k, slices, od.data_ptr(), oi.data_ptr(), int(id_offset), native.stream(Q.device))
    od, oi = od.view(mq, slices * k), oi.view(mq, slices * k)
    if slices > 1:
        od, oi = ops.topk_rows(od, k, ids=oi)
    return (od + qnorm.view(-1, 1)).clamp_min(0), oi


N_EDGES = [1, 3, 4, BK - 1, BK, BK + 1, 2 * BK + 1]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", N_EDGES)
def test_knn_lattice_tile_edges(dev, n):
    """mq and mi one short of, on and past the 128 tile, n around the k-tile, k = 1, 63, 64 and past
    the items: keys, ids and tie order equal the oracle exactly (amp 2: most distances tie)."""
    d = _dev(dev)
    Q, I, orc = cases.lattice_case(129, 257, n, amp=2, dups=(3, 127, 128, 256))
    Qt, It = torch.from_numpy(Q).to(d), torch.from_numpy(I).to(d)
    if dev == "cuda":
        assert _knn_vec(Qt.data_ptr(), Qt.stride(0), It.data_ptr(), It.stride(0), n) == (n % 4 == 0)
    for mq in (1, 127, 128, 129):
        for mi in (1, 127, 128, 129, 257):
            sub = orc.sub(mq, mi)
            for k in (1, 63, 64):
                dist, ids = ops.knn(Qt[:mq], It[:mi], k, id_offset=(1 << 31) + 9)
                cases.check_knn(sub, dist, ids, k, id_offset=(1 << 31) + 9, exact=True)
    assert (orc.D[0, [3, 127, 128, 256]] == 0).all()  # bit-identical rows on both sides of the tile edges


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 33])
def test_knn_lattice_inner_product(dev, n):
    d = _dev(dev)
    Q, I, orc = cases.lattice_case(129, 257, n, amp=3, seed=1, inner_product=True)
    Qt, It = torch.from_numpy(Q).to(d), torch.from_numpy(I).to(d)
    zi, zq = torch.zeros(257, device=d), torch.zeros(129, device=d)
    for k in (1, 64):
        dist, ids = ops.knn(Qt, It, k, inorm=zi, qnorm=zq)
        cases.check_knn(orc, dist, ids, k, exact=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, BK, 2 * BK])
def test_knn_scalar_routes(gpu_device, n):
    """``knn_kernel<false>`` reached with n % 4 = 0 by a base pointer one float off and by a row
    stride of n + 1; both routes are proven by the entry point's own alignment condition and are
    bit-identical to ``knn_kernel<true>``."""
    Q, I, orc = cases.lattice_case(129, 257, n, amp=2, dups=(3, 127, 128, 256))
    Qt, It = torch.from_numpy(Q).to(gpu_device), torch.from_numpy(I).to(gpu_device)
    assert _knn_vec(Qt.data_ptr(), n, It.data_ptr(), n, n)
    ref = ops.knn(Qt, It, 64)
    cases.check_knn(orc, ref[0], ref[1], 64, exact=True)
    Qo, Io = _offset_rows(Q, gpu_device), _offset_rows(I, gpu_device)
    assert Qo.is_contiguous() and Io.is_contiguous()  # ops.knn passes them on as they are
    assert not _knn_vec(Qo.data_ptr(), Qo.stride(0), Io.data_ptr(), Io.stride(0), n)
    got = ops.knn(Qo, Io, 64)
    assert cases.bits_equal(ref[0], got[0]) and cases.bits_equal(ref[1], got[1])
    Qs, Is = _offset_rows(Q, gpu_device, pad=1)[:], _offset_rows(I, gpu_device, pad=1)
    assert Qs.stride(0) == n + 1 and not _knn_vec(0, Qs.stride(0), 0, Is.stride(0), n)
    got = _raw_knn(Qs, Is, 64, 1)
    assert cases.bits_equal(ref[0], got[0]) and cases.bits_equal(ref[1], got[1])


@pytest.mark.gpu
def test_knn_raw_slice_counts(gpu_device):
    """1, 2 and 3 slices over 130 items: 128-item slices, the third one empty."""
    Q, I, orc = cases.lattice_case(129, 130, 5, amp=2, dups=(127, 128, 129))
    Qt, It = torch.from_numpy(Q).to(gpu_device), torch.from_numpy(I).to(gpu_device)
    for k in (1, 3, 64):
        outs = []
        for slices in (1, 2, 3):
            dist, ids = _raw_knn(Qt, It, k, slices, id_offset=(1 << 31) + 1)
            cases.check_knn(orc, dist, ids, k, id_offset=(1 << 31) + 1, exact=True)
            outs.append((dist, ids))
        assert all(cases.bits_equal(outs[0][0], o[0]) and cases.bits_equal(outs[0][1], o[1]) for o in outs[1:])


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("mi,edge", [(4097, 2176), (8193, 2816)])
def test_knn_lattice_slices(dev, mi, edge):
    """2 and 3 item slices through ``ops.knn`` (one query block: a slice per 4096 items, slice
    length = the share rounded up to 128); duplicates of the query on both sides of the first tile
    edge and of the first slice edge come back in id order."""
    slices = (mi + 4095) // 4096
    assert edge == -(-(-(-mi // slices)) // 128) * 128
    d = _dev(dev)
    dups = (5, 127, 128, edge - 1, edge, mi - 1)
    Q, I, orc = cases.lattice_case(1, mi, 4, amp=30, dups=dups)
    Qt, It = torch.from_numpy(Q).to(d), torch.from_numpy(I).to(d)
    for k in (1, 6, 64):
        dist, ids = ops.knn(Qt, It, k, id_offset=(1 << 31) + 3)
        cases.check_knn(orc, dist, ids, k, id_offset=(1 << 31) + 3, exact=True)
    assert (ids[0, :6] - ((1 << 31) + 3)).tolist() == list(dups)


def test_knn_host_ties_go_to_the_lower_id():
    """Three stacked copies of 50 random rows: each query's 12 nearest are 4 groups of bit-identical
    rows, which the host form returns in id order as the device does."""
    X = np.random.default_rng(0).standard_normal((50, 8)).astype(np.float32)
    I = torch.from_numpy(np.concatenate([X, X, X]))
    d, ids = ops.knn(torch.from_numpy(X), I, 12)
    g = ids.view(50, 4, 3)
    assert torch.equal(g[:, :, 1], g[:, :, 0] + 50) and torch.equal(g[:, :, 2], g[:, :, 0] + 100), g[0]
    assert (g[:, 0, 0] == torch.arange(50)).all()


GENERIC = [(129, 257, 33, 10), (40, 4097, 4, 64), (130, 300, 65, 63)]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("mq,mi,n,k", GENERIC)
def test_knn_generic_band(dev, mq, mi, n, k):
    d = _dev(dev)
    Q, I, orc = cases.generic_case(mq, mi, n, k)
    dist, ids = ops.knn(torch.from_numpy(Q).to(d), torch.from_numpy(I).to(d), k)
    _note("knn k<=64 %s n=%d" % (dev, n), cases.check_knn(orc, dist, ids, k))


# ---- k > 64 ------------------------------------------------------------------------------
def _count_calls(monkeypatch):
    launches = {}
    real = native.call

    def counting(name, *args):
        launches[name] = launches.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(native, "call", counting)
    return launches


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("k", [65, 130])
def test_knn_large_k_lattice_and_generic(dev, k):
    d = _dev(dev)
    Q, I, orc = cases.lattice_case(129, 257, 33, amp=2, dups=(3, 127, 128, 256))
    dist, ids = ops.knn(torch.from_numpy(Q).to(d), torch.from_numpy(I).to(d), k, id_offset=(1 << 31) + 9)
    cases.check_knn(orc, dist, ids, k, id_offset=(1 << 31) + 9, exact=True)
    dist, ids = ops.knn(torch.from_numpy(Q).to(d), torch.from_numpy(I[:100]).to(d), k)  # k past the items
    cases.check_knn(orc.sub(129, 100), dist, ids, k, exact=True)
    Q, I, orc = cases.generic_case(129, 257, 33, k)
    dist, ids = ops.knn(torch.from_numpy(Q).to(d), torch.from_numpy(I).to(d), k)
    _note("knn k>64 %s n=33" % dev, cases.check_knn(orc, dist, ids, k))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [65, 130])
@pytest.mark.parametrize("kind", ["lattice", "generic"])
def test_knn_large_k_chunked_bit_identical(gpu_device, monkeypatch, k, kind):
    """Two query chunks (129 queries against R = 128) x three item chunks (128, 128 and one
    column), proven by the launch count; every D element is one thread's accumulation in a fixed k
    order, so the chunked result equals the single launch bit for bit."""
    Q, I, orc = (cases.lattice_case(129, 257, 33, amp=2, dups=(3, 127, 128, 256)) if kind == "lattice"
                 else cases.generic_case(129, 257, 33, k))
    Qt, It = torch.from_numpy(Q).to(gpu_device), torch.from_numpy(I).to(gpu_device)
    launches = _count_calls(monkeypatch)
    one = ops.knn(Qt, It, k)
    assert launches["srml_knn_dist_f32"] == 1
    monkeypatch.setattr(ops, "_TOPK_SLICE", 8)               # item chunks of 16 * 8 = 128 columns
    monkeypatch.setattr(ops, "_KNN_DIST_BYTES", 128 * 128 * 4)  # R = 128 query rows
    launches.clear()
    got = ops.knn(Qt, It, k)
    assert launches["srml_knn_dist_f32"] == 6
    cases.check_knn(orc, got[0], got[1], k, exact=kind == "lattice")
    assert cases.bits_equal(one[0], got[0]) and cases.bits_equal(one[1], got[1])


# ------------------------------------------------------------------------------------------
# ops.knn_refine_sort (host form: models.knn._refine_sorted on CPU tensors)
# ------------------------------------------------------------------------------------------
N_REFINE = [1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 1100]


def _positions(mq, k, mi, rng):
    pos = rng.integers(0, mi, (mq, k)).astype(np.int64)
    pos[:, k // 3] = pos[:, 0]          # a repeated position
    pos[0, k // 2] = -1                 # -1 in the middle of a row
    if mq >= 3:
        pos[1] = -1                     # an all -1 row
    return pos


def _strided(a, dev, pad):
    """``a`` as the leading columns of a wider buffer (row stride = columns + pad)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.zeros((a.shape[0], a.shape[1] + pad), dtype=t.dtype)
    buf[:, :a.shape[1]] = t
    return buf.to(dev)[:, :a.shape[1]]


def _refine(dev, Q, X, pos, ip, strided):
    d = _dev(dev)
    if strided:
        Qt, Xt, pt = _strided(Q, d, 3), _strided(X, d, 1), _strided(pos, d, 2)
    else:
        Qt, Xt, pt = torch.from_numpy(Q).to(d), torch.from_numpy(X).to(d), torch.from_numpy(pos).to(d)
    if dev == "cuda":
        r = ops.knn_refine_sort(Qt, Xt, pt, inner_product=ip)
        assert r is not None, "the device form refused fp32 rows"
        return r
    assert ops.knn_refine_sort(Qt, Xt, pt, inner_product=ip) is None
    return mknn._refine_sorted(Qt, Xt, pt, "inner_product" if ip else "sqeuclidean")


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", N_REFINE)
def test_refine_sort_edges(dev, n):
    """n on each side of every register instantiation (64 QT, QT = 1, 2, 4, 8, 16) and in the
    streamed tail; mq around the four waves of a block; k around the 64-column panels. Lattice rows
    (ties keep the candidate order, distances exact), then generic rows within the derived bound."""
    rng = np.random.default_rng(n)
    amp = 2
    Xl, Ql = cases.lattice(60, n, amp, n), cases.lattice(5, n, amp, n + 1)
    Xl[:, n // 2:] = Xl[0, n // 2:]  # rows differ in few coordinates: many exact ties
    Xg, Qg = rng.standard_normal((60, n)).astype(np.float32), rng.standard_normal((5, n)).astype(np.float32)
    worst = [0.0, 0.0]
    for mq in (1, 3, 4, 5):
        for k in (1, 63, 64, 65, 129):
            pos = _positions(mq, k, 60, rng)
            for ip in (False, True):
                strided = (mq + k) % 2 == 1
                d, p = _refine(dev, Ql[:mq], Xl, pos, ip, strided)
                cases.check_refine(Ql[:mq], Xl, pos, d, p, ip, exact=True)
                d, p = _refine(dev, Qg[:mq], Xg, pos, ip, strided)
                worst[ip] = max(worst[ip], cases.check_refine(Qg[:mq], Xg, pos, d, p, ip))
    _note("refine sqeuclidean %s" % dev, worst[0])
    _note("refine inner_product %s" % dev, worst[1])


@pytest.mark.parametrize("dev", DEVICES)
def test_refine_sort_near_duplicates(dev):
    """x and x + 2^-10 e_j at ||x|| = 30: D = 2^-20, held to (n + 4) u D."""
    X = cases.near_duplicates()
    pos = np.tile(np.arange(X.shape[0], dtype=np.int64), (X.shape[0], 1))
    d, p = _refine(dev, X, X, pos, False, False)
    _note("refine near-duplicates %s" % dev, cases.check_refine(X, X, pos, d, p))
    assert (cases._np(d)[:, 0] == 0).all()  # every row against itself


# ------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------
def _model_case(monkeypatch, force_cpu):
    if force_cpu:
        monkeypatch.setenv("SRML_FORCE_CPU", "1")
    n = 6
    Q, I, orc = cases.lattice_case(20, 140, n, amp=2, seed=2, dups=(3, 127, 128, 139))
    for k in (64, 65, 150):
        model = NearestNeighbors(k=k, inputCol="features").fit(DataFrame.from_numpy(I))
        _, _, knn_df = model.kneighbors(DataFrame.from_numpy(Q))
        t = knn_df.toPandas().sort_values("query_unique_id")
        ind = np.stack([np.asarray(v) for v in t["indices"]]).astype(np.int64)
        dist = np.stack([np.asarray(v) for v in t["distances"]]).astype(np.float64)
        kk = min(k, 140)
        assert ind.shape == (20, kk) and np.array_equal(ind, orc.order[:, :kk]), "ids differ from the oracle's"
        # sqrt of a refined squared distance: (n + 4) u D under the root halves, the root and the
        # oracle's own rounding add 2 u
        want = np.sqrt(np.take_along_axis(orc.D, orc.order[:, :kk], 1))
        assert (np.abs(dist - want) <= ((n + 4) / 2 + 2) * cases.U24 * want).all()


def test_model_lattice_host(monkeypatch):
    _model_case(monkeypatch, True)


@pytest.mark.gpu
def test_model_lattice_device(gpu_device, monkeypatch):
    _model_case(monkeypatch, False)


def test_zz_report_ratios():
    """Prints the worst error / bound ratios of this run (the docs table is filled from it)."""
    for path in sorted(RATIOS):
        print("worst ratio %-40s %.3f" % (path, RATIOS[path]))
        assert RATIOS[path] <= 1.0
