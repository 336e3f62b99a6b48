"""``ops.svc_loss_grad`` (hinge / squared hinge) on every dispatch path against an fp64 oracle.

Labels 0 / 1, y' = 2y - 1, z = w.x + b, h = 1 - y'z. hinge: l = max(0, h), r = -y' where h > 0
(strictly: a row on the kink contributes nothing); squared hinge: l = max(0, h)^2, r = -2 y' max(0, h).
out += [X^T r | sum r | sum l].

Bounds (u32 = 2^-24, u64 = 2^-53, gamma_k(u) = k u / (1 - k u); u = unit roundoff of the path's
margins, u_res = that of its residual and gradient accumulation, ``CLASS`` below):

* dz_r = gamma_{n+2}(u) (sum_j |x_rj| |w_j| + |b|): an n-term dot product, the rounding of w to the
  margin precision and the bias add;
* dr_r = 0 for hinge (the residual is exactly -y' or 0 off the kink), 2 dz_r + u_res |r_r| for
  squared hinge (r = -2 y' h is linear in z, then cast to the accumulation type);
* gradient entry c: sum_r |x_rc| dr_r + gamma_{m+2}(u_res) sum_r |x_rc| |r_r|;
* bias gradient: sum_r dr_r + gamma_m(u64) sum_r |r_r|;
* loss: sum_r (1 + 2 |h_r| [squared]) dz_r + gamma_m(u64) sum_r l_r.

A hinge row with 0 < |h_r| <= dz_r could land on either side of the kink; the checker asserts that
no case holds one (``exact_z`` cases, whose margins are exact by construction, have dz = 0). The
u32-margin paths run at n > 16384, where dz is ~1e-3 of sum |x||w|: their inputs keep most of w
small so that the oracle alone satisfies this.

Paths (``ops.svc_path``, asserted in every case) and their classes: ``fused_svc_f32`` (u64, u32: fp64
margins, fp32 residual and register gradient), ``lds_svc_f32`` / ``lds_svc_f64`` / ``csr_svc`` (u64, u64),
``two_pass_svc_f32`` / ``two_pass_deterministic_svc_f32`` (u32, u32), ``two_pass_svc_f64`` and
``torch-cpu`` (u64, u64).

The partial-row workspace holds fp32 columns and an fp64 [gb, loss] tail per block: with
``leave_partials`` the test folds the tail on the device with ``srml_fold_partials_f64`` and the
fp32 columns (which that fp64 fold cannot read) on the host in fp64.
"""
import math

import numpy as np
import pytest
import torch

from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.core.base import CSR
from spark_rapids_ml_nai_amd.ops import native

U32 = 2.0 ** -24
U64 = 2.0 ** -53
LOSSES = ("hinge", "squared_hinge")

CLASS = {
    "torch-cpu": (U64, U64),
    "fused_svc_f32": (U64, U32),
    "lds_svc_f32": (U64, U64),
    "lds_svc_f64": (U64, U64),
    "csr_svc": (U64, U64),
    "two_pass_svc_f32": (U32, U32),
    "two_pass_deterministic_svc_f32": (U32, U32),
    "two_pass_svc_f64": (U64, U64),
}


def gamma(k, u):
    return k * u / (1.0 - k * u)


# ------------------------------------------------------------------------------------------
# the oracle and the checker
class Ref:
    pass


def reference(Xd, y, w, b, squared, kink_active=False):
    """Xd (m, n) fp64 = the device's X widened, y (m) in {0, 1}, w (n), b fp64; 80-bit sums."""
    ft = np.longdouble
    Xh = Xd.astype(ft)
    z = Xh @ w.astype(ft) + ft(b)
    s = 2 * y.astype(ft) - 1
    h = 1 - s * z
    act = (h >= 0) if kink_active else (h > 0)
    ref = Ref()
    ref.m, ref.n, ref.squared = Xd.shape[0], Xd.shape[1], squared
    ref.h = h.astype(np.float64)
    ref.r = np.where(act, -2 * s * h if squared else -s, 0)
    ref.l = np.where(act, h * h if squared else h, 0)
    ref.G, ref.gb, ref.loss = ref.r @ Xh, ref.r.sum(), ref.l.sum()
    ref.Xabs = np.abs(Xd)
    ref.A = ref.Xabs @ np.abs(w) + abs(b)
    return ref


def flat(G, gb, loss):
    return np.concatenate([np.asarray(G, dtype=np.float64).reshape(-1), [float(gb)], [float(loss)]])


def bounds(ref, u, u_res, exact_z=False):
    """Tolerance of [grad w | grad b | loss] (module docstring); asserts that no hinge row sits within
    dz of the kink."""
    m, n = ref.m, ref.n
    dz = np.zeros(m) if exact_z else gamma(n + 2, u) * ref.A
    rabs = np.abs(ref.r).astype(np.float64)
    if ref.squared:
        dr = 2 * dz + u_res * rabs
    else:
        near = (ref.h != 0) & (np.abs(ref.h) <= dz)
        assert not near.any(), "a hinge row within dz of the kink: rows %s" % np.nonzero(near)[0][:5]
        dr = np.zeros(m)
    tG = ref.Xabs.T @ dr + gamma(m + 2, u_res) * (ref.Xabs.T @ rabs)
    tb = dr.sum() + gamma(m, U64) * rabs.sum()
    tl = ((1 + (2 * np.abs(ref.h) if ref.squared else 0)) * dz).sum() + gamma(m, U64) * float(ref.l.sum())
    return np.concatenate([tG, [tb], [tl]])


def check(got, out0, ref, u, u_res, exact_z=False):
    """(within the bound, largest error / bound) of ``got`` = ``out0`` + the oracle's data term."""
    exp = flat(ref.G, ref.gb, ref.loss)
    tol = bounds(ref, u, u_res, exact_z) + gamma(ref.m + 2, U64) * np.abs(out0)
    err = np.abs((got.astype(np.longdouble) - out0.astype(np.longdouble)) - exp.astype(np.longdouble))
    ok = bool(np.isfinite(got).all() and (err <= tol).all())
    pos = tol > 0
    return ok, float((err[pos] / tol[pos]).max()) if pos.any() else 0.0


# ------------------------------------------------------------------------------------------
# inputs
def prefill(N):
    i = torch.arange(N, dtype=torch.float64)
    return (0.25 + 0.5 * torch.frac(i * 0.6180339887498949)) * (1.0 - 2.0 * (i % 2))


def inputs(m, n, kind, dtype, seed, sparse=None):
    """(X torch (dtype), y fp32, w (n) fp64, b) for a label / margin kind: ``mixed`` (margins of both
    signs around the kink), ``all_active`` (|z| < 1), ``none_active`` (labels agree, y'z > 1),
    ``zeros`` / ``ones`` (one class). Most of w is small, a few entries carry the margin (see the
    module docstring); ``sparse``: the CSR pattern ("rows": empty rows + one dense row)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((m, n))
    if sparse == "rows":
        mask = rng.random((m, n)) < min(1.0, 6.0 / n)
        mask[::3] = False  # empty rows
        mask[m - 1] = True  # one dense row
        X *= mask
    w = 0.05 * rng.standard_normal(n) / math.sqrt(n)
    big = np.unique(np.concatenate([rng.integers(0, n, 3), [n - 1]]))
    w[big] = rng.choice([-1.5, 1.5], len(big)) * rng.uniform(0.6, 1.0, len(big))
    b = 0.3
    X = torch.from_numpy(np.ascontiguousarray(X)).to(dtype)
    Xd = X.double().numpy()
    if kind == "all_active":
        sc = 0.5 / max(np.abs(Xd @ w).max(), 1e-300)
        w, b = w * sc, 0.25
        y = rng.random(m) < 0.5
    elif kind == "none_active":
        # rows scaled so that |w.x| lies in [4, 6], b = 2 (an empty CSR row has z = b), labels agree
        # with the sign of z: y'z >= 2 on every row
        b = 2.0
        t = rng.uniform(4.0, 6.0, m) / np.maximum(np.abs(Xd @ w), 1e-300)
        X = torch.from_numpy(Xd * np.minimum(t, 1e6)[:, None]).to(dtype)
        y = X.double().numpy() @ w + b > 0
    elif kind == "zeros":
        y = np.zeros(m)
    elif kind == "ones":
        y = np.ones(m)
    else:
        y = rng.random(m) < 0.45
    return X, torch.from_numpy(np.asarray(y, dtype=np.float32)), w, float(b)


def clear_inputs(m, n, kind, dtype, seed, sparse, u):
    """``inputs`` from the first seed of seed, seed + 1000, ... whose oracle has no hinge row within
    dz of the kink at margin precision u: the case is chosen by the oracle alone, and the checker
    still asserts it."""
    for k in range(64):
        X, y, w, b = inputs(m, n, kind, dtype, seed + 1000 * k, sparse)
        ref = reference(X.double().numpy(), y.numpy(), w, b, False)
        if not ((ref.h != 0) & (np.abs(ref.h) <= gamma(n + 2, u) * ref.A)).any():
            return X, y, w, b
    raise AssertionError("no seed keeps every row off the kink")


def to_csr(X, dev):
    nz = X != 0
    indptr = torch.zeros(X.shape[0] + 1, dtype=torch.int64)
    indptr[1:] = nz.sum(1).cumsum(0)
    cols = nz.nonzero()[:, 1].to(torch.int32)
    return CSR(indptr=indptr.to(dev), indices=cols.to(dev), data=X[nz].to(dev), shape=tuple(X.shape))


def expected_path(n, dtype, dev, csr=False, det=False):
    if dev.type == "cpu":
        return "torch-cpu"
    if csr:
        return "csr_svc"
    f32 = dtype == torch.float32
    if det and f32:
        return "two_pass_deterministic_svc_f32"
    if f32 and n <= 4096:
        return "fused_svc_f32"
    if n <= 16384:
        return "lds_svc_f32" if f32 else "lds_svc_f64"
    return "two_pass_svc_f32" if f32 else "two_pass_svc_f64"


def layout(X, how):
    """The same matrix behind an unaligned row stride (ld = n + 1) or a base pointer one element off."""
    m, n = X.shape
    if how == "stride":
        buf = torch.full((m, n + 1), 7.0, dtype=X.dtype, device=X.device)
        buf[:, :n] = X
        v = buf[:, :n]
        assert v.stride(0) == n + 1
        return v
    if how == "offset":
        buf = torch.full((m * n + 1,), 7.0, dtype=X.dtype, device=X.device)
        buf[1:] = X.reshape(-1)
        v = buf[1:].view(m, n)
        assert v.data_ptr() % 16 != 0
        return v
    return X


KINDS = ("mixed", "all_active", "none_active", "zeros", "ones")


def exercise(dev, m, n, dtype, path, *, kinds=KINDS, sparse=None, how=None, twice=False, seed=None):
    """One shape through ``ops.svc_loss_grad`` for both losses and every kind: the expected path, the
    bound on out - pre-fill, ``none_active`` leaving out bit-identical, flag = 1 leaving it untouched."""
    u, u_res = CLASS[path]
    out0 = prefill(n + 2)
    for kind in kinds:
        X, y, w, b = clear_inputs(m, n, kind, dtype, 7 * m + n if seed is None else seed, sparse, u)
        Xd = X.double().numpy()
        Xv = to_csr(X, dev) if sparse else layout(X.to(dev), how)
        assert ops.svc_path(Xv) == path
        yv = y.to(dev)
        wv, bv = torch.from_numpy(w).to(dev), torch.tensor([b], dtype=torch.float64, device=dev)
        for loss in LOSSES:
            what = "%s %s m=%d n=%d %s %s %s" % (path, loss, m, n, kind, sparse or "dense", how or "")
            ref = reference(Xd, y.numpy(), w, b, loss == "squared_hinge")
            out = out0.clone().to(dev)
            ops.svc_loss_grad(Xv, yv, wv, bv, out, loss=loss)
            got = out.cpu().numpy()
            ok, ratio = check(got, out0.numpy(), ref, u, u_res)
            print("SVC-RATIO %-60s %.3g" % (what, ratio))
            assert ok, "%s: error / bound = %.3g" % (what, ratio)
            if kind == "none_active":
                assert float(np.abs(ref.r).sum()) == 0.0, what
                assert torch.equal(out.cpu(), out0), "no active row, but out changed: " + what
            if twice:
                out_b = out0.clone().to(dev)
                ops.svc_loss_grad(Xv, yv, wv, bv, out_b, loss=loss)
                assert torch.equal(out_b, out), what
            if dev.type != "cpu":
                flag = torch.ones(1, dtype=torch.int32, device=dev)
                out = out0.clone().to(dev)
                ops.svc_loss_grad(Xv, yv, wv, bv, out, flag, loss=loss)
                assert torch.equal(out.cpu(), out0), "flag = 1 changed out: " + what


# ------------------------------------------------------------------------------------------
# the kink: exact margins
def kink_inputs(n, dtype):
    """Small-integer X, w, b: every margin is exact in fp32 and fp64. Per label, rows with y'z = 1
    exactly (inactive: nothing), 1 + 2^-20 (inactive), 1 - 2^-20 (active, h = 2^-20), and plain
    active / inactive rows. Columns 0..3 carry the values, the rest of X is zero."""
    e = 2.0 ** -20
    rows, ys, tag = [], [], []
    for yv in (0.0, 1.0):
        s = 2 * yv - 1
        for zt, t in ((1.0, "kink"), (1.0 + e, "above"), (1.0 - e, "below"), (-2.0, "active"), (3.0, "inactive")):
            zi = float(round(zt))  # w = [1, 2, -1, 1], b = 1: z = (s zi - 3) + 4 - 2 + s (zt - zi) + 1 = s zt
            x = np.zeros(n)
            x[0], x[1], x[2], x[3] = s * zi - 3.0, 2.0, 2.0, s * (zt - zi)
            rows.append(x)
            ys.append(yv)
            tag.append(t)
    X = torch.from_numpy(np.array(rows)).to(dtype)
    w = np.zeros(n)
    w[:4] = [1.0, 2.0, -1.0, 1.0]
    return X, torch.tensor(ys, dtype=torch.float32), w, 1.0, tag


def exercise_kink(dev, n, dtype, path, sparse=False):
    u, u_res = CLASS[path]
    X, y, w, b, tag = kink_inputs(n, dtype)
    Xd = X.double().numpy()
    s = 2 * y.numpy().astype(np.float64) - 1
    yz = s * (Xd @ w + b)
    e = 2.0 ** -20
    want = {"kink": 1.0, "above": 1.0 + e, "below": 1.0 - e, "active": -2.0, "inactive": 3.0}
    assert all(yz[i] == want[t] for i, t in enumerate(tag))  # the construction is exact
    out0 = prefill(n + 2)
    wv, bv = torch.from_numpy(w).to(dev), torch.tensor([b], dtype=torch.float64, device=dev)
    quiet = np.array([t in ("kink", "above", "inactive") for t in tag])
    for rows in (np.ones(len(tag), bool), quiet):
        Xs, ys = X[torch.from_numpy(rows)], y[torch.from_numpy(rows)]
        Xv = to_csr(Xs, dev) if sparse else Xs.to(dev)
        assert ops.svc_path(Xv) == path
        for loss in LOSSES:
            ref = reference(Xs.double().numpy(), ys.numpy(), w, b, loss == "squared_hinge")
            out = out0.clone().to(dev)
            ops.svc_loss_grad(Xv, ys.to(dev), wv, bv, out, loss=loss)
            ok, ratio = check(out.cpu().numpy(), out0.numpy(), ref, u, u_res, exact_z=True)
            assert ok, "kink %s %s n=%d: error / bound = %.3g" % (path, loss, n, ratio)
            if rows is quiet:  # rows on and above the kink: loss 0, zero gradient
                assert torch.equal(out.cpu(), out0), "a row on the kink contributed: %s %s n=%d" % (path, loss, n)


# ------------------------------------------------------------------------------------------
# shapes
def rows_per_block():
    """Rows one block of the fused kernels' grid owns at small m, read from ``srml_logreg_fold_parts``."""
    L = native.lib()
    for m in range(1, 4097):
        if int(L.srml_logreg_fold_parts(m)) == 1 and int(L.srml_logreg_fold_parts(m + 1)) == 2:
            return m
    raise AssertionError("no block edge below 4096 rows")


M_LIST = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257]
N_LIST = [1, 3, 4, 8, 128, 132, 256, 260, 508, 512, 516, 1020, 1024, 1028, 4092, 4096, 4100, 16380, 16384, 16388]


def m_cases():
    rpb = rows_per_block()
    return sorted(set(M_LIST + [rpb - 1, rpb + 1, 513]))  # 513: two blocks of the narrow kernel


# ------------------------------------------------------------------------------------------
# CPU: the checker itself, and the torch-cpu twin through the same matrix
def test_checker_rejects_faults():
    m, n = 40, 12
    X, y, w, b = inputs(m, n, "mixed", torch.float64, 3)
    Xd = X.numpy()
    zero = np.zeros(n + 2)
    for squared in (False, True):
        ref = reference(Xd, y.numpy(), w, b, squared)
        assert np.abs(ref.r).sum() > 0
        assert check(flat(ref.G, ref.gb, ref.loss), zero, ref, U64, U32)[0]
        act = np.nonzero(ref.r)[0]
        keep = np.ones(m, bool)
        keep[act[0]] = False  # a dropped row
        d = reference(Xd[keep], y.numpy()[keep], w, b, squared)
        assert not check(flat(d.G, d.gb, d.loss), zero, ref, U64, U32)[0], "dropped row"
    # hinge residuals returned for squared hinge
    ref = reference(Xd, y.numpy(), w, b, True)
    hin = reference(Xd, y.numpy(), w, b, False)
    assert not check(flat(hin.G, hin.gb, ref.loss), zero, ref, U64, U32)[0], "hinge residuals for squared hinge"
    # the kink taken as active
    Xk, yk, wk, bk, tag = kink_inputs(8, torch.float64)
    ref = reference(Xk.numpy(), yk.numpy(), wk, bk, False)
    bad = reference(Xk.numpy(), yk.numpy(), wk, bk, False, kink_active=True)
    z8 = np.zeros(10)
    assert check(flat(ref.G, ref.gb, ref.loss), z8, ref, U64, U32, exact_z=True)[0]
    assert not check(flat(bad.G, bad.gb, bad.loss), z8, ref, U64, U32, exact_z=True)[0], "kink taken as active"
    # a row within dz of the kink is refused, not skipped
    near = reference(np.array([[1.0]]), np.array([1.0]), np.array([1.0 - 1e-17]), 0.0, False)
    near.h = np.array([1e-17])
    with pytest.raises(AssertionError):
        bounds(near, U64, U64)


_CPU = torch.device("cpu")


@pytest.mark.parametrize("part", range(4))
def test_torch_cpu_matrix(part):
    for n in N_LIST[part::4]:
        for m in (1, 5, 65) if n < 16380 else (1, 5, 33):
            exercise(_CPU, m, n, torch.float32, "torch-cpu")
    for m in m_cases()[part::4]:
        exercise(_CPU, m, 8, torch.float64, "torch-cpu")
        exercise(_CPU, m, 37, torch.float32, "torch-cpu", sparse="rows")


def test_torch_cpu_kink():
    for n in (4, 8, 1028):
        exercise_kink(_CPU, n, torch.float32, "torch-cpu")
        exercise_kink(_CPU, n, torch.float64, "torch-cpu", sparse=True)


@pytest.mark.parametrize("sparse", [None, "rows"])
@pytest.mark.parametrize("m,n", [(1, 1), (5, 3), (65, 37), (300, 8)])
def test_exact_mode_is_split_invariant(m, n, sparse):
    """``exact=(xmax, m_total)`` on the torch-cpu path: the rows summed in one piece, in two and in
    three pieces (pieces added in either order) give the same bits, within the oracle's bound widened
    by the grid: each of the m terms of a sum moves by at most 2^-53 of a power of two >= the bound
    that ``_svc_exact_cpu`` derives, itself < 2 x that bound; the margins likewise."""
    for kind in ("mixed", "all_active", "zeros"):
        X, y, w, b = clear_inputs(m, n, kind, torch.float64, 5 * m + n, sparse, 4 * (n + 2) * U64)
        Xd = X.numpy()
        xmax = torch.from_numpy(np.abs(Xd).max(0))
        wv, bv = torch.from_numpy(w), torch.tensor([b], dtype=torch.float64)
        bz = float(np.abs(Xd).max(0) @ np.abs(w))
        hb = 2.0 + bz + abs(b)
        for loss in LOSSES:
            sq = loss == "squared_hinge"
            ref = reference(Xd, y.numpy(), w, b, sq)
            rb = 2 * hb if sq else 1.0
            dz = 2 * n * U64 * bz  # n terms, each moved by <= 2^-53 2^e, 2^e < 2 bz
            grid = np.concatenate([2 * m * U64 * m * rb * xmax.numpy(), [2 * m * U64 * m * rb],
                                   [2 * m * U64 * m * (hb * hb if sq else hb)]])
            # a margin moved by dz moves r by 2 dz (squared) and the loss by (1 + 2 |h|) dz
            dzt = np.concatenate([np.abs(Xd).sum(0) * 2 * dz * sq, [2 * dz * m * sq], [(1 + 2 * hb * sq) * dz * m]])
            outs = []
            for cuts in ([0, m], [0, m // 2, m], [0, m // 3, m // 2, m]):
                parts = []
                for r0, r1 in zip(cuts[:-1], cuts[1:]):
                    Xp = to_csr(X[r0:r1], _CPU) if sparse else X[r0:r1]
                    o = torch.zeros(n + 2, dtype=torch.float64)
                    ops.svc_loss_grad(Xp, y[r0:r1], wv, bv, o, loss=loss, exact=(xmax, m))
                    parts.append(o)
                outs.append(sum(parts[1:], parts[0]))
                outs.append(sum(reversed(parts[:-1]), parts[-1]))
            for o in outs[1:]:
                assert torch.equal(o, outs[0]), (kind, loss, m, n)
            tol = bounds(ref, U64, U64) + grid + dzt
            err = np.abs(outs[0].numpy().astype(np.longdouble) - flat(ref.G, ref.gb, ref.loss).astype(np.longdouble))
            assert (err <= tol).all(), (kind, loss, float((err / np.maximum(tol, 1e-300)).max()))


def test_bad_loss_raises():
    X, y, w, b = inputs(4, 3, "mixed", torch.float32, 1)
    with pytest.raises(ValueError):
        ops.svc_loss_grad(X, y, torch.from_numpy(w), torch.tensor([b], dtype=torch.float64),
                          torch.zeros(5, dtype=torch.float64), loss="logistic")


# ------------------------------------------------------------------------------------------
# GPU: every dispatch path
@pytest.mark.gpu
@pytest.mark.parametrize("n", N_LIST)
def test_dense_f32_by_n(gpu_device, n):
    """Both sides of every switch in n: the narrow kernel's lane groups (128 / 132: G = 2 -> 4, whose
    support-vector instantiation has its own ring depth; 256 / 260: G = 4 -> 8), narrow (<= 512), generic /
    prefetching (1024), fused -> LDS (4096), LDS -> two-pass (16384)."""
    path = expected_path(n, torch.float32, gpu_device)
    for m in (1, 5, 65) if n < 16380 else (1, 5, 65, 70):
        exercise(gpu_device, m, n, torch.float32, path)


@pytest.mark.gpu
@pytest.mark.parametrize("m", m_cases())
def test_dense_f32_by_m(gpu_device, m):
    """Row counts around the 4-row, 16-row and per-block steps on the narrow (n = 8, 256; 516 is generic),
    prefetching (1028), LDS (4100) and two-pass kernels."""
    for n in (8, 256, 516, 1028, 4100) + ((16388,) if m <= 70 else ()):
        exercise(gpu_device, m, n, torch.float32, expected_path(n, torch.float32, gpu_device),
                 kinds=("mixed", "none_active"))


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["stride", "offset"])
def test_dense_f32_unaligned(gpu_device, how):
    """ld = n + 1 / a base pointer one element off: scalar tails, narrow and prefetching kernels ineligible."""
    for m, n in ((5, 8), (65, 8), (17, 512), (65, 516), (17, 1028), (65, 2048), (17, 4100)):
        exercise(gpu_device, m, n, torch.float32, expected_path(n, torch.float32, gpu_device), how=how,
                 kinds=("mixed", "none_active"))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n", [(1, 8), (65, 8), (17, 4100), (5, 16384), (257, 516), (5, 16388), (70, 16388)])
def test_dense_f64(gpu_device, m, n):
    """``lds_svc_f64`` up to the 128 KiB of LDS at n = 16384, ``two_pass_svc_f64`` past it."""
    exercise(gpu_device, m, n, torch.float64, expected_path(n, torch.float64, gpu_device))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("m,n", [(1, 5), (3, 37), (65, 37), (257, 300), (64, 4100)])
def test_csr(gpu_device, m, n, dtype):
    """Empty rows, one dense row, m < 4."""
    exercise(gpu_device, m, n, dtype, "csr_svc", sparse="rows")


@pytest.mark.gpu
@pytest.mark.parametrize("m,n", [(1, 8), (65, 516), (257, 1028), (513, 8), (70, 16388)])
def test_deterministic(gpu_device, monkeypatch, m, n):
    """Within the bound, and bit-identical on a second call."""
    monkeypatch.setenv("SRML_DETERMINISTIC", "1")
    exercise(gpu_device, m, n, torch.float32, "two_pass_deterministic_svc_f32", kinds=("mixed", "none_active"),
             twice=True)


@pytest.mark.gpu
def test_kink(gpu_device, monkeypatch):
    """Rows exactly on the kink contribute nothing on every path; rows 2^-20 on either side do what
    their side says."""
    for n in (4, 8, 516, 1028, 4100, 16388):
        exercise_kink(gpu_device, n, torch.float32, expected_path(n, torch.float32, gpu_device))
    for n in (8, 4100, 16388):
        exercise_kink(gpu_device, n, torch.float64, expected_path(n, torch.float64, gpu_device))
    for dt in (torch.float32, torch.float64):
        exercise_kink(gpu_device, 37, dt, "csr_svc", sparse=True)
    monkeypatch.setenv("SRML_DETERMINISTIC", "1")
    for n in (8, 1028):
        exercise_kink(gpu_device, n, torch.float32, "two_pass_deterministic_svc_f32")


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 17, 800, 1057])
def test_partial_rows(gpu_device, m):
    """The prefetching kernel with the fit's partial-row workspace: folded inside the call, and left
    for the consumer (``leave_partials``), equal the atomic flush within the bound; accumulate-into-out
    and flag semantics hold on both."""
    dev, n = gpu_device, 1028
    X, y, w, b = clear_inputs(m, n, "mixed", torch.float32, 11 * m, None, U64)
    Xv, yv = X.to(dev), y.to(dev)
    ws = ops.logreg_workspace(Xv)
    assert ws is not None and ops.svc_path(Xv) == "fused_svc_f32"
    parts, wst = ops.logreg_fold_layout(Xv)
    assert ws.numel() == parts * wst and wst % 2 == 0
    wv, bv = torch.from_numpy(w).to(dev), torch.tensor([b], dtype=torch.float64, device=dev)
    out0 = prefill(n + 2)
    for loss in LOSSES:
        ref = reference(X.double().numpy(), y.numpy(), w, b, loss == "squared_hinge")
        out = out0.clone().to(dev)
        ops.svc_loss_grad(Xv, yv, wv, bv, out, loss=loss, ws=ws)
        ok, ratio = check(out.cpu().numpy(), out0.numpy(), ref, U64, U32)
        assert ok, "folded %s m=%d: %.3g" % (loss, m, ratio)
        ws.fill_(float("nan"))
        out = out0.clone().to(dev)
        ops.svc_loss_grad(Xv, yv, wv, bv, out, loss=loss, ws=ws, leave_partials=True)
        assert torch.equal(out.cpu(), out0), "leave_partials wrote into out"
        tail = torch.zeros(2, dtype=torch.float64, device=dev)
        wd = ws.view(torch.float64)  # (parts, wst / 2): the last two doubles of a row are [gb, loss]
        native.call("srml_fold_partials_f64", wd.data_ptr() + 8 * (wst // 2 - 2), parts, wst // 2, 2, 2,
                    tail.data_ptr(), 2, 1, None, native.stream(dev))
        cols = ws.view(parts, wst)[:, :n].double().sum(0)
        got = out0.numpy() + np.concatenate([cols.cpu().numpy(), tail.cpu().numpy()])
        ok, ratio = check(got, out0.numpy(), ref, U64, U32)
        assert ok, "left partials %s m=%d: %.3g" % (loss, m, ratio)
        flag = torch.ones(1, dtype=torch.int32, device=dev)
        out = out0.clone().to(dev)
        ops.svc_loss_grad(Xv, yv, wv, bv, out, flag, loss=loss, ws=ws)
        assert torch.equal(out.cpu(), out0), "flag = 1 changed out"
