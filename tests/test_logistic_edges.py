"""Every dispatch edge of the logistic loss/gradient kernels against a tail-accurate reference and a
derived forward error bound.

``ops.logistic_loss_grad`` (with ``ops.logistic_loss_grad_multi`` and ``ops.logreg_binary_loss_grad``)
dispatches on n (512 / 1024 / 4096 / 16384), n % 4 and alignment, K (1 / 3 / 5 / 16 / 32-class
panels), dtype, CSR or dense, ``SRML_LOGREG_FUSED`` and ``SRML_DETERMINISTIC``; every kernel has its
own row grouping. The cases here sit on both sides of each threshold, below one block / one row
group, at m < K, with empty and dense CSR rows, and in four margin regimes (benign, wide,
saturated-correct, extreme) with mixed and single-class labels. Only the default dispatch is tested:
the knobs read once per process (``SRML_LOGREG_NARROW`` / ``BLOCKS`` / ``FOLD``) would need a child
process each; the line-search margin cache stays with the fit-level tests in ``test_qn.py``.

Oracle. The reference is computed on the CPU from the inputs exactly as the device sees them
(``X.double()`` of the fp32 / fp64 tensor, fp64 W and b): in 80-bit ``longdouble`` for the fp64
class, whose bound is of the order of the fp64 rounding of the reference itself, in fp64 otherwise.
The binary residual is tail-accurate (``(1 - y) - q`` for z >= 0, ``q - y`` for z < 0, q = e/(1+e),
e = exp(-|z|); loss ``max(z, 0) - y z + log1p(e)``), the softmax goes through logsumexp. Every output
is compared elementwise with a forward bound. With u32 = 2^-24, u64 = 2^-53, g_k(u) = k u / (1 - k u):

    dz_r   = g_{n+2}(u64) max_k (sum_j |x_rj||w_kj| + |b_k|)            fp64 margins
           = g_{n+2}(u32) max_k sum_j |x_rj||w_kj| + u32 max_k |b_k|    fp32 margins
    dr_r   = 16 u_res + dz_r                (sigmoid / softmax have slope <= 1 in the margins)
    grad   tol[k, c] = sum_r |x_rc| dr_r + g_{m+2}(u_acc) sum_r |x_rc||r_rk|
    bias   tol[k]    = sum_r dr_r + g_m(u64) sum_r |r_rk|
    loss   tol       = sum_r (dz_r + 32 u_res max(1, log K)) + g_m(u64) sum_r |l_r|

plus g_{m+2}(u64) |out0| for the value the call adds into (at most one rounding of the running sum
per block partial, and there are at most m of them). The 16 and 32 are caps for the handful of
roundings of a fast exp, an add, a divide and the fp32 store of R (resp. ``__logf`` / ``log1pf``), not
measurements.

Accuracy classes (u_res = u_acc):
  fp32: every path fed fp32 data, and the CSR fp64 multinomial paths (``csr_spmm`` / ``csr_wide`` on
        fp64 values run the fp32 SpMM and the fp32 residual kernel).
  fp64: ``lds_binary_f64``, ``two_pass_binary_f64``, ``two_pass_multinomial_f64`` (K <= 16 and K > 16),
        ``csr_binary`` on fp64 values, the eager fall-backs (``torch-cpu``, ``logreg_binary_loss_grad``
        past n = 4096).
fp64 margins: ``fused_binary_f32``, ``lds_binary_*``, ``csr_binary``, every dense fp64 path; fp32
margins: every ``two_pass_*_f32``, ``fused_multinomial_f32``, ``csr_spmm``, ``csr_wide``, the
multi-model passes.

Largest observed error / bound per path on an MI355X (``pytest -s`` prints them with the case):
  fused_binary_f32 0.11 (the same through logreg_binary_loss_grad), lds_binary_f32 0.061,
  two_pass_binary_f32 4e-6, two_pass_multinomial_f32 0.37, fused_multinomial_f32 0.37,
  two_pass_wide_f32 0.062, two_pass_deterministic_f32 0.032, multi two-pass 0.19, multi fused 0.17,
  csr_binary fp32 0.065, csr_spmm 0.47, csr_wide 0.28, lds_binary_f64 0.059, two_pass_binary_f64 0.003,
  two_pass_multinomial_f64 0.30, csr_binary fp64 0.35, eager fp64 on the device 1.3e-5, torch-cpu 0.58.
With the fp32 sigmoid / log1p that the binary fp64 kernels shared with the fp32 ones before
``logistic_terms_f64``: lds_binary_f64 7.5e6, two_pass_binary_f64 6.2e2, csr_binary fp64 1.1e7.
"""
import math

import numpy as np
import pytest
import torch

from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.core.base import CSR

U32 = 2.0 ** -24
U64 = 2.0 ** -53

# path -> (unit roundoff of the margins, unit roundoff of the residual and the accumulation)
CLASS = {
    "torch-cpu": (U64, U64),
    "eager_f64": (U64, U64),  # logreg_binary_loss_grad past n = 4096
    "fused_binary_f32": (U64, U32),
    "lds_binary_f32": (U64, U32),
    "lds_binary_f64": (U64, U64),
    "two_pass_binary_f32": (U32, U32),
    "two_pass_binary_f64": (U64, U64),
    "two_pass_multinomial_f32": (U32, U32),
    "fused_multinomial_f32": (U32, U32),
    "two_pass_wide_f32": (U32, U32),
    "two_pass_deterministic_f32": (U32, U32),
    "two_pass_multinomial_f64": (U64, U64),
    "csr_binary_f32": (U64, U32),
    "csr_binary_f64": (U64, U64),
    "csr_spmm": (U32, U32),  # fp32 and fp64 values alike: fp32 SpMM, fp32 residual kernel
    "csr_wide": (U32, U32),
    "multi_fused_f32": (U32, U32),
    "multi_two_pass_f32": (U32, U32),
}

_worst = {}


def _record(path, ratio, what):
    if ratio >= _worst.get(path, (-1.0, ""))[0]:
        _worst[path] = (float(ratio), what)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_worst):
        print("\nEDGE-RATIO %-28s %.3g  (%s)" % ((k,) + _worst[k]), end="")
    print()


def gamma(k, u):
    return k * u / (1.0 - k * u)


# ------------------------------------------------------------------------------------------
# the oracle
class Ref:
    """G (K, n), gb (K), loss (1 softmax / K sigmoid models) with their bounds' ingredients."""


def reference(Xd, y, W, b, softmax, hp):
    """Xd (m, n) fp64 ndarray = the device's X widened; W (K, n), b (K) fp64; y (m) class labels.
    softmax: one K-class model, else K independent sigmoid models. hp: 80-bit arithmetic."""
    ft = np.longdouble if hp else np.float64
    m, n = Xd.shape
    K = W.shape[0]
    Xh, Wh, bh = Xd.astype(ft), W.astype(ft), b.astype(ft)
    Z = Xh @ Wh.T + bh
    rows = np.arange(m)
    if softmax:
        yi = y.astype(np.int64)
        zmax = Z.max(1, keepdims=True)
        lse = zmax[:, 0] + np.log(np.exp(Z - zmax).sum(1))
        R = np.exp(Z - lse[:, None])
        R[rows, yi] = 0
        R[rows, yi] = -R.sum(1)  # p_y - 1 as minus the other classes' mass: no cancellation
        L = (lse - Z[rows, yi])[:, None]
    else:
        yy = y.astype(ft)[:, None]
        e = np.exp(-np.abs(Z))
        q = e / (1 + e)
        R = np.where(Z >= 0, (1 - yy) - q, q - yy)
        L = np.maximum(Z, 0) - yy * Z + np.log1p(e)
    r = Ref()
    r.m, r.n, r.K, r.softmax = m, n, K, softmax
    r.Z, r.R, r.L = Z, R, L
    r.G = R.T @ Xh
    r.gb = R.sum(0)
    r.loss = L.sum(0)
    r.Xabs = np.abs(Xd)
    r.A = r.Xabs @ np.abs(W).T
    r.babs = np.abs(b)
    return r


def bounds(ref, u_margin, u_res):
    """(tol G (K, n), tol gb (K), tol loss) of the module docstring, fp64."""
    m, n = ref.m, ref.n
    if u_margin == U64:
        dz = gamma(n + 2, U64) * (ref.A + ref.babs[None, :]).max(1)
    else:
        dz = gamma(n + 2, U32) * ref.A.max(1) + U32 * ref.babs.max()
    dr = 16 * u_res + dz
    Rabs = np.abs(ref.R).astype(np.float64)
    tG = (ref.Xabs.T @ dr)[None, :] + gamma(m + 2, u_res) * (Rabs.T @ ref.Xabs)
    tb = dr.sum() + gamma(m, U64) * Rabs.sum(0)
    logk = max(1.0, math.log(ref.K)) if ref.softmax else 1.0
    tl = (dz + 32 * u_res * logk).sum() + gamma(m, U64) * np.abs(ref.L).astype(np.float64).sum(0)
    return tG, tb, tl


def flat(G, gb, loss):
    """Layout of ``logistic_loss_grad``'s out: [grad W (K n, class-major) | grad b (K) | loss]."""
    return np.concatenate([np.asarray(G).reshape(-1), np.asarray(gb).reshape(-1), np.asarray(loss).reshape(-1)])


def rows(G, gb, loss):
    """Layout of ``logistic_loss_grad_multi``'s out: one row [grad w_j | grad b_j | loss_j] per model."""
    return np.concatenate([np.asarray(G), np.asarray(gb)[:, None], np.asarray(loss)[:, None]], 1)


def compare(got, out0, exp, tol, m):
    """(within the bound, largest error / bound) of ``got`` = ``out0`` + the data term ``exp``."""
    err = np.abs((got.astype(np.longdouble) - out0.astype(np.longdouble)) - exp.astype(np.longdouble))
    tol = tol + gamma(m + 2, U64) * np.abs(out0)
    ok = bool(np.isfinite(got).all() and (err <= tol).all())
    pos = tol > 0
    ratio = float((err[pos] / tol[pos]).max()) if pos.any() else 0.0
    return ok, ratio


# ------------------------------------------------------------------------------------------
# inputs
def base(m, n, K, seed, csr_kind=None):
    """(X0 (m, n), w0 (K, n) with unit-variance margins, b0 (K)) fp64, fixed by the seed."""
    rng = np.random.default_rng(seed)
    X0 = rng.standard_normal((m, n))
    if csr_kind == "empty":  # nnz = 0
        X0[:] = 0.0
    elif csr_kind == "one_row":  # all rows empty but one
        keep = X0[m // 2] * (rng.random(n) < 0.5)
        keep[rng.integers(n)] = 1.5
        X0[:] = 0.0
        X0[m // 2] = keep
    elif csr_kind == "dense_row":  # one fully dense row among sparse ones
        mask = rng.random((m, n)) < min(1.0, 6.0 / n)
        mask[m - 1] = True
        X0 *= mask
    w0 = rng.standard_normal((K, n)) / math.sqrt(n)
    b0 = rng.standard_normal(K)
    return X0, w0, b0, rng


def regime_inputs(X0, w0, b0, rng, regime, labels, softmax, dtype, zext):
    """(X torch (dtype), y fp32 labels, W (K, n) fp64, b (K) fp64) of one regime and label pattern.
    benign: |z| <~ 2. wide: |z| up to ~90. saturated: every row scaled so that its margin (binary:
    |z|, softmax: the gap between the two largest) lies in [17, 90], to be used with labels that
    agree. extreme: rows scaled to |z| (softmax: the spread of the margins) = zext."""
    m, n = X0.shape
    K = w0.shape[0]
    b = 0.3 * b0
    if regime == "benign":
        X, W = X0, 0.7 * w0
    elif regime == "wide":
        X, W = X0, 30.0 * w0
    else:
        W = w0.copy()
        S = X0 @ W.T
        if softmax:
            srt = np.sort(S, 1)
            stat = srt[:, -1] - (srt[:, -2] if regime == "saturated" else srt[:, 0])
        else:
            stat = np.abs(S).max(1)
        t = rng.uniform(17.0, 90.0, m) if regime == "saturated" else np.full(m, float(zext))
        X = X0 * np.minimum(t / np.maximum(stat, 1e-300), 1e3)[:, None]
    X = torch.from_numpy(np.ascontiguousarray(X)).to(dtype)
    Z = X.double().numpy() @ W.T + b
    if labels == "mixed":
        y = rng.integers(0, K, m) if softmax else (rng.random(m) < 0.4)
    elif labels == "zeros":
        y = np.zeros(m)
    elif labels == "last":
        y = np.full(m, K - 1 if softmax else 1)
    else:  # agree with the sign / the arg-max
        y = Z.argmax(1) if softmax else (Z[:, 0] > 0)
    return X, torch.from_numpy(np.asarray(y, dtype=np.float32)), W, b


def to_csr(X, dev):
    nz = X != 0
    indptr = torch.zeros(X.shape[0] + 1, dtype=torch.int64)
    indptr[1:] = nz.sum(1).cumsum(0)
    cols = nz.nonzero()[:, 1].to(torch.int32)
    return CSR(indptr=indptr.to(dev), indices=cols.to(dev), data=X[nz].to(dev), shape=tuple(X.shape))


def prefill(*shape):
    """Non-zero fp64 values of both signs in [0.25, 0.75) to add into."""
    i = torch.arange(int(np.prod(shape)), dtype=torch.float64)
    v = 0.25 + 0.5 * torch.frac(i * 0.6180339887498949)
    return (v * (1.0 - 2.0 * (i % 2))).reshape(*shape)


RUNS = [("benign", "mixed"), ("benign", "zeros"), ("wide", "mixed"), ("wide", "last"), ("saturated", "agree"),
        ("extreme", "mixed")]
RUNS_SHORT = [("benign", "mixed"), ("wide", "mixed"), ("saturated", "agree"), ("extreme", "mixed")]


def mlogit_supported(n, K):
    KB = 4 * ((K + 3) // 4)
    return 2 <= K <= 16 and 0 < n <= 4096 and KB * ((n + 1023) // 1024) <= 36


def expected_path(n, K, dtype, dev, csr=False, fused=False, det=False):
    if dev.type == "cpu":
        return "torch-cpu"
    if csr:
        return "csr_binary" if K == 1 else ("csr_spmm" if K <= 16 else "csr_wide")
    f32 = dtype == torch.float32
    if det and f32 and K <= 16:
        return "two_pass_deterministic_f32"
    if K == 1:
        if f32:
            return "fused_binary_f32" if n <= 4096 else ("lds_binary_f32" if n <= 16384 else "two_pass_binary_f32")
        return "lds_binary_f64" if n <= 16384 else "two_pass_binary_f64"
    if f32 and K <= 16:
        return "fused_multinomial_f32" if fused and mlogit_supported(n, K) else "two_pass_multinomial_f32"
    return "two_pass_wide_f32" if f32 else "two_pass_multinomial_f64"


def _class_key(path, dtype):
    return path + ("_f32" if dtype == torch.float32 else "_f64") if path == "csr_binary" else path


def exercise(dev, m, n, K, dtype, path, *, csr_kind=None, runs=RUNS, binary_api=False, use_ws=False, twice=False,
             seed=None):
    """One shape through ``ops.logistic_loss_grad`` in every run of ``runs``: the expected path, the
    bound on out - pre-fill, finite outputs, and flag = 1 leaving ``out`` bit-identical. binary_api:
    the same inputs through ``ops.logreg_binary_loss_grad`` too. twice: a second call is bit-identical."""
    softmax = K >= 2
    key = _class_key(path, dtype)
    u_margin, u_res = CLASS[key]
    api_key = ("fused_binary_f32" if n <= 4096 else "eager_f64") if dev.type != "cpu" else "torch-cpu"
    hp = u_res == U64 or (binary_api and CLASS[api_key][1] == U64)
    X0, w0, b0, rng = base(m, n, K, 1000 * K + 7 * m + n if seed is None else seed, csr_kind)
    zext = 700.0 if u_margin == U64 else 1000.0
    N = K * n + K + 1
    out0 = prefill(N)
    for regime, labels in runs:
        X, y, W, b = regime_inputs(X0, w0, b0, rng, regime, labels, softmax, dtype, zext)
        what = "%s m=%d n=%d K=%d %s/%s %s" % (key, m, n, K, regime, labels, csr_kind or "dense")
        ref = reference(X.double().numpy(), y.numpy(), W, b, softmax, hp)
        tG, tb, tl = bounds(ref, u_margin, u_res)
        exp, tol = flat(ref.G, ref.gb, ref.loss), flat(tG, tb, tl)
        Xv = to_csr(X, dev) if csr_kind else X.to(dev)
        assert ops.logistic_path(Xv, K) == path, what
        yv = y.to(dev)
        wv, bv = torch.from_numpy(W.reshape(-1)).to(dev), torch.from_numpy(b).to(dev)
        ws = None
        if use_ws:
            ws = ops.logreg_workspace(Xv)
            assert ws is not None, what
        out = out0.clone().to(dev)
        ops.logistic_loss_grad(Xv, yv, wv, bv, K, out, ws=ws)
        got = out.cpu().numpy()
        ok, ratio = compare(got, out0.numpy(), exp, tol, m)
        _record(key, ratio, what)
        assert ok, "%s: error / bound = %.3g" % (what, ratio)
        if regime == "wide" and not softmax:
            # a misclassified row costs |z|: the loss is at least their sum
            z = ref.Z[:, 0].astype(np.float64)
            wrong = (z > 0) != (y.numpy() > 0.5)
            assert got[-1] - out0.numpy()[-1] >= np.abs(z[wrong]).sum() - tol[-1], what
        if twice:
            out_b = out0.clone().to(dev)
            ops.logistic_loss_grad(Xv, yv, wv, bv, K, out_b, ws=ws)
            assert torch.equal(out_b, out), what
        if binary_api:
            am, ar = CLASS[api_key]
            t2 = flat(*bounds(ref, am, ar))
            buf = out0.clone().to(dev)
            res = ops.logreg_binary_loss_grad(Xv, yv, wv, float(b[0]), out=buf)  # zeroes out itself
            ok, ratio = compare(res.cpu().numpy(), np.zeros(N), exp, t2, m)
            _record("binary_api:" + api_key, ratio, what)
            assert ok, "logreg_binary_loss_grad %s: error / bound = %.3g" % (what, ratio)
    if dev.type != "cpu":  # the done flag short-circuits every device pass
        flag = torch.ones(1, dtype=torch.int32, device=dev)
        out = out0.clone().to(dev)
        ops.logistic_loss_grad(Xv, yv, wv, bv, K, out, flag, ws=ws)
        assert torch.equal(out.cpu(), out0), "flag = 1 changed out: " + what


def exercise_multi(dev, m, n, M, fused):
    """M sigmoid models through ``ops.logistic_loss_grad_multi`` on strided WB / out views whose
    padding must stay untouched."""
    if dev.type == "cpu":
        key = "torch-cpu"
    else:
        key = "multi_fused_f32" if fused and mlogit_supported(n, max(2, min(M, 16))) else "multi_two_pass_f32"
    u_margin, u_res = CLASS[key]
    X0, w0, b0, rng = base(m, n, M, 2000 * M + 7 * m + n)
    zext = 700.0 if u_margin == U64 else 1000.0
    for i, (regime, labels) in enumerate(RUNS):
        sw, so = (n + 1, n + 2) if i % 2 == 0 else (n + 5, n + 6)
        X, y, W, b = regime_inputs(X0, w0, b0, rng, regime, labels, False, torch.float32, zext)
        what = "%s m=%d n=%d M=%d %s/%s strides %d/%d" % (key, m, n, M, regime, labels, sw, so)
        ref = reference(X.double().numpy(), y.numpy(), W, b, False, u_res == U64)
        exp, tol = rows(ref.G, ref.gb, ref.loss), rows(*bounds(ref, u_margin, u_res))
        WB0 = torch.full((M, sw), 7.25, dtype=torch.float64)  # columns past n + 1: padding
        WB0[:, :n] = torch.from_numpy(W)
        WB0[:, n] = torch.from_numpy(b)
        O0 = prefill(M, so)  # columns past n + 2: padding
        WBd, Od = WB0.clone().to(dev), O0.clone().to(dev)
        ops.logistic_loss_grad_multi(X.to(dev), y.to(dev), WBd[:, : n + 1], Od[:, : n + 2])
        got = Od.cpu()
        assert torch.equal(WBd.cpu(), WB0), "WB changed: " + what
        assert torch.equal(got[:, n + 2:], O0[:, n + 2:]), "out padding changed: " + what
        ok, ratio = compare(got[:, : n + 2].numpy(), O0[:, : n + 2].numpy(), exp, tol, m)
        _record(key, ratio, what)
        assert ok, "%s: error / bound = %.3g" % (what, ratio)


# ------------------------------------------------------------------------------------------
# the case matrix (the smallest shapes at which each kernel can go wrong; no full cross product)
BIN_N = [1, 3, 4, 60, 64, 68, 252, 256, 260, 508, 512, 513, 516, 1023, 1024, 1025, 1028, 2048, 2052, 3072, 3076,
         4092, 4095, 4096, 4097, 8192, 8193, 16384, 16385]
BIN_M = [1, 3, 5, 16, 17, 63, 65, 257]
BIN_SHAPES = sorted({(m, n) for n in BIN_N for m in (5, 65)}
                    | {(m, n) for m in BIN_M for n in (4, 64, 512, 513, 1028, 4096, 4097, 16385)})
WS_M = [16, 17, 784, 785, 1040, 1041]

MN_K = [2, 3, 4, 5, 8, 9, 12, 13, 16]
MN_N = [1, 5, 64, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097]
MN_M = [1, 2, 3, 4, 5, 8, 9, 255, 257, 513]
MN_SHAPES = sorted({(m, n, K) for K in MN_K for n in (5, 1025) for m in (5, 257)}
                   | {(9, n, K) for n in MN_N for K in (3, 5, 12, 16)}
                   | {(9, n, K) for n in (4096, 4097) for K in MN_K}
                   | {(m, n, K) for m in MN_M for (K, n) in ((3, 64), (16, 1025))})

WIDE_K = [17, 32, 33, 63, 64, 65, 129]
WIDE_SHAPES = sorted({(5, n, K) for K in WIDE_K for n in (5, 64, 1025)}
                     | {(m, 64, K) for m in (1, 3, 5, 65) for K in (17, 129)})

F64_M = [1, 5, 65, 257]
F64_BIN = [(m, n) for n in (1, 5, 64, 257, 8193, 16384, 16385) for m in F64_M]
F64_MN = [(m, n, K) for K in (2, 16, 17) for n in (5, 257) for m in F64_M]

CSR_SHAPES = [(m, n, K) for K in (1, 2, 16, 17, 33) for n in (1, 64, 1025) for m in (1, 5, 257)]
CSR_KINDS = ["empty", "one_row", "dense_row"]

DET_SHAPES = [(m, n, K) for K in (1, 4) for m in (1, 257, 513) for n in (5, 1028)]

MULTI_SHAPES = [(m, n, M) for M in (1, 2, 4, 5, 8, 9, 12, 13, 16, 17, 33) for n in (5, 1024, 1025) for m in (1, 5, 257)]


# ------------------------------------------------------------------------------------------
# CPU: the oracle itself
@pytest.mark.parametrize("m,n,K", [(5, 4, 1), (65, 64, 1), (257, 512, 1), (65, 16385, 1), (5, 4, 3), (65, 64, 5),
                                   (9, 1025, 16)])
def test_checker_rejects_wrong_results(m, n, K):
    """The exact result passes both classes; a dropped row, two swapped columns, two swapped class
    rows (and, against the fp64 class, an fp32 sigmoid) in the benign regime do not."""
    X0, w0, b0, rng = base(m, n, K, 5 * m + n + K)
    X, y, W, b = regime_inputs(X0, w0, b0, rng, "benign", "mixed", K >= 2, torch.float32, 700.0)
    Xd = X.double().numpy()
    ref = reference(Xd, y.numpy(), W, b, K >= 2, True)
    exp = flat(ref.G, ref.gb, ref.loss).astype(np.float64)
    zero = np.zeros_like(exp)
    for u_res in (U32, U64):
        tol = flat(*bounds(ref, U64, u_res))

        def rejected(G, gb=ref.gb, loss=ref.loss):
            return not compare(flat(G, gb, loss).astype(np.float64), zero, exp, tol, m)[0]

        ok, ratio = compare(exp, zero, exp, tol, m)
        assert ok and ratio <= 0.5
        r = m - 1  # the tail row
        Gd = ref.G - np.outer(ref.R[r], Xd[r])
        assert rejected(Gd), "dropped row in the gradient"
        assert rejected(Gd, ref.gb - ref.R[r], ref.loss - ref.L[r]), "dropped row"
        assert rejected(ref.G, ref.gb - ref.R[r]), "dropped row in the bias gradient"
        assert rejected(ref.G, ref.gb, ref.loss - ref.L[r]), "dropped row in the loss"
        Gs = ref.G.copy()
        Gs[:, [0, 1]] = Gs[:, [1, 0]]
        assert rejected(Gs), "swapped columns"
        if K >= 2:
            Gs = ref.G.copy()
            Gs[[0, 1]] = Gs[[1, 0]]
            assert rejected(Gs), "swapped classes"
    if K == 1:
        # exact fp64 accumulation of a residual whose sigmoid was evaluated in fp32
        z32 = ref.Z[:, 0].astype(np.float32)
        e = np.exp(-np.abs(z32))
        p = np.where(z32 >= 0, np.float32(1) / (np.float32(1) + e), e / (np.float32(1) + e)).astype(np.float32)
        r32 = p.astype(np.longdouble) - y.numpy().astype(np.longdouble)
        l32 = np.maximum(ref.Z[:, 0], 0) - y.numpy() * ref.Z[:, 0] + np.log1p(e).astype(np.longdouble)
        got = flat(r32 @ Xd.astype(np.longdouble), r32.sum(), l32.sum()).astype(np.float64)
        assert not compare(got, zero, exp, flat(*bounds(ref, U64, U64)), m)[0], "fp32 sigmoid in the fp64 class"
        assert compare(got, zero, exp, flat(*bounds(ref, U64, U32)), m)[0], "fp32 sigmoid in the fp32 class"


def test_reference_tails():
    """The reference keeps the relative accuracy of the tails: a correctly classified row at z = 40
    has residual -e^-40, not 0, and a saturated softmax row likewise."""
    X = np.array([[40.0], [-40.0]])
    ref = reference(X, np.array([1.0, 0.0]), np.array([[1.0]]), np.array([0.0]), False, False)
    np.testing.assert_allclose(ref.R[:, 0].astype(np.float64), [-math.exp(-40.0), math.exp(-40.0)], rtol=1e-12)
    np.testing.assert_allclose(ref.L[:, 0].astype(np.float64), [math.exp(-40.0)] * 2, rtol=1e-12)
    ref = reference(np.array([[700.0]]), np.array([0.0]), np.array([[1.0]]), np.array([0.0]), False, True)
    assert float(ref.L[0, 0]) == 700.0 and float(ref.R[0, 0]) == 1.0
    ref = reference(np.array([[30.0]]), np.array([0.0]), np.array([[1.0], [0.0]]), np.zeros(2), True, True)
    np.testing.assert_allclose(np.asarray(ref.R[0], dtype=np.float64), [-math.exp(-30.0), math.exp(-30.0)], rtol=1e-9)


_CPU = torch.device("cpu")


def _cpu_cases(family):
    """The family's cases as (function, args, kwargs), every dispatch dimension that the CPU ignores
    (SRML_LOGREG_FUSED, SRML_DETERMINISTIC, the workspace) folded away."""
    f32, f64 = torch.float32, torch.float64
    if family == "binary":
        return ([(exercise, (m, n, 1, f32), dict(binary_api=True)) for m, n in BIN_SHAPES]
                + [(exercise, (m, 1028, 1, f32), dict(runs=RUNS_SHORT)) for m in WS_M])
    if family == "multinomial":
        return [(exercise, (m, n, K, f32), {}) for m, n, K in MN_SHAPES]
    if family == "wide":
        return [(exercise, (m, n, K, dt), {}) for m, n, K in WIDE_SHAPES for dt in (f32, f64)]
    if family == "fp64":
        return ([(exercise, (m, n, 1, f64), {}) for m, n in F64_BIN]
                + [(exercise, (m, n, K, f64), {}) for m, n, K in F64_MN])
    if family == "csr":
        return [(exercise, (m, n, K, dt), dict(csr_kind=kind, runs=RUNS if kind == "dense_row" else RUNS_SHORT))
                for m, n, K in CSR_SHAPES for dt in (f32, f64) for kind in CSR_KINDS]
    if family == "deterministic":
        return [(exercise, (m, n, K, f32), dict(twice=True)) for m, n, K in DET_SHAPES]
    return [(exercise_multi, (m, n, M), {}) for m, n, M in MULTI_SHAPES]


@pytest.mark.parametrize("part", range(4))
@pytest.mark.parametrize("family", ["binary", "multinomial", "wide", "fp64", "csr", "deterministic", "multi"])
def test_torch_cpu_matrix(family, part):
    """The whole case matrix through the ``torch-cpu`` path (fp64 class), a quarter of a family at a time."""
    for fn, args, kw in _cpu_cases(family)[part::4]:
        if fn is exercise:
            exercise(_CPU, *args, "torch-cpu", **kw)
        else:
            exercise_multi(_CPU, *args, False)


# ------------------------------------------------------------------------------------------
# GPU: every dispatch path
@pytest.mark.gpu
@pytest.mark.parametrize("m,n", BIN_SHAPES)
def test_binary_f32(gpu_device, m, n):
    """``fused_binary_f32`` (narrow G = 1, 2, 4, 8; generic V = 1 .. 16 through unaligned n;
    prefetching VS = 2, 3, 4), ``lds_binary_f32`` on both sides of 64 KiB, ``two_pass_binary_f32``,
    through ``logistic_loss_grad`` and ``logreg_binary_loss_grad``."""
    exercise(gpu_device, m, n, 1, torch.float32, expected_path(n, 1, torch.float32, gpu_device), binary_api=True)


@pytest.mark.gpu
@pytest.mark.parametrize("m", WS_M)
def test_binary_f32_partial_rows(gpu_device, m):
    """The prefetching kernel with the fit's partial-row workspace: 1, 2, 49 / 50 and 65 / 66
    partial rows, around the 4-rows-in-flight loop of ``fold_rows_kernel``."""
    exercise(gpu_device, m, 1028, 1, torch.float32, "fused_binary_f32", runs=RUNS_SHORT, use_ws=True)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("m,n,K", MN_SHAPES)
def test_multinomial_f32(gpu_device, monkeypatch, m, n, K, fused):
    """Around ``XW_MFMA_MIN_K`` = 3, ``XTV_MFMA_MIN_K`` = 5, the fused kernel's KB = 4 / 8 / 12 / 16
    register tiers and the end of ``srml_mlogit_supported`` (KB V <= 36)."""
    monkeypatch.setenv("SRML_LOGREG_FUSED", str(fused))
    path = expected_path(n, K, torch.float32, gpu_device, fused=bool(fused))
    if fused:
        past = n > 4096 or (K > 12 and n > 2048) or (K > 8 and n > 3072)
        assert path == ("two_pass_multinomial_f32" if past else "fused_multinomial_f32")
    exercise(gpu_device, m, n, K, torch.float32, path)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("m,n,K", WIDE_SHAPES)
def test_wide(gpu_device, m, n, K, dtype):
    exercise(gpu_device, m, n, K, dtype, expected_path(n, K, dtype, gpu_device))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n", F64_BIN)
def test_binary_f64(gpu_device, m, n):
    """``lds_binary_f64`` up to the 128 KiB of dynamic LDS at n = 16384, ``two_pass_binary_f64`` past it."""
    exercise(gpu_device, m, n, 1, torch.float64, expected_path(n, 1, torch.float64, gpu_device))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,K", F64_MN)
def test_multinomial_f64(gpu_device, m, n, K):
    exercise(gpu_device, m, n, K, torch.float64, "two_pass_multinomial_f64")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("m,n,K", CSR_SHAPES)
def test_csr(gpu_device, m, n, K, dtype):
    """nnz = 0, all rows empty but one, one fully dense row among sparse ones."""
    for kind in CSR_KINDS:
        exercise(gpu_device, m, n, K, dtype, expected_path(n, K, dtype, gpu_device, csr=True), csr_kind=kind,
                 runs=RUNS if kind == "dense_row" else RUNS_SHORT)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,K", DET_SHAPES)
def test_deterministic(gpu_device, monkeypatch, m, n, K):
    """Within the bound, and bit-identical on a second call."""
    monkeypatch.setenv("SRML_DETERMINISTIC", "1")
    exercise(gpu_device, m, n, K, torch.float32, "two_pass_deterministic_f32", twice=True)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("m,n,M", MULTI_SHAPES)
def test_multi(gpu_device, monkeypatch, m, n, M, fused):
    monkeypatch.setenv("SRML_LOGREG_FUSED", str(fused))
    exercise_multi(gpu_device, m, n, M, bool(fused))
