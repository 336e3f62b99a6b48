"""The fp64 dense solvers behind LinearRegression on every dispatch path: the blocked Cholesky
(``srml_potrf_f64_variant``: panel width, register / LDS diagonal block, SYRK / full-DGEMM
trailing update), the triangular solves (``srml_potrs_f64_variant``, ``srml_potrs_backward_f64``),
the Gram-matrix coordinate descent (pipelined, block, row-at-a-time and global-memory sweeps) and
the f64 MFMA GEMM (in-kernel epilogue, split-K, lower-triangle SYRK).

Every property is checked against a plain torch / numpy fp64 oracle on the CPU. Each check runs
twice: unmarked on ``device="cpu"`` through the ops' CPU fallbacks and LAPACK (which proves that
the inputs and the oracles stay within their caps without a GPU), and under ``pytest.mark.gpu``
on the HIP kernels.

Margins (the yardstick is always the CPU reference's own error on the same problem):
  * factor error  max|tril(L) tril(L)^T - A| / max|A|  <= max(8 x LAPACK's, 4 eps)
  * solve backward error  eta = |Ax - b|_inf / (|A|_inf |x|_inf + |b|_inf)  <= max(16 x LAPACK's, 1 eps)
  * CD KKT residual  <= 4 x the CPU sweep's + 1e-14
The 8 x / 16 x allow for a different blocking and summation order, FMA contraction and a multiply
by a reciprocal where LAPACK divides. Measured device / reference ratios are in the docstrings of
the GPU tests below.
"""
import functools
import math

import numpy as np
import pytest
import torch

from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.ops import native

F64 = torch.float64
EPS = torch.finfo(F64).eps
CPU = torch.device("cpu")
NAN = float("nan")


# ------------------------------------------------------------------------------------------
# oracles (CPU, fp64)
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spd(n, kappa, seed):
    """A = Q diag(lam) Q^T, symmetrised: Q from the QR of a seeded Gaussian matrix, lam log-spaced
    from 1 down to 1/kappa. Cached: callers clone before they write."""
    g = torch.Generator().manual_seed(seed)
    Q, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=F64))
    lam = torch.logspace(0.0, -math.log10(kappa), n, dtype=F64)
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T)


@functools.lru_cache(maxsize=None)
def _lapack_factor(n, kappa, seed):
    L, info = torch.linalg.cholesky_ex(_spd(n, kappa, seed))
    assert int(info) == 0
    return L.contiguous()  # (LAPACK's result may come back column-major)


@functools.lru_cache(maxsize=None)
def _rhs(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed + 7919), dtype=F64)


def _factor_error(L, A):
    Lt = torch.tril(L)
    return (torch.tril(Lt @ Lt.T - A).abs().max() / A.abs().max()).item()


def _eta(A, x, b):
    r = (A @ x - b).abs().max()
    return (r / (A.abs().sum(1).max() * x.abs().max() + b.abs().max())).item()


def _kkt(A, b, l1, l2, w):
    """Elastic-net KKT residual over the live coordinates (A_jj + l2_j > 0)."""
    r = A @ w - b + l2 * w
    live = (torch.diagonal(A) + l2) > 0
    nz = live & (w != 0)
    z = live & (w == 0)
    res = 0.0
    if nz.any():
        res = max(res, (r[nz] + l1[nz] * torch.sign(w[nz])).abs().max().item())
    if z.any():
        res = max(res, (r[z].abs() - l1[z]).clamp_min(0.0).max().item())
    return res


def _cd_ref(A, b, l1, l2, max_iter, tol, w0=None):
    """Plain cyclic sweep; returns (w, iterations, [(max_delta, max_w) per sweep])."""
    Ah, bh, l1h, l2h = (t.numpy() for t in (A, b, l1, l2))
    n = Ah.shape[0]
    w = np.zeros(n) if w0 is None else w0.numpy().copy()
    g = Ah @ w
    diag = np.diag(Ah) + l2h
    hist = []
    it = 0
    for it in range(1, max(1, max_iter) + 1):
        max_delta = max_w = 0.0
        for j in range(n):
            if diag[j] <= 0:
                continue
            rho = bh[j] - g[j] + Ah[j, j] * w[j]
            nw = (rho - l1h[j]) / diag[j] if rho > l1h[j] else ((rho + l1h[j]) / diag[j] if rho < -l1h[j] else 0.0)
            d = nw - w[j]
            if d != 0.0:
                g += d * Ah[:, j]
                w[j] = nw
                max_delta = max(max_delta, abs(d))
            max_w = max(max_w, abs(nw))
        hist.append((max_delta, max_w))
        if max_delta <= tol * max(max_w, 1e-300):
            break
    return torch.from_numpy(w), it, hist


def _gemm_bound(a, b, c0, alpha, beta, K):
    """Elementwise 2 (K + 2) eps (|alpha| |op A| |op B| + |beta| |C0|): the dot-product rounding
    bound, doubled because the fp64 reference rounds too."""
    bound = abs(alpha) * (a.abs() @ b.abs())
    if beta != 0.0:
        bound = bound + abs(beta) * c0.abs()
    return 2.0 * (K + 2) * EPS * bound


def _bits(t):
    return t.contiguous().view(torch.int64)


def _padded(A, pad, device):
    """(buffer, view): A in the leading columns of a NaN-filled (rows, cols + pad) buffer."""
    rows, cols = A.shape
    buf = torch.full((rows, cols + pad), NAN, dtype=F64)
    buf[:, :cols] = A
    buf = buf.to(device)
    return buf, buf[:, :cols]


# ------------------------------------------------------------------------------------------
# the operations under test: native variant entries on the GPU, CPU fallbacks / LAPACK on the CPU
# ------------------------------------------------------------------------------------------
def _potrf(view, nb, diag_reg, syrk):
    """Factor the (possibly row-strided) square view in place; returns info."""
    n = view.shape[0]
    if not view.is_cuda:
        L, info = torch.linalg.cholesky_ex(view)
        i, j = torch.tril_indices(n, n)
        view[i, j] = L[i, j]
        return int(info)
    assert view.stride(1) == 1
    info = torch.full((1,), 77, dtype=torch.int32, device=view.device)
    native.call("srml_potrf_f64_variant", view.data_ptr(), n, view.stride(0), info.data_ptr(), nb, diag_reg, syrk,
                native.stream(view.device))
    return int(info.item())


def _potrs(Lview, b, variant):
    if not Lview.is_cuda:
        return torch.cholesky_solve(b.view(-1, 1), torch.tril(Lview)).view(-1)
    x = b.clone()
    assert Lview.stride(1) == 1
    native.call("srml_potrs_f64_variant", Lview.data_ptr(), Lview.shape[0], Lview.stride(0), x.data_ptr(), variant,
                native.stream(Lview.device))
    return x


def _potrs_backward(Lview, z):
    if not Lview.is_cuda:
        return torch.linalg.solve_triangular(torch.tril(Lview).T, z.view(-1, 1), upper=True).view(-1)
    x = z.clone()
    assert Lview.stride(1) == 1
    native.call("srml_potrs_backward_f64", Lview.data_ptr(), Lview.shape[0], Lview.stride(0), x.data_ptr(),
                native.stream(Lview.device))
    return x


CD_PATHS = ("pipe", "block", "row", "global")


def _cd_run(path, A, b, l1, l2, max_iter, tol, w0):
    """One CD solve on A's device. On the CPU every path is the ops' CPU sweep."""
    if not A.is_cuda:
        return ops.cd_gram(A, b, l1, l2, max_iter, tol, w0)
    n = A.shape[0]
    w = torch.zeros(n, dtype=F64, device=A.device) if w0 is None else w0.clone()
    if path == "global":
        return ops._cd_gram_global(A, b, l1, l2, max_iter, tol, w, w0 is not None)
    iters = torch.full((1,), -1, dtype=torch.int32, device=A.device)
    native.call("srml_cd_gram_f64_variant", A.data_ptr(), n, A.stride(0), b.data_ptr(), l1.data_ptr(), l2.data_ptr(),
                w.data_ptr(), max_iter, tol, iters.data_ptr(), CD_PATHS.index(path), native.stream(A.device))
    return w, int(iters.item())


def _syrk_lower(a, alpha, beta, c):
    """c = alpha a a^T + beta c in place on the 64 x 64 tiles that touch the lower triangle."""
    M, K = a.shape
    if not a.is_cuda:
        full = alpha * (a @ a.T) + (beta * c if beta != 0.0 else 0.0)
        t = torch.arange(M) // 64
        touched = t.view(1, -1) <= t.view(-1, 1)
        c.copy_(torch.where(touched, full, c))
        return
    native.call("srml_dgemm_syrk_lower", M, K, float(alpha), a.data_ptr(), a.stride(0), float(beta), c.data_ptr(),
                c.stride(0), native.stream(a.device))


# ------------------------------------------------------------------------------------------
# Cholesky factor
# ------------------------------------------------------------------------------------------
POTRF_VARIANTS = [(nb, reg, syrk) for nb in (32, 64) for reg in (1, 0) for syrk in (1, 0)]
POTRF_CASES = [(n, 1e2) for n in (1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 257, 1057)] + \
              [(65, 1e10), (257, 1e10), (129, 1e6)]


def _check_potrf(device, n, kappa, nb, reg, syrk, pad=0):
    A = _spd(n, kappa, n)
    ref = _lapack_factor(n, kappa, n)
    ref_err = _factor_error(ref, A)
    # Higham, Accuracy and Stability, thm 10.3: |A - L L^T| <= gamma_{n+1} |L| |L^T|, and
    # (|L| |L|^T)_ij <= sqrt(a_ii a_jj) <= max |A|: the yardstick itself stays under (n + 1) eps
    assert ref_err <= (n + 1) * EPS
    buf, view = _padded(A, pad, device)
    info = _potrf(view, nb, reg, syrk)
    assert info == 0
    L = view.cpu()
    assert (torch.diagonal(L) > 0).all()
    err = _factor_error(L, A)
    print("potrf n=%d kappa=%g nb=%d reg=%d syrk=%d: factor error %.3g eps, LAPACK %.3g eps, ratio %.3g"
          % (n, kappa, nb, reg, syrk, err / EPS, ref_err / EPS, err / max(ref_err, 1e-300)))
    assert err <= max(8.0 * ref_err, 4.0 * EPS)
    if kappa == 1e2:
        torch.testing.assert_close(torch.tril(L), ref, rtol=1e-9, atol=1e-9)
    if pad:
        assert view.stride(0) == n + pad
        assert torch.isnan(buf[:, n:]).all()


@pytest.mark.parametrize("n,kappa", POTRF_CASES)
def test_potrf_cpu(n, kappa):
    _check_potrf(CPU, n, kappa, 32, 1, 1)


def test_potrf_strided_cpu():
    _check_potrf(CPU, 97, 1e2, 32, 1, 1, pad=5)


@pytest.mark.gpu
@pytest.mark.parametrize("nb,reg,syrk", POTRF_VARIANTS)
@pytest.mark.parametrize("n,kappa", POTRF_CASES)
def test_potrf_variants(gpu_device, n, kappa, nb, reg, syrk):
    """Every (panel width, diagonal-block kernel, trailing update) combination at the panel and
    block edges; n = 1057 gives a TRSM over 1025 rows (five blocks, the last with one row).
    Measured on an MI355X over these 136 cases and the 8 strided ones: device / LAPACK factor error
    between 0 and 3.0 (limit 8), worst at n = 65, nb = 64, LDS diagonal block (1.95 eps against
    0.65 eps); largest device error 10.5 eps where LAPACK's largest is 8.0 eps."""
    _check_potrf(gpu_device, n, kappa, nb, reg, syrk)


@pytest.mark.gpu
@pytest.mark.parametrize("nb,reg,syrk", POTRF_VARIANTS)
def test_potrf_strided(gpu_device, nb, reg, syrk):
    """lda = n + 5 on a view of a NaN-filled buffer: the padding stays NaN."""
    _check_potrf(gpu_device, 97, 1e2, nb, reg, syrk, pad=5)


@pytest.mark.gpu
def test_potrf_variant_rejects_unknown_choices(gpu_device):
    fn = getattr(native.lib(), "srml_potrf_f64_variant")
    A = _spd(5, 1e2, 5).to(gpu_device)
    info = torch.zeros(1, dtype=torch.int32, device=gpu_device)
    st = native.stream(gpu_device)
    for nb, reg, syrk in [(16, 1, 1), (48, 1, 1), (32, 2, 1), (32, 1, -1), (0, 0, 0)]:
        assert fn(A.data_ptr(), 5, 5, info.data_ptr(), nb, reg, syrk, st) < 0
    torch.cuda.synchronize()
    assert torch.equal(A.cpu(), _spd(5, 1e2, 5))


# ------------------------------------------------------------------------------------------
# pivot failure
# ------------------------------------------------------------------------------------------
PIVOT_N = 150
PIVOT_CASES = [(0, -1.0), (31, -1.0), (32, -1.0), (33, -1.0), (63, -1.0), (64, -1.0), (100, -1.0),
               (PIVOT_N - 1, -1.0), (40, NAN)]


def _broken(k, value):
    A = _spd(PIVOT_N, 1e2, PIVOT_N).clone()
    if value == value:  # a negative pivot: row and column k zeroed
        A[k, :] = 0.0
        A[:, k] = 0.0
    A[k, k] = value
    return A


def _check_pivot(device, k, value):
    A = _broken(k, value)
    assert int(torch.linalg.cholesky_ex(A)[1]) == k + 1
    for nb, reg, syrk in (POTRF_VARIANTS if device.type == "cuda" else POTRF_VARIANTS[:1]):
        assert _potrf(A.clone().to(device), nb, reg, syrk) == k + 1, (nb, reg, syrk)
    b = _rhs(PIVOT_N, 0).to(device)
    _, ok = ops.spd_solve(A.to(device), b)
    assert ok is False
    _, ok = ops.spd_factor(A.to(device))
    assert ok is False
    if device.type == "cuda":
        torch.cuda.synchronize()


@pytest.mark.parametrize("k,value", PIVOT_CASES)
def test_pivot_failure_cpu(k, value):
    _check_pivot(CPU, k, value)


@pytest.mark.gpu
@pytest.mark.parametrize("k,value", PIVOT_CASES)
def test_pivot_failure(gpu_device, k, value):
    """info = first non-positive (or NaN) pivot column + 1 on every variant, as LAPACK reports it;
    ``spd_solve`` / ``spd_factor`` return ok = False and the run finishes normally."""
    _check_pivot(gpu_device, k, value)


# ------------------------------------------------------------------------------------------
# solves
# ------------------------------------------------------------------------------------------
def _check_eta(tag, A, x, b, x_ref):
    eta, eta_ref = _eta(A, x, b), _eta(A, x_ref, b)
    print("%s: eta %.3g eps, LAPACK %.3g eps, ratio %.3g" % (tag, eta / EPS, eta_ref / EPS, eta / max(eta_ref, 1e-300)))
    assert eta_ref <= EPS  # the yardstick is itself backward stable
    assert eta <= max(16.0 * eta_ref, EPS)


def _check_spd_solve(device, n, kappa):
    A, b = _spd(n, kappa, n), _rhs(n, n)
    x_ref = torch.cholesky_solve(b.view(-1, 1), _lapack_factor(n, kappa, n)).view(-1)
    x, ok = ops.spd_solve(A.to(device), b.to(device))
    assert ok
    _check_eta("spd_solve n=%d kappa=%g" % (n, kappa), A, x.cpu(), b, x_ref)


SPD_SOLVE_CASES = [(n, kappa) for n in (31, 63, 127, 300) for kappa in (1e2, 1e10)]


@pytest.mark.parametrize("n,kappa", SPD_SOLVE_CASES)
def test_spd_solve_backward_error_cpu(n, kappa):
    _check_spd_solve(CPU, n, kappa)


@pytest.mark.gpu
@pytest.mark.parametrize("n,kappa", SPD_SOLVE_CASES)
def test_spd_solve_backward_error(gpu_device, n, kappa):
    """The augmented factorisation at sizes n + 1 that are multiples of the 32-wide panel (a full
    last panel, no TRSM after it), well and ill conditioned, by backward error.
    Measured on an MI355X: eta 0.04 - 0.34 eps, device / LAPACK between 0.43 and 2.2 (limit 16,
    floor 1 eps); the worst is n = 127, kappa = 1e10 (0.16 eps against 0.07 eps)."""
    _check_spd_solve(gpu_device, n, kappa)


def _nan_upper(L):
    """The factor with NaN above the diagonal: the solves may read the lower triangle only."""
    out = L.clone(memory_format=torch.contiguous_format)
    i, j = torch.triu_indices(L.shape[0], L.shape[0], offset=1)
    out[i, j] = NAN
    return out


def _check_potrs(device, n, variant, pad=0):
    A, b = _spd(n, 1e2, n), _rhs(n, n)
    L = _lapack_factor(n, 1e2, n)
    x_ref = torch.cholesky_solve(b.view(-1, 1), L).view(-1)
    buf, view = _padded(_nan_upper(L), pad, device)
    x = _potrs(view, b.to(device), variant).cpu()
    _check_eta("potrs n=%d variant=%d" % (n, variant), A, x, b, x_ref)
    torch.testing.assert_close(x, x_ref, rtol=1e-9, atol=1e-9)
    if pad:
        assert view.stride(0) == n + pad
        assert torch.equal(_bits(buf.cpu()), _bits(_padded(_nan_upper(L), pad, CPU)[0]))


POTRS_SIZES = (1, 63, 64, 65, 128, 129, 449, 513, 577, 1100)


@pytest.mark.parametrize("n", POTRS_SIZES)
def test_potrs_cpu(n):
    _check_potrs(CPU, n, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n", POTRS_SIZES)
def test_potrs_variants(gpu_device, n, variant):
    """Blocked (0) and row-at-a-time (1) solves on a LAPACK factor uploaded to the device, so a
    potrf error cannot mask a potrs error; n >= 513 enters the 8-deep unrolled forward loop,
    n >= 177 the backward one.
    Measured on an MI355X: eta at most 0.26 eps, device / LAPACK at most 1.5 (n = 513, blocked)."""
    _check_potrs(gpu_device, n, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1])
def test_potrs_strided(gpu_device, variant):
    _check_potrs(gpu_device, 200, variant, pad=3)


def test_potrs_strided_cpu():
    _check_potrs(CPU, 200, 0, pad=3)


@pytest.mark.gpu
def test_potrs_variant_rejects_unknown_variant(gpu_device):
    fn = getattr(native.lib(), "srml_potrs_f64_variant")
    L = _lapack_factor(5, 1e2, 5).to(gpu_device)
    b = _rhs(5, 5).to(gpu_device)
    for variant in (-1, 2):
        assert fn(L.data_ptr(), 5, 5, b.data_ptr(), variant, native.stream(gpu_device)) < 0
    # each kernel keeps its own LDS limit: n doubles <= 110 KiB blocked, <= 150 KiB row at a time
    assert fn(L.data_ptr(), 14081, 14081, b.data_ptr(), 0, native.stream(gpu_device)) == -9
    assert fn(L.data_ptr(), 19201, 19201, b.data_ptr(), 1, native.stream(gpu_device)) == -9
    torch.cuda.synchronize()
    assert torch.equal(b.cpu(), _rhs(5, 5))


def _check_potrs_backward(device, n):
    L = _lapack_factor(n, 1e2, n)
    z = _rhs(n, n + 1)
    U = L.T.contiguous()
    x_ref = torch.linalg.solve_triangular(U, z.view(-1, 1), upper=True).view(-1)
    x = _potrs_backward(_nan_upper(L).to(device), z.to(device)).cpu()
    _check_eta("potrs_backward n=%d" % n, U, x, z, x_ref)
    torch.testing.assert_close(x, x_ref, rtol=1e-9, atol=1e-9)


POTRS_BACKWARD_SIZES = (1, 64, 65, 300, 1100)


@pytest.mark.parametrize("n", POTRS_BACKWARD_SIZES)
def test_potrs_backward_cpu(n):
    _check_potrs_backward(CPU, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", POTRS_BACKWARD_SIZES)
def test_potrs_backward(gpu_device, n):
    """L^T x = z alone (the augmented solve's second half) against a triangular solve.
    Measured on an MI355X: eta at most 0.22 eps, device / LAPACK at most 1.6 (n = 65)."""
    _check_potrs_backward(gpu_device, n)


# ------------------------------------------------------------------------------------------
# coordinate descent
# ------------------------------------------------------------------------------------------
CD_SIZES = (1, 3, 63, 64, 65, 100, 128, 129, 200, 700)
CD_TOL = 1e-12
CD_MAX_ITER = 100
# n -> seed of the converged problems (first seed n + 1000 s that meets test_cd_reference_conditions)
CD_SEEDS = {1: 1, 3: 12003, 63: 4063, 64: 64, 65: 2065, 100: 6100, 128: 15128, 129: 7129, 200: 7200, 700: 20700}


@functools.lru_cache(maxsize=None)
def _cd_problem(n, dead=True, bscale=0.03):
    """(A, b, l1, l2, w0): per-coordinate l1 in [0.02, 0.08], l2 in [0, 0.04]; with ``dead`` the
    coordinates 0, 63, 64 and n - 1 (where they exist) have a zero row and column and l2 = 0, so
    A_jj + l2_j = 0: what Lasso sees on a constant column. b = bscale * N(0, 1): 0.03 leaves
    10 - 20 % of the coordinates non-zero at the optimum (the sweep then contracts ~3 x per sweep,
    which the sweep-count condition needs), 0.3 nearly all of them. The warm start is dense."""
    seed = CD_SEEDS[n]
    A = _spd(n, 1e2, seed).clone()
    g = torch.Generator().manual_seed(seed + 104729)
    b = bscale * torch.randn(n, generator=g, dtype=F64)
    l1 = 0.02 + 0.06 * torch.rand(n, generator=g, dtype=F64)
    l2 = 0.04 * torch.rand(n, generator=g, dtype=F64)
    w0 = 0.5 * torch.randn(n, generator=g, dtype=F64)
    if dead:
        for j in sorted({0, 63, 64, n - 1}):
            if j < n:
                A[j, :] = 0.0
                A[:, j] = 0.0
                l2[j] = 0.0
    return A, b, l1, l2, w0


def _dead(A, l2):
    return (torch.diagonal(A) + l2) <= 0


@functools.lru_cache(maxsize=None)
def _cd_converged_ref(n, warm):
    A, b, l1, l2, w0 = _cd_problem(n)
    return _cd_ref(A, b, l1, l2, CD_MAX_ITER, CD_TOL, w0 if warm else None)


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("n", CD_SIZES)
def test_cd_reference_conditions(n, warm):
    """Conditions on the reference alone that make the device comparison well posed.

    The zero pattern cannot flip: every live |rho_j| is 1e-9 away from l1_j, on either side.

    The sweep count cannot straddle: with r = max_delta / (tol max_w), every sweep before the last
    has r >= 1.5 and the last r <= 0.66. The device and the reference run the same sweeps and differ
    by rounding: an iterate by at most ~n eps max_w (1.6e-13 max_w at n = 700), a delta by twice
    that, which is 0.3 in units of tol max_w = 1e-12 max_w. (A gap of 10 x on both sides of 1 cannot
    be had on this family: the sweep contracts max_delta 1.5 - 4 x per sweep, so the first r below 1
    is never below ~0.25. Seeds that meet the 1.5 / 0.66 gap are in CD_SEEDS.)"""
    A, b, l1, l2, w0 = _cd_problem(n)
    w, it, hist = _cd_converged_ref(n, warm)
    assert it <= 40 and len(hist) == it
    live = ~_dead(A, l2)
    if live.any():
        for md, mw in hist[:-1]:
            assert md >= 1.5 * CD_TOL * max(mw, 1e-300)
        md, mw = hist[-1]
        assert md <= 0.66 * CD_TOL * max(mw, 1e-300)
    rho = b - A @ w + torch.diagonal(A) * w
    zero = live & (w == 0)
    assert ((l1 - rho.abs())[zero] > 1e-9).all()
    assert ((rho.abs() - l1)[live & (w != 0)] > 1e-9).all()
    if n >= 3:
        assert (live & (w != 0)).any()
    if n >= 63:
        assert zero.any() and (live & (w != 0)).sum() >= 4
    start = w0 if warm else torch.zeros(n, dtype=F64)
    assert torch.equal(_bits(w[~live]), _bits(start[~live]))
    # the ops' CPU sweep is the same sweep
    w_ops, it_ops = ops.cd_gram(A, b, l1, l2, CD_MAX_ITER, CD_TOL, w0 if warm else None)
    assert it_ops == it and torch.equal(w_ops, w)


def _check_cd_converged(device, path, n, warm):
    A, b, l1, l2, w0 = _cd_problem(n)
    w_ref, it_ref, _ = _cd_converged_ref(n, warm)
    args = [t.to(device) for t in (A, b, l1, l2)]
    start = w0.to(device) if warm else None
    w, it = _cd_run(path, *args, CD_MAX_ITER, CD_TOL, start)
    w2, it2 = _cd_run(path, *args, CD_MAX_ITER, CD_TOL, start)
    if warm:
        assert torch.equal(start.cpu(), w0)  # the start vector is not written
    w, w2 = w.cpu(), w2.cpu()
    assert it == it_ref and it2 == it_ref
    assert torch.equal(w, w2)  # fixed fold order: run to run identical
    torch.testing.assert_close(w, w_ref, rtol=1e-9, atol=1e-12)
    assert torch.equal(w == 0, w_ref == 0)
    dead = _dead(A, l2)
    begin = w0 if warm else torch.zeros(n, dtype=F64)
    assert torch.equal(_bits(w[dead]), _bits(begin[dead]))  # dead coordinates: bit for bit
    kkt, kkt_ref = _kkt(A, b, l1, l2, w), _kkt(A, b, l1, l2, w_ref)
    print("cd %s n=%d warm=%d: %d sweeps, KKT %.3g, reference %.3g, ratio %.3g"
          % (path, n, warm, it, kkt, kkt_ref, kkt / max(kkt_ref, 1e-300)))
    assert kkt_ref <= 1e-11
    assert kkt <= 4.0 * kkt_ref + 1e-14


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("n", CD_SIZES)
def test_cd_converged_cpu(n, warm):
    _check_cd_converged(CPU, "cpu", n, warm)


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("path", CD_PATHS)
@pytest.mark.parametrize("n", CD_SIZES)
def test_cd_variants_converged(gpu_device, n, path, warm):
    """The pipelined, block, row-at-a-time and global-memory sweeps against the CPU sweep: iterate,
    zero pattern, sweep count, KKT residual, dead coordinates and run-to-run identity, with
    per-coordinate penalties, with and without a warm start; 65 <= n <= 128 is the two-block case
    of the pipelined kernel.
    Measured on an MI355X: device / CPU-sweep KKT residual at most 1.09 over all 80 cases
    (limit 4 x + 1e-14); the residuals themselves are 5e-16 - 1.9e-14."""
    _check_cd_converged(gpu_device, path, n, warm)


CD_CAPPED_SIZES = (1, 65, 200)


def _check_cd_capped(device, path, n, max_iter, warm, dead):
    A, b, l1, l2, w0 = _cd_problem(n, dead, 0.3)
    start = w0 if warm else None
    w_ref, it_ref, _ = _cd_ref(A, b, l1, l2, max_iter, 0.0, start)
    assert it_ref == max(1, max_iter) or n == 1  # (a single coordinate is exact after one sweep)
    dstart = None if start is None else start.to(device)
    w, it = _cd_run(path, *[t.to(device) for t in (A, b, l1, l2)], max_iter, 0.0, dstart)
    assert it == it_ref
    torch.testing.assert_close(w.cpu(), w_ref, rtol=1e-9, atol=1e-12)
    assert (w_ref != 0).any()


@pytest.mark.parametrize("max_iter", [0, 1, 3])
@pytest.mark.parametrize("n", CD_CAPPED_SIZES)
def test_cd_capped_cpu(n, max_iter):
    _check_cd_capped(CPU, "cpu", n, max_iter, warm=False, dead=False)
    _check_cd_capped(CPU, "cpu", n, max_iter, warm=True, dead=True)


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [1, 3])
@pytest.mark.parametrize("path", CD_PATHS)
@pytest.mark.parametrize("n", CD_CAPPED_SIZES)
def test_cd_variants_capped(gpu_device, n, path, max_iter):
    """tol = 0 and a sweep cap: the iterate after exactly max_iter sweeps, and the count."""
    _check_cd_capped(gpu_device, path, n, max_iter, warm=False, dead=False)
    _check_cd_capped(gpu_device, path, n, max_iter, warm=True, dead=True)


def _check_cd_zero_max_iter(device, n, warm):
    """``ops.cd_gram(max_iter=0)`` runs one sweep on every path."""
    A, b, l1, l2, w0 = _cd_problem(n, False, 0.3)
    start = w0 if warm else None
    w_ref, it_ref, _ = _cd_ref(A, b, l1, l2, 0, 0.0, start)
    assert it_ref == 1 and (w_ref != 0).any() and not torch.equal(w_ref, w0)
    dev = [t.to(device) for t in (A, b, l1, l2)]
    dstart = None if start is None else start.to(device)
    w, it = ops.cd_gram(*dev, 0, 0.0, dstart)
    assert it == 1
    torch.testing.assert_close(w.cpu(), w_ref, rtol=1e-9, atol=1e-12)
    if device.type == "cuda":
        wg = torch.zeros(n, dtype=F64, device=device) if dstart is None else dstart.clone()
        wg, it = ops._cd_gram_global(*dev, 0, 0.0, wg, warm)
        assert it == 1
        torch.testing.assert_close(wg.cpu(), w_ref, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("n", CD_CAPPED_SIZES)
def test_cd_zero_max_iter_cpu(n, warm):
    _check_cd_zero_max_iter(CPU, n, warm)


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("n", CD_CAPPED_SIZES)
def test_cd_zero_max_iter(gpu_device, n, warm):
    _check_cd_zero_max_iter(gpu_device, n, warm)


@pytest.mark.gpu
def test_cd_variant_rejects_unknown_variant_and_oversize(gpu_device):
    fn = getattr(native.lib(), "srml_cd_gram_f64_variant")
    A, b, l1, l2, w0 = (t.to(gpu_device) for t in _cd_problem(3))
    iters = torch.zeros(1, dtype=torch.int32, device=gpu_device)
    st = native.stream(gpu_device)
    w = w0.clone()

    def rc(n, variant):
        return fn(A.data_ptr(), n, n, b.data_ptr(), l1.data_ptr(), l2.data_ptr(), w.data_ptr(), 5, 0.0,
                  iters.data_ptr(), variant, st)

    assert rc(3, -1) < 0 and rc(3, 3) < 0
    # 150 KiB of LDS: 2 n + 64 * 65 + 18 * 64 doubles (pipe), 2 n + 64 * 65 + 64 (block), 2 n (row)
    assert rc(6945, 0) == -9 and rc(7489, 1) == -9 and rc(9601, 2) == -9
    torch.cuda.synchronize()
    assert torch.equal(w, w0)


# ------------------------------------------------------------------------------------------
# fp64 GEMM
# ------------------------------------------------------------------------------------------
def _gemm_inputs(M, N, K, ta, tb, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn((K, M) if ta else (M, K), generator=g, dtype=F64)
    B = torch.randn((N, K) if tb else (K, N), generator=g, dtype=F64)
    C0 = torch.randn(M, N, generator=g, dtype=F64)
    return A, B, C0


def _check_dgemm(device, M, N, K, ta, tb, alpha, beta, pad=0, expect_splits=None):
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    splits = ops._dgemm_splits(M, N, K, tiles)
    assert (splits == 1) if expect_splits == 1 else (expect_splits is None or splits > 1)
    A, B, C0 = _gemm_inputs(M, N, K, ta, tb, 1000 * M + K)
    a, b = (A.T if ta else A), (B.T if tb else B)
    ref = alpha * (a @ b) + (beta * C0 if beta != 0.0 else 0.0)
    bound = _gemm_bound(a, b, C0, alpha, beta, K)
    start = C0 if beta != 0.0 else torch.full((M, N), NAN, dtype=F64)  # beta = 0 never reads out
    buf, out = _padded(start, pad, device)
    before = buf.cpu().clone()
    res = ops.dgemm(A.to(device), B.to(device), ta=ta, tb=tb, alpha=alpha, beta=beta, out=out)
    assert res.data_ptr() == out.data_ptr()
    got = out.cpu()
    excess = ((got - ref).abs() - bound).max().item()
    assert torch.isfinite(got).all() and excess <= 0.0, excess
    if pad:
        assert torch.equal(_bits(buf.cpu()[:, N:]), _bits(before[:, N:]))


GEMM_SHAPES = [(1, 1, 1), (64, 64, 16), (65, 63, 17), (130, 67, 100), (200, 129, 127)]
GEMM_SCALARS = [(1.0, 0.0), (-1.0, 1.0), (0.5, 2.0)]
GEMM_OPS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize("alpha,beta", GEMM_SCALARS)
@pytest.mark.parametrize("M,N,K", [(65, 63, 17), (130, 67, 200)])
def test_dgemm_cpu(M, N, K, alpha, beta):
    _check_dgemm(CPU, M, N, K, True, True, alpha, beta, pad=3)


@pytest.mark.gpu
@pytest.mark.parametrize("alpha,beta", GEMM_SCALARS)
@pytest.mark.parametrize("ta,tb", GEMM_OPS)
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_dgemm_in_kernel_epilogue(gpu_device, M, N, K, ta, tb, alpha, beta):
    """K < 128: one pass of ``srml_dgemm`` with alpha * acc + beta * C in the kernel; with
    beta = 0 the output starts as NaN."""
    _check_dgemm(gpu_device, M, N, K, ta, tb, alpha, beta, expect_splits=1)


@pytest.mark.gpu
@pytest.mark.parametrize("alpha,beta", GEMM_SCALARS)
def test_dgemm_strided_out(gpu_device, alpha, beta):
    """A row-strided ``out`` view: the bytes outside the view are unchanged."""
    _check_dgemm(gpu_device, 65, 63, 17, False, True, alpha, beta, pad=7, expect_splits=1)
    _check_dgemm(gpu_device, 130, 67, 200, True, False, alpha, beta, pad=7, expect_splits=2)


@pytest.mark.gpu
def test_dgemm_many_tiles_no_split(gpu_device):
    """529 tiles and K >= 128: no split, K not a multiple of the 16-deep step."""
    _check_dgemm(gpu_device, 1472, 1472, 130, False, True, -1.0, 1.0, expect_splits=1)


@pytest.mark.gpu
@pytest.mark.parametrize("ta,tb", GEMM_OPS)
@pytest.mark.parametrize("K", [128, 130, 200, 260])
def test_dgemm_splitk_edges(gpu_device, K, ta, tb):
    _check_dgemm(gpu_device, 130, 67, K, ta, tb, 0.5, 2.0, expect_splits=2)


def _check_syrk_lower(device, M, K, alpha, beta, pad=0):
    g = torch.Generator().manual_seed(100 * M + K)
    a = torch.randn(M, K, generator=g, dtype=F64)
    C0 = torch.randn(M, M, generator=g, dtype=F64)
    start = C0.clone()
    if beta == 0.0:  # never read where computed, never written elsewhere
        start.fill_(NAN)
    ref = alpha * (a @ a.T) + (beta * C0 if beta != 0.0 else 0.0)
    bound = _gemm_bound(a, a.T, C0, alpha, beta, K)
    abuf, av = _padded(a, pad, device)
    cbuf, cv = _padded(start, pad, device)
    _syrk_lower(av, alpha, beta, cv)
    got = cv.cpu()
    t = torch.arange(M) // 64
    touched = t.view(1, -1) <= t.view(-1, 1)  # tile column <= tile row
    excess = ((got - ref).abs() - bound)[touched].max().item()
    assert torch.isfinite(got[touched]).all() and excess <= 0.0, excess
    # tiles wholly above the diagonal: bit-identical to before the call
    assert torch.equal(_bits(got)[~touched], _bits(start)[~touched])
    if pad:
        assert torch.isnan(cbuf[:, M:]).all()


SYRK_CASES = [(M, K) for M in (1, 64, 65, 200) for K in (5, 32, 64)]


@pytest.mark.parametrize("alpha,beta", [(-1.0, 1.0), (0.5, 0.0)])
@pytest.mark.parametrize("M,K", [(65, 5), (200, 32)])
def test_dgemm_syrk_lower_cpu(M, K, alpha, beta):
    _check_syrk_lower(CPU, M, K, alpha, beta, pad=2)


@pytest.mark.gpu
@pytest.mark.parametrize("alpha,beta", [(-1.0, 1.0), (0.5, 0.0)])
@pytest.mark.parametrize("M,K", SYRK_CASES)
def test_dgemm_syrk_lower(gpu_device, M, K, alpha, beta):
    """The Cholesky trailing update called directly: tiles that touch the lower triangle meet the
    GEMM bound, tiles wholly above the diagonal are not written."""
    _check_syrk_lower(gpu_device, M, K, alpha, beta)


@pytest.mark.gpu
def test_dgemm_syrk_lower_strided(gpu_device):
    _check_syrk_lower(gpu_device, 200, 32, -1.0, 1.0, pad=5)
