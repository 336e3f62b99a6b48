"""Distributed linear support-vector classifier (Spark ``LinearSVC`` / cuML ``LinearSVC``).

Objective: f(w, b) = 1/m sum_r l(y'_r z_r) + regParam/2 ||w||^2 with y' = 2y - 1, z = w.x + b, the
intercept unpenalised, and l the hinge max(0, 1 - y'z) (Spark's loss; strict kink: a row with
y'z == 1 contributes nothing) or the squared hinge max(0, 1 - y'z)^2 (cuML's default).
``standardization`` follows Spark's L2 rule (``logistic._problem`` with l1_ratio = 0): the penalty
acts on the sigma-scaled coefficients, constant columns get coefficient 0.

Every evaluation is ONE pass over the resident shard on the binary GLM kernels instantiated with
the support-vector terms (``ops.svc_loss_grad``), one all-reduce of [grad w | grad b | loss], and
the device-resident L-BFGS of ``models/qn.py``; the start point is theta = 0.

``SRML_DETERMINISTIC=1``: device fits run the ordered two-pass path (bit-identical run to run at a
fixed number of ranks). Fits on the host path (CPU tensors, gloo ranks) go further: the column
moments and every sum of the data term run on a fixed-point grid (``ops.exact_sum``), so a fit on
any number of ranks equals the one-rank fit on the same rows bit for bit.
"""
from __future__ import annotations

from typing import Any, Dict, Optional

import numpy as np
import torch

from .. import ops
from ..parallel.context import WorkerContext
from .logistic import GRAPH_MAX_BYTES, _eval_bytes, _problem, logistic_stats
from ..utils.determinism import deterministic
from .qn import minimize


def svc_stats(X: Any, y: torch.Tensor, m_total: int, ctx: WorkerContext, sparse: bool) -> Dict[str, Any]:
    """Column std-devs for the fit, after checking that every rank's labels are 0 / 1: the ranks
    agree on the verdict first, so all of them raise the same error."""
    bad = torch.tensor([1.0 if bool(((y != 0) & (y != 1)).any()) else 0.0], dtype=torch.float64, device=y.device)
    ctx.comm.allreduce(bad, op="max")
    if bad.item() > 0:
        raise ValueError("LinearSVC only supports binary classification: labels must be 0 or 1")
    stats = logistic_stats(X, y, m_total, ctx, sparse)
    if deterministic() and ops.svc_path(X) == "torch-cpu":
        # deterministic mode on the host path: the column moments on the fixed-point grid of
        # ops.exact_sum, so sigma (and with it the whole fit) is bit-identical for any split of the
        # rows over ranks. The maxima are exact under any split; the grid follows from them.
        Xd = (ops._csr_torch(X).to_dense() if sparse else X).double()
        n = Xd.shape[1]
        xmax = Xd.abs().max(0).values if Xd.shape[0] else torch.zeros(n, dtype=torch.float64)
        ctx.comm.allreduce(xmax, op="max")
        buf = torch.cat([ops.exact_sum(Xd, m_total * xmax), ops.exact_sum(Xd * Xd, m_total * xmax * xmax)])
        ctx.comm.allreduce(buf)
        mean = (buf[:n] / m_total).numpy()
        var = np.maximum((buf[n:] / m_total).numpy() - mean * mean, 0.0) * m_total / max(m_total - 1, 1)
        stats.update(sigma=np.sqrt(var), mean=mean, xmax=xmax)
    return stats


def svc_fit(X: Any, y: torch.Tensor, m_total: int, ctx: WorkerContext, reg: float, fit_intercept: bool,
            standardization: bool, max_iter: int, tol: float, loss: str = "hinge", sparse: bool = False,
            stats: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
    if loss not in ops.SVC_LOSSES:
        raise ValueError(f"loss must be 'hinge' or 'squared_hinge', got {loss!r}")
    n = X.shape[1]
    if stats is None:
        stats = svc_stats(X, y, m_total, ctx, sparse)
    P, theta0, inv_sigma = _problem(n, m_total, stats, reg, 0.0, fit_intercept, standardization, max_iter, tol, 1)
    theta0 = np.zeros_like(theta0)  # Spark's LinearSVC has no log-odds initial intercept
    y32 = (y if y.dtype == torch.float32 else y.to(torch.float32)).contiguous()
    path = ops.svc_path(X)
    ws = ops.logreg_workspace(X) if path == "fused_svc_f32" else None  # this fit's own partial rows

    # deterministic mode on the host path (svc_stats): order-independent sums
    exact = (stats["xmax"], m_total) if "xmax" in stats and path == "torch-cpu" else None

    def evaluate(w: torch.Tensor, b: torch.Tensor, flag: Optional[torch.Tensor], out: torch.Tensor) -> None:
        ops.svc_loss_grad(X, y32, w, b, out, flag, loss=loss, ws=ws, exact=exact)

    allreduce = ctx.comm.allreduce if ctx.distributed else None
    fold = evaluate_partials = None
    if ws is not None and allreduce is None:
        # one rank: the evaluation leaves its per-block partial rows, the fused optimiser step folds them
        parts, wst = ops.logreg_fold_layout(X)
        fold = (ws, parts, wst)
        _scratch = ops.zeros(n + 2, dtype=torch.float64, device=X.device)

        def evaluate_partials(w: torch.Tensor, b: torch.Tensor, flag: Optional[torch.Tensor]) -> None:
            ops.svc_loss_grad(X, y32, w, b, _scratch, flag, loss=loss, ws=ws, leave_partials=True)
    graph_safe = ((path in ("fused_svc_f32", "csr_svc", "two_pass_svc_f32") or path.startswith("lds_svc"))
                  and _eval_bytes(X) <= GRAPH_MAX_BYTES)
    res = minimize(P, theta0, evaluate, allreduce, y.device, batch=8 if path != "torch-cpu" else 2,
                   graph_safe=graph_safe, fold=fold, evaluate_partials=evaluate_partials)
    theta = res["theta"]
    if ctx.world_size > 1:  # every rank holds the same state; make the model bit-identical anyway
        th = torch.from_numpy(theta).to(ctx.device)
        ctx.comm.broadcast(th, 0)
        theta = th.cpu().numpy()
    dtype = "float32" if (X.dtype if not sparse else X.data.dtype) == torch.float32 else "float64"
    return {"coef_": (theta[:n] * inv_sigma).tolist(), "intercept_": float(theta[n]) if fit_intercept else 0.0,
            "n_cols": int(n), "dtype": dtype, "num_iters": int(res["iter"]), "objective": float(res["f"]),
            "_solver": {"n_evals": int(res["n_evals"]), "status": res["status"], "path": path}}
