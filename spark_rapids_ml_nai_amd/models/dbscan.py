"""Distributed DBSCAN (reference: ``DBSCANModel._transform`` + cuML ``DBSCANMG.fit_predict``,
``clustering.py:940-1091``).

The reference collects the whole dataset on the driver and broadcasts it (C21). Here every rank
all-gathers the rows over RCCL (each MI355X holds the full matrix in its 288 GB), takes a
contiguous share of the lower-triangle 128x128 tile pairs and runs two fused MFMA sweeps:
  1. eps-degrees -> all-reduce SUM -> core flags (degree >= min_samples, self included);
  2. core-core edges -> per-rank union-find forest (+ nearest core neighbour of border points);
the forests are all-gathered and merged on device (every rank ends with identical roots = the
smallest core index of each component), border keys all-reduced with MIN. Labels are numbered
by ascending root, i.e. in order of each cluster's first core point (sklearn's numbering);
noise is -1.

``algorithm="rbc"`` (ball cover): the rows are grouped by nearest landmark so that a tile is a compact
ball, the tile pairs whose balls are further apart than eps (plus the fp32 form's error band) are
dropped on the device, and the two sweeps run over the surviving list only, each rank on its share of
that list. Results are indexed by original row id throughout, so the answers are those of brute.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from .. import ops
from ..parallel.context import WorkerContext


def _share(total: int, rank: int, world: int) -> Tuple[int, int]:
    b = np.linspace(0, total, world + 1).astype(np.int64)
    return int(b[rank]), int(b[rank + 1])


def _prepare(X: torch.Tensor, eps: float, metric: str) -> Tuple[torch.Tensor, torch.Tensor, float]:
    """(rows, their squared norms, squared threshold) the tile sweeps run on; X is the full matrix.

    euclidean: the rows minus their column mean. DBSCAN is translation invariant, the expanded form
    ||a||^2 + ||b||^2 - 2 a.b of the sweeps is not: its fp32 error grows with the norms, so they are
    taken about the data's own centre. Every rank holds the same matrix and reduces it in the same
    order, so the centre is the same on every rank.
    cosine: unit rows, ||a - b||^2 = 2 (1 - cos). An all-zero row stays zero and gets the norm 1, so it
    is at ||0||^2 + ||b||^2 - 0 = 2, cosine distance 1, from every row but itself (sklearn's rule)."""
    if metric == "cosine":
        nrm = X.norm(dim=1, keepdim=True)
        X = X / nrm.clamp_min(1e-30)
        xn = ops.row_sqnorm(X)
        xn = torch.where(nrm.view(-1) == 0, torch.ones_like(xn), xn)
        return X, xn, 2.0 * float(eps)
    if metric in ("euclidean", "l2"):
        if X.shape[0]:
            X = (X - X.mean(0, dtype=torch.float64).float()).contiguous()
        return X, ops.row_sqnorm(X), float(eps) ** 2
    raise ValueError("Unsupported metric %r for DBSCAN" % metric)


RBC_MAX_LANDMARKS = 16384


def _rbc_order(X: torch.Tensor, xn: torch.Tensor) -> torch.Tensor:
    """Permutation (position -> row id, int32) that groups the rows by nearest landmark, so that a
    128-row tile of ``X[perm]`` is a compact ball. Landmarks: L = min(T, 16384) rows at a fixed stride.
    Neighbouring groups should be neighbours in space too (a tile that straddles two groups far apart is a
    ball that reaches everything), so the landmarks are ranked first: ceil(sqrt(L)) of them serve as
    second-level landmarks, and a landmark's rank is its place in the order (nearest second-level
    landmark, distance to it). The rows are then sorted by the unique keys (landmark rank << 32 | row):
    the order depends on ``X`` alone, every rank holds the same matrix and gets the same permutation.
    The grouping only affects how many tile pairs survive the pruning, never the result."""
    N = X.shape[0]
    T = (N + ops.DB_TILE - 1) // ops.DB_TILE
    L = min(T, RBC_MAX_LANDMARKS)
    lm = X[:: N // L][:L].contiguous()
    L2 = int(np.ceil(np.sqrt(L)))
    top, dtop = ops.nearest_centroid(lm, lm[:: L // L2][:L2].contiguous())
    # a distance >= 0 orders as its bits; the mask keeps a -0.0 out of the high word
    lkeys = (top.long() << 32) | (dtop.contiguous().view(torch.int32).long() & 0xFFFFFFFF)
    order = torch.arange(L, dtype=torch.int32, device=X.device)
    ops.radix_sort_pairs(lkeys, order, 32 + max(1, int(L2).bit_length()))
    rank = torch.empty(L, dtype=torch.int64, device=X.device)
    rank[order.long()] = torch.arange(L, dtype=torch.int64, device=X.device)
    owner, _ = ops.nearest_centroid(X, lm, xnorm=xn)
    perm = torch.arange(N, dtype=torch.int32, device=X.device)
    keys = (rank[owner.long()] << 32) | perm.long()
    ops.radix_sort_pairs(keys, perm, 32 + max(1, int(L).bit_length()))
    return perm


def _rbc_pairs(X: torch.Tensor, xn: torch.Tensor, eps2: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                                                                         torch.Tensor]:
    """(Xp, xnp, perm, pairs): the rows in ball order and the ascending list of the tile pairs of ``Xp`` that
    can hold a pair the brute sweep counts (``ops.dbscan_tile_pairs``). ``band`` widens eps2 by the expanded
    form's own error bound c(n) 2^-24 (2 R)^2, R the largest row norm, so no pair the brute sweep could
    still count is pruned: the two algorithms return the same labels, not merely both valid ones."""
    n = X.shape[1]
    perm = _rbc_order(X, xn)
    Xp = X[perm.long()].contiguous()
    xnp = xn[perm.long()].contiguous()
    band = (1.5 * n + 8.0) * 2.0 ** -24 * 4.0 * float(xn.max().item())
    centres, radii, cnorm = ops.dbscan_tile_balls(Xp)
    return Xp, xnp, perm, ops.dbscan_tile_pairs(centres, radii, cnorm, eps2, band)


def dbscan_fit_predict(X_local: torch.Tensor, ctx: WorkerContext, eps: float, min_samples: int,
                       metric: str = "euclidean", algorithm: str = "brute",
                       stats: Optional[Dict[str, Any]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(labels of this rank's rows, core-sample flags of this rank's rows). ``algorithm="rbc"`` (more than two
    row tiles): the two sweeps visit only the tile pairs whose balls can hold a neighbour; the answers
    are those of ``"brute"``. ``stats["tile_pairs"]`` receives (visited, total) tile pairs over all ranks."""
    parts = ctx.comm.allgatherv(X_local.float().contiguous())
    sizes = [p.shape[0] for p in parts]
    start = sum(sizes[: ctx.rank])
    X = torch.cat([p.to(X_local.device) for p in parts], 0).contiguous()
    N = X.shape[0]
    X, xn, eps2 = _prepare(X, eps, metric)
    total = ops.dbscan_num_tiles(N)
    parent = torch.arange(N, dtype=torch.int32, device=X.device)
    best = torch.full((N,), -1, dtype=torch.int64, device=X.device)
    if algorithm == "rbc" and N > 2 * ops.DB_TILE:
        Xp, xnp, perm, pairs = _rbc_pairs(X, xn, eps2)
        visited = int(pairs.shape[0])
        l0, l1 = _share(visited, ctx.rank, ctx.world_size)
        counts = ops.dbscan_degree_list(Xp, xnp, eps2, pairs, l0, l1, perm)
        ctx.comm.allreduce(counts)
        core = (counts >= int(min_samples)).to(torch.uint8)
        ops.dbscan_link_list(Xp, xnp, eps2, pairs, l0, l1, perm, core, parent, best)
    else:
        visited = total
        t0, t1 = _share(total, ctx.rank, ctx.world_size)
        counts = ops.dbscan_degree(X, xn, eps2, t0, t1)
        ctx.comm.allreduce(counts)
        core = (counts >= int(min_samples)).to(torch.uint8)
        ops.dbscan_link(X, xn, eps2, t0, t1, core, parent, best)
    if stats is not None:
        stats["tile_pairs"] = (visited, total)
    if ctx.world_size > 1:
        ctx.comm.allreduce(best, op="min")
        forests = ctx.comm.allgather(parent.view(1, -1))
        for r in range(ctx.world_size):
            if r != ctx.rank:
                ops.uf_unite_pairs(parent, forests[r].to(X.device))
    ops.uf_compress(parent)
    # clusters numbered by ascending root (root-flag prefix scan on the device)
    labels = ops.dbscan_labels(parent, core, best)
    sl = slice(start, start + X_local.shape[0])
    return labels[sl].cpu().numpy(), core[sl].bool().cpu().numpy()
