"""Silhouette score of a clustering (``ClusteringEvaluator``), Spark's closed form in two passes.

Pass 1 merges the per-cluster summaries of every partition in fp64 (``ops.silhouette_sums``: N, the
weighted sums; squaredEuclidean then adds Psi', the centred second moments about the merged global
mean, ``ops.silhouette_psi``). Pass 2 scores every row against the k summaries on the fused MFMA
kernel (``ops.silhouette``) and adds (sum of w s, sum of w) per partition. The partitions are placed
on the device once and stay resident between the passes: a pass over resident rows costs a
fraction of their host-to-device copy. A partition whose features are a ``scipy.sparse.csr_matrix``
stays CSR on the device and takes the CSR kernels of the same three ops (``csrc/csr_silhouette.hip``).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import scipy.sparse as sp
import torch

from .. import ops

# features (m, n) dense or scipy.sparse.csr_matrix, predictions (m), weights (m)
Partition = Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]


def _dense_ids(parts: List[Partition]) -> Tuple[List[Partition], List[np.ndarray], int]:
    """Drop the weightless rows and map the prediction values (any numbers) to ids 0..k-1."""
    kept: List[Partition] = []
    for X, pred, w in parts:
        pred = np.asarray(pred, np.float64).reshape(-1)
        if w is not None:
            w = np.asarray(w, np.float64).reshape(-1)
            if not (np.isfinite(w) & (w >= 0)).all():
                raise ValueError("ClusteringEvaluator: weights must be finite and non-negative")
            live = w > 0
            if not live.all():
                X, pred, w = X[live], pred[live], w[live]
        if len(pred):
            kept.append((X, pred, w))
    values = np.unique(np.concatenate([p[1] for p in kept])) if kept else np.zeros(0)
    if len(values) < 2:
        raise ValueError("ClusteringEvaluator: Number of clusters must be greater than one")
    return kept, [np.searchsorted(values, p[1]).astype(np.int32) for p in kept], len(values)


def silhouette_score(parts: List[Partition], measure: str, device: torch.device) -> float:
    """Weighted mean silhouette of the rows of ``parts`` under ``measure``."""
    from ..core.base import to_device

    if measure not in ops.SILHOUETTE_MEASURES:
        raise ValueError("ClusteringEvaluator: distanceMeasure must be one of %s, got %r"
                         % (ops.SILHOUETTE_MEASURES, measure))
    kept, ids, k = _dense_ids(parts)
    # a scipy CSR partition goes to the device as CSR (core.base.CSR) and is scored by the CSR kernels
    dev = [(to_device(X.sorted_indices() if sp.issparse(X) else np.ascontiguousarray(X, np.float32), device,
                      torch.float32),
            torch.from_numpy(lab).to(device),
            torch.from_numpy(w).to(device) if w is not None else None) for (X, _, w), lab in zip(kept, ids)]
    N = Y = None
    for X, lab, w in dev:
        n_p, y_p = ops.silhouette_sums(X, lab, k, w, measure)
        N, Y = (n_p, y_p) if N is None else (N + n_p, Y + y_p)
    psi = None
    if measure != "cosine":
        mu = ops.silhouette_centre(N, Y)
        for X, lab, w in dev:
            p_p = ops.silhouette_psi(X, lab, k, mu, w)
            psi = p_p if psi is None else psi + p_p
    tot = torch.zeros(2, dtype=torch.float64, device=device)
    for X, lab, w in dev:
        sws, sw = ops.silhouette(X, lab, k, w, measure, stats=(N, Y, psi))
        tot += torch.stack([sws, sw])
    sws, sw = tot.tolist()
    return sws / sw
