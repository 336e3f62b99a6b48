"""Seeded deterministic mode (SURVEY §5 "Sanitizers / deterministic mode").

The fast reductions accumulate with fp64/fp32 atomics (block partials folded in arrival order), so
their last bits can differ run to run. ``SRML_DETERMINISTIC=1`` (or ``set_deterministic(True)``,
or the Spark conf ``spark.rocm.ml.deterministic=true`` forwarded to the workers as the env var)
switches the affected kernels to fixed-order variants:

* KMeans cluster sums -> label-sorted segment sums, one block per (cluster, column chunk), no
  atomics (``srml_kmeans_segment_sums_*``); on CSR rows (``ops.csr_cluster_sums``) exact i64
  fixed-point integers added with integer atomics and converted to fp64 once, which also makes the
  sums independent of the row order;
* Gram / covariance (PCA, LinearRegression normal equations) -> each row chunk stores its
  partial tiles into a workspace (<= 64 chunks, <= 1 GB) folded in chunk order, instead of
  fp64 atomics (same fp32-per-chunk / fp64-across-chunk precision);
* fp64 GEMMs (``ops.dgemm``: X^T V, Krylov products) always fold split-K partials in index
  order, deterministic in either mode;
* LogisticRegression -> the two-pass path (residual stage + MFMA X^T R) with ordered block-partial
  folds instead of the fused atomics kernel;
* RandomForest regression histograms -> the cross-chunk fold adds exact i64 fixed-point integers
  (order-independent) converted to fp64 once (``srml_rf_hist_fixed``), node statistics one block
  per segment with a fixed-order reduction (``srml_rf_node_stats_det``); classification histograms
  are integer counts, exact in any order;
* UMAP layout epochs -> synchronous epochs (``ops.umap_epoch_sync`` / ``srml_umap_epoch_sync``)
  instead of the Hogwild kernel: every due edge reads the layout of the epoch's start, the head
  moves of a vertex are summed in edge order (in-wave segmented scan, then per-wave partial
  slots in ascending wave order: no float atomics, nothing read that the launch writes) and then
  applied. Only heads move, so a fit always takes the pull form (``SRML_UMAP_PULL=0`` is
  ignored) and a transform moves the new rows against the fixed training layout. On several
  ranks the ranks' summed moves are all-reduced and added. The dense spectral init takes its
  degrees from sorted-row sums instead of an atomic ``index_add_``.

Device RNG streams are counter-based and seeded
(k-means|| sampling, bootstrap, k-means++ draws, UMAP negative samples), so PCA, LinearRegression,
KMeans, LogisticRegression, RandomForestRegressor and UMAP fits on the same data and partitioning
are bit-reproducible with the flag on.

What the UMAP guarantee covers: ``random_state`` set (without it the mode warns: the drawn seed
cannot be repeated), the same device count, and one or two ranks — a two-term sum has one order;
more ranks rest on the collective's fixed reduction order and are not tested. The
``brute_force_knn`` (``auto`` up to 100k rows) and ``precomputed_knn`` graphs, the fuzzy set, the
categorical intersection and both spectral inits are fixed-order by construction. The ``ivf`` /
``nn_descent`` builders hand out candidate slots in arrival order and then select an
order-independent top k: their graphs were bit-equal in every repeated build tried (12k and 200k
rows) and are in the fit test, but rows with exactly tied neighbour distances could in principle
come out in either order. The Jacobi eigensolver of the dense spectral init (n <= 2048) measures
convergence with an atomic sum: a sweep more or less would need that sum to straddle the
tolerance in its last bits; it did not in any repeat. ``random_state`` alone does not turn the
mode on: the default epochs stay Hogwild.
"""
from __future__ import annotations

import os
from typing import Optional

_override: Optional[bool] = None


def deterministic() -> bool:
    if _override is not None:
        return _override
    return os.environ.get("SRML_DETERMINISTIC", "0") == "1"


def set_deterministic(flag: Optional[bool]) -> None:
    """Force the mode on/off for this process (None: follow ``SRML_DETERMINISTIC``)."""
    global _override
    _override = flag
