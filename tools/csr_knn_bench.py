"""The sparse (CSR x CSR) exact kNN graph against densify-and-search on one GPU.

Rows are seeded: ``--rows`` x ``cols`` fp32 with round(density x cols) standard-normal non-zeros per
row (one in each of that many equal column strata, so the indices are sorted and unique). Two
configurations build the all-points k-nearest-neighbour graph of the same rows:

* ``csr``:   ``ops.csr_prepare`` (validation, norms) + ``ops.csr_knn`` + ``ops.csr_refine_sort``;
* ``dense``: ``ops.knn`` + ``ops.knn_refine_sort`` on the densified rows, the path a sparse column
  takes with ``enable_sparse_data_optim=False``; the densification itself is timed apart.

Every timed call ends in a device synchronise; a time is the median of ``--reps`` runs after a
warm-up at the timed shape, the configurations alternating inside every repetition. The two
graphs are compared (share of rows with the same neighbour set).

    python tools/csr_knn_bench.py --out profiles/csr_knn_vs_dense.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spark_rapids_ml_nai_amd import ops  # noqa: E402
from spark_rapids_ml_nai_amd.core.base import CSR  # noqa: E402
from spark_rapids_ml_nai_amd.models.knn_graph import refine_sorted  # noqa: E402


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def timed(fn, dev):
    sync(dev)
    t0 = time.perf_counter()
    out = fn()
    sync(dev)
    return time.perf_counter() - t0, out


def strata_rows(m, n, density, seed, dev):
    per = max(1, int(round(density * n)))
    width = n // per
    rng = np.random.default_rng(seed)
    cols = (np.arange(per, dtype=np.int64) * width)[None, :] + rng.integers(0, width, (m, per))
    vals = rng.standard_normal((m, per)).astype(np.float32)
    indptr = np.arange(m + 1, dtype=np.int64) * per
    return CSR(indptr=torch.from_numpy(indptr).to(dev), indices=torch.from_numpy(cols.astype(np.int32).reshape(-1)).to(dev),
               data=torch.from_numpy(vals.reshape(-1)).to(dev), shape=(m, n)), per


def csr_graph(A, k):
    P = ops.csr_prepare(A, "sqeuclidean")
    _, ids = ops.csr_knn(P, P, k, "sqeuclidean")
    return ops.csr_refine_sort(P, P, ids)


def dense_graph(X, k):
    _, ids = ops.knn(X, X, k, inorm=ops.row_sqnorm(X))
    return refine_sorted(X, X, ids)  # ops.knn_refine_sort on the device


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--cols", type=int, nargs="+", default=[8192, 32768])
    ap.add_argument("--density", type=float, nargs="+", default=[0.001, 0.01])
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--rehearse", action="store_true", help="run the CPU paths at a tiny size: its times mean nothing")
    a = ap.parse_args()
    if not a.rehearse and not torch.cuda.is_available():
        raise SystemExit("csr_knn_bench needs a GPU: a CPU run gives no time (--rehearse checks the script only)")
    dev = torch.device("cpu") if a.rehearse else torch.device("cuda", 0)
    res = {"rows": a.rows, "k": a.k, "reps": a.reps, "shapes": [],
           "device": "cpu rehearsal: no timing here is a measurement" if a.rehearse else torch.cuda.get_device_name(dev)}
    for n in a.cols:
        for density in a.density:
            A, per = strata_rows(a.rows, n, density, 1, dev)
            ops.csr_prepare(A, "sqeuclidean").to_dense()  # warm-up
            t_dense_copy, X = timed(lambda: ops.csr_prepare(A, "sqeuclidean").to_dense(), dev)
            configs = {"csr": lambda: csr_graph(A, a.k), "dense": lambda: dense_graph(X, a.k)}
            outs = {name: fn() for name, fn in configs.items()}  # warm-up at the timed shape
            times = {name: [] for name in configs}
            for _ in range(a.reps):
                for name, fn in configs.items():
                    times[name].append(timed(fn, dev)[0])
            same = (torch.sort(outs["csr"][1], dim=1).values == torch.sort(outs["dense"][1], dim=1).values).all(1)
            med = {name: statistics.median(v) for name, v in times.items()}
            res["shapes"].append({
                "cols": n, "density": density, "nnz_per_row": per, "dense_bytes": a.rows * n * 4,
                "csr_bytes": a.rows * per * 8 + (a.rows + 1) * 8, "densify_s": t_dense_copy,
                "graph_s": {name: {"median": med[name], "min": min(v), "max": max(v)} for name, v in times.items()},
                "dense_over_csr": med["dense"] / med["csr"], "same_neighbour_sets": float(same.double().mean())})
            del X, A, outs
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
