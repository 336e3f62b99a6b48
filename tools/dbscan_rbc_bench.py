"""DBSCAN ``algorithm="rbc"`` (ball-cover tile pruning) against ``"brute"`` on one GPU.

Workload: the blobs of ``tools/kbench.py`` (50 centres x std 8, unit noise, eps 10, min_samples 5) at
``--rows`` x 64, and one unclustered case (uniform rows in [-8, 8]^64, where nothing can be pruned:
rbc's overhead over brute there is the price of the feature). Per size and algorithm:

* ``fit_s``: ``dbscan_fit_predict`` wall time, every call ending in a device synchronise, after a
  warm-up at the timed shape, the two algorithms alternating inside every repetition; median, min
  and max of ``--reps`` runs;
* ``tile_pairs``: (visited, total);
* rbc only: the time of the ordering, balls and pair-list steps, and of the two sweeps with their rate
  visited x 128^2 x n x 2 operations over the sweep's time.

The two label vectors are compared; they must be identical.

    python tools/dbscan_rbc_bench.py --out profiles/dbscan_rbc_vs_brute.json
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
from spark_rapids_ml_nai_amd.models import dbscan as mdl  # noqa: E402
from spark_rapids_ml_nai_amd.parallel.context import WorkerContext  # noqa: E402


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def timed(fn, dev):
    sync(dev)
    t0 = time.perf_counter()
    out = fn()
    sync(dev)
    return time.perf_counter() - t0, out


def rows_of(kind, N, n, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    if kind == "uniform":
        return (torch.rand(N, n, device=dev, generator=g) * 16.0 - 8.0).contiguous()
    C = torch.randn(50, n, device=dev, generator=g) * 8
    return C[torch.randint(0, 50, (N,), device=dev, generator=g)] + torch.randn(N, n, device=dev, generator=g)


def rbc_steps(X, eps, ms, dev):
    """The steps of the rbc path one by one, each synchronised (the fit itself does not synchronise between them)."""
    Xc, xn, eps2 = mdl._prepare(X, eps, "euclidean")
    n = X.shape[1]
    t_order, perm = timed(lambda: mdl._rbc_order(Xc, xn), dev)
    Xp, xnp = Xc[perm.long()].contiguous(), xn[perm.long()].contiguous()
    band = (1.5 * n + 8.0) * 2.0 ** -24 * 4.0 * float(xn.max().item())
    t_balls, (C, r, cn) = timed(lambda: ops.dbscan_tile_balls(Xp), dev)
    t_pairs, pairs = timed(lambda: ops.dbscan_tile_pairs(C, r, cn, eps2, band), dev)
    v = int(pairs.shape[0])
    t_deg, counts = timed(lambda: ops.dbscan_degree_list(Xp, xnp, eps2, pairs, 0, v, perm), dev)
    core = (counts >= ms).to(torch.uint8)
    parent = torch.arange(X.shape[0], dtype=torch.int32, device=dev)
    best = torch.full((X.shape[0],), -1, dtype=torch.int64, device=dev)
    t_link, _ = timed(lambda: ops.dbscan_link_list(Xp, xnp, eps2, pairs, 0, v, perm, core, parent, best), dev)
    flop = v * 128.0 * 128.0 * n * 2.0
    return {"order_s": t_order, "balls_s": t_balls, "pairs_s": t_pairs, "degree_sweep_s": t_deg, "link_sweep_s": t_link,
            "degree_sweep_tflops": flop / t_deg / 1e12, "link_sweep_tflops": flop / t_link / 1e12}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[200_000, 1_000_000])
    ap.add_argument("--uniform-rows", type=int, default=200_000)
    ap.add_argument("--cols", type=int, default=64)
    ap.add_argument("--eps", type=float, default=10.0)
    ap.add_argument("--min-samples", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--rehearse", action="store_true", help="run the CPU paths at a tiny size: its times mean nothing")
    a = ap.parse_args()
    if not a.rehearse and not torch.cuda.is_available():
        raise SystemExit("dbscan_rbc_bench needs a GPU: a CPU run gives no time (--rehearse checks the script only)")
    dev = torch.device("cpu") if a.rehearse else torch.device("cuda", 0)
    ctx = WorkerContext.single(dev)
    res = {"cols": a.cols, "eps": a.eps, "min_samples": a.min_samples, "reps": a.reps, "cases": [],
           "device": "cpu rehearsal: no timing here is a measurement" if a.rehearse else torch.cuda.get_device_name(dev)}
    for kind, N in [("blobs", N) for N in a.rows] + [("uniform", a.uniform_rows)]:
        X = rows_of(kind, N, a.cols, dev)
        stats = {"brute": {}, "rbc": {}}

        def fit(alg):
            return mdl.dbscan_fit_predict(X, ctx, a.eps, a.min_samples, "euclidean", alg, stats[alg])[0]

        labels = {alg: fit(alg) for alg in stats}  # warm-up at the timed shape
        times = {alg: [] for alg in stats}
        for _ in range(a.reps):
            for alg in stats:
                times[alg].append(timed(lambda: fit(alg), dev)[0])
        med = {alg: statistics.median(v) for alg, v in times.items()}
        res["cases"].append({
            "rows": kind, "N": N, "clusters": int(labels["brute"].max()) + 1, "noise": int((labels["brute"] == -1).sum()),
            "labels_identical": bool(np.array_equal(labels["brute"], labels["rbc"])),
            "fit_s": {alg: {"median": med[alg], "min": min(v), "max": max(v)} for alg, v in times.items()},
            "tile_pairs": {alg: list(stats[alg]["tile_pairs"]) for alg in stats},
            "brute_over_rbc": med["brute"] / med["rbc"], "rbc_steps": rbc_steps(X, a.eps, a.min_samples, dev)})
        del X
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
