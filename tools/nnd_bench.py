"""The approximate dense kNN graph in a non-Euclidean metric (``build_algo="metric_nn_descent"``)
against the exact chunked search on one GPU: recall per round, time per phase, the build-time ratio.

Rows are seeded and clustered: ``--rows`` x ``--cols`` fp32 around ``--clusters`` Gaussian centres
(centre scale 2, noise scale 1). One traced build gives the recall of the Euclidean candidates, of
round 0 and of each NN-descent round on ``--sample`` rows against ``ops.knn_metric`` (the unchanged
exact search) and the phases' times (each ends in a synchronise). Then the two builders alternate
inside every repetition; a time is the median of ``--reps`` runs after a warm-up at the timed shape,
min and max are kept.

    python tools/nnd_bench.py --out profiles/nnd_vs_exact.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spark_rapids_ml_nai_amd import ops  # noqa: E402
from spark_rapids_ml_nai_amd.models.knn_graph import build_knn_graph, knn_graph_metric_approx  # noqa: E402


def timed(fn, dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def recall(ids, lo, truth):
    return float((ids[lo: lo + truth.shape[0]].unsqueeze(2) == truth.unsqueeze(1)).any(2).sum()) / truth.numel()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--cols", type=int, default=64)
    ap.add_argument("--clusters", type=int, default=2000)
    ap.add_argument("--metric", default="manhattan")
    ap.add_argument("--p", type=float, default=2.0)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--nnd-iters", type=int, default=2)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--rehearse", action="store_true", help="run the CPU paths at a tiny size: its times mean nothing")
    a = ap.parse_args()
    if not a.rehearse and not torch.cuda.is_available():
        raise SystemExit("nnd_bench needs a GPU: a CPU run gives no time (--rehearse checks the script only)")
    dev = torch.device("cpu") if a.rehearse else torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    C = torch.randn((a.clusters, a.cols), generator=g, device=dev) * 2.0
    X = C[torch.arange(a.rows, device=dev) % a.clusters] + torch.randn((a.rows, a.cols), generator=g, device=dev)
    if ops.pairdist_metric(a.metric, a.p)[0] == "hellinger":
        X = X.abs() / X.abs().sum(1, keepdim=True)
    lo, size = a.rows // 3, min(a.rows, a.sample)
    truth = ops.knn_metric(X[lo: lo + size], X, a.k, a.metric, a.p)[1]
    kwds = {"nnd_iters": a.nnd_iters}
    rounds, phases = [], {}
    t, _ = timed(lambda: knn_graph_metric_approx(X, a.k, a.metric, a.p, seed=3, nnd_iters=a.nnd_iters, rounds=rounds,
                                                 phases=phases), dev)
    res = {"rows": a.rows, "cols": a.cols, "k": a.k, "metric": a.metric, "p": a.p, "clusters": a.clusters,
           "nnd_iters": a.nnd_iters, "reps": a.reps, "sample_rows": size,
           "device": "cpu rehearsal: no timing here is a measurement" if a.rehearse else torch.cuda.get_device_name(dev),
           "recall": {name: recall(ids, lo, truth) for name, _, ids in rounds},
           "phases_s": {name: v["s"] for name, v in phases.items()}, "traced_build_s": t}
    configs = {"metric_nn_descent": lambda: build_knn_graph(X, a.k, "metric_nn_descent", kwds, 3, metric=a.metric, p=a.p),
               "exact": lambda: build_knn_graph(X, a.k, "brute_force_knn", None, 3, metric=a.metric, p=a.p)}
    outs = {name: fn() for name, fn in configs.items()}  # warm-up at the timed shape
    times = {name: [] for name in configs}
    for _ in range(a.reps):
        for name, fn in configs.items():
            times[name].append(timed(fn, dev)[0])
    med = {name: statistics.median(v) for name, v in times.items()}
    res.update({"build_s": {name: {"median": med[name], "min": min(v), "max": max(v)} for name, v in times.items()},
                "exact_over_metric_nn_descent": med["exact"] / med["metric_nn_descent"],
                "recall_timed_graph": recall(outs["metric_nn_descent"][1], lo, truth),
                "recall_exact_builder": recall(outs["exact"][1], lo, truth)})
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
