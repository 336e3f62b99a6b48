"""The approximate sparse kNN graph (``build_algo="rp_nn_descent"``) against the exact CSR search on
one GPU: recall per stage, time per phase, and the build-time ratio.

Rows are seeded and clustered: ``--rows`` x ``--cols`` fp32, ``--clusters`` sparse centres of ``nnz``
columns each; a row keeps each of its centre's columns with probability 0.8 (value: the centre's
plus 0.3 x noise) and adds nnz / 5 columns of its own, so rows have about ``nnz`` non-zeros.

Per shape:

* for every ``--proj-dim`` one traced build: recall of the projected candidates, of round 0 (the
  candidates re-scored on the CSR rows) and of each NN-descent round, on ``--sample`` rows against
  ``ops.csr_knn`` (the unchanged exact search), and the phases' times (each ends in a synchronise);
* the build time of ``rp_nn_descent`` at ``--time-proj-dim`` against the exact builder
  (``build_knn_graph(..., "brute_force_knn")``): the two alternate inside every repetition, a time
  is the median of ``--reps`` runs after a warm-up at the timed shape, min and max are kept.

    python tools/csr_nnd_bench.py --out profiles/csr_nnd_vs_exact.json
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
from spark_rapids_ml_nai_amd.core.base import CSR  # noqa: E402
from spark_rapids_ml_nai_amd.models.knn_graph import (build_knn_graph, knn_graph_csr,  # noqa: E402
                                                      knn_graph_csr_approx)


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def timed(fn, dev):
    sync(dev)
    t0 = time.perf_counter()
    out = fn()
    sync(dev)
    return time.perf_counter() - t0, out


def clustered_rows(m, n, nnz, clusters, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    own = max(1, nnz // 5)
    ccols = torch.randint(0, n, (clusters, nnz), generator=g, device=dev)
    cvals = torch.randn((clusters, nnz), generator=g, device=dev) * 2.0
    keys, vals = [], []
    step = max(1, (1 << 24) // (nnz + own))
    for r0 in range(0, m, step):  # row chunks: the triples of a chunk sort within a fixed budget
        rows = torch.arange(r0, min(m, r0 + step), device=dev)
        c = rows % clusters
        keep = torch.rand((rows.numel(), nnz), generator=g, device=dev) < 0.8
        cols = torch.cat([ccols[c], torch.randint(0, n, (rows.numel(), own), generator=g, device=dev)], 1)
        v = torch.cat([cvals[c] + 0.3 * torch.randn((rows.numel(), nnz), generator=g, device=dev),
                       torch.randn((rows.numel(), own), generator=g, device=dev)], 1)
        ok = torch.cat([keep, torch.ones((rows.numel(), own), dtype=torch.bool, device=dev)], 1)
        key = (rows.view(-1, 1) * n + cols)[ok]
        key, o = torch.sort(key, stable=True)
        first = torch.ones_like(key, dtype=torch.bool)
        first[1:] = key[1:] != key[:-1]  # a column drawn twice: the first draw stays
        keys.append(key[first])
        vals.append(v[ok][o][first])
    key, val = torch.cat(keys), torch.cat(vals)
    val = torch.where(val == 0, torch.ones_like(val), val)
    rows = key // n
    indptr = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=m), 0)
    return CSR(indptr=indptr, indices=(key - rows * n).to(torch.int32), data=val.float().contiguous(), shape=(m, n))


def recall(ids, blocks, truth):
    hit = tot = 0
    for (lo, hi), t in zip(blocks, truth):
        got = ids[lo:hi]
        hit += int((got.unsqueeze(2) == t.unsqueeze(1)).any(2).sum())
        tot += t.numel()
    return hit / max(1, tot)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--cols", type=int, default=100000)
    ap.add_argument("--nnz", type=int, nargs="+", default=[30, 300])
    ap.add_argument("--clusters", type=int, default=2000)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--proj-dim", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--time-proj-dim", type=int, default=64)
    ap.add_argument("--nnd-iters", type=int, default=2)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--rehearse", action="store_true", help="run the CPU paths at a tiny size: its times mean nothing")
    a = ap.parse_args()
    if not a.rehearse and not torch.cuda.is_available():
        raise SystemExit("csr_nnd_bench needs a GPU: a CPU run gives no time (--rehearse checks the script only)")
    dev = torch.device("cpu") if a.rehearse else torch.device("cuda", 0)
    res = {"rows": a.rows, "cols": a.cols, "k": a.k, "reps": a.reps, "clusters": a.clusters, "nnd_iters": a.nnd_iters,
           "metric": "euclidean", "shapes": [],
           "device": "cpu rehearsal: no timing here is a measurement" if a.rehearse else torch.cuda.get_device_name(dev)}
    for nnz in a.nnz:
        A = clustered_rows(a.rows, a.cols, nnz, a.clusters, 1, dev)
        P = ops.csr_prepare(A, "sqeuclidean")
        nblk = max(1, min(8, a.sample // 512))
        size = min(a.rows, max(1, a.sample // nblk))
        g = torch.Generator().manual_seed(2)
        los = sorted(set(int(x) for x in torch.randint(0, max(1, a.rows - size + 1), (nblk,), generator=g)))
        blocks = [(lo, lo + size) for lo in los]
        truth = [knn_graph_csr(P.rows(lo, hi), P, a.k)[1] for lo, hi in blocks]
        shape = {"nnz_target": nnz, "nnz_per_row": float(A.data.numel()) / a.rows, "sample_rows": size * len(blocks),
                 "proj_dim": {}}
        for pd in a.proj_dim:
            rounds, phases = [], {}
            t, _ = timed(lambda: knn_graph_csr_approx(A, a.k, "euclidean", seed=3, proj_dim=pd, nnd_iters=a.nnd_iters,
                                                      rounds=rounds, phases=phases), dev)
            shape["proj_dim"][str(pd)] = {"recall": {name: recall(ids, blocks, truth) for name, _, ids in rounds},
                                          "phases_s": {name: v["s"] for name, v in phases.items()}, "build_s": t}
        configs = {"rp_nn_descent": lambda: build_knn_graph(A, a.k, "rp_nn_descent",
                                                            {"proj_dim": a.time_proj_dim, "nnd_iters": a.nnd_iters}, 3),
                   "exact": lambda: build_knn_graph(A, a.k, "brute_force_knn", None, 3)}
        outs = {name: fn() for name, fn in configs.items()}  # warm-up at the timed shape
        times = {name: [] for name in configs}
        for _ in range(a.reps):
            for name, fn in configs.items():
                times[name].append(timed(fn, dev)[0])
        med = {name: statistics.median(v) for name, v in times.items()}
        shape.update({"timed_proj_dim": a.time_proj_dim,
                      "build_s": {name: {"median": med[name], "min": min(v), "max": max(v)} for name, v in times.items()},
                      "exact_over_rp_nn_descent": med["exact"] / med["rp_nn_descent"],
                      "recall_timed_graph": recall(outs["rp_nn_descent"][1], blocks, truth),
                      "recall_exact_builder": recall(outs["exact"][1], blocks, truth)})
        res["shapes"].append(shape)
        del A, P, outs, truth
        line = json.dumps(res)
        if a.out:  # after every shape: a later shape that runs out of time keeps the earlier ones
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
