"""IVF-PQ against IVF-Flat on one GPU: build time, warm search time and recall@10.

Items are seeded Gaussian blobs (default 1M x 128 fp32, 10k queries, nlist 1024, nprobe 32, k 10).
Every timed call ends in a device synchronise; the search time is the median of ``--reps`` runs
after a warm-up, with the configurations alternating inside every repetition. Recall is against
the exact search on the first ``--recall-queries`` queries. The PQ search is also split into its
phases (probe, table build + scan, exact re-score); "tables only" scans an index of the same
centres and codebooks that holds one row per list, so it is the table build plus launch overhead.

    python tools/ivfpq_bench.py --out profiles/ivfpq_vs_ivfflat.json
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
from spark_rapids_ml_nai_amd.models import knn as mk  # noqa: E402
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=128)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--n-bits", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--rehearse", action="store_true", help="run the CPU paths at a tiny size: its times mean nothing")
    a = ap.parse_args()
    if not a.rehearse and not torch.cuda.is_available():
        raise SystemExit("ivfpq_bench needs a GPU: a CPU run gives no time (--rehearse checks the script only)")
    dev = torch.device("cpu") if a.rehearse else torch.device("cuda", 0)
    ctx = WorkerContext.single(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    cen = 3.0 * torch.randn((256, a.cols), generator=g, device=dev)
    X = cen[torch.randint(0, 256, (a.rows,), generator=g, device=dev)] + torch.randn((a.rows, a.cols), generator=g,
                                                                                   device=dev)
    Q = cen[torch.randint(0, 256, (a.queries,), generator=g, device=dev)] + torch.randn((a.queries, a.cols),
                                                                                      generator=g, device=dev)
    ids = torch.arange(a.rows, dtype=torch.int64, device=dev)
    res = {"rows": a.rows, "cols": a.cols, "queries": a.queries, "nlist": a.nlist, "nprobe": a.nprobe, "k": a.k,
           "M": a.M, "n_bits": a.n_bits, "reps": a.reps,
           "device": "cpu rehearsal: no timing here is a measurement" if a.rehearse else torch.cuda.get_device_name(dev)}

    mk.build_ivf(X[:20000], ids[:20000], 64)  # code objects loaded before the timed builds
    mk.build_ivfpq(X[:20000], ids[:20000], 64, a.M, a.n_bits)
    t_flat, flat = timed(lambda: mk.build_ivf(X, ids, a.nlist), dev)
    t_pq, pq = timed(lambda: mk.build_ivfpq(X, ids, a.nlist, a.M, a.n_bits), dev)
    res["build_s"] = {"ivfflat": t_flat, "ivfpq": t_pq}

    configs = {"ivfflat": lambda q: mk.ivf_knn(flat, q, a.k, a.nprobe, ctx),
               "ivfpq_refine1": lambda q: mk.ivfpq_knn(pq, q, a.k, a.nprobe, 1, ctx),
               "ivfpq_refine4": lambda q: mk.ivfpq_knn(pq, q, a.k, a.nprobe, 4, ctx)}
    Qr = Q[: a.recall_queries]
    _, exact = mk.exact_knn(X, ids, Qr, a.k, ctx)
    res["recall_at_k"] = {}
    for name, fn in configs.items():
        _, got = fn(Qr)
        res["recall_at_k"][name] = float(np.mean([len(set(x.tolist()) & set(y.tolist())) / float(a.k)
                                                  for x, y in zip(got, exact)]))
    times = {name: [] for name in configs}
    for name, fn in configs.items():
        fn(Q)  # warm-up at the timed shape
    for _ in range(a.reps):
        for name, fn in configs.items():
            times[name].append(timed(lambda: fn(Q), dev)[0])
    res["search_s"] = {name: {"median": statistics.median(v), "min": min(v), "max": max(v)}
                       for name, v in times.items()}

    # phases of the PQ search (kc = 4 k)
    kc = 4 * a.k
    nl = pq.centroids.shape[0]
    one = mk.IVFPQIndex(pq.centroids, pq.cnorm, torch.arange(nl + 1, device=dev), pq.items[:nl], pq.ids[:nl],
                        pq.codebooks, pq.codes[:nl].contiguous())
    qn = ops.row_sqnorm(Q)
    _, probes = ops.knn(Q, pq.centroids, a.nprobe, inorm=pq.cnorm, qnorm=qn)
    pr = probes.int()
    _, pos = ops.ivfpq_search(Q, pr, pq.list_off, pq.centroids, pq.codebooks, pq.codes, kc)
    pos_ids = torch.arange(a.rows, dtype=torch.int64, device=dev)
    phases = {"probe": lambda: ops.knn(Q, pq.centroids, a.nprobe, inorm=pq.cnorm, qnorm=qn),
              "pq_tables_and_scan": lambda: ops.ivfpq_search(Q, pr, pq.list_off, pq.centroids, pq.codebooks, pq.codes,
                                                             kc),
              "pq_tables_only": lambda: ops.ivfpq_search(Q, pr, one.list_off, one.centroids, one.codebooks, one.codes,
                                                         kc),
              "refine": lambda: mk._refine_sorted(Q, pq.items, pos, "euclidean"),
              "ivfflat_scan": lambda: ops.ivf_search(Q, pr, flat.list_off, flat.items, flat.inorm, pos_ids, a.k,
                                                     qnorm=qn)}
    ptimes = {name: [] for name in phases}
    for fn in phases.values():
        fn()
    for _ in range(a.reps):
        for name, fn in phases.items():
            ptimes[name].append(timed(fn, dev)[0])
    res["phase_s"] = {name: statistics.median(v) for name, v in ptimes.items()}
    rows_scanned = float((pq.list_off[1:] - pq.list_off[:-1])[probes.reshape(-1)].sum().item())
    res["rows_scanned"] = rows_scanned
    res["bytes_scanned"] = {"ivfflat": rows_scanned * a.cols * 4, "ivfpq": rows_scanned * a.M}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
