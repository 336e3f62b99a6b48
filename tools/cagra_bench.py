"""CAGRA against IVF-Flat and IVF-PQ on one GPU: build time, warm search time and recall@10.

Items are the seeded Gaussian blobs of ``tools/ivfpq_bench.py`` (default 1M x 128 fp32 from 256
blobs, 10k queries, k 10; IVF: nlist 1024, nprobe 32, PQ M 32 with refine_ratio 4). Every timed
call ends in a device synchronise; the search time is the median of ``--reps`` runs after a
warm-up, with the configurations alternating inside every repetition. Recall is against the exact
search on the first ``--recall-queries`` queries. The graph build is split into its phases (kNN
graph, prune, merge). ``cagra_itopk64_seeds1024`` is itopk_size 64 with num_random_samplings 16
(``cagra_itopk128_seeds1024``: 128 with 8): the blobs are separate components of the kNN graph, so
a query is answered only when one of its seeds falls into its blob. Progress goes to stderr, the
one JSON line to stdout and ``--out``.

    python tools/cagra_bench.py --out profiles/cagra_vs_ivf.json
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


def say(*a):
    print(*a, file=sys.stderr, flush=True)


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
    ap.add_argument("--igd", type=int, default=128, help="intermediate_graph_degree")
    ap.add_argument("--gd", type=int, default=64, help="graph_degree")
    ap.add_argument("--build-algo", default="auto")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--rehearse", action="store_true", help="run the CPU paths at a tiny size: its times mean nothing")
    a = ap.parse_args()
    if not a.rehearse and not torch.cuda.is_available():
        raise SystemExit("cagra_bench needs a GPU: a CPU run gives no time (--rehearse checks the script only)")
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
           "M": a.M, "intermediate_graph_degree": a.igd, "graph_degree": a.gd, "build_algo": a.build_algo,
           "reps": a.reps,
           "device": "cpu rehearsal: no timing here is a measurement" if a.rehearse else torch.cuda.get_device_name(dev)}

    def dump():
        line = json.dumps(res)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    w = min(20000, a.rows)
    mk.build_ivf(X[:w], ids[:w], 64)  # code objects loaded before the timed builds
    mk.build_ivfpq(X[:w], ids[:w], 64, a.M, 8)
    mk.build_cagra(X[:w], ids[:w], min(a.igd, 32), min(a.gd, 16), "ivf")
    t_flat, flat = timed(lambda: mk.build_ivf(X, ids, a.nlist), dev)
    say("ivfflat build %.2f s" % t_flat)
    t_pq, pq = timed(lambda: mk.build_ivfpq(X, ids, a.nlist, a.M, 8), dev)
    say("ivfpq build %.2f s" % t_pq)
    phases = {}
    t_cg, cg = timed(lambda: mk.build_cagra(X, ids, a.igd, a.gd, a.build_algo, 1, phases=phases), dev)
    say("cagra build %.2f s" % t_cg, phases)
    res["build_s"] = {"ivfflat": t_flat, "ivfpq": t_pq, "cagra": t_cg}
    res["cagra_build_phase_s"] = phases
    res["graph_edges_per_row"] = float((cg.graph >= 0).sum().item()) / a.rows
    dump()

    def cagra(itopk, nrs=1):
        return lambda q: mk.cagra_knn(cg, q, a.k, (itopk, 1, 0, 0, nrs, 1), ctx)

    configs = {"ivfflat": lambda q: mk.ivf_knn(flat, q, a.k, a.nprobe, ctx),
               "ivfpq_refine4": lambda q: mk.ivfpq_knn(pq, q, a.k, a.nprobe, 4, ctx),
               "cagra_itopk32": cagra(32), "cagra_itopk64": cagra(64), "cagra_itopk128": cagra(128),
               "cagra_itopk64_seeds1024": cagra(64, 16), "cagra_itopk128_seeds1024": cagra(128, 8)}
    Qr = Q[: a.recall_queries]
    _, exact = mk.exact_knn(X, ids, Qr, a.k, ctx)
    res["recall_at_k"] = {}
    for name, fn in configs.items():
        _, got = fn(Qr)
        res["recall_at_k"][name] = float(np.mean([len(set(x.tolist()) & set(y.tolist())) / float(a.k)
                                                  for x, y in zip(got, exact)]))
    say("recall", res["recall_at_k"])
    dump()
    times = {name: [] for name in configs}
    for name, fn in configs.items():
        fn(Q)  # warm-up at the timed shape
    for _ in range(a.reps):
        for name, fn in configs.items():
            times[name].append(timed(lambda: fn(Q), dev)[0])
    res["search_s"] = {name: {"median": statistics.median(v), "min": min(v), "max": max(v)}
                       for name, v in times.items()}
    print(dump())


if __name__ == "__main__":
    main()
