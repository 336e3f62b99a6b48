"""The CSR Gram kernel (``ops.csr_gram``) against densify + H2D + ``ops.gram`` on one GPU.

Rows are seeded: ``--rows`` x ``--cols`` fp32 with round(density x cols) standard-normal non-zeros
per row (one in each of that many equal column strata, so the indices are sorted and unique). Per
density three configurations form the upper triangle of X^T X for the same rows:

* ``csr_t64`` / ``csr_t128``: ``ops.csr_gram`` at either tile width, the CSR arrays already on the
  device (their H2D, ``csr_h2d_s``, is timed apart);
* ``dense``: the only route before the kernel existed: row blocks densified on the host into a
  pinned buffer, copied to the device and accumulated with ``ops.gram`` (fp32 MFMA SYRK);
  ``dense_gram_s`` is the share of the SYRK alone on blocks already on the device.

Every timed call ends in a device synchronise; a time is the median of ``--reps`` runs after a
warm-up at the timed shape, the configurations alternating inside every repetition, min and max
reported as the spread. The results are compared (largest difference over the largest entry).

    python tools/csr_gram_bench.py --out profiles/csr_gram_vs_dense.json
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


def timed(fn, dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def strata_rows(m, n, density, seed):
    per = max(1, int(round(density * n)))
    width = n // per
    rng = np.random.default_rng(seed)
    cols = (np.arange(per, dtype=np.int32) * width)[None, :] + rng.integers(0, width, (m, per), dtype=np.int32)
    vals = rng.standard_normal((m, per), dtype=np.float32)
    return np.arange(m + 1, dtype=np.int64) * per, cols.reshape(-1), vals.reshape(-1), per


def dense_route(cols, vals, per, m, n, block, stage, dev, G, resident=None):
    """G (upper triangle) += X^T X through densified row blocks; ``resident``: blocks already on the device."""
    ops.zero_(G)
    for i, r0 in enumerate(range(0, m, block)):
        r = min(block, m - r0)
        if resident is not None:
            Xb = resident[i]
        else:
            host = stage[:r]
            host.zero_()
            hv = host.numpy()
            hv[np.repeat(np.arange(r), per), cols[r0 * per:(r0 + r) * per]] = vals[r0 * per:(r0 + r) * per]
            Xb = host.to(dev, non_blocking=True)
        ops.gram(Xb, None, out=G, finalize=False)
        if resident is None and dev.type == "cuda":
            torch.cuda.synchronize(dev)  # the pinned block is rewritten next
    return G


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--cols", type=int, default=3000)
    ap.add_argument("--density", type=float, nargs="+", default=[0.001, 0.01, 0.1])
    ap.add_argument("--block", type=int, default=65536, help="rows of one densified block")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--rehearse", action="store_true", help="run the CPU paths at a tiny size: its times mean nothing")
    a = ap.parse_args()
    if not a.rehearse and not torch.cuda.is_available():
        raise SystemExit("csr_gram_bench needs a GPU: a CPU run gives no time (--rehearse checks the script only)")
    dev = torch.device("cpu") if a.rehearse else torch.device("cuda", 0)
    m, n = a.rows, a.cols
    res = {"rows": m, "cols": n, "reps": a.reps, "block": a.block, "default_tile": ops.csr_gram_config()[0], "shapes": [],
           "device": "cpu rehearsal: no timing here is a measurement" if a.rehearse else torch.cuda.get_device_name(dev)}
    stage = torch.empty((min(a.block, m), n), dtype=torch.float32, pin_memory=dev.type == "cuda")
    Gd = torch.empty((n, n), dtype=torch.float64, device=dev)
    for density in a.density:
        indptr, cols, vals, per = strata_rows(m, n, density, 1)
        host = [torch.from_numpy(x) for x in (indptr, cols, vals)]
        t_h2d, arrs = timed(lambda: [t.to(dev) for t in host], dev)
        A = CSR(arrs[0], arrs[1], arrs[2], (m, n))
        configs = {"dense": lambda: dense_route(cols, vals, per, m, n, a.block, stage, dev, Gd)}
        for t in (64, 128):
            configs["csr_t%d" % t] = (lambda t=t: ops.csr_gram(A, tile=t))
        outs = {name: fn().clone() for name, fn in configs.items()}  # warm-up at the timed shape
        times = {name: [] for name in configs}
        for _ in range(a.reps):
            for name, fn in configs.items():
                times[name].append(timed(fn, dev)[0])
        # the SYRK alone, on as many resident blocks as fit beside the rest (first blocks, scaled)
        nres = max(1, min(-(-m // a.block), 4))
        resident = [torch.randn((min(a.block, m), n), dtype=torch.float32, device=dev) for _ in range(nres)]
        rows_res = nres * min(a.block, m)
        dense_route(cols, vals, per, rows_res, n, a.block, stage, dev, Gd, resident)
        syrk = statistics.median(timed(lambda: dense_route(cols, vals, per, rows_res, n, a.block, stage, dev, Gd,
                                                           resident), dev)[0] for _ in range(a.reps)) * m / rows_res
        del resident
        top = float(outs["csr_t64"].abs().max())
        med = {name: statistics.median(v) for name, v in times.items()}
        res["shapes"].append({
            "density": density, "nnz_per_row": per, "dense_bytes": m * n * 4, "csr_bytes": m * per * 8 + (m + 1) * 8,
            "csr_h2d_s": t_h2d, "dense_gram_s": syrk,
            "gram_s": {name: {"median": med[name], "min": min(v), "max": max(v)} for name, v in times.items()},
            "dense_over_csr_t64": med["dense"] / med["csr_t64"], "dense_over_csr_t128": med["dense"] / med["csr_t128"],
            "max_diff_over_max": {
                name: float((torch.triu(outs[name]) - torch.triu(outs["csr_t64"])).abs().max()) / max(top, 1e-300)
                for name in outs}})
        del A, arrs, outs
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
