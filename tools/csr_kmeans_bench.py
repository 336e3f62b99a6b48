"""One Lloyd iteration of sparse KMeans on one GPU, its two passes timed apart.

Rows are seeded synthetic CSR: ``rows`` x ``cols`` fp32, Poisson(``nnz``) standard-normal non-zeros
per row at sorted distinct random columns; the k centres are the means of k random row groups (dense,
as a running fit's are). Timed, each as the median of ``--reps`` runs after a warm-up at the timed
shape, every run ending in a device synchronise:

* ``search``:     ``ops.csr_nearest_centroid`` (centre transpose / padding kernel included: a fit pays it
  every iteration, into a table it keeps) and, apart, the kernel launches alone on prepared centres;
* ``sums``:       ``ops.csr_cluster_sums`` with fp64 atomics;
* ``sums_fixed``: the same in deterministic mode (i64 fixed-point atomics + conversion, the max|x|
  pass included);
* ``--dense``:    the dense route's search + sums on the densified rows (``ops.nearest_centroid`` +
  ``ops.cluster_sums``), for shapes where rows x cols x 4 bytes fit.

Printed with the byte models: the search reads nnz x kp x 4 B of centre rows plus one pass over the
CSR (12 B per non-zero); the sums add 8 B per non-zero.

    python tools/csr_kmeans_bench.py --shape 1000000 65536 50 100 --shape 1000000 65536 50 1000 \\
        --shape 200000 4096 41 256 --dense 200000 --out profiles/csr_kmeans.json
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
from spark_rapids_ml_nai_amd.utils.determinism import set_deterministic  # noqa: E402


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def timed(fn, dev):
    sync(dev)
    t0 = time.perf_counter()
    out = fn()
    sync(dev)
    return time.perf_counter() - t0, out


def poisson_rows(m, n, nnz, seed, dev):
    """CSR with Poisson row lengths (at least 1): columns drawn with replacement and de-duplicated per
    row by sorting (row, column) keys, so the indices are sorted and distinct."""
    rng = np.random.default_rng(seed)
    counts = np.clip(rng.poisson(nnz, m), 1, n).astype(np.int64)
    rows = np.repeat(np.arange(m, dtype=np.int64), counts)
    keys = np.unique(rows * n + rng.integers(0, n, rows.size))
    rows, cols = keys // n, (keys % n).astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int64)
    vals = rng.standard_normal(cols.size).astype(np.float32)
    return CSR(indptr=torch.from_numpy(indptr).to(dev), indices=torch.from_numpy(cols).to(dev),
               data=torch.from_numpy(vals).to(dev), shape=(m, n))


def median_of(fn, dev, reps):
    fn()
    t = [timed(fn, dev)[0] for _ in range(reps)]
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def kernel_only(A, C):
    """The search launches alone: what ``ops.csr_nearest_centroid`` does after preparing CT / norms."""
    k, n = C.shape
    kp = (k + 63) // 64 * 64
    CT = torch.zeros((n, kp), dtype=torch.float32, device=C.device)
    CT[:, :k] = C.t()
    cn = torch.full((kp,), float("inf"), dtype=torch.float32, device=C.device)
    cn[:k] = (C.double() * C.double()).sum(1).float()
    lab = torch.empty(A.shape[0], dtype=torch.int32, device=C.device)
    d2 = torch.empty(A.shape[0], dtype=torch.float32, device=C.device)

    def run():
        ops.native.call("srml_csr_nearest_f32", A.indptr.data_ptr(), A.indices.data_ptr(), A.data.data_ptr(),
                        A.shape[0], CT.data_ptr(), cn.data_ptr(), k, kp, lab.data_ptr(), d2.data_ptr(),
                        ops.native.stream(C.device))
    return run


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, action="append", metavar=("ROWS", "COLS", "NNZ", "K"))
    ap.add_argument("--dense", type=int, default=0, help="also time the dense route on shapes with at most this many rows")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--rehearse", action="store_true", help="run the CPU paths at a tiny size: its times mean nothing")
    a = ap.parse_args()
    if not a.rehearse and not torch.cuda.is_available():
        raise SystemExit("csr_kmeans_bench needs a GPU: a CPU run gives no time (--rehearse checks the script only)")
    dev = torch.device("cpu") if a.rehearse else torch.device("cuda", 0)
    shapes = a.shape or ([[300, 500, 8, 5]] if a.rehearse else [[1000000, 65536, 50, 100]])
    res = {"reps": a.reps, "shapes": [],
           "device": "cpu rehearsal: no timing here is a measurement" if a.rehearse else torch.cuda.get_device_name(dev)}
    for m, n, nnz, k in shapes:
        A = poisson_rows(m, n, nnz, 1, dev)
        tot = int(A.data.numel())
        group = torch.from_numpy(np.random.default_rng(2).integers(0, k, m).astype(np.int32)).to(dev)
        sums, counts = ops.csr_cluster_sums(A, group, k)
        C = (sums / counts.clamp_min(1).view(-1, 1)).float()
        kp = (k + 63) // 64 * 64
        rec = {"rows": m, "cols": n, "k": k, "nnz": tot, "nnz_per_row": tot / m,
               "search_model_bytes": tot * kp * 4 + tot * 12 + (m + 1) * 8, "sums_added_bytes": tot * 8}
        labels, _ = ops.csr_nearest_centroid(A, C)
        ws = {}  # the transposed centre table, kept across calls as a fit keeps it
        rec["search_s"] = median_of(lambda: ops.csr_nearest_centroid(A, C, ws=ws), dev, a.reps)
        if dev.type == "cuda":
            rec["search_kernel_s"] = median_of(kernel_only(A, C), dev, a.reps)
            rec["search_model_tb_s"] = rec["search_model_bytes"] / rec["search_kernel_s"]["median"] / 1e12
        rec["sums_s"] = median_of(lambda: ops.csr_cluster_sums(A, labels, k), dev, a.reps)
        rec["sums_added_tb_s"] = rec["sums_added_bytes"] / rec["sums_s"]["median"] / 1e12
        set_deterministic(True)
        try:
            rec["sums_fixed_s"] = median_of(lambda: ops.csr_cluster_sums(A, labels, k), dev, a.reps)
        finally:
            set_deterministic(None)
        rec["fixed_over_default"] = rec["sums_fixed_s"]["median"] / rec["sums_s"]["median"]
        if m <= a.dense:
            X = ops.csr_gather_dense(A, torch.arange(m, device=dev))
            xn = ops.row_sqnorm(X) if X.is_cuda else (X * X).sum(1)
            dl, _ = ops.nearest_centroid(X, C, xn)
            rec["dense_search_s"] = median_of(lambda: ops.nearest_centroid(X, C, xn), dev, a.reps)
            rec["dense_sums_s"] = median_of(lambda: ops.cluster_sums(X, dl, k), dev, a.reps)
            rec["same_labels"] = float((dl.long() == labels.long()).double().mean())
            del X
        res["shapes"].append(rec)
        del A, C, sums
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
