"""The fused silhouette kernel against the nearest-centroid kernel on one GPU.

Rows are seeded unit-variance blobs (default 1M x 3000 fp32 around k = 1000 centres, generated on the
device in row blocks); the labels are each row's nearest centre. Timed, each call ending in a device
synchronise, median and (min, max) of ``--reps`` runs after a warm-up, the two kernels alternating
inside every repetition:

* ``silhouette_kernel_s``: ``srml_silhouette_f32`` alone (operands prepared before the clock);
* ``nearest_centroid_kernel_s``: ``srml_nearest_centroid_f32`` alone on the same rows and the k
  cluster means: the same product on the same tile core with an arg-min epilogue;
* ``silhouette_op_s``: ``ops.silhouette`` with the summaries given (operand preparation + kernel),
  ``summaries_s``: ``ops.silhouette_sums`` + ``ops.silhouette_psi``;
* ``score_from_host_s`` (``--host``): ``models.silhouette.silhouette_score`` from host arrays, the
  host-to-device copy of the rows included (``h2d_bytes``); the Arrow column extraction is not.

``--density D`` is the sparse mode (``sparse_main``): the CSR route against densify + copy + the dense
kernel on the same rows of ``--cols`` columns (the n of the table) at that density.

Progress goes to stderr, the one JSON line to stdout and ``--out``.

    python tools/silhouette_bench.py --host --out profiles/silhouette.json
    python tools/silhouette_bench.py --density 0.01 --k 8 --out profiles/silhouette_csr_k8_d01.json
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
from spark_rapids_ml_nai_amd.ops import native  # noqa: E402


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


def stat(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def sparse_main(a, dev) -> dict:
    """``--density D``: seeded rows with a fraction D of their ``--cols`` columns set (unit-variance noise
    around k centres, the label the row's centre), built on the device in row blocks. Timed, median and
    (min, max) of ``--reps`` runs after a warm-up, squaredEuclidean:

    * ``csr_kernel_s``: ``srml_csr_silhouette_f32`` alone (table and r_i prepared before the clock),
      ``csr_kernel_gbps`` against the table reads it must make, nnz kp 4 B;
    * ``csr_op_s``: ``ops.silhouette`` on the CSR with the summaries given; ``csr_summaries_s``:
      ``ops.silhouette_sums`` + ``ops.silhouette_psi`` on the CSR;
    * ``csr_from_host_s``: ``silhouette_score`` from a host scipy CSR (its host-to-device copy included);
    * ``dense_from_host_s``: the same rows densified on the host (``toarray``), copied and scored by
      the dense kernels: what ``enable_sparse_data_optim=False`` does with a sparse vector column."""
    import math

    import numpy as np
    import scipy.sparse as sp

    from spark_rapids_ml_nai_amd.core.base import CSR
    from spark_rapids_ml_nai_amd.models.silhouette import silhouette_score

    m, n, k = a.rows, a.cols, a.k
    g = torch.Generator(device=dev).manual_seed(0)
    cen = 3.0 * torch.randn((k, n), generator=g, device=dev)
    lab = torch.randint(0, k, (m,), generator=g, device=dev)
    counts, cols, vals = [], [], []
    for r0 in range(0, m, 65536):
        rows = min(65536, m - r0)
        nz = (torch.rand((rows, n), generator=g, device=dev) < a.density).nonzero()
        counts.append(torch.bincount(nz[:, 0], minlength=rows))
        cols.append(nz[:, 1].to(torch.int32))
        vals.append(cen[lab[r0 + nz[:, 0]], nz[:, 1]] + torch.randn(nz.shape[0], generator=g, device=dev))
    indptr = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.cat(counts), 0)
    A = CSR(indptr, torch.cat(cols), torch.cat(vals).float(), (m, n))
    nnz = int(indptr[-1])
    say("data ready: %d x %d at density %g (%d non-zeros), k = %d" % (m, n, a.density, nnz, k))

    def summaries():
        N_, Y_ = ops.silhouette_sums(A, lab, k)
        return N_, Y_, ops.silhouette_psi(A, lab, k, ops.silhouette_centre(N_, Y_))

    stats = summaries()
    kp = ops.csr_silhouette_kp(k)
    res = {"rows": m, "cols": n, "k": k, "kp": kp, "density": a.density, "nnz": nnz, "reps": a.reps}
    Ah = sp.csr_matrix((A.data.cpu().numpy(), A.indices.cpu().numpy(), A.indptr.cpu().numpy()), shape=(m, n))
    ph = lab.cpu().numpy().astype(np.float64)
    ts = {"csr_kernel_s": [], "csr_op_s": [], "csr_summaries_s": [], "csr_from_host_s": [], "dense_from_host_s": []}
    launch = None
    if not a.rehearse:  # the operands of the kernel, as ops._csr_silhouette forms them
        N, Y, psi = stats
        live = N > 0
        Nd = torch.where(live, N, torch.ones_like(N))
        mu = ops.silhouette_centre(N, Y).double()
        Mc = ((Y / Nd.view(-1, 1) - mu) * live.view(-1, 1)).float()
        MT = torch.zeros((n, kp), dtype=torch.float32, device=dev)
        MT[:, :k] = Mc.t()
        tc = torch.full((kp,), math.inf, dtype=torch.float64, device=dev)
        tc[:k] = torch.where(live, psi / Nd, tc[:k])
        gc = torch.zeros(kp, dtype=torch.float64, device=dev)
        gc[:k] = Mc.double() @ mu
        rv, lab32 = ops._csr_sil_rows(A, mu), lab.to(torch.int32).contiguous()
        rpb = ops.csr_silhouette_config()[2]
        part = torch.empty((m + rpb - 1) // rpb, dtype=torch.float64, device=dev)
        out = torch.empty(1, dtype=torch.float64, device=dev)
        if m > ops._CSR_KM_LAUNCH_ROWS:
            raise SystemExit("the kernel timing takes one launch: at most %d rows" % ops._CSR_KM_LAUNCH_ROWS)

        def launch():
            native.call("srml_csr_silhouette_f32", A.indptr.data_ptr(), A.indices.data_ptr(), A.data.data_ptr(), m,
                        MT.data_ptr(), k, kp, gc.data_ptr(), tc.data_ptr(), N.data_ptr(), rv.data_ptr(),
                        lab32.data_ptr(), None, 0, None, part.data_ptr(), out.data_ptr(), native.stream(dev))

    for rep in range(a.reps + 1):  # rep 0 warms up
        t = [timed(launch, dev)[0] if launch else 0.0,
             timed(lambda: ops.silhouette(A, lab, k, stats=stats), dev)[0],
             timed(summaries, dev)[0]]
        t_c, sc = timed(lambda: silhouette_score([(Ah, ph, None)], "squaredEuclidean", dev), dev)
        t_d, sd = timed(lambda: silhouette_score([(Ah.toarray(), ph, None)], "squaredEuclidean", dev), dev)
        say("rep %d: kernel %.4f s, op %.4f s, summaries %.4f s, CSR from host %.3f s, dense from host %.3f s"
            % (rep, *t, t_c, t_d))
        if rep:
            for key, v in zip(ts, t + [t_c, t_d]):
                ts[key].append(v)
    res.update({key: stat(v) for key, v in ts.items()})
    res["score_csr"], res["score_dense"] = sc, sd
    if launch:
        res["csr_kernel_gbps"] = nnz * kp * 4 / 1e9 / res["csr_kernel_s"]["median"]
    res["dense_over_csr_from_host"] = res["dense_from_host_s"]["median"] / res["csr_from_host_s"]["median"]
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--density", type=float, default=0.0,
                    help="> 0: the sparse mode (CSR route against densify + copy + dense kernel on the same rows)")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=3000)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--measure", default="squaredEuclidean")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", action="store_true", help="also time the score from host arrays (H2D included)")
    ap.add_argument("--out", default="")
    ap.add_argument("--rehearse", action="store_true", help="run the CPU paths at a tiny size: its times mean nothing")
    a = ap.parse_args()
    if not a.rehearse and not torch.cuda.is_available():
        raise SystemExit("silhouette_bench needs a GPU: a CPU run gives no time (--rehearse checks the script only)")
    dev = torch.device("cpu") if a.rehearse else torch.device("cuda", 0)
    m, n, k = a.rows, a.cols, a.k
    if a.density > 0:
        line = json.dumps(sparse_main(a, dev))
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    g = torch.Generator(device=dev).manual_seed(0)
    cen = 3.0 * torch.randn((k, n), generator=g, device=dev)
    X = torch.empty((m, n), dtype=torch.float32, device=dev)
    for r0 in range(0, m, 65536):
        rows = min(65536, m - r0)
        X[r0: r0 + rows] = cen[torch.randint(0, k, (rows,), generator=g, device=dev)] + torch.randn(
            (rows, n), generator=g, device=dev)
    lab = ops.nearest_centroid(X, cen)[0]
    say("data ready: %d x %d, k = %d" % (m, n, k))

    cos = a.measure == "cosine"

    def summaries():
        N_, Y_ = ops.silhouette_sums(X, lab, k, None, a.measure)
        return N_, Y_, None if cos else ops.silhouette_psi(X, lab, k, ops.silhouette_centre(N_, Y_))

    stats = summaries()
    res = {"rows": m, "cols": n, "k": k, "measure": a.measure, "reps": a.reps,
           "gflop": 2.0 * m * n * k / 1e9}
    ts = {"silhouette_kernel_s": [], "nearest_centroid_kernel_s": [], "silhouette_op_s": [], "summaries_s": []}
    if a.rehearse:
        sws, sw = ops.silhouette(X, lab, k, None, a.measure, stats=stats)
        res["score"] = float(sws) / float(sw)
    else:
        opnd = ops._sil_operands(X, lab, None, cos, *stats)
        C = (stats[1] / stats[0].clamp_min(1).view(-1, 1)).float().contiguous()
        cn = (C * C).sum(1).contiguous()
        best = torch.empty(m, dtype=torch.int64, device=dev)
        st = native.stream(dev)

        def nearest():
            native.call("srml_nearest_centroid_f32", X.data_ptr(), m, n, X.stride(0), C.data_ptr(), k, C.stride(0),
                        cn.data_ptr(), best.data_ptr(), st)

        for rep in range(a.reps + 1):  # rep 0 warms both up
            best.fill_(-1)
            t_s, (out, _) = timed(lambda: ops._sil_launch(X, k, opnd, False), dev)
            t_n, _ = timed(nearest, dev)
            t_o, _ = timed(lambda: ops.silhouette(X, lab, k, None, a.measure, stats=stats), dev)
            t_p, _ = timed(summaries, dev)
            say("rep %d: silhouette %.4f s, nearest %.4f s, op %.4f s, summaries %.4f s" % (rep, t_s, t_n, t_o, t_p))
            if rep:
                for key, t in zip(ts, (t_s, t_n, t_o, t_p)):
                    ts[key].append(t)
        res.update({key: stat(v) for key, v in ts.items()})
        res["kernel_ratio"] = res["silhouette_kernel_s"]["median"] / res["nearest_centroid_kernel_s"]["median"]
        res["silhouette_kernel_tflops"] = res["gflop"] / 1e3 / res["silhouette_kernel_s"]["median"]
        res["score"] = float(out[0]) / m
    if a.host:
        from spark_rapids_ml_nai_amd.models.silhouette import silhouette_score

        Xh, ph = X.cpu().numpy(), lab.cpu().numpy()
        del X
        hs = []
        for rep in range(3):
            t0 = time.perf_counter()
            sc = silhouette_score([(Xh, ph, None)], a.measure, dev)
            hs.append(time.perf_counter() - t0)
            say("host rep %d: %.3f s (score %.6f)" % (rep, hs[-1], sc))
        res["score_from_host_s"] = stat(hs[1:]) if len(hs) > 1 else stat(hs)
        res["h2d_bytes"] = int(Xh.nbytes)
        res["score_from_host"] = sc
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
