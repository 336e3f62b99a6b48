"""Distributed exact and approximate (IVF-Flat, IVF-PQ, CAGRA) k-nearest-neighbour search.

Reference: exact — cuML ``NearestNeighborsMG.kneighbors`` with UCX query fan-out and a partial
top-k merge (``knn.py:638-749``; every item row id additionally travelled through the Spark
driver); approximate — one cuML IVF-Flat index per item partition, queries broadcast, top-k
merged by a Spark SQL ``groupBy(query_id)`` (``knn.py:1154-1380``).

MI355X design (per rank = per item partition):
* query fan-out is a point-to-point RING (the role of the reference's UCX send/recv): every
  rank's query block travels once around the ranks together with its running top-k; at each hop
  the holder scores it against its local items and merges (device radix-select top-k with ids),
  and the NEXT block's transfer (isend/irecv over RCCL/xGMI) overlaps that compute. After W hops
  the finished block is back at its owner. Per-rank memory is two query blocks + their top-k
  lists, instead of every rank's queries (the all-gather's O(Q·n) per rank);
* exact: the fused MFMA distance + LDS top-k kernel (``srml_knn_f32``, k <= 64) or the distance
  chunk + radix-select path (k <= 1024) over the local items, candidates refined exactly;
* IVF-Flat: coarse quantiser trained with the device KMeans kernels, items bucketed into
  contiguous inverted lists (device sort), probes chosen with the same top-k kernel against the
  centroids, lists scanned by ``srml_ivf_search_f32``; queries ride the same ring;
* IVF-PQ (cuVS naming; the reference's docstring announces it, ``knn.py:895-914``): the same
  quantiser and lists, every row stored as M one-byte codes of its residual to the list centre
  (``srml_pq_encode_f32``, which is also the assignment step of the codebook training), the probed
  lists scanned through an fp32 lookup table in LDS (``srml_ivfpq_search_f32`` /
  ``srml_ivfpq_candidates_f32``) for ``k * refine_ratio`` candidates, which are re-scored exactly;
* CAGRA (cuVS naming; the later releases of the reference ship it): per rank the all-points kNN
  graph of ``models/knn_graph.py``, cut to a fixed degree by rank-based detour pruning and merged
  with its reverse edges (``csrc/cagra.hip``), walked by ``srml_cagra_search_f32``: one workgroup
  per query, the sorted candidate list, the visited hash and the query row in LDS.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np
import torch

from .. import ops
from ..parallel.context import WorkerContext


def _merge_lists(d1: torch.Tensor, i1: torch.Tensor, d2: torch.Tensor, i2: torch.Tensor, k: int
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """k smallest of two (distance, id) lists per row (ties keep the earlier list)."""
    D = torch.cat([d1, d2], 1)
    I = torch.cat([i1, i2], 1)
    return ops.topk_rows(D, k, ids=I)  # radix select on the device (k <= ops.TOPK_KMAX)


def _ring_search(queries: torch.Tensor, k: int, ctx: WorkerContext, local: Callable[[torch.Tensor], Tuple[
        torch.Tensor, torch.Tensor]]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Run ``local(Q) -> (d [q, k], global ids [q, k])`` for every rank's query block on every
    rank's items by passing (block, running top-k) around the ring; returns this rank's merged
    lists.

    Per hop: the NEXT query block's isend/irecv starts first and the held block is scored while it
    travels; the held block's running lists (sent by the previous rank after ITS merge) are only
    waited for after that scoring, merged, and forwarded at once — so each list exchange overlaps
    the next hop's scoring instead of sitting between hops on the critical path."""
    W, r = ctx.world_size, ctx.rank
    dev = queries.device
    nq = queries.shape[0]
    if W == 1:
        return local(queries)
    sizes = [int(v) for v in ctx.comm.allgather(torch.tensor([nq], dtype=torch.int64, device=ctx.device)).tolist()]
    n = queries.shape[1]
    nxt, prv = (r + 1) % W, (r - 1) % W
    Qc = queries.contiguous()
    dc = torch.full((nq, k), float("inf"), dtype=torch.float32, device=dev)
    ic = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
    h_lists = None  # in-flight exchange of the running lists of the block held at this hop
    for s in range(W):
        h_q = None
        if s < W - 1:  # the next block is already on its way while this one is scored
            rows = sizes[(r - s - 1) % W]
            Qn = torch.empty((rows, n), dtype=Qc.dtype, device=dev)
            h_q = ctx.comm.isendrecv(Qc, nxt, Qn, prv)
        ld = li = None
        if Qc.shape[0]:
            ld, li = local(Qc)
        if h_lists is not None:  # this block's lists, merged by the previous rank at the last hop
            for h in h_lists:
                ctx.comm.wait_sendrecv(h)
            h_lists = None
        if ld is not None:
            dc, ic = _merge_lists(dc, ic, ld.float(), li, k)
        if s < W - 1:
            ctx.comm.wait_sendrecv(h_q)
            dn = torch.empty((rows, k), dtype=torch.float32, device=dev)
            inn = torch.empty((rows, k), dtype=torch.int64, device=dev)
            # forward the merged lists with the block they belong to (already sent); overlaps the
            # next hop's scoring
            h_lists = (ctx.comm.isendrecv(dc.contiguous(), nxt, dn, prv),
                       ctx.comm.isendrecv(ic.contiguous(), nxt, inn, prv))
            Qc, dc, ic = Qn, dn, inn
    # the block now held belongs to the next rank: hand it home, receive ours
    d_own = torch.empty((nq, k), dtype=torch.float32, device=dev)
    i_own = torch.empty((nq, k), dtype=torch.int64, device=dev)
    h1 = ctx.comm.isendrecv(dc.contiguous(), nxt, d_own, prv)
    h2 = ctx.comm.isendrecv(ic.contiguous(), nxt, i_own, prv)
    ctx.comm.wait_sendrecv(h1)
    ctx.comm.wait_sendrecv(h2)
    return d_own, i_own


def _finish(d: torch.Tensor, metric: str) -> torch.Tensor:
    if metric in ("euclidean", "l2"):
        return torch.sqrt(d.clamp_min(0))
    if metric == "inner_product":
        return -0.5 * d
    return d


def _refine(Q: torch.Tensor, items: torch.Tensor, pos: torch.Tensor, metric: str) -> torch.Tensor:
    """Recompute the selected candidates' distances directly (q - i, not ||q||^2 + ||i||^2 - 2 q.i),
    so near-duplicates do not lose all their digits to fp32 cancellation. O(q k n), chunked."""
    nq, k = pos.shape
    n = Q.shape[1]
    out = torch.empty((nq, k), dtype=torch.float32, device=Q.device)
    step = max(1, (1 << 26) // max(1, k * n))
    valid = pos >= 0
    p = pos.clamp_min(0)
    for s in range(0, nq, step):
        rows = items.index_select(0, p[s: s + step].reshape(-1)).view(-1, k, n).float()
        q = Q[s: s + step].float().unsqueeze(1)
        if metric == "inner_product":
            out[s: s + step] = -2.0 * (rows * q).sum(-1)
        else:
            out[s: s + step] = ((rows - q) ** 2).sum(-1)
    return torch.where(valid, out, torch.full_like(out, float("inf")))


def _resort(d: torch.Tensor, i: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    v, j = torch.sort(d, dim=1)
    return v, i.gather(1, j)


def _refine_sorted(Q: torch.Tensor, items: torch.Tensor, pos: torch.Tensor, metric: str
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact re-scored candidates sorted per query: the fused device kernel
    (``ops.knn_refine_sort``) when it applies, else the chunked torch re-score + sort."""
    r = ops.knn_refine_sort(Q, items, pos, inner_product=metric == "inner_product")
    if r is not None:
        return r
    return _resort(_refine(Q, items, pos, metric), pos)


def _pad_k(d: torch.Tensor, gi: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    if d.shape[1] < k:  # fewer local items than k
        pad = k - d.shape[1]
        d = torch.cat([d, torch.full((d.shape[0], pad), float("inf"), device=d.device)], 1)
        gi = torch.cat([gi, torch.full((gi.shape[0], pad), -1, dtype=torch.int64, device=gi.device)], 1)
    return d, gi


def exact_knn(items: torch.Tensor, item_ids: torch.Tensor, queries: torch.Tensor, k: int, ctx: WorkerContext,
              metric: str = "euclidean") -> Tuple[np.ndarray, np.ndarray]:
    def local(Q: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if items.shape[0] == 0:
            return (torch.full((Q.shape[0], k), float("inf"), device=Q.device),
                    torch.full((Q.shape[0], k), -1, dtype=torch.int64, device=Q.device))
        if metric == "inner_product":
            z_i = ops.zeros(items.shape[0], device=items.device)
            z_q = ops.zeros(Q.shape[0], device=items.device)
            d, li = ops.knn(Q, items, k, inorm=z_i, qnorm=z_q)  # d = -2 q.i
        else:
            d, li = ops.knn(Q, items, k)
        d, li = _refine_sorted(Q, items, li, metric)
        gi = torch.where(li >= 0, item_ids[li.clamp_min(0)], torch.full_like(li, -1))
        return _pad_k(d, gi, k)

    d, gi = _ring_search(queries, k, ctx, local)
    return _finish(d, metric).cpu().numpy(), gi.cpu().numpy()


@dataclass
class IVFIndex:
    centroids: torch.Tensor
    cnorm: torch.Tensor
    list_off: torch.Tensor
    items: torch.Tensor
    inorm: torch.Tensor
    ids: torch.Tensor


def build_ivf(X: torch.Tensor, ids: torch.Tensor, nlist: int, seed: int = 1, iters: int = 20,
              train_rows_per_list: int = 256) -> IVFIndex:
    """Coarse quantiser (Lloyd on a row subsample, as IVF trainers do) + contiguous inverted lists."""
    m = X.shape[0]
    nlist = max(1, min(int(nlist), m))
    gen = torch.Generator().manual_seed(int(seed))
    ntrain = min(m, max(nlist * train_rows_per_list, 4 * nlist))
    T = X if ntrain == m else X.index_select(0, torch.randperm(m, generator=gen)[:ntrain].to(X.device))
    C = T.index_select(0, torch.randperm(T.shape[0], generator=gen)[:nlist].to(X.device)).float().clone()
    FT = ops.quantizer_planes(T) if nlist > 256 else None  # bucketing only: the fp16 filter's arg-min
    tn = ops.row_sqnorm(T) if FT is None else None
    for _ in range(max(1, iters)):
        lab = ops.nearest_list(T, C, FT, tn)
        sums, counts = ops.cluster_sums(T, lab, nlist)
        C = torch.where(counts.view(-1, 1) > 0, (sums / counts.clamp_min(1).double().view(-1, 1)).float(), C)
    lab = ops.nearest_list(X, C, ops.quantizer_planes(X) if nlist > 256 else None)
    order, off, _ = ops.label_sort(lab, nlist)  # stable: rows keep their order inside a list
    order = order.long()
    items = X.index_select(0, order).contiguous()
    return IVFIndex(C.contiguous(), ops.row_sqnorm(C), off, items, ops.row_sqnorm(items), ids.index_select(0, order))


def ivf_knn(index: Optional[IVFIndex], queries: torch.Tensor, k: int, nprobe: int, ctx: WorkerContext,
            metric: str = "euclidean") -> Tuple[np.ndarray, np.ndarray]:
    def local(Q: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if index is None:
            return (torch.full((Q.shape[0], k), float("inf"), device=Q.device),
                    torch.full((Q.shape[0], k), -1, dtype=torch.int64, device=Q.device))
        npb = max(1, min(int(nprobe), index.centroids.shape[0], ops.KNN_KMAX))
        qn = ops.row_sqnorm(Q)
        _, probes = ops.knn(Q, index.centroids, npb, inorm=index.cnorm, qnorm=qn)
        pos_ids = torch.arange(index.items.shape[0], dtype=torch.int64, device=Q.device)
        if metric == "inner_product":
            z = torch.zeros_like(index.inorm)
            d, pos = ops.ivf_search(Q, probes.int(), index.list_off, index.items, z, pos_ids, k,
                                    qnorm=torch.zeros_like(qn))
        else:
            d, pos = ops.ivf_search(Q, probes.int(), index.list_off, index.items, index.inorm, pos_ids, k, qnorm=qn)
        d, pos = _refine_sorted(Q, index.items, pos, metric)
        gi = torch.where(pos >= 0, index.ids[pos.clamp_min(0)], torch.full_like(pos, -1))
        return _pad_k(d, gi, k)

    d, gi = _ring_search(queries, k, ctx, local)
    return _finish(d, metric).cpu().numpy(), gi.cpu().numpy()


# ------------------------------------------------------------------------------------------
# IVF-PQ (cuVS / FAISS naming; beyond the reference version, whose docstring announces it)
# ------------------------------------------------------------------------------------------
@dataclass
class IVFPQIndex:
    centroids: torch.Tensor   # [nlist, n] coarse quantiser (build_ivf's)
    cnorm: torch.Tensor
    list_off: torch.Tensor    # [nlist + 1]
    items: torch.Tensor       # [N, n] rows in list order: the exact re-score reads them
    ids: torch.Tensor         # [N] item ids in list order
    codebooks: torch.Tensor   # fp32 [M, ksub, dsub] over residuals x - c_list
    codes: torch.Tensor       # uint8 [N, M], row-major, list order


def default_pq_m(n: int) -> int:
    """Largest divisor of n that is <= max(1, n // 4) (and <= ops.PQ_MMAX)."""
    top = min(max(1, n // 4), ops.PQ_MMAX)
    return max(m for m in range(1, top + 1) if n % m == 0)


def check_pq_args(n: int, M: int, n_bits: int, refine_ratio: int, k: int) -> None:
    """The checks of the IVF-PQ parameters that need the feature count (every rank raises alike)."""
    if M < 1 or M > ops.PQ_MMAX:
        raise ValueError("ivfpq: M=%d outside 1..%d" % (M, ops.PQ_MMAX))
    if n % M != 0:
        raise ValueError("ivfpq: M=%d does not divide the %d features" % (M, n))
    if n_bits < 4 or n_bits > 8:
        raise ValueError("ivfpq: n_bits=%d outside 4..8" % n_bits)
    if refine_ratio < 1:
        raise ValueError("ivfpq: refine_ratio=%d must be >= 1" % refine_ratio)
    if k * refine_ratio > ops.TOPK_KMAX:
        raise ValueError("ivfpq: k * refine_ratio = %d > %d" % (k * refine_ratio, ops.TOPK_KMAX))


def train_pq(R: torch.Tensor, M: int, ksub: int, seed: int, iters: int = 10) -> torch.Tensor:
    """Codebooks fp32 [M, ksub, dsub]: M independent Lloyd runs over the sub-vectors of the residual
    rows R, seeded from ``seed``. The assignment of every run goes through ``ops.pq_encode`` in one
    launch; the centre update is one ``ops.cluster_sums`` over the (run, codeword) pairs. A codeword
    that ends without rows (fewer distinct training rows than ksub) copies codeword 0."""
    T, n = R.shape
    dsub = n // M
    gen = torch.Generator().manual_seed(int(seed) + 0x5051)
    Rv = R.float().contiguous().view(T, M, dsub)
    cb = torch.empty((M, ksub, dsub), dtype=torch.float32, device=R.device)
    take = min(T, ksub)
    for m in range(M):  # its own rows for every run
        sel = torch.randperm(T, generator=gen)[:take].to(R.device)
        cb[m, :take] = Rv[:, m].index_select(0, sel)
        cb[m, take:] = cb[m, :1]
    base = (torch.arange(M, device=R.device, dtype=torch.int32) * ksub).view(1, M)
    flat = Rv.view(T * M, dsub)
    for _ in range(max(1, iters)):
        lab = (ops.pq_encode(Rv.view(T, n), cb).int() + base).view(-1)
        sums, counts = ops.cluster_sums(flat, lab, M * ksub)
        new = (sums / counts.clamp_min(1).double().view(-1, 1)).float().view(M, ksub, dsub)
        cb = torch.where(counts.view(M, ksub, 1) > 0, new, cb)
    lab = (ops.pq_encode(Rv.view(T, n), cb).int() + base).view(-1)
    used = ops.label_counts(lab, M * ksub).view(M, ksub, 1) > 0
    return torch.where(used, cb, cb[:, :1].expand_as(cb)).contiguous()


def build_ivfpq(X: torch.Tensor, ids: torch.Tensor, nlist: int, M: int, n_bits: int = 8, seed: int = 1,
                iters: int = 20, pq_iters: int = 10, train_rows_per_code: int = 64) -> IVFPQIndex:
    """``build_ivf``'s quantiser and list order, codebooks trained on the residuals of a row
    subsample, and every row's residual encoded (row-major uint8 [N, M] in list order)."""
    ivf = build_ivf(X, ids, nlist, seed, iters)
    N, n = ivf.items.shape
    ksub = 1 << int(n_bits)
    nl = ivf.centroids.shape[0]
    lab = torch.repeat_interleave(torch.arange(nl, device=X.device, dtype=torch.int32),
                                  ivf.list_off[1:] - ivf.list_off[:-1], output_size=N)
    ntrain = min(N, ksub * train_rows_per_code)
    if ntrain < N:
        gen = torch.Generator().manual_seed(int(seed) + 0x4956)
        sel = torch.randperm(N, generator=gen)[:ntrain].to(X.device)
        R = ivf.items.index_select(0, sel).float() - ivf.centroids.index_select(0, lab.index_select(0, sel).long())
    else:
        R = ivf.items.float() - ivf.centroids.index_select(0, lab.long())
    cb = train_pq(R, M, ksub, seed, pq_iters)
    codes = ops.pq_encode(ivf.items, cb, ivf.centroids, lab)
    return IVFPQIndex(ivf.centroids, ivf.cnorm, ivf.list_off, ivf.items, ivf.ids, cb, codes)


def ivfpq_knn(index: Optional[IVFPQIndex], queries: torch.Tensor, k: int, nprobe: int, refine_ratio: int,
              ctx: WorkerContext, metric: str = "euclidean") -> Tuple[np.ndarray, np.ndarray]:
    """Probe the coarse quantiser, take ``kc = k * refine_ratio`` candidates by PQ distance, re-score
    them exactly against the list-ordered rows and keep k; queries ride the ring as for IVF-Flat."""
    kc = int(k) * int(refine_ratio)
    if kc > ops.TOPK_KMAX:
        raise ValueError("ivfpq: k * refine_ratio = %d > %d" % (kc, ops.TOPK_KMAX))

    def local(Q: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if index is None:
            return (torch.full((Q.shape[0], k), float("inf"), device=Q.device),
                    torch.full((Q.shape[0], k), -1, dtype=torch.int64, device=Q.device))
        npb = max(1, min(int(nprobe), index.centroids.shape[0], ops.KNN_KMAX))
        _, probes = ops.knn(Q, index.centroids, npb, inorm=index.cnorm, qnorm=ops.row_sqnorm(Q))
        _, pos = ops.ivfpq_search(Q, probes.int(), index.list_off, index.centroids, index.codebooks, index.codes, kc,
                                  inner_product=metric == "inner_product")
        d, pos = _refine_sorted(Q, index.items, pos, metric)
        d, pos = d[:, :k], pos[:, :k]
        gi = torch.where(pos >= 0, index.ids[pos.clamp_min(0)], torch.full_like(pos, -1))
        return _pad_k(d, gi, k)

    d, gi = _ring_search(queries, k, ctx, local)
    return _finish(d, metric).cpu().numpy(), gi.cpu().numpy()


# ------------------------------------------------------------------------------------------
# CAGRA (cuVS naming; shipped by the later releases of the reference)
# ------------------------------------------------------------------------------------------
@dataclass
class CagraIndex:
    items: torch.Tensor   # [N, n] fp32, original order
    ids: torch.Tensor     # [N] int64
    graph: torch.Tensor   # [N, gd] int32, -1 padded at the tail


def check_cagra_args(params: Tuple, k: int, metric: str) -> None:
    """The checks of the CAGRA parameters (``knn._cagra_params``' tuple) that need k and the metric."""
    if metric not in ("euclidean", "l2", "sqeuclidean"):
        raise ValueError("cagra: metric %r is not supported (the build graph is Euclidean)" % (metric,))
    itopk = int(params[3])
    if k > itopk:
        raise ValueError("cagra: k=%d exceeds itopk_size=%d" % (k, itopk))


def build_cagra(X: torch.Tensor, ids: torch.Tensor, igd: int, gd: int, build_algo: str = "auto", seed: int = 1,
                phases: Optional[dict] = None) -> CagraIndex:
    """The kNN graph of ``build_knn_graph`` at ``igd + 1`` neighbours without each row's own index
    (absent among duplicate rows: the last entry goes instead), detour-pruned to ``gd`` edges
    (``ops.cagra_prune``) and merged with its reverse edges (``ops.cagra_merge``). Both degrees are
    clamped to N - 1. ``phases`` (seconds): "knn_graph", "prune", "merge"."""
    import time

    from .knn_graph import build_knn_graph

    N = int(X.shape[0])
    Xf = X.float().contiguous()
    igd = max(0, min(int(igd), N - 1))
    gd = min(int(gd), igd)
    if gd < 1:  # one row: no edge to give
        return CagraIndex(Xf, ids, torch.full((N, 1), -1, dtype=torch.int32, device=X.device))

    def lap(name: str, t0: float) -> float:
        if phases is not None:
            if X.is_cuda:
                torch.cuda.synchronize(X.device)
            phases[name] = phases.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    t0 = time.perf_counter()
    _, idx = build_knn_graph(Xf, igd + 1, build_algo, seed=int(seed))
    idx = idx.long()
    own = idx == torch.arange(N, device=X.device).view(N, 1)
    drop = torch.where(own.any(1), own.int().argmax(1), torch.full((N,), igd, device=X.device))
    keep = torch.arange(igd + 1, device=X.device).view(1, -1) != drop.view(N, 1)
    G = idx[keep].view(N, igd).to(torch.int32).contiguous()
    t0 = lap("knn_graph", t0)
    P = ops.cagra_prune(G, gd)
    t0 = lap("prune", t0)
    F = ops.cagra_merge(P, gd)
    lap("merge", t0)
    return CagraIndex(Xf, ids, F)


def cagra_knn(index: Optional[CagraIndex], queries: torch.Tensor, k: int, params: Tuple, ctx: WorkerContext,
              metric: str = "euclidean") -> Tuple[np.ndarray, np.ndarray]:
    """Beam search of this rank's graph (``ops.cagra_search``) for the k best of the list, re-scored
    exactly; queries ride the ring as for IVF-Flat. ``params`` = (itopk_size, search_width,
    max_iterations, min_iterations, num_random_samplings, seed)."""
    itopk, width, max_iter, min_iter, nrs, seed = (int(v) for v in params)
    if k > itopk:
        raise ValueError("cagra: k=%d exceeds itopk_size=%d" % (k, itopk))
    S = min(itopk * nrs, ops.CAGRA_SEED_MAX)

    def local(Q: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if index is None:
            return (torch.full((Q.shape[0], k), float("inf"), device=Q.device),
                    torch.full((Q.shape[0], k), -1, dtype=torch.int64, device=Q.device))
        _, pos = ops.cagra_search(Q, index.items, index.graph, k, itopk, width, max_iter, min_iter, S, seed)
        d, pos = _refine_sorted(Q, index.items, pos, metric)
        gi = torch.where(pos >= 0, index.ids[pos.clamp_min(0)], torch.full_like(pos, -1))
        return _pad_k(d, gi, k)

    d, gi = _ring_search(queries, k, ctx, local)
    return _finish(d, metric).cpu().numpy(), gi.cpu().numpy()
