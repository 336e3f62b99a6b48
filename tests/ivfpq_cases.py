"""Shared cases and fp64 oracles of the IVF-PQ tests (``test_ivfpq.py`` on the CPU path,
``test_ivfpq_gpu.py`` on the kernels).

Rounding bound of one (query q, list l, item with codewords cb), derived, not measured:
  L2:            S = sum_d (|q_d| + |c_{l,d}| + |cb_d|)^2
  inner product: S = sum_d |q_d| (|c_{l,d}| + |cb_d|)
  b = (n + 8) 2^-23 S
(at most three roundings to form the difference, squaring doubles the relative error, summing n
terms adds (n - 1) u with u = 2^-24). The encode check uses the same form per sub-space
(dsub dimensions instead of n), which is never wider."""
import numpy as np
import torch

U23 = 2.0 ** -23

# n, M, ksub, N, nlist, nprobe, kcs, special lists
SCAN_CASES = {
    "n32": (32, 8, 64, 2000, 16, 4, (40,), False),
    "n35": (35, 5, 32, 1500, 12, 4, (64, 65), True),
    "table128k": (128, 128, 256, 600, 4, 4, (10,), False),
    "one_list": (4, 1, 16, 70, 1, 1, (64,), False),
    "padding": (8, 2, 16, 5, 2, 2, (10,), False),
}
ENCODE_SHAPES = [(32, 8, 256), (35, 5, 32), (128, 128, 256), (4, 1, 16)]
ENCODE_ROWS = [1, 63, 64, 65, 1000]


def make_index(n, M, ksub, N, nlist, special=False, identical=0, seed=0):
    """A hand-made index: random centres, codebooks and codes (``special``: list 2 empty, list 3 one
    row; ``identical``: that many leading rows of list 0 share one code row)."""
    g = torch.Generator().manual_seed(seed)
    dsub = n // M
    lab = torch.randint(0, nlist, (N,), generator=g)
    if special:
        lab[lab == 2] = 0
        lab[lab == 3] = 1
        lab[N // 2] = 3
    if identical:
        lab[:] = 0
    lab, _ = torch.sort(lab)
    list_off = torch.searchsorted(lab, torch.arange(nlist + 1)).long()
    C = 2.0 * torch.randn((nlist, n), generator=g)
    cb = 0.5 * torch.randn((M, ksub, dsub), generator=g)
    codes = torch.randint(0, ksub, (N, M), generator=g).to(torch.uint8)
    if identical:
        codes[:identical] = codes[0]
    return {"n": n, "M": M, "ksub": ksub, "N": N, "nlist": nlist, "lab": lab, "list_off": list_off, "C": C, "cb": cb,
            "codes": codes}


def make_queries(index, nq, nprobe, minus_one=False, seed=1):
    g = torch.Generator().manual_seed(seed)
    Q = 1.5 * torch.randn((nq, index["n"]), generator=g)
    probes = torch.stack([torch.randperm(index["nlist"], generator=g)[:nprobe] for _ in range(nq)]).int() \
        if nq else torch.zeros((0, nprobe), dtype=torch.int32)
    if minus_one and nq:
        probes[::5, min(2, nprobe - 1)] = -1
    return Q, probes


def _recon(index):
    """fp64 reconstruction parts of every item: (centre [N, n], codeword [N, n])."""
    M = index["M"]
    c = index["C"].double()[index["lab"]].numpy()
    cb = index["cb"].double().numpy()
    cd = index["codes"].long().numpy()
    w = np.concatenate([cb[m][cd[:, m]] for m in range(M)], axis=1)
    return c, w


def check_scan(index, Q, probes, kc, ip, keys, pos):
    """The issue's assertions for every query against the fp64 keys."""
    keys = keys.detach().cpu().double().numpy()
    pos = pos.detach().cpu().numpy()
    nq, n = Q.shape
    assert keys.shape == (nq, kc) and pos.shape == (nq, kc)
    c, w = _recon(index)
    lo = index["list_off"].numpy()
    Qd = Q.double().numpy()
    pr = probes.numpy()
    worst = 0.0
    for q in range(nq):
        cand = np.concatenate([np.arange(lo[l], lo[l + 1]) for l in pr[q] if l >= 0] + [np.zeros(0, np.int64)])
        cand = cand.astype(np.int64)
        x = Qd[q]
        if ip:
            K = -(x * (c[cand] + w[cand])).sum(1)
            S = (np.abs(x) * (np.abs(c[cand]) + np.abs(w[cand]))).sum(1)
        else:
            K = ((x - c[cand] - w[cand]) ** 2).sum(1)
            S = ((np.abs(x) + np.abs(c[cand]) + np.abs(w[cand])) ** 2).sum(1)
        B = float(((n + 8) * U23 * S).max()) if cand.size else 0.0
        cnt = min(kc, cand.size)
        valid = pos[q] >= 0
        assert valid[:cnt].all() and not valid[cnt:].any(), (q, cnt, pos[q])  # padding comes last
        assert np.all(np.isposinf(keys[q, cnt:])), (q, keys[q, cnt:])
        p = pos[q, :cnt]
        assert len(set(p.tolist())) == cnt, (q, p)  # distinct
        where = {int(v): i for i, v in enumerate(cand)}
        assert all(int(v) in where for v in p), (q, p)  # inside a probed list
        if cnt == 0:
            continue
        kq = keys[q, :cnt]
        assert np.all(np.diff(kq) >= 0), (q, kq)
        Kp = K[[where[int(v)] for v in p]]
        err = np.abs(kq - Kp).max()
        worst = max(worst, err / B)
        assert err <= B, (q, err, B)
        kappa = np.sort(K)[kc - 1] if cand.size >= kc else np.inf
        assert np.all(Kp <= kappa + 2 * B), (q, Kp.max(), kappa, B)
        must = cand[K < kappa - 2 * B]
        assert set(must.tolist()) <= set(p.tolist()), (q, sorted(set(must.tolist()) - set(p.tolist())))
    return worst


def run_scan_case(ops, name, ip, device, nq=33):
    n, M, ksub, N, nlist, nprobe, kcs, special = SCAN_CASES[name]
    index = make_index(n, M, ksub, N, nlist, special=special)
    Q, probes = make_queries(index, nq, nprobe, minus_one=special)
    if special:
        lens = (index["list_off"][1:] - index["list_off"][:-1]).tolist()
        assert lens[2] == 0 and lens[3] == 1
        assert (probes == 2).any() and (probes == 3).any() and (probes == -1).any()
    for kc in kcs:
        keys, pos = scan(ops, index, Q, probes, kc, ip, device)
        check_scan(index, Q, probes, kc, ip, keys, pos)


def scan(ops, index, Q, probes, kc, ip, device):
    d = torch.device(device)
    return ops.ivfpq_search(Q.to(d), probes.to(d), index["list_off"].to(d), index["C"].to(d), index["cb"].to(d),
                            index["codes"].to(d), kc, inner_product=bool(ip))


def run_encode_case(ops, n, M, ksub, N, device, seed=0):
    """Chosen codeword within 2b of the fp64 minimum; two calls agree. Rows of list 0 (zero centre)
    are exact codewords and codeword 5 duplicates codeword 2."""
    g = torch.Generator().manual_seed(seed + N)
    dsub = n // M
    nlist = 3
    C = 2.0 * torch.randn((nlist, n), generator=g)
    C[0] = 0
    cb = 0.5 * torch.randn((M, ksub, dsub), generator=g)
    cb[:, 5] = cb[:, 2]
    lab = torch.randint(0, nlist, (N,), generator=g).int()
    X = 1.5 * torch.randn((N, n), generator=g)
    exact = torch.nonzero(lab == 0).view(-1)
    pick = torch.randint(0, ksub, (exact.numel(), M), generator=g)
    pick[::2, 0] = 2  # the duplicated codeword
    X[exact] = torch.cat([cb[m][pick[:, m]] for m in range(M)], 1)
    d = torch.device(device)
    a = ops.pq_encode(X.to(d), cb.to(d), C.to(d), lab.to(d))
    b = ops.pq_encode(X.to(d), cb.to(d), C.to(d), lab.to(d))
    assert a.dtype == torch.uint8 and a.shape == (N, M)
    assert torch.equal(a, b)
    a = a.cpu().long().numpy()
    assert a.max() < ksub
    Xd, Cd, cbd = X.double().numpy(), C.double()[lab.long()].numpy(), cb.double().numpy()
    for m in range(M):
        sl = slice(m * dsub, (m + 1) * dsub)
        x, c = Xd[:, sl], Cd[:, sl]
        D = ((x[:, None, :] - c[:, None, :] - cbd[m][None]) ** 2).sum(-1)  # [N, ksub]
        S = ((np.abs(x)[:, None, :] + np.abs(c)[:, None, :] + np.abs(cbd[m])[None]) ** 2).sum(-1)
        rows = np.arange(N)
        best = D.argmin(1)
        bound = (dsub + 8) * U23 * np.maximum(S[rows, a[:, m]], S[rows, best])
        assert np.all(D[rows, a[:, m]] <= D[rows, best] + 2 * bound), (m, np.max(D[rows, a[:, m]] - D[rows, best]))
    # without labels the rows are encoded as they are
    e = ops.pq_encode((X - C[lab.long()]).to(d), cb.to(d)).cpu().long().numpy()
    assert e.shape == (N, M)


def blobs(seed=0):
    """2000 x 32 rows from 20 Gaussian blobs (centres sigma 3, noise sigma 1) and 300 queries."""
    rng = np.random.default_rng(seed)
    cen = 3.0 * rng.standard_normal((20, 32))
    X = (cen[rng.integers(0, 20, 2000)] + rng.standard_normal((2000, 32))).astype(np.float32)
    Q = (cen[rng.integers(0, 20, 300)] + rng.standard_normal((300, 32))).astype(np.float32)
    return X, Q


def knn_arrays(knn_df, id_name="unique_id"):
    t = knn_df.toPandas()
    return (t["query_" + id_name].to_numpy(), np.stack([np.asarray(v) for v in t["indices"]]),
            np.stack([np.asarray(v) for v in t["distances"]]))


def direct_distance(X, Q, ind, metric):
    """fp64 distances of the returned ids, in the metric's reported form."""
    R = X.astype(np.float64)[ind]  # [q, k, n]
    q = Q.astype(np.float64)[:, None, :]
    if metric == "inner_product":
        return (R * q).sum(-1)
    d2 = ((R - q) ** 2).sum(-1)
    return d2 if metric == "sqeuclidean" else np.sqrt(d2)


def exact_ids(X, Q, k, metric):
    Xd, Qd = X.astype(np.float64), Q.astype(np.float64)
    if metric == "inner_product":
        D = -(Qd @ Xd.T)
    else:
        D = ((Qd[:, None, :] - Xd[None]) ** 2).sum(-1)
    return np.argsort(D, axis=1, kind="stable")[:, :k]


def recall(ind, exact):
    k = exact.shape[1]
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / float(k) for a, b in zip(ind, exact)]))
