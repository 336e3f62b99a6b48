"""Shared cases and numpy oracles of the CAGRA tests (``test_cagra.py`` on the CPU path,
``test_cagra_gpu.py`` on the kernels).

The oracles implement the definitions of ``ops.cagra_prune`` / ``cagra_merge`` / ``cagra_seeds`` /
``cagra_search`` literally, node by node and query by query. The search is pinned on lattice data
(integer coordinates in [-8, 8] as fp32): every squared distance is then an exact integer below
2^24 in any summation order, with or without FMA (n <= 260 gives at most 260 * 16^2 = 66 560), ties
are plentiful and the (d2, id) order resolves them, so both paths must equal the oracle bit for bit."""
import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)

# (N, d, gd) of the prune / merge cases; "tail" has only 19 valid edges per row
GRAPH_CASES = {"d8": (200, 8, 4), "d33": (200, 33, 16), "d128": (300, 128, 64), "tail": (20, 32, 32)}

# n, gd, itopk, width, k, max_iter (0 = auto), min_iter, nq, S
SEARCH_CASES = {
    "n4_gd4_it1": (4, 4, 32, 1, 1, 1, 0, 9, 32),
    "n35_gd32_it5": (35, 32, 64, 1, 10, 5, 0, 9, 64),
    "n128_gd64_w4_auto": (128, 64, 64, 4, 64, 0, 0, 9, 64),
    "n260_itopk512_auto": (260, 32, 512, 1, 10, 0, 0, 5, 512),
    "n35_gd4_w4_min3_nq257": (35, 4, 64, 4, 10, 5, 3, 257, 64),
    "n128_itopk512_k512_s1024": (128, 32, 512, 1, 512, 0, 0, 3, 1024),
    "n35_nq1_k32": (35, 32, 32, 1, 32, 0, 0, 1, 32),
    "n35_nq0": (35, 32, 32, 1, 10, 0, 0, 0, 32),
}


# ------------------------------------------------------------------------------------ oracles
def _mix(h):
    h = h & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    return h ^ (h >> np.uint64(16))


def oracle_seeds(Q, N, S, seed):
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    nq, n = Q.shape
    out = np.zeros((nq, S), np.int32)
    with np.errstate(over="ignore"):
        for q in range(nq):
            bits = Q[q].view(np.uint32).astype(np.uint64)
            col = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B9)) & M32
            rh = np.uint64(int(_mix(bits ^ col).sum()) & 0xFFFFFFFF)
            for s in range(S):
                slot = np.uint64(((seed & 0xFFFFFFFF) * 0x9E3779B9 + s * 0x85EBCA6B + 1) & 0xFFFFFFFF)
                out[q, s] = int(_mix(rh ^ _mix(slot))) % N
    return out


def oracle_prune(G, gd):
    N, d = G.shape
    P = np.full((N, gd), -1, np.int32)
    for a in range(N):
        row = G[a]
        det = []
        for i in range(d):
            b = row[i]
            if b < 0:
                continue
            js = row[:i][row[:i] >= 0]
            det.append((int((G[js, :i] == b).any(1).sum()) if i else 0, i))
        det.sort()
        for pos, (_, i) in enumerate(det[:gd]):
            P[a, pos] = row[i]
    return P


def oracle_merge(P, gd):
    N = P.shape[0]
    h = gd // 2
    rev = [[] for _ in range(N)]
    for p in range(gd):
        for u in range(N):
            if P[u, p] >= 0:
                rev[P[u, p]].append(u)
    F = np.full((N, gd), -1, np.int32)
    for v in range(N):
        r = rev[v][:gd]
        head = [int(w) for w in P[v, :h] if w >= 0]
        out = head + [u for u in r if u not in head] + [int(w) for w in P[v, h:] if w >= 0 and w not in r]
        out = out[:gd]
        F[v, :len(out)] = out
    return F


def oracle_search(Q, X, F, seeds, k, itopk, width, max_iter, min_iter):
    """(d2 fp32 [nq, k], pos int64 [nq, k]) by the rule of ``ops.cagra_search``; lattice data only."""
    nq = Q.shape[0]
    Xd, Qd = X.astype(np.float64), Q.astype(np.float64)
    od = np.full((nq, k), np.inf, np.float32)
    oi = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        visited, lst = set(), []

        def merge(cands):
            new = []
            for c in cands:
                c = int(c)
                if c >= 0 and c not in visited:
                    visited.add(c)
                    new.append(c)
            if new:
                d2 = ((Xd[new] - Qd[q]) ** 2).sum(1)
                assert np.all(d2 == np.round(d2)) and d2.max() < 2 ** 24
                lst.extend([float(d), c, False] for d, c in zip(d2, new))
                lst.sort(key=lambda e: (e[0], e[1]))
                del lst[itopk:]

        merge(seeds[q])
        for t in range(max_iter):
            parents = [e for e in lst if not e[2]][:width]
            if not parents:
                if t >= min_iter:
                    break
                continue
            for e in parents:
                e[2] = True
            merge(np.concatenate([F[e[1]] for e in parents]))
        for j, e in enumerate(lst[:k]):
            od[q, j], oi[q, j] = e[0], e[1]
    return od, oi


# ------------------------------------------------------------------------------------- inputs
def knn_rows(N, d, identical=0, seed=0):
    """Exact kNN lists int32 [N, d] of random rows without the row's own index (fp64, ties by index;
    ``identical`` leading rows are one point). d > N - 1 leaves a -1 tail."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, 6))
    if identical:
        X[:identical] = X[0]
    D = ((X[:, None, :] - X[None]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    order = np.argsort(D, axis=1, kind="stable")[:, :min(d, N - 1)]
    G = np.full((N, d), -1, np.int32)
    G[:, :order.shape[1]] = order
    return G


def lattice(N, n, seed=0):
    return np.random.default_rng(seed).integers(-8, 9, (N, n)).astype(np.float32)


def random_graph(N, gd, seed=0):
    """Hand-built F: random distinct valid rows with -1 tails of every length (row 0 is empty)."""
    rng = np.random.default_rng(seed)
    F = np.full((N, gd), -1, np.int32)
    for v in range(1, N):
        c = gd if v % 3 else int(rng.integers(0, gd + 1))
        c = min(c, N - 1)
        F[v, :c] = rng.choice(N, size=c, replace=False)
    return F


# -------------------------------------------------------------------------------- check bodies
def check_graph_properties(P, F, gd):
    h = gd // 2
    N = P.shape[0]
    for M in (P, F):
        valid = M >= 0
        assert not (valid[:, 1:] & ~valid[:, :-1]).any()  # no -1 before a valid entry
        for v in range(N):
            row = M[v][M[v] >= 0]
            assert len(set(row.tolist())) == row.size, (v, row)  # no duplicate
            assert v not in row  # no self edge
        assert M.max(initial=-1) < N
    assert np.array_equal(F[:, :h], P[:, :h])


def run_graph_case(ops, G, gd, device):
    """Prune and merge equal the oracle, repeat to the byte, and keep the row properties."""
    d = torch.device(device)
    Gt = torch.from_numpy(G).to(d)
    P1, P2 = ops.cagra_prune(Gt, gd), ops.cagra_prune(Gt, gd)
    assert P1.dtype == torch.int32 and tuple(P1.shape) == (G.shape[0], gd)
    assert torch.equal(P1, P2)
    P = P1.cpu().numpy()
    assert np.array_equal(P, oracle_prune(G, gd))
    F1, F2 = ops.cagra_merge(P1, gd), ops.cagra_merge(P1, gd)
    assert F1.dtype == torch.int32 and tuple(F1.shape) == (G.shape[0], gd)
    assert torch.equal(F1, F2)
    F = F1.cpu().numpy()
    assert np.array_equal(F, oracle_merge(P, gd))
    check_graph_properties(P, F, gd)
    return P, F


def run_seed_case(ops, device, n=35, nq=33, N=300, S=64, seed=7):
    d = torch.device(device)
    Q = lattice(nq, n, seed=5)
    Q[1] = -0.0 * Q[1]  # signed zeros are different bit patterns
    want = oracle_seeds(Q, N, S, seed)
    host = ops.cagra_seeds(torch.from_numpy(Q), N, S, seed)
    got = ops.cagra_seeds(torch.from_numpy(Q).to(d), N, S, seed)
    assert got.dtype == torch.int32 and tuple(got.shape) == (nq, S)
    assert np.array_equal(host.numpy(), want)
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.min() >= 0 and want.max() < N
    perm = np.random.default_rng(1).permutation(nq)
    gp = ops.cagra_seeds(torch.from_numpy(Q[perm]).to(d), N, S, seed)
    assert np.array_equal(gp.cpu().numpy(), want[perm])
    other = ops.cagra_seeds(torch.from_numpy(Q).to(d), N, S, seed + 1).cpu().numpy()
    assert (other != want).mean() > 0.9 - 1.0 / N  # another seed, other nodes (1 / N agree by chance)
    return want


def search(ops, Q, X, F, device, k, itopk, width, max_iter, min_iter, S, seed=3):
    d = torch.device(device)
    as_t = lambda a: a.to(d) if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(d)
    od, oi = ops.cagra_search(as_t(Q), as_t(X), as_t(F), k, itopk, width, max_iter, min_iter, S, seed)
    assert od.dtype == torch.float32 and oi.dtype == torch.int64
    return od.cpu().numpy(), oi.cpu().numpy()


def check_search(ops, Q, X, F, got, k, itopk, width, max_iter, min_iter, S, seed=3):
    """Bit-for-bit against the oracle (keys and ids)."""
    Qn = Q.cpu().numpy() if isinstance(Q, torch.Tensor) else Q
    Xn = X.cpu().numpy() if isinstance(X, torch.Tensor) else X
    if max_iter == 0:
        max_iter = ops.cagra_auto_iters(Qn.shape[1], itopk, width, F.shape[1], S)
    seeds = oracle_seeds(Qn, Xn.shape[0], S, seed)
    wd, wi = oracle_search(Qn, Xn, F, seeds, k, itopk, width, max_iter, min_iter)
    assert got[0].shape == wd.shape and got[1].shape == wi.shape
    assert np.array_equal(got[1], wi), np.argwhere(got[1] != wi)[:5]
    assert np.array_equal(got[0].view(np.uint32), wd.view(np.uint32))


def run_search_case(ops, name, device, N=300):
    n, gd, itopk, width, k, max_iter, min_iter, nq, S = SEARCH_CASES[name]
    X, Q, F = lattice(N, n, seed=1), lattice(nq, n, seed=2), random_graph(N, gd, seed=4)
    a = search(ops, Q, X, F, device, k, itopk, width, max_iter, min_iter, S)
    b = search(ops, Q, X, F, device, k, itopk, width, max_iter, min_iter, S)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    check_search(ops, Q, X, F, a, k, itopk, width, max_iter, min_iter, S)
    return a


def run_layout_case(ops, device, n, pad, shift):
    """A strided Q (ldq > n) and an X view with row stride n + pad starting `shift` floats into its
    buffer: pad or shift not a multiple of 4 takes the scalar-load path."""
    N, nq, gd = 300, 9, 32
    X, Q, F = lattice(N, n, seed=1), lattice(nq, n, seed=2), random_graph(N, gd, seed=4)
    d = torch.device(device)
    xb = torch.zeros(N * (n + pad) + shift, device=d)
    Xv = xb[shift:].view(N, n + pad)[:, :n]
    Xv.copy_(torch.from_numpy(X))
    qb = torch.zeros((nq, n + 5), device=d)
    qb[:, :n] = torch.from_numpy(Q)
    Qv = qb[:, :n]
    assert Xv.stride(0) == n + pad and Qv.stride(0) == n + 5
    got = search(ops, Qv, Xv, F, device, 10, 64, 1, 5, 0, 64)
    check_search(ops, Q, X, F, got, 10, 64, 1, 5, 0, 64)


def run_edge_cases(ops, device):
    # every row of F empty: the result is the best seeds
    N, n = 300, 35
    X, Q = lattice(N, n, seed=1), lattice(9, n, seed=2)
    F = np.full((N, 8), -1, np.int32)
    got = search(ops, Q, X, F, device, 10, 32, 1, 0, 0, 32)
    check_search(ops, Q, X, F, got, 10, 32, 1, 0, 0, 32)
    seeds = oracle_seeds(Q, N, 32, 3)
    for q in range(9):
        assert set(got[1][q].tolist()) <= set(seeds[q].tolist())
    # one row; more seeds than rows
    X1, F1 = lattice(1, n, seed=1), np.full((1, 1), -1, np.int32)
    got = search(ops, Q, X1, F1, device, 5, 32, 1, 0, 0, 32)
    check_search(ops, Q, X1, F1, got, 5, 32, 1, 0, 0, 32)
    assert np.all(got[1][:, 0] == 0) and np.all(got[1][:, 1:] == -1) and np.all(np.isinf(got[0][:, 1:]))
    # permuting Q permutes the rows of the result
    F = random_graph(N, 32, seed=4)
    Q = lattice(40, n, seed=2)
    a = search(ops, Q, X, F, device, 10, 64, 1, 0, 0, 64)
    perm = np.random.default_rng(1).permutation(40)
    b = search(ops, Q[perm], X, F, device, 10, 64, 1, 0, 0, 64)
    assert np.array_equal(a[0][perm], b[0]) and np.array_equal(a[1][perm], b[1])


def run_exhaustive_case(ops, device, seed=0):
    """itopk >= N and max_iter = N: nothing is evicted, every node reachable from the seeds is
    expanded, so the result is the exact kNN over the reachable set (positions with a clear gap)."""
    N, n, gd, k, itopk, S = 200, 16, 16, 10, 256, 256
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, n)).astype(np.float32)
    Q = rng.standard_normal((40, n)).astype(np.float32)
    d = torch.device(device)
    F = ops.cagra_merge(ops.cagra_prune(torch.from_numpy(knn_rows_of(X, 32)).to(d), gd), gd)
    Fn = F.cpu().numpy()
    seeds = ops.cagra_seeds(torch.from_numpy(Q).to(d), N, S, 3).cpu().numpy()
    od, oi = search(ops, Q, X, Fn, device, k, itopk, 1, N, 0, S)
    D = ((Q.astype(np.float64)[:, None, :] - X.astype(np.float64)[None]) ** 2).sum(-1)
    covered = []
    for q in range(Q.shape[0]):
        reach = set(int(s) for s in seeds[q])
        todo = list(reach)
        while todo:
            for w in Fn[todo.pop()]:
                if w >= 0 and int(w) not in reach:
                    reach.add(int(w))
                    todo.append(int(w))
        covered.append(len(reach) / N)
        r = np.array(sorted(reach))
        order = r[np.argsort(D[q, r], kind="stable")]
        full = D[q, order][:k + 1]
        gap = np.diff(full) > 1e-6 * np.abs(full[1:])
        clear = np.concatenate([[True], gap[:-1]]) & gap
        assert clear.mean() > 0.9
        assert np.array_equal(oi[q][clear], order[:k][clear]), (q, oi[q], order[:k])
        np.testing.assert_allclose(od[q], D[q, oi[q]], rtol=1e-5)
    assert min(covered) >= 0.95, min(covered)


def knn_rows_of(X, d):
    Xd = X.astype(np.float64)
    D = ((Xd[:, None, :] - Xd[None]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    return np.argsort(D, axis=1, kind="stable")[:, :d].astype(np.int32)


LIMITS = {  # gd, k, itopk, width, max_iter
    "itopk544": (32, 10, 544, 1, 0),
    "width_x_gd": (64, 10, 64, 9, 0),
    "k_gt_itopk": (32, 65, 64, 1, 0),
    "visited_table": (64, 10, 64, 1, 2000),
}


def run_limit_case(ops, name, device, monkeypatch):
    import pytest

    from spark_rapids_ml_nai_amd.ops import native

    gd, k, itopk, width, max_iter = LIMITS[name]
    X, Q, F = lattice(300, 16, seed=1), lattice(3, 16, seed=2), random_graph(300, gd, seed=4)
    monkeypatch.setattr(native, "call_status", lambda *a, **kw: pytest.fail("a refused search was launched"))
    monkeypatch.setattr(native, "call", lambda *a, **kw: pytest.fail("a refused search was launched"))
    with pytest.raises(ValueError):
        search(ops, Q, X, F, device, k, itopk, width, max_iter, 0, 64)
