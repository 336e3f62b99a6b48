"""Oracle, case builders and the contract checker of the NN-descent join on CSR rows.

The oracle is written from the join's description, not from ``ops``: the fp32 rows densified to
fp64 (``csr_knn_cases.Oracle``), the candidate union of every row computed literally in Python —

    own list                       pos[i, :]
    neighbours' neighbours         pos[pos[i, :a], :b]
    reverse neighbours             the first R sources of the edges (src, slot) -> i, in edge order

with -1 (and out-of-range) entries dropped — and the k smallest of the union by (distance, id).

Bounds (derived in ``csr_knn_cases``; u = 2^-24, t = nnz_x + nnz_y):
  sqeuclidean  |d2 - D| <= (t + 4) u D        (direct form, as srml_csr_refine_f32)
  hellinger    |d^2 - (1 - S)| <= (t + 4) u
  jaccard      bit-equal to the fp32 expression on the exact integer counts

Two kinds of case. LATTICE: the non-zeros are small integers and sum (x - y)^2 < 2^24 for every
pair (asserted), so every fp32 operation of the direct form is exact whatever its order: keys, ids
and tie order must equal the oracle bit for bit; every jaccard case is a lattice case. GENERIC:
standard-normal / probability rows; every returned pair lies within its bound, no omitted
candidate is decidedly nearer than a returned one, and on the rows the oracle decides alone (at
least 90 % of each case, asserted by the builder) the id set is the oracle's. No row is skipped."""
import functools

import numpy as np
import torch

import csr_knn_cases as C

VALUES = C.VALUES


def lattice_rows(N, n, mean_nnz, seed, special=()):
    """Sparse rows with non-zeros in {-3 .. 3} \\ {0}; ``special``: {row: nnz} overrides. Row 1 is
    empty and row 2 long (``csr_knn_cases.random_rows``); a few rows are bit-identical copies, so
    exact ties exist."""
    rng = np.random.default_rng(seed)
    rows = C.random_rows(N, n, mean_nnz, seed, "ones")
    for r, c in dict(special).items():
        cols = np.sort(rng.choice(n, int(c), replace=False)) if c else np.zeros(0, np.int64)
        rows[r] = (cols, np.ones(len(cols), np.float32))
    rows = [(c, rng.choice(np.array([-3, -2, -1, 1, 2, 3], np.float32), len(c))) for c, _ in rows]
    for r in range(5, N, 7):  # copies of the row before: tied distances to every query
        rows[r] = (rows[r - 1][0].copy(), rows[r - 1][1].copy())
    return rows


def generic_rows(N, n, mean_nnz, seed, values, special=()):
    rng = np.random.default_rng(seed + 17)
    rows = C.random_rows(N, n, mean_nnz, seed, values)
    for r, c in dict(special).items():
        cols = np.sort(rng.choice(n, int(c), replace=False)) if c else np.zeros(0, np.int64)
        if values == "normal":
            v = rng.standard_normal(len(cols))
            v[v == 0] = 1.0
        elif values == "ones":
            v = np.ones(len(cols))
        else:
            v = rng.random(len(cols)) + 1e-3
            v = v / v.sum() if len(cols) else v
        rows[r] = (cols, v.astype(np.float32))
    return rows


def start_graph(kind, N, kw, seed):
    """int64 [N, kw] start graphs: ``random``; ``ring`` (row i lists i + 1 .. i + kw mod N: every
    reverse list has exactly kw entries when kw < N); ``star`` (every row lists row 0 and nothing
    else: one reverse list of N entries, all others empty); ``padded`` (random with -1 entries,
    row 0 all -1); ``dups`` (every slot of a row holds the same id: the union is all duplicates)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        return torch.randint(0, N, (N, kw), generator=g)
    if kind == "ring":
        return (torch.arange(N).view(-1, 1) + 1 + torch.arange(kw).view(1, -1)) % N
    if kind == "star":
        pos = torch.full((N, kw), -1, dtype=torch.int64)
        pos[:, 0] = 0
        return pos
    if kind == "padded":
        pos = torch.randint(0, N, (N, kw), generator=g)
        pos[torch.rand((N, kw), generator=g) < 0.3] = -1
        pos[0] = -1
        return pos
    if kind == "dups":
        return torch.randint(0, N, (N, 1), generator=g).expand(N, kw).contiguous()
    raise ValueError(kind)


def reverse_lists(pos):
    """(perm, off) as the builders pass them: the N kw edges grouped by target, stable."""
    N = pos.shape[0]
    srt, perm = torch.sort(pos.reshape(-1), stable=True)
    return perm, torch.searchsorted(srt, torch.arange(N + 1, dtype=srt.dtype))


def candidate_sets(pos, a, b, R):
    """The candidate union of every row, literally: a list of sorted id lists."""
    pos = pos.tolist()
    N, kw = len(pos), len(pos[0])
    rev = [[] for _ in range(N)]
    for src in range(N):  # edge order: (source, slot) ascending
        for tgt in pos[src]:
            if 0 <= tgt < N:
                rev[tgt].append(src)
    out = []
    for i in range(N):
        c = set(pos[i])
        for nb in pos[i][:a]:
            if 0 <= nb < N:
                c.update(pos[nb][:b])
        c.update(rev[i][:R])
        out.append(sorted(j for j in c if 0 <= j < N))
    return out


class Join:
    """One join case: the rows, the graph, the fan-out, the oracle's answer."""

    def __init__(self, name, A, metric, pos, k, a, b, R, lattice):
        self.name, self.A, self.metric, self.pos, self.k, self.a, self.b, self.R = name, A, metric, pos, k, a, b, R
        self.lattice = lattice
        self.N = A.shape[0]
        self.orc = C.Oracle(A, A, metric)
        if lattice and metric == "sqeuclidean":
            assert float(self.orc.D.max()) < 2.0 ** 24, "not a lattice case"
        self.perm, self.off = reverse_lists(pos)
        self.cands = candidate_sets(pos, a, b, R)
        D, eps = self.orc.D.numpy(), self.orc.eps.numpy()
        self.want_ids, self.decided = [], np.zeros(self.N, dtype=bool)
        for i, c in enumerate(self.cands):
            c = np.asarray(c, dtype=np.int64)
            order = c[np.lexsort((c, D[i, c]))] if len(c) else c
            top, rest = order[:k], order[k:]
            self.want_ids.append(top)
            self.decided[i] = (len(rest) == 0 or len(top) == 0
                               or (D[i, top] + eps[i, top]).max() < (D[i, rest] - eps[i, rest]).min())
        if not lattice:
            share = float(self.decided.mean())
            assert share >= 0.9, "case %s: the oracle decides %.3f of the rows only" % (name, share)


def check_join(case, keys, ids, r0=0, r1=None):
    """The contract on rows r0 .. r1 of ``case``, none skipped; AssertionError names the violation."""
    r1 = case.N if r1 is None else r1
    k, D, eps = case.k, case.orc.D.numpy(), case.orc.eps.numpy()
    keys32 = keys.detach().cpu().contiguous().numpy()
    ids = ids.detach().cpu().numpy()
    assert keys32.dtype == np.float32 and ids.dtype == np.int64
    assert keys32.shape == (r1 - r0, k) and ids.shape == (r1 - r0, k), (keys32.shape, ids.shape)
    keys = keys32.astype(np.float64)
    for q in range(r1 - r0):
        i = r0 + q
        cand = case.cands[i]
        m = min(k, len(cand))
        assert np.all(np.isposinf(keys[q, m:])) and np.all(ids[q, m:] == -1), "row %d: padding" % i
        got, key = ids[q, :m], keys[q, :m]
        assert np.all(np.isin(got, cand)), "row %d returns an id that is no candidate" % i
        assert len(set(got.tolist())) == m, "row %d returns an id twice" % i
        assert np.all(np.isfinite(key)), "row %d: a candidate without a distance" % i
        nxt = (key[1:] > key[:-1]) | ((key[1:] == key[:-1]) & (got[1:] > got[:-1]))
        assert np.all(nxt), "row %d is not ascending by (key, id)" % i
        val = key * key if case.metric == "hellinger" else key
        err = np.abs(val - D[i, got])
        bad = int(np.argmax(err - eps[i, got])) if m else 0
        assert np.all(err <= eps[i, got]), "row %d: distance off its bound (err %.3e, bound %.3e)" % (
            i, float(err[bad]), float(eps[i, got][bad]))
        want = case.want_ids[i]
        if case.lattice:
            assert np.array_equal(got, want), "row %d: ids or tie order differ from the oracle" % i
            assert np.array_equal(keys32[q, :m], D[i, want].astype(np.float32)), (
                "row %d: keys differ from the oracle bit for bit" % i)
            continue
        rest = np.setdiff1d(np.asarray(cand, dtype=np.int64), got)
        if len(rest) and m:
            assert (D[i, got] - eps[i, got]).max() <= (D[i, rest] + eps[i, rest]).min(), (
                "row %d returns a candidate decidedly farther than one it omits" % i)
        if case.decided[i]:
            assert set(got.tolist()) == set(want.tolist()), "row %d (decided): the id set differs" % i


def run(case, device, r0=0, r1=None, **over):
    """``ops.csr_nnd_join`` on the case (rows r0 .. r1 as a block with absolute offsets)."""
    from spark_rapids_ml_nai_amd import ops

    r1 = case.N if r1 is None else r1
    P = ops.csr_prepare(C.to(case.A, device), case.metric)
    Q = P if (r0, r1) == (0, case.N) else P.rows(r0, r1)
    arg = dict(pos=case.pos.to(device), perm=case.perm.to(device), off=case.off.to(device), k=case.k, a=case.a,
               b=case.b, R=case.R)
    arg.update(over)
    return ops.csr_nnd_join(Q, P, arg["pos"], arg["perm"], arg["off"], arg["k"], arg["a"], arg["b"], arg["R"],
                            case.metric, row0=r0)


# name: (metric, lattice, N, n, mean nnz, special rows, graph, list width, k, (a, b, R))
CAP, LDS = 512, 2048  # ops.CSR_NND_CAND_CAP / ops.CSR_NND_LDS_CAP (test_csr_nnd_join compares them)
LONG = {3: LDS - 1, 4: LDS, 6: LDS + 1, 8: 2100}  # query rows around the LDS cap, and nnz = n
SPEC = {
    "n2_k1": ("sqeuclidean", True, 2, 50, 5, {}, "random", 1, 1, (0, 0, 0)),
    "n4_k5_padded_out": ("sqeuclidean", True, 4, 60, 6, {}, "random", 5, 5, (8, 8, 16)),
    "n4_k64_jaccard": ("jaccard", True, 4, 60, 6, {}, "ring", 3, 64, (8, 8, 16)),
    "n65_ring_k15": ("sqeuclidean", True, 65, 700, 12, {}, "ring", 15, 15, (8, 8, 16)),
    "n65_random_k33_jaccard": ("jaccard", True, 65, 300, 30, {}, "random", 33, 33, (8, 8, 16)),
    "n65_dups_k5_jaccard": ("jaccard", True, 65, 300, 30, {}, "dups", 5, 5, (8, 8, 16)),
    "n65_rescore_k15": ("sqeuclidean", False, 65, 900, 20, {}, "random", 15, 15, (0, 0, 0)),
    "n65_lds_cap": ("sqeuclidean", True, 65, 2100, 40, LONG, "random", 15, 15, (8, 8, 16)),
    "n65_lds_cap_jaccard": ("jaccard", True, 65, 2100, 40, LONG, "padded", 15, 15, (8, 8, 16)),
    "n65_lds_cap_hellinger": ("hellinger", False, 65, 2100, 300, LONG, "random", 15, 15, (8, 8, 16)),
    "n257_padded_k64": ("sqeuclidean", False, 257, 3000, 25, {}, "padded", 64, 64, (8, 8, 16)),
    "n257_star_k5_fan_gt_k": ("hellinger", False, 257, 300, 40, {}, "star", 5, 5, (9, 3, 16)),
    "n257_ring_k5_fan_gt_k": ("sqeuclidean", True, 257, 1500, 15, {}, "ring", 5, 5, (9, 7, 16)),
    "n257_cap_minus_1": ("sqeuclidean", True, 257, 1500, 15, {}, "random", 64, 33, (20, 20, CAP - 464 - 1)),
    "n257_cap": ("sqeuclidean", True, 257, 1500, 15, {}, "random", 64, 33, (20, 20, CAP - 464)),
    "n257_cap_plus_1": ("sqeuclidean", True, 257, 1500, 15, {}, "random", 64, 33, (20, 20, CAP - 464 + 1)),
    "n600_random_k15": ("sqeuclidean", False, 600, 4000, 30, {}, "random", 15, 15, (8, 8, 16)),
    "n600_random_k15_hellinger": ("hellinger", False, 600, 400, 40, {}, "random", 15, 15, (8, 8, 16)),
    "n600_star_k15_jaccard": ("jaccard", True, 600, 400, 40, {}, "star", 15, 15, (8, 8, 16)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    metric, lattice, N, n, nnz, special, graph, kw, k, (a, b, R) = SPEC[name]
    seed = sum(map(ord, name))
    if metric == "jaccard":
        rows = generic_rows(N, n, nnz, seed, "ones", special)
    elif lattice:
        rows = lattice_rows(N, n, nnz, seed, special)
    else:
        rows = generic_rows(N, n, nnz, seed, VALUES[metric], special)
    return Join(name, C.csr_from_rows(rows, n), metric, start_graph(graph, N, kw, seed), k, a, b, R, lattice)
