"""``ops.ivf_search`` (IVF-Flat scan) on a hand-made index at its edges: an empty list, a one-row
list, ``-1`` probes, a query that probes only the empty list, and k = 1 / 64 / 65 (the wave lists
in LDS, their limit, and the candidate-matrix path), at n = 7 (scalar loads) and n = 32 (16-byte
loads).

Oracle: fp64 brute force over exactly the probed lists, computed here. Tolerance: 1e-5 of the
largest reference distance, as ``test_knn`` and ``test_ivf_search`` use (the scan forms
||q||^2 + ||i||^2 - 2 q.i in fp32, whose rounding error scales with the norms, not with the
distance itself).
"""
import functools

import numpy as np
import pytest
import torch

from spark_rapids_ml_nai_amd import ops

import ivfpq_cases as cases

DEVICES = ["cpu", pytest.param("gpu", marks=pytest.mark.gpu)]
N, NLIST, NQ, NPROBE = 300, 6, 65, 3
EMPTY_ONLY = NQ - 1  # the query that probes the empty list and nothing else


@functools.lru_cache(maxsize=None)
def _case(n):
    """Index, queries and the fp64 distances of every query to its candidates (shared, read-only)."""
    lay = cases.make_index(n, 1, 2, N, NLIST, special=True)  # only the list layout is used
    list_off = lay["list_off"]
    lens = (list_off[1:] - list_off[:-1]).tolist()
    assert lens[2] == 0 and lens[3] == 1 and sum(lens) == N
    g = torch.Generator().manual_seed(7 + n)
    X = torch.randn((N, n), generator=g)
    Q = torch.randn((NQ, n), generator=g)
    _, probes = cases.make_queries(lay, NQ, NPROBE, minus_one=True)  # probes[::5, 2] = -1
    probes[EMPTY_ONLY] = torch.tensor([2, -1, -1], dtype=torch.int32)
    assert (probes == 2).any() and (probes == 3).any() and (probes[::5, 2] == -1).all()
    ids = 3 * torch.arange(N)
    lo = list_off.numpy()
    Xd, Qd = X.double().numpy(), Q.double().numpy()
    cand, ref = [], []
    for q in range(NQ):
        c = np.concatenate([np.arange(lo[l], lo[l + 1]) for l in probes[q].tolist() if l >= 0]
                           + [np.zeros(0, np.int64)]).astype(np.int64)
        cand.append(c)
        ref.append(((Xd[c] - Qd[q]) ** 2).sum(1))
    assert cand[EMPTY_ONLY].size == 0
    return X, Q, probes, list_off, ids, cand, ref


@pytest.mark.parametrize("k", [1, 64, 65])
@pytest.mark.parametrize("n", [7, 32])
@pytest.mark.parametrize("device", DEVICES)
def test_ivf_search_edges(device, n, k, monkeypatch):
    if device == "cpu":
        monkeypatch.setenv("SRML_FORCE_CPU", "1")
        d = torch.device("cpu")
    else:
        monkeypatch.delenv("SRML_FORCE_CPU", raising=False)
        d = torch.device("cuda", 0)
    X, Q, probes, list_off, ids, cand, ref = _case(n)
    Xg = X.to(d)
    dist, got = ops.ivf_search(Q.to(d), probes.to(d), list_off.to(d), Xg, ops.row_sqnorm(Xg), ids.to(d), k)
    assert dist.shape == (NQ, k) and got.shape == (NQ, k)
    dist, got = dist.cpu().double().numpy(), got.cpu().numpy()
    tol = 1e-5 * max(r.max() for r in ref if r.size)
    worst = 0.0
    for q in range(NQ):
        cnt = min(k, cand[q].size)
        assert np.all(got[q, cnt:] == -1) and np.all(np.isposinf(dist[q, cnt:])), (q, got[q], dist[q])
        g = got[q, :cnt]
        assert np.all(g >= 0) and np.all(g % 3 == 0), (q, g)
        assert len(set(g.tolist())) == cnt, (q, g)
        where = {int(v): i for i, v in enumerate(cand[q])}
        assert all(int(v) // 3 in where for v in g), (q, g)  # members of a probed list
        if cnt == 0:
            continue
        dq = dist[q, :cnt]
        assert np.all(np.diff(dq) >= 0), (q, dq)
        want = np.sort(ref[q])[:cnt]
        at_ids = ref[q][[where[int(v) // 3] for v in g]]
        err = max(np.abs(dq - want).max(), np.abs(at_ids - want).max())
        worst = max(worst, err)
        assert err < tol, (q, err, tol)
    print("ivf_search edges n=%d k=%d: largest error %.3g of %.3g allowed" % (n, k, worst, tol))
    assert cand[EMPTY_ONLY].size == 0 and np.all(got[EMPTY_ONLY] == -1)
