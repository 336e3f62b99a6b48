"""Shared cases of the CAGRA VPQ tests (``test_cagra_vpq.py`` on the CPU path, ``test_cagra_vpq_gpu.py``
on ``srml_cagra_search_vpq_f32``).

Oracle cases: integer queries and centres in -8..8 and codebooks in -4..4, so every term of the key is
an integer below 2^24 and the key is exactly ``||q - x^||^2``: ``cagra_cases.oracle_search`` over the
reconstruction is the expected result, bit for bit. Generic rows: every returned key within
``(n + M + 8) 2^-24 (||q|| + ||c_l|| + ||r^_i||)^2`` of the fp64 ``||q - x^_i||^2`` (derivation: the
"CAGRA VPQ" section of docs/coverage.md; first order the kernel's roundings sum to n + M + 3)."""
import numpy as np
import pytest
import torch

import cagra_cases as cases
import ivfpq_cases
from spark_rapids_ml_nai_amd import DataFrame, ops
from spark_rapids_ml_nai_amd.knn import ApproximateNearestNeighbors
from spark_rapids_ml_nai_amd.models import knn as mk

N = 300
ACCURACY_CASES = [(128, 32, 0.0), (33, 3, 0.0), (128, 32, 1000.0)]  # n, M, offset of every coordinate
# n, M, pq_bits, nv, (itopk, width, gd), k, nq, max_iter (0 = auto), codes: "" | "view" | "byte" | "wild"
ORACLE_CASES = {
    "n8_m1_nv1_k1_nq1_it1": (8, 1, 4, 1, (32, 1, 4), 1, 1, 1, ""),
    "n33_m3_bytes": (33, 3, 8, 37, (64, 4, 32), 64, 9, 0, ""),
    "n33_m3_row_view": (33, 3, 8, 37, (64, 4, 32), 10, 9, 0, "view"),   # codes start one row in: odd base
    "n8_m4_bits5_nq257": (8, 4, 5, 37, (32, 1, 4), 32, 257, 1, ""),
    "n8_m4_byte_offset": (8, 4, 8, 37, (32, 1, 4), 32, 9, 0, "byte"),    # M % 4 == 0, base not 4-byte aligned
    "n8_m4_codes_past_ksub": (8, 4, 4, 37, (32, 1, 4), 32, 9, 0, "wild"),
    "n128_m32_nv1024": (128, 32, 8, 1024, (64, 4, 32), 64, 9, 0, ""),
    "n128_m64_bits4_itopk512": (128, 64, 4, 37, (512, 1, 32), 512, 3, 0, ""),
    "n36_m12_k1": (36, 12, 8, 37, (64, 4, 32), 1, 9, 0, ""),
    "n36_m12_nq0": (36, 12, 8, 37, (64, 4, 32), 10, 0, 0, ""),
}


def recon(C, lab, cb, codes):  # fp64 (centre part, codeword part) [N, n] of every item; codes clamped
    cd = np.minimum(codes.astype(np.int64), cb.shape[1] - 1)
    return C.astype(np.float64)[lab], np.concatenate([cb.astype(np.float64)[m][cd[:, m]] for m in range(cb.shape[0])], 1)


def run_oracle_case(name, device):
    n, M, bits, nv, (itopk, width, gd), k, nq, max_iter, how = ORACLE_CASES[name]
    ksub, rng, d = 1 << bits, np.random.default_rng(7), torch.device(device)
    C = rng.integers(-8, 9, (nv, n)).astype(np.float32)
    cb = rng.integers(-4, 5, (M, ksub, n // M)).astype(np.float32)
    lab = rng.integers(0, nv, N).astype(np.int32)
    codes = rng.integers(0, 256 if how == "wild" else ksub, (N, M)).astype(np.uint8)
    Q, F = cases.lattice(nq, n, seed=2), cases.random_graph(N, gd, seed=4)
    Xhat = np.add(*recon(C, lab, cb, codes))
    if how == "view":
        ct = torch.from_numpy(np.concatenate([codes[:1], codes])).to(d)[1:]
    elif how == "byte":
        ct = torch.zeros(N * M + 1, dtype=torch.uint8, device=d)[1:].view(N, M)
        ct.copy_(torch.from_numpy(codes))
    else:
        ct = torch.from_numpy(codes).to(d)
    assert how not in ("view", "byte") or d.type != "cuda" or ct.data_ptr() % 4 != 0
    t = lambda a: torch.from_numpy(a).to(d)
    xn = t((Xhat ** 2).sum(1).astype(np.float32))
    od, oi = ops.cagra_search_vpq(t(Q), t(C), t(lab), t(cb), ct, xn, t(F), k, itopk, width, max_iter, 0, itopk, 3)
    od, oi = od.cpu().numpy(), oi.cpu().numpy()
    it = max_iter or ops.cagra_auto_iters(n, itopk, width, gd, itopk, (M, ksub, nv))
    wd, wi = cases.oracle_search(Q, Xhat, F, cases.oracle_seeds(Q, N, itopk, 3), k, itopk, width, it, 0)
    assert np.array_equal(oi, wi), np.argwhere(oi != wi)[:5]
    assert np.array_equal(od.view(np.uint32), wd.view(np.uint32))


def run_accuracy_case(n, M, offset, device):
    rng, d = np.random.default_rng(11), torch.device(device)
    X = (rng.standard_normal((N, n)) + offset).astype(np.float32)
    Q = (rng.standard_normal((40, n)) + offset).astype(np.float32)
    ix = mk.build_cagra(torch.from_numpy(X).to(d), torch.arange(N, device=d), 32, 16, "brute_force_knn", 1,
                        compression=(8, M, 0, 25))
    assert ix.codes.dtype == torch.uint8 and tuple(ix.codes.shape) == (N, M) and ix.vq_labels.dtype == torch.int32
    keys, pos = ops.cagra_search_vpq(torch.from_numpy(Q).to(d), ix.vq_centers, ix.vq_labels, ix.codebooks, ix.codes,
                                     ix.xhat_sqnorm, ix.graph, 64, 64, 1, 0, 0, 64, 3)
    keys, pos = keys.cpu().double().numpy(), pos.cpu().numpy()
    assert (pos >= 0).all()
    c, r = recon(ix.vq_centers.cpu().numpy(), ix.vq_labels.cpu().numpy(), ix.codebooks.cpu().numpy(),
                 ix.codes.cpu().numpy())
    np.testing.assert_allclose(ix.xhat_sqnorm.cpu().numpy(), ((c + r) ** 2).sum(1), rtol=2.0 ** -23)
    Qd = Q.astype(np.float64)[:, None, :]
    want = ((Qd - (c + r)[pos]) ** 2).sum(-1)
    s = np.linalg.norm(Qd, axis=-1) + np.linalg.norm(c, axis=1)[pos] + np.linalg.norm(r, axis=1)[pos]
    ratio = float((np.abs(keys - want) / ((n + M + 8) * 2.0 ** -24 * s ** 2)).max())
    print("cagra vpq key error / bound, n=%d M=%d offset=%g on %s: %.3f" % (n, M, offset, device, ratio))
    assert ratio <= 1.0, ratio


def run_limit_cases(device, monkeypatch):
    def call(n, M, ksub, nv, itopk=64, max_iter=0):
        t = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=torch.device(device))
        return ops.cagra_search_vpq(t(3, n), t(nv, n), t(N, dt=torch.int32), t(M, ksub, max(1, n // M)),
                                    t(N, M, dt=torch.uint8), t(N), torch.from_numpy(cases.random_graph(N, 32)).to(device),
                                    10, itopk, 1, max_iter, 0, 64, 3)
    assert call(128, 32, 256, 37)[1].shape == (3, 10)
    monkeypatch.setattr(ops.native, "call_status", lambda *a, **kw: pytest.fail("a refused search was launched"))
    for args in [(128, 128, 256, 37, 512, 64), (128, 32, 256, 1025), (36, 8, 16, 4)]:  # first: 128 KiB table + walk
        with pytest.raises(ValueError):
            call(*args)


# ---------------------------------------------------------------------------------------- model
AP = {"intermediate_graph_degree": 32, "graph_degree": 16, "itopk_size": 64, "build_algo": "brute_force",
      "compression": {"pq_dim": 0}}


def ann(k=10, **ap):
    return ApproximateNearestNeighbors(k=k, algorithm="cagra", algoParams=dict(AP, **ap), inputCol="features")


def run_model_case():
    X, Q = ivfpq_cases.blobs()
    _, _, knn_df = ann().fit(DataFrame.from_numpy(X)).kneighbors(DataFrame.from_numpy(Q[:60]))
    _, ind, dist = ivfpq_cases.knn_arrays(knn_df)
    assert ind.shape == (60, 10) and all(len(set(r.tolist())) == r.size for r in ind)
    np.testing.assert_allclose(dist, ivfpq_cases.direct_distance(X, Q[:60], ind, "euclidean"), rtol=1e-5, atol=1e-5)
    _, _, knn_df = ann(k=12).fit(DataFrame.from_numpy(X[:7])).kneighbors(DataFrame.from_numpy(Q[:4]))
    for r in ivfpq_cases.knn_arrays(knn_df)[1]:
        assert sorted(r.tolist()) == list(range(7))


def run_exhaustive_model_case():
    """N = 200 <= itopk_size = 256, 1024 seeds, max_iterations = N and kc = itopk_size: nothing is lost
    between the code-scored walk, the exact re-score and the id mapping, so the result is the exact kNN."""
    rng = np.random.default_rng(3)
    X, Q = rng.standard_normal((200, 16)).astype(np.float32), rng.standard_normal((40, 16)).astype(np.float32)
    model = ann(itopk_size=256, max_iterations=200, num_random_samplings=4, refine_ratio=26).fit(DataFrame.from_numpy(X))
    qid, ind, dist = ivfpq_cases.knn_arrays(model.kneighbors(DataFrame.from_numpy(Q))[2])
    exact = ivfpq_cases.exact_ids(X, Q, 10, "euclidean")[qid]
    assert np.array_equal(ind, exact)
    np.testing.assert_allclose(dist, ivfpq_cases.direct_distance(X, Q[qid], exact, "euclidean"), rtol=1e-5, atol=1e-6)
