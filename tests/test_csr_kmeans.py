"""Sparse KMeans on the CPU: the checkers of ``csr_kmeans_cases`` against wrong answers they must
reject, the torch reference forms of ``ops.csr_nearest_centroid`` / ``csr_cluster_sums`` /
``csr_gather_dense`` under the same contracts as the kernels, and the estimator route
(``KMeans(enable_sparse_data_optim=True)``): planted fit, transform, persistence, the unchanged
dense default, the 2^20-column fit and two gloo ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import csr_kmeans_cases as K
from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.clustering import KMeans, KMeansModel
from spark_rapids_ml_nai_amd.core.base import CSR
from spark_rapids_ml_nai_amd.core.dataframe import DataFrame
from spark_rapids_ml_nai_amd.utils.determinism import set_deterministic

TK, STAGE, ROWS = K.TK, K.STAGE, K.ROWS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exported_constants_are_the_kernels():
    """The edge shapes of the tests are derived from these: they must be the kernels' own."""
    lib = ops.native.lib()
    assert tuple(int(lib.srml_csr_kmeans_config(i)) for i in range(3)) == (TK, STAGE, ROWS)
    assert TK % 64 == 0 and ROWS * STAGE * 12 <= 64 * 1024  # the staged rows (index + fp64 value) fit static LDS


# ------------------------------------------------------------------------------------------ reference forms
@pytest.mark.parametrize("name", K.SEARCH_NAMES)
def test_reference_search_meets_the_contract(name):
    case = K.search_case(name)
    lab, d2 = ops.csr_nearest_centroid(case.A, case.centres())
    assert lab.dtype == torch.int32 and d2.dtype == case.A.data.dtype
    K.check_nearest(case, lab, d2)


def test_every_generic_case_is_decided_by_the_oracle():
    for name in ("generic", "generic_wide", "generic_f64"):
        case = K.search_case(name)
        assert ((case.gap > case.clear) | (case.gap == 0)).mean() >= 0.9


@pytest.mark.parametrize("name", K.SUMS_NAMES)
def test_reference_sums_meet_the_bound(name):
    case = K.sums_case(name)
    sums, counts = ops.csr_cluster_sums(case.A, case.labels_t(), case.k)
    K.check_sums(case, sums, counts)
    set_deterministic(True)
    try:
        fs, fc = ops.csr_cluster_sums(case.A, case.labels_t(), case.k)
    finally:
        set_deterministic(None)
    K.check_sums(case, fs, fc, fixed_scale=ops.csr_fixed_scale(case.A.shape[0], case.vmax) if case.vmax else 1.0)


def test_fixed_scale_keeps_every_sum_inside_i64():
    for rows, vmax in ((1, 1.0), (1200, 2.1), (10 ** 6, 3.4e38), (7, 1e-30), (3, 0.0)):
        s = ops.csr_fixed_scale(rows, vmax)
        assert s == 2.0 ** round(np.log2(s)) and rows * vmax * s <= 2.0 ** 62
        if vmax:
            assert rows * vmax * s > 2.0 ** 60
    with pytest.raises(ValueError, match="finite"):
        ops.csr_fixed_scale(2, float("inf"))


def test_row_offset_blocks_are_accepted():
    case = K.search_case("generic")
    lab, d2 = ops.csr_nearest_centroid(case.A, case.centres())
    labb, d2b = ops.csr_nearest_centroid(K.row_block(case.A, 37, 203), case.centres())
    assert torch.equal(labb, lab[37:203]) and torch.equal(d2b, d2[37:203])
    G = ops.csr_gather_dense(K.row_block(case.A, 37, 203), torch.tensor([0, 165, 3]))
    assert np.array_equal(G.numpy(), K.dense64(case.A)[[37, 202, 40]].astype(np.float32))


def test_gather_dense_and_its_budget(monkeypatch):
    case = K.search_case("stage%d" % STAGE)
    rows = torch.tensor([4, 1, 4, 0])
    assert np.array_equal(ops.csr_gather_dense(case.A, rows).numpy(), K.dense64(case.A)[[4, 1, 4, 0]].astype(np.float32))
    assert ops.csr_gather_dense(case.A, rows[:0]).shape == (0, case.n)
    with pytest.raises(ValueError, match="row outside"):
        ops.csr_gather_dense(case.A, torch.tensor([case.m]))
    monkeypatch.setattr(ops, "_CSR_KM_DENSE_BYTES", 3 * case.n * 4)
    with pytest.raises(ValueError, match=r"4 rows x %d features need %d bytes" % (case.n, 16 * case.n)):
        ops.csr_gather_dense(case.A, rows)


def test_sums_buffer_budget_names_the_sizes(monkeypatch):
    case = K.sums_case("generic")
    monkeypatch.setattr(ops, "_CSR_KM_SUMS_BYTES", case.k * 300 * 8 - 1)
    with pytest.raises(ValueError, match=r"%d x 300 fp64 cluster sums need %d bytes" % (case.k, case.k * 300 * 8)):
        ops.csr_cluster_sums(case.A, case.labels_t(), case.k)
    P = K.planted()
    with pytest.raises(ValueError, match=r"6 x 4096 fp64 cluster sums need"):
        KMeans(k=6, enable_sparse_data_optim=True).fit(DataFrame.from_numpy(P.M))
    monkeypatch.undo()
    monkeypatch.setattr(ops, "_CSR_KM_DENSE_BYTES", 1 << 16)
    with pytest.raises(ValueError, match="candidate rows"):
        KMeans(k=6, enable_sparse_data_optim=True).fit(DataFrame.from_numpy(P.M))


@pytest.mark.parametrize("cols,msg", [([4, 2], "strictly increasing"), ([2, 2], "strictly increasing"),
                                      ([1, 10], "out of range"), ([-1, 3], "out of range")])
def test_bad_indices_raise(cols, msg):
    A = K.csr_from_rows([(np.array([0, 5]), np.ones(2)), (np.array(cols), np.ones(2))], 10)
    for call in (lambda: ops.csr_nearest_centroid(A, torch.zeros((3, 10))),
                 lambda: ops.csr_cluster_sums(A, torch.zeros(2, dtype=torch.int32), 3),
                 lambda: ops.csr_gather_dense(A, torch.tensor([0]))):
        with pytest.raises(ValueError, match=msg):
            call()
    with pytest.raises(ValueError, match="do not match"):
        ops.csr_nearest_centroid(K.search_case("m1").A, torch.zeros((3, 7)))


# ------------------------------------------------------------------------------------------ checker self-tests
def _reference_keys(case, A=None, C=None, with_cnorm=True):
    """(labels, distances) of the expanded form in fp64 on possibly tampered operands."""
    X = K.dense64(case.A if A is None else A)
    C = case.C.astype(np.float64) if C is None else C
    key = (X * X).sum(1)[:, None] - 2 * X @ C.T + ((C * C).sum(1)[None, :] if with_cnorm else 0.0)
    key = np.maximum(key, 0)
    return key.argmin(1), key.min(1)


def test_checker_accepts_the_fp64_expanded_form():
    for name in ("k%d" % (2 * TK + 1), "generic", "stage%d" % (STAGE + 1)):
        case = K.search_case(name)
        K.check_nearest(case, *_reference_keys(case))


def test_checker_rejects_a_dropped_non_zero():
    case = K.search_case("generic")
    ip, ix, v = case.A.indptr.numpy(), case.A.indices.numpy(), case.A.data.numpy()
    rows = [(ix[ip[r]: ip[r + 1]], v[ip[r]: ip[r + 1]]) for r in range(case.m)]
    j = int(np.abs(rows[7][1]).argmax())
    rows[7] = (np.delete(rows[7][0], j), np.delete(rows[7][1], j))
    with pytest.raises(AssertionError, match="row 7"):
        K.check_nearest(case, *_reference_keys(case, A=K.csr_from_rows(rows, case.n)))


def test_checker_rejects_a_skipped_centre_tile():
    case = K.search_case("k%d" % (2 * TK + 1))
    lab, d = _reference_keys(case, C=case.C[:TK].astype(np.float64))  # only the first tile was searched
    assert (case.arg >= TK).any()
    with pytest.raises(AssertionError, match="farther than the band|label"):
        K.check_nearest(case, lab, d)


def test_checker_rejects_a_tie_resolved_to_the_higher_index():
    for name in ("k%d" % (TK + 1), "k%d_lattice" % (TK + 1)):
        case = K.search_case(name)
        lab, d = _reference_keys(case)
        assert lab[3] == 0 and case.gap[3] == 0
        lab[3] = case.k - 1  # the bit-identical copy of centre 0
        with pytest.raises(AssertionError, match="row 3"):
            K.check_nearest(case, lab, d)


def test_checker_rejects_a_label_off_by_one_tile():
    case = K.search_case("k%d" % (2 * TK + 1))
    lab, d = _reference_keys(case)
    move = lab + TK < case.k
    assert move.any()
    with pytest.raises(AssertionError):
        K.check_nearest(case, np.where(move, lab + TK, lab), d)


def test_checker_rejects_a_missing_centre_norm():
    case = K.search_case("generic")
    with pytest.raises(AssertionError):
        K.check_nearest(case, *_reference_keys(case, with_cnorm=False))


def test_sums_checker_rejects_a_row_added_twice_and_a_shifted_column():
    for name in ("generic", "lattice"):
        case = K.sums_case(name)
        K.check_sums(case, torch.from_numpy(case.sums), torch.from_numpy(case.counts))
        X = K.dense64(case.A)
        twice = case.sums.copy()
        twice[case.labels[5]] += X[5]
        with pytest.raises(AssertionError, match="cell"):
            K.check_sums(case, torch.from_numpy(twice), torch.from_numpy(case.counts))
        with pytest.raises(AssertionError, match="cell"):
            K.check_sums(case, torch.from_numpy(np.roll(case.sums, 1, axis=1)), torch.from_numpy(case.counts))
        wrong = case.counts.copy()
        wrong[0] += 1
        with pytest.raises(AssertionError, match="counts"):
            K.check_sums(case, torch.from_numpy(case.sums), torch.from_numpy(wrong))


# ------------------------------------------------------------------------------------------ estimator route
def _pred(model, frame):
    return np.asarray(model.transform(frame).to_numpy("prediction")).astype(np.int64)


@pytest.fixture(scope="module")
def planted_model():
    P = K.planted()
    return P, KMeans(k=K.PLANT_K, seed=K.PLANT_SEED, enable_sparse_data_optim=True).fit(DataFrame.from_numpy(P.M))


def test_sparse_fit_recovers_the_planted_partition(planted_model, tmp_path):
    P, model = planted_model
    frame = DataFrame.from_numpy(P.M)
    lab = _pred(model, frame)
    assert P.recovers(lab)
    assert P.recovers(_pred(KMeans(k=K.PLANT_K, seed=K.PLANT_SEED).fit(frame), frame))  # the dense route
    mean, bound = P.centre_bound(lab)
    err = np.abs(np.asarray(model.cluster_centers_, np.float64) - mean)
    assert (err <= bound).all(), float((err - bound).max())
    assert model.n_cols == K.PLANT_N and model.getOrDefault("enable_sparse_data_optim") is True
    assert model._model_attributes["delta_iters"] == 0 and model._model_attributes["refined_frac"] is None
    assert np.array_equal(_pred(model, DataFrame.from_numpy(P.M.toarray())), lab)  # a dense-array frame of the rows
    model.write().overwrite().save(str(tmp_path / "m"))
    loaded = KMeansModel.load(str(tmp_path / "m"))
    assert np.array_equal(_pred(loaded, frame), lab)


def test_an_empty_cluster_keeps_its_centre_bit_for_bit(monkeypatch):
    """One of the initial centres attracts no row in any iteration: the fit must return it unchanged
    (not 0 / 0, not zeroed), and the other five must be the means of their rows."""
    C0, res = K.fit_with_an_empty_cluster("cpu", monkeypatch)
    C = np.asarray(res["cluster_centers_"], np.float64)
    assert res["n_iter"] >= 2 and np.isfinite(C).all()
    assert np.array_equal(C[5], C0[5])
    assert not np.array_equal(C[:5], C0[:5]) and np.abs(C[:5] - (C0[:5] - 0.01)).max() < 1.0


def test_transform_keeps_sparse_partitions_csr(planted_model, monkeypatch):
    P, model = planted_model
    seen = []
    real = ops.csr_nearest_centroid
    monkeypatch.setattr(ops, "csr_nearest_centroid", lambda A, C, **kw: (seen.append(A.shape), real(A, C, **kw))[1])
    _pred(model, DataFrame.from_numpy(P.M, num_partitions=3))
    assert [s[1] for s in seen] == [K.PLANT_N] * 3 and sum(s[0] for s in seen) == K.PLANT_M


def test_default_is_dense_and_never_touches_the_csr_ops(monkeypatch):
    for name in ("csr_nearest_centroid", "csr_cluster_sums", "csr_gather_dense"):
        monkeypatch.setattr(ops, name, lambda *a, **kw: pytest.fail("a dense fit called a CSR op"))
    est = KMeans(k=3, seed=1)
    assert est.getOrDefault("enable_sparse_data_optim") is False
    X = np.random.default_rng(0).standard_normal((300, 12)).astype(np.float32)
    model = est.fit(DataFrame.from_numpy(X))
    assert _pred(model, DataFrame.from_numpy(X)).shape == (300,)
    M = sp.random(200, 50, density=0.2, format="csr", random_state=1, dtype=np.float32)
    frame = DataFrame.from_numpy(M)  # a sparse vector column under the default: densified, as before
    assert _pred(est.fit(frame), frame).shape == (200,)


def test_auto_route_follows_the_first_row(monkeypatch):
    calls = []
    real = ops.csr_nearest_centroid
    monkeypatch.setattr(ops, "csr_nearest_centroid", lambda A, C, **kw: (calls.append(1), real(A, C, **kw))[1])
    M = sp.random(200, 50, density=0.2, format="csr", random_state=1, dtype=np.float32)
    est = KMeans(k=3, seed=1, enable_sparse_data_optim=None, maxIter=2)
    est.fit(DataFrame.from_numpy(M.toarray()))
    assert not calls
    est.fit(DataFrame.from_numpy(M))
    assert calls


def test_random_init_picks_the_same_rows_sparse_and_dense(monkeypatch):
    P = K.planted()
    seen = {}
    real_csr, real_dense = ops.csr_nearest_centroid, ops.nearest_centroid

    def spy_csr(A, C, **kw):
        out = real_csr(A, C, **kw)
        seen.setdefault("csr", (C.detach().double().numpy(), out[0].numpy()))
        return out

    def spy_dense(X, C, *a, **kw):
        out = real_dense(X, C, *a, **kw)
        seen.setdefault("dense", (C.detach().double().numpy(), out[0].numpy()))
        return out

    monkeypatch.setattr(ops, "csr_nearest_centroid", spy_csr)
    monkeypatch.setattr(ops, "nearest_centroid", spy_dense)
    frame = DataFrame.from_numpy(P.M)
    KMeans(k=K.PLANT_K, seed=K.PLANT_SEED, enable_sparse_data_optim=True, initMode="random", maxIter=1).fit(frame)
    KMeans(k=K.PLANT_K, seed=K.PLANT_SEED, initMode="random", maxIter=1).fit(frame)
    (Cs, ls), (Cd, ld) = seen["csr"], seen["dense"]
    assert np.array_equal(Cs.astype(np.float32), Cd.astype(np.float32))
    decided = K.planted_decided(P, Cs)
    assert decided.mean() > 0.9
    assert np.array_equal(ls[decided], ld[decided])


def test_cosine_and_weights_still_raise():
    with pytest.raises(ValueError):
        KMeans(k=2, enable_sparse_data_optim=True).setWeightCol("w")
    with pytest.raises(ValueError):
        KMeans(k=2, enable_sparse_data_optim=True, distanceMeasure="cosine")


def test_a_million_columns_fit_without_densifying():
    """n = 2^20, m = 2000, k = 8: dense, X alone is 8.4 GB of fp32. The fit and transform run in a
    fresh child process, whose peak resident size is the measurement (this process's peak never
    falls, so it could hide anything). Live at the peak, in units of k n 8 bytes (64 MB): the fp64
    centres (1), their fp32 copy and its contiguous transpose (1/2 + 1/2), the all-reduce buffer (1)
    and the centre update's temporaries — quotient, new centres, squared shift (3): 6. Measured
    here: 5.3."""
    env = dict(os.environ, SRML_FORCE_CPU="1", PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-W", "ignore", "-c", "import csr_kmeans_cases as K; K.million_column_fit()"],
                       cwd=os.path.join(ROOT, "tests"), env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print("peak resident size grew by %.2f x k n 8" % (rec["grown"] / rec["knb"]))
    assert rec["centres"] == [8, 1 << 20] and rec["labels"] == 2000 and rec["clusters"] == 8
    assert rec["grown"] <= 6 * rec["knb"], "peak resident size grew by %d bytes (k n 8 = %d)" % (rec["grown"], rec["knb"])


@pytest.mark.dist
def test_two_gloo_ranks_match_one_rank(monkeypatch):
    monkeypatch.setenv("SRML_FORCE_CPU", "1")
    P = K.planted()
    kw = dict(k=K.PLANT_K, seed=K.PLANT_SEED, enable_sparse_data_optim=True, initMode="random")
    one = KMeans(**kw).fit(DataFrame.from_numpy(P.M))
    two = KMeans(num_workers=2, **kw).fit(DataFrame.from_numpy(P.M, num_partitions=2))
    frame = DataFrame.from_numpy(P.M)
    lab = _pred(one, frame)
    assert np.array_equal(_pred(two, frame), lab)
    # both are within the sums bound of the fp64 means of the same partition (two partial sums per
    # cell add one rounding), so they are within twice that of each other
    mean, bound = P.centre_bound(lab)
    bound = bound + 2 * K.U53 * np.abs(mean)
    a, b = np.asarray(one.cluster_centers_, np.float64), np.asarray(two.cluster_centers_, np.float64)
    assert (np.abs(a - mean) <= bound).all() and (np.abs(b - mean) <= bound).all()
