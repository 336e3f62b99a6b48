"""Sparse KMeans on the device: ``srml_csr_nearest_{f32,f64}`` and ``srml_csr_cluster_sums_{f32,f64}``
against the fp64 oracles of ``csr_kmeans_cases`` at every edge derived from the exported constants
(k, rows per block, staged row length, chunked launches, row-offset blocks), the deterministic
fixed-point sums, and the fit / transform / persistence route of
``KMeans(enable_sparse_data_optim=True)`` on planted data, one and two ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import csr_kmeans_cases as K
from spark_rapids_ml_nai_amd import ops
from spark_rapids_ml_nai_amd.clustering import KMeans, KMeansModel
from spark_rapids_ml_nai_amd.core.dataframe import DataFrame
from spark_rapids_ml_nai_amd.utils.determinism import set_deterministic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = {}  # the worst error / bound ratios seen (measurements for docs/coverage.md, not thresholds)


def _record(kind, name, ratio):
    if ratio is not None and ratio > RATIOS.get(kind, (-1.0, ""))[0]:
        RATIOS[kind] = (ratio, name)
    out = os.environ.get("SRML_CSR_KMEANS_RATIOS")
    if out:
        with open(out, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


def test_exported_constants_are_the_kernels():
    lib = ops.native.lib()
    assert tuple(int(lib.srml_csr_kmeans_config(i)) for i in range(3)) == (K.TK, K.STAGE, K.ROWS)
    assert K.TK % 64 == 0 and int(lib.srml_csr_kmeans_config(3)) == -1


@pytest.mark.parametrize("name", K.SEARCH_NAMES)
def test_search_meets_its_contract(gpu_device, name):
    case = K.search_case(name)
    lab, d2 = ops.csr_nearest_centroid(K.to(case.A, gpu_device), case.centres(gpu_device))
    assert lab.dtype == torch.int32 and d2.dtype == case.A.data.dtype and lab.is_cuda
    r = K.check_nearest(case, lab, d2)
    print("%s: label %.3g dist %.3g of the bound" % (name, r["label"], r["dist"]))
    _record("search_label_" + case.contract, name, r["label"])
    _record("search_dist_" + case.contract, name, r["dist"])


@pytest.mark.parametrize("name", ["all_empty", "m%d" % (K.ROWS + 1)])
def test_empty_rows_get_the_smallest_centre_norm(gpu_device, name):
    case = K.search_case(name)
    lab, d2 = ops.csr_nearest_centroid(K.to(case.A, gpu_device), case.centres(gpu_device))
    cn = (case.C.astype(np.float64) ** 2).sum(1)
    empty = np.nonzero(case.t == 0)[0]
    assert empty.size
    assert (lab.cpu().numpy()[empty] == cn.argmin()).all()
    assert (d2.cpu().numpy()[empty] == np.float32(cn.min())).all()  # the fp32 rounding of the fp64 sum, as it is


@pytest.mark.parametrize("name", ["k%d" % (2 * K.TK + 1), "stage%d" % (K.STAGE + 1), "generic", "generic_f64"])
def test_one_block_launches_equal_one_launch(gpu_device, monkeypatch, name):
    case = K.search_case(name)
    A, C = K.to(case.A, gpu_device), case.centres(gpu_device)
    lab, d2 = ops.csr_nearest_centroid(A, C)
    calls = []
    real = ops.native.call_status
    monkeypatch.setattr(ops.native, "call_status", lambda n, *a: (calls.append(n), real(n, *a))[1])
    monkeypatch.setattr(ops, "_CSR_KM_LAUNCH_ROWS", K.ROWS)
    lab1, d21 = ops.csr_nearest_centroid(A, C)
    assert sum(n.startswith("srml_csr_nearest_") for n in calls) == -(-case.m // K.ROWS)
    assert torch.equal(lab, lab1) and torch.equal(d2, d21)


def test_centre_table_budget_and_reuse(gpu_device, monkeypatch):
    """The transposed, padded centre table: refused with its sizes past the budget; kept in ``ws`` and
    rewritten in full by every call (fewer centres of other values after more leave nothing behind)."""
    case = K.search_case("k65")
    A, C = K.to(case.A, gpu_device), case.centres(gpu_device)
    ws = {}
    lab, d2 = ops.csr_nearest_centroid(A, C, ws=ws)
    (table,) = ws.values()
    assert table.shape == (case.n, 128)
    C2 = torch.cat([C[:64] * 0.5, C[64:] + 1.0])
    ops.csr_nearest_centroid(A, C2, ws=ws)
    lab1, d21 = ops.csr_nearest_centroid(A, C, ws=ws)
    assert list(ws.values())[0] is table and torch.equal(lab, lab1) and torch.equal(d2, d21)
    assert torch.equal(table[:, :65], C.t()) and not bool(table[:, 65:].any())
    monkeypatch.setattr(ops, "_CSR_KM_CT_BYTES", case.n * 128 * 4 - 1)
    with pytest.raises(ValueError, match=r"%d x 128 transposed centre table \(k = 65 padded to 128\) needs %d bytes"
                       % (case.n, case.n * 128 * 4)):
        ops.csr_nearest_centroid(A, C)


def test_row_offset_blocks_are_accepted(gpu_device):
    """A block whose row offsets do not start at 0 (absolute offsets into the whole matrix's arrays)."""
    case = K.search_case("generic")
    A, C = K.to(case.A, gpu_device), case.centres(gpu_device)
    lab, d2 = ops.csr_nearest_centroid(A, C)
    lo, hi = 37, 203
    labb, d2b = ops.csr_nearest_centroid(K.row_block(A, lo, hi), C)
    assert torch.equal(labb, lab[lo:hi]) and torch.equal(d2b, d2[lo:hi])
    sc = K.sums_case("generic")
    As, labels = K.to(sc.A, gpu_device), sc.labels_t(gpu_device)
    set_deterministic(True)
    try:
        whole, _ = ops.csr_cluster_sums(As, labels, sc.k)
        a, _ = ops.csr_cluster_sums(K.row_block(As, 0, 300), labels[:300], sc.k)
        b, cb = ops.csr_cluster_sums(K.row_block(As, 300, sc.A.shape[0]), labels[300:], sc.k)
    finally:
        set_deterministic(None)
    assert int(cb.sum()) == sc.A.shape[0] - 300
    assert (whole - (a + b)).abs().max() <= 2 * K.U53 * whole.abs().max()


def test_bad_indices_raise_before_any_launch(gpu_device, monkeypatch):
    monkeypatch.setattr(ops.native, "call_status", lambda *a: pytest.fail("a kernel was launched"))
    monkeypatch.setattr(ops.native, "call", lambda *a: pytest.fail("a kernel was launched"))
    C = torch.zeros((3, 10), device=gpu_device)
    for cols, msg in (([4, 2], "strictly increasing"), ([2, 2], "strictly increasing"), ([1, 10], "out of range"),
                      ([-1, 3], "out of range")):
        A = K.to(K.csr_from_rows([(np.array([0, 5]), np.ones(2)), (np.array(cols), np.ones(2))], 10), gpu_device)
        with pytest.raises(ValueError, match=msg):
            ops.csr_nearest_centroid(A, C)
        with pytest.raises(ValueError, match=msg):
            ops.csr_cluster_sums(A, torch.zeros(2, dtype=torch.int32, device=gpu_device), 3)


@pytest.mark.parametrize("name", K.SUMS_NAMES)
def test_cluster_sums_meet_their_bound(gpu_device, name):
    case = K.sums_case(name)
    sums, counts = ops.csr_cluster_sums(K.to(case.A, gpu_device), case.labels_t(gpu_device), case.k)
    assert sums.dtype == torch.float64 and counts.dtype == torch.int64
    _record("sums", name, K.check_sums(case, sums, counts))
    if case.k >= 3:  # the cluster no row was given
        assert int(counts[case.k - 2]) == 0 and not bool(sums[case.k - 2].any())


@pytest.mark.parametrize("name", ["generic", "wide", "lattice", "generic_f64", "all_empty"])
def test_deterministic_sums_repeat_and_ignore_the_row_order(gpu_device, name):
    case = K.sums_case(name)
    A, labels = K.to(case.A, gpu_device), case.labels_t(gpu_device)
    perm = np.random.default_rng(5).permutation(case.A.shape[0])
    Ap = K.to(K.take_rows(case.A, perm), gpu_device)
    labp = torch.from_numpy(case.labels[perm].copy()).to(gpu_device)
    set_deterministic(True)
    try:
        s1, c1 = ops.csr_cluster_sums(A, labels, case.k)
        s2, c2 = ops.csr_cluster_sums(A, labels, case.k)
        s3, c3 = ops.csr_cluster_sums(Ap, labp, case.k)
    finally:
        set_deterministic(None)
    assert torch.equal(s1, s2) and torch.equal(c1, c2), "two calls differ"
    assert torch.equal(s1, s3) and torch.equal(c1, c3), "a row permutation changed the sums"
    scale = ops.csr_fixed_scale(case.A.shape[0], case.vmax) if case.vmax else 1.0
    _record("sums_fixed", name, K.check_sums(case, s1, c1, fixed_scale=scale))


# ------------------------------------------------------------------------------------------ fit level
def _fit(P, **kw):
    return KMeans(k=K.PLANT_K, seed=K.PLANT_SEED, **kw).fit(DataFrame.from_numpy(P.M))


def _pred(model, frame):
    return np.asarray(model.transform(frame).to_numpy("prediction")).astype(np.int64)


def test_sparse_fit_recovers_the_planted_partition(gpu_device, tmp_path):
    P = K.planted()
    model = _fit(P, enable_sparse_data_optim=True)
    frame = DataFrame.from_numpy(P.M)
    lab = _pred(model, frame)
    assert P.recovers(lab)
    assert P.recovers(_pred(_fit(P), frame))  # the dense route on the same frame and seed
    mean, bound = P.centre_bound(lab)
    err = np.abs(np.asarray(model.cluster_centers_, np.float64) - mean)
    assert (err <= bound).all(), float((err - bound).max())
    _record("fit_centres", "planted", float((err[bound > 0] / bound[bound > 0]).max()))
    model.write().overwrite().save(str(tmp_path / "m"))
    loaded = KMeansModel.load(str(tmp_path / "m"))
    assert np.array_equal(_pred(loaded, frame), lab)
    assert loaded.getOrDefault("enable_sparse_data_optim") is True
    assert model._model_attributes["delta_iters"] == 0 and model._model_attributes["refined_frac"] is None


def test_an_empty_cluster_keeps_its_centre_bit_for_bit(gpu_device, monkeypatch):
    """One of the initial centres attracts no row in any iteration: the fit must return it unchanged
    (not 0 / 0, not zeroed), and the other five must be the means of their rows."""
    C0, res = K.fit_with_an_empty_cluster("cuda:0", monkeypatch)
    C = np.asarray(res["cluster_centers_"], np.float64)
    assert res["n_iter"] >= 2 and np.isfinite(C).all()
    assert np.array_equal(C[5], C0[5])
    assert not np.array_equal(C[:5], C0[:5]) and np.abs(C[:5] - (C0[:5] - 0.01)).max() < 1.0


def test_sparse_fit_repeats_bit_for_bit_in_deterministic_mode(gpu_device):
    P = K.planted()
    set_deterministic(True)
    try:
        a = np.asarray(_fit(P, enable_sparse_data_optim=True, initMode="random", maxIter=4).cluster_centers_)
        b = np.asarray(_fit(P, enable_sparse_data_optim=True, initMode="random", maxIter=4).cluster_centers_)
    finally:
        set_deterministic(None)
    assert np.array_equal(a, b)


def test_random_init_picks_the_same_rows_sparse_and_dense(gpu_device, monkeypatch):
    """One seed, initMode="random": the sparse and the dense fit start from the same rows, and their
    first searches agree on every row the oracle decides for both bands."""
    P = K.planted()
    seen = {}
    real_csr, real_dense = ops.csr_nearest_centroid, ops.nearest_centroid

    def spy_csr(A, C, **kw):
        out = real_csr(A, C, **kw)
        seen.setdefault("csr", (C.detach().cpu().double().numpy(), out[0].cpu().numpy()))
        return out

    def spy_dense(X, C, *a, **kw):
        out = real_dense(X, C, *a, **kw)
        seen.setdefault("dense", (C.detach().cpu().double().numpy(), out[0].cpu().numpy()))
        return out

    monkeypatch.setattr(ops, "csr_nearest_centroid", spy_csr)
    monkeypatch.setattr(ops, "nearest_centroid", spy_dense)
    _fit(P, enable_sparse_data_optim=True, initMode="random", maxIter=1)
    _fit(P, initMode="random", maxIter=1)
    (Cs, ls), (Cd, ld) = seen["csr"], seen["dense"]
    assert np.array_equal(Cs.astype(np.float32), Cd.astype(np.float32))
    decided = K.planted_decided(P, Cs)
    assert decided.mean() > 0.9
    assert np.array_equal(ls[decided], ld[decided])


def test_dense_fit_never_touches_the_csr_ops(gpu_device, monkeypatch):
    for name in ("csr_nearest_centroid", "csr_cluster_sums", "csr_gather_dense"):
        monkeypatch.setattr(ops, name, lambda *a, **kw: pytest.fail("a dense fit called a CSR op"))
    X = np.random.default_rng(0).standard_normal((500, 12)).astype(np.float32)
    model = KMeans(k=3, seed=1).fit(DataFrame.from_numpy(X))
    assert _pred(model, DataFrame.from_numpy(X)).shape == (500,)


def test_two_ranks_sharing_the_device():
    """torchrun, two ranks on cuda:0 (gloo): each rank fits its half of the planted rows; the centres
    lie within the sums bound (two partial sums per cell more) of the fp64 means."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29641", os.path.join(ROOT, "tools", "csr_kmeans_spmd_check.py")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["world"] == 2 and rec["recovers"] and rec["within_bound"], rec
