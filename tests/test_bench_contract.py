"""bench.py driver contract: one JSON line with the required keys, single process and SPMD
(torch.distributed.run, 2 gloo ranks on CPU — the same code path as one rank per MI355X)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


def _json_line(out: str) -> dict:
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def _env():
    env = dict(os.environ, SRML_FORCE_CPU="1", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    env["PYTHONPATH"] = ROOT
    return env


def test_bench_single_process(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", "--rows",
                        "3000", "--cols", "12", "--algos", "pca,linear_regression,kmeans", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, env=_env(), cwd="/tmp")
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert KEYS <= set(d)
    assert d["n_gpus"] == 1 and d["steps"] == 1 and d["value"] > 0
    assert {"model", "global_batch", "seq_len", "parallelism"} <= set(d["config"])
    assert not d["config"]["missing_or_failed"]
    # a plain run only fits: the transform pass and the held-out scoring belong to --full
    for w in d["config"]["workloads"].values():
        assert "transform_s" not in w and "quality" not in w
    # --dump-outputs: what each workload's last fit returned, as float32 / float64 .npy files
    arrays = {f: np.load(out / f, allow_pickle=False) for f in os.listdir(out)}
    assert {"pca.components_.npy", "pca.explained_variance_ratio_.npy", "linear_regression.coef_.npy",
            "linear_regression.intercept_.npy", "kmeans.cluster_centers_.npy"} <= set(arrays)
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert arrays["pca.components_.npy"].shape == (3, 12)
    assert arrays["kmeans.cluster_centers_.npy"].shape == (1000, 12)
    assert arrays["linear_regression.coef_.npy"].shape == (12,)


def test_bench_full_adds_transform_and_quality():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "1", "--warmup", "0",
                        "--rows", "3000", "--cols", "12", "--algos", "pca,linear_regression"],
                       capture_output=True, text=True, timeout=600, env=_env(), cwd="/tmp")
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert KEYS <= set(d) and not d["config"]["missing_or_failed"]
    for name, w in d["config"]["workloads"].items():
        assert w["transform_s"] > 0 and w["transform_rows"] == 3000, (name, w)
        assert "error" not in w["quality"], (name, w["quality"])
    assert d["config"]["workloads"]["linear_regression"]["quality"]["r2"] > 0.9


class _FakeForest:
    """The attribute layout of a fitted forest: a list of per-tree dicts of flat node arrays."""

    def __init__(self, n_big):
        rng = np.random.default_rng(3)
        self.attrs = {"big": rng.standard_normal(n_big).astype(np.float32), "n_iter": 7, "dtype": "float32",
                      "phase_s": [0.1, 0.2, 0.3], "none": None,
                      "trees": [{"feature": np.array([1, -1, -1], dtype=np.int32), "threshold": np.array([.5, 0., 0.]),
                                 "depth": 1},
                                {"feature": np.array([-1], dtype=np.int32), "threshold": np.array([0.]), "depth": 0}]}

    def _get_model_attributes(self):
        return self.attrs


def test_dump_outputs_samples_large_arrays_and_respects_budget(tmp_path):
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    n_big = 3 * bench.DUMP_ARRAY_ELEMS + 5
    m = _FakeForest(n_big)
    n1 = bench._dump_outputs(str(tmp_path / "a"), "w", m, bench.DUMP_BYTES)
    n2 = bench._dump_outputs(str(tmp_path / "b"), "w", m, bench.DUMP_BYTES)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["w.big.npy", "w.n_iter.npy", "w.trees.depth.npy", "w.trees.feature.npy", "w.trees.threshold.npy"]
    assert n1 == n2 == sum(os.path.getsize(tmp_path / "a" / f) for f in files)
    big = np.load(tmp_path / "a" / "w.big.npy")
    assert big.dtype == np.float32 and big.shape == (bench.DUMP_ARRAY_ELEMS,)
    assert np.isin(big, m.attrs["big"]).all()
    np.testing.assert_array_equal(big, np.load(tmp_path / "b" / "w.big.npy"))  # the same sample every run
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "w.trees.feature.npy"), np.array([1., -1., -1., -1.]))
    assert np.load(tmp_path / "a" / "w.trees.feature.npy").dtype == np.float64
    assert float(np.load(tmp_path / "a" / "w.n_iter.npy")) == 7.0
    # a nearly spent budget: nothing is written past it
    small = bench._dump_outputs(str(tmp_path / "c"), "w", m, 100_000)
    assert 0 < small <= 100_000
    assert small == sum(os.path.getsize(tmp_path / "c" / f) for f in os.listdir(tmp_path / "c"))


@pytest.mark.dist
def test_bench_spmd_two_ranks():
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29561", os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--steps", "1", "--warmup", "0", "--rows", "3000", "--cols", "12"],
                       capture_output=True, text=True, timeout=900, env=_env(), cwd="/tmp")
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2"
    assert not d["config"]["missing_or_failed"], d["config"]["missing_or_failed"]
    assert len(d["config"]["workloads"]) == 8
