"""Deterministic UMAP on two ranks sharing the GPU (gloo process group, launched by torchrun): the
synchronous epochs all-reduce the ranks' summed moves, so two seeded fits in one launch must give
the same bits on every rank, and the ranks must agree."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_umap_two_ranks_deterministic_fit_repeats():
    env = dict(os.environ, SRML_DETERMINISTIC="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29641",
           os.path.join(ROOT, "tests", "umap_sync_2rank_driver.py")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["world"] == 2 and rec["deterministic"], rec
    ranks = rec["ranks"]
    for rk in ranks:
        assert rk["shape"] == [3000, 2] and rk["finite"] and rk["spread"] > 1.0, rk
        assert rk["sync_epochs"] == 80 and rk["applied"] == 0, rk
        assert rk["equal"], rk
    assert ranks[0]["digest"] == ranks[1]["digest"], ranks
