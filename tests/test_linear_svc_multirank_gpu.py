"""LinearSVC on two ranks sharing the GPU (gloo process group over cuda:0 tensors, launched by
torchrun): each rank evaluates its shard on the fused kernel and the [grad | loss] sums are
all-reduced. Oracle: the one-rank fit on all the rows, through the strong-convexity bound
||theta_a - theta_b|| <= (||grad f(theta_a)|| + ||grad f(theta_b)||) / regParam with both gradients
recomputed in fp64 on the host."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _run(world, port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tools", "linear_svc_spmd_check.py")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_linear_svc_two_ranks_match_one_rank():
    import linear_svc_spmd_check as drv

    X, y = drv.data()
    Xd, s = X.astype(np.float64), 2 * y - 1

    def grad(w):
        h = np.maximum(0.0, 1.0 - s * (Xd @ w))
        return (-2.0 * s * h) @ Xd / len(y) + drv.REG * w

    one, two = _run(1, 29641), _run(2, 29642)
    assert one["world"] == 1 and two["world"] == 2
    assert one["solver"]["path"] == two["solver"]["path"] == "fused_svc_f32"
    wa, wb = np.asarray(one["coef"]), np.asarray(two["coef"])
    bound = (np.linalg.norm(grad(wa)) + np.linalg.norm(grad(wb))) / drv.REG
    assert np.linalg.norm(wa - wb) <= bound, (np.linalg.norm(wa - wb), bound)
    # both fits converged, so the bound is informative (not a large number that anything meets)
    assert one["solver"]["status"] == two["solver"]["status"] == "converged (gradient)", (one["solver"], two["solver"])
