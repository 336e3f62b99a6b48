"""One LinearSVC fit per torchrun rank on its shard of a fixed dataset (3000 x 64, squared hinge,
regParam 0.1, no intercept), run by tests/test_linear_svc_multirank_gpu.py with one and two ranks
sharing the GPU; rank 0 prints the model (coefficients, objective, solver info) as one JSON line."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, COLS, REG, NOISE = 3000, 64, 0.1, 2.0


def data():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((ROWS, COLS))
    wt = rng.standard_normal(COLS)
    y = (X @ wt + NOISE * rng.standard_normal(ROWS) > 0).astype(np.float64)
    return X.astype(np.float32), y


def main() -> None:
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo")
    X, y = data()
    b = np.linspace(0, ROWS, world + 1).astype(np.int64)
    from spark_rapids_ml_nai_amd import DataFrame
    from spark_rapids_ml_nai_amd.classification import LinearSVC

    est = LinearSVC(regParam=REG, fitIntercept=False, standardization=False, loss="squared_hinge", tol=1e-6)
    est.num_workers = world
    model = est.fit(DataFrame.from_numpy(X[b[rank]:b[rank + 1]], y[b[rank]:b[rank + 1]]))
    if rank == 0:
        print(json.dumps({"world": world, "coef": [float(c) for c in model.coef_], "objective": model.objective,
                          "solver": model._solver_info}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
