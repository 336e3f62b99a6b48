"""One sparse KMeans fit per torchrun rank on its half of the planted CSR rows of
tests/csr_kmeans_cases.py (k = 6, 4096 columns, ~20 non-zeros per row), run by
tests/test_csr_kmeans_gpu.py with two ranks sharing the device; rank 0 prints one JSON line: whether
the fit recovers the planted partition and whether its centres lie within the cluster-sum bound of
the fp64 means."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> None:
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if torch.cuda.is_available():
        torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo")
    import csr_kmeans_cases as K
    from spark_rapids_ml_nai_amd import DataFrame
    from spark_rapids_ml_nai_amd.clustering import KMeans

    P = K.Planted(0)
    b = np.linspace(0, K.PLANT_M, world + 1).astype(np.int64)
    est = KMeans(k=K.PLANT_K, seed=K.PLANT_SEED, enable_sparse_data_optim=True)
    est.num_workers = world
    model = est.fit(DataFrame.from_numpy(P.M[b[rank]:b[rank + 1]]))
    if rank == 0:
        lab = np.asarray(model.transform(DataFrame.from_numpy(P.M)).to_numpy("prediction")).astype(np.int64)
        ok = bool(P.recovers(lab))
        within = False
        if ok:
            mean, bound = P.centre_bound(lab)
            # each cell is the sum of `world` partial sums: one more rounding per rank
            within = bool((np.abs(np.asarray(model.cluster_centers_, np.float64) - mean)
                           <= bound + world * K.U53 * np.abs(mean)).all())
        print(json.dumps({"world": world, "recovers": ok, "within_bound": within}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
