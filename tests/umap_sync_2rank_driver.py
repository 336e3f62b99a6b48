"""Two seeded UMAP fits per torchrun rank in deterministic mode (3000 blob rows split over the ranks,
brute-force graph, 40 synchronous epochs with the ranks' summed moves all-reduced), run by
tests/test_umap_sync_2rank.py; rank 0 prints one JSON line: whether the two embeddings are
bit-equal on every rank and whether the ranks hold the same embedding."""
import hashlib
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, COLS = 3000, 16


def main() -> None:
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo")
    from sklearn.datasets import make_blobs

    from spark_rapids_ml_nai_amd import DataFrame, ops
    from spark_rapids_ml_nai_amd.umap import UMAP
    from spark_rapids_ml_nai_amd.utils.determinism import deterministic

    X = make_blobs(ROWS, COLS, centers=8, random_state=0)[0].astype(np.float32)
    b = np.linspace(0, ROWS, world + 1).astype(np.int64)
    calls = []
    sync = ops.umap_epoch_sync

    def counted(*args, **kwargs):
        calls.append(bool(kwargs.get("apply")))
        return sync(*args, **kwargs)

    ops.umap_epoch_sync = counted
    embs = []
    for _ in range(2):
        est = UMAP(n_neighbors=15, n_components=2, n_epochs=40, random_state=3, build_algo="brute_force_knn",
                   featuresCol="features")
        est.num_workers = world
        embs.append(np.asarray(est.fit(DataFrame.from_numpy(X[b[rank]:b[rank + 1]])).embedding_))
    mine = {"equal": bool(np.array_equal(embs[0], embs[1])), "shape": list(embs[0].shape),
            "finite": bool(np.isfinite(embs[0]).all()), "spread": float(np.ptp(embs[0], axis=0).min()),
            "digest": hashlib.sha256(np.ascontiguousarray(embs[0]).tobytes()).hexdigest(),
            # every epoch synchronous, and on several ranks none applied before the all-reduce
            "sync_epochs": len(calls), "applied": int(sum(calls))}
    every = [mine]
    if world > 1:
        every = [None] * world
        dist.all_gather_object(every, mine)
    if rank == 0:
        print(json.dumps({"world": world, "deterministic": deterministic(), "ranks": every}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
