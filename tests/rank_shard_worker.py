"""One rank of tests/test_gpu_rank_shard.py's multi-process test (started by torch.distributed.run, not collected by pytest):

    python tests/rank_shard_worker.py OUT_DIR

builds the spread pairs (1027, 64, seed 2), takes its shard_bounds shard, calls dist.sharded_ranks (HIP shard sweep, collectives of
whatever backend init_from_env chose) and writes its result to OUT_DIR/ranks_<rank>.npz."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(out_dir):
    import rank_refs as RR
    from vtc_amd import dist as vdist
    rank, local, world = vdist.init_from_env()
    n = 1027
    a, b = RR.spread_pairs(n, 64, 2)
    lo, hi = vdist.shard_bounds(n, rank, world)
    dev = torch.device("cuda", local)
    phases = {}
    ra, rb = vdist.sharded_ranks(torch.from_numpy(a[lo:hi]).to(dev), torch.from_numpy(b[lo:hi]).to(dev), n, rank, world, phases=phases)
    assert ra.device == dev and rb.device == dev and ra.dtype == torch.int64 and rb.dtype == torch.int64
    assert {"allgather_ms", "shard_sweep_ms", "allreduce_ms", "path"} <= set(phases), phases
    np.savez(os.path.join(out_dir, f"ranks_{rank}.npz"), rank_a=ra.cpu().numpy(), rank_b=rb.cpu().numpy(), world=world, lo=lo, hi=hi)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
