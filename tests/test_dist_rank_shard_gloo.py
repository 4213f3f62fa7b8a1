"""CPU, world_size 2 and 3, gloo: the bookkeeping of dist.sharded_ranks (ragged all-gather, the shard's window, ONE all-reduce of
[rank_a slices | partial rank_b | non-finite word]) against the unsharded fp64 reference of tests/rank_refs.py.  The shard sweep itself is
injected: a numpy stand-in for ops.rank_shard built on tests/rank_shard_refs.py::partial_b; on the GPU the HIP sweep takes its place
(tests/test_gpu_rank_shard.py)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import rank_refs as RR
import rank_shard_refs as SR

ONE_CARD = {"VTC_LOCAL_DEVICE": "0"}      # as tests/test_dist_gloo.py: every rank takes card 0 where a GPU is present


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _numpy_shard_op(a_all, b_all, row_base, n_local):
    """ops.rank_shard's contract in numpy fp64: the reference's rank_a over the window, partial_b, the non-finite word of both whole sets."""
    a, b = a_all.numpy(), b_all.numpy()
    rank_a, _, _ = RR.reference_ranks(a, b)
    bits = int(not np.isfinite(a).all()) | 2 * int(not np.isfinite(b).all())
    return (torch.from_numpy(rank_a[row_base:row_base + n_local].copy()), torch.from_numpy(SR.partial_b(a, b, row_base, row_base + n_local)),
            torch.tensor([bits], dtype=torch.int32))


def _worker(rank, world, port, n, poison, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), **ONE_CARD)
    from vtc_amd import dist as vdist
    r, _, w = vdist.init_from_env(backend="gloo")
    assert (r, w) == (rank, world)
    a, b = (x.copy() for x in RR.spread_pairs(n, 64, 2 if n == 1027 else 10 + n))
    if poison:
        a[n - 1, 3] = np.nan                                  # a row of the LAST rank's shard
    lo, hi = vdist.shard_bounds(n, rank, world)
    ta, tb = torch.from_numpy(a[lo:hi]), torch.from_numpy(b[lo:hi])
    ph = {}
    try:
        ra, rb = vdist.sharded_ranks(ta, tb, n, rank, world, shard_op=_numpy_shard_op, phases=ph)
    except ValueError as e:
        out.put((rank, "ValueError", str(e)))
    else:
        want_a, want_b, _ = RR.reference_ranks(a, b)
        ok = (ra.dtype == torch.int64 and rb.dtype == torch.int64 and ra.shape == rb.shape == (n,)
              and np.array_equal(ra.numpy(), want_a) and np.array_equal(rb.numpy(), want_b))
        st = vdist.sharded_rank_stats(ta, tb, n, rank, world, k_vals=(1, 5, 50), shard_op=_numpy_shard_op)
        from vtc_amd.host.metric import rank_statistics
        ok_st = st == (rank_statistics(want_a, (1, 5, 50)), rank_statistics(want_b, (1, 5, 50)))
        out.put((rank, ok and ok_st, ph.get("path")))
    dist.destroy_process_group()


def _run(world, n, poison):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, poison, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert [g[0] for g in got] == list(range(world))
    return got


@pytest.mark.parametrize("world,n", [(2, 65), (3, 65), (2, 1027), (3, 1027)])      # ragged shards: 33 + 32, 22 + 22 + 21, 514 + 513, 343 + 342 + 342
def test_sharded_ranks_over_gloo_equal_the_unsharded_reference(world, n):
    """Every rank returns the reference's two rank arrays, and sharded_rank_stats their rank_statistics."""
    for rank, ok, path in _run(world, n, poison=False):
        assert ok is True, (rank, ok, path)
        assert path == "injected shard op"


@pytest.mark.parametrize("world", [2, 3])
def test_a_nan_row_on_one_rank_raises_on_every_rank(world):
    for rank, what, msg in _run(world, 65, poison=True):
        assert what == "ValueError" and "non-finite" in msg and "sharded_ranks" in msg, (rank, what, msg)
