"""CPU, world_size 2 and 3, gloo: the sharded-sweep bookkeeping of vtc_amd/dist.py (shard bounds, ragged
all-gather, target offsets, counter all-reduce; the one-GEMM-per-rank path's column-plane exchange with
per-source row bases and padded blocks) against the oracle's unsharded Recall@K and top-k ids.
The searches themselves are injected (oracle CPU stand-ins); on the GPU box the HIP sweep takes their place."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import eval_ref as E


# CPU ranks over gloo.  Where a GPU is present, init_from_env puts each rank on card LOCAL_RANK, which a one-GPU machine lacks
# for rank >= 1: every rank takes card 0 instead, as in the one-card rehearsals (no effect without a GPU).
ONE_CARD = {"VTC_LOCAL_DEVICE": "0"}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cpu_topk(g, q, depth):
    ids, _ = E.l2_topk(g.numpy(), q.numpy(), depth)
    return torch.from_numpy(ids)


def _worker(rank, world, port, n, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), **ONE_CARD)
    from vtc_amd import dist as vdist
    r, _, w = vdist.init_from_env(backend="gloo")
    assert (r, w) == (rank, world)
    rng = np.random.default_rng(0)
    a = rng.standard_normal((n, 32)).astype(np.float32)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = a + 0.7 * rng.standard_normal((n, 32)).astype(np.float32)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    lo, hi = vdist.shard_bounds(n, rank, world)
    r_ab, r_ba = vdist.sharded_recall(torch.from_numpy(a[lo:hi]), torch.from_numpy(b[lo:hi]), n, [1, 5, 10], rank, world,
                                      topk=_cpu_topk)
    if rank == 0:
        ref_ab = dict(E.recall_at_k(a, b, [1, 5, 10]))
        ref_ba = dict(E.recall_at_k(b, a, [1, 5, 10]))
        out.put((r_ab == ref_ab, r_ba == ref_ba, r_ab, ref_ab))
    dist.destroy_process_group()


RB = 8      # row block of the stand-ins (the HIP epilogue: 128)


def _shard_ops():
    from oracle import sweep_planes as SP
    stats = {}

    def rows_fn(a_all, b_loc, depth, nbp):
        ids, planes = SP.shard_rows(a_all.numpy(), b_loc.numpy(), depth, nbp, RB)
        return torch.from_numpy(ids), torch.from_numpy(planes)

    def cols_fn(b_all, a_loc, depth, planes, src_base):
        return torch.from_numpy(SP.shard_cols(b_all.numpy(), a_loc.numpy(), depth, planes.numpy(), src_base.numpy(), RB, stats))
    return (rows_fn, cols_fn, RB), stats


def _worker_one_matrix(rank, world, port, n, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), **ONE_CARD)
    from vtc_amd import dist as vdist
    vdist.init_from_env(backend="gloo")
    rng = np.random.default_rng(0)
    a = rng.standard_normal((n, 32)).astype(np.float32)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = a + 0.7 * rng.standard_normal((n, 32)).astype(np.float32)
    b[: n // 2] /= np.linalg.norm(b[: n // 2], axis=1, keepdims=True)       # second half left un-normalised
    lo, hi = vdist.shard_bounds(n, rank, world)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    ops3, stats = _shard_ops()
    r_ab, r_ba = vdist.sharded_recall(ta[lo:hi], tb[lo:hi], n, [1, 5, 10], rank, world, shard_ops=ops3)
    # the exchange by hand: ids of this rank's columns against the unsharded search
    depth = 11
    bounds = [vdist.shard_bounds(n, r, world) for r in range(world)]
    nbp = -(-max(h - l for l, h in bounds) // RB)
    i1, planes = ops3[0](ta, tb[lo:hi], depth, nbp)
    recv = vdist.exchange_column_planes(planes, n, rank, world)
    assert recv.shape == (world, 4, nbp, hi - lo)
    i2 = ops3[1](tb, ta[lo:hi], depth, recv, torch.tensor([l for l, _ in bounds], dtype=torch.int32))
    ok_ids = torch.equal(i2, _cpu_topk(tb, ta[lo:hi], depth)) and torch.equal(i1, _cpu_topk(ta, tb[lo:hi], depth))
    flags = torch.tensor([int(ok_ids), stats.get("brute", 0), hi - lo])
    allf = [torch.zeros_like(flags) for _ in range(world)]
    dist.all_gather(allf, flags)
    if rank == 0:
        ref_ab = dict(E.recall_at_k(a, b, [1, 5, 10]))
        ref_ba = dict(E.recall_at_k(b, a, [1, 5, 10]))
        out.put((r_ab == ref_ab and r_ba == ref_ba, all(int(f[0]) for f in allf), sum(int(f[1]) for f in allf), (r_ab, ref_ab, r_ba, ref_ba)))
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(3, 601), (2, 400), (3, 101), (8, 1003)])       # ragged shards, padded blocks (601 = 201 + 200 + 200 rows); 8 ranks = the node the sweep is specified for (1003 = 3 x 126 + 5 x 125)
def test_one_matrix_sharded_sweep_exchange(world, n):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_one_matrix, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    ok_recall, ok_ids, brute, detail = q.get(timeout=180)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert ok_recall, detail
    assert ok_ids
    if n >= 400:                   # enough blocks for the certificate to hold: the exchanged planes are what was searched
        assert brute < n // 2


def _rank_ops():
    """CPU stand-ins for ops.recall_shard_rows / ops.recall_shard_cols (the recall-only finish of the sharded sweep: hit counters, no ids):
    the oracle's planes; the row direction counted from the oracle's fp64 ranks, the column direction FROM THE EXCHANGED PLANES."""
    from oracle import sweep_planes as SP
    stats = {}

    def rows_fn(a_all, b_loc, base, ks, nbp, hits):
        ids, planes = SP.shard_rows(a_all.numpy(), b_loc.numpy(), max(ks) + 1, nbp, RB)
        tgt = np.arange(base, base + b_loc.shape[0])[:, None]
        for j, k in enumerate(ks):
            hits[j] += int((ids[:, :k] == tgt).any(axis=1).sum())
        return torch.from_numpy(planes)

    def cols_fn(b_all, a_loc, base, ks, planes, src_bounds, hits):
        sb = src_bounds.numpy()
        assert sb[-1] == b_all.shape[0] and len(sb) == planes.shape[0] + 1
        ids = SP.shard_cols(b_all.numpy(), a_loc.numpy(), max(ks) + 1, planes.numpy(), sb[:-1].copy(), RB, stats)
        tgt = np.arange(base, base + a_loc.shape[0])[:, None]
        for j, k in enumerate(ks):
            hits[j] += int((ids[:, :k] == tgt).any(axis=1).sum())
    return (rows_fn, cols_fn, RB)


def _worker_rank_sharded(rank, world, port, n, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), **ONE_CARD)
    from vtc_amd import dist as vdist
    vdist.init_from_env(backend="gloo")
    rng = np.random.default_rng(1)
    a = rng.standard_normal((n, 32)).astype(np.float32)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = a + 0.7 * rng.standard_normal((n, 32)).astype(np.float32)
    b[: n // 2] /= np.linalg.norm(b[: n // 2], axis=1, keepdims=True)
    lo, hi = vdist.shard_bounds(n, rank, world)
    ph = {}
    r_ab, r_ba = vdist.sharded_recall(torch.from_numpy(a[lo:hi]), torch.from_numpy(b[lo:hi]), n, [1, 5, 10], rank, world, rank_ops=_rank_ops(), phases=ph)
    if rank == 0:
        ref_ab = dict(E.recall_at_k(a, b, [1, 5, 10]))
        ref_ba = dict(E.recall_at_k(b, a, [1, 5, 10]))
        out.put((r_ab == ref_ab and r_ba == ref_ba, ph.get("path"), (r_ab, ref_ab, r_ba, ref_ba)))
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(2, 400), (3, 601)])
def test_rank_sharded_sweep_over_gloo(world, n):
    """sharded_recall's recall-only branch for world > 1 (rows: counters with the GEMM; all-to-all of the column planes with the
    [n_src + 1] source bounds; columns: counters from the exchanged planes; all-reduce of the 2 x nk counters) == the unsharded oracle."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_rank_sharded, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    ok, path, detail = q.get(timeout=180)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert ok, detail
    assert path == "injected rank ops"


@pytest.mark.parametrize("n", [64, 101])          # even and ragged shards
def test_sharded_recall_world2(n):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n, q)) for r in range(2)]
    for p in procs:
        p.start()
    ok_ab, ok_ba, got, ref = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert ok_ab and ok_ba, (got, ref)


def test_shard_bounds_cover_everything():
    from vtc_amd.dist import shard_bounds
    for n in (1, 7, 8, 10000, 50001):
        for w in (1, 2, 3, 8):
            b = [shard_bounds(n, r, w) for r in range(w)]
            assert b[0][0] == 0 and b[-1][1] == n
            assert all(b[i][1] == b[i + 1][0] for i in range(w - 1))
            assert max(h - l for l, h in b) - min(h - l for l, h in b) <= 1


def test_bench_gpus_n_launches_its_own_ranks():
    """`python bench.py --gpus N` with no WORLD_SIZE in the environment must start its N ranks itself (a child
    torch.distributed.run, 127.0.0.1 rendezvous) and relay rank 0's JSON line -- never print n_gpus: 1 for --gpus 2.  Here on
    the CPU: gloo backend, and VTC_BENCH_RENDEZVOUS_ONLY=1 stops the ranks after the rendezvous + one all-reduce, before
    anything needs the card."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(VTC_DIST_BACKEND="gloo", VTC_BENCH_RENDEZVOUS_ONLY="1", **ONE_CARD)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["backend"] == "gloo" and j["allreduce_check"] == 2.0
    # a mismatch between --gpus and the launcher's world size is refused, not silently reported as the smaller job
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], env=env2, capture_output=True, text=True, timeout=300)
    assert r2.returncode != 0 and "refusing" in (r2.stderr + r2.stdout)


def test_ranks_sharing_a_card_select_the_multi_launch_cam(monkeypatch):
    """Several ranks on ONE device -- however they got there (VTC_LOCAL_DEVICE rehearsals, LOCAL_RANK modulo the device count, a narrowed
    HIP_VISIBLE_DEVICES): the one-launch CAM's grid barrier cannot be resident next to other processes' kernels (5-rank rehearsal:
    time-out, NaN), so vtc_amd/dist.py detects shared cards from the gathered (host, card id) pairs and sets the per-model
    VTC_CAM_NO_FUSED flag (no environment variable a library static may already have read) -- and leaves the production
    layout (one process per GPU) alone."""
    from vtc_amd import _lib as L
    from vtc_amd import dist as vdist
    from vtc_amd import towers
    monkeypatch.setattr(towers, "_CAM_SHARED_CARD", False)
    monkeypatch.setattr(vdist, "card_identity", lambda local: ("hostA", "GPU-1"))
    assert vdist.mark_shared_cards(0, identities=[("hostA", "GPU-1"), ("hostA", "GPU-2"), ("hostB", "GPU-1")]) is False
    assert towers._CAM_SHARED_CARD is False
    assert vdist.mark_shared_cards(0, identities=[("hostA", "GPU-1"), ("hostA", "GPU-2"), ("hostA", "GPU-1")]) is True
    assert towers._CAM_SHARED_CARD is True
    # the flag reaches a module that was packed BEFORE the process group existed: it is applied per forward
    class _W:
        flags = 0
    w = _W()
    if towers._CAM_SHARED_CARD:
        w.flags |= L.CAM_NO_FUSED
    assert w.flags & L.CAM_NO_FUSED
    towers.set_cam_shared_card(False)


def _shared_card_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), **ONE_CARD)
    from vtc_amd import dist as vdist
    from vtc_amd import towers
    # ranks 0 and 2 claim the same card, rank 1 another
    vdist.card_identity = lambda local: ("box", "GPU-A" if rank != 1 else "GPU-B")
    vdist.init_from_env(backend="gloo")
    out.put((rank, towers._CAM_SHARED_CARD))
    dist.destroy_process_group()


def test_shared_card_detection_over_gloo_world_3():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_shared_card_worker, args=(r, 3, port, q)) for r in range(3)]
    for p_ in ps:
        p_.start()
    got = dict(q.get(timeout=120) for _ in range(3))
    for p_ in ps:
        p_.join(60)
    assert got == {0: True, 1: False, 2: True}


def test_single_rank_path_of_sharded_recall_is_the_plain_recall():
    """the N = 1 line of a scaling run (`bench.py --gpus 1` -> sharded_recall(world=1)) must be the same computation as
    the single-GPU headline's (RecallAtK.compute_both): no collective, whole-matrix shard bounds, target offset 0, the reference's
    denominators.  CPU half of the check (the injected top-k is the oracle's); the GPU half -- the HIP sweep on both sides -- is
    tests/test_gpu_sweep.py::test_sharded_recall_world_1_equals_recallatk_compute_both."""
    from vtc_amd import dist as vdist
    rng = np.random.default_rng(4)
    n = 300
    a = rng.standard_normal((n, 32)).astype(np.float32)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = a + 0.7 * rng.standard_normal((n, 32)).astype(np.float32)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    assert vdist.shard_bounds(n, 0, 1) == (0, n)
    ph = {}
    r_ab, r_ba = vdist.sharded_recall(torch.from_numpy(a), torch.from_numpy(b), n, [1, 5, 10], 0, 1, topk=_cpu_topk, phases=ph)
    assert r_ab == dict(E.recall_at_k(a, b, [1, 5, 10])) and r_ba == dict(E.recall_at_k(b, a, [1, 5, 10]))
    assert vdist.sweep_path(n, 3, 1).startswith("two searches") and vdist.sweep_path(10000, 3, 1).startswith("one distance matrix")
    assert vdist.choose_sweep_path(10000, 512, 3, 1) not in (vdist.SweepPath.ONE_MATRIX_SHARDED, vdist.SweepPath.RANK_SHARDED)


def _worker_nonfinite(rank, world, port, n, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), **ONE_CARD)
    from vtc_amd import dist as vdist
    vdist.init_from_env(backend="gloo")
    rng = np.random.default_rng(1)
    a = rng.standard_normal((n, 32)).astype(np.float32)
    b = rng.standard_normal((n, 32)).astype(np.float32)
    lo, hi = vdist.shard_bounds(n, rank, world)
    if lo <= n - 2 < hi:
        b[n - 2, 5] = np.nan               # ONE bad row, on the last rank only
    try:
        vdist.sharded_recall(torch.from_numpy(a[lo:hi]), torch.from_numpy(b[lo:hi]), n, [1, 5, 10], rank, world, topk=_cpu_topk)
        out.put((rank, "returned"))
    except ValueError as e:
        out.put((rank, "raised" if "non-finite" in str(e) else str(e)))
    dist.destroy_process_group()


def test_a_nonfinite_row_on_one_rank_raises_on_every_rank():
    """ADVICE r5 (medium) / VERDICT r5 #2: NaN embeddings never reach a recall figure.  The flag word rides behind the hit counters through
    their all-reduce, so the rank that holds the bad row and the ranks that do not all raise -- nobody is left waiting in a collective."""
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    world, port = 3, _free_port()
    procs = [ctx.Process(target=_worker_nonfinite, args=(r, world, port, 90, out)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(out.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    assert got == [(0, "raised"), (1, "raised"), (2, "raised")], got
