"""GPU: the rank-sharded counting sweep (vtc_l2_rank_shard -> ops.rank_shard -> dist.sharded_ranks) against the numpy fp64 references of
tests/rank_refs.py and tests/rank_shard_refs.py.  Every comparison is exact integer equality, window by window: rank_a_local is the slice
of the unsharded reference, rank_b_part is partial_b of the window (not only the sum over the windows), on the data the paired sweep's
tests run on (min_gap > 1e-12 checked where the case is built)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import rank_refs as RR
import rank_shard_refs as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(got, want, what):
    bad = np.flatnonzero(got != want)
    assert got.shape == want.shape and bad.size == 0, (what, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def _shard(ta, tb, lo, hi, **kw):
    from vtc_amd import ops
    ra, rb, bits = ops.rank_shard(ta, tb, lo, hi - lo, **kw)
    assert ra.dtype == torch.int64 and rb.dtype == torch.int64 and ra.shape == (hi - lo,) and rb.shape == (ta.shape[0],)
    return ra.cpu().numpy(), rb.cpu().numpy(), int(bits.item())


def _check_cuts(a, b, want_a, cut_lists, want_bits=0, **kw):
    """Every window of every cut list: rank_a_local == the reference's slice, rank_b_part == partial_b, the non-finite word."""
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    D, dt, bad_b = SR.column_direction(a, b)
    for cuts in cut_lists:
        for lo, hi in SR.windows(cuts):
            got_a, got_b, bits = _shard(ta, tb, lo, hi, **kw)
            assert bits == want_bits, (cuts, lo, hi, bits)
            _check(got_a, want_a[lo:hi], f"rank_a_local of [{lo}, {hi}) in {cuts}")
            _check(got_b, SR.partial_from(D, dt, bad_b, lo, hi), f"rank_b_part of [{lo}, {hi}) in {cuts}")


@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_edge_sizes(n):
    """The whole, two ranks, a one-row shard at either end; at 257 with 256-row blocks a window that ends one row before the block edge and
    one that ends on it (its neighbour: one row); an empty window returns all-zero partials."""
    a, b, want_a, want_b = SR.case("spread", n, 64, 10 + n)
    if n >= 65:
        RR.assert_not_degenerate(want_a, n)
        RR.assert_not_degenerate(want_b, n)
    cut_lists = [[0, n], SR.shard_cuts(n, 2)]
    if n >= 2:
        cut_lists += [[0, 1, n], [0, n - 1, n]]
    if n == 257:
        cut_lists += [[0, 255, 257], [0, 256, 257]]
    _check_cuts(a, b, want_a, cut_lists, rows_per_block=256)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got_a, got_b, bits = _shard(ta, tb, n, n, rows_per_block=256)
    assert got_a.shape == (0,) and bits == 0 and not got_b.any()
    got_a, got_b, _ = _shard(ta, tb, 0, 0, rows_per_block=256)
    assert got_a.shape == (0,) and not got_b.any()


@pytest.mark.parametrize("world", [3, 8])
def test_spread_1027_in_256_row_blocks(world):
    """World 3: 343 / 342 / 342 rows, windows of two blocks (256 + 87) that start off the paired sweep's block grid; world 8: 129 / 128."""
    n = 1027
    a, b, want_a, want_b = SR.case("spread", n, 64, 2)
    RR.assert_not_degenerate(want_a, n)
    RR.assert_not_degenerate(want_b, n)
    _check_cuts(a, b, want_a, [SR.shard_cuts(n, world)], rows_per_block=256)


def test_spread_1500_d512_default_blocks():
    n = 1500
    a, b, want_a, want_b = SR.case("spread", n, 512, 1)
    RR.assert_not_degenerate(want_a, n)
    RR.assert_not_degenerate(want_b, n)
    _check_cuts(a, b, want_a, [SR.shard_cuts(n, 5)])


@pytest.mark.parametrize("scale", [1.0, 25.0])
def test_ties_and_clusters_cut_by_the_windows(scale):
    """The cut at 120 runs through the 40 exact duplicates, the cut at 1050 through the dense cluster (everything in reach, fp64 decides):
    bit-equal distances go to the lower GLOBAL row id, whichever window holds the row."""
    n = 1500
    a, b, want_a, want_b = SR.case("cluster", n, 512, 5, scale)
    assert want_a[99:104].tolist() == [0, 1, 2, 3, 4] and want_b[99:104].tolist() == [0, 1, 2, 3, 4]
    assert want_b[1000:1100].max() == 100 and max(want_a.max(), want_b.max()) > n / 2
    _check_cuts(a, b, want_a, [[0, 120, 1050, 1500]])


def test_bf16_midpoint_adversary():
    n = 1024
    a, b, want_a, want_b = SR.case("midpoint", n, 512, 5)
    assert want_a[0] == 0 and want_a.max() > n / 2 and want_b.max() > n / 2
    _check_cuts(a, b, want_a, [SR.shard_cuts(n, 2)])


def test_the_whole_window_is_the_paired_call():
    """row_base = 0, n_local = n: both outputs and the statistics words of ops.rank_bidir, element for element."""
    from vtc_amd import _lib as L
    from vtc_amd import ops
    n, d = 1027, 64
    a, b, want_a, want_b = SR.case("spread", n, d, 2)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    lib = L.lib()
    assert lib.vtc_l2_rank_shard_workspace_bytes(n, n, d, 256, 0) == lib.vtc_l2_rank_bidir_workspace_bytes(n, d, 256, 0)
    assert lib.vtc_l2_rank_shard_workspace_bytes(n, 129, d, 256, 0) < lib.vtc_l2_rank_bidir_workspace_bytes(n, d, 256, 0)
    ws1 = ops.workspace(lib.vtc_l2_rank_bidir_workspace_bytes(n, d, 256, 0), ta.device)
    ws2 = ops.workspace(lib.vtc_l2_rank_shard_workspace_bytes(n, n, d, 256, 0), ta.device)
    pa, pb, pbits = ops.rank_bidir(ta, tb, rows_per_block=256, ws=ws1)
    sa, sb, sbits = ops.rank_shard(ta, tb, 0, n, rows_per_block=256, ws=ws2)
    assert torch.equal(pa, sa) and torch.equal(pb, sb) and int(pbits.item()) == int(sbits.item()) == 0
    _check(sa.cpu().numpy(), want_a, "rank_a")
    _check(sb.cpu().numpy(), want_b, "rank_b")
    # the eight words of the paired sweep (the vunit_* keys are words only rank_grouped_vunit writes: whatever the workspace held)
    st1, st2 = ({k: v for k, v in ops.rank_sweep_stats(ws).items() if not k.startswith("vunit")} for ws in (ws1, ws2))
    assert set(st1) == {"in_reach", "in_reach_max", "brute_force_owners"}
    assert st1 == st2 and min(st1["in_reach"]) > 0, (st1, st2)
    assert ws1[48:64].view(torch.int64).tolist() == ws2[48:64].view(torch.int64).tolist() == [0, 0]      # the two unused words


def _shard_stats(ta, tb, cuts, want_a, D, dt, bad_b, reach_capacity):
    from vtc_amd import _lib as L
    from vtc_amd import ops
    n, d = ta.shape
    out = []
    for lo, hi in SR.windows(cuts):
        ws = ops.workspace(L.lib().vtc_l2_rank_shard_workspace_bytes(n, hi - lo, d, 256, reach_capacity), ta.device)
        got_a, got_b, _ = _shard(ta, tb, lo, hi, rows_per_block=256, reach_capacity=reach_capacity, ws=ws)
        _check(got_a, want_a[lo:hi], f"rank_a_local of [{lo}, {hi})")
        _check(got_b, SR.partial_from(D, dt, bad_b, lo, hi), f"rank_b_part of [{lo}, {hi})")
        out.append(ops.rank_sweep_stats(ws))
    return out


def test_in_reach_pairs_of_the_shards_are_the_paired_calls():
    """The thresholds are the whole matrix's (max |b|^2 over ALL of b), so a shard settles exactly the paired call's pairs that lie in its
    window: the in-reach counts of the shards add up to the paired call's, per direction."""
    from vtc_amd import _lib as L
    from vtc_amd import ops
    n, d = 1027, 64
    a, b, want_a, _ = SR.case("spread", n, d, 2)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ws = ops.workspace(L.lib().vtc_l2_rank_bidir_workspace_bytes(n, d, 256, 0), ta.device)
    ops.rank_bidir(ta, tb, rows_per_block=256, ws=ws)
    paired = ops.rank_sweep_stats(ws)
    shards = _shard_stats(ta, tb, SR.shard_cuts(n, 3), want_a, *SR.column_direction(a, b), 0)
    assert min(paired["in_reach"]) > 0
    assert tuple(sum(s["in_reach"][k] for s in shards) for k in (0, 1)) == paired["in_reach"], (paired, shards)
    assert all(s["brute_force_owners"] == (0, 0) for s in shards), shards
    assert tuple(max(s["in_reach_max"][k] for s in shards) for k in (0, 1))[0] == paired["in_reach_max"][0], (paired, shards)


def test_forced_pool_overflow_changes_nothing():
    """reach_capacity = 8: the owners' pairs miss the pool and the windowed fp64 brute force counts them -- the column direction over the
    window's rows only; the results are the same and every shard did take the path, in both directions."""
    from vtc_amd import ops
    n, d = 1027, 64
    a, b, want_a, _ = SR.case("spread", n, d, 2)
    assert RR.in_reach_total(a, b, ops.rank_kappa(d)) > 8                                    # else the test proves nothing
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    shards = _shard_stats(ta, tb, SR.shard_cuts(n, 3), want_a, *SR.column_direction(a, b), 8)
    for s in shards:
        assert min(s["in_reach"]) > 8 and min(s["brute_force_owners"]) > 0, shards


@pytest.mark.parametrize("world", [2, 3])
def test_nonfinite_rows(world):
    """NaN in a[333], inf in b[700]: the word is 3 on every shard; the window that holds a dead pair's row writes n for it, the others 0;
    its local rank_a is n."""
    n = 1027
    a, b, want_a, want_b = SR.case("nonfinite", n, 64, 2)
    assert want_a[333] == want_a[700] == want_b[333] == want_b[700] == n
    _check_cuts(a, b, want_a, [SR.shard_cuts(n, world)], want_bits=3, rows_per_block=256)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    total = np.zeros(n, np.int64)
    for lo, hi in SR.windows(SR.shard_cuts(n, world)):
        got_a, got_b, _ = _shard(ta, tb, lo, hi, rows_per_block=256)
        for j in (333, 700):
            assert got_b[j] == (n if lo <= j < hi else 0)
            if lo <= j < hi:
                assert got_a[j - lo] == n
        total += got_b
    _check(total, want_b, "the partials' sum")


def test_argument_errors_return_a_status_and_a_message():
    from vtc_amd import _lib as L
    from vtc_amd import ops
    lib = L.lib()
    n, d = 64, 128
    x = torch.zeros(n, d, device="cuda")
    ra = torch.zeros(n, dtype=torch.int64, device="cuda")
    rb = torch.zeros(n, dtype=torch.int64, device="cuda")
    f = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.vtc_l2_rank_shard_workspace_bytes(n, n, d, 0, 0), dtype=torch.uint8, device="cuda")

    def args(base=16, nl=32, d_=d, out=rb.data_ptr(), nbytes=ws.numel()):
        return (x.data_ptr(), x.data_ptr(), n, base, nl, d_, 0, 0, ra.data_ptr(), out, f.data_ptr(), ws.data_ptr(), nbytes, None)
    for bad, msg in ((dict(base=-1), b"row_base=-1"), (dict(base=33, nl=32), b"n_local=32"), (dict(d_=100), b"d=100"),
                     (dict(nbytes=1024), b"workspace too small"), (dict(out=None), b"null argument")):
        assert lib.vtc_l2_rank_shard(*args(**bad)) != 0, bad
        err = lib.vtc_last_error()
        assert msg in err and b"l2_rank_shard" in err, (bad, err)
        assert lib.vtc_l2_rank_shard(*args()) == 0
    torch.cuda.synchronize()
    # all rows equal: every distance ties at 0 and the lower index wins -- rank_a of row i is i, and the window's rows below j are closer to j
    assert ra[:32].cpu().tolist() == list(range(16, 48))
    assert rb.cpu().tolist() == [min(max(j - 16, 0), 32) for j in range(n)]
    with pytest.raises(ValueError, match="row_base=-1"):
        ops.rank_shard(x, x, -1, 4)
    with pytest.raises(ValueError, match="n_local=40"):
        ops.rank_shard(x, x, 30, 40)


def test_three_ranks_on_one_card_return_the_reference_on_every_rank(tmp_path):
    """torch.distributed.run, 3 ranks sharing card 0 over gloo (the layout of tests/test_gpu_eval_entry.py): every rank all-gathers, sweeps
    its 343 / 342 / 342 rows with the HIP shard sweep, all-reduces ONE int64 buffer, and holds the unsharded reference's two arrays."""
    n = 1027
    _, _, want_a, want_b = SR.case("spread", n, 64, 2)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, VTC_LOCAL_DEVICE="0", VTC_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "rank_shard_worker.py"), str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    for rank in range(3):
        got = np.load(tmp_path / f"ranks_{rank}.npz")
        assert int(got["world"]) == 3 and (int(got["lo"]), int(got["hi"])) == SR.windows(SR.shard_cuts(n, 3))[rank]
        _check(got["rank_a"], want_a, f"rank_a on rank {rank}")
        _check(got["rank_b"], want_b, f"rank_b on rank {rank}")


def test_world_one_takes_the_paired_call():
    from vtc_amd import dist as vdist
    n = 257
    a, b, want_a, want_b = SR.case("spread", n, 64, 10 + n)
    ph = {}
    ra, rb = vdist.sharded_ranks(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), n, 0, 1, phases=ph)
    assert ra.is_cuda and "shard_sweep_ms" in ph and "allreduce_ms" not in ph
    _check(ra.cpu().numpy(), want_a, "rank_a")
    _check(rb.cpu().numpy(), want_b, "rank_b")
    bad = a.copy()
    bad[5, 5] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        vdist.sharded_ranks(torch.from_numpy(bad).cuda(), torch.from_numpy(b).cuda(), n, 0, 1)
