"""GPU: the full-rank sweep (vtc_l2_rank_bidir -> ops.rank_bidir -> RecallAtK.ranks -> eval.py --rank-stats) against the numpy fp64
reference of tests/rank_refs.py.  Ranks are compared with array_equal in both directions: the sweep is exact.  Every comparison first
checks its own data: the smallest relative gap between a target's distance and any other (not bit-equal) distance exceeds 1e-12, so no
summation order decides a rank, and the ranks are not degenerate (on the spread data: they reach past n / 2 and 0.2 < R@1 < 0.8)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import rank_refs as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _case(kind, n, d, seed, scale=1.0):
    """(a, b, rank_a, rank_b) of a named data set: generated and referenced once, shared by the tests, never modified."""
    if kind == "spread":
        a, b = RR.spread_pairs(n, d, seed)
    elif kind == "unrelated":
        a, b = RR.unrelated_pairs(n, d, seed)
    elif kind == "cluster":
        a, b = RR.cluster_case(n, d, seed, scale)
    else:
        a, b = RR.midpoint_adversary(n, d, seed)
    rank_a, rank_b, gap = RR.reference_ranks(a, b)
    assert gap > 1e-12, gap
    for x in (a, b, rank_a, rank_b):
        x.setflags(write=False)
    return a, b, rank_a, rank_b


def _sweep(a, b, **kw):
    from vtc_amd import ops
    ra, rb, bits = ops.rank_bidir(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), **kw)
    assert ra.dtype == torch.int64 and rb.dtype == torch.int64 and ra.shape == rb.shape == (a.shape[0],)
    return ra.cpu().numpy(), rb.cpu().numpy(), int(bits.item())


def _check(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_edge_sizes(n):
    """One row, two rows, one short of / exactly / one past a 64-column strip, and 257 with 256-row blocks: a second block of ONE row, whose
    column counts are carried over from the first.  n % 4 != 0: the rows of the matrix are padded to 16 bytes, the row pass ends in its scalar
    tail and the column pass meets 3 / 2 / 1 / 3 / 3 padding columns (n = 1 .. 257), which it must neither count nor pool."""
    a, b, want_a, want_b = _case("spread", n, 64, 10 + n)
    if n >= 63:
        RR.assert_not_degenerate(want_a, n)
        RR.assert_not_degenerate(want_b, n)
    got_a, got_b, bits = _sweep(a, b, rows_per_block=256)
    assert bits == 0
    _check(got_a, want_a, "rank_a")
    _check(got_b, want_b, "rank_b")


@pytest.mark.parametrize("n,d,seed,rpb", [(1027, 64, 2, 256), (700, 128, 3, 0), (1500, 512, 1, 0), (600, 768, 4, 0)])
def test_spread_data_equals_the_fp64_reference(n, d, seed, rpb):
    """(1027, 64) in five blocks of 256 rows (rows padded to 1028 columns: scalar tail in the row pass, one padding column in the column pass);
    no padding at 700 / 1500 / 600 rows in one block; d = 64 .. 768."""
    a, b, want_a, want_b = _case("spread", n, d, seed)
    RR.assert_not_degenerate(want_a, n)
    RR.assert_not_degenerate(want_b, n)
    got_a, got_b, bits = _sweep(a, b, rows_per_block=rpb)
    assert bits == 0
    _check(got_a, want_a, "rank_a")
    _check(got_b, want_b, "rank_b")


def test_metric_ranks_pad_d_500():
    """RecallAtK.ranks zero-pads d = 500 to 512 (distances unchanged) and returns int64 ranks on the GPU; rank_result() names them."""
    from vtc_amd.host.metric import RecallAtK, rank_statistics
    n = 900
    a, b, want_a, want_b = _case("spread", n, 500, 6)
    RR.assert_not_degenerate(want_a, n)
    m = RecallAtK("videos", "titles", [1, 5, 10])
    ra, rb = m.ranks(a, b)
    assert ra.is_cuda and rb.is_cuda and ra.dtype == torch.int64
    _check(ra.cpu().numpy(), want_a, "rank_a")
    _check(rb.cpu().numpy(), want_b, "rank_b")
    m.update(None, (torch.from_numpy(a[:500]).cuda(), torch.from_numpy(b[:500]).cuda()), None)
    m.update(None, (torch.from_numpy(a[500:]).cuda(), torch.from_numpy(b[500:]).cuda()), None)
    res = m.rank_result()
    assert set(res) == {f"{p}-{k}" for p in ("titles_from_videos", "videos_from_titles") for k in ("median_rank", "mean_rank", "mrr")}
    sa, sb = rank_statistics(want_a, ()), rank_statistics(want_b, ())
    assert res["titles_from_videos-median_rank"] == sa["median_rank"] and res["videos_from_titles-mrr"] == sb["mrr"]
    assert res["titles_from_videos-mean_rank"] == sa["mean_rank"]


def test_unrelated_sets():
    """b independent of a: ranks roughly uniform over [0, n), nearly every target deep inside the bulk of its row's distances.  By
    construction R@1 is ~0 here, so the spread data's 0.2 < R@1 < 0.8 window does not apply: the condition is max rank > n / 2 and a median
    rank in the middle half."""
    n = 1027
    a, b, want_a, want_b = _case("unrelated", n, 64, 8)
    assert want_a.max() > n / 2 and n / 4 < np.median(want_a) < 3 * n / 4 and n / 4 < np.median(want_b) < 3 * n / 4
    got_a, got_b, _ = _sweep(a, b, rows_per_block=256)
    _check(got_a, want_a, "rank_a")
    _check(got_b, want_b, "rank_b")


@pytest.mark.parametrize("scale", [1.0, 25.0])
def test_ties_duplicates_and_clusters(scale):
    """40 exact duplicates of one pair on both sides (bit-equal distances: the lower index wins, so the copies' ranks count up), a dense
    cluster of 100 rows within 1e-7 of a target (everything in reach: fp64 decides all of it), un-normalised rows at scale 25 (the bound
    scales with the norms).  Not degenerate means here: the duplicates' and the cluster's ranks are the ones the construction dictates and
    some rank exceeds n / 2 (R@1 is 0.50 on this data; the window is not asserted because the planted rows, not the spread, are the point)."""
    n = 1500
    a, b, want_a, want_b = _case("cluster", n, 512, 5, scale)
    assert want_a[99:104].tolist() == [0, 1, 2, 3, 4] and want_b[99:104].tolist() == [0, 1, 2, 3, 4]     # the duplicates' ties
    assert want_b[1000:1100].max() == 100 and max(want_a.max(), want_b.max()) > n / 2
    got_a, got_b, bits = _sweep(a, b)
    assert bits == 0
    _check(got_a, want_a, "rank_a")
    _check(got_b, want_b, "rank_b")


def test_bf16_midpoint_adversary():
    """oracle.sweep_planes.midpoint_case in 1024 rows: operands whose bf16 roundings are coordinated to the worst case.  No entry may be
    counted or dropped as certain that is not: pair 0's target is its true nearest row.  800 of the 1 024 pairs are b_i == a_i, so R@1 is
    0.8 - 0.9 by construction and the spread data's R@1 window does not apply: the condition is rank 0 for pair 0 and max rank > n / 2 in
    both directions."""
    n = 1024
    a, b, want_a, want_b = _case("midpoint", n, 512, 5)
    assert want_a[0] == 0 and want_a.max() > n / 2 and want_b.max() > n / 2
    got_a, got_b, _ = _sweep(a, b)
    _check(got_a, want_a, "rank_a")
    _check(got_b, want_b, "rank_b")


def test_forced_pool_overflow_changes_nothing():
    """reach_capacity = 8: almost every owner's pairs miss the pool and go to the fp64 brute force; the ranks are the same."""
    from vtc_amd import _lib as L
    from vtc_amd import ops
    n, d = 1027, 64
    a, b, want_a, want_b = _case("spread", n, d, 2)
    kappa = ops.rank_kappa(d)
    assert kappa == pytest.approx(3.0 / 65536 + 4.0 * d / 16777216 + 1e-6, rel=1e-6)         # vtc_amd/csrc/sweep_front.hip, split_kappa
    assert RR.in_reach_total(a, b, kappa) > 8                                                # else the test proves nothing
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ws = ops.workspace(L.lib().vtc_l2_rank_bidir_workspace_bytes(n, d, 256, 8), ta.device)
    ra, rb, _ = ops.rank_bidir(ta, tb, rows_per_block=256, reach_capacity=8, ws=ws)
    _check(ra.cpu().numpy(), want_a, "rank_a")
    _check(rb.cpu().numpy(), want_b, "rank_b")
    st = ops.rank_sweep_stats(ws)
    assert min(st["in_reach"]) > 8 and min(st["brute_force_owners"]) > 0, st                # the path did run
    ws2 = ops.workspace(L.lib().vtc_l2_rank_bidir_workspace_bytes(n, d, 256, 0), ta.device)
    ops.rank_bidir(ta, tb, rows_per_block=256, ws=ws2)
    st2 = ops.rank_sweep_stats(ws2)
    assert st2["brute_force_owners"] == (0, 0) and st2["in_reach"] == st["in_reach"], (st, st2)


@pytest.mark.parametrize("n,d,seed", [(1027, 64, 2), (2500, 512, 7)])
def test_counts_equal_the_shipped_recall_counters(n, d, seed):
    """#{ rank < k } == vtc_l2_recall_bidir's counters, and vtc_l2_topk_bidir(EXACT) + vtc_recall_hits_pair's, bit for bit."""
    from vtc_amd import _lib as L
    from vtc_amd import ops
    a, b = RR.spread_pairs(n, d, seed)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ra, rb, bits = ops.rank_bidir(ta, tb)
    assert int(bits.item()) == 0
    ra, rb = ra.cpu().numpy(), rb.cpu().numpy()
    RR.assert_not_degenerate(ra, n)
    for ks in ([1, 5, 10], [1], [3, 7, 20, 50]):
        mine = np.array([[(ra < k).sum() for k in ks], [(rb < k).sum() for k in ks]])
        hits = ops.recall_bidir(ta, tb, ks).cpu().numpy()
        assert np.array_equal(mine, hits), (ks, mine.tolist(), hits.tolist())
        depth = max(ks) + 1
        ids_b2a, _, ids_a2b, _ = ops.l2_topk_bidir(ta, tb, depth, precision=L.SWEEP_EXACT, return_dists=False)
        pair = torch.zeros(2, len(ks), dtype=torch.int64, device="cuda")
        ops.recall_hits_pair(ids_b2a, ids_a2b, ks, 0, pair)
        assert np.array_equal(mine, pair.cpu().numpy()), (ks, mine.tolist(), pair.cpu().numpy().tolist())


def test_nonfinite_rows():
    """NaN in one row of a, inf in one row of b: the word says which side; those pairs have rank n in both directions (their own distance
    is not finite); every other rank is the reference's with those gallery rows never closer; RecallAtK.ranks raises."""
    from vtc_amd.host.metric import RecallAtK
    n, d, p, q = 1027, 64, 333, 700
    a, b = (x.copy() for x in RR.spread_pairs(n, d, 2))
    a[p, 5] = np.nan
    b[q, 17] = np.inf
    want_a, want_b, gap = RR.reference_ranks(a, b)
    assert gap > 1e-12 and want_a[p] == want_a[q] == want_b[p] == want_b[q] == n
    got_a, got_b, bits = _sweep(a, b, rows_per_block=256)
    assert bits == 3
    _check(got_a, want_a, "rank_a")
    _check(got_b, want_b, "rank_b")
    # the rank-n rule is the shipped counters' rule: #{ rank < k } == vtc_l2_recall_bidir's counters on these inputs too (marker bit taken off)
    from vtc_amd import ops
    ks = [1, 5, 10]
    hits, bad = ops.split_recall_counters(ops.recall_bidir(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), ks).cpu())
    assert bad
    mine = np.array([[(got_a < k).sum() for k in ks], [(got_b < k).sum() for k in ks]])
    assert np.array_equal(mine, hits.numpy()), (mine.tolist(), hits.numpy().tolist())
    clean = a.copy()
    clean[p, 5] = 0.0
    assert _sweep(clean, b)[2] == 2 and _sweep(a, np.where(np.isfinite(b), b, 0).astype(np.float32))[2] == 1
    m = RecallAtK("videos", "titles", [1, 5, 10])
    with pytest.raises(ValueError, match="non-finite"):
        m.ranks(a, b)
    m.check_finite = False
    _check(m.ranks(a, b)[0].cpu().numpy(), want_a, "rank_a (check_finite off)")


def test_argument_errors_return_a_status_and_a_message():
    from vtc_amd import _lib as L
    lib = L.lib()
    n = 64
    x = torch.zeros(n, 128, device="cuda")
    r = torch.zeros(n, dtype=torch.int64, device="cuda")
    f = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.vtc_l2_rank_bidir_workspace_bytes(n, 128, 0, 0), dtype=torch.uint8, device="cuda")
    args = lambda d=128, ra=r.data_ptr(), nbytes=ws.numel(): (x.data_ptr(), x.data_ptr(), n, d, 0, 0, ra, r.data_ptr(), f.data_ptr(),   # noqa: E731
                                                              ws.data_ptr(), nbytes, None)
    assert lib.vtc_l2_rank_bidir(*args(d=100)) != 0 and b"d=100" in lib.vtc_last_error()
    assert lib.vtc_l2_rank_bidir(*args(nbytes=1024)) != 0 and b"workspace too small" in lib.vtc_last_error()
    assert lib.vtc_l2_rank_bidir(*args(ra=None)) != 0 and b"null argument" in lib.vtc_last_error()
    assert lib.vtc_l2_rank_bidir(*args()) == 0
    torch.cuda.synchronize()
    assert r.cpu().tolist() == list(range(n))     # all rows equal: every distance ties at 0 and the lower index wins, so rank i = i


def test_eval_entry_rank_stats_and_the_rank_table(tmp_path):
    """eval.py --rank-stats: the six reference keys are those of the run without the flag, the new keys are rank_statistics of the reference
    ranks of the embeddings the run returns; compute_rank_table's R@K rows are compute_recall's."""
    from vtc_amd.host import eval as ev
    from vtc_amd.host import retrieval_evaluation as RE
    from vtc_amd.host.metric import rank_statistics
    cfg = os.path.join(ROOT, "configs", "synthetic", "pretrained_clip.jsonc")
    outs = []
    for extra in ([], ["--rank-stats"]):
        torch.manual_seed(1023)
        path = tmp_path / f"res{len(extra)}.json"
        out, fv, ft = ev.cli(["-c", cfg, "--bs", "16", "--n_pairs", "48", "--out", str(path)] + extra)
        assert json.load(open(path)) == out
        outs.append(out)
    plain, full = outs
    assert not any(k.startswith(("MedR", "MeanR", "MRR")) for k in plain)
    assert {k: v for k, v in full.items() if k in plain} == plain
    want_a, want_b, gap = RR.reference_ranks(fv.cpu().numpy(), ft.cpu().numpy())
    assert gap > 1e-12
    for name, r in (("title_from_im", want_a), ("im_from_title", want_b)):
        st = rank_statistics(r, ())
        assert (full[f"MedR_{name}"], full[f"MeanR_{name}"], full[f"MRR_{name}"]) == (st["median_rank"], st["mean_rank"], st["mrr"])
    a, b, _, _ = _case("spread", 700, 128, 3)
    table, recall = RE.compute_rank_table(a, b, "full-test", "MSRVTT"), RE.compute_recall(a, b, "full-test", "MSRVTT")
    assert list(table.index) == ["R@1", "R@5", "R@10", "MedR", "MeanR", "MRR"] and list(table.columns) == list(recall.columns)
    assert np.array_equal(table.loc[["R@1", "R@5", "R@10"]].to_numpy(), recall.to_numpy())


def test_the_documented_rank_snippet_runs_as_written(capsys):
    """INTEGRATION.md's rank-statistics block, executed as written; what it prints are rank_statistics of the reference ranks."""
    import re
    from vtc_amd.host.metric import rank_statistics
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "rank_statistics" in b]
    assert len(blocks) == 1
    ns = {}
    exec(blocks[0], ns)
    want_a, want_b, gap = RR.reference_ranks(ns["video"].numpy(), ns["title"].numpy())
    assert gap > 1e-12 and want_a.max() > 1000
    _check(ns["rank_title_from_video"].cpu().numpy(), want_a, "rank_a")
    _check(ns["rank_video_from_title"].cpu().numpy(), want_b, "rank_b")
    st = rank_statistics(want_a, (1, 5, 10, 50, 100))
    assert ns["stats"] == st and capsys.readouterr().out.split() == f"{st['recall_at_k']} {st['median_rank']} {st['mean_rank']} {st['mrr']}".split()
