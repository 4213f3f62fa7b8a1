"""GPU: the grouped rank sweep (vtc_l2_rank_grouped -> ops.rank_grouped -> RecallAtK.grouped_ranks -> compute_multi_caption_table) against
the numpy fp64 reference of tests/grouped_rank_refs.py.  Ranks are compared with array_equal in both directions: the sweep is exact.
Every comparison first checks its own data: the smallest relative gap between a target's distance and any other (not bit-equal) distance
exceeds 1e-12, so no summation order decides a rank, and the ranks are not degenerate (max rank_a > n / 2; 0.2 < R@1 < 0.8 in both
directions wherever n >= 63; max rank_b past the fraction of m stated per group of cases).  Data: grouped_spread(counts, d, 100 + n)."""
import functools

import numpy as np
import pytest
import torch

import grouped_rank_refs as GR
import rank_refs as RR

pytestmark = pytest.mark.gpu


def _counts(kind, n):
    """`kind`: an int c (c captions for every video), "lo-hi" (ragged, uniform in [lo, hi], drawn with seed 100 + n), "3x85+2", or the
    counts themselves as a tuple."""
    if isinstance(kind, int):
        return np.full(n, kind, np.int64)
    if isinstance(kind, tuple):
        return np.array(kind, np.int64)
    if kind == "3x85+2":
        return np.array([3] * 85 + [2], np.int64)
    lo, hi = (int(x) for x in kind.split("-"))
    return GR.ragged_counts(n, lo, hi, 100 + n)


@functools.lru_cache(maxsize=None)
def _case(kind, n, d):
    """(a, b, off, rank_a, rank_b) of a named data set: generated and referenced once, shared by the tests, never modified."""
    a, b, off = GR.grouped_spread(_counts(kind, n), d, 100 + n)
    rank_a, rank_b, gap = GR.reference_grouped_ranks(a, b, off)
    assert gap > 1e-12, gap
    for x in (a, b, off, rank_a, rank_b):
        x.setflags(write=False)
    return a, b, off, rank_a, rank_b


def _not_degenerate(rank_a, rank_b, n, m, b_frac):
    """max rank_a > n / 2, max rank_b > b_frac m (b_frac None: not asked), 0.2 < R@1 < 0.8 in both directions for n >= 63."""
    if n < 63:
        return
    r1a, r1b = float((rank_a < 1).mean()), float((rank_b < 1).mean())
    print(f"n={n} m={m}: max rank_a {int(rank_a.max())}, max rank_b {int(rank_b.max())}, R@1 {r1a:.3f} / {r1b:.3f}")
    assert rank_a.max() > n / 2 and 0.2 < r1a < 0.8 and 0.2 < r1b < 0.8, (int(rank_a.max()), r1a, r1b)
    if b_frac is not None:
        assert rank_b.max() > b_frac * m, (int(rank_b.max()), m)


def _sweep(a, b, off, **kw):
    from vtc_amd import ops
    ra, rb, bits = ops.rank_grouped(torch.tensor(a).cuda(), torch.tensor(b).cuda(), off, **kw)
    assert ra.dtype == torch.int64 and rb.dtype == torch.int64 and ra.shape == (b.shape[0],) and rb.shape == (a.shape[0],)
    return ra.cpu().numpy(), rb.cpu().numpy(), int(bits.item())


def _check(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


@pytest.mark.parametrize("kind,n", [((1,), 1), ((5,), 1), ((1, 3), 2), ("1-4", 63), ("1-4", 64), ("1-4", 65), ("3x85+2", 86)])
def test_edge_sizes(kind, n):
    """One video with one caption and with five; two videos with 1 and 3; n one short of / exactly / one past a 64-column strip of the column
    pass with ragged counts 1..4 (n % 4 != 0: the rows of the matrix are padded to 16 bytes, the row pass ends in its scalar tail and the
    column pass meets padding columns, which it must neither count nor pool); n = 86, m = 257 with 256-row blocks: a second block of ONE
    row, whose column counts are carried over from the first."""
    a, b, off, want_a, want_b = _case(kind, n, 64)
    m = b.shape[0]
    if kind == "3x85+2":
        assert m == 257
    _not_degenerate(want_a, want_b, n, m, 0.5)
    got_a, got_b, bits = _sweep(a, b, off, rows_per_block=256)
    assert bits == 0
    _check(got_a, want_a, "rank_a")
    _check(got_b, want_b, "rank_b")


@pytest.mark.parametrize("kind,n,d,rpb,b_frac", [("1-4", 257, 64, 0, 0.5), (20, 256, 64, 256, 0.1), ("1-8", 300, 512, 0, None),
                                                  ("1-3", 700, 128, 0, 0.5), (20, 500, 512, 0, 0.1)])
def test_bulk_equals_the_fp64_reference(kind, n, d, rpb, b_frac):
    """Odd n (padded rows, scalar tail); 256 videos x 20 captions in 20 row blocks of 256 (no padding); ragged 1..8 at d = 512; 700 videos at
    d = 128; 500 x 20 at d = 512 with the default block.  max rank_b > m / 2 for the ragged cases with at most four captions; with 20
    captions per video the best of 20 saturates (observed 0.18 m and 0.15 m): > m / 10."""
    a, b, off, want_a, want_b = _case(kind, n, d)
    _not_degenerate(want_a, want_b, n, b.shape[0], b_frac)
    got_a, got_b, bits = _sweep(a, b, off, rows_per_block=rpb)
    assert bits == 0
    _check(got_a, want_a, "rank_a")
    _check(got_b, want_b, "rank_b")


@pytest.mark.parametrize("n,d", [(65, 64), (700, 128), (1027, 64)])
def test_identity_offsets_are_the_paired_sweep(n, d):
    """off = 0, 1, ..., n with m = n: both outputs equal ops.rank_bidir's on the same tensors (and the paired reference), and so do the sweep's
    statistics -- the two entry points run the same passes over the same matrix.  (1027, 64): five blocks of 256 rows, one padding column."""
    from vtc_amd import _lib as L
    from vtc_amd import ops
    a, b = RR.spread_pairs(n, d, 10 + n)
    want_a, want_b, gap = RR.reference_ranks(a, b)
    assert gap > 1e-12
    RR.assert_not_degenerate(want_a, n)
    RR.assert_not_degenerate(want_b, n)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ws_p = ops.workspace(L.lib().vtc_l2_rank_bidir_workspace_bytes(n, d, 256, 0), ta.device)
    ws_g = ops.workspace(L.lib().vtc_l2_rank_grouped_workspace_bytes(n, n, d, 256, 0), ta.device)
    pa, pb, _ = ops.rank_bidir(ta, tb, rows_per_block=256, ws=ws_p)
    ga, gb, bits = ops.rank_grouped(ta, tb, np.arange(n + 1), rows_per_block=256, ws=ws_g)
    assert int(bits.item()) == 0
    assert torch.equal(ga, pa) and torch.equal(gb, pb)
    st_p, st_g = ops.rank_sweep_stats(ws_p), ops.rank_sweep_stats(ws_g)
    assert all(st_p[k] == st_g[k] for k in ("in_reach", "in_reach_max", "brute_force_owners")), (st_p, st_g)
    _check(ga.cpu().numpy(), want_a, "rank_a")
    _check(gb.cpu().numpy(), want_b, "rank_b")


def test_forced_pool_overflow_changes_nothing():
    """reach_capacity = 8 on the 256 x 20 case: owners of both directions miss the pool and go to the fp64 brute force; same ranks."""
    from vtc_amd import _lib as L
    from vtc_amd import ops
    n, d = 256, 64
    a, b, off, want_a, want_b = _case(20, n, d)
    m = b.shape[0]
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ws = ops.workspace(L.lib().vtc_l2_rank_grouped_workspace_bytes(n, m, d, 256, 8), ta.device)
    ra, rb, _ = ops.rank_grouped(ta, tb, off, rows_per_block=256, reach_capacity=8, ws=ws)
    _check(ra.cpu().numpy(), want_a, "rank_a")
    _check(rb.cpu().numpy(), want_b, "rank_b")
    st = ops.rank_sweep_stats(ws)
    assert min(st["in_reach"]) > 8 and min(st["brute_force_owners"]) > 0, st                # the path did run, in both directions
    ws2 = ops.workspace(L.lib().vtc_l2_rank_grouped_workspace_bytes(n, m, d, 256, 0), ta.device)
    ops.rank_grouped(ta, tb, off, rows_per_block=256, ws=ws2)
    st2 = ops.rank_sweep_stats(ws2)
    assert st2["brute_force_owners"] == (0, 0) and st2["in_reach"] == st["in_reach"], (st, st2)


@functools.lru_cache(maxsize=None)
def _ties_case(scale):
    """300 videos at d = 128, ragged 1..3 captions, with planted structure (video and caption indices below):
      video 10: 40 bit-equal copies of one caption, 0.01 from the video          -> c* is the first copy; rank_a = 0 for all, rank_b = 0
      videos 50..89 within 1e-3 of video 50, the first caption of each = a[50]    -> 40 copies of one caption over 40 videos: every other
                                                                                     caption is far, so rank_b[50 + i] = i (ties by index)
      videos 100..139 identical, the first caption of 100 + i 0.01 from them      -> rank_a of that caption = i (ties count up by g(c))
      video 150 with ONE caption 0.05 from it; the first captions of videos 160..259 within 1e-7 of that caption
                                                                                  -> a cluster of 100 captions in reach of video 150's target:
                                                                                     rank_b[150] = the number of them fp64 finds closer
    `scale` multiplies every row (un-normalised rows: the error bound scales with the norms)."""
    n, d = 300, 128
    rng = np.random.default_rng(77)
    counts = GR.ragged_counts(n, 1, 3, 100 + n)
    counts[10], counts[150] = 40, 1
    a, b, off = GR.grouped_spread(counts, d, 100 + n)
    a, b = a.astype(np.float64), b.astype(np.float64)
    noise = lambda k: RR.unit(rng.standard_normal((k, d)))                                     # noqa: E731
    b[off[10]:off[11]] = RR.unit(a[10] + 0.01 * noise(1))
    a[51:90] = a[50] + 1e-3 * noise(39)
    b[off[50:90]] = a[50]
    a[100:140] = a[100]
    b[off[100:140]] = RR.unit(a[100] + 0.01 * noise(40))
    b[off[150]] = RR.unit(a[150] + 0.05 * noise(1))
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    b32[off[160:260]] = b32[off[150]] + (1e-7 * rng.standard_normal((100, d))).astype(np.float32)
    a32, b32 = (a32 * np.float32(scale)).astype(np.float32), (b32 * np.float32(scale)).astype(np.float32)
    rank_a, rank_b, gap = GR.reference_grouped_ranks(a32, b32, off)
    assert gap > 1e-12, gap
    D150 = GR.distances(a32[150:151], b32[off[160:260]])[:, 0]
    dt150 = GR.distances(a32[150:151], b32[off[150]:off[150] + 1])[0, 0]
    for x in (a32, b32, off, rank_a, rank_b):
        x.setflags(write=False)
    return a32, b32, off, rank_a, rank_b, D150, dt150


@pytest.mark.parametrize("scale", [1.0, 25.0])
def test_ties_duplicates_and_clusters(scale):
    from vtc_amd import _lib as L
    from vtc_amd import ops
    a, b, off, want_a, want_b, D150, dt150 = _ties_case(scale)
    n, m, d = a.shape[0], b.shape[0], a.shape[1]
    # the ranks the construction dictates
    assert (want_a[off[10]:off[11]] == 0).all() and want_b[10] == 0 and off[11] - off[10] == 40
    assert want_b[50:90].tolist() == list(range(40))
    assert want_a[off[100:140]].tolist() == list(range(40))
    closer = int((D150 < dt150).sum())
    assert want_b[150] == closer and (D150 != dt150).all() and 10 < closer < 90
    kappa = ops.rank_kappa(d)
    eps = kappa * (float((a[150].astype(np.float64) ** 2).sum()) + float((b.astype(np.float64) ** 2).sum(1).max()))
    assert (np.abs(D150 - dt150) < 0.5 * eps).all()                                            # the whole cluster is in reach of the target
    assert max(want_a.max(), want_b.max()) > n / 2
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ws = ops.workspace(L.lib().vtc_l2_rank_grouped_workspace_bytes(n, m, d, 0, 0), ta.device)
    ra, rb, bits = ops.rank_grouped(ta, tb, off, ws=ws)
    assert int(bits.item()) == 0
    _check(ra.cpu().numpy(), want_a, "rank_a")
    _check(rb.cpu().numpy(), want_b, "rank_b")
    assert ops.rank_sweep_stats(ws)["in_reach_max"][1] >= 100                                  # video 150 had the cluster in reach


def test_nonfinite_caption_video_and_empty_group():
    """A NaN in one caption of a 3-caption group: that caption has rank_a = n, the video's rank_b comes from the other two, bits & 2.
    A NaN video row: its captions n, the video m, everyone else as the reference with that row never closer, bits & 1.  An empty group
    (the library takes it; RecallAtK.grouped_ranks refuses it): rank_b = m."""
    n, d = 65, 64
    a0, b0, off0, _, _ = _case("1-4", n, d)
    counts = np.diff(off0)
    p = int(np.flatnonzero(counts == 3)[0])
    m = b0.shape[0]
    b = b0.copy()
    c_bad = int(off0[p]) + 1
    b[c_bad, 5] = np.nan
    want_a, want_b, gap = GR.reference_grouped_ranks(a0, b, off0)
    assert gap > 1e-12 and want_a[c_bad] == n and want_b[p] < m
    got_a, got_b, bits = _sweep(a0, b, off0, rows_per_block=256)
    assert bits == 2
    _check(got_a, want_a, "rank_a")
    _check(got_b, want_b, "rank_b")

    q = int(np.flatnonzero(counts == 2)[0])
    a = a0.copy()
    a[q, 3] = np.nan
    want_a, want_b, gap = GR.reference_grouped_ranks(a, b0, off0)
    assert gap > 1e-12 and (want_a[off0[q]:off0[q + 1]] == n).all() and want_b[q] == m
    assert (np.delete(want_b, q) < m).all() and (np.delete(want_a, np.arange(off0[q], off0[q + 1])) < n).all()
    got_a, got_b, bits = _sweep(a, b0, off0, rows_per_block=256)
    assert bits == 1
    _check(got_a, want_a, "rank_a")
    _check(got_b, want_b, "rank_b")

    keep = np.ones(m, bool)
    keep[off0[p]:off0[p + 1]] = False                          # video p loses all its captions
    counts2 = counts.copy()
    counts2[p] = 0
    off2 = GR.counts_to_offsets(counts2)
    want_a, want_b, gap = GR.reference_grouped_ranks(a0, b0[keep], off2)
    assert gap > 1e-12 and want_b[p] == m - 3
    got_a, got_b, bits = _sweep(a0, b0[keep], off2, rows_per_block=256)
    assert bits == 0
    _check(got_a, want_a, "rank_a")
    _check(got_b, want_b, "rank_b")


def test_argument_errors_return_a_status_and_a_message():
    from vtc_amd import _lib as L
    lib = L.lib()
    n, m = 32, 64
    xa, xb = torch.zeros(n, 128, device="cuda"), torch.zeros(m, 128, device="cuda")
    off = torch.arange(0, m + 1, 2, dtype=torch.int32, device="cuda")
    ra, rb = torch.zeros(m, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    f = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.vtc_l2_rank_grouped_workspace_bytes(n, m, 128, 0, 0), dtype=torch.uint8, device="cuda")
    args = lambda d=128, mm=m, o=off.data_ptr(), nbytes=ws.numel(): (xa.data_ptr(), xb.data_ptr(), o, n, mm, d, 0, 0, ra.data_ptr(),   # noqa: E731
                                                                      rb.data_ptr(), f.data_ptr(), ws.data_ptr(), nbytes, None)
    assert lib.vtc_l2_rank_grouped(*args(d=100)) != 0 and b"d=100" in lib.vtc_last_error()
    assert lib.vtc_l2_rank_grouped(*args(nbytes=1024)) != 0 and b"workspace too small" in lib.vtc_last_error()
    assert lib.vtc_l2_rank_grouped(*args(o=None)) != 0 and b"null argument" in lib.vtc_last_error()
    assert lib.vtc_l2_rank_grouped(*args(mm=0)) != 0 and b"m=0" in lib.vtc_last_error()
    assert lib.vtc_l2_rank_grouped(*args()) == 0
    torch.cuda.synchronize()
    # all rows equal: every distance ties at 0 and the lower index wins.  Caption c of video c // 2: c // 2 videos precede its own;
    # video v: c* = caption 2 v, which 2 v captions precede
    assert ra.cpu().tolist() == [c // 2 for c in range(m)] and rb.cpu().tolist() == [2 * v for v in range(n)]


def test_metric_grouped_ranks_pad_d_500():
    """RecallAtK.grouped_ranks zero-pads d = 500 to 512 (distances unchanged), takes numpy or GPU tensors and returns int64 ranks on the GPU."""
    from vtc_amd.host.metric import RecallAtK
    n = 300
    a, b, off, want_a, want_b = _case("1-4", n, 500)
    _not_degenerate(want_a, want_b, n, b.shape[0], 0.5)
    m = RecallAtK("videos", "titles", [1, 5, 10])
    ra, rb = m.grouped_ranks(a, b, off)
    assert ra.is_cuda and rb.is_cuda and ra.dtype == torch.int64 and ra.shape == (b.shape[0],) and rb.shape == (n,)
    _check(ra.cpu().numpy(), want_a, "rank_a")
    _check(rb.cpu().numpy(), want_b, "rank_b")
    ra, rb = m.grouped_ranks(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(off))
    _check(ra.cpu().numpy(), want_a, "rank_a (tensors)")
    _check(rb.cpu().numpy(), want_b, "rank_b (tensors)")
    bad = b.copy()
    bad[7, 0] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        m.grouped_ranks(a, bad, off)


def test_multi_caption_table():
    """From the reference's -inf-padded [N, C, D] tensor with ragged counts: the table of the reference ranks; flat captions with offsets:
    the same; one caption per video: compute_rank_table's frame."""
    from pandas.testing import assert_frame_equal

    import evaluation.retrieval_evaluation as front
    from vtc_amd.host import retrieval_evaluation as RE
    n = 257
    a, b, off, want_a, want_b = _case("1-4", n, 64)
    want = GR.table_from_ranks(want_a, want_b, "full-test", "MSRVTT")
    got = front.compute_multi_caption_table(torch.from_numpy(a), torch.from_numpy(GR.pad_captions(b, off)))
    assert list(got.index) == ["R@1", "R@5", "R@10", "MedR", "MeanR", "MRR"]
    assert list(got.columns) == ["MSRVTT full-test split Video to Text", "MSRVTT full-test split Text to Video"]
    assert_frame_equal(got, want, check_exact=True)
    assert_frame_equal(RE.compute_multi_caption_table(a, b, offsets=off), want, check_exact=True)
    pa, pb = RR.spread_pairs(700, 128, 3)
    one = RE.compute_multi_caption_table(pa, pb[:, None, :], "1k-A", "MSVD")
    assert_frame_equal(one, RE.compute_rank_table(pa, pb, "1k-A", "MSVD"), check_exact=True)
    assert_frame_equal(RE.compute_multi_caption_table(pa, pb, "1k-A", "MSVD", offsets=np.arange(701)), one, check_exact=True)


def test_the_documented_multi_caption_snippet_runs_as_written(capsys):
    """INTEGRATION.md's multi-caption block, executed as written; its table is the one of the reference ranks."""
    import os
    import re
    from pandas.testing import assert_frame_equal
    from vtc_amd.host.retrieval_evaluation import padded_captions_to_offsets
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "compute_multi_caption_table" in b]
    assert len(blocks) == 1
    ns = {}
    exec(blocks[0], ns)
    flat, off = padded_captions_to_offsets(ns["padded"])
    assert off[-1] == int(ns["counts"].sum()) and np.array_equal(np.diff(off), ns["counts"].numpy())
    want_a, want_b, gap = GR.reference_grouped_ranks(ns["video"].numpy(), flat.numpy(), off)
    assert gap > 1e-12 and want_a.max() > 250 and want_b.max() > 100
    assert_frame_equal(ns["table"], GR.table_from_ranks(want_a, want_b, "full-test", "MSRVTT"), check_exact=True)
    assert "MedR" in capsys.readouterr().out
