"""GPU: the grouped query-time search (vtc_l2_search_grouped / ops.l2_search_grouped, vtc_l2_search_merge_grouped, dist.sharded_search_videos
and VideoIndex.search_videos / remove_videos) against the numpy reference of tests/search_grouped_refs.py -- the complete (distance, row)
list with every row that is not the first of its group deleted -- and bit for bit against the library's own ungrouped entry points.

Ids and groups are compared with exact equality; every such comparison asserts the reference's min_gap > 1e-12 first.  fp32 dists are
within one fp32 ulp of the reference, and bit-equal between the library's entry points."""
from dataclasses import asdict

import numpy as np
import pytest
import torch

import rank_refs as RR
import search_grouped_refs as GR
import search_mask_refs as MR
import search_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ops():
    from vtc_amd import ops
    return ops


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _words(live):
    return None if live is None else _t(MR.pack_words(live).view(np.int32))


def _assert_lists(got, want_ids, want_grp, want_d32):
    ids, grp, dists = got
    assert ids.dtype == torch.int64 and grp.dtype == torch.int32 and dists.dtype == torch.float32
    assert tuple(ids.shape) == tuple(grp.shape) == tuple(dists.shape) == want_ids.shape
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.array_equal(grp.cpu().numpy(), want_grp)
    SR.assert_dists_within_one_ulp(dists.cpu().numpy(), want_d32)


def _check(gallery, queries, groups, depth, live=None, id_base=0, want_bits=0, tg=None, tq=None, D=None):
    """One grouped search against the reference; returns (ids, groups, dists) of the device."""
    ops = _ops()
    D = SR.distances64(gallery, queries) if D is None else D
    want_ids, want_grp, want_d64, gap = GR.lists_by_sort(GR._masked(D, live), groups, depth, id_base)
    assert gap > 1e-12, gap
    ids, grp, dists, bits = ops.l2_search_grouped(_t(gallery) if tg is None else tg, _t(queries) if tq is None else tq, _t(groups), depth,
                                                  id_base=id_base, live=_words(live))
    _assert_lists((ids, grp, dists), want_ids, want_grp, want_d64.astype(np.float32))
    assert int(bits.item()) == want_bits
    return ids, grp, dists


@pytest.fixture(scope="module")
def spread64():
    return RR.spread_pairs(1027, 64, 21)


# ---- edge shapes x group kinds x mask kinds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ng,nq,depth", MR.edge_cases())
def test_edge_shapes_group_kinds_and_masks(spread64, ng, nq, depth):
    a, b = spread64
    tg, tq = _t(a[:ng]), _t(b[:nq])
    D = SR.distances64(a[:ng], b[:nq])
    for gk in GR.GROUP_KINDS:
        groups = GR.make_groups(gk, ng, seed=ng)
        unmasked = _check(a[:ng], b[:nq], groups, depth, None, tg=tg, tq=tq, D=D)
        for mk in GR.MASK_KINDS:
            live = MR.make_mask(mk, ng, seed=ng)
            got = _check(a[:ng], b[:nq], groups, depth, live, tg=tg, tq=tq, D=D)
            if mk == "all":                                   # every bit set against no mask at all: the same bits
                assert all(torch.equal(x, y) for x, y in zip(got, unmasked))
            if mk == "none":
                assert bool((got[0] == -1).all()) and bool((got[1] == -1).all()) and bool(torch.isposinf(got[2]).all())


# ---- one group per row: the ungrouped search, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 2, 4, 9])
@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "mask"])
def test_singletons_are_the_ungrouped_search_bit_for_bit(spread64, nq, masked):
    ops = _ops()
    a, b = spread64
    ng, depth = 1027, 40
    tg, tq = _t(a), _t(b[100:100 + nq])
    words = _words(MR.make_mask("random_0.5", ng, seed=nq)) if masked else None
    ws = ops.workspace(ops.l2_search_workspace_bytes(ng, nq, 64, depth), tg.device)
    ws2 = ops.workspace(ops.l2_search_grouped_workspace_bytes(ng, nq, 64, depth), tg.device)
    ids, dists, bits = ops.l2_search(tg, tq, depth, id_base=3, ws=ws, live=words)
    ids2, grp2, dists2, bits2 = ops.l2_search_grouped(tg, tq, _t(GR.make_groups("singletons", ng)), depth, id_base=3, ws=ws2, live=words)
    assert torch.equal(ids, ids2) and torch.equal(dists, dists2) and torch.equal(bits, bits2)
    assert torch.equal(ops.search_dists64(ws, nq, depth), ops.search_dists64(ws2, nq, depth))
    assert torch.equal(grp2.to(torch.int64), ids2 - 3)


# ---- the two insertion paths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["one", "blocks_of_40"])
@pytest.mark.parametrize("order", ["falling", "rising"])
def test_insertion_paths(spread64, kind, order):
    """Distance strictly falling with the row: every row of a group improves it, always the replace path.  Strictly rising: every row but a
    group's first is worse than the entry its group holds, always the drop path."""
    a, b = spread64
    q = b[:1]
    D = SR.distances64(a[:257], q)[0]
    assert np.unique(D).size == 257
    g = a[:257][np.argsort(-D if order == "falling" else D)]
    groups = GR.make_groups(kind, 257)
    for depth in (1, 5, 11):
        ids, grp, _ = _check(g, q, groups, depth)
        n_groups = np.unique(groups).size
        assert int((ids[0] >= 0).sum()) == min(depth, n_groups)
        rows = ids[0, :min(depth, n_groups)].cpu().numpy()
        firsts = np.array([np.flatnonzero(groups == v)[-1 if order == "falling" else 0] for v in groups[rows]])
        assert np.array_equal(rows, firsts)                   # the nearest row of a group is its last (falling) or first (rising) one


def test_the_over_fetch_case(spread64):
    """One video owns the 100 nearest of 257 rows: k = 10 gives 10 distinct videos, the first being that video by its nearest row, while the
    64 nearest ROWS -- the deepest list the scan has -- are all that one video's: collapsing an over-fetched row list on the host cannot
    see the second-nearest video."""
    ops = _ops()
    a, b = spread64
    g, q = a[:257], b[:1]
    D = SR.distances64(g, q)[0]
    by_distance = np.argsort(D)
    groups = np.empty(257, np.int32)
    groups[by_distance[:100]] = 0
    groups[by_distance[100:]] = 1 + np.arange(157) // 2
    ids, grp, _ = _check(g, q, groups, 10)
    assert len(set(grp[0].tolist())) == 10 and int(grp[0, 0]) == 0 and int(ids[0, 0]) == int(by_distance[0])
    assert int(ids[0, 1]) == int(by_distance[100])
    row_ids, _, _ = ops.l2_search(_t(g), _t(q), 64)
    assert set(groups[row_ids[0].cpu().numpy()].tolist()) == {0}


def test_exact_duplicates_go_to_the_lower_row(spread64):
    a, b = spread64
    g = a[:257].copy()
    groups = GR.make_groups("blocks_of_40", 257)
    g[57] = g[44]                                             # inside group 1
    g[130] = g[95]                                            # groups 2 and 3
    q = np.stack([g[44], g[95], b[0]])
    ids, grp, dists = _check(g, q, groups, 5)
    assert ids[0, 0].item() == 44 and grp[0, 0].item() == 1 and dists[0, 0].item() == 0.0
    assert ids[1, :2].tolist() == [95, 130] and grp[1, :2].tolist() == [2, 3] and dists[1, :2].tolist() == [0.0, 0.0]
    rev = groups.copy()                                       # the same rows with the two groups' ids swapped: still the lower ROW first
    rev[groups == 2], rev[groups == 3] = 3, 2
    ids, grp, _ = _check(g, q, rev, 5)
    assert ids[1, :2].tolist() == [95, 130] and grp[1, :2].tolist() == [3, 2]


# ---- rows and queries without a distance ---------------------------------------------------------------------------------------------
def test_nan_rows(spread64):
    a, b = spread64
    ng, nq, depth = 257, 9, 5
    g, q = a[:ng].copy(), b[:nq]
    groups = GR.make_groups("blocks_of_40", ng)
    ids0, grp0, _ = _check(g, q, groups, depth)
    best_row, best_group = int(ids0[0, 0]), int(grp0[0, 0])
    g[best_row, 3] = np.nan                                   # the row that represented its group for query 0
    ids, grp, _ = _check(g, q, groups, depth, want_bits=1)
    assert not (ids == best_row).any()
    where = (grp[0] == best_group).nonzero()
    assert where.numel() == 1 and int(ids[0, where.item()]) != best_row      # the group's next row represents it
    other = 2 if best_group != 2 else 3
    g[groups == other] = np.nan                               # a group of NaN rows only never appears
    ids, grp, _ = _check(g, q, groups, 7, want_bits=1)
    assert not (grp[ids >= 0] == other).any() and bool((ids[:, 6] == -1).all()) and bool((grp[:, 6] == -1).all())      # 7 groups, 6 left
    live = ~np.isnan(g).any(axis=1)                           # the NaN rows dead: they set nothing
    ids, grp, _ = _check(g, q, groups, 7, live=live, want_bits=0)
    assert not (ids == best_row).any()


@pytest.mark.parametrize("nq,bad", [(9, 3), (1, 0), (4, 2)])
def test_nan_query(spread64, nq, bad):
    ops = _ops()
    a, b = spread64
    ng, depth = 257, 11
    q = b[:nq].copy()
    q[bad, 17] = np.nan
    groups = GR.make_groups("random_50", ng, seed=1)
    ids, grp, dists, bits = ops.l2_search_grouped(_t(a[:ng]), _t(q), _t(groups), depth)
    assert int(bits.item()) == 2
    assert bool((ids[bad] == -1).all()) and bool((grp[bad] == -1).all()) and bool(torch.isposinf(dists[bad]).all())
    good = [i for i in range(nq) if i != bad]
    if good:
        want_ids, want_grp, want_d, gap = GR.reference_search_grouped(a[:ng], b[:nq][good], groups, depth)
        assert gap > 1e-12
        _assert_lists((ids[good], grp[good], dists[good]), want_ids, want_grp, want_d)


@pytest.mark.parametrize("d", [192, 512, 2048])
def test_feature_widths(d):
    a, b = RR.spread_pairs(1027, d, 22)
    groups = GR.make_groups("random_50", 1027, seed=d)
    _check(a, b[:9], groups, 11)
    _check(a, b[:9], groups, 11, live=MR.make_mask("random_0.5", 1027, seed=d))


# ---- windows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_windows,depth", [(2, 11), (3, 11), (7, 11), (64, 24)])
@pytest.mark.parametrize("kind", ["strided", "blocks_of_40", "random_50"])
def test_windows_merged_equal_the_whole(spread64, n_windows, depth, kind):
    """Windows cut at odd rows, through groups (`strided`: every window holds every group); 64 windows of 16 rows are shorter than the
    depth.  Bit-equal to the single search."""
    ops = _ops()
    a, b = spread64
    ng, nq = 1027, 9
    groups = GR.make_groups(kind, ng, seed=4)
    live = MR.make_mask("random_0.5", ng, seed=n_windows)
    tg, tq, tgr = _t(a), _t(b[:nq]), _t(groups)
    whole = _check(a, b[:nq], groups, depth, live, tg=tg, tq=tq)
    ws = ops.workspace(ops.l2_search_grouped_workspace_bytes(ng, nq, 64, depth), tg.device)
    ops.l2_search_grouped(tg, tq, tgr, depth, ws=ws, live=_words(live))
    whole64 = ops.search_dists64(ws, nq, depth).clone()
    cuts = [0] + [(ng * w // n_windows) | 1 for w in range(1, n_windows)] + [ng]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        dep = min(depth, hi - lo)
        ids, grp, d64, bits = ops.l2_search_grouped_part(tg[lo:hi], tq, tgr[lo:hi], dep, id_base=lo, live=_words(live[lo:hi]))
        assert int(bits.item()) == 0
        ids, d64 = ops.pad_search_part(ids, d64.clone(), depth)
        parts.append((ids, d64, torch.nn.functional.pad(grp, (0, depth - dep), value=-1)))
    assert n_windows < 64 or min(hi - lo for lo, hi in zip(cuts[:-1], cuts[1:])) < depth
    stacked = [torch.stack([p[i] for p in parts]) for i in range(3)]
    ids, grp, dists = ops.l2_search_merge_grouped(*stacked)
    assert torch.equal(ids, whole[0]) and torch.equal(grp, whole[1]) and torch.equal(dists, whole[2])
    assert torch.equal(dists, whole64.to(torch.float32))


# ---- containment -------------------------------------------------------------------------------------------------------------------
def test_no_write_outside_the_outputs_no_sync_any_stream(spread64):
    from vtc_amd import _lib as L
    lib = L.lib()
    a, b = spread64
    nq, depth, ng, d = 9, 11, 1027, 64
    live = MR.make_mask("random_0.5", ng, seed=11)
    groups = GR.make_groups("random_50", ng, seed=11)
    want_ids, want_grp, want_d, gap = GR.reference_search_grouped(a, b[:nq], groups, depth, live)
    assert gap > 1e-12
    tg, tq = _t(a), _t(b[:nq])
    G = 4                                                     # guard rows on each side
    ids = torch.full((nq + 2 * G, depth), -77, dtype=torch.int64, device=DEV)
    grp = torch.full((nq + 2 * G, depth), -77, dtype=torch.int32, device=DEV)
    dists = torch.full((nq + 2 * G, depth), -77.0, dtype=torch.float32, device=DEV)
    need = lib.vtc_l2_search_grouped_workspace_bytes(ng, nq, d, depth)
    guard = 4096
    ws = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    words = MR.pack_words(live).view(np.int32)
    mask = torch.full((words.size + 2 * 64,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    mask[64:64 + words.size] = _t(words)
    gids = torch.full((ng + 2 * 64,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    gids[64:64 + ng] = _t(groups)
    mask_before, gids_before = mask.clone(), gids.clone()
    bits = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(stream):
            rc = lib.vtc_l2_search_grouped(tg.data_ptr(), tq.data_ptr(), mask[64:].data_ptr(), gids[64:].data_ptr(), ng, nq, d, depth, 0,
                                           ids[G].data_ptr(), grp[G].data_ptr(), dists[G].data_ptr(), bits.data_ptr(),
                                           ws.data_ptr() + guard, need, stream.cuda_stream)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert rc == 0, lib.vtc_last_error()
    stream.synchronize()
    _assert_lists((ids[G:G + nq], grp[G:G + nq], dists[G:G + nq]), want_ids, want_grp, want_d)
    assert int(bits.item()) == 0
    for out, fill in ((ids, -77), (grp, -77), (dists, -77.0)):
        assert bool((out[:G] == fill).all()) and bool((out[G + nq:] == fill).all())
    assert bool((ws[:guard] == 0xA5).all()) and bool((ws[guard + need:] == 0xA5).all())
    assert torch.equal(mask, mask_before) and torch.equal(gids, gids_before)      # the scan only reads the mask and the groups
    d64 = ws[guard:guard + nq * depth * 8].view(torch.float64).view(nq, depth)
    assert torch.equal(d64.to(torch.float32), dists[G:G + nq])


def test_sharded_search_videos_at_world_one(spread64):
    from vtc_amd import dist as VD
    ops = _ops()
    a, b = spread64
    groups = GR.make_groups("random_50", 1027, seed=6)
    tg, tq, tgr = _t(a), _t(b[:9]), _t(groups)
    ids, grp, dists, _ = ops.l2_search_grouped(tg, tq, tgr, 11, id_base=500)
    videos, rows, d = VD.sharded_search_videos(tg, tgr, 500, tq, 11, 0, 1)
    assert videos.dtype == torch.int64 and torch.equal(rows, ids) and torch.equal(videos, grp.to(torch.int64)) and torch.equal(d, dists)
    videos, rows, d = VD.sharded_search_videos(tg[:5], tgr[:5], 0, tq, 11, 0, 1)          # fewer rows than k on the rank: padded
    ids, grp, dists, _ = ops.l2_search_grouped(tg[:5], tq, tgr[:5], 5)
    assert torch.equal(rows[:, :5], ids) and bool((rows[:, 5:] == -1).all()) and bool((videos[:, 5:] == -1).all())
    assert bool(torch.isposinf(d[:, 5:]).all())


# ---- the video-unit ranks of the evaluation side are the positions in this list ----------------------------------------------------
def test_cross_check_against_the_video_unit_ranks():
    from vtc_amd.host.metric import RecallAtK
    from vtc_amd.host.search import VideoIndex
    rng = np.random.default_rng(77)
    n, d, k = 37, 64, 11
    sizes = rng.integers(1, 7, n)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    owner = np.repeat(np.arange(n), sizes)
    videos = RR.unit(rng.standard_normal((n, d))).astype(np.float32)
    scale = np.exp(rng.uniform(np.log(0.5), np.log(20.0), (owner.size, 1)))
    captions = RR.unit(videos[owner] + scale * RR.unit(rng.standard_normal((owner.size, d)))).astype(np.float32)
    assert 100 <= owner.size <= 160
    _, rank_v = RecallAtK("videos", "captions", [1, 5]).grouped_ranks(_t(videos), _t(captions), _t(off), video_to_text="video")
    rank_v = rank_v.cpu().numpy()
    index = VideoIndex(d, device=DEV, normalized=True)
    index.add(_t(captions), video_ids=owner)
    got_videos, got_rows, _ = index.search_videos(_t(videos), k)
    got_videos, got_rows = got_videos.cpu().numpy(), got_rows.cpu().numpy()
    assert GR.reference_search_grouped64(captions, videos, owner.astype(np.int32), k)[3] > 1e-12
    checked = 0
    for v in range(n):
        if rank_v[v] < k:
            assert got_videos[v, rank_v[v]] == v, (v, rank_v[v], got_videos[v])
            assert owner[got_rows[v, rank_v[v]]] == v
            checked += 1
    assert checked >= 10


# ---- VideoIndex ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw_rows():
    rng = np.random.default_rng(31)
    a, b = RR.spread_pairs(600, 100, 25)                       # 100 columns: padded to 128
    scale = np.exp(rng.uniform(-1, 1, (600, 1))).astype(np.float32)
    vids = rng.integers(0, 60, 600) * 1000 + 7                 # 60 videos with sparse ids, their rows scattered
    return (a * scale).astype(np.float32), (b * scale).astype(np.float32), vids


def _index(rows, vids, pieces=1):
    from vtc_amd.host.search import VideoIndex
    index = VideoIndex(100, device=DEV)
    cuts = [len(rows) * p // pieces for p in range(pieces + 1)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        assert index.add(_t(rows[lo:hi]), video_ids=None if vids is None else vids[lo:hi]) == lo
    return index


def _reference_on_index(index, q, k, live=None):
    """The numpy reference over the rows the index stores and the queries as it prepares them."""
    g = index.rows.cpu().numpy()
    qq = index._prepared(q, "queries", check=False).cpu().numpy()
    ids, grp, d32, gap = GR.reference_search_grouped(g, qq, index.video_ids.cpu().numpy(), k, live)
    assert gap > 1e-12
    return ids, grp, d32


def _assert_index_result(got, want):
    videos, rows, scores = got
    ids, grp, d32 = want
    assert videos.dtype == torch.int64 and rows.dtype == torch.int64 and scores.dtype == torch.float32
    assert np.array_equal(rows.cpu().numpy(), ids) and np.array_equal(videos.cpu().numpy(), grp.astype(np.int64))
    dists = (2.0 * (1.0 - scores)).cpu().numpy()
    full = ids >= 0
    assert np.all(np.isneginf(scores.cpu().numpy()[~full]))
    assert np.allclose(dists[full], d32[full], rtol=0, atol=4e-7)         # score = 1 - d / 2 in fp32: an ulp of 1.0 each way


def test_video_index_search_videos(raw_rows):
    a, b, vids = raw_rows
    index = _index(a[:500], vids[:500], pieces=3)             # a video's rows arrive in three add calls
    assert index.grouped and len(index) == 500
    got_ids = index.video_ids
    assert got_ids.dtype == torch.int32 and np.array_equal(got_ids.cpu().numpy(), vids[:500])
    got_ids[0] = -5
    assert int(index.video_ids[0]) == vids[0]                 # a copy
    q = _t(b[:9])
    got = index.search_videos(q, 11)
    _assert_index_result(got, _reference_on_index(index, q, 11))
    assert all(len(set(r)) == 11 for r in got[0].tolist())
    # the best row of query 0's best video goes away: the video stays, by its next-best row
    video, row = int(got[0][0, 0]), int(got[1][0, 0])
    assert index.remove([row]) == 1
    got2 = index.search_videos(q, 11)
    live = np.ones(500, bool)
    live[row] = False
    _assert_index_result(got2, _reference_on_index(index, q, 11, live))
    assert video in got2[0][0].tolist() and row not in got2[1][0].tolist()
    # remove_videos: every live row of the videos, and how many those were
    gone = [video, int(got[0][0, 1]), 999999]                 # the last one is not in the index
    n_rows = int(np.isin(vids[:500], gone).sum()) - 1         # `row` is gone already
    assert index.remove_videos(gone) == n_rows and index.remove_videos(torch.tensor(gone)) == 0 and index.remove_videos([]) == 0
    live &= ~np.isin(vids[:500], gone)
    assert len(index) == int(live.sum()) and np.array_equal(index.live_mask.cpu().numpy(), live)
    got3 = index.search_videos(q, 11)
    _assert_index_result(got3, _reference_on_index(index, q, 11, live))
    assert not np.isin(got3[0].cpu().numpy(), gone).any()
    with pytest.raises(ValueError, match="video_ids"):
        index.remove_videos([-3])
    with pytest.raises(ValueError, match="k="):
        index.search_videos(q, 65)


def test_video_index_subset_and_padding(raw_rows):
    a, b, vids = raw_rows
    index = _index(a[:400], vids[:400])
    q = _t(b[:4])
    members = np.random.default_rng(41).random(400) < 0.3
    sub = index.subset(_t(members))
    got = index.search_videos(q, 11, subset=sub)
    _assert_index_result(got, _reference_on_index(index, q, 11, members))
    assert members[got[1].cpu().numpy()].all()
    three = np.unique(vids[:400])[:3]                         # fewer live videos than k: rows that end in -1 / -1 / -inf
    few = index.subset(_t(np.isin(vids[:400], three)))
    videos, rows, scores = index.search_videos(q, 5, subset=few)
    assert all(sorted(r) == sorted(three.tolist()) for r in videos[:, :3].tolist())
    assert bool((videos[:, 3:] == -1).all()) and bool((rows[:, 3:] == -1).all()) and bool(torch.isneginf(scores[:, 3:]).all())
    with pytest.raises(ValueError, match="another index"):
        _index(a[:400], vids[:400]).search_videos(q, 5, subset=sub)


def test_video_index_state_dict_grouped_and_ungrouped(raw_rows):
    from vtc_amd.host.search import VideoIndex
    a, b, vids = raw_rows
    q = _t(b[:4])
    index = _index(a[:300], vids[:300])
    index.remove([0, 5, 299])
    state = index.state_dict()
    assert set(state) == {"rows", "count", "dim", "normalized", "live", "video_ids"}
    assert state["video_ids"].dtype == torch.int32 and tuple(state["video_ids"].shape) == (300,)
    other = VideoIndex(100, device=DEV)
    other.load_state_dict({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in state.items()})
    assert other.grouped and len(other) == 297 and torch.equal(other.video_ids, index.video_ids)
    for x, y in zip(index.search_videos(q, 7), other.search_videos(q, 7)):
        assert torch.equal(x, y)
    plain = _index(a[:300], None)
    assert not plain.grouped and plain.video_ids is None and set(plain.state_dict()) == {"rows", "count", "dim", "normalized"}
    other.load_state_dict(plain.state_dict())                 # the form without video ids loads too, and the index is ungrouped again
    assert not other.grouped and len(other) == 300
    with pytest.raises(ValueError, match="video_ids"):
        other.search_videos(q, 7)
    for bad in (state["video_ids"][:10], state["video_ids"].to(torch.int64), -state["video_ids"] - 1):
        with pytest.raises(ValueError, match="video_ids"):
            VideoIndex(100, device=DEV).load_state_dict(dict(state, video_ids=bad))


def test_video_index_add_forms(raw_rows):
    from vtc_amd.host.search import VideoIndex
    a, b, vids = raw_rows
    q = _t(b[:4])
    grouped, plain = _index(a[:200], vids[:200]), _index(a[:200], None)
    with pytest.raises(ValueError, match="video_ids"):
        grouped.add(_t(a[200:210]))
    with pytest.raises(ValueError, match="video_ids"):
        plain.add(_t(a[200:210]), video_ids=vids[200:210])
    for bad in ([1.5] * 10, [-1] + [0] * 9, [2 ** 31] + [0] * 9, [0] * 9, np.zeros((10, 1), np.int64), [True] * 10):
        with pytest.raises(ValueError, match="video_ids"):
            grouped.add(_t(a[200:210]), video_ids=bad)
    assert grouped.ntotal == len(grouped) == 200 and plain.ntotal == 200 and not plain.grouped          # nothing changed
    assert np.array_equal(grouped.video_ids.cpu().numpy(), vids[:200])
    assert grouped.add(_t(a[200:210]), video_ids=torch.full((10,), 2 ** 31 - 1)) == 200 and int(grouped.video_ids[-1]) == 2 ** 31 - 1
    empty = VideoIndex(100, device=DEV)
    empty.add(_t(a[:0]))                                      # an empty add decides nothing
    assert not empty.grouped and empty.add(_t(a[:50]), video_ids=vids[:50]) == 0 and empty.grouped
    with pytest.raises(ValueError, match="video_ids"):
        plain.search_videos(q, 5)
    with pytest.raises(ValueError, match="video ids"):
        plain.remove_videos([7])
    # search() on a grouped index is the row search it is on an ungrouped one
    g2 = _index(a[:200], vids[:200])
    for x, y in zip(g2.search(q, 11), plain.search(q, 11)):
        assert torch.equal(x, y)
    g2.remove([3, 50])
    plain.remove([3, 50])
    for x, y in zip(g2.search(q, 11), plain.search(q, 11)):
        assert torch.equal(x, y)


def test_video_index_many_queries_run_in_slices_without_a_sync(raw_rows):
    """130 queries: three calls of the scan (64 + 64 + 2).  The same rows as one query at a time; a NaN query gets -1 / -1 / -inf."""
    a, b, vids = raw_rows
    index = _index(a[:500], vids[:500])
    q = b[:130].copy()
    q[66, 5] = np.nan
    q = _t(q)
    index.search_videos(q, 7)                                 # warm: the workspace is allocated
    torch.cuda.synchronize()
    from vtc_amd import _lib as L
    before = L.lib().vtc_debug_launch_count()
    torch.cuda.set_sync_debug_mode("error")
    try:
        videos, rows, scores = index.search_videos(q, 7)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    launches = L.lib().vtc_debug_launch_count() - before
    one = L.lib().vtc_debug_launch_count()
    index.search_videos(q[:1], 7)
    one = L.lib().vtc_debug_launch_count() - one
    assert launches == one + 2 * 2                            # two more slices, a scan and a merge each
    assert tuple(videos.shape) == (130, 7)
    for i in (0, 63, 64, 65, 66, 127, 128, 129):
        v1, r1, s1 = index.search_videos(q[i:i + 1], 7)
        assert torch.equal(videos[i:i + 1], v1) and torch.equal(rows[i:i + 1], r1) and torch.equal(scores[i:i + 1], s1)
    assert bool((videos[66] == -1).all()) and bool((rows[66] == -1).all()) and bool(torch.isneginf(scores[66]).all())
    assert bool((rows[65] >= 0).all())


def test_video_index_search_videos_text():
    from oracle import arch as A
    from vtc_amd.host import model as HM
    from vtc_amd.host.clip_arch import ClipConfig
    from vtc_amd.host.search import VideoIndex
    ops = _ops()
    torch.set_grad_enabled(False)
    arch = A.TINY
    m = HM.PretrainedCLIP(model_type=ClipConfig(**asdict(arch)))
    m.load_state_dict(A.synth_model(arch, 7, "clip"), strict=True)
    m = m.eval().to(DEV)
    dim = arch.embed_dim
    rng = np.random.default_rng(32)
    index = VideoIndex(dim, device=DEV)
    index.add(_t(rng.standard_normal((200, dim)).astype(np.float32)), video_ids=np.arange(200) // 4)
    sub = index.subset(list(range(0, 200, 3)))
    tokens = A.synth_tokens(5, arch, 9).to(DEV)
    for s in (None, sub):
        got = index.search_videos_text(m, tokens, 7, subset=s)
        want = index.search_videos(ops.normalize_rows(m.encode_text(tokens)), 7, subset=s)
        assert tuple(got[0].shape) == (5, 7) and all(torch.equal(x, y) for x, y in zip(got, want))
        assert all(len(set(r)) == 7 for r in got[0].tolist()) and torch.equal(got[0], got[1] // 4)
