"""GPU: set queries -- several vectors as one query, the minimum over them (vtc_l2_search_sets / ops.l2_search_sets, VideoIndex.search_any /
search_videos_any / similar_to_video) -- against the numpy reference of tests/search_set_refs.py, and bit for bit against the library's
own one-vector searches.

Ids and groups are compared with exact equality; every such comparison asserts the reference's min_gap > 1e-12 first (the seeds are shown
to have it on the CPU by tests/test_search_set_refs.py).  fp32 dists are within one fp32 ulp of the reference, and bit-equal between
the library's entry points.  The grid crosses every set size with every number of sets, depth, mask kind and storage, ungrouped and with
every group kind (one parametrised case per grid case and kind: eight searches with their references, well under a second); the
galleries and widths rotate, and a grid case's distances are formed once (search_set_refs.case_distances)."""
import numpy as np
import pytest
import torch

import search_grouped_refs as GR
import search_mask_refs as MR
import search_refs as SR
import search_set_refs as ST

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ops():
    from vtc_amd import ops
    return ops


def _index(*a, **kw):
    from vtc_amd.host.search import VideoIndex
    return VideoIndex(*a, device=DEV, **kw)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _words(live):
    return None if live is None else _t(MR.pack_words(live).view(np.int32))


def _stored(g, half):
    """(the gallery as the device holds it, the same rows widened to fp32 for the reference)"""
    if not half:
        return _t(g), g
    g16 = g.astype(np.float16)
    return _t(g16), g16.astype(np.float32)


def _assert_ungrouped(got, want_ids, want_d64):
    ids, grp, dists, _ = got
    assert grp is None and ids.dtype == torch.int64 and dists.dtype == torch.float32 and tuple(ids.shape) == tuple(dists.shape) == want_ids.shape
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    SR.assert_dists_within_one_ulp(dists.cpu().numpy(), want_d64.astype(np.float32))


def _assert_grouped(got, want_ids, want_grp, want_d64):
    ids, grp, dists, _ = got
    assert ids.dtype == torch.int64 and grp.dtype == torch.int32 and tuple(ids.shape) == tuple(grp.shape) == tuple(dists.shape) == want_ids.shape
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.array_equal(grp.cpu().numpy(), want_grp)
    SR.assert_dists_within_one_ulp(dists.cpu().numpy(), want_d64.astype(np.float32))


def _assert_scores(scores, want_d64):
    """VideoIndex's scores are 1 - dists / 2 in fp32 of the library's fp32 dists, which are within one ulp of the reference's: the score
    is that expression of the reference's fp32 distance or of one of its two neighbours; -inf where the list is empty."""
    d32 = np.asarray(want_d64).astype(np.float32)
    with np.errstate(all="ignore"):
        allowed = [np.float32(1.0) - c / np.float32(2.0) for c in (d32, np.nextafter(d32, np.float32(-np.inf)), np.nextafter(d32, np.float32(np.inf)))]
    got = scores.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == d32.shape
    assert np.all((got == allowed[0]) | ((got == allowed[1]) | (got == allowed[2])) & np.isfinite(d32)), (got, allowed[0])


# ---- 1. the grid -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ng,d,m,s,depth", ST.grid())
def test_grid(ng, d, m, s, depth):
    ops = _ops()
    for half in (False, True):
        stored, q, E = ST.case_distances(ng, d, m, s, half)
        tg, tq = _t(stored.copy()), _t(q.copy())
        for mk in GR.MASK_KINDS:
            live = MR.make_mask(mk, ng, seed=ng)
            words = _words(live)
            want_ids, want_d64, gap = SR.sorted_lists(ST.admissible(E, live), depth, 5)
            assert gap > 1e-12, gap
            got = ops.l2_search_sets(tg, tq, depth, live=words, id_base=5)
            _assert_ungrouped(got, want_ids, want_d64)
            assert int(got[3].item()) == 0
            if mk == "none":
                assert bool((got[0] == -1).all()) and bool(torch.isposinf(got[2]).all())
            if mk == "all":                                   # every bit set against no mask at all: the same bits
                bare = ops.l2_search_sets(tg, tq, depth, id_base=5)
                assert torch.equal(bare[0], got[0]) and torch.equal(bare[2], got[2])


@pytest.mark.parametrize("ng,d,m,s,depth,gk", ST.grouped_grid())
def test_grouped_grid(ng, d, m, s, depth, gk):
    """Every case of the grid with every group kind, `sparse_ids` (-1, INT32_MIN and INT32_MAX among the ids) included."""
    ops = _ops()
    groups = GR.make_groups(gk, ng, seed=ng)
    tgroups = _t(groups)
    for half in (False, True):
        stored, q, E = ST.case_distances(ng, d, m, s, half)
        tg, tq = _t(stored.copy()), _t(q.copy())
        for mk in GR.MASK_KINDS:
            live = MR.make_mask(mk, ng, seed=ng)
            want = GR.lists_by_sort(ST.admissible(E, live), groups, depth, 5)
            assert want[3] > 1e-12, want[3]
            got = ops.l2_search_sets(tg, tq, depth, groups=tgroups, live=_words(live), id_base=5)
            _assert_grouped(got, *want[:3])
            assert int(got[3].item()) == 0
            if mk == "none":
                assert bool((got[0] == -1).all()) and bool((got[1] == -1).all()) and bool(torch.isposinf(got[2]).all())


# ---- 2. a set of one member is the plain search, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "mask"])
@pytest.mark.parametrize("s", [1, 2, 4, 9])
def test_one_member_is_the_plain_search_bit_for_bit(s, masked, half):
    ops = _ops()
    ng, d, depth = 1000, 64, 40
    g, q = ST.make_case(ng, d, 1, s, seed=11 + s)
    tg, _ = _stored(g, half)
    tq = _t(q)
    words = _words(MR.make_mask("random_0.5", ng, seed=s)) if masked else None
    groups = _t(GR.make_groups("random_50", ng))
    first = ops.l2_search(tg, tq[:, 0], 1, live=words)[0][:, 0]
    for grouped in (False, True):
        # the excluded key: the nearest row's video, or the nearest row as a GLOBAL id
        for exclude in (None, groups[first].to(torch.int64) if grouped else first + 3):
            ws = ops.workspace(ops.l2_search_sets_workspace_bytes(ng, s, 1, d, depth, grouped), DEV)
            got = ops.l2_search_sets(tg, tq, depth, groups=groups if grouped else None, live=words, exclude=exclude, id_base=3, ws=ws)
            if grouped:
                ws1 = ops.workspace(ops.l2_search_grouped_workspace_bytes(ng, s, d, depth), DEV)
                ids, grp, dists, bits = ops.l2_search_grouped(tg, tq[:, 0], groups, depth, id_base=3, ws=ws1, live=words, exclude=exclude)
                assert torch.equal(got[1], grp)
            else:
                ws1 = ops.workspace(ops.l2_search_workspace_bytes(ng, s, d, depth), DEV)
                ids, dists, bits = ops.l2_search(tg, tq[:, 0], depth, id_base=3, ws=ws1, live=words, exclude=exclude)
            assert torch.equal(got[0], ids) and torch.equal(got[2], dists) and torch.equal(got[3], bits)
            assert torch.equal(ops.search_dists64(ws, s, depth), ops.search_dists64(ws1, s, depth))
            if exclude is not None:                            # and the key is gone
                assert not bool(((got[1].to(torch.int64) if grouped else got[0]) == exclude[:, None]).any())


# ---- 3. the same row in the lists of two tiles ---------------------------------------------------------------------------------------
def _two_tile_case(m, seed):
    """A set of m = 9 or 17 members: member 0 (first tile) and member m - 1 (last tile) next to gallery row 123, the last one nearer;
    the other members far from everything."""
    rng = np.random.default_rng(seed)
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    g = unit(rng.standard_normal((257, 64))).astype(np.float32)
    q = (-unit(g[rng.integers(0, 257, m)] + 0.5 * unit(rng.standard_normal((m, 64))))).astype(np.float32)      # antipodes: distances near 4
    noise = unit(rng.standard_normal((2, 64)))
    return g, q, noise


@pytest.mark.parametrize("m", [9, 17])
def test_a_row_listed_by_two_tiles_comes_out_once_with_the_smaller_distance(m):
    ops = _ops()
    g, q, noise = _two_tile_case(m, seed=m)
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    q[0] = unit(g[123] + 0.30 * noise[0])
    q[m - 1] = unit(g[123] + 0.10 * noise[1])
    D = SR.distances64(g, q)
    assert D[m - 1, 123] < D[0, 123] < np.delete(D[0], 123).min()      # row 123 is the nearest row of both members, in different tiles
    for depth in (1, 20, 64):
        want_ids, want_d64, gap = ST.reference_sets(g, q[None], depth)
        assert gap > 1e-12
        ws = ops.workspace(ops.l2_search_sets_workspace_bytes(257, 1, m, 64, depth), DEV)
        got = ops.l2_search_sets(_t(g), _t(q[None]), depth, ws=ws)
        _assert_ungrouped(got, want_ids, want_d64)
        row = got[0][0].tolist()
        assert row[0] == 123 and row.count(123) == 1 and len(set(row)) == depth
        assert float(ops.search_dists64(ws, 1, depth)[0, 0]) == float(ops.l2_pair_dists64(_t(g), _t(q[m - 1:m]), _t(np.array([123])))[0])


@pytest.mark.parametrize("m", [9, 17])
def test_a_video_listed_by_two_tiles_comes_out_once_by_its_nearer_row(m):
    ops = _ops()
    g, q, noise = _two_tile_case(m, seed=100 + m)
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    groups = GR.make_groups("singletons", 257)
    groups[200] = groups[50] = 7000                           # two rows of one video, each the nearest row of a member of another tile
    q[0] = unit(g[50] + 0.30 * noise[0])
    q[m - 1] = unit(g[200] + 0.10 * noise[1])
    D = SR.distances64(g, q)
    assert D[m - 1, 200] < D[0, 50] < min(np.delete(D[0], 50).min(), np.delete(D[m - 1], 200).min())
    for depth in (1, 20, 64):
        want = ST.reference_sets_grouped(g, q[None], groups, depth)
        assert want[3] > 1e-12
        got = ops.l2_search_sets(_t(g), _t(q[None]), depth, groups=_t(groups))
        _assert_grouped(got, *want[:3])
        assert got[0][0, 0].item() == 200 and got[1][0].tolist().count(7000) == 1 and 50 not in got[0][0].tolist()
        assert len(set(got[1][0].tolist())) == depth


# ---- 4. padding is free ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_a_ragged_batch_is_each_set_alone_at_its_own_size(half):
    g, q = ST.make_case(1000, 128, 17, 5, seed=3)
    index = _index(128, normalized=True, storage=torch.float16 if half else torch.float32)
    index.add(_t(g), video_ids=GR.make_groups("random_50", 1000) + 50)
    sizes = [17, 1, 9, 8, 3]
    tq = _t(q)
    ids, scores, members = index.search_any(tq, 11, sizes=sizes, return_members=True)
    videos, rows, vscores = index.search_videos_any(tq, 11, sizes=sizes)
    for s, size in enumerate(sizes):
        alone = index.search_any(tq[s:s + 1, :size], 11, return_members=True)
        assert all(torch.equal(x[s:s + 1], y) for x, y in zip((ids, scores, members), alone))
        alone = index.search_videos_any(tq[s:s + 1, :size], 11)
        assert all(torch.equal(x[s:s + 1], y) for x, y in zip((videos, rows, vscores), alone))
    _, wide = _stored(g, half)
    want_ids, want_d64, gap = ST.reference_sets(wide, q, 11, sizes=sizes)
    assert gap > 1e-12 and np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.array_equal(members.cpu().numpy(), ST.attaining_members(wide, q, want_ids, sizes=sizes))


@pytest.mark.parametrize("m,at,copy_of", [(1, 1, 0), (2, 0, 1), (4, 2, 3), (7, 7, 0), (8, 3, 5), (16, 16, 2), (23, 0, 22)])
def test_repeating_a_member_changes_no_output_bit(m, at, copy_of):
    """The repeated member goes in at any position -- which can change the tile shape (4 -> 5, 8 -> 9) and the tile a member is in."""
    ops = _ops()
    g, q = ST.make_case(1000, 64, m, 2, seed=40 + m)
    q2 = np.insert(q, at, q[:, copy_of], axis=1)
    groups = _t(GR.make_groups("random_50", 1000))
    for grouped in (False, True):
        out = []
        for sets in (q, q2):
            ws = ops.workspace(ops.l2_search_sets_workspace_bytes(1000, 2, sets.shape[1], 64, 30, grouped), DEV)
            got = ops.l2_search_sets(_t(g), _t(sets), 30, groups=groups if grouped else None, ws=ws)
            out.append([t for t in got if t is not None] + [ops.search_dists64(ws, 2, 30).clone()])
        assert all(torch.equal(x, y) for x, y in zip(*out))


# ---- 5. ties -------------------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_row_and_the_lower_member():
    g, q = ST.make_case(257, 64, 9, 2, seed=8)
    g[57] = g[44]
    g[130] = g[95]
    q[0, 8] = g[44]                                           # a member of the second tile on the duplicated rows
    q[1, 2] = g[95]
    q[1, 8] = q[1, 2]                                         # and two members at bit-equal distances from every row
    index = _index(64, normalized=True)
    index.add(_t(g))
    ids, scores, members = index.search_any(_t(q), 5, return_members=True)
    assert ids[0, :2].tolist() == [44, 57] and ids[1, :2].tolist() == [95, 130] and scores[:, :2].tolist() == [[1.0, 1.0], [1.0, 1.0]]
    assert members[0, :2].tolist() == [8, 8] and members[1, :2].tolist() == [2, 2]
    want_ids, _, gap = ST.reference_sets(g, q, 5)
    assert gap > 1e-12 and np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.array_equal(members.cpu().numpy(), ST.attaining_members(g, q, want_ids))


# ---- 6. exclusion ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_exclusion_of_a_row_and_of_a_video(half):
    ng, d, m, k = 1000, 64, 9, 10
    g, q = ST.make_case(ng, d, m, 3, seed=21)
    groups = GR.make_groups("random_50", ng) + 100
    index = _index(d, normalized=True, storage=torch.float16 if half else torch.float32)
    index.add(_t(g), video_ids=groups)
    _, wide = _stored(g, half)
    tq = _t(q)
    own = SR.sorted_lists(SR.distances64(wide, q[:, 8]), 1)[0][:, 0]          # the nearest row of every set's member in the SECOND tile
    ids, scores = index.search_any(tq, k, exclude=_t(own))
    want_ids, want_d64, gap = ST.reference_sets(wide, q, k, exclude=own)
    assert gap > 1e-12 and np.array_equal(ids.cpu().numpy(), want_ids) and not (want_ids == own[:, None]).any()
    assert (index.search_any(tq, k)[0] == _t(own)[:, None]).any(dim=1).all()          # without the exclusion it is there
    videos, rows, vscores = index.search_videos_any(tq, k, exclude_videos=_t(groups[own].astype(np.int64)))
    want = ST.reference_sets_grouped(wide, q, groups, k, exclude=groups[own].astype(np.int64))
    assert want[3] > 1e-12 and np.array_equal(rows.cpu().numpy(), want[0]) and np.array_equal(videos.cpu().numpy(), want[1].astype(np.int64))
    assert not (want[1] == groups[own][:, None]).any()
    _assert_scores(vscores, want[2])
    # with a subset and removed rows
    live = MR.make_mask("random_0.5", ng, seed=2)
    live[own] = True
    member = MR.make_mask("alt_words", ng)
    member[own] = True
    index.remove(np.flatnonzero(~live))
    sub = index.subset(_t(member))
    ids, _ = index.search_any(tq, k, subset=sub, exclude=_t(own))
    want_ids, _, gap = ST.reference_sets(wide, q, k, live=live & member, exclude=own)
    assert gap > 1e-12 and np.array_equal(ids.cpu().numpy(), want_ids)
    videos, rows, _ = index.search_videos_any(tq, k, subset=sub, exclude_videos=_t(groups[own].astype(np.int64)))
    want = ST.reference_sets_grouped(wide, q, groups, k, live=live & member, exclude=groups[own].astype(np.int64))
    assert want[3] > 1e-12 and np.array_equal(rows.cpu().numpy(), want[0])
    assert np.array_equal(videos.cpu().numpy(), np.where(want[0] >= 0, want[1].astype(np.int64), -1))
    # keys that exclude nothing
    plain, plain_v = index.search_any(tq, k, subset=sub), index.search_videos_any(tq, k, subset=sub)
    for nothing in (_t(np.full(3, -1, np.int64)), _t(np.array([ng, 1 << 40, -5], np.int64))):
        assert all(torch.equal(x, y) for x, y in zip(index.search_any(tq, k, subset=sub, exclude=nothing), plain))
    for nothing in (_t(np.full(3, -1, np.int64)), _t(np.array([5, 1 << 40, 99999], np.int64))):      # no video has these ids
        assert all(torch.equal(x, y) for x, y in zip(index.search_videos_any(tq, k, subset=sub, exclude_videos=nothing), plain_v))


# ---- 7. non-finite members and rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [3, 9])
def test_non_finite_members_and_rows(m):
    ops = _ops()
    ng, d, depth = 257, 64, 7
    g, q = ST.make_case(ng, d, m, 3, seed=31 + m)
    tg = _t(g)
    clean = ops.l2_search_sets(tg, _t(q), depth)
    assert int(clean[3].item()) == 0
    bad = q.copy()
    bad[0, m - 1, 5] = np.nan                                  # one NaN member among finite ones: the set without it
    bad[1] = np.inf                                            # no finite member: an empty row; set 2 is left alone
    got = ops.l2_search_sets(tg, _t(bad), depth)
    assert int(got[3].item()) == 2
    without = ops.l2_search_sets(tg, _t(q[:1, :m - 1]), depth)
    assert torch.equal(got[0][:1], without[0]) and torch.equal(got[2][:1], without[2])
    assert bool((got[0][1] == -1).all()) and bool(torch.isposinf(got[2][1]).all())
    assert torch.equal(got[0][2], clean[0][2]) and torch.equal(got[2][2], clean[2][2])
    want_ids, want_d64, gap = ST.reference_sets(g, bad, depth)
    assert gap > 1e-12
    _assert_ungrouped(got, want_ids, want_d64)
    # a dead member in SLOT 0 of a tile, next to live ones: the tile's finite test is taken from that (zeroed) slot
    slot0 = q.copy()
    slot0[0, 0, 5] = np.nan
    got0 = ops.l2_search_sets(tg, _t(slot0), depth)
    without0 = ops.l2_search_sets(tg, _t(q[:1, 1:]), depth)
    assert int(got0[3].item()) == 2 and int(without0[3].item()) == 0          # bit 2 set, bit 1 clear
    assert torch.equal(got0[0][:1], without0[0]) and torch.equal(got0[2][:1], without0[2])
    assert torch.equal(got0[0][1:], clean[0][1:]) and torch.equal(got0[2][1:], clean[2][1:])
    want_ids, want_d64, gap = ST.reference_sets(g, slot0, depth)
    assert gap > 1e-12
    _assert_ungrouped(got0, want_ids, want_d64)
    groups0 = GR.make_groups("pairs", ng)
    want = ST.reference_sets_grouped(g, slot0, groups0, depth)
    assert want[3] > 1e-12
    _assert_grouped(ops.l2_search_sets(tg, _t(slot0), depth, groups=_t(groups0)), *want[:3])
    grouped = ops.l2_search_sets(tg, _t(bad), depth, groups=_t(GR.make_groups("pairs", ng)))
    assert bool((grouped[0][1] == -1).all()) and bool((grouped[1][1] == -1).all()) and int(grouped[3].item()) == 2
    # a NaN in a live gallery row: bit 1, and the row is never returned; in a dead row: neither
    nearest = int(clean[0][0, 0])
    g2 = g.copy()
    g2[nearest, 9] = np.nan
    got = ops.l2_search_sets(_t(g2), _t(q), depth)
    assert int(got[3].item()) == 1 and nearest not in got[0].cpu().numpy()
    want_ids, want_d64, gap = ST.reference_sets(g2, q, depth)
    assert gap > 1e-12
    _assert_ungrouped(got, want_ids, want_d64)
    live = np.ones(ng, bool)
    live[nearest] = False
    got = ops.l2_search_sets(_t(g2), _t(q), depth, live=_words(live))
    masked = ops.l2_search_sets(tg, _t(q), depth, live=_words(live))
    assert int(got[3].item()) == 0 and torch.equal(got[0], masked[0]) and torch.equal(got[2], masked[2])


# ---- 8. return_members --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("m,s", [(1, 5), (4, 3), (9, 3), (17, 2), (64, 1)])
def test_return_members_names_the_member_that_attains_the_distance(m, s, half):
    ops = _ops()
    ng, d, k = 1000, 128, 12
    g, q = ST.make_case(ng, d, m, s, seed=50 + m)
    index = _index(d, normalized=True, storage=torch.float16 if half else torch.float32)
    index.add(_t(g), video_ids=GR.make_groups("blocks_of_40", ng))
    tq = _t(q)
    for grouped in (False, True):
        if grouped:
            _, rows, _, members = index.search_videos_any(tq, k, return_members=True)
        else:
            rows, _, members = index.search_any(tq, k, return_members=True)
        d64 = ops.search_dists64(index._ws, s, k).clone()      # one library call: s * m <= 64
        assert bool((rows >= 0).all()) and bool(((members >= 0) & (members < m)).all())
        pairs = ops.l2_pair_dists64(index.rows, tq[:, None].expand(s, k, m, d).reshape(-1, d), rows[:, :, None].expand(s, k, m).reshape(-1))
        pairs = pairs.view(s, k, m)
        assert torch.equal(pairs.gather(2, members[:, :, None])[:, :, 0], d64)          # the member's distance IS the list's, bit for bit
        lower = torch.arange(m, device=DEV)[None, None] < members[:, :, None]
        assert not bool(((pairs <= d64[:, :, None]) & lower).any())                     # and no lower member reaches it
        _, wide = _stored(g, half)
        assert np.array_equal(members.cpu().numpy(), ST.attaining_members(wide, q, rows.cpu().numpy()))


# ---- 9. similar_to_video ----------------------------------------------------------------------------------------------------------------
def _video_index(half, d=64):
    """Videos 500, 501, 502, 503 with 1, 2, 9 and 40 rows, added in interleaved calls among 60 filler videos of 5 rows."""
    rng = np.random.default_rng(77)
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    vids = np.concatenate([np.repeat([500, 501, 502, 503], [1, 2, 9, 40]), np.repeat(np.arange(60), 5)])
    vids = vids[rng.permutation(vids.size)]
    centres = unit(rng.standard_normal((600, d)))
    rows = unit(centres[vids] + 0.6 * unit(rng.standard_normal((vids.size, d)))).astype(np.float32)
    index = _index(d, normalized=True, storage=torch.float16 if half else torch.float32)
    for lo in range(0, vids.size, 97):                        # a video's rows come in different calls
        index.add(_t(rows[lo:lo + 97]), video_ids=vids[lo:lo + 97])
    return index, rows, vids.astype(np.int32)


def _video_reference(wide, vids, live, query_videos, k, allowed=None):
    """(the reference's lists, the members it used): every query video's LIVE rows in ascending order, padded by the first; the
    candidates are the live rows (of ``allowed``) of the other videos."""
    sizes = [max(int(((vids == v) & live).sum()), 1) for v in query_videos]
    q = np.full((len(query_videos), max(sizes), wide.shape[1]), np.nan, np.float32)
    for i, v in enumerate(query_videos):
        mine = np.flatnonzero((vids == v) & live)
        if mine.size:
            q[i, :mine.size] = wide[mine]
            q[i, mine.size:] = wide[mine[0]]
    want = ST.reference_sets_grouped(wide, q, vids, k, sizes=sizes, live=live if allowed is None else live & allowed,
                                     exclude=np.asarray(query_videos, np.int64))
    assert want[3] > 1e-12, want[3]
    return want, ST.attaining_members(wide, q, want[0], sizes=sizes)


def _assert_videos(got, want, want_members):
    videos, found, scores, members = got
    assert np.array_equal(found.cpu().numpy(), want[0])
    assert np.array_equal(videos.cpu().numpy(), np.where(want[0] >= 0, want[1].astype(np.int64), -1))
    _assert_scores(scores, want[2])
    assert np.array_equal(members.cpu().numpy(), want_members)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_similar_to_video(half):
    index, rows, vids = _video_index(half)
    _, wide = _stored(rows, half)
    live = np.ones(vids.size, bool)
    asked = [503, 500, 999999, 502, 501]                      # 1, 2, 9 and 40 rows; 999999: a video the index does not hold
    k = 15
    got = index.similar_to_video(asked, k, return_members=True)
    _assert_videos(got, *_video_reference(wide, vids, live, asked, k))
    videos, found, scores, _ = got
    assert not bool((videos == torch.tensor(asked, device=DEV)[:, None]).any())          # the own video is never returned
    assert bool((videos[2] == -1).all()) and bool((found[2] == -1).all()) and bool(torch.isneginf(scores[2]).all())
    assert bool((found[[0, 1, 3, 4]] >= 0).all())
    # a removed row of a query video is no member; a video with no live row left gives an empty row and leaves the others alone
    gone = np.concatenate([np.flatnonzero(vids == 502)[:4], np.flatnonzero(vids == 500)])
    assert index.remove(gone) == 5
    live[gone] = False
    got = index.similar_to_video(torch.tensor(asked), k, return_members=True)
    _assert_videos(got, *_video_reference(wide, vids, live, asked, k))
    videos, found, scores, _ = got
    assert bool((videos[1] == -1).all()) and bool(torch.isneginf(scores[1]).all()) and bool((found[[0, 3, 4]] >= 0).all())
    assert not bool((videos == torch.tensor(asked, device=DEV)[:, None]).any())
    # the candidates are the subset's rows, the members the video's live rows whatever the subset says
    allowed = MR.make_mask("alt_bits", vids.size)
    got = index.similar_to_video([503, 7], k, subset=index.subset(_t(allowed)), return_members=True)
    _assert_videos(got, *_video_reference(wide, vids, live, [503, 7], k, allowed=allowed))
    if half:                                                   # the half index: the fp32 index that holds the widened rows, bit for bit
        other = index.converted(torch.float32)
        assert all(torch.equal(x, y) for x, y in zip(index.similar_to_video(asked, k, return_members=True),
                                                     other.similar_to_video(asked, k, return_members=True)))


def test_similar_to_video_refuses_a_video_of_65_live_rows():
    rng = np.random.default_rng(5)
    g = rng.standard_normal((200, 64)).astype(np.float32)
    vids = np.where(np.arange(200) < 65, 9, 10 + np.arange(200))
    index = _index(64)
    index.add(_t(g), video_ids=vids)
    with pytest.raises(ValueError, match=r"VideoIndex\.similar_to_video: a video has 65 live rows, a set query takes at most 64 members"):
        index.similar_to_video([9], 5)
    index.remove([0])                                          # 64 live rows are a set
    videos, rows, _ = index.similar_to_video([9], 5)
    assert bool((videos >= 10).all()) and bool((rows >= 65).all())


# ---- 10. more than 64 members in a batch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_three_sets_of_forty_members_are_cut_into_calls(half):
    g, q = ST.make_case(1000, 64, 40, 3, seed=9)
    groups = GR.make_groups("random_50", 1000)
    index = _index(64, normalized=True, storage=torch.float16 if half else torch.float32)
    index.add(_t(g), video_ids=groups)
    _, wide = _stored(g, half)
    exclude = np.array([-1, 17, 400], np.int64)
    ids, scores, members = index.search_any(_t(q), 20, exclude=_t(exclude), return_members=True)
    want_ids, want_d64, gap = ST.reference_sets(wide, q, 20, exclude=exclude)
    assert gap > 1e-12 and np.array_equal(ids.cpu().numpy(), want_ids)
    _assert_scores(scores, want_d64)
    assert np.array_equal(members.cpu().numpy(), ST.attaining_members(wide, q, want_ids))
    videos, rows, _ = index.search_videos_any(_t(q), 20)
    want = ST.reference_sets_grouped(wide, q, groups, 20)
    assert want[3] > 1e-12 and np.array_equal(rows.cpu().numpy(), want[0]) and np.array_equal(videos.cpu().numpy(), want[1].astype(np.int64))


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from vtc_amd import _lib as L
    ops = _ops()
    g, q = ST.make_case(257, 64, 4, 2, seed=1)
    index, other = _index(64, normalized=True), _index(64, normalized=True)
    index.add(_t(g))
    other.add(_t(g))
    grouped = _index(64, normalized=True)
    grouped.add(_t(g), video_ids=np.arange(257) // 3)
    tq = _t(q)
    for call in (lambda: index.search_any(tq, 5, after=_t(np.zeros(2, np.int64))),
                 lambda: grouped.search_videos_any(tq, 5, after=_t(np.zeros(2, np.int64))),
                 lambda: grouped.similar_to_video([1], 5, after=_t(np.zeros(1, np.int64)))):
        with pytest.raises(TypeError, match="unexpected keyword argument 'after'"):
            call()
    for sets in (tq[:, :0], _t(np.zeros((1, 65, 64), np.float32)), tq[0], tq[:, :, :32]):
        with pytest.raises(ValueError, match=r"VideoIndex\.search_any: query_sets must be \[S, M, 64\] with 1 <= M <= 64 members a set"):
            index.search_any(sets, 5)
    for sizes in ([4], [0, 4], [4, 5], [1, 2, 3]):
        with pytest.raises(ValueError, match=r"VideoIndex\.search_any: sizes must be 2 ints in \[1, M = 4\], one per set"):
            index.search_any(tq, 5, sizes=sizes)
    for k in (0, 65, 258):
        with pytest.raises(ValueError, match=rf"VideoIndex\.search_any: k={k} must be in \[1, min\(64, len\(index\) = 257\)\]"):
            index.search_any(tq, k)
        with pytest.raises(ValueError, match=rf"VideoIndex\.search_videos_any: k={k} must be in"):
            grouped.search_videos_any(tq, k)
        with pytest.raises(ValueError, match=rf"VideoIndex\.similar_to_video: k={k} must be in"):
            grouped.similar_to_video([1], k)
    with pytest.raises(ValueError, match=r"VideoIndex\.search_any: the subset belongs to another index"):
        index.search_any(tq, 5, subset=other.subset([1, 2, 3]))
    with pytest.raises(ValueError, match=r"VideoIndex\.search_any: exclude must be an int64 \[2\] tensor"):
        index.search_any(tq, 5, exclude=_t(np.zeros(3, np.int64)))
    with pytest.raises(ValueError, match=r"VideoIndex\.search_videos_any: the index has no video ids"):
        index.search_videos_any(tq, 5)
    with pytest.raises(ValueError, match=r"VideoIndex\.similar_to_video: the index has no video ids"):
        index.similar_to_video([1], 5)
    with pytest.raises(ValueError, match=r"l2_search_sets: 5 sets of 13 members are 65 vectors, a call takes at most 64"):
        ops.l2_search_sets(_t(g), _t(np.zeros((5, 13, 64), np.float32)), 5)
    # the C level: reported, not thrown, and nothing is launched
    lib = L.lib()
    tg, ids = _t(g), torch.empty(2, 5, dtype=torch.int64, device=DEV)
    need = lib.vtc_l2_search_sets_workspace_bytes(257, 2, 4, 64, 5, 0)
    assert need > 0 and lib.vtc_l2_search_sets_workspace_bytes(257, 5, 13, 64, 5, 0) == 0
    ws = ops.workspace(need, DEV)
    before = lib.vtc_debug_launch_count()

    def call(n_sets=2, set_size=4, ids_ptr=ids.data_ptr(), ws_bytes=need):
        return lib.vtc_l2_search_sets(tg.data_ptr(), 0, tq.data_ptr(), None, None, None, 257, n_sets, set_size, 64, 5, 0, ids_ptr, None, None, None,
                                      ws.data_ptr(), ws_bytes, None)

    assert call(n_sets=5, set_size=13) != 0 and b"l2_search_sets: n_sets=5 and set_size=13 must be at least 1, n_sets * set_size at most 64" in lib.vtc_last_error()
    assert call(ids_ptr=None) != 0 and b"l2_search_sets: null argument" in lib.vtc_last_error()
    assert call(ws_bytes=need - 1) != 0 and b"l2_search_sets: workspace too small" in lib.vtc_last_error()
    assert lib.vtc_debug_launch_count() == before
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(ids, ops.l2_search_sets(tg, tq, 5)[0])


class _StubTextModel:
    """encode_text is a fixed projection of the token ids: what the text forms need of a model."""

    def __init__(self, ctx, dim):
        gen = torch.Generator(device=DEV).manual_seed(3)
        self.w = torch.randn(ctx, dim, device=DEV, generator=gen)
        self.calls = []

    def encode_text(self, tokens):
        self.calls.append(tuple(tokens.shape))
        return torch.sin(tokens.float() / 97.0) @ self.w


def test_the_text_forms_are_the_set_search_of_the_encoded_members():
    ops = _ops()
    g, _ = ST.make_case(1000, 64, 1, 1, seed=4)
    index = _index(64)
    index.add(_t(g), video_ids=GR.make_groups("random_50", 1000))
    model = _StubTextModel(77, 64)
    tokens = torch.randint(0, 49408, (3, 5, 77), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    feats = ops.normalize_rows(model.encode_text(tokens.reshape(15, 77)).float().contiguous()).view(3, 5, 64)
    ex = _t(np.array([3, -1, 7], np.int64))
    got = index.search_any_text(model, tokens, 9, sizes=[5, 2, 4], exclude=ex, return_members=True)
    assert model.calls[-1] == (15, 77)                          # the flattened tokens, one encode
    assert all(torch.equal(x, y) for x, y in zip(got, index.search_any(feats, 9, sizes=[5, 2, 4], exclude=ex, return_members=True)))
    got = index.search_videos_any_text(model, tokens, 9, exclude_videos=ex)
    assert all(torch.equal(x, y) for x, y in zip(got, index.search_videos_any(feats, 9, exclude_videos=ex)))
    assert not bool(torch.equal(feats[0, 0], feats[0, 1]))      # the members are different vectors: a wrong reshape would show
    for call, name in ((index.search_any_text, "search_any_text"), (index.search_videos_any_text, "search_videos_any_text")):
        for bad in (tokens[0], tokens.reshape(15, 77)[:, None, None]):
            with pytest.raises(ValueError, match=rf"VideoIndex\.{name}: tokens must be \[S, M, ctx\]"):
                call(model, bad, 9)
        with pytest.raises(RuntimeError, match=rf"VideoIndex\.{name}: token ids must be on the GPU"):
            call(model, tokens.cpu(), 9)
    with pytest.raises(ValueError, match=r"VideoIndex\.search_videos_any: the index has no video ids"):
        plain = _index(64)
        plain.add(_t(g))
        plain.search_videos_any_text(model, tokens, 9)


def test_the_set_searches_do_not_sync():
    """search_any and search_videos_any only enqueue, return_members included; similar_to_video reads one count back."""
    g, q = ST.make_case(1000, 64, 9, 3, seed=2)
    index = _index(64, normalized=True)
    index.add(_t(g), video_ids=GR.make_groups("random_50", 1000))
    tq, ex = _t(q), _t(np.array([1, 2, 3], np.int64))
    index.search_any(tq, 5, exclude=ex, return_members=True)      # warm: the workspace is allocated
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        index.search_any(tq, 5, exclude=ex, return_members=True)
        index.search_videos_any(tq, 5, exclude_videos=ex, return_members=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_the_integration_documents_block_runs_as_written():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "search_videos_any" in b]
    assert len(blocks) == 1, len(blocks)
    ns = {}
    exec(blocks[0], ns)                                       # its own asserts: distinct videos, the padding never matches, never the video itself
    assert tuple(ns["ids"].shape) == (4, 10) and tuple(ns["nearest"].shape) == (2, 10) and bool((ns["nearest"] >= 0).all())
