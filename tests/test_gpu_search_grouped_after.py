"""GPU: pages of distinct videos -- vtc_l2_group_mark_before + vtc_l2_search_grouped_after / ops.l2_group_mark_before /
ops.l2_search_grouped(after=...), the parts, VideoIndex.search_videos(after=...) / search_videos_deep / similar_videos(after=...) --
against the numpy reference of tests/search_grouped_after_refs.py and, bit for bit, against the library's own grouped search.

Ids and groups are compared with exact equality.  The exactness condition -- min_gap > 1e-12 over the full order of every input used
here -- is established on the CPU by tests/test_search_grouped_after_refs.py over search_grouped_after_refs.gpu_inputs(), the inputs
of this file: deleting rows from an order only widens its gaps, so it holds for every mask, prefix and exclusion drawn from them.  fp32
dists are within one fp32 ulp of the reference; the workspace's fp64 distances within 2 d 2^-53 4 of it (two summation orders of d terms
of a D <= 4), and bit-equal between the library's entry points."""
import functools

import numpy as np
import pytest
import torch

import search_after_refs as AR
import search_grouped_after_refs as PR
import search_grouped_refs as GR
import search_mask_refs as MR
import search_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NGS = [1, 2, 64, 65, 257, 1027]
NQS = [1, 2, 3, 5, 8, 9]                                      # every tile shape and a ragged last tile
DEPTHS = [1, 11, 64]
STORAGES = ("float32", "float16")
KINDS = ("singletons", "one", "pairs", "strided", "blocks_of_40", "random_50")


def _ops():
    from vtc_amd import ops
    return ops


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _i64(x):
    return _t(np.asarray(x, np.int64))


def _words(live):
    return None if live is None else _t(MR.pack_words(live).view(np.int32))


@functools.lru_cache(maxsize=None)
def _rows(storage):
    return PR.main_rows(storage)


@pytest.fixture(scope="module")
def data():
    g32, b = _rows("float32")
    return {"t": {"float32": _t(g32), "float16": _t(g32.astype(np.float16))}, "tb": _t(b)}


@functools.lru_cache(maxsize=None)
def _dist(storage):
    g, b = _rows(storage)
    return SR.distances64(g, b[:9])


def _live(ng, masked):
    return MR.make_mask("random_0.5", ng, seed=ng) if masked else None


@functools.lru_cache(maxsize=None)
def _groups(kind, ng):
    uniq, slot = PR.dense_slots(GR.make_groups(kind, ng, seed=ng))
    return slot, int(uniq.size)


def _cursor_rows(D, groups, live, exclude=None):
    """Per query a cursor inside its grouped order: entry 3 + 5 u of it, clamped to its last (-1 for an empty order)."""
    order = GR.lists_by_sort(PR.admissible(D, groups, live, exclude), groups, D.shape[1])[0]
    n_valid = (order >= 0).sum(1)
    return np.array([order[u, min(3 + 5 * u, n_valid[u] - 1)] if n_valid[u] else -1 for u in range(D.shape[0])], np.int64)


def _page(g, q, groups, n_groups, depth, after_rows, live=None, exclude=None, id_base=0, ban=None, cursor=None):
    """One page in a workspace of its own: (ids, groups, dists, fp64 dists, nonfinite bits).  The cursor's distance is formed by
    l2_pair_dists64 from the cursor ROW unless `cursor` = (d64, ids) is given."""
    ops = _ops()
    ws = ops.workspace(ops.l2_search_grouped_workspace_bytes(g.shape[0], q.shape[0], g.shape[1], depth), g.device)
    if cursor is None:
        cursor = (ops.l2_pair_dists64(g, q, after_rows, id_base), after_rows)
    ids, grp, dists, bits = ops.l2_search_grouped(g, q, groups, depth, id_base=id_base, ws=ws, live=live, exclude=exclude, after=cursor,
                                                  n_groups=n_groups, ban=ban)
    return ids, grp, dists, ops.search_dists64(ws, q.shape[0], depth).clone(), bits


def _plain(g, q, groups, depth, live=None, exclude=None):
    ops = _ops()
    ws = ops.workspace(ops.l2_search_grouped_workspace_bytes(g.shape[0], q.shape[0], g.shape[1], depth), g.device)
    ids, grp, dists, bits = ops.l2_search_grouped(g, q, groups, depth, ws=ws, live=live, exclude=exclude)
    return ids, grp, dists, ops.search_dists64(ws, q.shape[0], depth).clone(), bits


def _assert_against_reference(got, want, d=512):
    ids, grp, dists, d64 = got[:4]
    want_ids, want_grp, want_d64 = want[:3]
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert np.array_equal(grp.cpu().numpy(), want_grp)
    SR.assert_dists_within_one_ulp(dists.cpu().numpy(), want_d64.astype(np.float32))
    fin = np.isfinite(want_d64)
    have = d64.cpu().numpy()
    assert np.array_equal(np.isposinf(have), ~fin)
    if fin.any():
        assert np.abs(have[fin] - want_d64[fin]).max() <= 2 * d * 2.0 ** -53 * 4


def _assert_empty(got, rows=slice(None)):
    assert bool((got[0][rows] == -1).all()) and bool((got[1][rows] == -1).all()) and bool(torch.isposinf(got[2][rows]).all())
    assert bool(torch.isposinf(got[3][rows]).all())


def _check(data, storage, ng, nq, depth, masked, kind, with_exclude=False):
    g, q = data["t"][storage][:ng], data["tb"][:nq]
    D = _dist(storage)[:nq, :ng]
    live = _live(ng, masked)
    groups, n_groups = _groups(kind, ng)
    exclude = groups[(np.arange(nq) * 7 + 1) % ng].astype(np.int64) if with_exclude else None
    after = _cursor_rows(D, groups, live, exclude)
    want = PR.page_by_sort(D, groups, depth, after, live, exclude)
    got = _page(g, q, _t(groups), n_groups, depth, _i64(after), live=_words(live), exclude=None if exclude is None else _i64(exclude))
    _assert_against_reference(got, want)
    if with_exclude:
        assert bool((got[1] != _i64(exclude)[:, None]).all())
    return got, want


# ---- 1. against numpy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ng", NGS)
def test_against_the_reference_galleries_and_group_kinds(data, ng, kind):
    """Every gallery size x group kind; the queries, depths, storages and masks rotate so that each value meets each size."""
    case = NGS.index(ng) * len(KINDS) + KINDS.index(kind)
    for storage in STORAGES:
        for masked in (False, True):
            nq = NQS[(case + masked) % len(NQS)]
            depth = min(DEPTHS[(case + (storage == "float16")) % len(DEPTHS)], ng)
            _check(data, storage, ng, nq, depth, masked, kind)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("nq", NQS)
def test_against_the_reference_tiles_and_depths(data, nq, depth):
    """Every tile shape x depth x storage x mask on 257 and 1027 rows, with and without an excluded group."""
    for storage in STORAGES:
        for masked in (False, True):
            _check(data, storage, 257, nq, depth, masked, "pairs", with_exclude=masked)
            _check(data, storage, 1027, nq, depth, masked, "random_50", with_exclude=not masked)


@pytest.mark.parametrize("m", [1, 32, 33])
def test_n_groups_at_the_word_edges(data, m):
    ng, nq = 257, 5
    groups = (np.arange(ng) % m).astype(np.int32)
    D = _dist("float32")[:nq, :ng]
    after = _cursor_rows(D, groups, None)
    after[-1] = GR.lists_by_sort(D[-1:], groups, ng)[0][0, 0]              # ... and one right behind the first video
    g, q = data["t"]["float32"][:ng], data["tb"][:nq]
    for n_groups in (m, m + 31):                                           # the exact count, and a bitmap with spare bits
        got = _page(g, q, _t(groups), n_groups, min(11, ng), _i64(after))
        _assert_against_reference(got, PR.page_by_sort(D, groups, 11, after))
        assert int((got[0][-1] >= 0).sum()) == min(11, m - 1)


# ---- 2. against the library itself, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", NQS)
def test_cursor_values(data, nq):
    """-inf is l2_search_grouped bit for bit; +inf and NaN give empty pages; per query, not per call."""
    ops = _ops()
    for storage in STORAGES:
        for masked in (False, True):
            ng = 257
            g, q = data["t"][storage][:ng], data["tb"][:nq]
            groups, n_groups = _groups("random_50", ng)
            words = _words(_live(ng, masked))
            plain = _plain(g, q, _t(groups), 11, live=words)
            rows = _i64(np.zeros(nq))
            for value in (-np.inf, np.inf, np.nan):
                cd = torch.full((nq,), value, dtype=torch.float64, device=DEV)
                got = _page(g, q, _t(groups), n_groups, 11, None, live=words, cursor=(cd, rows))
                if value == -np.inf:
                    for x, y in zip(got, plain):
                        assert torch.equal(x, y)
                else:
                    _assert_empty(got)
            cd = torch.tensor([(-np.inf, np.inf, np.nan)[u % 3] for u in range(nq)], dtype=torch.float64, device=DEV)
            got = _page(g, q, _t(groups), n_groups, 11, None, live=words, cursor=(cd, rows))
            for u in range(nq):
                if u % 3 == 0:
                    assert all(torch.equal(x[u], y[u]) for x, y in zip(got[:4], plain[:4]))
                else:
                    _assert_empty(got, u)
    ban = ops.l2_group_mark_before(g, q, _t(groups), n_groups, (torch.full((nq,), np.nan, dtype=torch.float64, device=DEV), rows), live=words)
    live_groups = np.unique(groups[_live(257, True)])
    want = np.zeros(2, np.uint32)
    np.bitwise_or.at(want, live_groups >> 5, np.uint32(1) << (live_groups & 31).astype(np.uint32))
    assert np.array_equal(ban.cpu().numpy().view(np.uint32), np.tile(want, (nq, 1)))      # a NaN cursor marks every live group


@pytest.mark.parametrize("nq", NQS)
def test_four_pages_of_16_are_one_search_of_64(data, nq):
    for storage in STORAGES:
        for masked in (False, True):
            ng = 1027
            g, q = data["t"][storage][:ng], data["tb"][:nq]
            groups, n_groups = _groups("pairs", ng)
            words = _words(_live(ng, masked))
            want = _plain(g, q, _t(groups), 64, live=words)
            pages = [_plain(g, q, _t(groups), 16, live=words)]
            for _ in range(3):
                last = pages[-1]
                pages.append(_page(g, q, _t(groups), n_groups, 16, None, live=words, cursor=(last[3][:, -1].clone(), last[0][:, -1].clone())))
            for k in range(4):
                assert torch.equal(torch.cat([p[k] for p in pages], dim=1), want[k]), (storage, masked, k)


@pytest.mark.parametrize("kind", ["pairs", "blocks_of_40"])
def test_pages_of_64_until_exhausted_are_the_full_grouped_order(data, kind):
    ng, nq = 257, 3
    groups, n_groups = _groups(kind, ng)
    for storage in STORAGES:
        g, q = data["t"][storage][:ng], data["tb"][:nq]
        full = PR.full_grouped_order(_dist(storage)[:nq, :ng], groups)
        pages = [_plain(g, q, _t(groups), 64)]
        for _ in range(-(-n_groups // 64)):                                # one more than needed: the last is empty
            pages.append(_page(g, q, _t(groups), n_groups, 64, pages[-1][0][:, -1].clone()))
        _assert_empty(pages[-1])
        got = tuple(torch.cat([p[k] for p in pages], dim=1)[:, :ng] for k in range(4))
        width = got[0].shape[1]
        _assert_against_reference(got, tuple(x[:, :width] for x in full[:3]))
        assert int((got[0] >= 0).sum()) == nq * n_groups


# ---- 3. where the cursor stands -----------------------------------------------------------------------------------------------------------
def test_a_cursor_on_a_dead_row_and_on_a_row_of_the_excluded_video(data):
    ng, nq = 257, 5
    groups, n_groups = _groups("pairs", ng)
    for storage in STORAGES:
        g, q = data["t"][storage][:ng], data["tb"][:nq]
        D = _dist(storage)[:nq, :ng]
        cur = GR.lists_by_sort(D, groups, 20)[0][:, 4].copy()              # every query's fifth video, by its nearest row
        live = np.ones(ng, bool)
        live[cur] = False                                                 # ... which is dead for everybody
        got = _page(g, q, _t(groups), n_groups, 11, _i64(cur), live=_words(live))
        _assert_against_reference(got, PR.page_by_sort(D, groups, 11, cur, live))
        ex = groups[cur].astype(np.int64)
        got = _page(g, q, _t(groups), n_groups, 11, _i64(cur), exclude=_i64(ex))
        _assert_against_reference(got, PR.page_by_sort(D, groups, 11, cur, None, ex))
        assert bool((got[1] != _i64(ex)[:, None]).all())
        no_key = np.array([-1, ng, 2 ** 40, -2 ** 62, cur[4]], np.int64)     # no row of the gallery: an empty page for that query alone
        got = _page(g, q, _t(groups), n_groups, 11, _i64(no_key))
        _assert_empty(got, slice(0, 4))
        _assert_against_reference(got, PR.page_by_sort(D, groups, 11, no_key))


@pytest.mark.parametrize("nq", [1, 9])
def test_a_video_with_one_row_before_the_cursor_and_one_after_it_in_another_workgroups_share(data, nq):
    """Rows 0 and 1026 are one video.  The cursor is the row right before the farther of the two in the query's row order: the nearer
    one lies at or before it, so the video is behind the cursor -- but the farther row is the very next row after it, in the share of
    the scan's LAST workgroup while the nearer one is in the first's.  One pass would return it first."""
    ng = 1027
    groups = (np.arange(ng) // 2).astype(np.int32)
    groups[ng - 1] = groups[0]
    n_groups = int(groups.max()) + 1
    for storage in STORAGES:
        g, q = data["t"][storage], data["tb"][:nq]
        D = _dist(storage)[:nq]
        order = AR.full_order(_rows(storage)[0], _rows(storage)[1][:nq])[0]
        after, hi = np.empty(nq, np.int64), np.empty(nq, np.int64)
        for u in range(nq):
            hi[u] = 0 if D[u, 0] > D[u, ng - 1] else ng - 1
            after[u] = order[u, int(np.flatnonzero(order[u] == hi[u])[0]) - 1]
        got = _page(g, q, _t(groups), n_groups, 11, _i64(after))
        assert bool((got[1] != int(groups[0])).all()) and bool((got[0] != _i64(hi)[:, None]).all())
        _assert_against_reference(got, PR.page_by_sort(D, groups, 11, after))
        ungrouped = _ops().l2_search(g, q, 1, after=(_ops().l2_pair_dists64(g, q, _i64(after)), _i64(after)))[0]
        assert torch.equal(ungrouped[:, 0], _i64(hi))                      # the row a scan without the mark pass meets first


def test_a_run_of_bit_equal_distances_cut_by_the_cursor(data):
    g_np, q_np = PR.tied_rows()
    n = g_np.shape[0]
    g, q = _t(g_np), _t(q_np)
    D = SR.distances64(g_np, q_np)
    order = AR.full_order(g_np, q_np)[0]
    for kind in ("pairs", "random_50"):
        groups, n_groups = _groups(kind, n)
        for pos in (2, 7, 131):                                            # inside runs of five: videos straddle the cursor
            after = order[:, pos]
            got = _page(g, q, _t(groups), n_groups, 11, _i64(after))
            _assert_against_reference(got, PR.page_by_sort(D, groups, 11, after))
        full = PR.full_grouped_order(D, groups)
        pages = [_plain(g, q, _t(groups), 7)]
        while bool((pages[-1][0][:, -1] >= 0).any()):
            pages.append(_page(g, q, _t(groups), n_groups, 7, pages[-1][0][:, -1].clone()))
        got = tuple(torch.cat([p[k] for p in pages], dim=1) for k in range(4))
        width = min(got[0].shape[1], n)
        _assert_against_reference(tuple(x[:, :width] for x in got), tuple(x[:, :width] for x in full[:3]))


def test_groups_outside_the_range_are_never_returned_and_mark_nothing(data):
    ng, nq = 257, 5
    base, n_groups = _groups("pairs", ng)
    for storage in STORAGES:
        g, q = data["t"][storage][:ng], data["tb"][:nq]
        D = _dist(storage)[:nq, :ng]
        near = GR.lists_by_sort(D, base, 3)[0]
        groups = base.copy()
        outside = np.unique(np.concatenate([near[:, 0], near[:, 2]]))     # rows in front of every order, so that they matter
        groups[outside[0::2]] = n_groups
        groups[outside[1::2]] = -1
        live = np.ones(ng, bool)
        live[outside] = False                                             # the reference: the gallery without those rows
        after = _cursor_rows(D, base, live)
        got = _page(g, q, _t(groups), n_groups, 11, _i64(after))
        _assert_against_reference(got, PR.page_by_sort(D, base, 11, after, live))
        first = _page(g, q, _t(groups), n_groups, 11, None,
                      cursor=(torch.full((nq,), -np.inf, dtype=torch.float64, device=DEV), _i64(np.zeros(nq))))
        _assert_against_reference(first, GR.lists_by_sort(PR.admissible(D, base, live), base, 11))
        ban = _ops().l2_group_mark_before(g, q, _t(groups), n_groups,
                                          (torch.full((nq,), np.inf, dtype=torch.float64, device=DEV), _i64(np.zeros(nq))))
        with_mask = _ops().l2_group_mark_before(g, q, _t(base), n_groups,
                                                (torch.full((nq,), np.inf, dtype=torch.float64, device=DEV), _i64(np.zeros(nq))), live=_words(live))
        assert torch.equal(ban, with_mask)


def test_two_windows_marked_into_one_ban_buffer_and_merged(data):
    ops = _ops()
    ng, nq, cut, depth = 1027, 9, 500, 64
    groups, n_groups = _groups("random_50", ng)
    for storage in STORAGES:
        for masked in (False, True):
            g, q = data["t"][storage], data["tb"][:nq]
            live = _live(ng, masked)
            D = _dist(storage)[:nq]
            after = _i64(_cursor_rows(D, groups, live))
            ex = _i64(groups[(np.arange(nq) * 7 + 1) % ng])
            whole = _page(g, q, _t(groups), n_groups, depth, after, live=_words(live), exclude=ex)
            cursor = (ops.l2_pair_dists64(g, q, after), after)
            windows = [(g[:cut], _t(groups[:cut]), None if live is None else _words(live[:cut]), 0),
                       (g[cut:], _t(groups[cut:]), None if live is None else _words(live[cut:]), cut)]
            ban = None
            for rows, grp, words, base in windows:                        # EVERY window is marked before any is scanned
                ban = ops.l2_group_mark_before(rows, q, grp, n_groups, cursor, live=words, id_base=base, ban=ban)
            parts = [ops.l2_search_grouped_part(rows, q, grp, depth, id_base=base, live=words, exclude=ex, after=cursor, n_groups=n_groups,
                                                ban=ban)[:3] for rows, grp, words, base in windows]
            ids, grp, dists = ops.l2_search_merge_grouped(torch.stack([p[0] for p in parts]), torch.stack([p[2] for p in parts]),
                                                          torch.stack([p[1] for p in parts]))
            assert torch.equal(ids, whole[0]) and torch.equal(grp, whole[1]) and torch.equal(dists, whole[2]), (storage, masked)
            with pytest.raises(ValueError):
                ops.l2_search_grouped_part(g[:cut], q, _t(groups[:cut]), depth, after=cursor, n_groups=n_groups)


@pytest.mark.parametrize("d", PR.WIDTHS)                       # one and eight 256-column slices a lane walks
def test_feature_widths(d):
    g_np, q_np = PR.width_rows(d)
    ng = g_np.shape[0]
    groups, n_groups = _groups("strided", ng)
    D = SR.distances64(g_np, q_np)
    after = _cursor_rows(D, groups, None)
    got = _page(_t(g_np), _t(q_np), _t(groups), n_groups, 5, _i64(after))
    _assert_against_reference(got, PR.page_by_sort(D, groups, 5, after), d=d)
    assert int((got[0] >= 0).sum()) > 0


def test_a_nan_query_leaves_its_neighbours_alone(data):
    ng, nq = 257, 9
    groups, n_groups = _groups("pairs", ng)
    g = data["t"]["float32"][:ng]
    q = data["tb"][:nq].clone()
    q[4, 17] = float("nan")
    D = _dist("float32")[:nq, :ng]
    after = _cursor_rows(D, groups, None)
    clean = _page(g, data["tb"][:nq], _t(groups), n_groups, 11, _i64(after))
    got = _page(g, q, _t(groups), n_groups, 11, _i64(after))
    keep = [u for u in range(nq) if u != 4]
    for k in range(4):
        assert torch.equal(got[k][keep], clean[k][keep])
    _assert_empty(got, 4)
    assert int(got[4].item()) == int(_plain(g, q, _t(groups), 11)[4].item()) == 2 and int(clean[4].item()) == 0


def test_wrong_arguments_raise(data):
    ops = _ops()
    g, q = data["t"]["float32"][:257], data["tb"][:5]
    groups, n_groups = _groups("pairs", 257)
    gt = _t(groups)
    cd, ci = torch.zeros(5, dtype=torch.float64, device=DEV), torch.zeros(5, dtype=torch.int64, device=DEV)
    ok_ban = torch.zeros(5, (n_groups + 31) // 32, dtype=torch.int32, device=DEV)
    for after in ((cd[:4], ci), (cd.float(), ci), (cd, ci.int()), (cd.cpu(), ci), (cd,), cd):
        with pytest.raises(ValueError):
            ops.l2_search_grouped(g, q, gt, 5, after=after, n_groups=n_groups)
        with pytest.raises(ValueError):
            ops.l2_group_mark_before(g, q, gt, n_groups, after)
    for n in (None, 0, -3, 2 ** 31, 2.0):
        with pytest.raises(ValueError):
            ops.l2_search_grouped(g, q, gt, 5, after=(cd, ci), n_groups=n)
    for ban in (ok_ban[:4], ok_ban.long(), ok_ban.cpu(), ok_ban[:, :1], torch.zeros(5, 2 * ok_ban.shape[1], dtype=torch.int32, device=DEV)[:, ::2]):
        with pytest.raises(ValueError):
            ops.l2_search_grouped(g, q, gt, 5, after=(cd, ci), n_groups=n_groups, ban=ban)
        with pytest.raises(ValueError):
            ops.l2_group_mark_before(g, q, gt, n_groups, (cd, ci), ban=ban)
    assert ops.l2_group_mark_before(g, q, gt, n_groups, (cd, ci), ban=ok_ban) is ok_ban


# ---- 4. VideoIndex ------------------------------------------------------------------------------------------------------------------------
def _sparse_video_ids(groups):
    """Dense groups -> arbitrary video ids in [0, 2^31), 7, 2^31 - 1 and 123456789 among them, in no order."""
    table = (np.arange(int(groups.max()) + 1, dtype=np.int64) * 2654435761 + 11) % (2 ** 31 - 1)
    table[:3] = (7, 2 ** 31 - 1, 123456789)
    assert np.unique(table).size == table.size
    return table[groups]


def _index(data, storage, kind="pairs"):
    """A `normalized` index: its stored rows are the rows of search_grouped_after_refs.main_rows(storage), bit for bit."""
    from vtc_amd.host.search import VideoIndex
    vids = _sparse_video_ids(_groups(kind, 1027)[0])
    index = VideoIndex(512, device=DEV, normalized=True, storage={"float32": torch.float32, "float16": torch.float16}[storage])
    index.add(data["t"]["float32"][:600], video_ids=torch.from_numpy(vids[:600]))
    index.add(data["t"]["float32"][600:], video_ids=torch.from_numpy(vids[600:]))
    assert np.array_equal(index.rows.float().cpu().numpy(), _rows(storage)[0])
    return index, vids.astype(np.int32)


def _assert_videos(got, want):
    videos, rows, scores = got
    want_ids, want_grp, want_d64 = want[:3]
    assert np.array_equal(rows.cpu().numpy(), want_ids)
    assert np.array_equal(videos.cpu().numpy(), np.where(want_ids >= 0, want_grp.astype(np.int64), -1))
    s = scores.cpu().numpy().astype(np.float64)
    full = want_ids >= 0
    assert np.array_equal(np.isneginf(s), ~full)
    if full.any():
        assert np.abs(s[full] - (1.0 - want_d64[full] / 2.0)).max() < 5e-7      # fp32 scores of magnitude <= 1: a few ulps of 6e-8


@pytest.mark.parametrize("storage", STORAGES)
def test_index_pages(data, storage):
    index, vids = _index(data, storage)
    g_np, b = _rows(storage)
    nq = 65                                                   # two slices of queries
    queries = data["tb"][:nq]
    D = SR.distances64(g_np, b[:nq])
    first = index.search_videos(queries, 10)
    _assert_videos(first, GR.lists_by_sort(D, vids, 10))
    after = first[1][:, -1].clone()
    after[3], after[64] = -1, index.ntotal + 5                # no row: an empty page, for that query alone
    second = index.search_videos(queries, 10, after=after)
    _assert_videos(second, PR.page_by_sort(D, vids, 10, after.cpu().numpy()))
    assert bool((second[1][[3, 64]] == -1).all()) and bool((second[1][[0, 63]] >= 0).all())
    # a subset, after remove_videos, with exclude_videos
    member = MR.make_mask("random_0.5", 1027, seed=12)
    subset = index.subset(torch.from_numpy(member))
    gone = vids[[10, 500, 900]].astype(np.int64)
    assert index.remove_videos(torch.from_numpy(gone)) > 0
    live = index.live_mask.cpu().numpy() & member
    assert not live[np.isin(vids, gone)].any()
    ex = GR.lists_by_sort(PR.admissible(D, vids, live), vids, 1)[1][:, 0].astype(np.int64)      # every query's nearest video
    ex[5], ex[6] = -1, 5                                      # no video of the index: nothing is excluded
    assert 5 not in vids
    page1 = index.search_videos(queries, 7, subset=subset, exclude_videos=_i64(ex))
    _assert_videos(page1, GR.lists_by_sort(PR.admissible(D, vids, live, ex), vids, 7))
    page2 = index.search_videos(queries, 7, subset=subset, exclude_videos=_i64(ex), after=page1[1][:, -1])
    _assert_videos(page2, PR.page_by_sort(D, vids, 7, page1[1][:, -1].cpu().numpy(), live, ex))
    # deep: any k
    deep = index.search_videos_deep(queries[:3], 200, subset=subset, exclude_videos=_i64(ex[:3]))
    assert tuple(deep[0].shape) == (3, 200)
    full = PR.full_grouped_order(D[:3], vids, live, ex[:3])
    _assert_videos(deep, tuple(x[:, :200] for x in full[:3]))
    short = index.search_videos_deep(queries[:2], 40)
    _assert_videos(short, GR.lists_by_sort(PR.admissible(D[:2], vids, index.live_mask.cpu().numpy()), vids, 40))
    with pytest.raises(ValueError):
        index.search_videos_deep(queries[:2], len(index) + 1)
    for wrong in (after[:64], after.to(torch.int32), after.float()):
        with pytest.raises(ValueError):
            index.search_videos(queries, 5, after=wrong)


@pytest.mark.parametrize("storage", STORAGES)
def test_index_similar_videos_pages(data, storage):
    index, vids = _index(data, storage, kind="random_50")
    g_np = _rows(storage)[0]
    rows = PR.SIMILAR_ROWS
    D = SR.distances64(g_np, g_np[rows])
    own = vids[rows].astype(np.int64)
    first = index.similar_videos(_i64(rows), 10)
    _assert_videos(first, GR.lists_by_sort(PR.admissible(D, vids, None, own), vids, 10))
    second = index.similar_videos(_i64(rows), 10, after=first[1][:, -1])
    _assert_videos(second, PR.page_by_sort(D, vids, 10, first[1][:, -1].cpu().numpy(), None, own))
    assert bool((second[0] != _i64(own)[:, None]).all())
    own_row = index.similar_videos(_i64(rows), 10, after=_i64(rows))      # the cursor on the query's own row: distance 0, the first key
    _assert_videos(own_row, PR.page_by_sort(D, vids, 10, rows, None, own))


def test_after_none_is_the_call_without_the_argument(data):
    index, _ = _index(data, "float32")
    q, rows = data["tb"][:13], _i64(PR.SIMILAR_ROWS[:13])
    for a, b in ((index.search_videos(q, 7), index.search_videos(q, 7, after=None)),
                 (index.search_videos(q, 7, None, rows), index.search_videos(q, 7, subset=None, exclude_videos=rows, after=None)),
                 (index.similar_videos(rows, 7), index.similar_videos(rows, 7, after=None)),
                 (index.search_videos(q, 64), index.search_videos_deep(q, 64))):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    ops = _ops()
    g, vt = index.rows, index.video_ids
    for x, y in zip(ops.l2_search_grouped(g, q[:5], vt, 7), ops.l2_search_grouped(g, q[:5], vt, 7, after=None, n_groups=None, ban=None)):
        assert torch.equal(x, y)


def test_the_second_paged_call_after_an_add_does_not_sync(data):
    index, _ = _index(data, "float32")
    q, rows = data["tb"][:3], _i64([4, 77, 1000])
    calls = (lambda: index.search_videos(q, 5, after=rows), lambda: index.search_videos(q, 5, after=rows, exclude_videos=rows),
             lambda: index.similar_videos(rows, 5, after=rows), lambda: index.search_videos_deep(q, 100))
    want = [c() for c in calls]                               # the first paged call after the add: torch.unique's one sync, workspaces
    index.remove([5, 6])                                      # a remove does not invalidate the dense numbering
    want = [c() for c in calls]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [c() for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(got, want):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_the_integration_documents_block_runs_as_written():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "search_videos_deep" in b]
    assert len(blocks) == 1, len(blocks)
    ns = {}
    exec(blocks[0], ns)                                       # its own asserts: the pages are the deep ranking, no video twice
    assert tuple(ns["videos"].shape) == (4, 150) and bool((ns["videos"] >= 0).all())
