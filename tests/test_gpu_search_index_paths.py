"""GPU: every search method of VideoIndex reaches the scan its arguments ask for, in every slice.  The counterpart of
tests/test_gpu_search_dispatch.py one layer up: there a call of ops.l2_search / ops.l2_search_grouped is compared with the reference of ITS
OWN semantics, here a call of the index is -- through the one scan driver (VideoIndex._scan) and the one pager (VideoIndex._paged) that
every method goes through.

The data is the dispatch test's recipe: 333 rows of 64 columns (no multiple of 32, 4 or 2), 111 videos of three rows each, anywhere in the
gallery -- here under arbitrary video ids, so a page's dense slots differ from them.  1 query is one slice; 65 are a full slice and a
second one that holds ONE query.  The cursor, the excluded row, the excluded video and the stored row of ``similar`` differ from query to
query, so a slice that takes the wrong 64 entries of any of them gives its queries another list.  Each index is built through the public
API (``add``, ``remove``), as fp32 and as half, with every row live and with half of them removed.

Ids and videos are compared exactly: every reference order has min_gap > 1e-12 over its FULL length (deleting rows only widens gaps).
Scores: the index returns fl32(1 - d32 / 2) of the scan's fp32 distance d32, which lies within one fp32 ulp of the reference's (numpy's
summation order differs from the device's in the last fp64 bits, test_gpu_search_dispatch.py); d32 / 2 is exact, so the score must be
that expression of the reference's d32 or of one of its two fp32 neighbours."""
import functools

import numpy as np
import pytest
import torch

import search_after_refs as AR
import search_exclude_refs as XR
import search_grouped_after_refs as PR
import search_grouped_refs as GR
import search_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NG, D_, K, DEEP_K, NQ = 333, 64, 5, 70, 65
STORAGES = ("float32", "float16")
METHODS = ("search", "search_after", "search_exclude", "search_after_exclude", "search_videos", "search_videos_exclude",
           "search_videos_after_exclude", "similar", "similar_videos", "search_deep", "search_videos_deep")


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def _data():
    rng = np.random.default_rng(965)
    rows = rng.standard_normal((NG, D_)).astype(np.float32)
    queries = (rows[rng.choice(NG, NQ, replace=False)] + 0.5 * rng.standard_normal((NQ, D_))).astype(np.float32)
    videos = (7 * rng.permutation(np.arange(NG) // 3) + 3).astype(np.int32)      # 111 videos of three rows, anywhere; ids 3, 10, .. 773
    live = rng.random(NG) < 0.5
    stored = 5 * np.arange(NQ, dtype=np.int64) + 2                                # the stored rows ``similar`` takes: 2, 7, .. 322
    return rows, queries, videos, live, stored


def _cursor_positions(order):
    """Per query the first position p >= 2 of its order at which neither order[q, p] nor order[q, p + 1] is what an earlier query got:
    cursors on order[q, p] and excluded rows order[q, p + 1] that no two queries share."""
    cursors, excluded, pos = set(), set(), []
    for r in order.tolist():
        p = 2
        while r[p] in cursors or r[p + 1] in excluded:
            p += 1
        cursors.add(r[p])
        excluded.add(r[p + 1])
        pos.append(p)
    return np.array(pos)


@functools.lru_cache(maxsize=None)
def _refs(storage, removed):
    """(the arguments, {method: its reference lists}) for all 65 queries; a case with one query takes the first row of each.  The cursor
    stands on a query's third row (third video) or the first later one that no other query has, the excluded row is the one right after
    the cursor, the excluded video that of the query's nearest row (with a cursor: of the video right after it)."""
    rows, queries, videos, live, stored = _data()
    g = rows if storage == "float32" else rows.astype(np.float16).astype(np.float32)          # what the scan sees, widened
    live = live if removed else None
    none = np.full(NQ, -1)
    D, DS = SR.distances64(g, queries), SR.distances64(g, g[stored])
    L, LS = XR.excluded_distances(D, none, live), XR.excluded_distances(DS, none, live)      # the dead rows at +inf
    order, _, gap = SR.sorted_lists(L, NG)
    assert gap > 1e-12 and SR.sorted_lists(LS, NG)[2] > 1e-12, (gap, SR.sorted_lists(LS, NG)[2])
    gorder, gvid, _, _ = GR.lists_by_sort(L, videos, NG)
    every, p, gp = np.arange(NQ), _cursor_positions(order), _cursor_positions(gorder)
    a = dict(after=order[every, p], exclude=order[every, p + 1], ex_video=gvid[:, 0].astype(np.int64),
             page_after=gorder[every, gp], page_ex_video=gvid[every, gp + 1].astype(np.int64), stored=stored)
    for name in ("after", "exclude", "page_after", "stored"):  # per query: the second slice's entry is nobody's of the first slice
        assert len(set(a[name].tolist())) == NQ, name
    for name in ("ex_video", "page_ex_video"):                 # 111 videos cannot differ for 65 queries that each want a near one: the
        assert a[name][64] != a[name][0], name                 # second slice's query has not the video its slice's offset 0 would give it
    want = {"search": SR.sorted_lists(L, K)[:2],
            "search_after": AR.reference_search_after(g, queries, K, a["after"], live)[:2],
            "search_exclude": XR.reference_search_excluding(g, queries, K, a["exclude"], live)[:2],
            "search_after_exclude": XR.reference_search_excluding_after(g, queries, K, a["exclude"], a["after"], live)[:2],
            "search_videos": GR.lists_by_sort(L, videos, K)[:3],
            "search_videos_exclude": XR.reference_search_grouped_excluding(g, queries, videos, K, a["ex_video"], live)[:3],
            "search_videos_after_exclude": PR.page_by_sort(D, videos, K, a["page_after"], live, a["page_ex_video"])[:3],
            "similar": XR.reference_search_excluding(g, g[stored], K, stored, live)[:2],
            "similar_videos": XR.reference_search_grouped_excluding(g, g[stored], videos, K, videos[stored].astype(np.int64), live)[:3],
            "search_deep": SR.sorted_lists(L, DEEP_K)[:2],
            "search_videos_deep": GR.lists_by_sort(L, videos, DEEP_K)[:3]}
    for m, w in want.items():
        assert (w[0] >= 0).all(), m                            # every list is full: about 166 live rows of about 97 videos at the least
    return a, want


@functools.lru_cache(maxsize=None)
def _index(storage, removed):
    from vtc_amd.host.search import VideoIndex
    rows, _, videos, live, _ = _data()
    index = VideoIndex(D_, device=DEV, normalized=True, storage=getattr(torch, storage))      # the rows as they are: the recipe's are no unit rows
    index.add(_t(rows), video_ids=_t(videos))
    if removed:
        assert index.remove(np.flatnonzero(~live)) == int((~live).sum())
    return index


def _call(index, method, q, a, nq):
    arg = {name: _t(ids[:nq]) for name, ids in a.items()}
    if method == "search":
        return index.search(q, K)
    if method == "search_after":
        return index.search(q, K, after=arg["after"])
    if method == "search_exclude":
        return index.search(q, K, exclude=arg["exclude"])
    if method == "search_after_exclude":
        return index.search(q, K, after=arg["after"], exclude=arg["exclude"])
    if method == "search_videos":
        return index.search_videos(q, K)
    if method == "search_videos_exclude":
        return index.search_videos(q, K, exclude_videos=arg["ex_video"])
    if method == "search_videos_after_exclude":
        return index.search_videos(q, K, after=arg["page_after"], exclude_videos=arg["page_ex_video"])
    if method == "similar":
        return index.similar(arg["stored"], K)
    if method == "similar_videos":
        return index.similar_videos(arg["stored"], K)
    if method == "search_deep":
        return index.search_deep(q, DEEP_K)
    assert method == "search_videos_deep"
    return index.search_videos_deep(q, DEEP_K)


def _assert_scores(got, d64):
    """got == fl32(1 - x / 2) for x the reference's fp32 distance or one of its two fp32 neighbours (the module docstring)."""
    d32 = d64.astype(np.float32)
    one, two = np.float32(1.0), np.float32(2.0)
    ok = np.zeros(d32.shape, bool)
    for x in (np.nextafter(d32, np.float32(-np.inf)), d32, np.nextafter(d32, np.float32(np.inf))):
        ok |= got == one - x / two
    assert got.dtype == np.float32 and ok.all(), float(np.abs(got - (one - d32 / two)).max())


def _assert_result(got, want, nq):
    """Rows (and videos) exactly, scores by _assert_scores; ``want`` is (rows, [videos,] dists64) as the references return it, ``got``
    (ids, scores) or (videos, rows, scores) as the index does."""
    assert all(t.shape == got[0].shape and t.shape[0] == nq for t in got)
    rows = got[-2].cpu().numpy()
    assert rows.dtype == np.int64 and np.array_equal(rows, want[0][:nq])
    if len(want) == 3:
        videos = got[0].cpu().numpy()
        assert videos.dtype == np.int64 and np.array_equal(videos, want[1][:nq].astype(np.int64))
    _assert_scores(got[-1].cpu().numpy(), want[-1][:nq])


@pytest.mark.parametrize("removed", [False, True], ids=["all", "half-removed"])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("nq", (1, NQ))
@pytest.mark.parametrize("method", METHODS)
def test_every_method_reaches_its_own_scan_in_every_slice(method, nq, storage, removed):
    a, want = _refs(storage, removed)
    q = _t(_data()[1][:nq])
    _assert_result(_call(_index(storage, removed), method, q, a, nq), want[method], nq)


def test_both_routes_of_search_at_65_queries():
    """65 queries on an fp32 index with every row live go through vtc_l2_topk (test_every_method_... above); with the instance's
    constant above 65 the same call is the scan, two slices of it, and gives the same lists."""
    a, want = _refs("float32", False)
    index, q = _index("float32", False), _t(_data()[1])
    try:
        index.ROUTE_TOPK_MIN_QUERIES = NQ + 1
        scanned = index.search(q, K)
    finally:
        del index.ROUTE_TOPK_MIN_QUERIES
    routed = index.search(q, K)
    _assert_result(scanned, want["search"], NQ)
    _assert_result(routed, want["search"], NQ)
    assert torch.equal(scanned[0], routed[0])
