"""GPU: the range search (vtc_l2_range_count / vtc_l2_range_fill, ops.l2_range_count / ops.l2_range_search, VideoIndex.range_*) against
the numpy fp64 reference of tests/search_range_refs.py and against the device's own bits (vtc_l2_search's fp64 distances).

Membership is compared with exact equality.  Against numpy every case asserts min_margin > 1e-12 first: the radii are midpoints between
consecutive sorted reference distances, so no summation order can decide a hit.  AT the boundary the comparison is with the merged
search's own fp64 distances (the head of its workspace), which the range search must reproduce bit for bit.  fp32 dists are within one
ulp of the reference, as everywhere in the search tests.

Shapes are the smallest at which each mechanism can break: a word's tail and a step's tail (ng = 1 .. 1 003), several workgroups and a
partial last word (70 001), more hit words than a grid has waves so that a wave takes several (300 001: 9 376 words against at most
4 096 waves), a second, partly filled pass of the lane loop (d = 320), every tile shape and an unfilled tile slot (nq)."""
from dataclasses import asdict

import numpy as np
import pytest
import torch

import rank_refs as RR
import search_half_refs as HR
import search_range_refs as RG
import search_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NQS = (1, 2, 3, 5, 8, 9, 64)


def _ops():
    from vtc_amd import ops
    return ops


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _words(live):
    return None if live is None else _t(RG.pack_words(live).view(np.int32))


def _counts(nq, ng):
    """Hits asked of every query, in rotation: none, all, one, a few, about a third -- a query with no hits next to one with all rows."""
    kinds = (0, ng + 5, 1, 3, max(ng // 3, 1), 17)
    return np.array([kinds[i % len(kinds)] for i in range(nq)])


def _check(gallery, queries, counts, live=None, id_base=0, want_bits=0, radius2=None):
    """One l2_range_search against the reference: lims, ids, hit words exactly; dists within one fp32 ulp; dists64 to 1e-13 relative."""
    ops = _ops()
    wide = HR.widen(gallery) if gallery.dtype == np.float16 else gallery
    D = SR.distances64(wide, queries)
    r = RG.midpoint_radii(D, counts, live) if radius2 is None else np.asarray(radius2, np.float64)
    lims, ids, d64, member, margin = RG.range_lists(D, r, live, id_base)
    assert margin > 1e-12, margin
    got_lims, got_ids, got_d, got_d64, got_words = ops.l2_range_search(_t(gallery), _t(queries), _t(r), live=_words(live), id_base=id_base,
                                                                       return_dists64=True, return_words=True)
    assert got_lims.dtype == torch.int64 and got_ids.dtype == torch.int64 and got_d.dtype == torch.float32 and got_d64.dtype == torch.float64
    assert np.array_equal(got_lims.cpu().numpy(), lims), (got_lims.cpu().numpy(), lims)
    assert np.array_equal(got_ids.cpu().numpy(), ids)
    SR.assert_dists_within_one_ulp(got_d.cpu().numpy(), d64.astype(np.float32))
    assert np.allclose(got_d64.cpu().numpy(), d64, rtol=1e-13, atol=0)
    assert np.array_equal(got_d.cpu().numpy(), got_d64.cpu().numpy().astype(np.float32))       # dists = (float) D
    want_words = np.stack([RG.pack_words(m) for m in member])
    assert np.array_equal(got_words.cpu().numpy().view(np.uint32), want_words)
    lims_only, bits = ops.l2_range_count(_t(gallery), _t(queries), _t(r), live=_words(live), return_bits=True)
    assert torch.equal(lims_only, got_lims)                                                     # count alone = the lims of the full call
    assert int(bits.item()) == want_bits
    return got_lims, got_ids, got_d64


@pytest.fixture(scope="module")
def spread64():
    return RR.spread_pairs(1003, 64, 41)


@pytest.fixture(scope="module")
def large64():
    """(gallery [70 001, 64] with exact duplicates of row 5 in another word of the same workgroup's round (33), in other workgroups
    (40 000) and in the partial last word (69 999); queries [9, 64], query 0 near row 5)."""
    rng = np.random.default_rng(43)
    g = RR.unit(rng.standard_normal((70001, 64))).astype(np.float32)
    for j in (33, 40000, 69999):
        g[j] = g[5]
    q = RR.unit(rng.standard_normal((9, 64))).astype(np.float32)
    q[0] = RR.unit(g[5] + 0.05 * q[0]).astype(np.float32)
    q[4] = RR.unit(g[5] + 0.30 * q[4]).astype(np.float32)
    return g, q


# ---- 1. against numpy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ng", (1, 31, 32, 33, 257, 1003))
def test_edge_shapes_against_numpy(spread64, ng):
    a, b = spread64
    for nq in NQS:
        _check(a[:ng], b[:nq], _counts(nq, ng), id_base=(0 if nq % 2 else 10 ** 12))


@pytest.mark.parametrize("d", (320, 512))
def test_feature_widths(d):
    a, b = RR.spread_pairs(257, d, 45)
    for nq in (1, 5):
        _check(a, b[:nq], _counts(nq, 257))


@pytest.mark.parametrize("nq", (1, 9))
def test_several_workgroups_and_a_partial_last_word(large64, nq):
    g, q = large64
    lims, ids, _ = _check(g, q[:nq], np.array([40, 0, 70001, 3, 12, 1000, 1, 7, 25000])[:nq], id_base=7)
    assert int(lims[-1]) >= 40


def test_more_words_than_the_grid_has_waves():
    rng = np.random.default_rng(47)
    g = RR.unit(rng.standard_normal((300001, 64))).astype(np.float32)
    q = RR.unit(rng.standard_normal((9, 64))).astype(np.float32)
    live = rng.random(300001) < 0.7
    live[200000:260000] = False                                # whole words dead, deep in the second round of every wave
    _check(g, q, np.array([5, 0, 100, 3000, 1, 60, 2, 900, 11]))
    _check(g, q[:3], np.array([50, 2, 4000]), live=live)


# ---- 2. the boundary, against the device's own bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("half", (False, True), ids=("fp32", "half"))
def test_the_boundary_is_the_searchs_own_bits(large64, half):
    """radius2[q] = the fp64 distance of the k-th neighbour as vtc_l2_search left it in its workspace: the hits are exactly the search's
    entries with a distance <= it -- the first k and every row bit-equal to the k-th -- and one fp64 step below, the k-th and its ties
    are gone.  Query 0's four nearest rows are exact duplicates in different words, waves and workgroups."""
    ops = _ops()
    g, q = large64
    g = HR.round_half(g) if half else g
    tg, tq = _t(g), _t(q)
    ks = np.array([2, 11, 1, 40, 4, 3, 17, 5, 33])             # 2: inside query 0's group of four ties; 4 (query 4): at its end
    ws = ops.workspace(ops.l2_search_workspace_bytes(g.shape[0], 9, 64, 64), DEV)
    s_ids, _, _ = ops.l2_search(tg, tq, 64, ws=ws)
    s_ids, s_d64 = s_ids.cpu().numpy(), ops.search_dists64(ws, 9, 64).cpu().numpy().copy()
    assert set(s_ids[0, :4]) == {5, 33, 40000, 69999} and len(set(s_d64[0, :4])) == 1      # bit-equal on the device
    kth = s_d64[np.arange(9), ks - 1]
    for radius in (kth, np.nextafter(kth, -np.inf)):           # at the k-th neighbour's bits, and one fp64 step below
        lims, ids, _, d64 = ops.l2_range_search(tg, tq, _t(radius), return_dists64=True)
        lims, ids, d64 = lims.cpu().numpy(), ids.cpu().numpy(), d64.cpu().numpy()
        for i in range(9):
            want = s_d64[i] <= radius[i]
            assert not want[-1]                                # the 64 entries reach past the radius: nothing outside them can be a hit
            assert want[ks[i] - 1] == (radius is kth)          # the k-th itself: in at its own distance, out one step below
            got_ids, got_d = ids[lims[i]:lims[i + 1]], d64[lims[i]:lims[i + 1]]
            assert np.array_equal(got_ids, np.sort(s_ids[i, want])), i
            order = np.lexsort((got_ids, got_d))
            assert np.array_equal(got_ids[order], s_ids[i, want]) and np.array_equal(got_d[order], s_d64[i, want]), i     # bit-equal
            if radius is kth:
                assert got_ids.size >= ks[i] and set(s_ids[i, :ks[i]]) <= set(got_ids)
            else:
                assert got_ids.size < ks[i] and not np.any(got_d == kth[i])
    assert int(np.sum(s_d64[0] <= kth[0])) == 4                # k = 2 inside the four ties: all four came back above


# ---- 3. masks -----------------------------------------------------------------------------------------------------------------------
def test_masks(spread64):
    a, b = spread64
    rng = np.random.default_rng(49)
    live = rng.random(1003) < 0.5
    live[64:160] = False                                       # three entirely dead words
    live[320:352] = True                                       # an entirely live one
    _check(a, b[:9], _counts(9, 1003), live=live)
    _check(a, b[:2], np.array([1003, 4]), live=live)
    bad = a.copy()
    bad[70] = np.nan                                           # a dead row in a dead word, and one in a partly live word
    dead_in_live_word = int(np.flatnonzero(~live[:64])[0])
    bad[dead_in_live_word, 3] = np.inf
    _check(bad, b[:5], np.array([1003, 3, 0, 50, 1003]), live=live, want_bits=0)


def test_everything_dead(spread64):
    ops = _ops()
    a, b = spread64
    dead = np.zeros(1003, bool)
    lims, ids, d, words = ops.l2_range_search(_t(a), _t(b[:9]), float("inf"), live=_words(dead), return_words=True)
    assert torch.equal(lims, torch.zeros(10, dtype=torch.int64, device=DEV)) and ids.numel() == 0 and d.numel() == 0
    assert not bool(words.any())
    # fill writes nothing: canaries over the whole output
    canary = torch.full((16,), -77, dtype=torch.int64, device=DEV)
    _raw_fill(a, b[:9], float("inf"), dead, capacity=16, ids=canary)
    assert bool((canary == -77).all())


# ---- 4. half ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ng,nq", ((64, 257, 9), (320, 257, 3), (64, 33, 1), (512, 257, 2)))
def test_a_half_gallery_gives_the_bits_of_the_widened_rows(d, ng, nq):
    ops = _ops()
    g, q = HR.shape_case(d, ng, nq, 1)                         # subnormal halves, +-65504, -0.0, duplicates in the first rows
    D = SR.distances64(HR.widen(g), q)
    r = _t(RG.midpoint_radii(D, _counts(nq + 1, ng)[1:]))          # from "every row" on: no case without a hit
    live = np.random.default_rng(51).random(ng) < 0.8
    for lv in (None, live):
        h = ops.l2_range_search(_t(g), _t(q), r, live=_words(lv), return_dists64=True, return_words=True)
        w = ops.l2_range_search(_t(HR.widen(g)), _t(q), r, live=_words(lv), return_dists64=True, return_words=True)
        assert all(torch.equal(x, y) for x, y in zip(h, w))
        assert int(h[0][-1]) > 0
    _check(g, q, _counts(nq, ng))                              # and against numpy over the widened rows


# ---- 5. non-finite ------------------------------------------------------------------------------------------------------------------
def test_nonfinite_rows_queries_and_radii(spread64):
    a, b = spread64
    g = a[:257].copy()
    g[40, 5] = np.nan
    g[256, 63] = -np.inf
    _check(g, b[:5], np.array([257, 3, 0, 50, 1]), want_bits=1)
    q = b[:9].copy()
    q[1, 0] = np.nan
    q[8, 63] = np.inf                                          # in the second tile
    lims, _, _ = _check(a[:257], q, np.full(9, 300), want_bits=2, radius2=np.full(9, np.inf))
    assert np.array_equal(np.diff(lims.cpu().numpy()), [257, 0, 257, 257, 257, 257, 257, 257, 0])
    _check(g, q, None, want_bits=3, radius2=np.full(9, np.inf))
    D = SR.distances64(a[:257], b[:6])
    r = np.array([np.nan, -1.0, np.inf, -np.inf, RG.midpoint_radii(D[4:5], 7)[0], -0.0])
    lims, _, _ = _check(a[:257], b[:6], None, radius2=r)
    assert np.array_equal(np.diff(lims.cpu().numpy()), [0, 0, 257, 0, 7, 0])


# ---- 6. capacity --------------------------------------------------------------------------------------------------------------------
def _raw_fill(gallery, queries, radius2, live, capacity, ids, dists=None, dists64=None, id_base=0):
    """count through ops on a workspace of the caller's, then vtc_l2_range_fill itself with the given capacity and outputs."""
    from vtc_amd import _lib as L
    ops = _ops()
    tg, tq = _t(gallery), _t(queries)
    ws = ops.workspace(ops.l2_range_workspace_bytes(tg.shape[0], tq.shape[0], tg.shape[1]), DEV)
    lims = ops.l2_range_count(tg, tq, radius2, live=_words(live), ws=ws)
    ptr = lambda x: None if x is None else x.data_ptr()       # noqa: E731
    L.check(L.lib().vtc_l2_range_fill(tg.data_ptr(), int(tg.dtype == torch.float16), tq.data_ptr(), tg.shape[0], tq.shape[0], tg.shape[1],
                                      lims.data_ptr(), capacity, id_base, ptr(ids), ptr(dists), ptr(dists64), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream().cuda_stream), "vtc_l2_range_fill")
    torch.cuda.synchronize()
    return lims


def test_capacity_truncates_and_never_writes_past_it(spread64):
    ops = _ops()
    a, b = spread64
    D = SR.distances64(a, b[:5])
    r = RG.midpoint_radii(D, np.array([30, 0, 400, 5, 1003]))
    lims, ids, d, d64 = ops.l2_range_search(_t(a), _t(b[:5]), _t(r), return_dists64=True)
    total = int(lims[-1])
    for cap in (0, 1, 31, 437, total - 1, total):
        got_i = torch.full((total + 64,), -77, dtype=torch.int64, device=DEV)
        got_d = torch.full((total + 64,), -77.0, dtype=torch.float32, device=DEV)
        got_d64 = torch.full((total + 64,), -77.0, dtype=torch.float64, device=DEV)
        got_lims = _raw_fill(a, b[:5], _t(r), None, cap, got_i, got_d, got_d64)
        assert torch.equal(got_lims, lims)
        assert torch.equal(got_i[:cap], ids[:cap]) and torch.equal(got_d[:cap], d[:cap]) and torch.equal(got_d64[:cap], d64[:cap])
        assert bool((got_i[cap:] == -77).all()) and bool((got_d[cap:] == -77).all()) and bool((got_d64[cap:] == -77).all())
    only_ids = torch.full((total + 8,), -77, dtype=torch.int64, device=DEV)      # dists and dists64 may be NULL
    _raw_fill(a, b[:5], _t(r), None, total, only_ids)
    assert torch.equal(only_ids[:total], ids) and bool((only_ids[total:] == -77).all())


# ---- 8. hit words as a mask of the search ---------------------------------------------------------------------------------------------
def test_hit_words_are_a_live_mask_of_the_search(spread64):
    ops = _ops()
    a, b = spread64
    D = SR.distances64(a, b[:3])
    r = RG.midpoint_radii(D, np.array([200, 40, 7]))
    ta = _t(a)
    lims, ids, d, d64, words = ops.l2_range_search(ta, _t(b[:3]), _t(r), return_dists64=True, return_words=True)
    for i in range(3):
        other = _t(b[10 + i:11 + i])                           # another query: its nearest 5 among query i's hits
        got_ids, got_d, _ = ops.l2_search(ta, other, 5, live=words[i])
        members = np.zeros(1003, bool)
        members[ids[lims[i]:lims[i + 1]].cpu().numpy()] = True
        want_ids, want_d, _ = ops.l2_search(ta, other, 5, live=_words(members))
        assert torch.equal(got_ids, want_ids) and torch.equal(got_d, want_d) and bool(members[got_ids.cpu().numpy()].all())


# ---- 9. max_results -------------------------------------------------------------------------------------------------------------------
def test_max_results_raises_before_the_result_is_allocated(large64):
    ops = _ops()
    g, q = large64
    tg, tq = _t(g), _t(q[:8])
    ws = ops.workspace(ops.l2_range_workspace_bytes(70001, 8, 64), DEV)
    r = torch.full((8,), float("inf"), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="max_results"):
        ops.l2_range_search(tg, tq, r, max_results=8 * 70001 - 1, ws=ws)
    assert torch.cuda.max_memory_allocated() - before < 64 << 10          # lims and the flag word, not 8 x 70 001 ids and dists
    lims, ids, d = ops.l2_range_search(tg, tq, r, max_results=8 * 70001, ws=ws)
    assert int(lims[-1]) == 8 * 70001 and torch.equal(ids.view(8, 70001), torch.arange(70001, device=DEV).expand(8, 70001))
    with pytest.raises(ValueError, match="workspace"):
        ops.l2_range_search(tg, tq, r, ws=ws[:ws.numel() // 2])


# ---- 10. VideoIndex -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw_rows():
    rng = np.random.default_rng(53)
    a, b = RR.spread_pairs(1027, 100, 25)                      # 100 columns: padded to 128
    scale = np.exp(rng.uniform(-1, 1, (1027, 1))).astype(np.float32)
    return (a * scale).astype(np.float32), (b * scale).astype(np.float32)


def _index_reference(index, queries, min_score, live=None):
    """The reference over the index's stored rows and prepared queries: (lims, ids by row, ids nearest first, member, margin)."""
    g = index.rows.float().cpu().numpy()
    q = index._prepared(queries, "queries", check=False).cpu().numpy()
    r = 2.0 * (1.0 - np.broadcast_to(np.asarray(min_score, np.float64), (q.shape[0],)))
    D = SR.distances64(g, q)
    lims, ids, d64, member, margin = RG.range_lists(D, r, live)
    by_dist = np.concatenate([ids[lims[i]:lims[i + 1]][np.lexsort((ids[lims[i]:lims[i + 1]], d64[lims[i]:lims[i + 1]]))]
                              for i in range(q.shape[0])]) if ids.size else ids
    return lims, ids, by_dist, d64, margin


def _scores_for_counts(index, queries, counts, live=None):
    """min_score per query such that about counts[q] rows score at least it, halfway between two reference scores."""
    g = index.rows.float().cpu().numpy()
    q = index._prepared(queries, "queries", check=False).cpu().numpy()
    return 1.0 - RG.midpoint_radii(SR.distances64(g, q), counts, live) / 2.0


@pytest.mark.parametrize("storage", (torch.float32, torch.float16), ids=("fp32", "half"))
def test_video_index_range_search(raw_rows, storage):
    from vtc_amd.host.search import VideoIndex
    a, b = raw_rows
    index = VideoIndex(100, device=DEV, storage=storage)
    index.add(_t(a[:700]))
    index.add(_t(a[700:]))
    keys = set(index.state_dict())
    assert keys == ({"rows", "count", "dim", "normalized"} | ({"storage"} if storage == torch.float16 else set()))
    q = _t(b[:70])                                             # more than 64 queries: two calls, lims concatenated
    scores = _scores_for_counts(index, q, np.array([_counts(70, 1027)[i] if i % 7 else 25 for i in range(70)]))
    want_lims, want_ids, want_sorted, want_d64, margin = _index_reference(index, q, scores)
    assert margin > 1e-12
    lims, ids, sc = index.range_search(q, scores.tolist())
    assert lims.dtype == torch.int64 and ids.dtype == torch.int64 and sc.dtype == torch.float32 and lims.is_cuda and ids.is_cuda and sc.is_cuda
    assert np.array_equal(lims.cpu().numpy(), want_lims) and np.array_equal(ids.cpu().numpy(), want_sorted)
    lims_u, ids_u, sc_u = index.range_search(q, scores.tolist(), sort=False)
    assert np.array_equal(lims_u.cpu().numpy(), want_lims) and np.array_equal(ids_u.cpu().numpy(), want_ids)
    # score = 1 - d / 2 in fp32 of a d within one fp32 ulp of the reference's (d < 4: ulp <= 2^-22, halved) plus the score's own rounding
    # (|score| <= 1: 2^-24): 1.2e-7 + 6e-8 < 2e-7.  Bit-equality with search()'s scores is asserted below.
    assert float(np.abs(sc_u.cpu().numpy().astype(np.float64) - (1.0 - want_d64 / 2.0)).max()) <= 2e-7
    for i in (0, 5, 69):                                       # nearest first: the scores of a segment descend
        seg = sc[lims[i]:lims[i + 1]]
        assert bool((seg[1:] <= seg[:-1]).all())
    assert torch.equal(index.range_count(q, scores.tolist()), lims[1:] - lims[:-1])
    # a scalar min_score, and the segment of a query IS search()'s first rows
    s0 = float(_scores_for_counts(index, q[:1], 9)[0])
    lims1, ids1, sc1 = index.range_search(q[:3], s0)
    n0 = int(lims1[1])
    assert n0 >= 9
    top_ids, top_sc = index.search(q[:1], n0)
    assert torch.equal(ids1[:n0], top_ids[0]) and torch.equal(sc1[:n0], top_sc[0])
    assert torch.equal(index.range_count(q[:3], s0), lims1[1:] - lims1[:-1])
    # the existing methods and the state are what they were
    assert set(index.state_dict()) == keys and len(index) == 1027 and index.ntotal == 1027
    with pytest.raises(ValueError, match="max_results"):
        index.range_search(q, scores.tolist(), max_results=int(lims[-1]) - 1)
    with pytest.raises(ValueError, match="min_score"):
        index.range_search(q, [0.5, 0.5])


@pytest.mark.parametrize("storage", (torch.float32, torch.float16), ids=("fp32", "half"))
def test_video_index_range_search_after_remove_and_with_a_subset(raw_rows, storage):
    from vtc_amd.host.search import VideoIndex
    a, b = raw_rows
    rng = np.random.default_rng(55)
    index = VideoIndex(100, device=DEV, storage=storage)
    index.add(_t(a))
    q = _t(b[:9])
    gone = np.unique(rng.integers(0, 1027, 300))
    index.remove(torch.from_numpy(gone))
    live = np.ones(1027, bool)
    live[gone] = False
    scores = _scores_for_counts(index, q, _counts(9, 1027), live)
    want_lims, want_ids, want_sorted, _, margin = _index_reference(index, q, scores, live)
    assert margin > 1e-12
    lims, ids, _ = index.range_search(q, scores)
    assert np.array_equal(lims.cpu().numpy(), want_lims) and np.array_equal(ids.cpu().numpy(), want_sorted)
    assert torch.equal(index.range_count(q, scores), lims[1:] - lims[:-1])
    members = rng.random(1027) < 0.4
    sub = index.subset(torch.from_numpy(members))
    both = live & members
    scores = _scores_for_counts(index, q, _counts(9, 1027), both)
    want_lims, want_ids, want_sorted, _, margin = _index_reference(index, q, scores, both)
    assert margin > 1e-12
    lims, ids, _ = index.range_search(q, scores, subset=sub, sort=False)
    assert np.array_equal(lims.cpu().numpy(), want_lims) and np.array_equal(ids.cpu().numpy(), want_ids)
    assert torch.equal(index.range_count(q, scores, subset=sub), lims[1:] - lims[:-1])
    # range_subset: the nearest k among the rows scoring at least s = the first k of the sorted range result; and it chains
    s = float(_scores_for_counts(index, q[2:3], 40, live)[0])
    lims, ids, sc = index.range_search(q[2:3], s)
    near = index.range_subset(q[2], s)
    top_ids, top_sc = index.search(q[2:3], 7, subset=near)
    assert int(lims[1]) >= 40 and torch.equal(top_ids[0], ids[:7]) and torch.equal(top_sc[0], sc[:7])
    other_ids, _ = index.search(q[3:4], 5, subset=near)        # another query inside those rows
    assert bool(torch.isin(other_ids, ids).all())
    chained = index.range_subset(q[2:3], s, subset=sub)
    lims_c, ids_c, _ = index.range_search(q[2:3], -1.0, subset=chained, sort=False)
    assert np.array_equal(ids_c.cpu().numpy(), np.sort(ids.cpu().numpy()[members[ids.cpu().numpy()]]))
    index.remove(ids[:1])                                      # a subset built from hit words follows a later removal, as every RowSubset
    top_ids2, _ = index.search(q[2:3], 6, subset=near)
    assert torch.equal(top_ids2[0], ids[1:7])
    with pytest.raises(ValueError, match="subset"):
        index.range_search(q, 0.5, subset=VideoIndex(100, device=DEV).subset([]))
    with pytest.raises(ValueError, match="one query"):
        index.range_subset(q[:2], 0.5)


def test_video_index_does_not_sync_in_range_count_and_range_subset(raw_rows):
    from vtc_amd.host.search import VideoIndex
    a, b = raw_rows
    index = VideoIndex(100, device=DEV)
    index.add(_t(a))
    q = _t(b[:3])
    want = index.range_count(q, 0.2)                           # (warm: workspace allocated)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = index.range_count(q, 0.2)
        near = index.range_subset(q[0], 0.2)
        ids, _ = index.search(q[:1], 3, subset=near)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got, want) and int(want.sum()) > 0 and ids.shape == (1, 3)


def test_video_index_range_search_text():
    from oracle import arch as A
    from vtc_amd.host import model as HM
    from vtc_amd.host.clip_arch import ClipConfig
    from vtc_amd.host.search import VideoIndex
    torch.set_grad_enabled(False)
    arch = A.TINY
    m = HM.PretrainedCLIP(model_type=ClipConfig(**asdict(arch)))
    m.load_state_dict(A.synth_model(arch, 7, "clip"), strict=True)
    m = m.eval().to(DEV)
    dim = arch.embed_dim
    rng = np.random.default_rng(32)
    index = VideoIndex(dim, device=DEV)
    index.add(_t(rng.standard_normal((200, dim)).astype(np.float32)))
    tokens = A.synth_tokens(5, arch, 9).to(DEV)
    feats = index._text_queries(m, tokens, None, "range_search_text")
    score = float(index.search(feats, 10)[1][:, -1].min()) - 1e-4      # every query has at least its 10 nearest above it
    for kw in ({}, {"sort": False}):
        got = index.range_search_text(m, tokens, score, **kw)
        want = index.range_search(feats, score, **kw)
        assert all(torch.equal(x, y) for x, y in zip(got, want)) and int(got[0][-1]) >= 50
