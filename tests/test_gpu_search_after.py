"""GPU: the cursor search -- vtc_l2_search_after / ops.l2_search(after=...), vtc_l2_pair_dists64 / ops.l2_pair_dists64,
VideoIndex.search(after=...) / search_deep, dist.sharded_search(after=...) -- against the numpy reference of tests/search_after_refs.py
(the full (fp64 distance, row) order of the live finite rows, cut after the cursor's key) and bit for bit against the library's own
plain search: pages chained by their last key are, concatenated, ONE deeper search.

Ids are compared with exact equality; every comparison with the reference asserts its min_gap > 1e-12 first, over the FULL order (a page
can begin anywhere).  fp32 dists are within one fp32 ulp of the reference and bit-equal between the library's entry points."""
import numpy as np
import pytest
import torch

import rank_refs as RR
import search_after_refs as AR
import search_mask_refs as MR
import search_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NEG_INF, INF = float("-inf"), float("inf")


def _ops():
    from vtc_amd import ops
    return ops


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _words(live):
    return None if live is None else _t(MR.pack_words(live).view(np.int32))


@pytest.fixture(scope="module")
def data():
    """1027 x 64 spread rows as fp32 and rounded to half: numpy (the half rows widened again, what the reference sees) and device."""
    a, b = RR.spread_pairs(1027, 64, 21)
    ah = a.astype(np.float16)
    return {"np": {"float32": a, "float16": ah.astype(np.float32)}, "t": {"float32": _t(a), "float16": _t(ah)}, "b": b, "tb": _t(b)}


def _search(g, q, depth, after=None, live=None, id_base=0):
    """One call in a workspace of its own: (ids, dists, fp64 dists, nonfinite bits)."""
    ops = _ops()
    ws = ops.workspace(ops.l2_search_workspace_bytes(g.shape[0], q.shape[0], g.shape[1], depth), g.device)
    ids, dists, bits = ops.l2_search(g, q, depth, id_base=id_base, ws=ws, live=live, after=after)
    return ids, dists, ops.search_dists64(ws, q.shape[0], depth).clone(), bits


def _chain(g, q, depth, pages, live=None, first_after=None):
    """`pages` pages of `depth`, each after the last key of the one before; the first is the plain search unless given a cursor."""
    out, after = [], first_after
    for _ in range(pages):
        ids, dists, d64, _ = _search(g, q, depth, after=after, live=live)
        out.append((ids, dists, d64))
        after = (d64[:, -1].clone(), ids[:, -1].clone())
    return tuple(torch.cat([o[i] for o in out], dim=1) for i in range(3))


def _assert_empty(ids, dists):
    assert bool((ids == -1).all()) and bool(torch.isposinf(dists).all())


# ---- 1. pages equal one search, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 2, 3, 5, 9, 64])           # every tile shape, two tiles, eight tiles
@pytest.mark.parametrize("ng", [65, 257, 1027])
def test_four_pages_of_16_are_one_search_of_64(data, ng, nq):
    q = data["tb"][:nq]
    for storage in ("float32", "float16"):
        g = data["t"][storage][:ng]
        for live in (None, MR.make_mask("random_0.5", ng, seed=ng)):
            words = _words(live)
            ids, dists, d64 = _chain(g, q, 16, 4, live=words)
            want_ids, want_dists, want_d64, _ = _search(g, q, 64, live=words)
            assert torch.equal(ids, want_ids) and torch.equal(dists, want_dists) and torch.equal(d64, want_d64), (storage, live is None)
            n_live = ng if live is None else int(live.sum())  # 65 rows, half of them live: the chain ran past the end and stayed empty
            assert bool((ids[:, n_live:] == -1).all()) and bool((ids[:, :min(n_live, 64)] >= 0).all())


# ---- 2. beyond 64, against numpy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["float32", "float16"])
@pytest.mark.parametrize("ng,depth", [(1027, 64), (1, 1), (2, 2), (63, 11), (64, 11)])
def test_pages_until_exhausted_are_the_full_order(data, storage, ng, depth):
    nq = 3
    g, q = data["t"][storage][:ng], data["tb"][:nq]
    want_ids, want_d64, gap = AR.full_order(data["np"][storage][:ng], data["b"][:nq])
    assert gap > 1e-12, gap
    pages = -(-ng // depth)                                   # 17 for 1027 rows in pages of 64
    ids, dists, d64 = _chain(g, q, depth, pages)
    assert ng != 1027 or pages == 17
    assert np.array_equal(ids[:, :ng].cpu().numpy(), want_ids)
    SR.assert_dists_within_one_ulp(dists[:, :ng].cpu().numpy(), want_d64.astype(np.float32))
    # fp64 sums of 64 terms of a D <= 4: any summation order is within 64 * 2^-53 * 4 < 1e-13 of any other
    assert bool((d64[:, :ng].cpu() - torch.from_numpy(want_d64)).abs().max() <= 1e-13)
    _assert_empty(ids[:, ng:], dists[:, ng:])                 # the last page ends in -1 / +inf when ng is no multiple of depth
    assert ng % depth == 0 or bool((ids[:, -1] == -1).all())
    more = _search(g, q, depth, after=(d64[:, -1].clone(), ids[:, -1].clone()))
    _assert_empty(more[0], more[1])
    assert bool(torch.isposinf(more[2]).all())
    if ng % depth == 0:                                       # a full last page: its key is the order's last, nothing comes after it
        assert bool((ids[:, -1] >= 0).all())


# ---- 3. exact ties ----------------------------------------------------------------------------------------------------------------------
def test_cursors_inside_runs_of_bit_equal_distances(data):
    g_np = AR.tied_gallery(data["np"]["float32"][:200], 21)    # 1000 rows, every distance five times
    nq = 5
    want_ids, want_d64, gap = AR.full_order(g_np, data["b"][:nq])
    assert gap > 1e-12, gap
    assert (want_d64[:, 1:] == want_d64[:, :-1]).mean() > 0.7
    ids, dists, d64 = _chain(_t(g_np), data["tb"][:nq], 3, 334)
    assert np.array_equal(ids[:, :1000].cpu().numpy(), want_ids)
    _assert_empty(ids[:, 1000:], dists[:, 1000:])
    d64 = d64[:, :1000].cpu().numpy()
    assert np.array_equal(d64[:, 1:] == d64[:, :-1], want_d64[:, 1:] == want_d64[:, :-1])      # the device's ties are the reference's


# ---- 4. cursor bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["float32", "float16"])
@pytest.mark.parametrize("nq", [1, 2, 3, 5, 9, 64])
def test_pair_distance_has_the_bits_the_scan_leaves(data, storage, nq):
    """The invariant that keeps the cursor row from coming back and its successor from being skipped."""
    ops = _ops()
    g, q = data["t"][storage], data["tb"][:nq]
    for live, id_base, ng in ((None, 0, 1027), (None, 1000, 257), (MR.make_mask("random_0.05", 65, seed=2), 7, 65)):
        ids, _, d64, _ = _search(g[:ng], q, 11, live=_words(live), id_base=id_base)
        if live is not None:
            assert bool((ids[:, -1] == -1).all())             # fewer than 11 live rows: the empty entries are +inf on both sides
        for j in range(11):
            got = ops.l2_pair_dists64(g[:ng], q, ids[:, j], id_base=id_base)
            assert got.dtype == torch.float64 and torch.equal(got, d64[:, j]), (j, id_base)


def test_pair_distance_of_no_row_is_inf_and_dead_rows_are_read(data):
    ops = _ops()
    g, q = data["t"]["float32"][:257], data["tb"][:6]
    rows = torch.tensor([-1, 257, 256, 0, 2 ** 40, -2 ** 62], dtype=torch.int64, device=DEV)
    got = ops.l2_pair_dists64(g, q, rows).cpu().numpy()
    D = SR.distances64(data["np"]["float32"][:257], data["b"][:6])
    assert np.isposinf(got[[0, 1, 4, 5]]).all()
    assert abs(got[2] - D[2, 256]) <= 1e-13 and abs(got[3] - D[3, 0]) <= 1e-13
    got = ops.l2_pair_dists64(g, q, rows + 50, id_base=50).cpu().numpy()
    assert np.isposinf(got[[0, 1, 4, 5]]).all() and abs(got[2] - D[2, 256]) <= 1e-13


@pytest.mark.parametrize("d", [192, 512, 2048])               # one, two and eight 256-column slices a lane walks
def test_feature_widths(d):
    ops = _ops()
    a, b = RR.spread_pairs(300, d, 22)
    for g in (_t(a), _t(a.astype(np.float16))):
        for nq in (1, 9):
            q = _t(b[:nq])
            ids, dists, d64 = _chain(g, q, 32, 2)
            want = _search(g, q, 64)
            assert torch.equal(ids, want[0]) and torch.equal(dists, want[1]) and torch.equal(d64, want[2])
            assert torch.equal(ops.l2_pair_dists64(g, q, ids[:, 40]), d64[:, 40])


# ---- 5. cursor values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 2, 3, 5, 9, 64])
def test_minus_inf_is_the_plain_search_and_plus_inf_or_nan_admit_nothing(data, nq):
    q = data["tb"][:nq]
    ci = torch.full((nq,), -1, dtype=torch.int64, device=DEV)
    for storage in ("float32", "float16"):
        g = data["t"][storage][:257]
        for live in (None, MR.make_mask("random_0.5", 257, seed=9)):
            words = _words(live)
            plain = _search(g, q, 11, live=words)
            got = _search(g, q, 11, live=words, after=(torch.full((nq,), NEG_INF, dtype=torch.float64, device=DEV), ci))
            for x, y in zip(got, plain):
                assert torch.equal(x, y)
            # per query in rotation: -inf, +inf, NaN -- the neighbours of an empty row are not touched
            cd = torch.tensor([(NEG_INF, INF, float("nan"))[u % 3] for u in range(nq)], dtype=torch.float64, device=DEV)
            ids, dists, d64, _ = _search(g, q, 11, live=words, after=(cd, ci))
            for u in range(nq):
                if u % 3 == 0:
                    assert torch.equal(ids[u], plain[0][u]) and torch.equal(dists[u], plain[1][u]) and torch.equal(d64[u], plain[2][u])
                else:
                    _assert_empty(ids[u], dists[u])
                    assert bool(torch.isposinf(d64[u]).all())


def test_nan_query_and_nonfinite_bits_match_the_masked_search(data):
    g_np = data["np"]["float32"][:257].copy()
    live = MR.make_mask("random_0.5", 257, seed=4)
    g_np[np.flatnonzero(live)[5], 2] = np.inf                  # a live row without a distance: bit 0
    g_np[np.flatnonzero(~live)[5], 2] = np.nan                 # a dead one: nothing
    q_np = data["b"][:5].copy()
    q_np[3, 7] = np.nan                                        # bit 1
    g, q, words = _t(g_np), _t(q_np), _words(live)
    masked = _search(g, q, 11, live=words)
    assert int(masked[3].item()) == 3
    after = (masked[2][:, 4].clone(), masked[0][:, 4].clone())
    ids, dists, d64, bits = _search(g, q, 6, live=words, after=after)
    assert int(bits.item()) == int(masked[3].item())
    _assert_empty(ids[3], dists[3])
    keep = [0, 1, 2, 4]
    assert torch.equal(ids[keep], masked[0][keep, 5:]) and torch.equal(dists[keep], masked[1][keep, 5:])
    assert torch.equal(d64[keep], masked[2][keep, 5:])


# ---- 6. windows -----------------------------------------------------------------------------------------------------------------------
def test_windows_take_the_same_cursor(data):
    from vtc_amd import dist
    ops = _ops()
    nq, depth = 3, 40
    g_np, g, q = data["np"]["float32"], data["t"]["float32"], data["tb"][:3]
    cuts = [0, 400, 800, 1027]
    order, order_d64, gap = AR.full_order(g_np, data["b"][:nq])
    assert gap > 1e-12, gap
    for w in range(3):                                        # the cursor row in the first, the middle, the last window
        pos = [next(p for p in range(5, 1027) if cuts[w] <= order[u, p] < cuts[w + 1]) for u in range(nq)]
        ci = _t(np.array([order[u, pos[u]] for u in range(nq)], np.int64))
        cd = ops.l2_pair_dists64(g, q, ci)
        whole = _search(g, q, depth, after=(cd, ci))
        for u in range(nq):
            assert np.array_equal(whole[0][u].cpu().numpy(), order[u, pos[u] + 1:pos[u] + 1 + depth])
        parts = [ops.l2_search_part(g[lo:hi], q, depth, id_base=lo, after=(cd, ci))[:2] for lo, hi in zip(cuts[:-1], cuts[1:])]
        ids, dists = ops.l2_search_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
        assert torch.equal(ids, whole[0]) and torch.equal(dists, whole[1])
        ids, dists, d64 = dist.sharded_search(g, 0, q, depth, 0, 1, after=(cd, ci), return_dists64=True)
        assert torch.equal(ids, whole[0]) and torch.equal(dists, whole[1]) and torch.equal(d64, whole[2])
        # a window's own id_base moves the ids and the cursor alike
        ids, _, d64, _ = _search(g, q, depth, after=(cd, ci + 5000), id_base=5000)
        assert torch.equal(ids, whole[0] + 5000) and torch.equal(d64, whole[2])
    ids, dists = dist.sharded_search(g, 0, q, depth, 0, 1)    # without the new arguments: what it returned before
    plain = _search(g, q, depth)
    assert torch.equal(ids, plain[0]) and torch.equal(dists, plain[1])


# ---- 7. VideoIndex, in pages of 5 -------------------------------------------------------------------------------------------------------
def _index_order(index, queries, live=None):
    """The reference's full order over the index's STORED rows and prepared queries."""
    g = index.rows.float().cpu().numpy()
    q = index._prepared(queries, "queries", check=False).cpu().numpy()
    return g, q


def _assert_scores(scores, ids, want_d64):
    """score = 1 - D / 2 in fp32 from the fp32 D: D <= 4 rounds to fp32 within 2.4e-7, one more ulp (4.8e-7) for the summation order of
    the reference, halved, plus the rounding of a score of magnitude <= 1 (6e-8): below 5e-7."""
    s = scores.cpu().numpy().astype(np.float64)
    full = ids.cpu().numpy() >= 0
    assert np.isneginf(s[~full]).all()
    assert np.abs(s[full] - (1.0 - want_d64[full] / 2.0)).max() < 5e-7


@pytest.mark.parametrize("storage", [torch.float32, torch.float16])
def test_video_index_pages_survive_remove_and_subset(data, storage):
    from vtc_amd.host.search import VideoIndex
    nq = 70                                                   # two slices of queries
    index = VideoIndex(64, device=DEV, storage=storage)
    index.add(data["t"]["float32"])
    queries = data["tb"][:nq]
    g, q = _index_order(index, queries)
    page1, _ = index.search(queries, 5)
    cursor = page1[:, -1].clone()
    # a subset without the cursor rows, every row still live
    member = np.ones(1027, bool)
    member[cursor.cpu().numpy()] = False
    member[::7] = False
    want_ids, want_d64, gap = AR.reference_search_after(g, q, 5, cursor.cpu().numpy(), live=member)
    assert gap > 1e-12, gap
    ids, scores = index.search(queries, 5, subset=index.subset(torch.from_numpy(member)), after=cursor)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    _assert_scores(scores, ids, want_d64)
    # the cursor rows removed: the page token still stands
    assert index.remove(cursor) == len(set(cursor.tolist()))
    live = index.live_mask.cpu().numpy()
    want_ids, want_d64, gap = AR.reference_search_after(g, q, 5, cursor.cpu().numpy(), live=live)
    assert gap > 1e-12, gap
    ids, scores = index.search(queries, 5, after=cursor)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    _assert_scores(scores, ids, want_d64)
    ids3, _ = index.search(queries, 5, after=ids[:, -1])      # and the page after that
    want3, _, _ = AR.reference_search_after(g, q, 5, want_ids[:, -1], live=live)
    assert np.array_equal(ids3.cpu().numpy(), want3)


def test_video_index_ids_that_are_no_row_give_empty_rows(data):
    from vtc_amd.host.search import VideoIndex
    index = VideoIndex(64, device=DEV)
    index.add(data["t"]["float32"][:257])
    queries = data["tb"][:4]
    page1, _ = index.search(queries, 5)
    after = page1[:, -1].clone()
    good, _ = index.search(queries, 5, after=after)
    after[1], after[2] = -1, index.ntotal + 5
    ids, scores = index.search(queries, 5, after=after)
    assert bool((ids[1:3] == -1).all()) and bool(torch.isneginf(scores[1:3]).all())
    assert torch.equal(ids[[0, 3]], good[[0, 3]]) and bool((ids[[0, 3]] >= 0).all())
    with pytest.raises(ValueError):
        index.search(queries, 5, after=after[:3])
    with pytest.raises(ValueError):
        index.search(queries, 5, after=after.to(torch.int32))
    with pytest.raises(ValueError):
        index.search(queries, 65, after=after)


# ---- 8. search_deep ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [2, 13])                       # 13: page 1 takes the vtc_l2_topk route
def test_search_deep_200(data, nq):
    from vtc_amd.host.search import VideoIndex
    assert 2 < VideoIndex.ROUTE_TOPK_MIN_QUERIES <= 13
    index = VideoIndex(64, device=DEV)
    index.add(data["t"]["float32"])
    queries = data["tb"][100:100 + nq]
    g, q = _index_order(index, queries)
    want_ids, want_d64, gap = AR.full_order(g, q)
    assert gap > 1e-12, gap
    ids, scores = index.search_deep(queries, 200)
    assert tuple(ids.shape) == (nq, 200) and ids.dtype == torch.int64 and scores.dtype == torch.float32
    assert np.array_equal(ids.cpu().numpy(), want_ids[:, :200])
    _assert_scores(scores, ids, want_d64[:, :200])
    first = index.search(queries, 64)
    assert torch.equal(ids[:, :64], first[0]) and torch.equal(scores[:, :64], first[1])
    short = index.search_deep(queries, 7)                     # k <= 64: the plain search, nothing else
    assert torch.equal(short[0], first[0][:, :7])


def test_search_deep_subset_runs_out_and_k_is_bounded(data):
    from vtc_amd.host.search import VideoIndex
    index = VideoIndex(64, device=DEV, storage=torch.float16)
    index.add(data["t"]["float32"][:257])
    queries = data["tb"][:3]
    g, q = _index_order(index, queries)
    member = MR.make_mask("random_0.5", 257, seed=8)
    want_ids, _, gap = AR.full_order(g, q, live=member)
    assert gap > 1e-12, gap
    ids, scores = index.search_deep(queries, 257, subset=index.subset(torch.from_numpy(member)))
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert bool((ids[:, member.sum():] == -1).all()) and bool(torch.isneginf(scores[:, member.sum():]).all())
    for k in (0, 258):
        with pytest.raises(ValueError):
            index.search_deep(queries, k)
    index.remove([3])
    with pytest.raises(ValueError):
        index.search_deep(queries, 257)                       # k counts live rows
    with pytest.raises(ValueError):
        index.search(queries, 65)                             # search() keeps its limit


# ---- 9. no host sync --------------------------------------------------------------------------------------------------------------------
def test_cursor_search_and_search_deep_do_not_sync(data):
    from vtc_amd.host.search import VideoIndex
    index = VideoIndex(64, device=DEV)
    index.add(data["t"]["float32"])
    q = data["tb"][:2]
    page1, _ = index.search(q, 5)
    after = page1[:, -1].clone()
    want = index.search(q, 5, after=after)                    # (warm: workspace allocated)
    want_deep = index.search_deep(q, 200)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = index.search(q, 5, after=after)
        got_deep = index.search_deep(q, 200)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(got_deep[0], want_deep[0]) and torch.equal(got_deep[1], want_deep[1])


# ---- the document's example ---------------------------------------------------------------------------------------------------------
def test_the_integration_documents_block_runs_as_written():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "search_deep" in b]
    assert len(blocks) == 1, len(blocks)
    ns = {}
    exec(blocks[0], ns)                                       # its own assert: two pages are the head of the deep ranking
    assert tuple(ns["deep_ids"].shape) == (3, 500) and bool((ns["deep_ids"] >= 0).all())
