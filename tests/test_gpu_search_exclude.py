"""GPU: the excluding search -- vtc_l2_search_excluding / ops.l2_search(exclude=...) / ops.l2_search_grouped(exclude=...), the parts,
VideoIndex.search(exclude=...) / search_videos(exclude_videos=...) / search_deep(exclude=...) / similar / similar_videos -- bit for bit
against the library's own masked search of ONE query with the excluded rows' bits cleared, and against the numpy reference of
tests/search_exclude_refs.py (the order of the live finite rows, the excluded ones deleted, then cut).

Ids are compared with exact equality; every comparison with the reference asserts its min_gap > 1e-12 first, over the FULL order.  fp32
dists are within one fp32 ulp of the reference and bit-equal between the library's entry points.  The excluded rows are chosen from each
query's own top 11 (by the reference, so the references are computed once per gallery and shared), and the tests assert that the
exclusion changes the result."""
import functools

import numpy as np
import pytest
import torch

import rank_refs as RR
import search_after_refs as AR
import search_exclude_refs as XR
import search_grouped_refs as GR
import search_mask_refs as MR
import search_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NQS = [1, 2, 3, 5, 9, 64]                                     # every tile shape, two tiles, eight tiles
NGS = [65, 257, 1027]
STORAGES = ("float32", "float16")
KINDS = ("pairs", "blocks_of_40", "random_50", "sparse_ids")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
NO_ROW = (-1, None, 2 ** 40, -2 ** 62)                        # None: n_gallery, the first id past the gallery
NO_GROUP = (2 ** 31, -2 ** 31 - 1)


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
def _rows():
    """1027 x 64 spread rows as fp32 and rounded to half (widened again: what the reference sees), and 64 queries."""
    a, b = RR.spread_pairs(1027, 64, 21)
    return {"float32": a, "float16": a.astype(np.float16).astype(np.float32)}, b


@pytest.fixture(scope="module")
def data():
    g, b = _rows()
    return {"np": g, "t": {"float32": _t(g["float32"]), "float16": _t(g["float32"].astype(np.float16))}, "b": b, "tb": _t(b)}


@functools.lru_cache(maxsize=None)
def _dist(storage):
    g, b = _rows()
    return SR.distances64(g[storage], b[:64])


def _live(ng, masked):
    return MR.make_mask("random_0.5", ng, seed=ng) if masked else None


@functools.lru_cache(maxsize=None)
def _case(storage, ng, masked):
    """The shared reference of one gallery for all 64 queries (a test with fewer takes the first rows): the plain full order, the
    excluded row of every query -- entry u % 11 of its own order -- and the full order without it."""
    live = _live(ng, masked)
    D = _dist(storage)[:, :ng]
    plain, _, gap = SR.sorted_lists(XR.excluded_distances(D, np.full(64, -1), live), ng)
    assert gap > 1e-12, gap
    ex = np.array([plain[u, u % 11] for u in range(64)], np.int64)
    ids, d64, gap = SR.sorted_lists(XR.excluded_distances(D, ex, live), ng)
    assert gap > 1e-12, gap
    return dict(live=live, ex=ex, plain=plain, ids=ids, d64=d64)


@functools.lru_cache(maxsize=None)
def _gcase(storage, ng, masked, kind):
    """The grouped counterpart: the excluded group of query u is that of entry u % (its entries) of its own grouped top 11; with
    sparse_ids the first three queries exclude the groups -1, INT32_MIN and INT32_MAX.  The reference list is 64 deep."""
    live = _live(ng, masked)
    groups = GR.make_groups(kind, ng, seed=ng)
    D = XR.excluded_distances(_dist(storage)[:, :ng], np.full(64, -1), live)
    assert SR.sorted_lists(D, ng)[2] > 1e-12                  # deleting rows from an order only widens its gaps
    _, grp, d64, _ = GR.lists_by_sort(D, groups, 11)
    ex = np.array([grp[u, u % int(np.isfinite(d64[u]).sum())] for u in range(64)], np.int64)
    if kind == "sparse_ids":
        ex[:3] = (-1, I32_MIN, I32_MAX)
    alive = np.ones(ng, bool) if live is None else live
    has = np.array([bool((alive & (groups == e)).any()) for e in ex])
    assert live is not None or has.all()
    ids, grp, d64, gap = GR.lists_by_sort(XR.excluded_distances(D, ex, None, groups), groups, 64)
    assert gap > 1e-12, gap
    return dict(live=live, groups=groups, ex=ex, has=has, ids=ids, grp=grp, d64=d64)


def _search(g, q, depth, live=None, after=None, exclude=None, id_base=0):
    """One call in a workspace of its own: (ids, dists, fp64 dists, nonfinite bits)."""
    ops = _ops()
    ws = ops.workspace(ops.l2_search_workspace_bytes(g.shape[0], q.shape[0], g.shape[1], depth), g.device)
    ids, dists, bits = ops.l2_search(g, q, depth, id_base=id_base, ws=ws, live=live, after=after, exclude=exclude)
    return ids, dists, ops.search_dists64(ws, q.shape[0], depth).clone(), bits


def _gsearch(g, q, groups, depth, live=None, exclude=None, id_base=0):
    """(ids, groups, dists, fp64 dists, nonfinite bits)."""
    ops = _ops()
    ws = ops.workspace(ops.l2_search_grouped_workspace_bytes(g.shape[0], q.shape[0], g.shape[1], depth), g.device)
    ids, grp, dists, bits = ops.l2_search_grouped(g, q, groups, depth, id_base=id_base, ws=ws, live=live, exclude=exclude)
    return ids, grp, dists, ops.search_dists64(ws, q.shape[0], depth).clone(), bits


def _flags(live, ng):
    return torch.ones(ng, dtype=torch.uint8, device=DEV) if live is None else _t(live.astype(np.uint8))


def _cleared(flags, dead):
    """The packed words of `flags` with the rows `dead` (a bool tensor, or one row) cleared."""
    f = flags.clone()
    f[dead] = 0
    return _ops().row_mask_pack(f)


def _assert_empty(ids, dists):
    assert bool((ids == -1).all()) and bool(torch.isposinf(dists).all())


def _assert_against_reference(got, want_ids, want_d64):
    ids, dists, d64 = got
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    SR.assert_dists_within_one_ulp(dists.cpu().numpy(), want_d64.astype(np.float32))
    # fp64 sums of 64 terms of a D <= 4: any summation order is within 64 * 2^-53 * 4 < 1e-13 of any other
    fin = np.isfinite(want_d64)
    assert np.array_equal(np.isposinf(d64.cpu().numpy()), ~fin) and np.abs(d64.cpu().numpy()[fin] - want_d64[fin]).max() <= 1e-13


# ---- 1. against the library itself, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("ng", NGS)
def test_excluding_is_the_masked_search_without_that_row(data, ng, nq):
    q = data["tb"][:nq]
    for storage in STORAGES:
        g = data["t"][storage][:ng]
        for masked in (False, True):
            c = _case(storage, ng, masked)
            flags, words = _flags(c["live"], ng), _words(c["live"])
            got = _search(g, q, 11, live=words, exclude=_i64(c["ex"][:nq]))
            plain = _search(g, q, 11, live=words)
            for u in range(nq):
                want = _search(g, q[u:u + 1], 11, live=_cleared(flags, int(c["ex"][u])))
                for x, y in zip(got[:3], want[:3]):
                    assert torch.equal(x[u], y[0]), (storage, masked, u)
                assert not torch.equal(got[0][u], plain[0][u])      # the excluded row was in the query's top 11
            assert int(got[3].item()) == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("ng", NGS)
def test_grouped_excluding_is_the_masked_search_without_that_group(data, ng, nq, kind):
    q = data["tb"][:nq]
    for storage in STORAGES:
        g = data["t"][storage][:ng]
        for masked in (False, True):
            c = _gcase(storage, ng, masked, kind)
            groups = _t(c["groups"])
            flags, words = _flags(c["live"], ng), _words(c["live"])
            got = _gsearch(g, q, groups, 11, live=words, exclude=_i64(c["ex"][:nq]))
            plain = _gsearch(g, q, groups, 11, live=words)
            for u in range(nq):
                want = _gsearch(g, q[u:u + 1], groups, 11, live=_cleared(flags, groups == int(c["ex"][u])))
                for x, y in zip(got[:4], want[:4]):
                    assert torch.equal(x[u], y[0]), (storage, masked, u)
                assert torch.equal(got[0][u], plain[0][u]) != bool(c["has"][u])      # changed iff the group has a live row
            if kind == "sparse_ids" and nq >= 3:              # -1, INT32_MIN and INT32_MAX are groups like any other
                for u, e in enumerate((-1, I32_MIN, I32_MAX)):
                    full = got[0][u] >= 0
                    assert bool((got[1][u][full] != e).all()) and (not c["has"][u] or bool((plain[1][u] == e).any()))


# ---- 2. against numpy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [11, 64])
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("ng", NGS)
def test_against_the_reference(data, ng, nq, depth):
    q = data["tb"][:nq]
    for storage in STORAGES:
        g = data["t"][storage][:ng]
        for masked in (False, True):
            c = _case(storage, ng, masked)
            got = _search(g, q, depth, live=_words(c["live"]), exclude=_i64(c["ex"][:nq]))
            _assert_against_reference(got[:3], c["ids"][:nq, :depth], c["d64"][:nq, :depth])
            assert bool((got[0] != _i64(c["ex"][:nq])[:, None]).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("depth", [11, 64])
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("ng", NGS)
def test_grouped_against_the_reference(data, ng, nq, depth, kind):
    q = data["tb"][:nq]
    for storage in STORAGES:
        g = data["t"][storage][:ng]
        for masked in (False, True):
            c = _gcase(storage, ng, masked, kind)
            ids, grp, dists, d64, _ = _gsearch(g, q, _t(c["groups"]), depth, live=_words(c["live"]), exclude=_i64(c["ex"][:nq]))
            _assert_against_reference((ids, dists, d64), c["ids"][:nq, :depth], c["d64"][:nq, :depth])
            assert np.array_equal(grp.cpu().numpy(), c["grp"][:nq, :depth])


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("ng,depth", [(1, 1), (2, 2), (64, 64)])
def test_tiny_galleries_and_lists_that_run_empty(data, storage, ng, depth):
    nq = 3
    g, q = data["t"][storage][:ng], data["tb"][:nq]
    D = _dist(storage)[:nq, :ng]
    ex = np.array([0, ng - 1, -1], np.int64)
    want_ids, want_d64, gap = SR.sorted_lists(XR.excluded_distances(D, ex), ng)
    assert gap > 1e-12, gap
    got = _search(g, q, depth, exclude=_i64(ex))
    _assert_against_reference(got[:3], want_ids[:, :depth], want_d64[:, :depth])
    assert bool((got[0][:2, -1] == -1).all()) and bool((got[0][2] >= 0).all())      # ng - 1 rows are left: the last entry is empty
    if ng == 1:
        _assert_empty(got[0][:2], got[1][:2])                 # its only row excluded: an empty list
    # a grouped gallery of ONE group, excluded: an empty list; the group 5 + 1 is no group of it
    groups = GR.make_groups("one", ng)
    exg = np.array([5, 5, 6], np.int64)
    ids, grp, dists, d64, _ = _gsearch(g, q, _t(groups), depth, exclude=_i64(exg))
    want = GR.lists_by_sort(XR.excluded_distances(D, exg, None, groups), groups, depth)
    assert np.array_equal(ids.cpu().numpy(), want[0]) and np.array_equal(grp.cpu().numpy(), want[1])
    _assert_empty(ids[:2], dists[:2])
    assert int(ids[2, 0]) >= 0 and int(grp[2, 0]) == 5 and bool((ids[2, 1:] == -1).all())


# ---- 3. values that exclude nothing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", NQS)
def test_values_that_exclude_nothing(data, nq):
    ng = 257
    q = data["tb"][:nq]
    for storage in STORAGES:
        g = data["t"][storage][:ng]
        for masked in (False, True):
            c = _case(storage, ng, masked)
            words = _words(c["live"])
            plain, real = _search(g, q, 11, live=words), _search(g, q, 11, live=words, exclude=_i64(c["ex"][:nq]))
            # per query in rotation: a real exclusion, then the four values that are no row
            ex = np.array([c["ex"][u] if u % 5 == 0 else (NO_ROW[u % 5 - 1] if NO_ROW[u % 5 - 1] is not None else ng) for u in range(nq)], np.int64)
            got = _search(g, q, 11, live=words, exclude=_i64(ex))
            for u in range(nq):
                want = real if u % 5 == 0 else plain
                for x, y in zip(got[:3], want[:3]):
                    assert torch.equal(x[u], y[u]), (storage, masked, u)
            g_c = _gcase(storage, ng, masked, "sparse_ids")
            groups = _t(g_c["groups"])
            plain, real = _gsearch(g, q, groups, 11, live=words), _gsearch(g, q, groups, 11, live=words, exclude=_i64(g_c["ex"][:nq]))
            ex = np.array([g_c["ex"][u] if u % 3 == 0 else NO_GROUP[u % 3 - 1] for u in range(nq)], np.int64)
            got = _gsearch(g, q, groups, 11, live=words, exclude=_i64(ex))
            for u in range(nq):
                want = real if u % 3 == 0 else plain
                for x, y in zip(got[:4], want[:4]):
                    assert torch.equal(x[u], y[u]), (storage, masked, u)


def test_an_excluded_row_that_is_dead_changes_nothing(data):
    ng, nq = 257, 9
    g, q = data["t"]["float32"][:ng], data["tb"][:nq]
    live = _live(ng, True)
    dead = np.flatnonzero(~live)
    words = _words(live)
    plain = _search(g, q, 11, live=words)
    got = _search(g, q, 11, live=words, exclude=_i64(dead[:nq]))
    for x, y in zip(got, plain):
        assert torch.equal(x, y)


# ---- 4. exact ties ----------------------------------------------------------------------------------------------------------------------
def test_excluding_a_row_in_the_middle_of_a_run_of_bit_equal_distances(data):
    g_np = AR.tied_gallery(data["np"]["float32"][:200], 21)    # 1000 rows, every distance five times
    nq = 5
    D = SR.distances64(g_np, data["b"][:nq])
    plain, plain_d64, gap = SR.sorted_lists(D, 1000)
    assert gap > 1e-12, gap
    ex = np.empty(nq, np.int64)
    for u in range(nq):                                       # the middle of the first run of five inside the top 11 + u
        p = next(p for p in range(2 + u, 60) if plain_d64[u, p - 2] == plain_d64[u, p + 2])
        ex[u] = plain[u, p]
    want_ids, want_d64, gap = SR.sorted_lists(XR.excluded_distances(D, ex), 1000)
    assert gap > 1e-12, gap
    want_ids, want_d64 = want_ids[:, :64], want_d64[:, :64]
    assert (want_d64[:, 1:] == want_d64[:, :-1]).mean() > 0.7
    ids, dists, d64, _ = _search(_t(g_np), data["tb"][:nq], 64, exclude=_i64(ex))
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    d64 = d64.cpu().numpy()
    assert np.array_equal(d64[:, 1:] == d64[:, :-1], want_d64[:, 1:] == want_d64[:, :-1])      # the device's ties are the reference's


# ---- 5. exclusion plus cursor -------------------------------------------------------------------------------------------------------------
def _chain(g, q, depth, pages, exclude, live=None):
    """`pages` pages of `depth` with the same exclusion, each after the last key of the one before; the first has no cursor."""
    out, after = [], None
    for _ in range(pages):
        ids, dists, d64, _ = _search(g, q, depth, after=after, live=live, exclude=exclude)
        out.append((ids, dists, d64))
        after = (d64[:, -1].clone(), ids[:, -1].clone())
    return tuple(torch.cat([o[i] for o in out], dim=1) for i in range(3))


@pytest.mark.parametrize("nq", NQS)
def test_four_pages_of_16_with_exclude_are_one_excluding_search_of_64(data, nq):
    ng = 257
    q = data["tb"][:nq]
    for storage in STORAGES:
        g = data["t"][storage][:ng]
        for masked in (False, True):
            c = _case(storage, ng, masked)
            words, ex = _words(c["live"]), _i64(c["ex"][:nq])
            got = _chain(g, q, 16, 4, ex, live=words)
            want = _search(g, q, 64, live=words, exclude=ex)
            for x, y in zip(got, want[:3]):
                assert torch.equal(x, y), (storage, masked)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("ng,depth", [(65, 64), (257, 64), (257, 11)])
def test_pages_until_exhausted_are_the_order_without_the_excluded_row(data, storage, ng, depth):
    nq = 3
    g, q = data["t"][storage][:ng], data["tb"][:nq]
    c = _case(storage, ng, False)
    ex = _i64(c["ex"][:nq])
    pages = -(-(ng - 1) // depth)
    ids, dists, d64 = _chain(g, q, depth, pages, ex)
    assert bool((c["ids"][:nq, :ng - 1] >= 0).all()) and bool((c["ids"][:nq, ng - 1] == -1).all())      # the order has ng - 1 entries
    _assert_against_reference((ids[:, :ng], dists[:, :ng], d64[:, :ng]), c["ids"][:nq, :pages * depth][:, :ng],
                              c["d64"][:nq, :pages * depth][:, :ng])
    _assert_empty(ids[:, ng - 1:], dists[:, ng - 1:])
    last = _i64(c["ids"][:nq, ng - 2])                         # the last key of the order: nothing comes after it
    after = (_ops().l2_pair_dists64(g, q, last), last)
    more = _search(g, q, depth, after=after, exclude=ex)
    _assert_empty(more[0], more[1])
    assert bool(torch.isposinf(more[2]).all())


@pytest.mark.parametrize("storage", STORAGES)
def test_the_cursor_may_stand_on_the_excluded_row(data, storage):
    ng, nq = 257, 9
    ops = _ops()
    g, q = data["t"][storage][:ng], data["tb"][:nq]
    for masked in (False, True):
        c = _case(storage, ng, masked)
        words, ex = _words(c["live"]), _i64(c["ex"][:nq])
        after = (ops.l2_pair_dists64(g, q, ex), ex)
        got = _search(g, q, 11, live=words, after=after, exclude=ex)
        want_ids, want_d64, gap = XR.reference_search_excluding_after(data["np"][storage][:ng], data["b"][:nq], 11, c["ex"][:nq], c["ex"][:nq],
                                                                      live=c["live"])
        assert gap > 1e-12, gap
        _assert_against_reference(got[:3], want_ids, want_d64)
        for u in range(nq):                                   # the page starts right after the excluded row's key
            p = u % 11
            assert np.array_equal(want_ids[u], c["plain"][u, p + 1:p + 12])
        plain_after = _search(g, q, 11, live=words, after=after)      # the row at the cursor is not after it: the cursor scan's page
        for x, y in zip(got[:3], plain_after[:3]):
            assert torch.equal(x, y)


# ---- 6. non-finite ------------------------------------------------------------------------------------------------------------------------
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
    ex = masked[0][:, 2].clone()                               # -1 for the NaN query: nothing
    ids, dists, d64, bits = _search(g, q, 10, live=words, exclude=ex)
    assert int(bits.item()) == int(masked[3].item())
    _assert_empty(ids[3], dists[3])
    assert bool(torch.isposinf(d64[3]).all())
    keep = [0, 1, 2, 4]
    rest = [0, 1, 3, 4, 5, 6, 7, 8, 9, 10]
    assert torch.equal(ids[keep], masked[0][keep][:, rest]) and torch.equal(dists[keep], masked[1][keep][:, rest])
    assert torch.equal(d64[keep], masked[2][keep][:, rest])
    groups = _t(GR.make_groups("pairs", 257))
    gm = _gsearch(g, q, groups, 11, live=words)
    gx = _gsearch(g, q, groups, 10, live=words, exclude=gm[1][:, 2].to(torch.int64))
    assert int(gx[4].item()) == int(gm[4].item()) == 3
    _assert_empty(gx[0][3], gx[2][3])
    assert torch.equal(gx[0][keep], gm[0][keep][:, rest]) and torch.equal(gx[3][keep], gm[3][keep][:, rest])


# ---- 7. windows ---------------------------------------------------------------------------------------------------------------------------
def test_windows_exclude_the_same_global_row(data):
    ops = _ops()
    nq, depth = 3, 40
    g, q = data["t"]["float32"], data["tb"][:nq]
    cuts = [0, 400, 800, 1027]
    c = _case("float32", 1027, False)
    for w in range(3):                                        # the excluded row in the first, the middle, the last window
        pos = [next(p for p in range(depth) if cuts[w] <= c["plain"][u, p] < cuts[w + 1]) for u in range(nq)]
        ex_np = np.array([c["plain"][u, pos[u]] for u in range(nq)], np.int64)
        ex = _i64(ex_np)
        whole = _search(g, q, depth, exclude=ex)
        for u in range(nq):
            assert np.array_equal(whole[0][u].cpu().numpy(), np.delete(c["plain"][u, :depth + 1], pos[u]))
        parts = [ops.l2_search_part(g[lo:hi], q, depth, id_base=lo, exclude=ex)[:2] for lo, hi in zip(cuts[:-1], cuts[1:])]
        ids, dists = ops.l2_search_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
        assert torch.equal(ids, whole[0]) and torch.equal(dists, whole[1])
        # a window's own id_base moves the ids and the exclusion alike
        ids, _, d64, _ = _search(g, q, depth, exclude=ex + 5000, id_base=5000)
        assert torch.equal(ids, whole[0] + 5000) and torch.equal(d64, whole[2])
        ids, _, d64, _ = _search(g, q, depth, exclude=ex, id_base=5000)      # the same number is now another row, or none
        assert not torch.equal(ids, whole[0] + 5000)


def test_grouped_windows_exclude_the_same_group(data):
    ops = _ops()
    nq, depth = 3, 40
    g, q = data["t"]["float32"], data["tb"][:nq]
    cuts = [0, 400, 800, 1027]
    c = _gcase("float32", 1027, False, "random_50")           # 50 groups over 1027 rows: every group has rows in all three windows
    groups_np, groups = c["groups"], _t(c["groups"])
    for u in range(nq):
        assert all(((groups_np[lo:hi] == c["ex"][u]).any() for lo, hi in zip(cuts[:-1], cuts[1:])))
    ex = _i64(c["ex"][:nq])
    whole = _gsearch(g, q, groups, depth, exclude=ex)
    assert np.array_equal(whole[0].cpu().numpy(), c["ids"][:nq, :depth]) and np.array_equal(whole[1].cpu().numpy(), c["grp"][:nq, :depth])
    parts = [ops.l2_search_grouped_part(g[lo:hi], q, groups[lo:hi], depth, id_base=lo, exclude=ex)[:3] for lo, hi in zip(cuts[:-1], cuts[1:])]
    ids, grp, dists = ops.l2_search_merge_grouped(torch.stack([p[0] for p in parts]), torch.stack([p[2] for p in parts]),
                                                  torch.stack([p[1] for p in parts]))
    assert torch.equal(ids, whole[0]) and torch.equal(grp, whole[1]) and torch.equal(dists, whole[2])
    moved = _gsearch(g, q, groups, depth, exclude=ex, id_base=5000)      # groups are not ids: id_base moves the rows alone
    assert torch.equal(moved[0], whole[0] + 5000) and torch.equal(moved[1], whole[1]) and torch.equal(moved[3], whole[3])


# ---- 8. feature widths --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [192, 512, 2048])               # one, two and eight 256-column slices a lane walks
def test_feature_widths(d):
    a, b = RR.spread_pairs(300, d, 22)
    flags = _flags(None, 300)
    groups = _t(GR.make_groups("pairs", 300))
    for g in (_t(a), _t(a.astype(np.float16))):
        for nq in (1, 9):
            q = _t(b[:nq])
            plain = _search(g, q, 11)
            ex = torch.stack([plain[0][u, u % 11] for u in range(nq)])
            got = _search(g, q, 11, exclude=ex)
            gplain = _gsearch(g, q, groups, 11)
            exg = torch.stack([gplain[1][u, u % 11] for u in range(nq)]).to(torch.int64)
            ggot = _gsearch(g, q, groups, 11, exclude=exg)
            for u in range(nq):
                want = _search(g, q[u:u + 1], 11, live=_cleared(flags, ex[u]))
                for x, y in zip(got[:3], want[:3]):
                    assert torch.equal(x[u], y[0])
                assert not torch.equal(got[0][u], plain[0][u])
                want = _gsearch(g, q[u:u + 1], groups, 11, live=_cleared(flags, groups == exg[u]))
                for x, y in zip(ggot[:4], want[:4]):
                    assert torch.equal(x[u], y[0])
                assert not torch.equal(ggot[0][u], gplain[0][u])


# ---- 9. VideoIndex ------------------------------------------------------------------------------------------------------------------------
def _assert_scores(scores, ids, want_d64):
    """The bound of test_gpu_search_after.py::_assert_scores: score = 1 - D / 2 in fp32 from the fp32 D: D <= 4 rounds to fp32 within
    2.4e-7, one more ulp (4.8e-7) for the summation order of the reference, halved, plus the rounding of a score of magnitude <= 1
    (6e-8): below 5e-7."""
    s = scores.cpu().numpy().astype(np.float64)
    full = ids.cpu().numpy() >= 0
    assert np.isneginf(s[~full]).all()
    assert np.abs(s[full] - (1.0 - want_d64[full] / 2.0)).max() < 5e-7


def _index(data, storage, n=1027, video_ids=None):
    from vtc_amd.host.search import VideoIndex
    index = VideoIndex(64, device=DEV, storage=storage)
    index.add(data["t"]["float32"][:n], video_ids=video_ids)
    return index


def _stored(index):
    return index.rows.float().cpu().numpy()


@pytest.mark.parametrize("storage", [torch.float32, torch.float16])
def test_similar(data, storage):
    index = _index(data, storage)
    g = _stored(index)
    rows = np.arange(5, 5 + 70 * 13, 13, dtype=np.int64)      # 70 stored rows: two slices of queries
    want_ids, want_d64, gap = XR.full_order_excluding(g, g[rows], rows)
    assert gap > 1e-12, gap
    ids, scores = index.similar(_i64(rows), 5)
    assert tuple(ids.shape) == (70, 5) and ids.dtype == torch.int64 and scores.dtype == torch.float32
    assert bool((ids != _i64(rows)[:, None]).all())
    assert np.array_equal(ids.cpu().numpy(), want_ids[:, :5])
    _assert_scores(scores, ids, want_d64[:, :5])
    plain, _ = index.search(torch.from_numpy(g[rows[:8], :64]).to(DEV), 5)      # what the caller had before: itself in first place
    assert torch.equal(plain[:, 0], _i64(rows[:8]))
    # the next page, a subset the query rows are no members of, and a removed query row
    ids2, _ = index.similar(_i64(rows), 5, after=ids[:, -1])
    assert np.array_equal(ids2.cpu().numpy(), want_ids[:, 5:10])
    member = np.ones(1027, bool)
    member[rows] = False
    member[::7] = False
    sub_ids, _, gap = XR.full_order_excluding(g, g[rows], rows, live=member)
    assert gap > 1e-12, gap
    got, _ = index.similar(_i64(rows), 5, subset=index.subset(torch.from_numpy(member)))
    assert np.array_equal(got.cpu().numpy(), sub_ids[:, :5])
    assert index.remove(rows[:3]) == 3
    live = index.live_mask.cpu().numpy()
    want_ids, want_d64, gap = XR.full_order_excluding(g, g[rows], rows, live=live)
    assert gap > 1e-12, gap
    ids, scores = index.similar(_i64(rows), 5)
    assert np.array_equal(ids.cpu().numpy(), want_ids[:, :5]) and bool((ids[:3] >= 0).all())
    _assert_scores(scores, ids, want_d64[:, :5])


@pytest.mark.parametrize("storage", [torch.float32, torch.float16])
def test_similar_returns_a_bit_equal_duplicate_first_with_score_one(data, storage):
    from vtc_amd.host.search import VideoIndex
    index = VideoIndex(64, device=DEV, storage=storage)
    index.add(torch.cat([data["t"]["float32"][:100], data["t"]["float32"][7:8]]))      # row 100 is row 7 again
    assert torch.equal(index.rows[100], index.rows[7])
    ids, scores = index.similar(_i64([7, 100, 8]), 5)
    assert ids[0, 0].item() == 100 and ids[1, 0].item() == 7 and scores[0, 0].item() == 1.0 and scores[1, 0].item() == 1.0
    assert 7 not in ids[0].tolist() and 100 not in ids[1].tolist() and scores[2, 0].item() < 1.0


def test_similar_ids_that_are_no_row_give_empty_rows(data):
    index = _index(data, torch.float32, 257)
    rows = _i64([3, 50, 90, 256])
    good = index.similar(rows, 5)
    bad = rows.clone()
    bad[1], bad[2] = -1, index.ntotal + 5
    ids, scores = index.similar(bad, 5)
    assert bool((ids[1:3] == -1).all()) and bool(torch.isneginf(scores[1:3]).all())
    assert torch.equal(ids[[0, 3]], good[0][[0, 3]]) and torch.equal(scores[[0, 3]], good[1][[0, 3]]) and bool((ids[[0, 3]] >= 0).all())
    for wrong in (rows.to(torch.int32), rows.double(), rows[:, None], rows[:0], [3, 50]):
        with pytest.raises(ValueError):
            index.similar(wrong, 5)
    with pytest.raises(ValueError):
        index.similar(rows, 65)
    with pytest.raises(ValueError):
        index.similar_videos(rows, 5)                         # an ungrouped index


@pytest.mark.parametrize("storage", [torch.float32, torch.float16])
@pytest.mark.parametrize("kind", ["pairs", "random_50"])
def test_similar_videos_and_exclude_videos(data, storage, kind):
    groups = GR.make_groups(kind, 1027, seed=3)
    index = _index(data, storage, video_ids=torch.from_numpy(groups))
    g = _stored(index)
    rows = np.arange(2, 2 + 70 * 14, 14, dtype=np.int64)
    own = groups[rows].astype(np.int64)
    D = SR.distances64(g, g[rows])
    assert SR.sorted_lists(D, 1027)[2] > 1e-12
    want = GR.lists_by_sort(XR.excluded_distances(D, own, None, groups), groups, 5)
    videos, ids, scores = index.similar_videos(_i64(rows), 5)
    assert bool((videos != _i64(own)[:, None]).all())
    assert np.array_equal(ids.cpu().numpy(), want[0]) and np.array_equal(videos.cpu().numpy(), want[1].astype(np.int64))
    _assert_scores(scores, ids, want[2])
    bad = _i64(rows[:4])
    bad[1], bad[2] = -1, index.ntotal + 5
    v2, i2, s2 = index.similar_videos(bad, 5)
    assert bool((i2[1:3] == -1).all()) and bool((v2[1:3] == -1).all()) and bool(torch.isneginf(s2[1:3]).all())
    assert torch.equal(i2[[0, 3]], ids[[0, 3]]) and torch.equal(v2[[0, 3]], videos[[0, 3]])
    # hard negatives: text queries, each without its own video, in a subset and after a remove
    member = MR.make_mask("random_0.5", 1027, seed=12)
    index.remove(np.flatnonzero(member)[:9])
    live = index.live_mask.cpu().numpy() & member
    qp = index._prepared(data["tb"][:70], "queries", check=False).cpu().numpy()
    D = XR.excluded_distances(SR.distances64(g, qp), np.full(70, -1), live)
    assert SR.sorted_lists(D, 1027)[2] > 1e-12
    near = GR.lists_by_sort(D, groups, 1)[1][:, 0].astype(np.int64)      # every query's nearest video: the one to leave out
    near[5], near[6] = -1, 2 ** 31 - 1                         # no video of the index: nothing is excluded
    want = GR.lists_by_sort(XR.excluded_distances(D, near, None, groups), groups, 5)
    subset = index.subset(torch.from_numpy(member))
    videos, ids, scores = index.search_videos(data["tb"][:70], 5, subset=subset, exclude_videos=_i64(near))
    assert np.array_equal(ids.cpu().numpy(), want[0]) and np.array_equal(videos.cpu().numpy(), want[1].astype(np.int64))
    _assert_scores(scores, ids, want[2])
    plain = index.search_videos(data["tb"][:70], 5, subset=subset)
    assert torch.equal(videos[5:7], plain[0][5:7]) and torch.equal(videos[:5, :4], plain[0][:5, 1:])
    for wrong in (_i64(near)[:69], _i64(near).to(torch.int32), _i64(near).float()):
        with pytest.raises(ValueError):
            index.search_videos(data["tb"][:70], 5, exclude_videos=wrong)


@pytest.mark.parametrize("storage", [torch.float32, torch.float16])
def test_search_exclude_with_subset_and_after_remove_and_search_deep(data, storage):
    index = _index(data, storage)
    g = _stored(index)
    queries = data["tb"][:70]
    qp = index._prepared(queries, "queries", check=False).cpu().numpy()
    first, _ = index.search(queries, 5)
    ex = first[:, 1].clone()                                  # every query's second-nearest row
    member = np.ones(1027, bool)
    member[::7] = False
    want_ids, want_d64, gap = XR.full_order_excluding(g, qp, ex.cpu().numpy(), live=member)
    assert gap > 1e-12, gap
    ids, scores = index.search(queries, 5, subset=index.subset(torch.from_numpy(member)), exclude=ex)
    assert np.array_equal(ids.cpu().numpy(), want_ids[:, :5])
    _assert_scores(scores, ids, want_d64[:, :5])
    index.remove(first[:, 0])                                 # every query's nearest row goes
    live = index.live_mask.cpu().numpy()
    want_ids, want_d64, gap = XR.full_order_excluding(g, qp, ex.cpu().numpy(), live=live)
    assert gap > 1e-12, gap
    ids, scores = index.search(queries, 5, exclude=ex)
    assert np.array_equal(ids.cpu().numpy(), want_ids[:, :5])
    _assert_scores(scores, ids, want_d64[:, :5])
    assert bool((ids != ex[:, None]).all())
    deep_ids, deep_scores = index.search_deep(queries[:3], 200, exclude=ex[:3])
    assert tuple(deep_ids.shape) == (3, 200)
    assert np.array_equal(deep_ids.cpu().numpy(), want_ids[:3, :200])
    _assert_scores(deep_scores, deep_ids, want_d64[:3, :200])
    for wrong in (ex[:69], ex.to(torch.int32), ex.float()):
        with pytest.raises(ValueError):
            index.search(queries, 5, exclude=wrong)
    with pytest.raises(ValueError):
        index.search(queries, 65, exclude=ex)


@pytest.mark.parametrize("storage", [torch.float32, torch.float16])
def test_none_is_the_call_without_the_argument(data, storage):
    index = _index(data, storage, video_ids=torch.from_numpy(GR.make_groups("pairs", 1027)))
    for nq in (3, 13):                                        # 13: an fp32 index with every row live takes the vtc_l2_topk route
        q = data["tb"][:nq]
        for a, b in ((index.search(q, 7), index.search(q, 7, exclude=None)),
                     (index.search(q, 7, None, None), index.search(q, 7, subset=None, after=None, exclude=None)),
                     (index.search_deep(q, 100), index.search_deep(q, 100, exclude=None)),
                     (index.search_videos(q, 7), index.search_videos(q, 7, exclude_videos=None))):
            for x, y in zip(a, b):
                assert torch.equal(x, y)
    ops = _ops()
    g, q = index.rows, index._prepared(data["tb"][:5], "queries", check=False)
    for x, y in zip(ops.l2_search(g, q, 7), ops.l2_search(g, q, 7, exclude=None)):
        assert torch.equal(x, y)
    for x, y in zip(ops.l2_search_grouped(g, q, index.video_ids, 7), ops.l2_search_grouped(g, q, index.video_ids, 7, exclude=None)):
        assert torch.equal(x, y)
    for wrong in (torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(5, dtype=torch.int32, device=DEV), torch.zeros(5, dtype=torch.int64)):
        with pytest.raises(ValueError):
            ops.l2_search(g, q, 7, exclude=wrong)
        with pytest.raises(ValueError):
            ops.l2_search_grouped(g, q, index.video_ids, 7, exclude=wrong)


# ---- 10. no host sync -------------------------------------------------------------------------------------------------------------------
def test_the_excluding_searches_do_not_sync(data):
    index = _index(data, torch.float32, video_ids=torch.from_numpy(GR.make_groups("pairs", 1027)))
    q, rows = data["tb"][:3], _i64([4, 77, 1000])
    calls = (lambda: index.similar(rows, 5), lambda: index.similar_videos(rows, 5), lambda: index.search(q, 5, exclude=rows),
             lambda: index.search_videos(q, 5, exclude_videos=rows))
    want = [c() for c in calls]                               # (warm: workspaces allocated)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [c() for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for a, b in zip(got, want):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ---- 11. the document's example ---------------------------------------------------------------------------------------------------------
def test_the_integration_documents_block_runs_as_written():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "similar_videos" in b]
    assert len(blocks) == 1, len(blocks)
    ns = {}
    exec(blocks[0], ns)                                       # its own assert: no video comes back for its own row or text
    assert tuple(ns["negatives"].shape) == (8, 10) and bool((ns["negatives"] >= 0).all())
