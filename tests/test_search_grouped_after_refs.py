"""CPU: the reference of the paged grouped search (tests/search_grouped_after_refs.py) against itself -- its two formulations agree, pages
chained to exhaustion are the full grouped order, the cursor's corner cases mean what the header says -- and the exactness condition of
the GPU tests (tests/test_gpu_search_grouped_after.py): on every input they compare ids on, min_gap > 1e-12 over the full order."""
import functools

import numpy as np
import pytest

import rank_refs as RR
import search_after_refs as AR
import search_grouped_after_refs as PR
import search_grouped_refs as GR
import search_mask_refs as MR
import search_refs as SR

NGS = [1, 2, 64, 65, 257, 1027]
KINDS = ("singletons", "one", "pairs", "strided", "blocks_of_40", "random_50")
DEPTHS = (1, 11, 64)
NQ = 3


@functools.lru_cache(maxsize=None)
def _D():
    a, b = RR.spread_pairs(1027, 64, 77)
    D = SR.distances64(a, b[:NQ])
    assert SR.sorted_lists(D, 1027)[2] > 1e-12
    return D


def _groups(kind, ng):
    return PR.dense_slots(GR.make_groups(kind, ng, seed=ng))[1]


def _cursors(D, groups, live, ng):
    """Per query a cursor inside its grouped order: entry (3 + 5 q) of it, clamped to its last."""
    order = GR.lists_by_sort(PR.admissible(D, groups, live), groups, ng)[0]
    n_valid = (order >= 0).sum(1)
    return np.array([order[q, min(3 + 5 * q, n_valid[q] - 1)] if n_valid[q] else -1 for q in range(D.shape[0])], np.int64)


def _same(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x[:3], y[:3]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ng", NGS)
def test_the_two_formulations_agree(ng, kind):
    D, groups = _D()[:, :ng], _groups(kind, ng)
    for masked in (False, True):
        live = MR.make_mask("random_0.5", ng, seed=ng) if masked else None
        after = _cursors(D, groups, live, ng)
        exclude = groups[(np.arange(NQ) * 7) % ng].astype(np.int64)
        for depth in DEPTHS:
            if depth > ng:
                continue
            for ex in (None, exclude):
                assert _same(PR.page_by_sort(D, groups, depth, after, live, ex), PR.page_by_minima(D, groups, depth, after, live, ex))
                shifted = np.where(after >= 0, after + 1000, -1)
                a, b = PR.page_by_sort(D, groups, depth, after, live, ex), PR.page_by_sort(D, groups, depth, shifted, live, ex, id_base=1000)
                assert np.array_equal(np.where(a[0] >= 0, a[0] + 1000, -1), b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
                assert _same(b, PR.page_by_minima(D, groups, depth, shifted, live, ex, id_base=1000))


@pytest.mark.parametrize("kind", ["pairs", "strided", "blocks_of_40", "random_50"])
@pytest.mark.parametrize("page", [1, 7, 64])
def test_pages_chained_to_exhaustion_are_the_full_grouped_order(page, kind):
    ng = 257
    D, groups = _D()[:, :ng], _groups(kind, ng)
    live = MR.make_mask("random_0.5", ng, seed=3)
    exclude = groups[[5, 6, 7]].astype(np.int64)
    for lv, ex in ((None, None), (live, None), (live, exclude)):
        full = PR.full_grouped_order(D, groups, lv, ex)
        for fn in (PR.page_by_sort, PR.page_by_minima):
            got = PR.chained_pages(D, groups, page, lv, ex, page=fn)
            width = min(got[0].shape[1], ng)
            for k in range(3):
                assert np.array_equal(got[k][:, :width], full[k][:, :width])
                assert (got[0][:, width:] == -1).all() and (full[0][:, width:] == -1).all()
            for q in range(NQ):                                   # no repeats: every video once
                v = got[1][q][got[0][q] >= 0]
                assert v.size == np.unique(v).size


def test_min_gap_of_every_input_the_gpu_tests_compare_ids_on():
    for name, g, q in PR.gpu_inputs():
        D = SR.distances64(g, q)
        assert np.isfinite(D).all(), name
        gap = PR.full_min_gap(D)
        assert gap > 1e-12, (name, gap)


def test_cursor_on_a_dead_row_an_excluded_row_minus_one_and_past_the_end():
    ng = 257
    D, groups = _D()[:, :ng], _groups("pairs", ng)
    live = np.ones(ng, bool)
    plain = GR.lists_by_sort(D, groups, 20)
    cur = plain[0][:, 4].copy()                                   # every query's fifth video, by its nearest row
    for q in range(NQ):
        live[cur[q]] = False                                      # ... which dies: the key stays a key
    for fn in (PR.page_by_sort, PR.page_by_minima):
        got = fn(D, groups, 5, cur, live)
        full = PR.full_grouped_order(D, groups, live)
        for q in range(NQ):
            cd = D[q, cur[q]]
            valid = full[0][q] >= 0
            keep = valid & ((full[2][q] > cd) | ((full[2][q] == cd) & (full[0][q] > cur[q])))
            assert np.array_equal(got[0][q], full[0][q][keep][:5])
            # the dead cursor row's video may come back by its OTHER row, if that one lies after the cursor
            assert cur[q] not in got[0][q]
        # the cursor on a row of the excluded video: a key like any other, and the video never comes back
        ex = groups[cur].astype(np.int64)
        got = fn(D, groups, 5, cur, None, ex)
        assert (got[0] >= 0).all() and not (got[1] == ex[:, None]).any()
        want = PR.full_grouped_order(D, groups, None, ex)
        for q in range(NQ):
            pos = int(np.searchsorted(want[2][q], D[q, cur[q]], side="right"))
            assert np.array_equal(got[0][q], want[0][q][pos:pos + 5])
        # no key: an empty page, for that query alone
        after = np.array([-1, ng, cur[2]], np.int64)
        got = fn(D, groups, 5, after)
        assert (got[0][:2] == -1).all() and (got[1][:2] == -1).all() and np.isinf(got[2][:2]).all() and (got[0][2] >= 0).all()
        got = fn(D, groups, 5, np.array([999, 1000 + ng, 1000 + cur[2]], np.int64), id_base=1000)
        assert (got[0][:2] == -1).all() and (got[0][2] >= 1000).all()


def test_a_tied_gallery_with_groups_cutting_through_the_runs():
    g, q = PR.tied_rows()
    D = SR.distances64(g, q)
    n = g.shape[0]
    for kind in ("pairs", "strided", "random_50"):
        groups = _groups(kind, n)
        full = PR.full_grouped_order(D, groups)
        assert full[3] > 1e-12
        order = AR.full_order(g, q)[0]
        for pos in (2, 7, 131):                                   # cursors in the middle of runs of five bit-equal distances
            after = order[:, pos]
            assert all(D[i, order[i, pos]] == D[i, order[i, pos + 1]] or D[i, order[i, pos]] == D[i, order[i, pos - 1]] for i in range(3))
            a, b = PR.page_by_sort(D, groups, 11, after), PR.page_by_minima(D, groups, 11, after)
            assert _same(a, b)
        for page in (7, 64):
            got = PR.chained_pages(D, groups, page)
            width = min(got[0].shape[1], n)
            assert np.array_equal(got[0][:, :width], full[0][:, :width]) and np.array_equal(got[1][:, :width], full[1][:, :width])


def test_dense_slots():
    vids = np.array([7, 2 ** 31 - 1, 123456789, 7, 0, 123456789], np.int64)
    uniq, slot = PR.dense_slots(vids)
    assert slot.dtype == np.int32 and np.array_equal(uniq[slot], vids) and np.array_equal(uniq, np.unique(vids)) and slot.max() == uniq.size - 1
