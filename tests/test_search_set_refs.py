"""CPU: the two formulations of the set queries' reference (tests/search_set_refs.py) agree on the whole grid of
tests/test_gpu_search_sets.py -- the minimum over the members followed by one sort, against the members' own top-`depth` lists
concatenated, sorted and de-duplicated by row or by group.  That is the argument the device's merge over the tiles of a set rests on (a
row of the set's first `depth` is in the list of the member that attains its minimum; the stale, worse entries of other members are
dropped), pinned without a GPU; and every seed of the grid, with every group kind, is shown to have a min_gap above 1e-12 here."""
import numpy as np
import pytest

import search_grouped_refs as GR
import search_mask_refs as MR
import search_refs as SR
import search_set_refs as ST


@pytest.mark.parametrize("ng,d,m,s,depth", ST.grid())
def test_the_two_formulations_agree_on_the_grid(ng, d, m, s, depth):
    for half in (False, True):
        stored, q, E = ST.case_distances(ng, d, m, s, half)
        g = stored.astype(np.float32)
        for mk in GR.MASK_KINDS:
            live = MR.make_mask(mk, ng, seed=ng)
            ids, d64, gap = SR.sorted_lists(ST.admissible(E, live), depth)
            assert gap > 1e-12, gap
            ids2, d642 = ST.merge_member_lists(g, q, depth, live=live)
            assert np.array_equal(ids, ids2) and np.array_equal(d64, d642)
            assert np.array_equal(ids >= 0, np.isfinite(d64))
            for row in ids:
                assert np.unique(row[row >= 0]).size == int((row >= 0).sum())


@pytest.mark.parametrize("ng,d,m,s,depth,gk", ST.grouped_grid())
def test_the_two_formulations_agree_on_the_grouped_grid(ng, d, m, s, depth, gk):
    groups = GR.make_groups(gk, ng, seed=ng)
    for half in (False, True):
        stored, q, E = ST.case_distances(ng, d, m, s, half)
        g = stored.astype(np.float32)
        for mk in GR.MASK_KINDS:
            live = MR.make_mask(mk, ng, seed=ng)
            gi, gg, gd, gap = GR.lists_by_sort(ST.admissible(E, live), groups, depth)
            assert gap > 1e-12, gap
            gi2, gg2, gd2 = ST.merge_member_lists(g, q, depth, groups=groups, live=live)
            assert np.array_equal(gi, gi2) and np.array_equal(gg, gg2) and np.array_equal(gd, gd2)


def test_ragged_sizes_exclusion_and_non_finite_members():
    g, q = ST.make_case(257, 64, 9, 3, seed=5)
    q[1, 4, 7] = np.nan
    q[2, :, 0] = np.inf                                        # a set with no finite member
    g[100, 3] = np.nan
    sizes, groups = [9, 6, 2], GR.make_groups("pairs", 257)
    live = MR.make_mask("random_0.5", 257, seed=1)
    live[100] = True
    first = ST.reference_sets(g, q, 7, sizes=sizes, live=live)[0][:, 0]
    for exclude in (None, np.array([first[0], -1, 5], np.int64)):
        ids, d64, gap = ST.reference_sets(g, q, 7, sizes=sizes, live=live, exclude=exclude)
        assert gap > 1e-12
        ids2, d642 = ST.merge_member_lists(g, q, 7, sizes=sizes, live=live, exclude=exclude)
        assert np.array_equal(ids, ids2) and np.array_equal(d64, d642)
        assert (ids[2] == -1).all() and np.isinf(d64[2]).all() and 100 not in ids
        if exclude is not None:
            assert first[0] not in ids[0]
    gx = np.array([groups[first[0]], 1 << 40, 3], np.int64)
    gi, gg, gd, gap = ST.reference_sets_grouped(g, q, groups, 7, sizes=sizes, live=live, exclude=gx)
    assert gap > 1e-12 and groups[first[0]] not in gg[0]
    gi2, gg2, gd2 = ST.merge_member_lists(g, q, 7, groups=groups, sizes=sizes, live=live, exclude=gx)
    assert np.array_equal(gi, gi2) and np.array_equal(gg, gg2) and np.array_equal(gd, gd2)
    assert ST.nonfinite_bits(g, q, live) == 3
    # a member past its set's size, and a repeated member, change nothing
    E = ST.set_distances64(g, q, sizes)
    q2 = q.copy()
    q2[1, 6:] = q[1, 0]
    assert np.array_equal(E[:2], ST.set_distances64(g, q2, [9, 9, 2])[:2], equal_nan=True)
    members = ST.attaining_members(g, q, ids, sizes=sizes)
    assert (members[2] == -1).all() and (members[1][ids[1] >= 0] < 6).all() and (members[1] != 4).all()
