"""CPU: the two formulations of the grouped search's reference (tests/search_grouped_refs.py) agree, its identities hold, its merge over
windows equals the whole, and every (data seed, shape, group kind, mask kind) the GPU tests compare ids on keeps min_gap > 1e-12."""
import numpy as np
import pytest

import rank_refs as RR
import search_grouped_refs as GR
import search_mask_refs as MR
import search_refs as SR


@pytest.fixture(scope="module")
def spread64():
    return RR.spread_pairs(1027, 64, 21)


def _live(kind, ng):
    return MR.make_mask(kind, ng, seed=ng)


@pytest.mark.parametrize("ng,nq,depth", MR.edge_cases())
def test_the_two_formulations_agree(spread64, ng, nq, depth):
    a, b = spread64
    D = SR.distances64(a[:ng], b[:nq])
    for gk in GR.GROUP_KINDS:
        groups = GR.make_groups(gk, ng, seed=ng)
        for mk in ("all", "random_0.5", "first_half_dead"):
            Dm = GR._masked(D, _live(mk, ng))
            ids, grp, d64, gap = GR.lists_by_sort(Dm, groups, depth)
            ids2, grp2, d642 = GR.lists_by_minima(Dm, groups, depth)
            assert gap > 1e-12, (gk, mk, gap)
            assert np.array_equal(ids, ids2) and np.array_equal(grp, grp2) and np.array_equal(d64, d642), (gk, mk)
            # the invariants of the definition
            for i in range(nq):
                m = ids[i] >= 0
                assert len(set(grp[i, m].tolist())) == int(m.sum()) and np.all(np.diff(d64[i, m]) >= 0)
                assert np.array_equal(grp[i, m], groups[ids[i, m]]) and np.all(grp[i, ~m] == -1) and np.all(np.isinf(d64[i, ~m]))


def test_min_gap_of_every_other_seed_the_gpu_tests_use():
    """The widths (seed 22) and the VideoIndex rows (seed 25, 100 columns): the assertion the GPU tests make, checked here first."""
    for d in (192, 512, 2048):
        a, b = RR.spread_pairs(1027, d, 22)
        assert GR.reference_search_grouped64(a, b[:9], GR.make_groups("random_50", 1027, seed=d), 11)[3] > 1e-12
    a, b = RR.spread_pairs(600, 100, 25)
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    assert GR.reference_search_grouped64(a[:500], b[:9], GR.make_groups("random_50", 500, seed=1), 11)[3] > 1e-12


def test_singletons_are_the_ungrouped_search(spread64):
    a, b = spread64
    for ng, nq, depth in ((1027, 9, 11), (65, 4, 64), (1, 1, 1)):
        ids, grp, d32, gap = GR.reference_search_grouped(a[:ng], b[:nq], GR.make_groups("singletons", ng), depth, id_base=7)
        want_ids, want_d, want_gap = SR.reference_search(a[:ng], b[:nq], depth, id_base=7)
        assert np.array_equal(ids, want_ids) and np.array_equal(d32, want_d) and gap == want_gap
        assert np.array_equal(grp, np.where(ids >= 0, ids - 7, -1))


def test_one_group_gives_a_list_of_length_one(spread64):
    a, b = spread64
    ids, grp, d32, _ = GR.reference_search_grouped(a[:257], b[:9], GR.make_groups("one", 257), 11)
    want_ids, want_d, _ = SR.reference_search(a[:257], b[:9], 1)
    assert np.array_equal(ids[:, :1], want_ids) and np.array_equal(d32[:, :1], want_d) and np.all(grp[:, 0] == 5)
    assert np.all(ids[:, 1:] == -1) and np.all(grp[:, 1:] == -1) and np.all(np.isinf(d32[:, 1:]))


def test_ties_and_non_finite_rows():
    a, b = RR.spread_pairs(64, 64, 3)
    g = a.copy()
    g[7] = g[4]                                                # duplicates inside group 0 ...
    g[30] = g[20]                                              # ... and across groups 2 and 3
    groups = (np.arange(64) // 10).astype(np.int32)
    q = np.stack([g[4], g[20]])
    ids, grp, d64, _ = GR.reference_search_grouped64(g, q, groups, 3)
    assert ids[0, 0] == 4 and grp[0, 0] == 0 and ids[1, 0] == 20 and grp[1, 0] == 2 and d64[0, 0] == 0.0
    assert 3 in grp[1, 1:].tolist() and 30 in ids[1].tolist()         # group 3 is still there, by its row 30 at distance 0
    g[4, 0] = np.nan                                           # the best row of group 0 for query 0 has no distance
    ids, grp, _, _ = GR.reference_search_grouped64(g, q, groups, 3)
    assert ids[0, 0] == 7 and grp[0, 0] == 0
    g[:10] = np.nan                                            # a group of NaN rows only
    ids, grp, _, _ = GR.reference_search_grouped64(g, q, groups, 7)
    assert 0 not in grp[ids >= 0].tolist() and np.all((ids[:, 6] == -1) & (grp[:, 6] == -1))      # six groups are left
    assert GR.reference_nonfinite_bits(g, q) == 1 and GR.reference_nonfinite_bits(g, q, np.arange(64) >= 10) == 0


@pytest.mark.parametrize("n_windows", [2, 3, 7])
@pytest.mark.parametrize("kind", ["strided", "blocks_of_40", "random_50", "sparse_ids"])
def test_windows_merged_equal_the_whole(spread64, n_windows, kind):
    a, b = spread64
    ng, nq, depth = 1027, 9, 11
    groups = GR.make_groups(kind, ng, seed=4)
    live = _live("random_0.5", ng)
    whole = GR.reference_search_grouped64(a, b[:nq], groups, depth, live)
    cuts = [0] + [(ng * w // n_windows) | 1 for w in range(1, n_windows)] + [ng]      # odd rows: through blocks of 40 and pairs
    parts = []
    cut_through = False
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        cut_through |= 0 < lo < ng and groups[lo - 1] == groups[lo] or kind in ("strided", "random_50", "sparse_ids")
        parts.append(GR.reference_search_grouped64(a[lo:hi], b[:nq], groups[lo:hi], min(depth, hi - lo), live[lo:hi], id_base=lo)[:3])
    assert cut_through
    ids, grp, d64 = GR.merge_grouped_lists(parts, depth)
    assert np.array_equal(ids, whole[0]) and np.array_equal(grp, whole[1]) and np.array_equal(d64, whole[2])
