"""CPU: self-tests of the range search's numpy reference (tests/search_range_refs.py) on hand-made cases, so that the GPU tests compare
against something that is itself pinned: an empty result, everything a hit, a mask, a NaN row, a NaN query, NaN / negative / inf radii,
the margin and the midpoint radii."""
import numpy as np

import search_range_refs as RG
import search_refs as SR

# six gallery rows on a line: D(q, j) = (j + 1)^2 for the query at the origin, (j - 1)^2 for the query at 2 (64 columns, one used)
G = np.zeros((6, 64), np.float32)
G[:, 0] = np.arange(1, 7)
Q = np.zeros((2, 64), np.float32)
Q[1, 0] = 2


def test_distances_of_the_hand_made_case():
    D = SR.distances64(G, Q)
    assert np.array_equal(D[0], [1, 4, 9, 16, 25, 36]) and np.array_equal(D[1], [1, 0, 1, 4, 9, 16])


def test_hits_in_row_order_and_lims():
    lims, ids, d64, member, margin = RG.reference_range(G, Q, [10.0, 1.5], id_base=100)
    assert np.array_equal(lims, [0, 3, 6])
    assert np.array_equal(ids, [100, 101, 102, 100, 101, 102]) and ids.dtype == np.int64
    assert np.array_equal(d64, [1, 4, 9, 1, 0, 1])
    assert np.array_equal(member, [[1, 1, 1, 0, 0, 0], [1, 1, 1, 0, 0, 0]])
    assert margin == min(1 / 10.0, 0.5 / 1.5)


def test_the_comparison_is_inclusive():
    lims, ids, _, _, margin = RG.reference_range(G, Q[:1], 9.0)
    assert np.array_equal(lims, [0, 3]) and np.array_equal(ids, [0, 1, 2]) and margin == 0.0
    lims, ids, _, _, _ = RG.reference_range(G, Q[:1], np.nextafter(9.0, 0.0))
    assert np.array_equal(lims, [0, 2]) and np.array_equal(ids, [0, 1])


def test_empty_result_and_everything_a_hit():
    lims, ids, d64, member, _ = RG.reference_range(G, Q, [0.5, 100.0])
    assert np.array_equal(lims, [0, 0, 6]) and np.array_equal(ids, np.arange(6)) and not member[0].any() and member[1].all()
    lims, ids, d64, _, _ = RG.reference_range(G, Q, 0.5 * np.ones(2) * np.array([1.0, -1.0]))
    assert np.array_equal(lims, [0, 0, 0]) and ids.size == 0 and d64.size == 0 and ids.dtype == np.int64


def test_a_mask():
    live = np.array([0, 1, 0, 1, 1, 0], bool)
    lims, ids, d64, member, margin = RG.reference_range(G, Q, [20.0, 20.0], live=live)
    assert np.array_equal(lims, [0, 2, 5]) and np.array_equal(ids, [1, 3, 1, 3, 4]) and np.array_equal(d64, [4, 16, 0, 4, 9])
    assert margin == 4 / 20.0                                  # D = 16 of query 0, live; the dead row at 25 would not be nearer anyway
    lims, ids, _, _, margin = RG.reference_range(G, Q, 20.0, live=np.zeros(6, bool))
    assert np.array_equal(lims, [0, 0, 0]) and ids.size == 0 and margin == np.inf


def test_a_nan_row_and_a_nan_query():
    g = G.copy()
    g[1, 5] = np.nan
    g[2, 7] = np.inf
    lims, ids, _, member, _ = RG.reference_range(g, Q, np.inf)
    assert np.array_equal(lims, [0, 4, 8]) and np.array_equal(ids, [0, 3, 4, 5, 0, 3, 4, 5]) and not member[:, 1:3].any()
    q = Q.copy()
    q[0, 9] = np.nan
    lims, ids, _, _, _ = RG.reference_range(G, q, [np.inf, 1.5])
    assert np.array_equal(lims, [0, 0, 3]) and np.array_equal(ids, [0, 1, 2])


def test_nan_negative_and_inf_radius():
    lims, ids, _, member, margin = RG.reference_range(G, np.repeat(Q[:1], 3, 0), [np.nan, -1.0, np.inf])
    assert np.array_equal(lims, [0, 0, 0, 6]) and np.array_equal(ids, np.arange(6))
    assert margin == np.inf                                    # no finite non-negative radius: nothing is near a decision
    lims, _, _, _, _ = RG.reference_range(G, Q[1:], 0.0)      # radius 0 keeps an exact duplicate
    assert np.array_equal(lims, [0, 1])


def test_midpoint_radii_give_the_asked_counts_with_a_margin():
    rng = np.random.default_rng(0)
    g = rng.standard_normal((200, 64)).astype(np.float32)
    g[150] = g[3]                                              # an exact duplicate: one distinct distance, two rows
    q = rng.standard_normal((4, 64)).astype(np.float32)
    D = SR.distances64(g, q)
    counts = np.array([0, 1, 17, 500])
    r = RG.midpoint_radii(D, counts)
    lims, _, _, member, margin = RG.range_lists(D, r)
    assert margin > 1e-6
    got = np.diff(lims)
    assert got[0] == 0 and got[3] == 200
    for qi in (1, 2):                                          # counts distinct distances: rows 3 and 150 count once
        assert got[qi] == counts[qi] + int(member[qi, 3] and member[qi, 150])
    live = rng.random(200) < 0.5
    r = RG.midpoint_radii(D, 5, live=live)
    lims, ids, _, _, margin = RG.range_lists(D, r, live=live)
    assert margin > 1e-6 and live[ids].all() and np.all(np.diff(lims) >= 5)


def test_pack_words_is_the_row_mask_format():
    m = np.zeros(70, bool)
    m[[0, 31, 32, 69]] = True
    assert np.array_equal(RG.pack_words(m), np.array([0x80000001, 1, 1 << 5], np.uint32))
