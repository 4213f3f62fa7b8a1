"""CPU: tests/search_after_refs.py against a brute-force slice of the full order, and the gap condition of the data the GPU tests use
(tests/test_gpu_search_after.py) at FULL depth -- a page can begin anywhere in a query's order."""
import numpy as np
import pytest

import rank_refs as RR
import search_after_refs as AR
import search_mask_refs as MR
import search_refs as SR


def _brute(gallery, queries, depth, after_ids, live, id_base):
    """Python, one key at a time: sort every live finite row by (D, row), cut everything up to the cursor's key."""
    D = SR.distances64(gallery, queries)
    n = D.shape[1]
    ids = np.full((len(queries), depth), -1, np.int64)
    d64 = np.full((len(queries), depth), np.inf)
    for i in range(len(queries)):
        a = int(after_ids[i]) - id_base
        if not 0 <= a < n:
            continue
        keys = sorted((D[i, j], j) for j in range(n) if np.isfinite(D[i, j]) and (live is None or live[j]))
        rest = [k for k in keys if k > (D[i, a], a)][:depth]
        for p, (dv, j) in enumerate(rest):
            ids[i, p], d64[i, p] = id_base + j, dv
    return ids, d64


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("id_base", [0, 1000])
def test_reference_against_brute_force(masked, id_base):
    a, b = RR.spread_pairs(203, 64, 7)
    a[17, 5] = np.nan                                          # a row without a distance is in nobody's order
    live = MR.make_mask("random_0.5", 203, seed=3) if masked else None
    rng = np.random.default_rng(1)
    after = id_base + rng.integers(0, 203, 6)
    after[1], after[2], after[3] = -1, id_base + 203, id_base - 1 if id_base else -7
    if masked:
        after[4] = id_base + np.flatnonzero(~live)[3]         # a dead cursor row still has a key
    got_i, got_d, _ = AR.reference_search_after(a, b[:6], 9, after, live, id_base)
    want_i, want_d = _brute(a, b[:6], 9, after, live, id_base)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_d, want_d)
    assert (got_i[1:4] == -1).all() and (got_i[0] >= 0).any()


def test_pages_concatenate_to_the_full_order():
    a, b = RR.spread_pairs(131, 64, 8)
    g = AR.tied_gallery(a[:40], 2)                             # 200 rows, every distance five times
    order, d64, _ = AR.full_order(g, b[:3])
    pages, after = [order[:, :7]], order[:, 6]
    while pages[-1][0, -1] >= 0:
        ids, _, _ = AR.reference_search_after(g, b[:3], 7, after)
        pages.append(ids)
        after = ids[:, -1]
    cat = np.concatenate(pages, axis=1)
    assert np.array_equal(cat[:, :200], order) and (cat[:, 200:] == -1).all()
    tie = d64[:, 1:] == d64[:, :-1]
    assert tie.mean() > 0.7 and (order[:, 1:][tie] > order[:, :-1][tie]).all()      # exact ties, ordered by row


def test_the_gpu_tests_data_is_decided_at_full_depth():
    a, b = RR.spread_pairs(1027, 64, 21)
    assert AR.full_order(a, b[:9])[2] > 1e-9
    assert AR.full_order(a.astype(np.float16).astype(np.float32), b[:9])[2] > 1e-9
    assert AR.full_order(AR.tied_gallery(a[:200], 21), b[:5])[2] > 1e-9
