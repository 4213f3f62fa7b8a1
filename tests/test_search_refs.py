"""The numpy reference of the query-time search (tests/search_refs.py) against plain Python and against the rank family's reference."""
import numpy as np

import rank_refs as RR
import search_refs as SR


def test_reference_matches_a_plain_python_sort():
    rng = np.random.default_rng(0)
    g = rng.standard_normal((7, 64)).astype(np.float32)
    q = rng.standard_normal((5, 64)).astype(np.float32)
    ids, dists, gap = SR.reference_search(g, q, 4, id_base=100)
    assert gap > 1e-12
    for i in range(5):
        keyed = sorted((sum((float(q[i, k]) - float(g[j, k])) ** 2 for k in range(64)), j) for j in range(7))
        assert [100 + j for _, j in keyed[:4]] == ids[i].tolist()
        assert np.allclose([v for v, _ in keyed[:4]], dists[i], rtol=1e-6)


def test_duplicates_go_to_the_lower_index():
    rng = np.random.default_rng(1)
    g = rng.standard_normal((9, 64)).astype(np.float32)
    g[6] = g[2]
    g[4] = g[2]
    ids, dists, _ = SR.reference_search(g, g[2:3], 3)
    assert ids[0].tolist() == [2, 4, 6] and np.all(dists[0] == 0)


def test_nan_gallery_row_is_never_returned_and_the_tail_is_padded():
    rng = np.random.default_rng(2)
    g = rng.standard_normal((5, 64)).astype(np.float32)
    g[1, 3] = np.nan
    g[3, 0] = np.inf
    ids, dists, _ = SR.reference_search(g, g[[0, 2]], 5)
    for row in ids:
        assert sorted(row[:3].tolist()) == [0, 2, 4] and row[3:].tolist() == [-1, -1]
    assert np.all(np.isinf(dists[:, 3:])) and np.all(np.isfinite(dists[0, :3]))


def test_nan_query_gets_an_empty_row():
    rng = np.random.default_rng(3)
    g = rng.standard_normal((6, 64)).astype(np.float32)
    q = rng.standard_normal((2, 64)).astype(np.float32)
    q[1, 5] = np.nan
    ids, dists, _ = SR.reference_search(g, q, 3)
    assert ids[1].tolist() == [-1, -1, -1] and np.all(np.isinf(dists[1])) and np.all(ids[0] >= 0)


def test_windows_merged_on_fp64_equal_the_whole_search():
    rng = np.random.default_rng(4)
    g = rng.standard_normal((10, 64)).astype(np.float32)
    g[7] = g[1]                                               # a duplicate across a cut
    q = np.concatenate([g[1:2], rng.standard_normal((3, 64)).astype(np.float32)])
    cuts = [0, 3, 4, 10]
    parts = [SR.reference_search64(g[lo:hi], q, min(4, hi - lo), id_base=lo)[:2] for lo, hi in zip(cuts[:-1], cuts[1:])]
    ids, d64 = SR.merge_lists(parts, 4)
    want_ids, want_d64, _ = SR.reference_search64(g, q, 4)
    assert np.array_equal(ids, want_ids) and np.array_equal(d64, want_d64)
    assert ids[0, :2].tolist() == [1, 7]


def test_lists_agree_with_the_rank_reference_on_paired_data():
    a, b = RR.spread_pairs(300, 64, 11)
    rank_a, _, gap_r = RR.reference_ranks(a, b)
    depth = 11
    ids, _, gap = SR.reference_search(a, b, depth)
    assert gap > 1e-12 and gap_r > 1e-12
    assert (rank_a < depth).any() and (rank_a >= depth).any()
    for i in range(300):
        if rank_a[i] < depth:
            assert ids[i, rank_a[i]] == i
        else:
            assert i not in ids[i]


def test_the_gpu_cases_have_no_near_ties():
    """min_gap > 1e-12 on the data of tests/test_gpu_search.py that is cheap to check here (the GPU tests assert it on every case)."""
    a, b = RR.cluster_case(1500, 512)
    assert SR.reference_search(a, b[90:154], 64)[2] > 1e-12
    a, b = RR.unrelated_pairs(257, 64, 3)
    assert SR.reference_search(a, b[:9], 11)[2] > 1e-12
