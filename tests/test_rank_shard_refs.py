"""CPU: the reference of the rank-sharded counting sweep is consistent with the paired one.  On every data set the sharded sweep's tests
run on, the partial column counts (tests/rank_shard_refs.py::partial_b) of windows that tile the rows add up to reference_ranks(a, b)[1],
element for element: for the shard_bounds cuts of worlds 1, 2, 3, 5 and 8 and for the cut lists the GPU tests use (a one-row shard at
either end, a cut through the exact duplicates and one through the dense cluster)."""
import numpy as np
import pytest

import rank_refs as RR
import rank_shard_refs as SR

WORLDS = (1, 2, 3, 5, 8)

CASES = [("spread", 1, 64, 11, 1.0), ("spread", 2, 64, 12, 1.0), ("spread", 65, 64, 75, 1.0), ("spread", 257, 64, 267, 1.0),
         ("spread", 1027, 64, 2, 1.0), ("spread", 1500, 512, 1, 1.0), ("cluster", 1500, 512, 5, 1.0), ("cluster", 1500, 512, 5, 25.0),
         ("midpoint", 1024, 512, 5, 1.0), ("nonfinite", 1027, 64, 2, 1.0)]


def _cut_lists(kind, n):
    cuts = [SR.shard_cuts(n, w) for w in WORLDS]
    if n >= 2:
        cuts += [[0, 1, n], [0, n - 1, n]]
    if n == 257:
        cuts += [[0, 255, 257], [0, 256, 257]]
    if kind == "cluster":
        cuts.append([0, 120, 1050, 1500])
    return cuts


def test_shard_cuts_are_shard_bounds():
    from vtc_amd import dist as vdist
    for n in (1, 2, 7, 65, 1027):
        for w in WORLDS:
            cuts = SR.shard_cuts(n, w)
            assert SR.windows(cuts) == [vdist.shard_bounds(n, r, w) for r in range(w)]
            assert cuts[0] == 0 and cuts[-1] == n and all(lo <= hi for lo, hi in SR.windows(cuts))


@pytest.mark.parametrize("kind,n,d,seed,scale", CASES)
def test_partials_sum_to_the_paired_reference(kind, n, d, seed, scale):
    a, b, _, want_b = SR.case(kind, n, d, seed, scale)
    D, dt, bad_b = SR.column_direction(a, b)
    for cuts in _cut_lists(kind, n):
        parts = [SR.partial_from(D, dt, bad_b, lo, hi) for lo, hi in SR.windows(cuts)]
        assert all(p.dtype == np.int64 and p.shape == (n,) and (p >= 0).all() for p in parts)
        assert np.array_equal(np.sum(parts, axis=0), want_b), cuts
    if kind == "nonfinite":
        # the owner-writes-n rule: the window that holds a dead pair's row carries its whole rank
        for j in (333, 700):
            assert want_b[j] == n
            for lo, hi in SR.windows(SR.shard_cuts(n, 3)):
                assert SR.partial_from(D, dt, bad_b, lo, hi)[j] == (n if lo <= j < hi else 0)
    if kind == "cluster":
        # the cut at 1050 runs through the dense cluster: the rows 1000 .. 1099 are split 0 / 51 / 49 where the rank is largest
        assert want_b[99:104].tolist() == [0, 1, 2, 3, 4] and want_b[1000:1100].max() == 100
        j = 1000 + int(np.argmax(want_b[1000:1100]))
        assert [int(SR.partial_from(D, dt, bad_b, lo, hi)[j]) for lo, hi in SR.windows([0, 120, 1050, 1500])] == [0, 51, 49]


def test_partial_b_is_the_one_shot_form():
    a, b, _, _ = SR.case("spread", 65, 64, 75)
    assert np.array_equal(SR.partial_b(a, b, 10, 40), SR.partials(a, b, [0, 10, 40, 65])[1])
    assert not SR.partial_b(a, b, 65, 65).any()              # an empty window counts nothing
