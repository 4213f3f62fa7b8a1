"""CPU: the reference of the masked search holds together -- its two formulations agree (compaction + map back, and dead rows at +inf in
the full distance matrix) over the grid the GPU test uses, and the numpy packer that defines the word layout does what the header says."""
import numpy as np
import pytest

import rank_refs as RR
import search_mask_refs as MR


@pytest.fixture(scope="module")
def spread64():
    return RR.spread_pairs(1027, 64, 21)


@pytest.mark.parametrize("ng,nq,depth", MR.edge_cases())
def test_two_formulations_agree(spread64, ng, nq, depth):
    a, b = spread64
    for kind in MR.MASK_KINDS:
        live = MR.make_mask(kind, ng, seed=ng)
        ids, d32, gap = MR.reference_search_masked(a[:ng], b[:nq], live, depth, id_base=7)
        ids2, d32b, gap2 = MR.reference_search_masked_by_inf(a[:ng], b[:nq], live, depth, id_base=7)
        assert gap > 1e-12 and gap2 > 1e-12, (kind, gap, gap2)
        assert np.array_equal(ids, ids2), kind
        assert np.array_equal(d32.view(np.uint32), d32b.view(np.uint32)), kind
        n_live = int(live.sum())
        assert (ids[:, :min(depth, n_live)] >= 7).all() and (ids[:, n_live:] == -1).all() and np.isinf(d32[:, n_live:]).all()
        assert live[ids[ids >= 0] - 7].all()                  # only live rows are returned


def test_dead_rows_influence_nothing(spread64):
    a, b = spread64
    g = a[:257].copy()
    live = MR.make_mask("random_0.5", 257, seed=3)
    want = MR.reference_search_masked(g, b[:9], live, 11)
    dead = np.flatnonzero(~live)
    g[dead[0]] = np.nan
    g[dead[1]] = np.inf
    g[dead[2]] = b[0]                                         # distance 0 to query 0
    got = MR.reference_search_masked(g, b[:9], live, 11)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert MR.reference_nonfinite_bits(g, b[:9], live) == 0
    live[dead[0]] = True
    assert MR.reference_nonfinite_bits(g, b[:9], live) == 1
    assert dead[0] not in MR.reference_search_masked(g, b[:9], live, 11)[0]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 1027])
def test_packer_is_the_word_layout(n):
    flags = np.random.default_rng(n).random(n) < 0.5
    flags[-1] = True
    words = MR.pack_words(flags)
    assert words.dtype == np.uint32 and words.shape == ((n + 31) // 32,)
    for j in range(n):
        assert bool((int(words[j >> 5]) >> (j & 31)) & 1) == bool(flags[j])
    for j in range(n, 32 * words.size):                       # the bits past the last row are 0
        assert not (int(words[j >> 5]) >> (j & 31)) & 1
    assert np.array_equal(MR.pack_words(flags.astype(np.uint8) * 7), words)      # any non-zero flag is a set bit
