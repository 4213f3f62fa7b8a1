"""CPU: the reference of the half-storage search (tests/search_half_refs.py).  numpy's fp32 -> binary16 rounding is torch's -- what
VideoIndex.add stores --, widening is exact, the references over widened rows are the fp32 ones, and every shape the GPU tests compare
ids on keeps min_gap > 1e-12 on this machine's CPU."""
import numpy as np
import pytest
import torch

import search_grouped_refs as GR
import search_half_refs as HR
import search_mask_refs as MR
import search_refs as SR


def test_numpy_rounds_to_half_as_torch_does():
    ulp1 = 2.0 ** -10                                         # the half ulp in [1, 2)
    x = np.array([
        1 + ulp1 / 2, 1 + 3 * ulp1 / 2, 1 + ulp1 / 2 + 2.0 ** -20, 1 + ulp1 / 2 - 2.0 ** -20,      # halfway: to even, both ways; just off it
        -(1 + ulp1 / 2), -(1 + 3 * ulp1 / 2),
        2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001, 3 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -26,      # subnormals
        65504.0, -65504.0, 65519.0, 65520.0, -65520.0, 1e5, -0.0, 0.0, 1.0 / 3.0, 0.044194173,
    ], np.float32)
    got = HR.round_half(x)
    want = torch.from_numpy(x).to(torch.float16).numpy()
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), (got, want)
    # what the table is there for
    assert got[0] == np.float16(1.0) and got[1] == np.float16(1 + 2 * ulp1) and got[2] == np.float16(1 + ulp1) and got[3] == np.float16(1.0)
    assert got[6] == HR.SUBNORMAL_MIN and got[7] == 0 and got[8] == HR.SUBNORMAL_MIN and got[10] == HR.SUBNORMAL_MAX
    assert got[13] == HR.HALF_MAX and got[15] == HR.HALF_MAX and np.isposinf(got[16]) and np.isneginf(got[17]) and np.isposinf(got[18])
    assert np.signbit(got[19]) and got[19] == 0 and not np.signbit(got[20])


def test_widening_is_exact_for_every_half():
    every = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    wide = HR.widen(every)
    assert wide.dtype == np.float32
    back = wide.astype(np.float16)
    fin = ~np.isnan(every)
    assert np.array_equal(back.view(np.uint16)[fin], every.view(np.uint16)[fin]) and np.isnan(wide[~fin]).all()
    assert np.array_equal(wide[fin].astype(np.float64), every[fin].astype(np.float64))
    assert np.array_equal(torch.from_numpy(every).float().numpy()[fin], wide[fin])
    with pytest.raises(AssertionError):
        HR.widen(np.zeros(3, np.float32))


def test_the_references_are_the_fp32_ones_over_the_widened_rows():
    g, q = HR.shape_case(64, 257, 5, 11)
    live = MR.make_mask("random_0.5", 257, seed=3)
    groups = GR.make_groups("strided", 257)
    for got, want in ((HR.reference_search64(g, q, 11, 7), SR.reference_search64(g.astype(np.float32), q, 11, 7)),
                      (HR.reference_search_masked(g, q, live, 11), MR.reference_search_masked(g.astype(np.float32), q, live, 11)),
                      (HR.reference_search_grouped64(g, q, groups, 11, live), GR.reference_search_grouped64(g.astype(np.float32), q, groups, 11, live))):
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
    bad = g.copy()
    bad[100, 3] = np.float16(np.inf)
    assert HR.reference_nonfinite_bits(bad, q) == 1 and HR.reference_nonfinite_bits(bad, q, live=np.arange(257) != 100) == 0


def test_special_rows_hold_what_they_say():
    g, q = HR.shape_case(64, 33, 4, 33)
    w = HR.widen(g)
    tiny = 2.0 ** -14
    assert np.any((np.abs(w[0]) > 0) & (np.abs(w[0]) < tiny)) and np.any((np.abs(w[1]) > 0) & (np.abs(w[1]) < tiny))
    assert w[2].max() == 65504.0 and w[2].min() == -65504.0 and np.any(np.signbit(w[2]) & (w[2] == 0))
    assert all(np.array_equal(g[r].view(np.uint16), g[6].view(np.uint16)) for r in (3, 4, 5))
    assert int((g[7] != g[8]).sum()) == 1 and int((g[9] != g[10]).sum()) == 1
    D = SR.distances64(w, q)
    assert np.all(D[:, 3] == D[:, 6]) and np.all(D[:, 9] != D[:, 10])
    assert np.array_equal(D[:, 9].astype(np.float32), D[:, 10].astype(np.float32))       # below the fp32 resolution of the distance
    ids, _, gap = HR.reference_search64(g, q, 33, id_base=2 ** 33)
    assert gap > 1e-12
    for i in range(4):                                        # the duplicates come back in row order
        pos = [int(np.flatnonzero(ids[i] == 2 ** 33 + r)[0]) for r in (3, 4, 5, 6)]
        assert pos == list(range(pos[0], pos[0] + 4))


def test_min_gap_of_the_large_case():
    g, q = HR.large_case()
    ng = g.shape[0]
    ids, _, gap = HR.reference_search64(g, q, 11)
    assert gap > 1e-12 and ids[0, 0] == ng - 1
    live = MR.make_mask("random_0.5", ng, seed=2) | (np.arange(ng) == ng - 1)
    assert HR.reference_search_grouped64(g, q[:2], (np.arange(ng) // 5).astype(np.int32), 11, live)[3] > 1e-12


@pytest.mark.parametrize("d,ng,nq,depth", HR.SHAPES)
def test_min_gap_of_every_shape_the_gpu_tests_use(d, ng, nq, depth):
    g, q = HR.shape_case(d, ng, nq, depth)
    assert g.dtype == np.float16 and g.shape == (ng, d) and q.dtype == np.float32 and q.shape == (nq, d)
    assert HR.reference_search64(g, q, depth)[2] > 1e-12
    if ng >= 33:
        for mk in ("alt_bits", "random_0.5"):
            assert HR.reference_search_masked(g, q, MR.make_mask(mk, ng, seed=ng), min(depth, ng), 0)[2] > 1e-12
        for gk in ("strided", "sparse_ids"):
            assert HR.reference_search_grouped64(g, q, GR.make_groups(gk, ng, seed=ng), depth)[3] > 1e-12
