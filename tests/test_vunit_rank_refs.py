"""CPU: the fp64 reference of the video-unit video -> text ranks (tests/vunit_rank_refs.py) against a literal triple loop on hand-made
inputs, the properties the definition implies on every data set the GPU tests run on (tests/vunit_cases.py), and the host-side checks of
the new entry points, which raise before any device is touched (this file runs without a GPU)."""
import numpy as np
import pytest
import torch

import grouped_rank_refs as GR
import vunit_cases as VC
import vunit_rank_refs as VR


def _triple_loop(a, b, off):
    """rank_v by the definition, one scalar at a time."""
    n = len(a)
    D = [[float(sum((np.float64(x) - np.float64(y)) ** 2 for x, y in zip(b[c], a[v]))) for v in range(n)] for c in range(len(b))]

    def E(u, v):
        best = np.inf
        for c in range(off[u], off[u + 1]):
            if np.isfinite(D[c][v]) and D[c][v] < best:
                best = D[c][v]
        return best
    out = []
    for v in range(n):
        t = E(v, v)
        if not np.isfinite(t):
            out.append(n)
            continue
        r = 0
        for u in range(n):
            e = E(u, v)
            if u != v and np.isfinite(e) and (e < t or (e == t and u < v)):
                r += 1
        out.append(r)
    return out


def _hand_case():
    """tests/test_grouped_rank_refs.py's: three videos (the last two identical), two captions each.
    D(c, j):           a0 = (0,0)   a1 = (4,0)   a2 = (4,0)
      b0 = (1,0)            1            9            9       video 0
      b1 = (1,0)            1            9            9       video 0
      b2 = (3,0)            9            1            1       video 1
      b3 = (1,0)            1            9            9       video 1: a copy of video 0's captions
      b4 = (3,0)            9            1            1       video 2: a copy of b2
      b5 = (10,0)         100           36           36       video 2"""
    a = np.array([[0, 0], [4, 0], [4, 0]], np.float32)
    b = np.array([[1, 0], [1, 0], [3, 0], [1, 0], [3, 0], [10, 0]], np.float32)
    return a, b, np.array([0, 2, 4, 6], np.int64)


def test_hand_written_cases_against_the_triple_loop():
    a, b, off = _hand_case()
    # E:         v0  v1  v2      video 0: group 1 ties at 1 with the HIGHER video index: not closer.  video 1: group 2 ties at 1, higher index.
    #   group 0   1   9   9      video 2: group 1 ties at 1 with the lower index: closer.
    #   group 1   1   1   1
    #   group 2   9   1   1
    assert VR.reference_vunit_ranks(a, b, off).tolist() == [0, 0, 1] == _triple_loop(a, b, off)
    b2 = b.copy()
    b2[0], b2[1] = (0, 7), (0, 2)                          # video 0's captions far: E(0, 0) = 4, group 1 (distance 1) is closer
    assert VR.reference_vunit_ranks(a, b2, off).tolist() == [1, 0, 1] == _triple_loop(a, b2, off)
    # two captions of ONE other group closer: the group counts once (caption level: twice)
    a3 = np.array([[0, 0], [9, 0]], np.float32)
    b3 = np.array([[5, 0], [1, 0], [2, 0], [8, 0]], np.float32)
    off3 = np.array([0, 1, 4], np.int64)
    assert VR.reference_vunit_ranks(a3, b3, off3).tolist() == [1, 0] == _triple_loop(a3, b3, off3)
    assert GR.reference_grouped_ranks(a3, b3, off3)[1].tolist() == [2, 0]
    # ragged, random, with duplicates across groups
    rng = np.random.default_rng(5)
    a4 = rng.integers(0, 3, (7, 3)).astype(np.float32)
    b4 = rng.integers(0, 3, (15, 3)).astype(np.float32)
    off4 = np.array([0, 1, 4, 4, 8, 9, 13, 15], np.int64)
    assert VR.reference_vunit_ranks(a4, b4, off4).tolist() == _triple_loop(a4, b4, off4)
    assert VR.reference_vunit_ranks(a4, b4, off4)[2] == 7       # the empty group


def test_hand_written_nonfinite_and_empty_groups():
    a, b, off = _hand_case()
    b = b.copy()
    b[2, 0] = np.nan                                      # video 1's best caption: E(1, 1) falls to b3 (9); groups 0 (9, lower index) and 2 (1) are closer
    assert VR.reference_vunit_ranks(a, b, off).tolist() == [0, 2, 0] == _triple_loop(a, b, off)
    off2 = np.array([0, 2, 2, 4])                         # video 1 has no caption at all: rank n, and its group is never closer
    assert VR.reference_vunit_ranks(a, b[[0, 1, 4, 5]], off2).tolist() == [0, 3, 0] == _triple_loop(a, b[[0, 1, 4, 5]], off2)
    a2 = a.copy()
    a2[0, 1] = np.nan                                     # a NaN video row: rank n; nobody else is affected
    assert VR.reference_vunit_ranks(a2, _hand_case()[1], off).tolist() == [3, 0, 1]


def test_all_equal_rows_rank_by_video_index():
    n = 32
    rank_v = VR.reference_vunit_ranks(np.zeros((n, 64), np.float32), np.zeros((2 * n, 64), np.float32), np.arange(0, 2 * n + 1, 2))
    assert rank_v.tolist() == list(range(n))


@pytest.mark.parametrize("kind,n,d", [c[:3] for c in VC.EDGE + VC.BULK])
def test_properties_on_the_spread_cases(kind, n, d):
    a, b, off, rank_a, rank_b, rank_v = VC.case(kind, n, d)
    VC.assert_properties(rank_b, rank_v)
    VC.assert_not_degenerate(rank_v, rank_b, n)


def test_properties_on_the_big_group_case():
    a, b, off, rank_a, rank_b, rank_v = VC.big_group_case()
    assert b.shape[0] == 1053 and off[11] - off[10] == 600 and off[38] - off[37] == 300
    VC.assert_properties(rank_b, rank_v)
    VC.assert_not_degenerate(rank_v, rank_b, 64)


@pytest.mark.parametrize("n,d", VC.IDENTITY)
def test_identity_offsets_reproduce_the_paired_reference(n, d):
    a, b, rank_a, rank_b = VC.identity_case(n, d)
    rank_v = VR.reference_vunit_ranks(a, b, np.arange(n + 1))
    assert np.array_equal(rank_v, rank_b)
    VC.assert_properties(rank_b, rank_v)


@pytest.mark.parametrize("scale", [1.0, 25.0])
def test_properties_and_plants_of_the_ties_case(scale):
    kappa = 3.0 / 65536.0 + 4.0 * 128 / 16777216.0 + 1e-6          # vtc_l2_rank_kappa(128), in fp64 (the GPU test asks the library)
    a, b, off, rank_a, rank_b, rank_v = VC.assert_ties_case(scale, kappa)
    VC.assert_properties(rank_b, rank_v)


def test_properties_on_the_nonfinite_cases():
    for name, a, b, off, rank_a, rank_b, rank_v, bits, idx in VC.nonfinite_cases():
        n = a.shape[0]
        VC.assert_properties(rank_b, rank_v)
        if name == "nan_caption":
            assert rank_v[idx] < n
        else:
            assert rank_v[idx] == n and (np.delete(rank_v, idx) < n).all()


def test_an_unknown_convention_is_refused_before_any_device_work():
    """CPU tensors throughout: a call that got past the check would fail on the missing GPU with another exception."""
    from vtc_amd.host.metric import RecallAtK
    from vtc_amd.host.retrieval_evaluation import compute_multi_caption_table
    a, b = torch.zeros(3, 64), torch.zeros(6, 64)
    with pytest.raises(ValueError, match="video_to_text"):
        RecallAtK("videos", "titles", [1]).grouped_ranks(a, b, [0, 2, 4, 6], video_to_text="bogus")
    with pytest.raises(ValueError, match="video_to_text"):
        compute_multi_caption_table(a, b, offsets=[0, 2, 4, 6], video_to_text="bogus")
    with pytest.raises(ValueError, match="video 1 has no caption"):
        RecallAtK("videos", "titles", [1]).grouped_ranks(a, b, [0, 2, 2, 6], video_to_text="video")


def test_offsets_are_validated_on_the_host_before_anything_is_launched():
    from vtc_amd import ops
    a, b = torch.zeros(3, 64), torch.zeros(6, 64)
    for bad, what in (([0, 2, 6], "expected 4 entries"), ([1, 2, 4, 6], "start at 0"), ([0, 2, 4, 5], "end at the number of captions"),
                      ([0, 4, 2, 6], "non-decreasing"), (np.array([0.0, 1.5, 4.0, 6.0]), "integers")):
        with pytest.raises(ValueError, match=what):
            ops.rank_grouped_vunit(a, b, bad)
    with pytest.raises(ValueError, match="a \\[n, d\\] and b \\[m, d\\]"):
        ops.rank_grouped_vunit(a, torch.zeros(6, 32), [0, 2, 4, 6])


def test_the_new_names_are_declared():
    from vtc_amd import _lib as L
    assert {"vtc_l2_rank_grouped_vunit", "vtc_l2_rank_grouped_vunit_workspace_bytes"} <= set(L.SIGNATURES)
    assert len(L.SIGNATURES["vtc_l2_rank_grouped_vunit"][1]) == len(L.SIGNATURES["vtc_l2_rank_grouped"][1]) + 1
