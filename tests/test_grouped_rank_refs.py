"""CPU: the fp64 reference of the grouped rank sweep (tests/grouped_rank_refs.py) on a hand-written case and against the paired reference,
the host helper that turns the reference's -inf-padded caption tensor into offsets, and the host-side validation of the multi-caption
entry points, which raises before any device is touched (this file runs without a GPU)."""
import numpy as np
import pytest
import torch

import grouped_rank_refs as GR
import rank_refs as RR


def _hand_case():
    """Three videos (the last two identical), two captions each.
    D(c, j):           a0 = (0,0)   a1 = (4,0)   a2 = (4,0)
      b0 = (1,0)            1            9            9       video 0
      b1 = (1,0)            1            9            9       video 0: a bit-equal copy of b0 inside the group
      b2 = (3,0)            9            1            1       video 1
      b3 = (1,0)            1            9            9       video 1: a copy of b0 / b1 in another group
      b4 = (3,0)            9            1            1       video 2: a copy of b2 in another group
      b5 = (10,0)         100           36           36       video 2"""
    a = np.array([[0, 0], [4, 0], [4, 0]], np.float32)
    b = np.array([[1, 0], [1, 0], [3, 0], [1, 0], [3, 0], [10, 0]], np.float32)
    return a, b, np.array([0, 2, 4, 6], np.int64)


def test_hand_written_case():
    a, b, off = _hand_case()
    rank_a, rank_b, _ = GR.reference_grouped_ranks(a, b, off)
    # text -> video.  b2: a2 ties with the target a1 but has the higher index.  b3: a0 is closer than its own video a1.
    # b4, b5 (video 2): the identical video a1 ties with the target a2 and has the lower index.
    assert rank_a.tolist() == [0, 0, 0, 1, 1, 1]
    # video -> text.  video 0: b0 and b1 tie, c* = b0 (the lower index); b1 (own) and b3 (another group's copy, higher index) do not count.
    # video 1: c* = b2; its copy b4 has the higher index.  video 2: c* = b4; its copy b2, in another group, has the LOWER index: counted.
    assert rank_b.tolist() == [0, 0, 1]
    # the same with video 0's captions swapped for far ones: its best own caption, b1, is behind b3 only
    b2 = b.copy()
    b2[0], b2[1] = (0, 7), (0, 2)
    rank_a, rank_b, _ = GR.reference_grouped_ranks(a, b2, off)
    assert rank_a.tolist() == [0, 0, 0, 1, 1, 1] and rank_b.tolist() == [1, 0, 1]


def test_hand_written_nonfinite_and_empty_groups():
    a, b, off = _hand_case()
    b = b.copy()
    b[2, 0] = np.nan                                      # video 1's best caption: rank_a = n; c* falls to b3 (distance 9)
    rank_a, rank_b, _ = GR.reference_grouped_ranks(a, b, off)
    assert rank_a.tolist() == [0, 0, 3, 1, 1, 1]
    assert rank_b.tolist() == [0, 3, 0]                   # column a1: b4 is closer (1 < 9), b0 and b1 tie at 9 with lower indices; the NaN row never is
    rank_a, rank_b, _ = GR.reference_grouped_ranks(a, b[[0, 1, 4, 5]], np.array([0, 2, 2, 4]))      # video 1 has no caption at all
    assert rank_a.tolist() == [0, 0, 1, 1] and rank_b.tolist() == [0, 4, 0]


def test_padded_reference_tensor_becomes_offsets():
    from vtc_amd.host.retrieval_evaluation import padded_captions_to_offsets
    counts = [1, 4, 2, 3]
    a, b, off = GR.grouped_spread(counts, 64, 5)
    padded = GR.pad_captions(b, off)
    assert padded.shape == (4, 4, 64) and np.isneginf(padded[0, 1:]).all() and np.isneginf(padded[2, 2:]).all()
    flat, got = padded_captions_to_offsets(torch.from_numpy(padded))
    assert got.tolist() == off.tolist() == [0, 1, 5, 7, 10]
    assert np.array_equal(flat.numpy(), b)
    flat, got = padded_captions_to_offsets(padded)          # numpy, as the reference's .numpy() hands it over
    assert got.tolist() == off.tolist() and np.array_equal(flat.numpy(), b)
    one = b[:4].copy()
    one[1, 3] = -np.inf                                     # a caption with ONE -inf entry is data (bad data), not padding
    flat, got = padded_captions_to_offsets(one[:, None, :])
    assert got.tolist() == [0, 1, 2, 3, 4]


def test_identity_offsets_reproduce_the_paired_reference():
    n = 300
    a, b = RR.spread_pairs(n, 64, 3)
    want_a, want_b, gap = RR.reference_ranks(a, b)
    got_a, got_b, ggap = GR.reference_grouped_ranks(a, b, np.arange(n + 1))
    assert gap > 1e-12 and ggap > 1e-12
    RR.assert_not_degenerate(want_a, n)
    RR.assert_not_degenerate(want_b, n)
    assert np.array_equal(got_a, want_a) and np.array_equal(got_b, want_b)


def test_grouped_spread_is_not_degenerate():
    """The generator's point: ranks leave the top in BOTH directions (a per-video noise scale), and the gaps are wide."""
    counts = GR.ragged_counts(65, 1, 4, 165)
    a, b, off = GR.grouped_spread(counts, 64, 165)
    n, m = a.shape[0], b.shape[0]
    assert off[-1] == m == counts.sum() and np.allclose(np.linalg.norm(b, axis=1), 1.0, atol=1e-6)
    rank_a, rank_b, gap = GR.reference_grouped_ranks(a, b, off)
    assert gap > 1e-12
    assert rank_a.max() > n / 2 and rank_b.max() > m / 2
    assert 0.2 < (rank_a < 1).mean() < 0.8 and 0.2 < (rank_b < 1).mean() < 0.8


def test_offsets_are_validated_on_the_host_before_anything_is_launched():
    """CPU tensors throughout: a call that got past the validation would fail on the missing GPU with another exception."""
    from vtc_amd import ops
    from vtc_amd.host.metric import RecallAtK
    from vtc_amd.host.retrieval_evaluation import compute_multi_caption_table
    a, b = torch.zeros(3, 64), torch.zeros(6, 64)
    for bad, what in (([0, 2, 6], "expected 4 entries"), ([0, 2, 4, 6, 6], "expected 4 entries"), ([1, 2, 4, 6], "start at 0"),
                      ([0, 2, 4, 5], "end at the number of captions"), ([0, 4, 2, 6], "non-decreasing"),
                      (torch.tensor([0, 2, 4, 7]), "end at the number of captions"), (np.array([0.0, 1.5, 4.0, 6.0]), "integers")):
        with pytest.raises(ValueError, match=what):
            ops.rank_grouped(a, b, bad)
        with pytest.raises(ValueError, match=what):
            RecallAtK("videos", "titles", [1]).grouped_ranks(a.numpy(), b.numpy(), bad)
    with pytest.raises(ValueError, match="video 1 has no caption"):              # allowed at the ABI, a data error in the metric
        RecallAtK("videos", "titles", [1]).grouped_ranks(a, b, [0, 2, 2, 6])
    with pytest.raises(ValueError, match="flat"):
        compute_multi_caption_table(a, torch.zeros(3, 2, 64), offsets=[0, 2, 4, 6])
    with pytest.raises(ValueError, match="padded captions"):
        compute_multi_caption_table(a, b)                                         # flat captions without offsets
    with pytest.raises(ValueError, match="video 1 has no caption"):
        padded = torch.zeros(3, 2, 64)
        padded[1] = float("-inf")
        compute_multi_caption_table(a, padded)


def test_the_table_is_exported_from_both_modules_and_the_default_path_keeps_its_assertion():
    import evaluation.retrieval_evaluation as front
    from vtc_amd.host import retrieval_evaluation as RE
    assert front.compute_multi_caption_table is RE.compute_multi_caption_table
    item = (torch.zeros(8, 3, 4, 4), torch.zeros(2, 77, dtype=torch.int64), "id")
    with pytest.raises(AssertionError, match="one caption per video"):
        RE._item_parts(item)
    fr, cap, com = RE._item_parts(item, multi_caption=True)
    assert cap.shape == (2, 77) and com is None
    assert RE._item_parts((item[0], item[1][0], "id"), multi_caption=True)[1].shape == (1, 77)
