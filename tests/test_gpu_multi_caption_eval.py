"""GPU: retrieval_evaluation(..., multi_caption=True) -- several captions per video through the towers, the CAM and the grouped rank
sweep -- against the oracle running the reference's per-video batch-1 loop (evaluation/retrieval_evaluation.py:143-260, which takes
[ncap, 77] captions) and the fp64 grouped ranks of the embeddings the run returns."""
import numpy as np
import pytest
import torch
from pandas.testing import assert_frame_equal

import grouped_rank_refs as GR
from oracle import arch as A
from oracle import eval_ref as E
from oracle import model_ref as M
from test_gpu_retrieval_eval import _build

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL = 1e-5                       # the fp32-mode tolerance of tests/test_gpu_retrieval_eval.py


def _items(a, counts, seed, with_comments):
    """Stand-in sized videos (1 .. 3 chunks, ragged tails) with counts[i] captions each; every second one carries real comments."""
    frames = [40, 16 * 8, 16 * 9 + 3, 50, 16 * 17, 129]
    items = []
    for i, ncap in enumerate(counts):
        fr = A.synth_pixels((frames[i % len(frames)], 3, a.image_resolution, a.image_resolution), seed + i)
        cap = A.synth_tokens(ncap, a, seed + 100 + i)
        if with_comments and i % 2 == 0:
            items.append((fr, cap, A.synth_tokens(5, a, seed + 200 + i, empty_frac=0.3), f"v{i}"))
        else:
            items.append((fr, cap, f"v{i}"))
    return items


def _check_table(df, v_emb, c_emb, offsets, name="videos", split="full-test"):
    """The table is computed from the GPU's embeddings: hold it to the fp64 grouped ranks of THOSE embeddings."""
    want_a, want_b, gap = GR.reference_grouped_ranks(v_emb.cpu().numpy(), c_emb.cpu().numpy(), offsets)
    assert gap > 1e-12, gap
    assert_frame_equal(df, GR.table_from_ranks(want_a, want_b, split, name), check_exact=True)


@pytest.mark.parametrize("cls_name,kind,branch", [("PretrainedCLIP_TimeSformer", "timesformer", None),
                                                  ("PretrainedCLIP_finaltf", "clip_finaltf", "text"),
                                                  ("PretrainedCLIP_finaltf", "clip_finaltf", "image")])
def test_three_captions_per_video_vs_the_per_video_loop(cls_name, kind, branch):
    from evaluation.retrieval_evaluation import retrieval_evaluation
    a = A.TINY
    cam = branch is not None
    m, sd = _build(kind, cls_name, a, 81, **(dict(branch_to_adapt_val=branch, n_heads=2) if cam else {}))
    items = _items(a, [3] * 6, 700, cam)
    df, v_emb, c_emb, offsets = retrieval_evaluation(m, items, "full-test", "cuda", return_embeddings=True, multi_caption=True)
    assert offsets.tolist() == [0, 3, 6, 9, 12, 15, 18] and v_emb.shape[0] == 6 and c_emb.shape[0] == 18
    if cam:
        fwd = lambda fr, cap, com: M.pretrained_clip_finaltf(fr, cap, com, sd, a, branch, n_heads=2)[:2]      # noqa: E731
    else:
        fwd = lambda fr, cap, com: M.pretrained_clip_timesformer(fr, cap, sd, a)[:2]                          # noqa: E731
    ref_v, ref_c = E.retrieval_evaluation_loop(fwd, items, cam, branch or "text")                              # [6, D], [6, 3, D]
    ev, ec = float((v_emb.cpu() - ref_v).abs().max()), float((c_emb.cpu() - ref_c.reshape(18, -1)).abs().max())
    print(f"[parity] multi-caption eval {cls_name} ({branch}): video max err {ev:.3e}, caption max err {ec:.3e} (tol {TOL})")
    assert ev < TOL and ec < TOL
    assert list(df.index) == ["R@1", "R@5", "R@10", "MedR", "MeanR", "MRR"]
    _check_table(df, v_emb, c_emb, offsets)


def test_ragged_counts_offsets_and_caption_order():
    """Counts 1, 2 and 4: the offsets, and every row of caption_emb against a ONE-caption call of the same model on that caption (the
    towers and the CAM are per-item functions), in order; the video embeddings do not depend on the captions."""
    from vtc_amd.host import retrieval_evaluation as RE
    a = A.TINY
    m, sd = _build("clip_finaltf", "PretrainedCLIP_finaltf", a, 82, branch_to_adapt_val="text", n_heads=2)
    items = _items(a, [1, 2, 4], 800, True)
    df, v_emb, c_emb, offsets = RE.retrieval_evaluation(m, items, "full-test", "cuda", return_embeddings=True, multi_caption=True,
                                                        videos_per_batch=2)
    assert offsets.tolist() == [0, 1, 3, 7] and offsets.dtype == np.int64 and c_emb.shape[0] == 7
    _check_table(df, v_emb, c_emb, offsets)
    row = 0
    for it in items:
        for k in range(it[1].shape[0]):
            single = (it[0], it[1][k]) + tuple(it[2:])
            _, v1, c1 = RE.retrieval_evaluation(m, [single], "full-test", "cuda", return_embeddings=True)
            assert (c1[0] - c_emb[row]).abs().max() < TOL, (row, k)
            row += 1
    assert row == 7
    # the flat captions padded the reference's way give the same table
    padded = GR.pad_captions(c_emb.cpu().numpy(), offsets)
    assert_frame_equal(RE.compute_multi_caption_table(v_emb, torch.from_numpy(padded), "full-test", "videos"), df, check_exact=True)


def test_the_default_path_keeps_its_assertion():
    from vtc_amd.host import retrieval_evaluation as RE
    a = A.TINY
    m, _ = _build("timesformer", "PretrainedCLIP_TimeSformer", a, 83)
    items = _items(a, [2, 2], 900, False)
    with pytest.raises(AssertionError, match="one caption per video"):
        RE.retrieval_evaluation(m, items, "full-test", "cuda")
