"""How a stored evaluation case (the JSON of tests/golden/eval_*.npz) turns back into its inputs.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Shared by tests/golden/make_eval_golden.py, which feeds the reference's own
``retrieval_evaluation``, and by the tests that hold the oracle and the HIP path to what it returned: the items are regenerated from
seeds on every side, so a fixture stores no pixels and no weights.
"""
from __future__ import annotations

import warnings
from typing import Dict

import torch

from . import arch as A
from . import model_ref as M

ARCH = {"TINY": A.TINY, "VIT_B32": A.VIT_B32}
DATASETS = {"MSRVTT_videos": "VideoDatasetMSRVTT", "MSVD_videos": "VideoDatasetMSVD", "K700_videos": "VideoDatasetK700Comments",
            "Reddit_videos": "VideoDatasetReddit", "livebot": "VideoDatasetLivebot"}
#: the per-element agreement the GPU tests assert on fp32 embeddings; the fixtures' boundary gap is held to rank_safety_bound(EPS, D)
EPS = 1e-5


def state_dict(case) -> Dict[str, torch.Tensor]:
    """The seeded state dict of the case's wrapper.  ``nonzero_seed``: the projections the synthetic CAM / time branch would leave
    small or zero (``temporal_fc``, the CAM's ``out_proj`` / ``c_proj``) get N(0, 0.02) weights, as a trained checkpoint has."""
    sd = A.synth_model(ARCH[case["arch"]], case["wseed"], case["model"], nframes=8)
    if case.get("nonzero_seed") is not None:
        g = torch.Generator().manual_seed(case["nonzero_seed"])
        for k in list(sd):
            if k.endswith("temporal_fc.weight") or (k.startswith("final_transformer.") and
                                                    (k.endswith("out_proj.weight") or k.endswith("c_proj.weight"))):
                sd[k] = torch.randn(sd[k].shape, generator=g) * 0.02
    return sd


def standin(case, defaults) -> dict:
    """The value of ``vtc_amd.host.datasets.VIDEO_STANDIN`` for the case (``defaults``: the module's own value)."""
    return dict(defaults, **case["standin"])


def dataset_class(case, module_data):
    """The stand-in class behind the case's dataset name.  ``lengths``: a subclass with these frame counts instead of drawn ones
    and, with ``bf16_pixels``, pixels rounded to bf16-representable values (so that a bf16 path and an fp32 one see the same input)."""
    base = getattr(module_data, DATASETS[case["dataset"]])
    if case.get("lengths") is None:
        return base
    lengths, bf16 = list(case["lengths"]), bool(case.get("bf16_pixels"))

    class FixedVideos(base):
        def __init__(self, train=False, split="full-test", **kw):
            super().__init__(train=train, split=split, **kw)
            assert self.n == len(lengths)
            self.lengths = torch.tensor(lengths)

        def __getitem__(self, i):
            item = super().__getitem__(i)
            return ((item[0].bfloat16().float(),) + tuple(item[1:])) if bf16 else item

    return FixedVideos


def items(case, module_data):
    """The dataset's items, as the loop sees them.  ``module_data.VIDEO_STANDIN`` must hold ``standin(case, ...)``."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ds = dataset_class(case, module_data)(train=False, split=case["split"])
    return [ds[i] for i in range(len(ds))]


def oracle_forward(case, sd):
    """``forward(frames, captions, comments | None) -> (feats_a, feats_b)`` of the case's wrapper, from oracle/model_ref.py."""
    a, kind, kw = ARCH[case["arch"]], case["model"], dict(case["ctor"])
    branch = kw.pop("branch_to_adapt_val", "text")
    if kind == "clip":
        return lambda fr, cap, com: M.pretrained_clip(fr, cap, sd, a)[:2]
    if kind == "clip_finaltf":
        return lambda fr, cap, com: M.pretrained_clip_finaltf(fr, cap, com, sd, a, branch, **kw)[:2]
    if kind == "timesformer":
        return lambda fr, cap, com: M.pretrained_clip_timesformer(fr, cap, sd, a)[:2]
    return lambda fr, cap, com: M.pretrained_clip_timesformer_finaltf(fr, cap, com, sd, a, branch, **kw)[:2]
