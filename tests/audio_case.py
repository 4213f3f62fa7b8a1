"""Seeded weights and inputs of the audio-branch cases (PretrainedCLIP_finaltf(init_audio_model=True), model/model.py:409-438 +
:220-230), shared by tests/golden/make_audio_golden.py and the tests that read its fixtures (tests/golden/audio_*.npz).

The architecture is oracle.arch.TINY with 512-d embeddings: the audio MLP is 512 x 512 (model/model.py:80-94), so the CAM and the
embeddings must be 512 wide.  The wrapper's feature_dim is ln_final's width (model/model.py:393), i.e. the TEXT tower's width, so
that is 512 too (8 heads of 64), not only embed_dim.  The MLP's weights and BatchNorm running statistics are NOT the init: a fold of the statistics that
were never exercised (mean 0, var 1, gamma 1, beta 0) would pass unnoticed."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from oracle import arch as A

ARCH = dataclasses.replace(A.TINY, embed_dim=512, transformer_width=512, transformer_heads=8)
N_HEADS = 8
N_COMMS, N_CLIPS, EMPTY_FRAC = 5, 5, 0.3
#: audio_model.base.* of the reference's state dict in the fixtures: a stand-in for GDT's resnet9 (never read by the forward)
BASE_SHAPES = {"conv1.weight": (4, 1, 3, 3), "fc.weight": (8, 4), "fc.bias": (8,)}


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def synth_audio_mlp(seed: int, width: int = 512, prefix: str = "audio_model.mlp.layers.") -> dict:
    """Linear(512, 512) -> BatchNorm1d(512) (eval: running statistics) -> ReLU -> Linear(512, 512), all non-trivial."""
    r = _rng(seed)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))     # noqa: E731
    s = width ** -0.5
    return {
        prefix + "1.weight": t(r.normal(0, s, (width, width))), prefix + "1.bias": t(r.normal(0, 0.1, width)),
        prefix + "2.weight": t(r.uniform(0.5, 1.5, width)), prefix + "2.bias": t(r.normal(0, 0.2, width)),
        prefix + "2.running_mean": t(r.normal(0, 0.3, width)), prefix + "2.running_var": t(r.uniform(0.3, 2.5, width)),
        prefix + "2.num_batches_tracked": torch.tensor(1000, dtype=torch.int64),
        prefix + "4.weight": t(r.normal(0, s, (width, width))), prefix + "4.bias": t(r.normal(0, 0.1, width)),
    }


def synth_audio_base(seed: int, prefix: str = "audio_model.base.") -> dict:
    r = _rng(seed)
    return {prefix + k: torch.from_numpy(r.normal(0, 1, shp).astype(np.float32)) for k, shp in BASE_SHAPES.items()}


def synth_state_dict(seed: int) -> dict:
    """The whole audio-config state dict: towers + CAM (oracle.arch.synth_model) + audio_model.{mlp, base}."""
    sd = A.synth_model(ARCH, seed, "clip_finaltf")
    sd.update(synth_audio_mlp(seed + 1))
    sd.update(synth_audio_base(seed + 2))
    return sd


def synth_audio(B: int, n_clips: int, seed: int) -> torch.Tensor:
    """[B, n_clips, 512] fp32 pre-extracted clip features (dataset_loaders.py:162-184 format of one item: [n_clips, 512])."""
    return torch.from_numpy(_rng(seed).normal(0, 1, (B, n_clips, 512)).astype(np.float32))


def inputs(case: dict):
    """(vis, title, comments, audio) of a fixture case, on the CPU."""
    B = case["B"]
    vis = A.synth_pixels((B, 3, ARCH.image_resolution, ARCH.image_resolution), case["xseed"])
    title = A.synth_tokens(B, ARCH, case["tseed"])
    comments = A.synth_tokens(B * case["nc"], ARCH, case["cseed"], empty_frac=case["empty_frac"]).reshape(B, case["nc"], -1)
    return vis, title, comments, synth_audio(B, case["na"], case["aseed"])


def mlp_fp64(sd: dict, x: torch.Tensor, prefix: str = "audio_model.mlp.layers.") -> torch.Tensor:
    """The eval-mode MLP restated in fp64: Linear, BatchNorm1d(running statistics, eps 1e-5), ReLU, Linear."""
    g = lambda k: sd[prefix + k].double().cpu()      # noqa: E731
    h = x.double().cpu() @ g("1.weight").T + g("1.bias")
    h = (h - g("2.running_mean")) / torch.sqrt(g("2.running_var") + 1e-5) * g("2.weight") + g("2.bias")
    return torch.relu(h) @ g("4.weight").T + g("4.bias")
