"""Generate tests/golden/audio_*.npz: the audio branch of PretrainedCLIP_finaltf (init_audio_model=True) by the REFERENCE's own
Python (unmodified), as make_golden.py does for the other wrappers.

Run in the build container only (needs the read-only reference checkout):

    python tests/golden/make_audio_golden.py [/root/reference]

The un-vendored ``clip`` package is replaced by tests/golden/clip_double.py at tests/audio_case.py's ARCH (oracle.arch.TINY with
512-d embeddings and a 512-wide text tower: the audio MLP is 512 x 512 and the wrapper's feature_dim is ln_final's width); the external GDT package by a sink module: its ``AudioBaseNetwork`` holds a few small parameters (so that
``audio_model.base.*`` keys exist, as in a real checkpoint) and is never called by the forward.  Weights and inputs are regenerated
from seeds by tests/audio_case.py, so each fixture stores the case description (as JSON) and the expected outputs.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import clip_double  # noqa: E402
import audio_case as AC  # noqa: E402

clip_double.install()
clip_double.ARCH = AC.ARCH


class _Base(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 4, 3, bias=False)
        self.fc = nn.Linear(4, 8)


class AudioBaseNetwork(nn.Module):
    """Sink for GDT.model.AudioBaseNetwork("resnet9", pretrained=True, duration=1) (model/model.py:419)."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        self.base = _Base()


gdt = types.ModuleType("GDT")
gdt_model = types.ModuleType("GDT.model")
gdt_model.AudioBaseNetwork, gdt_model.Identity = AudioBaseNetwork, nn.Identity
gdt.model = gdt_model
sys.modules["GDT"], sys.modules["GDT.model"] = gdt, gdt_model
sys.path.insert(0, REF)

import model.model as ref_model  # noqa: E402  (reference)

assert ref_model.__file__.startswith(REF), ref_model.__file__
torch.manual_seed(0)
torch.set_grad_enabled(False)
WSEED = 51


def save(name, case, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, case=np.array(json.dumps(case)), **{k: np.asarray(v) for k, v in arrays.items()})
    print("wrote", os.path.relpath(path, ROOT), {k: tuple(np.asarray(v).shape) for k, v in arrays.items()})


def build(branch):
    m = ref_model.PretrainedCLIP_finaltf(branch_to_adapt_val=branch, init_audio_model=True, n_heads=AC.N_HEADS).eval()
    sd = m.state_dict()
    mine = AC.synth_state_dict(WSEED)
    assert set(mine) == set(sd), (sorted(set(sd) ^ set(mine)))[:10]
    m.load_state_dict(mine, strict=True)
    return m


def gen_cases():
    for i, (branch, B) in enumerate((("text", 6), ("image", 6), ("skip", 6), ("text", 48))):
        m = build(branch)
        case = dict(kind="audio_wrapper", branch=branch, B=B, nc=AC.N_COMMS, na=AC.N_CLIPS, empty_frac=AC.EMPTY_FRAC, wseed=WSEED,
                    xseed=52 + i, tseed=62 + i, cseed=72 + i, aseed=82 + i, n_heads=AC.N_HEADS)
        vis, title, comments, audio = AC.inputs(case)
        # the list form default_collate makes of an item's (comments_tok, audio_clips) tuple (model/model.py:220-224)
        out = m(vis, title, [comments, audio])
        save(f"audio_{i:02d}_branch-{branch}_b{B}", case, feats_vis=out[0].numpy(), feats_text=out[1].numpy(), sim=out[2].numpy())


def gen_keys():
    m = ref_model.PretrainedCLIP_finaltf(init_audio_model=True, n_heads=AC.N_HEADS)
    sd = m.state_dict()
    save("audio_state_dict_keys", dict(kind="audio_state_dict_keys", n_heads=AC.N_HEADS),
         keys=np.array(list(sd)), shapes=np.array([json.dumps(list(v.shape)) for v in sd.values()]))


if __name__ == "__main__":
    gen_cases()
    gen_keys()
