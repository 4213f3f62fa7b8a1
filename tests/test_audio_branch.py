"""CPU: the audio-with-comments config (configs/pretrained_clip_comments_attention_audio.jsonc) resolves and builds, the audio
branch's state-dict contract matches the reference's (tests/golden/audio_state_dict_keys.npz), cached clip features are looked up
by id, the out-of-scope audio variants refuse with a reason, and the new kernels compile without spills."""
import inspect
import json
import os
from dataclasses import asdict

import numpy as np
import pytest
import torch

import audio_case as AC
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "pretrained_clip_comments_attention_audio.jsonc")


def _config(mods=None):
    from vtc_amd.host.parse_config import ConfigParser
    return ConfigParser.from_file(CFG, modification=dict({"dataset;args;n_pairs": 5}, **(mods or {})))


def _model(**kw):
    from vtc_amd.host import model as HM
    from vtc_amd.host.clip_arch import ClipConfig
    return HM.PretrainedCLIP_finaltf(model_type=ClipConfig(**asdict(AC.ARCH)), n_heads=AC.N_HEADS, init_audio_model=True, **kw)


@pytest.mark.filterwarnings("ignore::UserWarning")
def test_unmodified_audio_config_builds_dataset_and_arch():
    from torch.utils.data import DataLoader
    from vtc_amd.host import datasets as module_data
    from vtc_amd.host import model as module_arch
    config = _config()
    for train, test in ((True, False), (False, False), (False, True)):          # train.py:45-64 / eval.py:58
        ds = config.init_obj("dataset", module_data, train=train, test=test)
        assert len(ds) == 5
        vis, title, inner, meta = ds[0]
        assert isinstance(inner, tuple) and len(inner) == 2
        comments, audio = inner
        assert vis.shape == (3, 224, 224) and title.shape == (77,) and title.dtype == torch.int64
        assert comments.shape == (5, 77) and comments.dtype == torch.int64
        assert audio.shape == (5, 512) and audio.dtype == torch.float32
        assert meta == {"id": 0}
        vb, tb, cb, mb = next(iter(DataLoader(ds, batch_size=4)))
        assert isinstance(cb, list) and cb[0].shape == (4, 5, 77) and cb[1].shape == (4, 5, 512)
    # the splits are disjoint synthetic sets, the clips seeded
    a = config.init_obj("dataset", module_data, train=False, test=True)[1][2][1]
    b = config.init_obj("dataset", module_data, train=False, test=True)[1][2][1]
    assert torch.equal(a, b)
    cls = getattr(module_arch, config["arch"]["type"])
    args = dict(config["arch"]["args"])
    inspect.signature(cls).bind(**args)
    # the config's own arguments (empty checkpoint paths included) build the model; the tiny 512-wide architecture stands in for ViT-B/32
    from vtc_amd.host.clip_arch import ClipConfig
    args.update(model_type=ClipConfig(**asdict(AC.ARCH)))
    m = cls(**args)
    assert m.init_audio_model and any(k.startswith("audio_model.mlp.") for k in m.state_dict())


def test_state_dict_contract_matches_reference():
    case, g = load_golden("audio_state_dict_keys.npz")
    keys = [str(k) for k in g["keys"]]
    shapes = {k: tuple(json.loads(str(s))) for k, s in zip(keys, g["shapes"])}
    assert any(k.startswith("audio_model.base.") for k in keys)
    assert {k for k in keys if k.startswith("audio_model.mlp.")} == {
        f"audio_model.mlp.layers.{i}.{p}" for i in (1, 4) for p in ("weight", "bias")} | {
        f"audio_model.mlp.layers.2.{p}" for p in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    sd = AC.synth_state_dict(AC_SEED)
    assert set(sd) == set(keys) and all(tuple(sd[k].shape) == shapes[k] for k in keys)
    m = _model()
    m.load_state_dict(sd, strict=True)                                       # eval.py:90-91
    out = m.state_dict()
    assert set(out) == set(keys)
    for k in keys:
        assert torch.equal(out[k], sd[k]), k
    # round trip into a fresh model
    m2 = _model()
    m2.load_state_dict(out, strict=True)
    assert torch.equal(m2.state_dict()["audio_model.base.conv1.weight"], sd["audio_model.base.conv1.weight"])
    # strict still refuses keys that belong nowhere
    with pytest.raises(RuntimeError):
        m2.load_state_dict(dict(out, **{"audio_model.bogus": torch.zeros(1)}), strict=True)


AC_SEED = 51


def test_audio_branch_needs_512_wide_features():
    from vtc_amd.host import model as HM
    from oracle import arch as A
    from vtc_amd.host.clip_arch import ClipConfig
    with pytest.raises(ValueError, match="512"):
        HM.PretrainedCLIP_finaltf(model_type=ClipConfig(**asdict(A.TINY)), n_heads=2, init_audio_model=True)
    HM.PretrainedCLIP_finaltf(model_type=ClipConfig(**asdict(A.TINY)), n_heads=2, init_audio_model=False)


def test_checkpoint_paths(tmp_path):
    """audio_model_ckpt: GDT's audio tensors go to the base sink; clip_audio_ckpt: model/model.py:428-435 (strict into the CLIP)."""
    base = AC.synth_audio_base(3, prefix="")
    gdt = {"model": {"module.audio_network.base." + k: v for k, v in base.items()}}
    gdt["model"]["module.video_network.conv.weight"] = torch.zeros(2)
    torch.save(gdt, tmp_path / "gdt.pth")
    src = _model()
    clip_sd = {"model." + k: v for k, v in src.model.state_dict().items()}
    torch.save({"state_dict": clip_sd}, tmp_path / "clip.pth")
    m = _model(audio_model_ckpt=str(tmp_path / "gdt.pth"), clip_audio_ckpt=str(tmp_path / "clip.pth"))
    sd = m.state_dict()
    for k, v in base.items():
        assert torch.equal(sd["audio_model.base." + k], v)
    for k, v in src.model.state_dict().items():
        assert torch.equal(sd["model." + k], v)


def test_cached_audio_features_are_looked_up_by_id(tmp_path):
    from vtc_amd.host.datasets import ImTextDataset
    n = 7
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(0))
    emb = torch.randn(n, 3, 512)
    path = tmp_path / "audio.pth"
    torch.save({"reddit_ids": perm.to(torch.int64), "embeddings": emb}, path)   # dataset_loaders.py:162-184 (array form)
    with pytest.warns(UserWarning):
        ds = ImTextDataset("", train=False, test=True, add_comments="always", num_comms=2, cached_audio_features=str(path),
                           audio_with_comms=True, n_pairs=n)
    for i in range(n):
        _, _, (comments, audio), meta = ds[i]
        row = int((perm == meta["id"]).nonzero())
        assert torch.equal(audio, emb[row]) and comments.shape == (2, 77)


def test_audio_variants_without_a_model_refuse():
    from vtc_amd.host.datasets import ImTextDataset
    with pytest.raises(NotImplementedError, match="audio_instead_of_title"):
        ImTextDataset("", train=False, test=True, audio_instead_of_title=True, n_pairs=2)
    with pytest.raises(NotImplementedError, match="audio_with_comms"):
        ImTextDataset("", train=False, test=True, cached_audio_features="features.pth", n_pairs=2)


def test_train_refuses_the_audio_config():
    from vtc_amd.host import train
    with pytest.raises(NotImplementedError, match="audio MLP's backward.*Dropout and BatchNorm"):
        train.main(_config(), device="cpu")


def test_feature_mlp_and_cam_compile_without_spills(tmp_path):
    import shutil
    if not os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    from test_build_no_spills import _metadata
    meta = _metadata(os.path.join(ROOT, "vtc_amd", "csrc", "audio.hip"), tmp_path)
    for hc in (512, 256, 128, 64):
        hits = [k for k in meta if f"feature_mlp_kernelILi{hc}EE" in k]
        assert len(hits) == 1, (hc, hits)
        assert meta[hits[0]]["spill"] == 0 and meta[hits[0]]["scratch"] == 0, (hits[0], meta[hits[0]])
    meta = _metadata(os.path.join(ROOT, "vtc_amd", "csrc", "cam.hip"), tmp_path)
    hits = [k for k in meta if "cam_fused_kernelILi512EE" in k]
    assert len(hits) == 1 and meta[hits[0]]["spill"] == 0 and meta[hits[0]]["scratch"] == 0, (hits, meta)
