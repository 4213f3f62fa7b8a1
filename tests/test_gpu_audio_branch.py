"""GPU: the audio branch of PretrainedCLIP_finaltf (init_audio_model=True) against the reference's own outputs
(tests/golden/audio_*.npz, tests/golden/make_audio_golden.py), the feature-MLP kernel and the CAM's aux tokens against fp64
restatements, and the audio config through the eval entry point."""
import json
import os
from dataclasses import asdict

import numpy as np
import pytest
import torch

import audio_case as AC
from conftest import golden_files, load_golden
from oracle import arch as A
from oracle import eval_ref as E
from oracle import model_ref as M
from test_gpu_towers import report, report_text, tol_for

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [f for f in golden_files("audio_") if "keys" not in f]


def _model(branch, dtype):
    from vtc_amd.host import model as HM
    from vtc_amd.host.clip_arch import ClipConfig
    m = HM.PretrainedCLIP_finaltf(model_type=ClipConfig(**asdict(AC.ARCH)), branch_to_adapt_val=branch, n_heads=AC.N_HEADS,
                                  init_audio_model=True)
    m.load_state_dict(AC.synth_state_dict(51), strict=True)
    m = m.eval().cuda()
    m.compute_dtype = dtype
    return m


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("fname", CASES)
def test_audio_wrapper_vs_reference(fname, dtype):
    case, g = load_golden(fname)
    m = _model(case["branch"], dtype)
    vis, title, comments, audio = (t.cuda() for t in AC.inputs(case))
    # text branch: overlap_towers (default) runs the CAM behind the text tower, multi-launch; off, B = 6 takes the one-launch CAM
    modes = (True, False) if case["branch"] == "text" and dtype == torch.float32 else (True,)
    for overlap in modes:
        m.overlap_towers = overlap
        fv, ft, sim = (o.cpu().numpy() for o in m(vis, title, [comments, audio]))
        tol = tol_for(dtype, 512)
        tag = f"{fname} {dtype} overlap={overlap}"
        report(f"{tag} feats_vis", np.abs(fv - g["feats_vis"]).max(), tol)
        if dtype == torch.float32:
            report(f"{tag} feats_text", np.abs(ft - g["feats_text"]).max(), tol)
        else:
            report_text(f"{tag} feats_text", ft, g["feats_text"], dtype, 512)
        scale = float(np.exp(np.log(1 / 0.07)))
        report(f"{tag} cos-sim", np.abs(sim - g["sim"]).max() / scale, tol)
    m.check_finite()


@pytest.mark.parametrize("n", [1, 5, 250, 1037, 5120])
def test_feature_mlp_vs_fp64(n):
    from vtc_amd import towers
    sd = AC.synth_audio_mlp(7)
    packed = towers.PackedAudioMlp({k: v.cuda() for k, v in sd.items()})
    x = torch.from_numpy(np.random.default_rng(n).normal(0, 1, (n, 512)).astype(np.float32))
    y = packed.forward(x.cuda()).cpu().double()
    ref = AC.mlp_fp64(sd, x)
    err = ((y - ref).abs().amax(dim=1) / ref.abs().amax(dim=1)).max().item()
    print(f"[parity] feature MLP n={n}: max row-relative error {err:.2e}")
    assert err <= 1e-5
    assert torch.equal(packed.forward(x.cuda()).cpu().double(), y)          # bitwise reproducible


def _cam(B, nc, na, seed=5):
    from vtc_amd import towers
    sd = A.synth_model(AC.ARCH, 51, "clip_finaltf")
    cam = towers.PackedCam({k: v.cuda() for k, v in sd.items()}, torch.float32, AC.N_HEADS, True, None)
    g = torch.Generator().manual_seed(seed)
    main = torch.randn(B, 512, generator=g)
    comm = torch.randn(B * nc, 512, generator=g)
    comments = A.synth_tokens(B * nc, AC.ARCH, seed, empty_frac=0.3).reshape(B, nc, -1)
    aux = torch.randn(B * na, 512, generator=g)
    return cam, sd, main, comm, comments, aux


@pytest.mark.parametrize("B", [4, 100])          # 4 x 6 tokens: the one-launch CAM (fused=None); 600 rows: above its limit
@pytest.mark.parametrize("fused", [None, False])
def test_cam_aux_with_no_tokens_is_bit_identical(B, fused):
    from vtc_amd import _lib as L
    cam, _, main, comm, comments, _ = _cam(B, 5, 0)
    main, comm, comments = main.cuda(), comm.cuda(), comments.cuda()
    want = cam.forward(main, comm, comments, fused=fused)
    got = cam.forward(main, comm, comments, fused=fused, aux=torch.empty(0, 512, device="cuda"))
    assert torch.equal(want, got)
    assert not (cam.w.flags & L.CAM_NO_FUSED)


@pytest.mark.parametrize("B,nc,na,fused", [(6, 5, 5, None), (6, 5, 5, False), (48, 5, 5, None), (3, 5, 74, None), (2, 1, 3, None)])
def test_cam_aux_tokens_vs_fp64(B, nc, na, fused):
    cam, sd, main, comm, comments, aux = _cam(B, nc, na)
    got = cam.forward(main.cuda(), comm.cuda(), comments.cuda(), fused=fused, aux=aux.cuda()).cpu().double()
    sd64 = A.with_dtype(sd, torch.float64)
    fc = comm.double().reshape(B, nc, -1).clone()
    fc[comments[..., 1] == 49407] = sd64["mask_embedding"]
    tokens = torch.cat([fc.permute(1, 0, 2), aux.double().reshape(B, na, -1).permute(1, 0, 2)], dim=0)
    want = M.adapt_feature(main.double(), tokens, sd64, n_heads=AC.N_HEADS)
    err = (got - want).abs().max().item()
    print(f"[parity] CAM aux B={B} nc={nc} na={na} fused={fused}: max abs error {err:.2e}")
    assert err <= 1e-5


def test_eval_cli_audio_config_matches_oracle_recall(tmp_path):
    from vtc_amd.host import eval as ev
    n = 64
    out_json = tmp_path / "res.json"
    torch.manual_seed(1023)
    out, fv, ft = ev.cli(["-c", os.path.join(ROOT, "configs", "pretrained_clip_comments_attention_audio.jsonc"), "--bs", "16",
                          "--n_pairs", str(n), "--out", str(out_json)])
    saved = json.load(open(out_json))
    assert set(saved) == {"R1_title_from_im", "R5_title_from_im", "R10_title_from_im",
                          "R1_im_from_title", "R5_im_from_title", "R10_im_from_title", "synthetic", "n_pairs"}
    assert saved["synthetic"] is True and saved["n_pairs"] == n
    fv, ft = fv.cpu().numpy(), ft.cpu().numpy()
    assert fv.shape == (n, 512) and np.allclose(np.linalg.norm(ft, axis=1), 1, atol=1e-5)
    assert {k: v for k, v in out.items() if k.startswith("R")} == E.eval_result_dict(fv, ft, np.float64)


def test_nan_in_audio_input_raises():
    case, _ = load_golden(CASES[0])
    assert case["branch"] == "text"
    m = _model("text", torch.float32)
    vis, title, comments, audio = (t.cuda() for t in AC.inputs(case))
    audio[1, 2, 3] = float("nan")
    fv, ft, _ = m(vis, title, [comments, audio])
    with pytest.raises(RuntimeError, match="non-finite"):
        m.check_finite()
    from vtc_amd.host import model as HM
    with pytest.raises(RuntimeError, match="non-finite"):
        HM.raise_if_nonfinite("eval", fv, ft)
