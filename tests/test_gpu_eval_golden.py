"""GPU: the drop-in evaluation loop (evaluation/retrieval_evaluation.py -> vtc_amd/host/retrieval_evaluation.py: ragged chunk batches,
vtc_segment_mean, the rank sweep) vs fixtures produced by the reference's own ``retrieval_evaluation`` / ``compute_recall``
(tests/golden/make_eval_golden.py).  Embeddings within 1e-5, then the DataFrame identical -- unconditionally: every TINY fixture's
boundary gap was held to rank_safety_bound(1e-5, D) when it was made (tests/test_oracle_eval_golden.py re-checks the stored figures)."""
from dataclasses import asdict

import numpy as np
import pytest
import torch

from conftest import golden_files, load_golden
from oracle import eval_cases as C

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
CLASSES = {"clip": "PretrainedCLIP", "clip_finaltf": "PretrainedCLIP_finaltf", "timesformer": "PretrainedCLIP_TimeSformer",
           "timesformer_finaltf": "PretrainedCLIP_TimeSformer_finaltf"}
TINY_FIXTURES = [f for f in golden_files("eval_") if "vit_b32" not in f]
B32_FIXTURE = "eval_08_timesformer_finaltf_text_vit_b32.npz"


def _model(case, dtype):
    from vtc_amd.host import model as HM
    from vtc_amd.host.clip_arch import ClipConfig
    model_type = "ViT-B/32" if case["arch"] == "VIT_B32" else ClipConfig(**asdict(C.ARCH[case["arch"]]))
    m = getattr(HM, CLASSES[case["model"]])(model_type=model_type, **case["ctor"])
    m.load_state_dict(C.state_dict(case), strict=True)
    m = m.eval().cuda()
    m.compute_dtype = dtype
    return m


def _standin(case, monkeypatch):
    from vtc_amd.host import datasets as D
    monkeypatch.delenv("VTC_SYNTHETIC_VIDEOS", raising=False)
    monkeypatch.setattr(D, "VIDEO_STANDIN", C.standin(case, D.VIDEO_STANDIN))
    return D


def test_the_fixture_lists_are_what_the_generator_writes():
    assert len(TINY_FIXTURES) == 8 and B32_FIXTURE in golden_files("eval_")


@pytest.mark.parametrize("fname", TINY_FIXTURES)
def test_drop_in_loop_vs_reference_loop(fname, monkeypatch):
    from evaluation.retrieval_evaluation import retrieval_evaluation
    case, g = load_golden(fname)
    assert case["arch"] == "TINY" and case["gap"] >= case["two_delta"] > 1.8e-3 and case["eps"] == 1e-5
    _standin(case, monkeypatch)
    m = _model(case, torch.float32)
    df, v, t = retrieval_evaluation(m, case["dataset"], case["split"], "cuda", **case["loop"], return_embeddings=True)
    ev = float(np.abs(v.cpu().numpy() - g["tensor_v"]).max())
    et = float(np.abs(t.cpu().numpy() - g["tensor_t"][:, 0]).max())
    print(f"[parity] drop-in loop vs reference loop, {fname}: video {ev:.3e}, caption {et:.3e} (tol 1e-5)\n{df}")
    assert v.shape == g["tensor_v"].shape and ev < 1e-5 and et < 1e-5
    assert list(df.columns) == g["columns"].tolist() and list(df.index) == g["index"].tolist()
    np.testing.assert_array_equal(df.to_numpy(), g["table"])


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 1e-3)], ids=["fp32", "bf16"])
def test_drop_in_loop_vit_b32_timesformer_vs_reference_loop(dtype, tol, monkeypatch):
    """The TimeSformer wrapper at the only size the reference has it: one full chunk, two chunks with a resampled tail, one 8-frame
    item (a single frame after the stride); bf16-representable pixels, so both precisions read the reference's input.  Embeddings only
    (three videos); bf16 at the tolerance of test_ragged_chunked_eval_vit_b32_bf16_vs_per_video_oracle_loop."""
    from evaluation.retrieval_evaluation import retrieval_evaluation
    case, g = load_golden(B32_FIXTURE)
    D = _standin(case, monkeypatch)
    m = _model(case, dtype)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ds = C.dataset_class(case, D)(train=False, split=case["split"])
    assert ds.lengths.tolist() == case["lengths"]
    df, v, t = retrieval_evaluation(m, ds, case["split"], "cuda", **case["loop"], return_embeddings=True)
    ev = float(np.abs(v.cpu().numpy() - g["tensor_v"]).max())
    et = float(np.abs(t.cpu().numpy() - g["tensor_t"][:, 0]).max())
    print(f"[parity] drop-in loop ViT-B/32 {dtype} vs reference loop: video {ev:.3e}, caption {et:.3e} (tol {tol:g})")
    assert v.shape == g["tensor_v"].shape and ev < tol and et < tol
    assert list(df.index) == g["index"].tolist()


def test_drop_in_eval_main_vs_reference_eval_main(monkeypatch, tmp_path):
    """evaluation/eval.py::main (vtc_amd/host/eval.py) with a duck-typed config -- all main reads of it -- against what the reference's
    own main wrote and handed to RecallAtK: embeddings within 1e-5, then the six JSON values identical (the fixture's boundary gap was
    held to 2 delta), in the returned dict and in the file."""
    import argparse
    import json
    import logging

    from evaluation.eval import main
    from vtc_amd.host.clip_arch import ClipConfig
    case, g = load_golden("evalmain_00_finaltf_text.npz")
    assert case["gap"] >= case["two_delta"] > 1.8e-3 and case["eps"] == 1e-5
    monkeypatch.delenv("VTC_SYNTHETIC_PAIRS", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)

    class Config(dict):
        def get_logger(self, name):
            return logging.getLogger(name)

        def init_obj(self, name, module, *args, **kwargs):
            return getattr(module, self[name]["type"])(*args, **dict(self[name]["args"], **kwargs))

    config = Config(arch=dict(type=case["arch_type"], args=dict(case["ctor"], model_type=ClipConfig(**asdict(C.ARCH[case["arch"]])))),
                    dataset=dict(type=case["dataset_type"], args=dict(case["dataset_args"])), batch_size=case["batch_size"])
    ckpt = tmp_path / "checkpoint.pth"
    torch.save({"state_dict": C.state_dict(case)}, ckpt)
    args = argparse.Namespace(num_irrelevant_comments=case["num_irrelevant_comments"], dtype="f32")
    out, res_vis, res_text = main(config, args, ckpt, device="cuda")
    ev = float(np.abs(res_vis.cpu().numpy() - g["res_vis"]).max())
    et = float(np.abs(res_text.cpu().numpy() - g["res_text"]).max())
    print(f"[parity] drop-in eval main vs reference eval main: vis {ev:.3e}, text {et:.3e} (tol 1e-5); {out}")
    assert res_vis.shape == g["res_vis"].shape and ev < 1e-5 and et < 1e-5
    keys = g["keys"].tolist()
    assert list(out)[:6] == keys
    np.testing.assert_array_equal(np.array([out[k] for k in keys], dtype=np.float64), g["values"])
    written = json.load(open(tmp_path / "checkpoint_res_adapted_text_5_comms.json"))
    np.testing.assert_array_equal(np.array([written[k] for k in keys], dtype=np.float64), g["values"])
