"""CPU: the oracle's evaluation loop (oracle/eval_ref.py: retrieval_evaluation_loop + compute_recall_frame) vs fixtures produced by
the reference's own ``retrieval_evaluation`` / ``compute_recall`` (tests/golden/make_eval_golden.py).  This is what pins the loop's
restatement: the ``::frame_stride`` slice, the floor(linspace) tail, ``comments[0, :5]``, one comment set per chunk (image branch) or
per caption (text branch), the un-normalised mean over chunks, and which DataFrame column is which direction."""
import json

import numpy as np
import pytest
import torch

from conftest import golden_files, load_golden
from oracle import eval_cases as C
from oracle import eval_ref as E

torch.set_grad_enabled(False)
TOL = dict(rtol=0, atol=2e-5)          # tests/test_oracle_golden.py's: fp32 CPU, different op order
FIXTURES = golden_files("eval_")


def test_every_case_of_the_generator_has_its_fixture():
    names = [f[len("eval_00_"):-len(".npz")] for f in FIXTURES]
    assert names == ["clip_msrvtt", "finaltf_text_msrvtt_dummy_comments", "finaltf_image_k700", "finaltf_skip_k700",
                     "finaltf_text_msvd_first_frame", "finaltf_image_k700_first_chunk", "finaltf_image_k700_stride4",
                     "finaltf_text_reddit_one_frame", "timesformer_finaltf_text_vit_b32"]


@pytest.mark.parametrize("fname", FIXTURES)
def test_oracle_loop_vs_reference_loop(fname, monkeypatch):
    from vtc_amd.host import datasets as D
    case, g = load_golden(fname)
    monkeypatch.delenv("VTC_SYNTHETIC_VIDEOS", raising=False)
    monkeypatch.setattr(D, "VIDEO_STANDIN", C.standin(case, D.VIDEO_STANDIN))
    sd = C.state_dict(case)
    items = C.items(case, D)
    needs_comments = case["model"].endswith("finaltf")
    branch = case["ctor"].get("branch_to_adapt_val", "text")
    v, t = E.retrieval_evaluation_loop(C.oracle_forward(case, sd), items, needs_comments, branch, **case["loop"])
    ev, et = np.abs(v.numpy() - g["tensor_v"]).max(), np.abs(t.numpy() - g["tensor_t"]).max()
    print(f"[parity] oracle loop vs reference loop, {fname}: video {ev:.3e}, caption {et:.3e} (tol 2e-5)")
    assert t.shape == g["tensor_t"].shape
    np.testing.assert_allclose(v.numpy(), g["tensor_v"], **TOL)
    np.testing.assert_allclose(t.numpy(), g["tensor_t"], **TOL)
    # the stored gap is the fixture's own tensors', and (TINY) what lets embeddings within eps decide the same table
    gap = E.table_gap(g["tensor_v"], g["tensor_t"])
    assert gap == float(g["gap"]) == case["gap"]
    if case["arch"] != "TINY":
        return                                               # three videos: embeddings only
    assert case["two_delta"] == E.rank_safety_bound(case["eps"], v.shape[1]) and case["eps"] == 1e-5
    assert gap >= case["two_delta"] and len(items) >= 12
    for dtype in (np.float32, np.float64):
        df = E.compute_recall_frame(v, t, case["split"], case["dataset"], dtype)
        assert list(df.columns) == g["columns"].tolist() and list(df.index) == g["index"].tolist()
        np.testing.assert_array_equal(df.to_numpy(), g["table"])
    assert not np.array_equal(g["table"][:, 0], g["table"][:, 1])       # the two directions differ: a swapped column shows


def test_boundary_gap_is_what_near_ties_thresholds():
    """A planted case: the target of query 0 at rank 1 (0-based) with a known gap to rank 0, everything else far away."""
    a = np.eye(4)
    b = a.copy()
    b[0] = [0.6, 0.61, 0.0, 0.0]                             # closer to row 1 than to its own row 0, by 2 * 0.01
    gap = E.boundary_gap(a, b, [1])
    assert abs(gap - 0.02) < 1e-12
    assert E.near_ties(a, b, [1], tol=0.021) == 1 and E.near_ties(a, b, [1], tol=0.019) == 0
    assert E.boundary_gap(a, a, [1]) == 2.0 and E.boundary_gap(a, a, [5]) == np.inf
    # s = 2 eps sqrt(D), delta = 4 s + s^2
    s = 2 * 1e-5 * np.sqrt(128.0)
    assert abs(E.rank_safety_bound(1e-5, 128) - 2 * (4 * s + s * s)) < 1e-15 and 1.8e-3 < E.rank_safety_bound(1e-5, 128) < 1.82e-3


def test_case_json_is_complete():
    for fname in FIXTURES:
        case, g = load_golden(fname)
        assert {"model", "arch", "ctor", "wseed", "standin", "dataset", "split", "loop", "gap"} <= set(case), fname
        assert {"n_videos", "min_frames", "max_frames", "resolution", "context", "seed"} <= set(case["standin"]), fname
        json.dumps(case)


def test_oracle_eval_result_dict_vs_reference_eval_main(monkeypatch):
    """evaluation/eval.py::main of the reference (its own file, driven by a duck-typed config) wrote the six JSON values and handed
    res_vis / res_text to RecallAtK: the oracle's forward over the regenerated ImTextDataset items, in the loop's batches, and
    eval_result_dict on it."""
    import warnings

    from oracle import model_ref as M
    from vtc_amd.host import datasets as D
    case, g = load_golden("evalmain_00_finaltf_text.npz")
    monkeypatch.delenv("VTC_SYNTHETIC_PAIRS", raising=False)
    a, sd = C.ARCH[case["arch"]], C.state_dict(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ds = getattr(D, case["dataset_type"])(**case["dataset_args"], train=False, test=True)
    assert len(ds) == case["dataset_args"]["n_pairs"] >= 12 and len(ds) % case["batch_size"] > 1
    kw = dict(case["ctor"])
    branch = kw.pop("branch_to_adapt_val")
    res_vis, res_text = [], []
    for lo in range(0, len(ds), case["batch_size"]):
        batch = [ds[i] for i in range(lo, min(lo + case["batch_size"], len(ds)))]
        vis, title, comments = (torch.stack([it[j] for it in batch]) for j in range(3))
        fv, ft, _ = M.pretrained_clip_finaltf(vis, title, comments, sd, a, branch, **kw)
        res_vis.append(fv)
        res_text.append(ft)
    res_vis, res_text = torch.cat(res_vis).numpy(), torch.cat(res_text).numpy()
    print(f"[parity] oracle vs reference eval.py::main: vis {np.abs(res_vis - g['res_vis']).max():.3e}, "
          f"text {np.abs(res_text - g['res_text']).max():.3e} (tol 2e-5)")
    np.testing.assert_allclose(res_vis, g["res_vis"], **TOL)
    np.testing.assert_allclose(res_text, g["res_text"], **TOL)
    gap = E.table_gap(g["res_vis"], g["res_text"])
    assert gap == float(g["gap"]) == case["gap"] and gap >= case["two_delta"] == E.rank_safety_bound(case["eps"], a.embed_dim)
    for dtype in (np.float32, np.float64):
        out = E.eval_result_dict(res_vis, res_text, dtype)
        assert list(out) == g["keys"].tolist()
        np.testing.assert_array_equal(np.array(list(out.values()), dtype=np.float64), g["values"])
    assert not np.array_equal(g["values"][:3], g["values"][3:])         # the two directions differ: swapped keys show
