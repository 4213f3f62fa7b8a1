"""Generate tests/golden/eval_*.npz by running the REFERENCE's own evaluation loop (evaluation/retrieval_evaluation.py:
``retrieval_evaluation`` + ``compute_recall``, unmodified) over the stand-in datasets.

Run in the build container only (needs the read-only reference checkout), on the CPU:

    python tests/golden/make_eval_golden.py [/root/reference]            # writes every fixture, asserting the gap condition
    EVAL_GOLDEN_SEARCH=1 python tests/golden/make_eval_golden.py         # prints, per TINY case, the first stand-in seed that meets it

The reference's file is imported by path with its own ``model.model`` and ``model.metric`` behind it.  What it cannot import or run
here is replaced on the harness side only, none of it by editing or copying reference text:
  * ``clip``: tests/golden/clip_double.py, plus a ``clip.tokenize`` that takes empty strings only and returns ``[SOT, EOT, 0...]`` rows
    of the architecture's context length (what :214 asks for; the real tokeniser is un-vendored);
  * ``faiss`` and ``collections.Iterable``: tests/golden/faiss_double.py (shared with make_recall_golden.py);
  * ``dataset_loaders.dataset_loaders``: a module whose five class names are the stand-in classes of vtc_amd/host/datasets.py, configured
    through ``VIDEO_STANDIN`` in-process -- the tests regenerate the same items from the same seeds;
  * ``torch.nn.module = torch.nn.Module``: the annotation at :110 is evaluated at import;
  * ``DataLoader`` in the imported module's namespace: a wrapper that forces ``num_workers=0``;
  * ``compute_recall`` in that namespace: a spy that records ``tensor_v`` / ``tensor_t`` and calls the original (the reference
    returns only the DataFrame).
``evaluation/eval.py::main`` (the image-text evaluation) is run the same way: see the section above ``gen_eval_main``.  Its two
``logging.info("...: ", list)`` calls (:128-129) make the logging module print a formatting traceback to stderr; that is the
reference's own and harmless.
Each ``eval_*`` fixture stores the case (JSON: wrapper, constructor keywords, seeds, ``VIDEO_STANDIN`` values, dataset, split, loop flags), the two
captured tensors, the DataFrame (values, columns, index) and the boundary gap of the captured tensors with the bound it was held to.

The gap condition (oracle/eval_ref.py: ``table_gap`` >= ``rank_safety_bound(1e-5, D)``) is a condition on the DATA: it is what lets a
test compare embeddings within 1e-5 and then demand an identical table.  The stand-in seed of every TINY case is chosen for it.
"""
from __future__ import annotations

import json
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import faiss_double  # noqa: E402

faiss_double.install()                     # before model.metric is imported: clip_double leaves an installed ``faiss`` alone
import make_golden as G  # noqa: E402  (clip_double.install(), the reference's ``model`` package, build_wrapper)
import clip_double  # noqa: E402

from oracle import arch as A  # noqa: E402
from oracle import eval_cases as C  # noqa: E402
from oracle import eval_ref as E  # noqa: E402
from vtc_amd.host import datasets as D  # noqa: E402


def tokenize(texts, context_length=None, truncate=False):
    assert all(t == "" for t in texts), "the evaluation loop tokenises empty comments only (:214, :227)"
    out = torch.zeros(len(texts), clip_double.ARCH.context_length, dtype=torch.int64)
    if len(texts):
        out[:, 0], out[:, 1] = A.SOT, A.EOT
    return out


clip_double.tokenize = tokenize
torch.nn.module = torch.nn.Module          # :110

module_data = types.ModuleType("dataset_loaders.dataset_loaders")
package = types.ModuleType("dataset_loaders")
package.dataset_loaders = module_data
sys.modules["dataset_loaders"], sys.modules["dataset_loaders.dataset_loaders"] = package, module_data

import importlib.util  # noqa: E402

_spec = importlib.util.spec_from_file_location("ref_retrieval_evaluation", os.path.join(REF, "evaluation", "retrieval_evaluation.py"))
RE = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(RE)
assert RE.__file__.startswith(REF), RE.__file__
assert RE.module_arch.__file__.startswith(REF), RE.module_arch.__file__
assert RE.RecallAtK.__module__ == "model.metric" and sys.modules["model.metric"].__file__.startswith(REF)

_DataLoader = RE.DataLoader
RE.DataLoader = lambda dataset, **kw: _DataLoader(dataset, **dict(kw, num_workers=0))
_compute_recall = RE.compute_recall
captured = {}


def _spy(tensor_v, tensor_t, **kw):
    captured["v"], captured["t"] = tensor_v.clone(), tensor_t.clone()
    return _compute_recall(tensor_v, tensor_t, **kw)


RE.compute_recall = _spy

DEFAULT_STANDIN = dict(D.VIDEO_STANDIN)
TINY_STANDIN = dict(n_videos=12, min_frames=20, max_frames=16 * 8 * 3, resolution=A.TINY.image_resolution, context=A.TINY.context_length)
CAM = dict(n_heads=2)                       # TINY's embed_dim is 128: two heads keep the CAM's head_dim at 64
# (name, model, arch, ctor, wseed, dataset, split, loop flags, stand-in overrides incl. the chosen seed, extras)
CASES = [
    ("clip_msrvtt", "clip", "TINY", {}, 81, "MSRVTT_videos", "full-test", {}, dict(seed=130), {}),
    ("finaltf_text_msrvtt_dummy_comments", "clip_finaltf", "TINY", dict(branch_to_adapt_val="text", **CAM), 82,
     "MSRVTT_videos", "full-test", {}, dict(seed=135), {}),
    ("finaltf_image_k700", "clip_finaltf", "TINY", dict(branch_to_adapt_val="image", **CAM), 83,
     "K700_videos", "test", {}, dict(seed=124), {}),
    ("finaltf_skip_k700", "clip_finaltf", "TINY", dict(branch_to_adapt_val="skip", **CAM), 83,
     "K700_videos", "test", {}, dict(seed=130), {}),
    ("finaltf_text_msvd_first_frame", "clip_finaltf", "TINY", dict(branch_to_adapt_val="text", **CAM), 84,
     "MSVD_videos", "test", dict(first_frame_only=True), dict(seed=123), {}),
    ("finaltf_image_k700_first_chunk", "clip_finaltf", "TINY", dict(branch_to_adapt_val="image", **CAM), 85,
     "K700_videos", "test", dict(first_chunk_only=True), dict(seed=125), {}),
    ("finaltf_image_k700_stride4", "clip_finaltf", "TINY", dict(branch_to_adapt_val="image", **CAM), 86,
     "K700_videos", "test", dict(frame_stride=4), dict(seed=123, min_frames=5, max_frames=4 * 8 * 3), {}),
    ("finaltf_text_reddit_one_frame", "clip_finaltf", "TINY", dict(branch_to_adapt_val="text", **CAM), 87,
     "Reddit_videos", "test", {}, dict(seed=123), {}),
    # the TimeSformer wrappers exist in the reference at ViT-B/32 only: one full chunk, two chunks with a 5-frame tail, one 8-frame
    # item (one frame after the stride, resampled eight times); three videos, so embeddings only and no gap condition
    ("timesformer_finaltf_text_vit_b32", "timesformer_finaltf", "VIT_B32", dict(branch_to_adapt_val="text"), 88,
     "MSRVTT_videos", "full-test", {}, dict(seed=123, n_videos=3, resolution=224, context=77),
     dict(lengths=[16 * 8, 16 * 13 - 3, 8], bf16_pixels=True, nonzero_seed=89)),
]


def make_case(name, model, arch, ctor, wseed, dataset, split, loop, standin, extra):
    base = dict(DEFAULT_STANDIN, **(TINY_STANDIN if arch == "TINY" else {}))
    return dict(kind="retrieval_evaluation", name=name, model=model, arch=arch, ctor=ctor, wseed=wseed, dataset=dataset, split=split,
                loop=loop, standin=dict(base, **standin), **extra)


def run_reference(case):
    """One call of the reference's retrieval_evaluation on the reference's wrapper; (DataFrame, tensor_v, tensor_t)."""
    m, a = G.build_wrapper(case["model"], case["arch"], seed=case["wseed"], **case["ctor"])
    m.load_state_dict(C.state_dict(case), strict=True)
    D.VIDEO_STANDIN = C.standin(case, DEFAULT_STANDIN)
    for cls_name in C.DATASETS.values():
        setattr(module_data, cls_name, getattr(D, cls_name))
    setattr(module_data, C.DATASETS[case["dataset"]], C.dataset_class(case, D))
    captured.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        df = RE.retrieval_evaluation(m, case["dataset"], case["split"], "cpu", **case["loop"])
    return df, captured["v"], captured["t"]


def chunk_mix(case):
    """Whether the case's videos give 1, 2 and 3 chunks and a ragged tail among them (where the case chunks drawn lengths at all)."""
    if case.get("lengths") is not None or case["dataset"] == "Reddit_videos" or case["loop"].get("first_frame_only"):
        return True
    D.VIDEO_STANDIN = C.standin(case, DEFAULT_STANDIN)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lengths = C.dataset_class(case, D)(train=False, split=case["split"]).lengths.tolist()
    strided = [-(-n // case["loop"].get("frame_stride", 16)) for n in lengths]
    return {1, 2, 3} <= {-(-n // 8) for n in strided} and any(n % 8 for n in strided)


def search(case, tries=400):
    bound = E.rank_safety_bound(C.EPS, C.ARCH[case["arch"]].embed_dim)
    for seed in range(case["standin"]["seed"], case["standin"]["seed"] + tries):
        case["standin"]["seed"] = seed
        if not chunk_mix(case):
            continue
        _, v, t = run_reference(case)
        gap = E.table_gap(v.numpy(), t.numpy())
        print(f"  {case['name']}: seed {seed} gap {gap:.3e} (bound {bound:.3e})", flush=True)
        if gap >= bound:
            return seed
    raise SystemExit(f"{case['name']}: no seed in {tries} tries")


# ---- evaluation/eval.py::main (the image-text evaluation that writes the results JSON) ------------------------------------------------
# ``main`` touches its config through get_logger / init_obj / [...] only and its args through num_irrelevant_comments only, so a
# duck-typed config drives the reference's unmodified file; ``utils.parse_config`` (needs pyjson5 and the logger package) is a stand-in
# module whose ConfigParser is the annotation's name and nothing more.
class DuckConfig(dict):
    def get_logger(self, name):
        import logging
        return logging.getLogger(name)

    def init_obj(self, name, module, *args, **kwargs):
        return getattr(module, self[name]["type"])(*args, **dict(self[name]["args"], **kwargs))


def import_reference_eval():
    for name in ("utils", "utils.parse_config"):
        assert name not in sys.modules, name
        sys.modules[name] = types.ModuleType(name)
    sys.modules["utils.parse_config"].ConfigParser = object
    sys.modules["utils"].parse_config = sys.modules["utils.parse_config"]
    spec = importlib.util.spec_from_file_location("ref_eval", os.path.join(REF, "evaluation", "eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.__file__.startswith(REF) and mod.module_arch.__file__.startswith(REF), mod.__file__
    loader = mod.DataLoader
    mod.DataLoader = lambda dataset, **kw: loader(dataset, **dict(kw, num_workers=0))
    return mod


# n_pairs = 14 in batches of 4: three full batches and a last one of two (the reference's torch.squeeze breaks on a last batch of one)
EVAL_MAIN = dict(kind="eval_main", name="finaltf_text", model="clip_finaltf", arch="TINY", wseed=91,
                 ctor=dict(branch_to_adapt_val="text", **CAM), arch_type="PretrainedCLIP_finaltf", dataset_type="ImTextDataset",
                 dataset_args=dict(csv_file="", add_comments="always", num_comms=5, n_pairs=14, seed=123,
                                   resolution=A.TINY.image_resolution, context=A.TINY.context_length),
                 batch_size=4, num_irrelevant_comments=0)
KEYS = ["R1_title_from_im", "R5_title_from_im", "R10_title_from_im", "R1_im_from_title", "R5_im_from_title", "R10_im_from_title"]


def run_reference_eval_main(ref_eval, case):
    """One call of the reference's main() on a checkpoint holding the seeded state dict; (the written JSON, res_vis, res_text)."""
    import argparse
    import pathlib
    import tempfile
    clip_double.ARCH = C.ARCH[case["arch"]]
    module_data.ImTextDataset = D.ImTextDataset
    config = DuckConfig(arch=dict(type=case["arch_type"], args=dict(case["ctor"])),
                        dataset=dict(type=case["dataset_type"], args=dict(case["dataset_args"])), batch_size=case["batch_size"])
    stacked = []

    original = ref_eval.RecallAtK

    class Spy(original):                      # main returns nothing: record what it hands to RecallAtK.compute (:121-126)
        def compute(self, features_a, features_b):
            stacked.append((features_a.copy(), features_b.copy()))
            return super().compute(features_a, features_b)

    ref_eval.RecallAtK = Spy
    try:
        with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ckpt = pathlib.Path(tmp) / "checkpoint.pth"
            torch.save({"state_dict": C.state_dict(case)}, ckpt)
            ref_eval.main(config, argparse.Namespace(num_irrelevant_comments=case["num_irrelevant_comments"]), ckpt, device="cpu")
            written = [f for f in os.listdir(tmp) if f.endswith(".json")]
            assert written == [f"checkpoint_res_adapted_{case['ctor']['branch_to_adapt_val']}_{case['dataset_args']['num_comms']}_comms.json"]
            out = json.load(open(os.path.join(tmp, written[0])))
    finally:
        ref_eval.RecallAtK = original
    (res_vis, res_text), (text_again, vis_again) = stacked                   # compute(res_vis, res_text), compute(res_text, res_vis)
    assert np.array_equal(res_vis, vis_again) and np.array_equal(res_text, text_again)
    return out, res_vis, res_text


def gen_eval_main(search_mode):
    ref_eval = import_reference_eval()
    case = dict(EVAL_MAIN, dataset_args=dict(EVAL_MAIN["dataset_args"]))
    bound = E.rank_safety_bound(C.EPS, C.ARCH[case["arch"]].embed_dim)
    for seed in range(case["dataset_args"]["seed"], case["dataset_args"]["seed"] + (400 if search_mode else 1)):
        case["dataset_args"]["seed"] = seed
        out, res_vis, res_text = run_reference_eval_main(ref_eval, case)
        gap = E.table_gap(res_vis, res_text)
        if gap >= bound:
            break
    if search_mode:
        print(f"eval_main {case['name']}: seed {seed}")
        return
    assert list(out) == KEYS and res_vis.shape == res_text.shape == (case["dataset_args"]["n_pairs"], C.ARCH[case["arch"]].embed_dim)
    assert gap >= bound, f"eval_main: boundary gap {gap:.3e} < 2 delta {bound:.3e}: choose another seed"
    case.update(gap=gap, eps=C.EPS, two_delta=bound)
    G.save(f"evalmain_00_{case['name']}", case, res_vis=res_vis, res_text=res_text, values=np.array([out[k] for k in KEYS], dtype=np.float64),
           keys=np.array(KEYS), gap=np.float64(gap))
    print(f"  gap {gap:.3e} >= 2 delta {bound:.3e}", out)


if __name__ == "__main__":
    os.environ.pop("VTC_SYNTHETIC_VIDEOS", None)
    torch.manual_seed(0)
    only = os.environ.get("EVAL_GOLDEN_ONLY")
    for i, spec in enumerate(CASES):
        case = make_case(*spec)
        if only and only not in case["name"]:
            continue
        tiny = case["arch"] == "TINY"
        if os.environ.get("EVAL_GOLDEN_SEARCH"):
            if tiny:
                print(f"{case['name']}: seed {search(case)}")
            continue
        df, v, t = run_reference(case)
        assert chunk_mix(case), f"{case['name']}: the videos must give 1, 2 and 3 chunks with ragged tails: choose another seed"
        assert v.dtype == torch.float32 and t.dtype == torch.float32 and t.shape == (v.shape[0], 1, v.shape[1])
        gap = E.table_gap(v.numpy(), t.numpy())
        case["gap"] = gap
        if tiny:
            assert v.shape[0] >= 12, "R@10 must not be trivially 100 %"
            case["eps"], case["two_delta"] = C.EPS, E.rank_safety_bound(C.EPS, v.shape[1])
            assert gap >= case["two_delta"], f"{case['name']}: boundary gap {gap:.3e} < 2 delta {case['two_delta']:.3e}: choose another seed"
        G.save(f"eval_{i:02d}_{case['name']}", case, tensor_v=v.numpy(), tensor_t=t.numpy(), table=df.to_numpy().astype(np.float64),
               columns=np.array(list(df.columns)), index=np.array(list(df.index)), gap=np.float64(gap))
        print(f"  gap {gap:.3e}" + (f" >= 2 delta {case['two_delta']:.3e}" if tiny else " (no table assertion)"), df.to_numpy().T.tolist())
    if not only or only in "eval_main":
        gen_eval_main(bool(os.environ.get("EVAL_GOLDEN_SEARCH")))
