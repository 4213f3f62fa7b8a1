"""CPU: the integer restatement of Resize(size, BICUBIC) + CenterCrop(size) (tests/preproc_refs.py) against Pillow's own outputs
(tests/golden/resize_cases.npz; against Pillow itself where it imports), and vtc_resize_plan -- pure host code -- against the
restatement's plan, integer for integer.  The GPU tests (tests/test_gpu_preproc.py) hold the kernel to the restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

import preproc_refs as R
from conftest import load_golden

_CASE, _OUT = load_golden("resize_cases.npz")
CASES = [tuple(c) for c in _CASE["cases"]]
# what the GPU tests run, plus sizes around every branch of the plan: identity passes, the crop's round-half-even tie, both
# orientations, one-pixel edges, the largest frame the issue names and the edge limit
PLAN_CASES = sorted({(h, w, s) for h, w, s, _ in CASES} | {
    (224, 224, 224), (225, 224, 224), (224, 227, 224), (37, 61, 224), (96, 128, 224), (240, 320, 224), (320, 240, 224), (231, 500, 224),
    (500, 333, 224), (720, 1280, 224), (1080, 1920, 224), (2160, 3840, 224), (1300, 1300, 64), (1, 1, 16), (1, 40, 16), (40, 1, 16),
    (8192, 16, 16), (17, 8192, 32), (3, 5, 1024)})


def test_fixture_names_its_pillow_and_covers_the_issue():
    assert _CASE["pillow"]
    assert len({(h, w) for h, w, s, _ in CASES if s == 64}) >= 12 and len([c for c in CASES if c[2] == 224]) == 2
    assert {k for *_, k in CASES} == {"pattern", *R.SPECIALS}


@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{h}x{w}-{s}-{k}" for h, w, s, k in CASES])
def test_restatement_equals_pillow_fixture(i):
    h, w, size, kind = CASES[i]
    got = R.resize_crop(R.make_frame(h, w, kind), size)
    assert got.shape == (3, size, size) and got.dtype == np.uint8
    assert np.array_equal(got, _OUT[f"out{i}"])


def test_specials_exercise_the_clamp_and_the_coefficient_sum():
    """A 0 / 255 checker overshoots both ends before the clamp; a constant image must come back constant."""
    assert (R.resize_crop(R.make_frame(37, 61, "full"), 64) == 255).all() and (R.resize_crop(R.make_frame(240, 320, "zeros"), 64) == 0).all()
    up = R.resize_crop(R.make_frame(37, 61, "checker"), 64)
    assert up.min() == 0 and up.max() == 255


@pytest.mark.parametrize("h,w,size", [(37, 61, 64), (61, 37, 64), (225, 224, 224), (224, 224, 224), (240, 320, 224), (500, 333, 224),
                                      (231, 500, 64), (720, 1280, 224), (1080, 1920, 64)])
def test_restatement_equals_pillow(h, w, size):
    pytest.importorskip("PIL")
    for kind in ("pattern",) + R.SPECIALS:
        f = R.make_frame(h, w, kind)
        assert np.array_equal(R.resize_crop(f, size), R.pillow_resize_crop(f, size)), kind


def _lib():
    from vtc_amd import _lib as L
    return L.lib()


@pytest.mark.parametrize("h,w,size", PLAN_CASES, ids=[f"{h}x{w}-{s}" for h, w, s in PLAN_CASES])
def test_host_plan_equals_the_restatement(h, w, size):
    lib = _lib()
    want = R.plan_words(h, w, size)
    nbytes = lib.vtc_resize_plan_bytes(h, w, size)
    assert nbytes == want.nbytes
    got = np.full(want.size + 4, -7, np.int32)                 # four guard words behind the plan
    assert lib.vtc_resize_plan(h, w, size, got.ctypes.data, nbytes) == 0, lib.vtc_last_error()
    assert (got[want.size:] == -7).all()
    assert np.array_equal(got[:want.size], want)


def test_argument_errors_are_statuses_with_a_message():
    lib = _lib()
    buf = np.zeros(1 << 16, np.int32)
    for h, w, size in ((240, 320, 0), (240, 320, -16), (240, 320, 100), (240, 320, 1040), (0, 320, 224), (240, 0, 224), (8193, 320, 224),
                       (240, 8193, 224)):
        assert lib.vtc_resize_plan_bytes(h, w, size) == 0
        assert lib.vtc_resize_plan(h, w, size, buf.ctypes.data, buf.nbytes) != 0
        assert b"resize_plan" in lib.vtc_last_error()
        # the launch entry point refuses the same arguments before it touches the device (the pointers are never read)
        assert lib.vtc_resize_crop_u8(16, 1, h, w, 0, 16, size, 16, None) != 0
        assert b"resize_crop_u8" in lib.vtc_last_error()
    need = lib.vtc_resize_plan_bytes(240, 320, 224)
    assert need > 0
    assert lib.vtc_resize_plan(240, 320, 224, buf.ctypes.data, need - 4) != 0 and b"needed" in lib.vtc_last_error()
    assert lib.vtc_resize_plan(240, 320, 224, None, need) != 0
    for args in ((16, 1, 240, 320, 2, 16, 224, 16, None),      # layout
                 (16, 0, 240, 320, 0, 16, 224, 16, None),      # no frames
                 (None, 1, 240, 320, 0, 16, 224, 16, None),    # null frames
                 (16, 1, 240, 320, 0, 16, 224, 24, None)):     # out not 16-byte aligned
        assert lib.vtc_resize_crop_u8(*args) != 0 and b"resize_crop_u8" in lib.vtc_last_error()


def test_python_layer_refuses_bad_frames_before_any_launch():
    from vtc_amd import ops
    from vtc_amd.host.transforms import ClipPreprocessGPU
    ok = torch.zeros(2, 24, 32, 3, dtype=torch.uint8)
    for bad, kw in ((ok.float(), {}), (ok[0, 0], {}), (ok.reshape(1, 1, 2, 24, 32, 3), {}), (torch.zeros(24, 32, 4, dtype=torch.uint8), {}),
                    (ok, dict(size=100)), (ok, dict(size=0)), (ok, dict(layout="nhwc")), (ok, dict(layout="chw")),
                    (torch.zeros(0, 24, 32, 3, dtype=torch.uint8), {})):
        with pytest.raises(ValueError):
            ops.clip_resize_crop(bad, **kw)
    with pytest.raises(ValueError):
        ClipPreprocessGPU(64, layout="whc")
    with pytest.raises(ValueError):
        ClipPreprocessGPU(64, device="cpu")([])
    with pytest.raises(ValueError):
        ClipPreprocessGPU(64, device="cpu")([ok.float()])
