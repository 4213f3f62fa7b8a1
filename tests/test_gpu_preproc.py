"""GPU: vtc_resize_crop_u8 and the layers above it against the integer restatement of tests/preproc_refs.py (itself held to Pillow by
tests/test_preproc_refs.py).  Every comparison is torch.equal: the operation is integer arithmetic, there is no tolerance."""
import functools
from dataclasses import asdict

import numpy as np
import pytest
import torch

import preproc_refs as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# source size -> what it exercises (the smallest sizes that reach each way the kernel can go wrong)
SIZES = [(240, 320), (320, 240),      # landscape / portrait downscale
         (224, 224),                  # both passes the identity at size 224
         (225, 224),                  # one identity pass, an odd crop on the round-half-even tie
         (37, 61), (96, 128),         # upscale; taps clamped at both borders; odd, unaligned row pitch
         (231, 500),                  # extreme aspect ratio
         (500, 333)]                  # odd width, portrait
# (source, size): long supports in the LDS band
LONG = [(720, 1280, 224), (1080, 1920, 224),      # 15 and 21 taps, bands of 16 rows, the 1 024-thread workgroups
        (1080, 1920, 64),                         # 69 taps
        (1300, 1300, 64),                         # 83 taps, bands of 8 rows
        (2160, 3840, 224), (2160, 3840, 64)]      # the largest frame the limits must admit: 41 taps (bands of 4 rows) and 137


@functools.lru_cache(maxsize=None)
def _frames(n, h, w, kind):
    f = R.make_frames(n, h, w, kind)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _ref(n, h, w, kind, size):
    """[n, 3, size, size] uint8 (torch, CPU): computed once per case, shared, never written."""
    return torch.from_numpy(R.resize_crop_batch(_frames(n, h, w, kind), size))


def _gpu_frames(n, h, w, kind, layout):
    f = torch.from_numpy(_frames(n, h, w, kind).copy()).cuda()
    return f if layout == "hwc" else f.permute(0, 3, 1, 2).contiguous()


def _run_guarded(frames, size, layout):
    """The op into a buffer with 64 guard bytes on each side of `out`; returns the result on the CPU after checking the guards."""
    from vtc_amd import ops
    shape = tuple(frames.shape[:-3]) + (3, size, size)
    numel = int(np.prod(shape))
    buf = torch.full((numel + 128,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[64:64 + numel].view(shape)
    assert out.data_ptr() % 16 == 0
    got = ops.clip_resize_crop(frames, size, layout, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert bool((buf[:64] == 0xA5).all()) and bool((buf[64 + numel:] == 0xA5).all()), "guard bytes around `out` were written"
    return got.cpu()


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("size", [64, 224])
@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_resize_crop_equals_the_restatement(h, w, size, layout):
    got = _run_guarded(_gpu_frames(3, h, w, "pattern", layout), size, layout)
    assert torch.equal(got, _ref(3, h, w, "pattern", size))


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("h,w,size", [(240, 320, 224), (37, 61, 64), (500, 333, 64)])
def test_frame_counts(h, w, size, n, layout):
    got = _run_guarded(_gpu_frames(n, h, w, "pattern", layout), size, layout)
    assert torch.equal(got, _ref(n, h, w, "pattern", size))


@pytest.mark.parametrize("kind", R.SPECIALS)
@pytest.mark.parametrize("h,w,size", [(37, 61, 64), (240, 320, 224), (225, 224, 224), (500, 333, 64)])
def test_special_images(h, w, size, kind):
    """All 0, all 255 (the rounded coefficients sum as Pillow's do), and a 0 / 255 checker (the negative lobes overshoot: the clamp)."""
    for layout in ("hwc", "chw"):
        got = _run_guarded(_gpu_frames(2, h, w, kind, layout), size, layout)
        assert torch.equal(got, _ref(2, h, w, kind, size))


@pytest.mark.parametrize("h,w,size", LONG)
def test_long_supports_one_frame(h, w, size):
    for layout in ("hwc", "chw"):
        got = _run_guarded(_gpu_frames(1, h, w, "pattern", layout), size, layout)
        assert torch.equal(got, _ref(1, h, w, "pattern", size))


def test_frames_past_two_gib():
    """88 frames of 2160 x 3840 are 2.19e9 bytes: the last frame's offset does not fit 31 bits.  Only the first and the last frame carry
    the pattern (the others stay zero), so the reference is the one 2160 x 3840 frame of test_long_supports_one_frame."""
    n, h, w = 88, 2160, 3840
    assert (n - 1) * h * w * 3 > 2 ** 31
    from vtc_amd import ops
    one = torch.from_numpy(_frames(1, h, w, "pattern").copy()).cuda()
    frames = torch.zeros(n, h, w, 3, dtype=torch.uint8, device="cuda")
    frames[0], frames[n - 1] = one[0], one[0]
    got = ops.clip_resize_crop(frames, 224)
    want = _ref(1, h, w, "pattern", 224)[0]
    assert torch.equal(got[0].cpu(), want) and torch.equal(got[n - 1].cpu(), want)
    assert int(got[1:n - 1].max()) == 0


def test_non_contiguous_view_and_batch_of_videos():
    from vtc_amd import ops
    h, w = 96, 128
    want = _ref(6, h, w, "pattern", 64)
    base = torch.from_numpy(_frames(6, h, w, "pattern").copy()).cuda()
    big = torch.full((6, h + 5, w + 7, 3), 9, dtype=torch.uint8, device="cuda")
    big[:, 2:2 + h, 3:3 + w] = base
    view = big[:, 2:2 + h, 3:3 + w]
    assert not view.is_contiguous()
    assert torch.equal(ops.clip_resize_crop(view, 64).cpu(), want)
    planar = base.permute(0, 3, 1, 2)                                        # a CHW view of HWC memory
    assert not planar.is_contiguous()
    assert torch.equal(ops.clip_resize_crop(planar, 64, layout="chw").cpu(), want)
    vids = ops.clip_resize_crop(base.view(2, 3, h, w, 3), 64)                # [B, F, H, W, 3]
    assert vids.shape == (2, 3, 3, 64, 64) and torch.equal(vids.cpu(), want.view(2, 3, 3, 64, 64))
    single = ops.clip_resize_crop(base[4], 64)                               # one frame, no leading dimension
    assert single.shape == (3, 64, 64) and torch.equal(single.cpu(), want[4])


def test_mixed_sizes_keep_their_order():
    """Frames of different sizes, on the CPU (pinned and pageable) and on the GPU, one size met twice with another between: the result is one
    tensor in input order."""
    from vtc_amd.host.transforms import ClipPreprocessGPU
    spec = [(2, 240, 320), (1, 37, 61), (3, 240, 320), (3, 96, 128), (3, 96, 128), (1, 500, 333)]
    items, want = [], []
    for i, (n, h, w) in enumerate(spec):
        t = torch.from_numpy(_frames(n, h, w, "pattern").copy())
        want.append(_ref(n, h, w, "pattern", 64))
        if i == 1:
            t, want[-1] = t[0], want[-1][:1]                                 # a single [H, W, 3] frame
        items.append(t.cuda() if i % 3 == 0 else (t.pin_memory() if i % 3 == 1 else t))
    pre = ClipPreprocessGPU(64)
    got = pre(items)
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.cat(want))
    assert torch.equal(pre(items[2]).cpu(), want[2])                         # one tensor: the op's own shape rules


def test_a_plan_for_other_arguments_writes_nothing():
    """The call cannot read a plan in device memory; the kernel compares its header with the arguments and leaves `out` alone."""
    from vtc_amd import _lib as L
    from vtc_amd import ops
    frames = _gpu_frames(2, 96, 128, "pattern", "hwc")
    other = ops._resize_plan(240, 320, 64, frames.device)
    out = torch.full((2, 3, 64, 64), 0x5A, dtype=torch.uint8, device="cuda")
    rc = L.lib().vtc_resize_crop_u8(frames.data_ptr(), 2, 96, 128, 0, other.data_ptr(), 64, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    assert torch.equal(ops.clip_resize_crop(frames, 64, out=out).cpu(), _ref(2, 96, 128, "pattern", 64))


def test_model_preprocess_feeds_the_tower_bit_for_bit(tmp_path):
    """model.preprocess -> encode_image on the TINY architecture: the embeddings are those of the restatement's uint8 frames, bit for bit
    (same bytes in, same kernels); cache_clip_vit_embeddings(preprocess=...) stores the same rows from raw-size frames."""
    from oracle import arch as A
    from vtc_amd.host import cache_features as CF
    from vtc_amd.host import model as HM
    from vtc_amd.host.clip_arch import ClipConfig
    a = A.TINY
    res = a.image_resolution
    assert res % 16 == 0
    m = HM.PretrainedCLIP(model_type=ClipConfig(**asdict(a)))
    m.load_state_dict(A.synth_model(a, 72, "clip"), strict=True)
    m = m.eval().cuda()
    raw = [torch.from_numpy(_frames(2, 96, 128, "pattern").copy()), torch.from_numpy(_frames(3, 240, 320, "pattern").copy()).cuda()]
    want_px = torch.cat([_ref(2, 96, 128, "pattern", res), _ref(3, 240, 320, "pattern", res)])
    px = m.preprocess(raw)
    assert torch.equal(px.cpu(), want_px)
    for dtype in (torch.float32, torch.bfloat16):
        m.compute_dtype = dtype
        assert torch.equal(m.encode_image(px), m.encode_image(want_px.cuda()))
    want = torch.cat([m.encode_image(want_px[:2].cuda()), m.encode_image(want_px[2:].cuda())]).float().cpu()    # the producer's batches
    saved = CF.cache_clip_vit_embeddings(m, raw, [5, 6, 7, 8, 9], str(tmp_path / "emb.pth"), preprocess=m.preprocess)
    assert torch.equal(saved["embeddings"], want)


def test_the_documented_binding_runs():
    """INTEGRATION.md's ctypes example for the two entry points, executed as written against the built library."""
    import os
    import re
    from vtc_amd import _lib as L
    from vtc_amd import ops
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "vtc_resize_crop_u8" in b and "ctypes.CDLL" in b]
    assert len(blocks) == 1
    ns = {}
    exec(blocks[0].replace('ctypes.CDLL("libvtc_hip.so")', f'ctypes.CDLL("{L.LIB_PATH}")'), ns)
    torch.cuda.synchronize()
    assert ns["pixels"].shape == (8, 3, 224, 224) and torch.equal(ns["pixels"], ops.clip_resize_crop(ns["frames"], 224))
    want = R.resize_crop(ns["frames"][5].cpu().numpy(), 224)
    assert torch.equal(ns["pixels"][5].cpu(), torch.from_numpy(want))
