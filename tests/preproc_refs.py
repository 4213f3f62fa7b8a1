"""Integer restatement of the frame preprocessing (Resize(size, BICUBIC) + CenterCrop(size) of CLIP_TRANSFORM,
dataset_loaders/dataset_loaders.py:40-49) in numpy, and a closed-form input generator (no RNG).

The restatement follows Pillow's 8-bit resampling (two separable passes, horizontal first, the intermediate image rounded to uint8,
22-bit integer coefficients made from double weights) and torchvision's size and crop arithmetic; tests/test_preproc_refs.py holds it
to Pillow's own outputs (tests/golden/resize_cases.npz) bit for bit.  It is the reference of the GPU tests and lays the plan out
exactly as vtc_resize_plan does (include/vtc_hip.h), so the two can be compared integer for integer."""
import math

import numpy as np

PRECISION_BITS = 22
PLAN_MAGIC = 0x31505256          # "VRP1"
PLAN_HEADER_WORDS = 16
SPECIALS = ("zeros", "full", "checker")


# ---- inputs -------------------------------------------------------------------------------------
def make_frame(h, w, kind="pattern", index=0):
    """[h, w, 3] uint8, a closed form of (x, y, c) and the frame index.  "pattern": every byte value, a fine texture (so a wrong tap
    or a shifted window shows) over slow ramps; "zeros" / "full": constant 0 / 255 (do the rounded coefficients sum as Pillow's do);
    "checker": 0 / 255 alternating per pixel and channel (bicubic's negative lobes overshoot both ends: the clamp)."""
    y, x, c = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), np.arange(3, dtype=np.int64), indexing="ij")
    if kind == "pattern":
        v = x * 7 + y * 13 + c * 29 + ((x * y) % 31) * 5 + ((x >> 2) ^ (y >> 1)) * 3 + index * 37
    elif kind == "zeros":
        v = np.zeros_like(x)
    elif kind == "full":
        v = np.full_like(x, 255)
    elif kind == "checker":
        v = ((x + y + c + index) & 1) * 255
    else:
        raise ValueError(kind)
    return (v & 255).astype(np.uint8)


def make_frames(n, h, w, kind="pattern"):
    return np.stack([make_frame(h, w, kind, i) for i in range(n)])


# ---- the plan -----------------------------------------------------------------------------------
def resize_target(in_h, in_w, size):
    """torchvision Resize(size) with an int: (out_h, out_w)."""
    if in_w <= in_h:
        return int(size * in_h / in_w), size
    return size, int(size * in_w / in_h)


def crop_offset(n_out, size):
    """torchvision CenterCrop: Python's round (ties to even)."""
    return int(round((n_out - size) / 2.0))


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def axis_plan(n_in, n_out, lo, size):
    """(first [size], count [size], coef [size, ksize] int32, ksize) for the output indices lo .. lo + size - 1 of an axis resampled from
    n_in to n_out samples.  n_in == n_out: the pass is the identity (one tap of 2^22)."""
    if n_in == n_out:
        first = np.arange(lo, lo + size, dtype=np.int32)
        return first, np.ones(size, np.int32), np.full((size, 1), 1 << PRECISION_BITS, np.int32), 1
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs                                     # Pillow multiplies by the reciprocal
    first, count, coef = np.zeros(size, np.int32), np.zeros(size, np.int32), np.zeros((size, ksize), np.int32)
    for i in range(size):
        center = (lo + i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        first[i], count[i] = xmin, xmax
        for x, v in enumerate(w):
            coef[i, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return first, count, coef, ksize


def plan(in_h, in_w, size):
    out_h, out_w = resize_target(in_h, in_w, size)
    top, left = crop_offset(out_h, size), crop_offset(out_w, size)
    return dict(in_h=in_h, in_w=in_w, size=size, out_h=out_h, out_w=out_w, top=top, left=left,
                cols=axis_plan(in_w, out_w, left, size), rows=axis_plan(in_h, out_h, top, size))


def plan_words(in_h, in_w, size):
    """The plan as vtc_resize_plan lays it out: int32 words -- a 16-word header (magic, in_h, in_w, size, out_w, out_h, left, top, column
    taps, row taps, 0 ...), then per cropped output column (first, count, coefficients[column taps]), then the same per row."""
    p = plan(in_h, in_w, size)
    words = [PLAN_MAGIC, in_h, in_w, size, p["out_w"], p["out_h"], p["left"], p["top"], p["cols"][3], p["rows"][3]]
    words += [0] * (PLAN_HEADER_WORDS - len(words))
    parts = [np.asarray(words, np.int32)]
    for first, count, coef, _ in (p["cols"], p["rows"]):
        parts.append(np.concatenate([first[:, None], count[:, None], coef], axis=1).reshape(-1))
    return np.concatenate(parts).astype(np.int32)


# ---- the two passes -----------------------------------------------------------------------------
def _pass(src, first, count, coef, base):
    """src [n_in, m, 3] uint8 resampled along axis 0 -> [size, m, 3] uint8; row indices are first - base."""
    acc = np.full((first.shape[0],) + src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    for t in range(coef.shape[1]):
        live = t < count
        if not live.any():
            break
        idx = np.where(live, first - base + t, 0)
        acc += src[idx].astype(np.int64) * np.where(live, coef[:, t], 0).astype(np.int64)[:, None, None]
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_crop(frame, size):
    """frame [h, w, 3] uint8 -> [3, size, size] uint8."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
    p = plan(frame.shape[0], frame.shape[1], size)
    cf, cc, ck, _ = p["cols"]
    rf, rc, rk, _ = p["rows"]
    r0, r1 = int(rf.min()), int((rf + rc).max())                   # only the source rows in the vertical support
    tmp = _pass(frame[r0:r1].transpose(1, 0, 2), cf, cc, ck, 0)    # horizontal: [size(x), rows, 3], rounded to uint8
    out = _pass(tmp.transpose(1, 0, 2), rf, rc, rk, r0)            # vertical:   [size(y), size(x), 3]
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def resize_crop_batch(frames, size):
    return np.stack([resize_crop(f, size) for f in frames])


def pillow_resize_crop(frame, size):
    """The same through Pillow itself (what the fixtures hold)."""
    from PIL import Image
    h, w = frame.shape[:2]
    out_h, out_w = resize_target(h, w, size)
    im = Image.fromarray(frame, "RGB").resize((out_w, out_h), Image.BICUBIC)
    top, left = crop_offset(out_h, size), crop_offset(out_w, size)
    a = np.asarray(im)[top:top + size, left:left + size]
    return np.ascontiguousarray(a.transpose(2, 0, 1))
