"""Frame preprocessing on the GPU (ops.clip_resize_crop: Resize(224, BICUBIC) + CenterCrop(224), bit for bit Pillow's) against what it
replaces and what surrounds it:

    python tools/preproc_bench.py [--size 224] [--frames 8192] [--frames-large 1024] [--threads 16] [--out FILE]

For 240x320, 360x640, 720x1280 and 1080x1920 sources, one JSON line each:
  gpu_us_per_frame     HIP events around back-to-back calls on --frames frames (--frames-large at the two large sizes), warm, a window
                       of at least 0.3 s; median / min / max over 5 windows
  bytes_per_frame      what the kernel MUST move: the crop window of the source (the rows and columns in the support of the cropped
                       output, read once) + the output written once; gb_per_s = that over the GPU time
  pillow_us_per_frame  Image.resize(BICUBIC) + crop of the same frames on --threads host threads (Pillow releases the GIL), wall clock over
                       the whole set divided by the frame count; null where Pillow does not import
  upload_us_per_frame  pinned host -> device copy of the raw frames (what a pipeline pays in front of the kernel), events
  bound                "upload" or "kernel": the slower of the two per frame
and one line for the ViT-B/32 8-frame TimeSformer visual tower (bf16, raw uint8 pixels) on --frames frames of 224 x 224: the consumer,
on the same box in the same process, so that the share of a step that preprocessing is can be read off.
Frames are random bytes (the arithmetic does not depend on the content).  profiles/preproc.md holds a run's output."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vtc_amd import _lib as L  # noqa: E402
from vtc_amd import ops  # noqa: E402

SOURCES = [(240, 320, False), (360, 640, False), (720, 1280, True), (1080, 1920, True)]


def window_bytes(h, w, size):
    """(source bytes in the crop window's support, output bytes) per frame, from the host plan."""
    lib = L.lib()
    nbytes = lib.vtc_resize_plan_bytes(h, w, size)
    p = np.zeros(nbytes // 4, np.int32)
    L.check(lib.vtc_resize_plan(h, w, size, p.ctypes.data, nbytes), "vtc_resize_plan")
    kx, ky = int(p[8]), int(p[9])
    cols = p[16:16 + size * (2 + kx)].reshape(size, 2 + kx)
    rows = p[16 + size * (2 + kx):].reshape(size, 2 + ky)
    span = lambda r: int((r[:, 0] + r[:, 1]).max() - r[:, 0].min())            # noqa: E731
    return 3 * span(cols) * span(rows), 3 * size * size, kx, ky


def event_windows(fn, min_s=0.3, windows=5):
    """Per-call milliseconds over `windows` windows of back-to-back calls, each at least min_s long."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(1, int(min_s / max(time.perf_counter() - t0, 1e-6)) + 1)
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out, reps


def stat(ms_per_call, n):
    us = [1e3 * t / n for t in ms_per_call]
    return {"median": round(float(np.median(us)), 4), "min": round(min(us), 4), "max": round(max(us), 4)}


def pillow_time(frames, size, threads):
    try:
        from PIL import Image
    except ImportError:
        return None
    h, w = frames.shape[1:3]
    out_w, out_h = (size, int(size * h / w)) if w <= h else (int(size * w / h), size)
    top, left = int(round((out_h - size) / 2.0)), int(round((out_w - size) / 2.0))

    def one(i):
        im = Image.fromarray(frames[i], "RGB").resize((out_w, out_h), Image.BICUBIC)
        return np.asarray(im.crop((left, top, left + size, top + size)))

    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(one, range(min(len(frames), 2 * threads))))                 # warm
        t0 = time.perf_counter()
        list(pool.map(one, range(len(frames))))
        return 1e6 * (time.perf_counter() - t0) / len(frames)


def tower_line(n, size):
    """The ViT-B/32 8-frame TimeSformer visual tower in bf16 on n raw uint8 frames (the headline step's visual half)."""
    from oracle import arch as A
    from vtc_amd import towers
    a = A.VIT_B32
    sd = {k: v.cuda() for k, v in A.synth_visual(a, 171, nframes=8, prefix="v.").items()}
    pv = towers.PackedVision(sd, "v.", torch.bfloat16)
    chunk = min(n, 8192)
    px = torch.randint(0, 256, (chunk // 8, 8, 3, a.image_resolution, a.image_resolution), dtype=torch.uint8, device="cuda")
    ms, reps = event_windows(lambda: pv.forward(px), windows=3)
    return {"case": "vision_tower_vit_b32_timesformer8_bf16", "frames": chunk, "tower_us_per_frame": stat(ms, chunk), "reps_per_window": reps}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--frames-large", type=int, default=1024)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--pillow-frames", type=int, default=512, help="frames of each size the Pillow leg runs (its time is per frame)")
    ap.add_argument("--no-tower", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    lines = []
    g = torch.Generator(device="cuda").manual_seed(1)
    for h, w, large in SOURCES:
        n = args.frames_large if large else args.frames
        frames = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)
        out = torch.empty(n, 3, args.size, args.size, dtype=torch.uint8, device="cuda")
        ms, reps = event_windows(lambda: ops.clip_resize_crop(frames, args.size, out=out))
        src_b, out_b, kx, ky = window_bytes(h, w, args.size)
        gpu = stat(ms, n)
        # the upload a pipeline pays in front of the kernel: pinned host memory, at most 1 GiB of the frames
        m = max(1, min(n, (1 << 30) // (h * w * 3)))
        host = frames[:m].cpu().pin_memory()
        dst = torch.empty_like(frames[:m])
        up_ms, _ = event_windows(lambda: dst.copy_(host, non_blocking=True), min_s=0.2, windows=3)
        up = stat(up_ms, m)
        nf = min(n, args.pillow_frames)
        pil = pillow_time(frames[:nf].cpu().numpy(), args.size, args.threads)
        line = {"case": f"{h}x{w}", "size": args.size, "frames": n, "taps": [kx, ky], "reps_per_window": reps, "gpu_us_per_frame": gpu,
                "gpu_frames_per_s": round(1e6 / gpu["median"], 1), "bytes_per_frame": {"source_window": src_b, "output": out_b},
                "gb_per_s": round((src_b + out_b) / (1e3 * gpu["median"]), 2), "upload_us_per_frame": up,
                "upload_gb_per_s": round(h * w * 3 / (1e3 * up["median"]), 2), "bound": "upload" if up["median"] > gpu["median"] else "kernel",
                "pillow_threads": args.threads, "pillow_us_per_frame": None if pil is None else round(pil, 2),
                "pillow_over_gpu": None if pil is None else round(pil / gpu["median"], 1)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del frames, out, host, dst
        torch.cuda.empty_cache()
    if not args.no_tower:
        line = tower_line(args.frames, args.size)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
