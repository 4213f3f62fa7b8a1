"""The grouped rank sweep (ops.rank_grouped: several captions per video) against its yardstick, the paired sweep (ops.rank_bidir) at the
square size with the same number of matrix entries, alternating in ONE process:

    python tools/grouped_rank_bench.py [--d 512] [--iters 20] [--warmup 3] [--identity 10000] [--out FILE]

Shapes: the two multi-caption benchmarks -- 2 990 videos x 20 captions (MSR-VTT full) and 670 videos with about 41 captions each (MSVD:
counts uniform in 31 .. 51) -- each timed against ops.rank_bidir at n = round(sqrt(n m)) rows: equal GEMM work and equal scanned bytes.
Then ops.rank_grouped with identity offsets (one caption per video) against ops.rank_bidir on the SAME data at --identity rows.  One JSON
line per comparison: both times (HIP events around each call, median / min / max over the timed iterations), the pairs in reach of their
target per owner and the owners that went to the fp64 brute force per direction (a = the captions' row direction, b = the videos' column
direction), and the per-kernel split of one sweep of each from the library's own launch records (tags 101 .. 105 = prologue, row count,
column count, settle, brute force).  Data: the generator of tests/grouped_rank_refs.py (a per-video noise scale, log-uniform in
[0.5, 60], times a per-caption jitter), drawn on the GPU.  profiles/r11_grouped_rank.md holds a run's output.
On the two multi-caption shapes a second line each: ops.rank_grouped_vunit (the same sweep with the video-unit direction, a third pass
over every block) alternating with ops.rank_grouped on the SAME tensors -- both times and their ratio, the (video, group) pairs in reach
per video and the videos counted by brute force, and the new pass under tags of its own (106 = vunit_count, 107 = vunit_finish: settle,
brute force and write).  profiles/r13_vunit_rank.md holds a run's output."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from vtc_amd import _lib as L  # noqa: E402
from vtc_amd import ops  # noqa: E402
from rank_sweep_bench import kernel_split, make, timed, unit  # noqa: E402


def make_grouped(counts, d, seed):
    """tests/grouped_rank_refs.py::grouped_spread, on the GPU (fp64 draws, fp32 rows)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n, m = len(counts), int(np.sum(counts))
    rand = lambda *shape: torch.rand(*shape, generator=g, device="cuda", dtype=torch.float64)                       # noqa: E731
    a = unit(torch.randn(n, d, generator=g, device="cuda", dtype=torch.float64))
    u = unit(torch.randn(m, d, generator=g, device="cuda", dtype=torch.float64))
    s = torch.exp(rand(n, 1) * (np.log(60.0) - np.log(0.5)) + np.log(0.5))
    j = torch.exp(rand(m, 1) * (np.log(1.4) - np.log(0.7)) + np.log(0.7))
    gid = torch.repeat_interleave(torch.arange(n, device="cuda"), torch.as_tensor(counts, device="cuda"))
    b = unit(a[gid] + s[gid] * j * u)
    return a.float().contiguous(), b.float().contiguous(), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def stats_of(ws, owners):
    st = ops.rank_sweep_stats(ws)
    return {"in_reach_per_owner_mean": [round(x / o, 2) for x, o in zip(st["in_reach"], owners)],
            "in_reach_per_owner_max": list(st["in_reach_max"]), "brute_force_owners": list(st["brute_force_owners"])}


def ms(t):
    return {"median": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}


def compare(name, grouped, paired, args, extra):
    """`grouped`, `paired`: (callable, workspace, owners per direction).  Alternating: both see the same box at the same time."""
    (fg, wg, og), (fp, wp, op) = grouped, paired
    for _ in range(args.warmup):
        fg()
        fp()
    tg, tp = [], []
    for _ in range(args.iters):
        tg.append(timed(fg))
        tp.append(timed(fp))
    ra, rb, bits = fg()
    line = dict(extra, case=name, d=args.d, iters=args.iters, rank_grouped_ms=ms(tg), rank_bidir_ms=ms(tp),
                ratio=round(float(np.median(tg)) / float(np.median(tp)), 3),
                paired_spread_max_over_min=round(max(tp) / min(tp), 3),
                grouped=dict(stats_of(wg, og), kernel_split_ms=kernel_split(fg)),
                paired=dict(stats_of(wp, op), kernel_split_ms=kernel_split(fp)),
                nonfinite_bits=int(bits.item()),
                **{"R@1": [round(float((ra < 1).float().mean()), 4), round(float((rb < 1).float().mean()), 4)],
                   "median_rank_1based": [float(ra.median()) + 1, float(rb.median()) + 1]})
    print(json.dumps(line), flush=True)
    return line


def compare_vunit(name, a, b, off, args, extra):
    """ops.rank_grouped_vunit against ops.rank_grouped on the same tensors, alternating."""
    lib = L.lib()
    n, m = a.shape[0], b.shape[0]
    wv = ops.workspace(lib.vtc_l2_rank_grouped_vunit_workspace_bytes(n, m, args.d, 0, 0), a.device)
    wg = ops.workspace(lib.vtc_l2_rank_grouped_workspace_bytes(n, m, args.d, 0, 0), a.device)
    fv = lambda: ops.rank_grouped_vunit(a, b, off, ws=wv)                                                          # noqa: E731
    fg = lambda: ops.rank_grouped(a, b, off, ws=wg)                                                                # noqa: E731
    for _ in range(args.warmup):
        fv()
        fg()
    tv, tg = [], []
    for _ in range(args.iters):
        tv.append(timed(fv))
        tg.append(timed(fg))
    ra, rb, rv, bits = fv()
    ga, gb, _ = fg()
    st = ops.rank_sweep_stats(wv)
    line = dict(extra, case=name + "_vunit", d=args.d, iters=args.iters, rank_grouped_vunit_ms=ms(tv), rank_grouped_ms=ms(tg),
                ratio=round(float(np.median(tv)) / float(np.median(tg)), 3), grouped_spread_max_over_min=round(max(tg) / min(tg), 3),
                rank_a_b_equal_to_rank_grouped=bool(torch.equal(ra, ga) and torch.equal(rb, gb)),
                rank_v_le_rank_b=bool((rv <= rb).all()), videos_where_conventions_differ=int((rv != rb).sum()),
                vunit={"in_reach_per_video_mean": round(st["vunit_in_reach"] / n, 2), "in_reach_per_video_max": st["vunit_in_reach_max"],
                       "brute_force_videos": st["vunit_brute_force_owners"], "kernel_split_ms": kernel_split(fv)},
                grouped_kernel_split_ms=kernel_split(fg), nonfinite_bits=int(bits.item()),
                **{"R@1": [round(float((rb < 1).float().mean()), 4), round(float((rv < 1).float().mean()), 4)],
                   "median_rank_1based_caption_vs_video": [float(rb.median()) + 1, float(rv.median()) + 1]})
    print(json.dumps(line), flush=True)
    return line


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--identity", type=int, default=10000, help="rows of the identity-offsets comparison (0: skip)")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    lib = L.lib()
    lines = []
    shapes = [("msrvtt_full_2990x20", np.full(2990, 20, np.int64)),
              ("msvd_670x~41", np.random.default_rng(670).integers(31, 52, 670).astype(np.int64))]
    for name, counts in shapes:
        a, b, off = make_grouped(counts, args.d, 1000 + len(counts))
        n, m = a.shape[0], b.shape[0]
        sq = int(round(np.sqrt(float(n) * m)))
        pa, pb = make("spread", sq, args.d, 1000 + sq)
        wg = ops.workspace(lib.vtc_l2_rank_grouped_workspace_bytes(n, m, args.d, 0, 0), a.device)
        wp = ops.workspace(lib.vtc_l2_rank_bidir_workspace_bytes(sq, args.d, 0, 0), a.device)
        lines.append(compare(name, (lambda: ops.rank_grouped(a, b, off, ws=wg), wg, (m, n)),
                             (lambda: ops.rank_bidir(pa, pb, ws=wp), wp, (sq, sq)), args,
                             {"n": n, "m": m, "captions_per_video": [int(counts.min()), int(counts.max())], "paired_n": sq}))
        del wg, wp, pa, pb
        lines.append(compare_vunit(name, a, b, off, args, {"n": n, "m": m, "captions_per_video": [int(counts.min()), int(counts.max())]}))
        del a, b
        torch.cuda.empty_cache()
    if args.identity:
        n = args.identity
        a, b = make("spread", n, args.d, 1000 + n)
        off = np.arange(n + 1)
        wg = ops.workspace(lib.vtc_l2_rank_grouped_workspace_bytes(n, n, args.d, 0, 0), a.device)
        wp = ops.workspace(lib.vtc_l2_rank_bidir_workspace_bytes(n, args.d, 0, 0), a.device)
        line = compare("identity_offsets", (lambda: ops.rank_grouped(a, b, off, ws=wg), wg, (n, n)),
                       (lambda: ops.rank_bidir(a, b, ws=wp), wp, (n, n)), args, {"n": n, "m": n, "paired_n": n})
        ga, gb, _ = ops.rank_grouped(a, b, off, ws=wg)
        qa, qb, _ = ops.rank_bidir(a, b, ws=wp)
        line["equal_to_rank_bidir"] = bool(torch.equal(ga, qa) and torch.equal(gb, qb))
        print(json.dumps({"case": "identity_offsets", "equal_to_rank_bidir": line["equal_to_rank_bidir"]}), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
