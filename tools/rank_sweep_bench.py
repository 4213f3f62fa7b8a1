"""The full-rank sweep (ops.rank_bidir) against its yardstick, the BF16X3 two-direction top-k at the same size, alternating in ONE process:

    python tools/rank_sweep_bench.py [--n 10000 50000] [--d 512] [--iters 20] [--warmup 3] [--shards G] [--out FILE]

One JSON line per (size, data set): both times (HIP events around each call, median / min / max over the timed iterations), the pairs in
reach of their target per owner (mean and max, per direction), the owners that went to the fp64 brute force, and the per-kernel split of one
rank sweep from the library's own launch records (vtc_prof_begin / vtc_prof_end_records; tags 101 .. 105 = prologue, row count, column
count, settle, brute force; the GEMM launches carry their epilogue mode).  Data: the log-uniform-noise pairs of tests/rank_refs.py ("spread":
ranks from 0 to nearly n) and unrelated sets (every target inside the bulk of its row).  profiles/r10_rank_sweep.md holds a run's output.
--shards G adds the rank-sharded form (ops.rank_shard) on the same data, in the same alternation: the call of rank 0 of G (its shard_bounds
window), the G windows one after another on this one card (the simulated total: what the G ranks do between them), and the kernel split of
rank 0's call.  profiles/rank_shard.md holds a run's output."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vtc_amd import _lib as L  # noqa: E402
from vtc_amd import ops  # noqa: E402

STAGES = {101: "prologue", 102: "row_count", 103: "col_count", 104: "settle", 105: "brute_force", 106: "vunit_count", 107: "vunit_finish"}


def unit(x):
    return x / torch.linalg.norm(x, dim=-1, keepdim=True)


def make(kind, n, d, seed):
    """The generators of tests/rank_refs.py, on the GPU (fp64 draws, fp32 rows)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = unit(torch.randn(n, d, generator=g, device="cuda", dtype=torch.float64))
    noise = unit(torch.randn(n, d, generator=g, device="cuda", dtype=torch.float64))
    if kind == "unrelated":
        return a.float().contiguous(), noise.float().contiguous()
    s = torch.exp(torch.rand(n, 1, generator=g, device="cuda", dtype=torch.float64) * (np.log(60.0) - np.log(0.5)) + np.log(0.5))
    return a.float().contiguous(), unit(a + s * noise).float().contiguous()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel_split(fn, max_rec=4096):
    lib = L.lib()
    lib.vtc_prof_begin()
    fn()
    n = C.c_int(0)
    cls, reg, tag = (C.c_int * max_rec)(), (C.c_int * max_rec)(), (C.c_int * (3 * max_rec))()
    ms, work = (C.c_double * max_rec)(), (C.c_double * max_rec)()
    L.check(lib.vtc_prof_end_records(ops._stream(), max_rec, C.byref(n), cls, reg, ms, work, tag), "vtc_prof_end_records")
    out = {}
    for i in range(n.value):
        name = STAGES.get(tag[3 * i], "gemm" if L.PROF_CLASSES[cls[i]].startswith("gemm") else f"other_{tag[3 * i]}")
        out[name] = round(out.get(name, 0.0) + ms[i], 4)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10000, 50000])
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kinds", nargs="+", default=["spread", "unrelated"])
    ap.add_argument("--shards", type=int, default=0, help="G > 1: also time ops.rank_shard for rank 0 of G and for all G windows in turn")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    lib = L.lib()
    lines = []
    for n in args.n:
        for kind in args.kinds:
            a, b = make(kind, n, args.d, 1000 + n)
            ws_rank = ops.workspace(lib.vtc_l2_rank_bidir_workspace_bytes(n, args.d, 0, 0), a.device)
            ws_topk = ops.workspace(lib.vtc_l2_topk_bidir_workspace_bytes(n, n, args.d, L.SWEEP_BF16X3, 0), a.device)
            rank = lambda: ops.rank_bidir(a, b, ws=ws_rank)                                                                  # noqa: E731
            topk = lambda: ops.l2_topk_bidir(a, b, 11, precision=L.SWEEP_BF16X3, return_dists=False, ws=ws_topk)            # noqa: E731
            shard0 = shard_all = None
            if args.shards > 1:
                from vtc_amd.dist import shard_bounds
                wins = [shard_bounds(n, r, args.shards) for r in range(args.shards)]
                ws_shard = ops.workspace(max(lib.vtc_l2_rank_shard_workspace_bytes(n, hi - lo, args.d, 0, 0) for lo, hi in wins), a.device)
                shard0 = lambda: ops.rank_shard(a, b, wins[0][0], wins[0][1] - wins[0][0], ws=ws_shard)                       # noqa: E731
                shard_all = lambda: [ops.rank_shard(a, b, lo, hi - lo, ws=ws_shard) for lo, hi in wins]                      # noqa: E731
            for _ in range(args.warmup):
                rank()
                topk()
                if shard0:
                    shard0()
                    shard_all()
            t_rank, t_topk, t_shard0, t_shard_all = [], [], [], []
            for _ in range(args.iters):                      # alternating: all see the same box at the same time
                t_rank.append(timed(rank))
                t_topk.append(timed(topk))
                if shard0:
                    t_shard0.append(timed(shard0))
                    t_shard_all.append(timed(shard_all))
            ra, rb, bits = rank()
            st = ops.rank_sweep_stats(ws_rank)
            split = kernel_split(rank)
            split_topk = kernel_split(topk)                  # the yardstick's own split: its GEMM and its list kernels ("other_0")
            med = lambda t: float(np.median(t))                                                                              # noqa: E731
            line = {"n": n, "d": args.d, "data": kind, "iters": args.iters,
                    "rank_bidir_ms": {"median": round(med(t_rank), 4), "min": round(min(t_rank), 4), "max": round(max(t_rank), 4)},
                    "topk_bidir_bf16x3_depth11_ms": {"median": round(med(t_topk), 4), "min": round(min(t_topk), 4), "max": round(max(t_topk), 4)},
                    "ratio": round(med(t_rank) / med(t_topk), 3),
                    "in_reach_per_owner_mean": [round(x / n, 2) for x in st["in_reach"]], "in_reach_per_owner_max": list(st["in_reach_max"]),
                    "in_reach_fraction_of_gallery": [round(x / n / n, 6) for x in st["in_reach"]],
                    "brute_force_owners": list(st["brute_force_owners"]),
                    "kernel_split_ms": split, "topk_kernel_split_ms": {("list_kernels" if k.startswith("other") else k): v for k, v in split_topk.items()},
                    "nonfinite_bits": int(bits.item()),
                    "R@1": [round(float((ra < 1).float().mean()), 4), round(float((rb < 1).float().mean()), 4)],
                    "median_rank_1based": [float(ra.median()) + 1, float(rb.median()) + 1]}
            if shard0:
                parts = shard_all()
                assert torch.equal(torch.cat([p[0] for p in parts]), ra) and torch.equal(sum(p[1] for p in parts), rb)      # the windows' results ARE the paired call's
                shard0()
                st0 = ops.rank_sweep_stats(ws_shard)
                ms = lambda t: {"median": round(med(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}               # noqa: E731
                line.update({"shards": args.shards, "rank_shard_rank0_ms": ms(t_shard0), "rank_shard_all_windows_ms": ms(t_shard_all),
                             "shard_rank0_over_paired": round(med(t_shard0) / med(t_rank), 3),
                             "all_windows_over_paired": round(med(t_shard_all) / med(t_rank), 3),
                             "shard_rank0_kernel_split_ms": kernel_split(shard0), "shard_rank0_in_reach": list(st0["in_reach"]),
                             "shard_rank0_workspace_MiB": round(lib.vtc_l2_rank_shard_workspace_bytes(n, wins[0][1] - wins[0][0], args.d, 0, 0) / 2 ** 20, 1),
                             "paired_workspace_MiB": round(lib.vtc_l2_rank_bidir_workspace_bytes(n, args.d, 0, 0) / 2 ** 20, 1)})
                del ws_shard
            print(json.dumps(line), flush=True)
            lines.append(line)
            del ws_rank, ws_topk, a, b
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
