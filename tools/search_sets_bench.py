"""Set queries (ops.l2_search_sets = vtc_l2_search_sets) against the same vectors searched as separate queries:

    python tools/search_sets_bench.py [--galleries 100000,1000000] [--members 1,2,4,8,16,64] [--d 512] [--depth 11] [--calls 30]
                                      [--rows-per-video 5] [--baseline-lib OTHER/libvtc_hip.so] [--out FILE]

Per (n_gallery, storage float32 / float16, ungrouped / grouped, members m) one JSON line:
  set_us / separate_us     ONE set of m members, and ops.l2_search (grouped: ops.l2_search_grouped at --rows-per-video rows a video) of the
                           same m vectors as m separate queries over the same gallery -- what an application that merges on the host
                           pays before its merge.  One call each between a pair of HIP events, the entries taken in ALTERNATION in the
                           same run, after --warmup calls of each; median / min / max over --calls calls.  With --baseline-lib the
                           separate queries run in ANOTHER build of the library (the parent commit), bound for the call
  set_over_separate        ratio of the medians.  The expectation: not above 1 by more than `aa_spread`
  aa_spread                the separate queries are in the alternation TWICE (separate_us, separate_again_us): max / min of the two medians
                           - 1, what two runs of the same code differ by in this session
  same_ids_as_host         the set's ids equal the m separate lists merged on the host by (fp64 distance, row), a row (video) once
                           (asserted; outside the timing)
With --baseline-lib, per (n_gallery, storage, entry, n_queries in 1, 8) one more line: NAME_us and NAME_baseline_us, the non-set entry
(ops.l2_search, l2_search(live=) with every row live, l2_search_grouped, the excluding scans) in this build and in the other, with
NAME_over_baseline and the A/A spread of the baseline against itself -- their kernels are unchanged and must time the same.
And per n_gallery of at most 10^5 rows: similar_to_video_us, VideoIndex.similar_to_video of ONE video of 9 rows, k = --depth, end to end
on the host clock (its host sync included), and search_videos_us, search_videos of ONE query, only enqueued, then synchronised.
Unit rows from a seeded generator on the device, members = gallery rows plus noise.  One process on an otherwise idle card.
profiles/search_sets.md holds a run's table."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vtc_amd import _lib as L  # noqa: E402
from vtc_amd import ops  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b), out


def stat(us):
    return {"median": round(float(np.median(us)), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def alternate(entries, warmup, calls):
    """{name: [us]} of the entries taken in alternation."""
    for _ in range(warmup):
        for fn in entries.values():
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name in entries}
    for _ in range(calls):
        for name, fn in entries.items():
            us[name].append(timed(fn)[0])
    return us


def other_build(path):
    base = C.CDLL(os.path.abspath(path))
    for name, (res, argtypes) in L.SIGNATURES.items():        # the entries the other build has, with this tree's signatures
        if hasattr(base, name):
            getattr(base, name).restype, getattr(base, name).argtypes = res, argtypes
    return base


def bound_to(base, fn):
    """fn with the library calls of vtc_amd.ops going to another build for the call."""
    if base is None:
        return fn

    def call():
        mine, L._lib = L._lib, base
        try:
            return fn()
        finally:
            L._lib = mine
    return call


def host_merge(ids, d64, groups, depth):
    """The m separate lists [m, depth] merged on the host: by (fp64 distance, row), every row -- grouped: every video -- once."""
    ids, d64 = ids.reshape(-1).cpu().numpy(), d64.reshape(-1).cpu().numpy()
    out, seen = [], set()
    for o in np.lexsort((ids, d64)):
        if ids[o] < 0:
            continue
        key = int(ids[o]) if groups is None else int(groups[ids[o]])
        if key not in seen:
            seen.add(key)
            out.append(int(ids[o]))
    return out[:depth]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--galleries", default="100000,1000000")
    ap.add_argument("--members", default="1,2,4,8,16,64")
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--depth", type=int, default=11)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows-per-video", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    lib = L.lib()
    base = other_build(args.baseline_lib) if args.baseline_lib else None
    gen = torch.Generator(device="cuda").manual_seed(5)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    for ng in [int(x) for x in args.galleries.split(",")]:
        rows32 = ops.normalize_rows(torch.randn(ng, args.d, device="cuda", generator=gen))
        videos = (torch.arange(ng, device="cuda") // args.rows_per_video).to(torch.int32)
        videos_host = videos.cpu().numpy()
        for storage in ("float32", "float16"):
            gallery = rows32 if storage == "float32" else rows32.half()
            for grouped in (False, True):
                groups = videos if grouped else None
                for m in [int(x) for x in args.members.split(",")]:
                    pick = torch.randint(0, ng, (m,), device="cuda", generator=gen)
                    members = ops.normalize_rows(rows32[pick] + 0.5 * ops.normalize_rows(torch.randn(m, args.d, device="cuda", generator=gen)))
                    sets = members[None].contiguous()
                    ws_set = ops.workspace(lib.vtc_l2_search_sets_workspace_bytes(ng, 1, m, args.d, args.depth, int(grouped)), "cuda")
                    ws_sep = [ops.workspace(lib.vtc_l2_search_grouped_workspace_bytes(ng, m, args.d, args.depth), "cuda") for _ in range(2)]
                    as_set = lambda: ops.l2_search_sets(gallery, sets, args.depth, groups=groups, ws=ws_set)                       # noqa: E731

                    def separate(ws):
                        if grouped:
                            return lambda: ops.l2_search_grouped(gallery, members, groups, args.depth, ws=ws)
                        return lambda: ops.l2_search(gallery, members, args.depth, ws=ws)
                    us = alternate({"set": as_set, "separate": bound_to(base, separate(ws_sep[0])),
                                    "separate_again": bound_to(base, separate(ws_sep[1]))}, args.warmup, args.calls)
                    got = as_set()[0][0].tolist()
                    sep = bound_to(base, separate(ws_sep[0]))()
                    want = host_merge(sep[0], ops.search_dists64(ws_sep[0], m, args.depth), videos_host if grouped else None, args.depth)
                    assert got == want, (ng, storage, grouped, m, got, want)
                    med = {k: float(np.median(v)) for k, v in us.items()}
                    emit({"n_gallery": ng, "storage": storage, "grouped": grouped, "members": m, "d": args.d, "depth": args.depth,
                          "set_us": stat(us["set"]), "separate_us": stat(us["separate"]), "separate_again_us": stat(us["separate_again"]),
                          "set_over_separate": round(med["set"] / min(med["separate"], med["separate_again"]), 4),
                          "aa_spread": round(max(med["separate"], med["separate_again"]) / min(med["separate"], med["separate_again"]) - 1, 4),
                          "separate_in": "baseline" if base is not None else "this build", "same_ids_as_host": True})
            if base is not None:                               # the entries that were there before: this build against the other
                live = ops.row_mask_pack(torch.ones(ng, dtype=torch.uint8, device="cuda"))
                for nq in (1, 8):
                    pick = torch.randint(0, ng, (nq,), device="cuda", generator=gen)
                    q = ops.normalize_rows(rows32[pick] + 0.5 * ops.normalize_rows(torch.randn(nq, args.d, device="cuda", generator=gen)))
                    own = ops.l2_search(gallery, q, 1)[0][:, 0].contiguous()
                    own_video = videos[own].to(torch.int64)
                    need = lib.vtc_l2_search_grouped_workspace_bytes(ng, nq, args.d, args.depth)
                    calls = {"search": lambda ws: ops.l2_search(gallery, q, args.depth, ws=ws),
                             "search_live": lambda ws: ops.l2_search(gallery, q, args.depth, ws=ws, live=live),
                             "search_grouped": lambda ws: ops.l2_search_grouped(gallery, q, videos, args.depth, ws=ws),
                             "search_excluding": lambda ws: ops.l2_search(gallery, q, args.depth, ws=ws, exclude=own),
                             "search_grouped_excluding": lambda ws: ops.l2_search_grouped(gallery, q, videos, args.depth, ws=ws, exclude=own_video)}
                    for name, call in calls.items():
                        ws3 = [ops.workspace(need, "cuda") for _ in range(3)]
                        us = alternate({"new": lambda: call(ws3[0]), "base": bound_to(base, lambda: call(ws3[1])),
                                        "base_again": bound_to(base, lambda: call(ws3[2]))}, args.warmup, args.calls)
                        same = all(torch.equal(x, y) for x, y in zip(call(ws3[0])[:2], bound_to(base, lambda: call(ws3[1]))()[:2]))
                        assert same, (ng, storage, name, nq)
                        med = {k: float(np.median(v)) for k, v in us.items()}
                        emit({"n_gallery": ng, "storage": storage, "entry": name, "n_queries": nq, name + "_us": stat(us["new"]),
                              name + "_baseline_us": stat(us["base"]), name + "_over_baseline": round(med["new"] / min(med["base"], med["base_again"]), 4),
                              "aa_spread": round(max(med["base"], med["base_again"]) / min(med["base"], med["base_again"]) - 1, 4), "same_bits": True})
        if ng <= 100000:                                       # end to end on the host clock: the one host sync included
            from vtc_amd.host.search import VideoIndex
            n9 = ng - ng % 9
            index = VideoIndex(args.d, normalized=True)
            index.add(rows32[:n9], video_ids=torch.arange(n9, device="cuda") // 9)
            one = rows32[:1].contiguous()

            def wall(fn):
                out = []
                for _ in range(args.warmup + args.calls):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    out.append(1e6 * (time.perf_counter() - t0))
                return out[args.warmup:]
            emit({"n_gallery": n9, "rows_of_the_video": 9, "k": args.depth,
                  "similar_to_video_us": stat(wall(lambda: index.similar_to_video([n9 // 18], args.depth))),
                  "search_videos_any_us": stat(wall(lambda: index.search_videos_any(rows32[None, :9], args.depth))),
                  "search_videos_us": stat(wall(lambda: index.search_videos(one, args.depth)))})
            del index
        del rows32, gallery
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return lines


if __name__ == "__main__":
    main()
