"""Query-time search (ops.l2_search = vtc_l2_search) against the route it replaces for few queries (ops.l2_topk, EXACT = vtc_l2_topk):

    python tools/search_bench.py [--galleries 100000,1000000] [--queries 1,4,8,16,32,64] [--d 512] [--depth 11] [--calls 30] [--out FILE]

Per (n_gallery, n_queries) one JSON line:
  search_us / topk_us   one call each between a pair of HIP events, the two entries taken in ALTERNATION in the same run (so drift of the
                        box hits both), after --warmup calls of each; median / min / max over --calls calls
  topk_over_search      ratio of the medians; `faster` names the entry whose median is lower by MORE THAN 5 % (the +-3 % box-to-box spread
                        this project records, with margin), else "neither"
  gallery_tb_per_s      n_gallery * d * 4 bytes over the search's median: the gallery read ONCE, whatever the number of passes (`passes`,
                        ceil(Q / 8) above four queries) -- against the 6.0 - 6.3 TB/s streaming read of an MI355X
  same_ids              the two entries returned the same ids (asserted)
Unit rows from a seeded generator on the device, queries = gallery rows plus noise (a retrieval query has near neighbours).  One process
on an otherwise idle card.  profiles/search.md holds a run's table; VideoIndex.ROUTE_TOPK_MIN_QUERIES cites it."""
import argparse
import json
import os
import sys

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


def passes(nq):
    return 1 if nq <= 4 else -(-nq // 8)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--galleries", type=str, default="100000,1000000")
    ap.add_argument("--queries", type=str, default="1,4,8,16,32,64")
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--depth", type=int, default=11)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    assert args.calls >= 30, "at least 30 timed calls per entry"
    lib = L.lib()
    gen = torch.Generator(device="cuda").manual_seed(5)
    lines = []
    for ng in [int(x) for x in args.galleries.split(",")]:
        gallery = ops.normalize_rows(torch.randn(ng, args.d, device="cuda", generator=gen))
        for nq in [int(x) for x in args.queries.split(",")]:
            pick = torch.randint(0, ng, (nq,), device="cuda", generator=gen)
            queries = ops.normalize_rows(gallery[pick] + 0.5 * ops.normalize_rows(torch.randn(nq, args.d, device="cuda", generator=gen)))
            ws_s = ops.workspace(lib.vtc_l2_search_workspace_bytes(ng, nq, args.d, args.depth), gallery.device)
            ws_t = ops.workspace(lib.vtc_l2_topk_workspace_bytes(ng, nq, args.d, L.SWEEP_EXACT, 0), gallery.device)
            search = lambda: ops.l2_search(gallery, queries, args.depth, ws=ws_s)                                  # noqa: E731
            topk = lambda: ops.l2_topk(gallery, queries, args.depth, precision=L.SWEEP_EXACT, ws=ws_t)             # noqa: E731
            for _ in range(args.warmup):
                search()
                topk()
            torch.cuda.synchronize()
            t_s, t_t = [], []
            for _ in range(args.calls):
                us, (ids_s, dists_s, _) = timed(search)
                t_s.append(us)
                us, (ids_t, dists_t) = timed(topk)
                t_t.append(us)
            same = bool(torch.equal(ids_s, ids_t))
            s, t = stat(t_s), stat(t_t)
            ratio = t["median"] / s["median"]
            line = {"n_gallery": ng, "n_queries": nq, "d": args.d, "depth": args.depth, "calls": args.calls, "search_us": s, "topk_us": t,
                    "topk_over_search": round(ratio, 3), "faster": "search" if ratio > 1.05 else ("topk" if ratio < 1 / 1.05 else "neither"),
                    "passes": passes(nq), "gallery_tb_per_s": round(ng * args.d * 4 / (1e6 * s["median"]), 3),
                    "same_ids": same, "same_dists": bool(torch.equal(dists_s, dists_t)),
                    "workspace_mb": {"search": round(ws_s.numel() / 2 ** 20, 1), "topk": round(ws_t.numel() / 2 ** 20, 1)}}
            print(json.dumps(line), flush=True)
            lines.append(line)
            assert same, "vtc_l2_search and vtc_l2_topk(EXACT) returned different ids"
            del ws_s, ws_t
        del gallery
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
