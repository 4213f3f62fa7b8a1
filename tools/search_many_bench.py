"""The many-query search of a half gallery (ops.l2_search_many = vtc_l2_search_many_half) against the scan over the same half gallery
(ops.l2_search = vtc_l2_search_half), the only route a half gallery had:

    python tools/search_many_bench.py [--galleries 100000,1000000] [--queries 8,12,16,32,64] [--live 1.0,0.5] [--d 512] [--depth 11]
                                      [--calls 30] [--warmup 5] [--out FILE]

The protocol of tools/search_bench.py (profiles/search.md): per (n_gallery, n_queries, live fraction) one JSON line with
  many_us / scan_us     one call each between a pair of HIP events, the two entries taken in ALTERNATION in the same run, after --warmup
                        calls of each; median / min / max over --calls calls
  scan_over_many        ratio of the medians; `faster` names the entry whose median is lower by MORE THAN 5 %, else "neither"
  gallery_tb_per_s      n_gallery * d * 2 bytes over the new entry's median: the gallery read once
  fallback_queries      of the new entry's last call (ops.search_many_stats): 0 means every list was certified
  workspace_bytes       of the new entry and of the scan
  same_bits             ids, fp32 dists and the fp64 heads of the two are equal (asserted)
  outputs_sha1          SHA-1 over the new entry's ids, fp32 dists, non-finite word and fp64 head of its last call: equal between two
                        builds of the library (VTC_HIP_LIB) that compute the same
Unit rows from a seeded generator on the device rounded to half, queries = gallery rows plus noise.  A live fraction below 1 draws every
row's bit independently.  One process on an otherwise idle card.  profiles/search_many.md holds a run's table;
VideoIndex.ROUTE_MANY_MIN_QUERIES cites it."""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, stream):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    fn()
    stop.record(stream)
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--galleries", default="100000,1000000")
    ap.add_argument("--queries", default="8,12,16,32,64")
    ap.add_argument("--live", default="1.0,0.5")
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--depth", type=int, default=11)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vtc_amd import ops
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    out = open(args.out, "w") if args.out else None
    for ng in (int(x) for x in args.galleries.split(",")):
        gen = torch.Generator(device=dev).manual_seed(1234 + ng)
        g32 = torch.nn.functional.normalize(torch.randn(ng, args.d, device=dev, generator=gen), dim=1)
        g = g32.to(torch.float16)
        for frac in (float(x) for x in args.live.split(",")):
            words = None if frac >= 1.0 else ops.row_mask_pack(torch.rand(ng, device=dev, generator=gen) < frac)
            for nq in (int(x) for x in args.queries.split(",")):
                pick = torch.randint(0, ng, (nq,), device=dev, generator=gen)
                q = torch.nn.functional.normalize(g32[pick] + 0.3 * torch.randn(nq, args.d, device=dev, generator=gen) / args.d ** 0.5, dim=1)
                ws_many = ops.workspace(ops.l2_search_many_workspace_bytes(ng, nq, args.d, args.depth), dev)
                ws_scan = ops.workspace(ops.l2_search_workspace_bytes(ng, nq, args.d, args.depth), dev)
                many = lambda: ops.l2_search_many(g, q, args.depth, live=words, ws=ws_many)
                scan = lambda: ops.l2_search(g, q, args.depth, live=words, ws=ws_scan)
                for _ in range(args.warmup):
                    many()
                    scan()
                torch.cuda.synchronize(dev)
                t_many, t_scan = [], []
                for _ in range(args.calls):
                    t_many.append(timed(many, stream))
                    t_scan.append(timed(scan, stream))
                a, b = many(), scan()
                same = (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and
                        torch.equal(ops.search_dists64(ws_many, nq, args.depth), ops.search_dists64(ws_scan, nq, args.depth)))
                assert same, (ng, nq, frac)
                sha = hashlib.sha1()
                for t in (*a, ops.search_dists64(ws_many, nq, args.depth)):
                    sha.update(t.cpu().numpy().tobytes())
                m_many, m_scan = statistics.median(t_many), statistics.median(t_scan)
                line = dict(n_gallery=ng, n_queries=nq, d=args.d, depth=args.depth, live=frac,
                            many_us=dict(median=round(m_many, 1), min=round(min(t_many), 1), max=round(max(t_many), 1)),
                            scan_us=dict(median=round(m_scan, 1), min=round(min(t_scan), 1), max=round(max(t_scan), 1)),
                            scan_over_many=round(m_scan / m_many, 3),
                            faster="many" if m_many < 0.95 * m_scan else ("scan" if m_scan < 0.95 * m_many else "neither"),
                            gallery_tb_per_s=round(ng * args.d * 2 / m_many / 1e6, 3),
                            fallback_queries=ops.search_many_stats(ws_many, nq, args.depth)["fallback_queries"],
                            workspace_bytes=dict(many=ws_many.numel(), scan=ws_scan.numel()), same_bits=same, outputs_sha1=sha.hexdigest())
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n")
                    out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
