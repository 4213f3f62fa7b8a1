"""The many-query count pass of the range search over a half gallery (ops.l2_range_count_many = vtc_l2_range_count_many_half) against the
scan's count pass over the same half gallery (ops.l2_range_count = vtc_l2_range_count), which this tool never replaces as the comparator:

    python tools/range_many_bench.py [--galleries 100000,1000000] [--queries 8,9,12,16,32,64] [--live 1.0,0.5] [--hits 10,0.01]
                                     [--d 512] [--calls 30] [--warmup 5] [--step-timeout 300] [--out FILE]
    python tools/range_many_bench.py --near-duplicates 100000 [--d 512] [--step-timeout 300] [--out FILE]

The protocol of tools/search_many_bench.py (profiles/search_many.md): per (n_gallery, live fraction, radius, n_queries) one JSON line with
  many_us / scan_us     one call each between a pair of HIP events, the entries taken in ALTERNATION in the same run, after --warmup calls
                        of each; median / min / max over --calls calls
  search_many_us        ops.l2_search_many at depth 11 on the same gallery, queries and mask, in the same alternation: the pass that
                        keeps lists, for comparison
  scan_over_many        ratio of the medians; `faster` names the entry whose median is lower by MORE THAN 5 %, else "neither"
  hits_per_query        mean over the queries of the call
  exact_pairs           of the new entry's last call (ops.range_many_stats): the pairs the error bound could not decide
  same_bits             lims, the hit words and the non-finite word of the two are equal (asserted)
  outputs_sha1          SHA-1 over the new entry's lims, non-finite word and hit words of its last call: equal between two builds of the
                        library (VTC_HIP_LIB) that compute the same
--hits: a value >= 1 is a number of rows, below 1 a fraction of the live rows; the radius of a query is the midpoint between its
distances at that rank and the next (fp32 distances, good enough to choose a radius).  Unit rows from a seeded generator on the device
rounded to half, queries = gallery rows plus noise.  A live fraction below 1 draws every row's bit independently.
--near-duplicates N: the wall time of VideoIndex.near_duplicates(0.9) over a half index of N such rows with 1 % of the rows in planted
near-copies, once through the new entry and once through the scan (the routing constant set on the instance), and that the two agree.
Every step -- one (n_gallery, live fraction), or the near-duplicates run -- is a child process under its own --step-timeout; the parent
never opens the GPU and stops at the first step that fails.  One process at a time on an otherwise idle card.  profiles/range_many.md
holds a run's table; VideoIndex.ROUTE_RANGE_MANY_MIN_QUERIES cites it."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, stream):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(stream)
    fn()
    stop.record(stream)
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3


def emit(line, out):
    print(json.dumps(line), flush=True)
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")


def step(args, ng, frac):
    """One (n_gallery, live fraction): every radius and query count of it."""
    import torch
    from vtc_amd import ops
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    d, depth = args.d, 11
    gen = torch.Generator(device=dev).manual_seed(1234 + ng)
    g32 = torch.nn.functional.normalize(torch.randn(ng, d, device=dev, generator=gen), dim=1)
    g = g32.to(torch.float16)
    live = None if frac >= 1.0 else torch.rand(ng, device=dev, generator=gen) < frac
    words = None if live is None else ops.row_mask_pack(live)
    n_live = ng if live is None else int(live.sum())
    nq_max = max(int(x) for x in args.queries.split(","))
    pick = torch.randint(0, ng, (nq_max,), device=dev, generator=gen)
    q_all = torch.nn.functional.normalize(g32[pick] + 0.3 * torch.randn(nq_max, d, device=dev, generator=gen) / d ** 0.5, dim=1)
    dist = 2.0 - 2.0 * (q_all @ g.float().T)                    # fp32: only chooses the radii
    if live is not None:
        dist[:, ~live] = float("inf")
    for hits in (float(x) for x in args.hits.split(",")):
        rank = int(hits) if hits >= 1 else max(1, int(hits * n_live))
        low = torch.topk(dist, rank + 1, dim=1, largest=False, sorted=True).values
        r2_all = ((low[:, rank - 1] + low[:, rank]) / 2).double()
        for nq in (int(x) for x in args.queries.split(",")):
            q, r2 = q_all[:nq].contiguous(), r2_all[:nq].contiguous()
            ws_many = ops.workspace(ops.l2_range_many_workspace_bytes(ng, nq, d), dev)
            ws_scan = ops.workspace(ops.l2_range_workspace_bytes(ng, nq, d), dev)
            ws_topk = ops.workspace(ops.l2_search_many_workspace_bytes(ng, nq, d, depth), dev)
            many = lambda: ops.l2_range_count_many(g, q, r2, live=words, ws=ws_many, return_bits=True)
            scan = lambda: ops.l2_range_count(g, q, r2, live=words, ws=ws_scan, return_bits=True)
            topk = lambda: ops.l2_search_many(g, q, depth, live=words, ws=ws_topk)
            for _ in range(args.warmup):
                many()
                scan()
                topk()
            torch.cuda.synchronize(dev)
            t_many, t_scan, t_topk = [], [], []
            for _ in range(args.calls):
                t_many.append(timed(many, stream))
                t_scan.append(timed(scan, stream))
                t_topk.append(timed(topk, stream))
            a, b = many(), scan()
            same = (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and
                    torch.equal(ops.range_hit_words(ws_many, ng, nq), ops.range_hit_words(ws_scan, ng, nq)))
            assert same, (ng, nq, frac, hits)
            sha = hashlib.sha1()
            for t in (*a, ops.range_hit_words(ws_many, ng, nq)):
                sha.update(t.cpu().numpy().tobytes())
            m_many, m_scan, m_topk = statistics.median(t_many), statistics.median(t_scan), statistics.median(t_topk)
            spread = lambda t, m: dict(median=round(m, 1), min=round(min(t), 1), max=round(max(t), 1))
            emit(dict(n_gallery=ng, n_queries=nq, d=d, live=frac, hits=hits, hits_per_query=round(float(a[0][-1]) / nq, 1),
                      many_us=spread(t_many, m_many), scan_us=spread(t_scan, m_scan), search_many_us=spread(t_topk, m_topk),
                      scan_over_many=round(m_scan / m_many, 3), search_many_over_many=round(m_topk / m_many, 3),
                      faster="many" if m_many < 0.95 * m_scan else ("scan" if m_scan < 0.95 * m_many else "neither"),
                      gallery_tb_per_s=round(ng * d * 2 / m_many / 1e6, 3),
                      exact_pairs=ops.range_many_stats(ws_many, ng, nq, d)["exact_pairs"],
                      workspace_bytes=dict(many=ws_many.numel(), scan=ws_scan.numel()), same_bits=same, outputs_sha1=sha.hexdigest()), args.out)


def near_duplicates(args, n):
    import torch
    from vtc_amd.host.search import VideoIndex
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(99 + n)
    rows = torch.randn(n, args.d, device=dev, generator=gen)
    k = max(1, n // 200)                                        # 1 % of the rows are a planted pair's
    perm = torch.randperm(n, device=dev, generator=gen)
    rows[perm[k:2 * k]] = rows[perm[:k]] + 0.02 * torch.randn(k, args.d, device=dev, generator=gen)
    index = VideoIndex(args.d, device=dev, storage=torch.float16)
    index.add(rows)
    line, found = dict(near_duplicates_rows=n, d=args.d, min_score=0.9), {}
    for route, least in (("many", 9), ("scan", 65)):
        index.ROUTE_RANGE_MANY_MIN_QUERIES = least
        index.near_duplicates(0.9, subset=index.subset(torch.arange(0, min(n, 4096), device=dev)))      # warm: workspace, code objects
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        found[route] = index.near_duplicates(0.9)
        torch.cuda.synchronize(dev)
        line[route + "_wall_s"] = round(time.perf_counter() - t0, 3)
    assert all(torch.equal(x, y) for x, y in zip(found["many"], found["scan"]))
    line["pairs"] = int(found["many"][0].shape[0])
    emit(line, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--galleries", default="100000,1000000")
    ap.add_argument("--queries", default="8,9,12,16,32,64")
    ap.add_argument("--live", default="1.0,0.5")
    ap.add_argument("--hits", default="10,0.01")
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--near-duplicates", type=int, default=0)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="internal: GALLERY,LIVE or near-duplicates,N -- the one step a child process runs")
    args = ap.parse_args()
    if args.step:
        what, value = args.step.split(",")
        if what == "near-duplicates":
            near_duplicates(args, int(value))
        else:
            step(args, int(what), float(value))
        return 0
    if args.near_duplicates:
        steps = [f"near-duplicates,{args.near_duplicates}"]
    else:
        steps = [f"{ng},{frac}" for ng in args.galleries.split(",") for frac in args.live.split(",")]
    for s in steps:                                             # a fresh process per step, each under its own time limit
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), *sys.argv[1:], "--step", s], timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"range_many_bench: step {s} ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
