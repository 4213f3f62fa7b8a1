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
on an otherwise idle card.  profiles/search.md holds a run's table; VideoIndex.ROUTE_TOPK_MIN_QUERIES cites it.

With --live the tool measures the MASKED scan (ops.l2_search(live=...) = vtc_l2_search_masked) instead:

    python tools/search_bench.py --live 1.0,0.5,0.1,0.01 [--live-pattern random|blocked] [--topk-gathered] [--queries 1,8] ...

Per (n_gallery, n_queries, live fraction, pattern) one JSON line:
  masked_us / unmasked_us   the masked scan and the UNMASKED ops.l2_search over the same gallery (every row), in alternation as above
  masked_over_unmasked      ratio of the medians; at fraction 1.0 the mask is pure overhead and the ratio should stay within 1.05
  same_ids_as_compacted     the masked ids equal those of the unmasked search over the gallery compacted to its live rows, mapped back
                            (asserted; the compaction is outside the timing)
  topk_gathered_us          with --topk-gathered: gallery[live rows] gathered into a fresh tensor and ops.l2_topk(EXACT) over it, the gather
                            INSIDE the timing -- what routing many masked queries to vtc_l2_topk would cost
`random` draws every row's bit independently; `blocked` makes one contiguous run of rows live (a subreddit whose rows were added
together), starting at an odd row a third of the way in.  profiles/search_masked.md holds a run's table.

With --rows-per-video the tool measures the GROUPED scan (ops.l2_search_grouped = vtc_l2_search_grouped) instead:

    python tools/search_bench.py --rows-per-video 1,5,20 [--video-layout contiguous|scattered] [--queries 1,8] ...

Per (n_gallery, n_queries, rows per video, layout) one JSON line:
  grouped_us / ungrouped_us   the grouped scan and the ungrouped ops.l2_search over the same gallery, in alternation as above
  grouped_over_ungrouped      ratio of the medians; at one row per video the grouping is pure overhead and the ratio should stay within 1.05
  same_ids_as_collapsed       on the first 10^4 rows: the grouped ids equal the COMPLETE (fp64 distance, row) order of the slice, formed
                              outside the library, collapsed to the first row of every video on the host (asserted; outside the timing)
`contiguous` gives rows r * v .. r * v + r - 1 to video v (the captions of a video added together); `scattered` permutes that
assignment over the gallery.  profiles/search_grouped.md holds a run's table.

With --storage float16 the tool measures the scan over a gallery STORED AS IEEE HALF (ops.l2_search* with a torch.float16 gallery =
vtc_l2_search_half) against the fp32 scan, alone or with --live / --rows-per-video (default --storage float32: everything above):

    python tools/search_bench.py --storage float16 [--live 1.0,0.1] [--rows-per-video 5] [--queries 1,2,4,8] ...

Per (n_gallery, n_queries, variant) one JSON line:
  half_us / fp32_us        the scan over the half rows and the fp32 scan over the SAME rows widened to fp32 (the same values, twice the
                           bytes), same mask and groups, in alternation as above
  half_over_fp32           ratio of the medians
  same_bits_as_fp32        ids and fp32 dists of the two are equal (asserted: binary16 -> fp32 is exact)
  same_ids_as_host         on the first 10^4 rows: the half ids equal the complete fp64 (distance, row) order over the widened rows formed
                           outside the library, dead rows dropped, collapsed to the first row of every video (asserted; outside the timing)
  top_depth_agreement      the share of the ids an fp32 index of the UNROUNDED unit rows returns for the same queries (same mask and
                           groups) that the half index returns too: what rounding the stored rows to 11 bits costs
profiles/search_half.md holds a run's table.

With --storage int8 the tool measures the scan over a gallery STORED AS 8-BIT CODES and one scale a row (ops.quantize_rows_q8; ops.l2_search
with a torch.int8 gallery = vtc_l2_search_q8) against the fp32 scan and the half scan of the SAME unit rows, all three in one run:

    python tools/search_bench.py --storage int8 [--queries 1,8,64] ...

Per (n_gallery, n_queries) one JSON line:
  fp32_us / half_us / int8_us   the three scans, in alternation as above; int8_over_fp32 / int8_over_half: ratios of the medians
  *_mb                          the bytes each gallery holds (int8: (d + 16) a row)
  same_bits_as_stored_fp32      ids and fp32 dists of the int8 scan equal the fp32 scan's over the dequantised rows (asserted)
  top10_overlap                 the share of the 10 nearest ids of the fp32 index of the unit rows that the int8 index returns too (half_: the
                                half index's share), averaged over the queries
  max_score_diff                the largest |score over the int8 rows - score over the fp32 rows| among the returned (query, row) pairs,
                                score = 1 - D / 2 with both D in fp64 (half_: the half index's)
profiles/search_q8.md holds a run's table.

With --hits (or --min-score) the tool measures the RANGE search (ops.l2_range_count / vtc_l2_range_fill) against the scan:

    python tools/search_bench.py --hits 100,10000,all [--storage float16] [--queries 1,8,64] ...
    python tools/search_bench.py --min-score 0.9 ...

Per (n_gallery, n_queries, hits) one JSON line:
  count_baseline_us        with --baseline-lib: the same ops.l2_range_count bound to ANOTHER build of the library (the commit before a
                           change), in the same alternation; count_over_baseline is the ratio of the medians, and both builds must leave
                           the same lims and hit words (asserted)
  count_us / scan_us       the count pass (one gallery pass + the prefix launch; lims and the hit words, nothing fetched) and
                           ops.l2_search at --depth over the same gallery (fp32 or half as --storage says), in alternation as above
  count_over_scan          ratio of the medians: the count pass streams the scan's bytes and does less per row
  fill_us, fill_over_count vtc_l2_range_fill into preallocated outputs (ids, fp32 dists), timed in the same alternation
  hits_per_query           the mean number of hits; --hits N takes, per query, the radius halfway between its N-th and (N + 1)-th
                           nearest rows by an fp32 matrix product (about N hits; the count is what the device found), `all` is +inf,
                           --min-score s is radius 2 (1 - s) for every query
  same_hits_as_host        on the first 10^4 rows: lims and ids equal the fp64 membership formed outside the library (asserted)
profiles/search_range.md holds a run's table.

With --after-pages P the tool measures the CURSOR scan (ops.l2_search(after=...) = vtc_l2_search_after) against the plain scan:

    python tools/search_bench.py --after-pages 10 [--deep-k 256,1024] [--baseline-lib OTHER/libvtc_hip.so] [--queries 1,8,64] ...

Per (n_gallery, n_queries) one JSON line:
  plain_us                 ops.l2_search at --depth, no cursor
  after_first_us           the cursor scan with the cursor (-inf, -1): it admits every row, the result is the plain search's (asserted)
  after_deep_us            the cursor scan with the cursor on every query's (64 P)-th neighbour (found by chaining P pages of 64, outside
                           the timing): the rows before the cursor pass the depth-th key's compare for the whole scan and are turned
                           away by the cursor's
  baseline_plain_us        with --baseline-lib: the same ops.l2_search bound to ANOTHER build of the library (the commit before a change
                           to the scan) for the call, so both builds' plain scans run behind the same host code -- all entries in
                           alternation as above
  *_over_plain             ratios of the medians (baseline: plain_over_baseline)
  same_ids_as_host         on the first 10^4 rows: the page after the (64 P)-th neighbour equals that slice of the complete fp64
                           (distance, row) order formed outside the library (asserted; outside the timing)
and per (n_gallery, n_queries, k of --deep-k) one more:
  deep_us / range_us       VideoIndex.search_deep(queries, k) and VideoIndex.range_search at, per query, the score of its k-th neighbour
                           (about k hits; sorted, its host sync inside the timing), in alternation
  range_hits_per_query     what the range search returned
profiles/search_after.md holds a run's table.

With --exclude the tool measures the EXCLUDING scan (ops.l2_search(exclude=...) / ops.l2_search_grouped(exclude=...) =
vtc_l2_search_excluding) against the same call without ``exclude`` -- the scans that were there before it:

    python tools/search_bench.py --exclude [--queries 1,8,64] [--rows-per-video 5] ...

Per (n_gallery, n_queries, storage float32 / float16, ungrouped / grouped at --rows-per-video rows per video) one JSON line:
  excluding_us / plain_us   the excluding scan and the same search without ``exclude``, in alternation as above.  Every query excludes
                            its own NEAREST row (ungrouped) or the video of that row (grouped): the key every wave meets and has to
                            turn away while its lists fill, the case "more like this" and a hard-negative miner produce
  excluding_over_plain      ratio of the medians
  cursor_us                 ungrouped only: the cursor scan with the cursor (-inf, -1) and no ``exclude`` (vtc_l2_search_after), in the
                            same alternation -- the ungrouped excluding scan IS that scan plus the excluded row, so this splits its
                            distance from the plain scan into the cursor's share and the excluded key's (excluding_over_cursor)
  slower_than_spread        the excluding median exceeds the plain median by more than the plain scan's own max - min
  same_as_masked            the excluding result equals, bit for bit, the masked search with the excluded rows' bits cleared, query by
                            query (asserted; outside the timing)
profiles/search_exclude.md holds a run's table.

With --grouped-after P the tool measures a stateless PAGE OF VIDEOS (ops.l2_search_grouped(after=..., n_groups=...) =
vtc_l2_group_mark_before + vtc_l2_search_grouped_after) against ops.l2_search_grouped of the same shape:

    python tools/search_bench.py --grouped-after 1 [--rows-per-video 5] [--queries 1,2,4,8] [--baseline-lib OTHER/libvtc_hip.so] ...

Per (n_gallery, n_queries, storage float32 / float16) one JSON line:
  page_us / grouped_us      the stateless page -- a zeroed bitmap, the mark pass, the page scan, the merge -- with the cursor on the last
                            row of every query's (64 P)-th video (found by chaining P pages of 64, outside the timing), and
                            ops.l2_search_grouped at --depth, in alternation as above
  page_over_grouped         ratio of the medians
  mark_us / scan_us         the two halves on their own: ops.l2_group_mark_before (its torch.zeros included) and the page scan with the
                            bitmap given, in the same alternation
  same_ids_as_host          on the first 10^4 rows: the page equals that slice of the grouped order formed outside the library in fp64
                            (asserted; outside the timing)
  with --baseline-lib, for the entries the other build has (ops.l2_search, l2_search(live=) with every row live, l2_search_grouped, the
  excluding scans ungrouped and grouped, the cursor scan at (-inf, -1), and the page, mark and scan above when it has them): NAME_us, NAME_baseline_us -- the same call bound to ANOTHER
  build of the library (the parent commit) -- and NAME_over_baseline, all in the one alternation
profiles/search_grouped_after.md holds a run's table."""
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


def live_mask(ng, fraction, pattern, gen):
    if fraction >= 1.0:
        return torch.ones(ng, dtype=torch.bool, device="cuda")
    if pattern == "random":
        return torch.rand(ng, device="cuda", generator=gen) < fraction
    m = torch.zeros(ng, dtype=torch.bool, device="cuda")
    lo = (ng // 3) | 1
    m[lo:lo + max(1, int(round(fraction * ng)))] = True
    return m


def masked_main(args):
    lib = L.lib()
    gen = torch.Generator(device="cuda").manual_seed(5)
    lines = []
    for ng in [int(x) for x in args.galleries.split(",")]:
        gallery = ops.normalize_rows(torch.randn(ng, args.d, device="cuda", generator=gen))
        for nq in [int(x) for x in args.queries.split(",")]:
            pick = torch.randint(0, ng, (nq,), device="cuda", generator=gen)
            queries = ops.normalize_rows(gallery[pick] + 0.5 * ops.normalize_rows(torch.randn(nq, args.d, device="cuda", generator=gen)))
            ws_m = ops.workspace(lib.vtc_l2_search_workspace_bytes(ng, nq, args.d, args.depth), gallery.device)
            ws_u = ops.workspace(lib.vtc_l2_search_workspace_bytes(ng, nq, args.d, args.depth), gallery.device)
            for fraction in [float(x) for x in args.live.split(",")]:
                flags = live_mask(ng, fraction, args.live_pattern, gen)
                words = ops.row_mask_pack(flags)
                idx = torch.nonzero(flags).reshape(-1)
                n_live = int(idx.numel())
                assert n_live >= args.depth, "fewer live rows than the depth: nothing to compare"
                masked = lambda: ops.l2_search(gallery, queries, args.depth, ws=ws_m, live=words)                 # noqa: E731
                unmasked = lambda: ops.l2_search(gallery, queries, args.depth, ws=ws_u)                           # noqa: E731

                def topk():
                    rows = gallery[idx]
                    ws_t = ops.workspace(lib.vtc_l2_topk_workspace_bytes(n_live, nq, args.d, L.SWEEP_EXACT, 0), gallery.device)
                    return ops.l2_topk(rows, queries, args.depth, precision=L.SWEEP_EXACT, ws=ws_t)
                entries = [masked, unmasked] + ([topk] if args.topk_gathered else [])
                for _ in range(args.warmup):
                    for fn in entries:
                        fn()
                torch.cuda.synchronize()
                times = [[] for _ in entries]
                for _ in range(args.calls):
                    for t, fn in zip(times, entries):
                        us, out = timed(fn)
                        t.append(us)
                        if fn is masked:
                            ids_m = out[0]
                compact = gallery[idx].contiguous()
                ids_c = ops.l2_search(compact, queries, args.depth)[0]
                same = bool(torch.equal(ids_m, idx[ids_c]))
                del compact
                m, u = stat(times[0]), stat(times[1])
                line = {"n_gallery": ng, "n_queries": nq, "d": args.d, "depth": args.depth, "calls": args.calls, "live": fraction,
                        "pattern": args.live_pattern if fraction < 1.0 else "all", "n_live": n_live, "masked_us": m, "unmasked_us": u,
                        "masked_over_unmasked": round(m["median"] / u["median"], 3), "passes": passes(nq), "same_ids_as_compacted": same}
                if args.topk_gathered:
                    line["topk_gathered_us"] = stat(times[2])
                print(json.dumps(line), flush=True)
                lines.append(line)
                assert same, "the masked scan and the unmasked search over the compacted gallery returned different ids"
            del ws_m, ws_u
        del gallery
        torch.cuda.empty_cache()
    return lines


def collapsed_ids(gallery, queries, groups, depth, live=None):
    """The definition, outside the library: per query the full fp64 (distance, row) order (of the live rows), the first row of every
    group, cut."""
    g64, grp = gallery.double(), groups.cpu().numpy()
    out = np.full((queries.shape[0], depth), -1, np.int64)
    for i in range(queries.shape[0]):
        dist = ((g64 - queries[i].double()) ** 2).sum(1)
        if live is not None:
            dist = dist[live]                                  # compacted: positions are mapped back below
        order = torch.sort(dist, stable=True)[1]
        order = (order if live is None else torch.nonzero(live).reshape(-1)[order]).cpu().numpy()
        _, first = np.unique(grp[order], return_index=True)
        keep = order[np.sort(first)[:depth]]
        out[i, :keep.size] = keep
    return out


def grouped_main(args):
    lib = L.lib()
    gen = torch.Generator(device="cuda").manual_seed(5)
    lines = []
    for ng in [int(x) for x in args.galleries.split(",")]:
        gallery = ops.normalize_rows(torch.randn(ng, args.d, device="cuda", generator=gen))
        for nq in [int(x) for x in args.queries.split(",")]:
            pick = torch.randint(0, ng, (nq,), device="cuda", generator=gen)
            queries = ops.normalize_rows(gallery[pick] + 0.5 * ops.normalize_rows(torch.randn(nq, args.d, device="cuda", generator=gen)))
            ws_g = ops.workspace(lib.vtc_l2_search_grouped_workspace_bytes(ng, nq, args.d, args.depth), gallery.device)
            ws_u = ops.workspace(lib.vtc_l2_search_workspace_bytes(ng, nq, args.d, args.depth), gallery.device)
            for rpv in [int(x) for x in args.rows_per_video.split(",")]:
                groups = (torch.arange(ng, device="cuda") // rpv).to(torch.int32)
                if args.video_layout == "scattered":
                    groups = groups[torch.randperm(ng, device="cuda", generator=gen)].contiguous()
                assert ng // rpv >= args.depth, "fewer videos than the depth: nothing to compare"
                grouped = lambda: ops.l2_search_grouped(gallery, queries, groups, args.depth, ws=ws_g)           # noqa: E731
                ungrouped = lambda: ops.l2_search(gallery, queries, args.depth, ws=ws_u)                         # noqa: E731
                entries = [grouped, ungrouped]
                for _ in range(args.warmup):
                    for fn in entries:
                        fn()
                torch.cuda.synchronize()
                times = [[] for _ in entries]
                for _ in range(args.calls):
                    for t, fn in zip(times, entries):
                        us, out = timed(fn)
                        t.append(us)
                n_check = min(ng, 10 ** 4)
                got = ops.l2_search_grouped(gallery[:n_check], queries, groups[:n_check].contiguous(), args.depth)[0].cpu().numpy()
                same = bool(np.array_equal(got, collapsed_ids(gallery[:n_check], queries, groups[:n_check], args.depth)))
                g, u = stat(times[0]), stat(times[1])
                line = {"n_gallery": ng, "n_queries": nq, "d": args.d, "depth": args.depth, "calls": args.calls, "rows_per_video": rpv,
                        "layout": args.video_layout if rpv > 1 else "one row per video", "grouped_us": g, "ungrouped_us": u,
                        "grouped_over_ungrouped": round(g["median"] / u["median"], 3), "passes": passes(nq),
                        "gallery_tb_per_s": round(ng * args.d * 4 / (1e6 * g["median"]), 3), "same_ids_as_collapsed": same}
                print(json.dumps(line), flush=True)
                lines.append(line)
                assert same, "the grouped scan and the host-collapsed full order returned different ids"
            del ws_g, ws_u
        del gallery
        torch.cuda.empty_cache()
    return lines


def half_main(args):
    """--storage float16: the half scan against the fp32 scan over the same (widened) rows -- plain, with --live, with --rows-per-video."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    variants = [("plain", None, None)]
    if args.live:
        variants = [(f"live {f}", float(f), None) for f in args.live.split(",")]
    if args.rows_per_video:
        variants = [(f"{name}, {r} rows per video" if name != "plain" else f"{r} rows per video", f, int(r))
                    for name, f, _ in variants for r in args.rows_per_video.split(",")]
    lines = []
    for ng in [int(x) for x in args.galleries.split(",")]:
        unrounded = ops.normalize_rows(torch.randn(ng, args.d, device="cuda", generator=gen))
        half = unrounded.to(torch.float16)
        wide = half.float()
        for nq in [int(x) for x in args.queries.split(",")]:
            pick = torch.randint(0, ng, (nq,), device="cuda", generator=gen)
            queries = ops.normalize_rows(unrounded[pick] + 0.5 * ops.normalize_rows(torch.randn(nq, args.d, device="cuda", generator=gen)))
            for name, fraction, rpv in variants:
                words = flags = groups = None
                if fraction is not None:
                    flags = live_mask(ng, fraction, args.live_pattern, gen)
                    words = ops.row_mask_pack(flags)
                    assert int(flags.sum()) >= args.depth * (rpv or 1), "fewer live rows than the depth: nothing to compare"
                if rpv is not None:
                    groups = (torch.arange(ng, device="cuda") // rpv).to(torch.int32)
                    if args.video_layout == "scattered":
                        groups = groups[torch.randperm(ng, device="cuda", generator=gen)].contiguous()
                    assert ng // rpv >= args.depth, "fewer videos than the depth: nothing to compare"
                need = (ops.l2_search_grouped_workspace_bytes if rpv else ops.l2_search_workspace_bytes)(ng, nq, args.d, args.depth)
                ws_h, ws_f = ops.workspace(need, half.device), ops.workspace(need, half.device)

                def search(g, ws, n=None):                     # (ids, dists) of the variant over the first n rows of g
                    if n is not None:
                        g, w, gr = g[:n], None if flags is None else ops.row_mask_pack(flags[:n]), None if groups is None else groups[:n].contiguous()
                    else:
                        w, gr = words, groups
                    if gr is None:
                        return ops.l2_search(g, queries, args.depth, ws=ws, live=w)[:2]
                    out = ops.l2_search_grouped(g, queries, gr, args.depth, ws=ws, live=w)
                    return out[0], out[2]
                entries = [lambda: search(half, ws_h), lambda: search(wide, ws_f)]
                for _ in range(args.warmup):
                    for fn in entries:
                        fn()
                torch.cuda.synchronize()
                times, outs = [[] for _ in entries], [None, None]
                for _ in range(args.calls):
                    for k, fn in enumerate(entries):
                        us, outs[k] = timed(fn)
                        times[k].append(us)
                same_bits = bool(torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]))
                n_check = min(ng, 10 ** 4)
                got = search(half, None, n_check)[0].cpu().numpy()
                host_groups = torch.arange(n_check, device="cuda") if groups is None else groups[:n_check]
                same_host = bool(np.array_equal(got, collapsed_ids(wide[:n_check], queries, host_groups, args.depth,
                                                                   None if flags is None else flags[:n_check])))
                ids_u = search(unrounded, None)[0]
                ids_h = outs[0][0]
                agree = float(np.mean([np.isin(a, b).mean() for a, b in zip(ids_u.cpu().numpy(), ids_h.cpu().numpy())]))
                h, f = stat(times[0]), stat(times[1])
                line = {"n_gallery": ng, "n_queries": nq, "d": args.d, "depth": args.depth, "calls": args.calls, "variant": name,
                        "half_us": h, "fp32_us": f, "half_over_fp32": round(h["median"] / f["median"], 3), "passes": passes(nq),
                        "half_tb_per_s": round(ng * args.d * 2 / (1e6 * h["median"]), 3), "fp32_tb_per_s": round(ng * args.d * 4 / (1e6 * f["median"]), 3),
                        "same_bits_as_fp32": same_bits, "same_ids_as_host": same_host, "top_depth_agreement": round(agree, 4)}
                print(json.dumps(line), flush=True)
                lines.append(line)
                assert same_bits, "the half scan and the fp32 scan over the widened rows returned different bits"
                assert same_host, "the half scan and the host's full fp64 order over the widened rows returned different ids"
                del ws_h, ws_f
        del unrounded, half, wide
        torch.cuda.empty_cache()
    return lines


def q8_main(args):
    """--storage int8: the scan over q8 rows against the fp32 scan and the half scan of the same unit rows."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    lines = []
    for ng in [int(x) for x in args.galleries.split(",")]:
        fp32 = ops.normalize_rows(torch.randn(ng, args.d, device="cuda", generator=gen))
        galleries = {"fp32": fp32, "half": fp32.to(torch.float16), "int8": ops.quantize_rows_q8(fp32)}
        for nq in [int(x) for x in args.queries.split(",")]:
            pick = torch.randint(0, ng, (nq,), device="cuda", generator=gen)
            queries = ops.normalize_rows(fp32[pick] + 0.5 * ops.normalize_rows(torch.randn(nq, args.d, device="cuda", generator=gen)))
            need = ops.l2_search_workspace_bytes(ng, nq, args.d, args.depth)
            ws = {name: ops.workspace(need, fp32.device) for name in galleries}
            entries = {name: (lambda g=g, w=ws[name]: ops.l2_search(g, queries, args.depth, ws=w)[:2]) for name, g in galleries.items()}
            for _ in range(args.warmup):
                for fn in entries.values():
                    fn()
            torch.cuda.synchronize()
            times, outs = {name: [] for name in entries}, {}
            for _ in range(args.calls):
                for name, fn in entries.items():
                    us, outs[name] = timed(fn)
                    times[name].append(us)
            stored = ops.l2_search(ops.dequantize_rows_q8(galleries["int8"]), queries, args.depth)[:2]
            same_bits = bool(torch.equal(outs["int8"][0], stored[0]) and torch.equal(outs["int8"][1], stored[1]))
            top = min(10, args.depth)
            line = {"n_gallery": ng, "n_queries": nq, "d": args.d, "depth": args.depth, "calls": args.calls, "passes": passes(nq)}
            for name, g in galleries.items():
                line[name + "_us"] = stat(times[name])
                line[name + "_mb"] = round(g.numel() * g.element_size() / 2 ** 20, 1)
            for name in ("half", "int8"):
                line[f"{name}_over_fp32"] = round(line[name + "_us"]["median"] / line["fp32_us"]["median"], 3)
                ids = outs[name][0]
                overlap = float(np.mean([np.isin(a[:top], b[:top]).mean() for a, b in zip(outs["fp32"][0].cpu().numpy(), ids.cpu().numpy())]))
                rep = queries[:, None].expand(nq, args.depth, args.d).reshape(-1, args.d).contiguous()
                own = ops.l2_pair_dists64(galleries[name], rep, ids.reshape(-1))
                ref = ops.l2_pair_dists64(fp32, rep, ids.reshape(-1))
                prefix = "" if name == "int8" else "half_"
                line[prefix + "top10_overlap"] = round(overlap, 4)
                line[prefix + "max_score_diff"] = float(((own - ref).abs() / 2).max())
            line["int8_over_half"] = round(line["int8_us"]["median"] / line["half_us"]["median"], 3)
            line["same_bits_as_stored_fp32"] = same_bits
            print(json.dumps(line), flush=True)
            lines.append(line)
            assert same_bits, "the int8 scan and the fp32 scan over the dequantised rows returned different bits"
            del ws, entries
        del fp32, galleries
        torch.cuda.empty_cache()
    return lines


def range_main(args):
    """--hits / --min-score: the range search's count pass against the scan, and the fill pass relative to the count pass."""
    lib = L.lib()
    base = None
    if args.baseline_lib:
        import ctypes as C
        base = C.CDLL(os.path.abspath(args.baseline_lib))
        for name, (res, argtypes) in L.SIGNATURES.items():    # the entries the other build has, with this tree's signatures
            if hasattr(base, name):
                getattr(base, name).restype, getattr(base, name).argtypes = res, argtypes
    gen = torch.Generator(device="cuda").manual_seed(5)
    levels = [("min_score", float(x)) for x in args.min_score.split(",")] if args.min_score else [("hits", x) for x in args.hits.split(",")]
    lines = []
    for ng in [int(x) for x in args.galleries.split(",")]:
        gallery = ops.normalize_rows(torch.randn(ng, args.d, device="cuda", generator=gen))
        if args.storage == "float16":
            gallery = gallery.to(torch.float16)
        for nq in [int(x) for x in args.queries.split(",")]:
            pick = torch.randint(0, ng, (nq,), device="cuda", generator=gen)
            queries = ops.normalize_rows(gallery[pick].float() + 0.5 * ops.normalize_rows(torch.randn(nq, args.d, device="cuda", generator=gen)))
            ws_s = ops.workspace(lib.vtc_l2_search_workspace_bytes(ng, nq, args.d, args.depth), gallery.device)
            ws_r = ops.workspace(ops.l2_range_workspace_bytes(ng, nq, args.d), gallery.device)
            approx = None
            for kind, level in levels:
                if kind == "min_score":
                    radius2 = torch.full((nq,), 2.0 * (1.0 - level), dtype=torch.float64, device="cuda")
                elif level == "all":
                    radius2 = torch.full((nq,), float("inf"), dtype=torch.float64, device="cuda")
                else:
                    if approx is None:
                        approx = 2.0 - 2.0 * (queries @ gallery.float().t())           # [Q, n] fp32: only places the radius
                    low = torch.topk(approx, int(level) + 1, dim=1, largest=False)[0]
                    radius2 = ((low[:, -1].double() + low[:, -2].double()) / 2).contiguous()
                lims = ops.l2_range_count(gallery, queries, radius2, ws=ws_r)
                total = int(lims[-1])
                ids = torch.empty(total, dtype=torch.int64, device="cuda")
                dists = torch.empty(total, dtype=torch.float32, device="cuda")
                stream = torch.cuda.current_stream().cuda_stream

                def fill():
                    L.check(lib.vtc_l2_range_fill(gallery.data_ptr(), int(gallery.dtype == torch.float16), queries.data_ptr(), ng, nq, args.d,
                                                  lims.data_ptr(), total, 0, ids.data_ptr(), dists.data_ptr(), None, ws_r.data_ptr(), ws_r.numel(),
                                                  stream), "vtc_l2_range_fill")
                scan = lambda: ops.l2_search(gallery, queries, args.depth, ws=ws_s)                                # noqa: E731
                count = lambda: ops.l2_range_count(gallery, queries, radius2, ws=ws_r)                             # noqa: E731
                entries = [scan, count, fill]                  # fill follows a count over the same radius in the same workspace
                if base:
                    ws_b = ops.workspace(ops.l2_range_workspace_bytes(ng, nq, args.d), gallery.device)

                    def count_baseline():                      # the same ops.l2_range_count, bound to the other build for the call
                        mine, L._lib = L._lib, base
                        try:
                            return ops.l2_range_count(gallery, queries, radius2, ws=ws_b)
                        finally:
                            L._lib = mine
                    entries.append(count_baseline)
                for _ in range(args.warmup):
                    for fn in entries:
                        fn()
                torch.cuda.synchronize()
                times = [[] for _ in entries]
                for _ in range(args.calls):
                    for t, fn in zip(times, entries):
                        t.append(timed(fn)[0])
                n_check = min(ng, 10 ** 4)
                got = ops.l2_range_search(gallery[:n_check], queries, radius2, max_results=nq * n_check)
                g64 = gallery[:n_check].double()
                member = torch.stack([((g64 - queries[i].double()) ** 2).sum(1) <= radius2[i] for i in range(nq)])
                want_lims = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), member.sum(1).cumsum(0)])
                same = bool(torch.equal(got[0], want_lims) and torch.equal(got[1], torch.nonzero(member)[:, 1]))
                sc, c, f = stat(times[0]), stat(times[1]), stat(times[2])
                line = {"n_gallery": ng, "n_queries": nq, "d": args.d, "depth": args.depth, "calls": args.calls, "storage": args.storage,
                        kind: level, "hits_per_query": round(total / nq, 1), "count_us": c, "scan_us": sc, "fill_us": f,
                        "count_over_scan": round(c["median"] / sc["median"], 3), "fill_over_count": round(f["median"] / c["median"], 3),
                        "passes": passes(nq), "gallery_tb_per_s": round(ng * args.d * gallery.element_size() / (1e6 * c["median"]), 3),
                        "same_hits_as_host": same}
                if base:
                    same_base = bool(torch.equal(count(), count_baseline()) and
                                     torch.equal(ops.range_hit_words(ws_r, ng, nq), ops.range_hit_words(ws_b, ng, nq)))
                    cb = stat(times[3])
                    line.update({"count_baseline_us": cb, "count_over_baseline": round(c["median"] / cb["median"], 3), "same_as_baseline": same_base})
                print(json.dumps(line), flush=True)
                lines.append(line)
                assert same, "the range search and the host's fp64 membership differ on the first 10^4 rows"
                assert not base or same_base, "the two builds' count passes left different lims or hit words"
                del ids, dists
            del ws_s, ws_r, approx
        del gallery
        torch.cuda.empty_cache()
    return lines


def after_main(args):
    """--after-pages: the cursor scan against the plain scan (and another build's plain scan); search_deep against range_search."""
    import ctypes as C

    from vtc_amd.host.search import VideoIndex
    lib = L.lib()
    base = None
    if args.baseline_lib:
        base = C.CDLL(os.path.abspath(args.baseline_lib))
        for name, (res, argtypes) in L.SIGNATURES.items():    # the entries the other build has, with this tree's signatures
            if hasattr(base, name):
                getattr(base, name).restype, getattr(base, name).argtypes = res, argtypes
    gen = torch.Generator(device="cuda").manual_seed(5)
    deep_pages, lines = int(args.after_pages), []
    for ng in [int(x) for x in args.galleries.split(",")]:
        gallery = ops.normalize_rows(torch.randn(ng, args.d, device="cuda", generator=gen))
        index = VideoIndex(args.d, normalized=True)
        index.add(gallery)
        for nq in [int(x) for x in args.queries.split(",")]:
            pick = torch.randint(0, ng, (nq,), device="cuda", generator=gen)
            queries = ops.normalize_rows(gallery[pick] + 0.5 * ops.normalize_rows(torch.randn(nq, args.d, device="cuda", generator=gen)))
            need = lib.vtc_l2_search_workspace_bytes(ng, nq, args.d, args.depth)
            ws = [ops.workspace(need, gallery.device) for _ in range(4)]

            def cursor_after(g, pages):                        # the key of every query's (64 pages)-th neighbour in g
                ws64 = ops.workspace(lib.vtc_l2_search_workspace_bytes(g.shape[0], nq, args.d, 64), g.device)
                after = None
                for _ in range(pages):
                    ids = ops.l2_search(g, queries, 64, ws=ws64, after=after)[0]
                    after = (ops.search_dists64(ws64, nq, 64)[:, -1].clone(), ids[:, -1].clone())
                return after
            first = (torch.full((nq,), float("-inf"), dtype=torch.float64, device="cuda"), torch.full((nq,), -1, dtype=torch.int64, device="cuda"))
            deep = cursor_after(gallery, deep_pages)
            plain = lambda: ops.l2_search(gallery, queries, args.depth, ws=ws[0])                                  # noqa: E731
            after_first = lambda: ops.l2_search(gallery, queries, args.depth, ws=ws[1], after=first)              # noqa: E731
            after_deep = lambda: ops.l2_search(gallery, queries, args.depth, ws=ws[2], after=deep)                # noqa: E731

            def baseline():                                    # the same ops.l2_search, bound to the other build for the call
                mine, L._lib = L._lib, base
                try:
                    return ops.l2_search(gallery, queries, args.depth, ws=ws[3])
                finally:
                    L._lib = mine
            entries = [plain, after_first, after_deep] + ([baseline] if base else [])
            for _ in range(args.warmup):
                for fn in entries:
                    fn()
            torch.cuda.synchronize()
            times, outs = [[] for _ in entries], [None] * len(entries)
            for _ in range(args.calls):
                for k, fn in enumerate(entries):
                    us, outs[k] = timed(fn)
                    times[k].append(us)
            same_first = all(bool(torch.equal(outs[0][i], o[i])) for o in outs[1:2] + outs[3:] for i in (0, 1))
            n_check = min(ng, 10 ** 4)
            small = gallery[:n_check]
            got = ops.l2_search(small, queries, args.depth, after=cursor_after(small, deep_pages))[0]
            g64 = small.double()
            want = torch.stack([torch.sort(((g64 - queries[i].double()) ** 2).sum(1), stable=True)[1][64 * deep_pages:64 * deep_pages + args.depth]
                                for i in range(nq)])
            same_host = bool(torch.equal(got, want))
            st = [stat(t) for t in times]
            line = {"n_gallery": ng, "n_queries": nq, "d": args.d, "depth": args.depth, "calls": args.calls, "cursor_at": 64 * deep_pages,
                    "plain_us": st[0], "after_first_us": st[1], "after_deep_us": st[2],
                    "after_first_over_plain": round(st[1]["median"] / st[0]["median"], 3),
                    "after_deep_over_plain": round(st[2]["median"] / st[0]["median"], 3), "passes": passes(nq),
                    "same_as_plain": same_first, "same_ids_as_host": same_host}
            if base:
                line["baseline_plain_us"] = st[3]
                line["plain_over_baseline"] = round(st[0]["median"] / st[3]["median"], 3)
                line["after_first_over_baseline"] = round(st[1]["median"] / st[3]["median"], 3)
                line["after_deep_over_baseline"] = round(st[2]["median"] / st[3]["median"], 3)
            print(json.dumps(line), flush=True)
            lines.append(line)
            assert same_first, "the cursor scan at (-inf, -1) (or the baseline build) and the plain scan returned different bits"
            assert same_host, "the page after the cursor and the host's full fp64 order differ on the first 10^4 rows"
            del ws
            for k in [int(x) for x in args.deep_k.split(",") if x]:
                min_score = index.search_deep(queries, k)[1][:, -1].double().cpu().tolist()
                entries = [lambda: index.search_deep(queries, k), lambda: index.range_search(queries, min_score, max_results=1 << 26)]
                for _ in range(args.warmup):
                    for fn in entries:
                        fn()
                torch.cuda.synchronize()
                times, outs = [[], []], [None, None]
                for _ in range(args.calls):
                    for j, fn in enumerate(entries):
                        us, outs[j] = timed(fn)
                        times[j].append(us)
                dp, rg = stat(times[0]), stat(times[1])
                line = {"n_gallery": ng, "n_queries": nq, "d": args.d, "calls": args.calls, "search_deep_k": k, "deep_us": dp, "range_us": rg,
                        "deep_over_range": round(dp["median"] / rg["median"], 3), "deep_passes": passes(nq) * -(-k // 64),
                        "range_hits_per_query": round(outs[1][1].numel() / nq, 1)}
                print(json.dumps(line), flush=True)
                lines.append(line)
        del gallery, index
        torch.cuda.empty_cache()
    return lines


def exclude_main(args):
    """--exclude: the excluding scan against the same search without an excluded key, fp32 and half, ungrouped and grouped."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    rpv = int((args.rows_per_video or "5").split(",")[0])
    lines = []
    for ng in [int(x) for x in args.galleries.split(",")]:
        rows32 = ops.normalize_rows(torch.randn(ng, args.d, device="cuda", generator=gen))
        storages = {"float32": rows32, "float16": rows32.to(torch.float16)}
        groups = (torch.arange(ng, device="cuda") // rpv).to(torch.int32)
        assert ng // rpv > args.depth, "fewer videos than the depth: nothing to compare"
        flags = torch.ones(ng, dtype=torch.uint8, device="cuda")
        for nq in [int(x) for x in args.queries.split(",")]:
            pick = torch.randint(0, ng, (nq,), device="cuda", generator=gen)
            queries = ops.normalize_rows(rows32[pick] + 0.5 * ops.normalize_rows(torch.randn(nq, args.d, device="cuda", generator=gen)))
            for storage, gallery in storages.items():
                for grouped in (False, True):
                    need = (ops.l2_search_grouped_workspace_bytes if grouped else ops.l2_search_workspace_bytes)(ng, nq, args.d, args.depth)
                    ws_x, ws_p = ops.workspace(need, gallery.device), ops.workspace(need, gallery.device)

                    def search(ws, exclude=None, q=queries, live=None, after=None):      # (ids, dists)
                        if grouped:
                            out = ops.l2_search_grouped(gallery, q, groups, args.depth, ws=ws, live=live, exclude=exclude)
                            return out[0], out[2]
                        return ops.l2_search(gallery, q, args.depth, ws=ws, live=live, exclude=exclude, after=after)[:2]
                    nearest = search(None)[0][:, 0].clone()        # every query's nearest row: the key it excludes
                    exclude = groups[nearest].to(torch.int64) if grouped else nearest
                    entries = [lambda: search(ws_x, exclude), lambda: search(ws_p)]
                    if not grouped:
                        ws_c = ops.workspace(need, gallery.device)
                        first = (torch.full((nq,), float("-inf"), dtype=torch.float64, device="cuda"),
                                 torch.full((nq,), -1, dtype=torch.int64, device="cuda"))
                        entries.append(lambda: search(ws_c, after=first))
                    for _ in range(args.warmup):
                        for fn in entries:
                            fn()
                    torch.cuda.synchronize()
                    times, outs = [[] for _ in entries], [None] * len(entries)
                    for _ in range(args.calls):
                        for k, fn in enumerate(entries):
                            us, outs[k] = timed(fn)
                            times[k].append(us)
                    same = True
                    for u in range(nq):
                        f = flags.clone()
                        f[(groups == exclude[u]) if grouped else exclude[u]] = 0
                        want = search(None, q=queries[u:u + 1], live=ops.row_mask_pack(f))
                        same = same and bool(torch.equal(outs[0][0][u], want[0][0]) and torch.equal(outs[0][1][u], want[1][0]))
                    changed = not bool((outs[0][0][:, 0] == outs[1][0][:, 0]).any())
                    x, pl = stat(times[0]), stat(times[1])
                    line = {"n_gallery": ng, "n_queries": nq, "d": args.d, "depth": args.depth, "calls": args.calls, "storage": storage,
                            "variant": f"grouped, {rpv} rows per video" if grouped else "ungrouped", "excluding_us": x, "plain_us": pl,
                            "excluding_over_plain": round(x["median"] / pl["median"], 3),
                            "slower_than_spread": bool(x["median"] - pl["median"] > pl["max"] - pl["min"]), "passes": passes(nq),
                            "gallery_tb_per_s": round(ng * args.d * gallery.element_size() / (1e6 * x["median"]), 3),
                            "same_as_masked": same, "nearest_left_out": changed}
                    if not grouped:
                        line["cursor_us"] = stat(times[2])
                        line["excluding_over_cursor"] = round(x["median"] / line["cursor_us"]["median"], 3)
                        del ws_c
                    print(json.dumps(line), flush=True)
                    lines.append(line)
                    assert same and changed, "the excluding scan and the masked search without the excluded rows returned different bits"
                    del ws_x, ws_p
        del rows32, storages
        torch.cuda.empty_cache()
    return lines


def grouped_after_main(args):
    """--grouped-after: a stateless page of videos against the grouped scan; the older entries against another build."""
    import ctypes as C
    base = None
    if args.baseline_lib:
        base = C.CDLL(os.path.abspath(args.baseline_lib))
        for name, (res, argtypes) in L.SIGNATURES.items():    # the entries the other build has, with this tree's signatures
            if hasattr(base, name):
                getattr(base, name).restype, getattr(base, name).argtypes = res, argtypes
    gen = torch.Generator(device="cuda").manual_seed(5)
    rpv = int((args.rows_per_video or "5").split(",")[0])
    pages, lines = int(args.grouped_after), []

    def cursor_after(g, q, groups, n_groups, n_pages):         # the key of the last row of every query's (64 n_pages)-th video in g
        ws64 = ops.workspace(ops.l2_search_grouped_workspace_bytes(g.shape[0], q.shape[0], args.d, 64), g.device)
        after = None
        for _ in range(n_pages):
            ids = ops.l2_search_grouped(g, q, groups, 64, ws=ws64, after=after, n_groups=n_groups)[0]
            after = (ops.search_dists64(ws64, q.shape[0], 64)[:, -1].clone(), ids[:, -1].clone())
        return after
    for ng in [int(x) for x in args.galleries.split(",")]:
        rows32 = ops.normalize_rows(torch.randn(ng, args.d, device="cuda", generator=gen))
        storages = {"float32": rows32, "float16": rows32.to(torch.float16)}
        groups = (torch.arange(ng, device="cuda") // rpv).to(torch.int32)
        n_groups = -(-ng // rpv)
        assert n_groups > 64 * pages + args.depth, "fewer videos than the page reaches"
        all_live = ops.row_mask_pack(torch.ones(ng, dtype=torch.uint8, device="cuda"))
        for nq in [int(x) for x in args.queries.split(",")]:
            pick = torch.randint(0, ng, (nq,), device="cuda", generator=gen)
            queries = ops.normalize_rows(rows32[pick] + 0.5 * ops.normalize_rows(torch.randn(nq, args.d, device="cuda", generator=gen)))
            for storage, gallery in storages.items():
                need = ops.l2_search_grouped_workspace_bytes(ng, nq, args.d, args.depth)
                cursor = cursor_after(gallery, queries, groups, n_groups, pages)
                ban = ops.l2_group_mark_before(gallery, queries, groups, n_groups, cursor)
                first = (torch.full((nq,), float("-inf"), dtype=torch.float64, device="cuda"), torch.full((nq,), -1, dtype=torch.int64, device="cuda"))
                nearest = ops.l2_search(gallery, queries, 1)[0][:, 0].clone()
                own = groups[nearest].to(torch.int64)
                new = {"page": lambda ws: ops.l2_search_grouped(gallery, queries, groups, args.depth, ws=ws, after=cursor, n_groups=n_groups),
                       "mark": lambda ws: ops.l2_group_mark_before(gallery, queries, groups, n_groups, cursor),
                       "scan": lambda ws: ops.l2_search_grouped(gallery, queries, groups, args.depth, ws=ws, after=cursor, n_groups=n_groups, ban=ban)}
                old = {"grouped": lambda ws: ops.l2_search_grouped(gallery, queries, groups, args.depth, ws=ws),
                       "search": lambda ws: ops.l2_search(gallery, queries, args.depth, ws=ws),
                       "masked": lambda ws: ops.l2_search(gallery, queries, args.depth, ws=ws, live=all_live),
                       "cursor": lambda ws: ops.l2_search(gallery, queries, args.depth, ws=ws, after=first),
                       "excluding": lambda ws: ops.l2_search(gallery, queries, args.depth, ws=ws, exclude=nearest),
                       "excluding_grouped": lambda ws: ops.l2_search_grouped(gallery, queries, groups, args.depth, ws=ws, exclude=own)}

                def bound(fn, lib_, ws):                       # the same host code, bound to `lib_` for the call
                    def call():
                        mine, L._lib = L._lib, lib_
                        try:
                            return fn(ws)
                        finally:
                            L._lib = mine
                    return call
                names, entries = [], []
                for name, fn in list(new.items()) + list(old.items()):
                    names.append(name)
                    entries.append(bound(fn, L.lib(), ops.workspace(need, gallery.device)))
                    if base and (name in old or hasattr(base, "vtc_l2_search_grouped_after")):
                        names.append(name + "_baseline")
                        entries.append(bound(fn, base, ops.workspace(need, gallery.device)))
                for _ in range(args.warmup):
                    for fn in entries:
                        fn()
                torch.cuda.synchronize()
                times, outs = [[] for _ in entries], [None] * len(entries)
                for _ in range(args.calls):
                    for k, fn in enumerate(entries):
                        us, outs[k] = timed(fn)
                        times[k].append(us)
                st = {n: stat(t) for n, t in zip(names, times)}
                out = dict(zip(names, outs))
                same_halves = all(bool(torch.equal(a, b)) for a, b in zip(out["page"][:3], out["scan"][:3]))
                in_base = [n for n in names if n + "_baseline" in names]
                same_base = all(bool(torch.equal(a, b)) for n in in_base for a, b in zip(tuple(out[n])[:2] if n != "mark" else (out[n],),
                                                                                       tuple(out[n + "_baseline"])[:2] if n != "mark" else
                                                                                       (out[n + "_baseline"],)))
                n_check = min(ng, 10 ** 4)
                small, small_groups = gallery[:n_check], groups[:n_check].contiguous()
                got = ops.l2_search_grouped(small, queries, small_groups, args.depth, n_groups=n_groups,
                                            after=cursor_after(small, queries, small_groups, n_groups, pages))[0].cpu().numpy()
                g64, host_groups, want = small.double(), small_groups.cpu().numpy(), []
                for i in range(nq):
                    order = torch.sort(((g64 - queries[i].double()) ** 2).sum(1), stable=True)[1].cpu().numpy()
                    firsts = np.sort(np.unique(host_groups[order], return_index=True)[1])      # the first row of every video, in order
                    want.append(order[firsts][64 * pages:64 * pages + args.depth])
                same_host = bool(np.array_equal(got, np.stack(want)))
                line = {"n_gallery": ng, "n_queries": nq, "d": args.d, "depth": args.depth, "calls": args.calls, "storage": storage,
                        "rows_per_video": rpv, "cursor_at_video": 64 * pages, "passes": passes(nq)}
                for n in names:
                    line[n + "_us"] = st[n]
                line["page_over_grouped"] = round(st["page"]["median"] / st["grouped"]["median"], 3)
                line["mark_over_grouped"] = round(st["mark"]["median"] / st["grouped"]["median"], 3)
                line["scan_over_grouped"] = round(st["scan"]["median"] / st["grouped"]["median"], 3)
                if base:
                    for n in in_base:
                        line[n + "_over_baseline"] = round(st[n]["median"] / st[n + "_baseline"]["median"], 3)
                line.update({"page_is_mark_then_scan": same_halves, "same_as_baseline": same_base, "same_ids_as_host": same_host})
                print(json.dumps(line), flush=True)
                lines.append(line)
                assert same_halves and same_base, "the stateless page and its two halves, or the two builds, returned different bits"
                assert same_host, "the page after the cursor and the host's fp64 grouped order differ on the first 10^4 rows"
                del entries
        del rows32, storages
        torch.cuda.empty_cache()
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--galleries", type=str, default="100000,1000000")
    ap.add_argument("--queries", type=str, default="1,4,8,16,32,64")
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--depth", type=int, default=11)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--live", type=str, default=None, help="live fractions, e.g. 1.0,0.5,0.1,0.01: measure the masked scan (see above)")
    ap.add_argument("--live-pattern", type=str, default="random", choices=("random", "blocked"))
    ap.add_argument("--topk-gathered", action="store_true", help="with --live: also time gather + l2_topk(EXACT) over the live rows")
    ap.add_argument("--rows-per-video", type=str, default=None, help="rows per video, e.g. 1,5,20: measure the grouped scan (see above)")
    ap.add_argument("--video-layout", type=str, default="contiguous", choices=("contiguous", "scattered"))
    ap.add_argument("--storage", type=str, default="float32", choices=("float32", "float16", "int8"),
                    help="float16: measure the scan over a half gallery against the fp32 scan (see above); works with --live / --rows-per-video.  "
                         "int8: the scan over q8 rows against the fp32 and the half scan of the same rows (see above)")
    ap.add_argument("--hits", type=str, default=None, help="hits per query, e.g. 100,10000,all: measure the range search (see above)")
    ap.add_argument("--min-score", type=str, default=None, help="score thresholds, e.g. 0.9,0.5: the range search at radius 2 (1 - s)")
    ap.add_argument("--after-pages", type=int, default=None, help="P: measure the cursor scan, the cursor on the (64 P)-th neighbour (see above)")
    ap.add_argument("--deep-k", type=str, default="256,1024", help="with --after-pages: k of VideoIndex.search_deep against range_search")
    ap.add_argument("--exclude", action="store_true",
                    help="measure the excluding scan against the same search without an excluded key, fp32 and half, ungrouped and grouped (see above)")
    ap.add_argument("--baseline-lib", type=str, default=None,
                    help="with --after-pages / --grouped-after / --hits: another build of libvtc_hip.so whose older entries are timed too")
    ap.add_argument("--grouped-after", type=int, default=None,
                    help="P: measure a stateless page of videos, the cursor on the (64 P)-th video, against the grouped scan (see above)")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    assert args.calls >= 30, "at least 30 timed calls per entry"
    if args.storage == "int8":
        assert not (args.live or args.rows_per_video or args.hits or args.min_score or args.exclude or args.after_pages is not None or
                    args.grouped_after is not None), "the int8 mode measures the plain scan of the three storages"
        write_out(args.out, q8_main(args))
        return
    if args.grouped_after is not None:
        assert args.grouped_after >= 1 and not (args.live or args.hits or args.min_score or args.after_pages is not None or args.exclude), \
            "the page mode takes --rows-per-video and --baseline-lib only"
        write_out(args.out, grouped_after_main(args))
        return
    if args.exclude:
        assert not (args.live or args.hits or args.min_score or args.after_pages is not None), "the excluding mode takes --rows-per-video only"
        write_out(args.out, exclude_main(args))
        return
    if args.after_pages is not None:
        assert args.after_pages >= 1 and not (args.live or args.rows_per_video or args.hits or args.min_score or args.storage != "float32"), \
            "the cursor mode measures the plain fp32 scan's variants only"
        write_out(args.out, after_main(args))
        return
    if args.hits or args.min_score:
        assert not (args.live or args.rows_per_video), "the range mode has no --live / --rows-per-video variants"
        write_out(args.out, range_main(args))
        return
    if args.storage == "float16":
        write_out(args.out, half_main(args))
        return
    if args.live:
        write_out(args.out, masked_main(args))
        return
    if args.rows_per_video:
        write_out(args.out, grouped_main(args))
        return
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
    write_out(args.out, lines)


def write_out(out, lines):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
