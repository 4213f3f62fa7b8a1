"""GPU: the many-query search of a half gallery (vtc_l2_search_many_half; ops.l2_search_many; VideoIndex.search_many).  Its definition is
"vtc_l2_search_half without groups, bit for bit", so the first oracle is ops.l2_search on the same half gallery -- torch.equal on ids,
fp32 dists, the fp64 head of the workspace and the non-finite word -- and the second the numpy fp64 reference over the widened rows
(tests/search_half_refs.py / search_refs.py).  ops.search_many_stats tells the MFMA route from a scan in disguise: the number of queries
the exact fallback finished is 0 on separated data and at least 1 where the candidate list cannot be certified.

KAPPA below is the bound search_many.hip derives: |A - D| <= KAPPA(d) (|q|^2 + max|g|^2) + 1e-35."""
import numpy as np
import pytest
import torch

import search_half_refs as HR
import search_mask_refs as MR
import search_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def KAPPA(d):
    return (6 * d + 8) * 2.0 ** -24 + 2.0 ** -20


def _ops():
    from vtc_amd import ops
    return ops


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _words(live):
    return None if live is None else _t(MR.pack_words(live).view(np.int32))


def _both(g, q, depth, live=None, id_base=0):
    """((ids, dists, bits, dists64) of l2_search_many, the same of l2_search, fallback queries), each call in a workspace of its own."""
    ops = _ops()
    th, tq = (g if isinstance(g, torch.Tensor) else _t(g)), (q if isinstance(q, torch.Tensor) else _t(q))
    ng, d = th.shape
    nq = tq.shape[0]
    words = live if isinstance(live, torch.Tensor) or live is None else _words(live)
    ws = ops.workspace(ops.l2_search_many_workspace_bytes(ng, nq, d, depth), DEV)
    many = tuple(ops.l2_search_many(th, tq, depth, id_base=id_base, live=words, ws=ws)) + (ops.search_dists64(ws, nq, depth).clone(),)
    fallbacks = ops.search_many_stats(ws, nq, depth)["fallback_queries"]
    ws2 = ops.workspace(ops.l2_search_workspace_bytes(ng, nq, d, depth), DEV)
    scan = tuple(ops.l2_search(th, tq, depth, id_base=id_base, live=words, ws=ws2)) + (ops.search_dists64(ws2, nq, depth).clone(),)
    return many, scan, fallbacks


def _same_bits(many, scan):
    for x, y in zip(many, scan):
        assert x.dtype == y.dtype and torch.equal(x, y), (x, y)


def _check(g, q, depth, live=None, id_base=0, ref=None):
    """Both oracles; ref: (ids, dists64) of the CPU reference at this depth, when the caller has one.  Returns (result, fallback queries)."""
    many, scan, fallbacks = _both(g, q, depth, live, id_base)
    _same_bits(many, scan)
    if ref is not None:
        assert np.array_equal(many[0].cpu().numpy(), ref[0])
        SR.assert_dists_within_one_ulp(many[1].cpu().numpy(), ref[1].astype(np.float32))
    assert 0 <= fallbacks <= q.shape[0]
    return many, fallbacks


def _separated(ng, d, nq, seed=7):
    """Seeded unit-norm gaussian rows rounded to half, unit-norm gaussian queries."""
    rng = np.random.default_rng(seed)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return HR.round_half(unit(rng.standard_normal((ng, d)))), unit(rng.standard_normal((nq, d)))


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 192, 512, 2048])
@pytest.mark.parametrize("ng", [1, 31, 63, 64, 65, 257, 5000])
def test_shapes(d, ng):
    """Every n_queries in {1, 7, 33, 64} and depth in {1, 11, 32} that the gallery allows; 5000 rows are more than one step per workgroup.
    Galleries of 16 rows and more hold search_half_refs.special_rows (subnormals, +-65504, duplicates).  One CPU reference per gallery:
    the lists of fewer queries and smaller depths are its prefixes."""
    g, q = HR.half_pairs(max(ng, 64), d, HR.SEED + d)
    g = HR.special_rows(g[:ng], seed=d) if ng >= 16 else g[:ng]
    q = q[:64]
    deepest = min(32, ng)
    ids, d64, gap = HR.reference_search64(g, q, deepest, id_base=2 ** 33 + 5)
    assert gap > 1e-12, gap
    live = MR.make_mask("alt_bits", ng) if ng >= 33 else None
    if live is not None:
        mids, md32, mgap = HR.reference_search_masked(g, q, live, deepest, 3)
        assert mgap > 1e-12
    for nq in (1, 7, 33, 64):
        for depth in (1, 11, 32):
            if depth > ng:
                continue
            _check(g, q[:nq], depth, id_base=2 ** 33 + 5, ref=(ids[:nq, :depth], d64[:nq, :depth]))
            if live is not None and (nq, depth) in ((7, 11), (64, 32), (33, 1)):
                _check(g, q[:nq], depth, live=live, id_base=3, ref=(mids[:nq, :depth], md32[:nq, :depth].astype(np.float64)))


# ---- the MFMA route is taken -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,depth", [(64, 5), (512, 11), (512, 32)])
def test_separated_data_is_certified_without_the_fallback(d, depth):
    """4096 unit rows, 64 unit queries: the gap between the depth-th and the cdepth-th fp64 distance exceeds 2 eps for every query
    (recomputed here, not assumed), so every list must be certified: the fallback counter is 0."""
    ng, nq = 4096, 64
    g, q = _separated(ng, d, nq)
    D = SR.distances64(HR.widen(g), q)
    cdepth = min(64, ng, max(32, depth + 21))
    srt = np.sort(D, axis=1)
    gap = (srt[:, cdepth - 1] - srt[:, depth - 1]).min()
    gmax = (HR.widen(g).astype(np.float64) ** 2).sum(1).max()
    eps = (KAPPA(d) * ((q.astype(np.float64) ** 2).sum(1) + gmax) + 1e-35).max()
    print(f"d={d} depth={depth}: smallest gap {gap:.4g}, 2 eps {2 * eps:.4g}")
    assert gap > 2 * eps, (gap, eps)
    ids, d64, _ = SR.sorted_lists(D, depth)
    _, fallbacks = _check(g, q, depth, ref=(ids, d64))
    assert fallbacks == 0
    # ... and under a mask, with garbage in the dead rows' place in the counter's way
    live = MR.make_mask("random_0.5", ng, seed=3)
    Dm = D.copy()
    Dm[:, ~live] = np.inf
    ids, d64, _ = SR.sorted_lists(Dm, depth)
    _, fallbacks = _check(g, q, depth, live=live, ref=(ids, d64))
    assert fallbacks == 0


# ---- the fallback is taken, and is right -----------------------------------------------------------------------------------------------
def test_duplicates_deeper_than_the_list_go_to_the_fallback():
    """100 identical rows nearest query 0, at high row indices: no list of 32 can be certified for depth 11 (the 33rd duplicate ties with
    the 11th), the fallback finishes the query and returns the 11 LOWEST duplicate rows."""
    ng, d, depth = 3000, 64, 11
    g, q = _separated(ng, d, 5)
    dup = np.sort(np.random.default_rng(1).choice(np.arange(1500, ng), 100, replace=False))
    g[dup] = HR.round_half(q[0])
    many, fallbacks = _check(g, q, depth, id_base=7)
    assert fallbacks >= 1
    assert np.array_equal(many[0][0].cpu().numpy(), 7 + dup[:depth])
    d64 = many[3][0].cpu().numpy()
    assert (d64 == d64[0]).all()


def test_a_cluster_of_rows_one_half_ulp_apart():
    """80 rows that differ from one another by one half ulp in a single coordinate: far closer than the bound resolves."""
    ng, d, depth = 1000, 192, 11
    g, q = _separated(ng, d, 9)
    base = HR.round_half(q[3])
    cluster = np.arange(400, 480)
    g[cluster] = base
    for n, j in enumerate(cluster):
        c = n % d
        g[j, c] = np.nextafter(base[c], np.float16(np.inf if n % 2 else -np.inf))
    many, fallbacks = _check(g, q, depth)                                     # equal to the scan, bit for bit
    assert fallbacks >= 1
    assert np.isin(many[0][3].cpu().numpy(), cluster).all()
    assert np.allclose(many[3].cpu().numpy(), HR.reference_search64(g, q, depth)[1], rtol=1e-9, atol=0)


# ---- adversarial rounding ----------------------------------------------------------------------------------------------------------------
def test_queries_on_fp16_midpoints_against_rows_one_ulp_apart():
    """Every query component sits exactly between two halves with the residual of one sign (hi rounds to even, lo carries half an ulp
    everywhere); the rows are the two neighbouring halves in varying columns."""
    ng, d, depth = 600, 512, 11
    rng = np.random.default_rng(11)
    lo = np.abs(HR.round_half(rng.standard_normal((4, d)) / np.sqrt(d))) + np.float16(2.0 ** -10)
    lo = (lo.view(np.uint16) & np.uint16(0xfffe)).view(np.float16)            # even: the tie rounds DOWN, every residual is + half an ulp
    hi = np.nextafter(lo, np.float16(np.inf))
    q = ((lo.astype(np.float32) + hi.astype(np.float32)) / 2).astype(np.float32)          # exact: one more bit than a half has
    g, _ = _separated(ng, d, 1, seed=12)
    for j in range(100, 200):
        row = lo[j % 4].copy()
        pick = rng.random(d) < 0.5
        row[pick] = hi[j % 4][pick]
        g[j] = row
    ids, d64, _ = HR.reference_search64(g, q, depth)
    many, _ = _check(g, q, depth)
    assert np.allclose(many[3].cpu().numpy(), d64, rtol=1e-12)


def test_subnormal_rows_are_not_flushed_and_ties_go_to_the_lower_row():
    """A gallery of nothing but subnormal halves and zeros: the distances are |q|^2 minus terms far below the bound, every list is the
    scan's; rows 20 .. 23 are bit-equal and come back in row order when they are the nearest."""
    ng, d, depth = 300, 64, 11
    rng = np.random.default_rng(13)
    g = (rng.integers(-1023, 1024, (ng, d)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float16)
    q = (rng.standard_normal((6, d)) * 1e-3).astype(np.float32)
    q[0] = 0
    g[21:24] = g[20]
    q[1] = HR.widen(g[20:21])[0]
    many, _ = _check(g, q, depth)
    assert many[0][1, :4].tolist() == [20, 21, 22, 23]
    # the same with queries of the rows' own magnitude: the split's scale is 2^36 there
    many, _ = _check(g, HR.widen(g[::50]) * np.float32(1.5), depth)


@pytest.mark.parametrize("scale", [1e-30, 1e30])
def test_queries_far_outside_half_range(scale):
    """D is finite in fp64 for both.  At 1e30 |q|^2 overflows fp32, so A does: those queries go to the fallback."""
    ng, d, depth = 700, 128, 11
    g, q = _separated(ng, d, 8)
    q = q.copy()
    q[[1, 4]] *= np.float32(scale)
    many, fallbacks = _check(g, q, depth)                                     # the scan's bits, for the scaled queries too
    if scale > 1:
        assert fallbacks >= 2
    assert int(many[2].item()) == 0
    # (B) where numpy's summation order cannot matter: at 1e30 every distance of a query agrees to 1e-30, the order is the last bits'
    keep = [0, 2, 3, 5, 6, 7] + ([1, 4] if scale < 1 else [])
    ids, d64, _ = HR.reference_search64(g, q[keep], depth)
    assert np.array_equal(many[0][keep].cpu().numpy(), ids)
    assert bool(torch.isfinite(many[3]).all())


def test_rows_at_the_largest_half():
    ng, d, depth = 500, 64, 11
    g, q = _separated(ng, d, 7)
    g[40:60] = np.float16(65504.0)
    g[60:80] = np.float16(-65504.0)
    g[80, ::2] = np.float16(65504.0)
    q = q.copy()
    q[2] = 60000.0
    ids, d64, _ = HR.reference_search64(g, q, depth)
    many, _ = _check(g, q, depth, ref=(ids, d64))
    assert int(many[2].item()) == 0


# ---- non-finite values and masks -----------------------------------------------------------------------------------------------------
def test_non_finite_rows_queries_and_dead_rows():
    ng, d, depth = 4096, 64, 5
    g, q = _separated(ng, d, 64)
    D = SR.distances64(HR.widen(g), q)
    # live rows with a NaN / an inf are never returned and set bit 1
    bad = g.copy()
    nearest = int(np.argmin(D[0]))
    bad[nearest, 3] = np.float16(np.nan)
    bad[77, 0] = np.float16(np.inf)
    many, fallbacks = _check(bad, q, depth)
    assert int(many[2].item()) == 1 and fallbacks == 0
    assert not np.isin(many[0].cpu().numpy(), [nearest, 77]).any()
    # the same rows DEAD, and every other dead row full of NaN: nothing is set, max|g|^2 is not poisoned -- the counter stays 0
    live = MR.make_mask("random_0.5", ng, seed=5)
    live[[nearest, 77]] = False
    poisoned = g.copy()
    poisoned[~live] = np.float16(np.nan)
    many, fallbacks = _check(poisoned, q, depth, live=live)
    assert int(many[2].item()) == 0 and fallbacks == 0
    Dm = D.copy()
    Dm[:, ~live] = np.inf
    assert np.array_equal(many[0].cpu().numpy(), SR.sorted_lists(Dm, depth)[0])
    # a NaN query: a -1 row and bit 2, the other rows unchanged
    clean, _ = _check(g, q, depth)
    qn = q.copy()
    qn[9, 5] = np.nan
    qn[40, 0] = np.inf
    many, fallbacks = _check(g, qn, depth)
    assert int(many[2].item()) == 2 and fallbacks == 0
    keep = np.setdiff1d(np.arange(64), [9, 40])
    assert bool((many[0][[9, 40]] == -1).all()) and bool(torch.isinf(many[1][[9, 40]]).all()) and bool(torch.isinf(many[3][[9, 40]]).all())
    assert torch.equal(many[0][keep], clean[0][keep]) and torch.equal(many[3][keep], clean[3][keep])


@pytest.mark.parametrize("kind", ["all_dead", "one_live", "fewer_than_depth", "garbage_tail"])
def test_masks(kind):
    ng, d, depth = 333, 64, 11
    g, q = _separated(ng, d, 20)
    live = np.zeros(ng, bool)
    if kind == "one_live":
        live[200] = True
    elif kind == "fewer_than_depth":
        live[[5, 31, 32, 100, 332]] = True
    elif kind == "garbage_tail":
        live = MR.make_mask("random_0.5", ng, seed=9)
    words = MR.pack_words(live).copy()
    if kind == "garbage_tail":
        words[-1] |= np.uint32(0xffffffff) << np.uint32(ng % 32)              # bits past n_gallery in the last word
    ids, d32, _ = HR.reference_search_masked(g, q, live, depth)
    many, fallbacks = _check(g, q, depth, live=_t(words.view(np.int32)), ref=(ids, d32.astype(np.float64)))
    assert fallbacks == 0
    n_live = int(live.sum())
    if n_live < depth:
        assert bool((many[0][:, n_live:] == -1).all()) and bool(torch.isinf(many[1][:, n_live:]).all())


def _walk_mask(kind, ng):
    live = np.ones(ng, bool)
    if kind == "first_tiles":
        live[np.arange(ng) % 32 < 16] = False                                # the low half of every mask word: its first tile
    else:
        lo, hi = {"dead_front": (0, ng // 2), "dead_middle": (ng // 4, 3 * ng // 4), "dead_end": (ng // 2, ng)}[kind]
        live[lo:hi] = False
    return live


@pytest.mark.parametrize("ng,d,nq,kind", [(16384, 64, 33, "dead_front"), (16384, 64, 33, "dead_middle"), (16384, 64, 33, "dead_end"),
                                          (16384, 64, 33, "first_tiles"), (8192, 2048, 64, "dead_front")])
def test_the_walk_skips_runs_of_dead_tiles(ng, d, nq, kind):
    """The pass's walk over more than one tile per workgroup.  33 queries are three waves a workgroup and one workgroup a CU: on 256 CUs
    the 1024 tiles of 16 384 rows are 4 per workgroup, so a dead half of the gallery is a run of two dead tiles at the front, in the
    middle or at the end of every workgroup's walk, and `first_tiles` a dead tile between any two live ones.  d = 2048 is the image
    that is reloaded per item behind a barrier, with the front half dead.  NaN stands in the dead rows: it is not read, not returned
    and not flagged.  The data is separated -- the gap between the depth-th and the cdepth-th live distance exceeds 2 eps for every
    query, recomputed here from the reference's fp32 distances, whose rounding (2^-22 of a distance below 4) is allowed for -- so every
    list is certified by the pass itself: the fallback counter is 0."""
    depth, cdepth = 11, 32
    g, q = _separated(ng, d, nq)
    live = _walk_mask(kind, ng)
    g[~live] = np.float16(np.nan)
    ids, d32, ref_gap = HR.reference_search_masked(g, q, live, cdepth, 3)
    assert ref_gap > 1e-12, ref_gap
    gap = (d32[:, cdepth - 1].astype(np.float64) - d32[:, depth - 1].astype(np.float64)).min() - 2.0 ** -21
    gmax = (HR.widen(g[live]).astype(np.float64) ** 2).sum(1).max()
    eps = (KAPPA(d) * ((q.astype(np.float64) ** 2).sum(1) + gmax) + 1e-35).max()
    print(f"{kind} d={d}: smallest gap {gap:.4g}, 2 eps {2 * eps:.4g}")
    assert gap > 2 * eps, (gap, eps)
    many, fallbacks = _check(g, q, depth, live=live, id_base=3, ref=(ids[:, :depth], d32[:, :depth].astype(np.float64)))
    assert fallbacks == 0
    assert int(many[2].item()) == 0


# ---- windows ---------------------------------------------------------------------------------------------------------------------------
def test_three_windows_merge_to_the_whole():
    ops = _ops()
    ng, d, depth, nq = 3000, 192, 11, 33
    g, q = _separated(ng, d, nq)
    g[2500] = g[100]                                                          # a tie across windows
    tg, tq = _t(g), _t(q)
    whole, _ = _check(g, q, depth, id_base=1000)
    parts_i, parts_d = [], []
    for lo, hi in ((0, 900), (900, 2100), (2100, ng)):
        ws = ops.workspace(ops.l2_search_many_workspace_bytes(hi - lo, nq, d, depth), DEV)
        ids, _, _ = ops.l2_search_many(tg[lo:hi], tq, depth, id_base=1000 + lo, ws=ws)
        parts_i.append(ids)
        parts_d.append(ops.search_dists64(ws, nq, depth).clone())
    ids, dists = ops.l2_search_merge(torch.stack(parts_i), torch.stack(parts_d))
    assert torch.equal(ids, whole[0]) and torch.equal(dists, whole[1])


# ---- canaries ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("duplicates", [False, True], ids=["certified", "fallback"])
def test_nothing_outside_the_outputs_and_the_workspace_is_written(duplicates):
    from vtc_amd import _lib as L
    lib = L.lib()
    ng, d, depth, nq, G, guard = 1500, 64, 11, 33, 4, 4096
    g, q = _separated(ng, d, nq)
    live = MR.make_mask("random_0.5", ng, seed=2)
    if duplicates:
        g[1000:1100] = HR.round_half(q[0])
        live[1000:1100] = True
    tg, tq, words = _t(g), _t(q), _words(live)
    before = (tg.clone(), tq.clone(), words.clone())
    need = lib.vtc_l2_search_many_workspace_bytes(ng, nq, d, depth)
    ids = torch.full((G + nq + G, depth), -77, dtype=torch.int64, device=DEV)
    dists = torch.full((G + nq + G, depth), -77.0, dtype=torch.float32, device=DEV)
    ws = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    bits = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(stream):
            rc = lib.vtc_l2_search_many_half(tg.data_ptr(), tq.data_ptr(), words.data_ptr(), ng, nq, d, depth, 0, ids[G].data_ptr(),
                                             dists[G].data_ptr(), bits.data_ptr(), ws.data_ptr() + guard, need, stream.cuda_stream)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert rc == 0, lib.vtc_last_error()
    stream.synchronize()
    want_ids, want_d, _ = HR.reference_search_masked(g, q, live, depth)
    assert np.array_equal(ids[G:G + nq].cpu().numpy(), want_ids)
    SR.assert_dists_within_one_ulp(dists[G:G + nq].cpu().numpy(), want_d)
    assert bool((ids[:G] == -77).all()) and bool((ids[G + nq:] == -77).all())
    assert bool((dists[:G] == -77.0).all()) and bool((dists[G + nq:] == -77.0).all())
    assert bool((ws[:guard] == 0xA5).all()) and bool((ws[guard + need:] == 0xA5).all())
    assert (_ops().search_many_stats(ws[guard:], nq, depth)["fallback_queries"] >= 1) == duplicates
    for x, y in zip(before, (tg, tq, words)):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


# ---- VideoIndex.search_many ----------------------------------------------------------------------------------------------------------
def _index(storage, n=2000, dim=100, duplicates=False):
    from vtc_amd.host.search import VideoIndex
    rng = np.random.default_rng(21)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    if duplicates:
        rows[500:700] = rows[499]
    index = VideoIndex(dim, device=DEV, storage=storage)
    index.add(_t(rows))
    index.remove(torch.arange(0, n, 7))
    return index, rows


def test_index_search_many_equals_search_without_a_sync():
    from vtc_amd import _lib as L
    lib = L.lib()
    index, rows = _index(torch.float16)
    q = np.random.default_rng(22).standard_normal((70, 100)).astype(np.float32)
    q[13, 4] = np.nan
    flags = torch.zeros(index.ntotal, dtype=torch.bool, device=DEV)
    flags[::3] = True
    subset = index.subset(flags)
    tq = _t(q)
    want = index.search(tq, 11, subset=subset)
    index.search_many(tq, 11, subset=subset)                                 # (warm: workspace allocated, subset words packed)
    torch.cuda.synchronize()
    c0 = lib.vtc_debug_launch_count()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = index.search_many(tq, 11, subset=subset)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    launches = lib.vtc_debug_launch_count() - c0
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool((got[0][13] == -1).all()) and bool(torch.isneginf(got[1][13]).all())
    assert torch.equal(index.search_many(tq, 11)[0], index.search(tq, 11)[0])
    # the launches do not depend on the data: an index full of duplicates, whose queries go to the fallback
    dup_index, dup_rows = _index(torch.float16, duplicates=True)
    dq = _t(np.concatenate([dup_rows[499:500] + 0.01 * q[:1], q[1:]]))
    dup_subset = dup_index.subset(torch.ones(dup_index.ntotal, dtype=torch.bool, device=DEV))
    want = dup_index.search(dq, 11, subset=dup_subset)
    dup_index.search_many(dq, 11, subset=dup_subset)
    c0 = lib.vtc_debug_launch_count()
    got = dup_index.search_many(dq, 11, subset=dup_subset)
    assert lib.vtc_debug_launch_count() - c0 == launches
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert bool(((got[0][0] >= 499) & (got[0][0] < 700)).all())              # query 0's neighbours are the duplicates: it took the fallback


def test_index_search_many_is_search_elsewhere():
    """An fp32 index, k = 40 on a half index, and fewer queries than the routing constant: the call IS search -- the same launches, the
    same result, nothing of the new entry runs."""
    from vtc_amd import _lib as L
    from vtc_amd.host.search import VideoIndex
    lib = L.lib()
    q = _t(np.random.default_rng(23).standard_normal((20, 100)).astype(np.float32))
    few = q[:max(VideoIndex.ROUTE_MANY_MIN_QUERIES - 1, 1)]
    for storage, queries, k in ((torch.float32, q, 11), (torch.float16, q, 40), (torch.float16, few, 11)):
        if storage == torch.float16 and k == 11 and VideoIndex.ROUTE_MANY_MIN_QUERIES <= 1:
            continue
        index, _ = _index(storage)
        want = index.search(queries, k)
        c0 = lib.vtc_debug_launch_count()
        want = index.search(queries, k)
        search_launches = lib.vtc_debug_launch_count() - c0
        c0 = lib.vtc_debug_launch_count()
        got = index.search_many(queries, k)
        assert lib.vtc_debug_launch_count() - c0 == search_launches
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_an_fp32_gallery_is_refused_by_the_wrapper():
    g, q = _separated(100, 64, 4)
    with pytest.raises(ValueError, match="float16"):
        _ops().l2_search_many(_t(HR.widen(g)), _t(q), 5)
