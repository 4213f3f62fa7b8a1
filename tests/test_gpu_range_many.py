"""GPU: the many-query count pass of the range search over a half gallery (vtc_l2_range_count_many_half; ops.l2_range_count_many /
l2_range_search_many; VideoIndex.range_search_many / range_count_many / similar_within / near_duplicates).  Its definition is
"vtc_l2_range_count(gallery, half, ...), bit for bit", so the first oracle is ops.l2_range_count / ops.l2_range_search on the same half
gallery -- torch.equal on lims, the hit words, the non-finite word and, after the fill on the new entry's workspace, ids, fp32 dists and
fp64 dists -- and the second the numpy fp64 reference over the widened rows (tests/search_range_refs.py), with radii from midpoint_radii
so that no distance is near a radius (min_margin > 1e-12 is asserted).  ops.range_many_stats tells the MFMA route from a scan in
disguise: the number of pairs decided by their fp64 distance is 0 on separated data and at least the number of planted ties elsewhere.

KAPPA below is the bound search_many.hip derives and range_many.hip applies per pair: |A - D| <= KAPPA(d) (|q|^2 + |g|^2) + 1e-35."""
import numpy as np
import pytest
import torch

import search_half_refs as HR
import search_mask_refs as MR
import search_range_refs as RR
import search_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ID_BASE = 2 ** 33 + 5


def KAPPA(d):
    return (6 * d + 8) * 2.0 ** -24 + 2.0 ** -20


def _ops():
    from vtc_amd import ops
    return ops


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _words(live):
    return None if live is None else _t(MR.pack_words(live).view(np.int32))


def _separated(ng, d, nq, seed=7):
    """Seeded unit-norm gaussian rows rounded to half, unit-norm gaussian queries (test_gpu_search_many.py's)."""
    rng = np.random.default_rng(seed)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return HR.round_half(unit(rng.standard_normal((ng, d)))), unit(rng.standard_normal((nq, d)))


def _run(many, th, tq, r2, words, id_base, fill):
    """{lims, bits, words[, ids, d32, d64][, exact_pairs]} of one entry, each call in a workspace of its own."""
    ops = _ops()
    (ng, d), nq = th.shape, tq.shape[0]
    size = ops.l2_range_many_workspace_bytes if many else ops.l2_range_workspace_bytes
    count = ops.l2_range_count_many if many else ops.l2_range_count
    search = ops.l2_range_search_many if many else ops.l2_range_search
    ws = ops.workspace(size(ng, nq, d), DEV)
    ws.fill_(0xA5)                                             # the workspace is not cleared by the call: zero words must be written
    lims, bits = count(th, tq, r2, live=words, ws=ws, return_bits=True)
    out = {"lims": lims, "bits": bits, "words": ops.range_hit_words(ws, ng, nq).clone()}
    if many:
        out["exact_pairs"] = ops.range_many_stats(ws, ng, nq)["exact_pairs"]
        assert out["exact_pairs"] == ops.range_many_stats(ws, ng, nq, d)["exact_pairs"]
    if fill:
        lims2, ids, d32, d64, words2 = search(th, tq, r2, live=words, id_base=id_base, max_results=1 << 26, return_dists64=True,
                                              return_words=True, ws=ws)
        assert torch.equal(lims2, lims) and torch.equal(words2, out["words"])
        out.update(ids=ids, d32=d32, d64=d64)
    return out


def _check(g, q, r2, live=None, id_base=0, fill=True, ref=True, D=None):
    """Both oracles.  ``D``: the fp64 distance matrix of (g, q), when the caller has it.  Returns (the new entry's outputs, the
    reference's (lims, ids, d64, member, margin) or None)."""
    th, tq = (g if isinstance(g, torch.Tensor) else _t(g)), (q if isinstance(q, torch.Tensor) else _t(q))
    words = _words(live)
    r2 = np.asarray(r2, np.float64)
    many, scan = _run(True, th, tq, r2, words, id_base, fill), _run(False, th, tq, r2, words, id_base, fill)
    for key, want in scan.items():
        assert many[key].dtype == want.dtype and torch.equal(many[key], want), (key, many[key], want)
    nq, ng = tq.shape[0], th.shape[0]
    assert 0 <= many["exact_pairs"] <= nq * ng
    want = None
    if ref:
        want = RR.range_lists(D if D is not None else SR.distances64(HR.widen(th.cpu().numpy()), tq.cpu().numpy()), r2, live, id_base)
        assert want[4] > 1e-12, want[4]
        assert np.array_equal(many["lims"].cpu().numpy(), want[0])
        got_words = many["words"].cpu().numpy().view(np.uint32)
        for u in range(nq):
            assert np.array_equal(got_words[u], MR.pack_words(want[3][u])), u
        if fill:
            assert np.array_equal(many["ids"].cpu().numpy(), want[1])
            np.testing.assert_allclose(many["d64"].cpu().numpy(), want[2], rtol=1e-12, atol=1e-30)
    return many, want


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 192, 512, 2048])
@pytest.mark.parametrize("ng", [1, 31, 32, 33, 63, 64, 65, 257, 5000])
def test_shapes(d, ng):
    """Every n_queries in {1, 7, 16, 17, 33, 64}: one wave and four, a group of 16 that is full, one that holds a single query.  The
    gallery sizes are a last word partly inside the gallery, a word whose second tile lies past the end, and (5000 rows = 157 words,
    at most 40 workgroups) more than one unit per workgroup; d = 2048 is a row longer than the resident image.  Galleries of 16 rows
    and more hold search_half_refs.special_rows.  The per-query counts mix 0, 1, a few and all; the radii of four query slots are
    0.0, negative, NaN and +inf.  One distance matrix per gallery."""
    g, q = HR.half_pairs(max(ng, 64), d, HR.SEED + d)
    g = HR.special_rows(g[:ng], seed=d) if ng >= 16 else g[:ng]
    q = q[:64]
    D = SR.distances64(HR.widen(g), q)
    live = MR.make_mask("alt_bits", ng) if ng >= 33 else None
    counts = np.array([(0, 1, 3, ng, 2, 7, ng // 2, 1)[u % 8] for u in range(64)])
    tg = _t(g)
    for nq in (1, 7, 16, 17, 33, 64):
        for mask in (None, live) if nq in (7, 17, 64) and live is not None else (None,):
            r2 = RR.midpoint_radii(D[:nq], counts[:nq] if nq > 1 else [min(3, ng)], mask)
            if nq >= 7:
                r2[2], r2[3], r2[4], r2[5] = 0.0, -1.0, np.nan, np.inf
            many, want = _check(tg, q[:nq], r2, live=mask, id_base=ID_BASE, D=D[:nq])
            sizes = np.diff(want[0])
            if nq >= 7:
                assert sizes[3] == 0 and sizes[4] == 0 and sizes[5] == (ng if mask is None else int(mask.sum()))
            if nq == 64 and mask is None and ng >= 8:
                assert sizes[0] == 0 and sizes[1] >= 1 and sizes[11] == ng


# ---- the MFMA route is taken -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 512])
def test_separated_data_is_decided_without_an_exact_pair(d):
    """4096 unit rows, 64 unit queries; the radius of a query is the midpoint of the widest gap among its first 24 sorted fp64
    distances.  That gap exceeds 2 eps for every query (recomputed here, not assumed: 204 x at d = 64, 7.7 x at d = 512; d = 2048
    reaches only 1.26 x and is left out), so no pair lies in the band: the counter of exact pairs is 0, unmasked and under a mask."""
    ng, nq = 4096, 64
    g, q = _separated(ng, d, nq)
    D = SR.distances64(HR.widen(g), q)
    gmax = (HR.widen(g).astype(np.float64) ** 2).sum(1).max()
    eps = KAPPA(d) * ((q.astype(np.float64) ** 2).sum(1) + gmax) + 1e-35
    for live in (None, MR.make_mask("random_0.5", ng, seed=3)):
        Dl = D if live is None else D[:, live]
        srt = np.sort(Dl, axis=1)[:, :24]
        at = np.argmax(np.diff(srt, axis=1), axis=1)
        gap = srt[np.arange(nq), at + 1] - srt[np.arange(nq), at]
        print(f"d={d} masked={live is not None}: smallest gap / 2 eps = {(gap / (2 * eps)).min():.4g}")
        assert (gap > 2 * eps).all(), (gap / (2 * eps)).min()
        r2 = (srt[np.arange(nq), at + 1] + srt[np.arange(nq), at]) / 2
        many, want = _check(g, q, r2, live=live, D=D)
        assert np.array_equal(np.diff(want[0]), at + 1)
        assert many["exact_pairs"] == 0


# ---- the band is decided exactly -------------------------------------------------------------------------------------------------------
def test_the_band_is_decided_by_the_fp64_distance():
    """Queries that are widened half rows, 100 bit-equal copies of query 0's row in the gallery at high row indices.  Radius 0.0: the
    hits are exactly the copies, and every one of them was a band pair.  Then the radius is the fp64 distance the scan's fill returned
    for a query's c-th hit -- that row is a hit -- and the next double below it -- that row is not: both as the scan decides."""
    ng, d, nq = 3000, 64, 20
    g, _ = _separated(ng, d, 1)
    q = HR.widen(g[:nq]).copy()
    dup = np.sort(np.random.default_rng(1).choice(np.arange(1500, ng), 100, replace=False))
    g[dup] = g[0]
    many, _ = _check(g, q, np.zeros(nq), id_base=7, ref=False)      # (no reference: a radius that IS a distance has no margin)
    assert np.array_equal(many["ids"][:many["lims"][1]].cpu().numpy(), 7 + np.concatenate([[0], dup]))
    assert np.array_equal(np.diff(many["lims"].cpu().numpy())[1:], np.ones(nq - 1))      # every other query: its own row
    assert many["exact_pairs"] >= 100
    # a radius that is a distance of another row: nothing may decide it but the scan's own bits
    D = SR.distances64(HR.widen(g), q)
    wide, _ = _check(g, q, np.sort(D, axis=1)[:, 40] * 1.000001, ref=False)
    lims, d64 = wide["lims"].cpu().numpy(), wide["d64"].cpu().numpy()
    on = np.array([np.sort(d64[lims[u]:lims[u + 1]])[(5 + u) % 30] for u in range(nq)])
    hit, _ = _check(g, q, on, ref=False)
    miss, _ = _check(g, q, np.nextafter(on, -np.inf), ref=False)
    n_on, n_below = np.diff(hit["lims"].cpu().numpy()), np.diff(miss["lims"].cpu().numpy())
    for u in range(nq):
        seg = d64[lims[u]:lims[u + 1]]
        assert n_on[u] == (seg <= on[u]).sum() and n_below[u] == (seg < on[u]).sum() and n_on[u] > n_below[u], u
    assert hit["exact_pairs"] >= nq and miss["exact_pairs"] >= nq


# ---- masks ----------------------------------------------------------------------------------------------------------------------------
def _dead_run(ng, lo, hi):
    live = np.ones(ng, bool)
    live[lo:hi] = False
    return live


@pytest.mark.parametrize("kind", ["random_0.5", "dead_front", "dead_middle", "dead_end", "none", "dead_front_d2048", "dead_middle_d2048",
                                  "first_tiles"])
def test_masks(kind):
    """A run of wholly dead words at the front, in the middle and at the end, a random half, every row dead; the runs at the front and in
    the middle also at d = 2048, where the image is reloaded per item behind a barrier; `first_tiles`: the low half of every word
    dead, a live word whose first tile is skipped.  NaN stands in the dead rows: it is not read, not a hit and not flagged."""
    ng, d, nq = 1333, 2048 if kind.endswith("_d2048") else 64, 33
    kind = kind.replace("_d2048", "")
    g, q = _separated(ng, d, nq)
    live = {"dead_front": _dead_run(ng, 0, 200), "dead_middle": _dead_run(ng, 500, 900), "dead_end": _dead_run(ng, 1000, ng),
            "first_tiles": np.arange(ng) % 32 >= 16}.get(kind)
    if live is None:
        live = MR.make_mask(kind, ng, seed=4)
    g[~live] = np.float16(np.nan)
    D = SR.distances64(HR.widen(g), q)
    counts = np.array([(0, 1, 5, ng, 40)[u % 5] for u in range(nq)])
    many, want = _check(g, q, RR.midpoint_radii(D, counts, live), live=live, id_base=ID_BASE, D=D)
    assert int(many["bits"]) == 0
    if kind == "none":
        assert not many["lims"].any() and not many["words"].any()
    else:
        assert np.array_equal(np.diff(want[0])[:5], [0, 1, 5, live.sum(), 40])


def test_nothing_outside_the_workspace_is_written_and_nothing_syncs():
    from vtc_amd import _lib as L
    lib = L.lib()
    ng, d, nq, guard = 1500, 64, 33, 4096
    g, q = _separated(ng, d, nq)
    live = MR.make_mask("random_0.5", ng, seed=2)
    D = SR.distances64(HR.widen(g), q)
    r2 = RR.midpoint_radii(D, np.arange(nq), live)
    tg, tq, words, tr = _t(g), _t(q), _words(live), _t(r2)
    before = [x.clone() for x in (tg, tq, words, tr)]
    need = lib.vtc_l2_range_many_workspace_bytes(ng, nq, d)
    assert need >= lib.vtc_l2_range_workspace_bytes(ng, nq, d) > 0
    lims = torch.full((4 + nq + 1 + 4,), -77, dtype=torch.int64, device=DEV)
    ws = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    bits = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(stream):
            rc = lib.vtc_l2_range_count_many_half(tg.data_ptr(), tq.data_ptr(), words.data_ptr(), tr.data_ptr(), ng, nq, d, lims[4:].data_ptr(),
                                                  bits.data_ptr(), ws.data_ptr() + guard, need, stream.cuda_stream)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert rc == 0, lib.vtc_last_error()
    stream.synchronize()
    want = RR.reference_range(HR.widen(g), q, r2, live)
    assert want[4] > 1e-12
    assert np.array_equal(lims[4:4 + nq + 1].cpu().numpy(), want[0])
    assert bool((lims[:4] == -77).all()) and bool((lims[4 + nq + 1:] == -77).all())
    assert bool((ws[:guard] == 0xA5).all()) and bool((ws[guard + need:] == 0xA5).all())
    for x, y in zip(before, (tg, tq, words, tr)):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


# ---- non-finite values and range --------------------------------------------------------------------------------------------------------
def test_non_finite_queries_and_rows():
    ng, d, nq = 700, 64, 18
    g, q = _separated(ng, d, nq)
    D = SR.distances64(HR.widen(g), q)
    r2 = RR.midpoint_radii(D, np.full(nq, 9))
    clean, _ = _check(g, q, r2)
    assert int(clean["bits"]) == 0
    qn = q.copy()
    qn[5, 17] = np.nan
    qn[17, 0] = np.inf
    many, _ = _check(g, qn, r2)
    sizes = np.diff(many["lims"].cpu().numpy())
    assert int(many["bits"]) == 2 and sizes[5] == 0 and sizes[17] == 0 and (np.delete(sizes, [5, 17]) == 9).all()
    gi = g.copy()
    row = int(np.argmin(D[3]))                                  # query 3's nearest row: an inf in it, it is never a hit
    gi[row, 40] = np.float16(np.inf)
    many, _ = _check(gi, q, np.where(np.arange(nq) == 4, np.inf, r2))
    sizes = np.diff(many["lims"].cpu().numpy())
    assert int(many["bits"]) == 1 and sizes[3] == 8 and sizes[4] == ng - 1
    others = [u for u in range(nq) if u != 4 and D[u, row] > r2[u]]      # the queries the row was no hit of: unchanged
    assert len(others) >= nq - 3 and torch.equal(many["words"][others], clean["words"][others])
    live = np.ones(ng, bool)
    live[row] = False                                            # ... and dead, it is not even flagged
    many, _ = _check(gi, q, r2, live=live)
    assert int(many["bits"]) == 0


@pytest.mark.parametrize("scale", [2.0 ** -120, 2.0 ** 100, 2.0 ** 62])
def test_queries_outside_the_range_of_the_split(scale):
    """Queries scaled by 2^-120 take QF_FALLBACK: every pair is decided exactly.  Scaled by 2^100, |q|^2 overflows fp32 and A is not
    finite: the pairs go to the band.  2^62: finite and large.  The result is the scan's, whose fp64 distances do not overflow."""
    ng, d, nq = 300, 64, 17
    g, q = _separated(ng, d, nq)
    qs = (q.astype(np.float64) * scale).astype(np.float32)
    qs[0] = q[0]                                                 # one ordinary query among them
    D = SR.distances64(HR.widen(g), qs)
    if scale < 1:
        r2 = RR.midpoint_radii(D, np.array([(0, 1, 6, ng)[u % 4] for u in range(nq)]))
        many, _ = _check(g, qs, r2, D=D)
    else:
        # the distances of a huge query differ in their last fp64 bits at the most: no radius has a margin, so the scan is the only
        # oracle, on radii that ARE distances (each query's median, in the bits the fill of a +inf pass returned), 0 and +inf
        every, _ = _check(g, qs, np.full(nq, np.inf), ref=False)
        assert (np.diff(every["lims"].cpu().numpy()) == ng).all()
        median = np.sort(every["d64"].cpu().numpy().reshape(nq, ng), axis=1)[:, ng // 2]
        r2 = np.where(np.arange(nq) % 3 == 0, median, np.where(np.arange(nq) % 3 == 1, 0.0, np.inf))
        many, _ = _check(g, qs, r2, ref=False)
        sizes = np.diff(many["lims"].cpu().numpy())
        assert (sizes[1::3] == 0).all() and (sizes[2::3] == ng).all() and (sizes[3::3] > ng // 2).all()
    if scale != 2.0 ** 62:
        assert many["exact_pairs"] >= (nq - 1) * ng


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_give_an_error():
    from vtc_amd import _lib as L
    lib = L.lib()
    ops = _ops()
    ng, nq = 100, 4
    g, q = _separated(ng, 64, nq)
    with pytest.raises(ValueError, match="float16"):
        ops.l2_range_count_many(_t(HR.widen(g)), _t(q), 1.0)
    with pytest.raises(ValueError, match="float16"):
        ops.l2_range_search_many(_t(HR.widen(g)), _t(q), 1.0)
    assert lib.vtc_l2_range_many_workspace_bytes(ng, 65, 64) == 0 and lib.vtc_l2_range_many_workspace_bytes(ng, nq, 96) == 0
    assert lib.vtc_l2_range_many_workspace_bytes(0, nq, 64) == 0 and lib.vtc_l2_range_many_workspace_bytes(ng, 0, 64) == 0
    tg = _t(np.zeros((ng, 128), np.float16))
    tq = _t(np.zeros((65, 128), np.float32))
    r2 = torch.ones(65, dtype=torch.float64, device=DEV)
    lims = torch.full((66,), -77, dtype=torch.int64, device=DEV)
    ws = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device=DEV)
    need = lib.vtc_l2_range_many_workspace_bytes(ng, nq, 64)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for what, n_q, d, ws_bytes in (("65 queries", 65, 64, 1 << 20), ("d = 96", nq, 96, 1 << 20), ("a short workspace", nq, 64, need - 1)):
        rc = lib.vtc_l2_range_count_many_half(tg.data_ptr(), tq.data_ptr(), None, r2.data_ptr(), ng, n_q, d, lims.data_ptr(), None,
                                              ws.data_ptr(), ws_bytes, stream)
        assert rc != 0 and lib.vtc_last_error(), what
    torch.cuda.synchronize()
    assert bool((lims == -77).all()) and bool((ws == 0xA5).all())          # nothing was launched
    rc = lib.vtc_l2_range_count_many_half(tg.data_ptr(), tq.data_ptr(), None, r2.data_ptr(), ng, nq, 64, lims.data_ptr(), None, ws.data_ptr(),
                                          need, stream)
    assert rc == 0, lib.vtc_last_error()


# ---- VideoIndex -------------------------------------------------------------------------------------------------------------------------
def _index(storage, n=2000, dim=100):
    from vtc_amd.host.search import VideoIndex
    rows = np.random.default_rng(21).standard_normal((n, dim)).astype(np.float32)
    index = VideoIndex(dim, device=DEV, storage=storage)
    index.ROUTE_RANGE_MANY_MIN_QUERIES = 9                      # the route under test, whatever the measured constant says
    index.add(_t(rows))
    index.remove(torch.arange(0, n, 7))
    return index


def _index_queries(index, nq=130):
    """130 queries -- two full slices and a remainder of 2 -- each near a stored row, a threshold per query, one query with a NaN."""
    rng = np.random.default_rng(22)
    base = index.rows[:, :index.dim].float().cpu().numpy()[rng.integers(0, index.ntotal, nq)]
    q = (base + 0.08 * rng.standard_normal(base.shape)).astype(np.float32)
    if nq > 13:
        q[13, 4] = np.nan
    return _t(q), [(0.2, 0.05, 0.5, -1.0, 0.3)[u % 5] for u in range(nq)]


def test_index_range_many_equals_range_search():
    ops = _ops()
    index = _index(torch.float16)
    tq, min_score = _index_queries(index)
    flags = torch.ones(index.ntotal, dtype=torch.bool, device=DEV)
    flags[::3] = False
    subset = index.subset(flags)
    for sub in (subset, None):
        want_n = index.range_count(tq, min_score, subset=sub)
        index.range_count_many(tq, min_score, subset=sub)                      # (warm: the workspace allocated, the words packed)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got_n = index.range_count_many(tq, min_score, subset=sub)          # only enqueued
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(got_n, want_n) and int(got_n[13]) == 0 and int(got_n[3]) == (len(index) if sub is None else int(got_n[3]))
        for sort in (True, False):
            want = index.range_search(tq, min_score, subset=sub, sort=sort)
            got = index.range_search_many(tq, min_score, subset=sub, sort=sort)
            assert all(torch.equal(x, y) for x, y in zip(got, want)) and got[1].numel() > 130
            assert torch.equal(got[0][1:] - got[0][:-1], want_n)
    # the route is the new entry: its counter, poisoned before the call, is fresh after it
    n_last = tq.shape[0] % 64
    at = ops.l2_range_workspace_bytes(index.ntotal, n_last, index.width) + 64 * index.width + 768
    index._ws[at:at + 8] = 0xA5
    index.range_count_many(tq, min_score)
    assert 0 <= ops.range_many_stats(index._ws, index.ntotal, n_last, index.width)["exact_pairs"] <= n_last * index.ntotal
    with pytest.raises(ValueError, match="max_results"):
        index.range_search_many(tq, min_score, max_results=100)


def test_index_range_many_is_range_search_elsewhere():
    """An fp32 index, fewer queries than the routing constant on a half index, and a constant of 65 (never): the call IS range_search /
    range_count -- the same launches, the same result."""
    from vtc_amd import _lib as L
    lib = L.lib()
    for storage, nq, least in ((torch.float32, 70, 9), (torch.float16, 8, 9), (torch.float16, 70, 65)):      # 65: never
        index = _index(storage)
        index.ROUTE_RANGE_MANY_MIN_QUERIES = least
        tq, min_score = _index_queries(index, nq)
        want = index.range_search(tq, min_score)
        c0 = lib.vtc_debug_launch_count()
        want = index.range_search(tq, min_score)
        launches = lib.vtc_debug_launch_count() - c0
        c0 = lib.vtc_debug_launch_count()
        got = index.range_search_many(tq, min_score)
        assert lib.vtc_debug_launch_count() - c0 == launches
        assert all(torch.equal(x, y) for x, y in zip(got, want))
        assert torch.equal(index.range_count_many(tq, min_score), index.range_count(tq, min_score))


@pytest.fixture(scope="module")
def planted():
    """600 rows of 96 dimensions with planted bit-equal copies and near-duplicates at several distances; rows 100 .. 104 removed.  The
    brute force is numpy fp64 over the STORED half rows: S[a, b] = 1 - |a - b|^2 / 2."""
    n, dim = 600, 96
    rng = np.random.default_rng(31)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    for k in range(40):                                          # near-duplicates of rows 0 .. 39 at rows 300 .. 339, ever noisier
        rows[300 + k] = rows[k] + (0.01 + 0.012 * k) * rng.standard_normal(dim)
    rows[400:403] = rows[50]                                     # three copies of row 50 (bit-equal after the same rounding)
    rows[404] = rows[303]                                        # a copy of a near-duplicate: a cluster of three
    rows[450] = rows[101]                                        # a copy of a row that is removed
    return rows


def _planted_index(planted, storage):
    from vtc_amd.host.search import VideoIndex
    index = VideoIndex(planted.shape[1], device=DEV, storage=storage)
    index.ROUTE_RANGE_MANY_MIN_QUERIES = 9
    index.NEAR_DUPLICATES_SLICE = 256                            # three slices of rows
    index.add(_t(planted))
    index.remove(torch.arange(100, 105))
    stored = index.rows.float().cpu().numpy()
    return index, 1.0 - SR.distances64(stored, stored) / 2.0


@pytest.mark.parametrize("storage", [torch.float16, torch.float32], ids=["half", "fp32"])
def test_similar_within_and_near_duplicates_against_brute_force(planted, storage):
    index, S = _planted_index(planted, storage)
    n, min_score = index.ntotal, 0.95                           # the planted near-duplicates fall on both sides of it
    assert np.abs(S - min_score).min() > 1e-12
    live = np.ones(n, bool)
    live[100:105] = False
    member = live.copy()
    member[::5] = False
    member[[0, 300, 50, 400, 401]] = True
    subset = index.subset(_t(member))
    for sub, part in ((None, live), (subset, member)):
        # ---- similar_within: stored rows as queries -- a removed one, one outside the subset, ids outside the index
        ids = np.concatenate([np.arange(0, 60), [400, 401, 402, 404, 303, 450, 101, 5, -1, n, n + 7], np.arange(290, 345)])
        for sort in (True, False):
            lims, hit, score = (x.cpu().numpy() for x in index.similar_within(_t(ids.astype(np.int64)), min_score, subset=sub, sort=sort))
            assert lims[0] == 0 and lims[-1] == hit.size == score.size
            for u, a in enumerate(ids):
                got, got_s = hit[lims[u]:lims[u + 1]], score[lims[u]:lims[u + 1]]
                if not 0 <= a < n:
                    assert got.size == 0                        # an id outside the index: an empty segment
                    continue
                want = np.flatnonzero(part & (S[a] >= min_score) & (np.arange(n) != a))          # self excluded, live members only
                if sort:                                        # nearest first, bit-equal copies by ascending row
                    want = want[np.lexsort((want, -S[a, want]))]
                    assert (np.diff(got_s) <= 0).all()
                assert np.array_equal(got, want), (a, got, want)
                np.testing.assert_allclose(np.sort(got_s), np.sort(S[a, want]), atol=2e-6)
            at = {int(a): u for u, a in enumerate(ids)}
            copies = hit[lims[at[50]]:lims[at[50] + 1]]
            assert {400, 401} <= set(copies.tolist()) and 50 not in copies      # bit-equal copies are other rows, and are returned
            assert 101 not in hit[lims[at[450]]:lims[at[450] + 1]]              # a removed row is absent
        # ---- near_duplicates: every unordered pair, ascending by (a, b)
        pairs, score = (x.cpu().numpy() for x in index.near_duplicates(min_score, subset=sub))
        a, b = np.nonzero(np.triu(S >= min_score, 1) & part[:, None] & part[None, :])
        assert pairs.shape == (a.size, 2) and a.size >= (30 if sub is None else 5)
        assert np.array_equal(pairs[:, 0], a) and np.array_equal(pairs[:, 1], b) and (pairs[:, 0] < pairs[:, 1]).all()
        np.testing.assert_allclose(score, S[a, b], atol=2e-6)
        with pytest.raises(ValueError, match="max_results"):
            index.near_duplicates(min_score, subset=sub, max_results=a.size - 1)
        assert index.near_duplicates(min_score, subset=sub, max_results=a.size)[0].shape[0] == a.size
