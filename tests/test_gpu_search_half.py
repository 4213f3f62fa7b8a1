"""GPU: the query-time search over a gallery stored as IEEE binary16 (vtc_l2_search_half; ops.l2_search* with a torch.float16 gallery;
VideoIndex(storage=torch.float16)).  Two oracles, both independent of the new code:

  (A) the fp32 entry points over gallery.float() -- ops.l2_search / l2_search_grouped with the same mask --, compared with torch.equal
      on ids, fp32 dists, groups, the non-finite word and the fp64 distances of the workspace: binary16 -> fp32 is exact, so the half
      scan must form the same bits (a flushed subnormal or a reordered sum would not);
  (B) the numpy fp64 reference over the widened rows (tests/search_half_refs.py): ids where min_gap > 1e-12 (asserted; the same shapes
      are checked on the CPU in tests/test_search_half_refs.py), fp32 dists within one ulp."""
from dataclasses import asdict

import numpy as np
import pytest
import torch

import search_grouped_refs as GR
import search_half_refs as HR
import search_mask_refs as MR
import search_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN16 = np.float16(np.nan)


def _ops():
    from vtc_amd import ops
    return ops


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _words(live):
    return None if live is None else _t(MR.pack_words(live).view(np.int32))


def _both(g_half, q, depth, live=None, groups=None, id_base=0, g_wide=None):
    """The half search and oracle (A), each in a workspace of its own: ((ids, [groups,] dists, bits, dists64) half, the same fp32).
    `g_wide`: what the fp32 entry reads (default: the widened half gallery)."""
    ops = _ops()
    th, tq = (g_half if isinstance(g_half, torch.Tensor) else _t(g_half)), (q if isinstance(q, torch.Tensor) else _t(q))
    tw = th.float() if g_wide is None else g_wide
    assert th.dtype == torch.float16 and tw.dtype == torch.float32
    ng, d = th.shape
    nq = tq.shape[0]
    words = live if isinstance(live, torch.Tensor) or live is None else _words(live)
    out = []
    for g in (th, tw):
        if groups is None:
            ws = ops.workspace(ops.l2_search_workspace_bytes(ng, nq, d, depth), DEV)
            res = ops.l2_search(g, tq, depth, id_base=id_base, ws=ws, live=words)
        else:
            ws = ops.workspace(ops.l2_search_grouped_workspace_bytes(ng, nq, d, depth), DEV)
            res = ops.l2_search_grouped(g, tq, _t(groups), depth, id_base=id_base, ws=ws, live=words)
        out.append(tuple(res) + (ops.search_dists64(ws, nq, depth).clone(),))
    return out


def _assert_same_bits(half, wide):
    assert len(half) == len(wide)
    for x, y in zip(half, wide):
        assert x.dtype == y.dtype and torch.equal(x, y), (x, y)


def _check(g_half, q, depth, live=None, groups=None, id_base=0, want_bits=0):
    """Both oracles on one search; returns the half result."""
    half, wide = _both(g_half, q, depth, live, groups, id_base)
    _assert_same_bits(half, wide)                                                               # (A)
    alive = np.ones(len(g_half), bool) if live is None else np.asarray(live, bool)
    if groups is None:
        ids, d32, gap = HR.reference_search_masked(g_half, q, alive, depth, id_base)            # (B)
    else:
        ids, grp, d64, gap = HR.reference_search_grouped64(g_half, q, groups, depth, alive, id_base)
        d32 = d64.astype(np.float32)
        assert np.array_equal(half[1].cpu().numpy(), grp)
    assert gap > 1e-12, gap
    assert np.array_equal(half[0].cpu().numpy(), ids)
    SR.assert_dists_within_one_ulp(half[-3].cpu().numpy(), d32)
    assert int(half[-2].item()) == want_bits
    return half


# ---- shapes: every width class, tile shape and depth ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ng,nq,depth", HR.SHAPES)
def test_shapes_and_special_values(d, ng, nq, depth):
    """Galleries of 16 rows and more hold the special rows of search_half_refs.special_rows: subnormal halves, +-65504, -0.0, exact
    duplicates, rows that differ below the fp32 resolution of their distance.  id_base > 2^32."""
    g, q = HR.shape_case(d, ng, nq, depth)
    _check(g, q, depth, id_base=2 ** 33 + 5)
    if ng >= 33:
        _check(g, q, min(depth, ng), live=MR.make_mask("alt_bits", ng))
        _check(g, q, depth, groups=GR.make_groups("strided", ng), id_base=3)


def test_a_gallery_larger_than_one_pass_of_the_grid():
    """40 003 rows at d = 64 (search_half_refs.large_case): every wave takes several steps and the last one is partial."""
    g, q = HR.large_case()
    ng = g.shape[0]
    for nq in (1, 2, 4, 9):
        half = _check(g, q[:nq], 11)
        assert int(half[0][0, 0]) == ng - 1
    _check(g, q[:2], 11, live=MR.make_mask("random_0.5", ng, seed=2) | (np.arange(ng) == ng - 1), groups=j_div(ng, 5))


def test_subnormals_are_not_flushed_and_ties_go_to_the_lower_row():
    """The planted rows by name: rows 9 / 10 differ by 2^-24 in one component -- their fp64 distances differ, their fp32 ones do not;
    rows 3 .. 6 are bit-equal and come back in row order."""
    g, q = HR.shape_case(512, 33, 4, 33)
    half, wide = _both(g, q, 33, id_base=2 ** 33)
    _assert_same_bits(half, wide)
    ids, d64 = half[0].cpu().numpy() - 2 ** 33, half[3].cpu().numpy()
    D = SR.distances64(HR.widen(g), q)
    for i in range(4):
        pos = {int(r): int(np.flatnonzero(ids[i] == r)[0]) for r in (3, 4, 5, 6, 9, 10)}
        assert [pos[r] for r in (3, 4, 5, 6)] == list(range(pos[3], pos[3] + 4))
        assert d64[i, pos[9]] != d64[i, pos[10]] and abs(d64[i, pos[9]] - d64[i, pos[10]]) < 1e-7 * d64[i, pos[9]]
        assert (d64[i, pos[9]] < d64[i, pos[10]]) == (D[i, 9] < D[i, 10]) and abs(pos[9] - pos[10]) == 1
    # a gallery of nothing but subnormals and zeros: the distance is |q|^2 minus terms of 1e-5 .. 1e-8 relative
    rng = np.random.default_rng(8)
    tiny = (rng.integers(-1023, 1024, (40, 64)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float16)
    assert np.all(np.abs(tiny.astype(np.float32)) < 2.0 ** -14) and np.array_equal(tiny.astype(np.float32) * 2.0 ** 24, np.round(tiny.astype(np.float32) * 2.0 ** 24))
    half, wide = _both(tiny, q[:3, :64].copy(), 40)
    _assert_same_bits(half, wide)
    want = SR.reference_search64(HR.widen(tiny), q[:3, :64], 40)
    assert len(np.unique(half[3].cpu().numpy()[0])) > 30      # flushed, all forty distances would be |q|^2
    if want[2] > 1e-12:
        assert np.array_equal(half[0].cpu().numpy(), want[0])


# ---- non-finite ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 4, 9])
def test_nonfinite_half_rows_and_queries(nq):
    g, q = HR.shape_case(64, 257, 9, 11)
    q = q[:nq].copy()
    bad = g.copy()
    bad[20, 5], bad[21, 63], bad[200, 0], bad[256, 17] = np.float16(np.inf), np.float16(-np.inf), NAN16, NAN16
    half = _check(bad, q, 11, want_bits=1)
    assert not np.isin(half[0].cpu().numpy(), [20, 21, 200, 256]).any()
    _check(bad, q, 11, groups=GR.make_groups("pairs", 257), want_bits=1)
    # fewer finite rows than depth: the lists end in -1 / +inf
    few = np.full((40, 64), NAN16)
    few[[3, 17, 39]] = g[[3, 17, 39]]
    half = _check(few, q, 11, want_bits=1)
    assert bool((half[0][:, 3:] == -1).all()) and bool(torch.isposinf(half[1][:, 3:]).all()) and bool((half[0][:, :3] >= 0).all())
    # a non-finite query: -1 / +inf and bit 2
    qb = q.copy()
    qb[nq - 1, 7] = np.nan
    half, wide = _both(g, qb, 11)
    _assert_same_bits(half, wide)
    assert int(half[2].item()) == 2 and bool((half[0][nq - 1] == -1).all()) and bool(torch.isposinf(half[1][nq - 1]).all())
    if nq > 1:
        assert np.array_equal(half[0][:nq - 1].cpu().numpy(), HR.reference_search64(g, q[:nq - 1], 11)[0])
    half, wide = _both(bad, qb, 11, groups=GR.make_groups("pairs", 257))
    _assert_same_bits(half, wide)
    assert int(half[3].item()) == 3


# ---- masks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 2, 4, 8])
def test_masks_and_dead_rows_full_of_nan(nq):
    """The dead rows of the half gallery are NaN: they are never read as candidates, so nothing changes -- not the non-finite word
    either.  Oracle (A) reads the widened gallery with the dead rows left finite."""
    ng, depth = 257, 11
    g, q = HR.shape_case(64, ng, nq, depth)
    j = np.arange(ng)
    masks = {"all": np.ones(ng, bool), "one": j == 77, "every_other": j % 2 == 0, "run_across_a_word": (j >= 27) & (j < 41),
             "tail": j >= 250}
    tq = _t(q)
    for name, live in masks.items():
        dead_nan = g.copy()
        dead_nan[~live] = NAN16
        words = MR.pack_words(live)
        if name == "tail":
            words[-1] |= np.uint32(0xFFFFFFFE)                # bits above row 256 of the last word: garbage, ignored
        tw = _t(words.view(np.int32))
        half, wide = _both(dead_nan, tq, depth, live=tw, g_wide=_t(HR.widen(g)))
        _assert_same_bits(half, wide)
        ids, d32, gap = HR.reference_search_masked(g, q, live, depth)
        assert gap > 1e-12
        assert np.array_equal(half[0].cpu().numpy(), ids), name
        SR.assert_dists_within_one_ulp(half[1].cpu().numpy(), d32)
        assert int(half[2].item()) == 0, name
        if name == "all":
            _assert_same_bits(half, _both(g, tq, depth)[0])    # every bit set against no mask at all


# ---- groups --------------------------------------------------------------------------------------------------------------------------
def test_groups():
    ops = _ops()
    ng, nq, depth = 257, 5, 11
    g, q = HR.shape_case(64, ng, nq, depth)
    th, tq = _t(g), _t(q)
    # one row per group: the ungrouped half search, bit for bit
    ws = ops.workspace(ops.l2_search_workspace_bytes(ng, nq, 64, depth), DEV)
    ws2 = ops.workspace(ops.l2_search_grouped_workspace_bytes(ng, nq, 64, depth), DEV)
    ids, dists, bits = ops.l2_search(th, tq, depth, id_base=3, ws=ws)
    ids2, grp2, dists2, bits2 = ops.l2_search_grouped(th, tq, _t(GR.make_groups("singletons", ng)), depth, id_base=3, ws=ws2)
    assert torch.equal(ids, ids2) and torch.equal(dists, dists2) and torch.equal(bits, bits2) and torch.equal(grp2.to(torch.int64), ids2 - 3)
    assert torch.equal(ops.search_dists64(ws, nq, depth), ops.search_dists64(ws2, nq, depth))
    five_scattered = np.random.default_rng(4).permutation(ng) // 5
    kinds = {"five_contiguous": j_div(ng, 5), "five_scattered": five_scattered.astype(np.int32), "fewer_than_depth": GR.make_groups("strided", ng),
             "minus_one_and_int32_min": GR.make_groups("sparse_ids", ng, seed=1)}
    assert {-1, -2 ** 31} <= set(kinds["minus_one_and_int32_min"].tolist()) and len(set(kinds["fewer_than_depth"].tolist())) == 7 < depth
    for name, groups in kinds.items():
        half = _check(g, q, depth, groups=groups)
        if name == "fewer_than_depth":
            assert bool((half[0][:, 7:] == -1).all()) and bool((half[1][:, 7:] == -1).all()) and bool((half[0][:, :7] >= 0).all())
        live = MR.make_mask("random_0.5", ng, seed=9)
        dead_nan = g.copy()
        dead_nan[~live] = NAN16
        h, w = _both(dead_nan, tq, depth, live=live, groups=groups, g_wide=_t(HR.widen(g)))
        _assert_same_bits(h, w)
        want = HR.reference_search_grouped64(g, q, groups, depth, live)
        assert want[3] > 1e-12 and np.array_equal(h[0].cpu().numpy(), want[0]) and np.array_equal(h[1].cpu().numpy(), want[1])
        assert int(h[3].item()) == 0


def j_div(n, k):
    return (np.arange(n) // k).astype(np.int32)


# ---- windows -------------------------------------------------------------------------------------------------------------------------
def test_windows_of_a_half_gallery_merged_equal_the_whole():
    from vtc_amd import dist as VD
    ops = _ops()
    ng, nq, depth = 257, 9, 11
    g, q = HR.shape_case(64, ng, nq, depth)
    groups = j_div(ng, 5)
    th, tq, tgr = _t(g), _t(q), _t(groups)
    live = MR.make_mask("random_0.5", ng, seed=3)
    cuts = [0, 7, 131, ng]                                    # 7 rows: shorter than the depth
    ws = ops.workspace(ops.l2_search_grouped_workspace_bytes(ng, nq, 64, depth), DEV)
    whole = ops.l2_search(th, tq, depth, ws=ws, live=_words(live))
    whole64 = ops.search_dists64(ws, nq, depth).clone()
    parts, gparts = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        dep = min(depth, hi - lo)
        ids, d64, bits = ops.l2_search_part(th[lo:hi], tq, dep, id_base=lo, live=_words(live[lo:hi]))
        assert int(bits.item()) == 0 and d64.dtype == torch.float64
        parts.append(ops.pad_search_part(ids, d64.clone(), depth))
        ids, grp, d64, bits = ops.l2_search_grouped_part(th[lo:hi], tq, tgr[lo:hi], dep, id_base=lo, live=_words(live[lo:hi]))
        gparts.append(ops.pad_search_part(ids, d64.clone(), depth) + (torch.nn.functional.pad(grp, (0, depth - dep), value=-1),))
    ids, dists = ops.l2_search_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(ids, whole[0]) and torch.equal(dists, whole[1]) and torch.equal(dists, whole64.to(torch.float32))
    gwhole = ops.l2_search_grouped(th, tq, tgr, depth, live=_words(live))
    ids, grp, dists = ops.l2_search_merge_grouped(*[torch.stack([p[i] for p in gparts]) for i in range(3)])
    assert torch.equal(ids, gwhole[0]) and torch.equal(grp, gwhole[1]) and torch.equal(dists, gwhole[2])
    # the sharded entry points at world 1, fp16 local rows
    ids, dists, _ = ops.l2_search(th, tq, depth, id_base=500)
    got = VD.sharded_search(th, 500, tq, depth, 0, 1)
    assert torch.equal(got[0], ids) and torch.equal(got[1], dists)
    ids, grp, dists, _ = ops.l2_search_grouped(th, tq, tgr, depth, id_base=500)
    videos, rows, dd = VD.sharded_search_videos(th, tgr, 500, tq, depth, 0, 1)
    assert torch.equal(rows, ids) and torch.equal(videos, grp.to(torch.int64)) and torch.equal(dd, dists)
    rows5 = VD.sharded_search(th[:5], 0, tq, depth, 0, 1)     # fewer rows than k on the rank: padded
    assert torch.equal(rows5[0][:, :5], ops.l2_search(th[:5], tq, 5)[0]) and bool((rows5[0][:, 5:] == -1).all())


def test_other_gallery_dtypes_still_raise():
    ops = _ops()
    g, q = HR.shape_case(64, 33, 2, 5)
    tq = _t(q)
    for dtype in (torch.bfloat16, torch.float64, torch.int16):
        with pytest.raises(TypeError):
            ops.l2_search(_t(g).to(dtype), tq, 5)
        with pytest.raises(TypeError):
            ops.l2_search_grouped(_t(g).to(dtype), tq, _t(j_div(33, 2)), 5)
    with pytest.raises(TypeError):
        ops.l2_search(_t(g), tq.half(), 5)                    # the queries stay fp32


# ---- containment -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_no_write_outside_the_outputs_and_the_gallery_is_only_read(grouped):
    from vtc_amd import _lib as L
    lib = L.lib()
    nq, depth, ng, d = 9, 11, 257, 64
    g, q = HR.shape_case(d, ng, nq, depth)
    live = MR.make_mask("random_0.5", ng, seed=11)
    groups = GR.make_groups("random_50", ng, seed=11)
    if grouped:
        want_ids, want_grp, want_d64, gap = HR.reference_search_grouped64(g, q, groups, depth, live)
        want_d = want_d64.astype(np.float32)
    else:
        want_ids, want_d, gap = HR.reference_search_masked(g, q, live, depth)
    assert gap > 1e-12
    tq = _t(q)
    G, guard = 4, 4096
    POISON16 = 0x7E5A                                         # a NaN half: a read outside the gallery would set the non-finite word
    gal = torch.full(((ng + 2 * 8) * d,), POISON16, dtype=torch.int16, device=DEV)
    gal[8 * d:(8 + ng) * d] = _t(g.view(np.int16).reshape(-1))
    gal_before = gal.clone()
    ids = torch.full((nq + 2 * G, depth), -77, dtype=torch.int64, device=DEV)
    grp = torch.full((nq + 2 * G, depth), -77, dtype=torch.int32, device=DEV)
    dists = torch.full((nq + 2 * G, depth), -77.0, dtype=torch.float32, device=DEV)
    need = (lib.vtc_l2_search_grouped_workspace_bytes if grouped else lib.vtc_l2_search_workspace_bytes)(ng, nq, d, depth)
    ws = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    words = MR.pack_words(live).view(np.int32)
    mask = torch.full((words.size + 2 * 64,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    mask[64:64 + words.size] = _t(words)
    gids = torch.full((ng + 2 * 64,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    gids[64:64 + ng] = _t(groups)
    mask_before, gids_before = mask.clone(), gids.clone()
    bits = torch.full((3,), -77, dtype=torch.int32, device=DEV)
    bits[1] = 0
    args = (gal[8 * d:].data_ptr(), tq.data_ptr(), mask[64:].data_ptr(), gids[64:].data_ptr() if grouped else None, ng, nq, d, depth, 0,
            ids[G].data_ptr(), grp[G].data_ptr() if grouped else None, dists[G].data_ptr(), bits[1:].data_ptr())
    before = lib.vtc_debug_launch_count()
    assert lib.vtc_l2_search_half(*args, ws.data_ptr() + guard, need - 1, None) != 0 and b"workspace" in lib.vtc_last_error()
    assert lib.vtc_debug_launch_count() == before             # one byte too small: refused, nothing launched
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(stream):
            rc = lib.vtc_l2_search_half(*args, ws.data_ptr() + guard, need, stream.cuda_stream)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert rc == 0, lib.vtc_last_error()
    stream.synchronize()
    assert np.array_equal(ids[G:G + nq].cpu().numpy(), want_ids)
    SR.assert_dists_within_one_ulp(dists[G:G + nq].cpu().numpy(), want_d)
    if grouped:
        assert np.array_equal(grp[G:G + nq].cpu().numpy(), want_grp)
    else:
        assert bool((grp == -77).all())                       # out_groups is ignored without groups
    assert bits.tolist() == [-77, 0, -77]
    for out, fill in ((ids, -77), (grp, -77), (dists, -77.0)):
        assert bool((out[:G] == fill).all()) and bool((out[G + nq:] == fill).all())
    assert bool((ws[:guard] == 0xA5).all()) and bool((ws[guard + need:] == 0xA5).all())
    assert torch.equal(mask, mask_before) and torch.equal(gids, gids_before) and torch.equal(gal, gal_before)
    d64 = ws[guard:guard + nq * depth * 8].view(torch.float64).view(nq, depth)
    assert torch.equal(d64.to(torch.float32), dists[G:G + nq])


# ---- VideoIndex ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw_rows():
    import rank_refs as RR
    rng = np.random.default_rng(41)
    a, b = RR.spread_pairs(400, 100, 27)                      # 100 columns: padded to 128
    scale = np.exp(rng.uniform(-1, 1, (400, 1))).astype(np.float32)
    vids = rng.integers(0, 50, 400) * 1000 + 7
    return (a * scale).astype(np.float32), (b * scale).astype(np.float32), vids


def _pair(rows, vids=None):
    """A half index and the fp32 index built from its widened stored rows (normalized=True: taken as they are)."""
    from vtc_amd.host.search import VideoIndex
    half = VideoIndex(100, device=DEV, storage=torch.float16)
    half.add(_t(rows[:150]), video_ids=None if vids is None else vids[:150])
    half.add(_t(rows[150:]), video_ids=None if vids is None else vids[150:])
    wide = VideoIndex(100, device=DEV, normalized=True)
    wide.add(half.rows[:, :100].float(), video_ids=vids)
    return half, wide


def _same(x, y):
    assert len(x) == len(y) and all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(x, y))


def test_video_index_storage_and_search_equality(raw_rows):
    from vtc_amd.host.search import VideoIndex
    ops = _ops()
    a, b, vids = raw_rows
    half, wide = _pair(a, vids)
    assert half.storage == torch.float16 and wide.storage == torch.float32 == VideoIndex(100, device=DEV).storage
    assert half.rows.dtype == torch.float16 and tuple(half.rows.shape) == (400, 128) and half._rows.dtype == torch.float16
    unit = ops.normalize_rows(_t(a))
    assert torch.equal(half.rows[:, :100], unit.to(torch.float16)) and bool((half.rows[:, 100:] == 0).all())
    assert np.array_equal(half.rows[:, :100].cpu().numpy().view(np.uint16), HR.round_half(unit.cpu().numpy()).view(np.uint16))
    qn = wide._prepared(half._prepared(_t(b[:5]), "queries", check=False)[:, :100], "queries", check=False)     # unit queries for the fp32 index
    q = _t(b[:5])
    _same(half.search(q, 7), wide.search(qn[:, :100], 7))
    ids, scores = half.search(q, 7)                           # (B): the reference over the stored rows
    want = HR.reference_search64(half.rows.cpu().numpy(), qn.cpu().numpy(), 7)
    assert want[2] > 1e-12 and np.array_equal(ids.cpu().numpy(), want[0])
    assert np.allclose((2.0 * (1.0 - scores)).cpu().numpy(), want[1].astype(np.float32), rtol=0, atol=4e-7)
    sub_ids = list(range(0, 400, 3))
    _same(half.search(q, 7, subset=half.subset(sub_ids)), wide.search(qn[:, :100], 7, subset=wide.subset(sub_ids)))
    _same(half.search_videos(q, 7), wide.search_videos(qn[:, :100], 7))
    _same(half.search_videos(q, 7, subset=half.subset(sub_ids)), wide.search_videos(qn[:, :100], 7, subset=wide.subset(sub_ids)))
    gone = [int(i) for i in ids[:, 0].tolist()]
    assert half.remove(gone) == wide.remove(gone) == len(set(gone)) and len(half) == 400 - len(set(gone))
    got = half.search(q, 7)
    _same(got, wide.search(qn[:, :100], 7))
    assert not np.isin(got[0].cpu().numpy(), gone).any()
    assert half.remove_videos([int(vids[0])]) == wide.remove_videos([int(vids[0])]) > 0
    _same(half.search_videos(q, 7), wide.search_videos(qn[:, :100], 7))


def test_video_index_seventy_queries_are_two_slices_and_nothing_syncs(raw_rows):
    """A half index never takes the vtc_l2_topk route: 70 queries are two calls of the scan, equal to 70 single-query calls; search,
    masked search and search_videos are only enqueued, a NaN query gets -1 / -inf."""
    from vtc_amd import _lib as L
    a, b, vids = raw_rows
    half, _ = _pair(a, vids)
    q = b[:70].copy()
    q[66, 5] = np.nan
    q = _t(q)
    sub = half.subset(list(range(0, 400, 2)))
    warm = (half.search(q, 5), half.search(q, 5, subset=sub), half.search_videos(q, 5))       # workspace and packed words exist
    torch.cuda.synchronize()
    before = L.lib().vtc_debug_launch_count()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = (half.search(q, 5), half.search(q, 5, subset=sub), half.search_videos(q, 5))
        one = half.search(q[:1], 5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for x, y in zip(got, warm):
        _same(x, y)
    lib = L.lib()
    launches = lib.vtc_debug_launch_count() - before
    mark = lib.vtc_debug_launch_count()
    half.search(q[:1], 5)
    single = lib.vtc_debug_launch_count() - mark               # normalisation + scan + merge
    assert launches == 3 * (single + 2) + single               # each 70-query call: one more slice, a scan and a merge
    ids, scores = got[0]
    assert tuple(ids.shape) == (70, 5)
    for i in range(70):
        i1, s1 = half.search(q[i:i + 1], 5)
        assert torch.equal(ids[i:i + 1], i1) and torch.equal(scores[i:i + 1], s1), i
    assert bool((ids[66] == -1).all()) and bool(torch.isneginf(scores[66]).all()) and bool((ids[65] >= 0).all())
    assert torch.equal(one[0], ids[:1])


def test_video_index_rounding_state_dict_converted_and_constructor(raw_rows):
    from vtc_amd.host.search import VideoIndex
    a, b, vids = raw_rows
    with pytest.raises(ValueError, match="storage"):
        VideoIndex(100, device=DEV, storage=torch.bfloat16)
    # the check runs on the ROUNDED rows: 1e5 is finite in fp32 and inf as a half
    big = a[:3].copy()
    big[1, 7] = 1e5
    strict = VideoIndex(100, device=DEV, normalized=True, storage=torch.float16)
    with pytest.raises(ValueError, match="non-finite"):
        strict.add(_t(big))
    assert len(strict) == 0 and VideoIndex(100, device=DEV, normalized=True).add(_t(big)) == 0
    half, wide = _pair(a, vids)
    half.remove([3, 5, 399])
    q = _t(b[:4])
    # state dict: bit-exact round trip, storage named, mismatch refused, a legacy state is fp32
    state = half.state_dict()
    assert state["storage"] == "float16" and state["rows"].dtype == torch.float16 and tuple(state["rows"].shape) == (400, 100)
    other = VideoIndex(100, device=DEV, storage=torch.float16)
    other.load_state_dict({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in state.items()})
    assert torch.equal(other.rows.view(torch.int16), half.rows.view(torch.int16)) and len(other) == 397 and other.ntotal == 400
    _same(other.search(q, 5), half.search(q, 5))
    _same(other.search_videos(q, 5), half.search_videos(q, 5))
    with pytest.raises(ValueError, match="storage"):
        VideoIndex(100, device=DEV).load_state_dict(state)
    legacy = {k: v for k, v in wide.state_dict().items() if k != "storage"}
    with pytest.raises(ValueError, match="storage"):
        VideoIndex(100, device=DEV, storage=torch.float16).load_state_dict(legacy)
    old = VideoIndex(100, device=DEV, normalized=True)
    old.load_state_dict(legacy)
    assert old.storage == torch.float32 and torch.equal(old.rows, wide.rows)
    old.load_state_dict(dict(legacy, storage="float32"))
    # converted: both ways, and the same storage is a copy
    up = half.converted(torch.float32)
    assert up.storage == torch.float32 and up.rows.dtype == torch.float32 and torch.equal(up.rows, half.rows.float())
    down = wide.converted(torch.float16)
    assert down.storage == torch.float16 and torch.equal(down.rows.view(torch.int16), wide.rows.to(torch.float16).view(torch.int16))
    back = up.converted(torch.float16)
    copy = half.converted(torch.float16)
    for new in (up, back, copy):
        assert new.ntotal == 400 and len(new) == 397 and torch.equal(new.live_mask, half.live_mask) and torch.equal(new.video_ids, half.video_ids)
        assert new.normalized == half.normalized and new.grouped
    assert torch.equal(back.rows.view(torch.int16), half.rows.view(torch.int16))               # half -> fp32 -> half: the identity
    assert torch.equal(copy.rows.view(torch.int16), half.rows.view(torch.int16)) and copy._rows.data_ptr() != half._rows.data_ptr()
    _same(back.search_videos(q, 5), half.search_videos(q, 5))
    first = copy.add(_t(a[:2]), video_ids=[1, 2])             # the converted index grows on its own
    assert first == 400 and copy.ntotal == 402 and half.ntotal == 400
    with pytest.raises(ValueError, match="storage"):
        half.converted(torch.bfloat16)
    plain = VideoIndex(100, device=DEV)
    plain.add(_t(a[:50]))
    conv = plain.converted(torch.float16)
    assert not conv.grouped and conv.video_ids is None and conv._live is None and len(conv) == 50
    assert torch.equal(conv.rows, plain.rows.to(torch.float16))


def test_video_index_search_text_on_a_half_index():
    from oracle import arch as A
    from vtc_amd.host import model as HM
    from vtc_amd.host.clip_arch import ClipConfig
    from vtc_amd.host.search import VideoIndex
    torch.set_grad_enabled(False)
    arch = A.TINY
    m = HM.PretrainedCLIP(model_type=ClipConfig(**asdict(arch)))
    m.load_state_dict(A.synth_model(arch, 7, "clip"), strict=True)
    m = m.eval().to(DEV)
    dim = arch.embed_dim
    rng = np.random.default_rng(32)
    half = VideoIndex(dim, device=DEV, storage=torch.float16)
    half.add(_t(rng.standard_normal((200, dim)).astype(np.float32)))
    wide = VideoIndex(dim, device=DEV, normalized=True)
    wide.add(half.rows[:, :dim].float())
    tokens = A.synth_tokens(5, arch, 9).to(DEV)
    got = half.search_text(m, tokens, 7)
    # the queries as the half index prepares them (search normalises what search_text hands it once more; the fp32 index, built as
    # ``normalized``, takes its queries as they are)
    qn = _ops().normalize_rows(_ops().normalize_rows(m.encode_text(tokens).float().contiguous()))
    want = wide.search(qn, 7)
    assert tuple(got[0].shape) == (5, 7)
    _same(got, want)
    _same(got, half.search(_ops().normalize_rows(m.encode_text(tokens).float().contiguous()), 7))
