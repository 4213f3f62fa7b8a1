"""GPU: the query-time search over a gallery stored as 8-bit codes and one fp32 scale a row (vtc_quantize_rows_q8 and the *_q8 entries;
ops.l2_search* / l2_range_* with a torch.int8 gallery [n, d + 16]; VideoIndex(storage=torch.int8)).  Two oracles, both independent of
the new kernels:

  (A) the fp32 entry points over the fp32 gallery of the stored values (tests/search_q8_refs.stored, formed in numpy), compared with
      torch.equal on every output -- ids, fp32 dists, groups, the non-finite word, the fp64 distances of the workspace, hit words, lims:
      the q8 scan must form the same bits (a flushed subnormal product, a fused multiply or a reordered sum would not);
  (B) the numpy fp64 reference over the stored values: ids where min_gap > 1e-12 (asserted here; the same shapes are checked on the CPU
      in tests/test_search_q8_refs.py), fp32 dists within one ulp.
The quantiser is compared bit for bit with its numpy restatement."""
from dataclasses import asdict

import numpy as np
import pytest
import torch

import search_grouped_refs as GR
import search_mask_refs as MR
import search_q8_refs as QR
import search_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN32, INF32 = np.float32(np.nan), np.float32(np.inf)


def _ops():
    from vtc_amd import ops
    return ops


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _words(live):
    return None if live is None else _t(MR.pack_words(live).view(np.int32))


def j_div(n, k):
    return (np.arange(n) // k).astype(np.int32)


def _same(x, y):
    assert len(x) == len(y)
    for a, b in zip(x, y):
        if a is None or b is None:
            assert a is None and b is None
        elif a.dtype.is_floating_point:                       # bit for bit: NaN == NaN, -0.0 != 0.0
            as_int = {torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(as_int), b.view(as_int)), (a, b)
        else:
            assert a.dtype == b.dtype and torch.equal(a, b), (a, b)


def _on_both(rows, call, wide=None):
    """call(gallery) -> a tuple of tensors, over the q8 rows and over the fp32 gallery of their stored values (oracle A); asserts the
    two equal bit for bit and returns the q8 result.  `wide`: what the fp32 call reads instead."""
    tr = rows if isinstance(rows, torch.Tensor) else _t(rows)
    assert tr.dtype == torch.int8
    tw = _t(QR.stored(tr.cpu().numpy())) if wide is None else wide
    got, want = call(tr), call(tw)
    _same(got, want)
    return got


def _search(q, depth, live=None, groups=None, id_base=0, **kw):
    """A call for _on_both: l2_search / l2_search_grouped in a workspace of its own, the fp64 distances appended."""
    ops = _ops()
    tq = q if isinstance(q, torch.Tensor) else _t(q)
    words = live if isinstance(live, torch.Tensor) or live is None else _words(live)

    def call(g):
        ng, d = ops._gallery_shape(g)
        nq = tq.shape[0]
        if groups is None:
            ws = ops.workspace(ops.l2_search_workspace_bytes(ng, nq, d, depth), DEV)
            res = ops.l2_search(g, tq, depth, id_base=id_base, ws=ws, live=words, **kw)
        else:
            ws = ops.workspace(ops.l2_search_grouped_workspace_bytes(ng, nq, d, depth), DEV)
            res = ops.l2_search_grouped(g, tq, groups if isinstance(groups, torch.Tensor) else _t(groups), depth, id_base=id_base, ws=ws,
                                        live=words, **kw)
        return tuple(res) + (ops.search_dists64(ws, nq, depth).clone(),)
    return call


def _check(rows, q, depth, live=None, groups=None, id_base=0, want_bits=0):
    """Both oracles on one search; returns the q8 result (ids, [groups,] dists, bits, dists64)."""
    got = _on_both(rows, _search(q, depth, live, groups, id_base))
    alive = np.ones(len(rows), bool) if live is None else np.asarray(live, bool)
    if groups is None:
        ids, d32, gap = QR.reference_search_masked(rows, q, alive, depth, id_base)
    else:
        ids, grp, d64, gap = QR.reference_search_grouped64(rows, q, groups, depth, alive, id_base)
        d32 = d64.astype(np.float32)
        assert np.array_equal(got[1].cpu().numpy(), grp)
    assert gap > 1e-12, gap
    assert np.array_equal(got[0].cpu().numpy(), ids)
    SR.assert_dists_within_one_ulp(got[-3].cpu().numpy(), d32)
    assert int(got[-2].item()) == want_bits
    return got


# ---- 1. shapes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ng,nq,depth", QR.SHAPES)
def test_shapes_and_special_rows(d, ng, nq, depth):
    """Galleries of 16 rows and more hold the special rows of search_q8_refs.special_rows.  id_base > 2^32."""
    rows, q = QR.shape_case(d, ng, nq, depth)
    _check(rows, q, depth, id_base=2 ** 33 + 5)
    if ng >= 33:
        _check(rows, q, min(depth, ng), live=MR.make_mask("alt_bits", ng))
        _check(rows, q, depth, groups=GR.make_groups("strided", ng), id_base=3)


def test_a_gallery_larger_than_one_pass_of_the_grid():
    rows, q = QR.large_case()
    ng = rows.shape[0]
    tr, tw = _t(rows), _t(QR.stored(rows))
    for nq in (1, 2, 4, 9):
        got = _on_both(tr, _search(q[:nq], 11), wide=tw)
        ids, d64, gap = QR.reference_search64(rows, q[:nq], 11)
        assert gap > 1e-12 and np.array_equal(got[0].cpu().numpy(), ids) and int(got[0][0, 0]) == ng - 1 and int(got[2].item()) == 0
    live = MR.make_mask("random_0.5", ng, seed=2) | (np.arange(ng) == ng - 1)
    _on_both(tr, _search(q[:2], 11, live=live, groups=j_div(ng, 5)), wide=tw)


# ---- 2. special rows, by name --------------------------------------------------------------------------------------------------------
def test_special_rows_by_name():
    rows, q = QR.shape_case(512, 33, 4, 33)
    got = _on_both(rows, _search(q, 33, id_base=2 ** 33))
    ids, d32, d64 = got[0].cpu().numpy() - 2 ** 33, got[1].cpu().numpy(), got[3].cpu().numpy()
    assert (ids >= 0).all() and np.array_equal(np.sort(ids, axis=1), np.tile(np.arange(33), (4, 1)))      # every row is finite: all come back
    D = SR.distances64(QR.stored(rows), q)
    for i in range(4):
        pos = {int(r): int(np.flatnonzero(ids[i] == r)[0]) for r in range(16)}
        assert [pos[r] for r in (3, 4, 5, 6)] == list(range(pos[3], pos[3] + 4))                         # duplicates: the lower row first
        assert d64[i, pos[7]] != d64[i, pos[8]] and (d64[i, pos[7]] < d64[i, pos[8]]) == (D[i, 7] < D[i, 8])      # one code apart
        assert d64[i, pos[9]] != d64[i, pos[10]] and (d64[i, pos[9]] < d64[i, pos[10]]) == (D[i, 9] < D[i, 10])  # one scale step apart
        assert abs(d64[i, pos[9]] - d64[i, pos[10]]) < 1e-3 * d64[i, pos[9]]
        assert pos[11] == 32 and d64[i, 32] > 2.0 ** 200 and np.isposinf(d32[i, 32])                      # 2^100: a finite fp64 distance
        assert abs(pos[13] - pos[14]) == 1 and pos[14] == pos[13] + 1 and d64[i, pos[13]] == d64[i, pos[14]]      # |q|^2 twice: a tie
        assert np.isclose(d64[i, pos[15]], D[i, 15], rtol=1e-12)                                         # the rounded products
    # subnormal products are not flushed: a gallery of nothing else, queries of the same magnitude (taken as they are by the library)
    rng = np.random.default_rng(8)
    codes = rng.integers(-127, 128, (40, 64)).astype(np.int8)
    tiny = QR.pack_rows(codes, np.full(40, 2.0 ** -133, np.float32))
    tq = (rng.integers(-63, 64, (3, 64)) * 2.0 ** -131).astype(np.float32)
    assert np.all(np.abs(QR.stored(tiny)) < 2.0 ** -126) and np.count_nonzero(QR.stored(tiny)) == np.count_nonzero(codes)
    got = _on_both(tiny, _search(tq, 40))
    want = SR.reference_search64(QR.stored(tiny), tq, 40)
    assert len(np.unique(got[3].cpu().numpy()[0])) > 30       # flushed, all forty distances would be |q|^2 (or 0)
    assert want[2] > 1e-12 and np.array_equal(got[0].cpu().numpy(), want[0])
    assert np.allclose(got[3].cpu().numpy(), want[1], rtol=1e-12, atol=0)
    # ops.dequantize_rows_q8 (a torch expression) gives the stored values, bit for bit
    for r in (rows, tiny):
        assert np.array_equal(_ops().dequantize_rows_q8(_t(r)).cpu().numpy().view(np.uint32), QR.stored(r).view(np.uint32))


# ---- 3. non-finite -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 4, 9])
def test_nonfinite_scales_and_queries(nq):
    rows, q = QR.shape_case(64, 257, 9, 11)
    q = q[:nq].copy()
    codes, s = QR.unpack_rows(rows)
    bad_s = s.copy()
    bad_s[20], bad_s[21], bad_s[200], bad_s[256] = NAN32, INF32, -INF32, NAN32
    bad = QR.pack_rows(codes, bad_s)
    got = _check(bad, q, 11, want_bits=1)
    assert not np.isin(got[0].cpu().numpy(), [20, 21, 200, 256]).any()
    _check(bad, q, 11, groups=GR.make_groups("pairs", 257), want_bits=1)
    # a dead row full of NaN scales sets nothing: oracle (A) reads the gallery with the dead rows left finite
    live = np.ones(257, bool)
    live[[20, 21, 200, 256]] = False
    got = _on_both(bad, _search(q, 11, live=live), wide=_t(QR.stored(rows)))
    assert int(got[2].item()) == 0
    assert np.array_equal(got[0].cpu().numpy(), QR.reference_search_masked(rows, q, live, 11)[0])
    # fewer finite rows than depth: the lists end in -1 / +inf
    few_s = np.full(40, NAN32)
    few_s[[3, 17, 39]] = s[[3, 17, 39]]
    got = _check(QR.pack_rows(codes[:40], few_s), q, 11, want_bits=1)
    assert bool((got[0][:, 3:] == -1).all()) and bool(torch.isposinf(got[1][:, 3:]).all()) and bool((got[0][:, :3] >= 0).all())
    # a non-finite query: -1 / +inf and bit 2
    qb = q.copy()
    qb[nq - 1, 7] = np.nan
    got = _on_both(rows, _search(qb, 11))
    assert int(got[2].item()) == 2 and bool((got[0][nq - 1] == -1).all()) and bool(torch.isposinf(got[1][nq - 1]).all())
    if nq > 1:
        assert np.array_equal(got[0][:nq - 1].cpu().numpy(), QR.reference_search64(rows, q[:nq - 1], 11)[0])
    got = _on_both(bad, _search(qb, 11, groups=GR.make_groups("pairs", 257)))
    assert int(got[3].item()) == 3


# ---- 4. every mode on one small gallery ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """(rows q8 [257, 80] numpy, queries [9, 64], their tensors, the fp32 gallery of the stored values, groups dense in [0, 52))."""
    rows, q = QR.shape_case(64, 257, 9, 11)
    groups = j_div(257, 5)
    return rows, q, _t(rows), _t(q), _t(QR.stored(rows)), groups


def test_modes_masks_groups_and_exclusions(small):
    ops = _ops()
    rows, q, tr, tq, tw, groups = small
    ng, nq, depth = 257, 9, 11
    for name in ("alt_bits", "random_0.5"):
        live = MR.make_mask(name, ng, seed=9)
        _check(rows, q, depth, live=live)
        _check(rows, q, depth, live=live, groups=groups)
    first = _check(rows, q, depth)
    ex_rows = first[0][:, 0].clone()                          # every query without its nearest row
    ex_rows[3] = -1
    got = _on_both(tr, _search(tq, depth, exclude=ex_rows), wide=tw)
    assert not bool((got[0] == ex_rows[:, None]).any()) and torch.equal(got[0][3], first[0][3])
    assert torch.equal(got[0][0, :depth - 1], first[0][0, 1:])
    gfirst = _check(rows, q, depth, groups=groups)
    ex_groups = gfirst[1][:, 0].to(torch.int64)
    got = _on_both(tr, _search(tq, depth, groups=groups, exclude=ex_groups), wide=tw)
    assert not bool((got[1].to(torch.int64) == ex_groups[:, None]).any()) and torch.equal(got[0][:, :depth - 1], gfirst[0][:, 1:])
    live = MR.make_mask("random_0.5", ng, seed=4)
    _on_both(tr, _search(tq, depth, live=live, exclude=ex_rows), wide=tw)
    _on_both(tr, _search(tq, depth, live=live, groups=groups, exclude=ex_groups), wide=tw)


def test_modes_cursor_chained_to_the_end_and_pages_of_groups(small):
    ops = _ops()
    rows, q, tr, tq, tw, groups = small
    ng, nq, depth = 257, 9, 64
    order, _, gap = QR.reference_search64(rows, q, ng)
    assert gap > 1e-12
    pages, cursor = [], None
    for _ in range(6):
        got = _on_both(tr, _search(tq, depth, after=cursor, id_base=7), wide=tw)
        pages.append(got[0])
        cursor = (got[3][:, -1].clone(), got[0][:, -1].clone())
    chained = torch.cat(pages, dim=1).cpu().numpy()
    assert np.array_equal(chained[:, :ng], order + 7) and (chained[:, ng:] == -1).all()
    # a cursor from the row alone, with an excluded row, under a mask
    live = MR.make_mask("random_0.5", ng, seed=4)
    after_ids = pages[0][:, 20].clone()
    d64 = _on_both(tr, lambda g: (ops.l2_pair_dists64(g, tq, after_ids, id_base=7),), wide=tw)[0]
    assert torch.equal(d64, _on_both(tr, _search(tq, depth, id_base=7), wide=tw)[3][:, 20])
    _on_both(tr, _search(tq, 11, live=live, after=(d64, after_ids), exclude=pages[0][:, 22].clone(), id_base=7), wide=tw)
    # the page scan and its mark pass: distinct groups, chained to the end
    n_groups = int(groups.max()) + 1
    tg = _t(groups)
    gorder = QR.reference_search_grouped64(rows, q, groups, n_groups)
    assert gorder[3] > 1e-12
    gpages, cursor = [], None
    for page in range(3):
        kw = {} if cursor is None else dict(after=cursor, n_groups=n_groups)
        got = _on_both(tr, _search(tq, 20, groups=tg, **kw), wide=tw)
        if cursor is not None:
            ban = _on_both(tr, lambda g: (ops.l2_group_mark_before(g, tq, tg, n_groups, cursor),), wide=tw)[0]
            assert int((ban != 0).sum()) > 0
            _on_both(tr, _search(tq, 20, groups=tg, after=cursor, n_groups=n_groups, ban=ban, exclude=gorder_t[:, 30].clone()), wide=tw)
        else:
            gorder_t = _t(gorder[1].astype(np.int64))
        gpages.append(got[0])
        cursor = (got[4][:, -1].clone(), got[0][:, -1].clone())
    chained = torch.cat(gpages, dim=1).cpu().numpy()
    assert np.array_equal(chained[:, :n_groups], gorder[0]) and (chained[:, n_groups:] == -1).all()
    live_w = _words(live)
    _on_both(tr, lambda g: (ops.l2_group_mark_before(g, tq, tg, n_groups, (d64, after_ids), live=live_w, id_base=7),), wide=tw)


@pytest.mark.parametrize("members", [3, 9])
def test_modes_set_queries(small, members):
    import search_set_refs as TR
    ops = _ops()
    rows, q, tr, tq, tw, groups = small
    ng, depth = 257, 11
    rng = np.random.default_rng(members)
    sets = rng.standard_normal((4, members, 64)).astype(np.float32)
    sets /= np.linalg.norm(sets, axis=2, keepdims=True)
    ts, tg = _t(sets), _t(groups)
    live = MR.make_mask("random_0.5", ng, seed=6)

    def call(**kw):
        def run(g):
            ws = ops.workspace(ops.l2_search_sets_workspace_bytes(ng, 4, members, 64, depth, "groups" in kw), DEV)
            out = ops.l2_search_sets(g, ts, depth, ws=ws, **kw)
            return tuple(out) + (ops.search_dists64(ws, 4, depth).clone(),)
        return run
    got = _on_both(tr, call(), wide=tw)
    want = TR.reference_sets(QR.stored(rows), sets, depth)
    assert np.array_equal(got[0].cpu().numpy(), want[0])
    ex = got[0][:, 0].clone()
    _on_both(tr, call(live=_words(live), exclude=ex), wide=tw)
    got = _on_both(tr, call(groups=tg, id_base=5), wide=tw)
    _on_both(tr, call(groups=tg, live=_words(live), exclude=got[1][:, 0].to(torch.int64)), wide=tw)


def test_modes_pair_distances_range_and_windows(small):
    ops = _ops()
    rows, q, tr, tq, tw, groups = small
    ng, nq, depth = 257, 9, 11
    # pair distances, ids outside the window included
    ids = _t(np.array([0, 256, 17, -1, 257, 300, 5, 2 ** 40, 100], np.int64))
    pd = _on_both(tr, lambda g: (ops.l2_pair_dists64(g, tq, ids),), wide=tw)[0].cpu().numpy()
    D = SR.distances64(QR.stored(rows), q)
    assert np.isposinf(pd[[3, 4, 5, 7]]).all() and np.allclose(pd[[0, 1, 2, 6, 8]], D[[0, 1, 2, 6, 8], [0, 256, 17, 5, 100]], rtol=1e-13)
    win = _on_both(tr[100:200], lambda g: (ops.l2_pair_dists64(g, tq, ids + 100, id_base=100),), wide=tw[100:200])[0].cpu().numpy()
    whole = _on_both(tr, lambda g: (ops.l2_pair_dists64(g, tq, ids + 100),), wide=tw)[0].cpu().numpy()
    assert np.isposinf(win[[1, 3, 4, 5, 7, 8]]).all() and np.array_equal(win[[0, 2, 6]], whole[[0, 2, 6]]) and np.isfinite(whole[8])
    # range: a radius that equals one row's fp64 distance exactly -- that row is a hit (D <= radius2), the next one is not
    base = _on_both(tr, _search(tq, depth), wide=tw)
    radius2 = base[3][:, 5].clone()
    live = MR.make_mask("random_0.5", ng, seed=12)
    for lv in (None, _words(live)):
        def rng_call(g):
            ws = ops.workspace(ops.l2_range_workspace_bytes(ng, nq, 64), DEV)
            lims, bits = ops.l2_range_count(g, tq, radius2, live=lv, ws=ws, return_bits=True)
            return (lims, bits, ops.range_hit_words(ws, ng, nq).clone()) + tuple(
                ops.l2_range_search(g, tq, radius2, live=lv, id_base=9, return_dists64=True, return_words=True))
        got = _on_both(tr, rng_call, wide=tw)
        if lv is None:
            assert (got[0][1:] - got[0][:-1]).tolist() == [6] * nq
            hit = np.sort(got[4].cpu().numpy().reshape(nq, 6) - 9, axis=1)
            assert np.array_equal(hit, np.sort(base[0][:, :6].cpu().numpy(), axis=1))
            assert bool((got[6].view(nq, 6).max(dim=1).values == radius2).all())
    ex = base[0][:, 2].clone()
    _on_both(tr, lambda g: tuple(ops.l2_range_search(g, tq, radius2, exclude=ex, return_dists64=True)), wide=tw)
    # windows merged equal the whole (the partial lists do not know the storage: q8 and fp32 windows mix)
    cuts = [0, 7, 131, ng]
    tg = _t(groups)
    whole = ops.l2_search(tr, tq, depth, live=_words(live))
    gwhole = ops.l2_search_grouped(tr, tq, tg, depth, live=_words(live))
    parts, gparts = [], []
    for w, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        g = tw[lo:hi] if w == 1 else tr[lo:hi]
        dep = min(depth, hi - lo)
        pi, pd64, bits = ops.l2_search_part(g, tq, dep, id_base=lo, live=_words(live[lo:hi]))
        assert int(bits.item()) == 0
        parts.append(ops.pad_search_part(pi, pd64.clone(), depth))
        pi, pg, pd64, bits = ops.l2_search_grouped_part(g, tq, tg[lo:hi], dep, id_base=lo, live=_words(live[lo:hi]))
        gparts.append(ops.pad_search_part(pi, pd64.clone(), depth) + (torch.nn.functional.pad(pg, (0, depth - dep), value=-1),))
    mi, md = ops.l2_search_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(mi, whole[0]) and torch.equal(md, whole[1])
    mi, mg, md = ops.l2_search_merge_grouped(*[torch.stack([p[i] for p in gparts]) for i in range(3)])
    assert torch.equal(mi, gwhole[0]) and torch.equal(mg, gwhole[1]) and torch.equal(md, gwhole[2])


def test_refused_galleries_and_the_many_query_entries(small):
    ops = _ops()
    rows, q, tr, tq, tw, groups = small
    with pytest.raises(ValueError):
        ops.l2_search_many(tr, tq, 5)                         # the matrix-core passes stay half only
    with pytest.raises(ValueError):
        ops.l2_range_count_many(tr, tq, 0.5)
    with pytest.raises(ValueError, match="columns"):
        ops.l2_search(tr, _t(np.zeros((2, 80), np.float32)), 5)      # d is shape[1] - 16
    with pytest.raises(RuntimeError, match="multiple of 64"):
        ops.l2_search(_t(np.zeros((20, 64), np.int8)), _t(np.zeros((2, 48), np.float32)), 5)
    for dtype in (torch.uint8, torch.int16):
        with pytest.raises(TypeError):
            ops.l2_search(tr.to(dtype), tq, 5)


# ---- 5. the quantiser ----------------------------------------------------------------------------------------------------------------
def test_quantiser_equals_the_numpy_rule_and_writes_only_its_rows():
    from vtc_amd import _lib as L
    ops, lib = _ops(), L.lib()
    rng = np.random.default_rng(3)
    for d, n in ((64, 5), (192, 257), (2048, 9)):
        x = (rng.standard_normal((n, d)) * np.exp(rng.uniform(-3, 3, (n, 1)))).astype(np.float32)
        half = np.float32(2.0 ** -7)
        x[0] = 0
        x[0, 0] = 127 * half
        x[0, 1:9] = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 126.5], np.float32) * half      # half-way quotients: ties to even
        x[1] = 0
        x[2] *= np.float32(2.0 ** 120) / np.abs(x[2]).max()
        x[3] *= np.float32(2.0 ** -130) / np.abs(x[3]).max()
        x[4, d - 1] = np.nan
        want_c, want_s = QR.quantize(x)
        assert want_c[0, :9].tolist() == [127, 0, 2, 2, 4, 0, -2, -2, 126] and want_s[1] == 1 and want_s[3] < 2.0 ** -126
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = ops.quantize_rows_q8(_t(x), nonfinite=flag)
        assert got.dtype == torch.int8 and tuple(got.shape) == (n, d + 16) and int(flag.item()) == 1
        c, s = QR.unpack_rows(got.cpu().numpy())
        assert np.array_equal(c, want_c) and np.array_equal(s.view(np.uint32), want_s.view(np.uint32))
        assert np.array_equal(got.cpu().numpy(), QR.pack_rows(want_c, want_s))                          # the 12 tail bytes are zero
        assert np.array_equal(ops.q8_scales(got).cpu().numpy().view(np.uint32), want_s.view(np.uint32))
        assert torch.equal(ops.q8_rows(got[:, :d], ops.q8_scales(got)), got)
        x[4, d - 1], x[n - 1, 0] = 1.0, -np.inf                                                          # an inf; finite rows set nothing
        flag.zero_()
        assert int(ops.quantize_rows_q8(_t(x[:4]), nonfinite=flag)[0, 0]) == 127 and int(flag.item()) == 0
        got = ops.quantize_rows_q8(_t(x))
        c, s = QR.unpack_rows(got.cpu().numpy())
        assert np.isnan(s[n - 1]) and not c[n - 1].any() and np.array_equal(c, QR.quantize(x)[0])
    # guards: a poisoned buffer around the rows, the input only read
    n, d = 7, 192
    x = _t(rng.standard_normal((n + 2, d)).astype(np.float32))
    x_before = x.clone()
    out = torch.full((n + 2, d + 16), 0x5A, dtype=torch.int8, device=DEV)
    assert lib.vtc_quantize_rows_q8(x[1].data_ptr(), n, d, out[1].data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert bool((out[0] == 0x5A).all()) and bool((out[n + 1] == 0x5A).all()) and torch.equal(x, x_before)
    assert np.array_equal(out[1:n + 1].cpu().numpy(), QR.pack_rows(*QR.quantize(x[1:n + 1].cpu().numpy())))
    assert lib.vtc_quantize_rows_q8(x.data_ptr(), n, 100, out.data_ptr(), None, None) != 0 and b"multiple of 64" in lib.vtc_last_error()
    assert lib.vtc_q8_row_bytes(512) == 528 and lib.vtc_q8_row_bytes(100) == 0
    assert tuple(ops.quantize_rows_q8(_t(np.zeros((0, 64), np.float32))).shape) == (0, 80)


# ---- 6. containment ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_no_write_outside_the_outputs_and_the_gallery_is_only_read(grouped):
    from vtc_amd import _lib as L
    lib = L.lib()
    nq, depth, ng, d = 9, 11, 257, 64
    rows, q = QR.shape_case(d, ng, nq, depth)
    live = MR.make_mask("random_0.5", ng, seed=11)
    groups = GR.make_groups("random_50", ng, seed=11)
    if grouped:
        want_ids, want_grp, want_d64, gap = QR.reference_search_grouped64(rows, q, groups, depth, live)
        want_d = want_d64.astype(np.float32)
    else:
        want_ids, want_d, gap = QR.reference_search_masked(rows, q, live, depth)
    assert gap > 1e-12
    tq = _t(q)
    G, guard, rb = 4, 4096, d + 16
    gal = torch.full(((ng + 2 * 8) * rb,), -1, dtype=torch.int8, device=DEV)      # guard rows: a NaN scale -- a read outside would set bit 1
    gal[8 * rb:(8 + ng) * rb] = _t(rows.reshape(-1))
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
    args = (gal[8 * rb:].data_ptr(), tq.data_ptr(), mask[64:].data_ptr(), gids[64:].data_ptr() if grouped else None, 0, None, None, None, None,
            ng, nq, d, depth, 0, ids[G].data_ptr(), grp[G].data_ptr() if grouped else None, dists[G].data_ptr(), bits[1:].data_ptr())
    before = lib.vtc_debug_launch_count()
    assert lib.vtc_l2_search_q8(*args, ws.data_ptr() + guard, need - 1, None) != 0 and b"workspace" in lib.vtc_last_error()
    assert lib.vtc_debug_launch_count() == before             # one byte too small: refused, nothing launched
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(stream):
            rc = lib.vtc_l2_search_q8(*args, ws.data_ptr() + guard, need, stream.cuda_stream)
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
    # the range passes, inside the same guards
    r2 = d64[:, 5].clone()
    need = lib.vtc_l2_range_workspace_bytes(ng, nq, d)
    ws = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    lims = torch.full((nq + 1 + 2 * G,), -77, dtype=torch.int64, device=DEV)
    assert lib.vtc_l2_range_count_q8(gal[8 * rb:].data_ptr(), tq.data_ptr(), mask[64:].data_ptr(), r2.data_ptr(), ng, nq, d, lims[G:].data_ptr(),
                                     bits[1:].data_ptr(), ws.data_ptr() + guard, need, None) == 0
    total = int(lims[G + nq])
    assert total == 6 * nq or grouped
    hits = torch.full((total + 2 * G,), -77, dtype=torch.int64, device=DEV)
    hd = torch.full((total + 2 * G,), -77.0, dtype=torch.float32, device=DEV)
    assert lib.vtc_l2_range_fill_q8(gal[8 * rb:].data_ptr(), tq.data_ptr(), ng, nq, d, lims[G:].data_ptr(), total, 0, hits[G:].data_ptr(),
                                    hd[G:].data_ptr(), None, ws.data_ptr() + guard, need, None) == 0
    torch.cuda.synchronize()
    assert bool((lims[:G] == -77).all()) and bool((lims[G + nq + 1:] == -77).all()) and bits.tolist() == [-77, 0, -77]
    assert bool((hits[:G] == -77).all()) and bool((hits[G + total:] == -77).all()) and bool((hits[G:G + total] >= 0).all())
    assert bool((hd[:G] == -77).all()) and bool((hd[G + total:] == -77).all())
    assert bool((ws[:guard] == 0xA5).all()) and bool((ws[guard + need:] == 0xA5).all())
    assert torch.equal(mask, mask_before) and torch.equal(gal, gal_before)


# ---- 7. VideoIndex -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw_rows():
    import rank_refs as RR
    rng = np.random.default_rng(41)
    a, b = RR.spread_pairs(400, 100, 27)                      # 100 columns: padded to 128
    scale = np.exp(rng.uniform(-1, 1, (400, 1))).astype(np.float32)
    vids = rng.integers(0, 50, 400) * 1000 + 7
    a = (a * scale).astype(np.float32)
    a[301] = a[300] * np.float32(2.0)                         # scaled exactly: the same unit row, a bit-equal stored duplicate
    return a, (b * scale).astype(np.float32), vids


def _pair(rows, vids=None):
    """An int8 index (added to in two calls) and the fp32 index of its dequantised stored rows (normalized=True: taken as they are)."""
    from vtc_amd.host.search import VideoIndex
    q8 = VideoIndex(100, device=DEV, storage=torch.int8)
    q8.add(_t(rows[:150]), video_ids=None if vids is None else vids[:150])
    q8.add(_t(rows[150:]), video_ids=None if vids is None else vids[150:])
    wide = VideoIndex(100, device=DEV, normalized=True)
    wide.add(_ops().dequantize_rows_q8(q8.rows)[:, :100].contiguous(), video_ids=vids)
    return q8, wide


def test_video_index_storage_rows_and_add(raw_rows):
    from vtc_amd.host.search import VideoIndex
    ops = _ops()
    a, b, vids = raw_rows
    q8, wide = _pair(a, vids)
    assert q8.storage == torch.int8 and VideoIndex.STORAGE["int8"] == torch.int8 and q8.width == 128
    assert q8.rows.dtype == torch.int8 and tuple(q8.rows.shape) == (q8.ntotal, q8.width + 16) == (400, 144)
    unit = torch.nn.functional.pad(ops.normalize_rows(_t(a)), (0, 28))
    want = QR.pack_rows(*QR.quantize(unit.cpu().numpy()))
    assert np.array_equal(q8.rows.cpu().numpy(), want)                                  # fp32 normalisation, then the quantiser's rule
    assert bool((q8.rows[:, 100:128] == 0).all()) and bool((q8.rows[:, 132:] == 0).all())
    once = VideoIndex(100, device=DEV, storage=torch.int8)
    once.add(_t(a), video_ids=vids)
    assert torch.equal(once.rows, q8.rows)                                              # add in two calls equals one
    assert np.array_equal(wide.rows.cpu().numpy().view(np.uint32), QR.stored(want).view(np.uint32))
    bad = a[:3].copy()
    bad[1, 7] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        once.add(_t(bad), video_ids=[1, 2, 3])
    assert once.ntotal == 400
    with pytest.raises(ValueError, match="storage"):
        VideoIndex(100, device=DEV, storage=torch.bfloat16)
    with pytest.raises(ValueError, match="storage"):
        VideoIndex(100, device=DEV, storage=torch.uint8)


def test_video_index_every_search_method_equals_the_fp32_index_of_the_stored_rows(raw_rows):
    ops = _ops()
    a, b, vids = raw_rows
    q8, wide = _pair(a, vids)
    q = _t(b[:5])
    qn = ops.normalize_rows(q)                                # the fp32 index takes its queries as they are
    sub_ids = list(range(0, 400, 3))
    subs = {"subset": (q8.subset(sub_ids), wide.subset(sub_ids))}
    for rnd in range(2):                                      # second round: after a remove
        for k8, kw_ in ((None, None), subs["subset"]):
            kw = lambda i: {} if k8 is None else {"subset": (k8, kw_)[i]}
            _same(q8.search(q, 7, **kw(0)), wide.search(qn, 7, **kw(1)))
            _same(q8.search_videos(q, 7, **kw(0)), wide.search_videos(qn, 7, **kw(1)))
            _same(q8.range_search(q, 0.2, **kw(0)), wide.range_search(qn, 0.2, **kw(1)))
            _same((q8.range_count(q, 0.2, **kw(0)),), (wide.range_count(qn, 0.2, **kw(1)),))
        ids, scores = q8.search(q, 7)
        _same(q8.search(q, 7, after=ids[:, -1]), wide.search(qn, 7, after=ids[:, -1]))
        _same(q8.search(q, 7, exclude=ids[:, 0]), wide.search(qn, 7, exclude=ids[:, 0]))
        _same(q8.search_deep(q, 150), wide.search_deep(qn, 150))
        videos, rows, _ = q8.search_videos(q, 7)
        _same(q8.search_videos(q, 7, after=rows[:, -1], exclude_videos=videos[:, 0]),
              wide.search_videos(qn, 7, after=rows[:, -1], exclude_videos=videos[:, 0]))
        _same(q8.search_videos_deep(q, 45), wide.search_videos_deep(qn, 45))
        sets = _t(b[:24].reshape(4, 6, 100))
        setsn = ops.normalize_rows(_t(b[:24])).view(4, 6, 100)
        _same(q8.search_any(sets, 7, sizes=[6, 2, 1, 5], return_members=True), wide.search_any(setsn, 7, sizes=[6, 2, 1, 5], return_members=True))
        _same(q8.search_videos_any(sets, 7, exclude_videos=videos[:4, 0].contiguous()),
              wide.search_videos_any(setsn, 7, exclude_videos=videos[:4, 0].contiguous()))
        own = _t(np.array([300, 17, 399, -1, 5], np.int64))
        _same(q8.similar(own, 7), wide.similar(own, 7))
        _same(q8.similar_videos(own, 7), wide.similar_videos(own, 7))
        _same(q8.similar_within(own, 0.3), wide.similar_within(own, 0.3))
        _same(q8.similar_to_video([int(vids[0]), int(vids[9]), 123456], 7), wide.similar_to_video([int(vids[0]), int(vids[9]), 123456], 7))
        _same(q8.near_duplicates(0.5), wide.near_duplicates(0.5))
        r8, rw = q8.range_subset(q[0], 0.1), wide.range_subset(qn[0], 0.1)
        assert torch.equal(r8.words(), rw.words())
        _same(q8.search(q, 3, subset=r8), wide.search(qn, 3, subset=rw))
        # the batch forms ARE the scan on an int8 index
        q70 = _t(b[:70])
        _same(q8.search_many(q70, 7), q8.search(q70, 7))
        _same(q8.range_search_many(q70, 0.2), q8.range_search(q70, 0.2))
        _same((q8.range_count_many(q70, 0.2),), (q8.range_count(q70, 0.2),))
        _same(q8.search_many(q70, 7), wide.search(ops.normalize_rows(q70), 7, exclude=torch.full((70,), -1, dtype=torch.int64, device=DEV)))
        if rnd == 0:
            # a bit-equal duplicate scores exactly 1: the query is the row as stored
            assert torch.equal(q8.rows[300], q8.rows[301])
            ids, scores = q8.similar(own[:1], 3)
            assert int(ids[0, 0]) == 301 and float(scores[0, 0]) == 1.0
            gone = [int(i) for i in q8.search(q, 7)[0][:, 0].tolist()]
            assert q8.remove(gone) == wide.remove(gone) == len(set(gone))
            assert q8.remove_videos([int(vids[3])]) == wide.remove_videos([int(vids[3])]) > 0
    # (B): the reference over the stored rows
    ids, scores = q8.search(q, 7)
    alive = q8.live_mask.cpu().numpy()
    want = QR.reference_search_masked(q8.rows.cpu().numpy(), torch.nn.functional.pad(qn, (0, 28)).cpu().numpy(), alive, 7)
    assert want[2] > 1e-12 and np.array_equal(ids.cpu().numpy(), want[0])
    assert np.allclose((2.0 * (1.0 - scores)).cpu().numpy(), want[1], rtol=0, atol=4e-7)


def test_video_index_seventy_queries_are_two_slices_and_nothing_syncs(raw_rows):
    from vtc_amd import _lib as L
    a, b, vids = raw_rows
    q8, _ = _pair(a, vids)
    q = b[:70].copy()
    q[66, 5] = np.nan
    q = _t(q)
    sub = q8.subset(list(range(0, 400, 2)))
    warm = (q8.search(q, 5), q8.search(q, 5, subset=sub), q8.search_videos(q, 5), (q8.range_count(q, 0.2),))
    torch.cuda.synchronize()
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = (q8.search(q, 5), q8.search(q, 5, subset=sub), q8.search_videos(q, 5), (q8.range_count(q, 0.2),))
        q8.search(q[:1], 5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for x, y in zip(got, warm):
        _same(x, y)
    launches = lib.vtc_debug_launch_count() - before
    mark = lib.vtc_debug_launch_count()
    q8.search(q[:1], 5)
    single = lib.vtc_debug_launch_count() - mark               # normalisation + scan + merge
    mark = lib.vtc_debug_launch_count()
    q8.range_count(q, 0.2)
    assert launches == 3 * (single + 2) + (lib.vtc_debug_launch_count() - mark) + single      # each 70-query search: one more scan and merge
    ids, scores = got[0]
    assert tuple(ids.shape) == (70, 5)
    for i in (0, 63, 64, 69):
        i1, s1 = q8.search(q[i:i + 1], 5)
        assert torch.equal(ids[i:i + 1], i1) and torch.equal(scores[i:i + 1], s1), i
    assert bool((ids[66] == -1).all()) and bool(torch.isneginf(scores[66]).all()) and bool((ids[65] >= 0).all())


def test_video_index_state_dict_and_converted(raw_rows):
    from vtc_amd.host.search import VideoIndex
    ops = _ops()
    a, b, vids = raw_rows
    q8, wide = _pair(a, vids)
    q8.remove([3, 5, 399])
    q = _t(b[:4])
    state = q8.state_dict()
    assert state["storage"] == "int8" and state["rows"].dtype == torch.int8 and tuple(state["rows"].shape) == (400, 100)
    assert state["scales"].dtype == torch.float32 and tuple(state["scales"].shape) == (400,)
    other = VideoIndex(100, device=DEV, storage=torch.int8)
    other.load_state_dict({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in state.items()})
    assert torch.equal(other.rows, q8.rows) and len(other) == 397 and other.ntotal == 400
    _same(other.search(q, 5), q8.search(q, 5))
    _same(other.search_videos(q, 5), q8.search_videos(q, 5))
    with pytest.raises(ValueError, match="storage"):
        VideoIndex(100, device=DEV).load_state_dict(state)
    with pytest.raises(ValueError, match="storage"):
        VideoIndex(100, device=DEV, storage=torch.float16).load_state_dict(state)
    half = VideoIndex(100, device=DEV, storage=torch.float16)
    half.add(_t(a[:50]))
    with pytest.raises(ValueError, match="storage"):
        VideoIndex(100, device=DEV, storage=torch.int8).load_state_dict(half.state_dict())      # a half state is refused
    low = dict(state, scales=(state["scales"].view(torch.int32) | 1).view(torch.float32))
    with pytest.raises(ValueError, match="low 8"):
        VideoIndex(100, device=DEV, storage=torch.int8).load_state_dict(low)
    nan = dict(state, scales=state["scales"].clone())
    nan["scales"][7] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        VideoIndex(100, device=DEV, storage=torch.int8).load_state_dict(nan)
    with pytest.raises(ValueError, match="scales"):
        VideoIndex(100, device=DEV, storage=torch.int8).load_state_dict({k: v for k, v in state.items() if k != "scales"})
    assert set(wide.state_dict()) == {"rows", "count", "dim", "normalized", "video_ids"}           # fp32 and half keep their keys
    assert set(half.state_dict()) == {"rows", "count", "dim", "normalized", "storage"}
    # converted, all six directions
    stored = ops.dequantize_rows_q8(q8.rows)
    up = q8.converted(torch.float32)                                                               # int8 -> fp32: exact
    assert up.storage == torch.float32 and torch.equal(up.rows.view(torch.int32), stored.view(torch.int32))
    down = q8.converted(torch.float16)                                                             # int8 -> half: dequantised, then rounded
    assert down.storage == torch.float16 and torch.equal(down.rows.view(torch.int16), stored.to(torch.float16).view(torch.int16))
    back = wide.converted(torch.int8)                                                              # fp32 -> int8: the stored rows quantised
    assert back.storage == torch.int8 and torch.equal(back.rows, ops.quantize_rows_q8(wide.rows)) and torch.equal(back.rows, q8.rows)
    hq = down.converted(torch.int8)                                                                # half -> int8: the widened rows quantised
    assert torch.equal(hq.rows, ops.quantize_rows_q8(down.rows.float()))
    f2h, h2f = wide.converted(torch.float16), down.converted(torch.float32)                        # the two that were there
    assert torch.equal(f2h.rows.view(torch.int16), wide.rows.to(torch.float16).view(torch.int16)) and torch.equal(h2f.rows, down.rows.float())
    copy = q8.converted(torch.int8)
    assert torch.equal(copy.rows, q8.rows) and copy._rows.data_ptr() != q8._rows.data_ptr()
    for new in (up, down, hq, copy):
        assert new.ntotal == 400 and len(new) == 397 and torch.equal(new.live_mask, q8.live_mask) and torch.equal(new.video_ids, q8.video_ids)
        assert new.normalized == q8.normalized and new.grouped
    assert back.ntotal == 400 and back.grouped
    _same(up.search_videos(q, 5), q8.search_videos(q, 5))
    first = copy.add(_t(a[:2]), video_ids=[1, 2])
    assert first == 400 and copy.ntotal == 402 and q8.ntotal == 400 and tuple(copy.rows.shape) == (402, 144)
    empty = VideoIndex(100, device=DEV).converted(torch.int8)
    assert empty.ntotal == 0 and tuple(empty.rows.shape) == (0, 144) and empty.add(_t(a[:2])) == 0 and len(empty) == 2


def test_video_index_text_wrappers_on_an_int8_index():
    from oracle import arch as A
    from vtc_amd.host import model as HM
    from vtc_amd.host.clip_arch import ClipConfig
    from vtc_amd.host.search import VideoIndex
    ops = _ops()
    torch.set_grad_enabled(False)
    arch = A.TINY
    m = HM.PretrainedCLIP(model_type=ClipConfig(**asdict(arch)))
    m.load_state_dict(A.synth_model(arch, 7, "clip"), strict=True)
    m = m.eval().to(DEV)
    dim = arch.embed_dim
    rng = np.random.default_rng(32)
    q8 = VideoIndex(dim, device=DEV, storage=torch.int8)
    q8.add(_t(rng.standard_normal((200, dim)).astype(np.float32)), video_ids=np.arange(200) // 4)
    wide = VideoIndex(dim, device=DEV, normalized=True)
    wide.add(ops.dequantize_rows_q8(q8.rows)[:, :dim].contiguous(), video_ids=np.arange(200) // 4)
    tokens = A.synth_tokens(6, arch, 9).to(DEV)
    qn = ops.normalize_rows(ops.normalize_rows(m.encode_text(tokens).float().contiguous()))       # search normalises once more
    _same(q8.search_text(m, tokens, 7), wide.search(qn, 7))
    _same(q8.search_videos_text(m, tokens, 7), wide.search_videos(qn, 7))
    _same(q8.range_search_text(m, tokens, 0.0), wide.range_search(qn, 0.0))
    _same(q8.search_any_text(m, tokens.view(2, 3, -1), 7), wide.search_any(qn.view(2, 3, -1), 7))
    _same(q8.search_videos_any_text(m, tokens.view(2, 3, -1), 7), wide.search_videos_any(qn.view(2, 3, -1), 7))


def test_the_documented_int8_example_runs():
    """INTEGRATION.md's int8 block, executed as written: its own asserts hold the storage, the conversions and the state dict."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "torch.int8" in b]
    assert len(blocks) == 1, len(blocks)
    ns = {}
    exec(blocks[0], ns)
    assert tuple(ns["ids"].shape) == (3, 10) and bool((ns["ids"] >= 0).all()) and torch.equal(ns["other"].rows, ns["index"].rows)
