"""GPU: the masked query-time search (vtc_l2_search_masked / ops.l2_search(live=...), vtc_row_mask_pack / ops.row_mask_pack, and
VideoIndex.remove / subset) against the numpy reference of tests/search_mask_refs.py -- the unmasked search over the gallery compacted
to its live rows, ids mapped back -- and bit for bit against the library's own unmasked entry points over the compacted gallery.

Ids are compared with exact equality; every case asserts the reference's min_gap > 1e-12 first (tests/search_refs.py).  fp32 dists are
within one fp32 ulp of the reference, and bit-equal between the library's entry points."""
from dataclasses import asdict

import numpy as np
import pytest
import torch

import rank_refs as RR
import search_mask_refs as MR
import search_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ops():
    from vtc_amd import ops
    return ops


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _words(live):
    return _t(MR.pack_words(live).view(np.int32))


def _check_against_reference(gallery, queries, live, depth, id_base=0, want_bits=0, tg=None, tq=None):
    ops = _ops()
    want_ids, want_d, gap = MR.reference_search_masked(gallery, queries, live, depth, id_base)
    assert gap > 1e-12, gap
    ids, dists, bits = ops.l2_search(_t(gallery) if tg is None else tg, _t(queries) if tq is None else tq, depth, id_base=id_base,
                                     live=_words(live))
    assert ids.dtype == torch.int64 and dists.dtype == torch.float32 and tuple(ids.shape) == (queries.shape[0], depth)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    SR.assert_dists_within_one_ulp(dists.cpu().numpy(), want_d)
    assert int(bits.item()) == want_bits
    return ids, dists


# ---- edge shapes x mask kinds -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spread64():
    return RR.spread_pairs(1027, 64, 21)


@pytest.mark.parametrize("ng,nq,depth", MR.edge_cases())
def test_edge_shapes_and_mask_kinds(spread64, ng, nq, depth):
    a, b = spread64
    tg, tq = _t(a[:ng]), _t(b[:nq])
    for kind in MR.MASK_KINDS:
        live = MR.make_mask(kind, ng, seed=ng)
        ids, _ = _check_against_reference(a[:ng], b[:nq], live, depth, tg=tg, tq=tq)
        if not live.any():
            assert bool((ids == -1).all())


@pytest.mark.parametrize("ng", [33, 1027])
def test_garbage_bits_above_the_last_row_are_ignored(spread64, ng):
    ops = _ops()
    a, b = spread64
    tg, tq = _t(a[:ng]), _t(b[:9])
    live = MR.make_mask("random_0.5", ng, seed=ng)
    clean = MR.pack_words(live)
    dirty = clean.copy()
    dirty[-1] |= np.uint32((0xFFFFFFFF << (ng & 31)) & 0xFFFFFFFF)
    assert ng & 31 and dirty[-1] != clean[-1]
    depth = min(11, ng)
    need = ops.l2_search_workspace_bytes(ng, 9, 64, depth)
    out = []
    for w in (clean, dirty):
        ws = ops.workspace(need, tg.device)
        ids, dists, bits = ops.l2_search(tg, tq, depth, live=_t(w.view(np.int32)), ws=ws)
        out.append((ids, dists, ops.search_dists64(ws, 9, depth).clone(), bits))
    for x, y in zip(*out):
        assert torch.equal(x, y)
    assert np.array_equal(out[0][0].cpu().numpy(), MR.reference_search_masked(a[:ng], b[:9], live, depth)[0])


@pytest.mark.parametrize("d", [192, 512, 2048])
def test_feature_widths(d):
    a, b = RR.spread_pairs(1027, d, 22)
    _check_against_reference(a, b[:9], MR.make_mask("random_0.5", 1027, seed=d), 11)


def test_more_rows_than_the_grid_has_waves():
    a, b = RR.spread_pairs(40013, 64, 23)
    _check_against_reference(a, b[:3], MR.make_mask("random_0.3", 40013, seed=1), 64)


# ---- the same bits as the library's unmasked entry points over the compacted gallery ----------------------------------------------
@pytest.fixture(scope="module")
def spread512():
    a, b = RR.spread_pairs(1500, 512, 24)
    return a, b, _t(a), _t(b)


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 8, 64])
def test_bit_for_bit_against_the_compacted_gallery(spread512, nq):
    from vtc_amd import _lib as L
    ops = _ops()
    _, _, ta, tb = spread512
    depth = 40
    live = MR.make_mask("random_0.5", 1500, seed=nq)
    idx = _t(np.flatnonzero(live))
    q = tb[200:200 + nq].contiguous()
    need = ops.l2_search_workspace_bytes(1500, nq, 512, depth)
    ws, ws2 = ops.workspace(need, ta.device), ops.workspace(need, ta.device)
    ids, dists, bits = ops.l2_search(ta, q, depth, live=_words(live), ws=ws)
    compact = ta[idx].contiguous()
    ids2, dists2, _ = ops.l2_search(compact, q, depth, ws=ws2)
    assert int(bits.item()) == 0
    assert torch.equal(ids, idx[ids2]) and torch.equal(dists, dists2)
    assert torch.equal(ops.search_dists64(ws, nq, depth), ops.search_dists64(ws2, nq, depth))
    ids3, dists3 = ops.l2_topk(compact, q, depth, precision=L.SWEEP_EXACT)
    assert torch.equal(ids, idx[ids3]) and torch.equal(dists, dists3)
    # an all-live mask against no mask at all
    ids4, dists4, _ = ops.l2_search(ta, q, depth, live=_words(np.ones(1500, bool)), ws=ws)
    d64 = ops.search_dists64(ws, nq, depth).clone()
    ids5, dists5, _ = ops.l2_search(ta, q, depth, ws=ws)
    assert torch.equal(ids4, ids5) and torch.equal(dists4, dists5) and torch.equal(d64, ops.search_dists64(ws, nq, depth))


# ---- dead rows influence nothing ---------------------------------------------------------------------------------------------------
def test_poisoned_dead_rows(spread64):
    a, b = spread64
    ng, nq, depth = 257, 9, 11
    g, q = a[:ng].copy(), b[:nq]
    live = MR.make_mask("random_0.5", ng, seed=5)
    dead = np.flatnonzero(~live)
    assert dead.size > 40
    nan_rows, inf_rows, copies = dead[0:8], dead[8:16], dead[16:16 + nq]
    g[nan_rows, 3] = np.nan
    g[inf_rows, 60] = np.inf
    g[inf_rows[0]] = -np.inf
    g[copies] = q                                             # distance 0 to a query: would head every list
    ids, _ = _check_against_reference(g, q, live, depth, want_bits=0)
    assert not np.isin(ids.cpu().numpy(), dead).any()
    live[nan_rows[2]] = True                                  # one NaN row comes to life: the word says so, the row is still never returned
    ids, _ = _check_against_reference(g, q, live, depth, want_bits=1)
    assert not np.isin(ids.cpu().numpy(), np.flatnonzero(~live)).any() and not (ids == int(nan_rows[2])).any()


def test_ties_go_to_the_lower_live_row():
    """Gallery rows 99 .. 139 are bit-equal; 99 and the even ones up to 138 are dead, so the duplicates' query lists start 101, 103, 105."""
    a, b = RR.cluster_case(1500, 512)
    live = np.ones(1500, bool)
    live[99] = False
    live[100:140:2] = False
    ids, _ = _check_against_reference(a, b[90:154], live, 64, id_base=0)
    assert ids[9, :3].tolist() == [101, 103, 105]


# ---- windows -------------------------------------------------------------------------------------------------------------------------
def test_masked_windows_merged_equal_the_masked_whole(spread64):
    ops = _ops()
    a, b = spread64
    live = MR.make_mask("random_0.5", 1027, seed=9)
    live[340:350] = False                                     # a dead stretch across the cut at 343
    depth = 11
    cuts = [0, 343, 685, 1027]
    tg, tq = _t(a), _t(b[:9])
    whole_ids, whole_d, _ = ops.l2_search(tg, tq, depth, live=_words(live))
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        ids, d64, bits = ops.l2_search_part(tg[lo:hi], tq, min(depth, hi - lo), id_base=lo, live=_words(live[lo:hi]))
        assert int(bits.item()) == 0
        parts.append(ops.pad_search_part(ids, d64.clone(), depth))
    ids, dists = ops.l2_search_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(ids, whole_ids) and torch.equal(dists, whole_d)
    assert np.array_equal(ids.cpu().numpy(), MR.reference_search_masked(a, b[:9], live, depth)[0])


# ---- containment -------------------------------------------------------------------------------------------------------------------
def test_no_write_outside_the_outputs_no_sync_any_stream(spread64):
    from vtc_amd import _lib as L
    lib = L.lib()
    a, b = spread64
    nq, depth, ng, d = 9, 11, 1027, 64
    live = MR.make_mask("random_0.5", ng, seed=11)
    want_ids, want_d, _ = MR.reference_search_masked(a, b[:nq], live, depth)
    tg, tq = _t(a), _t(b[:nq])
    G = 4                                                     # guard rows on each side
    ids = torch.full((nq + 2 * G, depth), -77, dtype=torch.int64, device=DEV)
    dists = torch.full((nq + 2 * G, depth), -77.0, dtype=torch.float32, device=DEV)
    need = lib.vtc_l2_search_workspace_bytes(ng, nq, d, depth)
    guard = 4096
    ws = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    words = MR.pack_words(live).view(np.int32)
    mask = torch.full((words.size + 2 * 64,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)      # the words between two guard bands of 64
    mask[64:64 + words.size] = _t(words)
    mask_before = mask.clone()
    bits = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(stream):
            rc = lib.vtc_l2_search_masked(tg.data_ptr(), tq.data_ptr(), mask[64:].data_ptr(), ng, nq, d, depth, 0, ids[G].data_ptr(),
                                          dists[G].data_ptr(), bits.data_ptr(), ws.data_ptr() + guard, need, stream.cuda_stream)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert rc == 0, lib.vtc_last_error()
    stream.synchronize()
    assert np.array_equal(ids[G:G + nq].cpu().numpy(), want_ids)
    SR.assert_dists_within_one_ulp(dists[G:G + nq].cpu().numpy(), want_d)
    assert int(bits.item()) == 0
    assert bool((ids[:G] == -77).all()) and bool((ids[G + nq:] == -77).all())
    assert bool((dists[:G] == -77.0).all()) and bool((dists[G + nq:] == -77.0).all())
    assert bool((ws[:guard] == 0xA5).all()) and bool((ws[guard + need:] == 0xA5).all())
    assert torch.equal(mask, mask_before)                     # the scan only reads the mask
    d64 = ws[guard:guard + nq * depth * 8].view(torch.float64).view(nq, depth)
    assert torch.equal(d64.to(torch.float32), dists[G:G + nq])


# ---- the packer ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 1027])
def test_row_mask_pack(n):
    ops = _ops()
    rng = np.random.default_rng(100 + n)
    flags = rng.random(n) < 0.5
    flags[-1] = True
    want = MR.pack_words(flags)
    got = ops.row_mask_pack(_t(flags))
    assert got.dtype == torch.int32 and tuple(got.shape) == ((n + 31) // 32,)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(ops.row_mask_pack(_t(flags.astype(np.uint8) * 200)).cpu().numpy().view(np.uint32), want)
    other = rng.random(n) < 0.5
    and_words = MR.pack_words(other)
    and_words[-1] |= np.uint32((0xFFFFFFFF << (n & 31)) & 0xFFFFFFFF) if n & 31 else np.uint32(0)      # garbage in the AND mask's tail
    got = ops.row_mask_pack(_t(flags), and_mask=_t(and_words.view(np.int32))).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, MR.pack_words(flags & other))
    if n & 31:                                                # the tail bits are written as 0
        assert int(got[-1]) >> (n & 31) == 0


# ---- VideoIndex ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw_rows():
    rng = np.random.default_rng(31)
    a, b = RR.spread_pairs(600, 100, 25)                       # 100 columns: padded to 128
    scale = np.exp(rng.uniform(-1, 1, (600, 1))).astype(np.float32)
    return (a * scale).astype(np.float32), (b * scale).astype(np.float32)


def _index(rows):
    from vtc_amd.host.search import VideoIndex
    index = VideoIndex(100, device=DEV)
    index.add(_t(rows))
    return index


def test_video_index_remove(raw_rows):
    a, b = raw_rows
    index = _index(a[:500])
    q = _t(b[:9])
    assert len(index) == 500 and index.ntotal == 500 and bool(index.live_mask.all())
    gone = [3, 17, 17, 250, 499]
    assert index.remove(gone) == 4
    assert index.remove(torch.tensor([17, 250])) == 0 and index.remove([]) == 0      # idempotent
    assert len(index) == 496 and index.ntotal == 500 and tuple(index.rows.shape) == (500, 128)
    keep = np.setdiff1d(np.arange(500), gone)
    mask = index.live_mask
    assert mask.dtype == torch.bool and tuple(mask.shape) == (500,) and np.array_equal(np.flatnonzero(mask.cpu().numpy()), keep)
    ids, scores = index.search(q, 11)
    fresh = _index(a[keep])
    ids2, scores2 = fresh.search(q, 11)
    assert torch.equal(ids, _t(keep)[ids2]) and torch.equal(scores, scores2)
    for bad in ([500], [-1], [5, 7, 10 ** 12]):               # out of range: raises and changes nothing
        with pytest.raises(ValueError, match="ntotal"):
            index.remove(bad)
    assert len(index) == 496 and torch.equal(index.live_mask, mask)
    assert index.add(_t(a[500:520])) == 500                   # ids are never reused
    assert len(index) == 516 and index.ntotal == 520 and int(index.live_mask.sum()) == 516
    assert index.remove([3, 519]) == 1 and len(index) == 515


def test_video_index_state_dict(raw_rows):
    from vtc_amd.host.search import VideoIndex
    a, b = raw_rows
    index = _index(a[:300])
    q = _t(b[:4])
    assert set(index.state_dict()) == {"rows", "count", "dim", "normalized"}          # nothing removed: today's keys
    index.remove([0, 5, 299])
    state = index.state_dict()
    assert set(state) == {"rows", "count", "dim", "normalized", "live"} and state["count"] == 300
    assert state["live"].dtype == torch.bool and tuple(state["live"].shape) == (300,) and int(state["live"].sum()) == 297
    ids, scores = index.search(q, 5)
    other = VideoIndex(100, device=DEV)
    other.load_state_dict({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in state.items()})
    assert len(other) == 297 and other.ntotal == 300
    ids2, scores2 = other.search(q, 5)
    assert torch.equal(ids, ids2) and torch.equal(scores, scores2)
    assert not np.isin(ids.cpu().numpy(), [0, 5, 299]).any()
    plain = VideoIndex(100, device=DEV)                       # the form without "live" still loads
    plain.load_state_dict({k: v for k, v in state.items() if k != "live"})
    assert len(plain) == 300 and set(plain.state_dict()) == {"rows", "count", "dim", "normalized"}


def test_video_index_subset(raw_rows):
    ops = _ops()
    a, b = raw_rows
    index = _index(a[:400])
    q = _t(b[:9])
    members = np.random.default_rng(41).random(400) < 0.3
    by_mask = index.subset(_t(members))
    by_ids = index.subset(np.flatnonzero(members).tolist())
    ids, scores = index.search(q, 11, subset=by_mask)
    ids_b, scores_b = index.search(q, 11, subset=by_ids)
    assert torch.equal(ids, ids_b) and torch.equal(scores, scores_b)
    want_ids, want_d, _ = ops.l2_search(index.rows, index._prepared(q, "queries", check=False), 11, live=_words(members))
    assert torch.equal(ids, want_ids) and torch.equal(scores, 1.0 - want_d / 2.0)
    assert members[ids.cpu().numpy()].all()
    # intersected with removals: the cached words follow the index
    gone = np.flatnonzero(members)[:5]
    assert index.remove(gone.tolist()) == 5
    ids, _ = index.search(q, 11, subset=by_mask)
    still = members.copy()
    still[gone] = False
    want_ids, _, _ = ops.l2_search(index.rows, index._prepared(q, "queries", check=False), 11, live=_words(still))
    assert torch.equal(ids, want_ids) and not np.isin(ids.cpu().numpy(), gone).any()
    # rows added after the subset was built are not members, however near they are
    first = index.add(q)
    assert first == 400
    ids2, _ = index.search(q, 11, subset=by_mask)
    assert torch.equal(ids2, ids) and int(ids2.max()) < 400
    assert bool((index.search(q, 1)[0][:, 0] == torch.arange(400, 409, device=DEV)).all())      # unrestricted, a query finds itself
    with pytest.raises(ValueError, match="another index"):
        _index(a[:400]).search(q, 11, subset=by_mask)
    with pytest.raises(ValueError, match="ntotal"):
        index.subset([0, 409])
    with pytest.raises(ValueError, match="ntotal"):
        index.subset(torch.ones(400, dtype=torch.bool))


def test_video_index_masked_bounds(raw_rows):
    a, b = raw_rows
    index = _index(a[:300])
    q = _t(b[:4])
    index.remove(list(range(10, 300)))
    assert len(index) == 10
    with pytest.raises(ValueError, match="k="):
        index.search(q, 11)
    ids, _ = index.search(q, 10)
    assert sorted(ids[0].tolist()) == list(range(10))
    few = index.subset([1, 4, 7, 200])                        # three live members (200 was removed): fewer than k
    ids, scores = index.search(q, 5, subset=few)
    assert bool((ids[:, 3:] == -1).all()) and bool(torch.isneginf(scores[:, 3:]).all())
    assert all(sorted(row) == [1, 4, 7] for row in ids[:, :3].tolist()) and bool(torch.isfinite(scores[:, :3]).all())


def test_video_index_many_masked_queries_run_in_slices(raw_rows):
    """70 queries: two calls of the scan (64 + 6).  The same rows as one query at a time; a NaN query gets a row of -1 / -inf."""
    a, b = raw_rows
    index = _index(a[:500])
    index.remove([1, 2, 3])
    sub = index.subset(_t(np.random.default_rng(43).random(500) < 0.5))
    q = b[:70].copy()
    q[66, 5] = np.nan
    q = _t(q)
    ids, scores = index.search(q, 7, subset=sub)
    assert tuple(ids.shape) == (70, 7)
    for i in (0, 1, 63, 64, 65, 66, 69):
        ids1, scores1 = index.search(q[i:i + 1], 7, subset=sub)
        assert torch.equal(ids[i:i + 1], ids1) and torch.equal(scores[i:i + 1], scores1)
    assert bool((ids[66] == -1).all()) and bool(torch.isneginf(scores[66]).all()) and bool((ids[65] >= 0).all())


def test_video_index_prepared_subset_does_not_sync(raw_rows):
    a, b = raw_rows
    index = _index(a[:500])
    index.remove([0, 9])
    sub = index.subset(_t(np.random.default_rng(44).random(500) < 0.5))
    q = _t(b[:3])
    want_ids, want_scores = index.search(q, 5, subset=sub)   # (warm: workspace allocated, words packed)
    want_ids2, _ = index.search(q, 5)
    torch.cuda.synchronize()
    from vtc_amd import _lib as L
    torch.cuda.set_sync_debug_mode("error")
    try:
        before = L.lib().vtc_debug_launch_count()
        ids, scores = index.search(q, 5, subset=sub)
        masked_launches = L.lib().vtc_debug_launch_count() - before
        ids2, _ = index.search(q, 5)                           # removal alone: the index's own words
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(ids, want_ids) and torch.equal(scores, want_scores) and torch.equal(ids2, want_ids2)
    plain = _index(a[:500])
    plain.search(q, 5)
    before = L.lib().vtc_debug_launch_count()
    plain.search(q, 5)
    assert masked_launches == L.lib().vtc_debug_launch_count() - before      # an unchanged subset adds no launch over an unmasked query


def test_video_index_search_text_with_subset():
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
    index = VideoIndex(dim, device=DEV)
    index.add(_t(rng.standard_normal((200, dim)).astype(np.float32)))
    sub = index.subset(list(range(0, 200, 3)))
    tokens = A.synth_tokens(5, arch, 9).to(DEV)
    ids, scores = index.search_text(m, tokens, 7, subset=sub)
    want_ids, want_scores = index.search(ops.normalize_rows(m.encode_text(tokens)), 7, subset=sub)
    assert tuple(ids.shape) == (5, 7) and torch.equal(ids, want_ids) and torch.equal(scores, want_scores)
    assert bool((ids % 3 == 0).all())
