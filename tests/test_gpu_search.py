"""GPU: the query-time search (vtc_l2_search / ops.l2_search, ops.l2_search_merge, host.search.VideoIndex) against the numpy fp64 reference
of tests/search_refs.py, against the existing exact search (ops.l2_topk, EXACT) and against the rank sweep (ops.rank_bidir).

Ids are compared with exact equality -- every case asserts min_gap > 1e-12 first, so that no summation order can decide an id; exact
duplicates are bit-equal on the device too (one device function forms every distance) and go to the lower row.  fp32 dists are compared
within one fp32 ulp of the reference (numpy's summation order differs from the device's in the last fp64 bits), and bit for bit against the
entry points of the library itself."""
from dataclasses import asdict

import numpy as np
import pytest
import torch

import rank_refs as RR
import search_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ops():
    from vtc_amd import ops
    return ops


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _check_against_reference(gallery, queries, depth, id_base=0, want_bits=0):
    ops = _ops()
    want_ids, want_d, gap = SR.reference_search(gallery, queries, depth, id_base)
    assert gap > 1e-12, gap
    ids, dists, bits = ops.l2_search(_t(gallery), _t(queries), depth, id_base=id_base)
    assert ids.dtype == torch.int64 and dists.dtype == torch.float32 and tuple(ids.shape) == (queries.shape[0], depth)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    SR.assert_dists_within_one_ulp(dists.cpu().numpy(), want_d)
    assert int(bits.item()) == want_bits
    return ids, dists


# ---- edge shapes --------------------------------------------------------------------------------------------------------------------
NG = (1, 2, 63, 64, 65, 257, 1027)
NQ = (1, 2, 7, 8, 9, 33, 64)


def _depths(ng):
    return (1, min(11, ng), min(64, ng))


def _edge_cases():
    cases = set()
    for i, ng in enumerate(NG):
        for j, nq in enumerate(NQ):
            if (i - j) % 2 == 0:                              # half of the grid, every value of both axes, the depth kinds in rotation
                cases.add((ng, nq, _depths(ng)[(i + j) % 3]))
    for ng in (NG[0], NG[-1]):                                # the corners with every depth
        for nq in (NQ[0], NQ[-1]):
            for depth in _depths(ng):
                cases.add((ng, nq, depth))
    for ng in NG:                                             # every gallery size at its full depth
        cases.add((ng, 9, _depths(ng)[2]))
    return sorted(cases)


@pytest.fixture(scope="module")
def spread64():
    return RR.spread_pairs(1027, 64, 21)


@pytest.mark.parametrize("ng,nq,depth", _edge_cases())
def test_edge_shapes(spread64, ng, nq, depth):
    a, b = spread64
    _check_against_reference(a[:ng], b[:nq], depth)


@pytest.mark.parametrize("d", [192, 512, 576, 2048])
def test_feature_widths(d):
    """192 and 576 are no multiples of 256: the partial last chunk of the lane loop; 2048 is the widest row (a 64 KiB query tile)."""
    a, b = RR.spread_pairs(1027, d, 22)
    _check_against_reference(a, b[:9], 11)


def test_more_rows_than_the_grid_has_waves():
    a, b = RR.spread_pairs(40013, 64, 23)
    _check_against_reference(a, b[:3], 64)


def test_ties_and_int64_ids():
    """The 40 exact duplicates of gallery row 99 (queries 99 .. 139 are duplicates too) at depth 64, ids beyond 2^32."""
    a, b = RR.cluster_case(1500, 512)
    ids, _ = _check_against_reference(a, b[90:154], 64, id_base=2 ** 33)
    assert int(ids.min()) >= 2 ** 33


# ---- the same bits as the existing entry points -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spread512():
    a, b = RR.spread_pairs(1500, 512, 24)
    return a, b, _t(a), _t(b)


@pytest.mark.parametrize("depth", [11, 40])
def test_same_ids_and_dists_as_l2_topk_exact(spread512, depth):
    from vtc_amd import _lib as L
    ops = _ops()
    _, _, ta, tb = spread512
    q = tb[:64].contiguous()
    ids, dists, _ = ops.l2_search(ta, q, depth)
    ids2, dists2 = ops.l2_topk(ta, q, depth, precision=L.SWEEP_EXACT)
    assert torch.equal(ids, ids2)
    assert torch.equal(dists, dists2)


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 8])
def test_every_tile_shape_forms_the_bits_of_l2_topk_exact(spread512, nq):
    """1, 2, 3 - 4 and 5 - 64 queries run four instantiations of the scan (tiles of 1 x 4, 2 x 4, 4 x 2 and 8 x 1 queries x rows): each
    must give a distance the bits the existing search gives it -- the compiler contracts multiply-adds per instantiation."""
    from vtc_amd import _lib as L
    ops = _ops()
    _, _, ta, tb = spread512
    q = tb[200:200 + nq].contiguous()
    ids, dists, _ = ops.l2_search(ta, q, 40)
    ids2, dists2 = ops.l2_topk(ta, q, 40, precision=L.SWEEP_EXACT)
    assert torch.equal(ids, ids2)
    assert torch.equal(dists, dists2)


def test_a_workspace_that_does_not_fit_is_refused(spread512):
    """The caller reads the fp64 list out of the workspace it passed: a silent fresh one would leave it reading stale bytes."""
    ops = _ops()
    _, _, ta, tb = spread512
    need = ops.l2_search_workspace_bytes(1500, 4, 512, 11)
    with pytest.raises(ValueError, match="workspace"):
        ops.l2_search(ta, tb[:4].contiguous(), 11, ws=ops.workspace(need - 256, ta.device))
    ws = ops.workspace(need, ta.device)
    _, dists, _ = ops.l2_search(ta, tb[:4].contiguous(), 11, ws=ws)
    assert torch.equal(ops.search_dists64(ws, 4, 11).to(torch.float32), dists)


def test_same_definition_as_the_rank_sweep(spread512):
    ops = _ops()
    _, _, ta, tb = spread512
    depth = 11
    rank_a, _, bits = ops.rank_bidir(ta, tb)
    assert int(bits.item()) == 0
    ids, _, _ = ops.l2_search(ta, tb[700:764].contiguous(), depth)
    ids, rank_a = ids.cpu().numpy(), rank_a.cpu().numpy()
    inside = 0
    for r, i in enumerate(range(700, 764)):
        if rank_a[i] < depth:
            assert ids[r, rank_a[i]] == i
            inside += 1
        else:
            assert i not in ids[r]
    assert 0 < inside < 64                                    # both branches were taken


# ---- non-finite ---------------------------------------------------------------------------------------------------------------------
def test_nonfinite_gallery_rows_are_never_returned(spread64):
    a, b = spread64
    g = a[:257].copy()
    g[5, 3] = np.nan
    g[200, 63] = np.inf
    ids, _ = _check_against_reference(g, b[:9], 11, want_bits=1)
    assert not np.isin(ids.cpu().numpy(), [5, 200]).any()
    _check_against_reference(g, g[[6, 201]], 64, want_bits=1)            # the rows next to them, as queries, at full depth


def test_nonfinite_query_gets_an_empty_row(spread64):
    a, b = spread64
    q = b[:9].copy()
    q[4, 17] = np.nan
    q[8, 0] = -np.inf
    ids, dists = _check_against_reference(a[:257], q, 11, want_bits=2)
    assert bool((ids[[4, 8]] == -1).all()) and bool(torch.isinf(dists[[4, 8]]).all()) and bool((ids[[0, 1, 2, 3, 5, 6, 7]] >= 0).all())
    g = a[:257].copy()
    g[100, 1] = np.nan
    _check_against_reference(g, q, 11, want_bits=3)                       # both words; the gallery's is found although a query is NaN


def test_fewer_finite_rows_than_depth(spread64):
    a, b = spread64
    g = a[:5].copy()
    g[1, 0] = np.nan
    g[3, 9] = np.inf
    ids, dists = _check_against_reference(g, b[:2], 5, want_bits=1)
    assert bool((ids[:, 3:] == -1).all()) and bool(torch.isinf(dists[:, 3:]).all()) and bool((ids[:, :3] >= 0).all())


# ---- windows ------------------------------------------------------------------------------------------------------------------------
def test_windows_merged_equal_the_whole_search(spread64):
    """Duplicates on both sides of every cut: the merge has to decide them on the fp64 distance and then on the id."""
    ops = _ops()
    a, b = spread64
    g = a.copy()
    g[1] = g[0]                                               # across the cut at 1 (a window of ONE row)
    g[340:347] = g[339]                                       # across 343
    g[680:690] = g[679]                                       # across 685
    g[1000] = g[339]                                          # a duplicate in a far window
    q = np.concatenate([g[[0, 339, 679]], b[[0, 339, 679, 5, 500]]])
    depth = 11
    cuts = [0, 1, 343, 685, 1027]
    assert SR.reference_search(g, q, depth)[2] > 1e-12
    tg, tq = _t(g), _t(q)
    whole_ids, whole_d, _ = ops.l2_search(tg, tq, depth)
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        ids, d64, _ = ops.l2_search_part(tg[lo:hi], tq, min(depth, hi - lo), id_base=lo)
        parts.append(ops.pad_search_part(ids, d64.clone(), depth))
    ids, dists = ops.l2_search_merge(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(ids, whole_ids) and torch.equal(dists, whole_d)
    assert ids[1, :9].tolist() == [339, 340, 341, 342, 343, 344, 345, 346, 1000]
    # the sharded entry point at world = 1 is the same path: local search + merge
    from vtc_amd import dist as vdist
    ids1, dists1 = vdist.sharded_search(tg, 0, tq, depth, 0, 1)
    assert torch.equal(ids1, whole_ids) and torch.equal(dists1, whole_d)


# ---- containment --------------------------------------------------------------------------------------------------------------------
def test_no_write_outside_the_outputs_no_sync_any_stream(spread64):
    from vtc_amd import _lib as L
    lib = L.lib()
    a, b = spread64
    nq, depth, ng, d = 9, 11, 1027, 64
    want_ids, want_d, _ = SR.reference_search(a, b[:nq], depth)
    tg, tq = _t(a), _t(b[:nq])
    G = 4                                                     # guard rows on each side
    ids = torch.full((nq + 2 * G, depth), -77, dtype=torch.int64, device=DEV)
    dists = torch.full((nq + 2 * G, depth), -77.0, dtype=torch.float32, device=DEV)
    need = lib.vtc_l2_search_workspace_bytes(ng, nq, d, depth)
    guard = 4096
    ws = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    bits = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(stream):
            rc = lib.vtc_l2_search(tg.data_ptr(), tq.data_ptr(), ng, nq, d, depth, 0, ids[G].data_ptr(), dists[G].data_ptr(), bits.data_ptr(),
                                   ws.data_ptr() + guard, need, stream.cuda_stream)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert rc == 0, lib.vtc_last_error()
    stream.synchronize()
    assert np.array_equal(ids[G:G + nq].cpu().numpy(), want_ids)
    SR.assert_dists_within_one_ulp(dists[G:G + nq].cpu().numpy(), want_d)
    assert bool((ids[:G] == -77).all()) and bool((ids[G + nq:] == -77).all())
    assert bool((dists[:G] == -77.0).all()) and bool((dists[G + nq:] == -77.0).all())
    assert bool((ws[:guard] == 0xA5).all()) and bool((ws[guard + need:] == 0xA5).all())
    # the documented head of the workspace: the fp64 distances of the result
    d64 = ws[guard:guard + nq * depth * 8].view(torch.float64).view(nq, depth)
    assert torch.equal(d64.to(torch.float32), dists[G:G + nq])


# ---- VideoIndex ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raw_rows():
    rng = np.random.default_rng(31)
    a, b = RR.spread_pairs(1027, 100, 25)                      # 100 columns: padded to 128
    scale = np.exp(rng.uniform(-1, 1, (1027, 1))).astype(np.float32)
    return (a * scale).astype(np.float32), (b * scale).astype(np.float32)


def test_video_index_matches_l2_search(raw_rows):
    from vtc_amd.host.search import VideoIndex
    ops = _ops()
    a, b = raw_rows
    index = VideoIndex(100, device=DEV)
    assert index.add(_t(a[:700])) == 0 and index.add(_t(a[700:])) == 700 and len(index) == 1027
    q = _t(b[:9])
    ids, scores = index.search(q, 11)
    pad = lambda x: torch.nn.functional.pad(ops.normalize_rows(x), (0, 28)).contiguous()       # noqa: E731
    want_ids, want_d, _ = ops.l2_search(pad(_t(a)), pad(q), 11)
    assert torch.equal(ids, want_ids) and torch.equal(scores, 1.0 - want_d / 2.0)
    assert ids.is_cuda and scores.is_cuda and ids.dtype == torch.int64 and scores.dtype == torch.float32
    # the same neighbours as the fp64 reference on the normalised rows
    ref_ids, _, gap = SR.reference_search(pad(_t(a)).cpu().numpy(), pad(q).cpu().numpy(), 11)
    assert gap > 1e-12 and np.array_equal(ids.cpu().numpy(), ref_ids)


def test_video_index_routes_agree(raw_rows):
    """65 queries go through ops.l2_topk(EXACT), one through ops.l2_search: the same rows either way, and so for 64 queries sent down
    each route in turn (the routing constant is a measured crossover, not a limit: both routes take 64)."""
    from vtc_amd.host.search import VideoIndex
    a, b = raw_rows
    index = VideoIndex(100, device=DEV)
    index.add(_t(a))
    q = _t(b[:65])
    assert 1 < VideoIndex.ROUTE_TOPK_MIN_QUERIES <= 65
    ids, scores = index.search(q, 11)
    ids_a, scores_a = index.search(q[:64], 11)
    ids_b, scores_b = index.search(q[64:], 11)
    assert torch.equal(ids, torch.cat([ids_a, ids_b])) and torch.equal(scores, torch.cat([scores_a, scores_b]))
    index.ROUTE_TOPK_MIN_QUERIES = 65                         # everything up to 64 queries through ops.l2_search
    ids_s, scores_s = index.search(q[:64], 11)
    index.ROUTE_TOPK_MIN_QUERIES = 1                          # everything through ops.l2_topk
    ids_t, scores_t = index.search(q[:64], 11)
    assert torch.equal(ids_s, ids_t) and torch.equal(scores_s, scores_t) and torch.equal(ids_s, ids_a)


def test_video_index_state_dict_and_errors(raw_rows):
    from vtc_amd.host.search import VideoIndex
    a, b = raw_rows
    index = VideoIndex(100, device=DEV)
    index.add(_t(a[:300]))
    q = _t(b[:4])
    ids, scores = index.search(q, 5)
    other = VideoIndex(100, device=DEV)
    other.load_state_dict({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in index.state_dict().items()})
    assert len(other) == 300
    ids2, scores2 = other.search(q, 5)
    assert torch.equal(ids, ids2) and torch.equal(scores, scores2)
    bad = a[:3].copy()
    bad[1, 7] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        index.add(_t(bad))
    assert len(index) == 300
    with pytest.raises(ValueError, match="k="):
        index.search(q, 301)
    with pytest.raises(ValueError, match="k="):
        VideoIndex(100, device=DEV).search(q, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        VideoIndex(100, device="cpu")


def test_video_index_few_queries_do_not_sync(raw_rows):
    """Fewer queries than the routing constant are only enqueued (batch 1 is the design point): no device-to-host read.  A NaN query is
    not rejected there; it gets ids -1 and scores -inf."""
    from vtc_amd.host.search import VideoIndex
    a, b = raw_rows
    index = VideoIndex(100, device=DEV)
    index.add(_t(a))
    q = _t(b[:2].copy())
    bad = b[:2].copy()
    bad[1, 3] = np.nan
    bad = _t(bad)
    want_ids, want_scores = index.search(q, 5)               # (warm: workspace allocated)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ids, scores = index.search(q, 5)
        ids_bad, scores_bad = index.search(bad, 5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(ids, want_ids) and torch.equal(scores, want_scores)
    assert torch.equal(ids_bad[0], want_ids[0]) and bool((ids_bad[1] == -1).all()) and bool(torch.isneginf(scores_bad[1]).all())
    nine = b[:VideoIndex.ROUTE_TOPK_MIN_QUERIES].copy()       # the l2_topk route checks its queries and raises
    nine[2, 0] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        index.search(_t(nine), 5)


def test_video_index_search_text_with_comments():
    """A *_finaltf model that adapts the text branch: search_text(title, comments) searches with the text features the wrapper's eval
    forward returns for the same titles and comments.  The two run the same towers and the same CAM; the forward ends in the two-set
    normalisation launch, search_text in the one-set one, so scores are compared to 1e-5 (unit rows that agree to fp32 rounding, 1e-7 per
    coordinate, give scores that agree to about 1e-6; a wrong adapter moves them by 0.1) and ids exactly."""
    from oracle import arch as A
    from vtc_amd.host import model as HM
    from vtc_amd.host.clip_arch import ClipConfig
    from vtc_amd.host.search import VideoIndex
    torch.set_grad_enabled(False)
    arch = A.TINY
    m = HM.PretrainedCLIP_finaltf(model_type=ClipConfig(**asdict(arch)), branch_to_adapt_val="text", n_heads=2)
    m.load_state_dict(A.synth_model(arch, 7, "clip_finaltf"), strict=True)
    m = m.eval().to(DEV)
    dim = arch.embed_dim
    rng = np.random.default_rng(33)
    index = VideoIndex(dim, device=DEV)
    index.add(_t(rng.standard_normal((200, dim)).astype(np.float32)))
    B = 4
    title = A.synth_tokens(B, arch, 9).to(DEV)
    comments = A.synth_tokens(B * 5, arch, 10, empty_frac=0.3).reshape(B, 5, -1).to(DEV)
    vis = _t(rng.standard_normal((B, dim)).astype(np.float32))            # precomputed visual features: the text branch does not read them
    ft = m(vis, title, comments)[1]
    ids, scores = index.search_text(m, title, 7, comments=comments)
    want_ids, want_scores = index.search(ft, 7)
    assert torch.equal(ids, want_ids)
    assert float((scores - want_scores).abs().max()) <= 1e-5
    plain_ids, plain_scores = index.search_text(m, title, 7)              # the comments do change the query
    assert float((scores - plain_scores).abs().max()) > 1e-4 or not torch.equal(ids, plain_ids)
    clip = HM.PretrainedCLIP(model_type=ClipConfig(**asdict(arch)))
    with pytest.raises(ValueError, match="branch_to_adapt_val"):
        index.search_text(clip, title, 7, comments=comments)


def test_video_index_search_text():
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
    tokens = A.synth_tokens(5, arch, 9).to(DEV)
    ids, scores = index.search_text(m, tokens, 7)
    want_ids, want_scores = index.search(ops.normalize_rows(m.encode_text(tokens)), 7)
    assert tuple(ids.shape) == (5, 7) and torch.equal(ids, want_ids) and torch.equal(scores, want_scores)
