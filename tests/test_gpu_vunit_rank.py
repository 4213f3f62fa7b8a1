"""GPU: the grouped rank sweep with the video-unit direction (vtc_l2_rank_grouped_vunit -> ops.rank_grouped_vunit ->
RecallAtK.grouped_ranks(video_to_text="video") -> compute_multi_caption_table / retrieval_evaluation) against the numpy fp64 references of
tests/grouped_rank_refs.py and tests/vunit_rank_refs.py.  All three outputs are compared with array_equal: the sweep is exact.  Every
comparison first checks its own data (tests/vunit_cases.py): the smallest relative gap between a target's distance and any other (not
bit-equal) distance exceeds 1e-12, and for n >= 63 max rank_v > n / 2, 0.2 < R@1 < 0.8 and the two conventions differ for at least
n / 5 videos."""
import numpy as np
import pytest
import torch

import grouped_rank_refs as GR
import vunit_cases as VC
import vunit_rank_refs as VR

pytestmark = pytest.mark.gpu


def _sweep(a, b, off, **kw):
    from vtc_amd import ops
    ra, rb, rv, bits = ops.rank_grouped_vunit(torch.tensor(a).cuda(), torch.tensor(b).cuda(), off, **kw)
    n, m = a.shape[0], b.shape[0]
    assert ra.dtype == rb.dtype == rv.dtype == torch.int64 and ra.shape == (m,) and rb.shape == (n,) and rv.shape == (n,)
    return ra.cpu().numpy(), rb.cpu().numpy(), rv.cpu().numpy(), int(bits.item())


def _check(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def _check_all(got, want):
    for g, w, what in zip(got, want, ("rank_a", "rank_b", "rank_v")):
        _check(g, w, what)


@pytest.mark.parametrize("kind,n,d,rpb", VC.EDGE + VC.BULK)
def test_edge_sizes_and_bulk_equal_the_fp64_reference(kind, n, d, rpb):
    """The shapes of the grouped sweep's own tests.  "3x85+2": m = 257, the last group lies across the block boundary at row 256;
    256 x 20 in 256-row blocks: every boundary cuts a group; n = 63 / 64 / 65 around a 64-column strip, padding columns at n % 4 != 0."""
    a, b, off, want_a, want_b, want_v = VC.case(kind, n, d)
    if kind == "3x85+2":
        assert b.shape[0] == 257
    VC.assert_not_degenerate(want_v, want_b, n)
    got = _sweep(a, b, off, rows_per_block=rpb)
    assert got[3] == 0
    _check_all(got, (want_a, want_b, want_v))


def test_a_group_larger_than_a_block():
    """m = 1053 in 256-row blocks: video 10's 600 captions span three blocks (two of them wholly), video 37's 300 span two."""
    a, b, off, want_a, want_b, want_v = VC.big_group_case()
    assert b.shape[0] == 1053 and off[11] - off[10] == 600 and off[38] - off[37] == 300
    assert off[10] // 256 + 2 <= (off[11] - 1) // 256 and off[37] // 256 < (off[38] - 1) // 256
    VC.assert_not_degenerate(want_v, want_b, 64)
    got = _sweep(a, b, off, rows_per_block=256)
    assert got[3] == 0
    _check_all(got, (want_a, want_b, want_v))


@pytest.mark.parametrize("n,d", VC.IDENTITY)
def test_identity_offsets_are_the_paired_sweep(n, d):
    """off = 0, 1, ..., n with m = n: rank_v is ops.rank_bidir's rank_b, rank_a and rank_b are ops.rank_grouped's, element for element."""
    from vtc_amd import ops
    a, b, want_a, want_b = VC.identity_case(n, d)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    pa, pb, _ = ops.rank_bidir(ta, tb, rows_per_block=256)
    ga, gb, _ = ops.rank_grouped(ta, tb, np.arange(n + 1), rows_per_block=256)
    ra, rb, rv, bits = ops.rank_grouped_vunit(ta, tb, np.arange(n + 1), rows_per_block=256)
    assert int(bits.item()) == 0
    assert torch.equal(rv, pb) and torch.equal(ra, ga) and torch.equal(rb, gb) and torch.equal(ra, pa)
    _check(rv.cpu().numpy(), want_b, "rank_v")
    _check(ra.cpu().numpy(), want_a, "rank_a")


def test_forced_pool_overflow_changes_nothing():
    """reach_capacity = 8 on the 256 x 20 case: videos miss the pool of the video-unit direction and go to the fp64 brute force."""
    from vtc_amd import _lib as L
    from vtc_amd import ops
    n, d = 256, 64
    a, b, off, want_a, want_b, want_v = VC.case(20, n, d)
    m = b.shape[0]
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ws = ops.workspace(L.lib().vtc_l2_rank_grouped_vunit_workspace_bytes(n, m, d, 256, 8), ta.device)
    got = ops.rank_grouped_vunit(ta, tb, off, rows_per_block=256, reach_capacity=8, ws=ws)
    _check_all([x.cpu().numpy() for x in got[:3]], (want_a, want_b, want_v))
    st = ops.rank_sweep_stats(ws)
    assert st["vunit_in_reach"] > 8 and st["vunit_brute_force_owners"] > 0 and st["vunit_in_reach_max"] > 0, st
    ws2 = ops.workspace(L.lib().vtc_l2_rank_grouped_vunit_workspace_bytes(n, m, d, 256, 0), ta.device)
    got2 = ops.rank_grouped_vunit(ta, tb, off, rows_per_block=256, ws=ws2)
    _check_all([x.cpu().numpy() for x in got2[:3]], (want_a, want_b, want_v))
    st2 = ops.rank_sweep_stats(ws2)
    assert st2["vunit_brute_force_owners"] == 0 and st2["vunit_in_reach"] == st["vunit_in_reach"], (st, st2)
    assert st2["vunit_in_reach_max"] == st["vunit_in_reach_max"]
    # the first eight words are those of ops.rank_grouped on the same data
    ws3 = ops.workspace(L.lib().vtc_l2_rank_grouped_workspace_bytes(n, m, d, 256, 0), ta.device)
    ops.rank_grouped(ta, tb, off, rows_per_block=256, ws=ws3)
    st3 = ops.rank_sweep_stats(ws3)
    assert all(st2[k] == st3[k] for k in ("in_reach", "in_reach_max", "brute_force_owners")), (st2, st3)


@pytest.mark.parametrize("scale", [1.0, 25.0])
def test_ties_duplicates_and_clusters(scale):
    """tests/vunit_cases.py::ties_case: exact ties between groups go to the lower video index; two in-reach captions of one group count
    once; a group with a certain and an in-reach caption is counted and not pooled twice; the two conventions differ where planted."""
    from vtc_amd import _lib as L
    from vtc_amd import ops
    a, b, off, want_a, want_b, want_v = VC.assert_ties_case(scale, ops.rank_kappa(128))
    n, m, d = a.shape[0], b.shape[0], a.shape[1]
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    ws = ops.workspace(L.lib().vtc_l2_rank_grouped_vunit_workspace_bytes(n, m, d, 0, 0), ta.device)
    ra, rb, rv, bits = ops.rank_grouped_vunit(ta, tb, off, ws=ws)
    assert int(bits.item()) == 0
    _check_all((ra.cpu().numpy(), rb.cpu().numpy(), rv.cpu().numpy()), (want_a, want_b, want_v))
    st = ops.rank_sweep_stats(ws)
    assert st["vunit_in_reach_max"] >= 64, st              # video 150 had the cluster's 100 groups in reach, less the 36 that plant 2 makes certain


def test_nonfinite_caption_video_and_empty_group():
    """A NaN in one caption of a 3-caption group (bits 2); a NaN video row q: rank_v[q] = n, nobody else beyond the reference (bits 1);
    an empty group p: rank_v[p] = n and the group is never closer to anyone."""
    for name, a, b, off, want_a, want_b, want_v, bits, idx in VC.nonfinite_cases():
        n = a.shape[0]
        if name == "nan_caption":
            assert want_v[idx] < n
        else:
            assert want_v[idx] == n and (np.delete(want_v, idx) < n).all()
        got = _sweep(a, b, off, rows_per_block=256)
        assert got[3] == bits, name
        _check_all(got, (want_a, want_b, want_v))


def test_argument_errors_return_a_status_and_a_message():
    from vtc_amd import _lib as L
    lib = L.lib()
    n, m = 32, 64
    xa, xb = torch.zeros(n, 128, device="cuda"), torch.zeros(m, 128, device="cuda")
    off = torch.arange(0, m + 1, 2, dtype=torch.int32, device="cuda")
    ra = torch.zeros(m, dtype=torch.int64, device="cuda")
    rb, rv = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.full((n,), -1, dtype=torch.int64, device="cuda")
    f = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.vtc_l2_rank_grouped_vunit_workspace_bytes(n, m, 128, 0, 0), dtype=torch.uint8, device="cuda")
    assert ws.numel() > lib.vtc_l2_rank_grouped_workspace_bytes(n, m, 128, 0, 0)
    args = lambda d=128, mm=m, o=off.data_ptr(), v=rv.data_ptr(), nbytes=ws.numel(): (                                   # noqa: E731
        xa.data_ptr(), xb.data_ptr(), o, n, mm, d, 0, 0, ra.data_ptr(), rb.data_ptr(), v, f.data_ptr(), ws.data_ptr(), nbytes, None)
    call = lib.vtc_l2_rank_grouped_vunit
    assert call(*args(d=100)) != 0 and b"l2_rank_grouped_vunit: d=100" in lib.vtc_last_error()
    assert call(*args(nbytes=1024)) != 0 and b"l2_rank_grouped_vunit: workspace too small" in lib.vtc_last_error()
    assert call(*args(o=None)) != 0 and b"l2_rank_grouped_vunit: null argument" in lib.vtc_last_error()
    assert call(*args(v=None)) != 0 and b"l2_rank_grouped_vunit: null argument" in lib.vtc_last_error()
    assert call(*args(mm=0)) != 0 and b"l2_rank_grouped_vunit: m=0" in lib.vtc_last_error()
    assert call(*args()) == 0
    torch.cuda.synchronize()
    # all rows equal: every distance ties at 0 and the lower index wins, caption index for rank_b, VIDEO index for rank_v
    assert ra.cpu().tolist() == [c // 2 for c in range(m)] and rb.cpu().tolist() == [2 * v for v in range(n)]
    assert rv.cpu().tolist() == list(range(n))


def test_metric_grouped_ranks_video_unit_pad_d_500():
    """RecallAtK.grouped_ranks(video_to_text="video") zero-pads d = 500 to 512 and takes numpy or GPU tensors."""
    from vtc_amd.host.metric import RecallAtK
    n = 300
    a, b, off, want_a, want_b, want_v = VC.case("1-4", n, 500)
    VC.assert_not_degenerate(want_v, want_b, n)
    m = RecallAtK("videos", "titles", [1, 5, 10])
    ra, rv = m.grouped_ranks(a, b, off, video_to_text="video")
    assert ra.is_cuda and rv.is_cuda and rv.dtype == torch.int64 and ra.shape == (b.shape[0],) and rv.shape == (n,)
    _check(ra.cpu().numpy(), want_a, "rank_a")
    _check(rv.cpu().numpy(), want_v, "rank_v")
    ra, rv = m.grouped_ranks(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(off), video_to_text="video")
    _check(ra.cpu().numpy(), want_a, "rank_a (tensors)")
    _check(rv.cpu().numpy(), want_v, "rank_v (tensors)")
    ra, rb = m.grouped_ranks(a, b, off)                                                        # the default is the caption-level one
    _check(rb.cpu().numpy(), want_b, "rank_b (default)")
    bad = b.copy()
    bad[7, 0] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        m.grouped_ranks(a, bad, off, video_to_text="video")


def test_multi_caption_table_video_unit():
    """From the -inf-padded [N, C, D] tensor and from flat captions with offsets: the table of the reference ranks, attrs included; the
    default call keeps its "Text to Video" column and empty attrs; one caption per video: compute_rank_table's frame either way."""
    from pandas.testing import assert_frame_equal

    import evaluation.retrieval_evaluation as front
    import rank_refs as RR
    from vtc_amd.host import retrieval_evaluation as RE
    n = 257
    a, b, off, want_a, want_b, want_v = VC.case("1-4", n, 64)
    want = VR.table_from_ranks(want_a, want_v, "full-test", "MSRVTT")
    got = front.compute_multi_caption_table(torch.from_numpy(a), torch.from_numpy(GR.pad_captions(b, off)), video_to_text="video")
    assert list(got.index) == ["R@1", "R@5", "R@10", "MedR", "MeanR", "MRR"]
    assert list(got.columns) == ["MSRVTT full-test split Video to Text", "MSRVTT full-test split Text to Video"]
    assert got.attrs == {"video_to_text": "video"}
    assert_frame_equal(got, want, check_exact=True)
    got_flat = RE.compute_multi_caption_table(a, b, offsets=off, video_to_text="video")
    assert_frame_equal(got_flat, want, check_exact=True)
    assert got_flat.attrs == {"video_to_text": "video"}
    default = RE.compute_multi_caption_table(a, b, offsets=off)
    assert default.attrs == {}
    assert_frame_equal(default, GR.table_from_ranks(want_a, want_b, "full-test", "MSRVTT"), check_exact=True)
    assert default.iloc[:, 1].equals(got.iloc[:, 1]) and not default.iloc[:, 0].equals(got.iloc[:, 0])
    assert default.iloc[0, 0] == got.iloc[0, 0]                                                # the conventions agree on R@1
    pa, pb = RR.spread_pairs(700, 128, 3)
    paired = RE.compute_rank_table(pa, pb, "1k-A", "MSVD")
    for conv in ("caption", "video"):
        one = RE.compute_multi_caption_table(pa, pb[:, None, :], "1k-A", "MSVD", video_to_text=conv)
        assert_frame_equal(one, paired, check_exact=True)


def test_retrieval_evaluation_video_unit_end_to_end():
    """retrieval_evaluation(multi_caption=True, video_to_text="video") with the tiny model, six videos with three captions each: the table
    is held to the reference ranks of the returned embeddings; the default call returns the caption-level frame it returns today."""
    from pandas.testing import assert_frame_equal

    from evaluation.retrieval_evaluation import retrieval_evaluation
    from oracle import arch as A
    from test_gpu_multi_caption_eval import _items
    from test_gpu_retrieval_eval import _build
    with torch.no_grad():
        arch = A.TINY
        m, _ = _build("timesformer", "PretrainedCLIP_TimeSformer", arch, 81)
        items = _items(arch, [3] * 6, 700, False)
        df, v_emb, c_emb, offsets = retrieval_evaluation(m, items, "full-test", "cuda", return_embeddings=True, multi_caption=True,
                                                         video_to_text="video")
        assert offsets.tolist() == [0, 3, 6, 9, 12, 15, 18]
        v, c = v_emb.cpu().numpy(), c_emb.cpu().numpy()
        want_a, want_b, gap = GR.reference_grouped_ranks(v, c, offsets)
        assert gap > 1e-12, gap
        assert_frame_equal(df, VR.table_from_ranks(want_a, VR.reference_vunit_ranks(v, c, offsets), "full-test", "videos"), check_exact=True)
        assert df.attrs.get("video_to_text") == "video"
        df0, v0, c0, _ = retrieval_evaluation(m, items, "full-test", "cuda", return_embeddings=True, multi_caption=True)
        assert torch.equal(v0, v_emb) and torch.equal(c0, c_emb)
        assert_frame_equal(df0, GR.table_from_ranks(want_a, want_b, "full-test", "videos"), check_exact=True)
        assert "video_to_text" not in df0.attrs
