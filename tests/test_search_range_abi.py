"""CPU: the argument checks of the range search (vtc_l2_range_count, vtc_l2_range_fill, vtc_l2_range_workspace_bytes).  Every refused call
returns non-zero with "range" in vtc_last_error() before anything is launched -- no GPU is needed, the pointers are never dereferenced.
A NULL mask is no reason to refuse; a workspace one byte short is refused by name; the ABI version stays 7."""
import pytest

from vtc_amd import _lib as L

P = 0x1000        # a non-null "device pointer": a refused call never touches it


def _need(ng, nq, d):
    return L.lib().vtc_l2_range_workspace_bytes(ng, nq, d)


def _count(ng=100, nq=4, d=64, half=0, gallery=P, queries=P, live=P, radius2=P, lims=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(_need(ng, nq, d), 1 << 20)
    return L.lib().vtc_l2_range_count(gallery, half, queries, live, radius2, ng, nq, d, lims, None, ws, ws_bytes, None)


def _fill(ng=100, nq=4, d=64, half=0, capacity=10, id_base=0, gallery=P, queries=P, lims=P, ids=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(_need(ng, nq, d), 1 << 20)
    return L.lib().vtc_l2_range_fill(gallery, half, queries, ng, nq, d, lims, capacity, id_base, ids, None, None, ws, ws_bytes, None)


def _refused(rc):
    assert rc != 0 and b"range" in L.lib().vtc_last_error(), (rc, L.lib().vtc_last_error())


SHAPES_REFUSED = [dict(nq=0), dict(nq=65), dict(d=32), dict(d=100), dict(d=2112), dict(d=0), dict(ng=0), dict(ng=-5)]
COUNT_REFUSED = SHAPES_REFUSED + [dict(gallery=None), dict(queries=None), dict(radius2=None), dict(lims=None), dict(ws=None), dict(ws_bytes=1)]
FILL_REFUSED = SHAPES_REFUSED + [dict(gallery=None), dict(queries=None), dict(lims=None), dict(ids=None), dict(ws=None), dict(ws_bytes=1),
                                 dict(capacity=-1), dict(id_base=-1), dict(id_base=2 ** 63 - 50)]
_ids = lambda kw: ",".join(f"{k}={v}" for k, v in kw.items())      # noqa: E731


@pytest.mark.parametrize("half", [0, 1], ids=["fp32", "half"])
@pytest.mark.parametrize("live", [P, None], ids=["mask", "null-mask"])
@pytest.mark.parametrize("kw", COUNT_REFUSED, ids=_ids)
def test_count_refuses(kw, live, half):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_count(live=live, half=half, **kw))
    assert lib.vtc_debug_launch_count() == before


@pytest.mark.parametrize("half", [0, 1], ids=["fp32", "half"])
@pytest.mark.parametrize("kw", FILL_REFUSED, ids=_ids)
def test_fill_refuses(kw, half):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_fill(half=half, **kw))
    assert lib.vtc_debug_launch_count() == before


def test_a_workspace_one_byte_too_small_is_refused():
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    for shape in ((100, 4, 64), (70001, 64, 512), (1, 1, 2048)):
        need = _need(*shape)
        assert need > 0
        for call in (_count, _fill):
            _refused(call(*shape, ws_bytes=need - 1))
            assert b"workspace" in lib.vtc_last_error()
    assert lib.vtc_debug_launch_count() == before


def test_a_null_mask_is_not_a_refusal_reason():
    lib = L.lib()
    for kw in COUNT_REFUSED:
        _refused(_count(live=P, **kw))
        with_mask = lib.vtc_last_error()
        _refused(_count(live=None, **kw))
        assert lib.vtc_last_error() == with_mask, kw
        assert b"live" not in with_mask and b"mask" not in with_mask, with_mask


def test_workspace_bytes():
    for kw in SHAPES_REFUSED:
        a = dict(ng=100, nq=4, d=64)
        a.update(kw)
        assert _need(a["ng"], a["nq"], a["d"]) == 0, kw
    for ng, nq, d in ((1, 1, 64), (100, 4, 64), (1027, 64, 512), (10 ** 6, 8, 512), (2 ** 31 - 1, 64, 2048)):
        words = (ng + 31) // 32
        assert _need(ng, nq, d) >= nq * words * 4              # the documented head: the hit words of every query
        assert _need(ng, nq, d) <= nq * (words * 4 + 1024 * 4 + (words + 15) // 16 * 4) + 3 * 256
    assert _need(100, 4, 64) == _need(100, 4, 2048)            # nothing in it depends on d


def test_abi_version_is_unchanged():
    assert L.lib().vtc_abi_version() == 7 == L.ABI_VERSION
