"""CPU: the argument checks of vtc_l2_search_many_half, the many-query search of a half gallery.  Every refused call returns non-zero with
"search" in vtc_last_error() before anything is launched -- no GPU is needed, the pointers are never dereferenced.  The table is
vtc_l2_search_half's (tests/test_search_half_abi.py, imported), run with and without a mask, plus what only this entry refuses:
depth above 32 and its own workspace one byte short."""
import pytest

from vtc_amd import _lib as L

from test_search_half_abi import P, REFUSED as HALF_REFUSED

REFUSED = HALF_REFUSED + [dict(depth=33, ng=1000)]


def _search(ng=100, nq=4, d=64, depth=5, id_base=0, gallery=P, queries=P, live=P, ids=P, ws=P, ws_bytes=None):
    lib = L.lib()
    if ws_bytes is None:
        ws_bytes = max(lib.vtc_l2_search_many_workspace_bytes(ng, nq, d, depth), 1 << 20)
    return lib.vtc_l2_search_many_half(gallery, queries, live, ng, nq, d, depth, id_base, ids, None, None, ws, ws_bytes, None)


def _refused(rc):
    assert rc != 0 and b"search" in L.lib().vtc_last_error(), (rc, L.lib().vtc_last_error())


def test_the_table_is_the_half_one_and_depth_33():
    assert len(REFUSED) == len(HALF_REFUSED) + 1 == 16


@pytest.mark.parametrize("live", [P, None], ids=["mask", "null-mask"])
@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_many_search_refuses(kw, live):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_search(live=live, **kw))
    assert lib.vtc_debug_launch_count() == before


def test_depth_32_is_the_limit():
    lib = L.lib()
    assert lib.vtc_l2_search_many_workspace_bytes(1000, 4, 64, 32) > 0
    assert lib.vtc_l2_search_many_workspace_bytes(1000, 4, 64, 33) == 0
    _refused(_search(ng=1000, depth=33))
    assert b"depth" in lib.vtc_last_error()


@pytest.mark.parametrize("live", [P, None], ids=["mask", "null-mask"])
def test_a_workspace_one_byte_too_small_is_refused(live):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    for shape in ((100, 4, 64, 5), (10 ** 6, 64, 512, 11)):
        need = lib.vtc_l2_search_many_workspace_bytes(*shape)
        assert need > 0
        ng, nq, d, depth = shape
        _refused(_search(ng=ng, nq=nq, d=d, depth=depth, live=live, ws_bytes=need - 1))
        assert b"workspace" in lib.vtc_last_error()
    assert lib.vtc_debug_launch_count() == before


def test_workspace_bytes():
    """0 for every refused shape; otherwise the fp64 head, the counter behind it, and lists whose number does not grow with the gallery."""
    lib = L.lib()
    for kw in [kw for kw in REFUSED if set(kw) <= {"ng", "nq", "d", "depth"}]:
        a = dict(ng=100, nq=4, d=64, depth=5)
        a.update(kw)
        assert lib.vtc_l2_search_many_workspace_bytes(a["ng"], a["nq"], a["d"], a["depth"]) == 0, kw
    for nq in (1, 8, 16, 17, 33, 64):
        small, big = lib.vtc_l2_search_many_workspace_bytes(10 ** 6, nq, 512, 11), lib.vtc_l2_search_many_workspace_bytes(10 ** 8, nq, 512, 11)
        assert small == big > nq * 11 * 8 + 4                                 # no distance matrix: bounded in n_gallery
        assert big <= 16 << 20
    assert lib.vtc_l2_search_many_workspace_bytes(100, 4, 64, 5) < lib.vtc_l2_search_many_workspace_bytes(10 ** 6, 4, 64, 5)


def test_a_null_mask_is_not_a_refusal_reason():
    lib = L.lib()
    for kw in REFUSED:
        _refused(_search(live=P, **kw))
        with_mask = lib.vtc_last_error()
        _refused(_search(live=None, **kw))
        assert lib.vtc_last_error() == with_mask, kw
        assert b"live" not in with_mask and b"mask" not in with_mask, with_mask


def test_abi_version_is_unchanged():
    assert L.lib().vtc_abi_version() == 7 == L.ABI_VERSION
