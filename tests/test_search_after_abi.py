"""CPU: the argument checks of the cursor search's entry points (vtc_l2_search_after, vtc_l2_pair_dists64).  Every refused call returns
non-zero with "search" in vtc_last_error() before anything is launched -- no GPU is needed, the pointers are never dereferenced."""
import pytest

from vtc_amd import _lib as L

P = 0x1000        # a non-null "device pointer": a refused call never touches it


def _after(ng=100, nq=4, d=64, depth=5, id_base=0, half=0, gallery=P, queries=P, live=None, after_d=P, after_i=P, ids=P, ws=P, ws_bytes=None):
    lib = L.lib()
    if ws_bytes is None:
        ws_bytes = max(lib.vtc_l2_search_workspace_bytes(ng, nq, d, depth), 1 << 20)
    return lib.vtc_l2_search_after(gallery, half, queries, live, after_d, after_i, ng, nq, d, depth, id_base, ids, None, None, ws, ws_bytes, None)


def _pair(ng=100, nq=4, d=64, id_base=0, half=0, gallery=P, queries=P, rows=P, out=P):
    return L.lib().vtc_l2_pair_dists64(gallery, half, queries, rows, ng, nq, d, id_base, out, None)


def _refused(rc):
    assert rc != 0 and b"search" in L.lib().vtc_last_error(), (rc, L.lib().vtc_last_error())


SHAPES = [
    dict(nq=0), dict(nq=65),
    dict(depth=0), dict(depth=65, ng=1000), dict(depth=11, ng=10),
    dict(d=32), dict(d=100), dict(d=2112),
    dict(ng=0, depth=1),
    dict(id_base=-1),
    dict(gallery=None), dict(queries=None), dict(ids=None), dict(ws=None),
    dict(ws_bytes=1),
    dict(after_d=None), dict(after_i=None),
]


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("kw", SHAPES, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_search_after_refuses(kw, half):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_after(half=half, **kw))
    _refused(_after(half=half, live=P, **kw))
    assert lib.vtc_debug_launch_count() == before


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("kw", [
    dict(nq=0), dict(d=32), dict(d=100), dict(d=2112), dict(ng=0), dict(id_base=-1),
    dict(gallery=None), dict(queries=None), dict(rows=None), dict(out=None),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_pair_dists64_refuses(kw, half):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_pair(half=half, **kw))
    assert lib.vtc_debug_launch_count() == before


def test_id_base_plus_rows_must_be_an_int64():
    _refused(_after(ng=100, id_base=2 ** 63 - 50))
    _refused(_pair(ng=100, id_base=2 ** 63 - 50))


def test_workspace_is_the_plain_searchs():
    lib = L.lib()
    need = lib.vtc_l2_search_workspace_bytes(1027, 9, 64, 64)
    assert need > 0
    _refused(_after(ng=1027, nq=9, depth=64, ws_bytes=need - 1))


def test_abi_version_is_unchanged():
    assert L.lib().vtc_abi_version() == 7 == L.ABI_VERSION
