"""CPU: the argument checks of the masked search entry points (vtc_l2_search_masked, vtc_row_mask_pack).  Every refused call returns
non-zero with "search" in vtc_last_error() before anything is launched -- no GPU is needed, the pointers are never dereferenced.  The
table is vtc_l2_search's (tests/test_search_abi.py): the mask adds no limit of its own, and a NULL mask is no reason to refuse."""
import pytest

from vtc_amd import _lib as L

P = 0x1000        # a non-null "device pointer": a refused call never touches it


def _search(ng=100, nq=4, d=64, depth=5, id_base=0, gallery=P, queries=P, live=P, ids=P, ws=P, ws_bytes=None):
    lib = L.lib()
    if ws_bytes is None:
        ws_bytes = max(lib.vtc_l2_search_workspace_bytes(ng, nq, d, depth), 1 << 20)
    return lib.vtc_l2_search_masked(gallery, queries, live, ng, nq, d, depth, id_base, ids, None, None, ws, ws_bytes, None)


def _refused(rc):
    assert rc != 0 and b"search" in L.lib().vtc_last_error(), (rc, L.lib().vtc_last_error())


REFUSED = [
    dict(nq=0), dict(nq=65),
    dict(depth=0), dict(depth=65, ng=1000), dict(depth=11, ng=10),
    dict(d=32), dict(d=100), dict(d=2112),
    dict(ng=0, depth=1),
    dict(id_base=-1),
    dict(gallery=None), dict(queries=None), dict(ids=None), dict(ws=None),
    dict(ws_bytes=1),
]


@pytest.mark.parametrize("live", [P, None], ids=["mask", "null-mask"])
@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_masked_search_refuses(kw, live):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_search(live=live, **kw))
    assert lib.vtc_debug_launch_count() == before


def test_a_null_mask_is_not_a_refusal_reason():
    """Every refusal above names an argument other than the mask: with live = NULL the error text of each is the one with a mask."""
    lib = L.lib()
    for kw in REFUSED:
        _refused(_search(live=P, **kw))
        with_mask = lib.vtc_last_error()
        _refused(_search(live=None, **kw))
        assert lib.vtc_last_error() == with_mask, kw
        assert b"live" not in with_mask and b"mask" not in with_mask, with_mask


@pytest.mark.parametrize("kw", [dict(flags=None), dict(words=None), dict(n_rows=0), dict(n_rows=-5)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_row_mask_pack_refuses(kw):
    lib = L.lib()
    a = dict(flags=P, n_rows=100, and_mask=None, words=P)
    a.update(kw)
    before = lib.vtc_debug_launch_count()
    _refused(lib.vtc_row_mask_pack(a["flags"], a["n_rows"], a["and_mask"], a["words"], None))
    assert lib.vtc_debug_launch_count() == before


def test_abi_version_is_unchanged():
    assert L.lib().vtc_abi_version() == 7 == L.ABI_VERSION
