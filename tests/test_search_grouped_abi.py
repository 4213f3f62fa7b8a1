"""CPU: the argument checks of the grouped search entry points (vtc_l2_search_grouped, vtc_l2_search_merge_grouped).  Every refused call
returns non-zero with "search" in vtc_last_error() before anything is launched -- no GPU is needed, the pointers are never dereferenced.
The table is vtc_l2_search_masked's (tests/test_search_mask_abi.py) plus the group pointers; a NULL mask is no reason to refuse."""
import pytest

from vtc_amd import _lib as L

P = 0x1000        # a non-null "device pointer": a refused call never touches it


def _search(ng=100, nq=4, d=64, depth=5, id_base=0, gallery=P, queries=P, live=P, groups=P, ids=P, out_groups=P, ws=P, ws_bytes=None):
    lib = L.lib()
    if ws_bytes is None:
        ws_bytes = max(lib.vtc_l2_search_grouped_workspace_bytes(ng, nq, d, depth), 1 << 20)
    return lib.vtc_l2_search_grouped(gallery, queries, live, groups, ng, nq, d, depth, id_base, ids, out_groups, None, None, ws, ws_bytes, None)


def _merge(n_parts=3, nq=4, depth=5, ids_parts=P, dists_parts=P, groups_parts=P, ids=P, out_groups=P):
    return L.lib().vtc_l2_search_merge_grouped(ids_parts, dists_parts, groups_parts, n_parts, nq, depth, ids, out_groups, None, None)


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
    dict(groups=None), dict(out_groups=None),
]


@pytest.mark.parametrize("live", [P, None], ids=["mask", "null-mask"])
@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_grouped_search_refuses(kw, live):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_search(live=live, **kw))
    assert lib.vtc_debug_launch_count() == before


def test_a_null_mask_is_not_a_refusal_reason():
    lib = L.lib()
    for kw in REFUSED:
        _refused(_search(live=P, **kw))
        with_mask = lib.vtc_last_error()
        _refused(_search(live=None, **kw))
        assert lib.vtc_last_error() == with_mask, kw
        assert b"live" not in with_mask and b"mask" not in with_mask, with_mask


MERGE_REFUSED = [
    dict(n_parts=0), dict(n_parts=65), dict(nq=0), dict(nq=65), dict(depth=0), dict(depth=65),
    dict(ids_parts=None), dict(dists_parts=None), dict(groups_parts=None), dict(ids=None), dict(out_groups=None),
]


@pytest.mark.parametrize("kw", MERGE_REFUSED, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_grouped_merge_refuses(kw):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_merge(**kw))
    assert lib.vtc_debug_launch_count() == before


def test_workspace_bytes():
    lib = L.lib()
    for kw in REFUSED[:9]:
        a = dict(ng=100, nq=4, d=64, depth=5)
        a.update(kw)
        assert lib.vtc_l2_search_grouped_workspace_bytes(a["ng"], a["nq"], a["d"], a["depth"]) == 0, kw
    for ng, nq, d, depth in ((100, 4, 64, 5), (1027, 64, 512, 64), (10 ** 6, 8, 512, 11)):
        plain, grouped = lib.vtc_l2_search_workspace_bytes(ng, nq, d, depth), lib.vtc_l2_search_grouped_workspace_bytes(ng, nq, d, depth)
        lists = min(1024, (ng + 3) // 4)
        assert plain > 0 and plain + nq * depth * lists * 4 <= grouped <= plain + nq * depth * lists * 4 + 1024      # one more int per entry


def test_abi_version_is_unchanged():
    assert L.lib().vtc_abi_version() == 7 == L.ABI_VERSION
