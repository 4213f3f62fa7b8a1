"""CPU: the argument checks of vtc_l2_search_half, the search over a gallery stored as IEEE binary16.  Every refused call returns non-zero
with "search" in vtc_last_error() before anything is launched -- no GPU is needed, the pointers are never dereferenced.  The table is
vtc_l2_search_grouped's (tests/test_search_grouped_abi.py), run with groups (the grouped search: out_groups is required) and with
groups = NULL (the ungrouped one: out_groups is ignored); a NULL mask is no reason to refuse."""
import pytest

from vtc_amd import _lib as L

from test_search_grouped_abi import P, REFUSED as GROUPED_REFUSED

# the grouped table without its two group-pointer rows: what both forms refuse
REFUSED = [kw for kw in GROUPED_REFUSED if "groups" not in kw and "out_groups" not in kw]


def _search(ng=100, nq=4, d=64, depth=5, id_base=0, gallery=P, queries=P, live=P, groups=P, ids=P, out_groups=P, ws=P, ws_bytes=None):
    lib = L.lib()
    if ws_bytes is None:
        need = lib.vtc_l2_search_grouped_workspace_bytes if groups else lib.vtc_l2_search_workspace_bytes
        ws_bytes = max(need(ng, nq, d, depth), 1 << 20)
    return lib.vtc_l2_search_half(gallery, queries, live, groups, ng, nq, d, depth, id_base, ids, out_groups, None, None, ws, ws_bytes, None)


def _refused(rc):
    assert rc != 0 and b"search" in L.lib().vtc_last_error(), (rc, L.lib().vtc_last_error())


def test_the_table_is_the_grouped_one():
    assert len(REFUSED) == len(GROUPED_REFUSED) - 2 == 15


@pytest.mark.parametrize("groups", [P, None], ids=["groups", "no-groups"])
@pytest.mark.parametrize("live", [P, None], ids=["mask", "null-mask"])
@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_half_search_refuses(kw, live, groups):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_search(live=live, groups=groups, out_groups=P if groups else None, **kw))
    assert lib.vtc_debug_launch_count() == before


@pytest.mark.parametrize("live", [P, None], ids=["mask", "null-mask"])
def test_groups_without_out_groups_are_refused(live):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_search(live=live, groups=P, out_groups=None))
    assert lib.vtc_debug_launch_count() == before


def test_a_workspace_one_byte_too_small_is_refused():
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    for groups, need in ((None, lib.vtc_l2_search_workspace_bytes(100, 4, 64, 5)), (P, lib.vtc_l2_search_grouped_workspace_bytes(100, 4, 64, 5))):
        assert need > 0
        _refused(_search(groups=groups, ws_bytes=need - 1))
        assert b"workspace" in lib.vtc_last_error()
    # the grouped form needs the grouped workspace: the ungrouped size is too small for it
    _refused(_search(groups=P, ws_bytes=lib.vtc_l2_search_workspace_bytes(100, 4, 64, 5)))
    assert lib.vtc_debug_launch_count() == before


def test_a_null_mask_is_not_a_refusal_reason():
    lib = L.lib()
    for groups in (P, None):
        for kw in REFUSED + ([dict(out_groups=None)] if groups else []):
            kw = dict(dict(out_groups=P if groups else None), **kw)
            _refused(_search(live=P, groups=groups, **kw))
            with_mask = lib.vtc_last_error()
            _refused(_search(live=None, groups=groups, **kw))
            assert lib.vtc_last_error() == with_mask, kw
            assert b"live" not in with_mask and b"mask" not in with_mask, with_mask


def test_abi_version_is_unchanged():
    assert L.lib().vtc_abi_version() == 7 == L.ABI_VERSION
