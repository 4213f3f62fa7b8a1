"""CPU: the argument checks of the excluding search's entry point (vtc_l2_search_excluding).  Every refused call returns non-zero with
"search" in vtc_last_error() before anything is launched -- no GPU is needed, the pointers are never dereferenced."""
import pytest

from vtc_amd import _lib as L

P = 0x1000        # a non-null "device pointer": a refused call never touches it


def _excluding(ng=100, nq=4, d=64, depth=5, id_base=0, half=0, gallery=P, queries=P, live=None, groups=None, exclude=P, after_d=None, after_i=None,
               ids=P, out_groups=None, ws=P, ws_bytes=None):
    lib = L.lib()
    if ws_bytes is None:
        ws_bytes = max(lib.vtc_l2_search_grouped_workspace_bytes(ng, nq, d, depth), 1 << 20)
    return lib.vtc_l2_search_excluding(gallery, half, queries, live, groups, exclude, after_d, after_i, ng, nq, d, depth, id_base, ids, out_groups,
                                       None, None, ws, ws_bytes, None)


def _refused(rc):
    assert rc != 0 and b"search" in L.lib().vtc_last_error(), (rc, L.lib().vtc_last_error())


SHAPES = [
    dict(nq=0), dict(nq=65),
    dict(depth=0), dict(depth=65, ng=1000), dict(depth=11, ng=10),
    dict(d=32), dict(d=100), dict(d=2112),
    dict(ng=0, depth=1),
    dict(id_base=-1), dict(id_base=2 ** 63 - 50),
    dict(gallery=None), dict(queries=None), dict(ids=None), dict(ws=None), dict(exclude=None),
    dict(ws_bytes=1),
]
FORMS = {"plain": {}, "cursor": dict(after_d=P, after_i=P), "grouped": dict(groups=P, out_groups=P)}


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kw", SHAPES, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_search_excluding_refuses(kw, form, half):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_excluding(half=half, **FORMS[form], **kw))
    _refused(_excluding(half=half, live=P, **FORMS[form], **kw))
    assert lib.vtc_debug_launch_count() == before


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("kw", [
    dict(groups=P, out_groups=P, after_d=P, after_i=P),       # the grouped search has no cursor
    dict(after_d=P), dict(after_i=P),                         # a cursor is both or neither
    dict(groups=P),                                           # groups without out_groups
], ids=lambda kw: ",".join(sorted(kw)))
def test_combinations_that_are_refused(kw, half):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_excluding(half=half, **kw))
    _refused(_excluding(half=half, live=P, **kw))
    assert lib.vtc_debug_launch_count() == before


def test_workspace_is_the_plain_searchs_or_the_grouped_one():
    lib = L.lib()
    plain = lib.vtc_l2_search_workspace_bytes(1027, 9, 64, 64)
    grouped = lib.vtc_l2_search_grouped_workspace_bytes(1027, 9, 64, 64)
    assert 0 < plain < grouped
    _refused(_excluding(ng=1027, nq=9, depth=64, ws_bytes=plain - 1))
    _refused(_excluding(ng=1027, nq=9, depth=64, ws_bytes=plain - 1, after_d=P, after_i=P))
    _refused(_excluding(ng=1027, nq=9, depth=64, ws_bytes=grouped - 1, groups=P, out_groups=P))
    assert b"workspace" in lib.vtc_last_error()


def test_abi_version_is_unchanged():
    assert L.lib().vtc_abi_version() == 7 == L.ABI_VERSION
