"""CPU: the entry points of the paged grouped search (vtc_l2_group_ban_words, vtc_l2_group_mark_before, vtc_l2_search_grouped_after) --
the symbols, their ctypes signatures against the prototypes of include/vtc_hip.h, and the argument checks.  Every refused call returns
non-zero with "search" in vtc_last_error() before anything is launched -- no GPU is needed, the pointers are never dereferenced."""
import ctypes as C
import os
import re

import pytest

from vtc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x1000        # a non-null "device pointer": a refused call never touches it
NAMES = ("vtc_l2_group_ban_words", "vtc_l2_group_mark_before", "vtc_l2_search_grouped_after")


def _mark(ng=100, nq=4, d=64, n_groups=40, id_base=0, half=0, gallery=P, queries=P, live=None, groups=P, after_d=P, after_i=P, ban=P):
    return L.lib().vtc_l2_group_mark_before(gallery, half, queries, live, groups, n_groups, after_d, after_i, ng, nq, d, id_base, ban, None)


def _page(ng=100, nq=4, d=64, depth=5, n_groups=40, id_base=0, half=0, gallery=P, queries=P, live=None, groups=P, ban=P, exclude=None, after_d=P,
          after_i=P, ids=P, out_groups=P, ws=P, ws_bytes=None):
    lib = L.lib()
    if ws_bytes is None:
        ws_bytes = max(lib.vtc_l2_search_grouped_workspace_bytes(ng, nq, d, depth), 1 << 20)
    return lib.vtc_l2_search_grouped_after(gallery, half, queries, live, groups, n_groups, ban, exclude, after_d, after_i, ng, nq, d, depth, id_base,
                                           ids, out_groups, None, None, ws, ws_bytes, None)


def _refused(rc):
    assert rc != 0 and b"search" in L.lib().vtc_last_error(), (rc, L.lib().vtc_last_error())


def test_the_three_symbols_are_exported_and_bound():
    lib = L.lib()
    for name in NAMES:
        assert name in L.SIGNATURES and getattr(lib, name) is not None


CTYPES = {"int": C.c_int, "size_t": C.c_size_t, "int64_t": C.c_int64}


def test_the_signatures_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "vtc_hip.h")).read()
    for name in NAMES:
        m = re.search(r"^(size_t|int) " + name + r"\(([^;]*)\);", hdr, flags=re.M)
        assert m, name
        args = []
        for a in m.group(2).split(","):
            a = re.sub(r"/\*.*?\*/", "", a).strip()
            args.append(C.c_void_p if "*" in a else CTYPES[a.rsplit(" ", 1)[0].replace("const ", "").strip()])
        res, bound = L.SIGNATURES[name]
        assert res is CTYPES[m.group(1)], name
        assert list(bound) == args, (name, bound, args)


def test_ban_words():
    lib = L.lib()
    assert lib.vtc_l2_group_ban_words(1, 1) == 1 and lib.vtc_l2_group_ban_words(3, 32) == 3 and lib.vtc_l2_group_ban_words(3, 33) == 6
    assert lib.vtc_l2_group_ban_words(64, 2 ** 31 - 1) == 64 * 2 ** 26
    for nq, n_groups in ((0, 5), (65, 5), (4, 0), (4, -1)):
        assert lib.vtc_l2_group_ban_words(nq, n_groups) == 0


MARK_SHAPES = [
    dict(nq=0), dict(nq=65),
    dict(d=32), dict(d=100), dict(d=2112),
    dict(ng=0),
    dict(n_groups=0), dict(n_groups=-1),
    dict(id_base=-1), dict(id_base=2 ** 63 - 50),
    dict(gallery=None), dict(queries=None), dict(groups=None), dict(after_d=None), dict(after_i=None), dict(ban=None),
]
PAGE_SHAPES = MARK_SHAPES + [
    dict(depth=0), dict(depth=65, ng=1000), dict(depth=11, ng=10),
    dict(ids=None), dict(out_groups=None), dict(ws=None), dict(ws_bytes=1),
]
_ids = lambda kw: ",".join(f"{k}={v}" for k, v in kw.items())      # noqa: E731


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("kw", MARK_SHAPES, ids=_ids)
def test_mark_before_refuses(kw, half):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_mark(half=half, **kw))
    _refused(_mark(half=half, live=P, **kw))
    assert lib.vtc_debug_launch_count() == before


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("kw", PAGE_SHAPES, ids=_ids)
def test_search_grouped_after_refuses(kw, half):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    if kw.get("ng") == 0:
        kw = dict(kw, depth=1)
    for exclude in (None, P):
        _refused(_page(half=half, exclude=exclude, **kw))
        _refused(_page(half=half, exclude=exclude, live=P, **kw))
    assert lib.vtc_debug_launch_count() == before


def test_workspace_is_the_grouped_searchs():
    lib = L.lib()
    plain = lib.vtc_l2_search_workspace_bytes(1027, 9, 64, 64)
    grouped = lib.vtc_l2_search_grouped_workspace_bytes(1027, 9, 64, 64)
    assert 0 < plain < grouped
    _refused(_page(ng=1027, nq=9, depth=64, ws_bytes=grouped - 1))
    assert b"workspace" in lib.vtc_last_error()


def test_the_older_entry_still_refuses_a_cursor_with_groups():
    lib = L.lib()
    rc = lib.vtc_l2_search_excluding(P, 0, P, None, P, P, P, P, 100, 4, 64, 5, 0, P, P, None, None, P, 1 << 20, None)
    assert rc != 0 and b"no cursor" in lib.vtc_last_error()


def test_abi_version_is_unchanged():
    assert L.lib().vtc_abi_version() == 7 == L.ABI_VERSION
