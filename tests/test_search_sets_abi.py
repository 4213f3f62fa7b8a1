"""CPU: the argument checks of the set queries' entry points (vtc_l2_search_sets, vtc_l2_search_sets_workspace_bytes).  Every refused call
returns non-zero with the entry's name in vtc_last_error() before anything is launched -- no GPU is needed, the pointers are never
dereferenced."""
import pytest

from vtc_amd import _lib as L

P = 0x1000        # a non-null "device pointer": a refused call never touches it


def _sets(ng=100, n_sets=3, set_size=4, d=64, depth=5, id_base=0, half=0, gallery=P, queries=P, live=None, groups=None, exclude=None, ids=P,
          out_groups=None, ws=P, ws_bytes=None):
    lib = L.lib()
    if ws_bytes is None:
        ws_bytes = max(lib.vtc_l2_search_sets_workspace_bytes(ng, n_sets, set_size, d, depth, 1), 1 << 20)
    return lib.vtc_l2_search_sets(gallery, half, queries, live, groups, exclude, ng, n_sets, set_size, d, depth, id_base, ids, out_groups, None, None,
                                  ws, ws_bytes, None)


def _refused(rc, text=b"l2_search_sets"):
    assert rc != 0 and text in L.lib().vtc_last_error(), (rc, L.lib().vtc_last_error())


SHAPES = [
    dict(n_sets=0), dict(set_size=0), dict(n_sets=-1), dict(n_sets=65, set_size=1), dict(n_sets=1, set_size=65), dict(n_sets=5, set_size=13),
    dict(n_sets=1 << 16, set_size=1 << 16),                    # a product that is no int
    dict(depth=0), dict(depth=65, ng=1000), dict(depth=11, ng=10),
    dict(d=32), dict(d=100), dict(d=2112),
    dict(ng=0, depth=1),
    dict(id_base=-1), dict(id_base=2 ** 63 - 50),
    dict(gallery=None), dict(queries=None), dict(ids=None), dict(ws=None),
    dict(ws_bytes=1),
]
FORMS = {"plain": {}, "excluding": dict(exclude=P), "grouped": dict(groups=P, out_groups=P), "grouped excluding": dict(groups=P, out_groups=P, exclude=P)}


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kw", SHAPES, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_search_sets_refuses(kw, form, half):
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_sets(half=half, **FORMS[form], **kw))
    _refused(_sets(half=half, live=P, **FORMS[form], **kw))
    assert lib.vtc_debug_launch_count() == before
    args = dict(dict(ng=100, n_sets=3, set_size=4, d=64, depth=5), **{k: v for k, v in kw.items() if k in ("ng", "n_sets", "set_size", "d", "depth")})
    if set(kw) & set(args):                                    # a refused shape has no workspace size
        assert lib.vtc_l2_search_sets_workspace_bytes(args["ng"], args["n_sets"], args["set_size"], args["d"], args["depth"], 0) == 0


def test_the_messages_name_what_was_wrong():
    _refused(_sets(n_sets=5, set_size=13), b"l2_search_sets: n_sets=5 and set_size=13 must be at least 1, n_sets * set_size at most 64")
    _refused(_sets(ids=None), b"l2_search_sets: null argument")
    _refused(_sets(groups=P), b"l2_search_sets: null argument")          # groups without out_groups
    _refused(_sets(ng=0, n_sets=0), b"l2_search_sets: n_gallery=0 must be at least 1")      # the order of the checks: the gallery first
    _refused(_sets(depth=6, ng=5), b"l2_search_sets: depth=6 must be in [1, min(64, n_gallery)]")


def test_the_workspace_grows_with_the_tiles_of_a_set_and_with_groups():
    lib = L.lib()
    size = lambda set_size, grouped: lib.vtc_l2_search_sets_workspace_bytes(4099, 1, set_size, 64, 64, grouped)
    assert size(1, 0) == lib.vtc_l2_search_workspace_bytes(4099, 1, 64, 64)          # a set of one member is the plain search
    assert size(1, 1) == lib.vtc_l2_search_grouped_workspace_bytes(4099, 1, 64, 64)
    assert size(1, 0) == size(2, 0) == size(4, 0) == size(8, 0) < size(9, 0) == size(16, 0) < size(17, 0) < size(64, 0)
    assert all(size(m, 0) < size(m, 1) for m in (1, 8, 9, 64))
    for m, grouped in ((9, 0), (9, 1), (64, 1)):
        _refused(_sets(ng=4099, n_sets=1, set_size=m, depth=64, ws_bytes=size(m, grouped) - 1, **(FORMS["grouped"] if grouped else {})),
                 b"workspace too small")


def test_abi_version_is_unchanged():
    assert L.lib().vtc_abi_version() == 7 == L.ABI_VERSION
