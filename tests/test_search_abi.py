"""CPU: the argument checks of the query-time search entry points (vtc_l2_search, vtc_l2_search_merge).  Every refused call returns
non-zero with "search" in vtc_last_error() before anything is launched -- no GPU is needed, the pointers are never dereferenced."""
import pytest

from vtc_amd import _lib as L

P = 0x1000        # a non-null "device pointer": a refused call never touches it


def _search(ng=100, nq=4, d=64, depth=5, id_base=0, gallery=P, queries=P, ids=P, ws=P, ws_bytes=None):
    lib = L.lib()
    if ws_bytes is None:
        ws_bytes = max(lib.vtc_l2_search_workspace_bytes(ng, nq, d, depth), 1 << 20)
    return lib.vtc_l2_search(gallery, queries, ng, nq, d, depth, id_base, ids, None, None, ws, ws_bytes, None)


def _refused(rc):
    assert rc != 0 and b"search" in L.lib().vtc_last_error(), (rc, L.lib().vtc_last_error())


@pytest.mark.parametrize("kw", [
    dict(nq=0), dict(nq=65),
    dict(depth=0), dict(depth=65, ng=1000), dict(depth=11, ng=10),
    dict(d=32), dict(d=100), dict(d=2112),
    dict(ng=0, depth=1),
    dict(id_base=-1),
    dict(gallery=None), dict(queries=None), dict(ids=None), dict(ws=None),
    dict(ws_bytes=1),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_search_refuses(kw):
    _refused(_search(**kw))
    a = dict(ng=100, nq=4, d=64, depth=5)
    a.update({k: v for k, v in kw.items() if k in a})
    if set(kw) & set(a):                                     # a shape the call refuses has no workspace size
        assert L.lib().vtc_l2_search_workspace_bytes(a["ng"], a["nq"], a["d"], a["depth"]) == 0


def test_workspace_bytes_positive_and_non_decreasing_in_queries():
    lib = L.lib()
    for ng, d, depth in ((1, 64, 1), (63, 64, 11), (1027, 512, 64), (1_000_000, 512, 11), (2_000_000_000, 2048, 64)):
        sizes = [lib.vtc_l2_search_workspace_bytes(ng, nq, d, depth) for nq in range(1, 65)]
        assert sizes[0] > 0 and all(x <= y for x, y in zip(sizes, sizes[1:])), (ng, d, depth, sizes[:4])
        assert sizes[0] >= depth * 8                          # the documented fp64 list at the head of the workspace


@pytest.mark.parametrize("kw", [dict(n_parts=0), dict(n_parts=65), dict(nq=0), dict(nq=65), dict(depth=0), dict(depth=65),
                                dict(ids_parts=None), dict(dists_parts=None), dict(ids=None)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_merge_refuses(kw):
    a = dict(ids_parts=P, dists_parts=P, n_parts=3, nq=4, depth=5, ids=P)
    a.update(kw)
    _refused(L.lib().vtc_l2_search_merge(a["ids_parts"], a["dists_parts"], a["n_parts"], a["nq"], a["depth"], a["ids"], None, None))


def test_refused_calls_launch_nothing():
    lib = L.lib()
    before = lib.vtc_debug_launch_count()
    _refused(_search(nq=65))
    _refused(_search(ws_bytes=1))
    _refused(lib.vtc_l2_search_merge(P, P, 65, 4, 5, P, None, None))
    assert lib.vtc_debug_launch_count() == before
