"""GPU: every one of the 96 scans of vtc_amd/csrc/search.hip is the one its call should reach.  A call's arguments choose an
instantiation in one place (launch_scan_of): the tile shape by the number of queries, MASKED by ``live``, the gallery's element type,
and one of six modes by which of the groups, the cursor, the excluded key and the ban bitmap it has.  Every neighbouring instantiation
is legal code that would run and return a list, so each combination is compared here with the fp64 reference of ITS OWN semantics
(tests/*_refs.py), on data where the six modes' references differ pairwise wherever they can be compared and the mask changes every
one of them -- a call that reached a neighbour cannot pass.

333 gallery rows: no multiple of 32, 4 or 2, so the last mask word and the last step of every tile shape are partial.  n_queries 1, 2, 3
and 9 are the four tile shapes, the last tile partial.  Ids and groups are compared exactly (every reference order has min_gap >
1e-12), fp32 distances within one ulp."""
import functools

import numpy as np
import pytest
import torch

import search_after_refs as AR
import search_exclude_refs as XR
import search_grouped_after_refs as PR
import search_grouped_refs as GR
import search_mask_refs as MR
import search_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NG, D_, DEPTH = 333, 64, 5
NQS = (1, 2, 3, 9)
STORAGES = ("float32", "float16")
MODES = ("plain", "grouped", "cursor", "cursor_excluding", "grouped_excluding", "page")
N_GROUPS = 111


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def _data():
    rng = np.random.default_rng(96)
    rows = rng.standard_normal((NG, D_)).astype(np.float32)
    queries = (rows[rng.choice(NG, 9, replace=False)] + 0.5 * rng.standard_normal((9, D_))).astype(np.float32)
    groups = rng.permutation(np.arange(NG) // 3).astype(np.int32)          # 111 dense groups of three rows, anywhere
    live = rng.random(NG) < 0.5
    return rows, queries, groups, live


@functools.lru_cache(maxsize=None)
def _refs(storage, masked):
    """The six modes' references for all nine queries (a case with fewer takes the first rows), and the arguments that make them differ:
    the cursor stands on each query's third row (third video), the excluded row is the one right after the cursor, the excluded group
    that of the query's nearest row (the page's: of the video right after the cursor)."""
    rows, queries, groups, live = _data()
    g = rows if storage == "float32" else rows.astype(np.float16).astype(np.float32)          # what the scan sees, widened
    live = live if masked else None
    D = SR.distances64(g, queries)
    L = XR.excluded_distances(D, np.full(9, -1), live)                     # the dead rows at +inf
    order, _, gap = SR.sorted_lists(L, NG)
    assert gap > 1e-12, gap
    gorder, ggrp, _, _ = GR.lists_by_sort(L, groups, N_GROUPS)
    a = dict(after=order[:, 2].copy(), exclude=order[:, 3].copy(), ex_group=ggrp[:, 0].astype(np.int64),
             page_after=gorder[:, 2].copy(), page_ex_group=ggrp[:, 3].astype(np.int64))
    want = {"plain": SR.sorted_lists(L, DEPTH)[:2],
            "grouped": GR.lists_by_sort(L, groups, DEPTH)[:3],
            "cursor": AR.reference_search_after(g, queries, DEPTH, a["after"], live)[:2],
            "cursor_excluding": XR.reference_search_excluding_after(g, queries, DEPTH, a["exclude"], a["after"], live)[:2],
            "grouped_excluding": XR.reference_search_grouped_excluding(g, queries, groups, DEPTH, a["ex_group"], live)[:3],
            "page": PR.page_by_sort(D, groups, DEPTH, a["page_after"], live, a["page_ex_group"])[:3]}
    for m, w in want.items():
        assert (w[0] >= 0).all(), m                            # every list is full: 333 rows, about half of them live
    return a, want


def test_the_references_tell_the_instantiations_apart():
    """The data's own property, checked once: for every query, no two modes that return the same kind of list agree; the mask changes
    every list of the first query and the storage every distance -- so equality with a combination's own reference excludes every
    neighbour."""
    for storage in STORAGES:
        for masked in (False, True):
            _, want = _refs(storage, masked)
            for group in (("plain", "cursor", "cursor_excluding"), ("grouped", "grouped_excluding", "page")):
                for i, m in enumerate(group):
                    for other in group[i + 1:]:
                        assert not (want[m][0] == want[other][0]).all(axis=1).any(), (storage, masked, m, other)
        for m in MODES:                                        # query 0 is part of every case
            assert not (_refs(storage, False)[1][m][0][0] == _refs(storage, True)[1][m][0][0]).all(), (storage, m)
    for masked in (False, True):
        for m in MODES:                                        # the same rows, but not the same fp64 distances
            a, b = _refs("float32", masked)[1][m], _refs("float16", masked)[1][m]
            assert not (a[-1] == b[-1]).any(), (masked, m)


@pytest.fixture(scope="module")
def dev():
    rows, queries, groups, live = _data()
    return {"float32": _t(rows), "float16": _t(rows.astype(np.float16)), "queries": _t(queries), "groups": _t(groups),
            "live": _t(MR.pack_words(live).view(np.int32))}


@pytest.mark.parametrize("masked", [False, True], ids=["all", "half-live"])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("mode", MODES)
def test_every_combination_reaches_its_own_scan(dev, mode, nq, storage, masked):
    from vtc_amd import ops
    a, want = _refs(storage, masked)
    g, q, groups = dev[storage], dev["queries"][:nq].contiguous(), dev["groups"]
    live = dev["live"] if masked else None

    def cursor(ids):                                           # the cursor's distance with the bits the scan forms
        ids = _t(ids[:nq])
        return ops.l2_pair_dists64(g, q, ids), ids
    if mode == "plain":
        got = ops.l2_search(g, q, DEPTH, live=live)
    elif mode == "cursor":
        got = ops.l2_search(g, q, DEPTH, live=live, after=cursor(a["after"]))
    elif mode == "cursor_excluding":
        got = ops.l2_search(g, q, DEPTH, live=live, after=cursor(a["after"]), exclude=_t(a["exclude"][:nq]))
    elif mode == "grouped":
        got = ops.l2_search_grouped(g, q, groups, DEPTH, live=live)
    elif mode == "grouped_excluding":
        got = ops.l2_search_grouped(g, q, groups, DEPTH, live=live, exclude=_t(a["ex_group"][:nq]))
    else:
        got = ops.l2_search_grouped(g, q, groups, DEPTH, live=live, exclude=_t(a["page_ex_group"][:nq]), after=cursor(a["page_after"]),
                                    n_groups=N_GROUPS)
    w = want[mode]
    assert np.array_equal(got[0].cpu().numpy(), w[0][:nq])
    if len(w) == 3:
        assert np.array_equal(got[1].cpu().numpy(), w[1][:nq])
    SR.assert_dists_within_one_ulp(got[-2].cpu().numpy(), w[-1][:nq].astype(np.float32))
    assert int(got[-1].item()) == 0
