"""CPU: the reference of the excluding search (tests/search_exclude_refs.py) against a brute-force loop on tiny inputs -- the definition
spelled out row by row, with Python's own sort and no shared code."""
import numpy as np
import pytest

import search_exclude_refs as XR
import search_grouped_refs as GR


def _tiny(n, nq, d=8, seed=0):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, d)).astype(np.float32)
    g[n // 2] = g[0]                                          # an exact duplicate: a tie that the row decides
    return g, rng.standard_normal((nq, d)).astype(np.float32)


def _dist(q, row):
    return float(sum((float(a) - float(b)) ** 2 for a, b in zip(q, row)))


def _brute(g, q, depth, exclude, live=None, groups=None, after=None, id_base=0):
    ids = np.full((q.shape[0], depth), -1, np.int64)
    grp = np.full((q.shape[0], depth), -1, np.int32)
    for i in range(q.shape[0]):
        keys = sorted((_dist(q[i], g[j]), j) for j in range(g.shape[0]) if live is None or live[j])
        if groups is None:
            keys = [k for k in keys if id_base + k[1] != int(exclude[i])]
        else:
            keys = [k for k in keys if int(groups[k[1]]) != int(exclude[i])]
            seen, first = set(), []
            for k in keys:
                if int(groups[k[1]]) not in seen:
                    seen.add(int(groups[k[1]]))
                    first.append(k)
            keys = first
        if after is not None:
            a = int(after[i]) - id_base
            keys = [k for k in keys if k > (_dist(q[i], g[a]), a)] if 0 <= a < g.shape[0] else []
        for p, (_, j) in enumerate(keys[:depth]):
            ids[i, p] = id_base + j
            if groups is not None:
                grp[i, p] = groups[j]
    return ids, grp


@pytest.mark.parametrize("n,depth", [(1, 1), (2, 2), (13, 5), (13, 13)])
@pytest.mark.parametrize("id_base", [0, 100])
def test_ungrouped_reference_is_the_definition(n, depth, id_base):
    g, q = _tiny(n, 6, seed=n)
    live = None if n < 13 else np.arange(n) % 4 != 1
    exclude = np.array([id_base + 0, id_base + n // 2, id_base + n - 1, -1, id_base + n, 2 ** 40], np.int64)
    ids, _, _ = XR.reference_search_excluding(g, q, depth, exclude, live=live, id_base=id_base)
    assert np.array_equal(ids, _brute(g, q, depth, exclude, live=live, id_base=id_base)[0])
    for i in range(3):
        assert exclude[i] not in ids[i]
    if n == 1:
        assert ids[0, 0] == -1 and ids[3, 0] == id_base      # its only row excluded: empty; -1 excludes nothing


@pytest.mark.parametrize("kind", ["one", "pairs", "random_50", "sparse_ids"])
def test_grouped_reference_is_the_definition(kind):
    n = 23
    g, q = _tiny(n, 6, seed=5)
    groups = GR.make_groups(kind, n, seed=1)
    live = np.arange(n) % 5 != 2
    exclude = np.array([groups[0], groups[1], groups[2], groups[n // 2], 2 ** 31, -2 ** 31 - 1], np.int64)
    ids, grp, _, _ = XR.reference_search_grouped_excluding(g, q, groups, 7, exclude, live=live)
    want = _brute(g, q, 7, exclude, live=live, groups=groups)
    assert np.array_equal(ids, want[0]) and np.array_equal(grp, want[1])
    for i in range(4):
        assert not (grp[i][ids[i] >= 0] == exclude[i]).any()
    if kind == "one":
        assert (ids[:4] == -1).all() and (ids[4:, 0] >= 0).all()


def test_cursor_on_the_excluded_row_and_on_a_dead_one():
    n = 17
    g, q = _tiny(n, 5, seed=9)
    live = np.arange(n) % 3 != 0
    exclude = np.array([4, 5, 7, -1, 8], np.int64)
    after = np.array([4, 3, 10, 8, -1], np.int64)             # the excluded row itself, a dead row, a live one, a live one, no row
    ids, _, _ = XR.reference_search_excluding_after(g, q, 6, exclude, after, live=live)
    assert np.array_equal(ids, _brute(g, q, 6, exclude, live=live, after=after)[0])
    assert (ids[4] == -1).all() and (ids[:4, 0] >= 0).all()
