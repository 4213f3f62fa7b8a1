"""The reference of the set queries (vtc_l2_search_sets, ops.l2_search_sets, VideoIndex.search_any / search_videos_any /
similar_to_video), numpy fp64, built on the references of the searches they extend.

Definition (include/vtc_hip.h): a set query S is m >= 1 member vectors and E(S, j) = min over the members v of S with only finite
components of D(v, j), D being search_refs.distances64.  Ungrouped, the result is search_refs.sorted_lists(E, depth); grouped,
search_grouped_refs.lists_by_sort(E, groups, depth).  A dead row, an excluded row (ungrouped) and the rows of an excluded group
(grouped) are +inf in E.  `min_gap` is those functions' quantity on E; every test that compares ids asserts it > 1e-12.  Bit-equal
neighbours (duplicate gallery rows; duplicate members make none) go to the lower row by the definition.

Two independent formulations:
  (a) `reference_sets` / `reference_sets_grouped`  the minimum first, then ONE sort;
  (b) `merge_member_lists`                         what a host would do, and what the device's merge over tiles does with tiles of one
                                                   member: the top-`depth` list of every member by itself, all of them concatenated,
                                                   sorted by (distance, id), the first entry of every row (or group) kept, cut.
"""
import functools

import numpy as np

import search_exclude_refs as XR
import search_grouped_refs as GR
import search_refs as SR


def member_distances64(gallery, query_sets, sizes=None):
    """D [S, M, n] with the members that take no part -- a NaN / inf component, or at / past sizes[s] -- at +inf."""
    q = np.asarray(query_sets, np.float32)
    n_sets, m, _ = q.shape
    D = SR.distances64(gallery, q.reshape(n_sets * m, -1)).reshape(n_sets, m, -1)
    out = np.isfinite(q).all(axis=2)
    if sizes is not None:
        out &= np.arange(m)[None, :] < np.asarray(sizes)[:, None]
    D[~out] = np.inf
    return D


def set_distances64(gallery, query_sets, sizes=None):
    """E [S, n]: np.min over the finite members; a row with a NaN / inf stays non-finite (it is never returned)."""
    D = member_distances64(gallery, query_sets, sizes)
    with np.errstate(all="ignore"):
        E = np.min(np.where(np.isnan(D), np.inf, D), axis=1)
    bad_rows = ~np.isfinite(np.asarray(gallery, np.float32)).all(axis=1)
    E[:, bad_rows] = np.nan
    return E


def admissible(E, live=None, exclude=None, groups=None, id_base=0):
    """E with the dead rows and every set's excluded row / group at +inf (a copy)."""
    return XR.excluded_distances(E, np.full(E.shape[0], -1 << 40, np.int64) if exclude is None else exclude, live, groups, id_base)


def reference_sets(gallery, query_sets, depth, sizes=None, live=None, exclude=None, id_base=0):
    """(ids [S, depth] int64, dists64 [S, depth], min_gap)."""
    return SR.sorted_lists(admissible(set_distances64(gallery, query_sets, sizes), live, exclude, None, id_base), depth, id_base)


def reference_sets_grouped(gallery, query_sets, groups, depth, sizes=None, live=None, exclude=None, id_base=0):
    """(ids, groups [S, depth] int32, dists64, min_gap)."""
    return GR.lists_by_sort(admissible(set_distances64(gallery, query_sets, sizes), live, exclude, groups, id_base), groups, depth, id_base)


def merge_member_lists(gallery, query_sets, depth, groups=None, sizes=None, live=None, exclude=None, id_base=0):
    """(b): (ids, dists64), grouped (ids, groups, dists64)."""
    D = member_distances64(gallery, query_sets, sizes)
    bad_rows = ~np.isfinite(np.asarray(gallery, np.float32)).all(axis=1)
    n_sets, m, _ = D.shape
    ids = np.full((n_sets, depth), -1, np.int64)
    d64 = np.full((n_sets, depth), np.inf, np.float64)
    grp = np.full((n_sets, depth), -1, np.int32)
    for s in range(n_sets):
        Ds = np.array(D[s])
        Ds[:, bad_rows] = np.nan
        ex = None if exclude is None else np.full(m, exclude[s], np.int64)
        Ds = admissible(Ds, live, ex, groups, id_base)
        pi, pd = [], []
        for Dm in Ds:                                          # the member's own list: its first `depth` rows / first rows of groups
            fin = np.flatnonzero(np.isfinite(Dm))
            order = fin[np.lexsort((fin, Dm[fin]))]
            if groups is not None:
                order = order[np.sort(np.unique(np.asarray(groups)[order], return_index=True)[1])]
            pi.append(id_base + order[:depth])
            pd.append(Dm[order[:depth]])
        pi, pd = np.concatenate(pi), np.concatenate(pd)
        seen, p = set(), 0
        for o in np.lexsort((pi, pd)):
            key = int(pi[o]) if groups is None else int(groups[pi[o] - id_base])
            if key in seen:
                continue
            seen.add(key)
            ids[s, p], d64[s, p] = pi[o], pd[o]
            if groups is not None:
                grp[s, p] = groups[pi[o] - id_base]
            p += 1
            if p == depth:
                break
    return (ids, d64) if groups is None else (ids, grp, d64)


def attaining_members(gallery, query_sets, rows, sizes=None, id_base=0):
    """int64 [S, k]: the lowest member that attains E for every returned row, -1 where the row is -1."""
    D = member_distances64(gallery, query_sets, sizes)
    rows = np.asarray(rows, np.int64)
    out = np.full(rows.shape, -1, np.int64)
    for s in range(rows.shape[0]):
        for p, r in enumerate(rows[s]):
            if r >= 0:
                col = D[s, :, r - id_base]
                out[s, p] = int(np.argmin(np.where(np.isfinite(col), col, np.inf)))
    return out


def nonfinite_bits(gallery, query_sets, live=None):
    g = np.asarray(gallery) if live is None else np.asarray(gallery)[np.asarray(live, bool)]
    return int(not np.isfinite(g).all()) | 2 * int(not np.isfinite(np.asarray(query_sets)).all())


# ---- the shapes of the grid (tests/test_search_set_refs.py on the CPU, tests/test_gpu_search_sets.py on the device) --------------------
SET_SIZES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 64)              # every tile shape, one tile and several, a ragged last tile
DEPTHS = (1, 7, 64)
NG = (1, 3, 257, 1000, 4099)


def n_sets_of(m):
    """S in {1, 3, the most that fit in 64}, without repeats, for sets of m members."""
    return sorted({1, min(3, 64 // m), 64 // m})


def grid():
    """(ng, d, M, S, depth): every M x every S x every depth (depth <= ng) -- the galleries and widths in rotation, so that every ng meets
    every tile shape somewhere and the whole grid stays a few hundred small searches."""
    cases, i = [], 0
    for m in SET_SIZES:
        for s in n_sets_of(m):
            for depth in DEPTHS:
                ng = NG[i % len(NG)]
                if depth > ng:
                    ng = next(n for n in NG if n >= depth)
                cases.append((ng, (64, 128)[i % 2], m, s, depth))
                i += 1
    return cases


def grouped_grid():
    """(ng, d, M, S, depth, group kind): every case of the grid with every kind of search_grouped_refs.GROUP_KINDS."""
    return [case + (gk,) for case in grid() for gk in GR.GROUP_KINDS]


@functools.lru_cache(maxsize=4)
def case_distances(ng, d, m, s, half):
    """(gallery as stored -- fp32, or rounded to binary16 --, query_sets, E [S, n] over the stored rows widened) of a grid case, formed
    once and shared by the tests of the case (they follow each other); nobody writes to them."""
    g, q = make_case(ng, d, m, s, seed=ng + 7 * m + s)
    stored = g.astype(np.float16) if half else g
    E = set_distances64(stored.astype(np.float32), q)
    for x in (stored, q, E):
        x.setflags(write=False)
    return stored, q, E


def make_case(ng, d, m, s, seed):
    """(gallery [ng, d], query_sets [s, m, d]) unit rows: the members of a set are spread over the gallery's neighbourhoods, so that
    different members -- and different tiles -- own different parts of a result."""
    rng = np.random.default_rng(seed)
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    g = unit(rng.standard_normal((ng, d)))
    near = g[rng.integers(0, ng, (s, m))]
    q = unit(near + 0.35 * unit(rng.standard_normal((s, m, d))))
    return g.astype(np.float32), q.astype(np.float32)
