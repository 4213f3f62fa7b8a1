"""The reference of the paged grouped search (vtc_l2_group_mark_before + vtc_l2_search_grouped_after, ops.l2_search_grouped(after=...),
VideoIndex.search_videos(after=...) / search_videos_deep / similar_videos(after=...)), numpy fp64.

Definition (include/vtc_hip.h): for query q the ADMISSIBLE rows are the live rows with a finite D(q, j), minus the rows of the query's
excluded group where one is given.  K(q, g) is the smallest key (D(q, j), id_base + j) over the admissible rows of group g; the grouped
order of q is the groups with an admissible row, sorted by K.  The page after the cursor key (D*, r*) is the first `depth` groups of that
order with K strictly after it (K.d > D*, or K.d == D* and K.row > r*), each with its nearest row and that row's distance; the tail is
ids = -1, groups = -1, dists = +inf.

The cursor of query q is the ROW after_ids[q] (a global id): its key is (the reference's own D(q, after_ids[q]), after_ids[q]), taken
from the distances BEFORE the mask and the exclusion -- the cursor row may be dead or belong to the excluded group.  A cursor of -1, or
one that is no row of the gallery (outside [id_base, id_base + n)), has no key: the page is empty.

Two independent formulations:
  (a) `page_by_sort`    the full grouped order from search_grouped_refs.lists_by_sort at depth n, filtered by key > cursor, then cut;
  (b) `page_by_minima`  the group minima over the admissible rows with their arg-min rows (the lowest on a tie), the groups kept whose
                        (minimum, row) lies after the cursor, then sorted.

`min_gap` is taken over the FULL order of the admissible rows of every query (search_refs.sorted_lists at depth n), as search_after_refs
takes it: a page can begin anywhere, and the mark pass decides every row against the cursor.
"""
import numpy as np

import search_exclude_refs as XR
import search_grouped_refs as GR
import search_refs as SR


def dense_slots(video_ids):
    """(uniq, slot): arbitrary integer video ids -> the sorted distinct ids and, per row, the dense group number in [0, uniq.size) that
    the paged entries take (int32)."""
    uniq, slot = np.unique(np.asarray(video_ids, np.int64), return_inverse=True)
    return uniq, np.asarray(slot, np.int64).reshape(-1).astype(np.int32)


def admissible(D, groups, live=None, exclude=None):
    """D [Q, n] with the dead rows and (exclude given: int64 [Q] of groups) every query's excluded group set to +inf (a copy)."""
    ex = np.full(D.shape[0], 2 ** 40, np.int64) if exclude is None else np.asarray(exclude, np.int64)
    return XR.excluded_distances(D, ex, live, groups)


def cursor_keys(D, after_ids, id_base=0):
    """[(D(q, cursor row), cursor id) or None]: from the distances as they are, live or not."""
    n = D.shape[1]
    return [(D[i, int(a) - id_base], int(a)) if id_base <= int(a) < id_base + n else None for i, a in enumerate(np.asarray(after_ids, np.int64))]


def full_min_gap(A):
    """search_refs' min_gap over the full order of the admissible rows (A: admissible distances)."""
    return SR.sorted_lists(A, A.shape[1])[2]


def page_by_sort(D, groups, depth, after_ids, live=None, exclude=None, id_base=0):
    """(a): (ids [Q, depth] int64, groups [Q, depth] int32, dists64 [Q, depth], min_gap over the full order)."""
    A = admissible(D, groups, live, exclude)
    n = A.shape[1]
    order, grp, d64, _ = GR.lists_by_sort(A, groups, n, id_base)
    ids, out_g, out_d = GR._empty(A.shape[0], depth)
    for i, key in enumerate(cursor_keys(D, after_ids, id_base)):
        if key is None:
            continue
        cd, a = key
        keep = (order[i] >= 0) & ((d64[i] > cd) | ((d64[i] == cd) & (order[i] > a)))
        m = min(depth, int(keep.sum()))
        ids[i, :m], out_g[i, :m], out_d[i, :m] = order[i][keep][:m], grp[i][keep][:m], d64[i][keep][:m]
    return ids, out_g, out_d, full_min_gap(A)


def page_by_minima(D, groups, depth, after_ids, live=None, exclude=None, id_base=0):
    """(b): (ids, groups, dists64)."""
    A = admissible(D, groups, live, exclude)
    groups = np.asarray(groups, np.int32)
    ids, out_g, out_d = GR._empty(A.shape[0], depth)
    uniq, inv = np.unique(groups, return_inverse=True)
    members = [np.flatnonzero(inv == u) for u in range(uniq.size)]      # ascending rows: argmin takes the lowest row of a tie
    for i, key in enumerate(cursor_keys(D, after_ids, id_base)):
        if key is None:
            continue
        cd, a = key
        best = []
        for u, rows in enumerate(members):
            p = int(np.argmin(A[i, rows]))
            v, j = A[i, rows[p]], id_base + int(rows[p])
            if np.isfinite(v) and (v > cd or (v == cd and j > a)):
                best.append((v, j, int(uniq[u])))
        best.sort(key=lambda t: (t[0], t[1]))
        for p, (v, j, g) in enumerate(best[:depth]):
            ids[i, p], out_g[i, p], out_d[i, p] = j, g, v
    return ids, out_g, out_d


def full_grouped_order(D, groups, live=None, exclude=None, id_base=0):
    """(ids [Q, n], groups [Q, n], dists64 [Q, n], min_gap over the full order): the whole grouped order, padded with -1 / -1 / +inf."""
    A = admissible(D, groups, live, exclude)
    ids, grp, d64, _ = GR.lists_by_sort(A, groups, A.shape[1], id_base)
    return ids, grp, d64, full_min_gap(A)


def chained_pages(D, groups, depth, live=None, exclude=None, id_base=0, page=page_by_sort):
    """The pages of `depth` chained by their last rows until every query's page is empty, concatenated: (ids, groups, dists64) [Q, *].
    Page 1 is the plain grouped search (no cursor)."""
    A = admissible(D, groups, live, exclude)
    first = GR.lists_by_sort(A, groups, depth, id_base)[:3]
    pages = [first]
    while (pages[-1][0][:, -1] >= 0).any():
        pages.append(page(D, groups, depth, pages[-1][0][:, -1], live, exclude, id_base)[:3])
    return tuple(np.concatenate([p[k] for p in pages], axis=1) for k in range(3))


# ---- the inputs the GPU tests compare ids on (tests/test_gpu_search_grouped_after.py), built here so that the CPU test can establish the
# exactness condition on them: min_gap > 1e-12 over the FULL order of ALL rows of every query.  Deleting rows from an order (a mask, a
# shorter gallery, an excluded group, a subset) only widens its gaps, so the one check per input covers every case drawn from it.
SIMILAR_ROWS = np.arange(2, 2 + 70 * 14, 14, dtype=np.int64)      # the stored rows the index-level tests take as queries
WIDTHS = (192, 2048)


def main_rows(storage):
    """(gallery [1027, 512] as the reference sees it -- for float16 rounded to half and widened again --, queries [70, 512]), unit rows."""
    import rank_refs as RR
    a, b = RR.spread_pairs(1027, 512, 31)
    return (a if storage == "float32" else a.astype(np.float16).astype(np.float32)), b[:70]


def width_rows(d):
    import rank_refs as RR
    a, b = RR.spread_pairs(257, d, 40 + d)
    return a, b[:3]


def tied_rows():
    """260 rows, every distance five times bit for bit (search_after_refs.tied_gallery), and 3 queries."""
    import rank_refs as RR
    import search_after_refs as AR
    a, b = RR.spread_pairs(52, 512, 33)
    return AR.tied_gallery(a, 5), b[:3]


def gpu_inputs():
    """(name, gallery, queries) of every input the GPU tests compare ids on."""
    for storage in ("float32", "float16"):
        g, q = main_rows(storage)
        yield f"main-{storage}", g, q
        yield f"similar-{storage}", g, g[SIMILAR_ROWS]
    for d in WIDTHS:
        yield (f"d{d}",) + width_rows(d)
    yield ("tied",) + tied_rows()
