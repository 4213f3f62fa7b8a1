"""The reference of the excluding search (vtc_l2_search_excluding, ops.l2_search(exclude=...) / ops.l2_search_grouped(exclude=...),
VideoIndex.search(exclude=...) / search_videos(exclude_videos=...) / similar / similar_videos), numpy fp64.

Definition (include/vtc_hip.h): take the search order of a query -- its live rows with a finite distance by (D(q, j), j) -- or the grouped
order; DELETE the excluded rows; then cut.  Here: search_refs.distances64, the excluded entries of each query's row of D set to +inf (a
row with a non-finite distance is in no order), then the existing search_refs.sorted_lists / search_grouped_refs.lists_by_sort.
  ungrouped: query q excludes the one row j with id_base + j == exclude[q];
  grouped:   query q excludes every row j with (int64) groups[j] == exclude[q].
A value no row / no group has excludes nothing.  With a cursor (after_ids, global ids): search_after_refs' rule applied to that D, the
cursor's own key (D(q, after), after) taken from the UN-excluded D -- the cursor may be the excluded row, or a dead one.
"""
import numpy as np

import search_grouped_refs as GR
import search_refs as SR


def excluded_distances(D, exclude, live=None, groups=None, id_base=0):
    """D [Q, n] with the dead rows and every query's excluded rows set to +inf (a copy)."""
    D = np.array(D, np.float64)
    if live is not None:
        D[:, ~np.asarray(live, bool)] = np.inf
    keys = id_base + np.arange(D.shape[1], dtype=np.int64) if groups is None else np.asarray(groups, np.int32).astype(np.int64)
    for i, e in enumerate(np.asarray(exclude, np.int64)):
        D[i, keys == e] = np.inf
    return D


def reference_search_excluding(gallery, queries, depth, exclude, live=None, id_base=0):
    """(ids [Q, depth] int64, dists64 [Q, depth], min_gap) of the ungrouped excluding search."""
    return SR.sorted_lists(excluded_distances(SR.distances64(gallery, queries), exclude, live, None, id_base), depth, id_base)


def reference_search_grouped_excluding(gallery, queries, groups, depth, exclude, live=None, id_base=0):
    """(ids, groups [Q, depth] int32, dists64, min_gap) of the grouped excluding search."""
    return GR.lists_by_sort(excluded_distances(SR.distances64(gallery, queries), exclude, live, groups, id_base), groups, depth, id_base)


def full_order_excluding(gallery, queries, exclude, live=None, id_base=0):
    """The whole order without the excluded rows, padded with -1 / +inf to n columns."""
    return reference_search_excluding(gallery, queries, np.asarray(gallery).shape[0], exclude, live, id_base)


def reference_search_excluding_after(gallery, queries, depth, exclude, after_ids, live=None, id_base=0):
    """(ids, dists64, min_gap): the first `depth` of the excluded order whose key lies strictly after the cursor's; a cursor that is no
    row of the gallery has no key and gives an empty list (search_after_refs.reference_search_after's rule)."""
    after_ids = np.asarray(after_ids, np.int64)
    D = SR.distances64(gallery, queries)                     # the cursor's key: from the un-excluded distances
    order, d64, gap = full_order_excluding(gallery, queries, exclude, live, id_base)
    nq, n = D.shape
    ids = np.full((nq, depth), -1, np.int64)
    out = np.full((nq, depth), np.inf, np.float64)
    for i in range(nq):
        a = int(after_ids[i])
        if not id_base <= a < id_base + n:
            continue
        cd = D[i, a - id_base]
        keep = (order[i] >= 0) & ((d64[i] > cd) | ((d64[i] == cd) & (order[i] > a)))
        rest_i, rest_d = order[i][keep][:depth], d64[i][keep][:depth]
        ids[i, :rest_i.size], out[i, :rest_d.size] = rest_i, rest_d
    return ids, out, gap
