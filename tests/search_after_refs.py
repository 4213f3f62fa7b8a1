"""The reference of the cursor search (vtc_l2_search_after, ops.l2_search(after=...), VideoIndex.search(after=...) / search_deep), numpy.

Definition (include/vtc_hip.h): the search order of a query is the total order of its LIVE rows with a FINITE distance by the key
(D(q, j), j) -- the fp64 distance of search_refs.distances64, then the row.  The cursor of query q is the row after_ids[q]; its key is
(the reference's own D(q, after_ids[q]), after_ids[q]), taken whether or not that row is live.  The result is the first `depth` rows of
the order whose key is strictly greater than the cursor's, padded with -1 / +inf.  A cursor of -1, or one that is no row of the gallery
(outside [id_base, id_base + n)), has no key: the list is empty.

`min_gap` is search_refs.sorted_lists' over the FULL order of every query (depth = the number of rows): a page can begin anywhere in
it, so every neighbouring pair of the order has to be decided by more than a summation order.
"""
import numpy as np

import search_refs as SR


def full_order(gallery, queries, live=None, id_base=0):
    """(ids [Q, n] int64, dists64 [Q, n], min_gap): the whole search order of the live finite rows, padded with -1 / +inf."""
    D = SR.distances64(gallery, queries)
    if live is not None:
        D = D.copy()
        D[:, ~np.asarray(live, bool)] = np.inf
    return SR.sorted_lists(D, D.shape[1], id_base)


def reference_search_after(gallery, queries, depth, after_ids, live=None, id_base=0):
    """(ids [Q, depth] int64, dists64 [Q, depth] fp64, min_gap) -- see the module docstring.  after_ids: int64 [Q], global ids."""
    after_ids = np.asarray(after_ids, np.int64)
    D = SR.distances64(gallery, queries)                     # the cursor's key comes from here: a dead row has one too
    order, d64, gap = full_order(gallery, queries, live, id_base)
    nq, n = D.shape
    ids = np.full((nq, depth), -1, np.int64)
    out = np.full((nq, depth), np.inf, np.float64)
    for i in range(nq):
        a = int(after_ids[i])
        if not id_base <= a < id_base + n:
            continue
        cd = D[i, a - id_base]
        valid = order[i] >= 0
        keep = valid & ((d64[i] > cd) | ((d64[i] == cd) & (order[i] > a)))
        rest_i, rest_d = order[i][keep][:depth], d64[i][keep][:depth]
        ids[i, :rest_i.size], out[i, :rest_d.size] = rest_i, rest_d
    return ids, out, gap


def tied_gallery(rows, seed):
    """The gallery of exact ties: `rows` repeated five times and permuted -- every distance occurs five times, bit for bit."""
    rng = np.random.default_rng(seed)
    g = np.tile(np.asarray(rows), (5, 1))
    return np.ascontiguousarray(g[rng.permutation(g.shape[0])])
