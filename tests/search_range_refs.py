"""The reference of the range search (vtc_l2_range_count / vtc_l2_range_fill, ops.l2_range_search, VideoIndex.range_search), numpy fp64.

Semantics (include/vtc_hip.h): with D = search_refs.distances64 (the fp64 squared distances of the fp32 inputs), row j is a hit of query
q iff it is live, D[q, j] is finite and D[q, j] <= radius2[q].  A NaN or negative radius gives no hits, +inf every live finite row; a
query with a NaN / inf has no finite distance, so no hits.  Per query the hits come in ascending row order; lims is their prefix sum.

`min_margin`: the smallest |D - r| / max(r, tiny) over all (query, live row) pairs with a finite D and a finite r >= 0 -- how far the
nearest distance is from deciding differently under another summation order.  Every GPU test that compares membership with this
reference asserts min_margin > 1e-12; `midpoint_radii` chooses radii halfway between consecutive sorted distances so that this holds by
construction and nothing is left out of a comparison.
"""
import numpy as np

import search_refs as R
from search_mask_refs import pack_words  # noqa: F401  (vtc_row_mask_pack's format: what the hit words are compared with)

TINY = np.finfo(np.float64).tiny


def range_lists(D, radius2, live=None, id_base=0):
    """(lims [Q + 1] int64, ids [total] int64, dists64 [total], member [Q, n] bool, min_margin) of a distance matrix D [Q, n]."""
    D = np.asarray(D, np.float64)
    nq, n = D.shape
    r = np.broadcast_to(np.asarray(radius2, np.float64), (nq,))
    live = np.ones(n, bool) if live is None else np.asarray(live, bool)
    with np.errstate(all="ignore"):
        finite = np.isfinite(D) & live[None, :]
        member = finite & (D <= r[:, None])
    lims = np.zeros(nq + 1, np.int64)
    ids, d64, margin = [], [], np.inf
    for q in range(nq):
        rows = np.flatnonzero(member[q])
        lims[q + 1] = lims[q] + rows.size
        ids.append(id_base + rows.astype(np.int64))
        d64.append(D[q, rows])
        if np.isfinite(r[q]) and r[q] >= 0 and finite[q].any():
            margin = min(margin, float(np.min(np.abs(D[q, finite[q]] - r[q])) / max(r[q], TINY)))
    return lims, np.concatenate(ids) if ids else np.empty(0, np.int64), np.concatenate(d64) if d64 else np.empty(0), member, float(margin)


def reference_range(gallery, queries, radius2, live=None, id_base=0):
    """range_lists of the inputs' fp64 distances."""
    return range_lists(R.distances64(gallery, queries), radius2, live, id_base)


def midpoint_radii(D, counts, live=None):
    """radius2 [Q]: for query q the midpoint between its counts[q]-th and (counts[q] + 1)-th smallest DISTINCT finite live distances, so
    that exactly the rows up to and including the counts[q]-th distinct value are hits and no distance is near the radius.  counts[q] = 0:
    half the smallest distance (no hits, unless that distance is 0); counts[q] >= the number of distinct values: twice the largest."""
    D = np.asarray(D, np.float64)
    live = np.ones(D.shape[1], bool) if live is None else np.asarray(live, bool)
    out = np.empty(D.shape[0], np.float64)
    for q, c in enumerate(np.broadcast_to(np.asarray(counts), (D.shape[0],))):
        v = np.unique(D[q, live & np.isfinite(D[q])])
        if v.size == 0:
            out[q] = 1.0
        elif c <= 0:
            out[q] = v[0] / 2
        elif c >= v.size:
            out[q] = v[-1] * 2 if v[-1] > 0 else 1.0
        else:
            out[q] = (v[c - 1] + v[c]) / 2
    return out

