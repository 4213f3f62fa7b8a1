"""The reference of the query-time search (vtc_l2_search, ops.l2_search, VideoIndex), numpy fp64.

Semantics (include/vtc_hip.h): D(q, j) = sum_k (queries[q][k] - gallery[j][k])^2 in fp64 of the fp32 inputs (fp32 differences are exact
in fp64, so the einsum below is exact to 1e-16 relative); ids[q] = id_base + j of the `depth` rows with the smallest (D(q, j), j),
compared lexicographically; rows with a non-finite distance are never returned, the lists are padded with -1 / +inf; dists = (float) D.

`min_gap`: per query, over the sorted finite distances d at positions p < min(depth, n_finite - 1), the smallest (d[p+1] - d[p]) / d[p+1]
over neighbours that are NOT bit-equal -- the minimum over the queries is returned.  Every test that compares ids requires it to exceed
1e-12, so that no summation order can decide an id; bit-equal neighbours (exact duplicates) go to the lower index by definition.
"""
import numpy as np


def distances64(gallery, queries):
    g, q = np.asarray(gallery, np.float32).astype(np.float64), np.asarray(queries, np.float32).astype(np.float64)
    out = np.empty((q.shape[0], g.shape[0]), np.float64)
    with np.errstate(all="ignore"):
        for i in range(q.shape[0]):
            e = q[i][None, :] - g
            out[i] = np.einsum("ij,ij->i", e, e)
    return out


def sorted_lists(D, depth, id_base=0):
    """(ids [Q, depth] int64, dists64 [Q, depth], min_gap) of a distance matrix D [Q, n]."""
    nq, n = D.shape
    ids = np.full((nq, depth), -1, np.int64)
    d64 = np.full((nq, depth), np.inf, np.float64)
    min_gap = np.inf
    for i in range(nq):
        fin = np.flatnonzero(np.isfinite(D[i]))
        order = fin[np.lexsort((fin, D[i, fin]))]              # by distance, then by index
        m = min(depth, order.size)
        ids[i, :m] = id_base + order[:m]
        d64[i, :m] = D[i, order[:m]]
        ds = D[i, order[:min(depth, order.size - 1) + 1]] if order.size else np.empty(0)
        for p in range(ds.size - 1):
            if ds[p + 1] != ds[p]:
                min_gap = min(min_gap, (ds[p + 1] - ds[p]) / ds[p + 1])
    return ids, d64, float(min_gap)


def reference_search(gallery, queries, depth, id_base=0):
    """(ids [Q, depth] int64, dists32 [Q, depth] fp32, min_gap) -- see the module docstring."""
    ids, d64, min_gap = sorted_lists(distances64(gallery, queries), depth, id_base)
    return ids, d64.astype(np.float32), min_gap


def reference_search64(gallery, queries, depth, id_base=0):
    """The same with the fp64 distances (what a merge of partial lists compares)."""
    return sorted_lists(distances64(gallery, queries), depth, id_base)


def merge_lists(parts, depth):
    """parts: [(ids [Q, *], dists64 [Q, *])] of searches over disjoint windows -> (ids, dists64) [Q, depth] of the union by (dist, id);
    entries with id -1 are ignored."""
    nq = parts[0][0].shape[0]
    ids = np.full((nq, depth), -1, np.int64)
    d64 = np.full((nq, depth), np.inf, np.float64)
    for i in range(nq):
        pi = np.concatenate([p[0][i] for p in parts])
        pd = np.concatenate([p[1][i] for p in parts])
        keep = pi >= 0
        pi, pd = pi[keep], pd[keep]
        order = np.lexsort((pi, pd))[:depth]
        ids[i, :order.size], d64[i, :order.size] = pi[order], pd[order]
    return ids, d64


def ulp32(x):
    """One unit in the last place of the fp32 values x (inf where x is not finite)."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(x), np.spacing(np.abs(x)), np.inf).astype(np.float64)


def assert_dists_within_one_ulp(got, want):
    """fp32 distances within one ulp of the reference's (numpy's summation order differs from the device's in the last fp64 bits, which can
    move the rounding to fp32 by one step); +inf entries must match exactly."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    inf = ~np.isfinite(want)
    assert np.array_equal(got[inf], want[inf])
    err = np.abs(got[~inf].astype(np.float64) - want[~inf].astype(np.float64))
    assert np.all(err <= ulp32(want[~inf])), float(err.max())
