"""The reference of the grouped query-time search (vtc_l2_search_grouped, ops.l2_search_grouped, VideoIndex.search_videos), numpy fp64.

Definition (include/vtc_hip.h): take the complete list of live rows with a finite D(q, j), sorted by (D(q, j), j); delete every row that
is not the first of its group in that order; the first `depth` entries of what remains are the result -- per entry the row (id_base +
j), its group and its distance; the tail of a short list is ids = -1, groups = -1, dists = +inf.

Two independent formulations:
  (a) `reference_by_sort`    the definition's sentence: search_refs.distances64, a full lexsort by (distance, row), first-of-group, cut;
  (b) `reference_by_minima`  the group minima E(q, g) = min over the group's live finite rows, with the arg-min row (the lowest on a tie)
                             -- vunit_rank_refs.group_minima for arbitrary ids --, then the groups sorted by (minimum, row).

`min_gap` is search_refs' quantity over the COMPLETE sorted list of a query (not the de-duplicated one: the device decides every
neighbouring pair of it that it meets) up to one past the last returned entry: the smallest (d[p+1] - d[p]) / d[p+1] over neighbours that
are not bit-equal.  Every test that compares ids asserts it > 1e-12.
"""
import numpy as np

import search_refs as SR

GROUP_KINDS = ("singletons", "one", "pairs", "strided", "blocks_of_40", "random_50", "sparse_ids")
MASK_KINDS = ("all", "random_0.5", "first_half_dead", "none")


def make_groups(kind, n, seed=0):
    """The group kinds of the edge grid, int32 [n]."""
    j = np.arange(n)
    if kind == "singletons":
        g = j
    elif kind == "one":
        g = np.full(n, 5)
    elif kind == "pairs":
        g = j // 2
    elif kind == "strided":
        g = j % 7
    elif kind == "blocks_of_40":
        g = j // 40
    elif kind == "random_50":
        g = np.random.default_rng(2000 + seed).integers(0, 50, n)
    elif kind == "sparse_ids":
        pool = np.array([-1, -2 ** 31, 2 ** 31 - 1, 0, -7, 123456789, -987654321, 3, 1 << 30, -(1 << 30), 77], np.int64)
        g = pool[np.random.default_rng(3000 + seed).integers(0, pool.size, n)]
        g[:min(n, 4)] = pool[:min(n, 4)]                   # -1, INT32_MIN and INT32_MAX are always there (where n allows)
    else:
        raise ValueError(kind)
    return np.asarray(g, np.int64).astype(np.int32)


def _masked(D, live):
    D = np.array(D, np.float64)
    if live is not None:
        D[:, ~np.asarray(live, bool)] = np.inf
    return D


def _empty(nq, depth):
    return np.full((nq, depth), -1, np.int64), np.full((nq, depth), -1, np.int32), np.full((nq, depth), np.inf, np.float64)


def lists_by_sort(D, groups, depth, id_base=0):
    """(a) on a distance matrix whose dead rows are +inf: (ids, groups, dists64, min_gap)."""
    groups = np.asarray(groups, np.int32)
    nq = D.shape[0]
    ids, grp, d64 = _empty(nq, depth)
    min_gap = np.inf
    for i in range(nq):
        fin = np.flatnonzero(np.isfinite(D[i]))
        order = fin[np.lexsort((fin, D[i, fin]))]
        seen, kept = set(), []
        for pos, j in enumerate(order):
            if int(groups[j]) not in seen:
                seen.add(int(groups[j]))
                kept.append((pos, j))
                if len(kept) == depth + 1:
                    break
        take = kept[:depth]
        for p, (_, j) in enumerate(take):
            ids[i, p], grp[i, p], d64[i, p] = id_base + j, groups[j], D[i, j]
        # the complete list up to one past the last returned entry (to its end when fewer than depth + 1 groups exist)
        upto = kept[depth][0] + 1 if len(kept) > depth else order.size
        ds = D[i, order[:upto]]
        gaps = np.flatnonzero(ds[1:] != ds[:-1])
        if gaps.size:
            min_gap = min(min_gap, float(np.min((ds[gaps + 1] - ds[gaps]) / ds[gaps + 1])))
    return ids, grp, d64, float(min_gap)


def lists_by_minima(D, groups, depth, id_base=0):
    """(b): (ids, groups, dists64)."""
    groups = np.asarray(groups, np.int32)
    nq, n = D.shape
    ids, grp, d64 = _empty(nq, depth)
    uniq, inv = np.unique(groups, return_inverse=True)
    members = [np.flatnonzero(inv == u) for u in range(uniq.size)]      # ascending rows: argmin takes the lowest row of a tie
    for i in range(nq):
        best = []
        for u, rows in enumerate(members):
            vals = np.where(np.isfinite(D[i, rows]), D[i, rows], np.inf)
            a = int(np.argmin(vals))
            if np.isfinite(vals[a]):
                best.append((vals[a], int(rows[a]), int(uniq[u])))
        best.sort(key=lambda t: (t[0], t[1]))
        for p, (v, j, g) in enumerate(best[:depth]):
            ids[i, p], grp[i, p], d64[i, p] = id_base + j, g, v
    return ids, grp, d64


def reference_search_grouped64(gallery, queries, groups, depth, live=None, id_base=0):
    """(ids [Q, depth] int64, groups [Q, depth] int32, dists64 [Q, depth], min_gap) by formulation (a)."""
    return lists_by_sort(_masked(SR.distances64(gallery, queries), live), groups, depth, id_base)


def reference_search_grouped(gallery, queries, groups, depth, live=None, id_base=0):
    """The same with the fp32 distances of the C ABI's `dists`."""
    ids, grp, d64, gap = reference_search_grouped64(gallery, queries, groups, depth, live, id_base)
    return ids, grp, d64.astype(np.float32), gap


def reference_by_minima(gallery, queries, groups, depth, live=None, id_base=0):
    return lists_by_minima(_masked(SR.distances64(gallery, queries), live), groups, depth, id_base)


def reference_nonfinite_bits(gallery, queries, live=None):
    g = np.asarray(gallery) if live is None else np.asarray(gallery)[np.asarray(live, bool)]
    return int(not np.isfinite(g).all()) | 2 * int(not np.isfinite(np.asarray(queries)).all())


def merge_grouped_lists(parts, depth):
    """parts: [(ids [Q, *], groups [Q, *], dists64 [Q, *])] of grouped searches over disjoint windows -> (ids, groups, dists64) [Q, depth]
    of the union: all entries by (dist, id), the first of every group kept; entries with id -1 are ignored."""
    nq = parts[0][0].shape[0]
    ids, grp, d64 = _empty(nq, depth)
    for i in range(nq):
        pi = np.concatenate([p[0][i] for p in parts])
        pg = np.concatenate([p[1][i] for p in parts])
        pd = np.concatenate([p[2][i] for p in parts])
        keep = pi >= 0
        pi, pg, pd = pi[keep], pg[keep], pd[keep]
        seen, p = set(), 0
        for o in np.lexsort((pi, pd)):
            if int(pg[o]) in seen:
                continue
            seen.add(int(pg[o]))
            ids[i, p], grp[i, p], d64[i, p] = pi[o], pg[o], pd[o]
            p += 1
            if p == depth:
                break
    return ids, grp, d64
