"""The reference of the rank-sharded counting sweep (vtc_l2_rank_shard, dist.sharded_ranks), numpy fp64 on top of tests/rank_refs.py, and
the windows its tests cut.

A rank owns the rows [lo, hi) of D[i][j] = |b_i - a_j|^2.  Its rank_a is a slice of the unsharded reference; its share of rank_b is

    partial_b(a, b, lo, hi)[j] = #{ i in [lo, hi) : (D(i, j), i) < (D(j, j), j) }      D(j, j) finite
                               = n if lo <= j < hi else 0                              otherwise

(a row of b with a non-finite entry is never closer), and the partials of windows that tile [0, n) add up to reference_ranks(a, b)[1].
"""
import functools

import numpy as np

import rank_refs as RR


def shard_cuts(n, world):
    """The cut list of vtc_amd.dist.shard_bounds: contiguous shards whose sizes differ by at most one ([0, ..., n], world + 1 entries;
    shards are empty when n < world)."""
    base, rem = divmod(n, world)
    return [r * base + min(r, rem) for r in range(world)] + [n]


def windows(cuts):
    """[(lo, hi), ...] of a cut list."""
    return list(zip(cuts[:-1], cuts[1:]))


def column_direction(a, b):
    """(D, dt, bad_b) of the column direction, from the paired reference's own function: D[j, i] = |a_j - b_i|^2 (query a_j, gallery b),
    the entries near a target in the exact form; dt[j] = D[j, j]; bad_b = the rows of b that are never closer."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    bad_b = np.flatnonzero(~np.isfinite(b).all(1))
    _, _, D, dt = RR._one_direction(a, b, bad_b)
    return D, dt, bad_b


def partial_from(D, dt, bad_b, lo, hi):
    n = dt.shape[0]
    idx = np.arange(n)
    with np.errstate(all="ignore"):
        Dw = D[:, lo:hi]
        iw = idx[None, lo:hi]
        closer = (Dw < dt[:, None]) | ((Dw == dt[:, None]) & (iw < idx[:, None]))
    closer &= iw != idx[:, None]
    closer[:, np.isin(idx[lo:hi], bad_b)] = False
    part = closer.sum(1).astype(np.int64)
    dead = ~np.isfinite(dt)
    part[dead] = np.where((idx[dead] >= lo) & (idx[dead] < hi), n, 0)
    return part


def partial_b(a, b, lo, hi):
    """This window's share of rank_b (module docstring), int64 [n]."""
    return partial_from(*column_direction(a, b), lo, hi)


def partials(a, b, cuts):
    """partial_b of every window of a cut list, the distance matrix formed once."""
    D, dt, bad_b = column_direction(a, b)
    return [partial_from(D, dt, bad_b, lo, hi) for lo, hi in windows(cuts)]


def nonfinite_case():
    """The NaN / inf case of the paired sweep's test: spread (1027, 64, seed 2) with a[333, 5] = nan and b[700, 17] = inf."""
    a, b = (x.copy() for x in RR.spread_pairs(1027, 64, 2))
    a[333, 5] = np.nan
    b[700, 17] = np.inf
    return a, b


@functools.lru_cache(maxsize=None)
def case(kind, n, d, seed, scale=1.0):
    """(a, b, rank_a, rank_b) of a named data set with the conditions every comparison starts from (rank_refs: min_gap > 1e-12): generated
    and referenced once, shared by the tests, never modified."""
    if kind == "spread":
        a, b = RR.spread_pairs(n, d, seed)
    elif kind == "cluster":
        a, b = RR.cluster_case(n, d, seed, scale)
    elif kind == "midpoint":
        a, b = RR.midpoint_adversary(n, d, seed)
    else:
        assert kind == "nonfinite" and (n, d, seed) == (1027, 64, 2)
        a, b = nonfinite_case()
    rank_a, rank_b, gap = RR.reference_ranks(a, b)
    assert gap > 1e-12, gap
    for x in (a, b, rank_a, rank_b):
        x.setflags(write=False)
    return a, b, rank_a, rank_b
