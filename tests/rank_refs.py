"""The reference of the full-rank sweep (vtc_l2_rank_bidir, RecallAtK.ranks), numpy fp64, and the data its tests run on.

Semantics (include/vtc_hip.h): for n paired rows a_i <-> b_i

    rank_a[i] = #{ j : (|b_i - a_j|^2, j) < (|b_i - a_i|^2, i) }      gallery a, query b_i
    rank_b[i] = #{ j : (|a_i - b_j|^2, j) < (|a_i - b_i|^2, i) }      gallery b, query a_i

on the fp64 distances sum_k (q_k - g_k)^2 of the fp32 inputs, pairs compared lexicographically.  A gallery row with a non-finite distance
is never closer; a pair whose own distance is not finite has rank n in both directions (the library's rule: such a pair is a miss at every
k, as in vtc_l2_recall_bidir -- a literal evaluation would compare everything against NaN and read rank 0).

The bulk of the matrix comes from |q|^2 + |g|^2 - 2 q.g in fp64 (one matrix product); that form cancels, so every entry within
1e-9 (|q|^2 + |g|^2) of its query's target distance -- and the target itself -- is recomputed as sum (q - g)^2, which is exact to 1e-16
relative (fp32 differences are exact in fp64).  The norms form alone gets full ranks wrong inside dense clusters.  `min_gap` is the smallest
relative gap |d_ij - d_ii| / d_ii over the entries that are not bit-equal to their target's distance: the tests require it to exceed
1e-12, so that no summation order can decide a rank; bit-equal entries (exact duplicates) go to the lower index by definition.
"""
import numpy as np


def unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def spread_pairs(n, d, seed):
    """Pairs whose noise scale is log-uniform per row in [0.5, 60]: ranks from 0 to nearly n (tests/test_gpu_sweep.py's planted() leaves
    every rank at 0 at d = 512)."""
    rng = np.random.default_rng(seed)
    a = unit(rng.standard_normal((n, d)))
    s = np.exp(rng.uniform(np.log(0.5), np.log(60.0), (n, 1)))
    b = unit(a + s * unit(rng.standard_normal((n, d))))
    return a.astype(np.float32), b.astype(np.float32)


def unrelated_pairs(n, d, seed):
    """b independent of a: ranks roughly uniform."""
    rng = np.random.default_rng(seed)
    return unit(rng.standard_normal((n, d))).astype(np.float32), unit(rng.standard_normal((n, d))).astype(np.float32)


def cluster_case(n=1500, d=512, seed=5, scale=1.0):
    """Exact duplicates in both sets, a dense near-duplicate cluster around targets, optionally un-normalised rows (the construction of
    tests/test_gpu_sweep.py::test_recall_bidir_rank_path_ties_duplicates_scales_and_the_adversarial_case at n = 1500, on the spread data)."""
    rng = np.random.default_rng(seed)
    a, b = spread_pairs(n, d, seed + 72)
    a[100:140] = a[99]                       # 40 exact duplicates of gallery row 99 ...
    b[100:140] = b[99]                       # ... and of query 99
    a[1000:1100] = a[999] + (1e-7 * rng.standard_normal((100, d))).astype(np.float32)
    b[999:1100] = a[999]
    return (a * np.float32(scale)).astype(np.float32), (b * np.float32(scale)).astype(np.float32)


def midpoint_adversary(n=1024, d=512, seed=5):
    """oracle.sweep_planes.midpoint_case in n rows (as tests/test_gpu_sweep.py embeds it): pair 0 is the adversarial query -- rows whose
    bf16 roundings are the worst case -- against its true nearest neighbour, gallery row 0.  Pairs 1 .. 799 are b_i == a_i (rank 0); the
    tail pairs are their gallery row plus noise of a log-uniform scale, so that the case has ranks up to the gallery's size."""
    from oracle import sweep_planes as SP
    rng = np.random.default_rng(seed)
    g, q = SP.midpoint_case(d=d, depth=11)
    ga = g[:n].copy()
    qb = ga.copy()
    qb[0] = q[0]
    tail = np.arange(800, n)
    s = np.exp(rng.uniform(np.log(1.0), np.log(40.0), (tail.size, 1)))
    qb[tail] = (ga[tail] + s * rng.standard_normal((tail.size, d))).astype(np.float32)
    return ga, qb


def _sq(x):
    return np.einsum("ij,ij->i", x, x)


def _one_direction(q, g, never):
    """ranks of the targets g_i for the queries q_i; `never`: gallery rows that are never closer."""
    n = q.shape[0]
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    with np.errstate(all="ignore"):
        dt = _sq(q64 - g64)
        qn, gn = _sq(q64), _sq(g64)
        D = qn[:, None] + gn[None, :] - 2.0 * (q64 @ g64.T)
        near = np.abs(D - dt[:, None]) <= 1e-9 * (qn[:, None] + gn[None, :])
        near[np.arange(n), np.arange(n)] = True
        ii, jj = np.nonzero(near)
        for s in range(0, ii.size, 1 << 16):              # exact form, in chunks
            i, j = ii[s:s + (1 << 16)], jj[s:s + (1 << 16)]
            D[i, j] = _sq(q64[i] - g64[j])
        idx = np.arange(n)
        closer = (D < dt[:, None]) | ((D == dt[:, None]) & (idx[None, :] < idx[:, None]))
        closer[:, never] = False
        closer[idx, idx] = False
        ranks = closer.sum(1).astype(np.int64)
        finite = np.isfinite(dt)
        ranks[~finite] = n
        ne = (D != dt[:, None]) & finite[:, None] & np.isfinite(D)
        ne[:, never] = False
        rel = np.where(ne, np.abs(D - dt[:, None]) / np.where(dt[:, None] > 0, dt[:, None], np.nan), np.inf)
        rel = np.where(np.isnan(rel), np.inf, rel)        # a zero target distance: everything not bit-equal is infinitely far, relatively
        gap = float(rel.min()) if n > 1 else np.inf
    return ranks, gap, D, dt


def reference_ranks(a, b):
    """(rank_a, rank_b, min_gap) -- see the module docstring."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    bad_a = np.flatnonzero(~np.isfinite(a).all(1))
    bad_b = np.flatnonzero(~np.isfinite(b).all(1))
    rank_a, gap_a, _, _ = _one_direction(b, a, bad_a)
    rank_b, gap_b, _, _ = _one_direction(a, b, bad_b)
    return rank_a, rank_b, min(gap_a, gap_b)


def in_reach_total(a, b, kappa):
    """Entries (targets excluded) whose exact distance lies within eps = kappa (|q|^2 + max|g|^2) of their query's target distance, both
    directions summed: what a sweep that sees the distances to within eps has to settle in fp64, to within the entries at the window's edge."""
    total = 0
    for q, g in ((b, a), (a, b)):
        _, _, D, dt = _one_direction(q, g, np.array([], np.int64))
        eps = kappa * (_sq(q.astype(np.float64)) + _sq(g.astype(np.float64)).max())
        m = np.abs(D - dt[:, None]) <= eps[:, None]
        m[np.arange(len(dt)), np.arange(len(dt))] = False
        total += int(m.sum())
    return total


def assert_not_degenerate(rank, n):
    """The conditions every comparison starts from: ranks reach past n / 2 and R@1 is neither 0 nor 1."""
    r1 = float((rank < 1).mean())
    assert rank.max() > n / 2 and 0.2 < r1 < 0.8, (int(rank.max()), r1)
