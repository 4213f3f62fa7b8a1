"""The reference of the query-time search over a gallery stored as IEEE binary16 (vtc_l2_search_half, ops.l2_search* with a torch.float16
gallery, VideoIndex(storage=torch.float16)), numpy fp64.

Definition (include/vtc_hip.h): the search over the rows AS STORED -- D(q, j) = sum_k ((double)q_k - (double)(float)g_k)^2 with g the
half row.  binary16 -> fp32 is exact (`widen`), so every reference here is the fp32 one (search_refs, search_mask_refs,
search_grouped_refs) over the widened gallery, and nothing about the search itself is defined a second time.

`round_half` is numpy's fp32 -> binary16 conversion (round to nearest, ties to even; overflow to inf from 65520 on), which
tests/test_search_half_refs.py checks against torch's `.to(torch.float16)` -- what VideoIndex.add stores.
"""
import numpy as np

import search_grouped_refs as GR
import search_mask_refs as MR
import search_refs as SR


def widen(x_half):
    """float16 [.., d] -> the same values as float32 (exact: every binary16, subnormals included, is an fp32)."""
    x_half = np.asarray(x_half)
    assert x_half.dtype == np.float16, x_half.dtype
    return x_half.astype(np.float32)


def round_half(x):
    """fp32 -> binary16, round to nearest even (inf from 65520 on)."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16)


def reference_search64(gallery_half, queries, depth, id_base=0):
    """(ids [Q, depth] int64, dists64 [Q, depth], min_gap) over the widened rows."""
    return SR.reference_search64(widen(gallery_half), queries, depth, id_base)


def reference_search_masked(gallery_half, queries, live_bool, depth, id_base=0):
    """(ids, dists32, min_gap): search_mask_refs.reference_search_masked over the widened rows."""
    return MR.reference_search_masked(widen(gallery_half), queries, live_bool, depth, id_base)


def reference_search_grouped64(gallery_half, queries, groups, depth, live=None, id_base=0):
    """(ids, groups, dists64, min_gap): search_grouped_refs.reference_search_grouped64 over the widened rows."""
    return GR.reference_search_grouped64(widen(gallery_half), queries, groups, depth, live, id_base)


def reference_nonfinite_bits(gallery_half, queries, live=None):
    return GR.reference_nonfinite_bits(widen(gallery_half), queries, live)


# Values a half gallery can hold and an fp32 one of unit rows never does: the two ends of the subnormal range, the largest finite
# half, a negative zero -- a flushed subnormal, or a conversion that is not the exact one, changes the fp64 distance.
SUBNORMAL_MIN = np.float16(2.0 ** -24)
SUBNORMAL_MAX = np.nextafter(np.float16(2.0 ** -14), np.float16(0))        # 2^-14 minus one ulp
HALF_MAX = np.float16(65504.0)


def special_rows(base_half, seed=0):
    """A copy of the half gallery `base_half` [n >= 16, d] with special values planted in its first rows:
      rows 0, 1   subnormals (2^-24 and 2^-14 - ulp, both signs) in some columns, among them the first and the last;
      row 2       +-65504 and -0.0;
      rows 3 .. 5 exact duplicates of row 6 (ties go to the lower row);
      row 7       row 8 with ONE component moved by one half ulp -- far below the fp32 resolution of the row's distance."""
    g = np.array(base_half, np.float16)
    n, d = g.shape
    assert n >= 16
    rng = np.random.default_rng(seed)
    cols = np.unique(np.concatenate([[0, d - 1], rng.integers(0, d, 8)]))
    g[0, cols] = SUBNORMAL_MIN
    g[0, cols[::2]] = -SUBNORMAL_MIN
    g[1, cols] = SUBNORMAL_MAX
    g[1, cols[1::2]] = -SUBNORMAL_MAX
    g[2, cols[0]], g[2, cols[1]], g[2, cols[2 % cols.size]] = HALF_MAX, -HALF_MAX, np.float16(-0.0)
    g[3:6] = g[6]
    g[7] = g[8]
    c = int(np.argmax(np.abs(g[8].astype(np.float32))))
    g[7, c] = np.nextafter(g[8, c], np.float16(0))
    # rows 9, 10: equal but for one component, 2^-24 against 2^-23 -- their distances to a query differ by about 1e-8 of themselves,
    # below the fp32 resolution of the distance and only there if the subnormals are converted exactly
    g[9] = g[10]
    g[10, cols[-1]], g[9, cols[-1]] = SUBNORMAL_MIN, np.float16(2.0 ** -23)
    return g


def half_pairs(n, d, seed):
    """(gallery float16 [n, d], queries float32 [n, d]): rank_refs.spread_pairs with the gallery rounded to binary16."""
    import rank_refs as RR
    a, b = RR.spread_pairs(n, d, seed)
    return round_half(a), b


# The shapes tests/test_gpu_search_half.py runs (d, n_gallery, n_queries, depth); tests/test_search_half_refs.py asserts min_gap > 1e-12
# on every one.  d: 16 active lanes, a partial last 256-column piece, the common width, the limit.  n_queries: every tile shape, a
# ragged tile, several tiles.  depth: 1, 11, 64 and the whole gallery.
SHAPES = [
    (64, 1, 1, 1), (64, 3, 2, 3), (64, 5, 3, 5), (64, 33, 4, 33), (64, 257, 5, 11), (64, 257, 8, 64), (64, 257, 9, 1), (64, 257, 64, 11),
    (192, 33, 1, 11), (192, 257, 9, 64), (512, 257, 1, 11), (512, 257, 2, 64), (512, 33, 4, 1), (2048, 33, 3, 33), (2048, 257, 8, 11),
    (2048, 5, 1, 5),
]
SEED = 31


def large_case():
    """(gallery float16 [40 003, 64], queries float32 [9, 64]): more rows than a grid has waves x rows of a step (1024 workgroups x 4
    waves x 8 rows at the most), so every wave takes several steps and the last step is partial; its last row is query 0's nearest."""
    ng, d = 40003, 64
    rng = np.random.default_rng(5)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    g, q = round_half(unit(rng.standard_normal((ng, d)))), unit(rng.standard_normal((9, d)))
    g[ng - 1] = round_half(q[0])
    return g, q


def shape_case(d, ng, nq, depth):
    """The gallery (special rows planted where it has 16 rows or more) and the queries of one of SHAPES."""
    g, q = half_pairs(max(ng, nq), d, SEED + d)
    g = special_rows(g[:ng], seed=d) if ng >= 16 else g[:ng]
    return g, q[:nq]
