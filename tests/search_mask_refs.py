"""The reference of the masked query-time search (vtc_l2_search_masked, ops.l2_search(live=...), VideoIndex.remove / subset), numpy.

Definition (include/vtc_hip.h): the result is that of the unmasked search over the gallery COMPACTED to its live rows in order, every
returned position mapped back to the row's original index -- `reference_search_masked` is exactly that sentence on top of
search_refs.reference_search.  A dead row influences nothing: not the ids, not the distances, not the non-finite word.

The word layout is defined by `pack_words`: bit (j & 31) of uint32 word (j >> 5) is row j, bits past the last row are 0.
"""
import numpy as np

import search_refs as SR


def reference_search_masked(gallery, queries, live_bool, depth, id_base=0):
    """(ids [Q, depth] int64, dists32 [Q, depth] fp32, min_gap): compaction + search_refs.reference_search + the map back."""
    live_bool = np.asarray(live_bool, bool)
    idx = np.flatnonzero(live_bool)
    nq = np.asarray(queries).shape[0]
    if idx.size == 0:
        return np.full((nq, depth), -1, np.int64), np.full((nq, depth), np.inf, np.float32), float("inf")
    ids, d32, gap = SR.reference_search(np.asarray(gallery)[idx], queries, depth, 0)
    return np.where(ids >= 0, id_base + idx[np.maximum(ids, 0)], -1).astype(np.int64), d32, gap


def reference_search_masked_by_inf(gallery, queries, live_bool, depth, id_base=0):
    """The second formulation: the distances of the dead rows set to +inf in the full distance matrix."""
    D = SR.distances64(gallery, queries)
    D[:, ~np.asarray(live_bool, bool)] = np.inf
    ids, d64, gap = SR.sorted_lists(D, depth, id_base)
    return ids, d64.astype(np.float32), gap


def reference_nonfinite_bits(gallery, queries, live_bool):
    """The non-finite word: 1 if a LIVE gallery row holds a NaN / inf, 2 if a query does."""
    g = np.asarray(gallery)[np.asarray(live_bool, bool)]
    return int(not np.isfinite(g).all()) | 2 * int(not np.isfinite(np.asarray(queries)).all())


def pack_words(flags):
    """bool / uint8 [n] -> uint32 [ceil(n / 32)]: np.packbits, little bit order, viewed as little-endian words."""
    flags = np.asarray(flags) != 0
    n_words = (flags.size + 31) // 32
    by = np.zeros(n_words * 4, np.uint8)
    packed = np.packbits(flags, bitorder="little")
    by[:packed.size] = packed
    return by.view("<u4").astype(np.uint32)


NG = (1, 2, 31, 32, 33, 63, 64, 65, 257, 1027)      # word, step and wave boundaries
NQ = (1, 2, 4, 8, 9, 64)                            # the four tile shapes, two tiles, eight tiles


def edge_cases():
    """Half of the NG x NQ grid, every value of both axes, the depths 1, min(11, ng), min(64, ng) in rotation (as tests/test_gpu_search.py
    thins its own grid)."""
    cases = []
    for i, ng in enumerate(NG):
        for j, nq in enumerate(NQ):
            if (i - j) % 2 == 0:
                cases.append((ng, nq, (1, min(11, ng), min(64, ng))[(i + j) % 3]))
    return cases


MASK_KINDS = ("all", "none", "last", "row31", "row32", "alt_bits", "alt_words", "random_0.5", "random_0.05", "first_half_dead")


def make_mask(kind, n, seed=0):
    """The mask kinds of the edge grid, bool [n].  A kind that names a row the gallery does not have (row 31 of 2 rows) falls on the last row."""
    j = np.arange(n)
    if kind == "all":
        return np.ones(n, bool)
    if kind == "none":
        return np.zeros(n, bool)
    if kind in ("last", "row31", "row32"):
        m = np.zeros(n, bool)
        m[min({"last": n - 1, "row31": 31, "row32": 32}[kind], n - 1)] = True
        return m
    if kind == "alt_bits":
        return j % 2 == 1
    if kind == "alt_words":
        return (j // 32) % 2 == 0
    if kind.startswith("random_"):
        return np.random.default_rng(1000 + seed).random(n) < float(kind.split("_")[1])
    if kind == "first_half_dead":
        return j >= n // 2
    raise ValueError(kind)
