"""The reference of the grouped rank sweep (vtc_l2_rank_grouped, RecallAtK.grouped_ranks), numpy fp64, and the data its tests run on.

Semantics (include/vtc_hip.h): a [n, d] videos, b [m, d] captions, off [n + 1]; caption c belongs to video g(c), the v with
off[v] <= c < off[v + 1]; D(c, j) = sum_k (b_c[k] - a_j[k])^2 in fp64 of the fp32 inputs; pairs compare lexicographically.

    rank_a[c] = #{ j in [0, n) : (D(c, j), j) < (D(c, g(c)), g(c)) }                                     text -> video
    rank_b[v] = #{ c in [0, m) : (D(c, v), c) < (D(c*, v), c*) },  c* = the own caption with the smallest finite (D(c, v), c)   video -> text

An entry with a non-finite distance is never closer; a caption whose own distance is not finite has rank_a = n and is no candidate for
c*; a video without a finite own caption (an empty group too) has rank_b = m.

The distances are formed as sum (q - g)^2 DIRECTLY, in row chunks (fp32 differences are exact in fp64; the norms form
|q|^2 + |g|^2 - 2 q.g cancels and gets ranks wrong inside dense clusters).  `min_gap` is, as in rank_refs.py, the smallest relative gap
|D - d_t| / d_t over the entries that are not bit-equal to their owner's target distance, both directions: the tests require it to exceed
1e-12, so that no summation order can decide a rank; bit-equal entries go to the lower index by definition.
"""
import numpy as np

from rank_refs import unit


def counts_to_offsets(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


def ragged_counts(n, lo, hi, seed):
    """n caption counts, uniform in [lo, hi]."""
    return np.random.default_rng(seed).integers(lo, hi + 1, n).astype(np.int64)


def grouped_spread(counts, d, seed):
    """(a [n, d], b [m, d], off [n + 1]): unit videos; every caption is its video plus noise of the VIDEO's scale (log-uniform in
    [0.5, 60]) times a per-caption jitter (log-uniform in [0.7, 1.4]), normalised.  The scale is per video so that some videos have no good
    caption at all: with independent per-caption scales the best of 20 captions is always good and the video -> text ranks never leave the
    top.  The draws come in the order videos, caption noise directions, scales, jitters: with it every case of
    tests/test_gpu_grouped_rank.py meets its own non-degeneracy conditions at seed 100 + n (drawing the scales first leaves the
    85 x 3 + 2 case with max rank_b = 0.45 m, under its bar of m / 2)."""
    counts = np.asarray(counts, np.int64)
    n, m = counts.size, int(counts.sum())
    rng = np.random.default_rng(seed)
    a = unit(rng.standard_normal((n, d)))
    u = unit(rng.standard_normal((m, d)))
    s = np.exp(rng.uniform(np.log(0.5), np.log(60.0), (n, 1)))
    j = np.exp(rng.uniform(np.log(0.7), np.log(1.4), (m, 1)))
    g = np.repeat(np.arange(n), counts)
    b = unit(a[g] + s[g] * j * u)
    return a.astype(np.float32), b.astype(np.float32), counts_to_offsets(counts)


def distances(a, b):
    """D [m, n] fp64 = sum_k (b_c[k] - a_j[k])^2, formed directly, a chunk of caption rows (at most 2^22 differences) at a time."""
    a64, b64 = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    D = np.empty((b64.shape[0], a64.shape[0]), np.float64)
    chunk = max(1, (1 << 22) // max(1, a64.shape[0] * a64.shape[1]))

    def block(r):
        with np.errstate(all="ignore"):
            diff = b64[r:r + chunk, None, :] - a64[None, :, :]
            D[r:r + chunk] = np.einsum("ijk,ijk->ij", diff, diff)
    starts = range(0, b64.shape[0], chunk)
    if len(starts) < 8:
        for r in starts:
            block(r)
    else:                                                      # (numpy releases the GIL: the 10 000 x 500 x 512 case in 2 s instead of 9)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=8) as pool:
            list(pool.map(block, starts))
    return D


def _gap(D_own, dt):
    """smallest |D - d_t| / d_t over one owner's entries that are finite and not bit-equal to d_t (inf if there are none)."""
    x = D_own[np.isfinite(D_own) & (D_own != dt)]
    if x.size == 0:
        return np.inf
    if dt == 0:
        return np.inf
    return float(np.min(np.abs(x - dt)) / dt)


def reference_grouped_ranks(a, b, off):
    """(rank_a [m], rank_b [n], min_gap) -- see the module docstring."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    off = np.asarray(off, np.int64)
    n, m = a.shape[0], b.shape[0]
    assert off.shape == (n + 1,) and off[0] == 0 and off[-1] == m and (np.diff(off) >= 0).all()
    g = np.repeat(np.arange(n), np.diff(off))
    D = distances(a, b)
    rank_a, rank_b = np.empty(m, np.int64), np.empty(n, np.int64)
    gap = np.inf
    with np.errstate(all="ignore"):
        own = D[np.arange(m), g]                               # every caption's distance to its own video
        cols = np.arange(n)
        for c in range(m):
            dt, t = own[c], g[c]
            if not np.isfinite(dt):
                rank_a[c] = n
                continue
            row = D[c]
            closer = np.isfinite(row) & ((row < dt) | ((row == dt) & (cols < t)))
            closer[t] = False
            rank_a[c] = closer.sum()
            gap = min(gap, _gap(np.delete(row, t), dt))
        rows = np.arange(m)
        for v in range(n):
            mine = np.arange(off[v], off[v + 1])
            mine = mine[np.isfinite(own[mine])]
            if mine.size == 0:
                rank_b[v] = m
                continue
            cs = mine[np.lexsort((mine, own[mine]))[0]]        # smallest (D, c)
            dt = own[cs]
            col = D[:, v]
            closer = np.isfinite(col) & ((col < dt) | ((col == dt) & (rows < cs)))
            closer[cs] = False
            rank_b[v] = closer.sum()
            gap = min(gap, _gap(np.delete(col, cs), dt))
    return rank_a, rank_b, gap


def pad_captions(b, off):
    """The reference's padded caption tensor (evaluation/retrieval_evaluation.py:238-260): [n, max count, d], -inf rows after a video's
    own captions."""
    off = np.asarray(off, np.int64)
    n, cmax = off.size - 1, int(np.diff(off).max())
    out = np.full((n, cmax, b.shape[1]), -np.inf, np.float32)
    for v in range(n):
        out[v, :off[v + 1] - off[v]] = b[off[v]:off[v + 1]]
    return out


def table_from_ranks(rank_a, rank_b, split="full-test", dataset_name="MSRVTT"):
    """compute_multi_caption_table's frame from reference ranks: "Text to Video" from rank_a, "Video to Text" from rank_b."""
    import pandas as pd

    def column(r):
        r1 = np.asarray(r, np.int64).astype(np.float64) + 1.0
        return [float(np.count_nonzero(np.asarray(r) < k)) / len(r) * 100.0 for k in (1, 5, 10)] + [
            float(np.median(r1)), float(r1.mean()), float((1.0 / r1).mean())]
    return pd.DataFrame({f"{dataset_name} {split} split Video to Text": column(rank_b),
                         f"{dataset_name} {split} split Text to Video": column(rank_a)},
                        index=["R@1", "R@5", "R@10", "MedR", "MeanR", "MRR"])
