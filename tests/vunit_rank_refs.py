"""The reference of the video-unit video -> text ranks (vtc_l2_rank_grouped_vunit, RecallAtK.grouped_ranks(video_to_text="video")), numpy
fp64 on grouped_rank_refs.distances, straight from the definition (include/vtc_hip.h):

    E(u, v)   = min { D(c, v) : off[u] <= c < off[u + 1], D(c, v) finite }        (+inf if there is none)
    rank_v[v] = #{ u in [0, n), u != v : (E(u, v), u) < (E(v, v), v) }             if E(v, v) is finite
              = n                                                                  otherwise (no finite own caption, an empty group too)

E(u, v) is an entry of v's column of D, and E(v, v) the column direction's target distance, so the `min_gap` of
grouped_rank_refs.reference_grouped_ranks covers this direction too.
"""
import numpy as np

import grouped_rank_refs as GR


def group_minima(D, off):
    """E [n, n] from D [m, n]: E[u, v] = the smallest finite D(c, v) over the captions of group u, +inf if there is none."""
    off = np.asarray(off, np.int64)
    n = off.size - 1
    E = np.full((n, D.shape[1]), np.inf, np.float64)
    F = np.where(np.isfinite(D), D, np.inf)
    for u in range(n):
        if off[u + 1] > off[u]:
            E[u] = F[off[u]:off[u + 1]].min(axis=0)
    return E


def reference_vunit_ranks(a, b, off):
    """rank_v [n] int64 -- see the module docstring."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    off = np.asarray(off, np.int64)
    n, m = a.shape[0], b.shape[0]
    assert off.shape == (n + 1,) and off[0] == 0 and off[-1] == m and (np.diff(off) >= 0).all()
    E = group_minima(GR.distances(a, b), off)
    rank_v = np.empty(n, np.int64)
    us = np.arange(n)
    for v in range(n):
        t = E[v, v]
        if not np.isfinite(t):
            rank_v[v] = n
            continue
        col = E[:, v]
        closer = np.isfinite(col) & ((col < t) | ((col == t) & (us < v)))
        closer[v] = False
        rank_v[v] = closer.sum()
    return rank_v


def table_from_ranks(rank_a, rank_v, split="full-test", dataset_name="MSRVTT"):
    """compute_multi_caption_table(video_to_text="video")'s frame from reference ranks, attrs included."""
    df = GR.table_from_ranks(rank_a, rank_v, split, dataset_name)
    df.attrs["video_to_text"] = "video"
    return df
