"""The data sets of the video-unit rank tests (tests/test_vunit_rank_refs.py on the CPU, tests/test_gpu_vunit_rank.py on the GPU), each
generated and referenced ONCE per process and never modified: (a, b, off) with the fp64 references rank_a, rank_b
(grouped_rank_refs.reference_grouped_ranks, whose min_gap must exceed 1e-12: E(u, v) is an entry of v's column, so that gap covers the
video-unit direction) and rank_v (vunit_rank_refs.reference_vunit_ranks).  Data: grouped_spread(counts, d, 100 + n) unless stated."""
import functools

import numpy as np

import grouped_rank_refs as GR
import rank_refs as RR
import vunit_rank_refs as VR

# (kind, n, d, rows_per_block): the cases of test_edge_sizes and test_bulk_equals_the_fp64_reference of tests/test_gpu_grouped_rank.py
EDGE = [((1,), 1, 64, 256), ((5,), 1, 64, 256), ((1, 3), 2, 64, 256), ("1-4", 63, 64, 256), ("1-4", 64, 64, 256), ("1-4", 65, 64, 256),
        ("3x85+2", 86, 64, 256)]
BULK = [("1-4", 257, 64, 0), (20, 256, 64, 256), ("1-8", 300, 512, 0), ("1-3", 700, 128, 0), (20, 500, 512, 0)]
IDENTITY = [(65, 64), (700, 128), (1027, 64)]


def counts_of(kind, n):
    """`kind`: an int c (c captions for every video), "lo-hi" (ragged, uniform in [lo, hi], drawn with seed 100 + n), "3x85+2", or the
    counts themselves as a tuple."""
    if isinstance(kind, int):
        return np.full(n, kind, np.int64)
    if isinstance(kind, tuple):
        return np.array(kind, np.int64)
    if kind == "3x85+2":
        return np.array([3] * 85 + [2], np.int64)
    lo, hi = (int(x) for x in kind.split("-"))
    return GR.ragged_counts(n, lo, hi, 100 + n)


def _referenced(a, b, off):
    rank_a, rank_b, gap = GR.reference_grouped_ranks(a, b, off)
    assert gap > 1e-12, gap
    rank_v = VR.reference_vunit_ranks(a, b, off)
    out = (a, b, np.asarray(off, np.int64), rank_a, rank_b, rank_v)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(kind, n, d):
    """(a, b, off, rank_a, rank_b, rank_v) of a named data set."""
    return _referenced(*GR.grouped_spread(counts_of(kind, n), d, 100 + n))


@functools.lru_cache(maxsize=None)
def big_group_case():
    """64 videos at d = 64, ragged 1..4 captions, but video 10 has 600 and video 37 has 300: with 256-row blocks one group spans three
    blocks and another two."""
    counts = GR.ragged_counts(64, 1, 4, 164)
    counts[10], counts[37] = 600, 300
    return _referenced(*GR.grouped_spread(counts, 64, 164))


@functools.lru_cache(maxsize=None)
def identity_case(n, d):
    """(a, b, rank_a, rank_b) of n paired rows (rank_refs.spread_pairs(n, d, 10 + n)) with the PAIRED reference."""
    a, b = RR.spread_pairs(n, d, 10 + n)
    rank_a, rank_b, gap = RR.reference_ranks(a, b)
    assert gap > 1e-12, gap
    for x in (a, b, rank_a, rank_b):
        x.setflags(write=False)
    return a, b, rank_a, rank_b


def assert_not_degenerate(rank_v, rank_b, n):
    """For n >= 63: max rank_v > n / 2, 0.2 < R@1 < 0.8, and the two conventions differ for at least n / 5 videos."""
    if n < 63:
        return
    r1, differ = float((rank_v < 1).mean()), int((rank_v != rank_b).sum())
    print(f"n={n}: max rank_v {int(rank_v.max())}, videos with rank_v != rank_b {differ}, R@1 {r1:.2f}")
    assert rank_v.max() > n / 2 and 0.2 < r1 < 0.8 and differ >= n / 5, (int(rank_v.max()), r1, differ)


def assert_properties(rank_b, rank_v):
    """What the definition implies: rank_v <= rank_b, and rank 0 in one convention exactly when in the other."""
    assert (rank_v <= rank_b).all()
    assert np.array_equal(rank_v == 0, rank_b == 0)


@functools.lru_cache(maxsize=None)
def ties_case(scale):
    """The planted data of tests/test_gpu_grouped_rank.py::_ties_case (300 videos at d = 128, ragged 1..3 captions; video 10 with 40
    bit-equal captions; videos 50..89 sharing one caption; videos 100..139 identical; video 150 with ONE caption 0.05 from it and the first
    captions of videos 160..259 within 1e-7 of that caption), built the same way, with three more plants:
      1  the SECOND caption of every cluster video 160..259 that has one is another copy of video 150's caption + 1e-7 noise
                                                          -> two captions of one group in reach of video 150's target: the group counts once
      2  the THIRD caption of those with three is 0.01 from video 150
                                                          -> a certainly closer and an in-reach caption in one group: counted, not pooled
      3  video 280 = unit(a[10] + 0.3 noise), its first caption unit(a[280] + 0.5 noise)
                                                          -> video 10's 40 captions all precede it: rank_b[280] = 40, rank_v[280] = 1
    Returns (a, b, off, rank_a, rank_b, rank_v, info); info has video 150's target distance and its distances to the planted captions."""
    n, d = 300, 128
    rng = np.random.default_rng(77)
    counts = GR.ragged_counts(n, 1, 3, 100 + n)
    counts[10], counts[150] = 40, 1
    a, b, off = GR.grouped_spread(counts, d, 100 + n)
    a, b = a.astype(np.float64), b.astype(np.float64)
    noise = lambda k: RR.unit(rng.standard_normal((k, d)))                                     # noqa: E731
    b[off[10]:off[11]] = RR.unit(a[10] + 0.01 * noise(1))
    a[51:90] = a[50] + 1e-3 * noise(39)
    b[off[50:90]] = a[50]
    a[100:140] = a[100]
    b[off[100:140]] = RR.unit(a[100] + 0.01 * noise(40))
    b[off[150]] = RR.unit(a[150] + 0.05 * noise(1))
    cluster = np.arange(160, 260)
    two, three = cluster[counts[cluster] >= 2], cluster[counts[cluster] >= 3]
    b[off[three] + 2] = RR.unit(a[150] + 0.01 * noise(three.size))                             # plant 2
    a[280] = RR.unit(a[10] + 0.3 * noise(1))[0]                                                # plant 3
    b[off[280]] = RR.unit(a[280] + 0.5 * noise(1))[0]
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    b32[off[160:260]] = b32[off[150]] + (1e-7 * rng.standard_normal((100, d))).astype(np.float32)
    b32[off[two] + 1] = b32[off[150]] + (1e-7 * rng.standard_normal((two.size, d))).astype(np.float32)      # plant 1
    a32, b32 = (a32 * np.float32(scale)).astype(np.float32), (b32 * np.float32(scale)).astype(np.float32)
    a32, b32, off, rank_a, rank_b, rank_v = _referenced(a32, b32, off)
    info = {"two": two, "three": three,
            "dt150": GR.distances(a32[150:151], b32[off[150]:off[150] + 1])[0, 0],
            "D_first": GR.distances(a32[150:151], b32[off[160:260]])[:, 0],
            "D_second": GR.distances(a32[150:151], b32[off[two] + 1])[:, 0],
            "D_third": GR.distances(a32[150:151], b32[off[three] + 2])[:, 0]}
    return a32, b32, off, rank_a, rank_b, rank_v, info


def assert_ties_case(scale, kappa):
    """The ranks the construction of ties_case dictates, from the references alone.  `kappa`: the rank sweep's at d = 128."""
    a, b, off, rank_a, rank_b, rank_v, info = ties_case(scale)
    two, three, dt = info["two"], info["three"], info["dt150"]
    assert two.size == 74 and three.size == 36
    assert rank_v[50:90].tolist() == list(range(40))
    assert rank_v[10] == 0 and rank_b[10] == 0
    # video 150: the distinct groups with a caption exactly closer than its target
    closer = np.zeros(300, bool)
    closer[np.arange(160, 260)[info["D_first"] < dt]] = True
    closer[two[info["D_second"] < dt]] = True
    closer[three[info["D_third"] < dt]] = True
    D150 = GR.distances(a[150:151], b)[:, 0]
    g = np.repeat(np.arange(300), np.diff(off))
    assert set(g[D150 < dt].tolist()) == set(np.flatnonzero(closer).tolist())                   # nobody else is closer
    assert (info["D_first"] != dt).all() and (info["D_second"] != dt).all() and (info["D_third"] < dt).all()
    n_closer = int(closer.sum())
    print(f"scale {scale}: rank_v[150] {int(rank_v[150])}, rank_b[150] {int(rank_b[150])}, groups closer {n_closer}")
    assert rank_v[150] == n_closer == 83 and rank_b[150] in (124, 125)
    assert rank_v[150] < rank_b[150]
    both = (info["D_first"][two - 160] < dt) & (info["D_second"] < dt)
    assert both.sum() >= 10                                                                   # both planted captions closer: ONE group
    assert rank_v[280] == 1 and rank_b[280] == 40
    eps = kappa * (float((a[150].astype(np.float64) ** 2).sum()) + float((b.astype(np.float64) ** 2).sum(1).max()))
    assert (np.abs(info["D_first"] - dt) < 0.5 * eps).all() and (np.abs(info["D_second"] - dt) < 0.5 * eps).all()      # all in reach
    return a, b, off, rank_a, rank_b, rank_v


@functools.lru_cache(maxsize=None)
def nonfinite_cases():
    """The three constructions of test_nonfinite_caption_video_and_empty_group on the ("1-4", 65, 64) data:
    [(name, a, b, off, rank_a, rank_b, rank_v, bits, index)] with index = p (the 3-caption video whose second caption holds a NaN),
    q (the NaN video row), p (the emptied group)."""
    n, d = 65, 64
    a0, b0, off0 = case("1-4", n, d)[:3]
    counts = np.diff(off0)
    p, q = int(np.flatnonzero(counts == 3)[0]), int(np.flatnonzero(counts == 2)[0])
    b = b0.copy()
    b[int(off0[p]) + 1, 5] = np.nan
    a = a0.copy()
    a[q, 3] = np.nan
    keep = np.ones(b0.shape[0], bool)
    keep[off0[p]:off0[p + 1]] = False
    counts2 = counts.copy()
    counts2[p] = 0
    return [("nan_caption",) + _referenced(a0.copy(), b, off0.copy()) + (2, p),
            ("nan_video",) + _referenced(a, b0.copy(), off0.copy()) + (1, q),
            ("empty_group",) + _referenced(a0.copy(), b0[keep], GR.counts_to_offsets(counts2)) + (0, p)]
