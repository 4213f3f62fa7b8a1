"""The reference of the 8-bit gallery storage (vtc_quantize_rows_q8, the *_q8 entries, ops.l2_search* with a torch.int8 gallery,
VideoIndex(storage=torch.int8)), numpy.

Definitions (include/vtc_hip.h).  A q8 row of width d is d + 16 bytes: d signed codes, the row's fp32 scale at byte d, 12 zero bytes.  The
STORED VALUE of component k is the fp32 product fl32(scale * code_k), subnormals kept (`dequantize`; for the quantiser's scales, which
have 16 significant bits, the product is exact).  The search over a q8 gallery is the fp32 search over those stored values, so every
reference here is the fp32 one (search_refs, search_mask_refs, search_grouped_refs) over `stored(rows)` and nothing about the search
is defined a second time.

`quantize` restates the quantiser in fp32 arithmetic: m = max |x_k|; t = fl32(m / 127); s = t rounded UP to 16 significant bits,
bits(s) = (bits(t) + 0xFF) & ~0xFF; s = 1 when m = 0; code_k = clamp(rint(fl32(x_k / s)), -127, 127), rint to nearest even.  A row with a
NaN / inf gets s = NaN and codes of 0.  tests/test_search_q8_refs.py checks it against a torch restatement and asserts its error bound.
"""
import numpy as np

import search_grouped_refs as GR
import search_half_refs as HR
import search_mask_refs as MR
import search_refs as SR

TAIL = 16                                                  # bytes of a q8 row behind its codes


def quantize(x):
    """fp32 [n, d] -> (codes int8 [n, d], scales fp32 [n])."""
    x = np.asarray(x, np.float32)
    bad = ~np.isfinite(x).all(axis=1)
    safe = np.where(bad[:, None], np.float32(0), x)
    m = np.abs(safe).max(axis=1).astype(np.float32)
    t = (m / np.float32(127)).astype(np.float32)
    s = ((t.view(np.uint32) + np.uint32(0xFF)) & np.uint32(0xFFFFFF00)).view(np.float32).copy()
    s[m == 0] = np.float32(1)
    assert np.all(s > 0), "a maximum below 2^-142 has no scale: not a case of the tests"
    codes = np.clip(np.rint((safe / s[:, None]).astype(np.float32)), -127, 127).astype(np.int8)
    s[bad] = np.float32(np.nan)
    return codes, s


def dequantize(codes, scales):
    """The stored values fp32 [n, d]: one fp32 multiply per component."""
    with np.errstate(all="ignore"):
        return (np.asarray(scales, np.float32)[:, None] * np.asarray(codes, np.int8).astype(np.float32)).astype(np.float32)


def pack_rows(codes, scales):
    """(codes int8 [n, d], scales fp32 [n]) -> q8 rows int8 [n, d + 16]."""
    codes = np.asarray(codes, np.int8)
    n, d = codes.shape
    rows = np.zeros((n, d + TAIL), np.int8)
    rows[:, :d] = codes
    rows[:, d:d + 4] = np.ascontiguousarray(scales, np.float32).view(np.int8).reshape(n, 4)
    return rows


def unpack_rows(rows):
    rows = np.asarray(rows)
    assert rows.dtype == np.int8 and rows.ndim == 2, (rows.dtype, rows.shape)
    d = rows.shape[1] - TAIL
    return rows[:, :d].copy(), np.ascontiguousarray(rows[:, d:d + 4]).view(np.float32).reshape(-1).copy()


def stored(rows):
    """q8 rows -> the fp32 gallery they store."""
    return dequantize(*unpack_rows(rows))


def reference_search64(rows, queries, depth, id_base=0):
    return SR.reference_search64(stored(rows), queries, depth, id_base)


def reference_search_masked(rows, queries, live_bool, depth, id_base=0):
    return MR.reference_search_masked(stored(rows), queries, live_bool, depth, id_base)


def reference_search_grouped64(rows, queries, groups, depth, live=None, id_base=0):
    return GR.reference_search_grouped64(stored(rows), queries, groups, depth, live, id_base)


def f32_bits(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def special_rows(codes, scales, seed=0):
    """A copy of the q8 gallery (codes [n >= 16, d], scales [n]) with special rows planted in its first 16:
      row 0       every code +-127;                      row 1       ONE non-zero code;
      row 2       row 12 with one code of -128;          rows 3 .. 5 exact duplicates of row 6 (ties go to the lower row);
      row 7       row 8 with ONE code moved by 1;        row 9       row 10's codes, its scale one step of 2^-16 larger;
      row 11      a scale of 2^100;                      row 13      a scale of 2^-133: every product is subnormal;
      row 14      a scale of 0: a row of zeros;          row 15      a scale with all 24 bits set: the products are ROUNDED."""
    c, s = np.array(codes, np.int8), np.array(scales, np.float32)
    n, d = c.shape
    assert n >= 16
    rng = np.random.default_rng(seed)
    c[0] = np.where(rng.integers(0, 2, d) == 1, 127, -127)
    s[0] = f32_bits((np.float32(1.0 / (127.0 * np.sqrt(d))).view(np.uint32) + 0xFF) & 0xFFFFFF00)
    c[1] = 0
    c[1, int(rng.integers(0, d))] = -93
    c[2], s[2] = c[12], s[12]
    c[2, int(np.argmin(c[12]))] = -128
    c[3:6], s[3:6] = c[6], s[6]
    c[7], s[7] = c[8], s[8]
    k = int(np.argmax(np.abs(c[8].astype(np.int32))))
    c[7, k] -= np.sign(c[8, k])
    c[9] = c[10]
    s[9] = f32_bits(int(s[10].view(np.uint32)) + 0x100)
    s[11] = np.float32(2.0 ** 100)
    s[13] = np.float32(2.0 ** -133)
    s[14] = np.float32(0)
    s[15] = f32_bits((int(s[15].view(np.uint32)) & 0xFF800000) | 0x7FFFFF)
    return c, s


SHAPES = HR.SHAPES                                         # (d, n_gallery, n_queries, depth): the half tests' shapes
SEED = 53


def shape_case(d, ng, nq, depth):
    """(q8 rows int8 [ng, d + 16], queries fp32 [nq, d]) of one of SHAPES: rank_refs.spread_pairs quantised, the special rows planted
    where the gallery has 16 rows or more."""
    import rank_refs as RR
    a, b = RR.spread_pairs(max(ng, nq), d, SEED + d)
    codes, scales = quantize(a[:ng])
    if ng >= 16:
        codes, scales = special_rows(codes, scales, seed=d)
    return pack_rows(codes, scales), np.ascontiguousarray(b[:nq], np.float32)


def large_case():
    """(q8 rows [40 003, 64 + 16], queries fp32 [9, 64]): more rows than a grid has waves x rows of a step, a partial last step; the
    last row is the quantised query 0, its nearest."""
    ng, d = 40003, 64
    rng = np.random.default_rng(5)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    g, q = unit(rng.standard_normal((ng, d))), unit(rng.standard_normal((9, d)))
    g[ng - 1] = q[0]
    return pack_rows(*quantize(g)), q
