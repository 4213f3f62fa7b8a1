"""CPU: the numpy restatement of the 8-bit storage (tests/search_q8_refs.py) on every shape tests/test_gpu_search_q8.py uses -- the
stored values are exact products, the scales have 16 significant bits, the quantisation error is within its bound, the reference
rankings are decided by more than any summation order, and the numpy quantiser agrees with a torch restatement."""
import numpy as np
import pytest
import torch

import rank_refs as RR
import search_q8_refs as QR

CASES = QR.SHAPES + [(64, 40003, 9, 11)]


def _raw(d, ng):
    """The fp32 rows a shape's gallery is quantised from."""
    if ng == 40003:
        rng = np.random.default_rng(5)
        g = rng.standard_normal((ng, d))
        return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    return RR.spread_pairs(max(ng, 64), d, QR.SEED + d)[0][:ng]


def _torch_quantize(x):
    x = torch.from_numpy(x)
    m = x.abs().amax(dim=1)
    t = m / torch.tensor(127.0, dtype=torch.float32)
    s = ((t.view(torch.int32) + 0xFF) & ~0xFF).view(torch.float32).clone()
    s[m == 0] = 1.0
    codes = torch.clamp(torch.round(x / s[:, None]), -127, 127).to(torch.int8)
    return codes.numpy(), s.numpy()


@pytest.mark.parametrize("d,ng,nq,depth", CASES)
def test_quantiser_rule_on_every_shape(d, ng, nq, depth):
    x = _raw(d, ng)
    for scale in (1.0, 2.0 ** -130, 2.0 ** 120):
        xs = (x * np.float32(scale)).astype(np.float32)
        codes, s = QR.quantize(xs)
        assert not (s.view(np.uint32) & 0xFF).any() and np.all(np.isfinite(s)) and np.all(s > 0)
        v = QR.dequantize(codes, s)
        exact = s.astype(np.float64)[:, None] * codes.astype(np.float64)
        assert np.array_equal(v.astype(np.float64), exact)                 # the fp32 product IS the fp64 product
        err = np.abs(xs.astype(np.float64) - exact)
        assert np.all(err <= 0.5 * (1 + 2.0 ** -15) * s.astype(np.float64)[:, None])
        assert np.abs(codes.astype(np.int32)).max() <= 127
        tc, ts = _torch_quantize(xs)
        assert np.array_equal(ts.view(np.uint32), s.view(np.uint32)) and np.array_equal(tc, codes)


@pytest.mark.parametrize("d,ng,nq,depth", CASES)
def test_reference_rankings_are_decided(d, ng, nq, depth):
    rows, q = QR.large_case() if ng == 40003 else QR.shape_case(d, ng, nq, depth)
    assert rows.dtype == np.int8 and rows.shape == (ng, d + 16) and not rows[:, d + 4:].any()
    codes, s = QR.unpack_rows(rows)
    assert np.array_equal(QR.pack_rows(codes, s), rows)
    v = QR.stored(rows)
    with np.errstate(all="ignore"):
        exact = s.astype(np.float64)[:, None] * codes.astype(np.float64)
        assert np.array_equal(v, exact.astype(np.float32))                 # the correctly rounded product, whatever the scale's bits
    sixteen = (s.view(np.uint32) & 0xFF) == 0
    assert np.array_equal(v[sixteen].astype(np.float64), exact[sixteen]) and sixteen.sum() >= ng - 1
    ids, d64, gap = QR.reference_search64(rows, q, depth)
    assert gap > 1e-12, gap
    if ng == 40003:
        assert ids[0, 0] == ng - 1
    if 16 <= ng < 40003:                                                   # the planted rows are what their names say
        assert set(np.abs(codes[0]).tolist()) == {127} and np.count_nonzero(codes[1]) == 1 and codes[2].min() == -128
        assert all(np.array_equal(rows[r], rows[6]) for r in (3, 4, 5))
        assert np.abs(codes[7].astype(int) - codes[8].astype(int)).sum() == 1 and s[7] == s[8]
        assert np.array_equal(codes[9], codes[10]) and int(s[9].view(np.uint32)) - int(s[10].view(np.uint32)) == 0x100
        assert s[11] == 2.0 ** 100 and s[14] == 0 and not v[14].any()
        assert s[13] == 2.0 ** -133 and np.all(np.abs(v[13]) < 2.0 ** -126) and np.count_nonzero(v[13]) == np.count_nonzero(codes[13]) > 0
        assert (int(s[15].view(np.uint32)) & 0x7FFFFF) == 0x7FFFFF and not np.array_equal(v[15].astype(np.float64), exact[15])


def test_quantiser_special_rows():
    half = np.float32(2.0 ** -7)                                           # a scale of 2^-7 exactly: m = 127 * 2^-7
    x = np.zeros((6, 64), np.float32)
    x[0, 0] = 127 * half
    x[0, 1:9] = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 126.5], np.float32) * half      # exact half-way quotients: ties to even
    x[2] = np.float32(2.0 ** 120)
    x[3] = np.float32(-(2.0 ** -130))
    x[4, 5], x[5, 63] = np.nan, -np.inf
    codes, s = QR.quantize(x)
    assert s[0] == half and codes[0, :9].tolist() == [127, 0, 2, 2, 4, 0, -2, -2, 126]
    assert s[1] == 1 and not codes[1].any()
    assert set(codes[2].tolist()) == {127} and len(set(codes[3].tolist())) == 1 and -127 <= codes[3, 0] <= -64 and s[3] < 2.0 ** -126
    # (2^-130 / 127 is subnormal: it has 12 bits left, and rounding it up to a multiple of 2^-141 moves the largest code off 127)
    assert np.isnan(s[4]) and np.isnan(s[5]) and not codes[4:].any()
    assert np.isnan(QR.stored(QR.pack_rows(codes, s))[4:]).all()

