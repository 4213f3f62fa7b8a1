"""The wrapper-level fp32 ops of norm.hip (include/vtc_hip.h, "small fp32 ops of the wrappers") -- vtc_normalize_rows,
vtc_normalize_rows2, vtc_mean_groups, vtc_mean_head_groups, vtc_segment_mean, vtc_nonfinite_flag, vtc_nonfinite_flag2 -- and
vtc_layernorm at the widths nobody runs, each directly through the C ABI against a float64 reference: feature widths off the
64-lane grid, row counts off the 4-rows-per-workgroup grid, ragged segments of length 1, the grid-stride loop of the flag kernels.

References, case lists and the row-scaled error measure e = max |got - ref64| / scale: tests/primitive_refs.py.  The CPU half (no
`gpu` mark) calibrates the tolerances over the SAME case lists (TOL = 4 x the worst e of the float32 torch evaluation) and proves
that each deliberately wrong reference exceeds them.

Finding of these tests on the commit that introduced them (fixed with it): vtc_normalize_rows2 raised its flag from the squared norm
of the INPUT row being non-finite, so an all-zero row (a missing clip on the cached-feature path) -- squared norm 0, output 0/0 =
NaN as in the reference -- left the wrappers' fused watchdog silent (flag 0, output NaN) where the unfused one,
vtc_nonfinite_flag2 on the output, raises; the same for a row whose squares all underflow (output inf).  The kernel now also
flags a squared norm of zero.
"""
import pytest
import torch

import primitive_refs as PR

torch.set_grad_enabled(False)
gpu = pytest.mark.gpu

FLT_MAX = float(torch.finfo(torch.float32).max)
SUBNORMAL = 1e-41

# op -> output -> tolerance = 4 x (worst e of torch float32, on one CPU thread, over the op's cases: the figure in the comment), rounded up
TOL = {
    "normalize_rows": {"y": 7.2e-7},         # 1.779e-07
    "mean_groups": {"out": 8.1e-7},          # 2.011e-07
    "mean_head_groups": {"out": 9.0e-7},     # 2.229e-07
    "segment_mean": {"out": 9.5e-7},         # 2.364e-07
    "layernorm": {"y": 7.6e-7},              # 1.894e-07
}


def _cases(name):
    return pytest.mark.parametrize("case", PR.OPS[name].cases, ids=lambda c: "-".join(str(v) for v in c))


def _ops():
    from vtc_amd import ops
    return ops


# ==== CPU half ===========================================================================================================================
@pytest.mark.parametrize("name", PR.SMALL_OPS)
def test_calibration_float32_stays_within_a_quarter_of_the_tolerance(name):
    worst = PR.OPS[name].calibrate()
    print(f"[calibration] {name}: " + "  ".join(f"{o} {v:.3e}" for o, v in worst.items()))
    for o, v in worst.items():
        assert v <= TOL[name][o] / 4, (name, o, v, TOL[name][o])


@pytest.mark.parametrize("name,mut", [(n, m) for n in PR.SMALL_OPS for m in PR.OPS[n].muts])
def test_wrong_reference_exceeds_the_tolerance(name, mut):
    worst = PR.OPS[name].mutation_errors(mut)
    print(f"[mutation] {name} {mut}: " + "  ".join(f"{o} {v:.3e}" for o, v in worst.items()))
    assert any(v > TOL[name][o] for o, v in worst.items()), (name, mut, worst)


@pytest.mark.parametrize("name", ["mean_groups", "mean_head_groups", "segment_mean"])
def test_integer_cases_of_the_means_are_exact_in_float32(name):
    """What the equality assertion of the GPU tests rests on: on the integer-valued cases every fp32 partial sum is exact, so the
    float32 evaluation IS the float64 reference rounded once."""
    op = PR.OPS[name]
    for c in op.cases:
        if c[-1] == "int":
            inp = op.make(c)
            assert torch.equal(op.ref(inp, PR.F32)[0], op.ref(inp, PR.F64)[0].float()), c


# ==== GPU half ===========================================================================================================================
def _run(name, inp, dev="cuda"):
    ops = _ops()
    if name == "normalize_rows":
        return (ops.normalize_rows(inp["x"].to(dev)).cpu(),)
    if name == "mean_groups":
        return (ops.mean_groups(inp["x"].to(dev), inp["group"]).cpu(),)
    if name == "mean_head_groups":
        return (ops.mean_head_groups(inp["a"].to(dev), inp["b"][:inp["a"].shape[0] * inp["group"]].to(dev), inp["group"]).cpu(),)
    if name == "segment_mean":
        return (ops.segment_mean(inp["x"].to(dev), inp["offsets"].to(dev)).cpu(),)
    if name == "layernorm":
        return (ops.layernorm(inp["x"].to(dev), inp["gamma"].to(dev), inp["beta"].to(dev)).cpu(),)
    raise KeyError(name)


def _check(name, case):
    op = PR.OPS[name]
    inp = op.make(case)
    got = _run(name, inp)
    op.check(inp, got, TOL[name], str(case))
    if case[-1] == "int":                                         # the means on integer-valued data: no rounding freedom
        assert torch.equal(got[0], op.ref(inp, PR.F64)[0].float()), case
    return inp, got


@gpu
@_cases("normalize_rows")
def test_normalize_rows(case):
    _check("normalize_rows", case)


@gpu
@_cases("mean_groups")
def test_mean_groups(case):
    _check("mean_groups", case)


@gpu
@_cases("mean_head_groups")
def test_mean_head_groups(case):
    """group = 0 (allowed by the ABI: out = a, b = NULL) .. 5."""
    op = PR.OPS["mean_head_groups"]
    inp = op.make(case)
    if inp["group"] == 0:
        from vtc_amd import _lib as L
        a = inp["a"].cuda()
        out = torch.full_like(a, 7.0)
        L.check(L.lib().vtc_mean_head_groups(a.data_ptr(), None, out.data_ptr(), a.shape[0], 0, a.shape[1], _ops()._stream()), "vtc_mean_head_groups")
        assert torch.equal(out.cpu(), inp["a"])
    _check("mean_head_groups", case)


@gpu
@_cases("segment_mean")
def test_segment_mean(case):
    _check("segment_mean", case)


@gpu
@_cases("layernorm")
def test_layernorm_widths_rows_and_offset(case):
    """vtc_layernorm, fp32 output, at widths 8 / 64 / 640 / 1000 / 1024 beside 128 / 512 / 768, row counts off the 4-row grid, and
    x = 1e3 + randn: a variance formed as E[x^2] - E[x]^2 loses every digit there, the two-pass form does not."""
    _check("layernorm", case)


# ---- vtc_normalize_rows2: both sets in one launch + the watchdog word -----------------------------------------------------------------
NORMALIZE2_SHAPES = [(3, 5, 100), (5, 1027, 65), (1, 1, 1), (6, 3, 512), (1027, 2, 64), (5, 5, 1000), (2, 3, 63), (4, 4, 768)]


def _two_sets(nx, ny, d, seed=0):
    g = PR.gen(nx * 7 + ny * 3 + d + seed)
    return torch.randn(nx, d, generator=g) * PR.rowmag(nx, g, -3, 3), torch.randn(ny, d, generator=g) * PR.rowmag(ny, g, -3, 3)


def _flag(value=0):
    return torch.full((1,), value, dtype=torch.int32, device="cuda")


@gpu
@pytest.mark.parametrize("nx,ny,d", NORMALIZE2_SHAPES)
def test_normalize_rows2_is_bit_identical_to_two_normalize_rows(nx, ny, d):
    """nx != ny, nx % 4 != 0: one workgroup holds rows of both sets.  norm.hip: "per row the arithmetic of normalize_kernel"."""
    ops = _ops()
    x, y = _two_sets(nx, ny, d)
    flag = _flag()
    ox, oy = ops.normalize_rows2(x.cuda(), y.cuda(), flag)
    assert torch.equal(ox, ops.normalize_rows(x.cuda())) and torch.equal(oy, ops.normalize_rows(y.cuda()))
    assert int(flag.item()) == 0
    op = PR.OPS["normalize_rows"]
    op.check({"x": x}, (ox.cpu(),), TOL["normalize_rows"], f"rows2 x {(nx, ny, d)}")
    op.check({"x": y}, (oy.cpu(),), TOL["normalize_rows"], f"rows2 y {(nx, ny, d)}")
    ox2, oy2 = ops.normalize_rows2(x.cuda(), y.cuda(), None)       # flag = NULL is accepted
    assert torch.equal(ox2, ox) and torch.equal(oy2, oy)


@gpu
@pytest.mark.parametrize("nx,ny,d", [(3, 5, 100), (5, 6, 65), (1, 2, 3), (1027, 2, 64)])
def test_normalize_rows2_flag_word(nx, ny, d):
    ops = _ops()
    x, y = _two_sets(nx, ny, d, seed=1)
    nan, inf = float("nan"), float("inf")

    def bits(xv, yv, start=0):
        flag = _flag(start)
        ops.normalize_rows2(xv.cuda(), yv.cuda(), flag)
        return int(flag.item())

    def poked(t, r, c, v):
        t = t.clone()
        t[r, c] = v
        return t

    assert bits(x, y) == 0 and bits(x, y, start=4) == 4                             # clean: unchanged, a pre-set value survives
    assert bits(poked(x, 0, 0, nan), y) == 1                                        # NaN only in x
    assert bits(x, poked(y, 0, 0, inf)) == 2 and bits(x, poked(y, ny - 1, d // 2, -inf)) == 2      # +inf / -inf only in y
    assert bits(poked(x, nx - 1, d - 1, nan), y) == 1                               # the last column of the last row ...
    assert bits(x, poked(y, ny - 1, d - 1, nan)) == 2                               # ... of either set
    assert bits(poked(x, nx // 2, 0, inf), poked(y, 0, d - 1, nan)) == 3
    assert bits(poked(x, 0, 0, nan), y, start=4) == 5                               # the word is OR-ed
    # finite rows do not raise it: entries up to 1e15 (their squares still sum below FLT_MAX), subnormal entries in normal rows
    big = torch.full((nx, d), 1e15) * torch.sign(x)
    assert bits(big, poked(y, 0, 0, SUBNORMAL)) == 0
    assert bits(poked(x, nx - 1, d - 1, -SUBNORMAL), big[:1].expand(ny, d).contiguous()) == 0


@gpu
@pytest.mark.parametrize("nx,ny,d", [(3, 5, 100), (5, 6, 512), (2, 1027, 64)])
def test_normalize_rows2_flags_a_zero_row(nx, ny, d):
    """An all-zero row normalises to 0/0 = NaN, as in the reference (x / x.norm()), and a row whose squares all underflow to x/0 =
    inf: both leave the launch as non-finite embeddings, so both raise the word -- what vtc_nonfinite_flag2 says of the outputs."""
    ops = _ops()
    x, y = _two_sets(nx, ny, d, seed=2)
    x, y = x / x.norm(dim=1, keepdim=True), y / y.norm(dim=1, keepdim=True)

    def run(xv, yv):
        flag = _flag()
        ox, oy = ops.normalize_rows2(xv.cuda(), yv.cuda(), flag)
        return int(flag.item()), ox.cpu(), oy.cpu(), ops.nonfinite_bits(ox, oy)

    xz = x.clone()
    xz[nx - 1] = 0
    bits, ox, oy, of_outputs = run(xz, y)
    assert torch.isnan(ox[nx - 1]).all() and torch.isfinite(ox[:nx - 1]).all() and torch.isfinite(oy).all()
    print(f"[flag] zero row in x: flag {bits}, vtc_nonfinite_flag2 of the outputs {of_outputs}")
    assert of_outputs == 1 and bits == 1
    yz = y.clone()
    yz[0] = 0
    bits, ox, oy, of_outputs = run(x, yz)
    assert torch.isnan(oy[0]).all() and torch.isfinite(oy[1:]).all() and torch.isfinite(ox).all()
    print(f"[flag] zero row in y: flag {bits}, vtc_nonfinite_flag2 of the outputs {of_outputs}")
    assert of_outputs == 2 and bits == 2
    yu = y.clone()
    yu[ny - 1] = 1e-30                                             # every square underflows to 0: x / 0 = inf
    bits, ox, oy, of_outputs = run(xz, yu)
    assert torch.isinf(oy[ny - 1]).all()
    assert of_outputs == 3 and bits == 3


@gpu
@pytest.mark.parametrize("fused", [True, False])
def test_check_finite_raises_for_a_cached_feature_forward_with_a_zero_row(fused):
    """The 2-D cached-feature path (model/model.py:328-330): a missing clip's features are zeros, the forward hands back a NaN
    embedding for it, and check_finite() must say so -- with the watchdog fused into the last launch (vtc_normalize_rows2) and in
    its unfused form (vtc_nonfinite_flag2 on the normalised outputs)."""
    from dataclasses import asdict

    from oracle import arch as A
    from vtc_amd.host import model as HM
    from vtc_amd.host.clip_arch import ClipConfig
    a = A.TINY
    sd = A.synth_model(a, 72, "clip_finaltf")
    m = HM.PretrainedCLIP_finaltf(model_type=ClipConfig(**asdict(a)), branch_to_adapt_val="text", n_heads=2)
    m.load_state_dict(sd, strict=True)
    m = m.eval().cuda()
    m.compute_dtype = torch.float32
    feats = torch.randn(4, m.feature_dim, generator=PR.gen(3))
    title = A.synth_tokens(4, a, 74)
    comments = A.synth_tokens(20, a, 75, empty_frac=0.3).reshape(4, 5, -1)
    out = m(feats.cuda(), title.cuda(), comments.cuda())
    m.check_finite()                                               # clean features: nothing to report
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all()
    feats[2] = 0
    if fused:
        out = m(feats.cuda(), title.cuda(), comments.cuda())
    else:
        m.nonfinite_watchdog = False                               # the forward without its fused watchdog ...
        out = m(feats.cuda(), title.cuda(), comments.cuda())
        m.nonfinite_watchdog = True
        m._watch(out[0], out[1])                                   # ... and the unfused one over what it returned
    assert torch.isnan(out[0][2]).all() and torch.isfinite(out[0][[0, 1, 3]]).all() and torch.isfinite(out[1]).all()
    with pytest.raises(RuntimeError, match="non-finite values in its visual embeddings"):
        m.check_finite()
    m.check_finite()                                               # the flag is cleared


# ---- vtc_nonfinite_flag / vtc_nonfinite_flag2 (device-memory flag) --------------------------------------------------------------------
GRID_STRIDE_N = 1024 * 256 + 1            # one element more than 1024 workgroups of 256 threads cover: the grid-stride loop is taken


@gpu
def test_nonfinite_flag():
    ops = _ops()

    def bits(x, start=0):
        return int(ops.nonfinite_flag(x.cuda(), _flag(start)).item())

    for bad in (float("nan"), float("inf"), -float("inf")):
        assert bits(torch.tensor([bad])) == 1                                       # n = 1
        assert bits(torch.tensor([1.0])) == 0
        x = torch.ones(GRID_STRIDE_N)
        assert bits(x) == 0 and bits(x, start=6) == 6
        x[-1] = bad                                                                 # the only bad value LAST
        assert bits(x) == 1 and bits(x, start=6) == 7
        x[-1], x[0] = 1.0, bad                                                      # ... and first
        assert bits(x) == 1
    # the kernel tests the exponent bits: FLT_MAX, -FLT_MAX and subnormals are finite
    x = torch.tensor([FLT_MAX, -FLT_MAX, SUBNORMAL, -SUBNORMAL, 0.0, -0.0] * 50 + [FLT_MAX])
    assert x[2] != 0 and bits(x) == 0


@gpu
def test_nonfinite_flag2():
    ops = _ops()

    def bits(x, y, start=0):
        return int(ops.nonfinite_flag2(x.cuda(), y.cuda(), _flag(start)).item())

    one = torch.ones(1)
    nan = torch.tensor([float("nan")])
    assert bits(one, one) == 0 and bits(nan, one) == 1 and bits(one, nan) == 2 and bits(nan, nan) == 3      # n = m = 1
    for n, m_ in ((GRID_STRIDE_N, 1000), (1000, GRID_STRIDE_N), (GRID_STRIDE_N - 300, 301)):
        for bad in (float("nan"), float("inf"), -float("inf")):
            x, y = torch.ones(n), torch.ones(m_)
            assert bits(x, y) == 0 and bits(x, y, start=4) == 4
            x[-1] = bad                                                             # the last of x
            assert bits(x, y) == 1
            x[-1], y[0] = 1.0, bad                                                  # the first of y
            assert bits(x, y) == 2
            y[0], y[-1] = 1.0, bad                                                  # the last of y: the last element of the launch
            assert bits(x, y) == 2
            x[0] = bad                                                              # the first of x as well
            assert bits(x, y, start=4) == 7
    finite = torch.tensor([FLT_MAX, -FLT_MAX, SUBNORMAL, -SUBNORMAL, 0.0] * 60)
    assert bits(finite, finite[:7]) == 0
