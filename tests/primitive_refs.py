"""References, case lists and the error measure of the per-primitive tests (tests/test_gpu_small_ops.py,
tests/test_gpu_train_primitives.py): the wrapper-level fp32 ops of norm.hip and the training kernels of train.hip
(include/vtc_hip.h, sections "small fp32 ops of the wrappers" and "adapter-only training step").

Every reference is plain torch on the CPU, written from the formula in the header comment -- F.layer_norm, softmax(q k^T / 8) v,
x / x.norm(), 0.5 (CE(sim) + CE(sim^T)) with autograd behind them -- and takes the dtype it computes in: float64 is THE reference,
float32 is the yardstick the tolerances are calibrated with (a tolerance is 4 x the worst error of the float32 evaluation over the
op's cases: the margin covers another summation order and device expf / sqrtf an ulp or two from libm; it is never measured on a kernel).

The error measure is  e = max |got - ref64| / scale  with a per-row scale, so that an error is judged where it occurs and not
against the largest entry of the tensor: for a sum the fp64 sum of the absolute values of its terms, for the composite backward
formulas the largest intermediate magnitude of the row (per (sequence, head) block and third of dqkv for attention, per column for
colsum / dgamma / dbeta).

Every op also names deliberately wrong references (`muts`): the CPU half of the tests proves that each of them exceeds the op's
tolerance on at least one case, i.e. that the tests can fail.
"""
from __future__ import annotations

import contextlib
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32
TINY = float(torch.finfo(torch.float32).tiny)      # absolute floor of a scale: results down in the subnormals carry no relative precision


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


def rowmag(n: int, g: torch.Generator, lo: float, hi: float) -> torch.Tensor:
    """[n, 1] magnitudes 10^u, u uniform in [lo, hi]."""
    return 10.0 ** (lo + (hi - lo) * torch.rand(n, 1, generator=g))


def err(got: torch.Tensor, ref: torch.Tensor, scale) -> float:
    """max |got - ref64| / scale (NaN when `got` holds a NaN)."""
    d = (got.detach().cpu().to(F64) - ref.to(F64)).abs() / scale
    return float(d.max())


@contextlib.contextmanager
def single_thread():
    """The float32 yardstick is evaluated on ONE thread: torch splits its CPU reductions by the thread count, so the figure a
    tolerance is derived from would otherwise depend on the machine's core count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


@dataclass
class Op:
    name: str
    outs: Tuple[str, ...]                                        # names of the outputs, in the order ref / scale return them
    cases: List[tuple]
    make: Callable[[tuple], dict]                                # case -> inputs (fp32 / int CPU tensors and plain numbers)
    ref: Callable[..., tuple]                                    # (inputs, dtype = F64, mut = None) -> outputs in `dtype`
    scale: Callable[[dict], tuple]                               # inputs -> fp64 scales, broadcastable to the outputs
    muts: Tuple[str, ...]

    def errors(self, inp: dict, got: Sequence[torch.Tensor]) -> Dict[str, float]:
        ref, sc = self.ref(inp, F64), self.scale(inp)
        assert len(got) == len(self.outs)
        return {o: err(g, r, s) for o, g, r, s in zip(self.outs, got, ref, sc)}

    def check(self, inp: dict, got: Sequence[torch.Tensor], tol: Dict[str, float], what="") -> Dict[str, float]:
        """Print every figure, then assert all of them (exact ops: tol 0, i.e. equality with the fp32-rounded reference)."""
        e = self.errors(inp, got)
        print(f"[e] {self.name} {what}: " + "  ".join(f"{o} {v:.3e} (tol {tol[o]:.1e})" for o, v in e.items()))
        bad = {o: v for o, v in e.items() if not v <= tol[o]}
        assert not bad, (self.name, what, bad, tol)
        return e

    def calibrate(self) -> Dict[str, float]:
        """Worst error of the float32 evaluation over the op's cases, per output."""
        worst = {o: 0.0 for o in self.outs}
        for c in self.cases:
            inp = self.make(c)
            with single_thread():
                got = self.ref(inp, F32)
            for o, v in self.errors(inp, got).items():
                worst[o] = max(worst[o], v) if v == v else float("nan")
        return worst

    def mutation_errors(self, mut: str) -> Dict[str, float]:
        """Worst error of one wrong reference over the op's cases, per output."""
        worst = {o: 0.0 for o in self.outs}
        for c in self.cases:
            inp = self.make(c)
            for o, v in self.errors(inp, self.ref(inp, F64, mut)).items():
                worst[o] = max(worst[o], v if v == v else float("inf"))
        return worst


OPS: Dict[str, Op] = {}


def _register(op: Op) -> Op:
    OPS[op.name] = op
    return op


def _left(out: torch.Tensor, inp_like: torch.Tensor, mut: Optional[str]) -> torch.Tensor:
    """The "left at its input value" mutations: what a kernel that never wrote the last column / row would hand back."""
    if mut == "last_column_left":
        out = out.clone()
        out[..., -1] = inp_like[..., -1].to(out.dtype) if isinstance(inp_like, torch.Tensor) else inp_like
    elif mut == "last_row_left":
        out = out.clone()
        out[-1] = inp_like[-1].to(out.dtype) if isinstance(inp_like, torch.Tensor) else inp_like
    return out


# ---- the shape grid of the row-wise ops: rows on and off the 4-rows-per-workgroup grid, widths on and off the 64-lane grid ----------
ROW_SHAPES = [(1, 1), (1, 63), (3, 64), (4, 65), (5, 100), (1027, 512), (3, 768), (5, 1000), (4, 512), (1027, 1), (1, 1000), (3, 63),
              (1027, 65), (5, 64)]


# ---- vtc_normalize_rows: y = x / ||x|| -----------------------------------------------------------------------------------------------
def _make_rows(case):
    n, d = case
    g = gen(1000 * n + d)
    return {"x": torch.randn(n, d, generator=g) * rowmag(n, g, -3, 3)}       # row magnitudes spread over 1e-3 .. 1e3


def _ref_normalize(inp, dtype=F64, mut=None):
    x = inp["x"].to(dtype)
    xs = x[:, :-1] if mut == "norm_without_last_column" and x.shape[1] > 1 else x
    return (_left(x / xs.norm(dim=1, keepdim=True), x, mut),)


def _scale_normalize(inp):
    return (_ref_normalize(inp)[0].abs().amax(1, keepdim=True),)


_register(Op("normalize_rows", ("y",), ROW_SHAPES, _make_rows, _ref_normalize, _scale_normalize,
             ("norm_without_last_column", "last_column_left", "last_row_left")))


# ---- vtc_normalize_rows_bwd: dx of y = x / ||x|| ------------------------------------------------------------------------------------
def _make_norm_bwd(case):
    n, d = case
    g = gen(2000 * n + d)
    return {"x": torch.randn(n, d, generator=g) * rowmag(n, g, -3, 3), "dy": torch.randn(n, d, generator=g) * rowmag(n, g, -2, 2),
            "dx0": torch.full((n, d), 7.0)}


def _ref_norm_bwd(inp, dtype=F64, mut=None):
    x, dy = inp["x"].to(dtype), inp["dy"].to(dtype)
    if mut == "no_projection_term":
        dx = dy / x.norm(dim=1, keepdim=True)
    else:
        with torch.enable_grad():
            xl = x.clone().requires_grad_(True)
            (dx,) = torch.autograd.grad(xl / xl.norm(dim=1, keepdim=True), xl, dy)
    return (_left(dx, inp["dx0"], mut),)


def _scale_norm_bwd(inp):
    x, dy = inp["x"].to(F64), inp["dy"].to(F64)
    nrm = x.norm(dim=1, keepdim=True)
    y = x / nrm
    return ((dy.abs().amax(1, keepdim=True) + y.abs().amax(1, keepdim=True) * (y * dy).sum(1, keepdim=True).abs()) / nrm,)


_register(Op("normalize_rows_bwd", ("dx",), ROW_SHAPES, _make_norm_bwd, _ref_norm_bwd, _scale_norm_bwd,
             ("no_projection_term", "last_column_left", "last_row_left")))


# ---- the means: vtc_mean_groups, vtc_mean_head_groups, vtc_segment_mean --------------------------------------------------------------
# kind "int": small integers, every sum exact in fp32 (the GPU test asserts equality); kind "rand": random against fp64
def _mean_data(shape, kind, g):
    if kind == "int":
        return torch.randint(-50, 51, shape, generator=g).float()
    return torch.randn(shape, generator=g) * rowmag(shape[0], g, -2, 2)


MEAN_GROUPS_CASES = [(ng, grp, d, k) for (ng, grp, d) in [(1, 1, 1), (3, 8, 63), (5, 6, 100), (5, 6, 1000), (129, 8, 65), (7, 5, 512)]
                     for k in ("int", "rand")]


def _make_mean_groups(case):
    ng, grp, d, kind = case
    return {"x": _mean_data((ng * grp, d), kind, gen(ng * 131 + grp * 17 + d)), "group": grp}


def _ref_mean_groups(inp, dtype=F64, mut=None):
    x, grp = inp["x"].to(dtype), inp["group"]
    x3 = x.reshape(-1, grp, x.shape[1])
    if mut == "last_row_of_a_group_skipped":
        out = x3[:, :-1].sum(1) / grp
    elif mut == "divided_by_group_plus_one":
        out = x3.sum(1) / (grp + 1)
    else:
        out = x3.mean(1)
    return (_left(out, 7.0, mut),)


def _scale_mean_groups(inp):
    x, grp = inp["x"].to(F64), inp["group"]
    return (x.abs().reshape(-1, grp, x.shape[1]).sum(1) / grp + TINY,)


_register(Op("mean_groups", ("out",), MEAN_GROUPS_CASES, _make_mean_groups, _ref_mean_groups, _scale_mean_groups,
             ("last_row_of_a_group_skipped", "divided_by_group_plus_one", "last_column_left")))

# group = 0 is allowed by the ABI: out = a
MEAN_HEAD_CASES = [(ng, grp, d, k) for (ng, grp, d) in [(1, 0, 64), (3, 0, 100), (4, 5, 63), (5, 1, 65), (129, 5, 100), (3, 5, 1000)]
                   for k in ("int", "rand")]


def _make_mean_head(case):
    ng, grp, d, kind = case
    g = gen(ng * 137 + grp * 19 + d)
    return {"a": _mean_data((ng, d), kind, g), "b": _mean_data((max(ng * grp, 1), d), kind, g), "group": grp}


def _ref_mean_head(inp, dtype=F64, mut=None):
    a, b, grp = inp["a"].to(dtype), inp["b"].to(dtype), inp["group"]
    s = b[:a.shape[0] * grp].reshape(a.shape[0], grp, a.shape[1]).sum(1) if grp else torch.zeros_like(a)
    if mut == "head_row_missing":
        out = s / (1 + grp)
    elif mut == "divided_by_group":
        out = (a + s) / max(grp, 1) if grp != 1 else (a + s) / 3
    else:
        out = (a + s) / (1 + grp)
    return (_left(out, 7.0, mut),)


def _scale_mean_head(inp):
    a, b, grp = inp["a"].to(F64).abs(), inp["b"].to(F64).abs(), inp["group"]
    s = b[:a.shape[0] * grp].reshape(a.shape[0], grp, a.shape[1]).sum(1) if grp else torch.zeros_like(a)
    return ((a + s) / (1 + grp) + TINY,)


_register(Op("mean_head_groups", ("out",), MEAN_HEAD_CASES, _make_mean_head, _ref_mean_head, _scale_mean_head,
             ("head_row_missing", "divided_by_group", "last_column_left")))

SEGMENT_LENGTHS = [1, 2, 8, 37, 1, 8, 2, 37, 1]                   # first and last segment of length 1
SEGMENT_CASES = [(d, k) for d in (1, 65, 100, 1000) for k in ("int", "rand")]


def _make_segment(case):
    d, kind = case
    offs = torch.zeros(len(SEGMENT_LENGTHS) + 1, dtype=torch.int32)
    offs[1:] = torch.cumsum(torch.tensor(SEGMENT_LENGTHS), 0)
    return {"x": _mean_data((int(offs[-1]), d), kind, gen(7000 + d)), "offsets": offs}


def _ref_segment(inp, dtype=F64, mut=None):
    x, offs = inp["x"].to(dtype), inp["offsets"].tolist()
    rows = []
    for lo, hi in zip(offs[:-1], offs[1:]):
        if mut == "last_row_of_a_segment_skipped" and hi - lo > 1:
            rows.append(x[lo:hi - 1].sum(0) / (hi - lo))
        elif mut == "divided_by_length_plus_one":
            rows.append(x[lo:hi].sum(0) / (hi - lo + 1))
        else:
            rows.append(x[lo:hi].mean(0))
    return (_left(torch.stack(rows), 7.0, mut),)


def _scale_segment(inp):
    x, offs = inp["x"].to(F64).abs(), inp["offsets"].tolist()
    return (torch.stack([x[lo:hi].mean(0) for lo, hi in zip(offs[:-1], offs[1:])]) + TINY,)


_register(Op("segment_mean", ("out",), SEGMENT_CASES, _make_segment, _ref_segment, _scale_segment,
             ("last_row_of_a_segment_skipped", "divided_by_length_plus_one", "last_column_left")))


# ---- vtc_layernorm (forward), fp32 output: widths nobody runs beside 128 / 512 / 768, rows off the 4-row grid, one large common offset ----
LAYERNORM_CASES = [(1, 8, 0.0), (3, 64, 0.0), (5, 640, 0.0), (37, 1000, 0.0), (5, 1024, 0.0), (3, 128, 0.0), (1027, 512, 0.0),
                   (5, 768, 0.0), (37, 512, 1e3), (6, 1024, 1e3)]


def _make_layernorm(case):
    rows, width, offset = case
    g = gen(rows * 31 + width)
    mag = rowmag(rows, g, -3, 3) if offset == 0.0 else 1.0
    x = offset + (torch.randn(rows, width, generator=g) + 0.3) * mag       # x = 1e3 + randn separates a two-pass variance from E[x^2] - E[x]^2
    return {"x": x, "gamma": torch.randn(width, generator=g), "beta": torch.randn(width, generator=g)}


def _layernorm_fn(x, gamma, beta, mut):
    w = x.shape[1]
    if mut == "unbiased_variance":
        mu, var = x.mean(1, keepdim=True), x.var(1, unbiased=True, keepdim=True)
        return (x - mu) / torch.sqrt(var + 1e-5) * gamma + beta
    return F.layer_norm(x, (w,), gamma, beta, 1e-6 if mut == "eps_1e-6" else 1e-5)


def _ref_layernorm(inp, dtype=F64, mut=None):
    x = inp["x"].to(dtype)
    return (_left(_layernorm_fn(x, inp["gamma"].to(dtype), inp["beta"].to(dtype), mut), x, mut),)


def _ln_stats(x):
    mu = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5)
    return mu, rstd, (x - mu) * rstd


def _scale_layernorm(inp):
    x, gm, bt = inp["x"].to(F64), inp["gamma"].to(F64), inp["beta"].to(F64)
    mu, rstd, _ = _ln_stats(x)
    # y = (x - mean) rstd gamma + beta: the operands of the cancellation x - mean are |x| and |mean|
    return (((x.abs() + mu.abs()) * rstd * gm.abs() + bt.abs()).amax(1, keepdim=True),)


_register(Op("layernorm", ("y",), LAYERNORM_CASES, _make_layernorm, _ref_layernorm, _scale_layernorm,
             ("eps_1e-6", "unbiased_variance", "last_column_left", "last_row_left")))


# ---- vtc_layernorm_bwd ---------------------------------------------------------------------------------------------------------------
# (rows, width, accumulate_dx): width 100 = lanes with different element counts, 1024 = the register-array limit
LAYERNORM_BWD_CASES = [(1, 4, 0), (3, 64, 1), (4, 100, 0), (5, 100, 1), (257, 128, 1), (2310, 512, 1), (5, 768, 0), (257, 1024, 1),
                       (3, 1024, 0), (2310, 100, 0), (4, 512, 0), (1, 1024, 1), (257, 64, 0), (5, 4, 1)]


def _make_layernorm_bwd(case):
    rows, width, acc = case
    g = gen(rows * 37 + width + acc)
    return {"x": (torch.randn(rows, width, generator=g) + 0.3) * rowmag(rows, g, -2, 2), "gamma": torch.randn(width, generator=g),
            "dy": torch.randn(rows, width, generator=g) * rowmag(rows, g, -1, 1),
            "dx0": torch.randn(rows, width, generator=g),            # accumulate_dx = 1 starts from random data; = 0 must overwrite it
            "accumulate_dx": acc}


def _ref_layernorm_bwd(inp, dtype=F64, mut=None):
    x, gm, dy, dx0 = (inp[k].to(dtype) for k in ("x", "gamma", "dy", "dx0"))
    if mut == "dgamma_without_last_row":
        dy_g = dy.clone()
        dy_g[-1] = 0
    with torch.enable_grad():
        xl, gl, bl = x.clone().requires_grad_(True), gm.clone().requires_grad_(True), torch.zeros_like(gm).requires_grad_(True)
        y = _layernorm_fn(xl, gl, bl, mut)
        dx, dg, db = torch.autograd.grad(y, [xl, gl, bl], dy, retain_graph=True)
        if mut == "dgamma_without_last_row":
            (dg,) = torch.autograd.grad(y, [gl], dy_g)
    if inp["accumulate_dx"] and mut != "accumulate_ignored":
        dx = dx0 + dx
    elif mut == "accumulate_ignored" and not inp["accumulate_dx"]:
        dx = dx0 + dx
    return (_left(dx, dx0, mut), dg, db)


def _scale_layernorm_bwd(inp):
    x, gm, dy, dx0 = (inp[k].to(F64) for k in ("x", "gamma", "dy", "dx0"))
    mu, rstd, xh = _ln_stats(x)
    g = dy * gm
    a, b = g.mean(1, keepdim=True).abs(), (g * xh).mean(1, keepdim=True).abs()
    sdx = rstd * (g.abs().amax(1, keepdim=True) + a + xh.abs().amax(1, keepdim=True) * b)
    if inp["accumulate_dx"]:
        sdx = sdx + dx0.abs().amax(1, keepdim=True)
    # dgamma = sum_r dy xhat: a term's xhat carries the rounding of the cancellation x - mean, whose operands are |x| and |mean|
    return (sdx, (dy.abs() * (x.abs() + mu.abs()) * rstd).sum(0) + TINY, dy.abs().sum(0) + TINY)


_register(Op("layernorm_bwd", ("dx", "dgamma", "dbeta"), LAYERNORM_BWD_CASES, _make_layernorm_bwd, _ref_layernorm_bwd, _scale_layernorm_bwd,
             ("eps_1e-6", "unbiased_variance", "dgamma_without_last_row", "last_column_left", "accumulate_ignored")))


# ---- vtc_attention_small_bwd: unmasked, head_dim 64, contiguous sequences -----------------------------------------------------------
# (n_seq, L, heads, kind): n_seq * heads on and off the 4-waves-per-workgroup grid; "spread": qkv * 2, a softmax that is not near-uniform;
# "dominant": one key wins every query by a logit gap > 30, so that P has exact zeros in fp32
ATTENTION_BWD_CASES = [(3, 1, 1, "spread"), (5, 2, 2, "spread"), (33, 6, 8, "spread"), (3, 15, 12, "spread"), (5, 16, 2, "spread"),
                       (5, 15, 2, "spread"), (2, 16, 12, "spread"), (7, 16, 1, "dominant"), (3, 6, 1, "dominant"), (5, 2, 8, "dominant")]


def _make_attention_bwd(case):
    n_seq, L, heads, kind = case
    W = heads * 64
    g = gen(n_seq * 41 + L * 7 + heads)
    qkv = torch.randn(n_seq * L, 3 * W, generator=g) * 2
    if kind == "dominant":
        t = qkv.reshape(n_seq, L, 3, heads, 64)
        u = torch.sign(torch.randn(n_seq, 1, heads, 64, generator=g)) * 4        # q . k0 / 8 = 16 * 64 / 8 = 128 against |logits| ~ 12
        t[:, :, 0] = u + 0.3 * torch.randn(n_seq, L, heads, 64, generator=g)
        t[:, 0, 1] = u[:, 0]
        t[:, 1:, 1] = torch.randn(n_seq, L - 1, heads, 64, generator=g)
        qkv = t.reshape(n_seq * L, 3 * W).contiguous()
    return {"qkv": qkv, "dout": torch.randn(n_seq * L, W, generator=g), "dqkv0": torch.full((n_seq * L, 3 * W), 7.0),
            "n_seq": n_seq, "L": L, "heads": heads}


def split_qkv(inp, dtype):
    n_seq, L, heads = inp["n_seq"], inp["L"], inp["heads"]
    t = inp["qkv"].to(dtype).reshape(n_seq, L, 3, heads, 64).permute(2, 0, 3, 1, 4)       # [3, n_seq, heads, L, 64]
    dO = inp["dout"].to(dtype).reshape(n_seq, L, heads, 64).permute(0, 2, 1, 3)          # [n_seq, heads, L, 64]
    return t, dO


def _merge_dqkv(dt, inp):                                            # [3, n_seq, heads, L, 64] -> [n_seq * L, 3 W]
    return dt.permute(1, 3, 0, 2, 4).reshape(inp["n_seq"] * inp["L"], 3 * inp["heads"] * 64)


def _ref_attention_bwd(inp, dtype=F64, mut=None):
    t, dO = split_qkv(inp, dtype)
    if mut in ("no_1/8_scale", "dS_without_rowsum_term"):
        q, k, v = t
        sc = 1.0 if mut == "no_1/8_scale" else 0.125
        P = ((q @ k.transpose(-1, -2)) * sc).softmax(-1)
        dP = dO @ v.transpose(-1, -2)
        dS = P * (dP - (0 if mut == "dS_without_rowsum_term" else (dP * P).sum(-1, keepdim=True)))
        dt = torch.stack([dS @ k * sc, dS.transpose(-1, -2) @ q * sc, P.transpose(-1, -2) @ dO])
    else:
        with torch.enable_grad():
            tl = t.clone().requires_grad_(True)
            o = ((tl[0] @ tl[1].transpose(-1, -2)) / 8).softmax(-1) @ tl[2]
            (dt,) = torch.autograd.grad(o, tl, dO)
    if mut == "last_head_left":
        dt = dt.clone()
        dt[:, :, -1] = 7.0
    if mut == "last_sequence_left":
        dt = dt.clone()
        dt[:, -1] = 7.0
    return (_merge_dqkv(dt, inp),)


def _scale_attention_bwd(inp):
    (q, k, v), dO = split_qkv(inp, F64)
    P = ((q @ k.transpose(-1, -2)) / 8).softmax(-1)
    dP = dO @ v.transpose(-1, -2)
    adS = P * ((dO.abs() @ v.abs().transpose(-1, -2)) + (dP * P).sum(-1, keepdim=True).abs())
    s = torch.stack([(adS @ k.abs()) / 8, (adS.transpose(-1, -2) @ q.abs()) / 8, P.transpose(-1, -2) @ dO.abs()])
    s = s.amax((-1, -2), keepdim=True).expand(3, *P.shape[:2], inp["L"], 64)              # one scale per (third, sequence, head)
    return (_merge_dqkv(s, inp),)


_register(Op("attention_small_bwd", ("dqkv",), ATTENTION_BWD_CASES, _make_attention_bwd, _ref_attention_bwd, _scale_attention_bwd,
             ("no_1/8_scale", "dS_without_rowsum_term", "last_head_left", "last_sequence_left")))


# ---- vtc_clip_loss_bwd: dsim of 0.5 (CE(sim) + CE(sim^T)) ----------------------------------------------------------------------------
# "model": logits at the model's real scale, 100 x cosines of paired unit vectors (rows span about +-100); "randn4": randn * 4
CLIP_LOSS_BWD_CASES = [(n, k) for n in (1, 2, 63, 64, 65, 257, 1000) for k in ("model", "randn4")]


def _make_clip_loss_bwd(case):
    n, kind = case
    g = gen(n * 3 + len(kind))
    if kind == "model":
        v = F.normalize(torch.randn(n, 16, generator=g), dim=1)
        t = F.normalize(v + 0.2 * torch.randn(n, 16, generator=g), dim=1)
        sim = 100.0 * v @ t.t()
    else:
        sim = torch.randn(n, n, generator=g) * 4
    return {"sim": sim.contiguous(), "dsim0": torch.full((n, n), 7.0)}


def _ref_clip_loss_bwd(inp, dtype=F64, mut=None):
    sim = inp["sim"].to(dtype)
    n = sim.shape[0]
    with torch.enable_grad():
        sl = sim.clone().requires_grad_(True)
        tgt = torch.arange(n)
        (d,) = torch.autograd.grad(0.5 * (F.cross_entropy(sl, tgt) + F.cross_entropy(sl.t(), tgt)), sl)
    if mut == "no_diagonal_term":
        d = d + (0.5 / n) * 2 * torch.eye(n, dtype=dtype)
    if mut == "column_softmax_from_row_statistics":
        d = (0.5 / n) * (2 * sim.softmax(1) - 2 * torch.eye(n, dtype=dtype))
    return clip_loss_bwd_sums(_left(d, inp["dsim0"], mut))


def clip_loss_bwd_sums(dsim: torch.Tensor):
    """(dsim, its row sums and column sums in fp64): the structural half of the check.  The row-softmax half of dsim,
    (softmax_row - I) / 2n, sums to 0 along every row and the column half along every column; a row of the SUM of the two halves
    does not (its sum is (sum_j softmax_col_j[i] - 1) / 2n: only the total of the matrix is 0), so the sums are compared with
    the reference's, each against the sum of the absolute values of its terms."""
    d64 = dsim.detach().cpu().to(F64)
    return (dsim, d64.sum(1), d64.sum(0))


def _scale_clip_loss_bwd(inp):
    sim = inp["sim"].to(F64)
    n = sim.shape[0]
    terms = (0.5 / n) * (sim.softmax(1) + sim.softmax(0) + 2 * torch.eye(n, dtype=F64))      # |terms| of every entry
    return (terms.amax(1, keepdim=True), terms.sum(1), terms.sum(0))


_register(Op("clip_loss_bwd", ("dsim", "row_sums", "col_sums"), CLIP_LOSS_BWD_CASES, _make_clip_loss_bwd, _ref_clip_loss_bwd, _scale_clip_loss_bwd,
             ("no_diagonal_term", "column_softmax_from_row_statistics", "last_row_left", "last_column_left")))


# ---- vtc_quickgelu: y = x sigmoid(1.702 x), dx = dy (s + 1.702 x s (1 - s)) -------------------------------------------------------
# "lin": linspace(-60, 60); "lin120": linspace(-120, 120), far enough out for float64 to round to exactly 0 in fp32
QUICKGELU_CASES = [(1, "rand"), (255, "lin"), (4097, "lin"), (1001, "lin120"), (1000, "rand"), (4097, "rand")]


def _make_quickgelu(case):
    n, kind = case
    g = gen(n + len(kind))
    x = torch.randn(n, generator=g) * 3 if kind == "rand" else torch.linspace(-1, 1, n) * (60 if kind == "lin" else 120)
    return {"x": x, "dy": torch.randn(n, generator=g) * 10.0 ** (4 * torch.rand(n, generator=g) - 2), "out0": torch.full((n,), 7.0)}


def _ref_quickgelu(inp, dtype=F64, mut=None):
    x, dy = inp["x"].to(dtype), inp["dy"].to(dtype)
    c = 1.7 if mut == "1.7_instead_of_1.702" else 1.702
    s = torch.sigmoid(c * x)
    d = s if mut == "derivative_without_second_term" else s + c * x * s * (1 - s)
    return (_left(x * s, inp["out0"], mut), _left(dy * d, inp["out0"], mut))


def _scale_quickgelu(inp):
    # elementwise: every element is its own row; |sigmoid| <= 1 and |d/dx| <= 1.1, so the operands' magnitudes are the scale
    return (inp["x"].to(F64).abs() + TINY, inp["dy"].to(F64).abs() + TINY)


_register(Op("quickgelu", ("y", "dx"), QUICKGELU_CASES, _make_quickgelu, _ref_quickgelu, _scale_quickgelu,
             ("1.7_instead_of_1.702", "derivative_without_second_term", "last_column_left")))


# ---- vtc_adam_step: torch.optim.Adam single-tensor step, weight_decay 0 ------------------------------------------------------------
# The ABI passes lr, beta1, beta2, eps as float: the kernel can never see 0.999, so the reference takes them ROUNDED TO FP32 first
# (fed the unrounded 0.999 an fp64 reference disagrees with a correct fp32 evaluation by 7e-6 relative in the step).
ADAM_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
ADAM_STEPS = 5
ADAM_CASES = [(n, ams) for n in (1, 255, 1000, 4099) for ams in (0, 1)]


def adam_hyper32() -> Dict[str, float]:
    return {k: float(np.float32(v)) for k, v in ADAM_HYPER.items()}


def adam_sequence(case):
    """Initial state (p, m, v, vmax: zeros as torch.optim starts them) and the gradients of ADAM_STEPS consecutive steps: magnitudes
    1e-8 .. 1, on both sides of eps; from step 3 on they shrink by 1e-2, so v falls below vmax and amsgrad must keep vmax."""
    n, _ = case
    g = gen(n + 5)
    p = torch.randn(n, generator=g) * 10.0 ** (6 * torch.rand(n, generator=g) - 6)       # |p| 1e-6 .. 1: the update is seen next to a small p
    grads = [torch.sign(torch.randn(n, generator=g)) * 10.0 ** (8 * torch.rand(n, generator=g) - 8) * (1.0 if t < 2 else 1e-2)
             for t in range(ADAM_STEPS)]
    return {"p": p, "m": torch.zeros(n), "v": torch.zeros(n), "vmax": torch.zeros(n)}, grads


def _make_adam(case):
    """One step from a state in the middle of the sequence (the CPU calibration and mutation checks walk the whole sequence with
    adam_sequence; this is the single-step form the Op interface needs): step 3, state from two fp64 reference steps."""
    state, grads = adam_sequence(case)
    for t in (1, 2):
        out = _ref_adam({**state, "g": grads[t - 1], "step": t, "amsgrad": case[1]}, F64)
        state = {k: o.float() for k, o in zip(("p", "m", "v", "vmax"), out)}
    return {**state, "g": grads[2], "step": 3, "amsgrad": case[1]}


def _ref_adam(inp, dtype=F64, mut=None):
    h = adam_hyper32()
    lr, b1, b2, eps = h["lr"], h["beta1"], h["beta2"], h["eps"]
    p, m, v, vmax, g = (inp[k].to(dtype) for k in ("p", "m", "v", "vmax", "g"))
    t = inp["step"] - 1 if mut == "bias_correction_of_previous_step" and inp["step"] > 1 else inp["step"]
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t                       # scalars in double, as torch.optim computes them
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    vm = torch.maximum(vmax, v2) if inp["amsgrad"] else vmax
    vhat = vm if inp["amsgrad"] and mut != "vmax_ignored" else v2
    p2 = p - (lr / bc1) * m2 / (vhat.sqrt() / math.sqrt(bc2) + eps)
    if mut == "eps_inside_the_square_root":
        p2 = p - (lr / bc1) * m2 / ((vhat / bc2 + eps).sqrt())
    return (p2, m2, v2, vm)


def _scale_adam(inp):
    h = adam_hyper32()
    p2, m2, v2, vm = _ref_adam(inp, F64)
    p, m, g = inp["p"].to(F64), inp["m"].to(F64), inp["g"].to(F64)
    return (p.abs() + (p2 - p).abs() + TINY, h["beta1"] * m.abs() + (1 - h["beta1"]) * g.abs() + TINY, v2 + TINY, vm + TINY)


_register(Op("adam_step", ("p", "m", "v", "vmax"), ADAM_CASES, _make_adam, _ref_adam, _scale_adam,
             ("vmax_ignored", "bias_correction_of_previous_step", "eps_inside_the_square_root")))


# ---- vtc_colsum_f32: rows above and below the 64-way row split ------------------------------------------------------------------------
COLSUM_CASES = [(r, c, k) for (r, c) in [(1, 1), (63, 255), (64, 256), (65, 257), (5000, 1536), (5000, 1), (1, 1536), (65, 1536), (5000, 257)]
                for k in ("int", "rand")]


def _make_colsum(case):
    rows, cols, kind = case
    g = gen(rows * 3 + cols)
    x = torch.randint(-50, 51, (rows, cols), generator=g).float() if kind == "int" else torch.randn(rows, cols, generator=g) * rowmag(rows, g, -2, 2)
    return {"x": x, "out0": torch.full((cols,), 7.0)}


def _ref_colsum(inp, dtype=F64, mut=None):
    x = inp["x"].to(dtype)
    out = x[:-1].sum(0) if mut == "last_row_missing" else x.sum(0)
    if mut == "output_not_zeroed_first":
        out = out + inp["out0"].to(dtype)
    return (_left(out, inp["out0"], mut),)


def _scale_colsum(inp):
    return (inp["x"].to(F64).abs().sum(0) + TINY,)


_register(Op("colsum_f32", ("out",), COLSUM_CASES, _make_colsum, _ref_colsum, _scale_colsum,
             ("last_row_missing", "output_not_zeroed_first", "last_column_left")))


# ---- exact ops: no rounding freedom on exactly representable data, the GPU tests assert equality ---------------------------------------
TRANSPOSE_CASES = [(1, 1), (31, 33), (32, 32), (33, 31), (1, 1000), (1000, 1), (513, 2049)]


def _make_transpose(case):
    r, c = case
    return {"x": torch.arange(r * c, dtype=torch.float32).reshape(r, c), "y0": torch.full((c, r), -1.0)}     # distinct per element, < 2^24


def _ref_transpose(inp, dtype=F64, mut=None):
    x = inp["x"].to(dtype)
    if mut == "not_transposed":
        return (x.reshape(x.shape[1], x.shape[0]).clone(),)
    return (_left(x.t().contiguous(), inp["y0"], mut),)


_register(Op("transpose_f32", ("y",), TRANSPOSE_CASES, _make_transpose, _ref_transpose, lambda inp: (1.0,),
             ("not_transposed", "last_column_left", "last_row_left")))

# (n, form): out = a x + b y with y given, y = NULL (out = a x), and out aliasing x
AXPBY_CASES = [(n, f) for n in (1, 255, 4097) for f in ("y", "null", "alias")]


def _make_axpby(case):
    n, form = case
    g = gen(n + len(form))
    return {"x": torch.randint(-1000, 1001, (n,), generator=g).float(), "y": None if form == "null" else torch.randint(-1000, 1001, (n,), generator=g).float(),
            "a": 0.5, "b": -3.0, "alias": form == "alias", "out0": torch.full((n,), 7.0)}


def _ref_axpby(inp, dtype=F64, mut=None):
    x = inp["x"].to(dtype)
    out = inp["a"] * x
    if inp["y"] is not None:
        out = out + (inp["a"] if mut == "b_replaced_by_a" else inp["b"]) * inp["y"].to(dtype)
    elif mut == "b_replaced_by_a":
        out = out + inp["b"]
    if mut == "a_ignored":
        out = out - inp["a"] * x + x
    return (_left(out, inp["x"] if inp["alias"] else inp["out0"], mut),)


_register(Op("axpby", ("out",), AXPBY_CASES, _make_axpby, _ref_axpby, lambda inp: (1.0,), ("b_replaced_by_a", "a_ignored", "last_column_left")))

SCALE_ROWS_CASES = [(6, 63, 1), (12, 100, 6), (1026, 65, 6), (5, 512, 1), (6, 1, 6)]


def _make_scale_rows(case):
    rows, d, group = case
    g = gen(rows + d + group)
    return {"x": torch.randint(-1000, 1001, (rows, d), generator=g).float(),
            "s": 2.0 ** torch.randint(-3, 4, (rows // group,), generator=g).float() * torch.sign(torch.randn(rows // group, generator=g)), "group": group}


def _ref_scale_rows(inp, dtype=F64, mut=None):
    x, s, grp = inp["x"].to(dtype), inp["s"].to(dtype), inp["group"]
    idx = torch.arange(x.shape[0]) // grp
    if mut == "group_ignored":
        idx = torch.arange(x.shape[0]) % s.shape[0]
        if grp == 1:
            idx = idx.flip(0)
    return (_left(x * s[idx][:, None], x, mut),)


_register(Op("scale_rows", ("x",), SCALE_ROWS_CASES, _make_scale_rows, _ref_scale_rows, lambda inp: (1.0,),
             ("group_ignored", "last_row_left", "last_column_left")))

EXACT_OPS = ("transpose_f32", "axpby", "scale_rows")
#: the ops of each test file
SMALL_OPS = ("normalize_rows", "mean_groups", "mean_head_groups", "segment_mean", "layernorm")
TRAIN_OPS = ("layernorm_bwd", "attention_small_bwd", "normalize_rows_bwd", "clip_loss_bwd", "quickgelu", "adam_step", "colsum_f32",
             "transpose_f32", "axpby", "scale_rows")


def adam_walk(case, evaluate, mut=None):
    """The five-step sequence judged step by step: `evaluate(inp) -> (p, m, v, vmax)` is the implementation under test (a kernel, the
    float32 evaluation, a wrong reference); every step's reference starts from the state the implementation itself produced, so an
    error is charged to the step that made it.  Returns the worst error per output."""
    op = OPS["adam_step"]
    state, grads = adam_sequence(case)
    worst = {o: 0.0 for o in op.outs}
    for t, g in enumerate(grads, start=1):
        inp = {**state, "g": g, "step": t, "amsgrad": case[1]}
        got = [o.detach().cpu().float() for o in evaluate(inp)]
        for o, v in op.errors(inp, got).items():
            worst[o] = max(worst[o], v if v == v else float("inf"))
        state = dict(zip(("p", "m", "v", "vmax"), got))
    return worst
