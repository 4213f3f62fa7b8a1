"""References, case lists and mutations of tests/test_gpu_attention.py: vtc_attention and vtc_single_query_attention
(vtc_amd/csrc/attention.hip) through two instruments.

1. SELECTOR cases -- index arithmetic, masks, tiles and row maps, judged by EQUALITY in every dtype.  Per (row, head) a code of 64
   entries +-4; key j of a sequence is the code of its row, query i is the code of the key it targets, pi(i).  The target score is
   64 * 16 / 8 = 128, every other score 2 * (a sum of 64 signs), so the softmax is one-hot to fp32 precision and the output row is
   V[pi(i)] (V: integers 1 .. 15, strictly positive, so that nothing cancels).  TWIN keys (C[b] = C[a], pairs that straddle the
   16-key tile and 64-key chunk edges) make a query that targets `a` return (V[a] + V[b]) / 2 -- a multiple of 0.5, exact in bf16 --
   or, under the causal mask with a <= i < b, V[a] alone.  Every case is prechecked in float64 before it is used: the softmax weight
   outside the selected keys stays below 2^-30 and the reference, rounded to fp32, IS the mean of the selected V rows.

2. PARITY cases -- numerical quality, judged by  e = max |got - ref64| / scale,  scale = sum_j p_j |v_jd|  (floored at TINY): the
   project's "sum of the absolute values of the terms" (tests/primitive_refs.py).  The reference is softmax(q k^T / 8 [+ causal]) v
   in float64 on the operands as rounded to the dtype under test.  Regimes: logit standard deviation 1, 6 and 25, a common score
   offset of about +200, and V rows of magnitude 10^U(-2, 2).

A sequence is described by a Layout: rows[s, t] is the qkv row of token t of sequence s, exactly what the kernels' affine row map
(or the eot / offs arrays) must come to.  The mutations are deliberately wrong references; the CPU half of the tests proves which
instrument catches which.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

import primitive_refs as PR
from primitive_refs import F32, F64, TINY, gen

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}            # unit roundoff of the 16-bit operand formats
SENTINEL = 77.0                                       # exact in bf16 and f16
HEADS = 3

MUTATIONS = ("drop_last_key", "drop_last_tile", "causal_includes_next", "causal_excludes_self", "no_scale", "no_max_subtraction",
             "space_pstride_1", "cls_from_frame_0", "twin_not_averaged")
SQ_MUTATIONS = ("drop_last_key", "drop_last_tile", "no_scale", "no_max_subtraction", "space_pstride_1", "twin_not_averaged")


# ==== layouts ============================================================================================================================
@dataclass
class Layout:
    name: str
    rows: torch.Tensor                       # [n_seq, Lmax] int64: qkv row of token t of sequence s (t >= lens[s]: 0, masked)
    lens: torch.Tensor                       # [n_seq] int64
    n_rows: int                              # rows of the qkv buffer
    L: int                                   # the L argument of the entry point
    kw: dict = field(default_factory=dict)   # row-map arguments of ops.attention / ops.single_query_attention
    cls_out: bool = False                    # token 0 of every sequence is written to cls_out[s], not to out
    rows_pstride_1: Optional[torch.Tensor] = None      # the space map as a kernel that ignored pstride would read it
    group: int = 1                           # space map: the sequences s .. s + group - 1 of an item share token 0 (and the single query)
    heads: int = HEADS
    wrap: bool = False                       # selector cases: the twin (0, L - 1) takes precedence (twin_pairs)

    @property
    def n_seq(self) -> int:
        return self.rows.shape[0]

    @property
    def W(self) -> int:
        return self.heads * 64

    def valid(self) -> torch.Tensor:          # [n_seq, Lmax] bool
        return torch.arange(self.rows.shape[1])[None, :] < self.lens[:, None]

    def used_rows(self) -> torch.Tensor:      # [n_rows] bool: rows that belong to a sequence
        used = torch.zeros(self.n_rows, dtype=torch.bool)
        used[self.rows[self.valid()]] = True
        return used


def contiguous(L: int, n_seq: int = 5) -> Layout:
    """n_seq * heads = 15: not a multiple of the 4 waves of a workgroup."""
    rows = torch.arange(n_seq)[:, None] * L + torch.arange(L)[None, :]
    return Layout(f"L{L}", rows, torch.full((n_seq,), L), n_seq * L, L)


def time_map(F: int, B: int = 2, P: int = 5) -> Layout:
    """Sequences (b, n) over the frames t: row b T + 1 + n F + t; the cls rows b T belong to no sequence."""
    T = 1 + P * F
    s = torch.arange(B * P)
    rows = ((s // P) * T + 1 + (s % P) * F)[:, None] + torch.arange(F)[None, :]
    return Layout(f"time-F{F}", rows, torch.full((B * P,), F), B * T, F, kw=dict(s2=P, a0=1, a1=T, a2=F, a3=0, pstride=1))


def space_map(L: int, F: int = 2, B: int = 2) -> Layout:
    """Sequences (b, t): [cls row b T, patches n of frame t at rows b T + 1 + n F + t]; the cls row is shared by the item's F sequences."""
    P = L - 1
    T = 1 + P * F
    s = torch.arange(B * F)
    b, t = s // F, s % F
    tok = torch.arange(1, L)[None, :]
    rows = torch.cat([(b * T)[:, None], (b * T + 1 + t)[:, None] + (tok - 1) * F], 1)
    wrong = torch.cat([(b * T)[:, None], (b * T + 1 + t)[:, None] + (tok - 1)], 1)
    return Layout(f"space-L{L}", rows, torch.full((B * F,), L), B * T, L, kw=dict(s2=F, a0=0, a1=T, a2=0, a3=1, pstride=F), cls_out=True,
                  rows_pstride_1=wrong, group=F)


def eot_map(ctx: int, dense: bool) -> Layout:
    """The text tower's EOT query: sequence o = rows base .. eot[o], base = o ctx (dense) or offs[o] (ragged).  Lengths 1, ctx and two
    in between."""
    lens = torch.tensor([1, ctx, ctx // 3 + 1, (2 * ctx) // 3 + 2])
    offs = torch.zeros(5, dtype=torch.int64)
    offs[1:] = torch.cumsum(lens, 0)
    base = torch.arange(4) * ctx if dense else offs[:4]
    t = torch.arange(ctx)[None, :]
    rows = torch.where(t < lens[:, None], base[:, None] + t, torch.zeros_like(t))
    kw = dict(eot=(base + lens - 1).to(torch.int32), offs=None if dense else offs.to(torch.int32), ctx=ctx)
    return Layout(f"eot-ctx{ctx}-{'dense' if dense else 'ragged'}", rows, lens, 4 * ctx if dense else int(offs[-1]), 0, kw=kw)


# ==== the reference ======================================================================================================================
def gather(lay: Layout, qkv: torch.Tensor, dtype, rows: Optional[torch.Tensor] = None):
    """qkv [n_rows, 3 W] -> q, k, v [n_seq, heads, Lmax, 64] in `dtype`; tokens past a sequence's end are zeros."""
    rows = lay.rows if rows is None else rows
    t = qkv.reshape(lay.n_rows, 3, lay.heads, 64)[rows]                    # [n_seq, Lmax, 3, heads, 64]
    t = torch.where(lay.valid()[:, :, None, None, None], t, torch.zeros((), dtype=t.dtype)).to(dtype)
    q, k, v = t.permute(2, 0, 3, 1, 4)
    return q, k, v


def visible(lens: torch.Tensor, Lq: int, Lk: int, causal: bool, mut: Optional[str], k: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[n_seq, 1 | heads, Lq, Lk] bool: key j enters the softmax of query i."""
    j, i = torch.arange(Lk)[None, None, None, :], torch.arange(Lq)[None, None, :, None]
    ln = lens[:, None, None, None]
    end = ln
    if mut == "drop_last_key":
        end = torch.where(ln > 1, ln - 1, ln)
    elif mut == "drop_last_tile":
        cut = 16 * ((ln - 1) // 16)
        end = torch.where(cut > 0, cut, ln)
    vis = j < end
    if causal:
        if mut == "causal_includes_next":
            vis = vis & (j <= i + 1)
        elif mut == "causal_excludes_self":
            vis = vis & ((j < i) | ((i == 0) & (j == 0)))
        else:
            vis = vis & (j <= i)
    if mut == "twin_not_averaged":                                           # the first of two equal keys wins: later copies are dropped
        eq = (k[..., :, None, :] == k[..., None, :, :]).all(-1)               # [n_seq, heads, Lk, Lk]
        later = (eq & (torch.arange(Lk)[None, :] < torch.arange(Lk)[:, None])).any(-1)       # key j has an equal key a < j
        vis = vis & ~later[..., None, :]
    return vis


def _dot_chain(q, k, rev):
    qt, kt = q.transpose(-1, -2).contiguous(), k.transpose(-1, -2).contiguous()       # [.., 64, L]: one contiguous slice per step
    s = torch.zeros(*q.shape[:-1], k.shape[-2], dtype=q.dtype)
    for d in (reversed(range(64)) if rev else range(64)):
        s += qt[..., d, :, None] * kt[..., d, None, :]
    return s


def _pv_chain(e, v, rev):
    et = e.transpose(-1, -2).contiguous()                                            # [.., Lk, Lq]
    o, l = torch.zeros(*e.shape[:-1], 64, dtype=e.dtype), torch.zeros(*e.shape[:-1], dtype=e.dtype)
    n = e.shape[-1]
    for j in (reversed(range(n)) if rev else range(n)):
        o += et[..., j, :, None] * v[..., j, None, :]
        l += et[..., j, :]
    return o, l


def softmax_pv(q, k, v, lens, causal=False, mut=None, order="matmul", fmt=None):
    """softmax(q k^T / 8 [+ causal]) v in the dtype of q, k, v.  q [n, h, Lq, 64] (Lq = 1: the single query, never causal), k and v
    [n, h, L, 64].  `order`: "matmul" (torch's), "chain" (a sequential sum over d for the scores and over the keys for the
    normaliser and P.V, in index order) or "reverse".  `fmt` (a 16-bit torch dtype): the emulation of the all-rows kernel -- exponentials
    in float64, the normaliser summed from the unrounded exponentials, P rounded to `fmt` for P.V, fp32 for the rest.
    Returns (out, p): the output and the softmax weights."""
    Lq, Lk = q.shape[-2], k.shape[-2]
    vis = visible(lens, Lq, Lk, causal, mut, k)
    scale = 1.0 if mut == "no_scale" else 0.125
    if order == "matmul":
        s = (q @ k.transpose(-1, -2)) * scale
    else:
        s = _dot_chain(q, k, order == "reverse") * scale
    s = torch.where(vis, s, torch.full((), float("-inf"), dtype=s.dtype))
    if mut == "no_max_subtraction":                                           # exp of the raw scores in float32's range
        e = torch.exp(s.to(F32)).to(s.dtype)
    elif fmt is not None:
        e = torch.exp((s - s.amax(-1, keepdim=True)).to(F64)).to(s.dtype)
    else:
        e = torch.exp(s - s.amax(-1, keepdim=True))
    if order == "matmul":
        l = e.sum(-1)
        o = (e.to(fmt).to(e.dtype) if fmt is not None else e) @ v
    else:
        o, l = _pv_chain(e, v, order == "reverse")
    return o / l[..., None], e / l[..., None]


def scatter(lay: Layout, o_seq: torch.Tensor, mut: Optional[str] = None):
    """[n_seq, heads, L, 64] -> (out [n_rows, W] with SENTINEL on the rows nothing writes, cls_out [n_seq, W] or None)."""
    o = o_seq.permute(0, 2, 1, 3).reshape(lay.n_seq, -1, lay.W)             # [n_seq, L, W]
    out = torch.full((lay.n_rows, lay.W), SENTINEL, dtype=o.dtype)
    val = lay.valid()
    cls = None
    if lay.cls_out:
        cls = o[:, 0].clone()
        if mut == "cls_from_frame_0":
            cls = cls[(torch.arange(lay.n_seq) // lay.group) * lay.group]
        val = val.clone()
        val[:, 0] = False
    out[lay.rows[val]] = o[val]
    return out, cls


def written_rows(lay: Layout) -> torch.Tensor:
    val = lay.valid().clone()
    if lay.cls_out:
        val[:, 0] = False
    w = torch.zeros(lay.n_rows, dtype=torch.bool)
    w[lay.rows[val]] = True
    return w


def ref_attention(inp: dict, dtype=F64, mut=None, order="matmul", fmt=None):
    """vtc_attention: (out [n_rows, W], cls_out) of the case `inp` = {lay, qkv, causal}; qkv holds the operands already rounded."""
    lay = inp["lay"]
    rows = lay.rows_pstride_1 if mut == "space_pstride_1" and lay.rows_pstride_1 is not None else None
    q, k, v = gather(lay, inp["qkv"], dtype, rows)
    o, _ = softmax_pv(q, k, v, lay.lens, inp["causal"], mut, order, fmt)
    return scatter(lay, o, mut)


def scale_attention(inp: dict):
    """sum_j p_j |v_jd| per output element, in float64, laid out as the outputs are."""
    lay = inp["lay"]
    q, k, v = gather(lay, inp["qkv"], F64)
    _, p = softmax_pv(q, k, v, lay.lens, inp["causal"])
    out, cls = scatter(lay, p @ v.abs())
    return out + TINY, (cls + TINY if cls is not None else None)


def abs_v_sum(inp: dict):
    """sum_j |v_jd| over the keys a query sees (the f16 flush term), laid out as the outputs are."""
    lay = inp["lay"]
    _, _, v = gather(lay, inp["qkv"], F64)
    vis = visible(lay.lens, v.shape[-2], v.shape[-2], inp["causal"], None)
    return scatter(lay, vis.expand(-1, -1, v.shape[-2], -1).to(F64) @ v.abs())


def sq_query(inp: dict, dtype):
    lay = inp["lay"]
    q = inp["q"].to(dtype).reshape(-1, lay.heads, 1, 64)                    # [n_q, heads, 1, 64]
    return q[torch.arange(lay.n_seq) // lay.group]


def ref_single_query(inp: dict, dtype=F64, mut=None, order="matmul"):
    """vtc_single_query_attention: out [n_out, W] of the case `inp` = {lay, qkv, q}."""
    lay = inp["lay"]
    rows = lay.rows_pstride_1 if mut == "space_pstride_1" and lay.rows_pstride_1 is not None else None
    _, k, v = gather(lay, torch.nan_to_num(inp["qkv"], nan=0.0), dtype, rows)      # the Q third is NaN and never read
    o, _ = softmax_pv(sq_query(inp, dtype), k, v, lay.lens, False, mut, order)
    return o.reshape(lay.n_seq, lay.W)


def scale_single_query(inp: dict):
    lay = inp["lay"]
    _, k, v = gather(lay, torch.nan_to_num(inp["qkv"], nan=0.0), F64)
    _, p = softmax_pv(sq_query(inp, F64), k, v, lay.lens)
    return (p @ v.abs()).reshape(lay.n_seq, lay.W) + TINY


def err(got: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor, mask: Optional[torch.Tensor] = None, slack=None) -> float:
    """max (|got - ref64| - slack)+ / scale over the rows of `mask` (NaN when `got` holds a NaN there)."""
    d = (got.detach().cpu().to(F64) - ref.to(F64)).abs()
    if slack is not None:
        d = torch.where(d != d, d, (d - slack).clamp(min=0))
    d = d / scale
    if mask is not None:
        d = d[mask]
    return float("nan") if bool((d != d).any()) else float(d.max())


# ==== selector cases =====================================================================================================================
TWINS = ((15, 16), (63, 64), (79, 80), (255, 256))


def twin_pairs(L: int, wrap: bool = False) -> List[Tuple[int, int]]:
    """The pairs (a, b), b < L, and (0, L - 1), each where neither token is in a pair already (a triple's mean is no multiple of
    0.5).  `wrap`: (0, L - 1) is placed first, so that at L = 17, 65, 81 or 257 it displaces the pair that ends at L - 1."""
    pairs = []
    for a, b in (([(0, L - 1)] if wrap else []) + list(TWINS) + [(0, L - 1)]):
        if a < b < L and not {a, b} & {t for p in pairs for t in p}:
            pairs.append((a, b))
    return pairs


def _targets(L: int, causal: bool, shape, g, wrap: bool = False) -> torch.Tensor:
    """pi [*shape, L]: the key each query targets.  Random (under `causal`: <= the query), then pinned: every third query targets
    itself, every seventh key 0, the twins' `a` is targeted by a, by b and (first unpaired) by b + 1 targets b; the last query
    targets the last key or its twin; query 0 targets key 0 (the only one it sees under the mask; shared in the space map)."""
    i = torch.arange(L)
    r = torch.rand(*shape, L, generator=g)
    pi = (r * (i + 1 if causal else L)).long().clamp(max=L - 1)
    pi[..., i % 3 == 0] = i[i % 3 == 0]
    pi[..., i % 7 == 5] = 0
    pi[..., L - 1] = L - 1
    for a, b in twin_pairs(L, wrap):
        pi[..., a] = a
        pi[..., b] = a
        if b + 1 < L:
            pi[..., b + 1] = b
    pi[..., 0] = 0
    return pi


def _codes(lay: Layout, g) -> torch.Tensor:
    """[n_rows, heads, 64] of +-4, with the twins of every sequence copied in."""
    code = (torch.randint(0, 2, (lay.n_rows, lay.heads, 64), generator=g) * 8 - 4).float()
    for s in range(lay.n_seq):
        for a, b in twin_pairs(int(lay.lens[s]), lay.wrap):
            code[lay.rows[s, b]] = code[lay.rows[s, a]]
    return code


def _assemble(lay: Layout, qc, code, V) -> torch.Tensor:
    qkv = torch.stack([qc, code, V], 1).reshape(lay.n_rows, 3 * lay.W)
    qkv[~lay.used_rows()] = float("nan")                                     # rows of no sequence (time map: cls; dense eot: past the EOT) are never read
    return qkv


def selector_attention(lay: Layout, causal: bool, seed: int) -> dict:
    g = gen(seed)
    L = lay.L
    code = _codes(lay, g)
    V = torch.randint(1, 16, (lay.n_rows, lay.heads, 64), generator=g).float()
    pi = _targets(L, causal, (lay.n_seq, lay.heads), g, lay.wrap)                       # [n_seq, heads, L]
    qc = torch.full((lay.n_rows, lay.heads, 64), float("nan"))
    h = torch.arange(lay.heads)[None, :, None]
    src = lay.rows[torch.arange(lay.n_seq)[:, None, None], pi]                # [n_seq, heads, L]: the row whose code query i carries
    qc[lay.rows[:, None, :].expand_as(src), h.expand_as(src)] = code[src, h.expand_as(src)]
    return {"lay": lay, "qkv": _assemble(lay, qc, code, V), "causal": causal}


def selector_single_query(lay: Layout, seed: int) -> dict:
    """One target per (query, head): the last key, key 0, the twins and the keys on both sides of the pass edges (4 / 8 keys per
    pass) and of the per-lane slots at multiples of 64, then random ones.  In the space map the query is shared by the `group`
    sequences of an item, so token n carries one code in all of them (and a different V row in each)."""
    g = gen(seed)
    code = (torch.randint(0, 2, (lay.n_rows, lay.heads, 64), generator=g) * 8 - 4).float()
    if lay.group > 1:
        first = (torch.arange(lay.n_seq) // lay.group) * lay.group
        code[lay.rows] = code[lay.rows[first]]
    for s in range(lay.n_seq):
        for a, b in twin_pairs(int(lay.lens[s]), lay.wrap):
            code[lay.rows[s, b]] = code[lay.rows[s, a]]
    V = torch.randint(1, 16, (lay.n_rows, lay.heads, 64), generator=g).float()
    n_q = lay.n_seq // lay.group
    q = torch.empty(n_q, lay.heads, 64)
    for i in range(n_q):
        s = i * lay.group
        L = int(lay.lens[s])
        want = [L - 1, 0] + [a for a, _ in twin_pairs(L, lay.wrap)] + [t for t in (3, 4, 7, 8, 9, 63, 64, 65, 127, 128, 191, 192, 256, 319) if t < L]
        want += [int(t) for t in (torch.rand(lay.heads, generator=g) * L).long()]
        for h in range(lay.heads):
            q[i, h] = code[lay.rows[s, want[(i * lay.heads + h) % len(want)]], h]
    qkv = _assemble(lay, torch.full((lay.n_rows, lay.heads, 64), float("nan")), code, V)
    return {"lay": lay, "qkv": qkv, "q": q.reshape(n_q, lay.W)}


def selector_ideal(inp: dict):
    """The CPU precheck of a selector case and its ideal output.  In float64: the selected keys of a query are the visible keys whose
    score is exactly 128; there are one or two of them, the softmax weight outside them is below 2^-30, and the reference rounded to
    fp32 is the mean of the selected V rows -- which bf16 holds exactly.  Returns (out, cls_out) like ref_attention, or out [n_out, W]
    for a single-query case."""
    lay = inp["lay"]
    single = "q" in inp
    q, k, v = gather(lay, torch.nan_to_num(inp["qkv"], nan=0.0), F64)
    causal = inp.get("causal", False)
    if single:
        q = sq_query(inp, F64)
    vis = visible(lay.lens, q.shape[-2], k.shape[-2], causal, None)
    s = (q @ k.transpose(-1, -2)) * 0.125
    sel = (s == 128.0) & vis
    n_sel = sel.sum(-1)
    assert bool(((n_sel == 1) | (n_sel == 2)).all()), (lay.name, n_sel.unique())
    o, p = softmax_pv(q, k, v, lay.lens, causal)
    stray = float((p * ~sel).sum(-1).max())
    assert stray < 2.0 ** -30, (lay.name, stray)
    ideal = (sel.to(F64) @ v) / n_sel[..., None]
    assert torch.equal(o.float(), ideal.float()), lay.name
    assert torch.equal(ideal.bfloat16().to(F64), ideal) and torch.equal(ideal.half().to(F64), ideal)
    if single:
        return ideal.reshape(lay.n_seq, lay.W).float()
    out, cls = scatter(lay, ideal.float())
    return out, cls


SEL_SHORT = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 50, 64, 65, 77, 80)        # both edges of attn_kernel<T, 1 .. 5>
SEL_TILED = (81, 96, 97, 129, 197, 257, 272)                                  # 6, 6, 7, 9, 13, 17, 17 key tiles
SEL_SPACE = (5, 50, 197, 257)
SEL_TIME = (8, 16)
#: (kind, size, causal)
SELECTOR_CASES = ([("L", L, c) for L in SEL_SHORT + SEL_TILED for c in (False, True)] + [("wrap", 257, c) for c in (False, True)] + [("time", F, False) for F in SEL_TIME]
                  + [("space", L, False) for L in SEL_SPACE])
SQ_SELECTOR_CASES = ([("L", L) for L in (1, 7, 8, 9, 63, 64, 65, 77, 257, 320)] + [("wrap", 257)] + [("space", L) for L in (5, 50, 257)]
                     + [("eot-dense", c) for c in (77, 24)] + [("eot-ragged", c) for c in (77, 24)])


def layout_of(kind: str, size: int) -> Layout:
    if kind == "L":
        return contiguous(size)
    if kind == "wrap":                                                        # contiguous, the first-to-last twin in place of (L - 2, L - 1)
        lay = contiguous(size)
        lay.name, lay.wrap = f"wrap-L{size}", True
        return lay
    if kind == "time":
        return time_map(size)
    if kind == "space":
        return space_map(size)
    return eot_map(size, kind == "eot-dense")


def make_selector(case) -> dict:
    kind, size, causal = case
    return selector_attention(layout_of(kind, size), causal, 7 * size + 3 * len(kind) + int(causal))


def make_sq_selector(case) -> dict:
    kind, size = case
    return selector_single_query(layout_of(kind, size), 11 * size + len(kind))


# ==== parity cases =======================================================================================================================
REGIMES = ("std1", "std6", "std25", "offset", "rowmag")
#: (kind, size, causal): L = 5, 50, 197 contiguous and through the space map (cls_out), 77 and 272 causal
PARITY_LAYOUTS = (("L", 5, False), ("L", 50, False), ("L", 77, True), ("L", 197, False), ("L", 272, True),
                  ("space", 5, False), ("space", 50, False), ("space", 197, False))
PARITY_CASES = [(r,) + l for r in REGIMES for l in PARITY_LAYOUTS]
SQ_PARITY_LAYOUTS = (("L", 5), ("L", 50), ("L", 77), ("L", 197), ("L", 272), ("space", 5), ("space", 50), ("space", 197),
                     ("eot-ragged", 77))
SQ_PARITY_CASES = [(r,) + l for r in REGIMES for l in SQ_PARITY_LAYOUTS]


def _regime_data(regime: str, lay: Layout, n_q_rows: int, g):
    """q [n_q_rows, heads, 64], k, v [n_rows, heads, 64] in fp32.  A score is q . k / 8: with q, k ~ a N(0, 1) its standard deviation
    is a^2.  "offset": q and k share the component 5 in every dimension, 64 * 25 / 8 = 200 on every score (and +-5 per key on top).
    One twin key per sequence (token L // 2 repeats token 0) gives `twin_not_averaged` something to drop."""
    a = {"std6": 6.0 ** 0.5, "std25": 5.0}.get(regime, 1.0)
    q = torch.randn(n_q_rows, lay.heads, 64, generator=g) * a
    k = torch.randn(lay.n_rows, lay.heads, 64, generator=g) * a
    v = torch.randn(lay.n_rows, lay.heads, 64, generator=g)
    if regime == "offset":
        q, k = q + 5.0, k + 5.0
    if regime == "rowmag":
        v = v * PR.rowmag(lay.n_rows, g, -2, 2)[:, :, None]
    for s in range(lay.n_seq):
        n = int(lay.lens[s])
        if n >= 2:
            k[lay.rows[s, n // 2]] = k[lay.rows[s, 0]]
    return q, k, v


def _seed(case) -> int:
    return sum(ord(c) for c in str(case))


def make_parity(case, fmt: str) -> dict:
    """The qkv buffer of a vtc_attention parity case, ROUNDED to the operand format `fmt` and held in fp32."""
    regime, kind, size, causal = case
    lay = layout_of(kind, size)
    q, k, v = _regime_data(regime, lay, lay.n_rows, gen(_seed(case)))
    qkv = torch.stack([q, k, v], 1).reshape(lay.n_rows, 3 * lay.W)
    return {"lay": lay, "qkv": qkv.to(DTYPES[fmt]).float(), "causal": causal}


def make_sq_parity(case, fmt: str) -> dict:
    regime, kind, size = case
    lay = layout_of(kind, size)
    n_q = lay.n_seq // lay.group
    q, k, v = _regime_data(regime, lay, n_q, gen(_seed(case)))
    qkv = torch.stack([torch.full_like(k, float("nan")), k, v], 1).reshape(lay.n_rows, 3 * lay.W)
    return {"lay": lay, "qkv": qkv.to(DTYPES[fmt]).float(), "q": q.reshape(n_q, lay.W).to(DTYPES[fmt]).float()}


ORDERS = ("matmul", "chain", "reverse")


def parity_errors(inp: dict, got, fmt: Optional[str] = None) -> Dict[str, float]:
    """e of (out, cls_out) against the float64 reference, on the rows a sequence writes.  `fmt` = "f16": the absolute term
    2^-24 sum_j |v_jd| (P flushed below the half subnormal range) is taken off the difference first."""
    lay = inp["lay"]
    if "_ref" not in inp:                                                     # computed once per case, left unchanged
        inp["_ref"] = (ref_attention(inp), scale_attention(inp), abs_v_sum(inp))
    ref, sc, av = inp["_ref"]
    slack = [2.0 ** -24 * t if t is not None else None for t in av] if fmt == "f16" else (None, None)
    e = {"out": err(got[0], ref[0], sc[0], written_rows(lay), slack[0])}
    if lay.cls_out:
        e["cls_out"] = err(got[1], ref[1], sc[1], None, slack[1])
    return e


def sq_parity_error(inp: dict, got) -> float:
    if "_ref" not in inp:
        inp["_ref"] = (ref_single_query(inp), scale_single_query(inp))
    return err(got, *inp["_ref"])


def calibrate(regime: str) -> Dict[str, float]:
    """Worst e of the float32 evaluation of the regime's cases, on one thread, over the three operand roundings and the three
    summation orders: {"attention": ..., "single_query": ...}."""
    worst = {"attention": 0.0, "single_query": 0.0}
    with PR.single_thread():
        for fmt in DTYPES:
            for case in PARITY_CASES:
                if case[0] == regime:
                    inp = make_parity(case, fmt)
                    for order in ORDERS:
                        e = parity_errors(inp, ref_attention(inp, F32, order=order))
                        worst["attention"] = max(worst["attention"], *e.values())
            for case in SQ_PARITY_CASES:
                if case[0] == regime:
                    inp = make_sq_parity(case, fmt)
                    for order in ORDERS:
                        worst["single_query"] = max(worst["single_query"], sq_parity_error(inp, ref_single_query(inp, F32, order=order)))
    return worst


def bound16(fmt: str, tol32: float, output: str) -> float:
    """The derived bound of the 16-bit all-rows kernel: P rounded to the operand format (<= u scale), the normaliser summed from
    the unrounded exponentials (nothing), the output rounded once (<= u scale; cls_out is fp32: nothing), the fp32 arithmetic
    around them (tol32)."""
    return (2 if output == "out" else 1) * U[fmt] + tol32


# ==== the inputs of the attention tests of tests/test_gpu_primitives.py, rebuilt on the CPU ================================================
def old_test_inputs():
    """(name, fmt, absolute tolerance, inp) of test_attention_contiguous, test_attention_long_sequences_tiled and
    test_attention_short_and_off_grid_lengths as tests/test_gpu_primitives.py draws them (randn, one absolute tolerance per dtype)."""
    out = []

    def add(name, fmt, tol, L, n_seq, heads, causal, seed, mul=1.0):
        lay = contiguous(L, n_seq)
        lay.heads = heads
        qkv = (torch.randn(n_seq * L, 3 * heads * 64, generator=gen(seed)) * mul).to(DTYPES[fmt]).float()
        out.append((f"{name}-L{L}", fmt, tol, {"lay": lay, "qkv": qkv, "causal": causal}))

    for fmt, tol in (("f32", 1e-5), ("bf16", 2e-2)):
        for L, causal in ((6, False), (8, False), (16, False), (24, True), (50, False), (77, True)):
            add("contiguous", fmt, tol, L, 5, 3, causal, L)
    for fmt, tol in (("f32", 2e-5), ("bf16", 2e-2), ("f16", 2e-2)):
        for L, causal in ((81, False), (96, True), (129, True), (197, False), (257, False), (272, True)):
            add("tiled", fmt, tol, L, 3, 2, causal, L, 1.5)
    for fmt, tol in (("f32", 1e-5), ("bf16", 2e-2), ("f16", 3e-3)):
        for causal in (False, True):
            for L in (1, 2, 3, 4, 5, 7, 9, 17, 33, 49, 64, 65, 80):
                add("short", fmt, tol, L, 5, 3, causal, 1000 + L)
    return out
