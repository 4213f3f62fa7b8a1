"""Thin torch-tensor wrappers over the C ABI (include/vtc_hip.h).

torch is used for device memory and the current HIP stream only; every
computation below happens in libvtc_hip.so.  Inputs must live on a ROCm GPU.
"""
from __future__ import annotations

import ctypes as C
import functools
import numbers
from typing import Optional, Sequence

import torch

from . import _lib as L

_TDT = {torch.float32: L.VTC_F32, torch.bfloat16: L.VTC_BF16, torch.float16: L.VTC_F16}


def _stream() -> int:
    """The current HIP stream of the CURRENT device -- call inside an ``on_device`` wrapper, which makes the
    tensors' device current first."""
    return torch.cuda.current_stream().cuda_stream


def on_device(fn):
    """Every launch goes to the current stream of the device its tensors live on: the wrapper checks that all GPU
    tensor arguments share one device and makes it current for the call (the reference's entry points run on
    ``cuda:<-d>``, evaluation/eval.py:196, without that device being the current one)."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        dev = None
        for a in args + tuple(kwargs.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if dev is None:
                    dev = a.device
                elif a.device != dev:
                    raise RuntimeError(f"vtc_amd.{fn.__name__}: tensors on different devices ({dev} and {a.device})")
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapped


def _gpu(t: torch.Tensor, dtype=None, name="tensor") -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"vtc_amd: {name} must be on the GPU (got {t.device}); this package has no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"vtc_amd: {name} must be {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def dtype_code(dtype) -> int:
    if isinstance(dtype, int):
        return dtype
    return _TDT[dtype]


def torch_dtype(code: int):
    return {L.VTC_BF16: torch.bfloat16, L.VTC_F16: torch.float16}.get(code, torch.float32)


def workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _ws_for(ws: Optional[torch.Tensor], need: int, device) -> torch.Tensor:
    """The caller's workspace when it is large enough and on ``device``, else a fresh one."""
    return ws if ws is not None and ws.numel() >= need and ws.device == device else workspace(need, device)


def _k_array(k_vals: Sequence[int]):
    """The k values as the C ABI's ``const int *``."""
    return (C.c_int * len(k_vals))(*[int(k) for k in k_vals])


# ---- primitives ---------------------------------------------------------------------------
@on_device
def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = L.EPI_STORE,
         out: Optional[torch.Tensor] = None, out_dtype=None, skip_mod: int = 0) -> torch.Tensor:
    """out[M,N] = epi(a[M,K] @ w[N,K]^T + bias).  a, w: fp32 or bf16 (same dtype)."""
    a, w = _gpu(a, name="a"), _gpu(w, a.dtype, "w")
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K
    if bias is not None:
        bias = _gpu(bias, torch.float32, "bias")
    if epilogue == L.EPI_RESID:
        assert out is not None and out.dtype == torch.float32 and out.is_contiguous()
    elif out is None:
        out = torch.empty(M, N, dtype=out_dtype or a.dtype, device=a.device)
    L.check(L.lib().vtc_gemm(a.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, out.data_ptr(),
                             M, N, K, _TDT[a.dtype], epilogue, _TDT[out.dtype], skip_mod, _stream()), "vtc_gemm")
    return out


@on_device
def gemm_resid_layernorm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, ln_g: torch.Tensor,
                         ln_b: torch.Tensor, skip_mod: int = 0, ln_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out (fp32, in place) += a @ w^T + bias; returns LayerNorm(out) * ln_g + ln_b in a's dtype -- one launch."""
    a, w = _gpu(a, name="a"), _gpu(w, a.dtype, "w")
    M, K = a.shape
    N = w.shape[0]
    assert out.dtype == torch.float32 and out.shape == (M, N) and out.is_contiguous()
    lib = L.lib()
    if not lib.vtc_gemm_resid_layernorm_supported(M, N, K, _TDT[a.dtype]):
        raise ValueError(f"gemm_resid_layernorm: unsupported problem M={M} N={N} K={K} {a.dtype}")
    if ln_out is None:
        ln_out = torch.empty(M, N, dtype=a.dtype, device=a.device)
    ws = workspace(lib.vtc_gemm_resid_layernorm_workspace_bytes(M), a.device)
    L.check(lib.vtc_gemm_resid_layernorm(a.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, out.data_ptr(), M, N, K,
                                         _TDT[a.dtype], skip_mod, _gpu(ln_g, torch.float32).data_ptr(), _gpu(ln_b, torch.float32).data_ptr(),
                                         ln_out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "vtc_gemm_resid_layernorm")
    return ln_out


@on_device
def layernorm(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, out_dtype=torch.float32, rows: Optional[int] = None,
              row_index: Optional[torch.Tensor] = None, row_mul: int = 1) -> torch.Tensor:
    x = _gpu(x, torch.float32, "x")
    width = x.shape[-1]
    n = rows if rows is not None else (row_index.numel() if row_index is not None else x.numel() // width)
    y = torch.empty(n, width, dtype=out_dtype, device=x.device)
    ri = _gpu(row_index, torch.int32, "row_index").data_ptr() if row_index is not None else None
    L.check(L.lib().vtc_layernorm(x.data_ptr(), _gpu(g, torch.float32).data_ptr(), _gpu(b, torch.float32).data_ptr(),
                                  y.data_ptr(), n, width, _TDT[out_dtype], ri, row_mul, _stream()), "vtc_layernorm")
    return y


@on_device
def attention(qkv: torch.Tensor, n_seq: int, L_: int, heads: int, causal: bool = False, s2: int = 1, a0: int = 0,
              a1: Optional[int] = None, a2: int = 0, a3: int = 0, pstride: int = 1, cls_out: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    qkv = _gpu(qkv, name="qkv")
    rows, w3 = qkv.shape
    W = w3 // 3
    assert W == heads * 64
    if a1 is None:
        a1 = L_
    if out is None:
        out = torch.zeros(rows, W, dtype=qkv.dtype, device=qkv.device)
    L.check(L.lib().vtc_attention(qkv.data_ptr(), out.data_ptr(), cls_out.data_ptr() if cls_out is not None else None,
                                  n_seq, L_, heads, int(causal), s2, a0, a1, a2, a3, pstride, _TDT[qkv.dtype], _stream()),
            "vtc_attention")
    return out


@on_device
def single_query_attention(qkv: torch.Tensor, q: torch.Tensor, n_out: int, L_: int, heads: int, s2: int = 1, a0: int = 0,
                           a1: Optional[int] = None, a2: int = 0, a3: int = 0, pstride: int = 1, eot: Optional[torch.Tensor] = None,
                           offs: Optional[torch.Tensor] = None, ctx: int = 0) -> torch.Tensor:
    """One query per sequence over the keys / values of a packed qkv buffer (same row map as ``attention``; or, with ``eot``, the
    text tower's rows base .. eot[o]) -> [n_out, W] fp32.  The last block of a tower: only the output row asks."""
    qkv, q = _gpu(qkv, name="qkv"), _gpu(q, qkv.dtype, "q")
    W = qkv.shape[1] // 3
    assert W == heads * 64 and q.shape[1] == W
    if a1 is None:
        a1 = L_
    out = torch.empty(n_out, W, dtype=torch.float32, device=qkv.device)
    eot_p = _gpu(eot, torch.int32, "eot").data_ptr() if eot is not None else None
    offs_p = _gpu(offs, torch.int32, "offs").data_ptr() if offs is not None else None
    L.check(L.lib().vtc_single_query_attention(qkv.data_ptr(), q.data_ptr(), out.data_ptr(), n_out, L_, heads, s2, a0, a1, a2, a3, pstride,
                                               eot_p, offs_p, ctx, _TDT[qkv.dtype], _stream()), "vtc_single_query_attention")
    return out


# ---- frame preprocessing --------------------------------------------------------------------
_RESIZE_PLANS: dict = {}     # (device, in_h, in_w, size) -> the plan in device memory (int32)


def _resize_plan(in_h: int, in_w: int, size: int, device) -> torch.Tensor:
    key = (device, in_h, in_w, size)
    plan = _RESIZE_PLANS.get(key)
    if plan is None:
        lib = L.lib()
        nbytes = lib.vtc_resize_plan_bytes(in_h, in_w, size)
        host = torch.empty(max(nbytes, 4) // 4, dtype=torch.int32)
        L.check(lib.vtc_resize_plan(in_h, in_w, size, host.data_ptr(), nbytes), "vtc_resize_plan")
        if len(_RESIZE_PLANS) >= 256:        # a dataset has a handful of frame sizes; do not grow without bound on adversarial input
            _RESIZE_PLANS.clear()
        plan = _RESIZE_PLANS[key] = host.to(device)
    return plan


def clip_resize_crop(frames: torch.Tensor, size: int = 224, layout: str = "hwc", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Resize(size, BICUBIC) + CenterCrop(size) of CLIP_TRANSFORM (dataset_loaders/dataset_loaders.py:40-49) on decoded RGB uint8 frames,
    bit for bit what torchvision gives on PIL images (vtc_resize_crop_u8).  frames: [..., H, W, 3] (layout "hwc", what decoders deliver) or
    [..., 3, H, W] ("chw") with zero, one or two leading dimensions (n, or batch x frames), uint8 on the GPU; returns [..., 3, size, size]
    uint8, what the towers' uint8 pixel path takes.  ``out``: a contiguous uint8 tensor of that shape, 16-byte aligned.  Bad arguments
    raise ValueError before anything is launched; plans are cached per (H, W, size) and device."""
    if layout not in ("hwc", "chw"):
        raise ValueError(f"clip_resize_crop: layout {layout!r} (\"hwc\" or \"chw\")")
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        raise ValueError(f"clip_resize_crop: uint8 frames expected, got {getattr(frames, 'dtype', type(frames))}")
    if frames.dim() not in (3, 4, 5):
        raise ValueError(f"clip_resize_crop: frames of rank 3, 4 or 5 expected ([..., H, W, 3] or [..., 3, H, W]), got {tuple(frames.shape)}")
    lead = tuple(frames.shape[:-3])
    ch, (in_h, in_w) = (frames.shape[-1], frames.shape[-3:-1]) if layout == "hwc" else (frames.shape[-3], frames.shape[-2:])
    if ch != 3:
        raise ValueError(f"clip_resize_crop: 3 channels expected in layout {layout!r}, got shape {tuple(frames.shape)}")
    size = int(size)
    if size <= 0 or size % 16 or L.lib().vtc_resize_plan_bytes(int(in_h), int(in_w), size) == 0:
        raise ValueError(f"clip_resize_crop: size={size} must be a positive multiple of 16 (at most 1024) and the frame edges "
                         f"({in_h} x {in_w}) within [1, 8192]")
    n = 1
    for d in lead:
        n *= int(d)
    if n < 1:
        raise ValueError(f"clip_resize_crop: no frames in shape {tuple(frames.shape)}")
    if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != lead + (3, size, size) or not out.is_contiguous()
                            or out.device != frames.device or out.data_ptr() % 16):
        raise ValueError(f"clip_resize_crop: out must be a contiguous, 16-byte aligned uint8 tensor of shape {lead + (3, size, size)} on {frames.device}")
    return _clip_resize_crop(frames, n, int(in_h), int(in_w), size, 0 if layout == "hwc" else 1, lead, out)


@on_device
def _clip_resize_crop(frames, n, in_h, in_w, size, layout, lead, out):
    frames = _gpu(frames, torch.uint8, "frames")
    plan = _resize_plan(in_h, in_w, size, frames.device)
    if out is None:
        out = torch.empty(lead + (3, size, size), dtype=torch.uint8, device=frames.device)
    L.check(L.lib().vtc_resize_crop_u8(frames.data_ptr(), n, in_h, in_w, layout, plan.data_ptr(), size, out.data_ptr(), _stream()),
            "vtc_resize_crop_u8")
    return out


# ---- wrapper-level fp32 ops ---------------------------------------------------------------
@on_device
def normalize_rows(x: torch.Tensor) -> torch.Tensor:
    x = _gpu(x, torch.float32, "x")
    out = torch.empty_like(x)
    L.check(L.lib().vtc_normalize_rows(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], _stream()), "vtc_normalize_rows")
    return out


@on_device
def mean_groups(x: torch.Tensor, group: int) -> torch.Tensor:
    x = _gpu(x, torch.float32, "x")
    n, d = x.shape
    assert n % group == 0
    out = torch.empty(n // group, d, dtype=torch.float32, device=x.device)
    L.check(L.lib().vtc_mean_groups(x.data_ptr(), out.data_ptr(), n // group, group, d, _stream()), "vtc_mean_groups")
    return out


@on_device
def mean_head_groups(a: torch.Tensor, b: torch.Tensor, group: int) -> torch.Tensor:
    """out[g] = (a[g] + sum_k b[g * group + k]) / (1 + group)   (model/model.py:357-362)."""
    a, b = _gpu(a, torch.float32, "a"), _gpu(b, torch.float32, "b")
    n, d = a.shape
    assert b.shape == (n * group, d)
    out = torch.empty(n, d, dtype=torch.float32, device=a.device)
    L.check(L.lib().vtc_mean_head_groups(a.data_ptr(), b.data_ptr(), out.data_ptr(), n, group, d, _stream()), "vtc_mean_head_groups")
    return out


@on_device
def pack_tokens(tokens: torch.Tensor, offsets: torch.Tensor, ctx: int = 77, sot: int = 49406, eot: int = 49407) -> torch.Tensor:
    """[n_seq, ctx] int64 ids = [sot] + tokens[offsets[s]:offsets[s+1]] + [eot], zero padded; truncated to ctx - 1 ids + eot
    (dataset_loaders/dataset_loaders.py:224-248).  tokens int32 [total], offsets int32 [n_seq + 1], both on the GPU."""
    tokens, offsets = _gpu(tokens, torch.int32, "tokens"), _gpu(offsets, torch.int32, "offsets")
    n = offsets.numel() - 1
    ids = torch.empty(n, ctx, dtype=torch.int64, device=offsets.device)
    L.check(L.lib().vtc_pack_tokens(tokens.data_ptr(), offsets.data_ptr(), n, ctx, sot, eot, ids.data_ptr(), _stream()), "vtc_pack_tokens")
    return ids


@on_device
def segment_mean(x: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """Mean of rows [offsets[g], offsets[g+1]) per group g (int32 offsets on the GPU)."""
    x = _gpu(x, torch.float32, "x")
    offsets = _gpu(offsets, torch.int32, "offsets")
    n = offsets.numel() - 1
    out = torch.empty(n, x.shape[1], dtype=torch.float32, device=x.device)
    L.check(L.lib().vtc_segment_mean(x.data_ptr(), offsets.data_ptr(), out.data_ptr(), n, x.shape[1], _stream()), "vtc_segment_mean")
    return out


@on_device
def normalize_rows2(x: torch.Tensor, y: torch.Tensor, flag: Optional[torch.Tensor] = None):
    """(x / |x|, y / |y|) row-wise in ONE launch; flag (int32, device) |= 1 / 2 when x / y hold a NaN or inf."""
    x, y = _gpu(x, torch.float32, "x"), _gpu(y, torch.float32, "y")
    assert x.dim() == 2 and y.dim() == 2 and x.shape[1] == y.shape[1]
    ox, oy = torch.empty_like(x), torch.empty_like(y)
    L.check(L.lib().vtc_normalize_rows2(x.data_ptr(), ox.data_ptr(), x.shape[0], y.data_ptr(), oy.data_ptr(), y.shape[0], x.shape[1],
                                        flag.data_ptr() if flag is not None else None, _stream()), "vtc_normalize_rows2")
    return ox, oy


def nonfinite_flag2(a: torch.Tensor, b: torch.Tensor, flag: torch.Tensor) -> torch.Tensor:
    """flag[0] |= 1 when ``a`` holds a NaN / inf, |= 2 when ``b`` does (one launch, no synchronisation).  flag: int32 (or the low word of
    an int64) in device memory."""
    a, b = _gpu(a, torch.float32, "embeddings"), _gpu(b, torch.float32, "embeddings")
    with torch.cuda.device(a.device):
        L.check(L.lib().vtc_nonfinite_flag2(a.data_ptr(), a.numel(), b.data_ptr(), b.numel(), flag.data_ptr(), _stream()), "vtc_nonfinite_flag2")
    return flag


def nonfinite_bits(a: torch.Tensor, b: torch.Tensor) -> int:
    """Synchronous form: the flag word on the host (one 4-byte D2H)."""
    a = _gpu(a, torch.float32, "embeddings")
    return int(nonfinite_flag2(a, b, torch.zeros(1, dtype=torch.int32, device=a.device)).item())


@on_device
def similarity(v: torch.Tensor, t: torch.Tensor, logit_scale: torch.Tensor) -> torch.Tensor:
    v, t = _gpu(v, torch.float32, "v"), _gpu(t, torch.float32, "t")
    ls = _gpu(logit_scale.detach().reshape(1), torch.float32, "logit_scale")
    sim = torch.empty(v.shape[0], t.shape[0], dtype=torch.float32, device=v.device)
    L.check(L.lib().vtc_similarity(v.data_ptr(), t.data_ptr(), v.shape[0], t.shape[0], v.shape[1], ls.data_ptr(),
                                   sim.data_ptr(), _stream()), "vtc_similarity")
    return sim


@on_device
def clip_loss(sim: torch.Tensor) -> torch.Tensor:
    sim = _gpu(sim, torch.float32, "sim")
    n = sim.shape[0]
    assert sim.shape == (n, n)
    ws = workspace(L.lib().vtc_clip_loss_workspace_bytes(n), sim.device)
    loss = torch.empty((), dtype=torch.float32, device=sim.device)
    L.check(L.lib().vtc_clip_loss(sim.data_ptr(), n, loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "vtc_clip_loss")
    return loss


# ---- sweep --------------------------------------------------------------------------------
@on_device
def l2_topk(gallery: torch.Tensor, queries: torch.Tensor, depth: int, precision: int = L.SWEEP_EXACT,
            rows_per_block: int = 0, return_dists: bool = True, ws: Optional[torch.Tensor] = None):
    gallery, queries = _gpu(gallery, torch.float32, "gallery"), _gpu(queries, torch.float32, "queries")
    ng, d = gallery.shape
    nq = queries.shape[0]
    ws = _ws_for(ws, L.lib().vtc_l2_topk_workspace_bytes(ng, nq, d, precision, rows_per_block), gallery.device)
    ids = torch.empty(nq, depth, dtype=torch.int64, device=gallery.device)
    dists = torch.empty(nq, depth, dtype=torch.float32, device=gallery.device) if return_dists else None
    L.check(L.lib().vtc_l2_topk(gallery.data_ptr(), queries.data_ptr(), ng, nq, d, depth, precision, rows_per_block,
                                ids.data_ptr(), dists.data_ptr() if dists is not None else None, ws.data_ptr(), ws.numel(),
                                _stream()), "vtc_l2_topk")
    return ids, dists


@on_device
def l2_topk_bidir(a: torch.Tensor, b: torch.Tensor, depth: int, precision: int = L.SWEEP_EXACT, rows_per_block: int = 0,
                  return_dists: bool = True, ws: Optional[torch.Tensor] = None):
    """Both directions from one distance matrix: (ids_b2a [n_b, depth], dists_b2a, ids_a2b [n_a, depth], dists_a2b),
    where ids_b2a = l2_topk(gallery=a, queries=b) and ids_a2b = l2_topk(gallery=b, queries=a)."""
    a, b = _gpu(a, torch.float32, "a"), _gpu(b, torch.float32, "b")
    na, d = a.shape
    nb = b.shape[0]
    ws = _ws_for(ws, L.lib().vtc_l2_topk_bidir_workspace_bytes(na, nb, d, precision, rows_per_block), a.device)
    ids1 = torch.empty(nb, depth, dtype=torch.int64, device=a.device)
    ids2 = torch.empty(na, depth, dtype=torch.int64, device=a.device)
    d1 = torch.empty(nb, depth, dtype=torch.float32, device=a.device) if return_dists else None
    d2 = torch.empty(na, depth, dtype=torch.float32, device=a.device) if return_dists else None
    L.check(L.lib().vtc_l2_topk_bidir(a.data_ptr(), b.data_ptr(), na, nb, d, depth, precision, rows_per_block,
                                      ids1.data_ptr(), d1.data_ptr() if d1 is not None else None,
                                      ids2.data_ptr(), d2.data_ptr() if d2 is not None else None,
                                      ws.data_ptr(), ws.numel(), _stream()), "vtc_l2_topk_bidir")
    return ids1, d1, ids2, d2


SEARCH_MAX_QUERIES = 64       # vtc_l2_search's limit; more queries go through l2_topk


Q8_TAIL = 16                  # bytes of a q8 row behind its codes: the fp32 scale and 12 bytes of zero padding (include/vtc_hip.h)


def _search_gallery(gallery: torch.Tensor) -> torch.Tensor:
    """The gallery of a query-time search: fp32, IEEE half (vtc_l2_search_half) or q8 rows (``torch.int8`` [n, d + 16]: d codes, the fp32
    scale, 12 bytes of padding -- ``quantize_rows_q8``; the *_q8 entries); every other dtype raises TypeError."""
    gallery = _gpu(gallery, None, "gallery")
    if gallery.dtype not in (torch.float32, torch.float16, torch.int8):
        raise TypeError(f"vtc_amd: gallery must be torch.float32, torch.float16 or torch.int8 (q8 rows), got {gallery.dtype}")
    if gallery.dtype == torch.int8 and (gallery.dim() != 2 or gallery.shape[1] <= Q8_TAIL or gallery.data_ptr() % 16):
        raise ValueError(f"vtc_amd: a torch.int8 gallery is q8 rows [n, d + {Q8_TAIL}] with a 16-byte aligned base, got {tuple(gallery.shape)}")
    return gallery


def _gallery_shape(gallery: torch.Tensor):
    """(rows, columns) of a search gallery: a q8 row is its d codes and ``Q8_TAIL`` more bytes."""
    ng, d = gallery.shape
    return ng, d - Q8_TAIL if gallery.dtype == torch.int8 else d


@on_device
def quantize_rows_q8(x: torch.Tensor, nonfinite: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 rows [n, d] (d a multiple of 64 in [64, 2048]) -> q8 rows, ``torch.int8`` [n, d + 16] (vtc_quantize_rows_q8, one launch): d signed
    codes, the row's fp32 scale at byte d, 12 zero bytes.  In fp32 arithmetic, per row: m = max |x_k|; s = fl32(m / 127) rounded UP to 16
    significant bits (1 for a row of zeros); code_k = clamp(rint(fl32(x_k / s)), -127, 127), ties to even -- so s * code is exact in fp32
    and |x_k - s code_k| <= 0.5 (1 + 2^-15) s.  A row with a NaN / inf gets a NaN scale and codes of 0 and ORs 1 into ``nonfinite`` (a
    device int32 [1], optional).  Every search takes the result as its gallery and searches it AS STORED: ``dequantize_rows_q8`` gives the
    fp32 rows whose search it is, bit for bit.  n = 0 gives an empty [0, d + 16].  Only enqueued."""
    x = _gpu(x, torch.float32, "x")
    if x.dim() != 2 or x.shape[1] < 64 or x.shape[1] % 64:
        raise ValueError(f"quantize_rows_q8: x must be [n, d] with d a multiple of 64, got {tuple(x.shape)}")
    n, d = x.shape
    rows = torch.empty(n, d + Q8_TAIL, dtype=torch.int8, device=x.device)
    if nonfinite is not None:
        nonfinite = _gpu(nonfinite, torch.int32, "nonfinite")
    if n:
        L.check(L.lib().vtc_quantize_rows_q8(x.data_ptr(), n, d, rows.data_ptr(), _ptr(nonfinite), _stream()), "vtc_quantize_rows_q8")
    return rows


def q8_scales(rows: torch.Tensor) -> torch.Tensor:
    """The fp32 scales [n] of q8 rows [n, d + 16] (a copy)."""
    d = rows.shape[1] - Q8_TAIL
    return rows[:, d:d + 4].contiguous().view(torch.float32).reshape(-1)


def dequantize_rows_q8(rows: torch.Tensor) -> torch.Tensor:
    """q8 rows [n, d + 16] -> the fp32 rows [n, d] they store: fl32(scale * code), one IEEE multiply per component (exact for the
    quantiser's 16-bit scales).  A torch expression."""
    if rows.dtype != torch.int8 or rows.dim() != 2 or rows.shape[1] <= Q8_TAIL:
        raise ValueError(f"dequantize_rows_q8: q8 rows are torch.int8 [n, d + {Q8_TAIL}], got {rows.dtype} {tuple(rows.shape)}")
    return rows[:, :rows.shape[1] - Q8_TAIL].float() * q8_scales(rows)[:, None]


def q8_rows(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """int8 codes [n, d] and fp32 scales [n] -> q8 rows [n, d + 16] with a zero tail, bit for bit (no rounding, no check)."""
    n, d = codes.shape
    rows = torch.zeros(n, d + Q8_TAIL, dtype=torch.int8, device=codes.device)
    rows[:, :d] = codes
    rows[:, d:d + 4] = scales.to(device=codes.device, dtype=torch.float32).contiguous().view(torch.int8).view(n, 4)
    return rows


def _search_inputs(what, gallery, queries, groups=None, rows=None):
    """What every search entry opens with: the gallery (fp32 or half), the queries as fp32 with the gallery's column count and, where the
    call has one, its ``groups`` (int32, one per gallery row) or ``rows`` (int64, one per query) on the gallery's device.  Returns
    (gallery, queries, that vector or None, n_gallery, n_queries, d); ``what`` names the caller in every message."""
    gallery, queries = _search_gallery(gallery), _gpu(queries, torch.float32, "queries")
    ng, d = _gallery_shape(gallery)
    nq = queries.shape[0]
    vec = groups if rows is None else rows
    if vec is not None:
        name, dtype, n, one = ("groups", torch.int32, ng, "one id per gallery row") if rows is None else ("rows", torch.int64, nq, "one per query")
        vec = _gpu(vec, dtype, name)
    if queries.shape[1] != d:
        raise ValueError(f"{what}: gallery rows have {d} columns, queries {queries.shape[1]}")
    if vec is not None and (vec.device != gallery.device or tuple(vec.shape) != (n,)):
        raise ValueError(f"{what}: {name} must be {str(dtype)[6:]} [{n}] on {gallery.device} ({one}), got {tuple(vec.shape)} on {vec.device}")
    return gallery, queries, vec, ng, nq, d


def _exclude_arg(exclude, nq, device, what):
    """The excluded keys of an excluding search: an int64 [Q] tensor on the gallery's device, anything else raises ValueError."""
    if not isinstance(exclude, torch.Tensor) or exclude.dtype != torch.int64 or tuple(exclude.shape) != (nq,) or exclude.device != device:
        got = f"{exclude.dtype} {tuple(exclude.shape)} on {exclude.device}" if isinstance(exclude, torch.Tensor) else type(exclude).__name__
        raise ValueError(f"{what}: exclude must be an int64 [{nq}] tensor on {device} (one row or group per query), got {got}")
    return exclude.contiguous()


def _after_arg(after, nq, device, what):
    """The cursor of a search: (float64 [Q], int64 [Q]) on the gallery's device, anything else raises ValueError."""
    ok = isinstance(after, (tuple, list)) and len(after) == 2 and all(isinstance(t, torch.Tensor) for t in after)
    if ok:
        ok = (after[0].dtype == torch.float64 and after[1].dtype == torch.int64 and
              all(t.device == device and tuple(t.shape) == (nq,) for t in after))
    if not ok:
        got = ", ".join(f"{t.dtype} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
                        for t in (after if isinstance(after, (tuple, list)) else (after,)))
        raise ValueError(f"{what}: after must be (float64 [{nq}], int64 [{nq}]) on {device}, got ({got})")
    return after[0].contiguous(), after[1].contiguous()


def _live_arg(live, ng, device, what):
    """The row mask of a search: packed int32 words [ceil(n / 32)] on the gallery's device, or None."""
    if live is None:
        return None
    live = _gpu(live, torch.int32, "live")
    if live.device != device or tuple(live.shape) != ((ng + 31) // 32,):
        raise ValueError(f"{what}: live must be int32 [{(ng + 31) // 32}] on {device} (one bit per gallery row), got "
                         f"{tuple(live.shape)} on {live.device}")
    return live


def _search_ws_arg(ws, need, device, what):
    """The workspace of a search: a fresh one, or the caller's -- never a silent fresh one then: the caller reads the fp64 list out of the
    tensor it passed."""
    if ws is None:
        return workspace(need, device)
    if need and (ws.numel() < need or ws.device != device):
        raise ValueError(f"{what}: the workspace passed holds {ws.numel()} bytes on {ws.device}, the call needs {need} on {device}")
    return ws


def _search_outputs(nq, depth, device, return_dists, grouped):
    """(ids, groups or None, dists or None, nonfinite bits) of a search, to be filled by the library."""
    ids = torch.empty(nq, depth, dtype=torch.int64, device=device)
    out_groups = torch.empty(nq, depth, dtype=torch.int32, device=device) if grouped else None
    dists = torch.empty(nq, depth, dtype=torch.float32, device=device) if return_dists else None
    return ids, out_groups, dists, torch.zeros(1, dtype=torch.int32, device=device)


def _ptr(t):
    return t.data_ptr() if t is not None else None


@on_device
def l2_search(gallery: torch.Tensor, queries: torch.Tensor, depth: int, id_base: int = 0, return_dists: bool = True,
              ws: Optional[torch.Tensor] = None, live: Optional[torch.Tensor] = None, after=None, exclude: Optional[torch.Tensor] = None):
    """Query-time search (vtc_l2_search): the exact ``depth`` nearest gallery rows of at most 64 queries, by the fp64 squared distances of
    the fp32 rows, ties to the lower row.  Returns (ids [Q, depth] int64 = id_base + row, -1 where fewer rows have a finite distance;
    dists [Q, depth] fp32 or None; nonfinite_bits, a device int32 [1]: 1 = the gallery holds a NaN / inf, 2 = the queries do).  With a
    caller's ``ws`` of at least ``l2_search_workspace_bytes`` the fp64 distances of the result are ``search_dists64(ws, Q, depth)``.
    ``live`` (vtc_l2_search_masked): packed int32 words [ceil(n / 32)] on the gallery's device (``row_mask_pack``), row j takes part iff bit
    j & 31 of word j >> 5 is set.  The result is that of the search over the live rows alone, with their original row numbers; a dead
    row is neither read nor counted in nonfinite_bits.  ``depth`` is still bounded by the physical row count.
    A ``torch.float16`` gallery (vtc_l2_search_half) is searched as stored: the distances are the fp64 ones of the fp32 queries and the
    half rows widened to fp32, which is exact -- every output, the fp64 distances in ``ws`` included, has the bits of this call over
    ``gallery.float()``.  A ``torch.int8`` gallery [n, d + 16] is q8 rows (``quantize_rows_q8``; vtc_l2_search_q8), searched as stored
    likewise: the bits of this call over ``dequantize_rows_q8(gallery)``, in every mode below.  The queries stay fp32; any other gallery
    dtype raises TypeError.
    ``after`` (vtc_l2_search_after): a cursor per query, ``(after_d64 [Q] float64, after_ids [Q] int64)`` on the gallery's device; only
    the rows whose key (fp64 distance, id_base + row) lies strictly after it are returned -- the next page of a search whose previous
    page ended in that key.  ``after_d64`` must carry the bits the scan forms: ``search_dists64(ws, Q, depth)[:, -1]`` of the previous
    page (cloned: the next call overwrites it) or ``l2_pair_dists64``; -inf is the plain search, +inf / NaN an empty row.  The cursor
    row need not be live; with ``id_base`` the ids are global, so every window of a gallery takes the same cursor.  None: the call
    above, unchanged.
    ``exclude`` (vtc_l2_search_excluding): int64 [Q] on the gallery's device; query q is never given the row with the GLOBAL id
    ``exclude[q]`` -- the search order with that row deleted, then cut.  -1, or any id outside [id_base, id_base + n), excludes nothing.
    It composes with ``live``, a half gallery and ``after`` (the cursor may stand on the excluded row).  A wrong dtype, shape or device
    raises ValueError.  None: the call above, unchanged."""
    gallery, queries, _, ng, nq, d = _search_inputs("l2_search", gallery, queries)
    after_d, after_i = _after_arg(after, nq, gallery.device, "l2_search") if after is not None else (None, None)
    if exclude is not None:
        exclude = _exclude_arg(exclude, nq, gallery.device, "l2_search")
    live = _live_arg(live, ng, gallery.device, "l2_search")
    lib = L.lib()
    ws = _search_ws_arg(ws, lib.vtc_l2_search_workspace_bytes(ng, nq, d, depth), gallery.device, "l2_search")
    ids, _, dists, bits = _search_outputs(nq, depth, gallery.device, return_dists, grouped=False)
    half = int(gallery.dtype == torch.float16)
    shape = (ng, nq, d, depth, int(id_base), ids.data_ptr())
    tail = (_ptr(dists), bits.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    # The narrowest entry that takes the call.  A ladder on purpose: a table of (condition, entry, arguments) forms every entry's
    # arguments at every call, 2 us of host time on a 50 us call.
    if gallery.dtype == torch.int8:
        L.check(lib.vtc_l2_search_q8(gallery.data_ptr(), queries.data_ptr(), _ptr(live), None, 0, None, _ptr(exclude), _ptr(after_d), _ptr(after_i),
                                     *shape, None, *tail), "vtc_l2_search_q8")
    elif exclude is not None:
        L.check(lib.vtc_l2_search_excluding(gallery.data_ptr(), half, queries.data_ptr(), _ptr(live), None, exclude.data_ptr(), _ptr(after_d),
                                            _ptr(after_i), *shape, None, *tail), "vtc_l2_search_excluding")
    elif after is not None:
        L.check(lib.vtc_l2_search_after(gallery.data_ptr(), half, queries.data_ptr(), _ptr(live), after_d.data_ptr(), after_i.data_ptr(), *shape,
                                        *tail), "vtc_l2_search_after")
    elif half:
        L.check(lib.vtc_l2_search_half(gallery.data_ptr(), queries.data_ptr(), _ptr(live), None, *shape, None, *tail), "vtc_l2_search_half")
    elif live is None:
        L.check(lib.vtc_l2_search(gallery.data_ptr(), queries.data_ptr(), *shape, *tail), "vtc_l2_search")
    else:
        L.check(lib.vtc_l2_search_masked(gallery.data_ptr(), queries.data_ptr(), live.data_ptr(), *shape, *tail), "vtc_l2_search_masked")
    return ids, dists, bits


SEARCH_MANY_MAX_DEPTH = 32    # vtc_l2_search_many_half's limit: 21 spare ranks in a lane-per-entry candidate list


@on_device
def l2_search_many(gallery_half: torch.Tensor, queries: torch.Tensor, depth: int, id_base: int = 0, live: Optional[torch.Tensor] = None,
                   return_dists: bool = True, ws: Optional[torch.Tensor] = None, nonfinite: Optional[torch.Tensor] = None):
    """``l2_search`` of a ``torch.float16`` gallery for MANY queries (vtc_l2_search_many_half): at most 64 queries, depth <= 32, the same
    (ids, dists or None, nonfinite_bits) with the same bits -- the fp64 distances ``search_dists64(ws, Q, depth)`` of a caller's ``ws``
    (at least ``l2_search_many_workspace_bytes``) included -- by ONE pass of the gallery through the matrix cores and an exact fp64 finish
    instead of a scan per 8 queries.  ``live``: ``l2_search``'s mask.  ``nonfinite``: the int32 [1] device word the bits are ORed into
    (None: a fresh zero word).  ``search_many_stats(ws, Q, depth)`` tells how many queries needed the exact fallback scan.  An fp32
    gallery raises ValueError: the pass multiplies the stored half rows as they are.  Only enqueued."""
    gallery, queries, _, ng, nq, d = _search_inputs("l2_search_many", gallery_half, queries)
    if gallery.dtype != torch.float16:
        raise ValueError(f"l2_search_many: the gallery must be torch.float16 (the stored rows are the matrix cores' operand), got {gallery.dtype}")
    live = _live_arg(live, ng, gallery.device, "l2_search_many")
    lib = L.lib()
    ws = _search_ws_arg(ws, lib.vtc_l2_search_many_workspace_bytes(ng, nq, d, depth), gallery.device, "l2_search_many")
    ids, _, dists, bits = _search_outputs(nq, depth, gallery.device, return_dists, grouped=False)
    if nonfinite is not None:
        bits = _gpu(nonfinite, torch.int32, "nonfinite")
    L.check(lib.vtc_l2_search_many_half(gallery.data_ptr(), queries.data_ptr(), _ptr(live), ng, nq, d, depth, int(id_base), ids.data_ptr(),
                                        _ptr(dists), bits.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "vtc_l2_search_many_half")
    return ids, dists, bits


def l2_search_many_workspace_bytes(n_gallery: int, n_queries: int, d: int, depth: int) -> int:
    """0 for a shape vtc_l2_search_many_half refuses."""
    return int(L.lib().vtc_l2_search_many_workspace_bytes(int(n_gallery), int(n_queries), int(d), int(depth)))


def search_many_stats(ws: torch.Tensor, n_queries: int, depth: int) -> dict:
    """What the last ``l2_search_many`` on workspace ``ws`` left behind its fp64 head (include/vtc_hip.h): ``fallback_queries``, the
    queries of that call that the error bound could not certify and the exact fallback scan finished.  A device-to-host read."""
    at = (n_queries * depth * 8 + 255) // 256 * 256
    return {"fallback_queries": int(ws[at:at + 4].view(torch.int32).item())}


@on_device
def row_mask_pack(flags: torch.Tensor, and_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row flags (uint8 or bool [n], non-zero = the row takes part) -> the int32 words [ceil(n / 32)] l2_search's ``live`` takes
    (vtc_row_mask_pack): bit b of word w is flags[32 w + b], ANDed with ``and_mask`` (words of the same layout) when given; the bits past
    n are 0.  One launch."""
    if flags.dtype == torch.bool:
        flags = flags.view(torch.uint8) if flags.is_contiguous() else flags.contiguous().view(torch.uint8)
    flags = _gpu(flags, torch.uint8, "flags")
    if flags.dim() != 1 or flags.shape[0] < 1:
        raise ValueError(f"row_mask_pack: flags must be [n] with n >= 1, got {tuple(flags.shape)}")
    n = flags.shape[0]
    if and_mask is not None:
        and_mask = _gpu(and_mask, torch.int32, "and_mask")
        if and_mask.device != flags.device or tuple(and_mask.shape) != ((n + 31) // 32,):
            raise ValueError(f"row_mask_pack: and_mask must be int32 [{(n + 31) // 32}] on {flags.device}, got {tuple(and_mask.shape)} on "
                             f"{and_mask.device}")
    words = torch.empty((n + 31) // 32, dtype=torch.int32, device=flags.device)
    L.check(L.lib().vtc_row_mask_pack(flags.data_ptr(), n, and_mask.data_ptr() if and_mask is not None else None, words.data_ptr(), _stream()),
            "vtc_row_mask_pack")
    return words


@on_device
def l2_pair_dists64(gallery: torch.Tensor, queries: torch.Tensor, rows: torch.Tensor, id_base: int = 0) -> torch.Tensor:
    """float64 [Q] on the device (vtc_l2_pair_dists64): the fp64 squared distance of query q and the gallery row ``rows[q] - id_base``,
    one pair per query, with the bits ``l2_search`` leaves in its workspace for that pair -- what ``l2_search(after=...)`` takes as the
    cursor's distance when only the cursor's id is at hand.  ``rows``: int64 [Q]; -1, or any id outside [id_base, id_base + n), gives
    +inf and reads nothing.  The row is read whether or not any mask calls it live.  fp32, ``torch.float16`` or q8 gallery; any Q >= 1."""
    gallery, queries, rows, ng, nq, d = _search_inputs("l2_pair_dists64", gallery, queries, rows=rows)
    out = torch.empty(nq, dtype=torch.float64, device=gallery.device)
    if gallery.dtype == torch.int8:
        L.check(L.lib().vtc_l2_pair_dists64_q8(gallery.data_ptr(), queries.data_ptr(), rows.data_ptr(), ng, nq, d, int(id_base), out.data_ptr(),
                                               _stream()), "vtc_l2_pair_dists64_q8")
        return out
    L.check(L.lib().vtc_l2_pair_dists64(gallery.data_ptr(), int(gallery.dtype == torch.float16), queries.data_ptr(), rows.data_ptr(), ng, nq, d,
                                        int(id_base), out.data_ptr(), _stream()), "vtc_l2_pair_dists64")
    return out


def l2_search_workspace_bytes(n_gallery: int, n_queries: int, d: int, depth: int) -> int:
    """0 for a shape vtc_l2_search refuses."""
    return int(L.lib().vtc_l2_search_workspace_bytes(int(n_gallery), int(n_queries), int(d), int(depth)))


def search_dists64(ws: torch.Tensor, n_queries: int, depth: int) -> torch.Tensor:
    """The fp64 distances [Q, depth] of the last l2_search that ran in ``ws`` (a view of the workspace's head: the next call overwrites it)."""
    return ws[:n_queries * depth * 8].view(torch.float64).view(n_queries, depth)


def l2_range_workspace_bytes(n_gallery: int, n_queries: int, d: int) -> int:
    """0 for a shape vtc_l2_range_count / vtc_l2_range_fill refuse."""
    return int(L.lib().vtc_l2_range_workspace_bytes(int(n_gallery), int(n_queries), int(d)))


def range_hit_words(ws: torch.Tensor, n_gallery: int, n_queries: int) -> torch.Tensor:
    """The hit words [Q, ceil(n / 32)] int32 of the last l2_range_count that ran in ``ws`` (a view of the workspace's head: the next call
    overwrites it).  Row q is ``row_mask_pack``'s format: a valid ``live`` of l2_search."""
    nw = (n_gallery + 31) // 32
    return ws[:n_queries * nw * 4].view(torch.int32).view(n_queries, nw)


def _range_args(gallery, queries, radius2, live, ws, what, many=False):
    """``many``: the call is the many-query count pass -- a half gallery, and the larger workspace."""
    gallery, queries, _, ng, nq, d = _search_inputs(what, gallery, queries)
    if many and gallery.dtype != torch.float16:
        raise ValueError(f"{what}: the gallery must be torch.float16 (the stored rows are the matrix cores' operand), got {gallery.dtype}")
    if isinstance(radius2, torch.Tensor) and radius2.is_cuda:
        radius2 = _gpu(radius2, torch.float64, "radius2")
    elif isinstance(radius2, (int, float)):
        radius2 = torch.full((nq,), float(radius2), dtype=torch.float64, device=gallery.device)      # a fill launch: no copy, no sync
    else:
        # host values: through pinned memory and an asynchronous copy, so that the count pass stays free of host syncs
        radius2 = torch.as_tensor(radius2, dtype=torch.float64).reshape(-1).pin_memory().to(gallery.device, non_blocking=True)
    if radius2.device != gallery.device or tuple(radius2.shape) != (nq,):
        raise ValueError(f"{what}: radius2 must be a float or float64 [{nq}] (one squared radius per query), got {tuple(radius2.shape)}")
    live = _live_arg(live, ng, gallery.device, what)
    ws_bytes = L.lib().vtc_l2_range_many_workspace_bytes if many else L.lib().vtc_l2_range_workspace_bytes
    ws = _search_ws_arg(ws, ws_bytes(ng, nq, d), gallery.device, what)      # the hit words stay in it
    return gallery, queries, radius2, live, ws


def _range_count(gallery, queries, radius2, live, ws, many=False):
    ng, d = _gallery_shape(gallery)
    nq = queries.shape[0]
    lims = torch.empty(nq + 1, dtype=torch.int64, device=gallery.device)
    bits = torch.zeros(1, dtype=torch.int32, device=gallery.device)
    tail = (_ptr(live), radius2.data_ptr(), ng, nq, d, lims.data_ptr(), bits.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    if many:
        L.check(L.lib().vtc_l2_range_count_many_half(gallery.data_ptr(), queries.data_ptr(), *tail), "vtc_l2_range_count_many_half")
    elif gallery.dtype == torch.int8:
        L.check(L.lib().vtc_l2_range_count_q8(gallery.data_ptr(), queries.data_ptr(), *tail), "vtc_l2_range_count_q8")
    else:
        L.check(L.lib().vtc_l2_range_count(gallery.data_ptr(), int(gallery.dtype == torch.float16), queries.data_ptr(), *tail),
                "vtc_l2_range_count")
    return lims, bits


@on_device
def l2_range_count(gallery: torch.Tensor, queries: torch.Tensor, radius2, live: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
                   return_bits: bool = False):
    """Range search, the count pass alone (vtc_l2_range_count): ``lims`` int64 [Q + 1] on the device, lims[0] = 0 and lims[q + 1] - lims[q]
    the number of gallery rows with a finite fp64 squared distance D <= radius2[q] to query q (at most 64 queries).  Only enqueued: no
    host sync.  ``radius2``: a float, or float64 [Q].  ``live``: packed row mask as ``l2_search`` takes it.  A ``torch.float16`` gallery
    and a q8 one (``torch.int8`` [n, d + 16]) are searched as stored.  With a caller's ``ws`` (``l2_range_workspace_bytes``) the hit words are ``range_hit_words(ws, n, Q)``.
    ``return_bits``: also the non-finite word (device int32 [1]: 1 = a live gallery row holds a NaN / inf, 2 = a query does)."""
    gallery, queries, radius2, live, ws = _range_args(gallery, queries, radius2, live, ws, "l2_range_count")
    lims, bits = _range_count(gallery, queries, radius2, live, ws)
    return (lims, bits) if return_bits else lims


@on_device
def l2_range_search(gallery: torch.Tensor, queries: torch.Tensor, radius2, live: Optional[torch.Tensor] = None, id_base: int = 0,
                    max_results: int = 1 << 22, return_dists64: bool = False, return_words: bool = False, ws: Optional[torch.Tensor] = None,
                    exclude: Optional[torch.Tensor] = None):
    """Range search (vtc_l2_range_count + vtc_l2_range_fill): EVERY gallery row with a finite fp64 squared distance D <= radius2[q] to
    query q, for at most 64 queries.  Returns (lims int64 [Q + 1], ids int64 [total] = id_base + row, dists fp32 [total] = (float) D
    [, dists64 float64 [total]] [, words int32 [Q, ceil(n / 32)]]), all on the device: query q's hits are [lims[q], lims[q + 1]), in
    ascending row order.  ``words`` are the hit words, a copy; words[q] is a valid ``live`` of ``l2_search``.
    ONE host sync: lims[-1] is read back between the two passes, because the size of the output depends on the data.  A total above
    ``max_results`` raises ValueError BEFORE anything is allocated for it (``l2_range_count`` tells the size without fetching).
    ``radius2`` / ``live`` / a ``torch.float16`` gallery: as ``l2_range_count``.
    ``exclude``: int64 [Q] on the gallery's device; query q is never given the row with the GLOBAL id ``exclude[q]`` (-1, or any id
    outside [id_base, id_base + n), excludes nothing).  Whether that row is a hit is read from the hit words and comes back in the SAME
    host read as lims[-1]; the entry is dropped after the fill with torch ops and lims counts what is returned.  ``words`` stay the count
    pass's, the excluded row's bit included.  None: the call above, unchanged."""
    return _range_search(gallery, queries, radius2, live, id_base, max_results, return_dists64, return_words, ws, exclude, "l2_range_search",
                         False)


def _range_search(gallery, queries, radius2, live, id_base, max_results, return_dists64, return_words, ws, exclude, what, many):
    """The count pass (``many``: vtc_l2_range_count_many_half), the one host read of lims[-1], then vtc_l2_range_fill on the same workspace."""
    gallery, queries, radius2, live, ws = _range_args(gallery, queries, radius2, live, ws, what, many)
    ng, d = _gallery_shape(gallery)
    nq = queries.shape[0]
    if exclude is not None:
        exclude = _exclude_arg(exclude, nq, gallery.device, what)
    lims, _ = _range_count(gallery, queries, radius2, live, ws, many)
    n_self = 0
    if exclude is None:
        total = int(lims[-1])                                 # the one device-to-host read
    else:                                                     # ... which also says how many queries hit their excluded row: its bit
        row = exclude - int(id_base)
        at = row.clamp(0, ng - 1)
        word = range_hit_words(ws, ng, nq)[torch.arange(nq, device=gallery.device), at >> 5]
        self_hit = (row >= 0) & (row < ng) & (((word >> (at & 31).to(torch.int32)) & 1) != 0)
        total, n_self = torch.stack([lims[-1], self_hit.sum()]).tolist()
    if total - n_self > int(max_results):
        raise ValueError(f"{what}: {total - n_self} rows lie within the radius, max_results={int(max_results)} (raise it, tighten the radius, "
                         f"or count with {'l2_range_count_many' if many else 'l2_range_count'})")
    dev = gallery.device
    ids = torch.empty(total, dtype=torch.int64, device=dev)
    dists = torch.empty(total, dtype=torch.float32, device=dev)
    dists64 = torch.empty(total, dtype=torch.float64, device=dev) if return_dists64 else None
    fill = (queries.data_ptr(), ng, nq, d, lims.data_ptr(), total, int(id_base), ids.data_ptr(), dists.data_ptr(),
            dists64.data_ptr() if return_dists64 else None, ws.data_ptr(), ws.numel(), _stream())
    if gallery.dtype == torch.int8:
        L.check(L.lib().vtc_l2_range_fill_q8(gallery.data_ptr(), *fill), "vtc_l2_range_fill_q8")
    else:
        L.check(L.lib().vtc_l2_range_fill(gallery.data_ptr(), int(gallery.dtype == torch.float16), *fill), "vtc_l2_range_fill")
    if exclude is not None and total:
        # The excluded entries leave: every kept entry moves to its rank among the kept ones, the dropped ones to a spare slot behind
        # the result.  The sizes are host numbers already, so nothing here reads the device.
        seg = torch.repeat_interleave(torch.arange(nq, device=dev), lims[1:] - lims[:-1], output_size=total)
        keep = ids != exclude[seg]
        dest = torch.where(keep, torch.cumsum(keep, 0) - 1, total - n_self)

        def kept(x):
            out = x.new_empty(total - n_self + 1)
            out[dest] = x
            return out[:total - n_self]
        ids, dists, dists64 = kept(ids), kept(dists), kept(dists64) if return_dists64 else None
        lims = lims - torch.nn.functional.pad(torch.cumsum(self_hit, 0), (1, 0))
    out = (lims, ids, dists)
    if return_dists64:
        out += (dists64,)
    if return_words:
        out += (range_hit_words(ws, ng, nq).clone(),)
    return out


@on_device
def l2_range_count_many(gallery_half: torch.Tensor, queries: torch.Tensor, radius2, live: Optional[torch.Tensor] = None,
                        ws: Optional[torch.Tensor] = None, return_bits: bool = False):
    """``l2_range_count`` of a ``torch.float16`` gallery for MANY queries (vtc_l2_range_count_many_half): at most 64 queries, the same
    ``lims`` (and non-finite word) with the same bits, the same hit words ``range_hit_words(ws, n, Q)`` in a caller's ``ws`` (at least
    ``l2_range_many_workspace_bytes``) -- by ONE pass of the gallery through the matrix cores, only the pairs the error bound cannot decide
    taken in fp64, instead of an fp64 scan per 8 queries.  ``range_many_stats(ws, n, Q)`` tells how many pairs that were.  An fp32 gallery
    raises ValueError: the pass multiplies the stored half rows as they are.  Only enqueued."""
    gallery, queries, radius2, live, ws = _range_args(gallery_half, queries, radius2, live, ws, "l2_range_count_many", many=True)
    lims, bits = _range_count(gallery, queries, radius2, live, ws, many=True)
    return (lims, bits) if return_bits else lims


@on_device
def l2_range_search_many(gallery_half: torch.Tensor, queries: torch.Tensor, radius2, live: Optional[torch.Tensor] = None, id_base: int = 0,
                         max_results: int = 1 << 22, return_dists64: bool = False, return_words: bool = False,
                         ws: Optional[torch.Tensor] = None, exclude: Optional[torch.Tensor] = None):
    """``l2_range_search`` of a ``torch.float16`` gallery for MANY queries: ``l2_range_count_many``'s pass, the one host read of lims[-1],
    then vtc_l2_range_fill on the same workspace.  The arguments and the returns are ``l2_range_search``'s, bit for bit; ``ws`` is at least
    ``l2_range_many_workspace_bytes``.  An fp32 gallery raises ValueError."""
    return _range_search(gallery_half, queries, radius2, live, id_base, max_results, return_dists64, return_words, ws, exclude,
                         "l2_range_search_many", True)


def l2_range_many_workspace_bytes(n_gallery: int, n_queries: int, d: int) -> int:
    """0 for a shape vtc_l2_range_count_many_half refuses; never less than ``l2_range_workspace_bytes``."""
    return int(L.lib().vtc_l2_range_many_workspace_bytes(int(n_gallery), int(n_queries), int(d)))


def range_many_stats(ws: torch.Tensor, n_gallery: int, n_queries: int, d: int = None) -> dict:
    """What the last ``l2_range_count_many`` / ``l2_range_search_many`` on workspace ``ws`` left behind the scan's regions
    (include/vtc_hip.h): ``exact_pairs``, the (query, row) pairs of that call that the error bound could not decide and the fp64
    distance did.  The counter is the last region of the workspace the call asked for, so ``d`` is needed only to find it in a LARGER
    ``ws`` (None: ``ws`` is exactly ``l2_range_many_workspace_bytes`` long).  A device-to-host read."""
    if d is None:
        at = ws.numel() - 256
    else:
        at = l2_range_workspace_bytes(n_gallery, n_queries, d) + (n_queries + 15) // 16 * 64 * d + 768
    return {"exact_pairs": int(ws[at:at + 8].view(torch.int64).item())}


@on_device
def l2_search_part(gallery: torch.Tensor, queries: torch.Tensor, depth: int, id_base: int = 0, live: Optional[torch.Tensor] = None,
                   after=None, exclude: Optional[torch.Tensor] = None):
    """One window's share of a search over several: (ids [Q, depth] int64, dists64 [Q, depth] fp64, nonfinite_bits) -- what
    l2_search_merge takes.  ``depth`` is capped at the window's rows by the caller (a window may hold fewer rows than the merged list).
    ``live``: the window's own packed row mask (bit 0 of word 0 is the window's first row), as l2_search takes it.  The window may be
    fp32 or ``torch.float16``; the fp64 lists do not depend on how the rows are stored, so l2_search_merge takes both.
    ``after``: the cursor of l2_search in GLOBAL ids, the same pair for every window -- the merged lists are then the page after it.
    ``exclude``: the excluded rows of l2_search in GLOBAL ids, the same tensor for every window -- the merged lists then exclude them."""
    ng, d = _gallery_shape(gallery)
    nq = queries.shape[0]
    ws = workspace(l2_search_workspace_bytes(ng, nq, d, depth), gallery.device)
    ids, _, bits = l2_search(gallery, queries, depth, id_base, return_dists=False, ws=ws, live=live, after=after, exclude=exclude)
    return ids, search_dists64(ws, nq, depth), bits


@on_device
def l2_search_merge(ids_parts: torch.Tensor, dists64_parts: torch.Tensor, return_dists: bool = True):
    """The lists of searches over disjoint gallery windows -> the list of their union (vtc_l2_search_merge).  ids_parts [P, Q, depth] int64
    and dists64_parts [P, Q, depth] fp64 (l2_search_part's outputs, stacked; entries with id -1 are ignored); returns (ids [Q, depth],
    dists fp32 or None): the first ``depth`` by (distance, id)."""
    return _search_merge("l2_search_merge", return_dists, ids_parts, dists64_parts)


def _search_merge(what, return_dists, *stacks):
    """The body of both merges (the entry vtc_<what>): the stacks checked, the outputs allocated, the one library call.  A third stack,
    the groups, makes it the grouped merge, with a groups output between ids and dists."""
    kinds = (("ids_parts", torch.int64), ("dists64_parts", torch.float64), ("groups_parts", torch.int32))
    parts = [_gpu(t, dtype, name) for t, (name, dtype) in zip(stacks, kinds)]
    grouped = len(parts) == 3
    if parts[0].dim() != 3 or any(p.shape != parts[0].shape for p in parts[1:]):
        shapes = [str(tuple(p.shape)) for p in parts]
        raise ValueError(f"{what}: [parts, queries, depth] lists expected, got {', '.join(shapes[:-1])} and {shapes[-1]}")
    n_parts, nq, depth = parts[0].shape
    dev = parts[0].device
    outs = (torch.empty(nq, depth, dtype=torch.int64, device=dev),) + ((torch.empty(nq, depth, dtype=torch.int32, device=dev),) if grouped else ())
    dists = torch.empty(nq, depth, dtype=torch.float32, device=dev) if return_dists else None
    L.check(getattr(L.lib(), "vtc_" + what)(*[p.data_ptr() for p in parts], n_parts, nq, depth, *[o.data_ptr() for o in outs], _ptr(dists),
                                            _stream()), "vtc_" + what)
    return (*outs, dists)


def _n_groups_arg(n_groups, what):
    if isinstance(n_groups, bool) or not isinstance(n_groups, numbers.Integral) or not 1 <= n_groups < 2 ** 31:
        raise ValueError(f"{what}: a cursor needs n_groups, an int in [1, 2^31) with every group id in [0, n_groups), got {n_groups!r}")
    return int(n_groups)


def _ban_arg(ban, nq, n_groups, device, what):
    """The bitmap of banned groups: int32 [Q, ceil(n_groups / 32)] on the gallery's device, contiguous; anything else raises ValueError."""
    words = (n_groups + 31) // 32
    if (not isinstance(ban, torch.Tensor) or ban.dtype != torch.int32 or tuple(ban.shape) != (nq, words) or ban.device != device or
            not ban.is_contiguous()):
        got = f"{ban.dtype} {tuple(ban.shape)} on {ban.device}" if isinstance(ban, torch.Tensor) else type(ban).__name__
        raise ValueError(f"{what}: ban must be a contiguous int32 [{nq}, {words}] tensor on {device} (one bit per query and group), got {got}")
    return ban


@on_device
def l2_group_mark_before(gallery: torch.Tensor, queries: torch.Tensor, groups: torch.Tensor, n_groups: int, after,
                         live: Optional[torch.Tensor] = None, id_base: int = 0, ban: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The mark pass of a page of the grouped search (vtc_l2_group_mark_before): sets bit g of ``ban[q]`` for every group g that has a
    live row with a finite distance AT OR BEFORE query q's cursor ``after = (after_d64 [Q] float64, after_ids [Q] int64)`` -- the groups
    ``l2_search_grouped(after=...)`` must not return again.  ``groups``: int32 [n] with DENSE ids in [0, n_groups); a row whose group is
    outside the range marks nothing.  ``ban``: int32 [Q, ceil(n_groups / 32)] on the gallery's device, bit g & 31 of word g >> 5; None
    allocates and zeroes one, a given one is ORed into in place (the windows of one gallery mark into the same buffer, with their
    ``id_base``).  Returns ``ban``.  One gallery pass per tile of queries, only enqueued; fp32, ``torch.float16`` or q8 gallery.  Wrong
    dtypes, shapes or devices raise ValueError."""
    gallery, queries, groups, ng, nq, d = _search_inputs("l2_group_mark_before", gallery, queries, groups)
    n_groups = _n_groups_arg(n_groups, "l2_group_mark_before")
    after_d, after_i = _after_arg(after, nq, gallery.device, "l2_group_mark_before")
    live = _live_arg(live, ng, gallery.device, "l2_group_mark_before")
    if ban is None:
        ban = torch.zeros(nq, (n_groups + 31) // 32, dtype=torch.int32, device=gallery.device)
    else:
        ban = _ban_arg(ban, nq, n_groups, gallery.device, "l2_group_mark_before")
    if gallery.dtype == torch.int8:
        L.check(L.lib().vtc_l2_group_mark_before_q8(gallery.data_ptr(), queries.data_ptr(), _ptr(live), groups.data_ptr(), n_groups,
                                                    after_d.data_ptr(), after_i.data_ptr(), ng, nq, d, int(id_base), ban.data_ptr(), _stream()),
                "vtc_l2_group_mark_before_q8")
        return ban
    L.check(L.lib().vtc_l2_group_mark_before(gallery.data_ptr(), int(gallery.dtype == torch.float16), queries.data_ptr(),
                                             _ptr(live), groups.data_ptr(), n_groups, after_d.data_ptr(),
                                             after_i.data_ptr(), ng, nq, d, int(id_base), ban.data_ptr(), _stream()),
            "vtc_l2_group_mark_before")
    return ban


@on_device
def l2_search_grouped(gallery: torch.Tensor, queries: torch.Tensor, groups: torch.Tensor, depth: int, id_base: int = 0,
                      return_dists: bool = True, ws: Optional[torch.Tensor] = None, live: Optional[torch.Tensor] = None,
                      exclude: Optional[torch.Tensor] = None, after=None, n_groups: Optional[int] = None, ban: Optional[torch.Tensor] = None):
    """The grouped query-time search (vtc_l2_search_grouped): every gallery row belongs to the group ``groups[j]`` (int32 [n], ANY values,
    rows of a group anywhere), and of the complete (distance, row)-sorted list of the live rows with a finite distance only the FIRST row
    of every group stays; the first ``depth`` of those are the result -- the ``depth`` nearest distinct groups, each by its nearest row.
    Returns (ids [Q, depth] int64 = id_base + that row, -1 where fewer groups have a finite distance; groups [Q, depth] int32, -1 there
    too -- read ``ids`` to tell an empty entry, -1 is a legal group id; dists fp32 or None; nonfinite_bits as l2_search).  ``live`` and
    ``ws`` as in l2_search, the workspace being ``l2_search_grouped_workspace_bytes``; its head holds the fp64 distances.  A
    ``torch.float16`` gallery is searched as stored (vtc_l2_search_half), with the bits of this call over ``gallery.float()``; a q8 one
    (``torch.int8`` [n, d + 16], vtc_l2_search_q8) with the bits of this call over ``dequantize_rows_q8(gallery)``.
    ``exclude`` (vtc_l2_search_excluding): int64 [Q] on the gallery's device; query q is never given a row of the GROUP ``exclude[q]`` --
    the grouped search of the gallery without that group's rows.  A value outside int32 is no group and excludes nothing (-1 is a legal
    group).  A wrong dtype, shape or device raises ValueError.  None: the call above, unchanged.
    ``after`` (vtc_l2_search_grouped_after): a cursor per query as in l2_search, ``(after_d64 [Q] float64, after_ids [Q] int64)``; the
    result is the next page of the grouped order -- the first ``depth`` groups whose NEAREST admissible row's key (fp64 distance,
    id_base + row) lies strictly after the cursor.  ``n_groups`` is then required and the groups must be DENSE, in [0, n_groups): a
    bitmap of groups decides which are already behind the cursor, and a row whose group is outside the range is never returned.  With
    ``ban=None`` the call zeroes such a bitmap and runs the mark pass itself (``l2_group_mark_before``): the stateless call, two gallery
    passes.  A given ``ban`` (int32 [Q, ceil(n_groups / 32)]) is taken as it is -- the windows of one gallery are all marked into one
    buffer BEFORE any of them is scanned, and a caller may carry bits forward.  ``exclude`` composes with the cursor (the cursor may
    stand on a row of the excluded group).  -inf is the plain grouped search, +inf / NaN an empty row.  ``after=None``: the call above,
    argument for argument (``n_groups`` and ``ban`` are then not looked at)."""
    gallery, queries, groups, ng, nq, d = _search_inputs("l2_search_grouped", gallery, queries, groups)
    live = _live_arg(live, ng, gallery.device, "l2_search_grouped")
    lib = L.lib()
    ws = _search_ws_arg(ws, lib.vtc_l2_search_grouped_workspace_bytes(ng, nq, d, depth), gallery.device, "l2_search_grouped")
    ids, out_groups, dists, bits = _search_outputs(nq, depth, gallery.device, return_dists, grouped=True)
    half = int(gallery.dtype == torch.float16)
    head = (queries.data_ptr(), _ptr(live), groups.data_ptr())
    tail = (ng, nq, d, depth, int(id_base), ids.data_ptr(), out_groups.data_ptr(), _ptr(dists), bits.data_ptr(), ws.data_ptr(), ws.numel(),
            _stream())
    if exclude is not None:
        exclude = _exclude_arg(exclude, nq, gallery.device, "l2_search_grouped")
    after_d = after_i = None
    if after is not None:                                      # the narrowest entry that takes the call: a ladder, as in l2_search
        after_d, after_i = _after_arg(after, nq, gallery.device, "l2_search_grouped")
        n_groups = _n_groups_arg(n_groups, "l2_search_grouped")
        if ban is None:
            ban = l2_group_mark_before(gallery, queries, groups, n_groups, (after_d, after_i), live=live, id_base=id_base)
        else:
            ban = _ban_arg(ban, nq, n_groups, gallery.device, "l2_search_grouped")
    if gallery.dtype == torch.int8:
        paged = after is not None
        L.check(lib.vtc_l2_search_q8(gallery.data_ptr(), *head, n_groups if paged else 0, ban.data_ptr() if paged else None, _ptr(exclude),
                                     _ptr(after_d), _ptr(after_i), *tail), "vtc_l2_search_q8")
    elif after is not None:
        L.check(lib.vtc_l2_search_grouped_after(gallery.data_ptr(), half, *head, n_groups, ban.data_ptr(), _ptr(exclude), after_d.data_ptr(),
                                                after_i.data_ptr(), *tail), "vtc_l2_search_grouped_after")
    elif exclude is not None:
        L.check(lib.vtc_l2_search_excluding(gallery.data_ptr(), half, *head, exclude.data_ptr(), None, None, *tail), "vtc_l2_search_excluding")
    elif half:
        L.check(lib.vtc_l2_search_half(gallery.data_ptr(), *head, *tail), "vtc_l2_search_half")
    else:
        L.check(lib.vtc_l2_search_grouped(gallery.data_ptr(), *head, *tail), "vtc_l2_search_grouped")
    return ids, out_groups, dists, bits


def l2_search_grouped_workspace_bytes(n_gallery: int, n_queries: int, d: int, depth: int) -> int:
    """0 for a shape vtc_l2_search_grouped refuses."""
    return int(L.lib().vtc_l2_search_grouped_workspace_bytes(int(n_gallery), int(n_queries), int(d), int(depth)))


@on_device
def l2_search_sets(gallery: torch.Tensor, query_sets: torch.Tensor, depth: int, groups: Optional[torch.Tensor] = None,
                   live: Optional[torch.Tensor] = None, exclude: Optional[torch.Tensor] = None, id_base: int = 0, return_dists: bool = True,
                   ws: Optional[torch.Tensor] = None):
    """SET QUERIES (vtc_l2_search_sets): ``query_sets`` [S, M, d] is S queries of M member vectors each, and a set's distance to gallery row
    j is E(S, j) = the minimum, over its members with only finite components, of the fp64 squared distance every search forms.  Returns
    (ids [S, depth] int64, groups [S, depth] int32 or None, dists [S, depth] fp32 or None, nonfinite_bits): ungrouped the live rows with a
    finite E by (E, row), cut to ``depth``; with ``groups`` (int32 [n], as l2_search_grouped) that order with every row deleted that is not
    the first of its group -- the ``depth`` nearest distinct groups.  ``exclude``: int64 [S] on the gallery's device, ONE key per set,
    a global row id ungrouped and a group grouped, deleted from the order before the cut; -1, or a key that is not there, excludes nothing.
    A member with a NaN / inf takes no part (bit 2 of nonfinite_bits); a set with no finite member is a row of -1 / (-1) / +inf.  A set of
    one member is l2_search / l2_search_grouped of that vector, bit for bit; repeating a member changes nothing, which is how ragged sets
    are padded.  ``live``, ``id_base``, a ``torch.float16`` or q8 gallery and ``ws`` as in l2_search: with a caller's ``ws`` of at least
    ``l2_search_sets_workspace_bytes`` the fp64 distances are ``search_dists64(ws, S, depth)``.  S * M <= 64, otherwise ValueError.
    One gallery pass per started tile of 8 members per set.  There is no ``after``: a set of several tiles has no cursor a tile could test
    (include/vtc_hip.h)."""
    query_sets = _gpu(query_sets, torch.float32, "query_sets")
    if query_sets.dim() != 3 or query_sets.shape[0] < 1 or query_sets.shape[1] < 1:
        raise ValueError(f"l2_search_sets: query_sets must be [S, M, d] with S, M >= 1, got {tuple(query_sets.shape)}")
    n_sets, set_size = query_sets.shape[:2]
    if n_sets * set_size > SEARCH_MAX_QUERIES:
        raise ValueError(f"l2_search_sets: {n_sets} sets of {set_size} members are {n_sets * set_size} vectors, a call takes at most "
                         f"{SEARCH_MAX_QUERIES}")
    gallery, queries, groups, ng, _, d = _search_inputs("l2_search_sets", gallery, query_sets.reshape(n_sets * set_size, -1), groups)
    live = _live_arg(live, ng, gallery.device, "l2_search_sets")
    if exclude is not None:
        exclude = _exclude_arg(exclude, n_sets, gallery.device, "l2_search_sets")
    lib = L.lib()
    ws = _search_ws_arg(ws, lib.vtc_l2_search_sets_workspace_bytes(ng, n_sets, set_size, d, depth, int(groups is not None)), gallery.device,
                        "l2_search_sets")
    ids, out_groups, dists, bits = _search_outputs(n_sets, depth, gallery.device, return_dists, grouped=groups is not None)
    tail = (queries.data_ptr(), _ptr(live), _ptr(groups), _ptr(exclude), ng, n_sets, set_size, d, depth, int(id_base), ids.data_ptr(),
            _ptr(out_groups), _ptr(dists), bits.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    if gallery.dtype == torch.int8:
        L.check(lib.vtc_l2_search_sets_q8(gallery.data_ptr(), *tail), "vtc_l2_search_sets_q8")
    else:
        L.check(lib.vtc_l2_search_sets(gallery.data_ptr(), int(gallery.dtype == torch.float16), *tail), "vtc_l2_search_sets")
    return ids, out_groups, dists, bits


def l2_search_sets_workspace_bytes(n_gallery: int, n_sets: int, set_size: int, d: int, depth: int, grouped: bool = False) -> int:
    """0 for a shape vtc_l2_search_sets refuses."""
    return int(L.lib().vtc_l2_search_sets_workspace_bytes(int(n_gallery), int(n_sets), int(set_size), int(d), int(depth), int(bool(grouped))))


@on_device
def l2_search_grouped_part(gallery: torch.Tensor, queries: torch.Tensor, groups: torch.Tensor, depth: int, id_base: int = 0,
                           live: Optional[torch.Tensor] = None, exclude: Optional[torch.Tensor] = None, after=None,
                           n_groups: Optional[int] = None, ban: Optional[torch.Tensor] = None):
    """One window's share of a grouped search over several: (ids [Q, depth] int64, groups [Q, depth] int32, dists64 [Q, depth] fp64,
    nonfinite_bits) -- what l2_search_merge_grouped takes.  A group's rows may lie in several windows.  fp32 or ``torch.float16`` rows.
    ``exclude``: the excluded groups of l2_search_grouped, the same tensor for every window.
    ``after`` / ``n_groups`` / ``ban``: the cursor of l2_search_grouped in GLOBAL ids, the same for every window, and the ONE bitmap that
    ``l2_group_mark_before`` has filled over EVERY window before the first window is scanned (``ban`` is required here: a window cannot
    know what lies before the cursor in the others)."""
    if after is not None and ban is None:
        raise ValueError("l2_search_grouped_part: a cursor needs the ban bitmap marked over every window (l2_group_mark_before)")
    ng, d = _gallery_shape(gallery)
    nq = queries.shape[0]
    ws = workspace(l2_search_grouped_workspace_bytes(ng, nq, d, depth), gallery.device)
    ids, out_groups, _, bits = l2_search_grouped(gallery, queries, groups, depth, id_base, return_dists=False, ws=ws, live=live, exclude=exclude,
                                                 after=after, n_groups=n_groups, ban=ban)
    return ids, out_groups, search_dists64(ws, nq, depth), bits


@on_device
def l2_search_merge_grouped(ids_parts: torch.Tensor, dists64_parts: torch.Tensor, groups_parts: torch.Tensor, return_dists: bool = True):
    """Grouped lists over gallery windows -> the grouped list of their union (vtc_l2_search_merge_grouped): ids_parts [P, Q, depth] int64,
    dists64_parts fp64 and groups_parts int32 of the same shape (l2_search_grouped_part's outputs, stacked; entries with id -1 are
    ignored).  Of a group that several parts list, the entry first by (distance, id) stays.  Returns (ids, groups, dists fp32 or None)."""
    return _search_merge("l2_search_merge_grouped", return_dists, ids_parts, dists64_parts, groups_parts)


def pad_search_part(ids: torch.Tensor, dists64: torch.Tensor, depth: int):
    """A window's lists widened to ``depth`` columns with empty entries (-1 / +inf): windows with fewer rows than the merged list's depth."""
    short = depth - ids.shape[1]
    if short <= 0:
        return ids, dists64
    return (torch.nn.functional.pad(ids, (0, short), value=-1), torch.nn.functional.pad(dists64, (0, short), value=float("inf")))


def sweep_shard_supported(n_total: int, n_local: int, depth: int) -> bool:
    return bool(L.lib().vtc_l2_sweep_shard_supported(int(n_total), int(n_local), int(depth)))


def sweep_row_block() -> int:
    return int(L.lib().vtc_l2_sweep_row_block())


@on_device
def sweep_shard_rows(a_all: torch.Tensor, b_local: torch.Tensor, depth: int, nblk_pad: int, ws: Optional[torch.Tensor] = None):
    """Rank-local half of the sharded sweep: (ids [n_local, depth] = l2_topk(gallery=a_all, queries=b_local),
    col_planes [4, nblk_pad, n_total] uint32 (as int32 tensor) for the exchange).  include/vtc_hip.h."""
    a_all, b_local = _gpu(a_all, torch.float32, "a_all"), _gpu(b_local, torch.float32, "b_local")
    n, d = a_all.shape
    nl = b_local.shape[0]
    ws = _ws_for(ws, L.lib().vtc_l2_sweep_shard_workspace_bytes(n, nl, d), a_all.device)
    ids = torch.empty(nl, depth, dtype=torch.int64, device=a_all.device)
    planes = torch.empty(4, nblk_pad, n, dtype=torch.int32, device=a_all.device)
    L.check(L.lib().vtc_l2_sweep_shard_rows(a_all.data_ptr(), b_local.data_ptr(), n, nl, d, depth, ids.data_ptr(), None,
                                            planes.data_ptr(), nblk_pad, ws.data_ptr(), ws.numel(), _stream()),
            "vtc_l2_sweep_shard_rows")
    return ids, planes


@on_device
def sweep_shard_cols(b_all: torch.Tensor, a_local: torch.Tensor, depth: int, planes: torch.Tensor, src_base: torch.Tensor,
                     ws: Optional[torch.Tensor] = None):
    """Second half, after the exchange: planes [n_src, 4, nblk_pad, n_local] int32, src_base [n_src] int32 ->
    ids [n_local, depth] = l2_topk(gallery=b_all, queries=a_local)."""
    b_all, a_local = _gpu(b_all, torch.float32, "b_all"), _gpu(a_local, torch.float32, "a_local")
    planes, src_base = _gpu(planes, torch.int32, "planes"), _gpu(src_base, torch.int32, "src_base")
    n, d = b_all.shape
    nl = a_local.shape[0]
    n_src, four, nblk_pad, nl2 = planes.shape
    if four != 4 or nl2 != nl or src_base.numel() != n_src:
        raise ValueError(f"sweep_shard_cols: planes {tuple(planes.shape)} / src_base {tuple(src_base.shape)} do not match n_local={nl}")
    ws = _ws_for(ws, L.lib().vtc_l2_sweep_shard_workspace_bytes(n, nl, d), b_all.device)
    ids = torch.empty(nl, depth, dtype=torch.int64, device=b_all.device)
    L.check(L.lib().vtc_l2_sweep_shard_cols(b_all.data_ptr(), a_local.data_ptr(), n, nl, d, depth, planes.data_ptr(), n_src,
                                            nblk_pad, src_base.data_ptr(), ids.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                            _stream()), "vtc_l2_sweep_shard_cols")
    return ids


def recall_bidir_supported(n: int, d: int) -> bool:
    return bool(L.lib().vtc_l2_recall_bidir_supported(int(n), int(d)))


@on_device
def recall_bidir(a: torch.Tensor, b: torch.Tensor, k_vals: Sequence[int], ws: Optional[torch.Tensor] = None,
                 hits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """R@K hit counters of both directions of n paired rows WITHOUT the sorted neighbour lists (vtc_l2_recall_bidir: one distance GEMM +
    one rank launch): hits[0, j] += #{i : a_i among the k_j nearest a's of b_i} (= RecallAtK.compute(a, b) x n), hits[1, j] the transposed
    direction (= compute(b, a) x n).  The same counters as l2_topk_bidir(depth = max k + 1, EXACT) + recall_hits_pair.
    Non-finite rows are misses and raise bit 40 of hits[:, 0] (L.RECALL_NONFINITE): split_recall_counters() on the host copy."""
    a, b = _gpu(a, torch.float32, "a"), _gpu(b, torch.float32, "b")
    n, d = a.shape
    assert b.shape == (n, d) and 1 <= len(k_vals) <= 4
    if hits is None:
        hits = torch.zeros(2, len(k_vals), dtype=torch.int64, device=a.device)
    assert hits.shape == (2, len(k_vals)) and hits.is_contiguous() and hits.dtype == torch.int64
    ws = _ws_for(ws, L.lib().vtc_l2_recall_bidir_workspace_bytes(n, d), a.device)
    ks = _k_array(k_vals)
    L.check(L.lib().vtc_l2_recall_bidir(a.data_ptr(), b.data_ptr(), n, d, ks, len(k_vals), hits[0].data_ptr(), hits[1].data_ptr(),
                                        ws.data_ptr(), ws.numel(), _stream()), "vtc_l2_recall_bidir")
    return hits


def _rank_call(name, head, size_args, n_a, n_b, device, rows_per_block, reach_capacity, ws):
    """What both rank entry points do around the C call ``name(*head, rows_per_block, reach_capacity, outputs, workspace, stream)``: size the
    workspace (``name_workspace_bytes(*size_args, rows_per_block, reach_capacity)``), allocate rank_a [n_a], rank_b [n_b] and the non-finite
    word, call, return the three."""
    lib = L.lib()
    ws = _ws_for(ws, getattr(lib, name + "_workspace_bytes")(*size_args, rows_per_block, reach_capacity), device)
    rank_a = torch.empty(max(n_a, 1), dtype=torch.int64, device=device)      # (rank_shard's empty window: no null pointer for a tensor without elements)
    rank_b = torch.empty(n_b, dtype=torch.int64, device=device)
    bits = torch.empty(1, dtype=torch.int32, device=device)
    L.check(getattr(lib, name)(*head, rows_per_block, reach_capacity, rank_a.data_ptr(), rank_b.data_ptr(), bits.data_ptr(), ws.data_ptr(),
                               ws.numel(), _stream()), name)
    return rank_a[:n_a], rank_b, bits


@on_device
def rank_bidir(a: torch.Tensor, b: torch.Tensor, rows_per_block: int = 0, reach_capacity: int = 0, ws: Optional[torch.Tensor] = None):
    """Full 0-based ranks of both directions of n paired rows (vtc_l2_rank_bidir): (rank_a [n] int64 = the rank of a_i among the a's for
    query b_i, the direction of RecallAtK.compute(a, b); rank_b [n] the transposed direction; nonfinite_bits, a device int32 [1] with the
    meaning of nonfinite_bits(): 1 = a holds a NaN / inf, 2 = b does).  ``(rank < k).sum()`` are recall_bidir's counters for every k; a
    pair with a non-finite distance has rank n.  The ranks do not depend on reach_capacity (0: the default pool)."""
    a, b = _gpu(a, torch.float32, "a"), _gpu(b, torch.float32, "b")
    n, d = a.shape
    if b.shape != (n, d):
        raise ValueError(f"rank_bidir: paired rows expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    return _rank_call("vtc_l2_rank_bidir", (a.data_ptr(), b.data_ptr(), n, d), (n, d), n, n, a.device, rows_per_block, reach_capacity, ws)


def rank_shard(a_all: torch.Tensor, b_all: torch.Tensor, row_base: int, n_local: int, rows_per_block: int = 0, reach_capacity: int = 0,
               ws: Optional[torch.Tensor] = None):
    """One rank's share of rank_bidir on row-sharded embeddings (vtc_l2_rank_shard): the rank holds both gathered sets and owns the rows
    [row_base, row_base + n_local).  Returns (rank_a_local [n_local] int64 = rank_bidir's rank_a[row_base:row_base + n_local], complete;
    rank_b_part [n_total] int64 = this window's partial counts of rank_b -- their sum over windows that tile [0, n_total) is rank_bidir's
    rank_b, element for element; nonfinite_bits over both whole sets, as rank_bidir).  An empty window is valid: all-zero partials.  The
    window is validated on the host (ValueError) before anything is launched."""
    if a_all.dim() != 2 or a_all.shape[0] < 1 or b_all.shape != a_all.shape:
        raise ValueError(f"rank_shard: paired rows expected, got {tuple(a_all.shape)} and {tuple(b_all.shape)}")
    n = a_all.shape[0]
    row_base, n_local = int(row_base), int(n_local)
    if row_base < 0 or n_local < 0 or row_base + n_local > n:
        raise ValueError(f"rank_shard: window row_base={row_base}, n_local={n_local} must lie in [0, n_total={n}]")
    return _rank_shard(a_all, b_all, row_base, n_local, rows_per_block, reach_capacity, ws)


@on_device
def _rank_shard(a_all, b_all, row_base, n_local, rows_per_block, reach_capacity, ws):
    a_all, b_all = _gpu(a_all, torch.float32, "a_all"), _gpu(b_all, torch.float32, "b_all")
    n, d = a_all.shape
    return _rank_call("vtc_l2_rank_shard", (a_all.data_ptr(), b_all.data_ptr(), n, row_base, n_local, d), (n, n_local, d), n_local, n,
                      a_all.device, rows_per_block, reach_capacity, ws)


def check_offsets(offsets, n: int, m: int, allow_empty: bool = True):
    """The caption offsets of rank_grouped as a host int64 array, validated (ValueError): length n + 1, offsets[0] = 0, offsets[n] = m,
    non-decreasing (allow_empty=False: increasing -- no video without a caption).  Touches no device."""
    import numpy as np
    if isinstance(offsets, torch.Tensor):
        offsets = offsets.detach().cpu().numpy()
    off = np.asarray(offsets)
    if off.ndim != 1 or off.shape[0] != n + 1:
        raise ValueError(f"offsets: expected {n + 1} entries for {n} videos, got shape {tuple(off.shape)}")
    if off.dtype.kind not in "iu":
        if off.dtype.kind != "f" or not np.array_equal(off, np.floor(off)):
            raise ValueError(f"offsets: integers expected, got dtype {off.dtype}")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != m:
        raise ValueError(f"offsets: must start at 0 and end at the number of captions {m}, got {int(off[0])} .. {int(off[-1])}")
    steps = np.diff(off)
    if (steps < 0).any():
        raise ValueError(f"offsets: must be non-decreasing (first descent after video {int(np.flatnonzero(steps < 0)[0])})")
    if not allow_empty and (steps == 0).any():
        raise ValueError(f"offsets: video {int(np.flatnonzero(steps == 0)[0])} has no caption")
    return off


def rank_grouped(a: torch.Tensor, b: torch.Tensor, offsets, rows_per_block: int = 0, reach_capacity: int = 0,
                 ws: Optional[torch.Tensor] = None):
    """Full 0-based ranks for videos with several captions each (vtc_l2_rank_grouped): a [n, d] videos, b [m, d] captions (those of a video
    contiguous, in video order), offsets [n + 1] (host sequence or tensor; validated on the host BEFORE anything is launched, ValueError;
    uploaded as int32): the captions of video v are b[offsets[v]:offsets[v + 1]].  Returns (rank_a [m] int64 = the rank of the caption's own
    video among the n videos, rank_b [n] int64 = the best rank one of the video's own captions reaches among all m captions -- the
    caption-level convention, include/vtc_hip.h --, nonfinite_bits as rank_bidir).  A caption with a non-finite own distance has
    rank_a = n, a video without a finite own caption (an empty group too) rank_b = m."""
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or a.shape[0] < 1 or b.shape[0] < 1:
        raise ValueError(f"rank_grouped: a [n, d] and b [m, d] expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    off = check_offsets(offsets, a.shape[0], b.shape[0])
    return _rank_grouped(a, b, off, rows_per_block, reach_capacity, ws)


@on_device
def _rank_grouped(a, b, off, rows_per_block, reach_capacity, ws):
    a, b = _gpu(a, torch.float32, "a"), _gpu(b, torch.float32, "b")
    (n, d), m = a.shape, b.shape[0]
    off_dev = torch.from_numpy(off.astype("int32")).to(a.device)
    return _rank_call("vtc_l2_rank_grouped", (a.data_ptr(), b.data_ptr(), off_dev.data_ptr(), n, m, d), (n, m, d), m, n, a.device,
                      rows_per_block, reach_capacity, ws)


def rank_grouped_vunit(a: torch.Tensor, b: torch.Tensor, offsets, rows_per_block: int = 0, reach_capacity: int = 0,
                       ws: Optional[torch.Tensor] = None):
    """rank_grouped with video -> text in BOTH conventions from one sweep (vtc_l2_rank_grouped_vunit): returns (rank_a [m], rank_b [n],
    rank_v [n], nonfinite_bits).  rank_a and rank_b are rank_grouped's, element for element; rank_v[v] is the video-unit convention of the
    video-retrieval literature: the number of OTHER VIDEOS whose best caption is closer to video v than v's own best caption (an exact tie
    goes to the lower video index; include/vtc_hip.h has the definition).  rank_v <= rank_b, and the two agree on rank 0.  A video without
    a finite own caption (an empty group too) has rank_v = n.  Offsets are validated on the host before anything is launched."""
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or a.shape[0] < 1 or b.shape[0] < 1:
        raise ValueError(f"rank_grouped_vunit: a [n, d] and b [m, d] expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    off = check_offsets(offsets, a.shape[0], b.shape[0])
    return _rank_grouped_vunit(a, b, off, rows_per_block, reach_capacity, ws)


@on_device
def _rank_grouped_vunit(a, b, off, rows_per_block, reach_capacity, ws):
    a, b = _gpu(a, torch.float32, "a"), _gpu(b, torch.float32, "b")
    (n, d), m = a.shape, b.shape[0]
    lib = L.lib()
    off_dev = torch.from_numpy(off.astype("int32")).to(a.device)
    ws = _ws_for(ws, lib.vtc_l2_rank_grouped_vunit_workspace_bytes(n, m, d, rows_per_block, reach_capacity), a.device)
    rank_a = torch.empty(m, dtype=torch.int64, device=a.device)
    rank_b = torch.empty(n, dtype=torch.int64, device=a.device)
    rank_v = torch.empty(n, dtype=torch.int64, device=a.device)
    bits = torch.empty(1, dtype=torch.int32, device=a.device)
    L.check(lib.vtc_l2_rank_grouped_vunit(a.data_ptr(), b.data_ptr(), off_dev.data_ptr(), n, m, d, rows_per_block, reach_capacity,
                                          rank_a.data_ptr(), rank_b.data_ptr(), rank_v.data_ptr(), bits.data_ptr(), ws.data_ptr(),
                                          ws.numel(), _stream()), "vtc_l2_rank_grouped_vunit")
    return rank_a, rank_b, rank_v, bits


def rank_kappa(d: int) -> float:
    """kappa of the rank sweep's error bound eps = kappa (|q|^2 + max|g|^2) at feature width d."""
    return float(L.lib().vtc_l2_rank_kappa(int(d)))


def rank_sweep_stats(ws: torch.Tensor) -> dict:
    """What the last rank sweep on workspace ``ws`` left in its first words (include/vtc_hip.h): per direction the pairs in reach
    of their target, the largest number of them for one owner, and the owners counted by fp64 brute force.  The ``vunit_*`` keys are the
    video-unit direction's (video, group) figures; only rank_grouped_vunit writes them (after another call they hold what the workspace held)."""
    w = ws[:88].view(torch.int64).cpu().tolist()
    return {"in_reach": (w[0], w[1]), "in_reach_max": (w[2], w[3]), "brute_force_owners": (w[4], w[5]),
            "vunit_in_reach": w[8], "vunit_in_reach_max": w[9], "vunit_brute_force_owners": w[10]}


def split_recall_counters(hits_host: torch.Tensor):
    """(counters, nonfinite) of a HOST copy of the recall-only sweeps' hit counters: the NaN / inf marker (bit 40 and above of the first
    counter of a direction, summed over ranks) taken off."""
    h = hits_host.numpy()                # (numpy: a torch CPU op costs microseconds that the 10k sweep's 0.28 ms would show)
    return torch.from_numpy(h & (L.RECALL_NONFINITE - 1)), bool((h >> 40).any())


def recall_planes(k_vals: Sequence[int], n_total: int) -> int:
    """Key planes per (column, block) that the recall-only sweep keeps for these k at this gallery size (vtc_l2_recall_planes): 2, 3 or 4."""
    ks = _k_array(k_vals)
    return int(L.lib().vtc_l2_recall_planes(ks, len(k_vals), int(n_total)))


def recall_shard_supported(n_total: int, n_local: int, d: int) -> bool:
    return bool(L.lib().vtc_l2_recall_shard_supported(int(n_total), int(n_local), int(d)))


@on_device
def recall_shard_rows(a_all: torch.Tensor, b_local: torch.Tensor, row_base: int, k_vals: Sequence[int], nblk_pad: int, hits: torch.Tensor,
                      ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Rank-local half of the sharded sweep with the recall-only finish (vtc_l2_recall_shard_rows): hits [nk] int64 += this rank's
    counters of RecallAtK.compute(a, b); returns col_planes [P, nblk_pad, n_total] with P = vtc_l2_recall_planes(k_vals, n_local) = 2, 3 or 4 (int32 tensor) for the exchange."""
    a_all, b_local = _gpu(a_all, torch.float32, "a_all"), _gpu(b_local, torch.float32, "b_local")
    n, d = a_all.shape
    nl = b_local.shape[0]
    assert hits.shape == (len(k_vals),) and hits.dtype == torch.int64 and hits.is_contiguous() and hits.device == a_all.device
    ws = _ws_for(ws, L.lib().vtc_l2_sweep_shard_workspace_bytes(n, nl, d), a_all.device)
    ks = _k_array(k_vals)
    planes = torch.empty(L.lib().vtc_l2_recall_planes(ks, len(k_vals), n), nblk_pad, n, dtype=torch.int32, device=a_all.device)
    L.check(L.lib().vtc_l2_recall_shard_rows(a_all.data_ptr(), b_local.data_ptr(), n, nl, int(row_base), d, ks, len(k_vals), hits.data_ptr(),
                                             planes.data_ptr(), nblk_pad, ws.data_ptr(), ws.numel(), _stream()), "vtc_l2_recall_shard_rows")
    return planes


@on_device
def recall_shard_cols(b_all: torch.Tensor, a_local: torch.Tensor, row_base: int, k_vals: Sequence[int], planes: torch.Tensor,
                      src_bounds: torch.Tensor, hits: torch.Tensor, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Second half, after the exchange: planes [n_src, 4, nblk_pad, n_local] int32, src_bounds [n_src + 1] int32 (device); hits [nk] int64
    += this rank's counters of RecallAtK.compute(b, a)."""
    b_all, a_local = _gpu(b_all, torch.float32, "b_all"), _gpu(a_local, torch.float32, "a_local")
    planes, src_bounds = _gpu(planes, torch.int32, "planes"), _gpu(src_bounds, torch.int32, "src_bounds")
    n, d = b_all.shape
    nl = a_local.shape[0]
    n_src, npl, nblk_pad, nl2 = planes.shape
    ks = _k_array(k_vals)
    if npl != L.lib().vtc_l2_recall_planes(ks, len(k_vals), n) or nl2 != nl or src_bounds.numel() != n_src + 1:
        raise ValueError(f"recall_shard_cols: planes {tuple(planes.shape)} / src_bounds {tuple(src_bounds.shape)} do not match n_local={nl}, "
                         f"k_vals={list(k_vals)}")
    assert hits.shape == (len(k_vals),) and hits.dtype == torch.int64 and hits.is_contiguous() and hits.device == b_all.device
    ws = _ws_for(ws, L.lib().vtc_l2_sweep_shard_workspace_bytes(n, nl, d), b_all.device)
    L.check(L.lib().vtc_l2_recall_shard_cols(b_all.data_ptr(), a_local.data_ptr(), n, nl, int(row_base), d, ks, len(k_vals), planes.data_ptr(),
                                             n_src, nblk_pad, src_bounds.data_ptr(), hits.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
            "vtc_l2_recall_shard_cols")
    return hits


@on_device
def recall_hits_pair(ids_a: torch.Tensor, ids_b: torch.Tensor, k_vals: Sequence[int], target_offset: int, hits: torch.Tensor) -> torch.Tensor:
    """hits[0] += hits of ids_a, hits[1] += hits of ids_b (both [n, depth], same targets): one launch for both directions."""
    ids_a, ids_b = _gpu(ids_a, torch.int64, "ids_a"), _gpu(ids_b, torch.int64, "ids_b")
    assert ids_a.shape == ids_b.shape and hits.shape[0] == 2 and hits.is_contiguous()
    nq, depth = ids_a.shape
    ks = _k_array(k_vals)
    L.check(L.lib().vtc_recall_hits_pair(ids_a.data_ptr(), ids_b.data_ptr(), nq, depth, int(target_offset), ks, len(k_vals),
                                         hits[0].data_ptr(), hits[1].data_ptr(), _stream()), "vtc_recall_hits_pair")
    return hits


@on_device
def recall_hits(ids: torch.Tensor, k_vals: Sequence[int], target_offset: int = 0,
                hits: Optional[torch.Tensor] = None) -> torch.Tensor:
    ids = _gpu(ids, torch.int64, "ids")
    nq, depth = ids.shape
    if hits is None:
        hits = torch.zeros(len(k_vals), dtype=torch.int64, device=ids.device)
    ks = _k_array(k_vals)
    L.check(L.lib().vtc_recall_hits(ids.data_ptr(), nq, depth, int(target_offset), ks, len(k_vals), hits.data_ptr(), _stream()),
            "vtc_recall_hits")
    return hits


@on_device
def nonfinite_flag(x: torch.Tensor, flag: torch.Tensor) -> torch.Tensor:
    """flag[0] |= 1 when ``x`` holds a NaN / inf (vtc_nonfinite_flag).  flag: int32 in device memory."""
    x = _gpu(x, torch.float32, "x")
    L.check(L.lib().vtc_nonfinite_flag(x.data_ptr(), x.numel(), flag.data_ptr(), _stream()), "vtc_nonfinite_flag")
    return flag


# ---- adapter-only training step: backward + optimizer primitives (train.hip) --------------------
# Thin forms of the C ABI for callers that bring their own output buffers (vtc_amd/host/adapter_train.py keeps its private
# helpers); `out` buffers, where given, are written as they are -- the entry points own their zeroing.
def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    return _gpu(t, torch.float32, name)


@on_device
def transpose(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[c][r] = x[r][c]."""
    x = _f32(x, "x")
    r, c = x.shape
    out = torch.empty(c, r, dtype=torch.float32, device=x.device) if out is None else out
    L.check(L.lib().vtc_transpose_f32(x.data_ptr(), out.data_ptr(), r, c, _stream()), "vtc_transpose_f32")
    return out


@on_device
def colsum(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[c] = sum_r x[r][c] (the entry point zeroes ``out`` itself)."""
    x = _f32(x, "x")
    out = torch.empty(x.shape[1], dtype=torch.float32, device=x.device) if out is None else out
    L.check(L.lib().vtc_colsum_f32(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], _stream()), "vtc_colsum_f32")
    return out


@on_device
def layernorm_bwd(x: torch.Tensor, gamma: torch.Tensor, dy: torch.Tensor, dx: Optional[torch.Tensor] = None, accumulate_dx: bool = False,
                  dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None):
    """(dx, dgamma, dbeta) of LayerNorm (eps 1e-5, biased variance); with ``accumulate_dx`` the row gradients are ADDED to ``dx``.
    dgamma / dbeta are zeroed by the entry point."""
    x, gamma, dy = _f32(x, "x"), _f32(gamma, "gamma"), _f32(dy, "dy")
    if dx is None:
        assert not accumulate_dx
        dx = torch.empty_like(x)
    dgamma = torch.empty_like(gamma) if dgamma is None else dgamma
    dbeta = torch.empty_like(gamma) if dbeta is None else dbeta
    L.check(L.lib().vtc_layernorm_bwd(x.data_ptr(), gamma.data_ptr(), dy.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                      x.shape[0], x.shape[1], int(accumulate_dx), _stream()), "vtc_layernorm_bwd")
    return dx, dgamma, dbeta


@on_device
def attention_small_bwd(qkv: torch.Tensor, dout: torch.Tensor, n_seq: int, L_: int, heads: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dqkv of the unmasked attention on contiguous sequences, L <= 16, head_dim 64: qkv [n_seq * L, 3 W], dout [n_seq * L, W]."""
    qkv, dout = _f32(qkv, "qkv"), _f32(dout, "dout")
    out = torch.empty_like(qkv) if out is None else out
    L.check(L.lib().vtc_attention_small_bwd(qkv.data_ptr(), dout.data_ptr(), out.data_ptr(), n_seq, L_, heads, _stream()), "vtc_attention_small_bwd")
    return out


@on_device
def quickgelu(x: torch.Tensor, dy: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x sigmoid(1.702 x), or with ``dy`` its backward dy * d/dx."""
    x = _f32(x, "x")
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().vtc_quickgelu(x.data_ptr(), _f32(dy, "dy").data_ptr() if dy is not None else None, out.data_ptr(), x.numel(), _stream()),
            "vtc_quickgelu")
    return out


@on_device
def normalize_rows_bwd(x: torch.Tensor, dy: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx of y = x / |x| per row."""
    x, dy = _f32(x, "x"), _f32(dy, "dy")
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().vtc_normalize_rows_bwd(x.data_ptr(), dy.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], _stream()), "vtc_normalize_rows_bwd")
    return out


@on_device
def clip_loss_bwd(sim: torch.Tensor, out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dsim = d clip_loss / d sim.  ws: at least 4 n floats (allocated when not given)."""
    sim = _f32(sim, "sim")
    n = sim.shape[0]
    assert sim.shape == (n, n)
    out = torch.empty_like(sim) if out is None else out
    ws = torch.empty(4 * n, dtype=torch.float32, device=sim.device) if ws is None else ws
    L.check(L.lib().vtc_clip_loss_bwd(sim.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), _stream()), "vtc_clip_loss_bwd")
    return out


@on_device
def adam_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, vmax: Optional[torch.Tensor], lr: float, beta1: float,
              beta2: float, eps: float, step: int, amsgrad: bool) -> torch.Tensor:
    """torch.optim.Adam single-tensor step in place on p, m, v (and vmax with amsgrad); ``step`` counts from 1."""
    p, g, m, v = _f32(p, "p"), _f32(g, "g"), _f32(m, "m"), _f32(v, "v")
    L.check(L.lib().vtc_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _f32(vmax, "vmax").data_ptr() if vmax is not None else None,
                                  p.numel(), lr, beta1, beta2, eps, int(step), int(amsgrad), _stream()), "vtc_adam_step")
    return p


@on_device
def axpby(x: torch.Tensor, y: Optional[torch.Tensor], a: float, b: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = a x + b y (y None: a x); ``out`` may be ``x``."""
    x = _f32(x, "x")
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().vtc_axpby(out.data_ptr(), x.data_ptr(), _f32(y, "y").data_ptr() if y is not None else None, a, b, x.numel(), _stream()), "vtc_axpby")
    return out


@on_device
def scale_rows(x: torch.Tensor, s: torch.Tensor, group: int = 1) -> torch.Tensor:
    """x[r] *= s[r // group], in place."""
    x, s = _f32(x, "x"), _f32(s, "s")
    L.check(L.lib().vtc_scale_rows(x.data_ptr(), s.data_ptr(), x.shape[0], x.shape[1], group, _stream()), "vtc_scale_rows")
    return x
