"""One-process-per-GPU scale-out of the eval path (torch.distributed; backend "nccl" = RCCL).

The reference is single-process (nn.DataParallel, train.py:77-80; eval is single-GPU,
evaluation/eval.py:196).  Here encoding is embarrassingly parallel over pairs -- each rank
encodes its shard, no collective -- and the N x N sweep has exactly one exchange step
(SURVEY 8e):

    all_gather(V_r), all_gather(T_r)          [N/G, 512] fp32 per rank (2.56 MB at 10k, 12.8 MB at 50k)
    rank r sweeps its own query rows against the full gallery, both directions
    all_reduce(sum) of the 2 x len(k) int64 hit counters

No cross-rank top-k merge is needed there because a rank owns whole query rows -- at the price of two
[N/G, N] distance GEMMs per rank.  With VTC_SWEEP_EXACT the ranks instead run ONE GEMM each (rank r: its
b rows x all a columns): the row direction is complete locally, and for the column direction every rank
keeps, per column and per block of 128 of its rows, the three smallest distance keys + a bound
(include/vtc_hip.h, vtc_l2_sweep_shard_rows), sends each column owner its slice

    all_to_all(col_planes[:, :, lo_s:hi_s])   4 x ceil(N/G/128) x N/G uint32 per rank pair (4.9 MB at 50k, G=8)

and the owner certifies + re-ranks in fp64 across all sources (vtc_l2_sweep_shard_cols): the same ids as the
single-GPU search, bit for bit.  Works with "gloo" on CPU tensors for the collectives' bookkeeping
(tests inject CPU stand-ins for the two kernels), the sweep itself is HIP-only.
"""
from __future__ import annotations

import enum
import os
from typing import Callable, Optional, Sequence

import torch
import torch.distributed as dist

from . import _lib as L
from . import ops


def init_from_env(backend: Optional[str] = None):
    """Read RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* (torch.distributed.run); single process otherwise."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # rehearsal knobs: several ranks on ONE card (VTC_LOCAL_DEVICE=0) over gloo (VTC_DIST_BACKEND=gloo)
    local = int(os.environ.get("VTC_LOCAL_DEVICE", local))
    backend = os.environ.get("VTC_DIST_BACKEND", backend)
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        if torch.cuda.is_available():
            torch.cuda.set_device(local)     # every backend: the rank's tensors and launches live on its own card
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    if world > 1 and dist.is_initialized():
        mark_shared_cards(local)
    return rank, local, world


def card_identity(local: int):
    """(host, card) of the device this rank computes on -- the card by its UUID / PCI bus id, which survives HIP_VISIBLE_DEVICES
    renumbering and LOCAL_RANK modulo games; a CPU-only rank (gloo tests) is its own card."""
    import socket
    host = socket.gethostname()
    if not torch.cuda.is_available():
        return (host, f"cpu-{os.getpid()}")
    pr = torch.cuda.get_device_properties(local)
    card = str(getattr(pr, "uuid", "")) or ""
    if not card or set(card) <= set("0-"):
        card = f"pci-{getattr(pr, 'pci_domain_id', 0)}:{getattr(pr, 'pci_bus_id', local)}:{getattr(pr, 'pci_device_id', 0)}"
    return (host, card)


def mark_shared_cards(local: int, identities=None) -> bool:
    """ranks that SHARE a card (however they came to: VTC_LOCAL_DEVICE, LOCAL_RANK modulo the device count, a narrowed
    HIP_VISIBLE_DEVICES) must not take the one-launch CAM -- its software grid barrier needs the whole grid resident at once, which
    an ordinary launch can only promise against the process's OWN kernels; with another process's kernels on the same CUs the
    barrier gives up (NaN embeddings, vtc_amd/csrc/cam.hip).  Detected directly: one all_gather of (host, card id) after
    init_process_group; the result travels as the per-model flag VTC_CAM_NO_FUSED (towers.PackedCam), not as an environment
    variable a library static may already have read.  One process per GPU -- the production layout -- is not affected."""
    from . import towers
    mine = card_identity(local)
    if identities is None:
        identities = [None] * dist.get_world_size()
        dist.all_gather_object(identities, mine)
    shared = sum(1 for i in identities if tuple(i) == tuple(mine)) > 1
    towers.set_cam_shared_card(shared)
    return shared


def shard_bounds(n: int, rank: int, world: int):
    """Contiguous shards, sizes differ by at most one: rank r owns [lo, hi)."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def all_gather_rows(x: torch.Tensor, n_total: int, rank: int, world: int) -> torch.Tensor:
    """Concatenate every rank's [n_r, D] rows in rank order (shards may differ by one row)."""
    if world == 1:
        return x
    sizes = [shard_bounds(n_total, r, world) for r in range(world)]
    mx = max(hi - lo for lo, hi in sizes)
    pad = x
    if x.shape[0] < mx:
        pad = torch.cat([x, x.new_zeros(mx - x.shape[0], x.shape[1])])
    out = x.new_empty(world * mx, x.shape[1])
    dist.all_gather_into_tensor(out, pad.contiguous())
    if all(hi - lo == mx for lo, hi in sizes):
        return out
    return torch.cat([out[r * mx: r * mx + (hi - lo)] for r, (lo, hi) in enumerate(sizes)])


RANK_PATH = os.environ.get("VTC_SWEEP_RANK", "1") != "0"      # EXACT: hit counters without sorted lists (read at import; RecallAtK.rank_path's default)
RANK_MIN_ROWS = 1024        # the library's recall-only sweep takes n >= 1024
BIDIR_MIN_ROWS = 5120       # tools/bidir_threshold.py: one matrix wins from ~5k rows (EXACT 6k 0.49 vs 0.6+, 10k 0.64 vs 0.79 ms)
BIDIR_MIN_ROWS_F32 = 3000   # SWEEP_F32: the fp32-MFMA GEMM it saves is the expensive part at every size


class SweepPath(enum.Enum):
    """The five ways an N x N sweep of both directions runs; the value is the label that `phases["path"]` and bench.py print."""
    RANK = "one distance matrix, ranks of the paired rows (no sorted lists)"
    ONE_MATRIX = "one distance matrix, row + column top-k"
    RANK_SHARDED = "one [N/G, N] distance GEMM per rank, column block minima exchanged (all-to-all), ranks of the paired rows (no sorted lists)"
    ONE_MATRIX_SHARDED = "one [N/G, N] distance GEMM per rank, column block minima exchanged (all-to-all)"
    TWO_SEARCHES = "two searches per rank ([N/G, N] blocks)"


def choose_sweep_path(n_total: int, d: int, precision: int, world: int, nk: int = 3, depth: int = 11, *, paired: bool = True,
                      rank_path: Optional[bool] = None, bidir_min_rows: Optional[int] = None, bidir_min_rows_f32: Optional[int] = None,
                      rank_min_rows: Optional[int] = None) -> SweepPath:
    """THE decision which sweep a call takes (sharded_recall, RecallAtK.compute_both and sweep_path all ask here).  No tensors, no
    collectives, no GPU: world 1 needs no library at all, world > 1 asks its host-only `*_shard_supported` once per shard size.
    ``paired``: both embedding sets have the same shape.  The thresholds default to the constants above (RecallAtK passes its own
    attributes).  VTC_SWEEP_SHARD_TWO=1 (read at CALL time: bench.py sets it mid-process) forces two searches at world > 1."""
    rank_ok = (precision == L.SWEEP_EXACT and (RANK_PATH if rank_path is None else rank_path) and nk <= 4 and paired)
    if world <= 1:
        if rank_ok and n_total >= (RANK_MIN_ROWS if rank_min_rows is None else rank_min_rows) and d % 64 == 0:
            return SweepPath.RANK
        if precision == L.SWEEP_F32:
            one = n_total >= (BIDIR_MIN_ROWS_F32 if bidir_min_rows_f32 is None else bidir_min_rows_f32)
        else:
            one = n_total >= (BIDIR_MIN_ROWS if bidir_min_rows is None else bidir_min_rows)
        return SweepPath.ONE_MATRIX if one else SweepPath.TWO_SEARCHES
    if precision != L.SWEEP_EXACT or os.environ.get("VTC_SWEEP_SHARD_TWO") == "1":
        return SweepPath.TWO_SEARCHES
    shards = {hi - lo for lo, hi in (shard_bounds(n_total, r, world) for r in range(world))}      # at most two sizes
    if rank_ok and all(ops.recall_shard_supported(n_total, n_r, d) for n_r in shards):
        return SweepPath.RANK_SHARDED
    if all(ops.sweep_shard_supported(n_total, n_r, depth) for n_r in shards):
        return SweepPath.ONE_MATRIX_SHARDED
    return SweepPath.TWO_SEARCHES


def sweep_path(n_total: int, precision: int, world: int, depth: int = 11, d: int = 512) -> str:
    """The label of the path that paired embeddings of this shape take with the usual three k values."""
    return choose_sweep_path(n_total, d, precision, world, depth=depth).value


_A2A_SEND: dict = {}      # exchange_column_planes' padded send buffer / pinned host staging buffers, by shape


def exchange_column_planes(planes: torch.Tensor, n_total: int, rank: int, world: int) -> torch.Tensor:
    """planes [P, nblk_pad, n_total] of this rank's rows (P = 2, 3 or 4 key planes: vtc_l2_recall_planes) -> [world, P, nblk_pad, n_local]: what every rank (in rank order)
    holds for THIS rank's columns.  One equal-split all_to_all_single (shards differ by at most one column: the buffer is
    padded to the largest) -- the collective form RCCL and gloo both implement; gloo (tests, one-card rehearsals) has no
    device-memory transport, so there the buffer is staged through host memory."""
    bounds = [shard_bounds(n_total, r, world) for r in range(world)]
    lo, hi = bounds[rank]
    mx = max(b - a for a, b in bounds)
    P, NB = planes.shape[0], planes.shape[1]
    if planes.dim() != 3 or planes.shape[2] != n_total or not planes.is_contiguous():
        raise ValueError(f"exchange_column_planes: planes must be a contiguous [P, nblk_pad, n_total = {n_total}] tensor, got "
                         f"{tuple(planes.shape)} (contiguous: {planes.is_contiguous()})")
    nccl = dist.get_backend() == "nccl"
    if all(b - a == mx for a, b in bounds):
        send = planes.reshape(P, NB, world, mx).permute(2, 0, 1, 3).contiguous()
    else:
        # ragged shards: a padded send buffer, kept per (shape, dtype, device) -- the padding columns are sliced off on receipt, so
        # they need no zeroing and the buffer no re-allocation per call
        key = (world, P, NB, mx, planes.dtype, planes.device)
        send = _A2A_SEND.get(key)
        if send is None:
            _A2A_SEND.clear()
            send = _A2A_SEND[key] = planes.new_zeros(world, P, NB, mx)
        for r, (a, b) in enumerate(bounds):
            send[r, :, :, : b - a].copy_(planes[:, :, a:b])
    if nccl:
        recv = torch.empty_like(send)
        dist.all_to_all_single(recv, send)
    else:
        # gloo (tests, one-card rehearsals): staged through host memory -- pinned and cached when the planes live on a GPU
        if send.is_cuda:
            hk = ("host",) + tuple(send.shape) + (send.dtype,)
            bufs = _A2A_SEND.get(hk)
            if bufs is None:
                for k_ in [k_ for k_ in _A2A_SEND if k_ and k_[0] == "host"]:      # one pinned pair at a time: the last shape
                    del _A2A_SEND[k_]
                bufs = _A2A_SEND[hk] = (torch.empty(send.shape, dtype=send.dtype, pin_memory=True), torch.empty(send.shape, dtype=send.dtype, pin_memory=True))
            host, got = bufs
            host.copy_(send)
        else:
            host, got = send, torch.empty_like(send)
        dist.all_to_all_single(got, host)
        recv = got.to(planes.device)
    return recv if hi - lo == mx else recv[..., : hi - lo].contiguous()


def sweep_workspace_bytes(n_total: int, n_local: int, d: int, precision: int, world: int) -> int:
    """Bytes of caller-owned workspace that sharded_recall needs for this shape (largest of the paths it may take)."""
    lib = L.lib()
    need = lib.vtc_l2_topk_workspace_bytes(n_total, n_local, d, precision, 0)
    if world == 1:
        need = max(need, lib.vtc_l2_topk_bidir_workspace_bytes(n_total, n_total, d, precision, 0))
    elif precision == 3:
        need = max(need, lib.vtc_l2_sweep_shard_workspace_bytes(n_total, n_local, d))
    return int(need)


class _PhaseClock:
    """HIP events on the launch stream between the steps of a sweep: `phases[name + "_ms"]` += the GPU time since the previous mark."""

    def __init__(self, phases: Optional[dict], on_gpu: bool):
        self.phases, self.on, self.marks = phases, phases is not None and on_gpu, []

    def mark(self, name: str):
        if self.on:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.marks.append((name, e))

    def close(self, path: str, exchange: Optional[str] = None):
        """Call after the final D2H (the events have completed)."""
        if self.phases is None:
            return
        for (_, e0), (name, e1) in zip(self.marks, self.marks[1:]):
            self.phases[name + "_ms"] = round(self.phases.get(name + "_ms", 0.0) + e0.elapsed_time(e1), 4)
        self.phases["path"] = path
        if exchange is not None:
            self.phases["exchange"] = exchange


def _exchange_name() -> str:
    return "all_to_all_single (RCCL)" if dist.get_backend() == "nccl" else f"all_to_all_single through host memory ({dist.get_backend()})"


def gather_both(feats_a_local: torch.Tensor, feats_b_local: torch.Tensor, n_total: int, rank: int, world: int):
    """(a_all, b_all): every rank's rows in rank order.  ONE exchange for both embedding sets ([n_r, 2D] rows) when they have the same
    width: at 10k x 512 the all-gather is latency-bound, a second collective costs as much as the first."""
    if world > 1 and feats_a_local.shape[1] == feats_b_local.shape[1] and feats_a_local.dtype == feats_b_local.dtype:
        d = feats_a_local.shape[1]
        ab = all_gather_rows(torch.cat([feats_a_local, feats_b_local], dim=1), n_total, rank, world)
        return ab[:, :d].contiguous(), ab[:, d:].contiguous()
    return all_gather_rows(feats_a_local, n_total, rank, world), all_gather_rows(feats_b_local, n_total, rank, world)


def _flag_nonfinite(flag: torch.Tensor, a: torch.Tensor, b: torch.Tensor):
    """flag (one int64 slot behind the hit counters, so it travels with their all-reduce and D2H) |= 1 / 2 when a / b hold a NaN or inf."""
    if a.is_cuda:
        ops.nonfinite_flag2(a, b, flag)
    else:
        flag[0] = int(not bool(torch.isfinite(a).all())) | 2 * int(not bool(torch.isfinite(b).all()))


# ---- the five paths of sharded_recall: each fills `hits` [2, len(ks)] (this rank's partial counters) or returns the sorted ids -------------
def _world1_rank_path(a_all, b_all, ks, hits, ws, clock):
    """One rank owns every pair, EXACT: the hit counters come straight from the distance GEMM's key planes (vtc_l2_recall_bidir: the
    rank of each query's own gallery row; no sorted lists) -- what RecallAtK.compute_both does on one GPU."""
    ops.recall_bidir(a_all, b_all, ks, ws=ws, hits=hits)
    clock.mark("bidir_gemm_rank")


def _world1_one_matrix(a_all, b_all, depth, precision, ws, clock):
    """One rank owns the whole matrix: the sorted ids of both directions from one distance GEMM (vtc_l2_topk_bidir)."""
    i1, _, i2, _ = ops.l2_topk_bidir(a_all, b_all, depth, precision=precision, return_dists=False, ws=ws)
    clock.mark("bidir_gemm_select")
    return i1, i2


def _rank_sharded(a_all, b_all, a_local, b_local, n_total, lo, ks, hits, rank, world, rank_ops, ws, clock):
    """One [N/G, N] GEMM per rank, recall-only finish: this rank's hit counters of the row direction come with the GEMM, the column
    block minima go to the column owners (one all-to-all), whose rank launch counts the other direction."""
    if rank_ops is None:
        rank_ops = (lambda a_, b_, base, ks_, nbp, h: ops.recall_shard_rows(a_, b_, base, ks_, nbp, h, ws=ws),
                    lambda b_, a_, base, ks_, pl, sb, h: ops.recall_shard_cols(b_, a_, base, ks_, pl, sb, h, ws=ws), ops.sweep_row_block())
    rows_fn, cols_fn, rb = rank_ops
    bounds = [shard_bounds(n_total, r, world) for r in range(world)]
    nblk_pad = -(-max(h - l for l, h in bounds) // rb)
    planes = rows_fn(a_all, b_local, lo, ks, nblk_pad, hits[0])
    clock.mark("rows_gemm_rank")
    recv = exchange_column_planes(planes, n_total, rank, world)
    clock.mark("alltoall")
    src_bounds = torch.tensor([l for l, _ in bounds] + [n_total], dtype=torch.int32, device=planes.device)
    cols_fn(b_all, a_local, lo, ks, recv, src_bounds, hits[1])
    clock.mark("cols_rank")


def _one_matrix_sharded(a_all, b_all, a_local, b_local, n_total, depth, rank, world, shard_ops, ws, clock):
    """One [N/G, N] GEMM per rank, sorted ids: rows finished locally, column block minima to the column owners, who certify + re-rank."""
    if shard_ops is None:
        shard_ops = (lambda a_, b_, d_, nbp: ops.sweep_shard_rows(a_, b_, d_, nbp, ws=ws),
                     lambda b_, a_, d_, pl, sb: ops.sweep_shard_cols(b_, a_, d_, pl, sb, ws=ws), ops.sweep_row_block())
    rows_fn, cols_fn, rb = shard_ops
    bounds = [shard_bounds(n_total, r, world) for r in range(world)]
    nblk_pad = -(-max(h - l for l, h in bounds) // rb)
    i1, planes = rows_fn(a_all, b_local, depth, nblk_pad)          # gallery a, queries b: this rank's b rows
    clock.mark("rows_gemm_select")
    recv = exchange_column_planes(planes, n_total, rank, world)
    clock.mark("alltoall")
    src_base = torch.tensor([l for l, _ in bounds], dtype=torch.int32, device=planes.device)
    i2 = cols_fn(b_all, a_local, depth, recv, src_base)            # gallery b, queries a: this rank's a rows
    clock.mark("cols_select")
    return i1, i2


def _two_searches(a_all, b_all, a_local, b_local, depth, topk, precision, ws, clock):
    """compute(a, b): gallery a, queries b (model/metric.py:137-146) and the transposed search; this rank owns query rows [lo, hi)."""
    if topk is None:
        def topk(g, q, depth_):
            return ops.l2_topk(g, q, depth_, precision=precision, return_dists=False, ws=ws)[0]
    i1 = topk(a_all, b_local, depth)
    clock.mark("search_b_from_a")
    i2 = topk(b_all, a_local, depth)
    clock.mark("search_a_from_b")
    return i1, i2


def _hits_from_ids(both, ks, lo, hi, hits):
    """hits[d, j] = #{ local query i : lo + i among the first ks[j] ids of its row } for the two id arrays."""
    if both[0].is_cuda and len(ks) <= 4 and both[0].shape == both[1].shape:
        ops.recall_hits_pair(both[0], both[1], ks, lo, hits)        # both directions: one launch
        return
    for d_, ids in enumerate(both):
        if ids.is_cuda and len(ks) <= 4:
            ops.recall_hits(ids, ks, target_offset=lo, hits=hits[d_])
        else:
            tgt = torch.arange(lo, hi, device=ids.device)[:, None]
            for j, k in enumerate(ks):
                hits[d_, j] = (ids[:, :k] == tgt).any(dim=1).sum()


def sharded_recall(feats_a_local: torch.Tensor, feats_b_local: torch.Tensor, n_total: int, k_vals: Sequence[int],
                   rank: int, world: int,
                   topk: Optional[Callable[[torch.Tensor, torch.Tensor, int], torch.Tensor]] = None,
                   precision: int = 3,    # _lib.SWEEP_EXACT
                   ws: Optional[torch.Tensor] = None,
                   shard_ops: Optional[tuple] = None,
                   phases: Optional[dict] = None,
                   rank_ops: Optional[tuple] = None):
    """R@K both directions for row-sharded embeddings.

    Returns ({k: recall b_from_a-direction as RecallAtK.compute(a, b)}, {k: compute(b, a)}).
    ``topk(gallery, queries, depth) -> ids`` defaults to the HIP sweep; tests inject a CPU one to exercise the sharding logic under
    gloo.  ``ws``: a caller-owned uint8 workspace reused across calls (grown by the ops layer when too small).
    ``shard_ops = (rows_fn, cols_fn, row_block)``: stand-ins for ops.sweep_shard_rows / ops.sweep_shard_cols (tests: the
    one-GEMM-per-rank exchange under gloo).  ``rank_ops = (rows_fn, cols_fn, row_block)``: stand-ins for ops.recall_shard_rows /
    ops.recall_shard_cols (the same exchange with the recall-only finish: hit counters, no ids).
    ``phases``: a dict that receives this rank's GPU time per phase in ms (HIP events on the launch stream: allgather /
    rows_gemm_select / alltoall / cols_select / search_a / search_b / hits / allreduce) and the path taken -- what a scaling run is
    read from.

    The dispatcher only: choose_sweep_path decides ONCE, one function per path above runs (world 1: rank path, one matrix; world > 1:
    rank-sharded, one-matrix sharded; any world: two searches).  Injected stand-ins override the choice before it is made.  Non-finite
    embeddings on ANY rank raise ValueError on EVERY rank (the flag word rides behind the hit counters through their all-reduce)."""
    lo, hi = shard_bounds(n_total, rank, world)
    clock = _PhaseClock(phases, feats_a_local.is_cuda)
    clock.mark("start")
    assert feats_a_local.shape[0] == hi - lo and feats_b_local.shape[0] == hi - lo
    a_all, b_all = gather_both(feats_a_local, feats_b_local, n_total, rank, world)
    clock.mark("allgather")
    depth = min(int(max(k_vals)) + 1, n_total)
    ks = [min(int(k), depth) for k in k_vals]
    acc = torch.zeros(2 * len(ks) + 1, dtype=torch.int64, device=feats_a_local.device)        # hit counters + the non-finite word
    hits, flag = acc[: 2 * len(ks)].view(2, len(ks)), acc[2 * len(ks):]
    if world > 1 and rank_ops is not None:
        path, label = SweepPath.RANK_SHARDED, "injected rank ops"
    elif world > 1 and shard_ops is not None:
        path, label = SweepPath.ONE_MATRIX_SHARDED, "injected shard ops"
    elif topk is not None:
        path, label = SweepPath.TWO_SEARCHES, "injected top-k"
    else:
        path, label = choose_sweep_path(n_total, feats_a_local.shape[1], precision, world, len(ks), depth,
                                        paired=feats_a_local.shape == feats_b_local.shape), None
    # the finite check: the recall-only HIP paths report NaN / inf rows inside their counters (VTC_RECALL_NONFINITE: no launch of its own);
    # every other path gets one flag launch over this rank's rows
    marked = label is None and path in (SweepPath.RANK, SweepPath.RANK_SHARDED)
    if not marked:
        _flag_nonfinite(flag, feats_a_local, feats_b_local)
    both, exchange = None, None
    if path is SweepPath.RANK:
        _world1_rank_path(a_all, b_all, ks, hits, ws, clock)
    elif path is SweepPath.ONE_MATRIX:
        both = _world1_one_matrix(a_all, b_all, depth, precision, ws, clock)
    elif path is SweepPath.RANK_SHARDED:
        _rank_sharded(a_all, b_all, feats_a_local, feats_b_local, n_total, lo, ks, hits, rank, world, rank_ops, ws, clock)
        exchange = _exchange_name()
    elif path is SweepPath.ONE_MATRIX_SHARDED:
        both = _one_matrix_sharded(a_all, b_all, feats_a_local, feats_b_local, n_total, depth, rank, world, shard_ops, ws, clock)
        exchange = _exchange_name()
    else:
        both = _two_searches(a_all, b_all, feats_a_local, feats_b_local, depth, topk, precision, ws, clock)
    if both is not None:
        _hits_from_ids(both, ks, lo, hi, hits)
        clock.mark("hits")
    if world > 1:
        dist.all_reduce(acc, op=dist.ReduceOp.SUM)
        clock.mark("allreduce")
    vals = acc.cpu().tolist()            # ONE D2H; plain Python integers from here (torch CPU ops cost microseconds each: the 10k sweep is 0.28 ms)
    clock.close(label or path.value, exchange)
    nh = 2 * len(ks)
    if vals[-1] != 0 or (marked and any(v >> 40 for v in vals[:nh])):              # VTC_RECALL_NONFINITE, summed over the ranks
        raise ValueError("sharded_recall: non-finite values in the embeddings of at least one rank -- the ranks of such rows are undefined "
                         "(vtc_amd.host.model.nonfinite_cause lists what this build knows can produce them)")
    h = [v & ((1 << 40) - 1) for v in vals[:nh]] if marked else vals[:nh]
    nk = len(ks)
    return ({k: h[j] / n_total for j, k in enumerate(k_vals)}, {k: h[nk + j] / n_total for j, k in enumerate(k_vals)})


def sharded_ranks(feats_a_local: torch.Tensor, feats_b_local: torch.Tensor, n_total: int, rank: int, world: int,
                  ws: Optional[torch.Tensor] = None,
                  shard_op: Optional[Callable[[torch.Tensor, torch.Tensor, int, int], tuple]] = None,
                  phases: Optional[dict] = None):
    """The exact full ranks of both directions (what RecallAtK.ranks returns on one GPU) for row-sharded embeddings: (rank_a [n_total],
    rank_b [n_total]) int64, identical on every rank, on the inputs' device.

    all_gather of both sets, then every rank runs the counting sweep over its own rows of the distance matrix (ops.rank_shard: ONE
    [N/G, N] distance GEMM; rank_a of its rows is complete, rank_b comes as partial counts of every column), then ONE all_reduce(SUM) of
    one int64 buffer [2 n_total + 1]: zeros with rank_a_local at [lo, hi), the partial rank_b, the non-finite word -- counts are sums, so
    nothing else is exchanged (8 (2 n_total + 1) bytes per rank).  ``world == 1`` is ops.rank_bidir.
    ``shard_op(a_all, b_all, row_base, n_local) -> (rank_a_local, rank_b_part, nonfinite_bits)``: a stand-in for ops.rank_shard (tests:
    the exchange under gloo on CPU tensors).  ``phases`` receives this rank's GPU time per phase in ms (allgather / shard_sweep /
    allreduce) and the path's label.  Non-finite embeddings on ANY rank raise ValueError on EVERY rank."""
    lo, hi = shard_bounds(n_total, rank, world)
    clock = _PhaseClock(phases, feats_a_local.is_cuda)
    clock.mark("start")
    assert feats_a_local.shape[0] == hi - lo and feats_b_local.shape[0] == hi - lo
    a_all, b_all = gather_both(feats_a_local, feats_b_local, n_total, rank, world)
    clock.mark("allgather")
    if shard_op is not None:
        label = "injected shard op"
    elif world == 1:
        label = "one distance matrix, exact ranks of every pair (counting sweep)"
        shard_op = lambda a_, b_, base, nl: ops.rank_bidir(a_, b_, ws=ws)                                              # noqa: E731
    else:
        label = "one [N/G, N] distance GEMM per rank, exact ranks of every pair (counting sweep), partial column counts all-reduced"
        shard_op = lambda a_, b_, base, nl: ops.rank_shard(a_, b_, base, nl, ws=ws)                                    # noqa: E731
    rank_a_local, rank_b_part, bits = shard_op(a_all, b_all, lo, hi - lo)
    acc = torch.zeros(2 * n_total + 1, dtype=torch.int64, device=feats_a_local.device)      # rank_a | rank_b | the non-finite word
    acc[lo:hi] = rank_a_local
    acc[n_total: 2 * n_total] = rank_b_part
    acc[2 * n_total:] = torch.as_tensor(bits, device=acc.device).reshape(-1)[:1]
    clock.mark("shard_sweep")
    if world > 1:
        dist.all_reduce(acc, op=dist.ReduceOp.SUM)
        clock.mark("allreduce")
    flagged = int(acc[2 * n_total].item())      # (the D2H that ends the phases' events)
    clock.close(label)
    if flagged != 0:
        raise ValueError("sharded_ranks: non-finite values in the embeddings of at least one rank -- the ranks of such rows are undefined "
                         "(vtc_amd.host.model.nonfinite_cause lists what this build knows can produce them)")
    return acc[:n_total], acc[n_total: 2 * n_total]


def sharded_rank_stats(feats_a_local: torch.Tensor, feats_b_local: torch.Tensor, n_total: int, rank: int, world: int,
                       k_vals: Sequence[int] = (1, 5, 10), **kw):
    """host.metric.rank_statistics (recall at every k of ``k_vals``, median / mean rank, MRR) of the two rank arrays of sharded_ranks, in
    its order: (the direction of RecallAtK.compute(a, b), the direction of compute(b, a)).  The same pair of dicts on every rank.
    Keyword arguments go to sharded_ranks."""
    from .host.metric import rank_statistics
    rank_a, rank_b = sharded_ranks(feats_a_local, feats_b_local, n_total, rank, world, **kw)
    return rank_statistics(rank_a, k_vals), rank_statistics(rank_b, k_vals)


def sharded_search(index_rows_local: torch.Tensor, row_base: int, queries: torch.Tensor, k: int, rank: int, world: int, after=None,
                   return_dists64: bool = False):
    """Query-time search over a gallery that is row-sharded across ranks: this rank stores the rows [row_base, row_base + n_local) of the
    index (fp32 or torch.float16 [n_local, d], d % 64 == 0 -- half rows are searched as stored, ops.l2_search; the partial lists are fp64
    either way) and every rank holds the same fp32 queries [Q <= 64, d].  Returns (ids [Q, k] int64 -- global row
    ids --, dists [Q, k] fp32), identical on every rank and equal to ops.l2_search over the whole gallery.

    A local ops.l2_search_part(id_base = row_base), ONE all_gather of the partial lists -- ids and fp64 distances in one int64 buffer
    [2, Q, k] per rank: the fp32 distances alone would break ties that the fp64 values decide --, then ops.l2_search_merge.  A rank with
    fewer than k rows (none, too) sends a list padded with -1 / +inf; world <= 64 (the merge's limit on parts).
    ``after``: the cursor of ops.l2_search, ``(d64 [Q] float64, ids [Q] int64)`` in GLOBAL ids and the same on every rank; every rank
    passes it to its ops.l2_search_part, and the merged list is the page after that key.  ``return_dists64`` adds the merged list's
    fp64 distances [Q, k] as a third output -- gathered from the parts' lists, bit for bit -- so ``(d64[:, -1], ids[:, -1])`` is the
    next cursor without computing anything again.
    No multi-GPU box has run this: what is tested is the code path at world = 1 and the windowed merge on one card
    (tests/test_gpu_search.py, tests/test_gpu_search_after.py)."""
    if not 1 <= world <= 64:
        raise ValueError(f"sharded_search: world={world} must be in [1, 64]")
    nq, n_local = queries.shape[0], index_rows_local.shape[0]
    if n_local:
        ids, d64, _ = ops.l2_search_part(index_rows_local, queries, min(int(k), n_local), id_base=int(row_base), after=after)
        ids, d64 = ops.pad_search_part(ids, d64, int(k))
    else:
        ids = torch.full((nq, int(k)), -1, dtype=torch.int64, device=queries.device)
        d64 = torch.full((nq, int(k)), float("inf"), dtype=torch.float64, device=queries.device)
    mine = torch.stack([ids, d64.contiguous().view(torch.int64)])                 # [2, Q, k]: one buffer, one collective
    if world > 1:
        parts = torch.empty((world,) + tuple(mine.shape), dtype=torch.int64, device=mine.device)
        dist.all_gather_into_tensor(parts, mine.contiguous())
    else:
        parts = mine[None]
    ids_parts, d64_parts = parts[:, 0].contiguous(), parts[:, 1].contiguous().view(torch.float64)
    ids, dists = ops.l2_search_merge(ids_parts, d64_parts)
    if not return_dists64:
        return ids, dists
    # the fp64 value of every merged entry: the one part entry with its id (ids are unique across parts; an empty entry finds none)
    flat_ids, flat_d64 = ids_parts.permute(1, 0, 2).reshape(nq, -1), d64_parts.permute(1, 0, 2).reshape(nq, -1)      # [Q, P * k]
    where = (flat_ids[:, None, :] == ids[:, :, None]).to(torch.uint8).argmax(dim=2)                                  # [Q, k]
    return ids, dists, torch.where(ids >= 0, flat_d64.gather(1, where), torch.full_like(dists, float("inf"), dtype=torch.float64))


def sharded_search_videos(index_rows_local: torch.Tensor, video_ids_local: torch.Tensor, row_base: int, queries: torch.Tensor, k: int, rank: int,
                          world: int):
    """``sharded_search`` for a gallery with several rows per video: this rank stores the rows [row_base, row_base + n_local), fp32 or
    torch.float16 as there, and their video ids (int32 [n_local]); a video's rows may lie on different ranks.  Returns (video_ids [Q, k] int64, row_ids [Q, k] int64 --
    global row ids --, dists [Q, k] fp32), identical on every rank and equal to ops.l2_search_grouped over the whole gallery: the k
    nearest distinct videos, each by its nearest row, -1 / -1 / +inf where there are fewer.

    A local ops.l2_search_grouped_part(id_base = row_base), ONE all_gather of [3, Q, k] int64 per rank -- ids, the bits of the fp64
    distances, groups --, then ops.l2_search_merge_grouped, whose de-duplicating insertion absorbs the worse entries of a video that
    several ranks list.  world <= 64.  As with sharded_search, no multi-GPU box has run this: what is tested is the code path at
    world = 1 and the windowed merge on one card (tests/test_gpu_search_grouped.py)."""
    if not 1 <= world <= 64:
        raise ValueError(f"sharded_search_videos: world={world} must be in [1, 64]")
    k = int(k)
    nq, n_local = queries.shape[0], index_rows_local.shape[0]
    if n_local:
        depth = min(k, n_local)
        ids, groups, d64, _ = ops.l2_search_grouped_part(index_rows_local, queries, video_ids_local, depth, id_base=int(row_base))
        ids, d64 = ops.pad_search_part(ids, d64, k)
        groups = torch.nn.functional.pad(groups, (0, k - depth), value=-1)
    else:
        ids = torch.full((nq, k), -1, dtype=torch.int64, device=queries.device)
        d64 = torch.full((nq, k), float("inf"), dtype=torch.float64, device=queries.device)
        groups = torch.full((nq, k), -1, dtype=torch.int32, device=queries.device)
    mine = torch.stack([ids, d64.contiguous().view(torch.int64), groups.to(torch.int64)])      # [3, Q, k]: one buffer, one collective
    if world > 1:
        parts = torch.empty((world,) + tuple(mine.shape), dtype=torch.int64, device=mine.device)
        dist.all_gather_into_tensor(parts, mine.contiguous())
    else:
        parts = mine[None]
    ids, groups, dists = ops.l2_search_merge_grouped(parts[:, 0].contiguous(), parts[:, 1].contiguous().view(torch.float64),
                                                     parts[:, 2].to(torch.int32).contiguous())
    return torch.where(ids >= 0, groups.to(torch.int64), ids), ids, dists
