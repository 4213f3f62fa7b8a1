"""GPU: the exact finish (vtc_amd/csrc/exact_list.h) held to ONE answer across its users.  The fp64 list, the re-rank and the brute-force
scan are shared by the N x N sweep (ops.l2_topk, EXACT: re-rank, fallback, rescan), the query-time scan (ops.l2_search) and the
many-query search (ops.l2_search_many: finish, fallback); each promises the first `depth` rows by (fp64 distance, row).  So over one
gallery they must agree bit for bit, and with a numpy fp64 reference sorted the same way.

One seeded gallery of 1024 unit rows, d = 64, searched whole (the smallest the block-minima path takes: re-rank and rescan) and cut to its
first 600 rows (the distance-matrix path: re-rank and brute-force fallback; depth 40 takes that path at either size).  Rows 560 .. 589
are exact copies of row 17; rows 300 .. 359 lie within 1e-7 of row 41, far below what either approximate pass resolves, and are more
than a candidate list of 32 holds: the queries sitting there cannot be certified.  Rounded to half the near-copies become duplicates.

The reference's fp32 distances are compared within one ulp, as everywhere (search_refs.py: numpy's summation order differs in the last
fp64 bits); the ids must be equal, which the data's smallest relative gap between unequal neighbours (asserted > 1e-12) entitles to."""
import functools

import numpy as np
import pytest
import torch

import search_half_refs as HR
import search_refs as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D, NQ, N_FULL, DEEPEST = 64, 64, 1024, 40
COPIES, COPIED, NEAR, NEAR_OF = np.arange(560, 590), 17, np.arange(300, 360), 41


def _ops():
    from vtc_amd import ops
    return ops


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def _data():
    """(gallery fp32 [1024, 64], the same rounded to half, queries [64, 64])."""
    rng = np.random.default_rng(20241)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    g = unit(rng.standard_normal((N_FULL, D)))
    g[COPIES] = g[COPIED]
    g[NEAR] = g[NEAR_OF] + np.float32(1e-7) * rng.standard_normal((NEAR.size, D)).astype(np.float32)
    q = unit(rng.standard_normal((NQ, D)))
    q[0] = g[COPIED]                                                          # on the exact copies
    q[1] = g[NEAR_OF]                                                         # on the near-copies' centre,
    q[2] = g[NEAR[7]]                                                         #   on one of them,
    q[3] = g[NEAR_OF] + np.float32(1e-3) * q[3]                               #   and beside them
    q[4] = g[COPIED] + np.float32(1e-3) * q[4]
    return g, HR.round_half(g), q


@functools.lru_cache(maxsize=None)
def _reference(n, half):
    """(ids, dists64) [64, 40] of the first n rows by (fp64 distance, row): the lists of a smaller depth are its prefixes."""
    g, gh, q = _data()
    ids, d64, gap = SR.reference_search64(HR.widen(gh[:n]) if half else g[:n], q, DEEPEST)
    assert gap > 1e-12, gap
    return ids, d64


def _check_reference(ids, dists, n, half, depth):
    want_ids, want_d64 = _reference(n, half)
    assert np.array_equal(ids.cpu().numpy(), want_ids[:, :depth])
    SR.assert_dists_within_one_ulp(dists.cpu().numpy(), want_d64[:, :depth].astype(np.float32))


@pytest.mark.parametrize("depth", [11, 40])
@pytest.mark.parametrize("n", [600, N_FULL])
def test_sweep_equals_scan_and_reference(n, depth):
    from vtc_amd import _lib as L
    ops = _ops()
    g, _, q = _data()
    tg, tq = _t(g[:n]), _t(q)
    ids, dists = ops.l2_topk(tg, tq, depth, precision=L.SWEEP_EXACT)
    scan_ids, scan_dists, bits = ops.l2_search(tg, tq, depth)
    assert int(bits.item()) == 0
    assert torch.equal(ids, scan_ids)
    assert torch.equal(dists, scan_dists)                                     # fp32, bit for bit: the same doubles, rounded once
    _check_reference(ids, dists, n, False, depth)
    tied = ([COPIED] + COPIES.tolist())[:depth]
    assert ids[0, :len(tied)].tolist() == tied                                # exact ties in row order


@pytest.mark.parametrize("depth", [11, 32])
@pytest.mark.parametrize("n", [600, N_FULL])
def test_many_query_search_equals_scan_and_reference(n, depth):
    ops = _ops()
    _, gh, q = _data()
    th, tq = _t(gh[:n]), _t(q)
    ws = ops.workspace(ops.l2_search_many_workspace_bytes(n, NQ, D, depth), DEV)
    many = tuple(ops.l2_search_many(th, tq, depth, ws=ws)) + (ops.search_dists64(ws, NQ, depth).clone(),)
    fallbacks = ops.search_many_stats(ws, NQ, depth)["fallback_queries"]
    ws2 = ops.workspace(ops.l2_search_workspace_bytes(n, NQ, D, depth), DEV)
    scan = tuple(ops.l2_search(th, tq, depth, ws=ws2)) + (ops.search_dists64(ws2, NQ, depth).clone(),)
    for x, y in zip(many, scan):                                              # ids, fp32 dists, the non-finite word, fp64 dists
        assert x.dtype == y.dtype and torch.equal(x, y), (x, y)
    print(f"n={n} depth={depth}: {fallbacks} queries took the fallback")
    assert fallbacks >= 1
    _check_reference(many[0], many[1], n, True, depth)
    assert np.array_equal(many[3].cpu().numpy().astype(np.float32), many[1].cpu().numpy())
