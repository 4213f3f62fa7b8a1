"""CPU: the ONE decision which N x N sweep a call takes (vtc_amd.dist.choose_sweep_path), pinned case by case.

The expected paths below are written out from the rule table, not computed by the code under test (EXACT = 3, F32 = 0; `paired` = both
embedding sets have the same shape):

    world 1    RANK                 EXACT, rank path on, n >= 1024, nk <= 4, paired, d % 64 == 0
               ONE_MATRIX           n >= 3000 (F32) / n >= 5120 (every other precision)
               TWO_SEARCHES         otherwise
    world > 1  RANK_SHARDED         EXACT, rank path on, nk <= 4, paired, not VTC_SWEEP_SHARD_TWO=1, vtc_l2_recall_shard_supported(n, n_r, d) for every shard
               ONE_MATRIX_SHARDED   EXACT, not VTC_SWEEP_SHARD_TWO=1, vtc_l2_sweep_shard_supported(n, n_r, depth) for every shard
               TWO_SEARCHES         otherwise

The world > 1 rows ask the library's host-only `*_shard_supported` functions (they load and run without a GPU: galleries from 1 024 rows,
d a multiple of 64 for the rank finish, depth <= 32 for the sorted lists)."""
import os

import pytest

from vtc_amd import _lib as L
from vtc_amd import dist as vdist
from vtc_amd.dist import SweepPath as P

EXACT, F32, BF16X3 = 3, 0, 1

LABEL = {
    P.RANK: "one distance matrix, ranks of the paired rows (no sorted lists)",
    P.ONE_MATRIX: "one distance matrix, row + column top-k",
    P.RANK_SHARDED: "one [N/G, N] distance GEMM per rank, column block minima exchanged (all-to-all), ranks of the paired rows (no sorted lists)",
    P.ONE_MATRIX_SHARDED: "one [N/G, N] distance GEMM per rank, column block minima exchanged (all-to-all)",
    P.TWO_SEARCHES: "two searches per rank ([N/G, N] blocks)",
}

# (n, d, precision, nk, depth, paired) -> path with the rank path on, path with it off
WORLD_1 = [
    ((1023, 512, EXACT, 3, 11, True), P.TWO_SEARCHES, P.TWO_SEARCHES),
    ((1024, 512, EXACT, 3, 11, True), P.RANK, P.TWO_SEARCHES),
    ((5119, 512, EXACT, 3, 11, True), P.RANK, P.TWO_SEARCHES),
    ((5120, 512, EXACT, 3, 11, True), P.RANK, P.ONE_MATRIX),
    ((10000, 512, EXACT, 3, 11, True), P.RANK, P.ONE_MATRIX),
    ((2999, 512, F32, 3, 11, True), P.TWO_SEARCHES, P.TWO_SEARCHES),
    ((3000, 512, F32, 3, 11, True), P.ONE_MATRIX, P.ONE_MATRIX),
    ((5119, 512, BF16X3, 3, 11, True), P.TWO_SEARCHES, P.TWO_SEARCHES),
    ((5120, 512, BF16X3, 3, 11, True), P.ONE_MATRIX, P.ONE_MATRIX),
    ((2000, 512, EXACT, 5, 11, True), P.TWO_SEARCHES, P.TWO_SEARCHES),         # nk = 5: the rank launch takes four k values
    ((6000, 512, EXACT, 5, 11, True), P.ONE_MATRIX, P.ONE_MATRIX),
    ((2000, 512, EXACT, 4, 11, True), P.RANK, P.TWO_SEARCHES),
    ((2000, 96, EXACT, 3, 11, True), P.TWO_SEARCHES, P.TWO_SEARCHES),          # d = 96 is no multiple of 64
    ((6000, 96, EXACT, 3, 11, True), P.ONE_MATRIX, P.ONE_MATRIX),
    ((2000, 512, EXACT, 3, 11, False), P.TWO_SEARCHES, P.TWO_SEARCHES),        # sets of different shape
    ((6000, 512, EXACT, 3, 11, False), P.ONE_MATRIX, P.ONE_MATRIX),
]
WORLD_8 = [
    ((10000, 512, EXACT, 3, 11, True), P.RANK_SHARDED, P.ONE_MATRIX_SHARDED),  # shards of 1 250 rows
    ((1003, 512, EXACT, 3, 11, True), P.TWO_SEARCHES, P.TWO_SEARCHES),         # 3 x 126 + 5 x 125 rows of a gallery under 1 024
    ((10000, 512, EXACT, 5, 11, True), P.ONE_MATRIX_SHARDED, P.ONE_MATRIX_SHARDED),
    ((10000, 96, EXACT, 3, 11, True), P.ONE_MATRIX_SHARDED, P.ONE_MATRIX_SHARDED),
    ((10000, 512, EXACT, 3, 11, False), P.ONE_MATRIX_SHARDED, P.ONE_MATRIX_SHARDED),
    ((10000, 512, EXACT, 3, 40, True), P.RANK_SHARDED, P.TWO_SEARCHES),        # sorted lists deeper than 32: not from block minima
    ((10000, 512, F32, 3, 11, True), P.TWO_SEARCHES, P.TWO_SEARCHES),
    ((10000, 512, BF16X3, 3, 11, True), P.TWO_SEARCHES, P.TWO_SEARCHES),
]
needs_lib = pytest.mark.skipif(not os.path.exists(L.LIB_PATH), reason="libvtc_hip.so is not built (its host-only *_shard_supported decide at world > 1)")


def _check(world, case, rank_on, rank_off):
    n, d, precision, nk, depth, paired = case
    assert vdist.choose_sweep_path(n, d, precision, world, nk, depth, paired=paired, rank_path=True) is rank_on, case
    assert vdist.choose_sweep_path(n, d, precision, world, nk, depth, paired=paired, rank_path=False) is rank_off, case
    default = rank_on if vdist.RANK_PATH else rank_off                        # (VTC_SWEEP_RANK, read at import)
    assert vdist.choose_sweep_path(n, d, precision, world, nk, depth, paired=paired) is default, case
    if nk == 3 and paired:                                                    # what sweep_path() describes
        assert vdist.sweep_path(n, precision, world, depth, d) == LABEL[default], case


@pytest.mark.parametrize("case,rank_on,rank_off", WORLD_1)
def test_world_1_path(monkeypatch, case, rank_on, rank_off):
    monkeypatch.delenv("VTC_SWEEP_SHARD_TWO", raising=False)
    _check(1, case, rank_on, rank_off)
    monkeypatch.setenv("VTC_SWEEP_SHARD_TWO", "1")                              # a knob of the sharded sweep only
    _check(1, case, rank_on, rank_off)


@needs_lib
@pytest.mark.parametrize("case,rank_on,rank_off", WORLD_8)
def test_world_8_path(monkeypatch, case, rank_on, rank_off):
    monkeypatch.delenv("VTC_SWEEP_SHARD_TWO", raising=False)
    _check(8, case, rank_on, rank_off)
    monkeypatch.setenv("VTC_SWEEP_SHARD_TWO", "1")                              # read at call time: set AFTER the import
    _check(8, case, P.TWO_SEARCHES, P.TWO_SEARCHES)
    monkeypatch.setenv("VTC_SWEEP_SHARD_TWO", "0")
    _check(8, case, rank_on, rank_off)


@needs_lib
def test_the_library_answers_the_table_assumes():
    lib = L.lib()
    assert lib.vtc_l2_sweep_shard_supported(10000, 1250, 11) == 1 and lib.vtc_l2_sweep_shard_supported(10000, 1250, 40) == 0
    assert lib.vtc_l2_recall_shard_supported(10000, 1250, 512) == 1 and lib.vtc_l2_recall_shard_supported(10000, 1250, 96) == 0
    assert lib.vtc_l2_recall_shard_supported(1003, 125, 512) == 0 and lib.vtc_l2_sweep_shard_supported(1003, 126, 11) == 0


def test_thresholds_default_to_the_module_constants_and_can_be_passed():
    assert (vdist.RANK_MIN_ROWS, vdist.BIDIR_MIN_ROWS, vdist.BIDIR_MIN_ROWS_F32) == (1024, 5120, 3000)
    assert len(set(LABEL.values())) == 5 and all(p.value == LABEL[p] for p in P)
    # RecallAtK hands its own attributes in (tests set m.bidir_min_rows = 0 and m.rank_path = False)
    assert vdist.choose_sweep_path(600, 512, EXACT, 1, rank_path=True, bidir_min_rows=0) is P.ONE_MATRIX
    assert vdist.choose_sweep_path(600, 512, EXACT, 1, rank_path=True, rank_min_rows=512) is P.RANK
    assert vdist.choose_sweep_path(2999, 512, F32, 1, bidir_min_rows_f32=2999) is P.ONE_MATRIX
    assert vdist.choose_sweep_path(4000, 512, F32, 1, bidir_min_rows=0, bidir_min_rows_f32=4001) is P.TWO_SEARCHES


def test_recallatk_takes_its_defaults_from_dist():
    from vtc_amd.host.metric import RecallAtK
    m = RecallAtK("videos", "titles", [1, 5, 10])
    assert (m.rank_min_rows, m.bidir_min_rows, m.bidir_min_rows_f32, m.rank_path) == (1024, 5120, 3000, vdist.RANK_PATH)
