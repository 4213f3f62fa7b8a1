"""CPU: rank_statistics on hand-written ranks, the fp64 rank reference of the GPU tests against the oracle's R@K, the --rank-stats flag of
both entry points, and its refusal under WORLD_SIZE > 1."""
import os
import sys

import numpy as np
import pytest
import torch

import rank_refs as RR
from oracle import eval_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rank_statistics_on_hand_written_ranks():
    from model.metric import rank_statistics as reexported
    from vtc_amd.host.metric import rank_statistics
    assert reexported is rank_statistics
    st = rank_statistics([0, 4, 1, 9], (1, 2, 5, 10))                 # even n: the median falls between two ranks
    assert st["recall_at_k"] == {1: 0.25, 2: 0.5, 5: 0.75, 10: 1.0}
    assert st["median_rank"] == 3.5 and st["mean_rank"] == 4.5
    assert st["mrr"] == pytest.approx((1 + 1 / 5 + 1 / 2 + 1 / 10) / 4, rel=1e-15)
    st = rank_statistics(torch.tensor([7, 0, 2]), (1, 3))             # odd n, a tensor
    assert st == {"recall_at_k": {1: 1 / 3, 3: 2 / 3}, "median_rank": 3.0, "mean_rank": 4.0, "mrr": pytest.approx((1 / 8 + 1 + 1 / 3) / 3, rel=1e-15)}
    st = rank_statistics(np.zeros(5, np.int64))                       # every target first
    assert st == {"recall_at_k": {1: 1.0, 5: 1.0, 10: 1.0}, "median_rank": 1.0, "mean_rank": 1.0, "mrr": 1.0}
    st = rank_statistics([3, 1], (50, 2, 4, 1, 3, 7))                 # k beyond the largest rank, more than four k, any order
    assert st["recall_at_k"] == {50: 1.0, 2: 0.5, 4: 1.0, 1: 0.0, 3: 0.5, 7: 1.0}
    assert rank_statistics([5, 5], ())["recall_at_k"] == {}
    with pytest.raises(ValueError):
        rank_statistics([])


@pytest.mark.parametrize("n,d,seed", [(1027, 64, 2), (700, 128, 3)])
def test_reference_ranks_agree_with_the_oracle_recall(n, d, seed):
    a, b = RR.spread_pairs(n, d, seed)
    rank_a, rank_b, gap = RR.reference_ranks(a, b)
    assert gap > 1e-12
    RR.assert_not_degenerate(rank_a, n)
    RR.assert_not_degenerate(rank_b, n)
    for rank, (ga, qu) in ((rank_a, (a, b)), (rank_b, (b, a))):
        for k, r in E.recall_at_k(ga, qu, [1, 5, 10], np.float64):
            assert (rank < k).mean() == r, k


def test_reference_ranks_ties_and_nonfinite_rows():
    a = np.array([[0, 0], [1, 0], [1, 0], [5, 5]], np.float32)
    b = np.array([[1, 0], [1, 0], [1, 0], [5, 4]], np.float32)
    rank_a, rank_b, _ = RR.reference_ranks(a, b)
    # gallery a, query b_0 = (1, 0): a_1 and a_2 are closer than a_0; query b_2: a_1 ties with the target a_2 and has the lower index.
    # gallery b, query a_2 = (1, 0): b_0 and b_1 tie with the target b_2 and have lower indices
    assert rank_a.tolist() == [2, 0, 1, 0] and rank_b.tolist() == [0, 1, 2, 0]
    a[1, 0] = np.nan
    rank_a, rank_b, _ = RR.reference_ranks(a, b)
    assert rank_a.tolist() == [1, 4, 0, 0] and rank_b.tolist() == [0, 4, 2, 0]       # the NaN row: never closer, its own pair rank n


def test_both_entry_points_parse_rank_stats():
    from vtc_amd.host import eval as ev
    from vtc_amd.host import retrieval_evaluation as RE
    assert ev.build_parser().parse_args([]).rank_stats is False and ev.build_parser().parse_args(["--rank-stats"]).rank_stats is True
    assert RE.build_parser().parse_args([]).rank_stats is False
    assert RE.build_parser().parse_args(["-m", "pretrained_clip", "--rank-stats"]).rank_stats is True
    import evaluation.retrieval_evaluation as front
    assert front.compute_rank_table is RE.compute_rank_table


def test_rank_stats_is_refused_under_several_ranks_before_anything_runs(monkeypatch):
    """WORLD_SIZE = 2: main() raises before the process group, the dataset or a device is touched (the config is never read)."""
    from vtc_amd.host import eval as ev
    monkeypatch.setenv("WORLD_SIZE", "2")
    args = ev.build_parser().parse_args(["--rank-stats"])
    with pytest.raises(NotImplementedError, match="sharded counting sweep is not built"):
        ev.main(None, args)
    assert not torch.distributed.is_initialized()
