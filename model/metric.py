from vtc_amd.host.metric import BaseMetric, RecallAtK, rank_statistics  # noqa: F401
