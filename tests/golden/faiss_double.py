"""Tests-only numpy stand-in for ``faiss`` (faiss-gpu, environment.yml:12: not installed here and GPU-only), shared by the generator
scripts of this directory that run the reference's ``RecallAtK`` (model/metric.py:103-187) unmodified.  Never shipped, never
imported by the product or by a test.

It has the four names metric.py touches (GpuIndexFlatConfig, StandardGpuResources, GpuIndexFlatL2.add/.search).  Its search is faiss's
published exact-L2 definition (squared L2 = |q|^2 + |g|^2 - 2 q.g in fp32, k smallest, ascending); ties -- unspecified in faiss -- by
lowest index.  The stand-in's own arithmetic is NOT evidence about faiss."""
from __future__ import annotations

import collections
import collections.abc
import sys
import types

import numpy as np


class GpuIndexFlatConfig:
    useFloat16 = False
    device = 0


class StandardGpuResources:
    pass


class GpuIndexFlatL2:
    def __init__(self, res, dim, cfg):
        assert cfg.useFloat16 is False                    # metric.py:113
        self.dim, self.x = dim, np.zeros((0, dim), dtype=np.float32)

    def add(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.shape[1] == self.dim
        self.x = np.concatenate([self.x, x])

    def search(self, q, k):
        q = np.ascontiguousarray(q, dtype=np.float32)
        d = (q * q).sum(1)[:, None] + (self.x * self.x).sum(1)[None, :] - np.float32(2) * (q @ self.x.T)
        order = np.argsort(d, axis=1, kind="stable")[:, :k]
        if order.shape[1] < k:                            # faiss pads missing neighbours with -1
            pad = -np.ones((q.shape[0], k - order.shape[1]), dtype=order.dtype)
            return np.take_along_axis(d, order, 1), np.concatenate([order, pad], 1)
        return np.take_along_axis(d, order, 1), order


def install():
    """Register the stand-in as ``faiss`` and restore ``collections.Iterable`` (metric.py:106; gone in Python >= 3.10)."""
    collections.Iterable = collections.abc.Iterable
    faiss = types.ModuleType("faiss")
    faiss.GpuIndexFlatConfig, faiss.StandardGpuResources, faiss.GpuIndexFlatL2 = GpuIndexFlatConfig, StandardGpuResources, GpuIndexFlatL2
    sys.modules["faiss"] = faiss
    return faiss
