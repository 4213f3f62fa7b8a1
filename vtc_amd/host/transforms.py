"""The Resize + CenterCrop half of the reference's CLIP_TRANSFORM (dataset_loaders/dataset_loaders.py:40-49,
video_retrieval_videodatasets.py:21-29) for decoded frames, on the GPU: bit for bit what torchvision's
``Resize(size, BICUBIC)`` + ``CenterCrop(size)`` give on PIL images.  ToTensor + Normalize, the other half, are fused into the
towers' uint8 pixel path, so the result goes straight to ``forward()`` / ``encode_image()``."""
from __future__ import annotations

from typing import List, Sequence, Union

import torch

from .. import ops


class ClipPreprocessGPU:
    """``ClipPreprocessGPU(size)(frames)``: frames is ONE uint8 tensor ``[..., H, W, 3]`` (``layout="chw"``: ``[..., 3, H, W]``) with up to
    two leading dimensions, or a LIST of such tensors of DIFFERENT frame sizes (the videos of a dataset differ); each entry holds one
    frame (rank 3) or a stack of frames (rank 4).  Entries may live on the CPU -- uploaded with ``non_blocking=True``; pin them
    (``tensor.pin_memory()``) for the copy to overlap -- or on the GPU.  A tensor comes back as ``[..., 3, size, size]`` uint8 on the
    device; a list as ONE ``[n, 3, size, size]`` uint8 tensor, n the total number of frames, in input order (entries of one frame size
    share a launch)."""

    def __init__(self, size: int = 224, device: Union[str, torch.device] = "cuda", layout: str = "hwc"):
        if layout not in ("hwc", "chw"):
            raise ValueError(f"ClipPreprocessGPU: layout {layout!r} (\"hwc\" or \"chw\")")
        self.size, self.device, self.layout = int(size), torch.device(device), layout

    def _upload(self, t: torch.Tensor) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise ValueError(f"ClipPreprocessGPU: uint8 tensors expected, got {getattr(t, 'dtype', type(t))}")
        return t if t.is_cuda else t.to(self.device, non_blocking=True)

    def __call__(self, frames: Union[torch.Tensor, Sequence[torch.Tensor]]) -> torch.Tensor:
        if isinstance(frames, torch.Tensor):
            return ops.clip_resize_crop(self._upload(frames), self.size, self.layout)
        items: List[torch.Tensor] = []
        for t in frames:
            t = self._upload(t)
            if t.dim() not in (3, 4):
                raise ValueError(f"ClipPreprocessGPU: list entries hold one frame (rank 3) or a stack of frames (rank 4), got {tuple(t.shape)}")
            items.append(t if t.dim() == 4 else t.unsqueeze(0))
        if not items:
            raise ValueError("ClipPreprocessGPU: empty list")
        if len({t.device for t in items}) != 1:
            raise ValueError("ClipPreprocessGPU: entries on different devices")
        starts, total = [], 0
        for t in items:
            starts.append(total)
            total += t.shape[0]
        out = torch.empty(total, 3, self.size, self.size, dtype=torch.uint8, device=items[0].device)
        groups: dict = {}
        for i, t in enumerate(items):
            groups.setdefault(tuple(t.shape[1:]), []).append(i)
        for idx in groups.values():
            # entries that are neighbours in the output write their rows in place; the others go through one gathered batch
            run = all(b == a + 1 for a, b in zip(idx, idx[1:]))
            batch = items[idx[0]] if len(idx) == 1 else torch.cat([items[i] for i in idx])
            n = batch.shape[0]
            if run:
                ops.clip_resize_crop(batch, self.size, self.layout, out=out[starts[idx[0]]:starts[idx[0]] + n])
                continue
            res = ops.clip_resize_crop(batch, self.size, self.layout)
            o = 0
            for i in idx:
                m = items[i].shape[0]
                out[starts[i]:starts[i] + m] = res[o:o + m]
                o += m
        return out
