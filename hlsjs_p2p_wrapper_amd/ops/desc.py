"""Kernel-argument descriptors: pack many small host arrays into ONE host->device copy.

Every batched kernel needs per-segment metadata (offsets, lengths, prefix tables, round
keys, IVs).  Issuing one ``hipMemcpyAsync`` per array costs ~5-10 µs each on the launch
path; instead the arrays are laid out (16-byte aligned) in a single pinned staging buffer,
copied with one non-blocking H2D on the current stream, and handed to the kernels as
typed views of the device copy.  The pinned buffer comes from PyTorch's caching host
allocator, which records the stream use, so reuse is safe without a sync.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch


def check_ranges(op: str, what: str, offs: np.ndarray, lens: np.ndarray, numel: int) -> None:
    """Reject byte ranges ``[offs[i], offs[i] + lens[i])`` that do not lie inside a tensor of
    ``numel`` bytes, before the op branches on the device: the device bindings trust their
    descriptors, and ``-16 + 16 <= numel`` lets a negative offset through an upper-bound test.
    ``what`` names the tensor (``source`` / ``destination`` / ``ES``) in the message."""
    if offs.shape != lens.shape:
        raise ValueError(f"{op}: {what} offsets and lengths differ in size")
    if np.any(offs < 0):
        raise ValueError(f"{op}: negative {what} offset")
    if np.any(lens < 0):
        raise ValueError(f"{op}: negative length")
    if np.any(offs + lens > numel):
        raise ValueError(f"{op}: {what} range out of bounds")


def pack_to_device(arrays: Dict[str, np.ndarray], device: torch.device) -> Dict[str, torch.Tensor]:
    """Copy ``arrays`` to ``device`` in one transfer; returns typed device views.

    ``uint32`` arrays come back as ``int32`` views (same bits)."""
    if device.type == "cuda":  # native: one memcpy per array into the pinned block, one H2D
        from ._native import device as _dev

        idx = device.index if device.index is not None else torch.cuda.current_device()
        return dict(zip(arrays.keys(), _dev().pack_h2d(list(arrays.values()), idx)))
    if device.type != "cpu":
        raise ValueError(f"pack_to_device: unsupported device {device}")
    host = {name: np.ascontiguousarray(a) for name, a in arrays.items()}
    return {k: torch.from_numpy((a.view(np.int32) if a.dtype == np.uint32 else a).copy()) for k, a in host.items()}
