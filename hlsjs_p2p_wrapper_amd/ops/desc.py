"""Kernel-argument descriptors: pack many small host arrays into ONE host->device copy.

Every batched kernel needs per-segment metadata (offsets, lengths, prefix tables, round
keys, IVs).  Issuing one ``hipMemcpyAsync`` per array costs ~5-10 µs each on the launch
path; instead the arrays are laid out (16-byte aligned) in a single pinned staging buffer,
copied with one non-blocking H2D on the current stream, and handed to the kernels as
typed views of the device copy.  The pinned buffer comes from PyTorch's caching host
allocator, which records the stream use, so reuse is safe without a sync.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

_DT = {
    np.dtype(np.int64): torch.int64,
    np.dtype(np.int32): torch.int32,
    np.dtype(np.uint8): torch.uint8,
    np.dtype(np.int8): torch.int8,
    np.dtype(np.float64): torch.float64,
    np.dtype(np.uint32): torch.int32,
}


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
    layout: List[Tuple[str, int, np.ndarray]] = []
    off = 0
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        layout.append((name, off, a))
        off += (a.nbytes + 15) & ~15
    total = max(off, 16)
    if device.type == "cpu":
        out = {}
        for name, _, a in layout:
            out[name] = torch.from_numpy(a.copy())
        return out
    host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    for name, o, a in layout:
        hv[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    dev = host.to(device, non_blocking=True)
    out = {}
    for name, o, a in layout:
        t = dev[o:o + a.nbytes].view(_DT[a.dtype])
        out[name] = t
    return out
