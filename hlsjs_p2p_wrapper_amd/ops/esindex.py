"""Sample index of demuxed segments: NAL units, access units and ADTS frames
(``docs/ESINDEX.md`` holds the rules).

:func:`index_batch` takes the :class:`~.tsdemux.DemuxResult` of a batch and returns, per
segment (identical for the gfx950 kernels and the host implementation):

* ``nal[i, k] = (offset, length, type, access unit)`` of the k-th NAL unit of the video ES
  (Annex-B start codes; offsets relative to the video ES; emulation prevention stays);
* ``au[i, a] = (first NAL, NAL count, flags, size)`` per video PES (:data:`AU_FLAGS`);
* ``aframes[i, k] = (ADTS frames, bytes consumed)`` per audio PES;
* ``sinfo[i]`` = status bits and totals (slot names in :data:`SINFO`).

The ES bytes stay where the demux put them and the lengths are read from the ``info`` rows
on the device, so demux -> index needs no host round trip; ``caps`` (the host upper bounds
the demux was sized with) size the grid and bound every access.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from ._native import device as _dev
from ._native import runtime as _rt
from .desc import check_ranges, pack_to_device
from .tsdemux import DemuxResult

SINFO = {"status": 0, "n_nal": 1, "n_au": 2, "n_keyframe_aus": 3, "first_keyframe_au": 4, "n_adts_frames": 5,
         "audio_sample_rate": 6, "audio_channels": 7}
SINFO_WORDS = 8
SSTATUS = {"nal_overflow": 1, "adts_error": 2, "unsupported_video": 4}
AU_FLAGS = {"keyframe": 1, "sps": 2, "pps": 4, "aud": 8}
DEFAULT_MAX_NAL = 2048


@dataclass
class EsIndex:
    nal: torch.Tensor      # int32[B, max_nal, ES_NAL_WORDS]
    au: torch.Tensor       # int32[B, max_pes, ES_AU_WORDS]
    aframes: torch.Tensor  # int32[B, max_pes, ES_APES_WORDS]
    sinfo: torch.Tensor    # int64[B, SINFO_WORDS]

    def segment(self, i: int) -> dict:
        """Host view of segment ``i`` (syncs): the ``sinfo`` fields by name, ``independent``
        (access unit 0 holds a keyframe) and the filled rows of the three tables."""
        sinfo = self.sinfo[i].cpu().numpy()
        out = {k: int(sinfo[v]) for k, v in SINFO.items()}
        out["independent"] = out["first_keyframe_au"] == 0
        out["nal"] = self.nal[i, :min(out["n_nal"], self.nal.shape[1])].cpu().numpy()
        out["au"] = self.au[i, :out["n_au"]].cpu().numpy()
        af = self.aframes[i].cpu().numpy()
        out["aframes"] = af[af[:, 0] >= 0]
        return out


class BatchPlan:
    """What every op on a demuxed batch settles before its launch, once: the batch's arrays with
    the ES ranges checked (``op`` names the caller in every message), one allocation per result
    table on the batch's device, and for the device path the launch rules, the tile space and the
    packed descriptors.  :func:`index_batch` takes it as it is; the ops behind it take an
    :class:`IndexedBatch`."""

    __slots__ = ("op", "es", "eo", "cap", "B", "max_pes", "dev")

    def __init__(self, op: str, res: DemuxResult, caps: Sequence[int]):
        self.op, self.es = op, res.es
        self.eo = np.asarray(res.es_offs, dtype=np.int64)
        self.cap = np.asarray(caps, dtype=np.int64)
        self.B = len(self.eo)
        self.max_pes = int(res.pes.shape[2])
        self.dev = res.es.device
        check_ranges(op, "ES", self.eo, self.cap, res.es.numel())

    def table(self, rows: int, words: int, dtype: torch.dtype = torch.int32) -> torch.Tensor:
        """One result table ``[B, rows, words]`` (``rows == 0``: ``[B, words]``) on the batch's
        device; the CPU path hands its ``.numpy()`` view to the runtime."""
        return torch.empty((self.B, rows, words) if rows else (self.B, words), dtype=dtype, device=self.dev)

    def on_device(self, sized: np.ndarray, what: str, tile: int, **offsets) -> Tuple[Dict[str, torch.Tensor], int]:
        """The device path's descriptors ``eo`` / ``cap`` / ``tp`` plus one per ``offsets`` entry
        ``key=(name, array, alignment)``, and the tile count: ``sized[i]`` bytes of segment i
        (``what`` in the message) are cut into tiles of ``tile`` bytes.  ``tile == 0``: an op
        without a tile space (one workgroup per segment): no ``tp``, a tile count of 0."""
        op, es = self.op, self.es
        arrays = {"eo": self.eo, "cap": self.cap, "tp": None} if tile else {"eo": self.eo, "cap": self.cap}
        for key, (name, offs, align) in (("eo", ("ES", self.eo, 16)), *offsets.items()):
            if np.any(offs % align):
                raise ValueError(f"{op}: {name} offsets must be {align}-byte aligned on device")
            arrays[key] = offs
        if np.any(sized >= 2 ** 31 - tile):
            raise ValueError(f"{op}: a segment's {what} must be below 2 GiB")
        # the video ES is read in dwords: a segment may not reach into a trailing partial dword of the buffer
        if np.any(self.eo + self.cap > es.numel() - es.numel() % 4):
            raise ValueError(f"{op}: ES range reaches the buffer's last partial dword on device")
        if not tile:
            return pack_to_device(arrays, self.dev), 0
        tile_prefix = np.zeros(self.B + 1, dtype=np.int64)
        np.cumsum((sized + tile - 1) // tile, out=tile_prefix[1:])
        arrays["tp"] = tile_prefix
        return pack_to_device(arrays, self.dev), int(tile_prefix[-1])


class IndexedBatch(BatchPlan):
    """A :class:`BatchPlan` that also holds the batch's index: what ``remux_batch``,
    ``config_batch``, ``hevc_config_batch``, ``sample_decrypt_batch`` and ``caption_batch`` check
    and hand to their native call.  The batch and its index are on one device, the four index
    tables have the shapes of this batch, ``es`` is a contiguous one-dimensional uint8 tensor and
    ``nal`` contiguous, and the ES ranges lie inside ``es``."""

    __slots__ = ("res", "ix", "max_nal")

    def __init__(self, op: str, res: DemuxResult, ix: EsIndex, caps: Sequence[int]):
        B, max_pes, max_nal, rt = len(res.es_offs), int(res.pes.shape[2]), int(ix.nal.shape[1]), _rt()
        if ix.nal.device != res.es.device:
            raise ValueError(f"{op}: the batch and its index must be on one device")
        if res.es.dtype != torch.uint8 or res.es.dim() != 1 or not res.es.is_contiguous() or not ix.nal.is_contiguous():
            raise ValueError(f"{op}: es must be a contiguous one-dimensional uint8 tensor, nal contiguous")
        if tuple(ix.nal.shape) != (B, max_nal, rt.ES_NAL_WORDS) or tuple(ix.au.shape) != (B, max_pes, rt.ES_AU_WORDS) \
                or tuple(ix.aframes.shape) != (B, max_pes, rt.ES_APES_WORDS) \
                or tuple(ix.sinfo.shape) != (B, rt.ES_SINFO_WORDS):
            raise ValueError(f"{op}: the index does not belong to this batch")
        super().__init__(op, res, caps)
        self.res, self.ix, self.max_nal = res, ix, max_nal

    def host_args(self) -> tuple:
        """The eleven arguments every runtime entry point on an indexed batch starts with, as numpy views."""
        res, ix = self.res, self.ix
        return (res.es.numpy(), self.eo, self.cap, res.info.numpy(), res.pes.numpy(), self.max_pes, self.max_nal,
                ix.nal.numpy(), ix.au.numpy(), ix.aframes.numpy(), ix.sinfo.numpy())

    def device_args(self, d: Dict[str, torch.Tensor]) -> tuple:
        """The same eleven as tensors for ``_C``; ``d`` holds :meth:`on_device`'s ``eo`` and ``cap``."""
        res, ix = self.res, self.ix
        return (res.es, d["eo"], d["cap"], res.info, res.pes, self.max_pes, self.max_nal, ix.nal, ix.au, ix.aframes,
                ix.sinfo)


def index_batch(res: DemuxResult, caps: Sequence[int], max_nal: int = DEFAULT_MAX_NAL) -> EsIndex:
    """Index every segment of a demuxed batch on the device its tensors live on.  ``caps[i]``
    bounds segment i's ES bytes (what ``demux_batch`` was sized with)."""
    max_nal = int(max_nal)
    if max_nal <= 0:
        raise ValueError("index_batch: max_nal must be positive")
    plan = BatchPlan("index_batch", res, caps)
    B, max_pes, rt = plan.B, plan.max_pes, _rt()
    ix = EsIndex(plan.table(max_nal, rt.ES_NAL_WORDS), plan.table(max_pes, rt.ES_AU_WORDS),
                 plan.table(max_pes, rt.ES_APES_WORDS), plan.table(0, SINFO_WORDS, torch.int64))
    if plan.dev.type == "cpu":
        rt.index_batch(res.es.numpy(), plan.eo, plan.cap, res.info.numpy(), res.pes.numpy(), max_pes, max_nal,
                       ix.nal.numpy(), ix.au.numpy(), ix.aframes.numpy(), ix.sinfo.numpy())
        return ix
    d, total_tiles = plan.on_device(plan.cap, "ES", _dev().es_index_tile_bytes())
    scratch = torch.empty(_dev().es_index_scratch_words(total_tiles, B, max_nal), dtype=torch.int32, device=plan.dev)
    if B:
        _dev().es_index(res.es, d["eo"], d["cap"], d["tp"], total_tiles, res.info, res.pes, max_pes, max_nal, scratch,
                        ix.nal, ix.au, ix.aframes, ix.sinfo)
    return ix
