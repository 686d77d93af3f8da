"""Remux of demuxed and indexed segments to fMP4 samples and ``mdat`` boxes
(``docs/REMUX.md`` holds the rules).

:func:`remux_batch` takes the :class:`~.tsdemux.DemuxResult` of a batch and its
:class:`~.esindex.EsIndex` and writes, per segment (identical for the gfx950 kernels and the
host implementation, tables and bytes):

* into the caller's ``out`` buffer at ``out_offs[i]``: an ``mdat`` box whose payload holds every
  kept NAL unit as a 4-byte big-endian length plus its bytes, then, at the next multiple of 16,
  an ``mdat`` box with the bodies of the counted ADTS frames (``audio_gap`` free bytes in front of it
  on request: room for the audio ``moof`` of ``ops/fragment.py``);
* ``vsamples[i, a] = (offset, size, duration, cts, flags)`` per access unit;
* ``asamples[i, f] = (offset, size)`` per AAC frame;
* ``rinfo[i]`` = status bits and totals (slot names in :data:`RINFO`).

Everything the device path reads is already in HBM after ``index_batch``, so
demux -> index -> remux needs no host round trip; ``caps`` size the grid and bound every access.
The ``moof`` that goes with the boxes is host work in ``player/fmp4.py``, or device work in
``ops/fragment.py`` (``docs/FRAGMENT.md``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ._native import device as _dev
from ._native import runtime as _rt
from .desc import check_ranges
from .esindex import EsIndex, IndexedBatch
from .tsdemux import DemuxResult

RINFO = {"status": 0, "video_payload_bytes": 1, "n_vsamples": 2, "audio_box_offset": 3, "audio_payload_bytes": 4,
         "n_aframes": 5, "video_base_dts": 6, "audio_base_pts": 7}
RINFO_WORDS = 8
RSTATUS = {"truncated": 1, "aframe_overflow": 2, "bad_timestamps": 4, "unsupported_video": 8}
SAMPLE_FLAGS = {"sync": 0x02000000, "non_sync": 0x01010000}
DEFAULT_MAX_AFRAMES = 1024
OUT_ALIGN = 256


def remux_out_bytes(cap, max_nal: int):
    """Bytes of a segment's output region (scalar or array ``cap``): ``cap + max_nal + 32``."""
    return _rt().remux_out_bytes(cap, max_nal)


def remux_scratch_words(nseg: int, max_nal: int, max_aframes: int) -> int:
    """``int32`` elements of the device scratch of one ``remux_batch`` call."""
    return _rt().remux_scratch_words(nseg, max_nal, max_aframes)


def layout_out(caps: Sequence[int], max_nal: int, align: int = OUT_ALIGN, headroom: int = 0,
               audio_gap: int = 0) -> Tuple[np.ndarray, int]:
    """``(out_offs, size)``: one region of :func:`remux_out_bytes` per segment at ``align``-ed
    offsets, and the bytes of a buffer that holds them all.  ``audio_gap`` (what
    :func:`remux_batch` will take) makes every region that much longer; ``headroom``, a multiple of
    ``align``, leaves that many bytes in front of every region, inside the buffer: ``out_offs[i]``
    is moved that far into segment i's share (``ops/fragment.py`` writes the video ``moof`` there)."""
    headroom, audio_gap = int(headroom), int(audio_gap)
    if headroom < 0 or headroom % align:
        raise ValueError("layout_out: headroom must be a non-negative multiple of align")
    if audio_gap < 0 or audio_gap % 16:
        raise ValueError("layout_out: audio_gap must be a non-negative multiple of 16")
    region = remux_out_bytes(np.asarray(caps, dtype=np.int64), int(max_nal)) + audio_gap + headroom
    padded = (region + align - 1) // align * align
    offs = np.zeros(len(padded), dtype=np.int64)
    if len(padded):
        np.cumsum(padded[:-1], out=offs[1:])
    return offs + headroom, int(padded.sum())


@dataclass
class Remuxed:
    rinfo: torch.Tensor     # int64[B, RINFO_WORDS]
    vsamples: torch.Tensor  # int32[B, max_pes, ES_VSAMPLE_WORDS]
    asamples: torch.Tensor  # int32[B, max_aframes, ES_ASAMPLE_WORDS]
    out: torch.Tensor       # uint8, the caller's buffer
    out_offs: np.ndarray    # int64[B]
    headroom: int = 0       # bytes the caller says are free in front of every region (layout_out's)
    audio_gap: int = 0      # bytes left free in front of every audio box
    region: Optional[np.ndarray] = None  # int64[B]: bytes of each region from out_offs[i] on, the gap included

    def segment(self, i: int) -> dict:
        """Host view of segment ``i`` (syncs): the ``rinfo`` fields by name, the filled rows of
        both tables and the two boxes as bytes (``video_mdat`` / ``audio_mdat``)."""
        rinfo = self.rinfo[i].cpu().numpy()
        out = {k: int(rinfo[v]) for k, v in RINFO.items()}
        out["vsamples"] = self.vsamples[i, :out["n_vsamples"]].cpu().numpy()
        rows = self.asamples[i].cpu().numpy()
        out["asamples"] = rows[rows[:, 0] >= 0]
        o = int(self.out_offs[i])
        a0 = o + out["audio_box_offset"]
        out["video_mdat"] = self.out[o:o + 8 + out["video_payload_bytes"]].cpu().numpy().tobytes()
        out["audio_mdat"] = self.out[a0:a0 + 8 + out["audio_payload_bytes"]].cpu().numpy().tobytes()
        return out


def remux_batch(res: DemuxResult, ix: EsIndex, caps: Sequence[int], out: torch.Tensor, out_offs: Sequence[int],
                max_aframes: int = DEFAULT_MAX_AFRAMES, audio_gap: int = 0, headroom: int = 0) -> Remuxed:
    """Remux every segment of a demuxed and indexed batch on the device its tensors live on.
    ``caps`` are what ``index_batch`` took; segment i's boxes go to ``out[out_offs[i]:]``, a region
    of :func:`remux_out_bytes` ``+ audio_gap`` bytes (:func:`layout_out` lays them out) of which
    only the box headers and payloads are written.  ``audio_gap``, a non-negative multiple of 16,
    moves the audio box that far back: ``A0 = align16(8 + P + audio_gap)``.  ``headroom`` is only
    recorded: the bytes ``layout_out`` left in front of every region (``docs/FRAGMENT.md``)."""
    oo = np.asarray(out_offs, dtype=np.int64)
    max_aframes, audio_gap, headroom = int(max_aframes), int(audio_gap), int(headroom)
    if max_aframes <= 0:
        raise ValueError("remux_batch: max_aframes must be positive")
    if audio_gap < 0 or audio_gap % 16 or audio_gap >= 2 ** 30:
        raise ValueError("remux_batch: audio_gap must be a non-negative multiple of 16")
    if headroom < 0:
        raise ValueError("remux_batch: headroom must not be negative")
    if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous():
        raise ValueError("remux_batch: out must be a contiguous one-dimensional uint8 tensor")
    if out.device != res.es.device:
        raise ValueError("remux_batch: the batch, its index and out must be on one device")
    batch = IndexedBatch("remux_batch", res, ix, caps)
    B, max_pes, max_nal, rt = batch.B, batch.max_pes, batch.max_nal, _rt()
    region = remux_out_bytes(batch.cap, max_nal) + audio_gap
    check_ranges("remux_batch", "output", oo, region, out.numel())
    order = np.argsort(oo, kind="stable")
    if np.any(oo[order][1:] < (oo + region)[order][:-1]):
        raise ValueError("remux_batch: output regions overlap")
    rx = Remuxed(batch.table(0, RINFO_WORDS, torch.int64), batch.table(max_pes, rt.ES_VSAMPLE_WORDS),
                 batch.table(max_aframes, rt.ES_ASAMPLE_WORDS), out, oo, headroom, audio_gap, region)
    if batch.dev.type == "cpu":
        rt.remux_batch(*batch.host_args(), max_aframes, rx.vsamples.numpy(), rx.asamples.numpy(), rx.rinfo.numpy(),
                       out.numpy(), oo, audio_gap)
        return rx
    d, total_tiles = batch.on_device(region, "output region", _dev().remux_tile_bytes(), oo=("output", oo, OUT_ALIGN))
    scratch = torch.empty(_dev().remux_scratch_words(B, max_nal, max_aframes), dtype=torch.int32, device=batch.dev)
    if B:
        a = batch.device_args(d)  # the tile space goes behind es, eo and cap
        _dev().remux(*a[:3], d["tp"], total_tiles, *a[3:], max_aframes, scratch, rx.vsamples, rx.asamples, rx.rinfo,
                     out, d["oo"], audio_gap)
    return rx
