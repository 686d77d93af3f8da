"""Remux of demuxed and indexed segments to fMP4 samples and ``mdat`` boxes
(``docs/REMUX.md`` holds the rules).

:func:`remux_batch` takes the :class:`~.tsdemux.DemuxResult` of a batch and its
:class:`~.esindex.EsIndex` and writes, per segment (identical for the gfx950 kernels and the
host implementation, tables and bytes):

* into the caller's ``out`` buffer at ``out_offs[i]``: an ``mdat`` box whose payload holds every
  kept NAL unit as a 4-byte big-endian length plus its bytes, then, at the next multiple of 16,
  an ``mdat`` box with the bodies of the counted ADTS frames;
* ``vsamples[i, a] = (offset, size, duration, cts, flags)`` per access unit;
* ``asamples[i, f] = (offset, size)`` per AAC frame;
* ``rinfo[i]`` = status bits and totals (slot names in :data:`RINFO`).

Everything the device path reads is already in HBM after ``index_batch``, so
demux -> index -> remux needs no host round trip; ``caps`` size the grid and bound every access.
The ``moof`` that goes with the boxes is host work: ``player/fmp4.py``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np
import torch

from ._native import device as _dev
from ._native import runtime as _rt
from .desc import check_ranges
from .esindex import BatchPlan, EsIndex
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


def layout_out(caps: Sequence[int], max_nal: int, align: int = OUT_ALIGN) -> Tuple[np.ndarray, int]:
    """``(out_offs, size)``: one region of :func:`remux_out_bytes` per segment at ``align``-ed
    offsets, and the bytes of a buffer that holds them all."""
    region = remux_out_bytes(np.asarray(caps, dtype=np.int64), int(max_nal))
    padded = (region + align - 1) // align * align
    offs = np.zeros(len(padded), dtype=np.int64)
    if len(padded):
        np.cumsum(padded[:-1], out=offs[1:])
    return offs, int(padded.sum())


@dataclass
class Remuxed:
    rinfo: torch.Tensor     # int64[B, RINFO_WORDS]
    vsamples: torch.Tensor  # int32[B, max_pes, ES_VSAMPLE_WORDS]
    asamples: torch.Tensor  # int32[B, max_aframes, ES_ASAMPLE_WORDS]
    out: torch.Tensor       # uint8, the caller's buffer
    out_offs: np.ndarray    # int64[B]

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
                max_aframes: int = DEFAULT_MAX_AFRAMES) -> Remuxed:
    """Remux every segment of a demuxed and indexed batch on the device its tensors live on.
    ``caps`` are what ``index_batch`` took; segment i's boxes go to ``out[out_offs[i]:]``, a region
    of :func:`remux_out_bytes` bytes (:func:`layout_out` lays them out) of which only the box
    headers and payloads are written."""
    oo = np.asarray(out_offs, dtype=np.int64)
    B, max_pes, dev, rt = len(res.es_offs), int(res.pes.shape[2]), res.es.device, _rt()
    max_nal = int(ix.nal.shape[1])
    max_aframes = int(max_aframes)
    if max_aframes <= 0:
        raise ValueError("remux_batch: max_aframes must be positive")
    if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous():
        raise ValueError("remux_batch: out must be a contiguous one-dimensional uint8 tensor")
    if out.device != dev or ix.nal.device != dev:
        raise ValueError("remux_batch: the batch, its index and out must be on one device")
    if tuple(ix.nal.shape) != (B, max_nal, rt.ES_NAL_WORDS) or tuple(ix.au.shape) != (B, max_pes, rt.ES_AU_WORDS) \
            or tuple(ix.aframes.shape) != (B, max_pes, rt.ES_APES_WORDS) \
            or tuple(ix.sinfo.shape) != (B, rt.ES_SINFO_WORDS):
        raise ValueError("remux_batch: the index does not belong to this batch")
    plan = BatchPlan("remux_batch", res, caps)
    region = remux_out_bytes(plan.cap, max_nal)
    check_ranges("remux_batch", "output", oo, region, out.numel())
    order = np.argsort(oo, kind="stable")
    if np.any(oo[order][1:] < (oo + region)[order][:-1]):
        raise ValueError("remux_batch: output regions overlap")
    rx = Remuxed(plan.table(0, RINFO_WORDS, torch.int64), plan.table(max_pes, rt.ES_VSAMPLE_WORDS),
                 plan.table(max_aframes, rt.ES_ASAMPLE_WORDS), out, oo)
    if dev.type == "cpu":
        rt.remux_batch(res.es.numpy(), plan.eo, plan.cap, res.info.numpy(), res.pes.numpy(), max_pes, max_nal,
                       ix.nal.numpy(), ix.au.numpy(), ix.aframes.numpy(), ix.sinfo.numpy(), max_aframes,
                       rx.vsamples.numpy(), rx.asamples.numpy(), rx.rinfo.numpy(), out.numpy(), oo)
        return rx
    tile = _dev().remux_tile_bytes()
    d, total_tiles = plan.on_device(region, "output region", tile, oo=("output", oo, OUT_ALIGN))
    scratch = torch.empty(_dev().remux_scratch_words(B, max_nal, max_aframes), dtype=torch.int32, device=dev)
    if B:
        _dev().remux(res.es, d["eo"], d["cap"], d["tp"], total_tiles, res.info, res.pes, max_pes, max_nal, ix.nal,
                     ix.au, ix.aframes, ix.sinfo, max_aframes, scratch, rx.vsamples, rx.asamples, rx.rinfo, out,
                     d["oo"])
    return rx
