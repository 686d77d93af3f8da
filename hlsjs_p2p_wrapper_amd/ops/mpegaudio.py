"""MPEG audio (MP3 and its Layer I / II relatives) tracks of demuxed MPEG-TS segments, behind the
remux (``docs/MPEGAUDIO.md`` holds the rules).

The index, the remux and the codec configuration walk ADTS AAC only: for a segment whose PMT says
stream type ``0x03`` / ``0x04`` they leave an empty audio ``mdat``.  :func:`mpeg_audio_batch` takes
the :class:`~.tsdemux.DemuxResult` of a batch and the :class:`~.remux.Remuxed` that
``remux_batch`` returned for it, and for every segment whose audio *is* MPEG audio (identical for
the gfx950 kernels and the host implementation, tables and bytes):

* walks the frames of every audio PES, back to back, all with the version, layer, sample rate and
  channel mode of the first one;
* writes them whole (the header is part of an MP3 sample) behind the audio ``mdat`` header at
  ``A0``, and their ``(offset, size)`` rows into ``rx.asamples``;
* sets ``rx.rinfo``'s ``audio_payload_bytes`` / ``n_aframes`` (and the ``aframe_overflow`` bit);
* reports ``mframes[i, k] = (frames, bytes)`` per audio PES and ``mpainfo[i]`` (slot names in
  :data:`MPAINFO`).

Every other segment keeps each byte ``remux_batch`` left.  The call is made unconditionally: the
codec is only known on the device, and a segment of another codec exits at once.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import numpy as np
import torch

from ._native import device as _dev
from ._native import runtime as _rt
from .desc import check_ranges
from .esindex import BatchPlan
from .remux import OUT_ALIGN, Remuxed
from .tsdemux import DemuxResult

MPAINFO = {"status": 0, "n_frames": 1, "sample_rate": 2, "channels": 3, "version": 4, "layer": 5, "frame_samples": 6,
           "bitrate": 7}
MPAINFO_WORDS = 8
MPASTATUS = {"not_mpeg_audio": 1, "no_audio_config": 2, "mpa_error": 4, "format_change": 8, "aframe_overflow": 16}
NO_CONFIG = MPASTATUS["not_mpeg_audio"] | MPASTATUS["no_audio_config"]
AUDIO_TYPES = (0x03, 0x04)


@dataclass
class MpegAudio:
    mframes: torch.Tensor  # int32[B, max_pes, ES_APES_WORDS]
    mpainfo: torch.Tensor  # int64[B, MPAINFO_WORDS]
    rx: Remuxed            # the batch's remux: asamples, rinfo and out now hold the MPEG audio frames

    def segment(self, i: int) -> dict:
        """Host view of segment ``i`` (syncs): the ``mpainfo`` fields by name, ``status_names``,
        ``has_config`` and the recorded ``mframes`` rows."""
        row = self.mpainfo[i].cpu().numpy()
        out = {k: int(row[v]) for k, v in MPAINFO.items()}
        out["status_names"] = [k for k, v in MPASTATUS.items() if out["status"] & v]
        out["has_config"] = not out["status"] & NO_CONFIG
        mf = self.mframes[i].cpu().numpy()
        out["mframes"] = mf[mf[:, 0] >= 0]
        return out


def mpeg_audio_batch(res: DemuxResult, rx: Remuxed, caps: Sequence[int]) -> MpegAudio:
    """Remux the MPEG audio track of every segment of a demuxed batch on the device its tensors
    live on, on the caller's stream.  ``rx`` is what ``remux_batch`` returned for ``res`` with the
    same ``caps``; its ``asamples``, ``rinfo`` and ``out`` are rewritten for the segments that have
    an MPEG audio config and for no other."""
    op = "mpeg_audio_batch"
    rt = _rt()
    if res.es.dtype != torch.uint8 or res.es.dim() != 1 or not res.es.is_contiguous():
        raise ValueError(f"{op}: es must be a contiguous one-dimensional uint8 tensor")
    plan = BatchPlan(op, res, caps)
    B, max_pes, dev = plan.B, plan.max_pes, plan.dev
    if max_pes <= 0:
        raise ValueError(f"{op}: the batch has no PES rows")
    if rx.asamples.dim() != 3 or rx.region is None:
        raise ValueError(f"{op}: the remux does not belong to this batch")
    max_aframes = int(rx.asamples.shape[1])
    if tuple(rx.rinfo.shape) != (B, rt.ES_RINFO_WORDS) or max_aframes <= 0 \
            or tuple(rx.asamples.shape) != (B, max_aframes, rt.ES_ASAMPLE_WORDS) \
            or len(rx.out_offs) != B or len(rx.region) != B \
            or tuple(res.info.shape) != (B, rt.TS_INFO_WORDS) \
            or tuple(res.pes.shape) != (B, 3, max_pes, rt.TS_PES_WORDS):
        raise ValueError(f"{op}: the remux does not belong to this batch")
    tensors = (res.info, res.pes, rx.rinfo, rx.asamples, rx.out)
    if any(t.device != dev for t in tensors):
        raise ValueError(f"{op}: the batch, its remux and out must be on one device")
    if any(not t.is_contiguous() for t in tensors) or rx.out.dtype != torch.uint8 or rx.out.dim() != 1 \
            or rx.rinfo.dtype != torch.int64 or rx.asamples.dtype != torch.int32 or res.info.dtype != torch.int64 \
            or res.pes.dtype != torch.int64:
        raise ValueError(f"{op}: the tables and out must be contiguous and of their dtypes, out one-dimensional uint8")
    oo = np.asarray(rx.out_offs, dtype=np.int64)
    region = np.asarray(rx.region, dtype=np.int64)
    if np.any(region < plan.cap + 32):
        raise ValueError(f"{op}: a region is shorter than remux_batch makes it")
    check_ranges(op, "output", oo, region, rx.out.numel())
    order = np.argsort(oo, kind="stable")
    if np.any(oo[order][1:] < (oo + region)[order][:-1]):
        raise ValueError(f"{op}: output regions overlap")
    ma = MpegAudio(plan.table(max_pes, rt.ES_APES_WORDS), plan.table(0, MPAINFO_WORDS, torch.int64), rx)
    if dev.type == "cpu":
        rt.mpeg_audio_batch(res.es.numpy(), plan.eo, plan.cap, res.info.numpy(), res.pes.numpy(), max_pes, region,
                            max_aframes, ma.mframes.numpy(), ma.mpainfo.numpy(), rx.asamples.numpy(), rx.rinfo.numpy(),
                            rx.out.numpy(), oo)
        return ma
    d, total_tiles = plan.on_device(region, "output region", _dev().mpeg_audio_tile_bytes(),
                                    oo=("output", oo, OUT_ALIGN), rg=("region", region, 1))
    scratch = torch.empty(_dev().mpa_scratch_words(B, max_pes), dtype=torch.int32, device=dev)
    if B:
        _dev().mpeg_audio(res.es, d["eo"], d["cap"], d["tp"], total_tiles, res.info, res.pes, max_pes, d["rg"],
                          max_aframes, scratch, ma.mframes, ma.mpainfo, rx.asamples, rx.rinfo, rx.out, d["oo"])
    return ma
