"""AC-3 and E-AC-3 tracks of demuxed MPEG-TS segments, behind the remux (``docs/AC3AUDIO.md`` holds
the rules).

The index, the remux and the codec configuration walk ADTS AAC only: for a segment whose PMT says
stream type ``0x81`` / ``0x87`` they leave an empty audio ``mdat``.  :func:`ac3_audio_batch` takes
the :class:`~.tsdemux.DemuxResult` of a batch and the :class:`~.remux.Remuxed` that ``remux_batch``
returned for it (after ``mpeg_audio_batch`` where that runs), and for every segment whose audio *is*
Dolby audio (identical for the gfx950 kernels and the host implementation, tables and bytes):

* walks the syncframes of every audio PES, back to back, all with the codec, ``bsid``, sample rate,
  ``acmod`` and ``lfeon`` of the first one;
* writes them whole behind the audio ``mdat`` header at ``A0``, and their ``(offset, size)`` rows
  into ``rx.asamples``;
* sets ``rx.rinfo``'s ``audio_payload_bytes`` / ``n_aframes`` (and the ``aframe_overflow`` bit);
* reports ``dframes[i, k] = (frames, bytes)`` per audio PES and ``ac3info[i]`` (slot names in
  :data:`AC3INFO`).

``mpainfo`` is a new tensor in :data:`~.mpegaudio.MPAINFO`'s layout: the Dolby track's rate and frame
samples where there is one, else the row of the ``mpeg_audio`` argument (or "not MPEG audio"
without one), so ``fragment_batch(..., mpeg_audio=<Ac3Audio>)`` serves both codecs.  Every other
segment keeps each byte ``remux_batch`` (and ``mpeg_audio_batch``) left.  The call is made
unconditionally: the codec is only known on the device, and a segment of another codec exits at once.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from ._native import device as _dev
from ._native import runtime as _rt
from .desc import check_ranges
from .esindex import BatchPlan
from .mpegaudio import MPAINFO_WORDS, MpegAudio
from .remux import OUT_ALIGN, Remuxed
from .tsdemux import DemuxResult

AC3INFO = {"status": 0, "n_frames": 1, "sample_rate": 2, "channels": 3, "kind": 4, "bsid": 5, "frame_samples": 6,
           "bitrate": 7, "fscod": 8, "bsmod": 9, "acmod": 10, "lfeon": 11, "bit_rate_code": 12, "data_rate": 13,
           "first_frame_bytes": 14}
AC3INFO_WORDS = 16
AC3STATUS = {"not_dolby_audio": 1, "no_audio_config": 2, "ac3_error": 4, "format_change": 8, "aframe_overflow": 16,
             "unsupported_layout": 32}
NO_CONFIG = AC3STATUS["not_dolby_audio"] | AC3STATUS["no_audio_config"]
AUDIO_TYPES = (0x81, 0x87)
KIND_AC3, KIND_EAC3 = 1, 2
FRAME_SAMPLES = 1536


@dataclass
class Ac3Audio:
    dframes: torch.Tensor  # int32[B, max_pes, ES_APES_WORDS]
    ac3info: torch.Tensor  # int64[B, AC3INFO_WORDS]
    mpainfo: torch.Tensor  # int64[B, MPAINFO_WORDS]: what fragment_batch(mpeg_audio=) takes
    rx: Remuxed            # the batch's remux: asamples, rinfo and out now hold the Dolby syncframes

    def segment(self, i: int) -> dict:
        """Host view of segment ``i`` (syncs): the ``ac3info`` fields by name, ``status_names``,
        ``has_config`` and the recorded ``dframes`` rows."""
        row = self.ac3info[i].cpu().numpy()
        out = {k: int(row[v]) for k, v in AC3INFO.items()}
        out["status_names"] = [k for k, v in AC3STATUS.items() if out["status"] & v]
        out["has_config"] = not out["status"] & NO_CONFIG
        df = self.dframes[i].cpu().numpy()
        out["dframes"] = df[df[:, 0] >= 0]
        return out


def ac3_audio_batch(res: DemuxResult, rx: Remuxed, caps: Sequence[int],
                    mpeg_audio: Optional[MpegAudio] = None) -> Ac3Audio:
    """Remux the AC-3 / E-AC-3 track of every segment of a demuxed batch on the device its tensors
    live on, on the caller's stream.  ``rx`` is what ``remux_batch`` returned for ``res`` with the
    same ``caps``; its ``asamples``, ``rinfo`` and ``out`` are rewritten for the segments that have
    a Dolby audio config and for no other.  ``mpeg_audio`` is the batch's
    :class:`~.mpegaudio.MpegAudio` (or its ``mpainfo`` tensor), only read."""
    op = "ac3_audio_batch"
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
    mpa_in = getattr(mpeg_audio, "mpainfo", mpeg_audio)
    if mpa_in is not None and (not isinstance(mpa_in, torch.Tensor) or mpa_in.dtype != torch.int64
                               or tuple(mpa_in.shape) != (B, MPAINFO_WORDS) or not mpa_in.is_contiguous()
                               or mpa_in.device != dev):
        raise ValueError(f"{op}: mpeg_audio does not belong to this batch")
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
    da = Ac3Audio(plan.table(max_pes, rt.ES_APES_WORDS), plan.table(0, AC3INFO_WORDS, torch.int64),
                  plan.table(0, MPAINFO_WORDS, torch.int64), rx)
    if dev.type == "cpu":
        rt.ac3_audio_batch(res.es.numpy(), plan.eo, plan.cap, res.info.numpy(), res.pes.numpy(), max_pes, region,
                           max_aframes, da.dframes.numpy(), da.ac3info.numpy(), da.mpainfo.numpy(), rx.asamples.numpy(),
                           rx.rinfo.numpy(), rx.out.numpy(), oo, None if mpa_in is None else mpa_in.numpy())
        return da
    d, total_tiles = plan.on_device(region, "output region", _dev().ac3_audio_tile_bytes(),
                                    oo=("output", oo, OUT_ALIGN), rg=("region", region, 1))
    scratch = torch.empty(_dev().mpa_scratch_words(B, max_pes), dtype=torch.int32, device=dev)
    if B:
        _dev().ac3_audio(res.es, d["eo"], d["cap"], d["tp"], total_tiles, res.info, res.pes, max_pes, d["rg"],
                         max_aframes, scratch, da.dframes, da.ac3info, da.mpainfo, rx.asamples, rx.rinfo, rx.out,
                         d["oo"], mpa_in)
    return da
