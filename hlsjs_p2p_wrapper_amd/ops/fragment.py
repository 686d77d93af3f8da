"""The ``moof`` boxes of remuxed segments, written where the ``mdat`` boxes are
(``docs/FRAGMENT.md`` holds the rules).

:func:`fragment_batch` takes the :class:`~.remux.Remuxed` of a batch, made with room in front of
every region (``headroom``) and in front of every audio box (``audio_gap``), and writes per
segment (identical for the gfx950 kernel and the host implementation, row and bytes):

* the video ``moof`` so that it ends at ``out_offs[i]``, where the video ``mdat`` starts, and the
  audio ``moof`` so that it ends at ``out_offs[i] + A0``, where the audio ``mdat`` starts: each
  fragment is one byte range of ``out`` (:meth:`Fragments.video` / :meth:`Fragments.audio`);
* ``finfo[i]`` = status bits, the two box sizes, the two ``tfdt`` values and the time base that
  was used (slot names in :data:`FINFO`).

The boxes are byte for byte what ``player/fmp4.py:video_moof`` / ``audio_moof`` pack on the host.
The ``tfdt`` values are relative to a time base and unwrapped against a reference time, as
hls.js's remuxer does with ``_initPTS`` and ``_PTSNormalize``; a segment can also set the base
itself (``anchor``).  Everything the device path reads is already in HBM after ``remux_batch``;
the host adds one row of parameters per segment.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from ._native import device as _dev
from ._native import runtime as _rt
from .desc import pack_to_device
from .esindex import EsIndex
from .remux import OUT_ALIGN, RINFO, Remuxed

FINFO = {"status": 0, "video_moof_bytes": 1, "audio_moof_bytes": 2, "video_tfdt": 3, "audio_tfdt": 4, "time_base": 5,
         "n_asamples": 6, "spare": 7}
FINFO_WORDS = 8
FSTATUS = {"time_clamped": 1, "no_rate": 2}
FPARAM = {"out_off": 0, "region": 1, "sequence": 2, "time_base": 3, "time_ref": 4, "anchor": 5}
FPARAM_WORDS = 8


def moof_video_bytes(m):
    """Bytes of the video ``moof`` of ``m`` samples (scalar or array): ``88 + 16 m``."""
    return _rt().moof_video_bytes(m)


def moof_audio_bytes(n):
    """Bytes of the audio ``moof`` of ``n`` frames (scalar or array): ``96 + 4 n``."""
    return _rt().moof_audio_bytes(n)


def frag_headroom(max_pes: int) -> int:
    """The ``headroom`` of ``layout_out`` that holds any video ``moof`` of a batch with ``max_pes``
    sample rows: :func:`moof_video_bytes` rounded up to the output alignment."""
    return _rt().frag_headroom(int(max_pes))


def frag_audio_gap(max_aframes: int) -> int:
    """The ``audio_gap`` of ``remux_batch`` that holds any audio ``moof`` of ``max_aframes`` frame
    rows: :func:`moof_audio_bytes` rounded up to 16."""
    return _rt().frag_audio_gap(int(max_aframes))


@dataclass
class Fragments:
    finfo: torch.Tensor  # int64[B, FINFO_WORDS]
    rx: Remuxed          # the batch's remux: its out buffer now holds the moof boxes too

    def _view(self, i: int, moof_slot: str, start_slot: Optional[str], payload_slot: str, host=None) -> torch.Tensor:
        """``host``: the ``(finfo, rinfo)`` rows of segment i as numpy, where the caller has them;
        else this syncs on two small reads."""
        fi, ri = host if host is not None else (self.finfo[i].cpu().numpy(), self.rx.rinfo[i].cpu().numpy())
        end = int(self.rx.out_offs[i]) + (int(ri[RINFO[start_slot]]) if start_slot else 0)
        return self.rx.out[end - int(fi[FINFO[moof_slot]]):end + 8 + int(ri[RINFO[payload_slot]])]

    def video(self, i: int, host=None) -> torch.Tensor:
        """Segment i's video fragment, ``moof`` + ``mdat``: one contiguous view of ``out``."""
        return self._view(i, "video_moof_bytes", None, "video_payload_bytes", host)

    def audio(self, i: int, host=None) -> torch.Tensor:
        """Segment i's audio fragment, ``moof`` + ``mdat``: one contiguous view of ``out``."""
        return self._view(i, "audio_moof_bytes", "audio_box_offset", "audio_payload_bytes", host)

    def segment(self, i: int) -> dict:
        """Host view of segment ``i`` (syncs): the ``finfo`` fields by name and both fragments as
        bytes (``video`` / ``audio``)."""
        host = (self.finfo[i].cpu().numpy(), self.rx.rinfo[i].cpu().numpy())
        out = {k: int(host[0][v]) for k, v in FINFO.items()}
        out["video"] = self.video(i, host).cpu().numpy().tobytes()
        out["audio"] = self.audio(i, host).cpu().numpy().tobytes()
        return out


def _per_segment(name: str, value, B: int, default: int, dtype=np.int64) -> np.ndarray:
    if value is None:
        return np.full(B, default, dtype=dtype)
    if isinstance(value, torch.Tensor):
        value = value.cpu().numpy()
    arr = np.asarray(value).astype(dtype, copy=False).reshape(-1)
    if arr.shape != (B,):
        raise ValueError(f"fragment_batch: {name} must hold one value per segment")
    return arr


def fragment_batch(rx: Remuxed, ix: EsIndex, sequence_numbers: Sequence[int], time_base=None, time_ref=None,
                   anchor=None, mpeg_audio=None) -> Fragments:
    """Write both ``moof`` boxes of every segment of a remuxed batch on the device its tensors
    live on.  ``rx`` was made with ``headroom >= frag_headroom(max_pes)`` and ``audio_gap >=
    frag_audio_gap(max_aframes)``; ``ix`` is the batch's index (its ``sinfo`` holds the audio
    sample rate).  Per segment: ``sequence_numbers`` (``mfhd``, modulo 2^32), ``time_base``
    (default 0), ``time_ref`` (default -1: no unwrap) and ``anchor`` (default off; where set the
    segment's first stamp lands on ``time_ref``, which must then be >= 0).  ``mpeg_audio`` is the
    batch's :class:`~.mpegaudio.MpegAudio` (or its ``mpainfo`` tensor): a segment whose row has a
    config takes its audio ``tfhd`` default duration and its ``tfdt`` rate from there instead of
    1,024 and ``sinfo`` (``docs/MPEGAUDIO.md``)."""
    rt = _rt()
    B, max_pes, max_aframes = int(rx.rinfo.shape[0]), int(rx.vsamples.shape[1]), int(rx.asamples.shape[1])
    dev = rx.out.device
    if tuple(rx.rinfo.shape) != (B, rt.ES_RINFO_WORDS) \
            or tuple(rx.vsamples.shape) != (B, max_pes, rt.ES_VSAMPLE_WORDS) \
            or tuple(rx.asamples.shape) != (B, max_aframes, rt.ES_ASAMPLE_WORDS) or len(rx.out_offs) != B \
            or tuple(ix.sinfo.shape) != (B, rt.ES_SINFO_WORDS) or rx.region is None or len(rx.region) != B:
        raise ValueError("fragment_batch: the remux and the index do not belong to one batch")
    if any(t.device != dev for t in (rx.rinfo, rx.vsamples, rx.asamples, ix.sinfo)):
        raise ValueError("fragment_batch: the remux, its index and out must be on one device")
    if any(not t.is_contiguous() for t in (rx.rinfo, rx.vsamples, rx.asamples, ix.sinfo, rx.out)) \
            or rx.out.dtype != torch.uint8 or rx.out.dim() != 1:
        raise ValueError("fragment_batch: the tables and out must be contiguous, out one-dimensional uint8")
    if max_pes <= 0 or max_aframes <= 0:
        raise ValueError("fragment_batch: the sample tables have no rows")
    headroom, gap = int(rx.headroom), int(rx.audio_gap)
    if headroom < frag_headroom(max_pes):
        raise ValueError(f"fragment_batch: headroom {headroom} is below frag_headroom({max_pes}) = "
                         f"{frag_headroom(max_pes)}")
    if gap < frag_audio_gap(max_aframes) or gap % 16:
        raise ValueError(f"fragment_batch: audio_gap {gap} is below frag_audio_gap({max_aframes}) = "
                         f"{frag_audio_gap(max_aframes)} or no multiple of 16")
    oo = np.asarray(rx.out_offs, dtype=np.int64)
    region = np.asarray(rx.region, dtype=np.int64)
    # the headroom belongs to the segment: inside out, and no other segment's bytes
    if np.any(oo < headroom) or np.any(region < gap + 32) or np.any(oo + region > rx.out.numel()):
        raise ValueError("fragment_batch: a region or its headroom lies outside out")
    order = np.argsort(oo, kind="stable")
    if np.any((oo - headroom)[order][1:] < (oo + region)[order][:-1]):
        raise ValueError("fragment_batch: a headroom overlaps another segment's region")
    fp = np.zeros((B, FPARAM_WORDS), dtype=np.int64)
    fp[:, FPARAM["out_off"]] = oo
    fp[:, FPARAM["region"]] = region
    fp[:, FPARAM["sequence"]] = _per_segment("sequence_numbers", sequence_numbers, B, 0)
    fp[:, FPARAM["time_base"]] = _per_segment("time_base", time_base, B, 0)
    fp[:, FPARAM["time_ref"]] = _per_segment("time_ref", time_ref, B, -1)
    fp[:, FPARAM["anchor"]] = _per_segment("anchor", anchor, B, 0, dtype=bool)
    if np.any((fp[:, FPARAM["anchor"]] != 0) & (fp[:, FPARAM["time_ref"]] < 0)):
        raise ValueError("fragment_batch: an anchored segment needs a time_ref >= 0")
    mpainfo = getattr(mpeg_audio, "mpainfo", mpeg_audio)
    if mpainfo is not None and (not isinstance(mpainfo, torch.Tensor) or mpainfo.dtype != torch.int64
                                or tuple(mpainfo.shape) != (B, rt.ES_MPAINFO_WORDS) or mpainfo.device != dev
                                or not mpainfo.is_contiguous()):
        raise ValueError("fragment_batch: mpeg_audio does not belong to this batch")
    fr = Fragments(torch.empty((B, FINFO_WORDS), dtype=torch.int64, device=dev), rx)
    if dev.type == "cpu":
        rt.fragment_batch(rx.rinfo.numpy(), rx.vsamples.numpy(), rx.asamples.numpy(), ix.sinfo.numpy(), fp, max_pes,
                          max_aframes, headroom, gap, rx.out.numpy(), fr.finfo.numpy(),
                          None if mpainfo is None else mpainfo.numpy())
        return fr
    if np.any(oo % OUT_ALIGN):
        raise ValueError(f"fragment_batch: output offsets must be {OUT_ALIGN}-byte aligned on device")
    if B:
        d = pack_to_device({"fp": fp.reshape(-1)}, dev)
        _dev().fragment_moof(rx.rinfo, rx.vsamples, rx.asamples, ix.sinfo, d["fp"], max_pes, max_aframes, headroom, gap,
                             rx.out, fr.finfo, mpainfo)
    return fr
