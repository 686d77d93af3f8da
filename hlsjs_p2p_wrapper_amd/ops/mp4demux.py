"""Demux of fragmented-MP4 (CMAF) media segments: what hls.js's ``mp4demuxer``, passthrough remuxer
and ``mp4-tools`` read from a ``.m4s`` fragment (``docs/FMP4DEMUX.md`` holds the rules).

:func:`mp4_demux_batch` moves no payload.  Per segment (identical for the gfx950 kernels and the
host implementation) it returns:

* ``minfo[i]`` = status bits, box counts and per-track totals (slot names in :data:`MINFO` /
  :data:`MINFO_TRACK`);
* ``msamples[i, t, k] = (size, duration, cts, flags)`` of the k-th sample of track slot ``t``
  (0 video, 1 audio);
* ``runs[i, r]``: the r-th ``trun`` of a configured track (slot names in :data:`RUN`);
* ``emsg[i, e]``: the e-th top-level ``emsg`` box (slot names in :data:`EMSG`);
* ``info`` / ``pes`` in the layout of :class:`~.tsdemux.DemuxResult` (the whole segment is the
  video ES; ``pes[i, t, k] = (offset in the segment, pts, dts)`` in the track's timescale) and
  ``nal`` / ``au`` / ``aframes`` / ``sinfo`` in that of :class:`~.esindex.EsIndex`, so
  ``caption_batch`` runs on :meth:`Mp4Demux.as_demux` / :meth:`Mp4Demux.as_index` unchanged.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional, Sequence, Union

import numpy as np
import torch

from ._native import device as _dev
from ._native import runtime as _rt
from .desc import check_ranges, pack_to_device
from .esindex import DEFAULT_MAX_NAL, EsIndex
from .tsdemux import DEFAULT_MAX_PES, DemuxResult

TRACKS = 2
TRACK = {"id": 0, "kind": 1, "codec_type": 2, "nal_length_size": 3, "default_duration": 4, "default_size": 5,
         "default_flags": 6}
TRACK_WORDS = 8
KIND = {"none": 0, "video": 1, "audio": 2}
MINFO = {"status": 0, "n_moof": 1, "first_sequence": 2, "n_run": 3, "n_other_traf": 4, "n_emsg": 5}
MINFO_TRACK = {"n_samples": 0, "base_time": 1, "duration": 2, "min_pts": 3, "max_pts": 4, "first_sync": 5}
MINFO_TRACK0 = 6
MINFO_TRACK_WORDS = 6
MINFO_WORDS = 18
MSTATUS = {"bad_box": 1, "moof_overflow": 2, "emsg_overflow": 4, "run_overflow": 8, "no_tfdt": 16,
           "sample_out_of_range": 32, "sample_overflow": 64, "nal_error": 128, "bad_timestamps": 256}
MSAMPLE = {"size": 0, "duration": 1, "cts": 2, "flags": 3}
MSAMPLE_WORDS = 4
RUN = {"track": 0, "moof": 1, "first": 2, "count": 3, "entries": 4, "flags": 5, "traf_run": 6, "default_duration": 7,
       "default_size": 8, "default_flags": 9, "first_flags": 10, "start": 11, "start_sample": 12, "time": 13,
       "time_sample": 14}
RUN_WORDS = 16
EMSG = {"offset": 0, "size": 1, "version": 2, "timescale": 3, "time": 4, "time_is_delta": 5, "duration": 6, "id": 7,
        "data_offset": 8, "data_length": 9, "is_id3": 10}
EMSG_WORDS = 12
MAX_BOX_ROWS = 256
DEFAULT_MAX_MOOF = 64
DEFAULT_MAX_RUN = 128
DEFAULT_MAX_EMSG = 16
VIDEO_TYPES = (0, 0x1B, 0x24)
AUDIO_TYPES = (0, 0x0F)


@dataclass(frozen=True)
class Mp4Track:
    """What the init segment says about one track: ``kind`` is ``"video"`` or ``"audio"``;
    ``codec_type`` is ``0x1B`` / ``0x24`` / 0 (no NAL index) for video and ``0x0F`` (``mp4a``) / 0
    for audio; the three defaults are the track's ``trex``; ``protection`` is the
    :class:`~.cbcs.Mp4Protection` of a protected sample entry (``encv`` / ``enca``), which the demux
    itself does not read."""
    track_id: int
    kind: str
    codec_type: int = 0
    nal_length_size: int = 4
    default_duration: int = 0
    default_size: int = 0
    default_flags: int = 0
    protection: Any = None


def _track_rows(op: str, tracks) -> np.ndarray:
    """One segment's ``int64[TRACKS, TRACK_WORDS]``: slot 0 the video track, slot 1 the audio track."""
    tracks = getattr(tracks, "tracks", tracks)  # an Mp4Init
    rows = np.zeros((TRACKS, TRACK_WORDS), dtype=np.int64)
    for t in tracks:
        if t.kind not in ("video", "audio"):
            raise ValueError(f"{op}: a track is video or audio")
        slot = 0 if t.kind == "video" else 1
        if rows[slot, TRACK["id"]]:
            raise ValueError(f"{op}: at most one video and one audio track")
        if not 0 < int(t.track_id) < 2 ** 32:
            raise ValueError(f"{op}: track_id must be 1 to 2^32 - 1")
        if int(t.codec_type) not in (VIDEO_TYPES if slot == 0 else AUDIO_TYPES):
            raise ValueError(f"{op}: codec_type of a {t.kind} track must be one of "
                             f"{VIDEO_TYPES if slot == 0 else AUDIO_TYPES}")
        if slot == 0 and t.codec_type and t.nal_length_size not in (1, 2, 4):
            raise ValueError(f"{op}: nal_length_size must be 1, 2 or 4")
        for v in (t.default_duration, t.default_size, t.default_flags):
            if not 0 <= int(v) < 2 ** 32:
                raise ValueError(f"{op}: a trex default must fit 32 bits")
        rows[slot] = (t.track_id, KIND[t.kind], t.codec_type, t.nal_length_size if slot == 0 else 0, t.default_duration,
                      t.default_size, t.default_flags, 0)
    if rows[0, 0] and rows[0, 0] == rows[1, 0]:
        raise ValueError(f"{op}: the two tracks share a track_id")
    return rows


def pack_tracks(tracks, B: int, op: str = "mp4_demux_batch") -> np.ndarray:
    """``int64[B, TRACKS, TRACK_WORDS]`` from one track set for all segments (an ``Mp4Init`` or a
    sequence of :class:`Mp4Track`) or from ``B`` of them."""
    one = hasattr(tracks, "tracks") or all(isinstance(t, Mp4Track) for t in tracks)
    if one:
        return np.broadcast_to(_track_rows(op, tracks), (B, TRACKS, TRACK_WORDS)).copy()
    if len(tracks) != B:
        raise ValueError(f"{op}: one track set per segment, or one for all")
    return np.stack([_track_rows(op, t) for t in tracks]).reshape(B, TRACKS, TRACK_WORDS)


@dataclass
class Mp4Demux:
    minfo: torch.Tensor     # int64[B, MINFO_WORDS]
    msamples: torch.Tensor  # int32[B, TRACKS, max_pes, MSAMPLE_WORDS]
    runs: torch.Tensor      # int64[B, max_run, RUN_WORDS]
    emsg: torch.Tensor      # int64[B, max_emsg, EMSG_WORDS]
    info: torch.Tensor      # int64[B, tsdemux.INFO_WORDS]
    pes: torch.Tensor       # int64[B, 3, max_pes, 3]
    nal: torch.Tensor       # int32[B, max_nal, 4]
    au: torch.Tensor        # int32[B, max_pes, 4]
    aframes: torch.Tensor   # int32[B, max_pes, 2]
    sinfo: torch.Tensor     # int64[B, esindex.SINFO_WORDS]
    buf: torch.Tensor       # the segments, where they were
    offs: np.ndarray        # host int64[B]
    caps: np.ndarray        # host int64[B]: what caption_batch takes as caps

    def as_demux(self) -> DemuxResult:
        """The batch as the ops behind the TS demux take it, without a copy: the whole segment is
        the video ES."""
        return DemuxResult(self.info, self.pes, self.buf, self.offs)

    def as_index(self) -> EsIndex:
        """The NAL index of the video samples in ``index_batch``'s layout, without a copy."""
        return EsIndex(self.nal, self.au, self.aframes, self.sinfo)

    def segment(self, i: int) -> dict:
        """Host view of segment ``i`` (syncs): the ``minfo`` fields by name, ``video`` / ``audio``
        (the track's totals by name, ``samples`` = the recorded ``msamples`` rows, ``pes`` = their
        ``(offset, pts, dts)`` rows), the recorded ``runs`` and the ``emsg`` rows that were kept."""
        minfo = self.minfo[i].cpu().numpy()
        out = {k: int(minfo[v]) for k, v in MINFO.items()}
        ms, pes = self.msamples[i].cpu().numpy(), self.pes[i].cpu().numpy()
        for t, name in enumerate(("video", "audio")):
            tr = {k: int(minfo[MINFO_TRACK0 + MINFO_TRACK_WORDS * t + v]) for k, v in MINFO_TRACK.items()}
            rec = min(tr["n_samples"], ms.shape[1])
            tr["samples"], tr["pes"] = ms[t, :rec], pes[t, :rec]
            out[name] = tr
        runs = self.runs[i].cpu().numpy()
        out["runs"] = runs[:min(out["n_run"], runs.shape[0])]
        emsg = self.emsg[i].cpu().numpy()
        out["emsg"] = [{k: int(row[v]) for k, v in EMSG.items()} for row in emsg if row[EMSG["offset"]] >= 0]
        return out


def mp4_demux_batch(buf: torch.Tensor, offs: Sequence[int], lens: Union[Sequence[int], torch.Tensor], tracks,
                    caps: Optional[Sequence[int]] = None, max_pes: int = DEFAULT_MAX_PES,
                    max_nal: int = DEFAULT_MAX_NAL, max_moof: int = DEFAULT_MAX_MOOF, max_run: int = DEFAULT_MAX_RUN,
                    max_emsg: int = DEFAULT_MAX_EMSG) -> Mp4Demux:
    """Demux every fragmented-MP4 segment ``buf[offs[i] : offs[i] + lens[i]]`` on the device ``buf``
    lives on and on the caller's stream.  ``lens`` may be a device tensor (the decrypt's
    ``out_len``) with host ``caps``; ``tracks`` is one track set for all segments (an ``Mp4Init``
    or a sequence of :class:`Mp4Track`) or one per segment.  ``buf`` is only read."""
    op = "mp4_demux_batch"
    max_pes, max_nal, max_moof, max_run, max_emsg = (int(v) for v in (max_pes, max_nal, max_moof, max_run, max_emsg))
    if max_pes <= 0 or max_nal <= 0:
        raise ValueError(f"{op}: max_pes and max_nal must be positive")
    if not all(1 <= v <= MAX_BOX_ROWS for v in (max_moof, max_run, max_emsg)):
        raise ValueError(f"{op}: max_moof, max_run and max_emsg must be 1 to {MAX_BOX_ROWS}")
    if buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous():
        raise ValueError(f"{op}: buf must be a contiguous one-dimensional uint8 tensor")
    B = len(offs)
    o = np.asarray(offs, dtype=np.int64).reshape(B)
    if isinstance(lens, torch.Tensor):
        if caps is None:
            raise ValueError(f"{op}: caps (host upper bounds) are required when lens is a tensor")
        cap = np.asarray(caps, dtype=np.int64).reshape(-1)
    else:
        cap = np.asarray(lens, dtype=np.int64).reshape(-1)
    check_ranges(op, "source", o, cap, buf.numel())
    if np.any(cap >= 2 ** 31 - 64):
        raise ValueError(f"{op}: a segment must be below 2 GiB")
    tk = pack_tracks(tracks, B, op)
    dev = buf.device

    def table(shape, dtype):
        return torch.empty((B, *shape), dtype=dtype, device=dev)

    r = Mp4Demux(table((MINFO_WORDS,), torch.int64), table((TRACKS, max_pes, MSAMPLE_WORDS), torch.int32),
                 table((max_run, RUN_WORDS), torch.int64), table((max_emsg, EMSG_WORDS), torch.int64),
                 table((24,), torch.int64), table((3, max_pes, 3), torch.int64), table((max_nal, 4), torch.int32),
                 table((max_pes, 4), torch.int32), table((max_pes, 2), torch.int32), table((8,), torch.int64),
                 buf, o, cap)
    limits = (max_pes, max_nal, max_moof, max_run, max_emsg)
    if dev.type == "cpu":
        n = lens.numpy().astype(np.int64) if isinstance(lens, torch.Tensor) else cap
        n = np.minimum(np.maximum(n, 0), cap)
        _rt().mp4_demux_batch(buf.numpy(), o, n, tk, *limits, r.minfo.numpy(), r.msamples.numpy(), r.runs.numpy(),
                              r.emsg.numpy(), r.info.numpy(), r.pes.numpy(), r.nal.numpy(), r.au.numpy(),
                              r.aframes.numpy(), r.sinfo.numpy())
        return r
    if np.any(o % 16):
        raise ValueError(f"{op}: offsets must be 16-byte aligned on device")
    # a segment is read in dwords: it may not reach into a trailing partial dword of the buffer
    if np.any(o + cap > buf.numel() - buf.numel() % 4):
        raise ValueError(f"{op}: a segment reaches the buffer's last partial dword on device")
    if isinstance(lens, torch.Tensor) and (lens.device != dev or lens.dtype != torch.int64 or lens.numel() < B):
        raise ValueError(f"{op}: lens must be an int64 tensor of B elements on buf's device")
    arrays = {"o": o, "cap": cap, "tk": tk.reshape(-1)}  # one packed copy with the descriptors
    d = pack_to_device(arrays, dev)
    if B:
        _dev().mp4_demux(buf, d["o"], lens if isinstance(lens, torch.Tensor) else d["cap"], d["cap"], d["tk"], *limits,
                         r.minfo, r.msamples, r.runs, r.emsg, r.info, r.pes, r.nal, r.au, r.aframes, r.sinfo)
    return r
