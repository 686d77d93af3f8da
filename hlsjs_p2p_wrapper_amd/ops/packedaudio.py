"""Demux of packed-audio segments: one or more ID3v2 tags in front of raw ADTS AAC frames, what
hls.js's ``aacdemuxer`` and ``id3`` read from an ``.aac`` fragment (``docs/PACKEDAUDIO.md`` holds
the rules).

:func:`packed_audio_batch` moves no payload.  Per segment (identical for the gfx950 kernel and the
host implementation) it returns ``info`` / ``pes`` in the layout of :class:`~.tsdemux.DemuxResult`
(the audio ES starts behind the tags, four ADTS frames make one audio PES row stamped from the
tags' transport stream timestamp, the tags are the id3 ES) and ``nal`` / ``au`` / ``aframes`` /
``sinfo`` in that of :class:`~.esindex.EsIndex`, so ``remux_batch``, ``fragment_batch`` and
``config_batch`` run on :meth:`PackedAudio.as_demux` / :meth:`PackedAudio.as_index` unchanged;
``painfo[i]`` = status bits and totals (slot names in :data:`PAINFO`).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Union

import numpy as np
import torch

from ._native import device as _dev
from ._native import runtime as _rt
from .desc import check_ranges, pack_to_device
from .esindex import SINFO_WORDS, EsIndex
from .tsdemux import DEFAULT_MAX_PES, INFO_WORDS, DemuxResult

PAINFO = {"status": 0, "id3_bytes": 1, "n_tags": 2, "timestamp": 3, "n_frames": 4, "stop_offset": 5, "sample_rate": 6,
          "channels": 7}
PAINFO_WORDS = 8
PASTATUS = {"no_timestamp": 1, "bad_id3": 2, "no_frame": 4, "trailing_bytes": 8, "pes_overflow": 16, "bad_rate": 32}
FATAL = PASTATUS["no_timestamp"] | PASTATUS["bad_id3"] | PASTATUS["no_frame"] | PASTATUS["bad_rate"]
FRAMES_PER_PES = 4
NAL_ROWS = 1
MAX_PES_LIMIT = 4096
AUDIO_TYPE = 0x0F


def tile_bytes() -> int:
    """Bytes of a segment the kernel stages in LDS per round of its frame walk."""
    return int(_rt().ES_PACKED_TILE)


@dataclass
class PackedAudio:
    info: torch.Tensor     # int64[B, tsdemux.INFO_WORDS]
    pes: torch.Tensor      # int64[B, 3, max_pes, 3]
    nal: torch.Tensor      # int32[B, 1, 4]
    au: torch.Tensor       # int32[B, max_pes, 4]
    aframes: torch.Tensor  # int32[B, max_pes, 2]
    sinfo: torch.Tensor    # int64[B, esindex.SINFO_WORDS]
    painfo: torch.Tensor   # int64[B, PAINFO_WORDS]
    buf: torch.Tensor      # the segments, where they were
    offs: np.ndarray       # host int64[B]
    caps: np.ndarray       # host int64[B]: what the ops behind take as caps

    def as_demux(self) -> DemuxResult:
        """The batch as the ops behind the TS demux take it, without a copy: the segment is
        ``[id3 ES | audio ES]``."""
        return DemuxResult(self.info, self.pes, self.buf, self.offs)

    def as_index(self) -> EsIndex:
        """The ADTS frames in ``index_batch``'s layout, without a copy."""
        return EsIndex(self.nal, self.au, self.aframes, self.sinfo)

    def segment(self, i: int) -> dict:
        """Host view of segment ``i`` (syncs): the ``painfo`` fields by name, ``status_names`` and
        the recorded audio ``pes`` and ``aframes`` rows."""
        pa = self.painfo[i].cpu().numpy()
        out = {k: int(pa[v]) for k, v in PAINFO.items()}
        out["status_names"] = [k for k, v in PASTATUS.items() if out["status"] & v]
        groups = (out["n_frames"] + FRAMES_PER_PES - 1) // FRAMES_PER_PES
        rec = min(groups, self.pes.shape[2])
        out["pes"] = self.pes[i, 1, :rec].cpu().numpy()
        out["aframes"] = self.aframes[i, :rec].cpu().numpy()
        return out


def packed_audio_batch(buf: torch.Tensor, offs: Sequence[int], lens: Union[Sequence[int], torch.Tensor],
                       caps: Optional[Sequence[int]] = None, max_pes: int = DEFAULT_MAX_PES) -> PackedAudio:
    """Demux every packed-audio segment ``buf[offs[i] : offs[i] + lens[i]]`` on the device ``buf``
    lives on and on the caller's stream.  ``lens`` may be a device tensor (the decrypt's
    ``out_len``) with host ``caps``.  ``buf`` is only read."""
    op = "packed_audio_batch"
    max_pes = int(max_pes)
    if not 1 <= max_pes <= MAX_PES_LIMIT:
        raise ValueError(f"{op}: max_pes must be 1 to {MAX_PES_LIMIT}")
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
    dev = buf.device

    def table(shape, dtype):
        return torch.empty((B, *shape), dtype=dtype, device=dev)

    r = PackedAudio(table((INFO_WORDS,), torch.int64), table((3, max_pes, 3), torch.int64),
                    table((NAL_ROWS, 4), torch.int32), table((max_pes, 4), torch.int32),
                    table((max_pes, 2), torch.int32), table((SINFO_WORDS,), torch.int64),
                    table((PAINFO_WORDS,), torch.int64), buf, o, cap)
    if dev.type == "cpu":
        if isinstance(lens, torch.Tensor) and (lens.dtype != torch.int64 or lens.numel() < B):
            raise ValueError(f"{op}: lens must be an int64 tensor of B elements")
        n = lens.numpy().astype(np.int64).reshape(-1)[:B] if isinstance(lens, torch.Tensor) else cap
        n = np.minimum(np.maximum(n, 0), cap)
        _rt().packed_audio_batch(buf.numpy(), o, n, max_pes, r.info.numpy(), r.pes.numpy(), r.nal.numpy(),
                                 r.au.numpy(), r.aframes.numpy(), r.sinfo.numpy(), r.painfo.numpy())
        return r
    if np.any(o % 16):
        raise ValueError(f"{op}: offsets must be 16-byte aligned on device")
    # a segment is read in dwords: it may not reach into a trailing partial dword of the buffer
    if np.any(o + cap > buf.numel() - buf.numel() % 4):
        raise ValueError(f"{op}: a segment reaches the buffer's last partial dword on device")
    if isinstance(lens, torch.Tensor) and (lens.device != dev or lens.dtype != torch.int64 or lens.numel() < B):
        raise ValueError(f"{op}: lens must be an int64 tensor of B elements on buf's device")
    d = pack_to_device({"o": o, "cap": cap}, dev)  # one packed copy with the descriptors
    if B:
        _dev().packed_audio(buf, d["o"], lens if isinstance(lens, torch.Tensor) else d["cap"], d["cap"], max_pes,
                            r.info, r.pes, r.nal, r.au, r.aframes, r.sinfo, r.painfo)
    return r
