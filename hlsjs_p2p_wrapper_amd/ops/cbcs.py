"""``cbcs`` decryption (ISO/IEC 23001-7; HLS ``METHOD=SAMPLE-AES`` on fragmented MP4) of a demuxed
batch, out of place (``docs/CBCS.md`` holds the rules).

:func:`cbcs_decrypt_batch` takes the :class:`~.mp4demux.Mp4Demux` of the protected segments (their
``moof`` boxes, NAL lengths and headers are clear, so it already is the demux of the clear ones)
and returns, per enabled segment (identical for the gfx950 kernels and the host implementation):

* ``buf[offs[i] : offs[i] + n]``: a copy of the segment with every cipher block of every recorded
  range decrypted: AES-128-CBC over the ``crypt`` blocks of each ``crypt + skip`` group, a chain
  per subsample range;
* ``ranges[i, r] = (offset in the segment, length, track << 30 | sample, first cipher-block rank)``,
  video track first, ``-1`` rows behind the recorded ones (slot names in :data:`RANGE`);
* ``cinfo[i]`` = status bits and totals (slot names in :data:`CINFO`).

The source is only read: it may be the HBM arena that peers are served from.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import aes
from ._native import device as _dev
from ._native import runtime as _rt
from .desc import pack_to_device
from .mp4demux import MINFO_WORDS, MSAMPLE_WORDS, RUN_WORDS, TRACKS, Mp4Demux, Mp4Track
from .segment import copy_segments
from .tsdemux import INFO, INFO_WORDS

PROT = {"protected": 0, "crypt": 1, "skip": 2, "per_sample_iv_size": 3, "constant_iv_size": 4}
PROT_WORDS = 8
CINFO = {"status": 0, "n_ranges": 1, "video_samples": 2, "audio_samples": 3, "video_blocks": 4, "audio_blocks": 5,
         "n_senc": 6}
CINFO_WORDS = 8
CSTATUS = {"range_overflow": 1, "no_senc": 2, "bad_senc": 4, "demux_damaged": 8, "overlap": 16}
RANGE = {"offset": 0, "length": 1, "sample": 2, "rank": 3}
RANGE_WORDS = 4
TRACK_SHIFT = 30
AUX_WORDS = 4
DEFAULT_MAX_RANGE = 4096
MAX_RANGE_LIMIT = 65536
ALIGN = 256  # of a segment's copy, as the transmux pipeline lays its buffers out


@dataclass(frozen=True)
class Mp4Protection:
    """A track's ``sinf``: ``scheme`` is the ``schm`` scheme_type (``"cbcs"``), the two pattern
    counts and the IV sizes are the ``tenc`` box's, ``constant_iv`` its IV bytes (``b""`` when the
    samples carry their own) and ``kid`` its 16-byte default key id."""
    scheme: str
    crypt_byte_block: int
    skip_byte_block: int
    per_sample_iv_size: int
    constant_iv: bytes
    kid: bytes


def _prot_rows(op: str, tracks, scheme: str = "cbcs"):
    """One segment's ``int64[TRACKS, PROT_WORDS]`` and ``uint8[TRACKS, 16]`` constant IVs."""
    tracks = getattr(tracks, "tracks", tracks)  # an Mp4Init
    rows = np.zeros((TRACKS, PROT_WORDS), dtype=np.int64)
    civ = np.zeros((TRACKS, 16), dtype=np.uint8)
    for t in tracks:
        p = getattr(t, "protection", None)
        if p is None:
            continue
        if t.kind not in ("video", "audio"):
            raise ValueError(f"{op}: a track is video or audio")
        slot = 0 if t.kind == "video" else 1
        if p.scheme != scheme:
            raise ValueError(f"{op}: scheme {p.scheme!r} is not supported, only {scheme}")
        c, s = int(p.crypt_byte_block), int(p.skip_byte_block)
        size, const = int(p.per_sample_iv_size), bytes(p.constant_iv)
        if size not in (0, 8, 16) or len(const) not in (0, 8, 16):
            raise ValueError(f"{op}: an IV is 8 or 16 bytes")
        if not (0 <= c <= 255 and 0 <= s <= 255):
            raise ValueError(f"{op}: crypt_byte_block and skip_byte_block are 0 to 255")
        if s > 0 and c == 0:
            raise ValueError(f"{op}: a pattern that skips blocks must encrypt some (crypt_byte_block 0)")
        if scheme == "cenc" and (c or s):
            raise ValueError(f"{op}: a pattern ({c}:{s}) under AES-CTR is the cens scheme, which is not supported")
        rows[slot, :5] = (1, c, s, size, len(const) if size == 0 else 0)
        if size == 0 and const:
            civ[slot, :len(const)] = np.frombuffer(const, dtype=np.uint8)  # an 8-byte IV: zeros on the right
    return rows, civ


def pack_protection(protection, B: int, op: str = "cbcs_decrypt_batch", scheme: str = "cbcs"):
    """``int64[B, TRACKS, PROT_WORDS]`` and ``uint8[B, TRACKS, 16]`` from one track set for all
    segments (an ``Mp4Init`` or a sequence of :class:`~.mp4demux.Mp4Track`) or from ``B`` of them.
    ``scheme`` is the one scheme_type that is accepted."""
    one = hasattr(protection, "tracks") or all(isinstance(t, Mp4Track) for t in protection)
    if one:
        rows, civ = _prot_rows(op, protection, scheme)
        return (np.broadcast_to(rows, (B, TRACKS, PROT_WORDS)).copy(), np.broadcast_to(civ, (B, TRACKS, 16)).copy())
    if len(protection) != B:
        raise ValueError(f"{op}: one track set per segment, or one for all")
    both = [_prot_rows(op, p, scheme) for p in protection]
    return (np.stack([r for r, _ in both]).reshape(B, TRACKS, PROT_WORDS),
            np.stack([c for _, c in both]).reshape(B, TRACKS, 16))


def segment_view(cinfo_row) -> dict:
    """One segment's host ``cinfo`` row by name."""
    return {k: int(cinfo_row[v]) for k, v in CINFO.items()}


@dataclass
class Cbcs:
    buf: torch.Tensor     # the decrypted copies
    offs: np.ndarray      # host int64[B]: where segment i's copy starts, -1 for a segment that did not ask
    cinfo: torch.Tensor   # int64[B, CINFO_WORDS]
    ranges: torch.Tensor  # int32[B, max_range, RANGE_WORDS]
    md: Mp4Demux          # the demux over buf / offs: the ten tables are the source demux's own

    def segment(self, i: int) -> dict:
        """Host view of segment ``i`` (syncs): the ``cinfo`` fields by name and ``ranges``, the
        recorded rows."""
        out = segment_view(self.cinfo[i].cpu().numpy())
        rows = self.ranges[i].cpu().numpy()
        out["ranges"] = rows[:min(out["n_ranges"], rows.shape[0])]
        return out


def _check_md(op: str, md: Mp4Demux) -> int:
    B = len(md.offs)
    if md.pes.dim() != 4 or md.runs.dim() != 3:
        raise ValueError(f"{op}: md is not the result of mp4_demux_batch")
    max_pes, max_run = int(md.pes.shape[2]), int(md.runs.shape[1])
    want = {"minfo": (B, MINFO_WORDS), "msamples": (B, TRACKS, max_pes, MSAMPLE_WORDS), "runs": (B, max_run, RUN_WORDS),
            "info": (B, INFO_WORDS), "pes": (B, 3, max_pes, 3)}
    dev = md.buf.device
    for name, shape in want.items():
        t = getattr(md, name)
        if tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{op}: md.{name} does not belong to a batch of {B} segments on {dev}")
    if len(md.caps) != B or md.buf.dtype != torch.uint8 or md.buf.dim() != 1:
        raise ValueError(f"{op}: md does not belong to a batch of {B} segments")
    return B


class _Setup:
    """What ``cbcs_decrypt_batch`` and ``cenc_decrypt_batch`` share: the checks, the per-segment
    arrays, the output tensors and the copy of every enabled segment (made here)."""

    def pack(self):
        return pack_to_device({"so": self.src_off, "cap": self.cap, "do": self.offs, "prot": self.prot.reshape(-1),
                               "civ": self.civ.reshape(-1), "iv": self.iv.reshape(-1), "drk": self.rk.reshape(-1),
                               "en": self.en}, self.dev)

    def scratch(self):
        return torch.empty(self.B * TRACKS * self.max_pes * AUX_WORDS, dtype=torch.int32, device=self.dev)


def _setup(op: str, scheme: str, md: Mp4Demux, protection, keys, ivs, enable, max_range, range_words: int,
           cinfo_words: int, expand) -> _Setup:
    """``expand(key)`` gives the 44 round-key words of one key in the form the implementation that
    will run takes."""
    s = _Setup()
    B = s.B = _check_md(op, md)
    max_range = s.max_range = int(max_range)
    if not 1 <= max_range <= MAX_RANGE_LIMIT:
        raise ValueError(f"{op}: max_range must be 1 to {MAX_RANGE_LIMIT}")
    if len(keys) != B or (ivs is not None and len(ivs) != B) or (enable is not None and len(enable) != B):
        raise ValueError(f"{op}: one key, one IV and one enable flag per segment")
    s.prot, s.civ = pack_protection(protection, B, op, scheme)
    en = s.en = np.ones(B, dtype=np.uint8) if enable is None else np.asarray([bool(e) for e in enable], dtype=np.uint8)
    dev = s.dev = md.buf.device
    s.on_gpu = dev.type != "cpu"
    rk = s.rk = np.zeros((B, 44), dtype=np.uint32)
    iv = s.iv = np.zeros((B, 16), dtype=np.uint8)
    expanded = {}
    for i in range(B):
        if not en[i]:
            continue
        if keys[i] is None or len(keys[i]) != 16:
            raise ValueError(f"{op}: a key must be 16 bytes")
        # the kernel takes little-endian column words, the host big-endian ones; one key per rendition
        # is the usual case: it is expanded once
        key = bytes(keys[i])
        if key not in expanded:
            expanded[key] = expand(key)
        rk[i] = expanded[key]
        if ivs is not None and ivs[i] is not None:
            if len(ivs[i]) != 16:
                raise ValueError(f"{op}: an IV must be 16 bytes")
            iv[i] = np.frombuffer(bytes(ivs[i]), dtype=np.uint8)
    src_off = s.src_off = np.asarray(md.offs, dtype=np.int64).reshape(B)
    cap = s.cap = np.asarray(md.caps, dtype=np.int64).reshape(B)
    if np.any(cap < 0) or np.any(cap >= 2 ** 31 - 64) or np.any(src_off < 0) or np.any(src_off + cap > md.buf.numel()):
        raise ValueError(f"{op}: md's segments do not lie inside md.buf")
    on = s.on = np.flatnonzero(en)
    sizes = (cap[on] + (ALIGN - 1)) // ALIGN * ALIGN
    ends = np.cumsum(sizes)
    offs = s.offs = np.full(B, -1, dtype=np.int64)
    offs[on] = ends - sizes
    s.buf = torch.empty((int(ends[-1]) if len(on) else 0) + ALIGN, dtype=torch.uint8, device=dev)
    s.max_pes, s.max_run = int(md.pes.shape[2]), int(md.runs.shape[1])
    s.cinfo = torch.empty((B, cinfo_words), dtype=torch.int64, device=dev)
    s.ranges = torch.empty((B, max_range, range_words), dtype=torch.int32, device=dev)
    s.md = Mp4Demux(md.minfo, md.msamples, md.runs, md.emsg, md.info, md.pes, md.nal, md.au, md.aframes, md.sinfo,
                    s.buf, offs, cap)
    if not s.on_gpu:
        s.n = np.minimum(np.maximum(md.info[:, INFO["video_bytes"]].numpy().astype(np.int64), 0), cap) if B else cap
        copy_segments(md.buf, s.buf, src_off[on], offs[on], s.n[on])
        return s
    if np.any(src_off % 16):
        raise ValueError(f"{op}: offsets must be 16-byte aligned on device")
    if np.any(src_off + cap > md.buf.numel() - md.buf.numel() % 4):
        raise ValueError(f"{op}: a segment reaches the buffer's last partial dword on device")
    if B:
        copy_segments(md.buf, s.buf, src_off[on], offs[on], cap[on])  # whole caps: the true lengths live on the device
    return s


def cbcs_decrypt_batch(md: Mp4Demux, protection, keys: Sequence[Optional[bytes]],
                       ivs: Optional[Sequence[Optional[bytes]]] = None, enable: Optional[Sequence[bool]] = None,
                       max_range: int = DEFAULT_MAX_RANGE) -> Cbcs:
    """Decrypt every enabled segment of a demuxed fragmented-MP4 batch into a copy, on the device
    its tensors live on and on the caller's stream.  ``protection`` is an ``Mp4Init`` or a sequence
    of :class:`~.mp4demux.Mp4Track` (their ``protection`` fields count) for all segments, or one per
    segment; ``keys[i]`` is 16 bytes; ``ivs[i]`` (16 bytes) serves a track whose ``tenc`` has neither
    a per-sample nor a constant IV; ``enable[i]`` false leaves segment i alone with an all-zero
    ``cinfo`` row and ``offs[i] = -1`` (its key may be ``None``).  ``md.buf`` is only read."""
    s = _setup("cbcs_decrypt_batch", "cbcs", md, protection, keys, ivs, enable, max_range, RANGE_WORDS, CINFO_WORDS,
               aes.round_keys_le if md.buf.device.type != "cpu" else aes.round_keys)
    r = Cbcs(s.buf, s.offs, s.cinfo, s.ranges, s.md)
    if not s.on_gpu:
        _rt().cbcs_decrypt_batch(md.buf.numpy(), s.src_off, s.n, s.buf.numpy(), s.offs, md.minfo.numpy(),
                                 md.msamples.numpy(), md.runs.numpy(), md.info.numpy(), md.pes.numpy(), s.max_pes,
                                 s.max_run, s.prot, s.civ, s.iv, s.rk, s.en, s.max_range, s.ranges.numpy(),
                                 s.cinfo.numpy())
        return r
    if not s.B:
        return r
    d = s.pack()
    tdl, isb = aes.device_tables(s.dev)
    max_blocks = int(s.cap[s.on].max()) // 16 if len(s.on) else 0
    _dev().cbcs_decrypt(md.buf, d["so"], d["cap"], s.buf, d["do"], md.info, md.pes, md.minfo, md.msamples, md.runs,
                        s.max_pes, s.max_run, d["prot"], d["civ"], d["iv"], d["drk"], d["en"], tdl, isb, s.max_range,
                        max_blocks, s.scratch(), s.ranges, s.cinfo)
    return r
