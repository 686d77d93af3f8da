"""``cenc`` decryption (ISO/IEC 23001-7 AES-128-CTR; HLS ``METHOD=SAMPLE-AES-CTR`` on fragmented
MP4) of a demuxed batch, out of place (``docs/CENC.md`` holds the rules).

:func:`cenc_decrypt_batch` takes the :class:`~.mp4demux.Mp4Demux` of the protected segments and
returns, per enabled segment (identical for the gfx950 kernels and the host implementation):

* ``buf[offs[i] : offs[i] + n]``: a copy of the segment with every byte of every recorded range
  XORed with the sample's keystream, which runs on across the sample's clear bytes;
* ``ranges[i, r] = (offset in the segment, length, track << 30 | sample, first unit rank, stream
  position, offset of the sample's senc IV or -1, 0, 0)``, video track first, ``-1`` rows behind the
  recorded ones (slot names in :data:`RANGE`);
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
from .cbcs import (ALIGN, AUX_WORDS, CSTATUS, DEFAULT_MAX_RANGE, MAX_RANGE_LIMIT, PROT, PROT_WORDS, TRACK_SHIFT,
                   Mp4Protection, _setup, pack_protection)
from .mp4demux import Mp4Demux

CINFO = {"status": 0, "n_ranges": 1, "video_samples": 2, "audio_samples": 3, "video_bytes": 4, "audio_bytes": 5,
         "n_senc": 6, "n_units": 7}
CINFO_WORDS = 8
RANGE = {"offset": 0, "length": 1, "sample": 2, "rank": 3, "stream_pos": 4, "iv_offset": 5}
RANGE_WORDS = 8
TILE_UNITS = 4096  # keystream units per tile of the units kernel

__all__ = ["ALIGN", "AUX_WORDS", "CINFO", "CINFO_WORDS", "CSTATUS", "DEFAULT_MAX_RANGE", "MAX_RANGE_LIMIT", "PROT",
           "PROT_WORDS", "RANGE", "RANGE_WORDS", "TILE_UNITS", "TRACK_SHIFT", "Cenc", "Mp4Protection",
           "cenc_decrypt_batch", "pack_protection", "segment_view"]


def segment_view(cinfo_row) -> dict:
    """One segment's host ``cinfo`` row by name."""
    return {k: int(cinfo_row[v]) for k, v in CINFO.items()}


@dataclass
class Cenc:
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


def cenc_decrypt_batch(md: Mp4Demux, protection, keys: Sequence[Optional[bytes]],
                       ivs: Optional[Sequence[Optional[bytes]]] = None, enable: Optional[Sequence[bool]] = None,
                       max_range: int = DEFAULT_MAX_RANGE) -> Cenc:
    """Decrypt every enabled segment of a demuxed fragmented-MP4 batch into a copy, on the device
    its tensors live on and on the caller's stream.  The arguments are those of
    :func:`~.cbcs.cbcs_decrypt_batch`; the tracks' scheme must be ``cenc`` and their ``tenc``
    pattern 0:0 (anything else is ``cens``).  ``md.buf`` is only read."""
    on_gpu = md.buf.device.type != "cpu"
    s = _setup("cenc_decrypt_batch", "cenc", md, protection, keys, ivs, enable, max_range, RANGE_WORDS, CINFO_WORDS,
               aes.enc_round_keys_le if on_gpu else lambda key: _rt().expand_key_enc(key))
    r = Cenc(s.buf, s.offs, s.cinfo, s.ranges, s.md)
    if not s.on_gpu:
        _rt().cenc_decrypt_batch(md.buf.numpy(), s.src_off, s.n, s.buf.numpy(), s.offs, md.minfo.numpy(),
                                 md.msamples.numpy(), md.runs.numpy(), md.info.numpy(), md.pes.numpy(), s.max_pes,
                                 s.max_run, s.prot, s.civ, s.iv, s.rk, s.en, s.max_range, s.ranges.numpy(),
                                 s.cinfo.numpy())
        return r
    if not s.B:
        return r
    d = s.pack()
    tel, sbox = aes.device_enc_tables(s.dev)
    max_cap = int(s.cap[s.on].max()) if len(s.on) else 0
    _dev().cenc_decrypt(md.buf, d["so"], d["cap"], s.buf, d["do"], md.info, md.pes, md.minfo, md.msamples, md.runs,
                        s.max_pes, s.max_run, d["prot"], d["civ"], d["iv"], d["drk"], d["en"], tel, sbox, s.max_range,
                        max_cap, s.scratch(), s.ranges, s.cinfo)
    return r
