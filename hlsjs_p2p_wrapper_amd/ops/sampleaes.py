"""HLS ``METHOD=SAMPLE-AES`` decryption of demuxed and indexed segments, in place
(``docs/SAMPLEAES.md`` holds the rules).

:func:`sample_decrypt_batch` takes the :class:`~.tsdemux.DemuxResult` of a batch and its
:class:`~.esindex.EsIndex` and rewrites, per enabled segment (identical for the gfx950 kernel and
the host implementation, bytes and rows):

* every protected H.264 slice NAL (type 1 or 5, inside an access unit, more than 48 bytes without
  its emulation prevention): the NAL is unescaped where it lies, one 16-byte block in ten of it is
  decrypted as a CBC chain that restarts with the NAL, the freed tail becomes zeros and
  ``nal[i, k, length]`` the unescaped length;
* every counted ADTS frame: the whole 16-byte blocks of its payload behind a 16-byte leader, a CBC
  chain per frame;
* ``sainfo[i]`` = status bits and totals (slot names in :data:`SAINFO`).

Nothing else changes: not the ``au`` table, not ``sinfo``, no byte outside protected NALs and
frames.  ``remux_batch`` and the two configuration calls then read the decrypted ES.
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
from .esindex import EsIndex, IndexedBatch
from .tsdemux import DemuxResult

SAINFO = {"status": 0, "protected_nals": 1, "removed_bytes": 2, "video_blocks": 3, "audio_frames": 4,
          "audio_blocks": 5}
SAINFO_WORDS = 6
SASTATUS = {"truncated": 1, "unsupported_video": 2, "unsupported_audio": 4, "partial_audio": 8}


def sample_aes_round_bytes() -> int:
    """Raw NAL bytes the kernel unescapes per round (the host implementation has no rounds)."""
    return _rt().ES_SA_ROUND


@dataclass
class SampleAes:
    sainfo: torch.Tensor  # int64[B, SAINFO_WORDS]

    def segment(self, i: int) -> dict:
        """Host view of segment ``i`` (syncs): the ``sainfo`` fields by name."""
        return segment_view(self.sainfo[i].cpu().numpy())


def segment_view(sainfo_row) -> dict:
    """One segment's host row by name."""
    return {k: int(sainfo_row[v]) for k, v in SAINFO.items()}


def sample_decrypt_batch(res: DemuxResult, ix: EsIndex, caps: Sequence[int], keys: Sequence[Optional[bytes]],
                         ivs: Sequence[Optional[bytes]], enable: Optional[Sequence[bool]] = None) -> SampleAes:
    """Decrypt every enabled segment of a demuxed and indexed batch in place, on the device its
    tensors live on and on the caller's stream.  ``caps`` are what ``index_batch`` took;
    ``keys[i]`` / ``ivs[i]`` are 16 bytes each; ``enable[i]`` false leaves segment i alone with an
    all-zero ``sainfo`` row (its key and IV may be ``None``).  Writes ``res.es`` and the length
    column of ``ix.nal``."""
    B = len(res.es_offs)
    if len(keys) != B or len(ivs) != B or (enable is not None and len(enable) != B):
        raise ValueError("sample_decrypt_batch: one key, one IV and one enable flag per segment")
    batch = IndexedBatch("sample_decrypt_batch", res, ix, caps)
    if np.any(batch.cap >= 2 ** 31):  # NAL rows hold int32 offsets on either device
        raise ValueError("sample_decrypt_batch: a segment's ES must be below 2 GiB")
    en = np.ones(B, dtype=np.uint8) if enable is None else np.asarray([bool(e) for e in enable], dtype=np.uint8)
    drk = np.zeros((B, 44), dtype=np.uint32)
    iv = np.zeros((B, 16), dtype=np.uint8)
    on_gpu = batch.dev.type != "cpu"
    for i in range(B):
        if not en[i]:
            continue
        if keys[i] is None or len(keys[i]) != 16 or ivs[i] is None or len(ivs[i]) != 16:
            raise ValueError("sample_decrypt_batch: a key and an IV must be 16 bytes each")
        # the kernel takes little-endian column words, the host big-endian ones
        drk[i] = aes.round_keys_le(bytes(keys[i])) if on_gpu else aes.round_keys(bytes(keys[i]))
        iv[i] = np.frombuffer(bytes(ivs[i]), dtype=np.uint8)
    sa = SampleAes(batch.table(0, SAINFO_WORDS, torch.int64))
    if not on_gpu:
        _rt().sample_decrypt_batch(*batch.host_args(), drk, iv, en, sa.sainfo.numpy())
        return sa
    d, _ = batch.on_device(batch.cap, "ES", 0)
    if B:
        k = pack_to_device({"drk": drk, "iv": iv, "en": en}, batch.dev)
        tdl, isb = aes.device_tables(batch.dev)
        _dev().sample_aes_decrypt(*batch.device_args(d), k["drk"], k["iv"], k["en"], tdl, isb, sa.sainfo)
    return sa
