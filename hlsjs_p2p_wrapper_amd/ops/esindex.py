"""Sample index of demuxed segments: NAL units, access units and ADTS frames
(``docs/ESINDEX.md`` holds the rules).

:func:`index_batch` takes the :class:`~.tsdemux.DemuxResult` of a batch and returns, per
segment (identical for the gfx950 kernels and the host implementation):

* ``nal[i, k] = (offset, length, type, access unit)`` of the k-th NAL unit of the video ES
  (Annex-B start codes; offsets relative to the video ES; emulation prevention stays);
* ``au[i, a] = (first NAL, NAL count, flags, size)`` per video PES (:data:`AU_FLAGS`);
* ``aframes[i, k] = (ADTS frames, bytes consumed)`` per audio PES;
* ``sinfo[i]`` = status bits and totals (slot names in :data:`SINFO`).

The ES bytes stay where the demux put them and the lengths are read from the ``info`` rows
on the device, so demux -> index needs no host round trip; ``caps`` (the host upper bounds
the demux was sized with) size the grid and bound every access.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import numpy as np
import torch

from ._native import device as _dev
from ._native import runtime as _rt
from .desc import check_ranges, pack_to_device
from .tsdemux import DemuxResult

SINFO = {"status": 0, "n_nal": 1, "n_au": 2, "n_keyframe_aus": 3, "first_keyframe_au": 4, "n_adts_frames": 5,
         "audio_sample_rate": 6, "audio_channels": 7}
SINFO_WORDS = 8
SSTATUS = {"nal_overflow": 1, "adts_error": 2, "unsupported_video": 4}
AU_FLAGS = {"keyframe": 1, "sps": 2, "pps": 4, "aud": 8}
DEFAULT_MAX_NAL = 2048


@dataclass
class EsIndex:
    nal: torch.Tensor      # int32[B, max_nal, 4]
    au: torch.Tensor       # int32[B, max_pes, 4]
    aframes: torch.Tensor  # int32[B, max_pes, 2]
    sinfo: torch.Tensor    # int64[B, 8]

    def segment(self, i: int) -> dict:
        """Host view of segment ``i`` (syncs): the ``sinfo`` fields by name, ``independent``
        (access unit 0 holds a keyframe) and the filled rows of the three tables."""
        sinfo = self.sinfo[i].cpu().numpy()
        out = {k: int(sinfo[v]) for k, v in SINFO.items()}
        out["independent"] = out["first_keyframe_au"] == 0
        out["nal"] = self.nal[i, :min(out["n_nal"], self.nal.shape[1])].cpu().numpy()
        out["au"] = self.au[i, :out["n_au"]].cpu().numpy()
        af = self.aframes[i].cpu().numpy()
        out["aframes"] = af[af[:, 0] >= 0]
        return out


def index_batch(res: DemuxResult, caps: Sequence[int], max_nal: int = DEFAULT_MAX_NAL) -> EsIndex:
    """Index every segment of a demuxed batch on the device its tensors live on.  ``caps[i]``
    bounds segment i's ES bytes (what ``demux_batch`` was sized with)."""
    eo = np.asarray(res.es_offs, dtype=np.int64)
    cap = np.asarray(caps, dtype=np.int64)
    B = len(eo)
    max_pes = int(res.pes.shape[2])
    max_nal = int(max_nal)
    if max_nal <= 0:
        raise ValueError("index_batch: max_nal must be positive")
    es = res.es
    check_ranges("index_batch", "ES", eo, cap, es.numel())
    dev = es.device
    if dev.type == "cpu":
        nal = np.empty((B, max_nal, 4), dtype=np.int32)
        au = np.empty((B, max_pes, 4), dtype=np.int32)
        aframes = np.empty((B, max_pes, 2), dtype=np.int32)
        sinfo = np.empty((B, SINFO_WORDS), dtype=np.int64)
        _rt().index_batch(es.numpy(), eo, cap, res.info.numpy(), res.pes.numpy(), max_pes, max_nal, nal, au, aframes,
                          sinfo)
        return EsIndex(torch.from_numpy(nal), torch.from_numpy(au), torch.from_numpy(aframes), torch.from_numpy(sinfo))
    if np.any(eo % 16):
        raise ValueError("index_batch: ES offsets must be 16-byte aligned on device")
    tile = _dev().es_index_tile_bytes()
    if np.any(cap >= 2 ** 31 - tile):
        raise ValueError("index_batch: a segment's ES must be below 2 GiB")
    # the video ES is read in dwords: a segment may not reach into a trailing partial dword of the buffer
    if np.any(eo + cap > es.numel() - es.numel() % 4):
        raise ValueError("index_batch: ES range reaches the buffer's last partial dword on device")
    tiles = (cap + tile - 1) // tile
    tile_prefix = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(tiles, out=tile_prefix[1:])
    total_tiles = int(tile_prefix[-1])
    d = pack_to_device({"eo": eo, "cap": cap, "tp": tile_prefix}, dev)
    scratch = torch.empty(_dev().es_index_scratch_words(total_tiles, B, max_nal), dtype=torch.int32, device=dev)
    nal = torch.empty((B, max_nal, 4), dtype=torch.int32, device=dev)
    au = torch.empty((B, max_pes, 4), dtype=torch.int32, device=dev)
    aframes = torch.empty((B, max_pes, 2), dtype=torch.int32, device=dev)
    sinfo = torch.empty((B, SINFO_WORDS), dtype=torch.int64, device=dev)
    if B:
        _dev().es_index(es, d["eo"], d["cap"], d["tp"], total_tiles, res.info, res.pes, max_pes, max_nal, scratch, nal,
                        au, aframes, sinfo)
    return EsIndex(nal, au, aframes, sinfo)
