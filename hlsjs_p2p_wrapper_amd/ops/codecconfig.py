"""Codec configuration of demuxed and indexed segments: what an fMP4 init segment is built from
(``docs/INITSEGMENT.md`` holds the rules).

:func:`config_batch` takes the :class:`~.tsdemux.DemuxResult` of a batch and its
:class:`~.esindex.EsIndex` and returns, per segment (identical for the gfx950 kernel and the
host implementation):

* ``ps[i, 0]`` / ``ps[i, 1]``: the first SPS and PPS NAL units of an H.264 video ES as they
  are (header byte first, emulation prevention kept), zero behind the stored bytes;
* ``cinfo[i]``: status bits, where the two NAL units were found and how long they are, what the
  SPS says (profile, level, chroma format, bit depths, picture size, sample aspect ratio) and the
  three ADTS header fields of an AudioSpecificConfig (slot names in :data:`CINFO`).

Everything the device path reads is already in HBM after ``index_batch``: one launch of one
workgroup per segment, no scratch and no tile space.  The boxes are host work:
``player/fmp4.py``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import torch

from ._native import device as _dev
from ._native import runtime as _rt
from .esindex import EsIndex, IndexedBatch
from .tsdemux import DemuxResult

CINFO = {"status": 0, "sps_nal": 1, "sps_bytes": 2, "sps_rbsp_bytes": 3, "pps_nal": 4, "pps_bytes": 5,
         "profile_idc": 6, "profile_compat": 7, "level_idc": 8, "chroma_format_idc": 9, "bit_depth_luma": 10,
         "bit_depth_chroma": 11, "width": 12, "height": 13, "sar_width": 14, "sar_height": 15, "aac_object_type": 16,
         "aac_rate_index": 17, "aac_channel_config": 18}
CINFO_WORDS = 19
CSTATUS = {"no_sps": 1, "no_pps": 2, "ps_overflow": 4, "bad_sps": 8, "unsupported_video": 16, "no_audio_config": 32}
DEFAULT_MAX_PS = 256
MAX_PS_LIMIT = 1024


@dataclass
class CodecConfig:
    cinfo: torch.Tensor  # int32[B, CINFO_WORDS]
    ps: torch.Tensor     # uint8[B, 2, max_ps]

    def segment(self, i: int) -> dict:
        """Host view of segment ``i`` (syncs): the ``cinfo`` fields by name plus ``sps`` / ``pps``,
        the stored bytes of the two NAL units."""
        return segment_view(self.cinfo[i].cpu().numpy(), self.ps[i].cpu().numpy())


def segment_view(cinfo_row, ps_rows) -> dict:
    """One segment's host rows by name: the ``cinfo`` fields and ``sps`` / ``pps`` as bytes."""
    out = {k: int(cinfo_row[v]) for k, v in CINFO.items()}
    max_ps = ps_rows.shape[-1]
    out["sps"] = ps_rows[0, :min(max(out["sps_bytes"], 0), max_ps)].tobytes()
    out["pps"] = ps_rows[1, :min(max(out["pps_bytes"], 0), max_ps)].tobytes()
    return out


def config_batch(res: DemuxResult, ix: EsIndex, caps: Sequence[int], max_ps: int = DEFAULT_MAX_PS) -> CodecConfig:
    """The codec configuration of every segment of a demuxed and indexed batch, on the device
    its tensors live on.  ``caps`` are what ``index_batch`` took; ``max_ps`` bounds the stored
    bytes of a parameter set (a positive multiple of 16, at most 1024)."""
    max_ps = int(max_ps)
    if max_ps <= 0 or max_ps % 16 or max_ps > MAX_PS_LIMIT:
        raise ValueError("config_batch: max_ps must be a positive multiple of 16 up to 1024")
    batch = IndexedBatch("config_batch", res, ix, caps)
    cfg = CodecConfig(batch.table(0, CINFO_WORDS), batch.table(2, max_ps, torch.uint8))
    if batch.dev.type == "cpu":
        _rt().config_batch(*batch.host_args(), max_ps, cfg.cinfo.numpy(), cfg.ps.numpy())
        return cfg
    d, _ = batch.on_device(batch.cap, "ES", 0)
    if batch.B:
        _dev().codec_config(*batch.device_args(d), max_ps, cfg.cinfo, cfg.ps)
    return cfg
