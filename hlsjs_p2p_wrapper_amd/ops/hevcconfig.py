"""HEVC configuration of demuxed and indexed segments: what an ``hvc1`` init segment is built
from (``docs/INITSEGMENT.md`` holds the rules).

:func:`hevc_config_batch` takes the :class:`~.tsdemux.DemuxResult` of a batch and its
:class:`~.esindex.EsIndex` and returns, per segment (identical for the gfx950 kernel and the
host implementation):

* ``hps[i, 0]`` / ``hps[i, 1]`` / ``hps[i, 2]``: the first VPS, SPS and PPS NAL units of an HEVC
  video ES as they are (two header bytes first, emulation prevention kept), zero behind the
  stored bytes;
* ``hinfo[i]``: status bits, where the three NAL units were found and how long they are, and what
  the SPS says up to its bit depths (profile, tier, level, compatibility and constraint flags,
  temporal layers, chroma format, bit depths, picture size; slot names in :data:`HINFO`).

A segment of any other codec gets ``not_hevc`` and zeros.  Audio is not repeated here: it stays in
``cinfo`` (:mod:`.codecconfig`).  One launch of one workgroup per segment, no scratch and no tile
space.  The boxes are host work: ``player/fmp4.py``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import torch

from ._native import device as _dev
from ._native import runtime as _rt
from .esindex import EsIndex, IndexedBatch
from .tsdemux import DemuxResult

HINFO = {"status": 0, "vps_nal": 1, "vps_bytes": 2, "sps_nal": 3, "sps_bytes": 4, "sps_rbsp_bytes": 5, "pps_nal": 6,
         "pps_bytes": 7, "profile_space": 8, "tier_flag": 9, "profile_idc": 10, "profile_compat": 11,
         "constraint_hi": 12, "constraint_lo": 13, "level_idc": 14, "num_temporal_layers": 15,
         "temporal_id_nested": 16, "chroma_format_idc": 17, "bit_depth_luma": 18, "bit_depth_chroma": 19, "width": 20,
         "height": 21}
HINFO_WORDS = 22
HSTATUS = {"no_vps": 1, "no_sps": 2, "no_pps": 4, "ps_overflow": 8, "bad_sps": 16, "not_hevc": 32}
HPS_ROWS = 3
DEFAULT_MAX_PS = 256
MAX_PS_LIMIT = 1024


@dataclass
class HevcConfig:
    hinfo: torch.Tensor  # int32[B, HINFO_WORDS]
    hps: torch.Tensor    # uint8[B, 3, max_ps]

    def segment(self, i: int) -> dict:
        """Host view of segment ``i`` (syncs): the ``hinfo`` fields by name plus ``vps`` / ``sps`` /
        ``pps``, the stored bytes of the three NAL units."""
        return segment_view(self.hinfo[i].cpu().numpy(), self.hps[i].cpu().numpy())


def segment_view(hinfo_row, hps_rows) -> dict:
    """One segment's host rows by name: the ``hinfo`` fields and ``vps`` / ``sps`` / ``pps`` as bytes."""
    out = {k: int(hinfo_row[v]) for k, v in HINFO.items()}
    max_ps = hps_rows.shape[-1]
    for row, name in enumerate(("vps", "sps", "pps")):
        out[name] = hps_rows[row, :min(max(out[name + "_bytes"], 0), max_ps)].tobytes()
    return out


def hevc_config_batch(res: DemuxResult, ix: EsIndex, caps: Sequence[int], max_ps: int = DEFAULT_MAX_PS) -> HevcConfig:
    """The HEVC configuration of every segment of a demuxed and indexed batch, on the device its
    tensors live on.  ``caps`` are what ``index_batch`` took; ``max_ps`` bounds the stored bytes of
    a parameter set (a positive multiple of 16, at most 1024)."""
    max_ps = int(max_ps)
    if max_ps <= 0 or max_ps % 16 or max_ps > MAX_PS_LIMIT:
        raise ValueError("hevc_config_batch: max_ps must be a positive multiple of 16 up to 1024")
    batch = IndexedBatch("hevc_config_batch", res, ix, caps)
    cfg = HevcConfig(batch.table(0, HINFO_WORDS), batch.table(HPS_ROWS, max_ps, torch.uint8))
    if batch.dev.type == "cpu":
        _rt().hevc_config_batch(*batch.host_args(), max_ps, cfg.hinfo.numpy(), cfg.hps.numpy())
        return cfg
    d, _ = batch.on_device(batch.cap, "ES", 0)
    if batch.B:
        _dev().hevc_config(*batch.device_args(d), max_ps, cfg.hinfo, cfg.hps)
    return cfg
