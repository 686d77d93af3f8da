"""CEA-608/708 caption data of demuxed and indexed segments: what hls.js emits through
``FRAG_PARSING_USERDATA`` (``docs/CAPTIONS.md`` holds the rules).

:func:`caption_batch` takes the :class:`~.tsdemux.DemuxResult` of a batch and its
:class:`~.esindex.EsIndex` and returns, per enabled segment (identical for the gfx950 kernels and
the host implementation):

* ``ccsamples[i, r]`` = ``(nal, au, size, cc_count, order, field1_pairs, field2_pairs, flags)`` of
  the r-th SEI NAL unit (H.264 type 6, HEVC prefix SEI 39) that holds an ATSC A/53 ``GA94`` caption
  message, in NAL row order (slot names in :data:`CCROW`); ``order`` is its presentation rank;
* ``ccpts[i, r]``: the pts of its access unit;
* ``ccbytes[i, r]``: the ``2 + 3 cc_count`` bytes hls.js hands on (``cc_count`` byte, ``em_data``,
  the triples), zero behind;
* ``cc608[i, r, f]``: the 608 byte pairs of field ``f + 1``, parity stripped, two bytes each;
* ``ccinfo[i]`` = status bits and totals (slot names in :data:`CCINFO`).

The ES is only read.  The 608 / 708 decoding itself (control codes, screens, cues) is host work
for whoever listens.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from ._native import device as _dev
from ._native import runtime as _rt
from .esindex import EsIndex, IndexedBatch
from .tsdemux import DemuxResult

CCINFO = {"status": 0, "n_sei": 1, "n_samples": 2, "n_triples": 3, "field1_pairs": 4, "field2_pairs": 5,
          "first_pts": 6, "last_pts": 7}
CCINFO_WORDS = 8
CCSTATUS = {"truncated": 1, "unsupported_video": 2, "cc_overflow": 4, "sei_clipped": 8}
CCROW = {"nal": 0, "au": 1, "size": 2, "cc_count": 3, "order": 4, "field1_pairs": 5, "field2_pairs": 6, "flags": 7}
CCROW_WORDS = 8
CC_SLOT_BYTES = 96
CC_FIELD_BYTES = 64
CC_NAL_BYTES = 1024
DEFAULT_MAX_CC = 512
MAX_CC_LIMIT = 2048


@dataclass
class Captions:
    ccinfo: torch.Tensor     # int64[B, CCINFO_WORDS]
    ccsamples: torch.Tensor  # int32[B, max_cc, CCROW_WORDS]
    ccpts: torch.Tensor      # int64[B, max_cc]
    ccbytes: torch.Tensor    # uint8[B, max_cc, CC_SLOT_BYTES]
    cc608: torch.Tensor      # uint8[B, max_cc, 2, CC_FIELD_BYTES]

    def segment(self, i: int) -> dict:
        """Host view of segment ``i`` (syncs): the ``ccinfo`` fields by name, ``samples`` and
        ``field1`` / ``field2`` in presentation order."""
        return segment_view(self.ccinfo[i].cpu().numpy(), self.ccsamples[i].cpu().numpy(), self.ccpts[i].cpu().numpy(),
                            self.ccbytes[i].cpu().numpy(), self.cc608[i].cpu().numpy())


def segment_view(ccinfo_row, samples, pts, data, cc608) -> dict:
    """One segment's host rows by name: the ``ccinfo`` fields, ``samples`` (a list of
    ``{"type": 3, "pts", "bytes", "au", "nal"}``, hls.js's user-data samples) and ``field1`` /
    ``field2`` (lists of ``(pts, b1, b2)``), all in presentation order."""
    out = {k: int(ccinfo_row[v]) for k, v in CCINFO.items()}
    n = min(max(out["n_samples"], 0), samples.shape[0])
    rows = sorted(range(n), key=lambda r: int(samples[r, CCROW["order"]]))
    out["samples"] = [{"type": 3, "pts": int(pts[r]), "bytes": data[r, :int(samples[r, CCROW["size"]])].tobytes(),
                       "au": int(samples[r, CCROW["au"]]), "nal": int(samples[r, CCROW["nal"]])} for r in rows]
    for f, name in enumerate(("field1", "field2")):
        col = CCROW[name + "_pairs"]
        out[name] = [(int(pts[r]), int(cc608[r, f, 2 * j]), int(cc608[r, f, 2 * j + 1]))
                     for r in rows for j in range(int(samples[r, col]))]
    return out


def caption_batch(res: DemuxResult, ix: EsIndex, caps: Sequence[int], max_cc: int = DEFAULT_MAX_CC,
                  enable: Optional[Sequence[bool]] = None) -> Captions:
    """The caption samples of every enabled segment of a demuxed and indexed batch, on the device
    its tensors live on and on the caller's stream.  ``caps`` are what ``index_batch`` took;
    ``max_cc`` (1 to 2048) bounds the recorded samples of a segment; ``enable[i]`` false gives
    segment i the fill values and an all-zero ``ccinfo`` row."""
    max_cc = int(max_cc)
    if not 1 <= max_cc <= MAX_CC_LIMIT:
        raise ValueError("caption_batch: max_cc must be 1 to 2048")
    B = len(res.es_offs)
    if enable is not None and len(enable) != B:
        raise ValueError("caption_batch: one enable flag per segment")
    batch = IndexedBatch("caption_batch", res, ix, caps)
    dev = batch.dev
    en = np.ones(B, dtype=np.uint8) if enable is None else np.asarray([bool(e) for e in enable], dtype=np.uint8)
    cc = Captions(batch.table(0, CCINFO_WORDS, torch.int64), batch.table(max_cc, CCROW_WORDS),
                  torch.empty((B, max_cc), dtype=torch.int64, device=dev),
                  torch.empty((B, max_cc, CC_SLOT_BYTES), dtype=torch.uint8, device=dev),
                  torch.empty((B, max_cc, 2, CC_FIELD_BYTES), dtype=torch.uint8, device=dev))
    if dev.type == "cpu":
        _rt().caption_batch(*batch.host_args(), en, max_cc, cc.ccsamples.numpy(), cc.ccpts.numpy(), cc.ccbytes.numpy(),
                            cc.cc608.numpy(), cc.ccinfo.numpy())
        return cc
    d, _ = batch.on_device(batch.cap, "ES", 0, en=("enable", en, 1))  # one packed copy with the descriptors
    if B:
        scratch = torch.empty(_dev().cc_scratch_words(B, batch.max_nal), dtype=torch.int32, device=dev)
        _dev().cc_extract(*batch.device_args(d), d["en"], max_cc, scratch, cc.ccsamples, cc.ccpts, cc.ccbytes, cc.cc608,
                          cc.ccinfo)
    return cc
