"""Movie fragment boxes for the remuxed samples (``docs/REMUX.md``): the ``moof`` that goes in
front of an ``mdat`` box written by :func:`..ops.remux.remux_batch`.

Host work on a few KB: the per-sample rows are packed big-endian with numpy in one piece, no
Python loop per sample.  A fragment is ``moof{ mfhd, traf{ tfhd, tfdt, trun } }`` with
``default-base-is-moof`` and a ``trun`` data offset that points behind the 8-byte header of the
``mdat`` that follows the ``moof`` directly.
"""
from __future__ import annotations

import struct

import numpy as np

VIDEO_TRACK = 1
AUDIO_TRACK = 2
VIDEO_TIMESCALE = 90000
AAC_FRAME_SAMPLES = 1024
AUDIO_SAMPLE_FLAGS = 0x02000000  # every AAC frame is a sync sample

_TFHD_DEFAULT_DURATION = 0x000008
_TFHD_DEFAULT_FLAGS = 0x000020
_TFHD_BASE_IS_MOOF = 0x020000
_TRUN_DATA_OFFSET = 0x000001
_TRUN_DURATION = 0x000100
_TRUN_SIZE = 0x000200
_TRUN_FLAGS = 0x000400
_TRUN_CTS = 0x000800


def _box(kind: bytes, payload: bytes) -> bytes:
    return struct.pack(">I4s", 8 + len(payload), kind) + payload


def _full(kind: bytes, version: int, flags: int, payload: bytes) -> bytes:
    return _box(kind, struct.pack(">I", (version << 24) | flags) + payload)


def _moof(sequence_number: int, tfhd: bytes, base: int, trun_flags: int, version: int, rows: np.ndarray) -> bytes:
    """``rows``: ``>u4[n, k]``, the trun's per-sample fields in box order."""
    mfhd = _full(b"mfhd", 0, 0, struct.pack(">I", sequence_number & 0xFFFFFFFF))
    tfdt = _full(b"tfdt", 1, 0, struct.pack(">Q", max(int(base), 0)))
    body = rows.tobytes()
    trun_size = 8 + 4 + 4 + 4 + len(body)
    moof_size = 8 + len(mfhd) + 8 + len(tfhd) + len(tfdt) + trun_size
    trun = _full(b"trun", version, trun_flags, struct.pack(">Ii", len(rows), moof_size + 8) + body)
    return _box(b"moof", mfhd + _box(b"traf", tfhd + tfdt + trun))


def video_moof(sequence_number: int, base_dts: int, vsamples) -> bytes:
    """The video fragment: track 1 at 90 kHz, ``tfdt`` = ``base_dts``, a version-1 ``trun`` with
    duration, size, flags and signed composition offset per ``vsamples`` row
    ``(offset, size, duration, cts, flags)``."""
    v = np.asarray(vsamples, dtype=np.int32).reshape(-1, 5)
    rows = np.empty((len(v), 4), dtype=">u4")
    rows[:, 0] = v[:, 2].astype(np.uint32)
    rows[:, 1] = v[:, 1].astype(np.uint32)
    rows[:, 2] = v[:, 4].astype(np.uint32)
    rows[:, 3] = v[:, 3].astype(np.uint32)  # two's complement: the box field is signed in version 1
    tfhd = _full(b"tfhd", 0, _TFHD_BASE_IS_MOOF, struct.pack(">I", VIDEO_TRACK))
    return _moof(sequence_number, tfhd, base_dts,
                 _TRUN_DATA_OFFSET | _TRUN_DURATION | _TRUN_SIZE | _TRUN_FLAGS | _TRUN_CTS, 1, rows)


def audio_base(base_pts: int, sample_rate: int) -> int:
    """A 90 kHz stamp in the audio track's timescale (its sample rate), rounded to nearest."""
    if base_pts < 0 or sample_rate <= 0:
        return 0
    return (int(base_pts) * int(sample_rate) + VIDEO_TIMESCALE // 2) // VIDEO_TIMESCALE


def audio_moof(sequence_number: int, base_pts: int, sample_rate: int, asamples) -> bytes:
    """The audio fragment: track 2 in units of ``sample_rate``, ``tfdt`` = the rescaled
    ``base_pts``, 1024 samples and sync flags per frame as ``tfhd`` defaults, a ``trun`` with one
    size per ``asamples`` row ``(offset, size)``."""
    a = np.asarray(asamples, dtype=np.int32).reshape(-1, 2)
    rows = np.empty((len(a), 1), dtype=">u4")
    rows[:, 0] = a[:, 1].astype(np.uint32)
    tfhd = _full(b"tfhd", 0, _TFHD_BASE_IS_MOOF | _TFHD_DEFAULT_DURATION | _TFHD_DEFAULT_FLAGS,
                 struct.pack(">III", AUDIO_TRACK, AAC_FRAME_SAMPLES, AUDIO_SAMPLE_FLAGS))
    return _moof(sequence_number, tfhd, audio_base(base_pts, sample_rate), _TRUN_DATA_OFFSET | _TRUN_SIZE, 0, rows)
