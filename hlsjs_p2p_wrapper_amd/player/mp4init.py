"""The init segment of a fragmented-MP4 rendition (``#EXT-X-MAP``): what the fMP4 demux needs to
know about its tracks (``docs/FMP4DEMUX.md``).

A few hundred bytes once per rendition, host work by design.  :func:`parse_init` walks ``moov`` →
``trak`` → ``tkhd`` / ``mdia`` → ``mdhd`` / ``hdlr`` / ``minf`` → ``stbl`` → ``stsd`` (first entry)
and ``moov`` → ``mvex`` → ``trex``, keeps the first video and the first audio track, and hands the
raw bytes on untouched, as hls.js does.  A protected sample entry (``encv`` / ``enca`` with a
``sinf``) is read as the format its ``frma`` names, and its ``schm`` / ``tenc`` become the track's
``protection`` (``docs/CBCS.md``).
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Dict, Iterator, Optional, Tuple

from ..ops.cbcs import Mp4Protection
from ..ops.mp4demux import Mp4Track
from . import fmp4

_CONTAINERS = (b"moov", b"trak", b"mdia", b"minf", b"stbl", b"mvex")
_VISUAL_ENTRY_BYTES = 78  # SampleEntry (8) + VisualSampleEntry fields in front of the child boxes
_AUDIO_ENTRY_BYTES = 28   # SampleEntry (8) + AudioSampleEntry fields in front of the child boxes


@dataclass(frozen=True)
class Mp4Init:
    """``video`` / ``audio``: the first track of each kind or ``None``; ``timescale``: per kind;
    ``video_codec`` / ``audio_codec``: the codec string where one can be formed (``avc1.xxyyzz``,
    ``hvc1...``; ``mp4a`` by name only), else the sample entry's name; ``data``: the raw bytes;
    ``clear_data``: the bytes a consumer of decrypted fragments needs, of the same length: every
    protected entry carries its ``frma`` format as its type and its ``sinf`` box is a ``free`` box
    (``data`` itself when no track is protected)."""
    data: bytes
    video: Optional[Mp4Track]
    audio: Optional[Mp4Track]
    timescale: Dict[str, int]
    video_codec: Optional[str]
    audio_codec: Optional[str]
    clear_data: Optional[bytes] = None

    def __post_init__(self) -> None:
        if self.clear_data is None:
            object.__setattr__(self, "clear_data", self.data)

    @property
    def tracks(self) -> Tuple[Mp4Track, ...]:
        return tuple(t for t in (self.video, self.audio) if t is not None)


def _boxes(data: bytes, p: int, end: int) -> Iterator[Tuple[bytes, int, int]]:
    """(type, body start, box end) of every box of ``data[p:end]``; a malformed one raises."""
    while p < end:
        if end - p < 8:
            raise ValueError("init segment: bytes behind the last box")
        size, kind = struct.unpack_from(">I4s", data, p)
        hdr = 8
        if size == 1:
            if end - p < 16:
                raise ValueError("init segment: a 64-bit size runs off its container")
            size, hdr = struct.unpack_from(">Q", data, p + 8)[0], 16
        elif size == 0:
            size = end - p
        if size < hdr or p + size > end:
            raise ValueError(f"init segment: box {kind!r} does not fit its container")
        yield kind, p + hdr, p + size
        p += size


def _need(data: bytes, p: int, end: int, n: int, what: str) -> None:
    if end - p < n:
        raise ValueError(f"init segment: {what} too short")


def _hevc_codec(rec: bytes) -> Optional[str]:
    cfg = {"status": 0, "profile_space": rec[1] >> 6, "tier_flag": (rec[1] >> 5) & 1, "profile_idc": rec[1] & 31,
           "profile_compat": int.from_bytes(rec[2:6], "big"), "constraint_hi": int.from_bytes(rec[6:8], "big"),
           "constraint_lo": int.from_bytes(rec[8:12], "big"), "level_idc": rec[12],
           "bit_depth_luma": 8 + (rec[17] & 7), "bit_depth_chroma": 8 + (rec[18] & 7)}
    return fmp4.hevc_codec(cfg)


def _video_entry(data: bytes, kind: bytes, p: int, end: int):
    """(codec_type, nal_length_size, codec string) of a visual sample entry."""
    name = kind.decode("latin-1")
    if kind not in (b"avc1", b"avc3", b"hvc1", b"hev1") or end - p < _VISUAL_ENTRY_BYTES:
        return 0, 4, name
    for child, cp, ce in _boxes(data, p + _VISUAL_ENTRY_BYTES, end):
        if kind in (b"avc1", b"avc3") and child == b"avcC":
            _need(data, cp, ce, 5, "avcC")
            size = (data[cp + 4] & 3) + 1
            codec = "%s.%02x%02x%02x" % (name, data[cp + 1], data[cp + 2], data[cp + 3])
            return (0x1B, size, codec) if size != 3 else (0, 4, codec)
        if kind in (b"hvc1", b"hev1") and child == b"hvcC":
            _need(data, cp, ce, 22, "hvcC")
            size = (data[cp + 21] & 3) + 1
            codec = _hevc_codec(data[cp:ce])
            codec = name + codec[4:] if codec else name  # the entry's own name in front (hev1)
            return (0x24, size, codec) if size != 3 else (0, 4, codec)
    return 0, 4, name


def _type_at(data: bytes, body: int, kind: bytes) -> int:
    """Where the 4-byte type of the box with this body start lies (an 8- or a 16-byte header)."""
    return body - 4 if data[body - 4:body] == kind else body - 12


def _protected_entry(data: bytes, kind: bytes, p: int, end: int):
    """(original format, Mp4Protection or None, position of the sinf box's type) of an ``encv`` /
    ``enca`` entry whose ``sinf`` holds ``frma``, ``schm`` and ``schi`` / ``tenc``; ``None`` when a
    piece is missing or too short."""
    fixed = _VISUAL_ENTRY_BYTES if kind == b"encv" else _AUDIO_ENTRY_BYTES
    if end - p < fixed:
        return None
    try:
        sinf = next(((cp, ce) for child, cp, ce in _boxes(data, p + fixed, end) if child == b"sinf"), None)
        if sinf is None:
            return None
        frma = scheme = tenc = None
        for child, cp, ce in _boxes(data, *sinf):
            if child == b"frma" and frma is None and ce - cp >= 4:
                frma = data[cp:cp + 4]
            elif child == b"schm" and scheme is None and ce - cp >= 12:
                scheme = data[cp + 4:cp + 8].decode("latin-1")
            elif child == b"schi" and tenc is None:
                tenc = next(((tp, te) for t, tp, te in _boxes(data, cp, ce) if t == b"tenc"), None)
    except ValueError:
        return None
    if frma is None or scheme is None or tenc is None or tenc[1] - tenc[0] < 24:
        return None
    tp, te = tenc
    version, pattern, is_protected, iv_size = data[tp], data[tp + 5], data[tp + 6], data[tp + 7]
    kid, constant = data[tp + 8:tp + 24], b""
    if is_protected == 1 and iv_size == 0:
        if te - tp < 25 or te - tp < 25 + data[tp + 24]:
            return None
        constant = data[tp + 25:tp + 25 + data[tp + 24]]
    crypt, skip = (pattern >> 4, pattern & 15) if version >= 1 else (0, 0)
    protection = Mp4Protection(scheme, crypt, skip, iv_size, constant, kid) if is_protected else None
    return frma, protection, _type_at(data, sinf[0], b"sinf")


def parse_init(data: bytes) -> Mp4Init:
    """The tracks of an init segment; ``ValueError`` for a malformed box tree or one without a
    ``moov`` or without a video or audio track."""
    data = bytes(data)
    found: Dict[str, dict] = {}
    trex: Dict[int, Tuple[int, int, int]] = {}
    moov = next(((p, e) for kind, p, e in _boxes(data, 0, len(data)) if kind == b"moov"), None)
    if moov is None:
        raise ValueError("init segment: no moov box")
    for kind, p, e in _boxes(data, *moov):
        if kind == b"mvex":
            for child, cp, ce in _boxes(data, p, e):
                if child == b"trex":
                    _need(data, cp, ce, 24, "trex")
                    tid, _, dur, size, flags = struct.unpack_from(">IIIII", data, cp + 4)
                    trex.setdefault(tid, (dur, size, flags))
        elif kind == b"trak":
            track = {"id": None, "timescale": None, "handler": None, "entry": None}
            for child, cp, ce in _boxes(data, p, e):
                if child == b"tkhd":
                    _need(data, cp, ce, 4, "tkhd")
                    wide = data[cp] == 1
                    _need(data, cp, ce, 4 + (16 if wide else 8) + 4, "tkhd")
                    track["id"] = struct.unpack_from(">I", data, cp + 4 + (16 if wide else 8))[0]
                elif child == b"mdia":
                    for m, mp, me in _boxes(data, cp, ce):
                        if m == b"mdhd":
                            _need(data, mp, me, 4, "mdhd")
                            wide = data[mp] == 1
                            _need(data, mp, me, 4 + (16 if wide else 8) + 4, "mdhd")
                            track["timescale"] = struct.unpack_from(">I", data, mp + 4 + (16 if wide else 8))[0]
                        elif m == b"hdlr":
                            _need(data, mp, me, 12, "hdlr")
                            track["handler"] = data[mp + 8:mp + 12]
                        elif m == b"minf":
                            for s, sp, se in (x for k, a, b in _boxes(data, mp, me) if k == b"stbl"
                                              for x in _boxes(data, a, b)):
                                if s == b"stsd":
                                    _need(data, sp, se, 8, "stsd")
                                    track["entry"] = next(iter(_boxes(data, sp + 8, se)), None)
            name = {b"vide": "video", b"soun": "audio"}.get(track["handler"])
            if name and name not in found and track["id"] and track["entry"] is not None:
                found[name] = track
    if not found:
        raise ValueError("init segment: no video or audio track")
    tracks, codecs = {"video": None, "audio": None}, {"video": None, "audio": None}
    clear = None
    for name, t in found.items():
        kind, p, e = t["entry"]
        dur, size, flags = trex.get(t["id"], (0, 0, 0))
        protection = None
        if kind == (b"encv" if name == "video" else b"enca"):
            sinf = _protected_entry(data, kind, p, e)
            if sinf is not None:
                at = _type_at(data, p, kind)
                kind, protection = sinf[0], sinf[1]
                if protection is not None:
                    clear = bytearray(data) if clear is None else clear
                    clear[at:at + 4] = kind
                    clear[sinf[2]:sinf[2] + 4] = b"free"
        if name == "video":
            ctype, length_size, codecs[name] = _video_entry(data, kind, p, e)
        else:
            ctype, length_size, codecs[name] = (0x0F if kind == b"mp4a" else 0), 4, kind.decode("latin-1")
        tracks[name] = Mp4Track(t["id"], name, ctype, length_size, dur, size, flags, protection)
    return Mp4Init(data, tracks["video"], tracks["audio"], {k: int(t["timescale"] or 0) for k, t in found.items()},
                   codecs["video"], codecs["audio"], data if clear is None else bytes(clear))
