"""Movie fragment boxes for the remuxed samples (``docs/REMUX.md``): the ``moof`` that goes in
front of an ``mdat`` box written by :func:`..ops.remux.remux_batch`, and the init segment
(``ftyp`` + ``moov``) of each track from the codec configuration of
:func:`..ops.codecconfig.config_batch` (``docs/INITSEGMENT.md``), or for an HEVC track from
the configuration of :func:`..ops.hevcconfig.hevc_config_batch`.

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


# ---------------------------------------------------------------- init segments (docs/INITSEGMENT.md)
ADTS_RATES = (96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350)
VIDEO_DISQUALIFIED = 1 | 2 | 4 | 8 | 16  # no_sps, no_pps, ps_overflow, bad_sps, unsupported_video
AUDIO_DISQUALIFIED = 32                  # no_audio_config
HEVC_DISQUALIFIED = 1 | 2 | 4 | 8 | 16 | 32  # hinfo: no_vps, no_sps, no_pps, ps_overflow, bad_sps, not_hevc
VIDEO_TREX_FLAGS = 0x01010000            # a non-sync sample; every trun row carries its own flags
_MATRIX = struct.pack(">9I", 0x10000, 0, 0, 0, 0x10000, 0, 0, 0, 0x40000000)


def video_codec(cfg) -> str:
    """The RFC 6381 codec string of the video track of a codec configuration (``ops.codecconfig``)."""
    return "avc1.%02x%02x%02x" % (cfg["profile_idc"], cfg["profile_compat"], cfg["level_idc"])


def audio_codec(cfg) -> str:
    """``mp4a.40.<object type>``: what the ADTS header says, no HE-AAC guess."""
    return "mp4a.40.%d" % cfg["aac_object_type"]


def audio_sample_rate(cfg) -> int:
    idx = cfg["aac_rate_index"]
    return ADTS_RATES[idx] if 0 <= idx < len(ADTS_RATES) else 0


def audio_channels(cfg) -> int:
    """Channels of an ADTS channel configuration (7 is 7.1)."""
    c = cfg["aac_channel_config"]
    return 8 if c == 7 else c


def _init(track: int, timescale: int, handler: bytes, name: bytes, volume: int, width: int, height: int,
          media_header: bytes, entry: bytes, trex: bytes, brand: bytes = b"avc1") -> bytes:
    """``ftyp`` + ``moov`` of one track with empty sample tables and duration 0."""
    ftyp = _box(b"ftyp", b"isom" + struct.pack(">I", 1) + b"isom" + brand)
    mvhd = _full(b"mvhd", 0, 0, struct.pack(">IIIIIH10x", 0, 0, timescale, 0, 0x00010000, 0x0100) + _MATRIX +
                 bytes(24) + struct.pack(">I", 0xFFFFFFFF))
    tkhd = _full(b"tkhd", 0, 7, struct.pack(">III4xI8xHHH2x", 0, 0, track, 0, 0, 0, volume) + _MATRIX +
                 struct.pack(">II", width, height))
    mdhd = _full(b"mdhd", 0, 0, struct.pack(">IIIIHH", 0, 0, timescale, 0, 0x55C4, 0))
    hdlr = _full(b"hdlr", 0, 0, struct.pack(">I4s12x", 0, handler) + name + b"\x00")
    dinf = _box(b"dinf", _full(b"dref", 0, 0, struct.pack(">I", 1) + _full(b"url ", 0, 1, b"")))
    stbl = _box(b"stbl", _full(b"stsd", 0, 0, struct.pack(">I", 1) + entry) + _full(b"stts", 0, 0, bytes(4)) +
                _full(b"stsc", 0, 0, bytes(4)) + _full(b"stsz", 0, 0, bytes(8)) + _full(b"stco", 0, 0, bytes(4)))
    mdia = _box(b"mdia", mdhd + hdlr + _box(b"minf", media_header + dinf + stbl))
    mvex = _box(b"mvex", _full(b"trex", 0, 0, trex))
    return ftyp + _box(b"moov", mvhd + _box(b"trak", tkhd + mdia) + mvex)


def video_init(cfg):
    """The video track's init segment from a codec configuration (``CodecConfig.segment(i)`` or the
    pipeline's ``config`` mapping): ``ftyp`` + ``moov`` with one ``avc1{ avcC, pasp }`` entry, track 1 at
    90 kHz.  ``None`` when the configuration cannot describe the track (no SPS or PPS, an overflowed
    or unparsable SPS, a codec other than H.264)."""
    if cfg["status"] & VIDEO_DISQUALIFIED:
        return None
    sps, pps = bytes(cfg["sps"]), bytes(cfg["pps"])
    width, height, sar_w, sar_h = cfg["width"], cfg["height"], cfg["sar_width"], cfg["sar_height"]
    avcc = _box(b"avcC", bytes([1, cfg["profile_idc"], cfg["profile_compat"], cfg["level_idc"], 0xFF, 0xE1]) +
                struct.pack(">H", len(sps)) + sps + b"\x01" + struct.pack(">H", len(pps)) + pps)
    pasp = _box(b"pasp", struct.pack(">II", sar_w, sar_h))
    avc1 = _box(b"avc1", struct.pack(">6xH16xHHII4xH32xHh", 1, width, height, 0x00480000, 0x00480000, 1, 0x0018, -1)
                + avcc + pasp)
    shown = min((width * sar_w << 16) // sar_h, 0xFFFFFFFF)
    vmhd = _full(b"vmhd", 0, 1, bytes(8))
    trex = struct.pack(">IIIII", VIDEO_TRACK, 1, 0, 0, VIDEO_TREX_FLAGS)
    return _init(VIDEO_TRACK, VIDEO_TIMESCALE, b"vide", b"VideoHandler", 0, shown, height << 16, vmhd, avc1, trex)


def _hevc_constraint_bytes(hcfg) -> bytes:
    """The 48 general constraint-indicator bits of an HEVC configuration as six bytes."""
    return struct.pack(">HI", hcfg["constraint_hi"] & 0xFFFF, hcfg["constraint_lo"] & 0xFFFFFFFF)


def _hevc_describable(hcfg) -> bool:
    """An ``hvcC`` record can describe the configuration: no disqualifying bit, and bit depths its
    three-bit fields hold (up to 15; the SPS syntax goes up to 16)."""
    return not hcfg["status"] & HEVC_DISQUALIFIED and max(hcfg["bit_depth_luma"], hcfg["bit_depth_chroma"]) <= 15


def hevc_codec(hcfg):
    """The RFC 6381 codec string of an HEVC configuration (``ops.hevcconfig``) by ISO/IEC 14496-15
    Annex E: ``hvc1.<space><profile>.<compatibility flags, reversed, hex>.<tier><level>`` and one
    ``.XX`` per constraint byte up to the last non-zero one.  ``None`` like :func:`hevc_init`."""
    if not _hevc_describable(hcfg):
        return None
    compat = hcfg["profile_compat"] & 0xFFFFFFFF
    reversed_compat = int(format(compat, "032b")[::-1], 2)
    out = "hvc1.%s%d.%X.%s%d" % (("", "A", "B", "C")[hcfg["profile_space"]], hcfg["profile_idc"], reversed_compat,
                                 "H" if hcfg["tier_flag"] else "L", hcfg["level_idc"])
    return out + "".join(".%X" % b for b in _hevc_constraint_bytes(hcfg).rstrip(b"\x00"))


def hevc_init(hcfg):
    """The video track's init segment from an HEVC configuration (``HevcConfig.segment(i)`` or the
    pipeline's ``hevc`` mapping): ``ftyp`` (brands ``isom``, ``hvc1``) + ``moov`` with one
    ``hvc1{ hvcC }`` entry, track 1 at 90 kHz, no ``pasp``.  ``None`` when the configuration cannot
    describe the track (no VPS, SPS or PPS, an overflowed or unparsable SPS, a codec other than HEVC,
    a bit depth of 16)."""
    if not _hevc_describable(hcfg):
        return None
    width, height = hcfg["width"], hcfg["height"]
    record = bytes([1, (hcfg["profile_space"] << 6) | (hcfg["tier_flag"] << 5) | hcfg["profile_idc"]]) + \
        struct.pack(">I", hcfg["profile_compat"] & 0xFFFFFFFF) + _hevc_constraint_bytes(hcfg) + \
        bytes([hcfg["level_idc"], 0xF0, 0x00, 0xFC, 0xFC | hcfg["chroma_format_idc"],
               0xF8 | (hcfg["bit_depth_luma"] - 8), 0xF8 | (hcfg["bit_depth_chroma"] - 8), 0, 0,
               (hcfg["num_temporal_layers"] << 3) | (hcfg["temporal_id_nested"] << 2) | 3, 3])
    for nal_type, name in ((32, "vps"), (33, "sps"), (34, "pps")):  # one array per type, one NAL each, complete
        nal = bytes(hcfg[name])
        record += bytes([0x80 | nal_type]) + struct.pack(">HH", 1, len(nal)) + nal
    hvc1 = _box(b"hvc1", struct.pack(">6xH16xHHII4xH32xHh", 1, width, height, 0x00480000, 0x00480000, 1, 0x0018, -1)
                + _box(b"hvcC", record))
    vmhd = _full(b"vmhd", 0, 1, bytes(8))
    trex = struct.pack(">IIIII", VIDEO_TRACK, 1, 0, 0, VIDEO_TREX_FLAGS)
    return _init(VIDEO_TRACK, VIDEO_TIMESCALE, b"vide", b"VideoHandler", 0, width << 16, height << 16, vmhd, hvc1,
                 trex, brand=b"hvc1")


def audio_specific_config(cfg) -> bytes:
    """The two-byte AudioSpecificConfig of the ADTS header fields."""
    return struct.pack(">H", (cfg["aac_object_type"] << 11) | (cfg["aac_rate_index"] << 7) |
                       (cfg["aac_channel_config"] << 3))


def audio_init(cfg):
    """The audio track's init segment: ``ftyp`` + ``moov`` with one ``mp4a{ esds }`` entry, track 2 in
    units of the sample rate.  ``None`` without a usable ADTS header."""
    if cfg["status"] & AUDIO_DISQUALIFIED:
        return None
    rate, channels = audio_sample_rate(cfg), audio_channels(cfg)
    asc = audio_specific_config(cfg)
    dec_specific = b"\x05" + bytes([len(asc)]) + asc
    dec_config = b"\x04" + bytes([13 + len(dec_specific)]) + struct.pack(">BB3xII", 0x40, 0x15, 0, 0) + dec_specific
    es_body = struct.pack(">HB", 1, 0) + dec_config + b"\x06\x01\x02"  # ES_ID 1, no flags, ..., the SL config
    esds = _full(b"esds", 0, 0, b"\x03" + bytes([len(es_body)]) + es_body)
    mp4a = _box(b"mp4a", struct.pack(">6xH8xHHHHI", 1, channels, 16, 0, 0, (rate << 16) if rate < 65536 else 0) + esds)
    smhd = _full(b"smhd", 0, 0, bytes(4))
    trex = struct.pack(">IIIII", AUDIO_TRACK, 1, AAC_FRAME_SAMPLES, 0, AUDIO_SAMPLE_FLAGS)
    return _init(AUDIO_TRACK, rate, b"soun", b"SoundHandler", 0x0100, 0, 0, smhd, mp4a, trex)


MPEG_AUDIO_DISQUALIFIED = 1 | 2  # mpainfo: not_mpeg_audio, no_audio_config


def mpeg_audio_codec(m):
    """The RFC 6381 codec string of an MPEG audio track from its ``mpainfo`` fields
    (``ops.mpegaudio``, ``docs/MPEGAUDIO.md``): ``mp4a.6b`` (object type 0x6B, MPEG-1 audio) or
    ``mp4a.69`` (0x69, MPEG-2 audio, which MPEG-2.5 rides on).  ``None`` without a config."""
    if m["status"] & MPEG_AUDIO_DISQUALIFIED or m["frame_samples"] <= 0:
        return None
    return "mp4a.6b" if m["version"] == 1 else "mp4a.69"


def mpeg_audio_init(m):
    """The audio track's init segment for MPEG audio: :func:`audio_init`'s ``ftyp`` + ``moov`` with
    one ``mp4a{ esds }`` entry whose decoder configuration carries the object type 0x6B / 0x69 and
    no decoder-specific info, track 2 in units of the sample rate, ``trex`` default duration one
    frame's samples.  ``None`` without a config."""
    if mpeg_audio_codec(m) is None:
        return None
    rate, channels = int(m["sample_rate"]), int(m["channels"])
    dec_config = b"\x04" + bytes([13]) + struct.pack(">BB3xII", 0x6B if m["version"] == 1 else 0x69, 0x15, 0, 0)
    es_body = struct.pack(">HB", 1, 0) + dec_config + b"\x06\x01\x02"
    esds = _full(b"esds", 0, 0, b"\x03" + bytes([len(es_body)]) + es_body)
    mp4a = _box(b"mp4a", struct.pack(">6xH8xHHHHI", 1, channels, 16, 0, 0, (rate << 16) if rate < 65536 else 0) + esds)
    smhd = _full(b"smhd", 0, 0, bytes(4))
    trex = struct.pack(">IIIII", AUDIO_TRACK, 1, int(m["frame_samples"]), 0, AUDIO_SAMPLE_FLAGS)
    return _init(AUDIO_TRACK, rate, b"soun", b"SoundHandler", 0x0100, 0, 0, smhd, mp4a, trex)


AC3_AUDIO_DISQUALIFIED = 1 | 2  # ac3info: not_dolby_audio, no_audio_config
AC3_FRAME_SAMPLES = 1536


def ac3_audio_codec(info):
    """The codec string of a Dolby audio track from its ``ac3info`` fields (``ops.ac3audio``,
    ``docs/AC3AUDIO.md``): ``ac-3`` or ``ec-3``.  ``None`` without a config."""
    if info["status"] & AC3_AUDIO_DISQUALIFIED or info["kind"] not in (1, 2):
        return None
    return "ac-3" if info["kind"] == 1 else "ec-3"


def ac3_specific_box(info) -> bytes:
    """``dac3`` (3 bytes: ``fscod:2 bsid:5 bsmod:3 acmod:3 lfeon:1 bit_rate_code:5 0:5``) or ``dec3``
    (5 bytes, one independent substream without dependents: ``data_rate:13 0:3 | fscod:2 bsid:5 0:1
    0:1 bsmod:3 acmod:3 lfeon:1 0:3 0:4 0:1``) of ETSI TS 102 366 Annex F."""
    fscod, bsid, bsmod, acmod, lfeon = (int(info[k]) for k in ("fscod", "bsid", "bsmod", "acmod", "lfeon"))
    if info["kind"] == 1:
        bits = (fscod << 22) | (bsid << 17) | (bsmod << 14) | (acmod << 11) | (lfeon << 10) | \
            (int(info["bit_rate_code"]) << 5)
        return _box(b"dac3", bits.to_bytes(3, "big"))
    head = (int(info["data_rate"]) & 0x1FFF) << 3
    sub = (fscod << 22) | (bsid << 17) | (bsmod << 12) | (acmod << 9) | (lfeon << 8)
    return _box(b"dec3", head.to_bytes(2, "big") + sub.to_bytes(3, "big"))


def ac3_audio_init(info):
    """The audio track's init segment for AC-3 / E-AC-3: ``ftyp`` + ``moov`` with one ``ac-3{ dac3 }``
    or ``ec-3{ dec3 }`` entry, track 2 in units of the sample rate, ``trex`` default duration 1536.
    ``None`` without a config."""
    codec = ac3_audio_codec(info)
    if codec is None:
        return None
    rate, channels = int(info["sample_rate"]), int(info["channels"])
    entry = _box(codec.encode(), struct.pack(">6xH8xHHHHI", 1, channels, 16, 0, 0, rate << 16) + ac3_specific_box(info))
    smhd = _full(b"smhd", 0, 0, bytes(4))
    trex = struct.pack(">IIIII", AUDIO_TRACK, 1, AC3_FRAME_SAMPLES, 0, AUDIO_SAMPLE_FLAGS)
    return _init(AUDIO_TRACK, rate, b"soun", b"SoundHandler", 0x0100, 0, 0, smhd, entry, trex)


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


def audio_moof(sequence_number: int, base_pts: int, sample_rate: int, asamples,
               frame_samples: int = AAC_FRAME_SAMPLES) -> bytes:
    """The audio fragment: track 2 in units of ``sample_rate``, ``tfdt`` = the rescaled
    ``base_pts``, ``frame_samples`` (1024 for AAC; an MPEG audio track passes its own) and sync
    flags per frame as ``tfhd`` defaults, a ``trun`` with one size per ``asamples`` row
    ``(offset, size)``."""
    a = np.asarray(asamples, dtype=np.int32).reshape(-1, 2)
    rows = np.empty((len(a), 1), dtype=">u4")
    rows[:, 0] = a[:, 1].astype(np.uint32)
    tfhd = _full(b"tfhd", 0, _TFHD_BASE_IS_MOOF | _TFHD_DEFAULT_DURATION | _TFHD_DEFAULT_FLAGS,
                 struct.pack(">III", AUDIO_TRACK, int(frame_samples), AUDIO_SAMPLE_FLAGS))
    return _moof(sequence_number, tfhd, audio_base(base_pts, sample_rate), _TRUN_DATA_OFFSET | _TRUN_SIZE, 0, rows)
