"""Hand-built inputs and the reference for the HEVC configuration tests (``test_hevcconfig.py`` on
the host implementation, ``test_hevcconfig_gpu.py`` on the kernel, ``test_hevcconfig_native.py``
on a sanitized build of the host parser).

* :class:`Bits` writes HEVC SPS NAL units from field values, most significant bit first, and
  :func:`escape` inserts emulation-prevention bytes as the standard prescribes.
* The reference (:func:`ref_parse_sps`, :func:`ref_segment`, :func:`parse_hvcc`) is written from
  the rules of ``docs/INITSEGMENT.md`` over a string of bits, with its own copy of every rule on
  purpose: it shares no code with ``shared/grammar.hpp``, ``runtime/hevc.cpp``,
  ``kernels/hevc_config.hip`` or ``player/fmp4.py``.
* :data:`LITERAL_SPS` is derived by hand (the derivation stands next to it); the writer has to
  reproduce it byte for byte.
* Inputs come from ``esindex_cases`` (a ``DemuxResult`` built by hand) plus ``esindex.index_batch``
  on the host; damaged rows are written into the index by hand.
"""
from __future__ import annotations

import itertools
import struct
from typing import List, Optional

import numpy as np
import torch

from codec_cases import Case, build  # noqa: F401  (the batch builder: no rule of either codec in it)
from esindex_cases import INFO, SC, adts_frame, background, seg

WORDS = 22
NAMES = ("status", "vps_nal", "vps_bytes", "sps_nal", "sps_bytes", "sps_rbsp_bytes", "pps_nal", "pps_bytes",
         "profile_space", "tier_flag", "profile_idc", "profile_compat", "constraint_hi", "constraint_lo", "level_idc",
         "num_temporal_layers", "temporal_id_nested", "chroma_format_idc", "bit_depth_luma", "bit_depth_chroma",
         "width", "height")
H = {name: i for i, name in enumerate(NAMES)}
PARSED = NAMES[8:]
NO_VPS, NO_SPS, NO_PPS, PS_OVERFLOW, BAD_SPS, NOT_HEVC = 1, 2, 4, 8, 16, 32
VPS_HDR, SPS_HDR, PPS_HDR = b"\x40\x01", b"\x42\x01", b"\x44\x01"  # nal_unit_type 32, 33, 34; layer 0; temporal id 0
VPS = VPS_HDR + bytes.fromhex("0c01ffff016000000300900000030000030078959809")
PPS = PPS_HDR + bytes.fromhex("c172b46240")
SLICE = b"\x02\x01\xd0"  # TRAIL_R
IDR = b"\x26\x01\xaf"    # IDR_W_RADL


# ---------------------------------------------------------------- the writer
class Bits:
    """An MSB-first bit writer."""

    def __init__(self) -> None:
        self.bits: List[int] = []

    def u(self, n: int, v: int) -> "Bits":
        assert 0 <= v < (1 << n)
        self.bits.extend((v >> (n - 1 - i)) & 1 for i in range(n))
        return self

    def ue(self, v: int) -> "Bits":
        z = (v + 1).bit_length() - 1
        return self.u(z, 0).u(z + 1, v + 1)

    def rbsp(self) -> bytes:
        """The bytes, with the stop bit and zero alignment of ``rbsp_trailing_bits``."""
        bits = self.bits + [1]
        bits += [0] * (-len(bits) % 8)
        return bytes(int("".join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))


def escape(rbsp: bytes) -> bytes:
    """Emulation prevention as the standard inserts it: 03 in front of a byte <= 3 behind two zeros."""
    out, zeros = bytearray(), 0
    for b in rbsp:
        if zeros >= 2 and b <= 3:
            out.append(3)
            zeros = 0
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def sps_rbsp(vps_id=0, L=0, nested=1, space=0, tier=0, profile=1, compat=0x60000000, constraint=0x900000000000,
             level=93, sub=None, sub_fill=0x5A, sps_id=0, chroma=1, separate=0, W=1920, H=1080, window=None,
             depth_luma=0, depth_chroma=0, tail=4) -> bytes:
    """The RBSP of an HEVC SPS from field values.  ``sub``: per sub-layer ``(profile_present,
    level_present)``, ``L`` pairs (default: none present); ``sub_fill``: the byte a present
    sub-layer field is filled with; ``window``: four ue (left, right, top, bottom) or ``None``;
    ``tail``: a ue written behind the bit depths (``log2_max_pic_order_cnt_lsb_minus4``), which no
    rule reads."""
    sub = [(0, 0)] * L if sub is None else list(sub)
    assert len(sub) == L
    w = Bits().u(4, vps_id).u(3, L).u(1, nested).u(2, space).u(1, tier).u(5, profile).u(32, compat)
    w.u(48, constraint).u(8, level)
    for p, l in sub:
        w.u(1, p).u(1, l)
    if L > 0:
        for _ in range(L, 8):
            w.u(2, 0)
    for p, l in sub:
        if p:
            for _ in range(11):
                w.u(8, sub_fill)
        if l:
            w.u(8, sub_fill)
    w.ue(sps_id).ue(chroma)
    if chroma == 3:
        w.u(1, separate)
    w.ue(W).ue(H).u(1, 1 if window else 0)
    if window:
        for c in window:
            w.ue(c)
    w.ue(depth_luma).ue(depth_chroma).ue(tail)
    return w.rbsp()


def sps_nal(cut: Optional[int] = None, header: bytes = SPS_HDR, **kw) -> bytes:
    """An SPS NAL unit from field values (:func:`sps_rbsp`); ``cut``: keep that many RBSP bytes only."""
    body = sps_rbsp(**kw)
    if cut is not None:
        body = body[:cut]
    return header + escape(body)


# Main profile, level 3.1 (level_idc 93), 1920 x 1088 coded, conformance window bottom offset 4 at
# 4:2:0 (4 x 2 luma rows): 1920 x 1080 shown.  By hand, most significant bit first:
#   0000 000 1                          sps_video_parameter_set_id 0, max_sub_layers_minus1 0, nesting 1  -> 01
#   00 0 00001                          profile_space 0, tier 0, profile_idc 1                            -> 01
#   compatibility flags 1 and 2 (Main, Main 10 decoders)                                                  -> 60 00 00 00
#   progressive_source, frame_only_constraint and 44 zero bits                                      -> 90 00 00 00 00 00
#   general_level_idc 93                                                                                  -> 5D
#   1                                   sps_seq_parameter_set_id ue(0)
#   010                                 chroma_format_idc ue(1)
#   0000000000 11110000001              pic_width ue(1920): 1921 in 11 bits behind 10 zeros
#   0000000000 10001000001              pic_height ue(1088): 1089
#   1  1 1 1 00101                      conformance_window, left / right / top ue(0), bottom ue(4)
#   1 1                                 bit_depth_luma_minus8, bit_depth_chroma_minus8 ue(0)
#   00101  1 0                          a ue(4) nothing reads, the stop bit, alignment
#   -> 1010 0000 | 0000 0011 | 1100 0000 | 1000 0000 | 0001 0001 | 0000 0111 | 1100 1011 | 1001 0110
#   -> A0 03 C0 80 11 07 CB 96
# Emulation prevention: 60 00 00 [03] 00 and 90 00 00 [03] 00 00 [03] 00.
LITERAL_KW = dict(W=1920, H=1088, window=(0, 0, 0, 4))
LITERAL_RBSP = bytes.fromhex("0101600000009000000000005da003c0801107cb96")
LITERAL_SPS = bytes.fromhex("4201" "0101" "6000000300" "9000000300000300" "5d" "a003c0801107cb96")
LITERAL_FIELDS = dict(profile_space=0, tier_flag=0, profile_idc=1, profile_compat=0x60000000, constraint_hi=0x9000,
                      constraint_lo=0, level_idc=93, num_temporal_layers=1, temporal_id_nested=1,
                      chroma_format_idc=1, bit_depth_luma=8, bit_depth_chroma=8, width=1920, height=1080)
LITERAL_CODEC = "hvc1.1.6.L93.90"
LITERAL_HVCC = (bytes.fromhex("01" "01" "60000000" "900000000000" "5d" "f000" "fc" "fd" "f8" "f8" "0000" "0f" "03")
                + b"\xa0\x00\x01" + struct.pack(">H", len(VPS)) + VPS
                + b"\xa1\x00\x01" + struct.pack(">H", len(LITERAL_SPS)) + LITERAL_SPS
                + b"\xa2\x00\x01" + struct.pack(">H", len(PPS)) + PPS)


# ---------------------------------------------------------------- the reference
class _Bad(Exception):
    pass


class _Reader:
    def __init__(self, rbsp: bytes) -> None:
        self.s = "".join(f"{b:08b}" for b in rbsp)
        self.p = 0

    def u(self, n: int) -> int:
        if self.p + n > len(self.s):
            raise _Bad("end of data")
        v = int(self.s[self.p:self.p + n], 2) if n else 0
        self.p += n
        return v

    def ue(self) -> int:
        z = 0
        while self.u(1) == 0:
            z += 1
            if z > 31:
                raise _Bad("more than 31 leading zeros")
        return (1 << z) - 1 + self.u(z)


def _i32(v: int) -> int:
    """A 32-bit pattern as the int32 the row holds."""
    return v - (1 << 32) if v & 0x80000000 else v


def ref_unescape(nal: bytes) -> bytes:
    """The RBSP of an HEVC NAL unit by the sequential rule: 03 behind two zeros is dropped and the
    count restarts.  The count runs over the raw bytes from the first header byte on; the two
    header bytes are not output."""
    out, zeros = bytearray(), 0
    for j, b in enumerate(nal):
        if zeros >= 2 and b == 3 and j >= 2:
            zeros = 0
            continue
        if j >= 2:
            out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def ref_parse_sps(nal: bytes) -> dict:
    """The parsed fields of one SPS NAL unit as a dict of the ``hinfo`` names involved, plus ``ok``."""
    return ref_parse_rbsp(ref_unescape(nal))


def ref_parse_rbsp(rbsp: bytes) -> dict:
    """The same, from the RBSP.  Any error: every field 0."""
    out = {k: 0 for k in PARSED}
    out["sps_rbsp_bytes"] = len(rbsp)
    out["ok"] = False
    r = _Reader(rbsp)
    try:
        r.u(4)
        L, nested = r.u(3), r.u(1)
        if L == 7:
            raise _Bad("sps_max_sub_layers_minus1")
        space, tier, profile = r.u(2), r.u(1), r.u(5)
        compat, chi, clo, level = r.u(32), r.u(16), r.u(32), r.u(8)
        present = [(r.u(1), r.u(1)) for _ in range(L)]
        if L > 0:
            for _ in range(8 - L):
                r.u(2)
        for p, l in present:
            if p:
                r.u(88)
            if l:
                r.u(8)
        if r.ue() > 15:
            raise _Bad("sps_seq_parameter_set_id")
        chroma = r.ue()
        if chroma > 3:
            raise _Bad("chroma_format_idc")
        if chroma == 3:
            r.u(1)
        W, Hh = r.ue(), r.ue()
        left = right = top = bottom = 0
        if r.u(1):
            left, right, top, bottom = r.ue(), r.ue(), r.ue(), r.ue()
        dl, dc = r.ue(), r.ue()
        if dl > 8 or dc > 8:
            raise _Bad("bit depth")
        cx = 2 if chroma in (1, 2) else 1
        cy = 2 if chroma == 1 else 1
        width, height = W - cx * (left + right), Hh - cy * (top + bottom)
        if not (1 <= width <= 65535 and 1 <= height <= 65535):
            raise _Bad("picture size")
    except _Bad:
        return out
    out.update(profile_space=space, tier_flag=tier, profile_idc=profile, profile_compat=_i32(compat),
               constraint_hi=chi, constraint_lo=_i32(clo), level_idc=level, num_temporal_layers=L + 1,
               temporal_id_nested=nested, chroma_format_idc=chroma, bit_depth_luma=8 + dl, bit_depth_chroma=8 + dc,
               width=width, height=height, ok=True)
    return out


def _clamp(v: int, lo: int, hi: int) -> int:
    return lo if v < lo else hi if v > hi else v


def ref_segment(es: bytes, cap: int, info, nal, sinfo, max_ps: int):
    """``(hinfo int32[22], hps uint8[3, max_ps])`` of one segment; ``es`` holds its ES region."""
    max_nal = nal.shape[0]
    row = np.zeros(WORDS, np.int32)
    hps = np.zeros((3, max_ps), np.uint8)
    row[H["vps_nal"]] = row[H["sps_nal"]] = row[H["pps_nal"]] = -1
    if int(info[INFO["video_type"]]) != 0x24:
        row[H["status"]] = NOT_HEVC
        return row, hps
    status = 0
    R = min(max(int(sinfo[1]), 0), max_nal)
    for which, (typ, miss, name) in enumerate(((32, NO_VPS, "vps"), (33, NO_SPS, "sps"), (34, NO_PPS, "pps"))):
        k = next((k for k in range(R) if int(nal[k, 2]) == typ and int(nal[k, 1]) > 0), None)
        if k is None:
            status |= miss
            continue
        off = _clamp(int(nal[k, 0]), 0, cap)
        ln = _clamp(int(nal[k, 1]), 0, cap - off)
        data = es[off:off + min(ln, max_ps)]
        hps[which, :len(data)] = np.frombuffer(data, np.uint8)
        row[H[name + "_nal"]], row[H[name + "_bytes"]] = k, ln
        if ln > max_ps:
            status |= PS_OVERFLOW
        elif which == 1:
            f = ref_parse_sps(data)
            if not f.pop("ok"):
                status |= BAD_SPS
            for key, v in f.items():
                row[H[key]] = v
    row[H["status"]] = status
    return row, hps


def ref_batch(res, ix, caps, max_ps: int):
    """The reference for every segment of a batch, stacked like ``HevcConfig``: ``(hinfo, hps)``."""
    es, info = res.es.cpu().numpy(), res.info.cpu().numpy()
    nal, sinfo = ix.nal.cpu().numpy(), ix.sinfo.cpu().numpy()
    rows = [ref_segment(es[int(o):int(o) + int(c)].tobytes(), int(c), info[i], nal[i], sinfo[i], max_ps)
            for i, (o, c) in enumerate(zip(res.es_offs, caps))]
    if not rows:
        return np.zeros((0, WORDS), np.int32), np.zeros((0, 3, max_ps), np.uint8)
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def assert_hevc_equal(cfg, ref) -> None:
    """Exact equality of both tensors."""
    for name, want in (("hinfo", ref[0]), ("hps", ref[1])):
        got = getattr(cfg, name).cpu().numpy()
        assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype)
        bad = np.argwhere(got != want)
        assert not len(bad), f"{name}: first difference at {bad[0].tolist()}: got {got[tuple(bad[0])]}, " \
                             f"want {want[tuple(bad[0])]}"


def ref_view(hinfo_row, hps_rows) -> dict:
    """One reference segment by name, plus ``vps`` / ``sps`` / ``pps`` as bytes."""
    out = {k: int(hinfo_row[i]) for i, k in enumerate(NAMES)}
    for r, name in enumerate(("vps", "sps", "pps")):
        out[name] = hps_rows[r, :min(max(out[name + "_bytes"], 0), hps_rows.shape[-1])].tobytes()
    return out


def parse_hvcc(body: bytes) -> dict:
    """An HEVCDecoderConfigurationRecord (ISO/IEC 14496-15 8.3.3.1.2) field by field; raises unless
    every reserved bit is set as prescribed and the arrays end with the record."""
    r = _Reader(body)
    out = {"version": r.u(8), "profile_space": r.u(2), "tier_flag": r.u(1), "profile_idc": r.u(5),
           "profile_compat": r.u(32), "constraint": r.u(48), "level_idc": r.u(8)}
    for name, reserved, bits in (("min_spatial_segmentation_idc", 4, 12), ("parallelism_type", 6, 2),
                                 ("chroma_format_idc", 6, 2), ("bit_depth_luma_minus8", 5, 3),
                                 ("bit_depth_chroma_minus8", 5, 3)):
        if r.u(reserved) != (1 << reserved) - 1:
            raise ValueError(f"reserved bits in front of {name}")
        out[name] = r.u(bits)
    out["avg_frame_rate"], out["constant_frame_rate"] = r.u(16), r.u(2)
    out["num_temporal_layers"], out["temporal_id_nested"], out["length_size_minus_one"] = r.u(3), r.u(1), r.u(2)
    arrays = []
    for _ in range(r.u(8)):
        complete, zero, typ, count = r.u(1), r.u(1), r.u(6), r.u(16)
        if zero:
            raise ValueError("reserved bit of an array")
        nals = []
        for _ in range(count):
            n = r.u(16)
            nals.append(bytes(r.u(8) for _ in range(n)))
        arrays.append((complete, typ, nals))
    if r.p != len(r.s):
        raise ValueError(f"{(len(r.s) - r.p) // 8} stray bytes behind the arrays")
    out["arrays"] = arrays
    return out


def ref_codec(f: dict) -> str:
    """The codec string of parsed fields by ISO/IEC 14496-15 Annex E."""
    compat = f["profile_compat"] & 0xFFFFFFFF
    rev = sum(1 << j for j in range(32) if compat & (0x80000000 >> j))  # flag j becomes bit j
    s = "hvc1." + ["", "A", "B", "C"][f["profile_space"]] + str(f["profile_idc"]) + "." + format(rev, "X")
    s += "." + ("H" if f["tier_flag"] else "L") + str(f["level_idc"])
    cons = list(struct.pack(">H", f["constraint_hi"] & 0xFFFF) + struct.pack(">I", f["constraint_lo"] & 0xFFFFFFFF))
    while cons and cons[-1] == 0:
        cons.pop()
    return s + "".join("." + format(b, "X") for b in cons)


# ---------------------------------------------------------------- hand-built batches
def annexb(*nals: bytes) -> bytes:
    return b"".join(SC + n for n in nals)


def vseg(*nals: bytes, audio: bytes = b"", apes=(), **kw) -> dict:
    """An HEVC segment whose video ES is the NAL units behind start codes, one PES at 0."""
    kw.setdefault("vtype", 0x24)
    return seg(annexb(*nals), audio, vpes=kw.pop("vpes", [0]), apes=apes, **kw)


SPS_A = sps_nal(**LITERAL_KW)
SPS_B = sps_nal(W=1280, H=720, level=120)
SUB_MIXES = [list(m) for L in range(7) for m in itertools.product(((0, 0), (0, 1), (1, 0), (1, 1)), repeat=L)]


def sublayer_nals(full: bool) -> list:
    """``L = 0..6`` with every mix of the sub-layer flags (``full``: all 5461; otherwise the
    uniform mixes and 100 drawn ones), each with its own picture size behind the sub-layers."""
    mixes = SUB_MIXES
    if not full:
        rng = np.random.default_rng(51)
        uniform = [m for m in SUB_MIXES if len(set(m)) <= 1]
        mixes = uniform + [SUB_MIXES[int(i)] for i in rng.integers(0, len(SUB_MIXES), 100)]
    return [sps_nal(L=len(m), sub=m, nested=i & 1, W=64 + i, H=48 + 2 * i, sub_fill=(0, 0x5A, 0xFF)[i % 3])
            for i, m in enumerate(mixes)]


def parse_nals() -> tuple:
    """``(ok, bad, truncated)`` SPS NAL units."""
    ok = [SPS_A, SPS_B]
    ok += [sps_nal(space=s, tier=t, profile=p, level=lv, compat=c, constraint=k, vps_id=v)
           for s, t, p, lv, c, k, v in ((0, 1, 2, 153, 0x20000000, 0xB00000000000, 3),
                                        (1, 0, 4, 255, 0xFFFFFFFF, 0xFFFFFFFFFFFF, 15),
                                        (2, 1, 31, 0, 0x80000001, 0x000000000001, 0),
                                        (3, 0, 0, 30, 0, 0, 0))]
    for chroma, separate in ((0, 0), (1, 0), (2, 0), (3, 0), (3, 1)):
        ok.append(sps_nal(chroma=chroma, separate=separate, W=640, H=368))
        for side in range(4):
            window = [0, 0, 0, 0]
            window[side] = side + 1
            ok.append(sps_nal(chroma=chroma, separate=separate, W=640, H=368, window=window))
    ok += [sps_nal(depth_luma=a, depth_chroma=b) for a, b in ((0, 0), (2, 2), (8, 8), (8, 0), (0, 8))]
    ok += [sps_nal(W=1, H=1), sps_nal(W=65535, H=65535), sps_nal(W=65537, H=9, window=(1, 0, 0, 0)), sps_nal(sps_id=15)]
    bad = [sps_nal(depth_luma=9), sps_nal(depth_chroma=9), sps_nal(W=65536), sps_nal(H=65536), sps_nal(W=0),
           sps_nal(H=0), sps_nal(W=8, window=(2, 2, 0, 0)), sps_nal(H=8, window=(0, 0, 1, 3)), sps_nal(sps_id=16),
           sps_nal(L=7, sub=[(0, 0)] * 7), sps_nal(chroma=4),
           SPS_HDR + escape(sps_rbsp()[:13] + bytes(5) + b"\x80"),  # sps_id: 40 zero bits
           SPS_HDR, SPS_HDR[:1]]                                    # the header alone, and half of it
    long = sps_nal(L=3, sub=[(1, 0), (0, 1), (1, 1)], window=(1, 2, 3, 4))
    truncated = [sps_nal(L=3, sub=[(1, 0), (0, 1), (1, 1)], window=(1, 2, 3, 4), cut=k)
                 for k in range(len(ref_unescape(long)))]
    truncated += [sps_nal(**LITERAL_KW, cut=k) for k in range(len(LITERAL_RBSP))]
    return ok, bad, truncated


def parse_cases() -> Case:
    ok, bad, truncated = parse_nals()
    return Case([vseg(VPS, n, PPS) for n in ok + bad + truncated + sublayer_nals(False)], max_nal=8)


def sublayer_cases() -> Case:
    """Every mix of the sub-layer flags, 5461 segments: for the host only."""
    return Case([vseg(VPS, n, PPS) for n in sublayer_nals(True)], max_nal=4)


def filler_sps(n: int, at=(), tail: bytes = b"") -> bytes:
    """A valid SPS padded with FF (or cut) to ``n`` bytes, ``00 00 03`` placed so each 03 is at an index of ``at``."""
    head = SPS_A
    b = bytearray(head + b"\xff" * (n - len(head)))
    for j in at:
        assert j - 2 >= len(head)
        b[j - 2:j + 1] = b"\x00\x00\x03"
    return bytes(b[:n]) + tail


def escape_positions(nal: bytes) -> list:
    return [j for j in range(2, len(nal)) if nal[j] == 3 and nal[j - 1] == 0 and nal[j - 2] == 0]


def unescape_cases() -> Case:
    body = sps_rbsp(nested=0, profile=0, compat=0x01000000, W=352, H=288)  # RBSP 00 00 01 ...: an escape at raw 4
    assert body[:3] == b"\x00\x00\x01"
    nals = [SPS_HDR + escape(body)]
    nals.append(b"\x42\x00" + b"\x00\x03" + escape(body[1:]))  # 03 at raw 3: its zeros are header byte 1 and raw 2
    nals.append(sps_nal(compat=0x00000001))   # 01 00 00 [03] 00 01: inside the compatibility flags
    nals.append(sps_nal(compat=0x60000000))   # 60 00 00 [03] 00
    nals += [SPS_A + b"\x00\x00\x03", SPS_A + b"\x00\x00\x03\x00\x00\x03", SPS_A + b"\x00\x00\x03\x03\xff",
             SPS_A + b"\x00\x00\x00\x03\xff"]
    nals += [filler_sps(300, at=[j]) for j in (62, 63, 64, 65, 127, 128, 254, 255, 256, 257)]
    nals.append(filler_sps(512, at=[511]))  # the last stored byte
    nals.append(filler_sps(300, at=[63, 66, 128, 131, 254, 257]))  # 00 00 03 00 00 03 across the edges
    # parsed fields behind escapes that move across 63 | 64: sub-layer fields of zeros are escaped
    # every third byte, and the flags in front of them shift where they start
    for i, mix in enumerate(SUB_MIXES[-40:] + SUB_MIXES[400:420]):
        nals.append(sps_nal(L=len(mix), sub=mix, sub_fill=0, W=1280 + i, H=720, window=(0, 0, 0, i)))
    return Case([vseg(VPS, n, PPS) for n in nals], max_nal=8, max_ps=512)


def _tiny(n: int) -> list:
    return [SLICE] * n


def search_cases() -> Case:
    def zero_len(res, ix):  # segment 10: rows 0..2 claim a VPS, an SPS and a PPS of no bytes in front of the real ones
        for k, t in enumerate((32, 33, 34)):
            ix.nal[10, k, 1:3] = torch.tensor([0, t], dtype=torch.int32)

    segs = [
        vseg(VPS, SPS_A, PPS, *_tiny(3)),                    # rows 0, 1, 2
        vseg(*_tiny(255), VPS, SPS_A, PPS),                  # row 255, the others in the next round
        vseg(*_tiny(254), VPS, SPS_A, PPS),                  # rows 254, 255 | 256
        vseg(*_tiny(256), VPS, SPS_A, PPS),                  # row 256
        vseg(*_tiny(511), VPS, SPS_A, PPS),                  # row 511, the others in the third round
        vseg(VPS, *_tiny(300), SPS_A, *_tiny(200), PPS),     # a round each
        vseg(PPS, *_tiny(70), SPS_A, IDR, VPS),              # the PPS first
        vseg(VPS, VPS + b"\x11", SPS_A, SPS_B, PPS, PPS + b"\x11"),  # the first of each wins
        vseg(*_tiny(520), VPS, SPS_A, PPS),                  # behind the recorded rows
        vseg(*_tiny(518), VPS, SPS_A, PPS),                  # the SPS in the last recorded row, the PPS behind
        vseg(SLICE, SLICE, SLICE, VPS, SPS_B, PPS),          # hand-edited empty rows in front
        vseg(VPS, SPS_A, PPS, IDR, vpes=[3 * 3 + len(VPS) + len(SPS_A) + len(PPS)]),  # all in front of the first PES
        vseg(SPS_A, PPS, IDR),                               # no VPS
        vseg(VPS, PPS, IDR),                                 # no SPS
        vseg(VPS, SPS_A, IDR),                               # no PPS
        vseg(IDR),                                           # none
    ]
    return Case(segs, max_nal=520, edit=zero_len)


def sized(hdr: bytes, n: int, rng) -> bytes:
    """A NAL unit of exactly ``n`` bytes behind ``hdr`` (cut to ``n`` where it is shorter), non-zero bytes."""
    return (hdr + bytes(background(rng, max(n - 2, 0))))[:n]


def copy_cases(max_ps: int = 256) -> Case:
    rng = np.random.default_rng(52)
    aud = adts_frame(bytes(background(rng, 40)))
    segs = []
    for lead in range(0, 20):  # the VPS starts at every residue mod 4 and mod 16, the others follow it
        segs.append(seg(bytes(background(rng, lead)) + annexb(VPS, filler_sps(45 + lead), PPS), vpes=[0], vtype=0x24))
    lengths = (1, 2, 15, 16, 17, max_ps, max_ps + 1)
    for n in lengths:
        segs.append(vseg(sized(VPS_HDR, n, rng), SPS_A, PPS))
        # (a cut SPS_A could end with a zero, which the index gives to the next start code)
        segs.append(vseg(VPS, filler_sps(n) if n >= len(SPS_A) else sized(SPS_HDR, n, rng), PPS))
        segs.append(vseg(VPS, SPS_A, sized(PPS_HDR, n, rng)))
    segs.append(vseg(VPS, PPS, filler_sps(77), audio=aud, apes=[0]))  # the SPS ends the video ES, audio right behind
    segs.append(vseg(filler_sps(60), VPS, PPS))  # hand-edited below: the row reaches past the cap
    segs.append(vseg(filler_sps(60), VPS, PPS))  # ... and starts past it
    last = annexb(VPS, PPS, filler_sps(max_ps))  # cut below: the SPS ends with the ES tensor, a multiple of 4 bytes
    segs.append(seg(bytes(background(rng, -len(last) % 4)) + last, vpes=[0], vtype=0x24))
    n = len(segs)

    def damage(res, ix):
        ix.nal[n - 3, 0, 1] = 5000
        ix.nal[n - 2, 0, 0] = 1 << 20
        ix.nal[n - 2, 1, 0] = -5
        # the last segment's ES ends with the ES tensor
        res.es = res.es[:int(res.es_offs[-1]) + len(segs[-1]["video"])].clone()

    return Case(segs, max_nal=8, max_ps=max_ps, edit=damage)


def other_cases() -> Case:
    """Segments of other codecs (H.264, MPEG-2, none) around one HEVC one."""
    return Case([vseg(VPS, SPS_A, PPS, vtype=0x1B), vseg(VPS, SPS_A, PPS, vtype=0x02), seg(b""),
                 vseg(VPS, SPS_A, PPS), seg(b"", vtype=0x24)], max_nal=8)


def fuzz_case(count: int = 256, seed: int = 53) -> Case:
    """Fuzzed bytes behind an SPS header (a third of them behind a valid head cut somewhere),
    fuzzed VPS / PPS, and a few fuzzed rows."""
    rng = np.random.default_rng(seed)
    segs = []
    for i in range(count):
        n = int(rng.integers(1, 61))
        body = rng.integers(0, 256, n, dtype=np.uint8)
        body[rng.random(n) < 0.3] = 0
        if i % 2 and n >= 3:
            j = int(rng.integers(0, n - 2))
            body[j:j + 3] = (0, 0, 3)
        blob = body.tobytes()
        if i % 3 == 0:
            blob = SPS_A[2:int(rng.integers(2, len(SPS_A)))] + blob
        elif i % 3 == 1:
            blob = bytes([int(rng.integers(0, 2)), int(rng.integers(0, 64))]) + blob  # a plausible first 16 bits
        segs.append(vseg(sized(VPS_HDR, int(rng.integers(2, 40)), rng), SPS_HDR + blob + b"\x80",
                         sized(PPS_HDR, int(rng.integers(2, 40)), rng), IDR))

    def rows(res, ix):
        r = np.random.default_rng(seed + 1)
        for i in range(0, count, 7):
            ix.nal[i, int(r.integers(0, 4)), int(r.integers(0, 3))] = int(r.integers(-50, 400))

    return Case(segs, max_nal=16, edit=rows)


def mixed_case() -> Case:
    """64 segments of every family in one batch (``max_nal`` 520, ``max_ps`` 256)."""
    fams = [parse_cases(), unescape_cases(), search_cases(), copy_cases(), other_cases(), fuzz_case(12)]
    segs = []
    for j in range(64):
        fam = fams[j % len(fams)]
        segs.append(fam.segs[(j // len(fams)) * 3 % (len(fam.segs) - 1)])
    return Case(segs, max_nal=520)


CASES = {
    "parse": parse_cases,
    "unescape": unescape_cases,
    "search": search_cases,
    "copy": copy_cases,
    "copy_16": lambda: copy_cases(16),
    "copy_1024": lambda: copy_cases(1024),
    "other": other_cases,
    "fuzz": fuzz_case,
    "mixed": mixed_case,
}


def all_sps_blobs() -> list:
    """Every hand-built SPS NAL unit, for the stand-alone parser test."""
    ok, bad, truncated = parse_nals()
    out = ok + bad + truncated + sublayer_nals(False)
    for name in ("unescape", "fuzz"):
        for s in CASES[name]().segs:
            out += [part for part in s["video"].split(SC) if part and (part[0] >> 1) & 0x3F == 33]
    return out
