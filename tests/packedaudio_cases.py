"""Packed-audio segments for the demux tests: a builder of ID3v2 tags and ADTS frames, a sequential
reference with its own copy of every rule of ``docs/PACKEDAUDIO.md`` (nothing of the package's
parsing is imported), named batches, and an audio-only MPEG-TS of the same frames built with
``ts_builder`` for the equivalence tests.

Segments of a batch lie at 16-byte aligned offsets 16 to 31 bytes apart; the gaps hold whole
zero-payload ADTS frames, so a walk that read past a segment's end would count them."""
from __future__ import annotations

import numpy as np
import torch

import ts_builder as tb
from hlsjs_p2p_wrapper_amd.ops._native import runtime

NAMES = ("info", "pes", "nal", "au", "aframes", "sinfo", "painfo")
OWNER = b"com.apple.streaming.transportStreamTimestamp"
G = 4
GAP_FRAME = bytes([0xFF, 0xF1, 0x50, 0x80, 0x00, 0xFF, 0xFC])  # a whole 7-byte frame without payload
RATES = (96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350)
NO_TIMESTAMP, BAD_ID3, NO_FRAME, TRAILING, OVERFLOW, BAD_RATE = 1, 2, 4, 8, 16, 32


def tile_bytes() -> int:
    return int(runtime().ES_PACKED_TILE)


# ---------------------------------------------------------------- builder
def syncsafe(v: int) -> bytes:
    return bytes([(v >> 21) & 0x7F, (v >> 14) & 0x7F, (v >> 7) & 0x7F, v & 0x7F])


def id3_frame(fid: bytes, body: bytes, version: int = 4, size=None) -> bytes:
    n = len(body) if size is None else size
    return fid + (syncsafe(n) if version == 4 else n.to_bytes(4, "big")) + b"\x00\x00" + body


def priv(ts: int, version: int = 4, owner: bytes = OWNER, nul: bytes = b"\x00", upper: int = 0,
         tail: bytes = b"") -> bytes:
    """The PRIV frame that carries the transport stream timestamp; ``upper`` fills bits 33 to 63."""
    return id3_frame(b"PRIV", owner + nul + ((upper << 33) | ts).to_bytes(8, "big") + tail, version)


def text_frame(n: int, version: int = 4, fid: bytes = b"TIT2") -> bytes:
    return id3_frame(fid, b"\x03" + bytes((65 + i % 26) for i in range(n - 1)), version)


def tag(frames: bytes = b"", version: int = 4, flags: int = 0, footer: bool = False, pad: int = 0, size=None,
        revision: int = 0) -> bytes:
    body = frames + b"\x00" * pad
    flags |= 0x10 if footer else 0
    n = len(body) if size is None else size
    out = b"ID3" + bytes([version, revision, flags]) + syncsafe(n) + body
    if footer:
        out += b"3DI" + bytes([version, revision, flags]) + syncsafe(n)
    return out


def ts_tag(ts: int, version: int = 4, pad: int = 0, **kw) -> bytes:
    return tag(priv(ts, version), version, pad=pad, **kw)


def adts(payload: int, rate_index: int = 4, channels: int = 2, crc: bool = False, profile: int = 1, fill: int = 0x21,
         length=None, byte1=None) -> bytes:
    """One ADTS frame of ``payload`` bytes behind a 7-byte (9 with ``crc``) header."""
    hdr = 9 if crc else 7
    n = hdr + payload if length is None else length
    assert n < 8192
    b1 = (0xF0 if crc else 0xF1) if byte1 is None else byte1
    head = bytes([0xFF, b1, (profile << 6) | (rate_index << 2) | (channels >> 2), ((channels & 3) << 6) | (n >> 11),
                  (n >> 3) & 0xFF, ((n & 7) << 5) | 0x1F, 0xFC]) + (b"\xAB\xCD" if crc else b"")
    return head + bytes([fill]) * payload


def frames(count: int, seed: int = 0, lo: int = 0, hi: int = 400, **kw) -> list:
    rng = np.random.default_rng(seed)
    return [adts(int(rng.integers(lo, hi + 1)), crc=bool(rng.integers(0, 2)), fill=int(rng.integers(0, 256)), **kw)
            for _ in range(count)]


# ---------------------------------------------------------------- reference
def _frame_at(S, q, n):
    if q + 7 > n or S[q] != 0xFF or (S[q + 1] & 0xF6) != 0xF0:
        return 0
    length = ((S[q + 3] & 3) << 11) | (S[q + 4] << 3) | (S[q + 5] >> 5)
    hdr = 7 if S[q + 1] & 1 else 9
    return 0 if length < hdr or q + length > n else length


def _timestamp(S, t, size):
    version, flags = S[t + 3], S[t + 5]
    if version not in (3, 4) or flags & 0xC0:
        return -1
    f, end = t + 10, t + 10 + size
    for _ in range(32):
        if f + 10 > end or S[f] == 0:
            break
        raw = S[f + 4:f + 8]
        if version == 4:
            if any(b >= 0x80 for b in raw):
                break
            fsize = (raw[0] << 21) | (raw[1] << 14) | (raw[2] << 7) | raw[3]
        else:
            fsize = int.from_bytes(raw, "big")
        if fsize > end - (f + 10):
            break
        body = S[f + 10:f + 10 + fsize]
        if S[f:f + 4] == b"PRIV" and fsize == 53 and body[:45] == OWNER + b"\x00":
            return int.from_bytes(body[45:53], "big") & ((1 << 33) - 1)
        f += 10 + fsize
    return -1


def ref_segment(S: bytes, max_pes: int) -> dict:
    S = bytes(S)
    n = len(S)
    info = np.zeros(24, np.int64)
    pes = np.full((3, max_pes, 3), -1, np.int64)
    nal, au = np.full((1, 4), -1, np.int32), np.full((max_pes, 4), -1, np.int32)
    aframes = np.full((max_pes, 2), -1, np.int32)
    sinfo, painfo = np.zeros(8, np.int64), np.zeros(8, np.int64)
    t, ts, n_tags, status = 0, -1, 0, 0
    for _ in range(8):
        if t + 10 > n or S[t:t + 3] != b"ID3" or S[t + 3] == 0xFF or S[t + 4] == 0xFF or max(S[t + 6:t + 10]) >= 0x80:
            break
        size = (S[t + 6] << 21) | (S[t + 7] << 14) | (S[t + 8] << 7) | S[t + 9]
        total = 10 + size + (10 if S[t + 5] & 0x10 else 0)
        if t + total > n:
            status |= BAD_ID3
            break
        if ts < 0:
            ts = _timestamp(S, t, size)
        t += total
        n_tags += 1
    if ts < 0:
        status |= NO_TIMESTAMP
    T = t
    starts, q, rate, chans = [], T, 0, 0
    if not status & BAD_ID3:
        while True:
            length = _frame_at(S, q, n)
            if not length:
                break
            if not starts:
                idx = (S[q + 2] >> 2) & 15
                rate = RATES[idx] if idx < 13 else 0
                chans = ((S[q + 2] & 1) << 2) | (S[q + 3] >> 6)
            starts.append(q)
            q += length
        if not starts:
            status |= NO_FRAME
        elif q != n:
            status |= TRAILING
        if starts and rate == 0:
            status |= BAD_RATE
    n_frames = len(starts)
    groups = (n_frames + G - 1) // G
    if groups > max_pes:
        status |= OVERFLOW
    rec = min(groups, max_pes)
    stamp = lambda k: ts + (k * G * 1024 * 90000 + rate // 2) // rate if rate else ts  # noqa: E731
    for k in range(rec):
        first = starts[G * k]
        end = starts[G * (k + 1)] if G * (k + 1) < n_frames else q
        pes[1, k] = (first - T, stamp(k), stamp(k))
        aframes[k] = (min(G, n_frames - G * k), end - first)
    if T > 0:
        pes[2, 0] = (0, ts, ts)
    info[0] = 8 if groups > max_pes else 0
    info[1:5] = -1
    info[7], info[8], info[10], info[11], info[13], info[14] = n - T, T, groups, int(T > 0), 0x0F, n
    info[16:22] = -1
    if rec:
        info[17], info[20] = stamp(0), stamp(rec - 1)
    if T > 0:
        info[18] = info[21] = ts
    info[22] = T
    sinfo[:] = (2 if status & TRAILING else 0, 0, 0, 0, -1, n_frames, rate, chans)
    painfo[:] = (status, T, n_tags, ts, n_frames, q, rate, chans)
    return dict(info=info, pes=pes, nal=nal, au=au, aframes=aframes, sinfo=sinfo, painfo=painfo)


def ref_batch(buf, offs, lens, max_pes: int) -> dict:
    raw = buf.cpu().numpy().tobytes() if isinstance(buf, torch.Tensor) else bytes(buf)
    rows = [ref_segment(raw[o:o + max(n, 0)], max_pes) for o, n in zip(offs, lens)]
    return {k: np.stack([r[k] for r in rows]) for k in NAMES}


def assert_equal(got, ref) -> None:
    for k in NAMES:
        g = got[k] if isinstance(got, dict) else getattr(got, k)
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        assert g.shape == ref[k].shape and g.dtype == ref[k].dtype, (k, g.shape, g.dtype)
        bad = np.argwhere(g != ref[k])
        assert not len(bad), (k, bad[:4].tolist(), g[tuple(bad[0])], ref[k][tuple(bad[0])])


# ---------------------------------------------------------------- batches
def layout(segments, dev="cpu"):
    """``(buf, offs, lens)``: the segments 16 to 31 bytes apart at aligned offsets, frames in the gaps."""
    offs, p = [], 0
    for s in segments:
        offs.append(p)
        p = (p + len(s) + 16 + 15) & ~15
    raw = bytearray(p + 16)
    for i, (o, s) in enumerate(zip(offs, segments)):
        raw[o:o + len(s)] = s
        nxt = offs[i + 1] if i + 1 < len(offs) else len(raw)
        gap = nxt - (o + len(s))  # a whole frame starts right behind the segment
        raw[o + len(s):nxt] = (GAP_FRAME * (gap // 7 + 1))[:gap]
    return torch.from_numpy(np.frombuffer(bytes(raw), np.uint8).copy()).to(dev), offs, [len(s) for s in segments]


TS0 = 900_000


def seg(n_frames: int, ts: int = TS0, seed: int = 0, version: int = 4, pad: int = 0, **kw) -> bytes:
    return ts_tag(ts, version, pad) + b"".join(frames(n_frames, seed, **kw))


def case_counts():
    return [seg(c, seed=c) for c in (0, 1, 3, 4, 5)] + [b"".join(frames(c, 7)) for c in (0, 5)], 8


def case_overflow():
    return [seg(16, seed=1), seg(17, seed=2), seg(21, seed=3), seg(3, seed=4)], 4


def case_align():
    base = len(ts_tag(TS0))
    return [seg(6, seed=r, pad=(r - base) % 16) for r in range(16)], 8


def _until(target: int, start: int, seed: int, rate_index: int = 3) -> list:
    """Frames of at most 8191 bytes that fill exactly [start, target)."""
    rng, out, p = np.random.default_rng(seed), [], start
    while p < target:
        left = target - p
        take = left if left <= 8191 else int(rng.integers(4000, 8000))
        if 0 < left - take < 9:
            take -= 16
        crc = take >= 9 and bool(rng.integers(0, 2))
        out.append(adts(take - (9 if crc else 7), rate_index=rate_index, crc=crc, fill=int(rng.integers(0, 256))))
        p += take
    assert p == target
    return out


def case_tiles():
    """A frame that starts ``c`` bytes in front of the first tile's end for c = 0 .. 7 (0: exactly
    at the end; 1 .. 6: its header straddles it; 7: the header ends with the tile), and a segment
    of more than two tiles."""
    tile, head = tile_bytes(), ts_tag(TS0, pad=3)
    T = len(head)
    end0 = (T & ~15) + tile
    segs = []
    for c in range(8):
        body = _until(end0 - c, T, c) + frames(5, c, lo=20, hi=300, rate_index=3)
        segs.append(head + b"".join(body))
    long = _until(T + 2 * tile + 5000, T, 11) + frames(3, 12, rate_index=3)
    segs.append(head + b"".join(long))
    return segs, 16


def case_tags():
    f = b"".join(frames(5, 3))
    near = OWNER[:-1] + b"q"
    big = (1 << 32) + 12345
    return [
        f,                                                            # no tag
        tag(text_frame(40)) + f,                                      # a tag without the PRIV
        tag(text_frame(40) + priv(TS0)) + f,                          # the PRIV as second frame
        tag(text_frame(200, 3) + priv(TS0 + 1, 3), 3) + f,            # version 3, a plain size of 200 in front
        tag(text_frame(200) + priv(TS0 + 2)) + f,                     # version 4, the same syncsafe
        tag(text_frame(30)) + ts_tag(TS0 + 3) + f,                    # the timestamp in the second of two tags
        ts_tag(TS0 + 4) + ts_tag(TS0 + 5) + f,                        # the first one wins
        ts_tag(TS0, footer=True) + f,                                 # a footer
        b"".join(tag(pad=i) for i in range(8)) + ts_tag(TS0) + f,     # a ninth tag: no frame at T
        b"".join(tag(pad=i) for i in range(7)) + ts_tag(TS0) + f,     # the eighth holds the stamp
        ts_tag(TS0, size=len(priv(TS0)) + len(f) + 1) + f,            # a tag whose size passes the end
        ts_tag(TS0) + tag(size=4000) + f,                             # ... the second one does
        tag(priv(TS0, owner=near)) + f,                               # one character off
        tag(priv(TS0, nul=b"\x01")) + f,                              # no NUL
        tag(priv(TS0, owner=OWNER[:-1])) + f,                         # fsize 52
        tag(priv(TS0, tail=b"\x00")) + f,                             # fsize 54
        tag(id3_frame(b"PRIW", priv(TS0)[10:])) + f,                  # another frame id
        ts_tag(big) + f,                                              # a stamp >= 2^32
        tag(priv(TS0, upper=0x5A5A5A5A & 0x7FFFFFFF)) + f,            # garbage in the upper 31 bits
        tag(priv((1 << 33) - 1, upper=0x7FFFFFFF)) + f,               # all ones
        ts_tag(TS0, version=2) + f,                                   # version 2: the frames are not read
        ts_tag(TS0, flags=0x80) + f,                                  # unsynchronisation: not read
        ts_tag(TS0, flags=0x40) + f,                                  # extended header: not read
        b"ID3\xff\x00\x00" + syncsafe(0) + f,                         # version 0xFF: no tag
        b"ID3\x04\xff\x00" + syncsafe(0) + f,                         # revision 0xFF: no tag
        b"ID3\x04\x00\x00\x00\x00\x80\x00" + f,                       # a size byte >= 0x80: no tag
        tag(id3_frame(b"TIT2", b"x" * 9, size=4000) + priv(TS0)) + f,  # a frame size beyond the tag ends the walk
        tag(b"TIT2\x00\x00\x80\x05\x00\x00" + b"y" * 5 + priv(TS0)) + f,  # version 4: a size byte >= 0x80 ends it
        tag(b"".join(text_frame(4) for _ in range(32)) + priv(TS0)) + f,  # the PRIV as 33rd frame
        tag(b"".join(text_frame(4) for _ in range(31)) + priv(TS0)) + f,  # ... as 32nd
        ts_tag(TS0)[:9],                                              # nine bytes
        ts_tag(TS0),                                                  # a tag and nothing else
        b"",
    ], 8


def case_breaks():
    f = frames(6, 5)
    head = ts_tag(TS0)
    cut = b"".join(f)
    return [
        head + cut[:-3],                                              # a truncated last frame
        head + cut[:len(f[0]) + 6],                                   # ... truncated inside its header
        head + b"".join(f[:3]) + adts(0, length=5) + b"".join(f[3:]),  # len < header
        head + b"".join(f[:3]) + adts(0, crc=True, length=8) + b"".join(f[3:]),  # ... of a 9-byte header
        head + b"".join(f[:2]) + adts(30, byte1=0xF3) + b"".join(f[2:]),  # wrong layer bits
        head + b"".join(f[:2]) + adts(30, byte1=0xE1) + b"".join(f[2:]),  # a short sync word
        head + b"".join(f[:4]) + b"\x00\x17garbage" + b"".join(f[4:]),  # garbage between frames
        head + b"\x00" + cut,                                         # ... in front of the first
        head + b"".join(frames(5, 6, rate_index=13)),                 # a reserved rate
        head + b"".join(frames(5, 6, rate_index=15, channels=7)),
        head + b"".join(frames(5, 8, rate_index=0, channels=0)) + b"\xff",
        head + adts(8191 - 7) + adts(8191 - 9, crc=True) + adts(0) + adts(0, crc=True),  # the extremes
    ], 8


def case_mixed(count: int = 70):
    rng, segs = np.random.default_rng(21), []
    for i in range(count):
        c = int(rng.integers(0, 40))
        s = seg(c, ts=TS0 + 1000 * i, seed=100 + i, version=3 + i % 2, pad=int(rng.integers(0, 30)),
                rate_index=int(rng.integers(0, 13)), channels=int(rng.integers(1, 8)))
        if i % 9 == 4:
            s = s[:len(s) - int(rng.integers(1, 12))] if c else s
        segs.append(s)
    return segs, 8


def case_one():
    return [seg(9, seed=2)], 8


def case_random():
    rng, segs = np.random.default_rng(5), []
    for i in range(48):
        n = int(rng.integers(0, 600))
        s = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        if i % 3 == 1 and n >= 10:
            s[:10] = b"ID3" + bytes([3 + i % 2, 0, int(rng.integers(0, 256))]) + syncsafe(int(rng.integers(0, n)))
        if i % 3 == 2 and n >= 7:
            s[:7] = adts(0, length=int(rng.integers(0, 64)))
        segs.append(bytes(s))
    return segs, 8


def case_mutated():
    rng, segs = np.random.default_rng(6), []
    base = tag(text_frame(20) + priv(TS0)) + b"".join(frames(12, 9, hi=60))
    for i in range(64):
        s = bytearray(base)
        for _ in range(1 + i % 4):
            p = int(rng.integers(0, len(s) if i % 2 else min(len(s), 110)))
            s[p] = int(rng.integers(0, 256)) if i % 3 else s[p] ^ (1 << int(rng.integers(0, 8)))
        segs.append(bytes(s))
    return segs, 8


CASES = {"counts": case_counts, "overflow": case_overflow, "align": case_align, "tiles": case_tiles, "tags": case_tags,
         "breaks": case_breaks, "mixed": case_mixed, "one": case_one, "random": case_random, "mutated": case_mutated}


def batch(name: str, dev="cpu"):
    """``(buf, offs, lens, max_pes)`` of a named batch."""
    segs, max_pes = CASES[name]()
    buf, offs, lens = layout(segs, dev)
    return buf, offs, lens, max_pes


# ---------------------------------------------------------------- the same frames as an audio-only MPEG-TS
def audio_ts(frame_list, ts: int, rate: int) -> bytes:
    """An MPEG-TS with one ADTS audio stream: four frames per PES at the packed path's group stamps."""
    APID, PMTPID = 0x101, 0x1000
    m = tb._Muxer()
    m.psi(0, tb._section(0x00, 1, bytes([0, 1, 0xE0 | (PMTPID >> 8), PMTPID & 0xFF])))
    streams = bytes([0x0F, 0xE0 | (APID >> 8), APID & 0xFF, 0xF0, 0x00])
    m.psi(PMTPID, tb._section(0x02, 1, bytes([0xE0 | (APID >> 8), APID & 0xFF, 0xF0, 0x00]) + streams))
    for k in range(0, len(frame_list), G):
        stamp = ts + ((k // G) * G * 1024 * 90000 + rate // 2) // rate
        m.pes(APID, tb._pes(0xC0, b"".join(frame_list[k:k + G]), stamp, stamp))  # PTS and an equal DTS
    return b"".join(m.packets)
