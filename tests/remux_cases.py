"""Hand-built inputs and the reference for the remux tests (``test_remux.py`` on the host
implementation, ``test_remux_gpu.py`` on the kernels).

The reference is a sequential writer built from the rules of ``docs/REMUX.md`` with plain Python
loops over the index tables; it has its own copy of the keep rule and of the ADTS header rule
and shares no code with ``runtime/remux.cpp`` or ``kernels/remux.hip``.  A minimal ISO-BMFF box
parser for the ``moof`` tests lives here too.  Inputs come from ``esindex_cases`` (a
``DemuxResult`` built by hand from bytes, a PES table and an ``info`` row).
"""
from __future__ import annotations

import struct

import numpy as np
import torch

from esindex_cases import CASES as INDEX_CASES
from esindex_cases import INFO, SC, adts_frame, adts_segments, background, hand_batch, seg
from hlsjs_p2p_wrapper_amd.ops import esindex, tsdemux

TILE = 16384  # remux_tile_bytes(); the GPU tests pass the kernel's own value
FILL = 0x5A
SYNC, NON_SYNC = 0x02000000, 0x01010000
H264_KEPT = (1, 5, 6, 7, 8)
HEVC_DROPPED = (35, 36, 37, 38)


def out_bytes(cap: int, max_nal: int) -> int:
    return cap + max_nal + 32


# ---------------------------------------------------------------- the reference
def _fits32(v: int) -> bool:
    return -2 ** 31 <= v < 2 ** 31


def ref_segment(es: bytes, cap: int, info, pes, nal, au, aframes, sinfo, max_aframes: int):
    """``(rinfo, vsamples, asamples, region)`` of one segment; ``region`` is the whole output
    region, pre-filled with ``FILL``."""
    max_pes, max_nal = pes.shape[1], nal.shape[0]
    region = bytearray([FILL]) * out_bytes(cap, max_nal)
    vsamples = np.full((max_pes, 5), -1, np.int32)
    asamples = np.full((max_aframes, 2), -1, np.int32)
    vtype = int(info[INFO["video_type"]])
    supported = vtype in (0x1B, 0x24)
    status = 0 if supported else 8
    if int(sinfo[0]) & 1:
        status |= 1
    R = min(max(int(sinfo[1]), 0), max_nal) if supported else 0
    m = min(max(int(sinfo[2]), 0), max_pes) if supported else 0

    def clamp(v, lo, hi):
        return lo if v < lo else hi if v > hi else v

    # video payload
    payload = bytearray()
    sizes = [0] * m
    fit = True
    for k in range(R):
        s = clamp(int(nal[k, 0]), 0, cap)
        ln = clamp(int(nal[k, 1]), 0, cap - s)
        typ, unit = int(nal[k, 2]), int(nal[k, 3])
        kept = typ in H264_KEPT if vtype == 0x1B else (typ >= 0 and typ not in HEVC_DROPPED)
        if not (0 <= unit < m and ln > 0 and kept):
            continue
        if fit and len(payload) + 4 + ln > cap + max_nal:
            fit = False
            status |= 1
        if not fit:
            continue
        payload += struct.pack(">I", ln) + es[s:s + ln]
        sizes[unit] += 4 + ln
    P = len(payload)
    region[0:8] = struct.pack(">I4s", 8 + P, b"mdat")
    region[8:8 + P] = payload

    # video samples
    dts = [int(pes[0, a, 2]) for a in range(m)]
    pts = [int(pes[0, a, 1]) for a in range(m)]
    off = 0
    durations = []
    for a in range(m):
        if a + 1 < m:
            d = dts[a + 1] - dts[a]
            if d < 0 or not _fits32(d):
                d = 0
                status |= 4
        else:
            d = durations[a - 1] if m > 1 else 0
        durations.append(d)
        cts = pts[a] - dts[a]
        if not _fits32(cts):
            cts = 0
            status |= 4
        vsamples[a] = (off, sizes[a], d, cts, SYNC if int(au[a, 2]) & 1 else NON_SYNC)
        off += sizes[a]

    # audio
    A0 = (8 + P + 15) & ~15
    room = len(region) - (A0 + 8)
    ma = min(max(int(info[INFO["n_audio_pes"]]), 0), max_pes)
    body = bytearray()
    n_rec = n_frames = 0
    if int(info[INFO["audio_type"]]) == 0x0F:
        ao = clamp(int(info[INFO["audio_es_offset"]]), 0, cap)
        ab = clamp(int(info[INFO["audio_bytes"]]), 0, cap - ao)
        A = es[ao:ao + ab]
        is_open = True
        for k in range(ma):
            q = clamp(int(pes[1, k, 0]), 0, ab)
            end = clamp(int(pes[1, k + 1, 0]), q, ab) if k + 1 < ma else ab
            for _ in range(max(int(aframes[k, 0]), 0)):
                if q + 7 > end or A[q] != 0xFF or (A[q + 1] & 0xF6) != 0xF0:
                    break
                ln = ((A[q + 3] & 3) << 11) | (A[q + 4] << 3) | (A[q + 5] >> 5)
                header = 7 if A[q + 1] & 1 else 9
                if ln < header or q + ln > end:
                    break
                n_frames += 1
                size = ln - header
                if is_open and n_rec < max_aframes and len(body) + size <= room:
                    asamples[n_rec] = (len(body), size)
                    body += A[q + header:q + ln]
                    n_rec += 1
                else:
                    is_open = False
                    status |= 2
                q += ln
    Q = len(body)
    region[A0:A0 + 8] = struct.pack(">I4s", 8 + Q, b"mdat")
    region[A0 + 8:A0 + 8 + Q] = body
    rinfo = np.array([status, P, m, A0, Q, n_frames, dts[0] if m else -1, int(pes[1, 0, 1]) if ma else -1], np.int64)
    return rinfo, vsamples, asamples, bytes(region)


def ref_batch(res: tsdemux.DemuxResult, ix: esindex.EsIndex, caps, out_offs, out_size: int, max_aframes: int):
    """The reference for every segment, stacked like ``Remuxed``, and the whole ``out`` buffer
    as it must look when it was filled with ``FILL`` before the call."""
    es = res.es.cpu().numpy()
    info, pes = res.info.cpu().numpy(), res.pes.cpu().numpy()
    nal, au, af, sinfo = (t.cpu().numpy() for t in (ix.nal, ix.au, ix.aframes, ix.sinfo))
    B = len(caps)
    max_pes = pes.shape[2]
    out = np.full(out_size, FILL, np.uint8)
    rinfo = np.zeros((B, 8), np.int64)
    vs = np.zeros((B, max_pes, 5), np.int32)
    asamp = np.zeros((B, max_aframes, 2), np.int32)
    for i in range(B):
        o, c = int(res.es_offs[i]), int(caps[i])
        rinfo[i], vs[i], asamp[i], region = ref_segment(es[o:o + c].tobytes(), c, info[i], pes[i], nal[i], au[i],
                                                        af[i], sinfo[i], max_aframes)
        out[int(out_offs[i]):int(out_offs[i]) + len(region)] = np.frombuffer(region, np.uint8)
    return rinfo, vs, asamp, out


def assert_remux_equal(rx, ref) -> None:
    """Exact equality of the three tables and of every byte of ``out``."""
    for name, want in zip(("rinfo", "vsamples", "asamples", "out"), ref):
        got = getattr(rx, name).cpu().numpy()
        assert got.shape == want.shape and got.dtype == want.dtype, name
        bad = np.argwhere(got != want)
        assert not len(bad), f"{name}: first difference at {bad[0].tolist()}: got {got[tuple(bad[0])]}, " \
                             f"want {want[tuple(bad[0])]} ({len(bad)} differ)"


# ---------------------------------------------------------------- hand-built batches
def body(rng, header: int, n: int) -> bytes:
    """A NAL of ``n`` bytes: its header byte, then non-zero bytes."""
    return bytes([header]) + bytes(background(rng, n - 1))


def annexb(units, lead=b"", four=None):
    """``(video ES, PES offsets)`` of access units given as lists of NALs.  The first NAL of a
    unit gets the 4-byte start code unless ``four(k)`` decides per NAL ``k``."""
    v, offs, k = bytearray(lead), [], 0
    for unit in units:
        offs.append(len(v))
        for j, n in enumerate(unit):
            v += (b"\x00" if (four(k) if four else j == 0) else b"") + SC + n
            k += 1
    return bytes(v), offs


def stamp(s: dict, stamps) -> dict:
    """``(pts, dts)`` per video PES, written over ``hand_batch``'s by :func:`build`."""
    s["stamps"] = list(stamps)
    return s


def alignment_segments(seed: int = 21):
    """Six access units of kept NALs of lengths 1..40, behind a 4-byte and a 3-byte start code in
    turn.  A dropped AUD of 1..4 bytes in front of each unit shifts the source against the output,
    so that every output alignment meets every source alignment (the test counts them)."""
    rng = np.random.default_rng(seed)
    v, offs, k = bytearray(), [], 0
    for r in range(6):
        offs.append(len(v))
        v += SC + body(rng, 0x09, 1 + r % 4)
        for j in range(40):
            v += (b"\x00" if k % 2 == 0 else b"") + SC + body(rng, 0x41, 1 + j)
            k += 1
    return [seg(bytes(v), vpes=offs)]


def tile_edge_segments(T: int, seed: int = 22):
    """Per segment three kept NALs; the first body ends at region offset ``e`` and the second one
    begins at ``e + 4``, for ``e`` around the copy tile ``T``; the output reaches ``2 T + 40``
    (``P`` a multiple of 16) and in the last segment one byte more."""
    rng = np.random.default_rng(seed)
    out = []
    for e, extra in ((T - 5, 0), (T - 4, 0), (T - 3, 0), (T - 1, 0), (T, 0), (T + 1, 1)):
        l0, l1 = e - 12, 5
        l2 = 2 * T + 32 + extra - (4 + l0) - (4 + l1) - 4
        v, offs = annexb([[body(rng, 0x65, l0)], [body(rng, 0x41, l1), body(rng, 0x41, l2)]])
        out.append(seg(v, vpes=offs))
    return out


def dropping_segments(seed: int = 23):
    rng = np.random.default_rng(seed)
    aud = b"\x09\xf0"
    units = [
        [aud, body(rng, 0x67, 9), body(rng, 0x68, 4), body(rng, 0x65, 50)],
        [aud],                                                    # no kept NAL: a sample of size 0
        [aud, body(rng, 0x0C, 12), b"", body(rng, 0x41, 33)],      # filler data, a NAL of length 0
        [aud, body(rng, 0x0C, 3), body(rng, 0x0A, 2), b"\x41"],     # three dropped, then one kept byte
        [body(rng, 0x06, 7), body(rng, 0x41, 21)],
    ]
    lead = SC + body(rng, 0x41, 10) + SC + body(rng, 0x41, 6)      # in front of the first PES: no access unit
    v, offs = annexb(units, lead=lead)
    return [seg(v, vpes=offs)]


def codec_segments(seed: int = 24):
    """One byte string as H.264, as HEVC and as MPEG-2 video.  The header bytes are HEVC types
    19, 32, 33, 34, 35..38 and 1; read as H.264 they are types 6, 0, 2, 4, 6, 8, 10, 12 and 2."""
    rng = np.random.default_rng(seed)
    headers = [19 << 1, 32 << 1, 33 << 1, 34 << 1, 35 << 1, 36 << 1, 37 << 1, 38 << 1, 1 << 1]
    units = [[body(rng, h, 5 + 3 * j) for j, h in enumerate(headers[:5])],
             [body(rng, h, 8 + j) for j, h in enumerate(headers[5:])]]
    v, offs = annexb(units)
    audio = b"".join(adts_frame(bytes(background(rng, 40 + j))) for j in range(3))
    return [seg(v, audio, vpes=offs, apes=[0], vtype=t) for t in (0x1B, 0x24, 0x02)]


def audio_overflow_segments(seed: int = 25):
    rng = np.random.default_rng(seed)
    video = bytes(background(rng, 32))
    out = []
    for count in (3, 4, 5, 9):
        frames = [adts_frame(bytes(background(rng, 30 + 2 * j)), crc=bool(j & 1)) for j in range(count)]
        first = b"".join(frames[:2])
        out.append(seg(video, b"".join(frames), vpes=[0], apes=[0, len(first)]))
    return out


def timestamp_segments(seed: int = 26):
    rng = np.random.default_rng(seed)

    def video(n):
        return annexb([[body(rng, 0x65 if a == 0 else 0x41, 20 + a)] for a in range(n)])

    t0 = 900000
    v, offs = video(5)  # I P B B P in decode order: pts ahead of, behind and equal to dts
    reorder = stamp(seg(v, vpes=offs), [(t0 + 3600 * p, t0 + 3600 * d - 3600) for d, p in enumerate((0, 3, 1, 2, 4))])
    early = stamp(seg(v, vpes=offs), [(t0 + 3000 * a - 1500, t0 + 3000 * a) for a in range(5)])  # negative cts
    back = stamp(seg(v, vpes=offs), [(t0 + 3000 * a, t0 + 3000 * a) for a in (0, 1, 3, 2, 4)])  # a DTS step back
    wide = stamp(seg(v, vpes=offs), [(t0, t0), (2 ** 33 - 1, t0 + 1), (-1, 2 ** 32 + 5), (t0, 2 ** 32 + 6),
                                     (t0, 2 ** 32 + 7)])  # differences beyond int32
    v1, o1 = video(1)
    one = stamp(seg(v1, vpes=o1), [(t0 + 7, t0)])
    none = seg(bytes(background(rng, 24)), vpes=[])
    return [reorder, early, back, wide, one, none]


def tiny_segments(seed: int = 27):
    rng = np.random.default_rng(seed)
    audio = b"".join(adts_frame(bytes(background(rng, 25 + j))) for j in range(2))
    v, offs = annexb([[body(rng, 0x65, 17)]])
    return [seg(b"", audio, vpes=[], apes=[0]), seg(v, b"", vpes=offs, apes=[]), seg(b"", b""),
            seg(SC + b"\x65", vpes=[0]), seg(b"\x00", vpes=[0])]


def many_nal_segments(seed: int = 28):
    """4200 kept NALs of 1..3 bytes in 6 access units of 700: more than 4096 rows, so the copy
    kernel's wave lookup of a tile's rows runs three 64-way levels, and 25200 payload bytes, so the
    payload crosses a copy-tile edge."""
    rng = np.random.default_rng(seed)
    v, offs = annexb([[body(rng, 0x65 if a == 0 else 0x41, 1 + (700 * a + j) % 3) for j in range(700)]
                      for a in range(6)])
    return [seg(v, vpes=offs)]


def mixed_segments(T: int):
    return (dropping_segments() + codec_segments() + timestamp_segments() + adts_segments() + tiny_segments()
            + alignment_segments() + audio_overflow_segments() + tile_edge_segments(T)[-2:])


# name -> T -> (segments, max_pes, max_nal, max_aframes)
CASES = {
    "alignment": lambda T: (alignment_segments(), 8, 2048, 1024),
    "tile_edges": lambda T: (tile_edge_segments(T), 8, 2048, 1024),
    "dropping": lambda T: (dropping_segments(), 8, 2048, 1024),
    "codecs": lambda T: (codec_segments(), 8, 2048, 1024),
    "nal_overflow": lambda T: (INDEX_CASES["overflow"](T)[0], 8, 64, 1024),
    "audio_overflow": lambda T: (audio_overflow_segments(), 8, 2048, 4),
    "timestamps": lambda T: (timestamp_segments(), 8, 2048, 1024),
    "adts": lambda T: (adts_segments(), 4, 2048, 1024),
    "tiny": lambda T: (tiny_segments(), 8, 2048, 1024),
    "no_segments": lambda T: ([], 8, 2048, 1024),
    "mixed": lambda T: (mixed_segments(T), 8, 128, 4),
    "many_nals": lambda T: (many_nal_segments(), 8, 8192, 1024),
}


def build(segs, max_pes: int, max_nal: int, device="cpu"):
    """``(res, caps, ix)``: the hand-built batch with its stamps and its index on ``device``."""
    res, caps = hand_batch(segs, "cpu", max_pes)
    for i, s in enumerate(segs):
        for a, (pts, dts) in enumerate(s.get("stamps", ())[:max_pes]):
            res.pes[i, 0, a, 1], res.pes[i, 0, a, 2] = pts, dts
    dev = torch.device(device)
    res = tsdemux.DemuxResult(res.info.to(dev), res.pes.to(dev), res.es.to(dev), res.es_offs)
    return res, caps, esindex.index_batch(res, caps, max_nal=max_nal)


def run_case(name: str, T: int, device="cpu"):
    """``(segments, res, caps, ix, rx, ref)`` of one case: remuxed on ``device`` into a buffer
    filled with ``FILL``, next to the reference's tables and buffer."""
    from hlsjs_p2p_wrapper_amd.ops import remux

    segs, max_pes, max_nal, max_aframes = CASES[name](T)
    res, caps, ix = build(segs, max_pes, max_nal, device)
    offs, size = remux.layout_out(caps, max_nal)
    out = torch.full((size + 256,), FILL, dtype=torch.uint8, device=res.es.device)
    rx = remux.remux_batch(res, ix, caps, out, offs, max_aframes=max_aframes)
    return segs, res, caps, ix, rx, ref_batch(res, ix, caps, offs, size + 256, max_aframes)


# ---------------------------------------------------------------- ISO-BMFF
CONTAINERS = (b"moof", b"traf")


def parse_boxes(data: bytes, start: int = 0, end=None):
    """``[(type, start, size, children)]`` of the boxes that fill ``data[start:end]`` exactly."""
    end = len(data) if end is None else end
    out, p = [], start
    while p < end:
        assert p + 8 <= end, "a box header crosses the end of its parent"
        size, kind = struct.unpack_from(">I4s", data, p)
        assert size >= 8 and p + size <= end, f"box {kind!r} of {size} bytes does not fit its parent"
        out.append((kind, p, size, parse_boxes(data, p + 8, p + size) if kind in CONTAINERS else []))
        p += size
    assert p == end
    return out


def parse_moof(data: bytes) -> dict:
    """The fields of ``moof{ mfhd, traf{ tfhd, tfdt, trun } }``; asserts that shape."""
    top = parse_boxes(data)
    assert [b[0] for b in top] == [b"moof"] and top[0][2] == len(data)
    kids = top[0][3]
    assert [b[0] for b in kids] == [b"mfhd", b"traf"]
    assert [b[0] for b in kids[1][3]] == [b"tfhd", b"tfdt", b"trun"]
    out = {"size": len(data)}
    _, p, size, _ = kids[0]
    assert size == 16
    out["sequence_number"] = struct.unpack_from(">I", data, p + 12)[0]
    tfhd, tfdt, trun = kids[1][3]
    p = tfhd[1]
    flags = struct.unpack_from(">I", data, p + 8)[0] & 0xFFFFFF
    out["tfhd_flags"], out["track"] = flags, struct.unpack_from(">I", data, p + 12)[0]
    q = p + 16
    for bit, name, width in ((0x1, "base_data_offset", 8), (0x2, "sample_description_index", 4),
                             (0x8, "default_duration", 4), (0x10, "default_size", 4), (0x20, "default_flags", 4)):
        if flags & bit:
            out[name] = int.from_bytes(data[q:q + width], "big")
            q += width
    assert q == p + tfhd[2]
    p = tfdt[1]
    assert data[p + 8] == 1 and tfdt[2] == 20
    out["base"] = struct.unpack_from(">Q", data, p + 12)[0]
    p = trun[1]
    version, flags = data[p + 8], struct.unpack_from(">I", data, p + 8)[0] & 0xFFFFFF
    count = struct.unpack_from(">I", data, p + 12)[0]
    out["trun_version"], out["trun_flags"], out["count"] = version, flags, count
    q = p + 16
    if flags & 0x1:
        out["data_offset"] = struct.unpack_from(">i", data, q)[0]
        q += 4
    assert not flags & 0x4
    fields = [(0x100, "duration", ">I"), (0x200, "size", ">I"), (0x400, "flags", ">I"),
              (0x800, "cts", ">i" if version else ">I")]
    samples = []
    for _ in range(count):
        row = {}
        for bit, name, fmt in fields:
            if flags & bit:
                row[name] = struct.unpack_from(fmt, data, q)[0]
                q += 4
        samples.append(row)
    assert q == p + trun[2]
    out["samples"] = samples
    return out
