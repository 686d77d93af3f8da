"""Hand-built inputs and the reference for the sample-index tests (``test_esindex.py`` on the
host implementation, ``test_esindex_gpu.py`` on the kernels).

The reference is a sequential scanner written from the rules of ``docs/ESINDEX.md`` with
``bytes.find`` and a plain ADTS loop; it shares no code with ``runtime/es.cpp`` or
``kernels/es_index.hip``.  Inputs are ``DemuxResult`` objects built by hand from a byte buffer,
a PES table and an ``info`` row: no TS is needed to place a start code on a tile edge.
"""
from __future__ import annotations

import numpy as np
import torch

from hlsjs_p2p_wrapper_amd.ops import tsdemux

TILE = 16384  # es_index_tile_bytes(); the GPU tests pass the kernel's own value
INFO = tsdemux.INFO
ADTS_RATES = (96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350)
SC = b"\x00\x00\x01"


# ---------------------------------------------------------------- the reference
def ref_segment(es: bytes, info, pes, max_nal: int):
    """``(nal, au, aframes, sinfo)`` of one segment: ``es`` holds the segment's ES region from
    its start, ``info`` its demux info row, ``pes`` its PES table ``[3, max_pes, 3]``."""
    max_pes = pes.shape[1]
    nal = np.full((max_nal, 4), -1, np.int32)
    au = np.full((max_pes, 4), -1, np.int32)
    aframes = np.full((max_pes, 2), -1, np.int32)
    status = 0
    vtype = int(info[INFO["video_type"]])
    starts = []
    n = m = 0
    if vtype in (0x1B, 0x24):
        n = int(info[INFO["video_bytes"]])
        m = min(int(info[INFO["n_video_pes"]]), max_pes)
        V = es[:n]
        i = 0
        while True:
            p = V.find(SC, i)
            if p < 0 or p + 3 >= n:  # the NAL header byte must exist inside the video ES
                break
            starts.append(p)
            i = p + 3
    else:
        status |= 4
        V = b""
    if len(starts) > max_nal:
        status |= 1
    z = [1 if p > 0 and V[p - 1] == 0 else 0 for p in starts]
    offs = [int(pes[0, a, 0]) for a in range(m)]
    for k, p in enumerate(starts[:max_nal]):
        s = p + 3
        e = max(s, starts[k + 1] - z[k + 1]) if k + 1 < len(starts) else n
        if e == s:
            typ = -1
        elif vtype == 0x1B:
            typ = V[s] & 0x1f
        else:
            typ = (V[s] >> 1) & 0x3f
        unit = max([a for a in range(m) if offs[a] <= s], default=-1)
        nal[k] = (s, e - s, typ, unit)
    key = {5} if vtype == 0x1B else set(range(16, 22))
    sps, pps, aud = (7, 8, 9) if vtype == 0x1B else (33, 34, 35)
    n_key, first_key = 0, -1
    for a in range(m):
        mine = [k for k in range(min(len(starts), max_nal)) if nal[k, 3] == a]
        flags = 0
        for k in mine:
            t = int(nal[k, 2])
            flags |= (1 if t in key else 0) | (2 if t == sps else 0) | (4 if t == pps else 0) | (8 if t == aud else 0)
        size = (offs[a + 1] if a + 1 < m else n) - offs[a]
        au[a] = (mine[0] if mine else -1, len(mine), flags, size)
        if flags & 1:
            n_key += 1
            first_key = a if first_key < 0 else first_key
    n_frames = rate = chans = 0
    if int(info[INFO["audio_type"]]) == 0x0F:
        ao, ab = int(info[INFO["audio_es_offset"]]), int(info[INFO["audio_bytes"]])
        A = es[ao:ao + ab]
        ma = min(int(info[INFO["n_audio_pes"]]), max_pes)
        for k in range(ma):
            q = start = int(pes[1, k, 0])
            end = int(pes[1, k + 1, 0]) if k + 1 < ma else ab
            frames = 0
            while q != end:
                if q + 7 > end or A[q] != 0xFF or (A[q + 1] & 0xF6) != 0xF0:
                    status |= 2
                    break
                ln = ((A[q + 3] & 3) << 11) | (A[q + 4] << 3) | (A[q + 5] >> 5)
                header = 7 if A[q + 1] & 1 else 9
                if ln < header or q + ln > end:
                    status |= 2
                    break
                if k == 0 and frames == 0:
                    idx = (A[q + 2] >> 2) & 15
                    rate = ADTS_RATES[idx] if idx < 13 else 0
                    chans = ((A[q + 2] & 1) << 2) | (A[q + 3] >> 6)
                frames += 1
                q += ln
            aframes[k] = (frames, q - start)
            n_frames += frames
    sinfo = np.array([status, len(starts), m, n_key, first_key, n_frames, rate, chans], np.int64)
    return nal, au, aframes, sinfo


def ref_batch(res: tsdemux.DemuxResult, caps, max_nal: int):
    """The reference for every segment of a demuxed batch, stacked like ``EsIndex``."""
    es = res.es.cpu().numpy()
    info = res.info.cpu().numpy()
    pes = res.pes.cpu().numpy()
    out = [ref_segment(es[int(o):int(o) + int(c)].tobytes(), info[i], pes[i], max_nal)
           for i, (o, c) in enumerate(zip(res.es_offs, caps))]
    return tuple(np.stack([seg[j] for seg in out]) for j in range(4))


def assert_index_equal(ix, ref) -> None:
    """Exact equality of the four tensors."""
    for name, want in zip(("sinfo", "nal", "au", "aframes"), (ref[3], ref[0], ref[1], ref[2])):
        got = getattr(ix, name).cpu().numpy()
        assert got.shape == want.shape and got.dtype == want.dtype, name
        bad = np.argwhere(got != want)
        assert not len(bad), f"{name}: first difference at {bad[0].tolist()}: got {got[tuple(bad[0])]}, " \
                             f"want {want[tuple(bad[0])]}"


# ---------------------------------------------------------------- hand-built batches
def background(rng, n: int) -> bytearray:
    """``n`` non-zero bytes: no start code can form outside the planted ones."""
    return bytearray(rng.integers(1, 256, n, dtype=np.uint8).tobytes())


def seg(video=b"", audio=b"", vpes=(), apes=(), vtype=0x1B, atype=0x0F, n_vpes=None, n_apes=None) -> dict:
    return {"video": bytes(video), "audio": bytes(audio), "vpes": list(vpes), "apes": list(apes), "vtype": vtype,
            "atype": atype, "n_vpes": len(vpes) if n_vpes is None else n_vpes,
            "n_apes": len(apes) if n_apes is None else n_apes}


def hand_batch(segs, device="cpu", max_pes: int = 8):
    """A ``DemuxResult`` as the demux would leave it (``[video | audio]`` per segment at
    256-byte aligned offsets) and the caps to index it with."""
    B = len(segs)
    es_offs, caps, pos = [], [], 0
    for s in segs:
        es_offs.append(pos)
        caps.append(len(s["video"]) + len(s["audio"]))
        pos += (caps[-1] + 255) // 256 * 256
    es = np.full(pos + 256, 0xAA, np.uint8)
    info = np.zeros((B, tsdemux.INFO_WORDS), np.int64)
    pes = np.full((B, 3, max_pes, 3), -1, np.int64)
    for i, s in enumerate(segs):
        both = s["video"] + s["audio"]
        es[es_offs[i]:es_offs[i] + len(both)] = np.frombuffer(both, np.uint8)
        row = info[i]
        row[INFO["video_bytes"]], row[INFO["audio_bytes"]] = len(s["video"]), len(s["audio"])
        row[INFO["n_video_pes"]], row[INFO["n_audio_pes"]] = s["n_vpes"], s["n_apes"]
        row[INFO["video_type"]], row[INFO["audio_type"]] = s["vtype"], s["atype"]
        row[INFO["audio_es_offset"]] = len(s["video"])
        row[INFO["id3_es_offset"]] = len(both)
        row[INFO["payload_bytes"]] = len(both)
        for c, offs in ((0, s["vpes"]), (1, s["apes"])):
            for k, o in enumerate(offs[:max_pes]):
                pes[i, c, k] = (o, 90000 + 3600 * k, 90000 + 3600 * k)
    dev = torch.device(device)
    res = tsdemux.DemuxResult(torch.from_numpy(info).to(dev), torch.from_numpy(pes).to(dev),
                              torch.from_numpy(es).to(dev), np.asarray(es_offs, np.int64))
    return res, caps


def plant(v: bytearray, p: int, four: bool = False) -> None:
    """A start code at ``p`` (``four``: the 4-byte form, a zero at ``p - 1`` as well)."""
    v[p:p + 3] = SC
    if four:
        v[p - 1] = 0


def boundary_segments(T: int, seed: int = 5):
    """Video ES of ``2 T + 40`` bytes with start codes on every edge the kernel has: the lane's
    16 bytes, the wave's 1 KiB, the iteration's 4 KiB, the tile and the end of the ES.
    Positions that would overlap go to different segments; tiny and empty segments sit between."""
    rng = np.random.default_rng(seed)
    n = 2 * T + 40
    want = sorted({0, 1, 13, 14, 15, 16, *range(1021, 1025), *range(4093, 4097), T - 3, T - 2, T - 1, T, 2 * T - 2,
                   n - 4, n - 3})
    groups = []
    for p in want:
        for g in groups:
            if p - g[-1] >= 4:
                g.append(p)
                break
        else:
            groups.append([p])
    vpes = [0, 5000, T, 2 * T - 1]
    full = []
    for g in groups:
        v = background(rng, n)
        for p in g:
            plant(v, p)
        full.append(seg(v, vpes=vpes))
    v = background(rng, n)  # the 4-byte form at 0, and with its zero on either side of the tile edge
    plant(v, 1, four=True)
    plant(v, T - 1, four=True)
    plant(v, 2 * T, four=True)
    full.append(seg(v, vpes=vpes))
    tiny = [seg(b"", vpes=[]), seg(b"\x00", vpes=[0]), seg(SC, vpes=[0]), seg(SC + b"\x65", vpes=[0])]
    return [full[0], seg(b""), full[1], tiny[1], *full[2:], tiny[2], tiny[3], tiny[0]], groups


def end_of_video_segments(seed: int = 6):
    rng = np.random.default_rng(seed)
    a = background(rng, 300)
    a[-2:] = b"\x00\x00"  # the audio's 01 must not complete it
    b = background(rng, 300)
    b[-4:] = SC + b"\x65"
    tail = bytes(background(rng, 40))
    return [seg(a, b"\x01\x65" + tail, vpes=[0], atype=0x03), seg(b, b"\x01\x65" + tail, vpes=[0], atype=0x03)]


def zero_run_segments(seed: int = 7):
    rng = np.random.default_rng(seed)
    v = background(rng, 400)
    plant(v, 20)
    v[40:45] = b"\x00\x00\x00\x00\x01"  # start code at 42, 4-byte form; the zero at 40 stays in the NAL before
    v[100:106] = SC + SC  # a NAL of length 0, then a second one
    v[160:178] = SC * 6   # six start codes begin inside one lane's 16 bytes
    return [seg(v, vpes=[0, 90])]


def many_nal_segments(counts, seed: int = 8):
    rng = np.random.default_rng(seed)
    out = []
    for c in counts:
        v = background(rng, 16 + 37 * c)
        for k in range(c):
            plant(v, 5 + 37 * k, four=bool(k & 1))
        out.append(seg(v, vpes=[0, 37 * (c // 2)]))
    return out


def au_mapping_segments(seed: int = 9):
    rng = np.random.default_rng(seed)
    v = background(rng, 600)
    for p in (3, 20, 98, 147, 199, 300, 450):
        plant(v, p)
    # units start at 40: the NALs before it belong to none; 98..100 straddles the boundary at 100
    # (its NAL starts at 101); 147 starts a NAL exactly on 150; 199 one byte past 201's unit start
    a = seg(v, vpes=[40, 100, 150, 201, 201, 500])
    b = seg(v, vpes=[0, 30, 100, 150, 201, 250, 300, 350, 400, 460], n_vpes=10)  # more units than max_pes rows
    c = seg(v, vpes=[0, 100], vtype=0x24)
    d = seg(v, vpes=[0, 100], vtype=0x02)  # MPEG-2 video: unsupported
    return [a, b, c, d]


def adts_frame(payload: bytes, crc: bool = False, rate_idx: int = 3, channels: int = 2, length=None) -> bytes:
    header = 9 if crc else 7
    ln = header + len(payload) if length is None else length
    h = bytes([0xFF, 0xF0 | (0 if crc else 1), (1 << 6) | (rate_idx << 2) | (channels >> 2),
               ((channels & 3) << 6) | ((ln >> 11) & 3), (ln >> 3) & 0xFF, ((ln & 7) << 5) | 0x1F, 0xFC])
    return h + (b"\x12\x34" if crc else b"") + payload


def adts_segments(seed: int = 10):
    rng = np.random.default_rng(seed)

    def frames(k, size=120, **kw):
        return [adts_frame(bytes(background(rng, size + 3 * j)), **kw) for j in range(k)]

    def audio(groups):
        offs, data = [], b""
        for g in groups:
            offs.append(len(data))
            data += b"".join(g)
        return data, offs

    video = bytes(background(rng, 64))
    out = []
    a, o = audio([frames(2), frames(3), frames(1)])
    out.append(seg(video, a, vpes=[0], apes=o))  # clean
    a, o = audio([frames(2, crc=True, rate_idx=4, channels=6), frames(2, crc=True)])
    out.append(seg(video, a, vpes=[0], apes=o))  # 9-byte headers
    a, o = audio([frames(2), [b"\x00\x01\x02"] + frames(2), frames(1)])
    out.append(seg(video, a, vpes=[0], apes=o))  # lost sync at a PES start
    a, o = audio([frames(2), frames(2)])
    out.append(seg(video, a, vpes=[0], apes=[0, o[1] + 50]))  # the boundary cuts a frame: both PES fail
    a, o = audio([frames(1) + [adts_frame(b"", length=5)] + frames(1), frames(1)])
    out.append(seg(video, a, vpes=[0], apes=o))  # len < header
    a, o = audio([frames(2), frames(2)])
    out.append(seg(video + b"\x55", a, vpes=[0], apes=o))  # audio ES at an odd byte offset
    out.append(seg(video, a, vpes=[0], apes=o, atype=0x03))  # MPEG-1 audio: not walked
    a, o = audio([frames(1), frames(1), frames(1), frames(1), frames(1)])
    out.append(seg(video, a, vpes=[0], apes=o, n_apes=5))
    return out


CASES = {
    "boundary": lambda T: (boundary_segments(T)[0], 8, 2048),
    "end_of_video": lambda T: (end_of_video_segments(), 8, 2048),
    "zero_runs": lambda T: (zero_run_segments(), 8, 2048),
    "overflow": lambda T: (many_nal_segments([65, 200, 64, 63]), 8, 64),
    "au_mapping": lambda T: (au_mapping_segments(), 8, 2048),
    "adts": lambda T: (adts_segments(), 4, 2048),
}
