"""Fragmented-MP4 builders, hand-built batches and an independent sequential reference for
``ops.mp4_demux_batch`` (``docs/FMP4DEMUX.md`` holds the rules; this file keeps its own copy of
every one of them on purpose and shares no code with ``ops/csrc``)."""
import struct

import numpy as np
import torch

from hlsjs_p2p_wrapper_amd.ops.mp4demux import Mp4Track

M64 = (1 << 64) - 1
ID3_SCHEME = b"https://aomedia.org/emsg/ID3"
NAMES = ("minfo", "msamples", "runs", "emsg", "info", "pes", "nal", "au", "aframes", "sinfo")
# status bits, this file's copy
BAD_BOX, MOOF_OVERFLOW, EMSG_OVERFLOW, RUN_OVERFLOW, NO_TFDT, OUT_OF_RANGE, SAMPLE_OVERFLOW, NAL_ERROR, BAD_TS = \
    1, 2, 4, 8, 16, 32, 64, 128, 256
NAL_OVERFLOW, UNSUPPORTED_VIDEO = 1, 4
VIDEO = Mp4Track(1, "video", 0x1B, 4)
AUDIO = Mp4Track(2, "audio", 0x0F)
AV = (VIDEO, AUDIO)


# ------------------------------------------------------------------ boxes
def box(typ, payload=b"", largesize=False, size0=False, size=None):
    """One box.  ``largesize``: ``size == 1`` and a 64-bit size; ``size0``: ``size == 0`` (the box
    runs to the end of its container); ``size``: that value in the size field whatever the payload."""
    typ = typ if isinstance(typ, bytes) else typ.encode()
    if largesize:
        return struct.pack(">I4sQ", 1, typ, 16 + len(payload) if size is None else size) + payload
    n = 0 if size0 else 8 + len(payload) if size is None else size
    return struct.pack(">I4s", n, typ) + payload


def full_box(typ, version, flags, payload=b"", **kw):
    return box(typ, struct.pack(">I", (version << 24) | flags) + payload, **kw)


def mfhd(seq):
    return full_box("mfhd", 0, 0, struct.pack(">I", seq))


def tfhd(track_id, base_data_offset=None, sample_description_index=None, default_duration=None, default_size=None,
         default_flags=None, base_is_moof=True, **kw):
    flags, body = (0x020000 if base_is_moof else 0), struct.pack(">I", track_id)
    for bit, fmt, v in ((0x1, ">Q", base_data_offset), (0x2, ">I", sample_description_index),
                        (0x8, ">I", default_duration), (0x10, ">I", default_size), (0x20, ">I", default_flags)):
        if v is not None:
            flags |= bit
            body += struct.pack(fmt, v)
    return full_box("tfhd", 0, flags, body, **kw)


def tfdt(time, version=None, **kw):
    version = (1 if time >= 1 << 32 else 0) if version is None else version
    return full_box("tfdt", version, 0, struct.pack(">Q" if version else ">I", time), **kw)


def trun(entries, fields="dsfc", data_offset=None, first_sample_flags=None, version=0, sample_count=None, cut=0, **kw):
    """``entries``: ``(duration, size, flags, cts)`` per sample; ``fields`` names the per-sample
    fields that are written (``d``, ``s``, ``f``, ``c``); ``cut`` bytes are taken off the end."""
    flags = sum(bit for ch, bit in zip("dsfc", (0x100, 0x200, 0x400, 0x800)) if ch in fields)
    body = struct.pack(">I", len(entries) if sample_count is None else sample_count)
    if data_offset is not None:
        flags |= 1
        body += struct.pack(">i", data_offset)
    if first_sample_flags is not None:
        flags |= 4
        body += struct.pack(">I", first_sample_flags)
    for d, s, f, c in entries:
        for ch, v in zip("dsfc", (d, s, f, c)):
            if ch in fields:
                body += struct.pack(">i" if ch == "c" else ">I", v)
    return full_box("trun", version, flags, body[:len(body) - cut], **kw)


def emsg(version, scheme, value, timescale, time, duration, ident, data, terminate=True, **kw):
    z = b"\0" if terminate else b""
    strings = scheme + b"\0" + value + z
    if version == 0:
        body = strings + struct.pack(">IIII", timescale, time, duration, ident)
    else:
        body = struct.pack(">IQII", timescale, time, duration, ident) + strings
    return full_box("emsg", version, 0, body + data, **kw)


def nal(typ, payload=b"", hevc=False):
    return (bytes([typ << 1, 1]) if hevc else bytes([0x60 | typ])) + payload


def length_prefixed(nals, L=4):
    """An AVCC / HVCC sample from its NAL units."""
    return b"".join(len(x).to_bytes(L, "big") + x for x in nals)


def fragment(trafs, seq=1, front=b"", base_is_moof=True, mdat_extra=0):
    """``moof`` + ``mdat`` from ``[(track_id, tfdt or None, [sample bytes], [(duration, flags, cts)]), ...]``:
    one ``trun`` per ``traf`` with all four fields and a ``data_offset``."""
    def build(offsets):
        kids = [mfhd(seq)]
        for (tid, time, samples, meta), off in zip(trafs, offsets):
            entries = [(d, len(s), f, c) for s, (d, f, c) in zip(samples, meta)]
            kids.append(box("traf", tfhd(tid, base_is_moof=base_is_moof) + (tfdt(time) if time is not None else b"") +
                            trun(entries, data_offset=off)))
        return box("moof", b"".join(kids))
    size = len(build([0] * len(trafs)))
    offsets, pos = [], size + 8
    for _, _, samples, _ in trafs:
        offsets.append(pos)
        pos += sum(len(s) for s in samples)
    payload = b"".join(b"".join(samples) for _, _, samples, _ in trafs)
    return front + build(offsets) + box("mdat", payload, size=8 + len(payload) + mdat_extra)


def video_samples(count, nals_per=3, L=4, hevc=False, seed=0, key_every=30):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        types = ([35, 39, 19 if i % key_every == 0 else 1] if hevc else [9, 6, 5 if i % key_every == 0 else 1])
        out.append(length_prefixed([nal(t, rng.integers(0, 256, 3 + (i + k) % 5, dtype=np.uint8).tobytes(), hevc)
                                    for k, t in enumerate(types[:nals_per])], L))
    return out


def meta(count, duration=3000, cts=0, key_every=30):
    return [(duration, 0x02000000 if i % key_every == 0 else 0x01010000, cts) for i in range(count)]


def init_segment(tracks, timescales=(90000, 48000), avcc_length_size=4, bad=None):
    """A ``moov`` with one ``trak`` per ``(track_id, handler, sample entry name)`` and an ``mvex``."""
    traks, trexs = [], []
    for (tid, handler, entry), scale in zip(tracks, timescales):
        tkhd = full_box("tkhd", 0, 7, struct.pack(">III", 0, 0, tid) + bytes(68))
        mdhd = full_box("mdhd", 0, 0, struct.pack(">IIII", 0, 0, scale, 0) + bytes(4))
        hdlr = full_box("hdlr", 0, 0, bytes(4) + handler + bytes(12) + b"\0")
        if entry in (b"avc1", b"avc3"):
            avcc = box("avcC", bytes([1, 0x64, 0x00, 0x1F, 0xFC | (avcc_length_size - 1), 0xE0, 0]))
            se = box(entry, bytes(6) + struct.pack(">H", 1) + bytes(16) + struct.pack(">HH", 640, 360) + bytes(50) +
                     avcc)
        elif entry in (b"hvc1", b"hev1"):
            hv = bytearray(23)
            hv[0], hv[1], hv[12], hv[21] = 1, 1, 93, 0xFC | (avcc_length_size - 1)
            se = box(entry, bytes(6) + struct.pack(">H", 1) + bytes(16) + struct.pack(">HH", 640, 360) + bytes(50) +
                     box("hvcC", bytes(hv)))
        else:
            se = box(entry, bytes(6) + struct.pack(">H", 1) + bytes(20))
        stsd = full_box("stsd", 0, 0, struct.pack(">I", 1) + se)
        minf = box("minf", box("stbl", stsd))
        traks.append(box("trak", tkhd + box("mdia", mdhd + hdlr + minf)))
        trexs.append(full_box("trex", 0, 0, struct.pack(">IIIII", tid, 1, 1000 + tid, 100 + tid, 0x01010000)))
    moov = box("moov", full_box("mvhd", 0, 0, bytes(96)) + b"".join(traks) + box("mvex", b"".join(trexs)))
    data = box("ftyp", b"iso6" + bytes(4) + b"iso6cmfc") + moov
    return data[:-3] if bad == "cut" else data


# ------------------------------------------------------------------ the reference
def _s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def _u(S, p, k):
    return int.from_bytes(S[p:p + k], "big")


def _box(S, p, limit):
    """(type, header bytes, size) of the box at p of [p, limit), or None."""
    if limit - p < 8:
        return None
    size, typ, hdr = _u(S, p, 4), bytes(S[p + 4:p + 8]), 8
    if size == 1:
        if limit - p < 16:
            return None
        size, hdr = _u(S, p + 8, 8), 16
        if size >= 1 << 31:
            return None
    elif size == 0:
        size = limit - p
    if size < hdr or p + size > limit:
        return None
    return typ, hdr, size


def _cstring(S, q, end):
    z = S.find(b"\0", q, end)
    return (None, None) if z < 0 else (bytes(S[q:z]), z + 1)


def _emsg(S, p, hdr, size):
    body, end = p + hdr, p + size
    if end - body < 4:
        return None
    version = S[body]
    if version == 0:
        scheme, q = _cstring(S, body + 4, end)
        if q is None:
            return None
        value, q = _cstring(S, q, end)
        if q is None or end - q < 16:
            return None
        scale, time, dur, ident = struct.unpack(">IIII", S[q:q + 16])
        delta, q = 1, q + 16
    elif version == 1:
        if end - body < 24:
            return None
        scale, time, dur, ident = struct.unpack(">IQII", S[body + 4:body + 24])
        time = _s64(time)
        scheme, q = _cstring(S, body + 24, end)
        if q is None:
            return None
        value, q = _cstring(S, q, end)
        if q is None:
            return None
        delta = 0
    else:
        return None
    return [p, size, version, scale, time, delta, dur, ident, q, end - q, int(scheme == ID3_SCHEME), 0]


def ref_segment(S, tk, max_pes, max_nal, max_moof, max_run, max_emsg):
    """One segment of ``n = len(S)`` bytes with the track rows ``tk`` (``int64[2, 8]``): the ten
    tables as a dict of numpy arrays."""
    S, n = bytes(S), len(S)
    out = {"minfo": np.zeros(18, np.int64), "msamples": np.full((2, max_pes, 4), -1, np.int32),
           "runs": np.full((max_run, 16), -1, np.int64), "emsg": np.full((max_emsg, 12), -1, np.int64),
           "info": np.zeros(24, np.int64), "pes": np.full((3, max_pes, 3), -1, np.int64),
           "nal": np.full((max_nal, 4), -1, np.int32), "au": np.full((max_pes, 4), -1, np.int32),
           "aframes": np.full((max_pes, 2), -1, np.int32), "sinfo": np.zeros(8, np.int64)}
    status = 0
    ids = [int(tk[0, 0]), int(tk[1, 0])]

    # the top level
    moofs, n_moof, n_emsg, p = [], 0, 0, 0
    while p < n:
        b = _box(S, p, n)
        if b is None:
            status |= BAD_BOX
            break
        typ, hdr, size = b
        if typ == b"moof":
            if n_moof < max_moof:
                moofs.append((p, hdr, size))
            n_moof += 1
        elif typ == b"emsg":
            if n_emsg < max_emsg:
                row = _emsg(S, p, hdr, size)
                if row is None:
                    status |= BAD_BOX
                else:
                    out["emsg"][n_emsg] = row
            n_emsg += 1
        p += size
    if n_moof > max_moof:
        status |= MOOF_OVERFLOW
    if n_emsg > max_emsg:
        status |= EMSG_OVERFLOW

    # the moofs: runs in order, with the state a sequential reader keeps
    runs, n_run, n_other, first_seq = [], 0, 0, -1
    seen = [0, 0]                # samples of each track so far
    clock = [(0, 0), (0, 0)]     # (decode time, at sample) of the last tfdt-bearing traf that had a run
    for k, (mp, mhdr, msize) in enumerate(moofs):
        p, mend, seen_mfhd = mp + mhdr, mp + msize, False
        while p < mend:
            b = _box(S, p, mend)
            if b is None:
                status |= BAD_BOX
                break
            typ, hdr, size = b
            body, end = p + hdr, p + size
            if typ == b"mfhd" and not seen_mfhd:
                seen_mfhd = True
                if end - body >= 8:
                    if k == 0:
                        first_seq = _u(S, body + 4, 4)
                else:
                    status |= BAD_BOX
            elif typ == b"traf":
                slot, base, time, has_time = None, mp, 0, False
                seen_tfhd = seen_tfdt = seen_trun = False
                dd = ds = df = 0
                traf_run, place = 0, None
                q = body
                while q < end:
                    c = _box(S, q, end)
                    if c is None:
                        status |= BAD_BOX
                        break
                    ctyp, chdr, csize = c
                    cb, ce = q + chdr, q + csize
                    if ctyp == b"tfhd" and not seen_tfhd:
                        seen_tfhd = True
                        f = _u(S, cb, 4) & 0xFFFFFF if ce - cb >= 8 else 0
                        need = 8 + 8 * bool(f & 1) + 4 * sum(bool(f & bit) for bit in (2, 8, 16, 32))
                        if ce - cb < need:
                            status |= BAD_BOX
                        else:
                            tid = _u(S, cb + 4, 4)
                            slot = 0 if ids[0] > 0 and tid == ids[0] else 1 if ids[1] > 0 and tid == ids[1] else -1
                            r = cb + 8
                            if f & 1:
                                base, r = _s64(_u(S, r, 8)), r + 8
                            if f & 2:
                                r += 4
                            if slot >= 0:
                                dd, ds, df = (int(tk[slot, 4]) & 0xFFFFFFFF, int(tk[slot, 5]) & 0xFFFFFFFF,
                                              int(tk[slot, 6]) & 0xFFFFFFFF)
                            if f & 8:
                                dd, r = _u(S, r, 4), r + 4
                            if f & 16:
                                ds, r = _u(S, r, 4), r + 4
                            if f & 32:
                                df = _u(S, r, 4)
                    elif ctyp == b"tfdt" and not seen_tfdt and not seen_trun:
                        seen_tfdt = True
                        version = S[cb] if ce - cb >= 8 else 0
                        if ce - cb < (8 if version == 0 else 12):
                            status |= BAD_BOX
                        else:
                            time, has_time = (_u(S, cb + 4, 4) if version == 0 else _s64(_u(S, cb + 4, 8))), True
                    elif ctyp == b"trun":
                        seen_trun = True
                        if slot is None:
                            status |= BAD_BOX
                        elif slot >= 0:
                            vf = _u(S, cb, 4) if ce - cb >= 8 else 0
                            f = vf & 0xFFFFFF
                            if ce - cb < 8 + 4 * bool(f & 1) + 4 * bool(f & 4):
                                status |= BAD_BOX
                            else:
                                count, r = _u(S, cb + 4, 4), cb + 8
                                if f & 1:
                                    off = _u(S, r, 4)
                                    place, r = (_s64(base + (off - (1 << 32) if off >> 31 else off)), seen[slot]), r + 4
                                elif traf_run == 0:
                                    place = (base, seen[slot])
                                first_flags = -1
                                if f & 4:
                                    first_flags, r = _u(S, r, 4), r + 4
                                stride = 4 * bin(f & 0xF00).count("1")
                                fit = (ce - r) // stride if stride else n
                                if count > fit:
                                    status |= BAD_BOX
                                    count = fit
                                if traf_run == 0 and has_time:
                                    clock[slot] = (time, seen[slot])
                                if n_run < max_run:
                                    runs.append([slot, k, seen[slot], count, r, vf, traf_run, dd, ds, df, first_flags,
                                                 place[0], place[1], clock[slot][0], clock[slot][1], 0])
                                    seen[slot] += count
                                n_run += 1
                                traf_run += 1
                    q = ce
                if slot is None:
                    status |= BAD_BOX
                elif slot < 0:
                    n_other += 1
                elif not has_time:
                    status |= NO_TFDT
            p = end
    if n_run > max_run:
        status |= RUN_OVERFLOW
    for r, row in enumerate(runs):
        out["runs"][r] = row


    # the samples of each track, in run and entry order; sums wrap at 64 bits
    first_pts, last_pts, totals = [-1, -1], [-1, -1], [0, 0]
    for t in (0, 1):
        sizes = durations = i = 0
        size_at, time_at = {}, {}
        min_pts = max_pts = first_sync = base_time = -1
        started = False
        for row in runs:
            if row[0] != t:
                continue
            _, _, first, count, q, vf, _, dd, ds, df, first_flags, start, start_sample, time, time_sample, _ = row
            size_at[first], time_at[first] = sizes, durations
            if not started:
                started, base_time = True, time
            for j in range(count):
                d, s, f, c = dd, ds, df, 0
                if vf & 0x100:
                    d, q = _u(S, q, 4), q + 4
                if vf & 0x200:
                    s, q = _u(S, q, 4), q + 4
                if vf & 0x400:
                    f, q = _u(S, q, 4), q + 4
                if vf & 0x800:
                    c, q = struct.unpack(">i", S[q:q + 4])[0], q + 4
                if j == 0 and first_flags >= 0:
                    f = first_flags
                if i < max_pes:
                    off = _s64(start + sizes - size_at[start_sample])
                    dts = _s64(time + durations - time_at[time_sample])
                    pts = _s64(dts + c)
                    stop = _s64(off + s)
                    if not (0 <= off <= stop <= n):
                        status |= OUT_OF_RANGE
                    a = min(max(off, 0), n)
                    e = n if stop < off else min(max(stop, a), n)
                    if d > 0x7FFFFFFF:
                        status |= BAD_TS
                    out["pes"][t, i] = (a, pts, dts)
                    out["msamples"][t, i] = (e - a, d if d <= 0x7FFFFFFF else 0, c, f - (1 << 32) if f >> 31 else f)
                    min_pts = pts if i == 0 else min(min_pts, pts)
                    max_pts = pts if i == 0 else max(max_pts, pts)
                    if first_sync < 0 and not f & 0x10000:
                        first_sync = i
                    if i == 0:
                        first_pts[t] = pts
                    last_pts[t] = pts
                sizes, durations, i = sizes + s, durations + d, i + 1
        if i > max_pes:
            status |= SAMPLE_OVERFLOW
        totals[t] = i
        out["minfo"][6 + 6 * t:12 + 6 * t] = (i, base_time, _s64(durations), min_pts, max_pts, first_sync)

    # the demux row
    vt, L = int(tk[0, 2]), int(tk[0, 3])
    indexed = ids[0] > 0 and vt in (0x1B, 0x24) and L in (1, 2, 4)
    info = out["info"]
    info[1], info[2], info[3], info[4] = -1, ids[0] if ids[0] > 0 else -1, ids[1] if ids[1] > 0 else -1, -1
    info[6], info[9], info[12], info[14] = n, totals[0], vt if indexed else 0, n
    info[13] = int(tk[1, 2]) if ids[1] > 0 else 0
    info[16:19], info[19:22], info[22] = first_pts + [-1], last_pts + [-1], n

    # the NAL units of the recorded video samples
    sinfo = out["sinfo"]
    sinfo[4] = -1
    if not indexed:
        sinfo[0] = UNSUPPORTED_VIDEO
    else:
        hevc, m, n_nal, keys, first_key = vt == 0x24, min(totals[0], max_pes), 0, 0, -1
        for a in range(m):
            q = int(out["pes"][0, a, 0])
            end = q + int(out["msamples"][0, a, 0])
            first, count, flags = -1, 0, 0
            while q + L <= end:
                ln, s = _u(S, q, L), q + L
                if ln > end - s:
                    status |= NAL_ERROR
                    break
                if n_nal < max_nal:
                    typ = -1 if ln == 0 else (S[s] >> 1) & 0x3F if hevc else S[s] & 0x1F
                    out["nal"][n_nal] = (s, ln, typ, a)
                    first, count = (n_nal if count == 0 else first), count + 1
                    if hevc:
                        flags |= (1 if 16 <= typ <= 21 else 0) | {33: 2, 34: 4, 35: 8}.get(typ, 0)
                    else:
                        flags |= {5: 1, 7: 2, 8: 4, 9: 8}.get(typ, 0)
                n_nal += 1
                q = s + ln
            else:
                if q != end:
                    status |= NAL_ERROR
            out["au"][a] = (first, count, flags, int(out["msamples"][0, a, 0]))
            if flags & 1:
                keys, first_key = keys + 1, (a if first_key < 0 else first_key)
        sinfo[0] = NAL_OVERFLOW if n_nal > max_nal else 0
        sinfo[1:5] = (n_nal, m, keys, first_key)
    out["minfo"][:6] = (status, n_moof, first_seq, n_run, n_other, n_emsg)
    return out


# ------------------------------------------------------------------ batches
LIMITS = dict(max_pes=512, max_nal=2048, max_moof=64, max_run=128, max_emsg=16)
GAP = 48  # canary bytes between segments


def layout(segments, tail=GAP):
    """The segments at 16-byte aligned offsets with ``GAP`` canary bytes in front of each and
    ``tail`` behind the last, the buffer's size a multiple of 4: (bytes, offsets, lengths)."""
    buf, offs = bytearray(), []
    for s in segments:
        buf += b"\xA5" * GAP
        buf += b"\xA5" * (-len(buf) % 16)
        offs.append(len(buf))
        buf += s
    buf += b"\xA5" * tail
    buf += b"\xA5" * (-len(buf) % 4)
    return bytes(buf), offs, [len(s) for s in segments]


def batch(name, dev="cpu"):
    """Case ``name`` on ``dev``: (buf tensor, offs, lens, tracks, limits)."""
    segments, tracks, limits = CASES[name]()
    raw, offs, lens = layout(segments, tail=0 if name == "nal" else GAP)
    return torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev), offs, lens, tracks, {**LIMITS, **limits}


def track_rows(tracks, B):
    """This file's own ``int64[B, 2, 8]`` track rows: slot 0 the video track, slot 1 the audio track,
    each ``(track_ID, kind 1 / 2, codec_type, nal_length_size (0 for audio), trex duration, size, flags, 0)``."""
    def one(ts):
        rows = np.zeros((2, 8), np.int64)
        for t in ts:
            slot = {"video": 0, "audio": 1}[t.kind]
            rows[slot] = (t.track_id, slot + 1, t.codec_type, t.nal_length_size if slot == 0 else 0,
                          t.default_duration, t.default_size, t.default_flags, 0)
        return rows
    per_segment = not all(isinstance(t, Mp4Track) for t in tracks)
    rows = [one(tracks[i] if per_segment else tracks) for i in range(B)]
    return np.stack(rows) if B else np.zeros((0, 2, 8), np.int64)


def ref_batch(buf, offs, lens, tracks, limits):
    """The reference over a batch: the ten tables stacked, by name."""
    raw = buf.cpu().numpy().tobytes()
    tk = track_rows(tracks, len(offs))
    rows = [ref_segment(raw[o:o + n], tk[i], **limits) for i, (o, n) in enumerate(zip(offs, lens))]
    shapes = ref_segment(b"", np.zeros((2, 8), np.int64), **limits)
    return {k: np.stack([r[k] for r in rows]) if rows else np.zeros((0, *shapes[k].shape), shapes[k].dtype)
            for k in NAMES}


def assert_equal(got, ref):
    """All ten tensors of ``got`` (an ``Mp4Demux`` or a dict of arrays) equal ``ref`` bit for bit."""
    for k in NAMES:
        g = got[k] if isinstance(got, dict) else getattr(got, k).cpu().numpy()
        assert g.shape == ref[k].shape and g.dtype == ref[k].dtype, (k, g.shape, ref[k].shape, g.dtype)
        if not np.array_equal(g, ref[k]):
            bad = np.argwhere(g != ref[k])[0]
            raise AssertionError(f"{k}{tuple(bad)}: got {g[tuple(bad)]}, reference {ref[k][tuple(bad)]}")


def two_pass(make):
    """A segment whose moof needs to know its own size: ``make(moof_size)`` returns the moof."""
    return make(len(make(0)))


def patch_size(seg, typ, size):
    i = seg.index(typ) - 4
    return seg[:i] + struct.pack(">I", size) + seg[i + 4:]


def _frag(n_video=2, n_audio=0, **kw):
    trafs = [(1, 9000, video_samples(n_video), meta(n_video))] if n_video else []
    if n_audio:
        trafs.append((2, 4800, [bytes([i & 0xFF]) * 6 for i in range(n_audio)], meta(n_audio, 1024, key_every=1)))
    return fragment(trafs, **kw)


def case_headers():
    F = _frag()
    segs = [F, _frag(mdat_extra=-1), _frag(mdat_extra=1), patch_size(F, b"mdat", 0),
            _frag(front=box("free", b"x" * 5, largesize=True)),
            _frag(front=box("free", b"", largesize=True, size=1 << 31)),
            _frag(front=box("free", b"", size=7)), box("styp", b"msdh" + bytes(4) + b"msdhmsix") + F,
            box("prft", bytes(20)) + box("sidx", bytes(32)) + F + box("what", b"??")]
    segs += [F + bytes(k) for k in range(1, 8)]
    segs += [_frag(front=box("free", bytes(k))) for k in range(16)]
    segs += [b"", bytes(7), box("free"), F[:8], F[:24]]
    return segs, AV, dict(max_pes=16, max_nal=64)


def _one_traf(make_traf, payload=bytes(range(64))):
    return two_pass(lambda size: box("moof", mfhd(7) + box("traf", make_traf(size + 8)))) + box("mdat", payload)


def case_fields():
    segs = []
    e3 = [(100, 7, 0x01010000, 3), (200, 9, 0x02000000, -2), (300, 11, 0x01010000, 0)]
    for m in range(32):  # every subset of the five tfhd optionals; the trun has no per-sample field
        kw = dict(base_data_offset=100 if m & 1 else None, sample_description_index=1 if m & 2 else None,
                  default_duration=512 if m & 4 else None, default_size=5 if m & 8 else None,
                  default_flags=0x10000 if m & 16 else None, base_is_moof=bool(m & 1) or m % 3 != 0)
        segs.append(_one_traf(lambda off, kw=kw: tfhd(1, **kw) + tfdt(5) +
                              trun(e3, fields="", data_offset=None if kw["base_data_offset"] else off)))
    segs.append(_one_traf(lambda off: tfhd(1) + tfdt(0xFFFFFFFF, version=0) + trun(e3, data_offset=off)))
    segs.append(_one_traf(lambda off: tfhd(1) + tfdt((1 << 32) + 77, version=1) + trun(e3, data_offset=off)))
    segs.append(_one_traf(lambda off: tfhd(1) + tfdt((1 << 63) + 5, version=1) + trun(e3, data_offset=off)))
    for m in range(64):  # the 16 per-sample subsets x data_offset x first_sample_flags
        fields = "".join(ch for b, ch in enumerate("dsfc") if m & (1 << b))
        segs.append(_one_traf(lambda off, m=m, fields=fields: tfhd(1, default_size=6, default_duration=90) +
                              tfdt(1000) +
                              trun(e3, fields=fields, data_offset=off if m & 16 else None,
                                   first_sample_flags=0x02000000 if m & 32 else None)))
    segs.append(_one_traf(lambda off: tfhd(1) + tfdt(0) + trun(e3, data_offset=-40)))
    segs.append(_one_traf(lambda off: tfhd(1, base_data_offset=(1 << 64) - 8) + tfdt(0) + trun(e3, data_offset=off)))
    for version in (0, 1):
        segs.append(_one_traf(lambda off, v=version: tfhd(1) + tfdt(10) +
                              trun([(10, 4, 0, -25), (10, 4, 0, -(1 << 31)), (10, 4, 0, (1 << 31) - 1)],
                                   data_offset=off, version=v)))
    for cut in (1, 4, 15, 16, 17):  # a trun one entry (or part of one) too short
        segs.append(_one_traf(lambda off, cut=cut: tfhd(1) + tfdt(0) + trun(e3, data_offset=off, cut=cut)))
    segs.append(_one_traf(lambda off: tfhd(1) + tfdt(0) + trun(e3, data_offset=off, sample_count=0xFFFFFFFF)))
    segs.append(_one_traf(lambda off: tfhd(1) + tfdt(0) +
                          trun([], fields="", data_offset=off, sample_count=0xFFFFFFFF)))
    segs.append(_one_traf(lambda off: tfhd(1) + tfdt(0) + full_box("trun", 0, 5, struct.pack(">I", 1))))  # header cut
    segs.append(_one_traf(lambda off: full_box("tfhd", 0, 0x39, struct.pack(">II", 1, 9)) + trun(e3, data_offset=off)))
    segs.append(_one_traf(lambda off: trun(e3, data_offset=off) + tfhd(1) + tfdt(3) + trun(e3, data_offset=off)))
    segs.append(_one_traf(lambda off: tfhd(1) + full_box("tfdt", 1, 0, bytes(4)) + trun(e3, data_offset=off)))
    segs.append(_one_traf(lambda off: tfhd(1) + tfdt(3) + tfdt(9) + tfhd(2) + trun(e3, data_offset=off) + tfdt(4)))
    segs.append(box("moof", box("mfhd", bytes(3)) + box("traf", tfdt(3))) + box("moof", mfhd(5) + mfhd(6)))
    tracks = (Mp4Track(1, "video", 0x1B, 4, default_duration=1001, default_size=4, default_flags=0x01010000), AUDIO)
    return segs, tracks, dict(max_pes=8, max_nal=32)


def _audio(count, byte=0x11):
    return [(1024, 1, 0x02000000, 0)] * count, bytes([byte]) * count


def case_runs():
    segs = []
    e2, e3 = [(10, 4, 0, 0), (20, 6, 0x10000, 1)], [(5, 3, 0, 0), (6, 2, 0, 0), (7, 1, 0, 0)]
    for second in (None, 40):  # two runs in one traf, the second with and without a data_offset
        segs.append(_one_traf(lambda off, s=second: tfhd(2) + tfdt(100) + trun(e2, data_offset=off) +
                              trun(e3, data_offset=None if s is None else off + s)))
    segs.append(_one_traf(lambda off: tfhd(2) + tfdt(100) + trun([], data_offset=off) + trun(e2) + trun([]) + trun(e3)))
    # two trafs of one track in one moof, and in two moofs; a missing tfdt on the first and on the second
    for t1, t2 in ((100, 500), (None, 500), (100, None), (None, None)):
        a = tfhd(2) + (tfdt(t1) if t1 is not None else b"")
        b = tfhd(2) + (tfdt(t2) if t2 is not None else b"")
        segs.append(two_pass(lambda size: box("moof", mfhd(1) + box("traf", a + trun(e2, data_offset=size + 8)) +
                                              box("traf", b + trun(e3, data_offset=size + 18)))) +
                    box("mdat", bytes(40)))
        one = two_pass(lambda size: box("moof", mfhd(1) + box("traf", a + trun(e2, data_offset=size + 8))))
        two = two_pass(lambda size: box("moof", mfhd(2) + box("traf", b + trun(e3, data_offset=size + 8))))
        segs.append(one + box("mdat", bytes(10)) + two + box("mdat", bytes(6)))
    # interleaved video and audio trafs and a traf of an unknown track
    v = video_samples(4)
    segs.append(fragment([(1, 0, v[:2], meta(2)), (2, 0, [b"ab", b"cd"], meta(2, 1024)), (9, 0, [b"zz"], meta(1)),
                          (1, None, v[2:], meta(2)), (2, 7, [b"ef"], meta(1, 1024))]))
    for count in (63, 64, 65, 255, 256, 257, 600):  # the rounds of the sample pass, max_pes 512
        e, payload = _audio(count)
        segs.append(_one_traf(lambda off: tfhd(2) + tfdt(1 << 33) + trun(e, fields="ds", data_offset=off), payload))
    segs.append(_frag(n_video=65, n_audio=70))
    for count in (127, 128, 129):  # runs of one sample each, max_run 128
        segs.append(_one_traf(lambda off: tfhd(2) + tfdt(0) + trun([(3, 1, 0, 0)], data_offset=off) +
                              b"".join(trun([(3 + r, 1, 0, 0)]) for r in range(1, count)), bytes(range(129))))
    for count in (63, 64, 65):  # moofs of one sample each, max_moof 64
        segs.append(b"".join(_one_traf(lambda off, k=k: tfhd(2) + (tfdt(50) if k == 0 else b"") +
                                        trun([(2, 1, 0, k)], data_offset=off), bytes([k])) for k in range(count)))
    big = [(0x7FFFFFFF, 1, 0, 0)] * 3 + [(0x80000000, 1, 0, 0), (0xFFFFFFFF, 1, 0, 0), (1, 1, 0, 0)]
    segs.append(_one_traf(lambda off: tfhd(2) + tfdt((1 << 32) - 5) + trun(big, data_offset=off)))
    return segs, AV, {}


def _nal_seg(samples, hevc=False):
    return fragment([(1, 0, samples, meta(len(samples)))])


def case_nal():
    segs, tracks = [], []
    for L in (1, 2, 4):
        segs.append(_nal_seg(video_samples(5, L=L, seed=L)))
        tracks.append((Mp4Track(1, "video", 0x1B, L), AUDIO))
    segs.append(_nal_seg(video_samples(5)))
    tracks.append((Mp4Track(1, "video", 0, 4), AUDIO))
    segs.append(_nal_seg(video_samples(3)))
    tracks.append((AUDIO,))  # no video track at all
    one = [length_prefixed([nal(1 + i % 5, bytes(range(12)))]) for i in range(33)]  # 17 bytes each: every offset mod 16
    segs.append(_nal_seg(one))
    tracks.append(AV)
    odd = [length_prefixed([b"", nal(5, b"abc"), b""]), struct.pack(">I", 6) + nal(5, b"abcd"),
           length_prefixed([nal(1, b"xy")]) + b"\0", b"", length_prefixed([nal(7, b"s"), nal(8, b"p")]) + bytes(3),
           struct.pack(">I", 0xFFFFFFFF) + b"q"]
    segs.append(_nal_seg(odd))
    tracks.append(AV)
    for total in (2047, 2048, 2049):  # zero-length NAL units with a one-byte length field
        segs.append(_nal_seg([bytes(1000), bytes(total - 1000 - 1) + length_prefixed([nal(5, b"k")], 1)]))
        tracks.append((Mp4Track(1, "video", 0x1B, 1), AUDIO))
    hv = [length_prefixed([nal(t, b"hevc" + bytes([t]), hevc=True)], 2) for t in (35, 33, 34, 39, 19, 1, 21, 40)]
    segs.append(_nal_seg(hv))
    tracks.append((Mp4Track(1, "video", 0x24, 2), AUDIO))
    # 300 video samples of seven NAL units: the NAL pass runs a second round of 256 samples with its
    # carry, and the rows cross max_nal (2048) inside that round, at sample 292
    many = [length_prefixed([nal(5 if i % 100 == 0 else 1, bytes([i & 0xFF])) for _ in range(7)], 1)
            for i in range(300)]
    segs.append(_nal_seg(many))
    tracks.append((Mp4Track(1, "video", 0x1B, 1), AUDIO))
    segs.append(_nal_seg(video_samples(7, seed=9)))  # the batch's last segment ends the buffer
    tracks.append(AV)
    return segs, tracks, {}


def case_emsg():
    id3 = b"ID3\x04\0\0\0\0\0\x0aTXXX....."
    boxes = [emsg(0, ID3_SCHEME, b"", 90000, 1234, 90000, 7, id3),
             emsg(1, ID3_SCHEME, b"v", 1000, (1 << 40) + 9, 5, 8, id3),
             emsg(1, b"urn:scte:scte35:2013:bin", b"x", 1, 2, 3, 4, b"\xFC"),
             emsg(0, ID3_SCHEME[:-1] + b"4", b"", 1, 2, 3, 4, id3),
             emsg(0, ID3_SCHEME + b"x", b"", 1, 2, 3, 4, id3), emsg(1, ID3_SCHEME[:-1], b"", 1, 2, 3, 4, id3),
             emsg(1, b"", b"", 1, 2, 3, 4, b""), emsg(1, ID3_SCHEME, b"value", 1, 2, 3, 4, b"", terminate=False),
             full_box("emsg", 0, 0, ID3_SCHEME), full_box("emsg", 0, 0, ID3_SCHEME + b"\0v\0" + bytes(15)),
             full_box("emsg", 1, 0, bytes(19)), full_box("emsg", 2, 0, bytes(40)), box("emsg", b"\0\0"),
             emsg(0, ID3_SCHEME, b"", 1, 2, 3, 4, id3, largesize=True)]
    more = [emsg(1, ID3_SCHEME, b"", 1000, k, 1, k, bytes([k])) for k in range(17)]
    return [b"".join(boxes) + _frag(), b"".join(more) + _frag(), _frag(front=box("free", bytes(3)) + boxes[1])], AV, {}


def case_random():
    rng = np.random.default_rng(2024)
    segs = [rng.integers(0, 256, int(rng.integers(16, 400)), dtype=np.uint8).tobytes() for _ in range(40)]
    for _ in range(8):  # a believable frame around random bytes
        inner = rng.integers(0, 256, int(rng.integers(24, 200)), dtype=np.uint8).tobytes()
        segs.append(box("moof", mfhd(1) + box("traf", tfhd(1) + inner)) + box("mdat", bytes(32)))
        segs.append(box("moof", box("traf", tfhd(2) + full_box("trun", 0, int(rng.integers(0, 0xFFF)), inner))))
    return segs, AV, dict(max_pes=32, max_nal=64, max_moof=4, max_run=8, max_emsg=2)


def case_mutated():
    rng = np.random.default_rng(77)
    good = [_frag(n_video=4, n_audio=5), case_runs()[0][0], case_emsg()[0][2]]
    segs = []
    for k in range(48):
        s = bytearray(good[k % 3])
        end = s.index(b"mdat") - 4
        for _ in range(1 + k % 2):
            s[int(rng.integers(0, end))] = int(rng.integers(0, 256))
        segs.append(bytes(s))
    return segs, AV, dict(max_pes=32, max_nal=64)


def case_small():
    return [_frag(n_video=3, n_audio=4), b"", _frag(n_video=1)], AV, dict(max_pes=8, max_nal=16, max_moof=2, max_run=4,
                                                                           max_emsg=2)


def case_captions(duration=3000, audio_duration=1024):
    """Video samples whose SEI NAL units carry GA94 captions, H.264 and HEVC, with composition
    offsets that reorder them: what ``caption_batch`` reads through the views."""
    import captions_cases as cc

    segs, tracks = [], []
    for hevc in (False, True):
        samples, m = [], []
        for i in range(6):
            aud = nal(35 if hevc else 9, b"\xf0", hevc)
            sei = cc.sei(cc.caption(cc.triples(1 + i, seed=i)), hevc=hevc)
            pic = nal((19 if hevc else 5) if i == 0 else 1, bytes([0x80 + i]) * 9, hevc)
            samples.append(length_prefixed([aud, sei, pic] if i != 3 else [aud, pic]))
            m.append((duration, 0x02000000 if i == 0 else 0x01010000, (0, 6000, -3000, 3000, 0, 9000)[i]))
        segs.append(fragment([(1, 90000, samples, m), (2, 48000, [b"aac!"] * 3, meta(3, audio_duration))]))
        tracks.append((Mp4Track(1, "video", 0x24 if hevc else 0x1B, 4), AUDIO))
    return segs, tracks, dict(max_pes=8, max_nal=32)


CASES = {"captions": case_captions, "headers": case_headers, "fields": case_fields, "runs": case_runs, "nal": case_nal,
         "emsg": case_emsg,
         "random": case_random, "mutated": case_mutated, "small": case_small}
