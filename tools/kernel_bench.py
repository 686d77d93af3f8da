"""Per-kernel microbenchmark on one bench round's batch: 64 x ~3 MB AES-128 TS segments
(the 1080p 6 Mb/s config).  Times AES-CBC decrypt, TS demux (psi+scan+gather), the sample
index over the demuxed ES, the remux to fMP4 samples, the moof boxes in front of them (next to the
host packing they replace), the codec configuration for the init segments
(H.264 and HEVC), the SAMPLE-AES decrypt of the same ES protected by the tool, the caption extraction
on a video ES the tool writes itself, the fragmented-MP4 demux on segments the tool writes itself (one
``moof`` and thirty), the cbcs decrypt of such segments protected by the tool (the demux row's segment and
one of about 3 MB), the cenc decrypt of the same two segments protected under cenc, the packed-audio demux
on segments the tool writes itself (the walk through LDS tiles, the one through global memory and the
batched copy of the same bytes), the MPEG audio remux on the bench's video with an MP3 track the tool
writes in place of the AAC one, and the MFMA CRC
with HIP events and reports us / GB/s of input.
Checks results against the host oracles once.

    PYTHONPATH=. python tools/kernel_bench.py [--segs 64] [--iters 20] [--only packedaudio|mpegaudio|ac3audio]
"""
import argparse
import json
import struct
import time

import numpy as np
import torch

from hlsjs_p2p_wrapper_amd.net.origin import PRESET_1080P_6M, SyntheticHlsOrigin
from hlsjs_p2p_wrapper_amd.ops import (ac3audio, aes, captions, cbcs, cenc, codecconfig, crc, esindex, fragment,
                                       hevcconfig, mp4demux, mpegaudio, packedaudio, remux, sampleaes, segment, tsdemux)
from hlsjs_p2p_wrapper_amd.ops._native import device, runtime
from hlsjs_p2p_wrapper_amd.player import fmp4


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def timed_each(setup, fn, iters):
    """``fn`` alone, with ``setup`` in front of every call and outside the timed intervals."""
    setup()
    fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(iters):
        setup()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs) * 1e3 / iters  # us


def protect_es(es, es_offs, info, pes, nal, sinfo, aframes, key, iv):
    """The tool's packager: the demuxed ES (host array, changed in place) with every block the
    SAMPLE-AES format encrypts encrypted, one CBC chain per slice NAL and per ADTS frame.  No
    emulation prevention is inserted (the ES keeps its size): where ciphertext happens to hold
    ``00 00 03`` the decrypt drops a byte, a few times in a million blocks."""
    I, S = tsdemux.INFO, esindex.SINFO
    blocks = 0

    def chain(at):  # the 16-byte blocks at the ascending byte offsets ``at``, as one CBC chain
        idx = (at[:, None] + np.arange(16)[None, :]).reshape(-1)
        es[idx] = aes.cbc_encrypt(key, iv, es[idx])[:len(idx)]
        return len(at)

    for i, base in enumerate(es_offs):
        m = int(sinfo[i, S["n_au"]])
        for off, n, typ, au in nal[i, :min(int(sinfo[i, S["n_nal"]]), nal.shape[1])]:
            if typ in (1, 5) and 0 <= au < m and n > 48:
                blocks += chain(base + off + np.arange(32, n - 16, 160))
        a0 = base + int(info[i, I["audio_es_offset"]])
        for k in range(int(info[i, I["n_audio_pes"]])):
            q = a0 + int(pes[i, 1, k, 0])
            for _ in range(int(aframes[i, k, 0])):
                ln = ((int(es[q + 3]) & 3) << 11) | (int(es[q + 4]) << 3) | (int(es[q + 5]) >> 5)
                hdr = 7 if es[q + 1] & 1 else 9
                if ln - hdr >= 32:
                    blocks += chain(q + hdr + 16 + 16 * np.arange((ln - hdr - 16) // 16))
                q += ln
    return blocks


def caption_batch_inputs(offs, lens, size, dev, n_au=120, seed=5):
    """A demuxed batch written by hand for the caption row: per segment ``n_au`` access units of an
    AUD, one caption SEI of 20 triples and a slice of random bytes free of start codes, sized to the
    shortest segment; the demux tables filled by hand.  ``(DemuxResult, caps, host DemuxResult of
    segment 0)``."""
    I = tsdemux.INFO
    B, body = len(offs), (min(lens) - 256) // n_au
    tri = b"".join(bytes([0xFC | (t & 1), 0x20 + t, 0x40 + t]) for t in range(20))
    payload = b"\xb5\x00\x31GA94\x03" + bytes([0x40 | 20, 0xFF]) + tri + b"\xff"
    head = b"\x00\x00\x00\x01\x09\xf0\x00\x00\x01\x06\x04" + bytes([len(payload)]) + payload + b"\x80\x00\x00\x01\x41"
    units = np.random.default_rng(seed).integers(1, 256, (n_au, body), dtype=np.uint8)
    units[:, :len(head)] = np.frombuffer(head, np.uint8)
    ves = units.reshape(-1)
    max_pes = 256
    info = np.zeros((B, tsdemux.INFO_WORDS), np.int64)
    info[:, I["video_bytes"]] = info[:, I["audio_es_offset"]] = info[:, I["id3_es_offset"]] = len(ves)
    info[:, I["payload_bytes"]] = len(ves)
    info[:, I["n_video_pes"]], info[:, I["video_type"]] = n_au, 0x1B
    pes = np.full((B, 3, max_pes, 3), -1, np.int64)
    a = np.arange(n_au)
    pes[:, 0, :n_au, 0], pes[:, 0, :n_au, 2] = a * body, 90000 + 3000 * a
    pes[:, 0, :n_au, 1] = 90000 + 3000 * (a ^ 1) + 6000  # pairs of access units swap their presentation order
    es = np.zeros(size, np.uint8)
    for o in offs:
        es[o:o + len(ves)] = ves
    dres = tsdemux.DemuxResult(torch.from_numpy(info).to(dev), torch.from_numpy(pes).to(dev),
                               torch.from_numpy(es).to(dev), np.asarray(offs, np.int64))
    hres = tsdemux.DemuxResult(torch.from_numpy(info[:1].copy()), torch.from_numpy(pes[:1].copy()),
                               torch.from_numpy(np.concatenate([ves, np.zeros(256, np.uint8)])), np.zeros(1, np.int64))
    return dres, [len(ves)] * B, hres


def mp4_segment(moofs, n_video=120, n_audio=188, seed=7, slice_bytes=200, senc=False):
    """One fragmented-MP4 segment written by hand: ``n_video`` video samples of three NAL units (an
    AUD, an SEI-sized unit and a slice, 4-byte lengths) in track 1 and ``n_audio`` audio samples in
    track 2, spread over ``moofs`` pairs of ``moof`` + ``mdat``, each ``moof`` with one ``traf`` per
    track (``tfhd``, ``tfdt``, one ``trun`` with every per-sample field and a ``data_offset``).
    ``senc``: each ``traf`` also gets a ``senc`` box behind its ``trun``, the video one with a subsample
    per NAL unit (its length and header byte clear), the audio one without subsample tables;
    ``senc="iv8"``: every entry of both also starts with the sample's 8-byte IV (:func:`cenc_iv`)."""
    rng = np.random.default_rng(seed)

    def box(kind, payload):
        return struct.pack(">I4s", 8 + len(payload), kind) + payload

    def full(kind, version, flags, payload):
        return box(kind, struct.pack(">I", (version << 24) | flags) + payload)

    def nal(header, n):
        body = bytes([header]) + rng.integers(1, 256, n, dtype=np.uint8).tobytes()
        return struct.pack(">I", len(body)) + body

    video = [nal(0x09, 1) + nal(0x06, 70) + nal(0x65 if i % 30 == 0 else 0x41, slice_bytes + i % 7)
             for i in range(n_video)]
    audio = [rng.integers(0, 256, 300 + i % 5, dtype=np.uint8).tobytes() for i in range(n_audio)]
    out, vt, at = b"", 90000, 48000
    for k in range(moofs):
        v = video[n_video * k // moofs:n_video * (k + 1) // moofs]
        a = audio[n_audio * k // moofs:n_audio * (k + 1) // moofs]
        v0, a0 = n_video * k // moofs, n_audio * k // moofs

        vsenc = asenc = b""
        if senc:
            iv = (lambda t, i: cenc_iv(t, i)) if senc == "iv8" else (lambda t, i: b"")
            subs = b"".join(iv(0, v0 + i) + struct.pack(">H", 3) + struct.pack(">HIHIHI", 5, 1, 5, 70, 5, len(x) - 86)
                            for i, x in enumerate(v))
            vsenc = full(b"senc", 0, 2, struct.pack(">I", len(v)) + subs)
            asenc = full(b"senc", 0, 0, struct.pack(">I", len(a)) + b"".join(iv(1, a0 + i) for i in range(len(a))))

        def moof(voff, aoff):
            vrows = b"".join(struct.pack(">IIIi", 3000, len(x), 0x02000000 if (v0 + i) % 30 == 0 else 0x01010000,
                                         3000 * ((v0 + i) % 3)) for i, x in enumerate(v))
            arows = b"".join(struct.pack(">IIIi", 1024, len(x), 0x02000000, 0) for x in a)
            trafs = [box(b"traf", full(b"tfhd", 0, 0x020000, struct.pack(">I", tid)) +
                         full(b"tfdt", 1, 0, struct.pack(">Q", time)) +
                         full(b"trun", 0, 0xF01, struct.pack(">Ii", len(rows) // 16, off) + rows) + aux)
                     for tid, time, off, rows, aux in ((1, vt, voff, vrows, vsenc), (2, at, aoff, arows, asenc))]
            return box(b"moof", full(b"mfhd", 0, 0, struct.pack(">I", k + 1)) + b"".join(trafs))

        size = len(moof(0, 0))
        vbytes = b"".join(v)
        out += moof(size + 8, size + 8 + len(vbytes)) + box(b"mdat", vbytes + b"".join(a))
        vt, at = vt + 3000 * len(v), at + 1024 * len(a)
    return out


def mp4_row(moofs, segs, iters, dev):
    """``mp4_demux_batch`` on ``segs`` copies of :func:`mp4_segment`: us per call, after checking the
    totals and segment 0 of the device result against the host implementation."""
    seg = np.frombuffer(mp4_segment(moofs), np.uint8)
    stride = (len(seg) + 255) // 256 * 256
    buf = np.zeros(stride * segs + 256, np.uint8)
    offs, lens = [stride * i for i in range(segs)], [len(seg)] * segs
    for o in offs:
        buf[o:o + len(seg)] = seg
    tracks = (mp4demux.Mp4Track(1, "video", 0x1B, 4), mp4demux.Mp4Track(2, "audio", 0x0F))
    d = torch.from_numpy(buf).to(dev)
    got = mp4demux.mp4_demux_batch(d, offs, lens, tracks)
    host = mp4demux.mp4_demux_batch(torch.from_numpy(buf[:stride + 256].copy()), offs[:1], lens[:1], tracks)
    names = ("minfo", "msamples", "runs", "emsg", "info", "pes", "nal", "au", "aframes", "sinfo")
    assert all(torch.equal(getattr(got, k)[0].cpu(), getattr(host, k)[0]) for k in names), "mp4demux mismatch"
    mi = got.minfo.cpu()
    assert mi[:, 0].sum() == 0 and (mi[:, 1] == moofs).all() and (mi[:, 6] == 120).all() and (mi[:, 12] == 188).all() \
        and (got.sinfo[:, 1].cpu() == 360).all(), "mp4demux totals"
    return round(timed(lambda: mp4demux.mp4_demux_batch(d, offs, lens, tracks), iters), 1)


def packed_segment(seed, n_frames=470, stamp=900000):
    """A packed-audio segment (``docs/PACKEDAUDIO.md``) of about 160 KB: one ID3v2.4 tag whose PRIV frame
    holds the transport stream timestamp, then ``n_frames`` ADTS frames (48 kHz stereo AAC-LC, 7-byte
    headers) of 310 to 370 bytes, about ten seconds at 128 kb/s."""
    rng = np.random.default_rng(seed)
    body = b"com.apple.streaming.transportStreamTimestamp\0" + struct.pack(">Q", stamp + seed)
    out = [b"ID3\x04\0\0" + bytes([0, 0, 0, 10 + len(body)]) + b"PRIV" + bytes([0, 0, 0, len(body)]) + b"\0\0" + body]
    for n in rng.integers(310, 371, n_frames).tolist():
        out.append(bytes([0xFF, 0xF1, 0x4C, 0x80 | (n >> 11), (n >> 3) & 0xFF, ((n & 7) << 5) | 0x1F, 0xFC])
                   + rng.integers(0, 256, n - 7, dtype=np.uint8).tobytes())
    return b"".join(out)


def packed_row(segs, iters, dev):
    """``packed_audio_batch`` on ``segs`` segments of :func:`packed_segment`: us per call of the op, of the
    kernel's two frame walks through the raw binding (LDS tiles, global memory) and of ``copy_segments``
    over the same bytes, after checking the totals and the first and the last segment of both walks
    against the host implementation."""
    data = [np.frombuffer(packed_segment(i), np.uint8) for i in range(segs)]
    lens = [len(x) for x in data]
    stride = (max(lens) + 255) // 256 * 256
    buf = np.zeros(stride * segs + 256, np.uint8)
    offs = [stride * i for i in range(segs)]
    for o, x in zip(offs, data):
        buf[o:o + len(x)] = x
    d = torch.from_numpy(buf).to(dev)
    names = ("info", "pes", "nal", "au", "aframes", "sinfo", "painfo")
    got = packedaudio.packed_audio_batch(d, offs, lens)
    host = packedaudio.packed_audio_batch(torch.from_numpy(buf), offs, lens)
    t = {k: getattr(got, k) for k in names}
    o_d, n_d = (torch.tensor(v, dtype=torch.int64, device=dev) for v in (offs, lens))
    raw = lambda staged: device().packed_audio(d, o_d, n_d, n_d, got.pes.shape[2], *t.values(), staged=staged)  # noqa: E731
    for staged in (True, False):
        for v in t.values():
            v.fill_(-7)
        raw(staged)
        for i in (0, segs - 1):
            assert all(torch.equal(t[k][i].cpu(), getattr(host, k)[i]) for k in names), "packedaudio mismatch"
    pa = host.painfo.numpy()
    assert not pa[:, 0].any() and (pa[:, 4] == 470).all() and (pa[:, 6] == 48000).all(), "packedaudio totals"
    cp = torch.empty_like(d)
    return {"packedaudio_us": round(timed(lambda: packedaudio.packed_audio_batch(d, offs, lens), iters), 1),
            "packedaudio_kernel_us": round(timed(lambda: raw(True), iters), 1),
            "packedaudio_direct_us": round(timed(lambda: raw(False), iters), 1),
            "packedaudio_copy_us": round(timed(lambda: segment.copy_segments(d, cp, offs, offs, lens), iters), 1),
            "packedaudio_bytes": int(sum(lens))}


CBCS_KEY, CBCS_IV = bytes(range(0x40, 0x50)), (bytes(range(0x70, 0x80)), bytes(range(0x90, 0xA0)))


def mp3_frames(n, seed):
    """``n`` MPEG-1 Layer III frames of 128 kbit/s at 44,100 Hz (417 bytes, 418 with the padding bit, which
    47 frames of 49 carry) with random bytes behind the header."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        pad = 1 if i % 49 < 47 else 0
        body = rng.integers(0, 255, 413 + pad, dtype=np.uint8).tobytes()
        out.append(bytes([0xFF, 0xFB, 0x90 | (pad << 1), 0x00]) + body)
    return out


def ac3_frames(n, seed):
    """``n`` AC-3 syncframes of 384 kbit/s at 48,000 Hz, 3/2 + LFE: 1,536 bytes each (payload bytes are
    never 0B, so no syncword forms inside)."""
    rng = np.random.default_rng(seed)
    return [bytes([0x0B, 0x77, 0x5A, 0x5A, 0x1C, 0x40, 0xE1]) + rng.integers(0x10, 256, 1529, dtype=np.uint8).tobytes()
            for _ in range(n)]


def frame_audio_batches(r, caps, dev, atype, make_frames, rate, samples, per_pes):
    """The demuxed batch ``r`` with every segment's AAC track replaced by a track of whole frames
    (``make_frames(n, seed)``, ``samples`` samples at ``rate`` Hz each, PMT type ``atype``) as long as its
    video, ``per_pes`` frames to an audio PES: ``(batch(device, rows) -> (res, rx, caps), frames in all)``
    with ``batch`` indexed and remuxed."""
    info, pes, es = r.info.cpu().numpy().copy(), r.pes.cpu().numpy().copy(), r.es.cpu().numpy()
    I, B, max_pes = tsdemux.INFO, len(caps), pes.shape[2]
    parts, offs2, caps2, pos, frames_total = [], [], [], 0, 0
    for i in range(B):
        row = info[i]
        vb = int(row[I["video_bytes"]])
        span = int(row[I["video_last_pts"]] - row[I["video_first_pts"]])
        n = min(max(1, span * rate // (90000 * samples)), per_pes * max_pes)
        frames = make_frames(n, 100 + i)
        groups = [frames[j:j + per_pes] for j in range(0, n, per_pes)]
        audio, first = b"".join(frames), int(row[I["video_first_pts"]])
        pes[i, 1:] = -1
        at = 0
        for k, g in enumerate(groups):
            stamp = first + k * per_pes * samples * 90000 // rate
            pes[i, 1, k] = (at, stamp, stamp)
            at += sum(map(len, g))
        row[I["audio_type"]], row[I["audio_bytes"]], row[I["n_audio_pes"]] = atype, len(audio), len(groups)
        row[I["audio_es_offset"]], row[I["id3_es_offset"]] = vb, vb + len(audio)
        row[I["id3_bytes"]], row[I["n_id3_pes"]], row[I["payload_bytes"]] = 0, 0, vb + len(audio)
        row[I["audio_first_pts"]], row[I["audio_last_pts"]] = first, int(pes[i, 1, len(groups) - 1, 1])
        o = int(r.es_offs[i])
        seg = es[o:o + vb].tobytes() + audio
        offs2.append(pos)
        caps2.append(len(seg))
        parts.append(seg + bytes(-len(seg) % 256))
        pos += len(parts[-1])
        frames_total += n
    buf = np.frombuffer(b"".join(parts) + bytes(256), np.uint8).copy()
    offs2 = np.asarray(offs2, np.int64)

    def batch(device_, sel):
        res = tsdemux.DemuxResult(torch.from_numpy(info[sel]).to(device_), torch.from_numpy(pes[sel]).to(device_),
                                  torch.from_numpy(buf).to(device_), offs2[sel])
        cp = [caps2[j] for j in sel]
        ix = esindex.index_batch(res, cp)
        oo, size = remux.layout_out(cp, ix.nal.shape[1])
        rx = remux.remux_batch(res, ix, cp, torch.zeros(size, dtype=torch.uint8, device=device_), oo)
        return res, rx, cp

    return batch, frames_total


def mpegaudio_row(r, caps, iters, dev, per_pes=4):
    """``mpeg_audio_batch`` (``docs/MPEGAUDIO.md``) on the demuxed batch ``r`` with every segment's AAC
    track replaced by an MP3 track of 128 kbit/s at 44,100 Hz as long as its video, ``per_pes`` frames to
    an audio PES: us per call of the op behind the remux, after segment 0 was checked against the host."""
    batch, frames_total = frame_audio_batches(r, caps, dev, 0x03, mp3_frames, 44100, 1152, per_pes)
    res, rx, cp = batch(dev, list(range(len(caps))))
    ma = mpegaudio.mpeg_audio_batch(res, rx, cp)
    hres, hrx, hcp = batch("cpu", [0])
    hma = mpegaudio.mpeg_audio_batch(hres, hrx, hcp)
    assert torch.equal(ma.mpainfo[0].cpu(), hma.mpainfo[0]) and torch.equal(ma.mframes[0].cpu(), hma.mframes[0]), \
        "mpegaudio mismatch"
    assert torch.equal(rx.rinfo[0].cpu(), hrx.rinfo[0]) and torch.equal(rx.asamples[0].cpu(), hrx.asamples[0]), \
        "mpegaudio mismatch"
    end = int(hrx.rinfo[0, remux.RINFO["audio_box_offset"]] + 8 + hrx.rinfo[0, remux.RINFO["audio_payload_bytes"]])
    assert torch.equal(rx.out[int(rx.out_offs[0]):int(rx.out_offs[0]) + end].cpu(), hrx.out[:end]), "mpegaudio mismatch"
    mp = ma.mpainfo.cpu().numpy()
    assert not mp[:, 0].any() and int(mp[:, 1].sum()) == frames_total and (mp[:, 2] == 44100).all(), "mpegaudio totals"
    return {"mpegaudio_us": round(timed(lambda: mpegaudio.mpeg_audio_batch(res, rx, cp), iters), 1),
            "mpegaudio_frames": frames_total,
            "mpegaudio_bytes": int(rx.rinfo[:, remux.RINFO["audio_payload_bytes"]].sum().item())}


def ac3audio_row(r, caps, iters, dev, per_pes=4):
    """``ac3_audio_batch`` (``docs/AC3AUDIO.md``) on the demuxed batch ``r`` with every segment's AAC
    track replaced by an AC-3 track of 384 kbit/s at 48,000 Hz as long as its video, ``per_pes`` frames to
    an audio PES: us per call of the op behind the remux, after segment 0 was checked against the host."""
    batch, frames_total = frame_audio_batches(r, caps, dev, 0x81, ac3_frames, 48000, 1536, per_pes)
    res, rx, cp = batch(dev, list(range(len(caps))))
    da = ac3audio.ac3_audio_batch(res, rx, cp)
    hres, hrx, hcp = batch("cpu", [0])
    hda = ac3audio.ac3_audio_batch(hres, hrx, hcp)
    assert torch.equal(da.ac3info[0].cpu(), hda.ac3info[0]) and torch.equal(da.dframes[0].cpu(), hda.dframes[0]) \
        and torch.equal(da.mpainfo[0].cpu(), hda.mpainfo[0]), "ac3audio mismatch"
    assert torch.equal(rx.rinfo[0].cpu(), hrx.rinfo[0]) and torch.equal(rx.asamples[0].cpu(), hrx.asamples[0]), \
        "ac3audio mismatch"
    end = int(hrx.rinfo[0, remux.RINFO["audio_box_offset"]] + 8 + hrx.rinfo[0, remux.RINFO["audio_payload_bytes"]])
    assert torch.equal(rx.out[int(rx.out_offs[0]):int(rx.out_offs[0]) + end].cpu(), hrx.out[:end]), "ac3audio mismatch"
    ai = da.ac3info.cpu().numpy()
    assert not ai[:, 0].any() and int(ai[:, 1].sum()) == frames_total and (ai[:, 2] == 48000).all() \
        and (ai[:, 3] == 6).all() and (ai[:, 7] == 384000).all(), "ac3audio totals"
    return {"ac3audio_us": round(timed(lambda: ac3audio.ac3_audio_batch(res, rx, cp), iters), 1),
            "ac3audio_frames": frames_total,
            "ac3audio_bytes": int(rx.rinfo[:, remux.RINFO["audio_payload_bytes"]].sum().item())}


def cbcs_protect(seg, md):
    """The tool's cbcs packager: ``seg`` (a host array of one :func:`mp4_segment` with ``senc`` boxes,
    changed in place) with one 16-byte block in ten of every video NAL unit behind its header byte and
    every whole block of every audio sample encrypted, a CBC chain per range from the track's
    constant IV.  ``md`` is the segment's host demux.  Returns the cipher blocks written."""
    blocks = 0

    def chain(at, iv):
        nonlocal blocks
        idx = (at[:, None] + np.arange(16)[None, :]).reshape(-1)
        seg[idx] = aes.cbc_encrypt(CBCS_KEY, iv, seg[idx])[:len(idx)]
        blocks += len(at)
    for off, n in md.nal[0, :int(md.sinfo[0, 1]), :2].tolist():
        if n - 1 >= 16:
            chain(off + 1 + 160 * np.arange(((n - 1) // 16 + 9) // 10), CBCS_IV[0])
    for k in range(int(md.minfo[0, 12])):
        off, n = int(md.pes[0, 1, k, 0]), int(md.msamples[0, 1, k, 0])
        if n >= 16:
            chain(off + 16 * np.arange(n // 16), CBCS_IV[1])
    return blocks


def cbcs_row(slice_bytes, segs, iters, dev):
    """``cbcs_decrypt_batch`` on ``segs`` copies of :func:`mp4_segment` protected by the tool, 1:9 video
    with a subsample per NAL unit and 0:0 audio: (us per call, us of ``copy_segments`` over the same
    bytes, cipher blocks per call), after checking segment 0 of the device result against the host
    implementation and against the clear bytes."""
    clear = np.frombuffer(mp4_segment(1, slice_bytes=slice_bytes, senc=True), np.uint8)
    prot = [cbcs.Mp4Protection("cbcs", c, s, 0, iv, bytes(16)) for (c, s), iv in zip(((1, 9), (0, 0)), CBCS_IV)]
    tracks = (mp4demux.Mp4Track(1, "video", 0x1B, 4, protection=prot[0]),
              mp4demux.Mp4Track(2, "audio", 0x0F, protection=prot[1]))
    stride = (len(clear) + 255) // 256 * 256
    one = np.zeros(stride + 256, np.uint8)
    one[:len(clear)] = clear
    hmd = mp4demux.mp4_demux_batch(torch.from_numpy(one), [0], [len(clear)], tracks)
    blocks = cbcs_protect(one, hmd)
    buf = np.zeros(stride * segs + 256, np.uint8)
    offs, lens = [stride * i for i in range(segs)], [len(clear)] * segs
    for o in offs:
        buf[o:o + len(clear)] = one[:len(clear)]
    d = torch.from_numpy(buf).to(dev)
    md = mp4demux.mp4_demux_batch(d, offs, lens, tracks)
    keys = [CBCS_KEY] * segs
    got = cbcs.cbcs_decrypt_batch(md, tracks, keys)
    host = cbcs.cbcs_decrypt_batch(hmd, tracks, keys[:1])
    ci = got.cinfo.cpu()
    assert torch.equal(ci[0], host.cinfo[0]) and torch.equal(got.ranges[0].cpu(), host.ranges[0]), "cbcs mismatch"
    assert ci[:, 0].sum() == 0 and ((ci[:, 4] + ci[:, 5]) == blocks).all() and blocks > 0, "cbcs totals"
    for i in (0, segs - 1):
        mine = got.buf[int(got.offs[i]):int(got.offs[i]) + len(clear)].cpu().numpy()
        assert np.array_equal(mine, host.buf[:len(clear)].numpy()) and np.array_equal(mine, clear), "cbcs bytes"
    assert not np.array_equal(one[:len(clear)], clear), "cbcs packager"
    cp = torch.empty_like(d)
    return (round(timed(lambda: cbcs.cbcs_decrypt_batch(md, tracks, keys), iters), 1),
            round(timed(lambda: segment.copy_segments(d, cp, offs, offs, lens), iters), 1), blocks * segs)


def cenc_iv(track, index):
    """The tool's 8-byte per-sample IV of sample ``index`` of track slot ``track``."""
    return struct.pack(">II", 0xC0DE0000 | track, index)


def cenc_protect(seg, md):
    """The tool's cenc packager: ``seg`` (a host array of one :func:`mp4_segment` with ``senc="iv8"``,
    changed in place) with every NAL unit behind its header byte and every audio sample XORed with
    the sample's AES-CTR keystream (low 64 counter bits, the keystream running on across a sample's
    clear bytes), block by block with the host's forward AES.  Returns the bytes protected."""
    enc, total = runtime().aes_encrypt_block, 0

    def sample(track, index, ranges):
        nonlocal total
        n = sum(z for _, z in ranges)
        iv = cenc_iv(track, index)
        ks = np.frombuffer(b"".join(enc(CBCS_KEY, iv + j.to_bytes(8, "big")) for j in range((n + 15) // 16)), np.uint8)
        p = 0
        for off, z in ranges:
            seg[off:off + z] ^= ks[p:p + z]
            p += z
        total += n
    for k in range(int(md.minfo[0, 6])):
        off, n = int(md.pes[0, 0, k, 0]), int(md.msamples[0, 0, k, 0])
        sample(0, k, [(off + 5, 1), (off + 11, 70), (off + 86, n - 86)])
    for k in range(int(md.minfo[0, 12])):
        sample(1, k, [(int(md.pes[0, 1, k, 0]), int(md.msamples[0, 1, k, 0]))])
    return total


def cenc_row(slice_bytes, segs, iters, dev):
    """``cenc_decrypt_batch`` on ``segs`` copies of the :func:`cbcs_row` segment protected under cenc
    instead (8-byte per-sample IVs, a subsample per NAL unit, audio whole): (us per call, bytes
    protected per call), after checking segment 0 and the last segment of the device result against
    the host implementation and against the clear bytes."""
    clear = np.frombuffer(mp4_segment(1, slice_bytes=slice_bytes, senc="iv8"), np.uint8)
    prot = cenc.Mp4Protection("cenc", 0, 0, 8, b"", bytes(16))
    tracks = (mp4demux.Mp4Track(1, "video", 0x1B, 4, protection=prot),
              mp4demux.Mp4Track(2, "audio", 0x0F, protection=prot))
    stride = (len(clear) + 255) // 256 * 256
    one = np.zeros(stride + 256, np.uint8)
    one[:len(clear)] = clear
    hmd = mp4demux.mp4_demux_batch(torch.from_numpy(one), [0], [len(clear)], tracks)
    nbytes = cenc_protect(one, hmd)
    buf = np.zeros(stride * segs + 256, np.uint8)
    offs, lens = [stride * i for i in range(segs)], [len(clear)] * segs
    for o in offs:
        buf[o:o + len(clear)] = one[:len(clear)]
    d = torch.from_numpy(buf).to(dev)
    md = mp4demux.mp4_demux_batch(d, offs, lens, tracks)
    keys = [CBCS_KEY] * segs
    got = cenc.cenc_decrypt_batch(md, tracks, keys)
    host = cenc.cenc_decrypt_batch(hmd, tracks, keys[:1])
    ci = got.cinfo.cpu()
    for i in (0, segs - 1):
        assert torch.equal(ci[i], host.cinfo[0]) and torch.equal(got.ranges[i].cpu(), host.ranges[0]), "cenc mismatch"
        mine = got.buf[int(got.offs[i]):int(got.offs[i]) + len(clear)].cpu().numpy()
        assert np.array_equal(mine, host.buf[:len(clear)].numpy()) and np.array_equal(mine, clear), "cenc bytes"
    assert ci[:, 0].sum() == 0 and ((ci[:, 4] + ci[:, 5]) == nbytes).all() and nbytes > 0, "cenc totals"
    assert not np.array_equal(one[:len(clear)], clear), "cenc packager"
    return round(timed(lambda: cenc.cenc_decrypt_batch(md, tracks, keys), iters), 1), nbytes * segs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segs", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", choices=["packedaudio", "mpegaudio", "ac3audio"], default=None,
                    help="run that row alone (for a profiler)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    if args.only == "packedaudio":
        print(json.dumps(packed_row(args.segs, args.iters, dev)))
        return
    origin = SyntheticHlsOrigin("http://cdn.kb/", renditions=PRESET_1080P_6M, num_segments=args.segs,
                                encrypted=True, pool_size=args.segs, pin_memory=True, seed=3)
    pool = origin.pools[0]
    offs = [int(o) for o in pool.offsets[:args.segs]]
    lens = [int(n) for n in pool.lengths[:args.segs]]
    src = pool.data.to(dev)
    total = sum(lens)
    keys = [origin.key] * args.segs
    ivs = [origin.iv] * args.segs
    dec = torch.empty_like(src)
    res = {}
    out_len = aes.cbc_decrypt_batch(src, offs, lens, keys, ivs, dec, offs)
    res["aes_us"] = timed(lambda: aes.cbc_decrypt_batch(src, offs, lens, keys, ivs, dec, offs), args.iters)
    # correctness vs host (first segment)
    ref = aes.cbc_decrypt(origin.key, origin.iv, pool.data[offs[0]:offs[0] + lens[0]].numpy())
    assert dec[offs[0]:offs[0] + len(ref)].cpu().numpy().tobytes() == ref.tobytes(), "AES mismatch"
    es = torch.empty_like(src)
    caps = lens
    r = tsdemux.demux_batch(dec, offs, out_len, es, offs, caps=caps)
    res["demux_us"] = timed(lambda: tsdemux.demux_batch(dec, offs, out_len, es, offs, caps=caps), args.iters)
    cpu = tsdemux.demux_batch(torch.from_numpy(ref.copy()), [0], [len(ref)], torch.empty(len(ref) + 256,
                                                                                           dtype=torch.uint8), [0])
    g, c = r.segment(0), cpu.segment(0)
    assert g["video_bytes"] == c["video_bytes"] and torch.equal(g["video"]["es"].cpu(), c["video"]["es"]), \
        "demux mismatch"
    if args.only == "mpegaudio":
        print(json.dumps(mpegaudio_row(r, caps, args.iters, dev)))
        return
    if args.only == "ac3audio":
        print(json.dumps(ac3audio_row(r, caps, args.iters, dev)))
        return
    # the sample index over the ES the demux just wrote (count + prefix + emit + finish)
    ix = esindex.index_batch(r, caps)
    res["esindex_us"] = timed(lambda: esindex.index_batch(r, caps), args.iters)
    hx = esindex.index_batch(cpu, [len(ref)])
    assert all(torch.equal(getattr(ix, k)[0].cpu(), getattr(hx, k)[0]) for k in ("sinfo", "nal", "au", "aframes")), \
        "esindex mismatch"
    # the remux of the indexed ES into mdat boxes and sample tables (plan + copy)
    oo, size = remux.layout_out(caps, ix.nal.shape[1])
    boxes = torch.empty(size, dtype=torch.uint8, device=dev)
    rx = remux.remux_batch(r, ix, caps, boxes, oo)
    res["remux_us"] = timed(lambda: remux.remux_batch(r, ix, caps, boxes, oo), args.iters)
    ho, hsize = remux.layout_out([len(ref)], hx.nal.shape[1])
    hr = remux.remux_batch(cpu, hx, [len(ref)], torch.empty(hsize, dtype=torch.uint8), ho)
    assert all(torch.equal(getattr(rx, k)[0].cpu(), getattr(hr, k)[0]) for k in ("rinfo", "vsamples", "asamples")), \
        "remux mismatch"
    used = int(hr.rinfo[0, remux.RINFO["audio_box_offset"]] + 8 + hr.rinfo[0, remux.RINFO["audio_payload_bytes"]])
    vend = 8 + int(hr.rinfo[0, remux.RINFO["video_payload_bytes"]])
    a0 = int(hr.rinfo[0, remux.RINFO["audio_box_offset"]])
    for lo, hi in ((0, vend), (a0, used)):  # both boxes; the bytes between and behind them belong to nobody
        assert torch.equal(boxes[int(oo[0]) + lo:int(oo[0]) + hi].cpu(), hr.out[lo:hi]), "remux mismatch"
    # the moof boxes of the remuxed batch, written in front of its mdat boxes (one workgroup per
    # segment), next to the host work the call replaces: fmp4.video_moof + fmp4.audio_moof per segment
    # over the same rows, already on the host (the pipeline has them in pinned memory by then)
    head, gap = fragment.frag_headroom(r.pes.shape[2]), fragment.frag_audio_gap(remux.DEFAULT_MAX_AFRAMES)
    fo, fsize = remux.layout_out(caps, ix.nal.shape[1], headroom=head, audio_gap=gap)
    fboxes = torch.empty(fsize, dtype=torch.uint8, device=dev)
    frx = remux.remux_batch(r, ix, caps, fboxes, fo, audio_gap=gap, headroom=head)
    res["remux_gap_us"] = timed(lambda: remux.remux_batch(r, ix, caps, fboxes, fo, audio_gap=gap, headroom=head),
                                args.iters)
    seqs = np.arange(args.segs, dtype=np.int64)
    fr = fragment.fragment_batch(frx, ix, seqs)
    res["fragment_us"] = timed(lambda: fragment.fragment_batch(frx, ix, seqs), args.iters)
    rinfo, vs, asamp = (t.cpu().numpy() for t in (frx.rinfo, frx.vsamples, frx.asamples))
    rates = ix.sinfo.cpu().numpy()[:, esindex.SINFO["audio_sample_rate"]]
    R = remux.RINFO

    def host_moofs():
        out = []
        for i in range(args.segs):
            rows = asamp[i]
            out.append((fmp4.video_moof(int(seqs[i]), int(rinfo[i, R["video_base_dts"]]),
                                        vs[i, :rinfo[i, R["n_vsamples"]]]),
                        fmp4.audio_moof(int(seqs[i]), int(rinfo[i, R["audio_base_pts"]]), int(rates[i]),
                                        rows[rows[:, 0] >= 0])))
        return out

    t0 = time.perf_counter()
    for _ in range(args.iters):
        moofs = host_moofs()
    res["host_moof_us"] = round((time.perf_counter() - t0) / args.iters * 1e6, 1)
    for i in (0, args.segs - 1):
        s = fr.segment(i)
        assert s["video"][:s["video_moof_bytes"]] == moofs[i][0], "fragment mismatch (video)"
        assert s["audio"][:s["audio_moof_bytes"]] == moofs[i][1], "fragment mismatch (audio)"
    # the codec configuration of the indexed ES for the init segments (one workgroup per segment)
    cfg = codecconfig.config_batch(r, ix, caps)
    res["codecconfig_us"] = timed(lambda: codecconfig.config_batch(r, ix, caps), args.iters)
    hc = codecconfig.config_batch(cpu, hx, [len(ref)])
    assert all(torch.equal(getattr(cfg, k)[0].cpu(), getattr(hc, k)[0]) for k in ("cinfo", "ps")), \
        "codecconfig mismatch"
    # the HEVC configuration launched behind it: on this H.264 batch every workgroup exits at once,
    # which is what the launch adds to a remuxFmp4 group ...
    hv = hevcconfig.hevc_config_batch(r, ix, caps)
    res["hevcconfig_us"] = timed(lambda: hevcconfig.hevc_config_batch(r, ix, caps), args.iters)
    hh = hevcconfig.hevc_config_batch(cpu, hx, [len(ref)])
    assert all(torch.equal(getattr(hv, k)[0].cpu(), getattr(hh, k)[0]) for k in ("hinfo", "hps")), \
        "hevcconfig mismatch"
    # ... and with the same bytes declared HEVC and indexed as such: the row search runs over every
    # recorded NAL of a segment that holds no parameter set, the longest path the kernel has
    r24 = tsdemux.DemuxResult(r.info.clone(), r.pes, r.es, r.es_offs)
    r24.info[:, tsdemux.INFO["video_type"]] = 0x24
    ix24 = esindex.index_batch(r24, caps)
    hv = hevcconfig.hevc_config_batch(r24, ix24, caps)
    res["hevcconfig_search_us"] = timed(lambda: hevcconfig.hevc_config_batch(r24, ix24, caps), args.iters)
    cpu24 = tsdemux.DemuxResult(cpu.info.clone(), cpu.pes, cpu.es, cpu.es_offs)
    cpu24.info[:, tsdemux.INFO["video_type"]] = 0x24
    hh = hevcconfig.hevc_config_batch(cpu24, esindex.index_batch(cpu24, [len(ref)]), [len(ref)])
    assert all(torch.equal(getattr(hv, k)[0].cpu(), getattr(hh, k)[0]) for k in ("hinfo", "hps")), \
        "hevcconfig (HEVC) mismatch"
    # the SAMPLE-AES decrypt of the same ES, protected here with the batch's key (plan + decrypt).  The
    # call rewrites es and nal, so every timed call sees protected input again: the restore from
    # device copies runs in front of it, outside the timed interval, and is reported next to it
    skeys, sivs = [origin.key] * args.segs, [origin.iv] * args.segs
    es_host = r.es.cpu().numpy().copy()
    n_blocks = protect_es(es_host, r.es_offs, r.info.cpu().numpy(), r.pes.cpu().numpy(), ix.nal.cpu().numpy(),
                          ix.sinfo.cpu().numpy(), ix.aframes.cpu().numpy(), origin.key, origin.iv)
    es_prot, nal0 = torch.from_numpy(es_host).to(dev), ix.nal.clone()
    rs = tsdemux.DemuxResult(r.info, r.pes, torch.empty_like(es_prot), r.es_offs)
    sx = esindex.EsIndex(torch.empty_like(nal0), ix.au, ix.aframes, ix.sinfo)

    def restore():
        rs.es.copy_(es_prot)
        sx.nal.copy_(nal0)

    decrypt = lambda: sampleaes.sample_decrypt_batch(rs, sx, caps, skeys, sivs)  # noqa: E731
    res["sampleaes_us"] = timed_each(restore, decrypt, args.iters)
    res["sampleaes_restore_us"] = round(timed(restore, args.iters), 1)
    restore()
    sa = sampleaes.sample_decrypt_batch(rs, sx, caps, skeys, sivs)
    res["sampleaes_blocks"] = int(sa.sainfo[:, 3].sum() + sa.sainfo[:, 5].sum())
    assert abs(res["sampleaes_blocks"] - n_blocks) <= 64, "sampleaes block count"
    o0 = int(r.es_offs[0])
    hs = tsdemux.DemuxResult(cpu.info, cpu.pes, torch.from_numpy(es_host[o0:o0 + len(ref) + 256].copy()), cpu.es_offs)
    hsx = esindex.EsIndex(hx.nal.clone(), hx.au, hx.aframes, hx.sinfo)
    hsa = sampleaes.sample_decrypt_batch(hs, hsx, [len(ref)], skeys[:1], sivs[:1])
    assert torch.equal(sa.sainfo[0].cpu(), hsa.sainfo[0]) and torch.equal(sx.nal[0].cpu(), hsx.nal[0]) and \
        torch.equal(rs.es[o0:o0 + len(ref)].cpu(), hs.es[:len(ref)]), "sampleaes mismatch"
    if int(sa.sainfo[0, 2]) == 0:  # no ciphertext looked like emulation prevention: the clear ES is back
        assert torch.equal(rs.es[o0:o0 + len(ref)], r.es[o0:o0 + len(ref)]), "sampleaes does not invert the packager"
    # the caption extraction (scan + pack) on a batch of the tool's own: 120 caption SEI per segment,
    # indexed here; the ES is only read, so the call repeats as it is
    cr, ccaps, hcr = caption_batch_inputs(offs, lens, src.numel(), dev)
    cix = esindex.index_batch(cr, ccaps)
    cc = captions.caption_batch(cr, cix, ccaps)
    res["captions_us"] = round(timed(lambda: captions.caption_batch(cr, cix, ccaps), args.iters), 1)
    res["captions_samples"] = int(cc.ccinfo[:, captions.CCINFO["n_samples"]].sum())
    assert res["captions_samples"] == 120 * args.segs and not int(cc.ccinfo[:, 0].sum()), "captions sample count"
    hcc = captions.caption_batch(hcr, esindex.index_batch(hcr, ccaps[:1]), ccaps[:1])
    assert all(torch.equal(getattr(cc, k)[0].cpu(), getattr(hcc, k)[0])
               for k in ("ccinfo", "ccsamples", "ccpts", "ccbytes", "cc608")), "captions mismatch"
    # the fragmented-MP4 demux (boxes, samples, NAL units) on segments of the tool's own: 120 video and
    # 188 audio samples in one moof + mdat, and the same samples in 30 (the serial top-level chain)
    res["mp4demux_us"] = mp4_row(1, args.segs, args.iters, dev)
    res["mp4demux_chunked_us"] = mp4_row(30, args.segs, args.iters, dev)
    # the cbcs decrypt (copy, plan, a lane per cipher block) of that segment protected by the tool, and of
    # one with 120 video samples of about 23 KB: beside each the batched copy of the same bytes
    res["cbcs_us"], res["cbcs_copy_us"], res["cbcs_blocks"] = cbcs_row(200, args.segs, args.iters, dev)
    res["cbcs_large_us"], res["cbcs_large_copy_us"], res["cbcs_large_blocks"] = cbcs_row(23000, args.segs, args.iters,
                                                                                        dev)
    # the cenc decrypt (copy, plan, the AES-CTR units on the bulk decrypt's LDS image) of the same two
    # segments protected under cenc: every NAL unit behind its header byte and the audio whole
    res["cenc_us"], res["cenc_bytes"] = cenc_row(200, args.segs, args.iters, dev)
    res["cenc_large_us"], res["cenc_large_bytes"] = cenc_row(23000, args.segs, args.iters, dev)
    # the packed-audio demux (tags, the serial frame chain, rows) on 64 segments of the tool's own: about
    # 470 ADTS frames behind one ID3 tag each; beside it the kernel through the raw binding with the chain
    # walked in LDS tiles and in global memory, and the batched copy of the same bytes
    res.update(packed_row(args.segs, args.iters, dev))
    # the MPEG audio remux behind the remux (plan + copy) on the bench's video with an MP3 track in place
    # of the AAC one
    res.update(mpegaudio_row(r, caps, args.iters, dev))
    res.update(ac3audio_row(r, caps, args.iters, dev))
    res["crc_us"] = timed(lambda: crc.crc32_batch(src, offs, lens), args.iters)
    got = crc.crc32_batch(src, offs, lens)[0].cpu().numpy().view(np.uint32)
    assert int(got[0]) == crc.crc32(pool.data[offs[0]:offs[0] + lens[0]].numpy()), "CRC mismatch"
    # byte-moving rooflines on the same bytes: the batched K4 segment copy and torch's copy_
    cp = torch.empty_like(src)
    res["copy_us"] = timed(lambda: segment.copy_segments(src, cp, offs, offs, lens), args.iters)
    assert torch.equal(cp[offs[5]:offs[5] + lens[5]], src[offs[5]:offs[5] + lens[5]]), "copy mismatch"
    res["torch_copy_us"] = timed(lambda: cp.copy_(src), args.iters)
    res["remux_gap_us"], res["fragment_us"] = round(res["remux_gap_us"], 1), round(res["fragment_us"], 1)
    for k in ("aes", "demux", "esindex", "remux", "codecconfig", "hevcconfig", "hevcconfig_search", "sampleaes", "crc",
              "copy", "torch_copy"):
        res[f"{k}_GBps"] = round(total / (res[f"{k}_us"] * 1e-6) / 1e9, 1)
        res[f"{k}_us"] = round(res[f"{k}_us"], 1)
    res["bytes"] = total
    print(json.dumps(res))


if __name__ == "__main__":
    main()
