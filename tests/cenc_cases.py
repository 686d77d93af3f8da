"""``cenc`` (AES-CTR) packager, hand-built batches and an independent sequential reference for
``ops.cenc_decrypt_batch`` (``docs/CENC.md`` holds the rules; this file keeps its own copy of every
one of them on purpose and shares no code with ``ops/csrc``).  The boxes are those of
``cbcs_cases.py`` (``Traf``, ``senc_box``, the ``moof`` builder of its ``protect``); the samples are
encrypted here with the forward AES of ``sampleaes_cases.py``."""
import struct
from contextlib import contextmanager
from dataclasses import replace
from typing import Dict, List, Tuple

import numpy as np

import cbcs_cases as cc
import mp4_cases as mc
import sampleaes_cases as sa
from cbcs_cases import (BAD_SENC, DAMAGED_MASK, DEMUX_DAMAGED, IV_MODES, KID, NO_SENC, OVERLAP, RANGE_OVERFLOW, Batch,
                        Seg, Traf, assert_equal, blob, iv_of, key_of, make, nal_sample)
from hlsjs_p2p_wrapper_amd.ops.mp4demux import Mp4Track

__all__ = ["BAD_SENC", "DEMUX_DAMAGED", "NO_SENC", "OVERLAP", "RANGE_OVERFLOW", "Batch", "Seg", "Traf", "assert_equal",
           "KID", "key_of", "make"]

TILE = 4096  # the units kernel's tile, this file's copy
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33)
NIST_KEY = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")
NIST_IV = bytes.fromhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
# NIST SP 800-38A F.5.1 / F.5.2
NIST_PLAIN = bytes.fromhex("6bc1bee22e409f96e93d7e117393172a" "ae2d8a571e03ac9c9eb76fac45af8e51"
                           "30c81c46a35ce411e5fbc1191a0a52ef" "f69f2445df4f9b17ad2b417be66c3710")
NIST_CIPHER = bytes.fromhex("874d6191b620e3261bef6864990db6ce" "9806f66b7970fdff8617187bb9fffdff"
                            "5ae4df3edbd5d35e5b4f09020db03eab" "1e031dda2fbe03d1792170a0f3009cee")
_CBCS_PROTECT, _CBCS_TRACK_OF, _CBCS_TRAF_IV = cc.protect, cc.track_of, cc.traf_iv


# ------------------------------------------------------------------ the keystream, this file's copy
def counter_block(iv: bytes, j: int) -> bytes:
    """Block j's counter: the IV, padded on the right to 16 bytes, with its last 8 bytes read as a
    big-endian number that j is added to modulo 2^64; the first 8 bytes stay."""
    iv = iv + bytes(16 - len(iv))
    return iv[:8] + ((int.from_bytes(iv[8:], "big") + j) % (1 << 64)).to_bytes(8, "big")


class Keystream:
    """Byte p of the keystream of one sample (blocks are computed once)."""

    def __init__(self, rk, iv: bytes):
        self.rk, self.iv, self.blocks = rk, iv, {}

    def __call__(self, p: int) -> int:
        j = p >> 4
        if j not in self.blocks:
            self.blocks[j] = sa.encrypt_block(self.rk, counter_block(self.iv, j))
        return self.blocks[j][p & 15]


def units(p0: int, length: int) -> int:
    """Keystream blocks that a range of ``length`` >= 1 bytes at stream position ``p0`` touches."""
    return len({(p0 + i) >> 4 for i in range(length)}) if length < 64 else ((p0 + length - 1) >> 4) - (p0 >> 4) + 1


def crypt_sample(data: bytearray, o: int, ranges, rk, iv: bytes, src=None) -> int:
    """XOR the ranges ((offset in the sample, length), ...) of the sample at ``o`` with the sample's
    keystream, which runs on from range to range; reads ``src`` (default ``data``).  Returns the
    number of protected bytes."""
    src, ks, p = data if src is None else src, Keystream(rk, iv), 0
    for off, n in ranges:
        for i in range(n):
            data[o + off + i] = src[o + off + i] ^ ks(p + i)
        p += n
    return p


# ------------------------------------------------------------------ the packager
def traf_iv(t: Traf, seg_iv: bytes, k: int) -> bytes:
    """``cbcs_cases.traf_iv``, but ``t.ivs`` (one per sample) wins for a per-sample mode."""
    if t.ivs and t.iv_mode in ("per8", "per16"):
        return t.ivs[k]
    return _CBCS_TRAF_IV(t, seg_iv, k)


def protect(trafs: List[Traf], key: bytes, seg_iv: bytes = bytes(16), seq: int = 1, front: bytes = b""):
    """``moof`` + ``mdat`` twice, the clear twin and the fragment protected under ``cenc`` (same
    boxes, ``senc`` included), and how many bytes were encrypted."""
    cc.traf_iv = traf_iv  # senc_box writes the IVs it gets from there
    try:
        clear = _CBCS_PROTECT(trafs, key, seg_iv, seq, front)[0]
    finally:
        cc.traf_iv = _CBCS_TRAF_IV
    rk, prot, count = sa.expand_key(key), bytearray(clear), 0
    pos = len(clear) - sum(len(s) for t in trafs for s in t.samples)  # the mdat holds the samples in order
    for t in trafs:
        for k, s in enumerate(t.samples):
            if t.protected:
                rs = cc.sample_ranges(len(s), t.subs[k] if t.subs is not None else None)[0]
                count += crypt_sample(prot, pos, rs, rk, traf_iv(t, seg_iv, k))
            pos += len(s)
    return clear, bytes(prot), count


def track_of(t: Traf, L: int = 4) -> Mp4Track:
    track = _CBCS_TRACK_OF(t, L)
    if track.protection is None:
        return track
    return replace(track, protection=replace(track.protection, scheme="cenc", crypt_byte_block=0, skip_byte_block=0))


@contextmanager
def as_cenc():
    """``cbcs_cases``' case builders package with this file's ``protect`` and ``track_of``."""
    cc.protect, cc.track_of = protect, track_of
    try:
        yield
    finally:
        cc.protect, cc.track_of = _CBCS_PROTECT, _CBCS_TRACK_OF


def _seg(trafs, i, **kw) -> Seg:
    with as_cenc():
        return cc._seg(trafs, i, **kw)


def cenc_init(video=True, audio=True, video_scheme=b"cenc", audio_scheme=b"cenc", video_tenc=None, audio_tenc=None,
              **kw) -> bytes:
    """An init segment with entries protected under ``cenc``: 8-byte per-sample IVs on the video
    track, a constant IV on the audio track."""
    data = mc.init_segment([(1, b"vide", b"avc1"), (2, b"soun", b"mp4a")], **kw)
    if video:
        tb = video_tenc if video_tenc is not None else cc.tenc(version=0, pattern=(0, 0), iv_size=8)
        data = cc.protect_init(data, 0, cc.sinf(b"avc1", scheme=video_scheme, tenc_box=tb))
    if audio:
        tb = audio_tenc if audio_tenc is not None else cc.tenc(version=1, pattern=(0, 0), constant_iv=iv_of(2))
        data = cc.protect_init(data, 1, cc.sinf(b"mp4a", scheme=audio_scheme, tenc_box=tb))
    return data


# ------------------------------------------------------------------ the reference
def ref_segment(S: bytes, demux: dict, prot: np.ndarray, civ: np.ndarray, iv: bytes, key: bytes, max_range: int):
    """One segment: (decrypted bytes, ranges int32[max_range, 8], cinfo int64[8])."""
    S, n = bytes(S), len(S)
    out = bytearray(S)
    ranges, cinfo = np.full((max_range, 8), -1, np.int32), np.zeros(8, np.int64)
    minfo, runs, pes, ms = demux["minfo"], demux["runs"], demux["pes"], demux["msamples"]
    max_pes = pes.shape[1]
    status = DEMUX_DAMAGED if int(minfo[0]) & DAMAGED_MASK else 0
    on = [int(prot[t, 0]) == 1 for t in (0, 1)]
    cinfo[0] = status
    if not any(on):
        return bytes(out), ranges, cinfo
    rec = [min(max(int(minfo[6 + 6 * t]), 0), max_pes) if on[t] else 0 for t in (0, 1)]
    nr = min(max(int(minfo[3]), 0), runs.shape[0])
    ivsz = [int(prot[t, 3]) if int(prot[t, 3]) in (8, 16) else 0 for t in (0, 1)]
    rk = sa.expand_key(key)
    aux: List[Dict[int, Tuple[int, object, int]]] = [dict(), dict()]  # sample -> (entry, subsample count or None, run)

    # the senc of every traf that has a recorded run of a protected track (the cbcs walk)
    n_senc, p, k = 0, 0, 0
    while p < n:
        b = mc._box(S, p, n)
        if b is None:
            break
        typ, hdr, size = b
        if typ == b"moof":
            if k < 256:
                q, mend = p + hdr, p + size
                while q < mend:
                    c = mc._box(S, q, mend)
                    if c is None:
                        break
                    if c[0] == b"traf":
                        body, end = q + c[1], q + c[2]
                        rows = [g for g in range(nr) if runs[g, 1] == k and body < runs[g, 4] <= end]
                        senc, r = None, body
                        while r < end:
                            d = mc._box(S, r, end)
                            if d is None:
                                break
                            if d[0] == b"senc" and senc is None:
                                senc = (r + d[1], r + d[2])
                            r += d[2]
                        slot = int(runs[rows[0], 0]) if rows else -1
                        if rows and on[slot] and senc is not None:
                            n_senc += 1
                            sb, se = senc
                            if se - sb < 8:
                                status |= BAD_SENC
                            else:
                                subs = bool(mc._u(S, sb, 4) & 2)
                                count, e, at = mc._u(S, sb + 4, 4), 0, sb + 8
                                samples = [(g, int(runs[g, 2]) + j) for g in rows for j in range(int(runs[g, 3]))
                                           if int(runs[g, 2]) + j < rec[slot]]
                                for g, smp in samples:
                                    if e >= count:
                                        break
                                    need = ivsz[slot] + (2 if subs else 0)
                                    if se - at < need:
                                        status |= BAD_SENC
                                        break
                                    ns = mc._u(S, at + ivsz[slot], 2) if subs else None
                                    if subs and se - at < need + 6 * ns:
                                        status |= BAD_SENC
                                        break
                                    aux[slot][smp] = (at, ns, g)
                                    at += need + (6 * ns if subs else 0)
                                    e += 1
                    q += c[2]
            k += 1
        p += size

    def placed(t, smp):
        o = min(max(int(pes[t, smp, 0]), 0), n)
        return o, min(max(int(ms[t, smp, 0]), 0), n - o)
    span = {}
    for t in (0, 1):
        for smp, (_, _, g) in aux[t].items():
            o, z = placed(t, smp)
            if z > 0:
                lo, hi = span.get(g, (o, o + z))
                span[g] = (min(lo, o), max(hi, o + z))
    shadow = {g for g in span for f in span if f < g and span[f][0] < span[g][1] and span[g][0] < span[f][1]}

    n_ranges = rank = 0
    for t in (0, 1):
        for smp in range(rec[t]):
            if smp not in aux[t]:
                status |= NO_SENC
                continue
            at, ns, g = aux[t][smp]
            if g in shadow:
                status |= OVERLAP
                continue
            o, z = placed(t, smp)
            sub = at + ivsz[t] + 2
            pairs = None
            if ns is not None:
                pairs = [(mc._u(S, sub + 6 * i, 2), mc._u(S, sub + 6 * i + 2, 4)) for i in range(ns)]
            rs, ok = cc.sample_ranges(z, pairs)
            if not ok:
                status |= BAD_SENC
            if ivsz[t]:
                iv_s = S[at:at + ivsz[t]]
            elif int(prot[t, 4]) in (8, 16):
                iv_s = bytes(civ[t].tolist())
            else:
                iv_s = iv
            ks, p0 = Keystream(rk, iv_s), 0
            for off, P in rs:
                if P >= 1:
                    if n_ranges < max_range:
                        ranges[n_ranges] = (o + off, P, (t << 30) | smp, rank, p0, at if ivsz[t] else -1, 0, 0)
                        for i in range(P):
                            out[o + off + i] = S[o + off + i] ^ ks(p0 + i)
                    n_ranges, rank = n_ranges + 1, rank + units(p0, P)
                p0 += P
            if p0:
                cinfo[2 + t] += 1
                cinfo[4 + t] += p0
    if n_ranges > max_range:
        status |= RANGE_OVERFLOW
    cinfo[0], cinfo[1], cinfo[6], cinfo[7] = status, n_ranges, n_senc, rank
    return bytes(out), ranges, cinfo


_REF_CACHE: dict = {}


def ref_batch(b: Batch):
    """The reference over a batch: (demux tables by name, decrypted bytes per segment or ``None`` for
    a disabled one, ranges, cinfo)."""
    demux = mc.ref_batch(b.buf, b.offs, b.lens, b.tracks, b.limits)
    raw = b.buf.cpu().numpy().tobytes()
    outs, ranges, cinfo = [], [], []
    for i, (o, n) in enumerate(zip(b.offs, b.lens)):
        if b.enable is not None and not b.enable[i]:
            outs.append(None)
            ranges.append(np.full((b.max_range, 8), -1, np.int32))
            cinfo.append(np.zeros(8, np.int64))
            continue
        prot, civ = cc.prot_rows(b.tracks[i])
        rows = {k: v[i] for k, v in demux.items()}
        got = ref_segment(raw[o:o + n], rows, prot, civ, b.ivs[i], b.keys[i], b.max_range)
        outs.append(got[0])
        ranges.append(got[1])
        cinfo.append(got[2])
    shape = (len(b.offs),)
    return (demux, outs, np.stack(ranges) if ranges else np.zeros(shape + (b.max_range, 8), np.int32),
            np.stack(cinfo) if cinfo else np.zeros(shape + (8,), np.int64))


def ref_of(name: str):
    """The reference of the case's batch with its own mask, computed once and only read after."""
    if name not in _REF_CACHE:
        _REF_CACHE[name] = ref_batch(batch(name))
    return _REF_CACHE[name]


# ------------------------------------------------------------------ batches
def case_known():
    """The four blocks of NIST SP 800-38A F.5.1: the literal ciphertext planted as one audio sample
    (not encrypted here), its IV in the senc; and the same through the packager."""
    t = Traf(2, 0, [NIST_PLAIN], (0, 0), None, iv_mode="per16", ivs=[NIST_IV], duration=1024)
    clear, prot, n = protect([t], NIST_KEY)
    assert n == 64
    planted = clear[:len(clear) - 64] + NIST_CIPHER
    tracks = (track_of(t),)
    segs = [Seg(clear, planted, 64, tracks, NIST_KEY, bytes(16)), Seg(clear, prot, 64, tracks, NIST_KEY, bytes(16))]
    return segs, {}, 8


def case_counter():
    """A 16-byte IV whose low half is ff..fe over four blocks (the counter wraps to 0 and the high
    half stays), an 8-byte IV, constant IVs of both sizes and the job's IV."""
    wrap = bytes(range(0x10, 0x18)) + b"\xff" * 7 + b"\xfe"
    a = [blob(64, 1), blob(70, 2)]
    segs = [_seg([Traf(2, 0, a, (0, 0), None, iv_mode="per16", ivs=[wrap, b"\xff" * 16], duration=1024)], 0)]
    for i, mode in enumerate(IV_MODES):
        v = [nal_sample(40 + 16 * k, seed=k) for k in range(4)]
        au = [blob(33 + k, k) for k in range(3)]
        segs.append(_seg([Traf(1, 90000, v, (0, 0), [[(5, len(s) - 5)] for s in v], iv_mode=mode),
                          Traf(2, 48000, au, (0, 0), None, iv_mode=mode, duration=1024)], 1 + i))
    return segs, {}, 64


def residue_samples():
    """Per stream-position residue and per length of ``LENGTHS`` one sample of two subsamples: 2
    clear bytes and ``r`` protected ones, then 1 + (index mod 3) clear bytes and the length
    protected.  Every sample ends with its second range."""
    samples, subs = [], []
    for r in range(16):
        for L in LENGTHS:
            c = 1 + len(samples) % 3
            samples.append(blob(2 + r + c + L, 100 + len(samples)))
            subs.append([(2, r), (c, L)])
    return samples, subs


def case_lengths():
    """``residue_samples`` behind a ``free`` box of 0 to 15 bytes, so every length at every stream
    residue also lies at every file-offset residue; the last range ends with the segment."""
    samples, subs = residue_samples()
    segs = [_seg([Traf(2, 0, samples, (0, 0), subs, iv_mode="per8", duration=1024)], k, front=mc.box("free", bytes(k)))
            for k in range(16)]
    return segs, dict(max_pes=128), 256


STRADDLE = [(3, 1), (2, 2), (1, 3), (4, 4), (2, 5), (1, 6), (3, 7)] * 6


def case_straddles():
    """One sample whose subsamples protect 1 to 7 bytes each with clear bytes between: a keystream
    block spans three or more ranges."""
    n = sum(c + p for c, p in STRADDLE)
    segs = [_seg([Traf(1, 0, [blob(n, 7), blob(n + 5, 8)], (0, 0), [STRADDLE, STRADDLE + [(5, 0)]], iv_mode=mode)], i)
            for i, mode in enumerate(("per16", "const8"))]
    return segs, {}, 128


def case_tiles():
    """One range of ``TILE + 1`` units and ``TILE + 1`` ranges of one unit each."""
    segs = [_seg([Traf(2, 0, [blob(16 * TILE + 1, 1)], (0, 0), None, duration=1024)], 0),
            _seg([Traf(1, 0, [blob(17 * (TILE + 1), 2)], (0, 0), [[(1, 16)] * (TILE + 1)], iv_mode="per8")], 1)]
    return segs, {}, 8192


GRID_SEGMENTS = 300


def case_grid():
    """About 300 tiny segments under three keys, interleaved: more (segment, tile) pairs than the
    device has workgroups."""
    kinds = [_seg([Traf(2, 0, [blob(20, k), blob(33, k + 1)], (0, 0), None, iv_mode="per8", duration=1024)], k)
             for k in range(3)]
    return [kinds[i % 3] for i in range(GRID_SEGMENTS)], dict(max_pes=4, max_nal=4), 4


GRID_MASK = [i % 7 not in (2, 3) for i in range(GRID_SEGMENTS)]


def _recase(name):
    def build():
        with as_cenc():
            return cc.CASES[name]()
    return build


CASES = {"known": case_known, "counter": case_counter, "lengths": case_lengths, "straddles": case_straddles,
         "tiles": case_tiles, "grid": case_grid,
         # the cbcs shapes, re-protected
         "subsamples": _recase("subsamples"), "placement": _recase("placement"), "limits": _recase("limits"),
         "overlap": _recase("overlap"), "damaged": _recase("damaged")}
MASKS = {"grid": GRID_MASK}


def batch(name: str, dev="cpu", enable=None) -> Batch:
    segs, limits, max_range = CASES[name]()
    return make(segs, limits, max_range, MASKS.get(name) if enable is None else enable, dev)


def run(b: Batch, **kw):
    """The batch through ``mp4_demux_batch`` and ``cenc_decrypt_batch`` on the device its buffer is on."""
    from hlsjs_p2p_wrapper_amd.ops import cenc, mp4demux

    md = mp4demux.mp4_demux_batch(b.buf, b.offs, b.lens, b.tracks, **b.limits)
    return md, cenc.cenc_decrypt_batch(md, b.tracks, b.keys, b.ivs, b.enable, **{"max_range": b.max_range, **kw})


def nist_check() -> None:
    """This file's AES and counter rule give the NIST vectors."""
    rk, out = sa.expand_key(NIST_KEY), bytearray(NIST_PLAIN)
    crypt_sample(out, 0, [(0, 64)], rk, NIST_IV)
    assert bytes(out) == NIST_CIPHER, "the tests' AES-CTR misses NIST SP 800-38A F.5.1"
    assert struct.unpack(">QQ", counter_block(b"\x01" * 8 + b"\xff" * 8, 1)) == (0x0101010101010101, 0)
