"""``cbcs`` builders, hand-built batches and an independent sequential reference for
``ops.cbcs_decrypt_batch`` (``docs/CBCS.md`` holds the rules; this file keeps its own copy of every
one of them on purpose and shares no code with ``ops/csrc``).  The packager writes ``senc`` boxes
and encrypts with the AES of ``sampleaes_cases.py``; the box builders and the demux reference are
``mp4_cases.py``'s."""
import struct
from dataclasses import dataclass, field, replace
from typing import List, Optional, Tuple

import numpy as np
import torch

import mp4_cases as mc
import sampleaes_cases as sa
from hlsjs_p2p_wrapper_amd.ops.cbcs import Mp4Protection
from hlsjs_p2p_wrapper_amd.ops.mp4demux import Mp4Track

# status bits and widths, this file's copy
RANGE_OVERFLOW, NO_SENC, BAD_SENC, DEMUX_DAMAGED, OVERLAP = 1, 2, 4, 8, 16
DAMAGED_MASK = mc.BAD_BOX | mc.MOOF_OVERFLOW | mc.EMSG_OVERFLOW | mc.RUN_OVERFLOW | mc.SAMPLE_OVERFLOW | mc.OUT_OF_RANGE
PATTERNS = ((1, 9), (0, 0), (1, 0), (2, 8), (10, 0))
LENGTHS = (0, 15, 16, 17, 31, 32, 159, 160, 161, 175, 176, 177, 191, 192, 336)
# what the rules give for the lengths above, stated here and not computed
BLOCKS_1_9 = (0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3)
BLOCKS_2_8 = (0, 0, 0, 0, 0, 2, 2, 2, 2, 2, 2, 2, 2, 4, 4)  # 336 bytes: two groups of ten blocks and one block more
IV_MODES = ("const16", "const8", "per8", "per16", "fallback")
KID = bytes(range(0x30, 0x40))
KEY = bytes(range(0xA0, 0xB0))


def key_of(i: int) -> bytes:
    return bytes((0x11 * (i + 1) + j) & 0xFF for j in range(16))


def iv_of(i: int, n: int = 16) -> bytes:
    return bytes((0xC0 + 7 * i + 3 * j) & 0xFF for j in range(n))


# ------------------------------------------------------------------ the pattern, this file's copy
def cipher_positions(P: int, c: int, s: int) -> List[int]:
    """Byte offsets of the cipher blocks of a range of P bytes: a loop over the whole blocks; a block
    of a crypt group is encrypted when the whole group fits."""
    nb = P // 16
    if s == 0:
        return [16 * b for b in range(nb)]
    out = []
    for b in range(nb):
        pos = b % (c + s)
        if pos < c and b - pos + c <= nb:
            out.append(16 * b)
    return out


def pad_iv(iv: bytes) -> bytes:
    return iv + bytes(16 - len(iv))


def sample_ranges(z: int, pairs) -> Tuple[List[Tuple[int, int]], bool]:
    """((offset in the sample, length), ...) of a sample of z bytes and whether its table is sound."""
    if pairs is None:
        return [(0, z)], True
    out, q = [], 0
    for clear, prot in pairs:
        if clear > z - q:
            return out, False
        q += clear
        if prot > z - q:
            return out, False
        out.append((q, prot))
        q += prot
    return out, True


def crypt_range(data: bytearray, off: int, P: int, pattern, iv: bytes, rk, decrypt_from=None) -> int:
    """CBC over the cipher blocks of data[off : off + P], the chain starting at ``iv``: encrypts in
    place, or with ``decrypt_from`` (the ciphertext) writes the plaintext.  Returns the block count."""
    chain, n = pad_iv(iv), 0
    for b in cipher_positions(P, *pattern):
        a = off + b
        if decrypt_from is None:
            data[a:a + 16] = chain = sa.encrypt_block(rk, sa._xor(bytes(data[a:a + 16]), chain))
        else:
            c = bytes(decrypt_from[a:a + 16])
            data[a:a + 16] = sa._xor(sa.decrypt_block(rk, c), chain)
            chain = c
        n += 1
    return n


# ------------------------------------------------------------------ the packager
@dataclass
class Traf:
    """One ``traf`` of a protected fragment.  ``subs``: ``None`` (the ``senc`` has no subsample
    tables: every sample is one range) or one list of ``(clear, protected)`` pairs per sample;
    ``iv_mode``: one of ``IV_MODES``; ``senc``: ``"after"`` / ``"before"`` the ``trun``(s) or ``None``;
    ``split``: the first ``trun`` ends in front of that sample; ``sample_count`` / ``cut``: the
    ``senc``'s count field whatever its entries, and bytes taken off its end."""
    tid: int
    time: Optional[int]
    samples: List[bytes]
    pattern: Tuple[int, int] = (1, 9)
    subs: Optional[List[List[Tuple[int, int]]]] = None
    iv_mode: str = "const16"
    senc: Optional[str] = "after"
    split: Optional[int] = None
    sample_count: Optional[int] = None
    cut: int = 0
    protected: bool = True
    duration: int = 3000
    data_offset: Optional[int] = None  # where the samples are said to lie, whatever the layout
    ivs: List[bytes] = field(default_factory=list)


def traf_iv(t: Traf, seg_iv: bytes, k: int) -> bytes:
    if t.iv_mode in ("per8", "per16"):
        return iv_of(1000 * t.tid + k, 8 if t.iv_mode == "per8" else 16)
    return {"const16": iv_of(t.tid), "const8": iv_of(t.tid, 8), "fallback": seg_iv}[t.iv_mode]


def senc_box(t: Traf, seg_iv: bytes) -> bytes:
    body = struct.pack(">I", len(t.samples) if t.sample_count is None else t.sample_count)
    for k in range(len(t.samples)):
        if t.iv_mode in ("per8", "per16"):
            body += traf_iv(t, seg_iv, k)
        if t.subs is not None:
            body += struct.pack(">H", len(t.subs[k])) + b"".join(struct.pack(">HI", c, p) for c, p in t.subs[k])
    return mc.full_box("senc", 0, 2 if t.subs is not None else 0, body[:len(body) - t.cut])


def protect(trafs: List[Traf], key: bytes, seg_iv: bytes = bytes(16), seq: int = 1, front: bytes = b""):
    """``moof`` + ``mdat`` twice: the clear twin and the protected fragment (same boxes, ``senc``
    included; only sample bytes differ), and how many cipher blocks were written."""
    rk = sa.expand_key(key)

    def build(offsets):
        kids = [mc.mfhd(seq)]
        for t, off in zip(trafs, offsets):
            entries = [(t.duration, len(s), 0x02000000 if k == 0 else 0x01010000, 0) for k, s in enumerate(t.samples)]
            off = off if t.data_offset is None else t.data_offset
            if t.split is None:
                truns = mc.trun(entries, data_offset=off)
            else:
                truns = mc.trun(entries[:t.split], data_offset=off) + mc.trun(entries[t.split:])
            senc = senc_box(t, seg_iv) if t.protected and t.senc else b""
            kids.append(mc.box("traf", mc.tfhd(t.tid) + (mc.tfdt(t.time) if t.time is not None else b"") +
                               (senc if t.senc == "before" else b"") + truns + (senc if t.senc == "after" else b"")))
        return mc.box("moof", b"".join(kids))
    size = len(build([0] * len(trafs)))
    offsets, pos = [], size + 8
    for t in trafs:
        offsets.append(pos)
        pos += sum(len(s) for s in t.samples)
    moof, blocks = build(offsets), 0
    clear, prot = bytearray(), bytearray()
    for t in trafs:
        for k, s in enumerate(t.samples):
            e = bytearray(s)
            if t.protected:
                for off, P in sample_ranges(len(s), t.subs[k] if t.subs is not None else None)[0]:
                    blocks += crypt_range(e, off, P, t.pattern, traf_iv(t, seg_iv, k), rk)
            clear += s
            prot += e
    return (front + moof + mc.box("mdat", bytes(clear)), front + moof + mc.box("mdat", bytes(prot)), blocks)


def track_of(t: Traf, L: int = 4) -> Mp4Track:
    """The ``Mp4Track`` an init segment for this traf's track would give."""
    p = None
    if t.protected:
        per = {"per8": 8, "per16": 16}.get(t.iv_mode, 0)
        const = {"const16": iv_of(t.tid), "const8": iv_of(t.tid, 8)}.get(t.iv_mode, b"")
        p = Mp4Protection("cbcs", t.pattern[0], t.pattern[1], per, const, KID)
    if t.tid == 1:
        return Mp4Track(t.tid, "video", 0x1B, L, protection=p)
    return Mp4Track(t.tid, "audio", 0x0F, protection=p)


# ------------------------------------------------------------------ init segments
def tenc(version=1, pattern=(1, 9), is_protected=1, iv_size=0, constant_iv=iv_of(1), kid=KID, cut=0):
    body = bytes([0, (pattern[0] << 4 | pattern[1]) if version else 0, is_protected, iv_size]) + kid
    if is_protected == 1 and iv_size == 0:
        body += bytes([len(constant_iv)]) + constant_iv
    return mc.full_box("tenc", version, 0, body[:len(body) - cut])


def sinf(original: bytes, scheme=b"cbcs", tenc_box=None, drop=()):
    """A ``sinf``; ``drop`` names the children to leave out (``frma``, ``schm``, ``schi``, ``tenc``)."""
    tenc_box = tenc() if tenc_box is None else tenc_box
    kids = {"frma": mc.box("frma", original), "schm": mc.full_box("schm", 0, 0, scheme + struct.pack(">I", 0x10000)),
            "schi": mc.box("schi", b"" if "tenc" in drop else tenc_box)}
    return mc.box("sinf", b"".join(v for k, v in kids.items() if k not in drop))


def _rewrite(blob: bytes, path, fn) -> bytes:
    """``blob`` is a box; the box at ``path`` (``(type, nth)`` per level) below it becomes ``fn(box)``
    and every ancestor's size follows."""
    if not path:
        return fn(blob)
    typ, nth = path[0]
    out, p, seen = bytearray(), 8, 0
    while p < len(blob):
        size = int.from_bytes(blob[p:p + 4], "big")
        child = blob[p:p + size]
        if child[4:8] == typ:
            if seen == nth:
                child = _rewrite(child, path[1:], fn)
            seen += 1
        out += child
        p += size
    return struct.pack(">I4s", 8 + len(out), blob[4:8]) + bytes(out)


def protect_init(data: bytes, track: int, sinf_box: bytes) -> bytes:
    """The init segment with the sample entry of ``trak`` number ``track`` turned into ``encv`` /
    ``enca`` and ``sinf_box`` appended to it."""
    def at_stsd(stsd):
        e = stsd[16:]
        name = b"encv" if e[4:8] in (b"avc1", b"avc3", b"hvc1", b"hev1") else b"enca"
        e = struct.pack(">I4s", len(e) + len(sinf_box), name) + e[8:] + sinf_box
        return struct.pack(">I4s", 16 + len(e), b"stsd") + stsd[8:16] + e
    path = [(b"moov", 0), (b"trak", track), (b"mdia", 0), (b"minf", 0), (b"stbl", 0), (b"stsd", 0)]
    return _rewrite(struct.pack(">I4s", 8 + len(data), b"root") + data, path, at_stsd)[8:]


def cbcs_init(video=True, audio=True, video_tenc=None, audio_tenc=None, entry=b"avc1", **kw):
    """An init segment with a protected video and / or audio entry."""
    data = mc.init_segment([(1, b"vide", entry), (2, b"soun", b"mp4a")], **kw)
    if video:
        data = protect_init(data, 0, sinf(entry, tenc_box=video_tenc))
    if audio:
        data = protect_init(data, 1, sinf(b"mp4a", tenc_box=audio_tenc if audio_tenc is not None
                                          else tenc(pattern=(0, 0), constant_iv=iv_of(2))))
    return data


# ------------------------------------------------------------------ the reference
def prot_rows(tracks) -> Tuple[np.ndarray, np.ndarray]:
    """This file's own ``int64[2, 8]`` protection rows and ``uint8[2, 16]`` constant IVs."""
    rows, civ = np.zeros((2, 8), np.int64), np.zeros((2, 16), np.uint8)
    for t in tracks:
        if t.protection is None:
            continue
        p, slot = t.protection, {"video": 0, "audio": 1}[t.kind]
        const = p.constant_iv if p.per_sample_iv_size == 0 else b""
        rows[slot, :5] = (1, p.crypt_byte_block, p.skip_byte_block, p.per_sample_iv_size, len(const))
        civ[slot, :len(const)] = list(const)
    return rows, civ


def ref_segment(S: bytes, demux: dict, prot: np.ndarray, civ: np.ndarray, iv: bytes, key: bytes, max_range: int):
    """One segment: (decrypted bytes, ranges int32[max_range, 4], cinfo int64[8]).  ``demux`` is
    ``mp4_cases.ref_segment``'s result for ``S``."""
    S, n = bytes(S), len(S)
    out = bytearray(S)
    ranges, cinfo = np.full((max_range, 4), -1, np.int32), np.zeros(8, np.int64)
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
    aux = [dict(), dict()]  # sample -> (entry offset, subsample count or None, run row)

    # the senc of every traf that has a recorded run of a protected track
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
    # a run that shares bytes with a run in front of it is left alone
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
        pattern = (int(prot[t, 1]), int(prot[t, 2]))
        if pattern[0] <= 0 or pattern[1] <= 0:
            pattern = (1, 0)  # every block
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
            rs, ok = sample_ranges(z, pairs)
            if not ok:
                status |= BAD_SENC
            if ivsz[t]:
                iv_s = S[at:at + ivsz[t]]
            elif int(prot[t, 4]) in (8, 16):
                iv_s = bytes(civ[t].tolist())
            else:
                iv_s = iv
            blocks = 0
            for off, P in rs:
                nb = len(cipher_positions(P, *pattern))
                if nb == 0:
                    continue
                if n_ranges < max_range:
                    ranges[n_ranges] = (o + off, P, (t << 30) | smp, rank)
                    crypt_range(out, o + off, P, pattern, iv_s, rk, decrypt_from=S)
                n_ranges, rank, blocks = n_ranges + 1, rank + nb, blocks + nb
            if blocks:
                cinfo[2 + t] += 1
                cinfo[4 + t] += blocks
    if n_ranges > max_range:
        status |= RANGE_OVERFLOW
    cinfo[0], cinfo[1], cinfo[6] = status, n_ranges, n_senc
    return bytes(out), ranges, cinfo


# ------------------------------------------------------------------ batches
@dataclass
class Seg:
    clear: Optional[bytes]  # the clear twin where the segment is well-formed
    prot: bytes
    blocks: int             # cipher blocks the packager wrote
    tracks: tuple
    key: bytes
    iv: bytes               # the playlist's IV: for a track without one of its own


@dataclass
class Batch:
    buf: torch.Tensor
    offs: List[int]
    lens: List[int]
    tracks: list           # one track set per segment
    keys: List[bytes]
    ivs: List[bytes]
    enable: Optional[List[bool]]
    limits: dict
    max_range: int
    clear: List[Optional[bytes]]  # the clear twin where the segment is well-formed
    blocks: List[int]             # cipher blocks the packager wrote


def make(segments, limits=None, max_range=64, enable=None, dev="cpu") -> Batch:
    raw, offs, lens = mc.layout([s.prot for s in segments])
    buf = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev)
    return Batch(buf, offs, lens, [s.tracks for s in segments], [s.key for s in segments], [s.iv for s in segments],
                 enable,
                 {**mc.LIMITS, **dict(max_pes=64, max_nal=256), **(limits or {})}, max_range,
                 [s.clear for s in segments], [s.blocks for s in segments])


def ref_batch(b: Batch):
    """The reference over a batch: (demux tables by name, decrypted bytes per segment or ``None`` for
    a disabled one, ranges, cinfo)."""
    demux = mc.ref_batch(b.buf, b.offs, b.lens, b.tracks, b.limits)
    raw = b.buf.cpu().numpy().tobytes()
    outs, ranges, cinfo = [], [], []
    for i, (o, n) in enumerate(zip(b.offs, b.lens)):
        if b.enable is not None and not b.enable[i]:
            outs.append(None)
            ranges.append(np.full((b.max_range, 4), -1, np.int32))
            cinfo.append(np.zeros(8, np.int64))
            continue
        prot, civ = prot_rows(b.tracks[i])
        rows = {k: v[i] for k, v in demux.items()}
        got = ref_segment(raw[o:o + n], rows, prot, civ, b.ivs[i], b.keys[i], b.max_range)
        outs.append(got[0])
        ranges.append(got[1])
        cinfo.append(got[2])
    shape = (len(b.offs),)
    return (demux, outs, np.stack(ranges) if ranges else np.zeros(shape + (b.max_range, 4), np.int32),
            np.stack(cinfo) if cinfo else np.zeros(shape + (8,), np.int64))


def nal_sample(payload: int, seed: int = 0, typ: int = 1) -> bytes:
    """One length-prefixed NAL unit: 4 length bytes, the header byte and ``payload`` more."""
    rng = np.random.default_rng(1000 + seed)
    return mc.length_prefixed([mc.nal(typ, rng.integers(0, 256, payload, dtype=np.uint8).tobytes())])


def blob(n: int, seed: int = 0) -> bytes:
    return np.random.default_rng(2000 + seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _seg(trafs, i, **kw):
    """A segment from its trafs, packaged with key and playlist IV number ``i``."""
    clear, prot, blocks = protect(trafs, key_of(i), iv_of(50 + i), **kw)
    return Seg(clear, prot, blocks, tuple(track_of(t) for t in trafs), key_of(i), iv_of(50 + i))


def case_patterns():
    """Per pattern one segment: a video sample per length of ``LENGTHS`` with one subsample (5 clear
    bytes, the length protected) and an audio traf of whole-sample ranges of the same lengths."""
    segs = []
    for i, pattern in enumerate(PATTERNS):
        v = [nal_sample(n, seed=n) for n in LENGTHS]
        a = [blob(n, seed=n) for n in LENGTHS]
        segs.append(_seg([Traf(1, 0, v, pattern, [[(5, n)] for n in LENGTHS]),
                          Traf(2, 0, a, pattern, None, duration=1024)], i))
    return segs, {}, 64


def case_ivs():
    segs = []
    for i, mode in enumerate(IV_MODES):
        v = [nal_sample(40 + 16 * k, seed=k) for k in range(4)]
        a = [blob(33 + k, k) for k in range(3)]
        segs.append(_seg([Traf(1, 90000, v, (1, 9), [[(5, len(s) - 5)] for s in v], iv_mode=mode),
                          Traf(2, 48000, a, (0, 0), None, iv_mode=mode, duration=1024)], i))
    return segs, {}, 64


def case_subsamples():
    v = [mc.length_prefixed([mc.nal(6, blob(20, k)), mc.nal(1, blob(70 + k, k + 9))]) for k in range(4)]
    per_nal = [[(5, 20), (5, len(s) - 30)] for s in v]
    tables = {
        "flag unset": None,
        "one": [[(5, len(s) - 5)] for s in v],
        "several": per_nal,
        "count 0": [[] for _ in v],
        "clear only": [[(len(s), 0)] for s in v],
        "short of the sample": [[(5, 32)] for s in v],
        "mixed": [[(5, 20), (5, len(v[0]) - 30)], [], [(len(v[2]), 0)], [(0, 16), (1, 16), (2, 16)]],
        "clear beyond the sample": [per_nal[0], [(5, 20), (len(v[1]), 16)], per_nal[2], per_nal[3]],
        "protected beyond the sample": [per_nal[0], per_nal[1], [(5, 20), (5, len(v[2]))], per_nal[3]],
    }
    segs = [_seg([Traf(1, 0, v, (1, 9), t, iv_mode="per8")], i) for i, t in enumerate(tables.values())]
    sound = len(segs) - 2
    i = len(segs)
    for cut in (1, 6, 7, 14, 8 + 8 + 2 + 12 + 1):  # the senc cut inside its last and inside an earlier entry
        segs.append(_seg([Traf(1, 0, v, (1, 9), per_nal, iv_mode="per8", cut=cut)], i))
        i += 1
    segs.append(_seg([Traf(1, 0, v, (1, 9), per_nal, cut=4 * (2 + 12) + 1)], i))  # the fixed fields cut
    for count in (0, 2, 9, 0xFFFFFFFF):  # sample_count below and above the traf's samples
        segs.append(_seg([Traf(1, 0, v, (1, 9), per_nal, iv_mode="per16", sample_count=count)], i + 1))
        i += 1
    segs.append(_seg([Traf(1, 0, v, (1, 9), per_nal, senc=None)], i + 1))  # no senc at all
    # only the first `sound` segments decrypt to their clear twins
    return [s if k < sound else replace(s, clear=None) for k, s in enumerate(segs)], {}, 64


def case_placement():
    v = [nal_sample(60 + 3 * k, seed=k) for k in range(6)]
    subs = [[(5, len(s) - 5)] for s in v]
    a = [blob(40 + k, k) for k in range(5)]
    segs = [_seg([Traf(1, 0, v, (1, 9), subs, senc="before")], 0),
            _seg([Traf(1, 0, v, (1, 9), subs, senc="after", iv_mode="per16")], 1),
            _seg([Traf(1, 0, v, (1, 9), subs, split=2, iv_mode="per8")], 2),
            _seg([Traf(1, 0, v, (1, 9), subs, split=0)], 3),
            _seg([Traf(1, 0, v, (1, 9), subs, iv_mode="per8"), Traf(2, 0, a, (0, 0), None, duration=1024)], 4),
            _seg([Traf(2, 0, a, (1, 0), None, duration=1024), Traf(1, 0, v, (1, 9), subs, senc="before")], 5),
            _seg([Traf(1, 0, v, (1, 9), subs), Traf(2, 0, a, (0, 0), None, protected=False)], 6)]
    # three moofs: video, audio and video again, each with its own mdat
    parts = [protect([Traf(1, 0, v[:3], (1, 9), subs[:3], iv_mode="per8")], key_of(7), iv_of(57), seq=1),
             protect([Traf(2, 0, a, (0, 0), None, duration=1024)], key_of(7), iv_of(57), seq=2),
             protect([Traf(1, None, v[3:], (1, 9), subs[3:], iv_mode="per8")], key_of(7), iv_of(57), seq=3)]
    tracks = (track_of(Traf(1, 0, [], iv_mode="per8")), track_of(Traf(2, 0, [], (0, 0))))
    segs.append(Seg(b"".join(p[0] for p in parts), b"".join(p[1] for p in parts), sum(p[2] for p in parts), tracks,
                    key_of(7), iv_of(57)))
    segs.append(_seg([Traf(1, 0, v, (1, 9), subs)], 8, front=mc.box("styp", b"msdh" + bytes(4) + b"msdhmsix")))
    return segs, {}, 64


def case_alignment():
    """33 whole-sample ranges of 17 bytes, so a cipher block at every offset mod 16, and a last
    sample of 32 bytes whose second block ends with the segment."""
    a = [blob(17, k) for k in range(33)] + [blob(32, 99)]
    segs = [_seg([Traf(2, 0, a, (1, 0), None, duration=1024)], 0, front=mc.box("free", bytes(k))) for k in (0, 1, 2, 3)]
    v = [nal_sample(27 + k, seed=k) for k in range(20)]
    segs.append(_seg([Traf(1, 0, v, (1, 9), [[(5, len(s) - 5)] for s in v], iv_mode="per16")], 4))
    return segs, {}, 64


def case_tiles():
    """One 0:0 range of 600 blocks (two tile borders inside it), 300 ranges of one block each in
    300 samples (a second round of samples too) and 300 ranges in one sample."""
    one = blob(16 * 300 + 300, 5)
    segs = [_seg([Traf(2, 0, [blob(9600, 1)], (0, 0), None, duration=1024)], 0),
            _seg([Traf(2, 0, [blob(16, k) for k in range(300)], (1, 0), None, duration=1024, iv_mode="per8")], 1),
            _seg([Traf(1, 0, [one], (1, 9), [[(1, 16)] * 300])], 2)]
    return segs, dict(max_pes=512), 512


def case_limits():
    v = [nal_sample(60 + 3 * k, seed=k) for k in range(6)]
    subs = [[(5, len(s) - 5)] for s in v]
    return [replace(_seg([Traf(1, 0, v, (1, 9), subs)], i), clear=None) for i in range(3)], {}, 4


def case_overlap():
    """Two trafs whose runs are said to lie on the same bytes: the second is left encrypted."""
    a = [blob(48, k) for k in range(2)]
    two = [Traf(2, 0, a, (0, 0), None, duration=1024), Traf(2, 5000, a, (0, 0), None, duration=1024)]
    apart = _seg(two, 0)
    moof = struct.unpack(">I", apart.prot[:4])[0]
    two[1].data_offset = moof + 8 + 16  # inside the first traf's samples
    one = apart.tracks[:1]  # the two trafs are of one track
    return [replace(_seg(two, 1), clear=None, tracks=one), replace(apart, tracks=one)], {}, 64


def case_damaged():
    """Seeded valid segments with one or two bytes overwritten inside the ``moof``."""
    rng = np.random.default_rng(4242)
    good = case_placement()[0][4:8] + case_subsamples()[0][2:3] + case_ivs()[0][2:4]
    segs = []
    for k in range(56):
        g = good[k % len(good)]
        s = bytearray(g.prot)
        end = s.index(b"mdat") - 4
        for _ in range(1 + k % 2):
            s[int(rng.integers(0, end))] = int(rng.integers(0, 256))
        segs.append(replace(g, clear=None, prot=bytes(s)))
    return segs, dict(max_pes=16, max_nal=64), 16


CASES = {"patterns": case_patterns, "ivs": case_ivs, "subsamples": case_subsamples, "placement": case_placement,
         "alignment": case_alignment, "tiles": case_tiles, "limits": case_limits, "overlap": case_overlap,
         "damaged": case_damaged}


def batch(name: str, dev="cpu", enable=None) -> Batch:
    segs, limits, max_range = CASES[name]()
    return make(segs, limits, max_range, enable, dev)


def run(b: Batch, **kw):
    """The batch through ``mp4_demux_batch`` and ``cbcs_decrypt_batch`` on the device its buffer is on."""
    from hlsjs_p2p_wrapper_amd.ops import cbcs, mp4demux

    md = mp4demux.mp4_demux_batch(b.buf, b.offs, b.lens, b.tracks, **b.limits)
    return md, cbcs.cbcs_decrypt_batch(md, b.tracks, b.keys, b.ivs, b.enable, **{"max_range": b.max_range, **kw})


def assert_equal(b: Batch, cb, ref) -> None:
    """``cb`` (a ``Cbcs``) equals the reference bit for bit: the bytes of every enabled segment,
    ``ranges`` and ``cinfo``; a disabled segment has ``offs -1``."""
    _, outs, ranges, cinfo = ref
    got_c, got_r = cb.cinfo.cpu().numpy(), cb.ranges.cpu().numpy()
    assert got_c.shape == cinfo.shape and got_c.dtype == cinfo.dtype and got_r.shape == ranges.shape \
        and got_r.dtype == ranges.dtype
    for name, g, r in (("cinfo", got_c, cinfo), ("ranges", got_r, ranges)):
        if not np.array_equal(g, r):
            bad = np.argwhere(g != r)[0]
            raise AssertionError(f"{name}{tuple(bad)}: got {g[tuple(bad)]}, reference {r[tuple(bad)]}")
    raw = cb.buf.cpu().numpy()
    for i, want in enumerate(outs):
        if want is None:
            assert cb.offs[i] == -1, i
            continue
        o = int(cb.offs[i])
        assert o >= 0 and o % 16 == 0
        got = raw[o:o + len(want)].tobytes()
        if got != want:
            at = next(k for k in range(len(want)) if got[k] != want[k])
            raise AssertionError(f"segment {i} differs from the reference at byte {at} of {len(want)}")
