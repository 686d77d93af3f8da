"""Hand-built inputs, the packager and the reference for the SAMPLE-AES tests (``test_sampleaes.py``
on the host implementation, ``test_sampleaes_gpu.py`` on the kernel).

Everything here follows ``docs/SAMPLEAES.md`` with plain Python loops and shares no code with
``runtime/sampleaes.cpp`` or ``kernels/sample_aes.hip``: its own AES-128 (tables derived from
GF(2^8) arithmetic, pinned by the FIPS-197 appendix C.1 vector), its own escape / unescape, its own
block rules.  :func:`protect` is the packager: clear NAL units and ADTS frames in, the protected
twin out.  Batches are built as ``remux_cases`` builds them.
"""
from __future__ import annotations

import numpy as np
import torch

from hlsjs_p2p_wrapper_amd.ops import esindex, tsdemux
from remux_cases import adts_frame, annexb, background, hand_batch, seg

INFO = tsdemux.INFO
ROUND = 4096  # sample_aes_round_bytes(); the tests assert the kernel's own value equals it
SA_WORDS = 6
TRUNCATED, UNSUPPORTED_VIDEO, UNSUPPORTED_AUDIO, PARTIAL_AUDIO = 1, 2, 4, 8


# ---------------------------------------------------------------- AES-128, a second copy
def _xtime(a: int) -> int:
    a <<= 1
    return (a ^ 0x11B) & 0xFF if a & 0x100 else a


def _gmul(a: int, b: int) -> int:
    p = 0
    while b:
        if b & 1:
            p ^= a
        a = _xtime(a)
        b >>= 1
    return p


def _tables():
    inv = [0] * 256
    for a in range(1, 256):
        if not inv[a]:
            for b in range(1, 256):
                if _gmul(a, b) == 1:
                    inv[a], inv[b] = b, a
                    break
    sbox = [0] * 256
    for x in range(256):
        b = inv[x]
        s = b
        for i in range(1, 5):
            s ^= ((b << i) | (b >> (8 - i))) & 0xFF
        sbox[x] = s ^ 0x63
    isbox = [0] * 256
    for x, s in enumerate(sbox):
        isbox[s] = x
    return sbox, isbox


SBOX, ISBOX = _tables()
_MUL = {k: [_gmul(x, k) for x in range(256)] for k in (2, 3, 9, 11, 13, 14)}


def expand_key(key: bytes):
    w = [list(key[4 * i:4 * i + 4]) for i in range(4)]
    rcon = 1
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = [SBOX[t[1]] ^ rcon, SBOX[t[2]], SBOX[t[3]], SBOX[t[0]]]
            rcon = _xtime(rcon)
        w.append([a ^ b for a, b in zip(w[i - 4], t)])
    return [sum(w[4 * r:4 * r + 4], []) for r in range(11)]  # 11 round keys of 16 bytes, column-major


def _shift(s, inverse=False):
    # state byte 4 c + r is row r of column c
    return [s[4 * ((c + (-r if inverse else r)) % 4) + r] for c in range(4) for r in range(4)]


def encrypt_block(rk, block: bytes) -> bytes:
    s = [a ^ b for a, b in zip(block, rk[0])]
    for rnd in range(1, 11):
        s = _shift([SBOX[x] for x in s])
        if rnd < 10:
            m2, m3 = _MUL[2], _MUL[3]
            t = []
            for c in range(4):
                a0, a1, a2, a3 = s[4 * c:4 * c + 4]
                t += [m2[a0] ^ m3[a1] ^ a2 ^ a3, a0 ^ m2[a1] ^ m3[a2] ^ a3, a0 ^ a1 ^ m2[a2] ^ m3[a3],
                      m3[a0] ^ a1 ^ a2 ^ m2[a3]]
            s = t
        s = [a ^ b for a, b in zip(s, rk[rnd])]
    return bytes(s)


def decrypt_block(rk, block: bytes) -> bytes:
    s = [a ^ b for a, b in zip(block, rk[10])]
    for rnd in range(9, -1, -1):
        s = [ISBOX[x] for x in _shift(s, inverse=True)]
        s = [a ^ b for a, b in zip(s, rk[rnd])]
        if rnd > 0:
            m9, m11, m13, m14 = _MUL[9], _MUL[11], _MUL[13], _MUL[14]
            t = []
            for c in range(4):
                a0, a1, a2, a3 = s[4 * c:4 * c + 4]
                t += [m14[a0] ^ m11[a1] ^ m13[a2] ^ m9[a3], m9[a0] ^ m14[a1] ^ m11[a2] ^ m13[a3],
                      m13[a0] ^ m9[a1] ^ m14[a2] ^ m11[a3], m11[a0] ^ m13[a1] ^ m9[a2] ^ m14[a3]]
            s = t
    return bytes(s)


def _xor(a: bytes, b: bytes) -> bytes:
    return bytes(x ^ y for x, y in zip(a, b))


# ---------------------------------------------------------------- the byte rules, a second copy
def escape(u: bytes) -> bytes:
    """Start-code emulation prevention: ``03`` in front of any byte <= 3 that follows two zeros."""
    out, zeros = bytearray(), 0
    for b in u:
        if zeros >= 2 and b <= 3:
            out.append(3)
            zeros = 0
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def unescape(raw: bytes) -> bytes:
    return bytes(b for j, b in enumerate(raw) if not (j >= 2 and b == 3 and raw[j - 1] == 0 and raw[j - 2] == 0))


def inserted(u: bytes):
    """Raw offsets of the ``03`` bytes :func:`escape` inserts into ``u``."""
    raw = escape(u)
    return [j for j in range(2, len(raw)) if raw[j] == 3 and raw[j - 1] == 0 and raw[j - 2] == 0]


def video_blocks(u: int):
    """Offsets of the cipher blocks of a protected NAL of ``u`` unescaped bytes."""
    return [c for c in range(32, max(u, 0), 160) if c + 16 < u]


def audio_blocks(frame_len: int, header: int):
    payload = frame_len - header
    nb = (payload - 16) // 16 if payload >= 32 else 0
    return [header + 16 + 16 * j for j in range(nb)]


def nal_protected(u: bytes) -> bool:
    return len(u) > 48 and (u[0] & 0x1F) in (1, 5)


# ---------------------------------------------------------------- the packager
def encrypt_nal(u: bytes, rk, iv: bytes) -> bytes:
    out, chain = bytearray(u), iv
    for c in video_blocks(len(u)):
        chain = encrypt_block(rk, _xor(u[c:c + 16], chain))
        out[c:c + 16] = chain
    return bytes(out)


def encrypt_frame(frame: bytes, rk, iv: bytes) -> bytes:
    header = 7 if frame[1] & 1 else 9
    out, chain = bytearray(frame), iv
    for c in audio_blocks(len(frame), header):
        chain = encrypt_block(rk, _xor(frame[c:c + 16], chain))
        out[c:c + 16] = chain
    return bytes(out)


def protect(units, audio, key: bytes, iv: bytes):
    """The protected twin of clear access units (lists of unescaped NAL units) and of clear audio
    PES (lists of ADTS frames): slices of more than 48 bytes are encrypted by the format and
    escaped, every other NAL is escaped only; every frame's whole blocks behind its leader are
    encrypted."""
    rk = expand_key(key)
    punits = [[escape(encrypt_nal(u, rk, iv)) if nal_protected(u) else escape(u) for u in unit] for unit in units]
    return punits, [[encrypt_frame(f, rk, iv) for f in p] for p in audio]


def clear_twin(units):
    """What the decrypted ES holds: a protected NAL without emulation prevention, any other as packaged."""
    return [[u if nal_protected(u) else escape(u) for u in unit] for unit in units]


def craft(u: bytes, key: bytes, iv: bytes, j: int, cipher: bytes) -> bytes:
    """``u`` with the plaintext of cipher block ``j`` chosen so that the packager's ciphertext of
    that block is ``cipher``."""
    rk = expand_key(key)
    blocks = video_blocks(len(u))
    chain = iv if j == 0 else encrypt_nal(u, rk, iv)[blocks[j - 1]:blocks[j - 1] + 16]
    c = blocks[j]
    return u[:c] + _xor(decrypt_block(rk, cipher), chain) + u[c + 16:]


# ---------------------------------------------------------------- the reference decrypt
def _clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def ref_segment(es: bytearray, cap: int, info, pes, nal, aframes, sinfo, key: bytes, iv: bytes):
    """Decrypts ``es`` (the segment's ES region) and ``nal`` in place; returns the ``sainfo`` row."""
    rk = expand_key(key)
    max_pes, max_nal = pes.shape[1], nal.shape[0]
    vtype, atype = int(info[INFO["video_type"]]), int(info[INFO["audio_type"]])
    n_apes = _clamp(int(info[INFO["n_audio_pes"]]), 0, max_pes)
    status = 0
    if int(sinfo[0]) & 1:
        status |= TRUNCATED
    if vtype != 0x1B and _clamp(int(info[INFO["video_bytes"]]), 0, cap) > 0:
        status |= UNSUPPORTED_VIDEO
    if atype != 0x0F and n_apes > 0:
        status |= UNSUPPORTED_AUDIO
    if int(sinfo[0]) & 2:
        status |= PARTIAL_AUDIO
    protected = removed = vblocks = frames = ablocks = 0
    if vtype == 0x1B:
        R = _clamp(int(sinfo[1]), 0, max_nal)
        m = _clamp(int(sinfo[2]), 0, max_pes)
        for k in range(R):
            off = _clamp(int(nal[k, 0]), 0, cap)
            n = _clamp(int(nal[k, 1]), 0, cap - off)
            if int(nal[k, 2]) not in (1, 5) or not 0 <= int(nal[k, 3]) < m or n <= 0:
                continue
            u = bytearray(unescape(bytes(es[off:off + n])))
            if len(u) <= 48:
                continue
            chain = iv
            for c in video_blocks(len(u)):
                block = bytes(u[c:c + 16])
                u[c:c + 16] = _xor(decrypt_block(rk, block), chain)
                chain = block
                vblocks += 1
            es[off:off + n] = bytes(u) + bytes(n - len(u))
            nal[k, 1] = len(u)
            protected += 1
            removed += n - len(u)
    if atype == 0x0F:
        ao = _clamp(int(info[INFO["audio_es_offset"]]), 0, cap)
        ab = _clamp(int(info[INFO["audio_bytes"]]), 0, cap - ao)
        for k in range(n_apes):
            q = _clamp(int(pes[1, k, 0]), 0, ab)
            end = _clamp(int(pes[1, k + 1, 0]), q, ab) if k + 1 < n_apes else ab
            for _ in range(max(int(aframes[k, 0]), 0)):
                A = es[ao:ao + ab]
                if q + 7 > end or A[q] != 0xFF or (A[q + 1] & 0xF6) != 0xF0:
                    break
                ln = ((A[q + 3] & 3) << 11) | (A[q + 4] << 3) | (A[q + 5] >> 5)
                header = 7 if A[q + 1] & 1 else 9
                if ln < header or q + ln > end:
                    break
                chain, cs = iv, audio_blocks(ln, header)
                for c in cs:
                    block = bytes(A[q + c:q + c + 16])
                    es[ao + q + c:ao + q + c + 16] = _xor(decrypt_block(rk, block), chain)
                    chain = block
                if cs:
                    frames += 1
                    ablocks += len(cs)
                q += ln
    return np.array([status, protected, removed, vblocks, frames, ablocks], np.int64)


def ref_batch(res, ix, caps, keys, ivs, enable=None):
    """``(es, nal, sainfo)`` as the call must leave them: the whole ES buffer, canaries included."""
    es = bytearray(res.es.cpu().numpy().tobytes())
    info, pes = res.info.cpu().numpy(), res.pes.cpu().numpy()
    nal, af, sinfo = ix.nal.cpu().numpy().copy(), ix.aframes.cpu().numpy(), ix.sinfo.cpu().numpy()
    sainfo = np.zeros((len(caps), SA_WORDS), np.int64)
    for i, c in enumerate(caps):
        if enable is not None and not enable[i]:
            continue
        o = int(res.es_offs[i])
        region = bytearray(es[o:o + c])
        sainfo[i] = ref_segment(region, int(c), info[i], pes[i], nal[i], af[i], sinfo[i], keys[i], ivs[i])
        es[o:o + c] = region
    return np.frombuffer(bytes(es), np.uint8), nal, sainfo


# ---------------------------------------------------------------- hand-built batches
def key_of(i: int) -> bytes:
    return bytes((37 * i + 11 * j + 5) & 0xFF for j in range(16))


def iv_of(i: int) -> bytes:
    return bytes((91 * i + 7 * j + 200) & 0xFF for j in range(16))


def nalu(rng, header: int, n: int) -> bytes:
    """A clear NAL of ``n`` bytes: its header byte, then bytes above 3 (nothing to escape)."""
    return bytes([header]) + bytes(rng.integers(4, 256, n - 1, dtype=np.uint8).tobytes())


def plant(u: bytes, at, pattern=b"\x00\x00\x02") -> bytes:
    """``pattern`` over ``u[p:]`` for every ``p`` in ``at``."""
    out = bytearray(u)
    for p in at:
        out[p:p + len(pattern)] = pattern
    return bytes(out)


def spec(units=(), audio=(), lead=b"", four=None, vtype=0x1B, atype=0x0F, garbage=None):
    """One segment: clear access units (lists of unescaped NALs) and clear audio PES (lists of ADTS
    frames); ``lead`` are video ES bytes in front of the first PES; ``garbage[k]`` are bytes in
    front of the frames of audio PES ``k`` (the index stops there: ``adts_error``)."""
    return {"units": [list(u) for u in units], "audio": [list(p) for p in audio], "lead": lead, "four": four,
            "vtype": vtype, "atype": atype, "garbage": garbage or {}}


def _segment(s, units, audio):
    v, voffs = annexb(units, lead=s["lead"], four=s["four"])
    a, aoffs = bytearray(), []
    for k, p in enumerate(audio):
        aoffs.append(len(a))
        a += s["garbage"].get(k, b"") + b"".join(p)
    return seg(v, bytes(a), vpes=voffs, apes=aoffs, vtype=s["vtype"], atype=s["atype"])


def twins(specs, keys, ivs):
    """``(clear segments, protected segments)`` for ``hand_batch``."""
    clear, prot = [], []
    for s, key, iv in zip(specs, keys, ivs):
        punits, paudio = protect(s["units"], s["audio"], key, iv)
        if s.get("plain_video"):
            punits = clear_twin(s["units"])
        clear.append(_segment(s, clear_twin(s["units"]), s["audio"]))
        prot.append(_segment(s, punits, paudio))
    return clear, prot


def with_canaries(res, caps, fill: int = 0xC3):
    """The same batch with 256 canary bytes in front of every segment and behind the last."""
    old = res.es.cpu().numpy()
    offs = np.asarray(res.es_offs, np.int64) + 256 * (np.arange(len(caps), dtype=np.int64) + 1)
    es = np.full(len(old) + 256 * (len(caps) + 1), fill, np.uint8)
    for o, n, c in zip(res.es_offs, offs, caps):
        es[n:n + c] = old[o:o + c]
    return tsdemux.DemuxResult(res.info, res.pes, torch.from_numpy(es).to(res.es.device), offs)


# ---- video
LENGTHS = (48, 49, 63, 64, 65, 207, 208, 209, 368, 369)


def length_spec(seed: int = 41):
    rng = np.random.default_rng(seed)
    return spec([[nalu(rng, 0x65 if j % 2 else 0x41, n)] for j, n in enumerate(LENGTHS)])


def type_spec(seed: int = 42):
    """Types 6, 7, 8 and 9 of 300 bytes with an escaped ``00 00 03`` inside, a slice in front of the
    first PES, and one protected slice behind them."""
    rng = np.random.default_rng(seed)
    others = [plant(nalu(rng, h, 300), [100], b"\x00\x00\x03") for h in (0x06, 0x67, 0x68, 0x09)]
    lead = b"\x00\x00\x01" + encrypt_nal(nalu(rng, 0x41, 200), expand_key(key_of(0)), iv_of(0))
    return spec([others + [nalu(rng, 0x65, 300)]], lead=lead)


def emulation_spec(key: bytes, iv: bytes, seed: int = 43):
    """Emulation prevention the ciphertext causes.  NAL 0: inside cipher block 1; NAL 1: across the
    clear / cipher edge in front of block 0 (two clear zeros, then a cipher byte <= 3); NAL 2:
    across the edge behind block 0 (two cipher zeros, then a clear 02); NAL 3: two in consecutive
    positions; NAL 4: raw length above 48, unescaped length 47."""
    rng = np.random.default_rng(seed)
    fill = bytes(rng.integers(4, 256, 16, dtype=np.uint8).tobytes())
    inside = craft(nalu(rng, 0x41, 400), key, iv, 1, fill[:5] + b"\x00\x00\x01" + fill[8:])
    front = craft(plant(nalu(rng, 0x65, 230), [30], b"\x00\x00"), key, iv, 0, b"\x02" + fill[1:])
    behind = craft(plant(nalu(rng, 0x41, 230), [48], b"\x02"), key, iv, 0, fill[:14] + b"\x00\x00")
    twice = plant(nalu(rng, 0x41, 300), [100], b"\x00\x00\x00\x00\x02")
    short = plant(nalu(rng, 0x41, 47), [10, 20])
    return spec([[inside, front], [behind, twice, short]])


def round_edge_spec(seed: int = 44):
    """Three NALs with an inserted ``03`` at raw offsets ROUND - 1, ROUND and ROUND + 1."""
    rng = np.random.default_rng(seed)
    return spec([[plant(nalu(rng, 0x41, ROUND + 300), [p - 2])] for p in (ROUND - 1, ROUND, ROUND + 1)])


def long_spec(seed: int = 45):
    """A NAL of 4 ROUND + 37 bytes and one of 70,000 with 25 removed bytes, some next to round edges."""
    rng = np.random.default_rng(seed)
    at = [200 + 2777 * i for i in range(22)] + [ROUND + 60, 3 * ROUND - 1, 5 * ROUND + 1]
    return spec([[nalu(rng, 0x65, 4 * ROUND + 37)], [plant(nalu(rng, 0x41, 70000), at)]])


def alignment_spec(seed: int = 46):
    """32 protected NALs that start at every alignment mod 16 behind a 3- and a 4-byte start code:
    the NAL in front of each one (an AUD in front of the first) is as long as that takes."""
    rng = np.random.default_rng(seed)
    nals, codes = [], [3]
    start, header, base = 3, 0x09, 20  # the pending NAL: where it starts, and its least length
    for k in range(32):
        code, want = (4 if k % 2 == 0 else 3), k // 2
        n = base + (want - code - (start + base)) % 16
        nals.append(nalu(rng, header, n))
        codes.append(code)
        start, header, base = start + n + code, 0x41, 100 + 7 * k
    nals.append(nalu(rng, header, base))
    return spec([nals], four=lambda k: codes[k] == 4)


def tiny_nal_spec(seed: int = 47):
    """An access unit of 700 NALs of 1..3 bytes and one protected NAL behind them."""
    rng = np.random.default_rng(seed)
    return spec([[nalu(rng, 0x41, 1 + j % 3) for j in range(700)] + [nalu(rng, 0x65, 500)]])


def overflow_spec(seed: int = 48):
    """100 protected NALs of 60 bytes in two access units: more than max_nal = 64 rows."""
    rng = np.random.default_rng(seed)
    return spec([[nalu(rng, 0x41, 60) for _ in range(50)] for _ in range(2)])


def codec_spec(vtype: int, seed: int = 49):
    """Bytes that would be protected slices, in a video ES of another codec."""
    rng = np.random.default_rng(seed)
    s = spec([[nalu(rng, 0x41, 200)], [nalu(rng, 0x65, 300)]], [[adts_frame(bytes(background(rng, 64)))]], vtype=vtype)
    s["plain_video"] = True  # both twins carry the same video bytes
    return s


# ---- audio
PAYLOADS = (15, 16, 31, 32, 33, 47, 2048)


def frame(rng, n: int, crc: bool = False) -> bytes:
    return adts_frame(bytes(background(rng, n)), crc=crc)


def payload_spec(seed: int = 50):
    rng = np.random.default_rng(seed)
    video = [[nalu(rng, 0x65, 100)]]
    return spec(video, [[frame(rng, n, crc) for n in PAYLOADS] for crc in (False, True)])


def many_frames_spec(seed: int = 51):
    rng = np.random.default_rng(seed)
    return spec([], [[frame(rng, 33 + j % 40, crc=bool(j % 5 == 0)) for j in range(300)]])


def many_pes_spec(seed: int = 52):
    rng = np.random.default_rng(seed)
    return spec([[nalu(rng, 0x41, 77)]], [[frame(rng, 40 + 16 * j + k) for j in range(1 + k % 3)] for k in range(40)])


def many_units_spec(seed: int = 61):
    """150 access units of one protected NAL and 150 audio PES of one frame: more units than the
    kernel's grid has workgroups per segment (128), so a workgroup takes a second unit."""
    rng = np.random.default_rng(seed)
    return spec([[nalu(rng, 0x65 if a % 25 == 0 else 0x41, 50 + a)] for a in range(150)],
                [[frame(rng, 32 + k % 50, crc=bool(k % 2))] for k in range(150)])


def adts_error_spec(seed: int = 53):
    rng = np.random.default_rng(seed)
    return spec([], [[frame(rng, 64), frame(rng, 80)], [frame(rng, 64)], [frame(rng, 96)]],
                garbage={1: b"\x00\x01\x02"})


def mpeg_audio_spec(seed: int = 54):
    rng = np.random.default_rng(seed)
    return spec([[nalu(rng, 0x65, 120)]], [[frame(rng, 64), frame(rng, 80)]], atype=0x03)


# name -> (specs, max_pes, max_nal); keys, IVs and enable flags come from `batch`
CASES = {
    "video": lambda: ([length_spec(), type_spec(), emulation_spec(key_of(2), iv_of(2)), alignment_spec()], 16, 2048),
    "long": lambda: ([round_edge_spec(), long_spec(), tiny_nal_spec()], 8, 2048),
    "rows": lambda: ([overflow_spec(), codec_spec(0x24), codec_spec(0x02), length_spec(55)], 16, 64),
    "audio": lambda: ([payload_spec(), many_frames_spec(), many_pes_spec(), adts_error_spec(), mpeg_audio_spec()],
                      48, 256),
    "units": lambda: ([many_units_spec(), length_spec(62)], 160, 256),
    "tiny": lambda: ([spec(), spec([[nalu(np.random.default_rng(56), 0x65, 90)]]),
                      spec([], [[frame(np.random.default_rng(57), 50)]])], 8, 64),
    "no_segments": lambda: ([], 8, 64),
}
DISABLED = {"mixed": 1}  # case -> the segment that did not ask


def batch(name: str, device="cpu"):
    """``(clear, protected, keys, ivs, enable, specs)`` of one case: ``clear`` and ``protected`` are
    ``(res, caps, ix)`` with canaries around every segment; segment i has its own key and IV."""
    if name == "mixed":
        specs, max_pes, max_nal = [length_spec(58), payload_spec(59), length_spec(60)], 16, 256
    else:
        specs, max_pes, max_nal = CASES[name]()
    keys, ivs = [key_of(i) for i in range(len(specs))], [iv_of(i) for i in range(len(specs))]
    enable = [i != DISABLED.get(name, -1) for i in range(len(specs))]
    clear, prot = twins(specs, keys, ivs)
    out = []
    for segs in (clear, prot):
        res, caps = hand_batch(segs, "cpu", max_pes)
        res = with_canaries(res, caps)
        dev = torch.device(device)
        res = tsdemux.DemuxResult(res.info.to(dev), res.pes.to(dev), res.es.to(dev), res.es_offs)
        out.append((res, caps, esindex.index_batch(res, caps, max_nal=max_nal)))
    return out[0], out[1], keys, ivs, enable, specs


ALL_CASES = tuple(CASES) + ("mixed",)
