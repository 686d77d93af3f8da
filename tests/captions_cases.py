"""Hand-built inputs and the reference for the caption tests (``test_captions.py`` on the host
implementation, ``test_captions_gpu.py`` on the kernels, ``test_captions_native.py`` on the
stand-alone driver).

The reference is a sequential walk written from the rules of ``docs/CAPTIONS.md`` over Python
``bytes``; it imports nothing from ``ops/captions.py`` and shares no code with
``runtime/captions.cpp`` or ``kernels/captions.hip``.  Inputs are built with the helpers of
``esindex_cases`` (a video ES with planted NAL units, indexed by ``index_batch``).
"""
from __future__ import annotations

import numpy as np
import torch

import esindex_cases as esc
from hlsjs_p2p_wrapper_amd.ops import esindex, tsdemux

INFO = tsdemux.INFO
NAL_BYTES, SLOT, FIELD = 1024, 96, 64
TRUNCATED, UNSUPPORTED, OVERFLOW, CLIPPED = 1, 2, 4, 8


# ---------------------------------------------------------------- the reference
def unescape(raw: bytes, h: int) -> bytes:
    return bytes(raw[j] for j in range(h, len(raw))
                 if not (j >= 2 and raw[j] == 3 and raw[j - 1] == 0 and raw[j - 2] == 0))


def find_caption(U: bytes):
    """``(start, cc_count)`` of the sample of the first GA94 message, or None."""
    p, u = 0, len(U)
    while u - p >= 2:
        T = 0
        while p < u and U[p] == 0xFF:
            T, p = T + 255, p + 1
        if p >= u:
            return None
        T, p = T + U[p], p + 1
        S = 0
        while p < u and U[p] == 0xFF:
            S, p = S + 255, p + 1
        if p >= u:
            return None
        S, p = S + U[p], p + 1
        if S > u - p:
            return None
        if T == 4 and S >= 10 and U[p] == 0xB5 and U[p + 1:p + 3] == b"\x00\x31" and U[p + 3:p + 7] == b"GA94" \
                and U[p + 7] == 3:
            c = U[p + 8] & 31
            if 10 + 3 * c <= S:
                return p + 8, c
        p += S
    return None


def ref_segment(es: bytes, cap: int, info, pes, nal, sinfo, max_cc: int, enable: bool = True):
    """``(ccsamples, ccpts, ccbytes, cc608, ccinfo)`` of one segment from its ES region, its demux
    rows and its index rows as they are."""
    samples = np.full((max_cc, 8), -1, np.int32)
    pts = np.full(max_cc, -1, np.int64)
    data = np.zeros((max_cc, SLOT), np.uint8)
    f608 = np.zeros((max_cc, 2, FIELD), np.uint8)
    ccinfo = np.zeros(8, np.int64)
    if not enable:
        return samples, pts, data, f608, ccinfo
    max_nal, max_pes = nal.shape[0], pes.shape[1]
    vtype = int(info[INFO["video_type"]])
    vbytes = min(max(int(info[INFO["video_bytes"]]), 0), cap)
    status = TRUNCATED if int(sinfo[esindex.SINFO["status"]]) & esindex.SSTATUS["nal_overflow"] else 0
    R = m = 0
    if vtype in (0x1B, 0x24):
        R = min(max(int(sinfo[esindex.SINFO["n_nal"]]), 0), max_nal)
        m = min(max(int(sinfo[esindex.SINFO["n_au"]]), 0), max_pes)
    elif vbytes > 0:
        status |= UNSUPPORTED
    want, h = (6, 1) if vtype == 0x1B else (39, 2)
    n_sei = total = 0
    kept = []
    for k in range(R):
        off = min(max(int(nal[k, 0]), 0), cap)
        n = min(max(int(nal[k, 1]), 0), cap - off)
        au = int(nal[k, 3])
        if int(nal[k, 2]) != want or not 0 <= au < m or n <= h:
            continue
        n_sei += 1
        if n > NAL_BYTES:
            status |= CLIPPED
        U = unescape(es[off:off + min(n, NAL_BYTES)], h)
        hit = find_caption(U)
        if hit is None:
            continue
        total += 1
        if len(kept) < max_cc:
            kept.append((k, au, U[hit[0]:hit[0] + 2 + 3 * hit[1]], int(pes[0, au, 1])))
    if total > max_cc:
        status |= OVERFLOW
    for r, (k, au, b, p) in enumerate(kept):
        pairs = ([], [])
        for t in range((len(b) - 2) // 3):
            f, b1, b2 = b[2 + 3 * t], b[3 + 3 * t] & 0x7f, b[4 + 3 * t] & 0x7f
            if f & 4 and (f & 3) < 2 and (b1 or b2):
                pairs[f & 3].append((b1, b2))
        order = sum(1 for q, other in enumerate(kept) if (other[3], q) < (p, r))
        samples[r] = (k, au, len(b), (len(b) - 2) // 3, order, len(pairs[0]), len(pairs[1]), 1 if b[0] & 0x40 else 0)
        pts[r] = p
        data[r, :len(b)] = np.frombuffer(b, np.uint8)
        for f in range(2):
            flat = bytes(x for pair in pairs[f] for x in pair)
            f608[r, f, :len(flat)] = np.frombuffer(flat, np.uint8)
        ccinfo[3] += (len(b) - 2) // 3
        ccinfo[4] += len(pairs[0])
        ccinfo[5] += len(pairs[1])
    ccinfo[0], ccinfo[1], ccinfo[2] = status, n_sei, total
    ccinfo[6] = min((x[3] for x in kept), default=-1)
    ccinfo[7] = max((x[3] for x in kept), default=-1)
    return samples, pts, data, f608, ccinfo


def ref_batch(res, ix, caps, max_cc: int, enable=None):
    """The reference for every segment, stacked like ``Captions``: ``(ccsamples, ccpts, ccbytes, cc608, ccinfo)``."""
    es, info, pes = res.es.cpu().numpy(), res.info.cpu().numpy(), res.pes.cpu().numpy()
    nal, sinfo = ix.nal.cpu().numpy(), ix.sinfo.cpu().numpy()
    out = [ref_segment(es[int(o):int(o) + int(c)].tobytes(), int(c), info[i], pes[i], nal[i], sinfo[i], max_cc,
                       True if enable is None else bool(enable[i]))
           for i, (o, c) in enumerate(zip(res.es_offs, caps))]
    return tuple(np.stack([seg[j] for seg in out]) for j in range(5))


NAMES = ("ccsamples", "ccpts", "ccbytes", "cc608", "ccinfo")


def assert_captions_equal(cc, ref) -> None:
    """Exact equality of the five tensors."""
    for name, want in zip(NAMES, ref):
        got = getattr(cc, name).cpu().numpy() if not isinstance(cc, dict) else cc[name]
        assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype)
        bad = np.argwhere(got != want)
        assert not len(bad), f"{name}: first difference at {bad[0].tolist()}: got {got[tuple(bad[0])]}, " \
                             f"want {want[tuple(bad[0])]}"


# ---------------------------------------------------------------- the SEI builder
def coded(v: int) -> bytes:
    return b"\xff" * (v // 255) + bytes([v % 255])


def message(T: int, payload: bytes, S=None) -> bytes:
    """One sei_message: type and size with their FF extension bytes (``S``: a size that lies)."""
    return coded(T) + coded(len(payload) if S is None else S) + payload


def ga94_payload(triples, first=0x40, em=0xFF, marker=True, code=b"GA94", country=0xB5, provider=b"\x00\x31",
                 type_code=3, count=None) -> bytes:
    c = len(triples) if count is None else count
    body = b"".join(bytes(t) for t in triples)
    return bytes([country]) + provider + code + bytes([type_code, first | c, em]) + body + (b"\xff" if marker else b"")


def caption(triples, S_delta: int = 0, **kw) -> bytes:
    """A type-4 message with a GA94 payload; ``S_delta`` moves the coded size off the payload's."""
    p = ga94_payload(triples, **kw)
    return message(4, p, len(p) + S_delta)


def escape(rbsp: bytes) -> bytes:
    out, zeros = bytearray(), 0
    for b in rbsp:
        if zeros >= 2 and b <= 3:
            out.append(3)
            zeros = 0
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def sei(*messages, hevc=False, tail=b"\x80", header=None) -> bytes:
    head = header if header is not None else (b"\x4e\x01" if hevc else b"\x06")
    return head + escape(b"".join(messages) + tail)


def dropped(nal: bytes):
    """Raw offsets of the emulation-prevention bytes of a NAL."""
    return [j for j in range(2, len(nal)) if nal[j] == 3 and nal[j - 1] == 0 and nal[j - 2] == 0]


def triples(n: int, seed: int = 0, f=0xFC):
    rng = np.random.default_rng(100 + seed)
    return [(f, int(rng.integers(0x20, 0x7f)), int(rng.integers(0x20, 0x7f))) for _ in range(n)]


def filler(rng, n: int, hevc=False) -> bytes:
    """A slice NAL of ``n`` bytes free of zeros."""
    return (b"\x02\x01" if hevc else b"\x41") + bytes(esc.background(rng, n - (2 if hevc else 1)))


def video(nals, lead: int = 0):
    """``(video ES, vpes)`` from ``[(nal bytes, four-byte start code, starts an access unit)]``;
    ``lead`` bytes of zero-free background come first."""
    rng = np.random.default_rng(len(nals))
    v, vpes = bytearray(esc.background(rng, lead)), []
    for body, four, new_au in nals:
        if new_au:
            vpes.append(len(v))
        v += (b"\x00" if four else b"") + esc.SC + body
    return bytes(v), vpes


def each_own_au(bodies, hevc=False):
    """Every NAL in its own access unit behind an AUD, start codes alternating 3 / 4 bytes."""
    aud = b"\x46\x01\x50" if hevc else b"\x09\xf0"
    out = []
    for i, b in enumerate(bodies):
        out += [(aud, i % 2 == 1, True), (b, i % 2 == 0, False)]
    return out


# ---------------------------------------------------------------- the cases
def header_nals():
    t5 = message(5, bytes(range(1, 21)))
    big = message(1, bytes(esc.background(np.random.default_rng(1), 271)))
    return [
        sei(caption(triples(3, 1))),                                                  # first message
        sei(message(1, b"\x11\x22\x33"), caption(triples(2, 2))),                      # second
        sei(message(1, b"\x01"), message(0, b""), t5, message(6, b"\x09"), caption(triples(4, 3))),  # fifth
        sei(message(260, b"\x10\x20\x30\x40"), caption(triples(2, 4))),                # type FF 05
        sei(big, caption(triples(2, 5))),                                              # size FF 10
        sei(caption(triples(3, 6), marker=False)),                                     # S == 10 + 3c
        sei(caption(triples(3, 7), marker=False, S_delta=-1)),                         # S one less: rejected
        sei(caption([], first=0x40)),                                                  # c == 0
        sei(caption(triples(1, 8))),
        sei(caption(triples(31, 9))),
        sei(caption(triples(2, 10)), tail=b""),                                        # no trailing bits
        sei(message(1, b"\x01\x02"), message(4, b"\xb5\x00\x31GA94\x03\x41\xff", S=200)),  # S > u - p
        sei(message(1, b"\x01\x02"), tail=b"\x80"),                                    # one byte left
        b"\x06\x04",                                                                   # u == 1
        b"\x06",                                                                       # n == h: no candidate
        sei(b"\xff\xff\xff", tail=b""),                                                # a type that never ends
        sei(b"\x04\xff\xff", tail=b""),                                                # a size that never ends
    ]


def near_miss_nals():
    tr = triples(2, 20)
    return [
        sei(caption(tr, code=b"DTG1")),
        sei(caption(tr, country=0xB4)),
        sei(caption(tr, provider=b"\x00\x2f")),
        sei(caption(tr, type_code=6), caption(triples(3, 21))),                        # walks on to a real match
        sei(caption(triples(2, 22)), caption(triples(5, 23))),                         # the first wins
        sei(caption(tr, code=b"DTG1"), caption(tr, country=0xB4), caption(triples(1, 24))),
        sei(caption(tr, count=9, marker=False)),                                       # cc_count does not fit S
        sei(message(4, b"\xb5\x00\x31GA9")),                                           # a short type-4 message
    ]


def padded_to(target: int, tr):
    """An SEI whose padding message puts an emulation-prevention byte at raw offset ``target``."""
    for L in range(0, target + 8):
        nal = sei(message(5, b"\x55" * L), caption(tr))
        if target in dropped(nal):
            return nal
    raise AssertionError(target)


def emulation_nals():
    zeros = [(0xFC, 0, 0), (0, 0, 1), (0xFD, 0, 0), (3, 0x41, 0), (0, 0, 0), (0, 0, 3), (0xFC, 0x41, 0x42)]
    out = [
        sei(message(5, b"\x00\x00\x01\x00\x00\x00\x00\x02"), caption(triples(2, 30))),  # in front, shifting the match
        sei(caption(zeros)),                                                           # inside the triples
        sei(caption(triples(2, 31))) + b"\x00\x00\x03",                                # as the NAL's last bytes
    ]
    out += [padded_to(t, zeros) for t in (63, 64, 65, 255, 256, 257)]
    assert all(dropped(n) for n in out)
    return out


def clip_nals():
    """Matches whose message ends at raw offset 1023 and 1024 (found) and 1025 (not found)."""
    tr = triples(4, 40)
    cap_msg = caption(tr)
    out = []
    for end in (1023, 1024, 1025):
        for tail in (b"", b"\x80"):
            fits = [nal for nal in (sei(message(5, b"\x66" * L), cap_msg, tail=tail) for L in range(900, 1030))
                    if len(nal) - len(tail) == end and not dropped(nal)]
            out.append(fits[0])
    assert len(out) == 6, len(out)
    out.append(sei(message(5, b"\x77" * 1100), caption(tr)))  # the caption lies behind the stored bytes
    return out


def placement_segments(rng):
    """NAL starts at every offset mod 16; a candidate at the video ES's last byte, with audio behind
    it and with nothing behind it."""
    nals, seen, pos = [], set(), 0
    for i in range(40):
        sc = 4 if i % 3 == 0 else 3
        pad = filler(rng, 2 + (i * 7 - pos - 5 - sc) % 16)  # the SEI's first byte lands on offset 7 i mod 16
        body = sei(caption(triples(1 + i % 5, 50 + i)))
        nals += [(pad, False, True), (body, i % 3 == 0, False)]
        pos += 3 + len(pad) + sc
        seen.add(pos % 16)
        pos += len(body)
    assert seen == set(range(16)), seen
    v, vpes = video(nals)
    last = sei(caption(triples(3, 99)), tail=b"")
    a, ap = video([(b"\x09\xf0", False, True), (last, False, False)])
    return [esc.seg(v, vpes=vpes[:60]), esc.seg(a, b"\x01\x65" + bytes(esc.background(rng, 40)), vpes=ap, atype=0x03),
            esc.seg(a, vpes=ap)]


def row_segment(rng, matches=(0, 255, 256, 257, 300, 600, 601)):
    """620 NAL rows with candidates on the edges of the rounds of 256; the rows before the first
    access unit have ``au == -1``, and zero-length rows sit between."""
    nals = []
    for k in range(620):
        new_au = k > 0 and k % 90 == 1
        if k in matches or k in (5, 511, 512):
            nals.append((sei(caption(triples(1 + k % 4, k))), False, new_au))
        elif k % 50 == 7:
            nals.append((b"", False, new_au))  # a start code right behind a start code
        else:
            nals.append((filler(rng, 2 + k % 5), k % 9 == 0, new_au))
    v, vpes = video(nals)
    return esc.seg(v, vpes=vpes)


def order_segment():
    """A B-frame pts pattern with equal and -1 stamps; the triples cover the 608 pair rule."""
    bodies = [
        # 80 80 and cc_valid off
        sei(caption([(0xFC, 0x94, 0x20), (0xFD, 0x15, 0x2C), (0xFC, 0x80, 0x80), (0xF8, 0x41, 0x42)])),
        sei(caption([(0xFE, 0x41, 0x42), (0xFF, 0x43, 0x44), (0xFC, 0x45, 0x46)])),              # types 2 and 3
        sei(caption(triples(31, 60))),                                                           # 31 of field 1
        sei(caption([(0xFC | (t & 1), 0x20 + t, 0x80 if t % 3 else 0x21) for t in range(12)])),  # mixed fields
        sei(caption(triples(31, 61, f=0xFD), first=0x00)),                                       # field 2, flag off
        sei(caption(triples(2, 62))), sei(caption(triples(2, 63))), sei(caption(triples(2, 64))),
    ]
    v, vpes = video(each_own_au(bodies))
    return esc.seg(v, vpes=vpes), [0, 10800, 3600, 7200, 7200, -1, 3600, -1]


def stamp(res, i: int, pts) -> None:
    for a, p in enumerate(pts):
        res.pes[i, 0, a, 1] = p


def main_case():
    """``(segments, max_pes, max_nal, max_cc, pts overrides)`` of the large batch."""
    rng = np.random.default_rng(11)
    segs, pts = [], {}
    for bodies in (header_nals(), near_miss_nals(), emulation_nals(), clip_nals()):
        v, vpes = video(each_own_au(bodies), lead=len(segs))
        segs.append(esc.seg(v, vpes=vpes))
    segs += placement_segments(rng)
    segs.append(row_segment(rng))
    o, stamps = order_segment()
    pts[len(segs)] = stamps
    segs.append(o)
    # HEVC: prefix SEI 39 against suffix SEI 40, and H.264's byte 06 under HEVC
    hb = [sei(caption(triples(2, 70)), hevc=True), sei(caption(triples(2, 71)), header=b"\x50\x01"),
          sei(caption(triples(2, 72))), sei(caption(triples(3, 73)), hevc=True, tail=b"\x80")]
    v, vpes = video(each_own_au(hb, hevc=True))
    segs.append(esc.seg(v, vpes=vpes, vtype=0x24))
    v, vpes = video(each_own_au([sei(caption(triples(2, 74)))]))
    segs += [esc.seg(v, vpes=vpes, vtype=0x24), esc.seg(v, vpes=vpes, vtype=0x02), esc.seg(b"", vtype=0x02),
             esc.seg(b"")]
    return segs, 64, 1024, 64, pts


def small_case():
    """``max_cc`` of 4 with 6 matches, and more NAL units than ``max_nal`` rows."""
    a, ap = video(each_own_au([sei(caption(triples(1 + i, 80 + i))) for i in range(6)]))
    b, bp = video(each_own_au([sei(caption(triples(2, 90 + i))) for i in range(14)]))
    c, cp = video(each_own_au([sei(caption(triples(2, 95 + i))) for i in range(3)]))
    return [esc.seg(a, vpes=ap), esc.seg(b, vpes=bp), esc.seg(c, vpes=cp)], 16, 16, 4, {}


def long_case():
    """A 70,000-byte SEI whose caption is its first message."""
    body = sei(caption(triples(5, 110)), message(5, b"\x42" * 70000))
    v, vpes = video(each_own_au([body, sei(caption(triples(2, 111)))]))
    return [esc.seg(v, vpes=vpes)], 8, 64, 8, {}


CASES = {"main": main_case, "small": small_case, "long": long_case}


def batch(name: str, device="cpu"):
    """``(res, caps, ix, max_cc)`` of a case, demux rows by hand and the index by ``index_batch``."""
    segs, max_pes, max_nal, max_cc, pts = CASES[name]()
    res, caps = esc.hand_batch(segs, "cpu", max_pes=max_pes)
    for i, stamps in pts.items():
        stamp(res, i, stamps)
    if torch.device(device).type != "cpu":
        res = tsdemux.DemuxResult(res.info.to(device), res.pes.to(device), res.es.to(device), res.es_offs)
    return res, caps, esindex.index_batch(res, caps, max_nal=max_nal), max_cc


def damage(res, caps, ix, seed: int = 3) -> None:
    """Rows that lie, in place: offsets and lengths negative and beyond ``cap``, overlapping rows,
    garbage access units, counts beyond the tables; most rows stay SEI so that there is work left."""
    rng = np.random.default_rng(seed)
    nal, sinfo = ix.nal.cpu().numpy(), ix.sinfo.cpu().numpy()
    B, max_nal = nal.shape[:2]
    for i in range(B):
        cap = int(caps[i])
        for k in range(max_nal):
            roll = rng.integers(0, 10)
            if roll == 0:
                nal[i, k, 0] = rng.integers(-2 ** 31, 0)
            elif roll == 1:
                nal[i, k, 0] = cap + rng.integers(-8, 2 ** 30)
            elif roll == 2:
                nal[i, k, 1] = rng.integers(-2 ** 31, 0)
            elif roll == 3:
                nal[i, k, 1] = rng.integers(cap // 2, 2 ** 31 - 1)
            elif roll == 4 and k:
                # overlaps its neighbour
                nal[i, k, :2] = (min(int(nal[i, k - 1, 0]) + 1, 2 ** 31 - 1), max(int(nal[i, k - 1, 1]), 40))
            elif roll == 5:
                nal[i, k, 3] = rng.choice([-7, -1, 2 ** 31 - 1, -2 ** 31, 10 ** 6])
            elif roll == 6:
                nal[i, k, :2] = (rng.integers(0, max(cap, 1)), rng.integers(0, 3000))
            if roll != 7:
                nal[i, k, 2] = 6
            if nal[i, k, 3] == -1 and roll != 5:
                nal[i, k, 3] = rng.integers(0, 4)
        sinfo[i, 1] = rng.choice([max_nal, max_nal + 5, 2 ** 40, int(sinfo[i, 1])])
        sinfo[i, 2] = rng.choice([4, 2 ** 40, int(sinfo[i, 2])])
    ix.nal.copy_(torch.from_numpy(nal))
    ix.sinfo.copy_(torch.from_numpy(sinfo))
