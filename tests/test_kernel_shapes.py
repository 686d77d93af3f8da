"""Batch-walk, boundary and alignment shapes of the HIP kernels.

The content checks of ``test_kernels_gpu.py`` run at one family of shapes (at most 52 members,
256-aligned offsets, no empty member after the first, zero gaps).  These tests keep the same
references -- zlib, the plaintext that was encrypted, the serial CPU demux, a numpy copy loop --
and move the shapes to where the kernels' segment walk, tails and alignment splits take their
other paths: thousands of tiny members (``find_seg_wave`` past one level, a wave that crosses or
jumps members), empty members in the middle and at the end, non-zero gaps, block-boundary packet
counts, every ES destination residue, the PKCS#7 table on every lane position.

Every device test runs twice: the ``cpu`` leg sends the same inputs through the host oracle, which
proves without a GPU that the builder is well formed and that the reference alone satisfies every
stated precondition; the ``cuda`` leg runs the kernels.  All comparisons are exact.  Each test ends
with one deliberate change of the *input* that the comparison must notice.
"""
import zlib

import numpy as np
import pytest
import torch

from hlsjs_p2p_wrapper_amd.ops import aes, crc, segment, tsdemux
from hlsjs_p2p_wrapper_amd.ops._native import device as _dev

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
ST = tsdemux.STATUS
I = tsdemux.INFO
PKT = tsdemux.PACKET
SENTINEL = 0xEE
# packet counts around the wave (64), block (256) and 4-block scan group (1024) edges, and one
# past the first block of a second scan group
COUNTS = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1279, 1281]
PARTIAL = 257 * PKT + 100  # a trailing partial packet


def _device(dev, request):
    """(torch device, CU count that sizes the persistent grids; 256 on the cpu leg)."""
    if dev == "cuda":
        d = request.getfixturevalue("cuda")
        return d, int(_dev().device_cus(torch.zeros(16, dtype=torch.uint8, device=d)))
    return torch.device("cpu"), 256


def _nseg(cus):
    n = 32 * cus + 500
    assert n > 4096  # find_seg_wave takes its third level only past 4096 entries
    return n


def _np(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def shared():
    """Inputs and references built once and shared by the legs and variants that need them (the
    tests copy what they change); dropped with the module."""
    cache = {}

    def get(key, build):
        if key not in cache:
            cache[key] = build()
        return cache[key]

    yield get
    cache.clear()


# ------------------------------------------------------------------ 1. many-segment walk: CRC
_CRC_SMALL = [1, 600, 15, 16, 17, 255, 256, 257, 33, 511, 512, 513, 100, 3, 64, 300, 599, 2, 129, 447]
_CRC_BIG = [8191, 8192, 8193, 20_000, 70_001]


def _crc_batch(nseg):
    """Lengths cycling a fixed pattern (most 1..600 bytes; every 7th empty, with runs of three
    empties and two empties at the end; every 50th around the 8 KiB tile or several tiles long),
    offsets 16-aligned and packed 16..47 bytes apart, 0xA5 between the members."""
    lens = np.empty(nseg, np.int64)
    for i in range(nseg):
        if i % 50 == 25:
            lens[i] = _CRC_BIG[(i // 50) % len(_CRC_BIG)]
        elif i % 7 == 0 or i % 210 in (1, 2):  # 210 = 7 * 30: members 210 m, +1, +2 are empty
            lens[i] = 0
        else:
            lens[i] = _CRC_SMALL[i % len(_CRC_SMALL)]
    lens[-2:] = 0
    offs = np.empty(nseg, np.int64)
    pos = 16
    for i in range(nseg):
        offs[i] = pos
        pos = (pos + int(lens[i]) + 15) // 16 * 16 + 16 * (1 + i % 2)
    buf = np.full(pos + 256, 0xA5, np.uint8)
    data = np.random.default_rng(21).integers(0, 256, int(lens.sum()), dtype=np.uint8)
    cut = np.concatenate([[0], np.cumsum(lens)])
    for i in range(nseg):
        buf[offs[i]:offs[i] + lens[i]] = data[cut[i]:cut[i + 1]]
    return buf, offs, lens


def _crc_batch_with_expect(nseg):
    buf, offs, lens = _crc_batch(nseg)
    return buf, offs, lens, [zlib.crc32(buf[o:o + n].tobytes()) for o, n in zip(offs.tolist(), lens.tolist())]


@pytest.mark.parametrize("variant", ["fp4", "i8"])
@pytest.mark.parametrize("dev", DEVICES)
def test_crc_many_segments_wave_crosses_members(dev, variant, request, shared):
    """``nseg`` > 4096 members, most under one tile: the residue kernels' waves own two or more
    tiles, so each wave walks from one member into the next (``t + 1 >= tend``, the prefetch of
    the next member's first tile), over single empties, runs of three and a trailing pair."""
    device, cus = _device(dev, request)
    nseg = _nseg(cus)
    buf, offs, lens, expect = shared(("crc", nseg), lambda: _crc_batch_with_expect(nseg))
    # preconditions of the paths this test is for
    assert not (offs % 16).any() and np.count_nonzero(offs % 256) > nseg * 3 // 4
    zero = lens == 0
    assert zero[-2:].all() and (zero[:-2] & zero[1:-1] & zero[2:]).any() and zero[7] and not zero[8]
    assert {8191, 8192, 8193, 20_000, 70_001} <= set(lens.tolist())
    total_tiles = int((((lens + 255) // 256 + 31) // 32).sum())
    tiles_per_wave = -(-total_tiles // (cus * 16))  # crc32_mfma.hip: 2 workgroups x 8 waves per CU
    assert tiles_per_wave >= 2, (total_tiles, cus)

    t = torch.from_numpy(buf.copy()).to(device)
    got, ok = crc.crc32_batch(t, offs, lens, expect=expect, variant=variant)
    assert _np(got).view(np.uint32).tolist() == expect
    assert _np(ok).tolist() == [1] * nseg
    # the same batch scattered through a permutation: the whole table, untouched slots included
    ids = np.random.default_rng(22).permutation(nseg + 9)[:nseg]
    table = torch.full((nseg + 9,), 7, dtype=torch.int32, device=device)
    got2, _ = crc.crc32_batch(t, offs, lens, scatter_to=table, scatter_idx=ids, variant=variant)
    ref = np.full(nseg + 9, 7, np.int32)
    ref[ids] = np.asarray(expect, np.uint32).view(np.int32)
    assert np.array_equal(_np(table), ref)
    assert _np(got2).view(np.uint32).tolist() == expect
    # liveness: one byte of a member that follows a run of three empties -> exactly its ok drops
    j = next(i for i in range(100, nseg) if zero[i - 3:i].all() and lens[i] > 0)
    t[int(offs[j]) + int(lens[j]) // 2] ^= 0x40
    _, ok3 = crc.crc32_batch(t, offs, lens, expect=expect, variant=variant)
    assert np.flatnonzero(_np(ok3) == 0).tolist() == [j]


# ------------------------------------------------------------------ 1. many-segment walk: decrypt
_AES_SIZES = [16, 32, 4080, 4096, 4112, 8192, 12_288, 12_304]  # 1, 1, 1, 1, 2, 2, 3, 4 chunks
_KEYS = [bytes(range(16)), bytes(range(100, 116)), bytes([0xC3] * 8 + [0x3C] * 8)]


def _aes_batch(nseg):
    """``nseg`` ciphertexts of cycling sizes (pad lengths 1..16), three keys interleaved so that
    neighbours differ, per-member IVs, source and destination offsets 16-aligned, packed 16..48
    bytes apart (differently on the two sides), 0xA5 between the ciphertexts."""
    rng = np.random.default_rng(31)
    sizes = np.array([_AES_SIZES[i % len(_AES_SIZES)] for i in range(nseg)], np.int64)
    plen = sizes - 1 - (np.arange(nseg) % 16)
    keys = [_KEYS[i % 3] for i in range(nseg)]
    ivs = rng.integers(0, 256, (nseg, 16), dtype=np.uint8)
    data = rng.integers(0, 256, int(plen.sum()), dtype=np.uint8)
    cut = np.concatenate([[0], np.cumsum(plen)])
    so, do = np.empty(nseg, np.int64), np.empty(nseg, np.int64)
    spos, dpos = 16, 48
    for i in range(nseg):
        so[i], do[i] = spos, dpos
        spos += int(sizes[i]) + 16 * (1 + i % 3)
        dpos += int(sizes[i]) + 16 * (1 + (i + 1) % 3)
    src = np.full(spos + 256, 0xA5, np.uint8)
    ref = np.full(dpos + 256, SENTINEL, np.uint8)  # the whole destination after the decrypt
    for i in range(nseg):
        p = data[cut[i]:cut[i + 1]]
        ct = aes.cbc_encrypt(keys[i], ivs[i].tobytes(), p)
        n = int(sizes[i])
        assert len(ct) == n
        src[so[i]:so[i] + n] = ct
        ref[do[i]:do[i] + len(p)] = p
        ref[do[i] + len(p):do[i] + n] = n - len(p)  # the PKCS#7 run is decrypted like any block
    return src, so, do, sizes, plen, keys, [v.tobytes() for v in ivs], ref


@pytest.mark.parametrize("dev", DEVICES)
def test_decrypt_many_segments_wave_jumps_members(dev, request, shared):
    """More than 32 chunks per CU: every wave of the persistent grid steps 16 chunks at a time and
    lands several members further on, on a member's first chunk (IV) or inside one (chained from
    the previous chunk's last block); round keys change at every border."""
    device, cus = _device(dev, request)
    nseg = _nseg(cus)
    src, so, do, sizes, plen, keys, ivs, ref = shared(("aes", nseg), lambda: _aes_batch(nseg))
    chunk = (int(_dev().aes_chunk_blocks()) if dev == "cuda" else 256) * 16
    total_chunks = int(((sizes + chunk - 1) // chunk).sum())
    assert total_chunks > 32 * cus, (total_chunks, cus)
    assert all(a != b for a, b in zip(keys, keys[1:])) and len(set(keys)) >= 3
    assert not (so % 16).any() and np.count_nonzero(so % 256) > nseg * 3 // 4
    assert not (do % 16).any() and np.count_nonzero(do % 256) > nseg * 3 // 4

    s = torch.from_numpy(src.copy()).to(device)
    d = torch.full((len(ref),), SENTINEL, dtype=torch.uint8, device=device)
    out_len = aes.cbc_decrypt_batch(s, so, sizes, keys, ivs, d, do)
    assert np.array_equal(_np(out_len), plen)
    # every plaintext byte, and 0xEE everywhere outside the members' ciphertext extents
    assert np.array_equal(_np(d), ref)
    # liveness: one ciphertext byte in the second chunk of a four-chunk member deep in the batch
    j = next(i for i in range(nseg // 2, nseg) if sizes[i] == 12_304)
    s[int(so[j]) + 4096 + 5] ^= 0x01
    d2 = torch.full_like(d, SENTINEL)
    aes.cbc_decrypt_batch(s, so, sizes, keys, ivs, d2, do)
    diff = np.flatnonzero(_np(d2) != ref)
    assert len(diff) and diff.min() >= do[j] + 4096 and diff.max() < do[j] + 4096 + 32


# ------------------------------------------------------------------ demux inputs
@pytest.fixture(scope="module")
def stream():
    """One synthetic TS segment (2127 packets, id3 track) and its payload-only video packets."""
    seg, _ = tsdemux.mux_segment(target_bytes=400_000, with_id3=True, seed=3)
    seg = np.frombuffer(bytes(seg), np.uint8).copy()
    assert len(seg) % PKT == 0 and len(seg) // PKT > max(COUNTS)
    full = tsdemux.demux_batch(torch.from_numpy(seg), [0], [len(seg)], torch.zeros(len(seg) + 256, dtype=torch.uint8),
                               [0]).info[0].numpy()
    assert full[I["status"]] == 0
    pk = seg.reshape(-1, PKT)
    pid = ((pk[:, 1].astype(int) & 0x1F) << 8) | pk[:, 2]
    plain_video = (pid == full[I["video_pid"]]) & ((pk[:, 1] & 0x40) == 0) & ((pk[:, 3] & 0x30) == 0x10)
    assert plain_video.sum() >= 8
    return seg, pk[plain_video][:8].copy()


def _demux_layout(seg, filler, nbytes, es_slack):
    """Members (the first ``nbytes[i]`` bytes of ``seg``) at 16-aligned, mostly not 256-aligned
    offsets; right behind each member -- where one packet too many would be read -- and after
    the last one sit valid video-PID payload packets; the rest of the gaps is 0xA5.  ES
    destinations take all four residues modulo 4 and leave ``es_slack`` spare bytes each."""
    B = len(nbytes)
    fill = filler[:2].reshape(-1)
    offs, eo = np.empty(B, np.int64), np.empty(B, np.int64)
    pos, epos = 16, 0
    for i, n in enumerate(nbytes):
        offs[i] = pos
        pos = (pos + n + len(fill) + 15) // 16 * 16 + 16
        eo[i] = epos + (i % 4)
        epos += (n + es_slack + 4 + 15) // 16 * 16
    buf = np.full(pos + 256, 0xA5, np.uint8)
    for i, n in enumerate(nbytes):
        buf[offs[i]:offs[i] + n] = seg[:n]
        buf[offs[i] + n:offs[i] + n + len(fill)] = fill
    return buf, offs, eo, epos + 256


def _assert_es_untouched(es, eo, payload):
    """Every ES byte outside ``[eo[i], eo[i] + payload[i])`` still holds the sentinel."""
    ends = eo + payload
    assert (eo[1:] >= ends[:-1]).all() and payload.any()
    for a, b in zip([0] + ends.tolist(), eo.tolist() + [len(es)]):
        assert (es[a:b] == SENTINEL).all(), (a, b)


def _demux(device, buf, offs, nbytes, eo, es_len, max_pes):
    es = torch.full((es_len,), SENTINEL, dtype=torch.uint8, device=device)
    return tsdemux.demux_batch(torch.from_numpy(buf).to(device), offs, nbytes, es, eo, max_pes=max_pes)


def _assert_demux_equal(got, ref, eo):
    gi, ri = _np(got.info), _np(ref.info)
    assert np.array_equal(gi, ri), np.flatnonzero((gi != ri).any(axis=1))[:8]
    assert np.array_equal(_np(got.pes), _np(ref.pes))
    ges, res = _np(got.es), _np(ref.es)
    assert np.array_equal(ges, res)  # the members' ES bytes and the sentinel everywhere else
    _assert_es_untouched(ges, eo, ri[:, I["payload_bytes"]])


# ------------------------------------------------------------------ 1. many-segment walk: demux
_DEMUX_K = [0, 1, 2, 3, 255, 256, 257, 511, 513]


@pytest.mark.parametrize("dev", DEVICES)
def test_demux_many_segments_with_empty_members(dev, request, stream, shared):
    """``nseg`` > 4096 members of 0..3 blocks: the scan's four-block groups and the gather's
    blocks look their member up in a three-level table with zero-block members in the middle
    and two at the end; ``max_pes=8`` is below the PES count of the longer members."""
    device, cus = _device(dev, request)
    nseg = _nseg(cus)
    seg, filler = stream
    ks = np.array([_DEMUX_K[i % len(_DEMUX_K)] for i in range(nseg - 2)] + [0, 0])
    nbytes = (ks * PKT).tolist()

    def build():
        buf, offs, eo, es_len = _demux_layout(seg, filler, nbytes, 32)
        return buf, offs, eo, es_len, _demux(torch.device("cpu"), buf, offs, nbytes, eo, es_len, 8)

    buf, offs, eo, es_len, ref = shared(("demux", nseg), build)
    ri = ref.info.numpy()
    assert (ks[:-2] == 0).any() and (ri[ks == 0, I["status"]] == ST["no_pat"]).all()
    assert (ri[ks == 1, I["status"]] == ST["no_pmt"]).all()
    for k in (511, 513):  # 20 video PES, more than max_pes
        rows = ri[ks == k]
        assert (rows[:, I["n_video_pes"]] > 8).all() and (rows[:, I["status"]] & ST["pes_overflow"]).all()
    assert not (ri[ks >= 2, I["status"]] & ~ST["pes_overflow"]).any()
    got = ref if dev == "cpu" else _demux(device, buf, offs, nbytes, eo, es_len, 8)
    _assert_demux_equal(got, ref, eo)
    del got
    # liveness: one payload byte of a 257-packet member in the last third of the batch
    j = next(i for i in range(2 * nseg // 3, nseg) if ks[i] == 257)
    at = int(offs[j]) + 256 * PKT + PKT - 1
    try:
        buf[at] ^= 0xFF
        got2 = _demux(device, buf, offs, nbytes, eo, es_len, 8)
    finally:
        buf[at] ^= 0xFF  # the shared input goes back as it was
    assert np.array_equal(_np(got2.info), ri)  # a payload byte: same layout
    diff = np.flatnonzero(_np(got2.es) != ref.es.numpy())
    assert len(diff) == 1 and eo[j] <= diff[0] < eo[j] + ri[j, I["payload_bytes"]]


# ------------------------------------------------------------------ 2. demux boundaries
@pytest.mark.parametrize("dev", DEVICES)
def test_demux_block_boundaries_overread_and_es_alignment(dev, request, stream):
    """Packet counts on both sides of the wave, block and scan-group edges and a trailing partial
    packet, with valid video packets behind every member (one packet read too many changes
    ``video_bytes``), all four ES destination residues, default ``max_pes`` and ``max_pes=4``."""
    device, _ = _device(dev, request)
    seg, filler = stream
    nbytes = [k * PKT for k in COUNTS] + [PARTIAL]
    buf, offs, eo, es_len = _demux_layout(seg, filler, nbytes, 260)
    assert {int(e) % 4 for e in eo} == {0, 1, 2, 3}
    cpu = torch.device("cpu")
    for max_pes in (tsdemux.DEFAULT_MAX_PES, 4):
        ref = _demux(cpu, buf, offs, nbytes, eo, es_len, max_pes)
        ri = ref.info.numpy()
        st = dict(zip(COUNTS + ["partial"], ri[:, I["status"]].tolist()))
        assert st[0] == ST["no_pat"] and st[1] == ST["no_pmt"]
        if max_pes == 4:  # 1025 packets carry more than four PES of a class; so does the partial member
            assert st[1025] == ST["pes_overflow"] and st["partial"] == ST["bad_length"] | ST["pes_overflow"]
        else:
            assert all(st[k] == 0 for k in COUNTS[2:]) and st["partial"] == ST["bad_length"]
        assert ri[:, I["n_packets"]].tolist() == COUNTS + [257]
        got = ref if dev == "cpu" else _demux(device, buf, offs, nbytes, eo, es_len, max_pes)
        _assert_demux_equal(got, ref, eo)
    # liveness: a member cut by one packet (1025 -> 1024) no longer matches the expectation
    cut = list(nbytes)
    cut[COUNTS.index(1025)] -= PKT
    got = _demux(device, buf, offs, cut, eo, es_len, 4)
    bad = np.flatnonzero((_np(got.info) != ri).any(axis=1))
    assert bad.tolist() == [COUNTS.index(1025)]


# ------------------------------------------------------------------ 3. mixed transmux batch
def _keep_tensors(keep):
    """transmux.cpp: after the per-group scratch tuples come dec, desc and hdr_rec."""
    return [k for k in keep if isinstance(k, torch.Tensor)]


def _mixed_batch(seg):
    """~70 members: encrypted and clear alternate irregularly, three clear members are empty (one
    of them last), two encrypted ones carry the round keys of another key."""
    rng = np.random.default_rng(41)
    B = 70
    enc = rng.random(B) < 0.55
    ks = [COUNTS[int(x)] for x in rng.integers(0, len(COUNTS), B)]
    for i in (9, 37, B - 1):
        enc[i], ks[i] = False, 0
    wrong = [14, 52]
    for i in wrong:
        enc[i], ks[i] = True, 1023
    enc[0], enc[1], enc[2] = True, False, False
    key_of = [_KEYS[i % 3] for i in range(B)]
    ivs = rng.integers(0, 256, (B, 16), dtype=np.uint8)
    payloads, plains = [], []
    for i in range(B):
        p = seg[:ks[i] * PKT]
        plains.append(p)
        payloads.append(aes.cbc_encrypt(key_of[i], ivs[i].tobytes(), p) if enc[i] else p)
    used = list(key_of)
    for i in wrong:
        used[i] = bytes(16)
    so, pos = np.empty(B, np.int64), 32
    for i, p in enumerate(payloads):
        so[i] = pos
        pos = (pos + len(p) + 15) // 16 * 16 + 16 * (1 + i % 3)
    src = np.full(pos + 256, 0xA5, np.uint8)
    for o, p in zip(so, payloads):
        src[o:o + len(p)] = p
    nb = np.array([len(p) for p in payloads], np.int64)
    return src, so, nb, enc, used, ivs, wrong


def _mixed_reference(src, so, nb, enc, used, ivs, max_pes):
    """The CPU oracle per group: CPU-tensor decrypt, then the serial CPU demux of the plaintext
    with the decrypt's lengths (encrypted group) or of the payloads in place (clear group)."""
    out = {}
    e = np.flatnonzero(enc)
    do = np.concatenate([[0], np.cumsum((nb[e] + 255) // 256 * 256)])[:-1]
    dec = torch.full((int(do[-1] + nb[e[-1]]) + 512,), SENTINEL, dtype=torch.uint8)
    lens = aes.cbc_decrypt_batch(torch.from_numpy(src), so[e], nb[e], [used[i] for i in e],
                                 [ivs[i].tobytes() for i in e], dec, do)
    es = torch.full((int(do[-1] + nb[e[-1]]) + 512,), SENTINEL, dtype=torch.uint8)
    out["enc"] = (e, tsdemux.demux_batch(dec, do, lens, es, do, caps=nb[e], max_pes=max_pes), lens.numpy(), do)
    c = np.flatnonzero(~enc)
    ceo = np.concatenate([[0], np.cumsum((nb[c] + 255) // 256 * 256 + 256)])[:-1]
    ces = torch.full((int(ceo[-1] + nb[c[-1]]) + 512,), SENTINEL, dtype=torch.uint8)
    out["clear"] = (c, tsdemux.demux_batch(torch.from_numpy(src), so[c], nb[c], ces, ceo, max_pes=max_pes), nb[c], ceo)
    return out


def _transmux(cuda, src, so, nb, enc, used, ivs, max_pes, expect=None):
    td0, isb = aes.device_tables(cuda)
    drk = np.stack([aes.round_keys_le(k) for k in used]).astype(np.uint32)
    extra = ()
    if expect is not None:
        extra = (np.asarray(expect, np.int64),) + tuple(crc.fused_consts(cuda))
    out = _dev().transmux_launch(torch.from_numpy(src).to(cuda), np.asarray(so, np.int64), np.asarray(nb, np.int64),
                                 np.asarray(enc, np.uint8), drk, np.ascontiguousarray(ivs), td0, isb, max_pes, *extra)
    torch.cuda.synchronize()
    return out


def _as_groups(ref):
    """The oracle's results in the form ``transmux_launch`` returns its groups."""
    return [(idx, r.info, r.pes, r.es, reo, r.info, torch.from_numpy(np.asarray(lens)))
            for idx, r, lens, reo in (ref["enc"], ref["clear"])]


def _group_mismatches(groups, ref):
    """Batch indices whose info row, PES table or ES bytes differ from the oracle's."""
    bad = []
    by_first = {int(g[0][0]): g for g in groups}
    for name in ("enc", "clear"):
        idx, r, lens, reo = ref[name]
        g_idx, info, pes, es, eo, hinfo, hlens = by_first[int(idx[0])]
        assert np.array_equal(np.asarray(g_idx), idx)
        gi, ri = _np(info), r.info.numpy()
        # the pinned host copies carry what the device tensors hold, and the oracle's lengths
        assert np.array_equal(hinfo.numpy(), gi)
        assert np.array_equal(np.asarray(hlens.numpy() if isinstance(hlens, torch.Tensor) else hlens), lens)
        gp, rp, ges, res = _np(pes), r.pes.numpy(), _np(es), r.es.numpy()
        for m, i in enumerate(idx.tolist()):
            n = int(ri[m, I["payload_bytes"]])
            a, b = int(eo[m]), int(reo[m])
            if not (np.array_equal(gi[m], ri[m]) and np.array_equal(gp[m], rp[m])
                    and np.array_equal(ges[a:a + n], res[b:b + n])):
                bad.append(i)
    return bad


@pytest.mark.parametrize("dev", DEVICES)
def test_transmux_mixed_batch_matches_cpu_oracle(dev, request, stream):
    """One native transmux call over encrypted and clear members of boundary packet counts, with
    empty clear members and two decrypts that fail: each group's info rows, PES tables and ES
    bytes equal the CPU oracle's, and a failed member reports ``bad_length`` and nothing else."""
    device, _ = _device(dev, request)
    seg, _ = stream
    src, so, nb, enc, used, ivs, wrong = _mixed_batch(seg)
    assert 20 < enc.sum() < 50 and (np.diff(np.flatnonzero(np.diff(enc.astype(int)))) > 1).any()
    assert (nb[~enc] == 0).sum() >= 3 and nb[-1] == 0 and not enc[-1]
    ref = _mixed_reference(src, so, nb, enc, used, ivs, tsdemux.DEFAULT_MAX_PES)
    e, r, lens, _ = ref["enc"]
    failed = [int(np.flatnonzero(e == i)[0]) for i in wrong]
    assert np.flatnonzero(lens < 0).tolist() == failed
    ri = r.info.numpy()
    for m in failed:  # bad_length (with the no_pat of an empty member) and no packets, bytes or PES
        assert ri[m, I["status"]] == ST["bad_length"] | ST["no_pat"]
        assert not ri[m, I["n_packets"]:I["payload_bytes"] + 1].any()
    ok_rows = np.setdiff1d(np.arange(len(e)), failed)
    assert not (ri[ok_rows, I["status"]] & ST["bad_length"]).any()

    def run(src):
        if dev == "cpu":
            return _as_groups(_mixed_reference(src, so, nb, enc, used, ivs, tsdemux.DEFAULT_MAX_PES)), None
        groups, keep, _, _ = _transmux(device, src, so, nb, enc, used, ivs, tsdemux.DEFAULT_MAX_PES)
        return groups, keep  # keep: the batch's scratch lives until the results are read

    groups, keep = run(src)
    assert _group_mismatches(groups, ref) == []
    # liveness: one ciphertext byte in the payload of an encrypted member that decrypts
    j = next(i for i in range(len(nb)) if enc[i] and i not in wrong and nb[i] >= 63 * PKT)
    src2 = src.copy()
    src2[so[j] + 40 * PKT + 100] ^= 0x10
    groups2, keep2 = run(src2)
    assert _group_mismatches(groups2, ref) == [j]
    del keep, keep2


# ------------------------------------------------------------------ 4. fused decrypt variants
_FUSED_SIZES = [16, 4096, 4112, 188 * 300, 300_000, 1_000_016]


def _fused_batch():
    rng = np.random.default_rng(51)
    B = len(_FUSED_SIZES)
    assert all(n % 16 == 0 for n in _FUSED_SIZES)
    ivs = rng.integers(0, 256, (B, 16), dtype=np.uint8)
    keys = [_KEYS[i % 3] for i in range(B)]
    plains = []  # the full decrypt output: plaintext followed by its PKCS#7 run
    so, pos = np.empty(B, np.int64), 16
    cts = []
    for i, n in enumerate(_FUSED_SIZES):
        pad = 1 + (5 * i) % 16
        p = rng.integers(0, 256, n - pad, dtype=np.uint8)
        cts.append(aes.cbc_encrypt(keys[i], ivs[i].tobytes(), p))
        assert len(cts[-1]) == n
        plains.append(np.concatenate([p, np.full(pad, pad, np.uint8)]))
        so[i] = pos
        pos += n + 16 * (1 + i % 3)
    src = np.full(pos + 256, 0xA5, np.uint8)
    for o, c in zip(so, cts):
        src[o:o + len(c)] = c
    return src, so, np.array(_FUSED_SIZES, np.int64), keys, ivs, plains


def _host_raw_decrypt(src, so, nb, keys, ivs):
    """Host decrypt of every member, padding run included (``out[i]`` has ``nb[i]`` bytes)."""
    do = np.concatenate([[0], np.cumsum(nb)])[:-1]
    dst = torch.zeros(int(nb.sum()), dtype=torch.uint8)
    lens = aes.cbc_decrypt_batch(torch.from_numpy(src), so, nb, keys, [v.tobytes() for v in ivs], dst, do)
    d = dst.numpy()
    return [d[o:o + n] for o, n in zip(do, nb)], lens.numpy()


def _assert_fused_outputs(keep, nb, plains):
    """The decrypt buffer holds every member's whole plaintext, and record q of a member is the
    16-byte plaintext block that holds byte 188 q (the packet's TS header)."""
    dec, _, hdr_rec = _keep_tensors(keep)[:3]
    dec, rec = _np(dec), _np(hdr_rec).reshape(-1, 16)
    dpos = hpos = 0
    for n, p in zip(nb.tolist(), plains):
        assert np.array_equal(dec[dpos:dpos + n], p)
        q = np.arange((n + PKT - 1) // PKT)  # packets with 188 q < nbytes
        blocks = p[((PKT * q) // 16 * 16)[:, None] + np.arange(16)]
        assert np.array_equal(rec[hpos + q], blocks)
        dpos += (n + 255) // 256 * 256
        hpos += n // PKT + 2
    assert hpos <= len(rec)


@pytest.mark.parametrize("dev", DEVICES)
def test_fused_decrypt_variants_byte_for_byte(dev, request):
    """``aes128_cbc_decrypt_kernel<0,1>`` (header records) and ``<1,1>`` (records + fused CRC), the
    kernels the node runs: whole plaintext, every header record and the CRC flags."""
    device, _ = _device(dev, request)
    src, so, nb, keys, ivs, plains = _fused_batch()
    B = len(nb)
    raw, lens = _host_raw_decrypt(src, so, nb, keys, ivs)
    assert all(np.array_equal(a, b) for a, b in zip(raw, plains))  # the reference meets the expectation
    assert lens.tolist() == [n - int(p[-1]) for n, p in zip(nb.tolist(), plains)]
    crcs = [zlib.crc32(src[o:o + n].tobytes()) for o, n in zip(so.tolist(), nb.tolist())]
    flip = _FUSED_SIZES.index(300_000)
    src2 = src.copy()
    src2[so[flip] + 123_457] ^= 0x80
    raw2, _ = _host_raw_decrypt(src2, so, nb, keys, ivs)
    assert not np.array_equal(raw2[flip], plains[flip])
    if dev == "cpu":
        return
    enc = np.ones(B, np.uint8)
    for expect in (None, crcs):
        groups, keep, _, verify = _transmux(device, src, so, nb, enc, keys, ivs, tsdemux.DEFAULT_MAX_PES, expect)
        _assert_fused_outputs(keep, nb, plains)
        assert np.array_equal(groups[0][6].numpy(), lens)
        if expect is None:
            assert verify is None
        else:
            assert np.asarray(verify[0]).tolist() == list(range(B)) and verify[1].tolist() == [1] * B
    # one ciphertext byte flipped: only that member's ok drops; its plaintext is still the host's
    # decrypt of what was given
    groups, keep, _, verify = _transmux(device, src2, so, nb, enc, keys, ivs, tsdemux.DEFAULT_MAX_PES, crcs)
    assert np.flatnonzero(verify[1].numpy() == 0).tolist() == [flip]
    _assert_fused_outputs(keep, nb, raw2)
    with pytest.raises(AssertionError):  # liveness of the byte comparison itself
        _assert_fused_outputs(keep, nb, plains)


# ------------------------------------------------------------------ 5. PKCS#7 table
_PKCS_BLOCKS = [1, 2, 64, 65, 193, 256, 257]  # last block on lane 0 / 63, chains 0..3, second chunk


def _pkcs_cases(r):
    """(last plaintext block, plaintext length relative to the ciphertext size n; None = -1)."""
    r = [int(x) for x in r]
    return [(r[:15] + [0], None), (r[:15] + [17], None), (r[:15] + [255], None), ([16] * 16, 16),
            ([15] + [16] * 15, None), (r[:15] + [1], 1), (r[:14] + [3, 2], None), (r[:14] + [2, 2], 2),
            ([99] + [15] * 15, 15), ([99, 14] + [15] * 14, None)]


@pytest.mark.parametrize("dev", DEVICES)
def test_pkcs7_table_on_every_lane_position(dev, request):
    """Pad 0, 17, 255, a full block, a wrong leading byte, a mismatch inside the run -- each with
    the padding block on lane 0 and lane 63, on each of the four chains and in a second chunk."""
    device, _ = _device(dev, request)
    rng = np.random.default_rng(61)
    members = []
    for nblk in _PKCS_BLOCKS:
        for last, pad in _pkcs_cases(rng.integers(17, 256, 16)):
            n = 16 * nblk
            P = np.concatenate([rng.integers(0, 256, n - 16, dtype=np.uint8), np.array(last, np.uint8)])
            members.append((P, -1 if pad is None else n - pad))
    B = len(members)
    assert B == 70
    keys = [_KEYS[i % 3] for i in range(B)]
    ivs = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes() for _ in range(B)]
    nb = np.array([len(P) for P, _ in members], np.int64)
    so = np.concatenate([[0], np.cumsum(nb + 16 * (1 + np.arange(B) % 3))])[:-1] + 16
    src = np.full(int(so[-1] + nb[-1]) + 256, 0xA5, np.uint8)
    for i, (P, _) in enumerate(members):
        ct = aes.cbc_encrypt(keys[i], ivs[i], P)[:-16]  # drop the encryptor's own padding block
        assert len(ct) == len(P)
        src[so[i]:so[i] + len(ct)] = ct
    want = np.array([w for _, w in members], np.int64)

    def run(device, src):
        d = torch.full((len(src),), SENTINEL, dtype=torch.uint8, device=device)
        out = aes.cbc_decrypt_batch(torch.from_numpy(src).to(device), so, nb, keys, ivs, d, so)
        return _np(out), _np(d)

    ref_len, ref_d = run(torch.device("cpu"), src)
    assert np.array_equal(ref_len, want)  # the host oracle gives the table of the specification
    got_len, got_d = (ref_len, ref_d) if dev == "cpu" else run(device, src)
    assert np.array_equal(got_len, ref_len)
    for i, (P, _) in enumerate(members):  # the bytes are decrypted whether or not the padding holds
        assert np.array_equal(got_d[so[i]:so[i] + len(P)], P), i
    # liveness: the last byte of a 65-block member's block 63 flips its pad byte 16 -> 17
    j = _PKCS_BLOCKS.index(65) * 10 + 3
    assert want[j] == 65 * 16 - 16
    src2 = src.copy()
    src2[so[j] + 64 * 16 - 1] ^= 0x01
    got2, _ = run(device, src2)
    assert np.flatnonzero(got2 != ref_len).tolist() == [j] and got2[j] == -1


# ------------------------------------------------------------------ 6. copy kernel
_COPY_PAIRS = [(0, 0), (0, 1), (1, 0), (5, 5), (8, 8), (3, 11)]  # (src % 16, dst % 16)
_COPY_LENS = [1, 15, 16, 17, 31, 65_535, 65_536, 65_537, 131_077]


def _copy_batch():
    rng = np.random.default_rng(71)
    items = [(n, p) for n in _COPY_LENS for p in _COPY_PAIRS] + [(n, p) for n in (1, 17, 65_537) for p in _COPY_PAIRS]
    items = [items[i] for i in rng.permutation(len(items))]
    for at in (10, 30, 30, 30, 55):  # empty copies: one, three in a row, one more, and the last
        items.insert(at, (0, _COPY_PAIRS[at % 6]))
    items.append((0, (3, 11)))
    so, do, n = [], [], []
    spos, dpos = 0, 7
    for i, (length, (a, b)) in enumerate(items):
        spos = (spos + 15) // 16 * 16 + a
        g = 1 + i % 24
        while (dpos + g) % 16 != b:
            g += 1
        assert 1 <= g <= 40
        dpos += g
        so.append(spos)
        do.append(dpos)
        n.append(length)
        spos += length
        dpos += length
    src = np.full(spos + 64, 0x5A, np.uint8)  # the two buffers start from different sentinels
    for a, c in zip(so, n):
        src[a:a + c] = rng.integers(0, 256, c, dtype=np.uint8)
    return src, np.array(so), np.array(do), np.array(n), dpos + 300


@pytest.mark.parametrize("dev", DEVICES)
def test_copy_segments_tails_alignment_and_untouched_bytes(dev, request):
    """~80 copies: empty ones (middle, three in a row, last), lengths around 16 bytes and around
    the 64 KiB chunk, six alignment pairs, destinations 1..40 bytes apart.  The whole destination
    is compared, so a byte written outside a copy's range shows."""
    device, _ = _device(dev, request)
    src, so, do, n, dlen = _copy_batch()
    assert 75 <= len(n) <= 85 and n[-1] == 0 and ((n[:-2] == 0) & (n[1:-1] == 0) & (n[2:] == 0)).any()
    assert {(int(a) % 16, int(b) % 16) for a, b in zip(so, do)} == set(_COPY_PAIRS)
    assert (do[1:] - (do[:-1] + n[:-1]) >= 1).all() and (do[1:] - (do[:-1] + n[:-1]) <= 40).all()

    def reference(src):
        ref = np.full(dlen, SENTINEL, np.uint8)
        for a, b, c in zip(so.tolist(), do.tolist(), n.tolist()):
            ref[b:b + c] = src[a:a + c]
        return ref

    def run(src):
        d = torch.full((dlen,), SENTINEL, dtype=torch.uint8, device=device)
        segment.copy_segments(torch.from_numpy(src).to(device), d, so, do, n)
        return _np(d)

    ref = reference(src)
    assert np.array_equal(run(src), ref)
    # liveness: one source byte in the second chunk of a 131 077-byte copy
    j = int(np.flatnonzero(n == 131_077)[3])
    src2 = src.copy()
    src2[so[j] + 70_000] ^= 0x55
    assert np.flatnonzero(run(src2) != ref).tolist() == [int(do[j]) + 70_000]


# ------------------------------------------------------------------ 7. range validation (host side)
def test_copy_segments_rejects_bad_ranges():
    src, dst = torch.zeros(256, dtype=torch.uint8), torch.zeros(256, dtype=torch.uint8)
    with pytest.raises(ValueError, match="copy_segments: negative source offset"):
        segment.copy_segments(src, dst, [-16], [0], [16])
    with pytest.raises(ValueError, match="copy_segments: negative destination offset"):
        segment.copy_segments(src, dst, [0], [-16], [16])
    with pytest.raises(ValueError, match="copy_segments: negative length"):
        segment.copy_segments(src, dst, [32], [32], [-16])
    with pytest.raises(ValueError, match="copy_segments: source range out of bounds"):
        segment.copy_segments(src, dst, [250], [0], [16])
    with pytest.raises(ValueError, match="copy_segments: destination range out of bounds"):
        segment.copy_segments(src, dst, [0], [250], [16])
    assert not dst.any()
    segment.copy_segments(src + 1, dst, [0, 240], [240, 0], [16, 16])  # the edges themselves are fine
    assert dst[:16].all() and dst[240:].all() and not dst[16:240].any()


def test_cbc_decrypt_batch_rejects_bad_ranges():
    key, iv = _KEYS[0], bytes(16)
    ct = aes.cbc_encrypt(key, iv, np.arange(40, dtype=np.uint8))
    src = torch.from_numpy(np.concatenate([np.zeros(16, np.uint8), ct]))
    dst = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="cbc_decrypt_batch: negative source offset"):
        aes.cbc_decrypt_batch(src, [-16], [16], [key], [iv], dst, [0])
    with pytest.raises(ValueError, match="cbc_decrypt_batch: negative destination offset"):
        aes.cbc_decrypt_batch(src, [16], [16], [key], [iv], dst, [-16])
    with pytest.raises(ValueError, match="cbc_decrypt_batch: source range out of bounds"):
        aes.cbc_decrypt_batch(src, [32], [48], [key], [iv], dst, [0])
    with pytest.raises(ValueError, match="cbc_decrypt_batch: destination range out of bounds"):
        aes.cbc_decrypt_batch(src, [16], [48], [key], [iv], dst, [32])
    with pytest.raises(ValueError, match="cbc_decrypt_batch: negative length"):
        aes.cbc_decrypt_batch(src, [16], [-16], [key], [iv], dst, [0])
    assert not dst.any()
    assert aes.cbc_decrypt_batch(src, [16], [48], [key], [iv], dst, [16]).tolist() == [40]
    assert dst[16:56].tolist() == list(range(40))


def test_demux_batch_rejects_bad_ranges(stream):
    seg, _ = stream
    n = 64 * PKT
    buf = torch.from_numpy(seg[:n].copy())
    es = torch.zeros(n, dtype=torch.uint8)
    with pytest.raises(ValueError, match="demux_batch: negative source offset"):
        tsdemux.demux_batch(buf, [-PKT], [PKT], es, [0])
    with pytest.raises(ValueError, match="demux_batch: negative ES offset"):
        tsdemux.demux_batch(buf, [0], [PKT], es, [-16])
    with pytest.raises(ValueError, match="demux_batch: negative length"):
        tsdemux.demux_batch(buf, [0], [-PKT], es, [0])
    with pytest.raises(ValueError, match="demux_batch: negative length"):  # host bounds of device lengths
        tsdemux.demux_batch(buf, [0], torch.tensor([n]), es, [0], caps=[-PKT])
    with pytest.raises(ValueError, match="demux_batch: source range out of bounds"):
        tsdemux.demux_batch(buf, [PKT], [n], es, [0])
    with pytest.raises(ValueError, match="demux_batch: ES range out of bounds"):
        tsdemux.demux_batch(buf, [0], [n], es, [16])
    assert not es.any()
    res = tsdemux.demux_batch(buf, [0], torch.tensor([-1]), es, [0], caps=[n])  # a failed decrypt's length is legal
    assert int(res.info[0, I["status"]]) & ST["bad_length"]
    assert int(tsdemux.demux_batch(buf, [0], [n], es, [0]).info[0, I["n_packets"]]) == 64
