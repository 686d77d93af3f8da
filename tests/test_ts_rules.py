"""The demux's PSI and per-packet rules against stated expectations.

The host oracle and the kernels call the same rule functions (``ops/csrc/shared/grammar.hpp``), so
"cpu leg equals cuda leg" no longer checks a rule.  Here every malformed-packet and PSI-window
case has its status bits, byte and PES counts, PES rows and ES bytes written down as literals, and
both legs must give them: ``cpu`` through the host demux, ``cuda`` through the kernels (all cases
as one batch), and once more through the fused decrypt + demux path, where the scan takes its
header bytes from the decrypt's records.

Unless a case says otherwise a segment is PAT (program 1 -> PMT 0x1000), PMT (0x1B on 0x100, 0x0F
on 0x101), one good video PES packet *G* (PUSI, PTS 1000 only, ``PES_header_data_length`` 5, 170 ES
bytes), the malformed video packet *M* and a plain 184-byte video continuation *C*.
"""
import numpy as np
import pytest
import torch

from hlsjs_p2p_wrapper_amd.ops import aes, tsdemux
from test_kernel_shapes import _KEYS, _transmux
from ts_builder import _section, _ts_timestamp

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
I = tsdemux.INFO
PKT = tsdemux.PACKET
MAX_PES = 4
VPID, APID, PMTPID = 0x100, 0x101, 0x1000
SENTINEL = 0xEE

_rng = np.random.default_rng(81)
ES_G = _rng.integers(0, 256, 170, dtype=np.uint8).tobytes()
ES_C = _rng.integers(0, 256, 184, dtype=np.uint8).tobytes()


def _pkt(pid, body, pusi=False, afc=1, sync=0x47):
    """A raw packet: 4 header bytes, then ``body`` cut or padded with 0xFF to 184 bytes."""
    body = (body + b"\xff" * 184)[:184]
    return bytes([sync, (0x40 if pusi else 0) | ((pid >> 8) & 0x1F), pid & 0xFF, afc << 4]) + body


def _af(length, payload=b""):
    """``adaptation_field_length``, a field of that many bytes (flags 0, stuffing), the payload."""
    return bytes([length]) + (b"\x00" + b"\xff" * (length - 1) if length else b"") + payload


def _af_leaving(room, payload):
    """An adaptation field that leaves exactly ``room`` payload bytes."""
    assert len(payload) == room
    return _af(184 - 1 - room, payload)


def _pes_head(flags, hdl, opt=b""):
    return b"\x00\x00\x01\xe0\x00\x00\x80" + bytes([flags, hdl]) + opt


PAT = _pkt(0, b"\x00" + _section(0x00, 1, bytes([0x00, 0x01, 0xE0 | (PMTPID >> 8), PMTPID & 0xFF])), pusi=True)
PMT = _pkt(PMTPID, b"\x00" + _section(0x02, 1, bytes([0xE0 | (VPID >> 8), VPID & 0xFF, 0xF0, 0x00,
                                                      0x1B, 0xE0 | (VPID >> 8), VPID & 0xFF, 0xF0, 0x00,
                                                      0x0F, 0xE0 | (APID >> 8), APID & 0xFF, 0xF0, 0x00])), pusi=True)
NULL = _pkt(0x1FFF, b"")
G = _pkt(VPID, _pes_head(0x80, 5, _ts_timestamp(0x2, 1000)) + ES_G, pusi=True)
C = _pkt(VPID, ES_C)
assert len(G) == len(C) == len(PAT) == len(PMT) == PKT and G[18:] == ES_G


def _around(m):
    return PAT + PMT + G + m + C


def _header_ending_at(hdl):
    """*M* with a 184-byte payload: PUSI, flags 0, ``PES_header_data_length`` ``hdl``."""
    return _pkt(VPID, _pes_head(0x00, hdl), pusi=True)


M_AF_TOO_LONG = _pkt(VPID, _af(184), afc=3)
ROW_G = (0, 1000, -1)
# name -> (segment bytes, status, video_bytes, n_video_pes, video PES rows, video ES, other info slots)
CASES = {
    "bad sync": (_around(_pkt(VPID, ES_C, sync=0x48)), 1, 354, 1, [ROW_G], ES_G + ES_C, {}),
    "AF too long": (_around(M_AF_TOO_LONG), 32, 354, 1, [ROW_G], ES_G + ES_C, {}),
    "AF fills packet": (_around(_pkt(VPID, _af(183), afc=3)), 0, 354, 1, [ROW_G], ES_G + ES_C, {}),
    "PES in 8 bytes": (_around(_pkt(VPID, _af_leaving(8, _pes_head(0x00, 0)[:8]), pusi=True, afc=3)),
                       16, 354, 1, [ROW_G], ES_G + ES_C, {}),
    "bad prefix": (_around(_pkt(VPID, b"\x00\x00\x02" + _pes_head(0x00, 0)[3:], pusi=True)),
                   16, 354, 1, [ROW_G], ES_G + ES_C, {}),
    "header past packet": (_around(_header_ending_at(176)), 16, 354, 1, [ROW_G], ES_G + ES_C, {}),
    "header fills packet": (_around(_header_ending_at(175)), 0, 354, 2, [ROW_G, (170, -1, -1)], ES_G + ES_C, {}),
    "PTS flag, 13 bytes": (_around(_pkt(VPID, _af_leaving(13, _pes_head(0x80, 4, b"\xff" * 4)), pusi=True, afc=3)),
                           0, 354, 2, [ROW_G, (170, -1, -1)], ES_G + ES_C, {}),
    "DTS flag, 18 bytes": (_around(_pkt(VPID, _af_leaving(18, _pes_head(0xC0, 9, _ts_timestamp(0x3, 2000)
                                                                         + _ts_timestamp(0x1, 1500)[:4])),
                                        pusi=True, afc=3)),
                           0, 354, 2, [ROW_G, (170, 2000, -1)], ES_G + ES_C, {}),
    "PAT at packet 64": (NULL * 64 + PAT + PMT + G, 2, 0, 0, [], b"", {"video_pid": -1, "n_packets": 67}),
    "PAT at packet 62": (NULL * 62 + PAT + PMT + G, 0, 170, 1, [ROW_G], ES_G, {}),
    "no PMT": (PAT + G + C, 4, 0, 0, [], b"", {"video_pid": -1}),
    "ragged tail": (PAT + PMT + G + C[:100], 32, 170, 1, [ROW_G], ES_G, {"n_packets": 3}),
    "PES overflow": (PAT + PMT + G * 5, 8, 850, 5, [(0, 1000, -1), (170, 1000, -1), (340, 1000, -1), (510, 1000, -1)],
                     ES_G * 5, {}),
}
assert all(3 * PKT <= len(c[0]) <= 67 * PKT for c in CASES.values())
# the fused path only: two null packets ahead of G put *M* at packet 5, whose header sits at byte
# 188 * 5 % 16 == 12 of its 16-byte record, so byte 4 (the adaptation field length) is not in the
# record and comes from the plaintext.  Nothing but n_packets changes.
AF_TOO_LONG_AT_12 = (PAT + PMT + NULL * 2 + G + M_AF_TOO_LONG + C, 32, 354, 1, [ROW_G], ES_G + ES_C, {"n_packets": 7})
assert AF_TOO_LONG_AT_12[0][5 * PKT:6 * PKT] == M_AF_TOO_LONG and PKT * 5 % 16 == 12


def _check(case, info, pes, es):
    """One segment's info row, PES table ``[3, MAX_PES, 3]`` and ES bytes against the literals."""
    _, status, video_bytes, n_video_pes, rows, video_es, other = case
    assert info[I["status"]] == status
    assert info[I["video_bytes"]] == video_bytes and info[I["n_video_pes"]] == n_video_pes
    assert pes[0].tolist() == [list(r) for r in rows] + [[-1, -1, -1]] * (MAX_PES - len(rows))
    assert bytes(es[:video_bytes]) == video_es[:video_bytes] and len(video_es) == video_bytes
    for slot, value in other.items():
        assert info[I[slot]] == value, slot


def _demux(cases, device):
    """All segments as one batch at 16-aligned offsets: (info, pes, [ES bytes per segment])."""
    segs = [c[0] for c in cases]
    offs = np.concatenate([[0], np.cumsum([(len(s) + 15) // 16 * 16 + 16 for s in segs])])[:-1]
    buf = np.full(int(offs[-1]) + len(segs[-1]) + 256, 0xA5, np.uint8)
    for o, s in zip(offs, segs):
        buf[o:o + len(s)] = np.frombuffer(s, np.uint8)
    es = torch.full((len(buf),), SENTINEL, dtype=torch.uint8, device=device)
    r = tsdemux.demux_batch(torch.from_numpy(buf).to(device), offs, [len(s) for s in segs], es, offs, max_pes=MAX_PES)
    es = r.es.cpu().numpy()
    return r.info.cpu().numpy(), r.pes.cpu().numpy(), [es[o:o + len(s)] for o, s in zip(offs, segs)]


@pytest.mark.parametrize("dev", DEVICES)
def test_demux_rules_give_the_stated_rows(dev, request):
    device = request.getfixturevalue("cuda") if dev == "cuda" else torch.device("cpu")
    names = list(CASES)
    info, pes, es = _demux([CASES[n] for n in names], device)
    for k, name in enumerate(names):
        try:
            _check(CASES[name], info[k], pes[k], es[k])
        except AssertionError as e:
            raise AssertionError(f"case {name!r}: {e}") from e
    # liveness: PES_header_data_length 176 -> 175 no longer meets the "header past packet" row
    changed = (_around(_header_ending_at(175)),) + CASES["header past packet"][1:]
    info, pes, es = _demux([changed], device)
    with pytest.raises(AssertionError):
        _check(changed, info[0], pes[0], es[0])
    assert info[0, I["status"]] == 0 and info[0, I["n_video_pes"]] == 2


@pytest.mark.gpu
def test_fused_decrypt_demux_gives_the_stated_rows(cuda):
    """The same table, encrypted, through the native transmux call: the scan reads packet headers
    and byte 4 from the decrypt's header records."""
    names = list(CASES) + ["AF too long, header at byte 12"]
    cases = [CASES[n] for n in names[:-1]] + [AF_TOO_LONG_AT_12]
    B = len(cases)
    rng = np.random.default_rng(82)
    keys = [_KEYS[i % 3] for i in range(B)]
    ivs = rng.integers(0, 256, (B, 16), dtype=np.uint8)

    def run(cases):
        cts = [aes.cbc_encrypt(keys[i], ivs[i].tobytes(), np.frombuffer(c[0], np.uint8)) for i, c in enumerate(cases)]
        nb = np.array([len(ct) for ct in cts], np.int64)
        so = np.concatenate([[0], np.cumsum((nb + 15) // 16 * 16 + 16)])[:-1] + 32
        src = np.full(int(so[-1] + nb[-1]) + 256, 0xA5, np.uint8)
        for o, ct in zip(so, cts):
            src[o:o + len(ct)] = ct
        groups, keep, _, _ = _transmux(cuda, src, so, nb, np.ones(len(cases), np.uint8), keys[:len(cases)],
                                       ivs[:len(cases)], MAX_PES)
        (idx, info, pes, es, eo, _, lens), = groups
        assert np.asarray(idx).tolist() == list(range(len(cases)))
        assert lens.tolist() == [len(c[0]) for c in cases]
        info, pes, es = info.cpu().numpy(), pes.cpu().numpy(), es.cpu().numpy()
        del keep  # the batch's scratch lived until the results were read
        return info, pes, [es[int(eo[m]):int(eo[m]) + len(c[0])] for m, c in enumerate(cases)]

    info, pes, es = run(cases)
    for k, name in enumerate(names):
        try:
            _check(cases[k], info[k], pes[k], es[k])
        except AssertionError as e:
            raise AssertionError(f"case {name!r}: {e}") from e
    # liveness: adaptation_field_length 184 -> 183 at the byte the record does not hold
    seg = bytearray(AF_TOO_LONG_AT_12[0])
    assert seg[5 * PKT + 4] == 184
    seg[5 * PKT + 4] = 183
    changed = (bytes(seg),) + AF_TOO_LONG_AT_12[1:]
    info, pes, es = run([changed])
    with pytest.raises(AssertionError):
        _check(changed, info[0], pes[0], es[0])
    assert info[0, I["status"]] == 0
