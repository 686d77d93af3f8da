"""The PMT selection of AC-3 (``0x81``) and E-AC-3 (``0x87``) streams through ``ts_demux`` (host and
MI355X): a Dolby stream is the audio class only where no AAC / MPEG audio stream is listed, wherever
it stands in the PMT; the first of two Dolby streams wins; the SAMPLE-AES types ``0xC1`` / ``0xC2``
select nothing.  The TS is built with the packet helpers of ``mpegaudio_cases.py`` and a PMT of its
own."""
import numpy as np
import pytest
import torch

import ac3audio_cases as ac
import esindex_cases as ec
import mpegaudio_cases as mc
from hlsjs_p2p_wrapper_amd.ops import tsdemux

PIDS = (0x101, 0x102, 0x103)


def mux(streams, payloads, video=True) -> bytes:
    """PAT, a PMT listing (video and) ``streams`` = ``(stream_type, pid)`` in that order, one video
    PES, then two PES of ``payloads[pid]`` per listed audio PID."""
    body = (bytes([0x1B]) + (0xE000 | mc.VIDEO_PID).to_bytes(2, "big") + b"\xF0\x00") if video else b""
    for stype, pid in streams:
        body += bytes([stype]) + (0xE000 | pid).to_bytes(2, "big") + b"\xF0\x00"
    pcr = mc.VIDEO_PID if video else streams[0][1]
    out = mc._psi_packet(0, mc._section(0x00, 1, (1).to_bytes(2, "big") + (0xE000 | mc.PMT_PID).to_bytes(2, "big")))
    out += mc._psi_packet(mc.PMT_PID, mc._section(0x02, 1, (0xE000 | pcr).to_bytes(2, "big") + b"\xF0\x00" + body))
    if video:
        unit = ec.SC + b"\x09\xF0" + ec.SC + b"\x65" + bytes(range(1, 150))
        out += mc._pes_packets(mc.VIDEO_PID, 0xE0, 903600, 900000, unit, [0])
    for _, pid in streams:
        cc = [0]
        for j, chunk in enumerate(payloads[pid]):
            out += mc._pes_packets(pid, 0xBD, 900000 + 2880 * j, None, chunk, cc)
    return out


def demux(device, segments):
    caps = [len(s) for s in segments]
    offs = np.cumsum([0] + [(c + 255) // 256 * 256 for c in caps])[:-1]
    buf = torch.zeros(int(offs[-1]) + caps[-1] + 256, dtype=torch.uint8)
    for o, s in zip(offs, segments):
        buf[int(o):int(o) + len(s)] = torch.frombuffer(bytearray(s), dtype=torch.uint8)
    buf = buf.to(device)
    es = torch.zeros_like(buf)
    res = tsdemux.demux_batch(buf, offs, caps, es, offs, max_pes=8)
    return [res.segment(i) for i in range(len(segments))]


def cases():
    rng = np.random.default_rng(71)
    dolby = [b"".join(ac.small(rng, 128) for _ in range(2)) for _ in range(2)]
    edolby = [b"".join(ac.small(rng, 24) for _ in range(3)) for _ in range(2)]
    aac = [b"".join(ec.adts_frame(bytes(ec.background(rng, 60))) for _ in range(2)) for _ in range(2)]
    mp3 = [b"".join(mc.small(rng) for _ in range(2)) for _ in range(2)]
    a, b, c = PIDS
    return {
        "only_ac3": (mux([(0x81, a)], {a: dolby}), 0x81, a, b"".join(dolby)),
        "only_eac3": (mux([(0x87, a)], {a: edolby}), 0x87, a, b"".join(edolby)),
        "only_ac3_no_video": (mux([(0x81, a)], {a: dolby}, video=False), 0x81, a, b"".join(dolby)),
        "ac3_before_aac": (mux([(0x81, a), (0x0F, b)], {a: dolby, b: aac}), 0x0F, b, b"".join(aac)),
        "aac_alone": (mux([(0x0F, b)], {b: aac}), 0x0F, b, b"".join(aac)),
        "eac3_before_mp3": (mux([(0x87, a), (0x03, b)], {a: edolby, b: mp3}), 0x03, b, b"".join(mp3)),
        "aac_before_ac3": (mux([(0x0F, a), (0x81, b)], {a: aac, b: dolby}), 0x0F, a, b"".join(aac)),
        "two_dolby": (mux([(0x87, b), (0x81, a)], {a: dolby, b: edolby}), 0x87, b, b"".join(edolby)),
        "two_dolby_other_order": (mux([(0x81, c), (0x87, b)], {c: dolby, b: edolby}), 0x81, c, b"".join(dolby)),
        "sample_aes_ac3": (mux([(0xC1, a)], {a: dolby}), 0, -1, b""),
        "sample_aes_eac3": (mux([(0xC2, a)], {a: edolby}), 0, -1, b""),
        "dvb_private": (mux([(0x06, a)], {a: dolby}), 0, -1, b""),
    }


def check(device):
    table = cases()
    segs = demux(device, [v[0] for v in table.values()])
    got = dict(zip(table, segs))
    for name, (_, atype, pid, audio) in table.items():
        s = got[name]
        assert s["status"] == 0, name
        assert (s["audio_type"], s["audio_pid"]) == (atype, pid), name
        assert bytes(s["audio"]["es"].cpu().numpy()) == audio, name
        assert s["n_audio_pes"] == (2 if audio else 0), name
        if name != "only_ac3_no_video":
            assert (s["video_type"], s["video_pid"], s["n_video_pes"]) == (0x1B, mc.VIDEO_PID, 1), name
    # AC-3 listed in front of AAC: the info row and the ES of the same segment without the AC-3 stream
    # (the PID differs by construction; the packet count by the Dolby packets that are dropped)
    with_, without = got["ac3_before_aac"], got["aac_alone"]
    same = [k for k in tsdemux.INFO if k != "n_packets"]
    assert {k: with_[k] for k in same} == {k: without[k] for k in same}
    assert np.array_equal(with_["audio"]["pes"], without["audio"]["pes"])
    assert bytes(with_["video"]["es"].cpu().numpy()) == bytes(without["video"]["es"].cpu().numpy())
    return got


def test_pmt_selection_on_the_host():
    check("cpu")


@pytest.mark.gpu
def test_pmt_selection_on_the_device_equals_the_host(cuda):
    dev, cpu = check(cuda), check("cpu")
    for name in cpu:
        d, c = dev[name], cpu[name]
        assert {k: d[k] for k in tsdemux.INFO} == {k: c[k] for k in tsdemux.INFO}, name
        for cls in ("video", "audio"):
            assert np.array_equal(d[cls]["pes"], c[cls]["pes"]), (name, cls)
