"""MPEG audio behind the remux on the host implementation (``runtime/mpegaudio.cpp`` through
``ops.mpegaudio.mpeg_audio_batch``) against the independent reference of ``mpegaudio_cases.py``:
the header rule on every field combination and on literals stated by hand, the walk cases, the
overflow, a mixed batch whose other segments keep every byte, canaries, damaged PES rows, a fuzz,
and the boxes that go with the samples (init segment, ``moof``) through the independent box
walkers of ``codec_cases.py`` and ``remux_cases.py``."""
import struct

import numpy as np
import pytest
import torch

import codec_cases as cc
import mpegaudio_cases as mc
import remux_cases as rc
from hlsjs_p2p_wrapper_amd.ops import fragment, mpegaudio, remux
from hlsjs_p2p_wrapper_amd.ops._native import runtime
from hlsjs_p2p_wrapper_amd.player import fmp4
from test_codecconfig import tree

FIELDS = ("len", "samples", "rate", "channels", "version", "layer", "bitrate")


def host_frame(b: bytes, end=None):
    """``es::mpa_frame_at`` at byte 0 of ``b`` as a dict, ``None`` without a header."""
    ln, counts, key, *rest = runtime().mpa_frame(np.frombuffer(b, np.uint8), 0, len(b) if end is None else end)
    return None if ln == 0 else dict(zip(FIELDS, (ln, *rest)), counts=bool(counts), key=key)


def test_header_rule_on_every_field_combination():
    """4 x 4 x 16 x 4 x 2 headers (version, layer, bitrate index, rate index, padding), each for
    stereo and mono, first bytes FF Ex and FF Fx, and a first byte that is not FF."""
    keys = {}
    for V in range(4):
        for L in range(4):
            for bi in range(16):
                for ri in range(4):
                    for pad in range(2):
                        for b3 in (0x00, 0xC0, 0x40):
                            b1 = 0xE0 | (V << 3) | (L << 1) | (bi & 1)
                            h = bytes([0xFF, b1, (bi << 4) | (ri << 2) | (pad << 1), b3])
                            want, got = mc.ref_header(*h), host_frame(h + bytes(3000))
                            assert (want is None) == (got is None), h.hex()
                            if want is None:
                                continue
                            assert {k: got[k] for k in FIELDS} == {k: want[k] for k in FIELDS}, h.hex()
                            assert got["counts"] and not host_frame(h + bytes(want["len"] - 5))["counts"]
                            keys.setdefault(got["key"], set()).add(want["key"])
                            assert host_frame(bytes([0xFE]) + h[1:] + bytes(3000)) is None
                            assert host_frame(bytes([0xFF, h[1] & 0xDF]) + h[2:] + bytes(3000)) is None
    # the packed key is the reference's tuple
    assert all(len(v) == 1 for v in keys.values()) and len(keys) == 3 * 3 * 3 * 2


@pytest.mark.parametrize("hexbytes,want", [
    ("FFFB9000", dict(len=417, samples=1152, rate=44100, channels=2, version=1, layer=3, bitrate=128000)),
    ("FFFB9200", dict(len=418)),
    ("FFFA90C0", dict(len=417, channels=1)),
    ("FFFD9000", dict(len=522, layer=2, samples=1152)),
    ("FFFF9000", dict(len=312, layer=1, samples=384)),
    ("FFF38000", dict(len=208, samples=576, rate=22050, version=2)),
    ("FFE38000", dict(len=417, version=25, rate=11025, samples=576)),
    ("FFF31400", dict(len=24, rate=24000)),
    ("FFF31600", dict(len=25)),
    ("FFF31800", dict(len=36, rate=16000)),
    ("FFFB0000", None), ("FFFBF000", None), ("FFFB9C00", None), ("FFEB9000", None), ("FFF1500080", None),
])
def test_literals(hexbytes, want):
    for f in (host_frame(bytes.fromhex(hexbytes) + bytes(600)), mc.ref_header(*bytes.fromhex(hexbytes)[:4])):
        if want is None:
            assert f is None
        else:
            assert {k: f[k] for k in want} == want


def test_a_header_needs_four_bytes_and_a_frame_its_whole_length():
    f = bytes.fromhex("FFF31400") + bytes(20)
    assert host_frame(f, 3) is None and not host_frame(f, 4)["counts"] and not host_frame(f, 23)["counts"]
    assert host_frame(f, 24)["counts"]


@pytest.mark.parametrize("name", sorted(mc.BATCHES))
def test_batches_match_the_reference(name):
    r = mc.host(name)
    mc.assert_equal(r.got(), mc.expected(name))
    assert np.array_equal(r.res.es.numpy(), r.es_before)  # the ES is only read


def test_walk_cases_hold_what_they_are_meant_to():
    r = mc.host("walk")
    assert len(mc.WALK_NAMES) == len(r.caps)
    for i, name in enumerate(mc.WALK_NAMES):
        s = r.ma.segment(i)
        assert (s["status"], s["n_frames"]) == (mc.WALK_STATUS[name], mc.WALK_FRAMES[name]), name
        rx = r.rx.segment(i)
        if name == "no_config":
            assert not s["has_config"] and len(s["mframes"]) == 0 and rx["n_aframes"] == 0
            continue
        assert s["has_config"] and rx["n_aframes"] == s["n_frames"] == s["mframes"][:, 0].sum() == len(rx["asamples"])
        assert rx["audio_payload_bytes"] == s["mframes"][:, 1].sum() == rx["asamples"][:, 1].sum()
        assert rx["audio_mdat"][:8] == struct.pack(">I4s", 8 + rx["audio_payload_bytes"], b"mdat")
    first = r.ma.segment(0)
    assert {k: first[k] for k in ("sample_rate", "channels", "version", "layer", "frame_samples", "bitrate")} == \
        {"sample_rate": 44100, "channels": 2, "version": 1, "layer": 3, "frame_samples": 1152, "bitrate": 128000}
    assert r.ma.segment(1)["mframes"].tolist() == [[3, 3 * 417], [3, 3 * 418]]      # ends exactly at the PES's end
    assert r.ma.segment(2)["mframes"].tolist() == [[2, 48], [0, 0]]                 # one byte past
    assert r.ma.segment(3)["mframes"].tolist() == [[2, 48], [2, 48]]                # the 3-byte tail is no frame
    assert r.ma.segment(7)["mframes"].tolist() == [[2, 48], [2, 48]]                # stops at the other key
    assert r.ma.segment(8)["mframes"].tolist() == [[2, 48], [0, 0], [2, 50]]  # the PES of the other key is left out
    mono = r.ma.segment(10)
    assert (mono["channels"], mono["sample_rate"], mono["frame_samples"], mono["version"]) == (1, 24000, 576, 2)
    l1 = r.ma.segment(11)
    assert (l1["layer"], l1["version"], l1["sample_rate"], l1["frame_samples"]) == (1, 25, 8000, 384)
    assert l1["bitrate"] == 56000
    # the samples are the frames, whole and in stream order
    seg = mc.walk_segments()[0]
    assert r.rx.segment(0)["audio_mdat"][8:] == seg["audio"]


def test_no_config_and_other_codecs_keep_every_byte_of_the_remux():
    for name, keep in (("walk", [mc.WALK_NAMES.index("no_config")]), ("mixed", [0, 4])):
        r = mc.host(name)
        got = r.got()
        for i in keep:
            oo, region = int(r.offs[i]), int(r.rx.region[i])
            assert np.array_equal(got["out"][oo - r.headroom:oo + region], r.before["out"][oo - r.headroom:oo + region])
            assert np.array_equal(got["asamples"][i], r.before["asamples"][i])
            assert np.array_equal(got["rinfo"][i], r.before["rinfo"][i])
            assert (got["mframes"][i] == -1).all() and (got["mpainfo"][i, 1:] == 0).all()
    r = mc.host("mixed")
    assert r.ma.mpainfo[:, 0].tolist() == [1, 0, 0, 0, 1]
    adts = r.rx.segment(0)  # the ADTS segment's audio stays
    assert adts["n_aframes"] == 4 and adts["audio_payload_bytes"] > 0
    assert [r.ma.segment(i)["n_frames"] for i in (1, 2, 3)] == [3, 9, 2]
    assert r.ma.segment(3)["layer"] == 2 and r.rx.segment(2)["n_vsamples"] == 2  # HEVC video beside it


def test_nine_frames_for_eight_rows():
    r = mc.host("overflow")
    a, b = r.ma.segment(0), r.ma.segment(1)
    assert a["status"] == mpegaudio.MPASTATUS["aframe_overflow"] and a["n_frames"] == 9 and b["status"] == 0
    ra, rb = r.rx.segment(0), r.rx.segment(1)
    assert ra["status"] & remux.RSTATUS["aframe_overflow"] and not rb["status"] & remux.RSTATUS["aframe_overflow"]
    assert (ra["n_aframes"], len(ra["asamples"]), ra["audio_payload_bytes"]) == (9, 8, 4 * 24 + 4 * 25)
    assert (rb["n_aframes"], len(rb["asamples"]), rb["audio_payload_bytes"]) == (8, 8, 8 * 24)


def test_frames_stop_where_the_region_ends():
    """The "frames while they fit behind the audio header" rule: a region cut short by the caller."""
    segs, max_pes, max_aframes = mc.BATCHES["overflow"]()
    r = mc.Run(segs, max_pes, max_aframes)
    full = r.rx.segment(1)
    res = r.res
    out = torch.full_like(r.out, mc.FILL)
    rx2 = remux.remux_batch(res, r.ix, r.caps, out, r.offs, max_aframes=max_aframes, audio_gap=r.gap,
                            headroom=r.headroom)
    rx2.region = rx2.region.copy()
    rx2.region[1] = full["audio_box_offset"] + 8 + 3 * 24 + 5  # room for three frames and five bytes
    mframes, mpainfo = np.zeros((2, max_pes, 2), np.int32), np.zeros((2, 8), np.int64)
    runtime().mpeg_audio_batch(res.es.numpy(), r.res.es_offs, np.asarray(r.caps, np.int64), res.info.numpy(),
                               res.pes.numpy(), max_pes, rx2.region, max_aframes, mframes, mpainfo,
                               rx2.asamples.numpy(), rx2.rinfo.numpy(), out.numpy(), np.asarray(r.offs, np.int64))
    cut = rx2.segment(1)
    assert mpainfo[1, 0] == 16 and (cut["n_aframes"], len(cut["asamples"]), cut["audio_payload_bytes"]) == (8, 3, 72)
    end = int(r.offs[1]) + int(rx2.region[1])
    assert (out.numpy()[end - 5:end + 64] == mc.FILL).all()


def raw_with_canaries(r, call):
    """``call(mframes, mpainfo, asamples, rinfo, out)`` on fresh over-allocated copies of what the
    remux left; returns them.  Behind every output stand 64 canary elements."""
    B, pad = len(r.caps), 64
    mk = lambda a, v: np.concatenate([a.reshape(-1), np.full(pad, v, a.dtype)])  # noqa: E731
    arrays = [mk(np.zeros((B, r.max_pes, 2), np.int32), -77), mk(np.zeros((B, 8), np.int64), -77),
              mk(r.before["asamples"], -77), mk(r.before["rinfo"], -77), mk(r.before["out"], 0x3C)]
    call(*arrays)
    return arrays, pad


@pytest.mark.parametrize("name", ["walk", "damaged", "fuzz0", "overflow"])
def test_canaries_behind_every_output(name):
    r = mc.host(name)
    res = r.res

    def call(mframes, mpainfo, asamples, rinfo, out):
        runtime().mpeg_audio_batch(res.es.numpy(), r.res.es_offs, np.asarray(r.caps, np.int64), res.info.numpy(),
                                   res.pes.numpy(), r.max_pes, np.asarray(r.rx.region, np.int64), r.max_aframes,
                                   mframes, mpainfo, asamples, rinfo, out, np.asarray(r.offs, np.int64))
    arrays, pad = raw_with_canaries(r, call)
    want = mc.expected(name)
    for a, k, canary in zip(arrays, mc.NAMES, (-77, -77, -77, -77, 0x3C)):
        assert (a[-pad:] == canary).all(), k
        assert np.array_equal(a[:-pad], want[k].reshape(-1)), k


def test_damaged_rows_write_nothing_outside_the_regions():
    r = mc.host("damaged")
    got, before = r.got()["out"], r.before["out"]
    inside = np.zeros(len(got), bool)
    for oo, region in zip(r.offs, r.rx.region):
        inside[int(oo):int(oo) + int(region)] = True
    assert np.array_equal(got[~inside], before[~inside])
    assert r.ma.mpainfo[:, 0].tolist() == [0, 0, 2, 0, 0]  # a negative offset clamps to 0: rows 2 and 4 differ in PES 0


def test_fuzz_reaches_frames_and_errors():
    """Asserted on the reference alone: at least a quarter of the segments have a frame, and at
    least a quarter end a walk early."""
    rows = np.concatenate([mc.expected(f"fuzz{j}")["mpainfo"] for j in range(len(mc.FUZZ_SEEDS))])
    assert len(rows) == 24
    assert (rows[:, 1] > 0).sum() * 4 >= len(rows) and ((rows[:, 0] & 4) != 0).sum() * 4 >= len(rows)


def test_layout_names_equal_the_runtime_exports():
    rt = runtime()
    assert mpegaudio.MPAINFO == dict(rt.ES_MPAINFO) and mpegaudio.MPASTATUS == dict(rt.ES_MPASTATUS)
    assert mpegaudio.MPAINFO_WORDS == rt.ES_MPAINFO_WORDS == len(mpegaudio.MPAINFO)
    assert rt.mpa_scratch_words(3, 10) == 3 * (9 + 2 * 10)


def test_rejections_on_the_host():
    segs, max_pes, max_aframes = mc.BATCHES["mixed"]()
    r = mc.Run(segs, max_pes, max_aframes)
    with pytest.raises(ValueError, match="ES"):
        mpegaudio.mpeg_audio_batch(r.res, r.rx, [c + (1 << 40) for c in r.caps])
    other = mc.Run(segs[:2], max_pes, max_aframes)
    with pytest.raises(ValueError, match="does not belong"):
        mpegaudio.mpeg_audio_batch(r.res, other.rx, r.caps)
    bad = remux.Remuxed(r.rx.rinfo, r.rx.vsamples, r.rx.asamples, r.rx.out[:100], r.rx.out_offs, r.rx.headroom,
                        r.rx.audio_gap, r.rx.region)
    with pytest.raises(ValueError, match="output"):
        mpegaudio.mpeg_audio_batch(r.res, bad, r.caps)
    bad = remux.Remuxed(r.rx.rinfo, r.rx.vsamples, r.rx.asamples.to(torch.int64), r.rx.out, r.rx.out_offs,
                        r.rx.headroom, r.rx.audio_gap, r.rx.region)
    with pytest.raises(ValueError, match="dtypes"):
        mpegaudio.mpeg_audio_batch(r.res, bad, r.caps)
    bad = remux.Remuxed(r.rx.rinfo, r.rx.vsamples, r.rx.asamples, r.rx.out, r.rx.out_offs, r.rx.headroom,
                        r.rx.audio_gap, None)
    with pytest.raises(ValueError, match="does not belong"):
        mpegaudio.mpeg_audio_batch(r.res, bad, r.caps)
    with pytest.raises(ValueError, match="too small"):
        runtime().mpeg_audio_batch(r.res.es.numpy(), r.res.es_offs, np.asarray(r.caps, np.int64), r.res.info.numpy(),
                                   r.res.pes.numpy(), max_pes + 1, np.asarray(r.rx.region, np.int64), max_aframes,
                                   r.ma.mframes.numpy(), r.ma.mpainfo.numpy(), r.rx.asamples.numpy(),
                                   r.rx.rinfo.numpy(), r.out.numpy(), np.asarray(r.offs, np.int64))


# ---------------------------------------------------------------- the boxes that go with the samples
@pytest.mark.parametrize("batch,i,obj,codec", [("walk", 0, 0x6B, "mp4a.6b"), ("walk", 10, 0x69, "mp4a.69"),
                                               ("walk", 11, 0x69, "mp4a.69")])
def test_init_segment(batch, i, obj, codec):
    m = mc.host(batch).ma.segment(i)
    data = fmp4.mpeg_audio_init(m)
    boxes = cc.walk_boxes(data)
    assert cc.box_kinds(boxes) == tree("smhd", ["mp4a", ["esds"]])
    mp4a = cc.find_box(boxes, "moov/trak/mdia/minf/stbl/stsd/mp4a").body
    assert struct.unpack(">HHHHI", mp4a[16:28]) == (m["channels"], 16, 0, 0, m["sample_rate"] << 16)
    want = bytes(4) + bytes([3, 21, 0, 1, 0, 4, 13, obj, 0x15]) + bytes(11) + bytes([6, 1, 2])  # no 05 descriptor
    assert cc.find_box(boxes, "moov/trak/mdia/minf/stbl/stsd/mp4a/esds").body == want
    mdhd = cc.find_box(boxes, "moov/trak/mdia/mdhd").body
    assert struct.unpack(">II", mdhd[12:20]) == (m["sample_rate"], 0)
    trex = cc.find_box(boxes, "moov/mvex/trex").body
    assert struct.unpack(">IIIIII", trex) == (0, fmp4.AUDIO_TRACK, 1, m["frame_samples"], 0, 0x02000000)
    assert struct.unpack(">I", cc.find_box(boxes, "moov/trak/tkhd").body[12:16]) == (fmp4.AUDIO_TRACK,)
    assert fmp4.mpeg_audio_codec(m) == codec


def test_no_init_segment_without_a_config():
    r = mc.host("walk")
    for m in (r.ma.segment(mc.WALK_NAMES.index("no_config")), mc.host("mixed").ma.segment(0)):
        assert fmp4.mpeg_audio_init(m) is None and fmp4.mpeg_audio_codec(m) is None


def test_audio_moof_takes_the_frame_samples():
    rows = np.array([[0, 417], [417, 418]], np.int32)
    m = rc.parse_moof(fmp4.audio_moof(9, 90000, 44100, rows, frame_samples=1152))
    assert (m["default_duration"], m["base"], m["track"], m["count"]) == (1152, 44100, fmp4.AUDIO_TRACK, 2)
    assert [s["size"] for s in m["samples"]] == [417, 418]
    assert rc.parse_moof(fmp4.audio_moof(9, 90000, 44100, rows))["default_duration"] == 1024


def fragments(name: str, with_mpa: bool):
    segs, max_pes, max_aframes = mc.BATCHES[name]()
    r = mc.Run(segs, max_pes, max_aframes)
    B = len(r.caps)
    seq = np.arange(5, 5 + B)
    fr = fragment.fragment_batch(r.rx, r.ix, seq, mpeg_audio=r.ma if with_mpa else None)
    return r, fr, seq


@pytest.mark.parametrize("name", ["mixed", "walk"])
def test_fragment_batch_with_mpeg_audio_is_fmp4_byte_for_byte(name):
    r, fr, seq = fragments(name, True)
    for i in range(len(r.caps)):
        m, rx, f, ix = r.ma.segment(i), r.rx.segment(i), fr.segment(i), r.ix.segment(i)
        if m["has_config"]:
            want = fmp4.audio_moof(int(seq[i]), rx["audio_base_pts"], m["sample_rate"], rx["asamples"],
                                   frame_samples=m["frame_samples"])
            assert f["status"] & fragment.FSTATUS["no_rate"] == 0
            assert f["audio_tfdt"] == (rx["audio_base_pts"] * m["sample_rate"] + 45000) // 90000
        else:
            want = fmp4.audio_moof(int(seq[i]), rx["audio_base_pts"], ix["audio_sample_rate"], rx["asamples"])
        assert f["audio"] == want + rx["audio_mdat"], i
        p = rc.parse_moof(f["audio"][:f["audio_moof_bytes"]])
        assert p["count"] == len(rx["asamples"]) and p["default_duration"] == (m["frame_samples"] or 1024)
        assert f["audio"][f["audio_moof_bytes"] + 8:] == rx["audio_mdat"][8:]


def test_fragment_batch_without_the_argument_is_unchanged():
    """Without ``mpeg_audio`` an MPEG audio segment gets what it got before the op existed: the AAC
    frame, no rate (``sinfo`` has none); an ADTS segment the same bytes with and without."""
    r, fr, seq = fragments("mixed", False)
    _, fr2, _ = fragments("mixed", True)
    assert fr.segment(0) == fr2.segment(0) and fr.segment(4) == fr2.segment(4)
    for i in range(len(r.caps)):
        rx, f, ix = r.rx.segment(i), fr.segment(i), r.ix.segment(i)
        moof = fmp4.audio_moof(int(seq[i]), rx["audio_base_pts"], ix["audio_sample_rate"], rx["asamples"])
        assert f["audio"] == moof + rx["audio_mdat"]
    assert fr.segment(1)["status"] & fragment.FSTATUS["no_rate"]
    with pytest.raises(ValueError, match="mpeg_audio"):
        fragment.fragment_batch(r.rx, r.ix, seq, mpeg_audio=r.ma.mpainfo[:2])
