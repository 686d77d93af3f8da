"""Codec configuration (``ops/codecconfig.py``) on the host implementation (``runtime/codec.cpp``):
``cinfo`` and ``ps`` equal the independent sequential reference (``tests/codec_cases.py``) exactly on
the hand-built cases and on the fuzz batch; the properties those cases exist for are stated on
the results; the init segments (``player/fmp4.py``) walk as ISO-BMFF boxes whose sizes add up and
carry the parameter sets verbatim; the configuration reaches the pipeline's results and the
player's ``FRAG_PARSING_INIT_SEGMENT`` only under the remux."""
import struct

import numpy as np
import pytest
import torch

import codec_cases as cc
from esindex_cases import SC, adts_frame, background
from hlsjs_p2p_wrapper_amd import Hls
from hlsjs_p2p_wrapper_amd.ops import aes, codecconfig, esindex
from hlsjs_p2p_wrapper_amd.ops._native import runtime
from hlsjs_p2p_wrapper_amd.player import fmp4

C, ST = codecconfig.CINFO, codecconfig.CSTATUS


def run_case(name: str, device="cpu"):
    case = cc.CASES[name]()
    res, ix, caps = cc.build(case, device)
    cfg = codecconfig.config_batch(res, ix, caps, case.max_ps)
    return case, res, ix, caps, cfg, cc.ref_batch(res, ix, caps, case.max_ps)


@pytest.fixture(scope="module")
def ran():
    """Every case once, on the host."""
    return {name: run_case(name) for name in cc.CASES}


@pytest.mark.parametrize("case", sorted(cc.CASES))
def test_hand_built_cases_match_the_reference(case, ran):
    _, _, _, _, cfg, ref = ran[case]
    cc.assert_config_equal(cfg, ref)
    assert tuple(cfg.cinfo.shape) == (len(ref[0]), codecconfig.CINFO_WORDS) and cfg.cinfo.dtype == torch.int32


def rows(cfg, *names):
    return [[int(r[C[n]]) for n in names] for r in cfg.cinfo.numpy()]


# ---------------------------------------------------------------- the properties the cases exist for
def test_parse_cases_hold_what_they_are_meant_to(ran):
    _, _, _, _, cfg, _ = ran["parse"]
    got = rows(cfg, "status", "profile_idc", "level_idc", "chroma_format_idc", "bit_depth_luma", "width", "height",
               "sar_width", "sar_height")
    audio = ST["no_audio_config"]
    assert got[0] == [audio, 66, 30, 1, 8, 640, 360, 1, 1]
    assert got[1] == [audio, 100, 40, 1, 8, 1920, 1080, 1, 1]
    assert got[2][5:7] == [640, 368] and got[3][5:7] == [640, 368]  # pic_order_cnt_type 1 and 2
    assert got[4][1:7] == [77, 30, 1, 8, 720 - 2 * 3, 576 - 4 * 7]  # interlaced: cropping counts fourfold
    assert got[5][3:7] == [0, 8, 640 - 7, 368 - 3]                  # monochrome: cropping in luma samples
    assert got[6][3:7] == [2, 10, 640 - 14, 368 - 3]                # 4:2:2
    assert got[7][3:7] == [3, 8, 640 - 7, 368 - 3] and got[8][3:7] == [3, 8, 640 - 7, 2 * 368 - 2 * 3]
    assert [g[7:9] for g in got[9:15]] == [[4, 3], [4, 3], [1, 1], [1, 1], [1, 1], [1, 1]]
    raw = cfg.segment(15)["sps"]
    assert raw[:5] == bytes([0x67, 0, 0, 3, 30]) and got[15][:3] == [audio, 0, 30]  # the level is raw byte 4
    assert all(g[0] == audio for g in got[:16])
    # every error: the status bit, zeros behind level_idc
    n_bad = 7
    for g in got[16:16 + n_bad]:
        assert g[0] == audio | ST["bad_sps"] and g[3:] == [0] * 6 and g[1] in (66, 100, 110)
    cuts = got[16 + n_bad:-2]
    assert len(cuts) > 80 and all(g[0] == audio | ST["bad_sps"] and g[3:] == [0] * 6 for g in cuts)
    assert cuts[0][1:3] == [0, 0] and cuts[2][1:3] == [0, 0] and cuts[3][1:3] == [100, 40]  # fewer than 3 bytes: 0
    assert got[-2][0] == audio | ST["bad_sps"] and got[-2][1:3] == [66, 30]  # 40 zero bits where sps_id is read
    one = cfg.segment(len(got) - 1)
    assert one["sps"] == b"\x67" and one["sps_rbsp_bytes"] == 0 and one["status"] == audio | ST["bad_sps"]
    assert all(s["pps"] == cc.PPS and s["pps_nal"] == s["sps_nal"] + 1 for s in map(cfg.segment, range(len(got))))


def test_scaling_lists_and_signed_offsets_are_in_the_cases():
    """Counted on the writer's input: both list sizes, fall-back flags, both signs, a stop at
    ``next == 0`` and a wrap of the modulo in the 1080p SPS."""
    lists = cc.SCALING_1080
    assert [None if d is None else len(d) for d in lists] == [16, None, 1, 16, None, 16, 64, None]
    assert any(x < 0 for x in lists[0]) and any(x > 0 for x in lists[0]) and lists[2] == [-8]
    assert 8 + sum(lists[5][:3]) >= 256
    assert cc.ref_parse_sps(cc.sps_nal(**cc.HIGH_1080))["ok"]
    bent = dict(cc.HIGH_1080, scaling=[[1] * 16] + cc.SCALING_1080[1:])  # another list 0: the same picture
    assert cc.ref_parse_sps(cc.sps_nal(**bent))["width"] == 1920


def test_unescape_cases_hold_what_they_are_meant_to(ran):
    case, _, _, _, cfg, _ = ran["unescape"]
    segs = [cfg.segment(i) for i in range(len(case.segs))]
    assert segs[0]["sps"][:3] == b"\x67\x00\x03" and segs[0]["sps_rbsp_bytes"] == 39  # 03 at raw index 2 stays
    assert segs[1]["sps"][:4] == b"\x67\x00\x00\x03" and segs[1]["sps_rbsp_bytes"] == 38
    for s, j in zip(segs[2:10], (63, 64, 65, 127, 128, 255, 256, 257)):
        assert cc.escape_positions(s["sps"]) == [j] and s["sps_bytes"] == 300 and s["sps_rbsp_bytes"] == 298
        assert (s["width"], s["height"], s["status"] & ST["bad_sps"]) == (640, 360, 0)
    assert cc.escape_positions(segs[10]["sps"]) == [511] and segs[10]["sps_bytes"] == 512 == case.max_ps
    assert segs[10]["sps_rbsp_bytes"] == 510 and not segs[10]["status"] & ST["ps_overflow"]
    assert segs[11]["sps_rbsp_bytes"] == 299 - 6
    head = len(cc.SPS_A)
    assert [s["sps_rbsp_bytes"] - (head - 1) for s in segs[12:15]] == [5, 4, 4]  # two dropped; one; one
    # a parsed field behind an escape on either side of 63 | 64
    moving = segs[15:]
    first = [cc.escape_positions(s["sps"])[0] for s in moving]
    assert {62, 63, 64, 65} <= set(first)
    for s in moving:
        assert (s["width"], s["height"], s["sar_width"], s["sar_height"]) == (1280, 720, 64, 45)
        assert s["sps_rbsp_bytes"] == s["sps_bytes"] - 1 - len(cc.escape_positions(s["sps"]))
        kept = cc.ref_parse_rbsp(s["sps"][1:])  # what a parser that kept the 03 bytes would read
        assert (kept["width"], kept["height"]) != (1280, 720)


def test_search_cases_hold_what_they_are_meant_to(ran):
    _, _, ix, _, cfg, _ = ran["search"]
    got = rows(cfg, "status", "sps_nal", "pps_nal")
    audio = ST["no_audio_config"]
    assert got[0] == [audio, 0, 1] and got[1] == [audio, 255, 256] and got[2] == [audio, 256, 257]
    assert got[3] == [audio, 257, 278] and got[4] == [audio, 71, 0]
    assert got[5] == [audio, 0, 2] and cfg.segment(5)["sps"] == cc.SPS_A and cfg.segment(5)["pps"] == cc.PPS
    assert got[6] == [audio | ST["no_sps"] | ST["no_pps"], -1, -1]
    assert int(ix.sinfo[6, esindex.SINFO["status"]]) & esindex.SSTATUS["nal_overflow"]
    assert got[7] == [audio | ST["no_pps"], 299, -1]
    assert got[8] == [audio, 2, 3] and ix.nal[8, 1].tolist()[1:3] == [0, 7] and cfg.segment(8)["sps"] == cc.SPS_B
    assert got[9] == [audio, 0, 1] and ix.nal[9, :3, 3].tolist() == [-1, -1, 0]
    assert got[10] == [audio | ST["no_pps"], 0, -1] and got[11] == [audio | ST["no_sps"], -1, 1]
    assert cfg.segment(10)["pps"] == b"" and not cfg.ps[10, 1].any()


@pytest.mark.parametrize("name", ["copy_16", "copy", "copy_1024"])
def test_copy_cases_hold_what_they_are_meant_to(name, ran):
    case, res, ix, caps, cfg, _ = ran[name]
    max_ps, n = case.max_ps, len(case.segs)
    assert tuple(cfg.ps.shape) == (n, 2, max_ps)
    offs = [int(ix.nal[i, 0, 0]) for i in range(20)]
    assert {o % 4 for o in offs} == {0, 1, 2, 3} and {o % 16 for o in offs} >= set(range(3, 16))
    es = res.es.numpy()
    for i in range(n - 2):  # stored bytes are the ES bytes, zero behind them
        s = cfg.segment(i)
        for which, name_ in ((0, "sps"), (1, "pps")):
            k, ln = s[name_ + "_nal"], s[name_ + "_bytes"]
            o = int(res.es_offs[i]) + int(ix.nal[i, k, 0])
            stored = min(ln, max_ps, caps[i] - int(ix.nal[i, k, 0]))
            assert cfg.ps[i, which, :stored].numpy().tobytes() == es[o:o + stored].tobytes() == s[name_]
            assert not cfg.ps[i, which, stored:].any()
    exact, over, pps_over, tail, tail_full, long_row, far_row = (cfg.segment(i) for i in range(20, 27))
    assert exact["sps_bytes"] == max_ps and not exact["status"] & ST["ps_overflow"]
    assert exact["sps_rbsp_bytes"] == max_ps - 1 and exact["width"] == 640
    assert over["sps_bytes"] == max_ps + 1 and over["status"] & ST["ps_overflow"] and len(over["sps"]) == max_ps
    assert [over[k] for k in cc.NAMES[3:4] + cc.NAMES[6:16]] == [0] * 11 and not over["status"] & ST["bad_sps"]
    assert pps_over["pps_bytes"] == max_ps + 1 and pps_over["status"] & ST["ps_overflow"]
    assert (pps_over["width"] == 640) == (len(cc.SPS_A) <= max_ps)
    for s, i in ((tail, 23), (tail_full, 24)):  # the SPS is the last bytes of the video ES
        end = int(ix.nal[i, 1, 0]) + s["sps_bytes"]
        assert end == int(res.info[i, cc.INFO["video_bytes"]]) and es[int(res.es_offs[i]) + end] == 0xFF
        assert cfg.ps[i, 0, min(s["sps_bytes"], max_ps):].sum() == 0
    assert long_row["sps_bytes"] == caps[25] - 3 and int(ix.nal[25, 0, 1]) == 5000  # clamped to the cap
    assert far_row["sps_bytes"] == 0 and far_row["status"] & ST["bad_sps"] and far_row["sps"] == b""
    assert far_row["pps"] == (SC + cc.filler_sps(60))[:4]  # a negative offset reads from the segment's start


def test_audio_cases_hold_what_they_are_meant_to(ran):
    _, _, _, _, cfg, _ = ran["audio"]
    got = rows(cfg, "status", "aac_object_type", "aac_rate_index", "aac_channel_config")
    bad = ST["no_audio_config"]
    assert got[:4] == [[0, o, 3, 2] for o in (1, 2, 3, 4)]
    assert got[4:10] == [[0, 2, 3, 2], [0, 2, 4, 2], [0, 2, 11, 2], [0, 2, 12, 2], [bad, 2, 13, 2], [bad, 2, 15, 2]]
    assert got[10:15] == [[bad, 2, 3, 0], [0, 2, 3, 1], [0, 2, 3, 2], [0, 2, 3, 6], [0, 2, 3, 7]]
    assert got[15] == [0, 2, 4, 6] and got[16] == [0, 2, 3, 2]  # a 9-byte header; an odd audio offset
    assert got[17] == [bad, 0, 0, 0] and got[18] == [bad, 0, 0, 0] and got[19] == [bad, 0, 0, 0]
    assert got[20] == [0, 2, 7, 2]  # two PES: the first frame of the first
    assert got[21] == [bad, 0, 0, 0]  # claimed frames, no room for a header: nothing is read


def test_other_cases_hold_what_they_are_meant_to(ran):
    _, _, _, _, cfg, _ = ran["other"]
    got = rows(cfg, "status", "sps_nal", "pps_nal", "sps_bytes", "width")
    bad = ST["no_audio_config"]
    assert got[0] == got[1] == [bad | ST["unsupported_video"], -1, -1, 0, 0] and not cfg.ps[:2].any()
    assert got[2] == [bad | ST["no_sps"] | ST["no_pps"], -1, -1, 0, 0]
    assert got[3] == [bad, 0, 1, len(cc.SPS_A), 640]


def test_fuzz_reaches_both_outcomes(ran):
    _, _, _, _, cfg, _ = ran["fuzz"]
    status = cfg.cinfo[:, C["status"]].numpy()
    assert len(status) == 256 and 0 < int(((status & ST["bad_sps"]) != 0).sum()) < 256
    assert int((cfg.cinfo[:, C["sps_rbsp_bytes"]] < cfg.cinfo[:, C["sps_bytes"]] - 1).sum()) > 10  # escapes occur


def test_empty_batch_and_argument_errors():
    res, ix, caps = cc.build(cc.Case([]))
    cfg = codecconfig.config_batch(res, ix, caps)
    assert tuple(cfg.cinfo.shape) == (0, 19) and tuple(cfg.ps.shape) == (0, 2, 256)
    res, ix, caps = cc.build(cc.other_cases())
    for bad in (0, 24, 2048, -16):
        with pytest.raises(ValueError, match="max_ps"):
            codecconfig.config_batch(res, ix, caps, bad)
    other = esindex.index_batch(res, caps, max_nal=8)
    other = esindex.EsIndex(other.nal[:3], other.au[:3], other.aframes[:3], other.sinfo[:3])
    with pytest.raises(ValueError, match="does not belong"):
        codecconfig.config_batch(res, other, caps)
    with pytest.raises(ValueError, match="out of bounds"):
        codecconfig.config_batch(res, ix, [c + (1 << 20) for c in caps])
    rt = runtime()
    args = (res.es.numpy(), np.asarray(res.es_offs), np.asarray(caps, np.int64), res.info.numpy(), res.pes.numpy(), 8,
            8, ix.nal.numpy(), ix.au.numpy(), ix.aframes.numpy(), ix.sinfo.numpy())
    with pytest.raises(ValueError, match="max_ps"):
        rt.config_batch(*args, 24, np.zeros((4, 19), np.int32), np.zeros((4, 2, 24), np.uint8))
    with pytest.raises(ValueError, match="too small"):
        rt.config_batch(*args, 32, np.zeros(4 * 19 - 1, np.int32), np.zeros((4, 2, 32), np.uint8))
    with pytest.raises(ValueError, match="too small"):
        rt.config_batch(*args, 32, np.zeros(4 * 19, np.int32), np.zeros(4 * 2 * 32 - 1, np.uint8))


@pytest.mark.gpu
def test_mixed_devices_are_rejected(cuda):
    res, ix, caps = cc.build(cc.other_cases())
    _, ix_dev, _ = cc.build(cc.other_cases(), cuda)
    with pytest.raises(ValueError, match="one device"):
        codecconfig.config_batch(res, ix_dev, caps)


# ---------------------------------------------------------------- layout
def test_layout_names_equal_the_runtime_exports():
    rt = runtime()
    assert codecconfig.CINFO == dict(rt.ES_CINFO) and codecconfig.CINFO_WORDS == rt.ES_CINFO_WORDS == 19
    assert codecconfig.CSTATUS == dict(rt.ES_CSTATUS) and codecconfig.DEFAULT_MAX_PS == rt.ES_DEFAULT_MAX_PS == 256
    assert sorted(codecconfig.CINFO.values()) == list(range(codecconfig.CINFO_WORDS))
    assert list(codecconfig.CINFO) == list(cc.NAMES) and codecconfig.CINFO == cc.C
    assert codecconfig.CSTATUS == {"no_sps": 1, "no_pps": 2, "ps_overflow": 4, "bad_sps": 8, "unsupported_video": 16,
                                   "no_audio_config": 32}
    assert fmp4.VIDEO_DISQUALIFIED == 31 and fmp4.AUDIO_DISQUALIFIED == 32
    assert rt.ES_SINFO_WORDS == 8 and rt.ES_RINFO_WORDS == 8  # no slot was added to either row
    from hlsjs_p2p_wrapper_amd import ops

    assert ops.config_batch is codecconfig.config_batch and ops.CodecConfig is codecconfig.CodecConfig


# ---------------------------------------------------------------- init segments
TREE = ["ftyp", ["moov", ["mvhd", ["trak", ["tkhd", ["mdia", ["mdhd", "hdlr", ["minf", [
    "MEDIA", ["dinf", [["dref", ["url "]]]], ["stbl", [["stsd", ["ENTRY"]], "stts", "stsc", "stsz", "stco"]]]]]]]],
    ["mvex", ["trex"]]]]]


def tree(media, entry):
    def sub(node):
        if isinstance(node, list):
            return [sub(x) for x in node]
        return {"MEDIA": media, "ENTRY": entry}.get(node, node)
    return sub(TREE)


def config_of(name: str, i: int, ran) -> dict:
    return ran[name][4].segment(i)


def test_video_init_segment(ran):
    cfg = config_of("parse", 10, ran)  # 640 x 368 at 4:3
    data = fmp4.video_init(cfg)
    boxes = cc.walk_boxes(data)
    assert cc.box_kinds(boxes) == tree("vmhd", ["avc1", ["avcC", "pasp"]])
    assert cc.find_box(boxes, "ftyp").body == b"isom\x00\x00\x00\x01isomavc1"
    avc1 = cc.find_box(boxes, "moov/trak/mdia/minf/stbl/stsd/avc1")
    assert struct.unpack(">HH", avc1.body[24:28]) == (640, 368) and avc1.body[6:8] == b"\x00\x01"
    sps, pps = cfg["sps"], cfg["pps"]
    want = bytes([1, 66, 0xC0, 30, 0xFF, 0xE1, 0, len(sps)]) + sps + bytes([1, 0, len(pps)]) + pps
    assert cc.find_box(boxes, "moov/trak/mdia/minf/stbl/stsd/avc1/avcC").body == want and sps[0] == 0x67
    assert cc.find_box(boxes, "moov/trak/mdia/minf/stbl/stsd/avc1/pasp").body == struct.pack(">II", 4, 3)
    tkhd = cc.find_box(boxes, "moov/trak/tkhd").body
    assert struct.unpack(">I", tkhd[12:16]) == (fmp4.VIDEO_TRACK,) and tkhd[:4] == b"\x00\x00\x00\x07"
    assert struct.unpack(">II", tkhd[-8:]) == ((640 * 4 << 16) // 3, 368 << 16)
    mdhd = cc.find_box(boxes, "moov/trak/mdia/mdhd").body
    assert struct.unpack(">II", mdhd[12:20]) == (fmp4.VIDEO_TIMESCALE, 0)  # the tfdt's units, duration 0
    assert struct.unpack(">II", cc.find_box(boxes, "moov/mvhd").body[12:20]) == (fmp4.VIDEO_TIMESCALE, 0)
    assert cc.find_box(boxes, "moov/trak/mdia/hdlr").body[8:12] == b"vide"
    trex = cc.find_box(boxes, "moov/mvex/trex").body
    assert struct.unpack(">IIIIII", trex) == (0, fmp4.VIDEO_TRACK, 1, 0, 0, 0x01010000)
    for kind in ("stts", "stsc", "stco"):
        assert cc.find_box(boxes, f"moov/trak/mdia/minf/stbl/{kind}").body == bytes(8)
    assert cc.find_box(boxes, "moov/trak/mdia/minf/stbl/stsz").body == bytes(12)
    assert fmp4.video_codec(cfg) == "avc1.42c01e"
    hd = config_of("parse", 1, ran)
    boxes = cc.walk_boxes(fmp4.video_init(hd))
    avc1 = cc.find_box(boxes, "moov/trak/mdia/minf/stbl/stsd/avc1")
    assert struct.unpack(">HH", avc1.body[24:28]) == (1920, 1080) and fmp4.video_codec(hd) == "avc1.640028"
    assert hd["sps"] in cc.find_box(boxes, "moov/trak/mdia/minf/stbl/stsd/avc1/avcC").body
    with pytest.raises(ValueError):
        cc.walk_boxes(data[:-1])
    with pytest.raises(ValueError):
        cc.walk_boxes(data + b"\x00")


@pytest.mark.parametrize("i,obj,rate,chans", [(5, 2, 44100, 2), (3, 4, 48000, 2), (14, 2, 48000, 8), (7, 2, 7350, 2)])
def test_audio_init_segment(i, obj, rate, chans, ran):
    cfg = config_of("audio", i, ran)
    data = fmp4.audio_init(cfg)
    boxes = cc.walk_boxes(data)
    assert cc.box_kinds(boxes) == tree("smhd", ["mp4a", ["esds"]])
    mp4a = cc.find_box(boxes, "moov/trak/mdia/minf/stbl/stsd/mp4a").body
    assert struct.unpack(">HHHHI", mp4a[16:28]) == (chans, 16, 0, 0, rate << 16)
    asc = struct.pack(">H", (obj << 11) | (cfg["aac_rate_index"] << 7) | (cfg["aac_channel_config"] << 3))
    want = bytes(4) + bytes([3, 25, 0, 1, 0, 4, 17, 0x40, 0x15]) + bytes(11) + bytes([5, 2]) + asc + bytes([6, 1, 2])
    assert cc.find_box(boxes, "moov/trak/mdia/minf/stbl/stsd/mp4a/esds").body == want
    mdhd = cc.find_box(boxes, "moov/trak/mdia/mdhd").body
    assert struct.unpack(">II", mdhd[12:20]) == (rate, 0)  # the audio tfdt is in units of the sample rate
    assert cc.find_box(boxes, "moov/trak/mdia/hdlr").body[8:12] == b"soun"
    assert struct.unpack(">I", cc.find_box(boxes, "moov/trak/tkhd").body[12:16]) == (fmp4.AUDIO_TRACK,)
    trex = cc.find_box(boxes, "moov/mvex/trex").body
    assert struct.unpack(">IIIIII", trex) == (0, fmp4.AUDIO_TRACK, 1, 1024, 0, 0x02000000)
    assert fmp4.audio_codec(cfg) == f"mp4a.40.{obj}"


def test_track_ids_and_timescales_are_the_moofs(ran):
    import remux_cases as rc

    v = rc.parse_moof(fmp4.video_moof(7, 1234, np.array([[0, 10, 3600, 0, 0x02000000]], np.int32)))
    a = rc.parse_moof(fmp4.audio_moof(7, 90000, 44100, np.array([[0, 10]], np.int32)))
    vi = cc.walk_boxes(fmp4.video_init(config_of("parse", 0, ran)))
    ai = cc.walk_boxes(fmp4.audio_init(config_of("audio", 5, ran)))
    for moof, init in ((v, vi), (a, ai)):
        trex = struct.unpack(">IIIIII", cc.find_box(init, "moov/mvex/trex").body)
        tkhd = struct.unpack(">I", cc.find_box(init, "moov/trak/tkhd").body[12:16])
        assert moof["track"] == trex[1] == tkhd[0]
    assert a["base"] == 44100  # one second of 90 kHz in the mdhd timescale of the audio init segment


def test_no_init_segment_for_a_disqualifying_status(ran):
    good = dict(config_of("audio", 5, ran))
    assert good["status"] == 0 and fmp4.video_init(good) and fmp4.audio_init(good)
    for bit in ("no_sps", "no_pps", "ps_overflow", "bad_sps", "unsupported_video"):
        cfg = dict(good, status=ST[bit])
        assert fmp4.video_init(cfg) is None and fmp4.audio_init(cfg) is not None, bit
    cfg = dict(good, status=ST["no_audio_config"])
    assert fmp4.audio_init(cfg) is None and fmp4.video_init(cfg) is not None
    # and on real rows: every case row with such a bit
    for name in ("parse", "search", "copy", "audio", "other"):
        cfg_all = ran[name][4]
        for i in range(cfg_all.cinfo.shape[0]):
            s = cfg_all.segment(i)
            assert (fmp4.video_init(s) is None) == bool(s["status"] & 31), (name, i)
            assert (fmp4.audio_init(s) is None) == bool(s["status"] & 32), (name, i)


# ---------------------------------------------------------------- pipeline and player
REAL_SPS = cc.sps_nal(profile=100, compat=0, level=31, W=79, H=44, vui={"idc": 1})


def real_jobs():
    """Four spec-built streams around a real SPS / PPS (two of them encrypted): ``(ts, payload, key, iv)``."""
    from test_esindex import _spec_stream

    rng = np.random.default_rng(31)
    key, out = bytes(range(16)), []
    for i in range(4):
        sps = cc.sps_nal(**cc.BASELINE) if i == 3 else REAL_SPS
        units = [b"\x00" + SC + b"\x09\xf0" + b"\x00" + SC + sps + SC + cc.PPS + SC + b"\x65" +
                 bytes(background(rng, 700 + 40 * i))]
        units += [b"\x00" + SC + b"\x09\xf0" + SC + b"\x41" + bytes(background(rng, 300)) for _ in range(3)]
        audio = [adts_frame(bytes(background(rng, 100)), rate_idx=4) for _ in range(4)]
        ts = _spec_stream(0x1B, units, audio)
        enc = i % 2 == 0
        iv = aes.iv_from_sn(i)
        raw = np.frombuffer(ts, np.uint8)
        out.append((ts, aes.cbc_encrypt(key, iv, raw) if enc else raw, key if enc else None, iv if enc else None))
    return out


def run_pipeline(device, ask):
    from hlsjs_p2p_wrapper_amd.net import new_event_loop
    from hlsjs_p2p_wrapper_amd.player.transmux import MediaPipeline, TransmuxJob

    pipe = MediaPipeline(torch.device(device), new_event_loop("virtual"))
    out = {}
    jobs = real_jobs()
    for n, (_, payload, key, iv) in enumerate(jobs):
        pipe.submit(TransmuxJob(torch.from_numpy(np.array(payload)), key, iv, lambda r, n=n: out.__setitem__(n, r),
                                remux=ask[n]))
    pipe.flush()
    return jobs, out


def reference_config(ts: bytes) -> dict:
    from test_esindex import _demux_cpu

    res, lens = _demux_cpu([ts])
    ix = esindex.index_batch(res, lens)
    cinfo, ps = cc.ref_batch(res, ix, lens, 256)
    return codecconfig.segment_view(cinfo[0], ps[0])


def check_config(jobs, out, ask):
    for n, (ts, _, _, _) in enumerate(jobs):
        r = out[n]
        assert r.get("error") is None and r["status"] == 0 and ("fmp4" in r) == ask[n]
        if not ask[n]:
            continue
        want = reference_config(ts)
        f = r["fmp4"]
        cfg = f["config"]
        assert dict(cfg) == want and want["status"] == 0 and "config" in f.keys() and f["config"] is cfg
        assert want["sps"] == (cc.sps_nal(**cc.BASELINE) if n == 3 else REAL_SPS) and want["pps"] == cc.PPS
        with pytest.raises(TypeError):
            cfg["width"] = 1
        v, a = f["video"], f["audio"]
        assert v["init"] == fmp4.video_init(want) and v["init"] is v["init"] and a["init"] == fmp4.audio_init(want)
        size = (640, 360) if n == 3 else (1280, 720)
        assert (v["width"], v["height"]) == size and v["codec"] == ("avc1.42c01e" if n == 3 else "avc1.64001f")
        assert (a["channelCount"], a["samplerate"], a["codec"]) == (2, 44100, "mp4a.40.2")
        assert (v["container"], a["container"]) == ("video/mp4", "audio/mp4")
        assert a["samplerate"] == a["timescale"] and {"init", "codec", "width"} <= set(v.keys())
        assert "channelCount" in a.keys() and "width" not in a.keys() and a.get("width") is None
        avcc = cc.find_box(cc.walk_boxes(v["init"]), "moov/trak/mdia/minf/stbl/stsd/avc1/avcC").body
        assert want["sps"] in avcc and want["pps"] in avcc


def test_pipeline_configures_only_the_jobs_that_remux():
    ask = [True, False, True, True]
    jobs, out = run_pipeline("cpu", ask)
    check_config(jobs, out, ask)
    _, plain = run_pipeline("cpu", [False] * 4)
    a, b = out[1], plain[1]  # a job that did not ask: the result a pipeline without the feature gives
    assert dict(a).keys() == dict(b).keys() and a["status"] == b["status"] and a["plain_bytes"] == b["plain_bytes"]
    assert a["info"].to_dict() == b["info"].to_dict()
    assert torch.equal(a["video"], b["video"]) and torch.equal(a["audio"], b["audio"])


from test_esindex import fresh  # noqa: E402,F401  (fixture)


def _play_init(config):
    from hlsjs_p2p_wrapper_amd.net import new_event_loop
    from hlsjs_p2p_wrapper_amd.net.origin import Rendition, SyntheticHlsOrigin
    from hlsjs_p2p_wrapper_amd.player import MediaElement

    loop = new_event_loop("virtual")
    origin = SyntheticHlsOrigin("http://cdn.cfg/vod/", renditions=[Rendition(300_000, 640, 360)], num_segments=4,
                                segment_duration=2.0, encrypted=True)
    hls = Hls(dict(config, transmuxDevice="cpu"), {"streamrootKey": "cfg", "gpuSwarm": {"device": "cpu",
                                                                                         "cacheBytes": 32 << 20}})
    media = MediaElement()
    inits, data, parsed = [], [], []
    hls.on(Hls.Events.FRAG_PARSING_INIT_SEGMENT, lambda e, d: inits.append(d))
    hls.on(Hls.Events.FRAG_PARSING_DATA, lambda e, d: data.append(d))
    hls.on(Hls.Events.FRAG_PARSED, lambda e, d: parsed.append(d))
    hls.loadSource(origin.master_url())
    hls.attachMedia(media)
    hls.on(Hls.Events.MANIFEST_PARSED, lambda e, d: media.play())
    assert loop.run_until(lambda: len(parsed) >= 3, timeout_ms=60_000)
    hls.destroy()
    return inits, data


def test_controller_announces_init_segments_only_under_remuxFmp4(fresh):  # noqa: F811
    from hlsjs_p2p_wrapper_amd.agent import set_current_node
    from hlsjs_p2p_wrapper_amd.net import clear_origins

    off, raw = _play_init({})
    assert len(off) == 1 and set(off[0]) == {"frag", "tracks"}
    assert off[0]["tracks"] == {"video": {"pid": 0x100, "type": 0x1B}, "audio": {"pid": 0x101, "type": 0x0F}}
    clear_origins()
    set_current_node(None)
    on, data = _play_init({"remuxFmp4": True})
    # the synthetic muxer's parameter sets are random bytes: what a fragment announces is the
    # reference parse of those same bytes, whatever it yields, and it announces when they changed
    video_es = {d["frag"].sn: d for d in raw if d["type"] == "video"}
    audio_es = {d["frag"].sn: d for d in raw if d["type"] == "audio"}
    wants, expected, last = {}, [], None
    for sn in [d["frag"].sn for d in data if d["type"] == "video"]:
        if sn not in video_es:
            break
        v, a = video_es[sn]["data1"].numpy().tobytes(), audio_es[sn]["data1"].numpy().tobytes()
        w = wants[sn] = reference_from_es(v, a)
        sig = (w["sps"], w["pps"], w["aac_object_type"], w["aac_rate_index"], w["aac_channel_config"])
        if sig != last:
            expected.append(sn)
            last = sig
    assert len(wants) >= 3 and expected[0] == min(wants)
    assert [d["frag"].sn for d in on if d["frag"].sn in wants] == expected
    for d in on:
        sn = d["frag"].sn
        if sn not in wants:
            continue
        want = wants[sn]
        tv, ta = d["tracks"]["video"], d["tracks"]["audio"]
        assert (tv["pid"], tv["type"], ta["pid"], ta["type"]) == (0x100, 0x1B, 0x101, 0x0F)
        if want["status"] & 31:
            assert set(tv) == {"pid", "type"}
        else:
            assert set(tv) == {"pid", "type", "container", "codec", "initSegment", "metadata"}
            assert tv["initSegment"] == fmp4.video_init(want) and tv["container"] == "video/mp4"
            assert tv["codec"] == fmp4.video_codec(want)
            assert tv["metadata"] == {"width": want["width"], "height": want["height"]}
            avcc = cc.find_box(cc.walk_boxes(tv["initSegment"]), "moov/trak/mdia/minf/stbl/stsd/avc1/avcC").body
            assert want["sps"] in avcc and want["pps"] in avcc
        assert not want["status"] & 32 and ta["initSegment"] == fmp4.audio_init(want)
        assert ta["metadata"] == {"channelCount": 2} and ta["codec"] == "mp4a.40.2" and ta["container"] == "audio/mp4"
        cc.walk_boxes(ta["initSegment"])


def reference_from_es(video: bytes, audio: bytes) -> dict:
    """The reference configuration of one fragment from its two ES as the raw events carry them."""
    from esindex_cases import hand_batch, seg

    s = seg(video, audio, vpes=[0], apes=[0])
    res, caps = hand_batch([s], "cpu", max_pes=8)
    ix = esindex.index_batch(res, caps)
    cinfo, ps = cc.ref_batch(res, ix, caps, 256)
    return codecconfig.segment_view(cinfo[0], ps[0])
