"""HEVC configuration (``ops/hevcconfig.py``) on the host implementation (``runtime/hevc.cpp``):
``hinfo`` and ``hps`` equal the independent sequential reference (``tests/hevc_cases.py``) exactly
on the hand-built cases and on the fuzz batch; the properties those cases exist for are stated on
the results; the ``hvc1`` init segment (``player/fmp4.py``) walks as ISO-BMFF boxes whose sizes add
up, its ``hvcC`` reads back through an independent parser and equals a hand-derived vector; the
configuration reaches the pipeline's results and the player's ``FRAG_PARSING_INIT_SEGMENT``, and
leaves every H.264 result as it was."""
import struct

import numpy as np
import pytest
import torch

import codec_cases as cc
import hevc_cases as hc
from esindex_cases import SC, adts_frame, background
from hlsjs_p2p_wrapper_amd.ops import aes, codecconfig, esindex, hevcconfig
from hlsjs_p2p_wrapper_amd.ops._native import runtime
from hlsjs_p2p_wrapper_amd.player import fmp4

HI, ST = hevcconfig.HINFO, hevcconfig.HSTATUS


def run_case(name: str, device="cpu"):
    case = hc.CASES[name]()
    res, ix, caps = hc.build(case, device)
    cfg = hevcconfig.hevc_config_batch(res, ix, caps, case.max_ps)
    return case, res, ix, caps, cfg, hc.ref_batch(res, ix, caps, case.max_ps)


@pytest.fixture(scope="module")
def ran():
    """Every case once, on the host."""
    return {name: run_case(name) for name in hc.CASES}


@pytest.mark.parametrize("case", sorted(hc.CASES))
def test_hand_built_cases_match_the_reference(case, ran):
    _, _, _, _, cfg, ref = ran[case]
    hc.assert_hevc_equal(cfg, ref)
    assert tuple(cfg.hinfo.shape) == (len(ref[0]), hevcconfig.HINFO_WORDS) and cfg.hinfo.dtype == torch.int32
    assert tuple(cfg.hps.shape[:2]) == (len(ref[0]), 3) and cfg.hps.dtype == torch.uint8


def rows(cfg, *names):
    return [[int(r[HI[n]]) for n in names] for r in cfg.hinfo.numpy()]


# ---------------------------------------------------------------- the hand-derived vector
def test_the_writer_and_both_parsers_agree_with_the_hand_derived_vector(ran):
    assert hc.sps_rbsp(**hc.LITERAL_KW) == hc.LITERAL_RBSP and hc.SPS_A == hc.LITERAL_SPS
    assert hc.ref_unescape(hc.LITERAL_SPS) == hc.LITERAL_RBSP and hc.escape_positions(hc.LITERAL_SPS) == [7, 12, 15]
    f = hc.ref_parse_sps(hc.LITERAL_SPS)
    assert f["ok"] and {k: f[k] for k in hc.LITERAL_FIELDS} == hc.LITERAL_FIELDS
    s = ran["parse"][4].segment(0)  # the host twin on VPS, the literal SPS, PPS
    assert {k: s[k] for k in hc.LITERAL_FIELDS} == hc.LITERAL_FIELDS and s["status"] == 0
    assert (s["vps"], s["sps"], s["pps"]) == (hc.VPS, hc.LITERAL_SPS, hc.PPS)
    assert (s["width"], s["height"], s["sps_rbsp_bytes"]) == (1920, 1080, 21)
    assert fmp4.hevc_codec(s) == hc.LITERAL_CODEC == hc.ref_codec(f) == "hvc1.1.6.L93.90"
    boxes = cc.walk_boxes(fmp4.hevc_init(s))
    hvc1 = cc.find_box(boxes, "moov/trak/mdia/minf/stbl/stsd/hvc1").body
    assert cc.find_box(cc.walk_boxes(hvc1[78:]), "hvcC").body == hc.LITERAL_HVCC


# ---------------------------------------------------------------- the properties the cases exist for
def test_parse_cases_hold_what_they_are_meant_to(ran):
    case, _, _, _, cfg, _ = ran["parse"]
    ok, bad, truncated = hc.parse_nals()
    got = rows(cfg, "status", *hc.PARSED)
    assert all(g[0] == 0 for g in got[:len(ok)])
    g = rows(cfg, "profile_space", "tier_flag", "profile_idc", "level_idc", "profile_compat", "constraint_hi",
             "constraint_lo")
    assert g[2] == [0, 1, 2, 153, 0x20000000, 0xB000, 0]
    assert g[3] == [1, 0, 4, 255, -1, 0xFFFF, -1]  # all 32 and all 48 bits: the int32 bit patterns
    assert g[4] == [2, 1, 31, 0, -0x7FFFFFFF, 0, 1] and g[5] == [3, 0, 0, 30, 0, 0, 0]
    size = rows(cfg, "chroma_format_idc", "width", "height")
    # per chroma format: no window, then one side each (left 1, right 2, top 3, bottom 4)
    assert size[6:11] == [[0, 640, 368], [0, 639, 368], [0, 638, 368], [0, 640, 365], [0, 640, 364]]
    assert size[11:16] == [[1, 640, 368], [1, 638, 368], [1, 636, 368], [1, 640, 362], [1, 640, 360]]
    assert size[16:21] == [[2, 640, 368], [2, 638, 368], [2, 636, 368], [2, 640, 365], [2, 640, 364]]
    assert size[21:26] == size[26:31] == [[3, 640, 368], [3, 639, 368], [3, 638, 368], [3, 640, 365], [3, 640, 364]]
    assert rows(cfg, "bit_depth_luma", "bit_depth_chroma")[31:36] == [[8, 8], [10, 10], [16, 16], [16, 8], [8, 16]]
    assert size[36:39] == [[1, 1, 1], [1, 65535, 65535], [1, 65535, 9]] and got[39][0] == 0
    assert len(ok) == 40
    for i in range(len(ok), len(ok) + len(bad) + len(truncated)):  # every error: the bit, and zeros in every field
        assert got[i] == [ST["bad_sps"]] + [0] * len(hc.PARSED), i
    seg = cfg.segment(len(ok) + len(bad) - 2)
    assert seg["sps"] == hc.SPS_HDR and seg["sps_rbsp_bytes"] == 0
    seg = cfg.segment(len(ok) + len(bad) - 1)
    assert seg["sps"] == hc.SPS_HDR[:1] and seg["sps_bytes"] == 1 and seg["sps_rbsp_bytes"] == 0
    assert len(truncated) > 50
    # the sub-layer mixes: the picture size sits behind them
    first = len(ok) + len(bad) + len(truncated)
    layers = rows(cfg, "status", "num_temporal_layers", "temporal_id_nested", "width", "height")[first:]
    assert len(layers) == 25 + 100 and {l[1] for l in layers} == set(range(1, 8))
    assert all(l == [0, l[1], i & 1, 64 + i, 48 + 2 * i] for i, l in enumerate(layers))
    assert all(s["vps"] == hc.VPS and s["pps"] == hc.PPS and (s["vps_nal"], s["sps_nal"], s["pps_nal"]) == (0, 1, 2)
               for s in map(cfg.segment, range(0, len(got), 7)))


def test_every_mix_of_the_sub_layer_flags():
    """``L = 0..6``, all 4^L mixes of (profile present, level present): 5461 SPS."""
    case = hc.sublayer_cases()
    assert len(case.segs) == sum(4 ** L for L in range(7)) == 5461
    res, ix, caps = hc.build(case)
    cfg = hevcconfig.hevc_config_batch(res, ix, caps)
    hc.assert_hevc_equal(cfg, hc.ref_batch(res, ix, caps, 256))
    got = rows(cfg, "status", "num_temporal_layers", "width", "height")
    assert all(g == [0, len(m) + 1, 64 + i, 48 + 2 * i] for i, (g, m) in enumerate(zip(got, hc.SUB_MIXES)))


def test_unescape_cases_hold_what_they_are_meant_to(ran):
    case, _, _, _, cfg, _ = ran["unescape"]
    segs = [cfg.segment(i) for i in range(len(case.segs))]
    assert all(s["status"] == 0 for s in segs)
    assert segs[0]["sps"][:6] == b"\x42\x01\x00\x00\x03\x01" and hc.escape_positions(segs[0]["sps"])[0] == 4
    assert segs[1]["sps"][:4] == b"\x42\x00\x00\x03" and hc.escape_positions(segs[1]["sps"])[0] == 3
    assert (segs[0]["width"], segs[0]["height"]) == (segs[1]["width"], segs[1]["height"]) == (352, 288)
    assert segs[1]["sps_rbsp_bytes"] == segs[0]["sps_rbsp_bytes"]
    assert hc.escape_positions(segs[2]["sps"])[0] == 6 and segs[2]["profile_compat"] == 1  # inside the 32 flags
    assert hc.escape_positions(segs[3]["sps"])[0] == 7 and segs[3]["profile_compat"] == 0x60000000
    n = len(hc.SPS_A)
    assert [s["sps_rbsp_bytes"] - (n - 2 - 3) for s in segs[4:8]] == [2, 4, 4, 4]  # 03 at the end; two; one; one
    for s, j in zip(segs[8:18], (62, 63, 64, 65, 127, 128, 254, 255, 256, 257)):
        assert hc.escape_positions(s["sps"])[-1] == j and s["sps_bytes"] == 300
        assert s["sps_rbsp_bytes"] == 300 - 2 - len(hc.escape_positions(s["sps"]))
        assert (s["width"], s["height"]) == (1920, 1080)
    assert hc.escape_positions(segs[18]["sps"])[-1] == 511 and segs[18]["sps_bytes"] == 512 == case.max_ps
    assert not segs[18]["status"] & ST["ps_overflow"]
    assert segs[19]["sps_rbsp_bytes"] == 300 - 2 - 3 - 6
    moving = segs[20:]
    at = set()
    for i, s in enumerate(moving):
        pos = hc.escape_positions(s["sps"])
        at |= set(pos)
        assert (s["width"], s["height"]) == (1280 + i, 720 - 2 * i) and len(pos) >= 3
        assert s["sps_rbsp_bytes"] == s["sps_bytes"] - 2 - len(pos)
        kept = hc.ref_parse_rbsp(s["sps"][2:])  # what a parser that kept the 03 bytes would read
        assert (kept["width"], kept["height"]) != (s["width"], s["height"])
    assert {63, 64} <= at  # an escape on either side of the first wave edge, parsed fields behind it


def test_search_cases_hold_what_they_are_meant_to(ran):
    _, _, ix, _, cfg, _ = ran["search"]
    got = rows(cfg, "status", "vps_nal", "sps_nal", "pps_nal")
    assert got[0] == [0, 0, 1, 2] and got[1] == [0, 255, 256, 257] and got[2] == [0, 254, 255, 256]
    assert got[3] == [0, 256, 257, 258] and got[4] == [0, 511, 512, 513] and got[5] == [0, 0, 301, 502]
    assert got[6] == [0, 73, 71, 0]
    s = cfg.segment(7)
    assert got[7] == [0, 0, 2, 4] and (s["vps"], s["sps"], s["pps"]) == (hc.VPS, hc.SPS_A, hc.PPS)
    assert got[8] == [ST["no_vps"] | ST["no_sps"] | ST["no_pps"], -1, -1, -1]
    assert int(ix.sinfo[8, esindex.SINFO["status"]]) & esindex.SSTATUS["nal_overflow"]
    assert got[9] == [ST["no_pps"], 518, 519, -1]
    assert got[10] == [0, 3, 4, 5] and ix.nal[10, :3, 1:3].tolist() == [[0, 32], [0, 33], [0, 34]]
    assert cfg.segment(10)["sps"] == hc.SPS_B
    assert got[11] == [0, 0, 1, 2] and ix.nal[11, :4, 3].tolist() == [-1, -1, -1, 0]
    assert got[12] == [ST["no_vps"], -1, 0, 1] and got[13] == [ST["no_sps"], 0, -1, 1]
    assert got[14] == [ST["no_pps"], 0, 1, -1] and got[15] == [7, -1, -1, -1]
    assert cfg.segment(13)["sps"] == b"" and not cfg.hps[13, 1].any() and cfg.segment(13)["width"] == 0


@pytest.mark.parametrize("name", ["copy_16", "copy", "copy_1024"])
def test_copy_cases_hold_what_they_are_meant_to(name, ran):
    case, res, ix, caps, cfg, _ = ran[name]
    max_ps, n = case.max_ps, len(case.segs)
    assert tuple(cfg.hps.shape) == (n, 3, max_ps)
    offs = [int(ix.nal[i, 0, 0]) for i in range(20)]
    assert {o % 4 for o in offs} == {0, 1, 2, 3} and {o % 16 for o in offs} >= set(range(3, 16))
    es = res.es.numpy()
    for i in list(range(n - 3)) + [n - 1]:  # stored bytes are the ES bytes, zero behind them
        s = cfg.segment(i)
        for which, name_ in enumerate(("vps", "sps", "pps")):
            k, ln = s[name_ + "_nal"], s[name_ + "_bytes"]
            o = int(res.es_offs[i]) + int(ix.nal[i, k, 0])
            stored = min(ln, max_ps)
            assert cfg.hps[i, which, :stored].numpy().tobytes() == es[o:o + stored].tobytes() == s[name_]
            assert not cfg.hps[i, which, stored:].any()
    lengths = (1, 2, 15, 16, 17, max_ps, max_ps + 1)
    for j, ln in enumerate(lengths):
        v, s, p = (cfg.segment(20 + 3 * j + k) for k in range(3))
        assert (v["vps_bytes"], s["sps_bytes"], p["pps_bytes"]) == (ln, ln, ln)
        for seg_ in (v, s, p):
            over = any(seg_[k + "_bytes"] > max_ps for k in ("vps", "sps", "pps"))
            assert bool(seg_["status"] & ST["ps_overflow"]) == over
        if ln > max_ps:  # an overflowed SPS is not parsed
            assert [s[k] for k in ("sps_rbsp_bytes",) + hc.PARSED] == [0] * 15 and not s["status"] & ST["bad_sps"]
            assert len(s["sps"]) == max_ps
        elif ln >= len(hc.SPS_A):
            assert s["width"] == 1920 and s["sps_rbsp_bytes"] == ln - 2 - 3
        else:
            assert s["status"] & ST["bad_sps"]
            assert s["sps_rbsp_bytes"] == max(ln - 2 - len(hc.escape_positions(s["sps"])), 0)
    tail, long_row, far_row, last = (cfg.segment(i) for i in range(n - 4, n))
    end = int(ix.nal[n - 4, 2, 0]) + tail["sps_bytes"]  # the SPS is the last bytes of the video ES
    assert end == int(res.info[n - 4, hc.INFO["video_bytes"]]) and es[int(res.es_offs[n - 4]) + end] == 0xFF
    assert long_row["sps_bytes"] == caps[n - 3] - 3 and int(ix.nal[n - 3, 0, 1]) == 5000  # clamped to the cap
    assert far_row["sps_bytes"] == 0 and far_row["status"] & ST["bad_sps"] and far_row["sps"] == b""
    # a negative offset reads from the segment's start
    assert far_row["vps"] == (SC + hc.filler_sps(60))[:min(len(hc.VPS), max_ps)]
    assert int(res.es_offs[-1]) + caps[-1] == res.es.numel() and res.es.numel() % 4 == 0  # the ES ends with the tensor
    assert last["sps_bytes"] == max_ps and last["sps"] == hc.filler_sps(max_ps)


def test_other_codecs_get_not_hevc_and_untouched_zeros(ran):
    _, _, _, _, cfg, _ = ran["other"]
    got = rows(cfg, *hc.NAMES)
    blank = [ST["not_hevc"], -1, 0, -1, 0, 0, -1] + [0] * 15
    assert got[0] == got[1] == got[2] == blank and not cfg.hps[:3].any()
    assert got[3][:8] == [0, 0, len(hc.VPS), 1, len(hc.SPS_A), 21, 2, len(hc.PPS)] and got[3][20:] == [1920, 1080]
    assert got[4] == [7, -1, 0, -1, 0, 0, -1] + [0] * 15  # HEVC without a byte: searched, nothing found


def test_fuzz_reaches_both_outcomes(ran):
    _, _, _, _, cfg, _ = ran["fuzz"]
    status = cfg.hinfo[:, HI["status"]].numpy()
    parsed = cfg.hinfo[:, HI["sps_nal"]].numpy() >= 0
    bad = (status & ST["bad_sps"]) != 0
    good = parsed & ~bad & (cfg.hinfo[:, HI["width"]].numpy() > 0)
    assert len(status) == 256 and int(bad.sum()) > 0 and int(good.sum()) > 0
    assert int((cfg.hinfo[:, HI["sps_rbsp_bytes"]] < cfg.hinfo[:, HI["sps_bytes"]] - 2).sum()) > 10  # escapes occur


def test_empty_batch_and_argument_errors():
    res, ix, caps = hc.build(hc.Case([]))
    cfg = hevcconfig.hevc_config_batch(res, ix, caps)
    assert tuple(cfg.hinfo.shape) == (0, 22) and tuple(cfg.hps.shape) == (0, 3, 256)
    res, ix, caps = hc.build(hc.other_cases())
    for bad in (0, 24, 2048, -16):
        with pytest.raises(ValueError, match="max_ps"):
            hevcconfig.hevc_config_batch(res, ix, caps, bad)
    other = esindex.index_batch(res, caps, max_nal=8)
    other = esindex.EsIndex(other.nal[:3], other.au[:3], other.aframes[:3], other.sinfo[:3])
    with pytest.raises(ValueError, match="does not belong"):
        hevcconfig.hevc_config_batch(res, other, caps)
    with pytest.raises(ValueError, match="out of bounds"):
        hevcconfig.hevc_config_batch(res, ix, [c + (1 << 20) for c in caps])
    rt = runtime()
    args = (res.es.numpy(), np.asarray(res.es_offs), np.asarray(caps, np.int64), res.info.numpy(), res.pes.numpy(), 8,
            8, ix.nal.numpy(), ix.au.numpy(), ix.aframes.numpy(), ix.sinfo.numpy())
    with pytest.raises(ValueError, match="max_ps"):
        rt.hevc_config_batch(*args, 24, np.zeros((5, 22), np.int32), np.zeros((5, 3, 24), np.uint8))
    with pytest.raises(ValueError, match="too small"):
        rt.hevc_config_batch(*args, 32, np.zeros(5 * 22 - 1, np.int32), np.zeros((5, 3, 32), np.uint8))
    with pytest.raises(ValueError, match="too small"):
        rt.hevc_config_batch(*args, 32, np.zeros(5 * 22, np.int32), np.zeros(5 * 3 * 32 - 1, np.uint8))
    with pytest.raises(ValueError, match="max_pes and max_nal"):
        rt.hevc_config_batch(*args[:5], 0, *args[6:], 32, np.zeros(5 * 22, np.int32), np.zeros(5 * 3 * 32, np.uint8))


def test_layout_names_equal_the_runtime_exports():
    rt = runtime()
    assert hevcconfig.HINFO == dict(rt.ES_HINFO) and hevcconfig.HINFO_WORDS == rt.ES_HINFO_WORDS == 22
    assert hevcconfig.HSTATUS == dict(rt.ES_HSTATUS) and hevcconfig.DEFAULT_MAX_PS == rt.ES_DEFAULT_MAX_PS == 256
    assert hevcconfig.HPS_ROWS == rt.ES_HPS_ROWS == 3
    assert sorted(hevcconfig.HINFO.values()) == list(range(hevcconfig.HINFO_WORDS))
    assert list(hevcconfig.HINFO) == list(hc.NAMES) and hevcconfig.HINFO == hc.H
    assert hevcconfig.HSTATUS == {"no_vps": 1, "no_sps": 2, "no_pps": 4, "ps_overflow": 8, "bad_sps": 16,
                                  "not_hevc": 32}
    assert fmp4.HEVC_DISQUALIFIED == 63 and fmp4.VIDEO_DISQUALIFIED == 31
    assert rt.ES_CINFO_WORDS == 19 and codecconfig.CSTATUS == dict(rt.ES_CSTATUS)  # cinfo did not move
    from hlsjs_p2p_wrapper_amd import ops

    assert ops.hevc_config_batch is hevcconfig.hevc_config_batch and ops.HevcConfig is hevcconfig.HevcConfig
    assert ops.config_batch is codecconfig.config_batch


# ---------------------------------------------------------------- init segments
from test_codecconfig import tree  # noqa: E402  (the box tree every init segment has)


def hvcc_of(data: bytes) -> bytes:
    hvc1 = cc.find_box(cc.walk_boxes(data), "moov/trak/mdia/minf/stbl/stsd/hvc1").body
    inner = cc.walk_boxes(hvc1[78:])
    assert [b.kind for b in inner] == ["hvcC"]  # no pasp
    return inner[0].body


def test_hevc_init_segment(ran):
    cfg = ran["parse"][4].segment(15)  # 4:2:0, 640 x 368 with a bottom offset of 4: 640 x 360
    assert (cfg["width"], cfg["height"]) == (640, 360)
    data = fmp4.hevc_init(cfg)
    boxes = cc.walk_boxes(data)
    assert cc.box_kinds(boxes) == tree("vmhd", "hvc1")
    assert cc.find_box(boxes, "ftyp").body == b"isom\x00\x00\x00\x01isomhvc1"
    hvc1 = cc.find_box(boxes, "moov/trak/mdia/minf/stbl/stsd/hvc1").body
    assert struct.unpack(">HH", hvc1[24:28]) == (640, 360) and hvc1[6:8] == b"\x00\x01"
    avc = fmp4.video_init(dict(codecconfig.segment_view(np.zeros(19, np.int32), np.zeros((2, 16), np.uint8)),
                               width=640, height=360, sar_width=1, sar_height=1))
    avc1 = cc.find_box(cc.walk_boxes(avc), "moov/trak/mdia/minf/stbl/stsd/avc1").body
    assert hvc1[:78] == avc1 and len(avc1) == 78  # the same visual sample entry
    tkhd = cc.find_box(boxes, "moov/trak/tkhd").body
    assert struct.unpack(">I", tkhd[12:16]) == (fmp4.VIDEO_TRACK,) and tkhd[:4] == b"\x00\x00\x00\x07"
    assert struct.unpack(">II", tkhd[-8:]) == (640 << 16, 360 << 16)  # the plain 16.16 values
    assert struct.unpack(">II", cc.find_box(boxes, "moov/trak/mdia/mdhd").body[12:20]) == (fmp4.VIDEO_TIMESCALE, 0)
    assert cc.find_box(boxes, "moov/trak/mdia/hdlr").body[8:12] == b"vide"
    for path in ("moov/mvex/trex", "moov/mvhd", "moov/trak/mdia/mdhd", "moov/trak/mdia/hdlr",
                 "moov/trak/mdia/minf/vmhd"):
        assert cc.find_box(boxes, path).body == cc.find_box(cc.walk_boxes(avc), path).body, path
    with pytest.raises(ValueError):
        cc.walk_boxes(data[:-1])
    with pytest.raises(ValueError):
        hc.parse_hvcc(hvcc_of(data) + b"\x00")


def test_hvcc_reads_back_through_the_independent_parser(ran):
    cfg_all, ref = ran["parse"][4], ran["parse"][5]
    seen = 0
    for i in range(cfg_all.hinfo.shape[0]):
        s = cfg_all.segment(i)
        if s["status"] or max(s["bit_depth_luma"], s["bit_depth_chroma"]) > 15:  # hvcC has three bits per depth
            assert fmp4.hevc_init(s) is None and fmp4.hevc_codec(s) is None
            continue
        want = hc.ref_view(ref[0][i], ref[1][i])
        r = hc.parse_hvcc(hvcc_of(fmp4.hevc_init(s)))
        assert r["version"] == 1 and r["length_size_minus_one"] == 3 and r["avg_frame_rate"] == 0
        assert (r["min_spatial_segmentation_idc"], r["parallelism_type"], r["constant_frame_rate"]) == (0, 0, 0)
        assert (r["profile_space"], r["tier_flag"], r["profile_idc"], r["level_idc"]) == \
            (want["profile_space"], want["tier_flag"], want["profile_idc"], want["level_idc"])
        assert r["profile_compat"] == want["profile_compat"] & 0xFFFFFFFF
        assert r["constraint"] == (want["constraint_hi"] << 32) | (want["constraint_lo"] & 0xFFFFFFFF)
        assert (r["chroma_format_idc"], r["bit_depth_luma_minus8"] + 8, r["bit_depth_chroma_minus8"] + 8) == \
            (want["chroma_format_idc"], want["bit_depth_luma"], want["bit_depth_chroma"])
        assert (r["num_temporal_layers"], r["temporal_id_nested"]) == \
            (want["num_temporal_layers"], want["temporal_id_nested"])
        assert r["arrays"] == [(1, 32, [want["vps"]]), (1, 33, [want["sps"]]), (1, 34, [want["pps"]])]
        assert fmp4.hevc_codec(s) == hc.ref_codec(want)
        seen += 1
    assert seen > 150


def test_codec_strings(ran):
    cfg = ran["parse"][4]
    assert fmp4.hevc_codec(cfg.segment(0)) == "hvc1.1.6.L93.90"
    assert fmp4.hevc_codec(cfg.segment(2)) == "hvc1.2.4.H153.B0"  # Main 10, high tier, level 5.1
    assert fmp4.hevc_codec(cfg.segment(3)) == "hvc1.A4.FFFFFFFF.L255.FF.FF.FF.FF.FF.FF"
    assert fmp4.hevc_codec(cfg.segment(4)) == "hvc1.B31.80000001.H0.0.0.0.0.0.1"  # zero bytes in front of the last stay
    assert fmp4.hevc_codec(cfg.segment(5)) == "hvc1.C0.0.L30"  # no constraint byte left


def test_no_init_segment_for_a_disqualifying_status(ran):
    good = dict(ran["parse"][4].segment(0))
    assert good["status"] == 0 and fmp4.hevc_init(good) and fmp4.hevc_codec(good)
    for bit in ST:
        cfg = dict(good, status=ST[bit])
        assert fmp4.hevc_init(cfg) is None and fmp4.hevc_codec(cfg) is None, bit
    deep = dict(good, bit_depth_luma=16)
    assert fmp4.hevc_init(deep) is None and fmp4.hevc_codec(deep) is None
    assert fmp4.hevc_init(dict(good, bit_depth_luma=15))
    for name in ("search", "copy", "other", "fuzz"):
        cfg_all = ran[name][4]
        for i in range(cfg_all.hinfo.shape[0]):
            s = cfg_all.segment(i)
            none = bool(s["status"] & 63) or max(s["bit_depth_luma"], s["bit_depth_chroma"]) > 15
            assert (fmp4.hevc_init(s) is None) == (fmp4.hevc_codec(s) is None) == none, (name, i)


# ---------------------------------------------------------------- pipeline and player
def hevc_jobs(vps=hc.VPS):
    """Six spec-built streams, HEVC and H.264 alternating, every third encrypted:
    ``(ts, payload, key, iv, hevc)``."""
    from test_codecconfig import REAL_SPS
    from test_esindex import _spec_stream

    rng = np.random.default_rng(61)
    key, out = bytes(range(16)), []
    for i in range(6):
        hevc = i % 2 == 0
        if hevc:
            sps = hc.SPS_B if i == 4 else hc.SPS_A
            units = [b"\x00" + SC + b"\x46\x01\x50" + b"\x00" + SC + vps + SC + sps + SC + hc.PPS + SC + b"\x26\x01" +
                     bytes(background(rng, 700 + 40 * i))]
            units += [b"\x00" + SC + b"\x46\x01\x50" + SC + b"\x02\x01" + bytes(background(rng, 300)) for _ in range(3)]
        else:
            units = [b"\x00" + SC + b"\x09\xf0" + b"\x00" + SC + REAL_SPS + SC + cc.PPS + SC + b"\x65" +
                     bytes(background(rng, 700 + 40 * i))]
            units += [b"\x00" + SC + b"\x09\xf0" + SC + b"\x41" + bytes(background(rng, 300)) for _ in range(3)]
        audio = [adts_frame(bytes(background(rng, 100)), rate_idx=4) for _ in range(4)]
        ts = _spec_stream(0x24 if hevc else 0x1B, units, audio)
        enc = i % 3 == 0
        iv = aes.iv_from_sn(i)
        raw = np.frombuffer(ts, np.uint8)
        out.append((ts, aes.cbc_encrypt(key, iv, raw) if enc else raw, key if enc else None, iv if enc else None, hevc))
    return out


def run_pipeline(device, jobs, remux=True):
    from hlsjs_p2p_wrapper_amd.net import new_event_loop
    from hlsjs_p2p_wrapper_amd.player.transmux import MediaPipeline, TransmuxJob

    pipe = MediaPipeline(torch.device(device), new_event_loop("virtual"))
    out = {}
    for n, (_, payload, key, iv, _) in enumerate(jobs):
        pipe.submit(TransmuxJob(torch.from_numpy(np.array(payload)), key, iv, lambda r, n=n: out.__setitem__(n, r),
                                remux=remux))
    pipe.flush()
    return out


def reference_rows(ts: bytes):
    """``(config, hevc)`` of one stream by the two references."""
    from test_esindex import _demux_cpu

    res, lens = _demux_cpu([ts])
    ix = esindex.index_batch(res, lens)
    cinfo, ps = cc.ref_batch(res, ix, lens, 256)
    hinfo, hps = hc.ref_batch(res, ix, lens, 256)
    return codecconfig.segment_view(cinfo[0], ps[0]), hc.ref_view(hinfo[0], hps[0])


def check_pipeline(jobs, out):
    for n, (ts, _, _, _, hevc) in enumerate(jobs):
        r = out[n]
        assert r.get("error") is None and r["status"] == 0 and "fmp4" in r
        want_cfg, want_hevc = reference_rows(ts)
        f = r["fmp4"]
        assert dict(f["config"]) == want_cfg and dict(f["hevc"]) == want_hevc and f["hevc"] is f["hevc"]
        assert {"config", "hevc"} <= set(f.keys())
        with pytest.raises(TypeError):
            f["hevc"]["width"] = 1
        v, a = f["video"], f["audio"]
        assert a["init"] == fmp4.audio_init(want_cfg) is not None and a["codec"] == "mp4a.40.2"
        assert v["container"] == "video/mp4"
        if hevc:
            assert want_cfg["status"] == codecconfig.CSTATUS["unsupported_video"] and want_hevc["status"] == 0
            sps = hc.SPS_B if n == 4 else hc.SPS_A
            assert (want_hevc["vps"], want_hevc["sps"], want_hevc["pps"]) == (hc.VPS, sps, hc.PPS)
            # the reference's bytes: the init segment of the reference rows, and its hvcC piece by piece
            assert v["init"] == fmp4.hevc_init(want_hevc) is not None and v["init"] is v["init"]
            got = hc.parse_hvcc(hvcc_of(v["init"]))
            assert got["arrays"] == [(1, 32, [hc.VPS]), (1, 33, [sps]), (1, 34, [hc.PPS])]
            assert v["codec"] == hc.ref_codec(want_hevc) == ("hvc1.1.6.L120.90" if n == 4 else "hvc1.1.6.L93.90")
            assert (v["width"], v["height"]) == ((1280, 720) if n == 4 else (1920, 1080))
            if n != 4:
                assert hvcc_of(v["init"]) == hc.LITERAL_HVCC
        else:
            assert want_cfg["status"] == 0 and want_hevc["status"] == hevcconfig.HSTATUS["not_hevc"]
            assert (want_hevc["vps"], want_hevc["sps"], want_hevc["pps"]) == (b"", b"", b"")
            assert v["init"] == fmp4.video_init(want_cfg) is not None and v["codec"] == "avc1.64001f"
            assert (v["width"], v["height"]) == (1280, 720)


def test_pipeline_builds_hevc_init_segments_and_leaves_h264_alone():
    jobs = hevc_jobs()
    out = run_pipeline("cpu", jobs)
    check_pipeline(jobs, out)
    # the H.264 jobs alone, in a batch no HEVC job is part of: the same results
    avc = [j for j in jobs if not j[4]]
    alone = run_pipeline("cpu", avc)
    for k, n in enumerate(i for i, j in enumerate(jobs) if not j[4]):
        a, b = out[n]["fmp4"], alone[k]["fmp4"]
        assert dict(a["config"]) == dict(b["config"])
        for track in ("video", "audio"):
            assert a[track]["init"] == b[track]["init"] and a[track]["codec"] == b[track]["codec"]
            assert a[track]["moof"](7) == b[track]["moof"](7)
            assert torch.equal(a[track]["mdat"], b[track]["mdat"])
    plain = run_pipeline("cpu", jobs, remux=False)  # without the remux nothing of this is there
    assert all("fmp4" not in plain[n] for n in plain)


from test_esindex import fresh  # noqa: E402,F401  (fixture)


def _announce(config, results):
    """The stream controller's parsing step on pipeline results, as ``onFragLoaded`` hands them
    over: the ``FRAG_PARSING_INIT_SEGMENT`` events they cause."""
    from hlsjs_p2p_wrapper_amd.net import new_event_loop
    from hlsjs_p2p_wrapper_amd.player import Hls
    from hlsjs_p2p_wrapper_amd.player.level import Fragment

    new_event_loop("virtual")
    hls = Hls(dict(config, transmuxDevice="cpu", autoStartLoad=False))
    inits = []
    hls.on(Hls.Events.FRAG_PARSING_INIT_SEGMENT, lambda e, d: inits.append(d))
    sc = hls.streamController
    for sn, r in enumerate(results):
        frag = Fragment(f"http://cdn.hevc/seg{sn}.ts", sn, 2.0 * sn, 2.0)
        sc.inflight[(frag.level, frag.sn)] = frag
        sc._on_parsed(frag, {"trequest": 0, "tfirst": 0, "length": 1000}, r)
    hls.destroy()
    return inits


def test_player_announces_the_hevc_track_and_again_on_a_changed_vps(fresh):  # noqa: F811
    vps_b = hc.VPS[:-1] + b"\x0a"
    first, second = hevc_jobs(), hevc_jobs(vps_b)
    a, b = run_pipeline("cpu", first), run_pipeline("cpu", second)
    # HEVC with VPS A twice, the same with VPS B, then the 1280 x 720 one (another SPS) with VPS B
    results = [a[0], a[2], b[0], b[4], b[4]]
    inits = _announce({"remuxFmp4": True}, results)
    assert [d["frag"].sn for d in inits] == [0, 2, 3]
    want = [reference_rows(first[0][0])[1], reference_rows(second[0][0])[1], reference_rows(second[4][0])[1]]
    assert want[0]["vps"] == hc.VPS and want[1]["vps"] == vps_b and want[0]["sps"] == want[1]["sps"]
    for d, w in zip(inits, want):
        tv, ta = d["tracks"]["video"], d["tracks"]["audio"]
        assert (tv["pid"], tv["type"], ta["pid"], ta["type"]) == (0x100, 0x24, 0x101, 0x0F)
        assert set(tv) == {"pid", "type", "container", "codec", "initSegment", "metadata"}
        assert tv["initSegment"] == fmp4.hevc_init(w) and tv["container"] == "video/mp4"
        assert tv["codec"] == hc.ref_codec(w) and tv["metadata"] == {"width": w["width"], "height": w["height"]}
        assert hc.parse_hvcc(hvcc_of(tv["initSegment"]))["arrays"][0] == (1, 32, [w["vps"]])
        assert ta["codec"] == "mp4a.40.2" and ta["initSegment"] is not None
    assert inits[2]["tracks"]["video"]["metadata"] == {"width": 1280, "height": 720}
    # with remuxFmp4 off nothing changes: one announcement per level, pids and types only
    off = _announce({}, results)
    assert len(off) == 1 and off[0]["tracks"] == {"video": {"pid": 0x100, "type": 0x24},
                                                  "audio": {"pid": 0x101, "type": 0x0F}}
