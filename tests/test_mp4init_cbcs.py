"""``parse_init`` on protected sample entries (``encv`` / ``enca`` with a ``sinf``): ``tenc`` version
0 and 1, the IV forms, every missing-piece fallback, ``clear_data``, and unprotected init segments
parsing to exactly what they parsed to before."""
import pytest

import cbcs_cases as cc
import mp4_cases as mc
from hlsjs_p2p_wrapper_amd.ops.cbcs import Mp4Protection
from hlsjs_p2p_wrapper_amd.ops.mp4demux import Mp4Track
from hlsjs_p2p_wrapper_amd.player.mp4init import Mp4Init, parse_init

PLAIN = [(1, b"vide", b"avc1"), (2, b"soun", b"mp4a")]


def video_init(sinf_box, entry=b"avc1"):
    return cc.protect_init(mc.init_segment([(1, b"vide", entry), (2, b"soun", b"mp4a")]), 0, sinf_box)


def test_tenc_version_1_carries_the_pattern_and_version_0_does_not():
    init = parse_init(cc.cbcs_init())
    assert init.video == Mp4Track(1, "video", 0x1B, 4, 1001, 101, 0x01010000,
                                  Mp4Protection("cbcs", 1, 9, 0, cc.iv_of(1), cc.KID))
    assert init.audio == Mp4Track(2, "audio", 0x0F, 4, 1002, 102, 0x01010000,
                                  Mp4Protection("cbcs", 0, 0, 0, cc.iv_of(2), cc.KID))
    assert (init.video_codec, init.audio_codec) == ("avc1.64001f", "mp4a") and init.timescale["video"] == 90000
    v0 = parse_init(video_init(cc.sinf(b"avc1", tenc_box=cc.tenc(version=0, pattern=(5, 5))))).video.protection
    assert (v0.crypt_byte_block, v0.skip_byte_block, v0.constant_iv) == (0, 0, cc.iv_of(1))
    v1 = parse_init(video_init(cc.sinf(b"avc1", tenc_box=cc.tenc(pattern=(2, 8), constant_iv=cc.iv_of(4, 8)))))
    assert v1.video.protection == Mp4Protection("cbcs", 2, 8, 0, cc.iv_of(4, 8), cc.KID)


def test_per_sample_ivs_other_schemes_and_hevc():
    for size in (8, 16):
        p = parse_init(video_init(cc.sinf(b"avc1", tenc_box=cc.tenc(iv_size=size)))).video.protection
        assert (p.per_sample_iv_size, p.constant_iv) == (size, b"")
    p = parse_init(video_init(cc.sinf(b"avc1", scheme=b"cenc", tenc_box=cc.tenc(version=0, iv_size=8))))
    assert p.video.protection.scheme == "cenc" and p.video_codec == "avc1.64001f"  # parsed; the decrypt refuses it
    h = parse_init(video_init(cc.sinf(b"hvc1"), entry=b"hvc1"))
    plain = parse_init(mc.init_segment([(1, b"vide", b"hvc1"), (2, b"soun", b"mp4a")]))
    assert h.video.codec_type == 0x24 and h.video_codec == plain.video_codec and h.video.protection.scheme == "cbcs"
    assert h.audio == plain.audio


@pytest.mark.parametrize("drop", ["frma", "schm", "schi", "tenc", "sinf", "short tenc", "short iv"])
def test_a_missing_piece_keeps_the_answer_of_an_unknown_entry(drop):
    if drop == "sinf":
        data = video_init(mc.box("free", bytes(12)))
    elif drop == "short tenc":
        data = video_init(cc.sinf(b"avc1", tenc_box=cc.tenc(iv_size=8, cut=1)))
    elif drop == "short iv":
        data = video_init(cc.sinf(b"avc1", tenc_box=cc.tenc(cut=1)))
    else:
        data = video_init(cc.sinf(b"avc1", drop=(drop,)))
    init = parse_init(data)
    assert init.video == Mp4Track(1, "video", 0, 4, 1001, 101, 0x01010000) and init.video_codec == "encv"
    assert init.clear_data is init.data and init.audio.codec_type == 0x0F


def test_is_protected_0_gives_no_protection_and_the_original_format():
    init = parse_init(video_init(cc.sinf(b"avc1", tenc_box=cc.tenc(is_protected=0))))
    assert init.video == Mp4Track(1, "video", 0x1B, 4, 1001, 101, 0x01010000) and init.video_codec == "avc1.64001f"
    assert init.clear_data is init.data


def test_clear_data_renames_the_entry_and_frees_the_sinf():
    data = cc.cbcs_init(audio=False)
    init = parse_init(data)
    clear = init.clear_data
    assert len(clear) == len(data) and init.data == data
    diff = [i for i in range(len(data)) if data[i] != clear[i]]
    at, sinf = data.index(b"encv"), data.index(b"sinf")
    assert diff == [at, at + 1, at + 3] + [sinf, sinf + 1, sinf + 2, sinf + 3]  # (the c of encv and avc1 stays)
    assert clear[at:at + 4] == b"avc1" and clear[sinf:sinf + 4] == b"free"
    assert parse_init(clear).video == parse_init(mc.init_segment(PLAIN)).video


def test_unprotected_init_segments_parse_to_what_they_parsed_to():
    for tracks in (PLAIN, [(1, b"vide", b"hev1"), (2, b"soun", b"mp4a")], [(7, b"vide", b"vp09")],
                   [(2, b"soun", b"ac-3")]):
        data = mc.init_segment(tracks)
        init = parse_init(data)
        assert init.clear_data is init.data and init.data == data
        for t in init.tracks:
            assert t.protection is None and t == Mp4Track(t.track_id, t.kind, t.codec_type, t.nal_length_size,
                                                          t.default_duration, t.default_size, t.default_flags)
    init = parse_init(mc.init_segment(PLAIN))
    assert init.video == Mp4Track(1, "video", 0x1B, 4, 1001, 101, 0x01010000) and init.video_codec == "avc1.64001f"
    assert init.audio == Mp4Track(2, "audio", 0x0F, 4, 1002, 102, 0x01010000) and init.audio_codec == "mp4a"
    six = Mp4Init(data, init.video, init.audio, init.timescale, init.video_codec, init.audio_codec)
    assert six.clear_data is data  # the constructor of six fields still stands
    with pytest.raises(ValueError):
        parse_init(mc.init_segment(PLAIN, bad="cut"))
