"""The host parts that make a fragmented-MP4 playlist readable: ``player.mp4init.parse_init`` on
hand-built init segments and ``#EXT-X-MAP`` in ``player.playlist``."""
import pytest

import mp4_cases as mc
from hlsjs_p2p_wrapper_amd.ops import mp4demux
from hlsjs_p2p_wrapper_amd.player import playlist
from hlsjs_p2p_wrapper_amd.player.level import InitSegment
from hlsjs_p2p_wrapper_amd.player.mp4init import parse_init

VA = [(1, b"vide", b"avc1"), (2, b"soun", b"mp4a")]


def test_tracks_of_an_avc_and_aac_init_segment():
    data = mc.init_segment(VA)
    init = parse_init(data)
    assert init.data == data and init.timescale == {"video": 90000, "audio": 48000}
    assert init.video == mp4demux.Mp4Track(1, "video", 0x1B, 4, 1001, 101, 0x01010000)
    assert init.audio == mp4demux.Mp4Track(2, "audio", 0x0F, 4, 1002, 102, 0x01010000)
    assert init.video_codec == "avc1.64001f" and init.audio_codec == "mp4a" and init.tracks == (init.video, init.audio)
    rows = mp4demux.pack_tracks(init, 3)  # an Mp4Init is a track set
    assert rows.shape == (3, 2, 8) and rows[2, 0].tolist() == [1, 1, 0x1B, 4, 1001, 101, 0x01010000, 0]
    assert rows[0, 1].tolist() == [2, 2, 0x0F, 0, 1002, 102, 0x01010000, 0]


@pytest.mark.parametrize("entry, size, want", [(b"avc3", 2, (0x1B, 2)), (b"avc1", 1, (0x1B, 1)), (b"avc1", 3, (0, 4)),
                                               (b"hvc1", 4, (0x24, 4)), (b"hev1", 2, (0x24, 2)), (b"hvc1", 3, (0, 4)),
                                               (b"vp09", 4, (0, 4))])
def test_video_entries_and_length_sizes(entry, size, want):
    init = parse_init(mc.init_segment([(7, b"vide", entry)], avcc_length_size=size))
    assert (init.video.codec_type, init.video.nal_length_size) == want and init.audio is None
    assert init.video.track_id == 7 and init.video_codec.startswith(entry.decode()[:3])


def test_first_track_of_each_kind_and_other_entries():
    init = parse_init(mc.init_segment([(5, b"soun", b"ac-3"), (6, b"soun", b"mp4a"), (9, b"vide", b"hvc1"),
                                       (3, b"vide", b"avc1")], timescales=(44100, 48000, 25000, 90000)))
    assert init.audio.track_id == 5 and init.audio.codec_type == 0 and init.audio_codec == "ac-3"
    assert init.video.track_id == 9 and init.video.codec_type == 0x24 and init.video_codec.startswith("hvc1.")
    assert init.timescale == {"audio": 44100, "video": 25000}


def test_malformed_trees_raise():
    good = mc.init_segment(VA)
    for bad in (good[:-3], good[:40], mc.box("ftyp", b"iso6"), b"", mc.box("moov", mc.box("trak", b"\0" * 5)),
                mc.box("moov", mc.box("mvex", mc.full_box("trex", 0, 0, bytes(8))))):
        with pytest.raises(ValueError):
            parse_init(bad)


def test_an_init_segment_feeds_the_demux():
    init = parse_init(mc.init_segment(VA))
    seg = mc.two_pass(lambda size: mc.box("moof", mc.mfhd(1) + mc.box("traf", mc.tfhd(1) + mc.tfdt(0) + mc.trun(
        [(0, 0, 0, 0)] * 2, fields="", data_offset=size + 8)))) + mc.box("mdat", bytes(202))
    buf, offs, lens = mc.layout([seg])
    import numpy as np
    import torch

    got = mp4demux.mp4_demux_batch(torch.from_numpy(np.frombuffer(buf, np.uint8).copy()), offs, lens, init, max_pes=4)
    v = got.segment(0)["video"]  # size, duration and flags are the trex defaults
    assert v["n_samples"] == 2 and v["samples"].tolist() == [[101, 1001, 0, 0x01010000]] * 2 and v["duration"] == 2002


M3U8 = """#EXTM3U
#EXT-X-VERSION:7
#EXT-X-TARGETDURATION:4
#EXTINF:4.0,
a0.ts
#EXT-X-MAP:URI="init.mp4"
#EXTINF:4.0,
s1.m4s
#EXTINF:4.0,
s2.m4s
#EXT-X-MAP:URI="all.mp4",BYTERANGE="720@16"
#EXT-X-BYTERANGE:1000@736
#EXTINF:4.0,
all.mp4
#EXT-X-MAP:URI="http://other/i.mp4",BYTERANGE="99"
#EXTINF:4.0,
s4.m4s
#EXT-X-ENDLIST
"""


def test_ext_x_map_applies_to_the_fragments_that_follow():
    d = playlist.parse_media(M3U8, "http://h/p/live.m3u8", 0)
    maps = [f.initSegment for f in d.fragments]
    assert maps[0] is None and maps[1] == maps[2] == InitSegment("http://h/p/init.mp4", None, None)
    assert maps[3] == InitSegment("http://h/p/all.mp4", 16, 736) and maps[4] == InitSegment("http://other/i.mp4", 0, 99)
    assert (d.fragments[3].byteRangeStartOffset, d.fragments[3].byteRangeEndOffset) == (736, 1736)
    assert len({maps[1], maps[3], maps[4]}) == 3  # hashable: what a loader caches by
    with pytest.raises(playlist.PlaylistError):
        playlist.parse_media("#EXTM3U\n#EXT-X-MAP:BYTERANGE=\"1@0\"\n", "http://h/", 0)


def test_playlists_without_the_tag_parse_as_before():
    text = playlist.write_media_playlist([("a.ts", 4.0), ("b.ts", 4.0)], 4)
    d = playlist.parse_media(text, "http://h/x.m3u8", 2)
    assert [f.initSegment for f in d.fragments] == [None, None] and [f.url for f in d.fragments] == \
        ["http://h/a.ts", "http://h/b.ts"]
