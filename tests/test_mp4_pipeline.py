"""Fragmented-MP4 fragments through the transmux pipeline (``TransmuxJob(mp4=...)``) and through a
player whose playlist carries ``#EXT-X-MAP``: the result mapping, AES-128 rows, jobs with and
without an ``Mp4Init`` in one batch, the parsing events, the init segment loaded once, and damaged
fragments as ``FRAG_PARSING_ERROR``."""
import numpy as np
import pytest
import torch

import mp4_cases as mc
from hlsjs_p2p_wrapper_amd.net import new_event_loop
from hlsjs_p2p_wrapper_amd.net.origin import StaticOrigin
from hlsjs_p2p_wrapper_amd.ops import aes, tsdemux
from hlsjs_p2p_wrapper_amd.player import Hls, MediaElement
from hlsjs_p2p_wrapper_amd.player.mp4init import parse_init
from hlsjs_p2p_wrapper_amd.player.transmux import MediaPipeline, TransmuxJob
from test_esindex import fresh  # noqa: F401  (fixture)

KEY, IV = bytes(range(16)), bytes(range(16, 32))
INIT = mc.init_segment([(1, b"vide", b"avc1"), (2, b"soun", b"mp4a")])


def fragments():
    """Two fragments of two seconds each: the H.264 caption fragment of ``mp4_cases``, and an ID3
    ``emsg`` in front of three video and three audio samples that follow it in time."""
    first = mc.case_captions(duration=30000, audio_duration=32000)[0][0]
    id3 = mc.emsg(1, mc.ID3_SCHEME, b"", 90000, 180000, 0, 3, b"ID3\x04\0\0\0\0\0\0")
    second = mc.fragment([(1, 270000, mc.video_samples(3), mc.meta(3, 60000)),
                          (2, 144000, [b"aac!"] * 3, mc.meta(3, 32000))], seq=2)
    return [first, id3 + second]


def run(device, jobs):
    p = MediaPipeline(torch.device(device))
    p.auto_flush = False
    for j in jobs:
        p.submit(j)
    p.complete(p.launch())


def check_pipeline(device):
    init = parse_init(INIT)
    frags = fragments()
    ts, _ = tsdemux.mux_segment(target_bytes=40 * 188, seed=5)
    cipher = aes.cbc_encrypt(KEY, IV, np.frombuffer(frags[1], np.uint8))  # (pads by PKCS#7)
    out = {}
    run(device, [TransmuxJob(frags[0], None, None, lambda r: out.__setitem__("clear", r), mp4=init, captions=True),
                 TransmuxJob(ts, None, None, lambda r: out.__setitem__("ts", r)),
                 TransmuxJob(bytes(cipher), KEY, IV, lambda r: out.__setitem__("enc", r), mp4=init, remux=True),
                 TransmuxJob(bytes(cipher)[:-3], KEY, IV, lambda r: out.__setitem__("odd", r), mp4=init)])
    assert "container" not in out["ts"] and out["ts"]["status"] == 0 and out["ts"]["info"]["n_packets"] > 0
    c, e = out["clear"], out["enc"]
    assert c["container"] == e["container"] == "mp4" and c["status"] == e["status"] == 0 and c["init"] is init
    assert c["plain_bytes"] == len(frags[0]) and e["plain_bytes"] == len(frags[1])
    assert bytes(c["data"].cpu().numpy()) == frags[0] and bytes(e["data"].cpu().numpy()) == frags[1]
    assert c["info"]["n_moof"] == 1 and c["info"]["first_sequence"] == 1 and c["emsg"] == []
    v, a = c["video"], c["audio"]
    assert (v["nb"], v["base"], v["duration"], v["timescale"], v["first_pts"], v["last_pts"]) == \
        (6, 90000, 180000, 90000, 90000, 249000)
    assert (a["nb"], a["base"], a["duration"], a["timescale"]) == (3, 48000, 96000, 48000)
    assert (a["id"], a["codec"]) == (2, "mp4a")
    assert v["samples"].shape == (6, 4) and v["samples"].device.type == torch.device(device).type
    assert v["samples"][:, 1].tolist() == [30000] * 6 and v["pes"][0].tolist()[1:] == [90000, 90000]
    assert c["captions"]["n_samples"] == 5 and len(c["captions"].host()["samples"]) == 5
    assert c["samples"]["independent"] and c["samples"]["n_nal"] == 17  # captions imply the index
    assert "captions" not in e and "samples" not in e and "fmp4" not in e  # remux is ignored
    assert [m["is_id3"] for m in e["emsg"]] == [1] and e["emsg"][0]["time"] == 180000 and e["video"]["nb"] == 3
    assert isinstance(out["odd"]["error"], ValueError) and out["odd"]["container"] == "mp4"
    with pytest.raises(ValueError, match="SAMPLE-AES"):
        TransmuxJob(frags[0], None, None, print, mp4=init, sample_key=KEY, sample_iv=IV)
    return out


def test_pipeline_demuxes_mp4_jobs_beside_ts_jobs():
    check_pipeline("cpu")


@pytest.mark.gpu
def test_pipeline_on_the_device_equals_the_cpu_pipeline(cuda):
    dev, cpu = check_pipeline(cuda), check_pipeline("cpu")
    for name in ("clear", "enc"):
        for t in ("video", "audio"):
            for k in dev[name][t].keys():
                a, b = dev[name][t][k], cpu[name][t][k]
                assert torch.equal(a.cpu(), b) if isinstance(a, torch.Tensor) else a == b, (name, t, k)
        assert dev[name]["info"] == cpu[name]["info"] and dev[name]["emsg"] == cpu[name]["emsg"]
    assert torch.equal(dev["clear"]["captions"]["bytes"].cpu(), cpu["clear"]["captions"]["bytes"])


# ---------------------------------------------------------------- the player
def play(segments, config=None, want=2, durations=(2.0, 2.0)):
    """Fragments behind one ``#EXT-X-MAP`` through a player: (events in order, errors, the origin).
    ``durations`` are what the fragments' ``trun`` boxes add up to."""
    lines = ["#EXTM3U", "#EXT-X-VERSION:7", "#EXT-X-TARGETDURATION:2", "#EXT-X-MEDIA-SEQUENCE:3",
             '#EXT-X-MAP:URI="init.mp4"']
    res = {"init.mp4": np.frombuffer(INIT, np.uint8).copy()}
    for k, seg in enumerate(segments):
        lines += [f"#EXTINF:{durations[k]},", f"s{k}.m4s"]
        res[f"s{k}.m4s"] = np.frombuffer(seg, np.uint8).copy()
    res["media.m3u8"] = "\n".join(lines + ["#EXT-X-ENDLIST", ""])
    res["master.m3u8"] = "#EXTM3U\n#EXT-X-STREAM-INF:BANDWIDTH=300000,RESOLUTION=640x360\nmedia.m3u8\n"
    origin = StaticOrigin("http://cdn.mp4/vod/", res)
    loop = new_event_loop("virtual")
    hls = Hls(dict(config or {}, transmuxDevice="cpu"))
    media_el = MediaElement()
    events, errors = [], []
    E = Hls.Events
    for name in (E.FRAG_PARSING_INIT_SEGMENT, E.FRAG_PARSING_METADATA, E.FRAG_PARSING_USERDATA, E.FRAG_PARSING_DATA,
                 E.FRAG_PARSED, E.FRAG_BUFFERED):
        hls.on(name, lambda e, d: events.append((e, d)))
    hls.on(E.ERROR, lambda e, d: errors.append(d))
    hls.loadSource("http://cdn.mp4/vod/master.m3u8")
    hls.attachMedia(media_el)
    hls.on(E.MANIFEST_PARSED, lambda e, d: media_el.play())
    assert loop.run_until(lambda: sum(e == E.FRAG_BUFFERED for e, _ in events) >= want or errors, timeout_ms=60_000)
    hls.destroy()
    return events, errors, origin


def test_player_plays_an_ext_x_map_playlist(fresh):  # noqa: F811
    events, errors, origin = play(fragments(), {"enableCEA708Captions": True})
    E = Hls.Events
    assert not errors
    assert sum(u.endswith("init.mp4") for u in origin.requests) == 1  # once per (URL, range)
    names = [e for e, _ in events]
    assert names == [E.FRAG_PARSING_INIT_SEGMENT, E.FRAG_PARSING_USERDATA, E.FRAG_PARSING_DATA, E.FRAG_PARSING_DATA,
                     E.FRAG_PARSED, E.FRAG_BUFFERED, E.FRAG_PARSING_METADATA, E.FRAG_PARSING_DATA, E.FRAG_PARSING_DATA,
                     E.FRAG_PARSED, E.FRAG_BUFFERED]
    tracks = events[0][1]["tracks"]
    assert tracks["video"]["codec"] == "avc1.64001f" and tracks["video"]["container"] == "video/mp4"
    assert tracks["audio"]["initSegment"] == INIT and tracks["audio"]["codec"] == "mp4a"
    assert events[1][1]["samples"]["n_samples"] == 5
    v, a = events[2][1], events[3][1]
    assert (v["type"], a["type"], v["data1"], v["nb"], a["nb"]) == ("video", "audio", None, 6, 3)
    assert bytes(v["data2"].numpy()) == fragments()[0] and v["frag"].sn == 3
    assert (v["startDTS"], v["endDTS"], v["startPTS"]) == (1.0, 3.0, 1.0)
    assert v["endPTS"] == pytest.approx(249000 / 90000 + 1 / 3) and (a["startDTS"], a["endDTS"]) == (1.0, 3.0)
    assert events[4][1]["independent"] is True and events[9][1]["independent"] is True
    assert [m["id"] for m in events[6][1]["samples"]] == [3] and events[6][1]["frag"].sn == 4


def test_a_damaged_fragment_is_a_parsing_error(fresh):  # noqa: F811
    good = fragments()[0]
    _, errors, _ = play([good[:len(good) - 40]], {"fragLoadingMaxRetry": 0}, want=1)  # the mdat runs off the segment
    assert errors and errors[0]["details"] == Hls.ErrorDetails.FRAG_PARSING_ERROR and "fMP4" in errors[0]["reason"]
    _, errors, origin = play([good], {"fragLoadingMaxRetry": 0}, want=1)
    assert not errors


def test_a_bad_init_segment_is_a_parsing_error(fresh, monkeypatch):  # noqa: F811
    monkeypatch.setattr("test_mp4_pipeline.INIT", INIT[:60])
    _, errors, _ = play(fragments()[:1], {"fragLoadingMaxRetry": 0}, want=1)
    assert errors and errors[0]["details"] == Hls.ErrorDetails.FRAG_PARSING_ERROR
    assert "init segment" in errors[0]["reason"]
