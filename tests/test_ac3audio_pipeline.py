"""MPEG-TS fragments with an AC-3 or E-AC-3 track through the transmux pipeline (``remux`` /
``fragment`` jobs beside ADTS, MP3 and fragmented-MP4 jobs in one batch) and through a player on a TS
playlist under ``remuxFmp4``: the audio fragment is ``moof`` + ``mdat`` whose samples are the muxed
syncframes byte for byte, its ``tfdt`` the first audio stamp in units of the sample rate, the init
segment announces ``ac-3`` with its ``dac3``, and the data event carries the frames.  The TS comes
from the small muxer of ``mpegaudio_cases.py``."""
import numpy as np
import pytest
import torch

import ac3audio_cases as ac
import mp4_cases
import mpegaudio_cases as mc
import remux_cases as rc
from hlsjs_p2p_wrapper_amd.net import new_event_loop
from hlsjs_p2p_wrapper_amd.net.origin import StaticOrigin
from hlsjs_p2p_wrapper_amd.ops import tsdemux
from hlsjs_p2p_wrapper_amd.player import Hls, MediaElement, fmp4
from hlsjs_p2p_wrapper_amd.player.mp4init import parse_init
from hlsjs_p2p_wrapper_amd.player.transmux import MediaPipeline, TransmuxJob
from test_esindex import fresh  # noqa: F401  (fixture)

SURROUND = dict(fscod=0, code=28, acmod=7, lfeon=1)  # 384 kbit/s at 48 kHz, 3/2 + LFE: 1536-byte frames


def run(device, jobs):
    p = MediaPipeline(torch.device(device))
    p.auto_flush = False
    for j in jobs:
        p.submit(j)
    p.complete(p.launch())
    return p


def check_pipeline(device):
    dolby, frames, first = ac.ac3_ts(0, **SURROUND)
    edolby, eframes, efirst = ac.ac3_ts(1, video=False, eac3=True, fscod=1, acmod=2)  # E-AC-3 at 44.1 kHz, audio only
    mp3, mframes, _ = mc.mp3_ts(2)
    adts, _ = tsdemux.mux_segment(target_bytes=40 * 188, seed=5)
    init = parse_init(mp4_cases.init_segment([(1, b"vide", b"avc1"), (2, b"soun", b"mp4a")]))
    m4s = mp4_cases.case_captions(duration=30000, audio_duration=32000)[0][0]
    out = {}
    put = lambda name: (lambda r: out.__setitem__(name, r))  # noqa: E731
    run(device, [TransmuxJob(dolby, None, None, put("ac3"), fragment=True, sequence_number=7),
                 TransmuxJob(adts, None, None, put("adts"), fragment=True, sequence_number=8),
                 TransmuxJob(edolby, None, None, put("eac3"), remux=True),
                 TransmuxJob(mp3, None, None, put("mp3"), fragment=True, sequence_number=9),
                 TransmuxJob(m4s, None, None, put("mp4"), mp4=init),
                 TransmuxJob(dolby, None, None, put("plain"))])
    for name in ("ac3", "adts", "eac3", "mp3", "mp4", "plain"):
        assert "error" not in out[name] and out[name]["status"] == 0, name
    assert "fmp4" not in out["plain"] and out["plain"]["info"]["audio_type"] == 0x81
    surround = dict(sample_rate=48000, channels=6, kind=1, acmod=7, lfeon=1, bit_rate_code=14, bitrate=384000)
    stereo = dict(sample_rate=44100, channels=2, kind=2, acmod=2, lfeon=0, bsid=16)
    for name, fr, stamp, want in (("ac3", frames, first, surround), ("eac3", eframes, efirst, stereo)):
        f = out[name]["fmp4"]
        m, a = f["ac3_audio"], f["audio"]
        assert "ac3_audio" in f.keys()
        assert m["status"] == 0 and m["n_frames"] == len(fr) and m["frame_samples"] == 1536
        assert {k: m[k] for k in want} == want and m["first_frame_bytes"] == len(fr[0])
        with pytest.raises(TypeError):
            m["status"] = 1
        assert f["mpeg_audio"]["status"] == 1  # the MPEG audio op's own row: not MPEG audio
        assert a["nb"] == len(fr) and bytes(a["mdat"].cpu().numpy())[8:] == b"".join(fr)
        assert (a["timescale"], a["samplerate"], a["channelCount"]) == (want["sample_rate"],) * 2 + (want["channels"],)
        assert a["duration"] == 1536 * len(fr)
        assert a["base"] == fmp4.audio_base(stamp, want["sample_rate"])
        assert a["codec"] == ("ac-3" if want["kind"] == 1 else "ec-3") and a["container"] == "audio/mp4"
        assert a["init"] == fmp4.ac3_audio_init(m) and (b"dac3" if want["kind"] == 1 else b"dec3") in a["init"]
        moof = rc.parse_moof(a["moof"](3))
        assert moof["default_duration"] == 1536
        assert [s["size"] for s in moof["samples"]] == [len(x) for x in fr]
        assert f["audio_payload_bytes"] == sum(map(len, fr)) and f["n_aframes"] == len(fr)
        assert out[name]["info"]["audio_type"] == (0x81 if want["kind"] == 1 else 0x87)
    assert b"\x10\x3D\xC0" in out["ac3"]["fmp4"]["audio"]["init"]  # the dac3 of the issue's vector
    # the fragment view: moof + mdat in one range, the samples the muxed frames, tfdt in units of the rate
    a = out["ac3"]["fmp4"]["audio"]
    frag = bytes(a["fragment"].cpu().numpy())
    n = len(bytes(a["moof_view"].cpu().numpy()))
    moof = rc.parse_moof(frag[:n])
    assert frag[n + 4:n + 8] == b"mdat" and frag[n + 8:] == b"".join(frames) and moof["sequence_number"] == 7
    assert moof["data_offset"] == n + 8 and moof["default_duration"] == 1536 and moof["count"] == len(frames)
    base = out["ac3"]["fmp4"]["time_base"]
    assert a["tfdt"] == moof["base"] == ((first - base) * 48000 + 45000) // 90000
    assert frag[:n] == fmp4.audio_moof(7, first - base, 48000, a["samples"].cpu().numpy(), frame_samples=1536)
    assert out["ac3"]["fmp4"]["video"]["nb"] == 5
    # the jobs whose audio is not Dolby audio keep what they had
    assert out["mp4"]["container"] == "mp4" and "fmp4" not in out["mp4"]
    f = out["adts"]["fmp4"]
    assert f["ac3_audio"]["status"] == 1 and "ac3_audio" not in f.keys()
    assert all(f["ac3_audio"][k] == 0 for k in ("n_frames", "frame_samples", "kind"))
    a = f["audio"]
    assert a["nb"] > 0 and a["duration"] == 1024 * a["nb"] and a["codec"].startswith("mp4a.40.")
    assert rc.parse_moof(bytes(a["moof_view"].cpu().numpy()))["default_duration"] == 1024
    f = out["mp3"]["fmp4"]
    assert f["ac3_audio"]["status"] == 1 and f["mpeg_audio"]["status"] == 0 and f["audio"]["codec"] == "mp4a.6b"
    assert bytes(f["audio"]["mdat"].cpu().numpy())[8:] == b"".join(mframes)
    assert rc.parse_moof(bytes(f["audio"]["moof_view"].cpu().numpy()))["default_duration"] == 1152
    return out


def test_pipeline_remuxes_dolby_tracks_beside_adts_mp3_and_mp4_jobs():
    check_pipeline("cpu")


@pytest.mark.gpu
def test_pipeline_on_the_device_equals_the_cpu_pipeline(cuda):
    dev, cpu = check_pipeline(cuda), check_pipeline("cpu")
    for name in ("ac3", "eac3", "adts", "mp3"):
        d, c = dev[name]["fmp4"], cpu[name]["fmp4"]
        assert dict(d["ac3_audio"]) == dict(c["ac3_audio"]) and dict(d["mpeg_audio"]) == dict(c["mpeg_audio"]), name
        for k in ("nb", "base", "duration", "timescale", "codec", "init", "channelCount", "samplerate"):
            assert d["audio"][k] == c["audio"][k], (name, k)
        assert d["audio"]["mdat"].is_cuda and torch.equal(d["audio"]["mdat"].cpu(), c["audio"]["mdat"])
        assert torch.equal(d["audio"]["samples"].cpu(), c["audio"]["samples"])
        assert d["audio"]["moof"](5) == c["audio"]["moof"](5)
    for name in ("ac3", "adts", "mp3"):
        assert torch.equal(dev[name]["fmp4"]["audio"]["fragment"].cpu(), cpu[name]["fmp4"]["audio"]["fragment"])
        assert torch.equal(dev[name]["fmp4"]["video"]["fragment"].cpu(), cpu[name]["fmp4"]["video"]["fragment"])


# ---------------------------------------------------------------- the player
def play(segments, config=None, want=2):
    """TS fragments through a player: (events in order, errors)."""
    data = lambda b: np.frombuffer(bytes(b), np.uint8).copy()  # noqa: E731
    lines = ["#EXTM3U", "#EXT-X-VERSION:3", "#EXT-X-TARGETDURATION:2", "#EXT-X-MEDIA-SEQUENCE:3"]
    res = {}
    for k, seg in enumerate(segments):
        lines += ["#EXTINF:2.0,", f"s{k}.ts"]
        res[f"s{k}.ts"] = data(seg)
    res["media.m3u8"] = "\n".join(lines + ["#EXT-X-ENDLIST", ""])
    res["master.m3u8"] = '#EXTM3U\n#EXT-X-STREAM-INF:BANDWIDTH=712000,CODECS="avc1.42c01e,ac-3"\nmedia.m3u8\n'
    StaticOrigin("http://cdn.ac3/vod/", res)
    loop = new_event_loop("virtual")
    hls = Hls(dict(config or {}, transmuxDevice="cpu"))
    media_el = MediaElement()
    events, errors = [], []
    E = Hls.Events
    for name in (E.FRAG_PARSING_INIT_SEGMENT, E.FRAG_PARSING_DATA, E.FRAG_PARSED, E.FRAG_BUFFERED):
        hls.on(name, lambda e, d: events.append((e, d)))
    hls.on(E.ERROR, lambda e, d: errors.append(d))
    hls.loadSource("http://cdn.ac3/vod/master.m3u8")
    hls.attachMedia(media_el)
    hls.on(E.MANIFEST_PARSED, lambda e, d: media_el.play())
    fatal = lambda: any(d.get("fatal") for d in errors)  # noqa: E731
    assert loop.run_until(lambda: sum(e == E.FRAG_BUFFERED for e, _ in events) >= want or fatal(), timeout_ms=120_000)
    hls.destroy()
    return events, errors


def two_seconds(k: int, **kw):
    """Segment ``k`` of a playlist of two-second segments: 63 frames of 1,536 samples at 48,000 Hz."""
    return ac.ac3_ts(k, n_pes=21, per_pes=3, spacing=180000, **kw)


def test_player_plays_a_ts_playlist_with_an_ac3_track(fresh):  # noqa: F811
    segs = [two_seconds(0, **SURROUND), two_seconds(1, **SURROUND)]
    events, errors = play([s for s, _, _ in segs], {"remuxFmp4": True})
    assert not errors
    E = Hls.Events
    inits = [d for e, d in events if e == E.FRAG_PARSING_INIT_SEGMENT]
    assert len(inits) == 1  # the second fragment has the same (kind, rate, acmod, lfeon)
    audio = inits[0]["tracks"]["audio"]
    assert audio["type"] == 0x81 and audio["codec"] == "ac-3" and audio["container"] == "audio/mp4"
    assert b"dac3\x10\x3D\xC0" in audio["initSegment"] and audio["metadata"] == {"channelCount": 6}
    adata = [d for e, d in events if e == E.FRAG_PARSING_DATA and d["type"] == "audio"]
    assert len(adata) == 2
    for d, (_, frames, first) in zip(adata, segs):
        assert d["nb"] == len(frames) > 0 and bytes(d["data2"].numpy())[8:] == b"".join(frames)
        moof = rc.parse_moof(d["data1"])
        assert moof["default_duration"] == 1536 and moof["count"] == d["nb"] and moof["sequence_number"] == d["frag"].sn
        assert d["startDTS"] == pytest.approx(first / 90000, abs=1e-4)
        assert d["endDTS"] - d["startDTS"] == pytest.approx(1536 * len(frames) / 48000, abs=1e-6)


def test_player_announces_again_when_the_channels_change(fresh):  # noqa: F811
    segs = [two_seconds(0, **SURROUND), two_seconds(1, fscod=0, code=28, acmod=2, lfeon=0)]
    events, errors = play([s for s, _, _ in segs], {"remuxFmp4": True})
    assert not errors
    inits = [d["tracks"]["audio"] for e, d in events if e == Hls.Events.FRAG_PARSING_INIT_SEGMENT]
    assert [t["metadata"]["channelCount"] for t in inits] == [6, 2] and all(t["codec"] == "ac-3" for t in inits)
    assert all(t["type"] == 0x81 for t in inits) and inits[0]["initSegment"] != inits[1]["initSegment"]


def test_player_announces_an_eac3_track(fresh):  # noqa: F811
    events, errors = play([two_seconds(0, eac3=True, acmod=7, lfeon=1)[0]], {"remuxFmp4": True}, want=1)
    assert not errors
    audio = next(d for e, d in events if e == Hls.Events.FRAG_PARSING_INIT_SEGMENT)["tracks"]["audio"]
    assert audio["type"] == 0x87 and audio["codec"] == "ec-3" and b"dec3" in audio["initSegment"]
    assert audio["metadata"] == {"channelCount": 6}


def test_player_without_the_remux_emits_the_audio_es(fresh):  # noqa: F811
    events, errors = play([two_seconds(0, **SURROUND)[0]], want=1)
    assert not errors
    init = next(d for e, d in events if e == Hls.Events.FRAG_PARSING_INIT_SEGMENT)
    assert init["tracks"]["audio"] == {"pid": mc.AUDIO_PID, "type": 0x81}
    a = next(d for e, d in events if e == Hls.Events.FRAG_PARSING_DATA and d["type"] == "audio")
    assert a["nb"] == 21 and "data2" not in a
