"""Packed-audio fragments through the transmux pipeline (``TransmuxJob(packed_audio=True)``) and
through a player on an ``.aac`` playlist: clear and AES-128 jobs beside an MPEG-TS and a
fragmented-MP4 job in one batch, the result mapping with ``remux`` and ``fragment``, the parsing
events of the TS branch, the key loaded once, a segment without a timestamp as
``FRAG_PARSING_ERROR``, and the ``packedAudio`` config key."""
import numpy as np
import pytest
import torch

import mp4_cases as mc
import packedaudio_cases as pc
from hlsjs_p2p_wrapper_amd.net import new_event_loop
from hlsjs_p2p_wrapper_amd.net.origin import StaticOrigin
from hlsjs_p2p_wrapper_amd.ops import aes, tsdemux
from hlsjs_p2p_wrapper_amd.player import Hls, MediaElement
from hlsjs_p2p_wrapper_amd.player.mp4init import parse_init
from hlsjs_p2p_wrapper_amd.player.transmux import MediaPipeline, TransmuxJob
from test_esindex import fresh  # noqa: F401  (fixture)

KEY, IV = bytes(range(16)), bytes(range(16, 32))
RATE_INDEX, RATE = 3, 48000


def segment(k: int, count: int = 10, stamp=None):
    """Packed-audio segment ``k``: its frames, its stamp and its bytes (one tag with a TIT2 in front of the PRIV)."""
    f = pc.frames(count, 60 + k, rate_index=RATE_INDEX, channels=2, lo=1, hi=300)
    ts = pc.TS0 + k * 180000 if stamp is None else stamp
    return f, ts, pc.tag(pc.text_frame(12) + pc.priv(ts)) + b"".join(f)


def run(device, jobs):
    p = MediaPipeline(torch.device(device))
    p.auto_flush = False
    for j in jobs:
        p.submit(j)
    p.complete(p.launch())
    return p


def check_pipeline(device):
    (f0, ts0, s0), (f1, ts1, s1) = segment(0), segment(1, 7)
    ts, _ = tsdemux.mux_segment(target_bytes=40 * 188, seed=5)
    init = parse_init(mc.init_segment([(1, b"vide", b"avc1"), (2, b"soun", b"mp4a")]))
    m4s = mc.case_captions(duration=30000, audio_duration=32000)[0][0]
    cipher = bytes(aes.cbc_encrypt(KEY, IV, np.frombuffer(s1, np.uint8)))  # (pads by PKCS#7)
    out = {}
    put = lambda name: (lambda r: out.__setitem__(name, r))  # noqa: E731
    run(device, [TransmuxJob(s0, None, None, put("clear"), packed_audio=True, fragment=True, sequence_number=9),
                 TransmuxJob(ts, None, None, put("ts")),
                 TransmuxJob(cipher, KEY, IV, put("enc"), packed_audio=True, remux=True),
                 TransmuxJob(m4s, None, None, put("mp4"), mp4=init),
                 TransmuxJob(cipher[:-3], KEY, IV, put("odd"), packed_audio=True),
                 TransmuxJob(s0[len(s0) - sum(map(len, f0)):], None, None, put("bare"), packed_audio=True, index=True),
                 TransmuxJob(s1, None, None, put("plain"), packed_audio=True)])
    assert "container" not in out["ts"] and out["ts"]["status"] == 0 and out["ts"]["info"]["n_packets"] > 0
    assert out["mp4"]["container"] == "mp4" and out["mp4"]["status"] == 0
    c, e = out["clear"], out["enc"]
    assert c["container"] == e["container"] == "aac" and c["status"] == e["status"] == 0
    assert "error" not in c and "error" not in e
    assert c["plain_bytes"] == len(s0) and e["plain_bytes"] == len(s1)
    T = len(s0) - sum(map(len, f0))
    pa = c["packed_audio"]
    assert dict(pa) == {"status": 0, "id3_bytes": T, "n_tags": 1, "timestamp": ts0, "n_frames": 10,
                        "stop_offset": len(s0), "sample_rate": RATE, "channels": 2}
    with pytest.raises(TypeError):
        pa["status"] = 1
    assert e["packed_audio"]["timestamp"] == ts1 and e["packed_audio"]["n_frames"] == 7
    info = c["info"]
    assert (info["audio_type"], info["n_audio_pes"], info["audio_first_pts"], info["video_type"]) == (0x0F, 3, ts0, 0)
    assert info["audio_last_pts"] == ts0 + 2 * 7680 and info["id3_first_pts"] == ts0
    assert bytes(c["audio"].cpu().numpy()) == b"".join(f0) and bytes(c["id3"].cpu().numpy()) == s0[:T]
    assert c["video"].numel() == 0 and bytes(e["audio"].cpu().numpy()) == b"".join(f1)
    assert c["demux"].pes[c["index"], 1, :3, 1].tolist() == [ts0, ts0 + 7680, ts0 + 15360]
    # remux / fragment over the views
    for r, f, stamp in ((c, f0, ts0), (e, f1, ts1)):
        a = r["fmp4"]["audio"]
        bodies = b"".join(x[7 if x[1] & 1 else 9:] for x in f)
        assert a["nb"] == len(f) and bytes(a["mdat"].cpu().numpy())[8:] == bodies
        assert a["init"] is not None and a["codec"] == "mp4a.40.2" and a["timescale"] == RATE
        assert r["fmp4"]["audio_base_pts"] == stamp and r["fmp4"]["video"]["nb"] == 0
        assert r["samples"]["n_adts_frames"] == len(f) and r["samples"]["audio_sample_rate"] == RATE
    frag = bytes(c["fmp4"]["audio"]["fragment"].cpu().numpy())
    assert frag[4:8] == b"moof" and frag[20:24] == (9).to_bytes(4, "big") and frag.endswith(bodies_of(f0))
    assert "fragment" not in e["fmp4"]["audio"] and "time_base" in c["fmp4"] and "time_base" not in e["fmp4"]
    assert "fmp4" not in out["plain"] and "samples" not in out["plain"] and out["plain"]["status"] == 0
    # errors
    assert isinstance(out["odd"]["error"], ValueError) and out["odd"]["container"] == "aac"
    b = out["bare"]
    assert "no_timestamp" in str(b["error"]) and b["packed_audio"]["n_frames"] == 10
    assert b["samples"]["n_adts_frames"] == 10
    with pytest.raises(ValueError, match="SAMPLE-AES"):
        TransmuxJob(s0, None, None, print, packed_audio=True, sample_key=KEY, sample_iv=IV)
    with pytest.raises(ValueError, match="not both"):
        TransmuxJob(s0, None, None, print, packed_audio=True, mp4=init)
    return out


def bodies_of(f):
    return b"".join(x[7 if x[1] & 1 else 9:] for x in f)


def test_pipeline_demuxes_packed_audio_jobs_beside_ts_and_mp4_jobs():
    check_pipeline("cpu")


def test_a_batch_of_packed_jobs_alone_and_a_failed_stage():
    out = []
    p = run("cpu", [TransmuxJob(segment(2)[2], None, None, out.append, packed_audio=True)])
    assert out[0]["container"] == "aac" and "error" not in out[0] and p.segments == 1
    out.clear()
    run("cpu", [TransmuxJob(3.5, None, None, out.append, packed_audio=True)])  # no payload type: the stage fails
    assert isinstance(out[0]["error"], TypeError) and out[0]["container"] == "aac"


@pytest.mark.gpu
def test_pipeline_on_the_device_equals_the_cpu_pipeline(cuda):
    dev, cpu = check_pipeline(cuda), check_pipeline("cpu")
    for name in ("clear", "enc", "plain", "bare"):
        d, c = dev[name], cpu[name]
        assert d["info"].to_dict() == c["info"].to_dict() and dict(d["packed_audio"]) == dict(c["packed_audio"])
        assert d["audio"].is_cuda and torch.equal(d["audio"].cpu(), c["audio"])
        assert torch.equal(d["id3"].cpu(), c["id3"])
    for name in ("clear", "enc"):
        for k in ("nb", "base", "duration", "timescale", "codec", "init"):
            assert dev[name]["fmp4"]["audio"][k] == cpu[name]["fmp4"]["audio"][k], (name, k)
        assert torch.equal(dev[name]["fmp4"]["audio"]["mdat"].cpu(), cpu[name]["fmp4"]["audio"]["mdat"])
        assert torch.equal(dev[name]["samples"]["aframes"].cpu(), cpu[name]["samples"]["aframes"])
    assert torch.equal(dev["clear"]["fmp4"]["audio"]["fragment"].cpu(), cpu["clear"]["fmp4"]["audio"]["fragment"])


# ---------------------------------------------------------------- the player
def play(segments, config=None, want=2, suffix=".aac", key=False):
    """Packed-audio fragments through a player: (events in order, errors, the origin)."""
    data = lambda b: np.frombuffer(bytes(b), np.uint8).copy()  # noqa: E731
    lines = ["#EXTM3U", "#EXT-X-VERSION:3", "#EXT-X-TARGETDURATION:2", "#EXT-X-MEDIA-SEQUENCE:3"]
    res = {}
    if key:
        lines.append(f'#EXT-X-KEY:METHOD=AES-128,URI="key.bin",IV=0x{IV.hex()}')
        res["key.bin"] = data(KEY)
    for k, seg in enumerate(segments):
        lines += ["#EXTINF:2.0,", f"a{k}{suffix}?token=x.ts"]
        res[f"a{k}{suffix}?token=x.ts"] = data(aes.cbc_encrypt(KEY, IV, data(seg)) if key else seg)
    res["media.m3u8"] = "\n".join(lines + ["#EXT-X-ENDLIST", ""])
    res["master.m3u8"] = '#EXTM3U\n#EXT-X-STREAM-INF:BANDWIDTH=128000,CODECS="mp4a.40.2"\nmedia.m3u8\n'
    origin = StaticOrigin("http://cdn.aac/vod/", res)
    loop = new_event_loop("virtual")
    hls = Hls(dict(config or {}, transmuxDevice="cpu"))
    media_el = MediaElement()
    events, errors = [], []
    E = Hls.Events
    for name in (E.FRAG_PARSING_INIT_SEGMENT, E.FRAG_PARSING_METADATA, E.FRAG_PARSING_USERDATA, E.FRAG_PARSING_DATA,
                 E.FRAG_PARSED, E.FRAG_BUFFERED):
        hls.on(name, lambda e, d: events.append((e, d)))
    hls.on(E.ERROR, lambda e, d: errors.append(d))
    hls.loadSource("http://cdn.aac/vod/master.m3u8")
    hls.attachMedia(media_el)
    hls.on(E.MANIFEST_PARSED, lambda e, d: media_el.play())
    fatal = lambda: any(d.get("fatal") for d in errors)  # noqa: E731
    assert loop.run_until(lambda: sum(e == E.FRAG_BUFFERED for e, _ in events) >= want or fatal(), timeout_ms=120_000)
    hls.destroy()
    return events, errors, origin


def check_events(events, segs):
    E = Hls.Events
    names = [e for e, _ in events]
    per = [E.FRAG_PARSING_METADATA, E.FRAG_PARSING_DATA, E.FRAG_PARSING_DATA, E.FRAG_PARSED, E.FRAG_BUFFERED]
    assert names == [E.FRAG_PARSING_INIT_SEGMENT] + per + per
    tracks = events[0][1]["tracks"]
    assert tracks["audio"]["type"] == 0x0F and tracks["video"]["type"] == 0 and tracks["audio"]["pid"] == -1
    for n, (f, stamp, s) in enumerate(segs):
        meta, v, a = (events[1 + 5 * n + j][1] for j in range(3))
        T = len(s) - sum(map(len, f))
        assert bytes(meta["samples"].numpy()) == s[:T] and meta["frag"].sn == 3 + n
        assert (v["type"], a["type"], v["nb"], a["nb"]) == ("video", "audio", 0, 3)
        assert bytes(a["data1"].numpy()) == b"".join(f) and v["data1"].numel() == 0
        assert a["pts"] == (stamp, stamp + 2 * 7680) and (a["startPTS"], a["endPTS"]) == (2.0 * n, 2.0 * n + 2.0)
    return tracks


def test_player_plays_an_aac_playlist(fresh):  # noqa: F811
    segs = [segment(0), segment(1)]
    events, errors, _ = play([s for _, _, s in segs])
    assert not errors
    tracks = check_events(events, segs)
    assert "initSegment" not in tracks["audio"]


def test_player_plays_an_aes_128_aac_playlist_under_remux(fresh):  # noqa: F811
    segs = [segment(0), segment(1)]
    events, errors, origin = play([s for _, _, s in segs], {"remuxFmp4": True}, key=True)
    assert not errors and origin.requests.count("key.bin") == 1
    E = Hls.Events
    assert [e for e, _ in events][:4] == [E.FRAG_PARSING_INIT_SEGMENT, E.FRAG_PARSING_METADATA, E.FRAG_PARSING_DATA,
                                          E.FRAG_PARSING_DATA]
    audio = events[0][1]["tracks"]["audio"]
    assert audio["type"] == 0x0F and audio["codec"] == "mp4a.40.2" and audio["container"] == "audio/mp4"
    assert b"esds" in audio["initSegment"] and audio["metadata"] == {"channelCount": 2}
    assert "initSegment" not in events[0][1]["tracks"]["video"]
    a = events[3][1]
    assert a["nb"] == 10 and bytes(a["data2"].numpy())[8:] == bodies_of(segs[0][0]) and a["data1"][4:8] == b"moof"
    assert a["startDTS"] == pytest.approx(segs[0][1] / 90000, abs=1e-4) and a["samples"]["n_adts_frames"] == 10
    assert bytes(events[1][1]["samples"].numpy()) == segs[0][2][:len(segs[0][2]) - sum(map(len, segs[0][0]))]


def test_a_segment_without_a_timestamp_is_a_parsing_error_under_the_retry_rule(fresh):  # noqa: F811
    f, _, s = segment(0)
    bare = pc.tag(pc.text_frame(12)) + b"".join(f)
    events, errors, origin = play([bare], {"fragLoadingMaxRetry": 1, "fragLoadingRetryDelay": 10}, want=1)
    assert [d["details"] for d in errors] == [Hls.ErrorDetails.FRAG_PARSING_ERROR] * 2
    assert [d["fatal"] for d in errors] == [False, True] and "no_timestamp" in errors[0]["reason"]
    assert sum(u.startswith("a0.aac") for u in origin.requests) == 2 and not events


def test_packed_audio_false_gives_the_ts_demux_error(fresh):  # noqa: F811
    _, _, s = segment(0)
    events, errors, _ = play([s], {"packedAudio": False, "fragLoadingMaxRetry": 0}, want=1)
    assert errors and errors[0]["details"] == Hls.ErrorDetails.FRAG_PARSING_ERROR and errors[0]["fatal"]
    assert "packed" not in errors[0]["reason"] and not events


def test_packed_audio_true_takes_any_url_and_auto_only_aac(fresh):  # noqa: F811
    segs = [segment(0), segment(1)]
    events, errors, _ = play([s for _, _, s in segs], {"packedAudio": True}, suffix=".bin")
    assert not errors
    check_events(events, segs)
    _, errors, _ = play([segs[0][2]], {"fragLoadingMaxRetry": 0}, want=1, suffix=".bin")  # auto: not packed audio
    assert errors and errors[0]["details"] == Hls.ErrorDetails.FRAG_PARSING_ERROR
    events, errors, _ = play([s for _, _, s in segs], suffix=".AAC")
    assert not errors and len(events) == 11
