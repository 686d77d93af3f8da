"""``cbcs``-protected fragmented-MP4 fragments through the transmux pipeline
(``TransmuxJob(mp4=init, sample_key=...)``) and through a player on a ``METHOD=SAMPLE-AES``
``#EXT-X-MAP`` playlist: a cbcs job beside a clear fMP4 job and a TS job in one batch, the result
mapping, the device pipeline against the CPU pipeline, ``clear_data`` and the codec string, the
event sequence, the buffered bytes against the clear twin, and ``FRAG_DECRYPT_ERROR`` for a fragment
whose ``senc`` was removed."""
import numpy as np
import pytest
import torch

import cbcs_cases as cc
import mp4_cases as mc
from hlsjs_p2p_wrapper_amd.net import new_event_loop
from hlsjs_p2p_wrapper_amd.net.origin import StaticOrigin
from hlsjs_p2p_wrapper_amd.ops import tsdemux
from hlsjs_p2p_wrapper_amd.ops.cbcs import CINFO
from hlsjs_p2p_wrapper_amd.player import Hls, MediaElement
from hlsjs_p2p_wrapper_amd.player.mp4init import parse_init
from hlsjs_p2p_wrapper_amd.player.transmux import MediaPipeline, TransmuxJob
from test_esindex import fresh  # noqa: F401  (fixture)
from test_mp4_pipeline import fragments

KEY, IV = cc.key_of(5), cc.iv_of(9)
# video 1:9 with the constant IV of cbcs_cases.tenc(), audio 0:0 with one of its own
INIT = cc.cbcs_init()
CLEAR_INIT = mc.init_segment([(1, b"vide", b"avc1"), (2, b"soun", b"mp4a")])


def twins(senc="after"):
    """Two fragments of two seconds each, (clear twin, protected) each: six caption-bearing video
    samples with a subsample per NAL unit and three audio samples, then three and three."""
    out = []
    for k, (t0, a0, count) in enumerate(((90000, 48000, 6), (270000, 144000, 3))):
        if k == 0:
            src = mc.case_captions(duration=30000, audio_duration=32000)[0][0]
            init = parse_init(CLEAR_INIT)
            from hlsjs_p2p_wrapper_amd.ops import mp4demux
            raw, offs, lens = mc.layout([src])
            md = mp4demux.mp4_demux_batch(torch.from_numpy(np.frombuffer(raw, np.uint8).copy()), offs, lens, init)
            v = [raw[offs[0] + int(md.pes[0, 0, a, 0]):][:int(md.msamples[0, 0, a, 0])] for a in range(count)]
            nal, au = md.nal[0].numpy(), md.au[0].numpy()
            subs = [[(5, int(nal[j, 1]) - 1) for j in range(au[a, 0], au[a, 0] + au[a, 1])] for a in range(count)]
        else:
            v = mc.video_samples(count)
            subs = [[(5, len(s) - 5)] for s in v]  # (the first NAL only: what is left over is clear)
        audio = [cc.blob(40 + j, j) for j in range(3)]
        out.append(cc.protect([cc.Traf(1, t0, v, (1, 9), subs, duration=180000 // count, senc=senc),
                               cc.Traf(2, a0, audio, (0, 0), None, duration=32000, senc=senc)], KEY, IV, seq=k + 1)[:2])
    return out


def run(device, jobs):
    p = MediaPipeline(torch.device(device))
    p.auto_flush = False
    for j in jobs:
        p.submit(j)
    p.complete(p.launch())


def check_pipeline(device):
    init, clear_init = parse_init(INIT), parse_init(CLEAR_INIT)
    (clear, prot), _ = twins()
    ts, _ = tsdemux.mux_segment(target_bytes=40 * 188, seed=5)
    out = {}
    run(device, [TransmuxJob(prot, None, None, lambda r: out.__setitem__("cbcs", r), mp4=init, captions=True,
                             sample_key=KEY, sample_iv=IV),
                 TransmuxJob(fragments()[0], None, None, lambda r: out.__setitem__("clear", r), mp4=clear_init,
                             captions=True),
                 TransmuxJob(ts, None, None, lambda r: out.__setitem__("ts", r)),
                 TransmuxJob(prot, None, None, lambda r: out.__setitem__("raw", r), mp4=init)])
    assert out["ts"]["status"] == 0 and not any("cbcs" in out[k] for k in ("ts", "clear", "raw"))
    r = out["cbcs"]
    assert r["container"] == "mp4" and r["status"] == 0 and r["init"] is init and r["plain_bytes"] == len(prot)
    assert bytes(r["data"].cpu().numpy()) == clear and bytes(out["raw"]["data"].cpu().numpy()) == prot
    # of a video sample's NAL units only the SEI is long enough for a cipher block, and sample 3 has none
    assert dict(r["cbcs"]) == {"status": 0, "n_ranges": 5 + 3, "video_samples": 5, "audio_samples": 3,
                               "video_blocks": r["cbcs"]["video_blocks"], "audio_blocks": 2 + 2 + 2, "n_senc": 2}
    assert set(r["cbcs"]) == set(CINFO) and r["cbcs"]["video_blocks"] >= 5
    with pytest.raises(TypeError):
        r["cbcs"]["status"] = 1  # read-only
    assert r["video"]["nb"] == 6 and r["audio"]["nb"] == 3 and r["video"]["codec"] == "avc1.64001f"
    # the caption bytes come out of the decrypted copy: those of the clear job beside it, which the
    # job that did not ask for the decrypt does not give
    assert r["captions"]["n_samples"] == 5 and r["samples"]["n_nal"] == 17
    assert torch.equal(r["captions"]["bytes"].cpu(), out["clear"]["captions"]["bytes"].cpu())
    assert bytes(out["clear"]["data"].cpu().numpy()) == fragments()[0]
    with pytest.raises(ValueError, match=r"SAMPLE-AES \(cbcs\) fragmented MP4 is not supported"):
        TransmuxJob(prot, None, None, print, mp4=clear_init, sample_key=KEY, sample_iv=IV)
    with pytest.raises(ValueError, match="not both"):
        TransmuxJob(prot, KEY, IV, print, mp4=init, sample_key=KEY, sample_iv=IV)
    return out


def test_pipeline_decrypts_cbcs_jobs_beside_clear_mp4_and_ts_jobs():
    check_pipeline("cpu")


@pytest.mark.gpu
def test_pipeline_on_the_device_equals_the_cpu_pipeline(cuda):
    dev, cpu = check_pipeline(cuda), check_pipeline("cpu")
    for name in ("cbcs", "clear", "raw"):
        for t in ("video", "audio"):
            for k in dev[name][t].keys():
                a, b = dev[name][t][k], cpu[name][t][k]
                assert torch.equal(a.cpu(), b) if isinstance(a, torch.Tensor) else a == b, (name, t, k)
        assert dev[name]["info"] == cpu[name]["info"] and torch.equal(dev[name]["data"].cpu(), cpu[name]["data"])
    assert dict(dev["cbcs"]["cbcs"]) == dict(cpu["cbcs"]["cbcs"])
    assert torch.equal(dev["cbcs"]["captions"]["bytes"].cpu(), cpu["cbcs"]["captions"]["bytes"])


def test_clear_data_and_the_codec_string():
    init = parse_init(INIT)
    assert (init.video_codec, init.audio_codec) == ("avc1.64001f", "mp4a") and init.data == INIT
    assert len(init.clear_data) == len(INIT) and init.clear_data != INIT
    again = parse_init(init.clear_data)  # a consumer sees plain avc1 / mp4a entries and two free boxes
    assert again.video.protection is None and again.audio.protection is None and again.clear_data is again.data
    assert (again.video_codec, again.audio_codec) == ("avc1.64001f", "mp4a")
    assert again.video == parse_init(CLEAR_INIT).video and init.clear_data.count(b"free") == 2
    assert b"sinf" not in init.clear_data and b"encv" not in init.clear_data and b"enca" not in init.clear_data


# ---------------------------------------------------------------- the player
def play(segments, config=None, want=2, init=INIT):
    lines = ["#EXTM3U", "#EXT-X-VERSION:7", "#EXT-X-TARGETDURATION:2", "#EXT-X-MEDIA-SEQUENCE:3",
             '#EXT-X-MAP:URI="init.mp4"', f'#EXT-X-KEY:METHOD=SAMPLE-AES,URI="key.bin",IV=0x{IV.hex()}']
    data = lambda b: np.frombuffer(b, np.uint8).copy()  # noqa: E731
    res = {"init.mp4": data(init), "key.bin": data(KEY)}
    for k, seg in enumerate(segments):
        lines += ["#EXTINF:2.0,", f"s{k}.m4s"]
        res[f"s{k}.m4s"] = data(seg)
    res["media.m3u8"] = "\n".join(lines + ["#EXT-X-ENDLIST", ""])
    res["master.m3u8"] = "#EXTM3U\n#EXT-X-STREAM-INF:BANDWIDTH=300000,RESOLUTION=640x360\nmedia.m3u8\n"
    origin = StaticOrigin("http://cdn.cbcs/vod/", res)
    loop = new_event_loop("virtual")
    hls = Hls(dict(config or {}, transmuxDevice="cpu"))
    media_el = MediaElement()
    events, errors = [], []
    E = Hls.Events
    for name in (E.FRAG_PARSING_INIT_SEGMENT, E.FRAG_PARSING_USERDATA, E.FRAG_PARSING_DATA, E.FRAG_PARSED,
                 E.FRAG_BUFFERED):
        hls.on(name, lambda e, d: events.append((e, d)))
    hls.on(E.ERROR, lambda e, d: errors.append(d))
    hls.loadSource("http://cdn.cbcs/vod/master.m3u8")
    hls.attachMedia(media_el)
    hls.on(E.MANIFEST_PARSED, lambda e, d: media_el.play())
    assert loop.run_until(lambda: sum(e == E.FRAG_BUFFERED for e, _ in events) >= want or errors, timeout_ms=60_000)
    hls.destroy()
    return events, errors, origin


def test_player_plays_a_sample_aes_ext_x_map_playlist(fresh):  # noqa: F811
    pairs = twins()
    events, errors, origin = play([p for _, p in pairs], {"enableCEA708Captions": True})
    E = Hls.Events
    assert not errors
    assert origin.requests.count("key.bin") == 1 and sum(u.endswith("init.mp4") for u in origin.requests) == 1
    assert [e for e, _ in events] == [E.FRAG_PARSING_INIT_SEGMENT, E.FRAG_PARSING_USERDATA, E.FRAG_PARSING_DATA,
                                      E.FRAG_PARSING_DATA, E.FRAG_PARSED, E.FRAG_BUFFERED, E.FRAG_PARSING_DATA,
                                      E.FRAG_PARSING_DATA, E.FRAG_PARSED, E.FRAG_BUFFERED]
    tracks = events[0][1]["tracks"]
    assert tracks["video"]["codec"] == "avc1.64001f" and tracks["audio"]["codec"] == "mp4a"
    assert tracks["video"]["initSegment"] == parse_init(INIT).clear_data != INIT
    assert events[1][1]["samples"]["n_samples"] == 5
    buffered = [d for e, d in events if e == E.FRAG_PARSING_DATA and d["type"] == "video"]
    assert [bytes(d["data2"].numpy()) for d in buffered] == [c for c, _ in pairs]  # the clear twins
    assert [d["nb"] for d in buffered] == [6, 3] and buffered[0]["frag"].sn == 3


def test_a_fragment_without_its_senc_is_a_decrypt_error(fresh):  # noqa: F811
    (_, stripped), _ = twins(senc=None)
    _, errors, _ = play([stripped], {"fragLoadingMaxRetry": 0}, want=1)
    assert errors and errors[0]["details"] == Hls.ErrorDetails.FRAG_DECRYPT_ERROR and "cbcs" in errors[0]["reason"]
    (_, good), _ = twins()
    _, errors, _ = play([good], {"fragLoadingMaxRetry": 0}, want=1)
    assert not errors
