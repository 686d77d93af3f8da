"""``cenc``-protected fragmented-MP4 fragments through the transmux pipeline
(``TransmuxJob(mp4=init, sample_key=...)``) and through a player on a ``METHOD=SAMPLE-AES-CTR``
``#EXT-X-MAP`` playlist: a cenc job beside a cbcs job, a clear fMP4 job and a TS job in one batch,
the result mapping, the device pipeline against the CPU pipeline, the event sequence, the key
requested once, the buffered bytes against the clear twin, ``FRAG_DECRYPT_ERROR`` for a fragment
whose ``senc`` was removed, and the init segments that are refused."""
import numpy as np
import pytest
import torch

import cbcs_cases as cc
import cenc_cases as ce
import test_cbcs_pipeline as cp
from hlsjs_p2p_wrapper_amd.net import new_event_loop
from hlsjs_p2p_wrapper_amd.net.origin import StaticOrigin
from hlsjs_p2p_wrapper_amd.ops import tsdemux
from hlsjs_p2p_wrapper_amd.ops.cenc import CINFO
from hlsjs_p2p_wrapper_amd.player import Hls, MediaElement
from hlsjs_p2p_wrapper_amd.player.level import DecryptData, Fragment
from hlsjs_p2p_wrapper_amd.player.mp4init import parse_init
from hlsjs_p2p_wrapper_amd.player.transmux import TransmuxJob
from test_esindex import fresh  # noqa: F401  (fixture)
from test_mp4_pipeline import fragments

KEY, IV = cp.KEY, cp.IV
# both tracks with the constant IVs that the twins of test_cbcs_pipeline are packaged with
INIT = ce.cenc_init(video_tenc=cc.tenc(pattern=(0, 0)))


def twins(senc="after"):
    """``test_cbcs_pipeline.twins`` packaged under cenc: (clear twin, protected) of two fragments."""
    with ce.as_cenc():
        return cp.twins(senc)


def check_pipeline(device):
    init, cbcs_init, clear_init = parse_init(INIT), parse_init(cp.INIT), parse_init(cp.CLEAR_INIT)
    assert [t.protection.scheme for t in init.tracks] == ["cenc", "cenc"]
    (clear, prot), _ = twins()
    (cbcs_clear, cbcs_prot), _ = cp.twins()
    assert clear == cbcs_clear and prot != cbcs_prot
    ts, _ = tsdemux.mux_segment(target_bytes=40 * 188, seed=5)
    out = {}
    cp.run(device, [TransmuxJob(prot, None, None, lambda r: out.__setitem__("cenc", r), mp4=init, captions=True,
                                sample_key=KEY, sample_iv=IV),
                    TransmuxJob(cbcs_prot, None, None, lambda r: out.__setitem__("cbcs", r), mp4=cbcs_init,
                                captions=True, sample_key=KEY, sample_iv=IV),
                    TransmuxJob(fragments()[0], None, None, lambda r: out.__setitem__("clear", r), mp4=clear_init,
                                captions=True),
                    TransmuxJob(ts, None, None, lambda r: out.__setitem__("ts", r)),
                    TransmuxJob(prot, None, None, lambda r: out.__setitem__("raw", r), mp4=init)])
    assert out["ts"]["status"] == 0 and not any("cenc" in out[k] for k in ("ts", "clear", "raw", "cbcs"))
    assert "cbcs" in out["cbcs"] and "cbcs" not in out["cenc"]
    r = out["cenc"]
    assert r["container"] == "mp4" and r["status"] == 0 and r["init"] is init and r["plain_bytes"] == len(prot)
    assert bytes(r["data"].cpu().numpy()) == clear and bytes(out["raw"]["data"].cpu().numpy()) == prot
    assert bytes(out["cbcs"]["data"].cpu().numpy()) == clear
    # a subsample per NAL unit, 17 in the six video samples; three whole audio samples of 40, 41, 42 bytes
    assert dict(r["cenc"]) == {"status": 0, "n_ranges": 17 + 3, "video_samples": 6, "audio_samples": 3,
                               "video_bytes": r["cenc"]["video_bytes"], "audio_bytes": 40 + 41 + 42, "n_senc": 2,
                               "n_units": r["cenc"]["n_units"]}
    assert set(r["cenc"]) == set(CINFO) and r["cenc"]["video_bytes"] > 17 and r["cenc"]["n_units"] >= 17 + 3 * 3
    with pytest.raises(TypeError):
        r["cenc"]["status"] = 1  # read-only
    assert r["video"]["nb"] == 6 and r["audio"]["nb"] == 3 and r["video"]["codec"] == "avc1.64001f"
    assert r["captions"]["n_samples"] == 5 and r["samples"]["n_nal"] == 17
    assert torch.equal(r["captions"]["bytes"].cpu(), out["clear"]["captions"]["bytes"].cpu())
    assert torch.equal(r["captions"]["bytes"].cpu(), out["cbcs"]["captions"]["bytes"].cpu())
    return out


def test_pipeline_decrypts_a_cenc_job_beside_cbcs_clear_mp4_and_ts_jobs():
    check_pipeline("cpu")


@pytest.mark.gpu
def test_pipeline_on_the_device_equals_the_cpu_pipeline(cuda):
    dev, cpu = check_pipeline(cuda), check_pipeline("cpu")
    for name in ("cenc", "cbcs", "clear", "raw"):
        for t in ("video", "audio"):
            for k in dev[name][t].keys():
                a, b = dev[name][t][k], cpu[name][t][k]
                assert torch.equal(a.cpu(), b) if isinstance(a, torch.Tensor) else a == b, (name, t, k)
        assert dev[name]["info"] == cpu[name]["info"] and torch.equal(dev[name]["data"].cpu(), cpu[name]["data"])
    assert dict(dev["cenc"]["cenc"]) == dict(cpu["cenc"]["cenc"])
    assert torch.equal(dev["cenc"]["captions"]["bytes"].cpu(), cpu["cenc"]["captions"]["bytes"])


def test_init_segments_that_are_refused_and_accepted():
    (_, prot), _ = twins()
    mixed = parse_init(ce.cenc_init(video_scheme=b"cbcs", video_tenc=cc.tenc()))
    assert [t.protection.scheme for t in mixed.tracks] == ["cbcs", "cenc"]
    with pytest.raises(ValueError, match="a cbcs and a cenc track"):
        TransmuxJob(prot, None, None, print, mp4=mixed, sample_key=KEY, sample_iv=IV)
    with pytest.raises(ValueError, match=r"SAMPLE-AES \(cbcs\) fragmented MP4 is not supported"):
        TransmuxJob(prot, None, None, print, mp4=parse_init(cp.CLEAR_INIT), sample_key=KEY, sample_iv=IV)
    with pytest.raises(ValueError, match="not both"):
        TransmuxJob(prot, KEY, IV, print, mp4=parse_init(INIT), sample_key=KEY, sample_iv=IV)
    assert TransmuxJob(prot, None, None, print, mp4=parse_init(INIT), sample_key=KEY, sample_iv=IV).scheme == "cenc"
    assert TransmuxJob(prot, None, None, print, mp4=parse_init(cp.INIT), sample_key=KEY, sample_iv=IV).scheme == "cbcs"
    assert TransmuxJob(prot, None, None, print, mp4=parse_init(INIT)).scheme is None
    one = parse_init(ce.cenc_init(audio=False))  # one protected track is enough; 8-byte per-sample IVs
    assert one.video.protection.per_sample_iv_size == 8 and one.audio.protection is None
    assert TransmuxJob(prot, None, None, print, mp4=one, sample_key=KEY, sample_iv=IV).scheme == "cenc"


def test_the_playlist_model_loads_the_key_of_a_sample_aes_ctr_fragment():
    dd = DecryptData(method="SAMPLE-AES-CTR", uri="http://cdn/key.bin")
    assert dd.needs_key
    dd.key = KEY
    assert not dd.needs_key
    assert Fragment("u", 7, 0.0, 2.0, decryptdata=dd).iv_for_decrypt() == (7).to_bytes(16, "big")
    assert Fragment("u", 7, 0.0, 2.0, decryptdata=DecryptData("SAMPLE-AES-CTR", "k", IV)).iv_for_decrypt() == IV
    assert not DecryptData(method="SAMPLE-AES-CENC", uri="k").needs_key


# ---------------------------------------------------------------- the player
def play(segments, config=None, want=2, init=INIT, method="SAMPLE-AES-CTR"):
    lines = ["#EXTM3U", "#EXT-X-VERSION:7", "#EXT-X-TARGETDURATION:2", "#EXT-X-MEDIA-SEQUENCE:3",
             '#EXT-X-MAP:URI="init.mp4"', f'#EXT-X-KEY:METHOD={method},URI="key.bin",IV=0x{IV.hex()}']
    data = lambda b: np.frombuffer(b, np.uint8).copy()  # noqa: E731
    res = {"init.mp4": data(init), "key.bin": data(KEY)}
    for k, seg in enumerate(segments):
        lines += ["#EXTINF:2.0,", f"s{k}.m4s"]
        res[f"s{k}.m4s"] = data(seg)
    res["media.m3u8"] = "\n".join(lines + ["#EXT-X-ENDLIST", ""])
    res["master.m3u8"] = "#EXTM3U\n#EXT-X-STREAM-INF:BANDWIDTH=300000,RESOLUTION=640x360\nmedia.m3u8\n"
    origin = StaticOrigin("http://cdn.cenc/vod/", res)
    loop = new_event_loop("virtual")
    hls = Hls(dict(config or {}, transmuxDevice="cpu"))
    media_el = MediaElement()
    events, errors = [], []
    E = Hls.Events
    for name in (E.FRAG_PARSING_INIT_SEGMENT, E.FRAG_PARSING_USERDATA, E.FRAG_PARSING_DATA, E.FRAG_PARSED,
                 E.FRAG_BUFFERED):
        hls.on(name, lambda e, d: events.append((e, d)))
    hls.on(E.ERROR, lambda e, d: errors.append(d))
    hls.loadSource("http://cdn.cenc/vod/master.m3u8")
    hls.attachMedia(media_el)
    hls.on(E.MANIFEST_PARSED, lambda e, d: media_el.play())
    assert loop.run_until(lambda: sum(e == E.FRAG_BUFFERED for e, _ in events) >= want or errors, timeout_ms=60_000)
    hls.destroy()
    return events, errors, origin


def test_player_plays_a_sample_aes_ctr_ext_x_map_playlist(fresh):  # noqa: F811
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


def test_the_init_segment_decides_when_the_method_disagrees(fresh):  # noqa: F811
    pairs = twins()
    events, errors, _ = play([p for _, p in pairs], method="SAMPLE-AES")  # a cenc init segment under the cbcs method
    buffered = [d for e, d in events if e == Hls.Events.FRAG_PARSING_DATA and d["type"] == "video"]
    assert not errors and [bytes(d["data2"].numpy()) for d in buffered] == [c for c, _ in pairs]


def test_a_fragment_without_its_senc_is_a_decrypt_error(fresh):  # noqa: F811
    (_, stripped), _ = twins(senc=None)
    _, errors, _ = play([stripped], {"fragLoadingMaxRetry": 0}, want=1)
    assert errors and errors[0]["details"] == Hls.ErrorDetails.FRAG_DECRYPT_ERROR and "cenc" in errors[0]["reason"]
    (_, good), _ = twins()
    _, errors, _ = play([good], {"fragLoadingMaxRetry": 0}, want=1)
    assert not errors
