"""Captions through the transmux pipeline and the player: a job with ``captions=True`` beside one
without in one batch, SAMPLE-AES and the remux combined with captions, the device pipeline against
the CPU pipeline, and ``FRAG_PARSING_USERDATA`` with ``enableCEA708Captions`` on, off and on a stream
without captions."""
import numpy as np
import pytest
import torch

import captions_cases as cc
import codec_cases
import sampleaes_cases as sc
from esindex_cases import adts_frame, background
from hlsjs_p2p_wrapper_amd.net import new_event_loop
from hlsjs_p2p_wrapper_amd.net.origin import StaticOrigin
from hlsjs_p2p_wrapper_amd.ops import captions
from hlsjs_p2p_wrapper_amd.player import Hls, MediaElement
from hlsjs_p2p_wrapper_amd.player.transmux import TransmuxJob
from test_codecconfig import REAL_SPS
from test_esindex import fresh  # noqa: F401  (fixture)
from test_sampleaes_pipeline import IV, KEY, SC3, captured_jobs, mux, run_pipeline

PAIRS = [[(0xFC, 0x94, 0x2C), (0xFD, 0x15, 0x2C)], [(0xFC, 0x94, 0xAE)], [(0xFC, 0xC8, 0xE9), (0xFC, 0x80, 0x80)],
         [(0xFC, 0x94, 0x2F), (0xFD, 0x41, 0x42), (0xFE, 0x01, 0x02)]]


def caption_streams(seed: int = 91, with_sei: bool = True, **timing):
    """``(protected TS, clear TS)``: four access units of AUD (+ SPS + PPS) + caption SEI + slice and
    four audio PES; slices and frames protected by the SAMPLE-AES cases' packager, the SEI left clear."""
    rng = np.random.default_rng(seed)
    slices = [[sc.nalu(rng, 0x65, 700)]] + [[sc.nalu(rng, 0x41, 300 + 17 * i)] for i in range(3)]
    frames = [[adts_frame(bytes(background(rng, 100 + 9 * i)), rate_idx=4)] for i in range(4)]
    pslices, pframes = sc.protect(slices, frames, KEY, IV)
    out = []
    for sl, fr, vt, at in ((pslices, pframes, 0xDB, 0xCF), (sc.clear_twin(slices), frames, 0x1B, 0x0F)):
        units = [b"\x00" + SC3 + b"\x09\xf0" + (b"\x00" + SC3 + REAL_SPS + SC3 + codec_cases.PPS if i == 0 else b"")
                 + (SC3 + cc.sei(cc.caption(PAIRS[i])) if with_sei else b"") + SC3 + u[0] for i, u in enumerate(sl)]
        out.append(mux(vt, at, units, [f[0] for f in fr], **timing))
    return out[0], out[1]


def check_pipeline(device):
    prot, clear = caption_streams()
    bare = caption_streams(with_sei=False)[1]
    out = run_pipeline(device, [(clear, dict(captions=True)), (clear, dict(remux=True)),
                                (prot, dict(captions=True, remux=True, sample_key=KEY, sample_iv=IV)),
                                (bare, dict(captions=True)), (clear, {})])
    for r in out.values():
        assert r.get("error") is None and r["status"] == 0
    a, b, c, d, e = (out[i] for i in range(5))
    assert "captions" not in b and "captions" not in e and "samples" in a and "fmp4" not in a and "samples" not in e
    ca = a["captions"]
    assert set(ca.keys()) == set(captions.CCINFO) | {"samples", "pts", "bytes", "cc608", "host"}
    assert (ca["status"], ca["n_sei"], ca["n_samples"], ca["n_triples"]) == (0, 4, 4, 8)
    assert (ca["field1_pairs"], ca["field2_pairs"]) == (4, 2)
    with pytest.raises(TypeError):
        ca["status"] = 1
    assert ca["samples"].shape == (captions.DEFAULT_MAX_CC, 8) and ca["samples"].device == a["demux"].es.device
    assert ca["bytes"].shape == (512, 96) and ca["cc608"].shape == (512, 2, 64) and ca["pts"].shape == (512,)
    host = ca.host()
    assert host is ca["host"]() and [s["bytes"] for s in host["samples"]] == \
        [bytes([0x40 | len(p), 0xFF]) + b"".join(bytes(t) for t in p) for p in PAIRS]
    pts = [s["pts"] for s in host["samples"]]
    assert pts == sorted(pts) and pts[0] == a["info"]["video_first_pts"]
    assert all(s["type"] == 3 for s in host["samples"])
    assert host["field1"] == [(pts[0], 0x14, 0x2C), (pts[1], 0x14, 0x2E), (pts[2], 0x48, 0x69), (pts[3], 0x14, 0x2F)]
    assert host["field2"] == [(pts[0], 0x15, 0x2C), (pts[3], 0x41, 0x42)]
    # SAMPLE-AES and the remux combined with captions: the clear stream's captions, and the clear stream's fMP4
    hc = c["captions"].host()
    assert hc["samples"] == host["samples"] and hc["field1"] == host["field1"] and hc["field2"] == host["field2"]
    for name in ("samples", "pts", "bytes", "cc608"):
        assert torch.equal(c["captions"][name].cpu(), ca[name].cpu()), name
    assert c["sample_aes"]["protected_nals"] == 4
    for track in ("video", "audio"):
        assert torch.equal(c["fmp4"][track]["mdat"].cpu(), b["fmp4"][track]["mdat"].cpu())
    # a stream without captions
    assert (d["captions"]["n_samples"], d["captions"]["n_sei"], d["captions"].host()["samples"]) == (0, 0, [])
    # the jobs that did not ask got what a batch without the feature gives, key for key
    alone = run_pipeline(device, [(clear, dict(remux=True)), (clear, {})])
    views = {"video", "audio", "id3"}  # made on first access
    for got, want in ((b, alone[0]), (e, alone[1])):
        assert set(dict(got)) - views == set(dict(want)) - views
        assert torch.equal(got["video"].cpu(), want["video"].cpu())
        assert dict(got["info"].items()) == dict(want["info"].items())
    assert torch.equal(alone[0]["fmp4"]["video"]["mdat"].cpu(), b["fmp4"]["video"]["mdat"].cpu())
    assert dict(alone[0]["fmp4"]["config"]) == dict(b["fmp4"]["config"])
    return out


def test_pipeline_extracts_for_the_jobs_that_ask_and_leaves_the_others_alone():
    check_pipeline("cpu")
    job = TransmuxJob(b"", None, None, print, captions=True)
    assert job.index and job.captions and not job.remux and job.sample_key is None
    assert not TransmuxJob(b"", None, None, print).captions


@pytest.mark.gpu
def test_pipeline_on_the_device_equals_the_cpu_pipeline(cuda):
    out, host = check_pipeline(cuda), check_pipeline("cpu")
    for i in (0, 2, 3):
        assert dict((k, out[i]["captions"][k]) for k in captions.CCINFO) == \
            dict((k, host[i]["captions"][k]) for k in captions.CCINFO)
        for name in ("samples", "pts", "bytes", "cc608"):
            assert torch.equal(out[i]["captions"][name].cpu(), host[i]["captions"][name]), name


# ---------------------------------------------------------------- the player
def play(config, with_sei=True, listen=True):
    """Two segments through a player; ``(events in order, errors, jobs' caption flags)``."""
    segs = [caption_streams(seed=92 + k, with_sei=with_sei, t0=900_000 + 180_000 * k, step=45_000)[1] for k in range(2)]
    media = "\n".join(["#EXTM3U", "#EXT-X-VERSION:3", "#EXT-X-TARGETDURATION:2", "#EXT-X-MEDIA-SEQUENCE:7",
                       "#EXTINF:2.0,", "seg7.ts", "#EXTINF:2.0,", "seg8.ts", "#EXT-X-ENDLIST", ""])
    master = "#EXTM3U\n#EXT-X-STREAM-INF:BANDWIDTH=300000,RESOLUTION=1280x720\nmedia.m3u8\n"
    data = lambda b: np.frombuffer(b, np.uint8).copy()  # noqa: E731
    StaticOrigin("http://cdn.cc/vod/", {"master.m3u8": master, "media.m3u8": media, "seg7.ts": data(segs[0]),
                                        "seg8.ts": data(segs[1])})
    loop = new_event_loop("virtual")
    hls = Hls(dict(config, transmuxDevice="cpu"))
    media_el = MediaElement()
    events, errors = [], []
    E = Hls.Events
    watched = [E.FRAG_PARSING_INIT_SEGMENT, E.FRAG_PARSING_METADATA, E.FRAG_PARSING_DATA, E.FRAG_PARSED]
    for name in watched + ([E.FRAG_PARSING_USERDATA] if listen else []):
        hls.on(name, lambda e, d: events.append((e, d)))
    hls.on(E.ERROR, lambda e, d: errors.append(d))
    hls.loadSource("http://cdn.cc/vod/master.m3u8")
    hls.attachMedia(media_el)
    hls.on(E.MANIFEST_PARSED, lambda e, d: media_el.play())
    assert loop.run_until(lambda: sum(e == E.FRAG_PARSED for e, _ in events) >= 2 or errors, timeout_ms=60_000)
    hls.destroy()
    return events, errors


def plain(events):
    """The events without user data, as comparable values."""
    out = []
    for e, d in events:
        if e == Hls.Events.FRAG_PARSING_USERDATA:
            continue
        row = {k: (v.cpu().numpy().tobytes() if isinstance(v, torch.Tensor) else v) for k, v in d.items()
               if k not in ("frag", "samples", "tracks")}
        out.append((e, d["frag"].sn, row, sorted(d.get("tracks", {}))))
    return out


def test_userdata_fires_with_the_key_on_and_captions_present(fresh, monkeypatch):  # noqa: F811
    jobs = captured_jobs(monkeypatch)
    events, errors = play({"enableCEA708Captions": True})
    assert not errors and jobs and all(j.captions and j.index and not j.remux for j in jobs)
    E = Hls.Events
    user = [(i, d) for i, (e, d) in enumerate(events) if e == E.FRAG_PARSING_USERDATA]
    assert [d["frag"].sn for _, d in user[:2]] == [7, 8]
    for i, d in user[:2]:
        assert set(d) == {"frag", "samples"} and d["samples"]["n_samples"] == 4
        host = d["samples"].host()
        pts = [s["pts"] for s in host["samples"]]
        assert pts == sorted(pts) and len(pts) == 4 and host["samples"][0]["bytes"][:2] == b"\x42\xff"
        # between the metadata and the data events of its fragment
        assert events[i + 1][0] == E.FRAG_PARSING_DATA and events[i + 1][1]["frag"] is d["frag"]
        assert events[i - 1][0] in (E.FRAG_PARSING_INIT_SEGMENT, E.FRAG_PARSING_METADATA, E.FRAG_PARSED)
    # the other events' payloads are what they are with the key off
    off, errors_off = play({})
    assert not errors_off and plain(off) == plain(events)


def test_userdata_does_not_fire_with_the_key_off_or_without_captions(fresh, monkeypatch):  # noqa: F811
    jobs = captured_jobs(monkeypatch)
    E = Hls.Events
    events, errors = play({})
    assert not errors and not any(e == E.FRAG_PARSING_USERDATA for e, _ in events)
    assert jobs and not any(j.captions or j.index for j in jobs)
    assert Hls({}).config.get("enableCEA708Captions") is False
    events, errors = play({"enableCEA708Captions": True}, with_sei=False)
    assert not errors and not any(e == E.FRAG_PARSING_USERDATA for e, _ in events)
    assert sum(e == E.FRAG_PARSED for e, _ in events) >= 2
    # nobody listens: nothing is built, the fragments parse as before
    events, errors = play({"enableCEA708Captions": True}, listen=False)
    assert not errors and sum(e == E.FRAG_PARSED for e, _ in events) >= 2
