"""SAMPLE-AES through the layers above the op: the two PMT stream types the format mandates
(``0xDB`` protected H.264, ``0xCF`` protected ADTS AAC) demux like ``0x1B`` / ``0x0F``; a TS muxed
from a protected ES and submitted with ``sample_key`` / ``sample_iv`` gives the fMP4 of its clear
twin; a ``METHOD=SAMPLE-AES`` playlist makes the player load the key and hand it to the pipeline as
``sample_key`` with ``key`` left ``None``; an unsupported codec raises ``FRAG_DECRYPT_ERROR``."""
import numpy as np
import pytest
import torch

import codec_cases as cc
import sampleaes_cases as sc
import ts_builder
from esindex_cases import adts_frame, background
from hlsjs_p2p_wrapper_amd.net import new_event_loop
from hlsjs_p2p_wrapper_amd.net.origin import Rendition, StaticOrigin, SyntheticHlsOrigin
from hlsjs_p2p_wrapper_amd.ops import sampleaes, tsdemux
from hlsjs_p2p_wrapper_amd.player import ErrorDetails, Hls, MediaElement
from hlsjs_p2p_wrapper_amd.player.level import Fragment
from hlsjs_p2p_wrapper_amd.player.transmux import MediaPipeline, TransmuxJob
from test_codecconfig import REAL_SPS
from test_esindex import fresh  # noqa: F401  (fixture)
from ts_builder import _Muxer, _pes, _section

SC3 = b"\x00\x00\x01"
KEY, IV = bytes(range(40, 56)), bytes(range(200, 216))
APID, PMTPID = 0x101, 0x1000


# ---------------------------------------------------------------- the PMT stream types
def protected_audio_type(ts: bytes) -> bytes:
    """``ts`` with the audio stream type of every PMT section set to 0xCF and its CRC redone."""
    out = bytearray(ts)
    patched = 0
    for p in range(0, len(out), 188):
        pkt = out[p:p + 188]
        if ((pkt[1] & 0x1F) << 8 | pkt[2]) != PMTPID or not pkt[1] & 0x40:
            continue
        s = 4 + (1 + pkt[4] if pkt[3] & 0x20 else 0)
        s += 1 + pkt[s]  # pointer field
        n = 3 + ((pkt[s + 1] & 0x0F) << 8 | pkt[s + 2])
        entry = bytes([0x0F, 0xE0 | (APID >> 8), APID & 0xFF])
        at = bytes(pkt[s:s + n]).index(entry)
        pkt[s + at] = 0xCF
        pkt[s + n - 4:s + n] = ts_builder._crc32_mpeg(bytes(pkt[s:s + n - 4])).to_bytes(4, "big")
        out[p:p + 188] = pkt
        patched += 1
    assert patched == 2  # the PMT repeats mid-segment
    return bytes(out)


def demux(streams, device="cpu"):
    offs, pos = [], 0
    for s in streams:
        offs.append(pos)
        pos += (len(s) + 255) // 256 * 256
    buf = np.zeros(pos + 256, np.uint8)
    for o, s in zip(offs, streams):
        buf[o:o + len(s)] = np.frombuffer(s, np.uint8)
    dev = torch.device(device)
    return tsdemux.demux_batch(torch.from_numpy(buf).to(dev), offs, [len(s) for s in streams],
                               torch.zeros(pos + 256, dtype=torch.uint8, device=dev), offs)


def check_psi(device):
    clear, truth = ts_builder.build(seed=3)
    prot, _ = ts_builder.build(seed=3, video_type=0xDB)
    prot = protected_audio_type(prot)
    assert len(prot) == len(clear) and prot != clear
    res = demux([clear, prot], device)
    info = res.info.cpu().numpy()
    I = tsdemux.INFO
    assert info[1, I["video_type"]] == 0x1B and info[1, I["audio_type"]] == 0x0F and info[1, I["status"]] == 0
    assert info[1, I["video_pid"]] == truth["video"]["pid"] and info[1, I["audio_pid"]] == APID
    assert np.array_equal(info[0], info[1]) and torch.equal(res.pes[0], res.pes[1])
    n = int(info[0, I["payload_bytes"]])
    assert n == sum(len(truth[c]["es"]) for c in ts_builder.CLASSES)
    es = res.es.cpu()
    o0, o1 = (int(o) for o in res.es_offs)
    assert torch.equal(es[o0:o0 + n], es[o1:o1 + n])
    assert es[o0:o0 + len(truth["video"]["es"])].numpy().tobytes() == truth["video"]["es"]


def test_protected_stream_types_demux_like_the_clear_ones():
    check_psi("cpu")


@pytest.mark.gpu
def test_protected_stream_types_demux_like_the_clear_ones_on_the_device(cuda):
    check_psi(cuda)


# ---------------------------------------------------------------- the pipeline
def mux(video_type: int, audio_type: int, units, audio_units, t0: int = 900_000, step: int = 3600) -> bytes:
    """A TS built with ``ts_builder``'s muxer: one video PES per access unit, one audio PES per entry."""
    VPID = 0x100
    m = _Muxer()
    streams = b""
    for st, pid in ((video_type, VPID), (audio_type, APID)):
        streams += bytes([st, 0xE0 | (pid >> 8), pid & 0xFF, 0xF0, 0x00])
    m.psi(0, _section(0x00, 1, bytes([0, 1, 0xE0 | (PMTPID >> 8), PMTPID & 0xFF])))
    m.psi(PMTPID, _section(0x02, 1, bytes([0xE0 | (VPID >> 8), VPID & 0xFF, 0xF0, 0x00]) + streams))
    for i, payload in enumerate(units):
        m.pes(VPID, _pes(0xE0, payload, t0 + step * i + step, t0 + step * i, length_field=False))
        if i < len(audio_units):
            m.pes(APID, _pes(0xC0, audio_units[i], t0 + step * i))
    return b"".join(m.packets)


def twin_streams(seed: int = 81, video_type: int = 0xDB, **timing):
    """``(protected TS, clear TS)``: AUD + SPS + PPS + IDR, then three AUD + slice units, and four
    audio PES of one frame; slices and frames protected with ``KEY`` / ``IV`` by the cases' packager."""
    rng = np.random.default_rng(seed)
    slices = [[sc.nalu(rng, 0x65, 700)]] + [[sc.nalu(rng, 0x41, 300 + 17 * i)] for i in range(3)]
    frames = [[adts_frame(bytes(background(rng, 100 + 9 * i)), rate_idx=4)] for i in range(4)]
    pslices, pframes = sc.protect(slices, frames, KEY, IV)
    out = []
    for sl, fr, vt, at in ((pslices, pframes, video_type, 0xCF), (sc.clear_twin(slices), frames, 0x1B, 0x0F)):
        units = [b"\x00" + SC3 + b"\x09\xf0" + (b"\x00" + SC3 + REAL_SPS + SC3 + cc.PPS if i == 0 else b"") + SC3 + u[0]
                 for i, u in enumerate(sl)]
        out.append(mux(vt, at, units, [f[0] for f in fr], **timing))
    return out[0], out[1]


def run_pipeline(device, jobs):
    """``jobs``: ``(ts, kwargs)``; one batch; results by position."""
    pipe = MediaPipeline(torch.device(device), new_event_loop("virtual"))
    out = {}
    for n, (ts, kw) in enumerate(jobs):
        pipe.submit(TransmuxJob(torch.from_numpy(np.frombuffer(ts, np.uint8).copy()), None, None,
                                lambda r, n=n: out.__setitem__(n, r), **kw))
    pipe.flush()
    return out


def check_pipeline(device):
    prot, clear = twin_streams()
    ask = dict(sample_key=KEY, sample_iv=IV)
    out = run_pipeline(device, [(prot, dict(remux=True, **ask)), (clear, dict(remux=True)), (prot, ask)])
    a, b, c = out[0], out[1], out[2]
    for r in (a, b, c):
        assert r.get("error") is None and r["status"] == 0
    assert "sample_aes" not in b and "fmp4" in b and "fmp4" not in c and "samples" in c
    sa = a["sample_aes"]
    assert dict(sa) == dict(c["sample_aes"]) and set(sa) == set(sampleaes.SAINFO)
    assert (sa["status"], sa["protected_nals"], sa["audio_frames"]) == (0, 4, 4)
    assert sa["video_blocks"] == 5 + 2 + 2 + 2 and sa["audio_blocks"] == sum((100 + 9 * i - 16) // 16 for i in range(4))
    with pytest.raises(TypeError):
        sa["status"] = 1
    assert a["info"]["video_type"] == 0x1B and a["info"]["audio_type"] == 0x0F
    fa, fb = a["fmp4"], b["fmp4"]
    for track in ("video", "audio"):
        ta, tb = fa[track], fb[track]
        assert torch.equal(ta["mdat"].cpu(), tb["mdat"].cpu()) and ta["mdat"].numel() > 8
        assert ta.moof(7) == tb.moof(7) and ta["init"] == tb["init"] is not None and ta["codec"] == tb["codec"]
        assert torch.equal(ta["samples"].cpu(), tb["samples"].cpu())
    assert fa["video"]["codec"] == "avc1.64001f" and dict(fa["config"]) == dict(fb["config"])
    # the raw views are those of the decrypted ES: the audio equals the clear twin's byte for byte
    assert torch.equal(a["audio"].cpu(), b["audio"].cpu()) and torch.equal(c["audio"].cpu(), b["audio"].cpu())
    assert a["samples"]["n_nal"] == b["samples"]["n_nal"]
    # the twin got what a batch without the feature gives
    alone = run_pipeline(device, [(clear, dict(remux=True))])[0]
    views = {"video", "audio", "id3"}  # made on first access
    assert set(dict(alone)) - views == set(dict(b)) - views and torch.equal(alone["video"].cpu(), b["video"].cpu())
    assert torch.equal(alone["fmp4"]["video"]["mdat"].cpu(), fb["video"]["mdat"].cpu())
    return out


def test_pipeline_decrypts_the_jobs_that_ask_and_leaves_the_others_alone():
    check_pipeline("cpu")
    with pytest.raises(ValueError, match="go together"):
        TransmuxJob(b"", None, None, print, sample_key=KEY)
    job = TransmuxJob(b"", None, None, print, sample_key=KEY, sample_iv=IV)
    assert job.index and not job.remux and job.key is None and job.iv is None


@pytest.mark.gpu
def test_pipeline_on_the_device_equals_the_cpu_pipeline(cuda):
    out, host = check_pipeline(cuda), check_pipeline("cpu")
    assert dict(out[0]["sample_aes"]) == dict(host[0]["sample_aes"])
    for track in ("video", "audio"):
        assert torch.equal(out[0]["fmp4"][track]["mdat"].cpu(), host[0]["fmp4"][track]["mdat"])
        assert torch.equal(out[0][track].cpu(), host[0][track])


# ---------------------------------------------------------------- the player
def captured_jobs(monkeypatch):
    jobs = []
    submit = MediaPipeline.submit

    def record(self, job):
        jobs.append(job)
        submit(self, job)

    monkeypatch.setattr(MediaPipeline, "submit", record)
    return jobs


def play(url, config, until=2):
    loop = new_event_loop("virtual")
    hls = Hls(dict(config, transmuxDevice="cpu"))
    media = MediaElement()
    parsed, errors, keys = [], [], []
    hls.on(Hls.Events.FRAG_PARSED, lambda e, d: parsed.append(d))
    hls.on(Hls.Events.ERROR, lambda e, d: errors.append(d))
    hls.on(Hls.Events.KEY_LOADED, lambda e, d: keys.append(d["frag"].sn))
    hls.loadSource(url)
    hls.attachMedia(media)
    hls.on(Hls.Events.MANIFEST_PARSED, lambda e, d: media.play())
    assert loop.run_until(lambda: len(parsed) >= until or errors, timeout_ms=60_000)
    hls.destroy()
    return parsed, errors, keys


def test_a_sample_aes_playlist_loads_the_key_and_submits_it_as_the_sample_key(fresh, monkeypatch):  # noqa: F811
    # two segments of 2 s: four access units half a second apart each
    first, second = (twin_streams(seed=82 + k, t0=900_000 + 180_000 * k, step=45_000)[0] for k in range(2))
    media = "\n".join(["#EXTM3U", "#EXT-X-VERSION:3", "#EXT-X-TARGETDURATION:2", "#EXT-X-MEDIA-SEQUENCE:7",
                       f'#EXT-X-KEY:METHOD=SAMPLE-AES,URI="key.bin",IV=0x{IV.hex()}', "#EXTINF:2.0,", "seg7.ts",
                       '#EXT-X-KEY:METHOD=SAMPLE-AES,URI="key.bin"', "#EXTINF:2.0,", "seg8.ts", "#EXT-X-ENDLIST", ""])
    master = "#EXTM3U\n#EXT-X-STREAM-INF:BANDWIDTH=300000,RESOLUTION=1280x720\nmedia.m3u8\n"
    data = lambda b: np.frombuffer(b, np.uint8).copy()  # noqa: E731
    origin = StaticOrigin("http://cdn.sa/vod/", {"master.m3u8": master, "media.m3u8": media, "key.bin": data(KEY),
                                                 "seg7.ts": data(first), "seg8.ts": data(second)})
    jobs = captured_jobs(monkeypatch)
    parsed, errors, keys = play("http://cdn.sa/vod/master.m3u8", {"remuxFmp4": True})
    assert not errors and [d["frag"].sn for d in parsed[:2]] == [7, 8]
    assert origin.requests.count("key.bin") == 1 and keys[0] == 7  # fetched once, in front of the first fragment
    by_sn = {j.frag.sn: j for j in jobs}
    for sn, iv in ((7, IV), (8, (8).to_bytes(16, "big"))):  # the attribute, else the sequence number
        j = by_sn[sn]
        assert j.sample_key == KEY and j.sample_iv == iv and j.key is None and j.iv is None and j.index and j.remux
        assert j.frag.decryptdata.method == "SAMPLE-AES"


def test_an_aes_128_playlists_job_is_unchanged(fresh, monkeypatch):  # noqa: F811
    origin = SyntheticHlsOrigin("http://cdn.sa128/vod/", renditions=[Rendition(300_000, 640, 360)], num_segments=3,
                                segment_duration=2.0, encrypted=True)
    jobs = captured_jobs(monkeypatch)
    parsed, errors, _ = play(origin.master_url(), {})
    assert not errors and len(parsed) >= 2 and jobs
    for j in jobs:
        assert j.key == origin.key and j.iv == origin.iv and j.sample_key is None and j.sample_iv is None
        assert not j.index and not j.remux


def test_an_unsupported_codec_under_sample_aes_is_a_decrypt_error(fresh):  # noqa: F811
    """HEVC has no SAMPLE-AES TS format: the fragment would buffer ciphertext, so it fails like a
    bad PKCS#7 length and goes through the retry path."""
    prot, clear = twin_streams(video_type=0x24)
    out = run_pipeline("cpu", [(prot, dict(sample_key=KEY, sample_iv=IV)), (clear, dict(sample_key=KEY, sample_iv=IV))])
    assert out[0]["sample_aes"]["status"] == sampleaes.SASTATUS["unsupported_video"] and out[0]["status"] == 0
    assert out[1]["sample_aes"]["status"] == 0
    new_event_loop("virtual")
    hls = Hls(dict(transmuxDevice="cpu", autoStartLoad=False))
    errors, parsed = [], []
    hls.on(Hls.Events.ERROR, lambda e, d: errors.append(d))
    hls.on(Hls.Events.FRAG_PARSED, lambda e, d: parsed.append(d))
    ctl = hls.streamController
    for sn, r in enumerate((out[0], out[1])):
        frag = Fragment(f"http://cdn.sa/seg{sn}.ts", sn, 2.0 * sn, 2.0)
        ctl.inflight[(frag.level, frag.sn)] = frag
        ctl._on_parsed(frag, {"trequest": 0, "tfirst": 0, "length": 1000}, r)
    hls.destroy()
    assert len(errors) == 1 and errors[0]["details"] == ErrorDetails.FRAG_DECRYPT_ERROR and not errors[0]["fatal"]
    assert errors[0]["frag"].sn == 0 and "SAMPLE-AES" in errors[0]["reason"]
    assert [d["frag"].sn for d in parsed] == [1]
