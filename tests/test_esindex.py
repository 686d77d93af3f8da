"""Sample index (``ops/esindex.py``) on the host implementation: NAL units, access units and
ADTS frames of demuxed segments equal an independent sequential reference
(``tests/esindex_cases.py``) exactly -- on hand-built edge cases, on the synthetic muxer's
output, on a spec-built stream -- and the index reaches the pipeline's results and the
player's events only when asked for."""
import numpy as np
import pytest
import torch

from esindex_cases import CASES, SC, TILE, adts_frame, assert_index_equal, background, hand_batch, ref_batch
from hlsjs_p2p_wrapper_amd import Hls
from hlsjs_p2p_wrapper_amd.agent import set_current_node
from hlsjs_p2p_wrapper_amd.net import clear_origins, new_event_loop
from hlsjs_p2p_wrapper_amd.net.origin import Rendition, SyntheticHlsOrigin
from hlsjs_p2p_wrapper_amd.ops import aes, esindex, tsdemux
from hlsjs_p2p_wrapper_amd.ops._native import runtime
from hlsjs_p2p_wrapper_amd.player import MediaElement
from hlsjs_p2p_wrapper_amd.player.transmux import MediaPipeline, Samples, TransmuxJob
from ts_builder import _Muxer, _pes, _section


@pytest.mark.parametrize("case", sorted(CASES))
def test_hand_built_cases_match_the_reference(case):
    segs, max_pes, max_nal = CASES[case](TILE)
    res, caps = hand_batch(segs, "cpu", max_pes)
    ix = esindex.index_batch(res, caps, max_nal=max_nal)
    assert_index_equal(ix, ref_batch(res, caps, max_nal))


def test_the_cases_hold_what_they_are_meant_to():
    """The properties the cases exist for, stated on the result itself (a reference that was
    wrong in the same way as the code would not show in the comparison above)."""
    S, ST = esindex.SINFO, esindex.SSTATUS
    segs, max_pes, max_nal = CASES["end_of_video"](TILE)
    res, caps = hand_batch(segs, "cpu", max_pes)
    ix = esindex.index_batch(res, caps, max_nal=max_nal)
    assert ix.sinfo[0, S["n_nal"]] == 0  # 00 00 | 01 65 across the video / audio seam: no match
    assert ix.sinfo[1, S["n_nal"]] == 1 and ix.nal[1, 0].tolist()[:2] == [299, 1]

    segs, max_pes, max_nal = CASES["zero_runs"](TILE)
    res, caps = hand_batch(segs, "cpu", max_pes)
    s = esindex.index_batch(res, caps, max_nal=max_nal).segment(0)
    nal = s["nal"]
    assert s["n_nal"] == 10 and nal[:, 0].tolist() == [23, 45, 103, 106, 163, 166, 169, 172, 175, 178]
    assert nal[0, 1] == 41 - 23  # 00 00 00 00 01: only the zero next to the start code is stripped
    assert nal[2, 1:3].tolist() == [0, -1] and nal[3, 1] > 0
    assert (nal[4:9, 1] == 0).all()

    segs, max_pes, max_nal = CASES["overflow"](TILE)
    res, caps = hand_batch(segs, "cpu", max_pes)
    ix = esindex.index_batch(res, caps, max_nal=max_nal)
    assert ix.sinfo[:, S["n_nal"]].tolist() == [65, 200, 64, 63]
    assert [int(x) & ST["nal_overflow"] for x in ix.sinfo[:, S["status"]]] == [1, 1, 0, 0]
    assert (ix.nal[:2, :, 0] >= 0).all() and ix.nal[3, 63, 0] == -1

    segs, max_pes, max_nal = CASES["au_mapping"](TILE)
    res, caps = hand_batch(segs, "cpu", max_pes)
    ix = esindex.index_batch(res, caps, max_nal=max_nal)
    assert ix.nal[0, :7, 3].tolist() == [-1, -1, 1, 2, 4, 4, 4]  # 201 twice: the later unit owns the NAL
    assert ix.au[0, 3].tolist() == [-1, 0, 0, 0] and ix.au[0, 4, :2].tolist() == [4, 3]
    assert ix.sinfo[1, S["n_au"]] == 8
    assert int(ix.sinfo[3, S["status"]]) == ST["unsupported_video"] and ix.sinfo[3, S["n_au"]] == 0

    segs, max_pes, max_nal = CASES["adts"](TILE)
    res, caps = hand_batch(segs, "cpu", max_pes)
    ix = esindex.index_batch(res, caps, max_nal=max_nal)
    err = [(int(x) & ST["adts_error"]) != 0 for x in ix.sinfo[:, S["status"]]]
    assert err == [False, False, True, True, True, False, False, False]
    assert ix.sinfo[:, S["n_adts_frames"]].tolist() == [6, 4, 3, 2, 2, 4, 0, 5]
    assert ix.sinfo[0, S["audio_sample_rate"]:].tolist() == [48000, 2]
    assert ix.sinfo[1, S["audio_sample_rate"]:].tolist() == [44100, 6]
    assert ix.aframes[2, :3, 0].tolist() == [2, 0, 1] and ix.aframes[6, 0, 0] == -1


def test_no_row_is_written_past_the_tables():
    """65 and 200 NALs into tables of 64 rows, with sentinel rows behind every table."""
    segs, max_pes, max_nal = CASES["overflow"](TILE)
    res, caps = hand_batch(segs, "cpu", max_pes)
    B = len(segs)
    nal = np.full((B * max_nal + 1, 4), 0x5A5A5A5A, np.int32)
    au = np.full((B * max_pes + 1, 4), 0x5A5A5A5A, np.int32)
    af = np.full((B * max_pes + 1, 2), 0x5A5A5A5A, np.int32)
    sinfo = np.full((B + 1, 8), 0x5A5A5A5A, np.int64)
    runtime().index_batch(res.es.numpy(), res.es_offs, np.asarray(caps, np.int64), res.info.numpy(), res.pes.numpy(),
                          max_pes, max_nal, nal, au, af, sinfo)
    for t in (nal, au, af, sinfo):
        assert (t[-1] == 0x5A5A5A5A).all()
    ref = ref_batch(res, caps, max_nal)
    assert np.array_equal(nal[:-1].reshape(B, max_nal, 4), ref[0]) and np.array_equal(sinfo[:-1], ref[3])


def test_ranges_are_checked_before_anything_runs():
    res, caps = hand_batch(CASES["zero_runs"](TILE)[0], "cpu")
    with pytest.raises(ValueError, match="out of bounds"):
        esindex.index_batch(res, [res.es.numel() + 1])
    with pytest.raises(ValueError, match="negative"):
        esindex.index_batch(res, [-1])
    with pytest.raises(ValueError, match="max_nal"):
        esindex.index_batch(res, caps, max_nal=0)


def _demux_cpu(segs):
    offs, pos = [], 0
    for s in segs:
        offs.append(pos)
        pos += (len(s) + 255) // 256 * 256
    buf = np.zeros(pos + 256, np.uint8)
    for o, s in zip(offs, segs):
        buf[o:o + len(s)] = np.frombuffer(s, np.uint8)
    lens = [len(s) for s in segs]
    return tsdemux.demux_batch(torch.from_numpy(buf), offs, lens, torch.zeros(pos + 256, dtype=torch.uint8), offs), lens


def test_synthetic_segment_end_to_end():
    """The packager's payloads are non-zero, so the counts are known: 25 fps x 0.4 s = 10 access
    units, AUD + SPS + PPS + IDR in the first and AUD + slice in the other nine."""
    seg, st = tsdemux.mux_segment(duration=0.4, target_bytes=188 * 300)
    res, lens = _demux_cpu([bytes(seg)])
    ix = esindex.index_batch(res, lens)
    assert_index_equal(ix, ref_batch(res, lens, esindex.DEFAULT_MAX_NAL))
    s = ix.segment(0)
    assert s["status"] == 0 and s["n_au"] == 10 and s["n_nal"] == 4 + 2 * 9
    F = esindex.AU_FLAGS
    assert s["au"][0, 2] == F["keyframe"] | F["sps"] | F["pps"] | F["aud"] and s["au"][0, :2].tolist() == [0, 4]
    assert (s["au"][1:, 2] == F["aud"]).all() and (s["au"][1:, 1] == 2).all()
    assert s["independent"] and s["n_keyframe_aus"] == 1 and s["first_keyframe_au"] == 0
    n_frames = max(1, int(0.4 * 48000 / 1024))  # the packager's frame count
    assert s["n_adts_frames"] == n_frames and s["aframes"][:, 0].sum() == n_frames
    assert s["aframes"][:, 1].sum() == st["es_bytes"][1]  # every audio byte consumed: a clean walk
    assert (s["audio_sample_rate"], s["audio_channels"]) == (48000, 2)


def _spec_stream(video_type: int, units, audio_units):
    """A TS built with ``ts_builder._Muxer`` whose video PES payloads are the given NAL
    layouts; returns the stream."""
    VPID, APID, PMTPID = 0x100, 0x101, 0x1000
    m = _Muxer()
    pat = _section(0x00, 1, bytes([0, 1, 0xE0 | (PMTPID >> 8), PMTPID & 0xFF]))
    streams = b""
    for st, pid in ((video_type, VPID), (0x0F, APID)):
        streams += bytes([st, 0xE0 | (pid >> 8), pid & 0xFF, 0xF0, 0x00])
    pmt = _section(0x02, 1, bytes([0xE0 | (VPID >> 8), VPID & 0xFF, 0xF0, 0x00]) + streams)
    m.psi(0, pat)
    m.psi(PMTPID, pmt)
    t0 = 900_000
    for i, payload in enumerate(units):
        m.pes(VPID, _pes(0xE0, payload, t0 + 3600 * i + 3600, t0 + 3600 * i, length_field=False))
        if i < len(audio_units):
            m.pes(APID, _pes(0xC0, audio_units[i], t0 + 1920 * i))
    return b"".join(m.packets)


@pytest.mark.parametrize("video_type", [0x1B, 0x24])
def test_spec_built_stream_end_to_end(video_type):
    """NAL layouts of our choosing through a spec-built TS (4-byte and 3-byte start codes, a
    trailing-zero run, an empty NAL, a unit that begins mid-NAL), H.264 and HEVC."""
    rng = np.random.default_rng(video_type)

    def nal(header: int, size: int, four: bool = True) -> bytes:
        return (b"\x00" if four else b"") + SC + bytes([header]) + bytes(background(rng, size))

    if video_type == 0x1B:
        aud, sps, pps, idr, non = 0x09, 0x67, 0x68, 0x65, 0x41
    else:
        aud, sps, pps, idr, non = 35 << 1, 33 << 1, 34 << 1, 19 << 1, 1 << 1
    units = [nal(aud, 1) + nal(sps, 12) + nal(pps, 5, four=False) + nal(idr, 3000),
             nal(aud, 1) + nal(non, 700) + b"\x00\x00\x00",            # trailing zeros stay in the NAL
             nal(aud, 1) + SC + nal(non, 400, four=False),              # an empty NAL
             bytes(background(rng, 300)),                               # a unit that continues the NAL before
             nal(aud, 1) + nal(idr, 900)]
    audio = [adts_frame(bytes(background(rng, 100))) + adts_frame(bytes(background(rng, 90))) for _ in range(4)]
    res, lens = _demux_cpu([_spec_stream(video_type, units, audio)])
    assert res.info[0, tsdemux.INFO["status"]] == 0 and res.info[0, tsdemux.INFO["video_type"]] == video_type
    ix = esindex.index_batch(res, lens)
    assert_index_equal(ix, ref_batch(res, lens, esindex.DEFAULT_MAX_NAL))
    s = ix.segment(0)
    F = esindex.AU_FLAGS
    assert s["status"] == 0 and s["n_au"] == 5 and s["n_nal"] == 4 + 2 + 3 + 0 + 2
    assert s["au"][:, 1].tolist() == [4, 2, 3, 0, 2] and s["au"][3, 0] == -1
    assert s["au"][:, 2].tolist() == [15, F["aud"], F["aud"], 0, F["aud"] | F["keyframe"]]
    assert s["n_keyframe_aus"] == 2 and s["independent"] and s["n_adts_frames"] == 8


# ---------------------------------------------------------------- pipeline and player
def _mixed_jobs():
    key = bytes(range(16))
    out = []
    for i, (nbytes, enc) in enumerate([(188 * 400, True), (188 * 300, False), (188 * 500, True), (188 * 350, False)]):
        seg, _ = tsdemux.mux_segment(duration=0.8, target_bytes=nbytes, seed=20 + i, sn=i)
        iv = aes.iv_from_sn(i)
        out.append((bytes(seg), aes.cbc_encrypt(key, iv, seg) if enc else seg, key if enc else None,
                    iv if enc else None))
    return out


def run_pipeline(device, ask):
    """One batch through a pipeline; ``ask[n]``: job n wants the index.  Returns the results."""
    pipe = MediaPipeline(torch.device(device), new_event_loop("virtual"))
    out = {}
    jobs = _mixed_jobs()
    for n, (_, payload, key, iv) in enumerate(jobs):
        pipe.submit(TransmuxJob(torch.from_numpy(np.array(payload)), key, iv, lambda r, n=n: out.__setitem__(n, r),
                                index=ask[n]))
    pipe.flush()
    return jobs, out


def check_samples(jobs, out, ask):
    for n, (seg, _, _, _) in enumerate(jobs):
        r = out[n]
        assert r.get("error") is None and r["status"] == 0
        assert ("samples" in r) == ask[n]
        if not ask[n]:
            continue
        res, lens = _demux_cpu([seg])
        nal, au, af, sinfo = (t[0] for t in ref_batch(res, lens, esindex.DEFAULT_MAX_NAL))
        s = r["samples"]
        assert isinstance(s, Samples)
        assert [s[k] for k in esindex.SINFO] == sinfo.tolist()
        assert s["independent"] is True and s["n_au"] == 20 and "nal" in s and s.get("nope") is None
        assert np.array_equal(s["nal"].cpu().numpy(), nal) and np.array_equal(s["au"].cpu().numpy(), au)
        assert np.array_equal(s["aframes"].cpu().numpy(), af)
        with pytest.raises(TypeError):
            s["n_nal"] = 0  # read-only


def test_pipeline_indexes_only_the_jobs_that_ask():
    ask = [True, False, False, True]
    jobs, out = run_pipeline("cpu", ask)
    check_samples(jobs, out, ask)
    _, plain = run_pipeline("cpu", [False] * 4)
    for n in (1, 2):  # jobs that did not ask: the result a pipeline without the feature gives
        a, b = out[n], plain[n]
        assert dict(a).keys() == dict(b).keys()
        assert a["status"] == b["status"] and a["plain_bytes"] == b["plain_bytes"] and a["index"] == b["index"]
        assert a["info"].to_dict() == b["info"].to_dict()
        assert torch.equal(a["video"], b["video"]) and torch.equal(a["audio"], b["audio"])


@pytest.fixture
def fresh():
    clear_origins()
    set_current_node(None)
    yield
    clear_origins()
    set_current_node(None)


def _play(config):
    loop = new_event_loop("virtual")
    origin = SyntheticHlsOrigin("http://cdn.esx/vod/", renditions=[Rendition(300_000, 640, 360)], num_segments=4,
                                segment_duration=2.0, encrypted=True)
    hls = Hls(dict(config, transmuxDevice="cpu"), {"streamrootKey": "esx", "gpuSwarm": {"device": "cpu",
                                                                                         "cacheBytes": 32 << 20}})
    media = MediaElement()
    data, parsed = [], []
    hls.on(Hls.Events.FRAG_PARSING_DATA, lambda e, d: data.append(d))
    hls.on(Hls.Events.FRAG_PARSED, lambda e, d: parsed.append(d))
    hls.loadSource(origin.master_url())
    hls.attachMedia(media)
    hls.on(Hls.Events.MANIFEST_PARSED, lambda e, d: media.play())
    assert loop.run_until(lambda: len(parsed) >= 2, timeout_ms=60_000)
    hls.destroy()
    return data, parsed


def test_controller_emits_the_index_only_under_indexSamples(fresh):
    data, parsed = _play({})
    assert all(set(d) == {"frag", "type", "startPTS", "endPTS", "data1", "nb", "pts"} for d in data)
    assert all(set(d) == {"frag"} for d in parsed)
    clear_origins()
    set_current_node(None)
    data, parsed = _play({"indexSamples": True})
    assert len(data) >= 4 and all("samples" in d for d in data)
    video = [d for d in data if d["type"] == "video"]
    assert all(d["samples"]["n_au"] == d["nb"] and d["samples"]["independent"] for d in video)
    assert all(d["independent"] is True for d in parsed)
