"""The moof boxes through the transmux pipeline (``TransmuxJob(fragment=True)``) and through a
player under ``fmp4Fragments``: jobs with and without the boxes in one group, a playlist with
``#EXT-X-DISCONTINUITY`` whose two sides start at unrelated stamps (the second side crosses the
33-bit rollover), and a player with the key off, whose events are what they were."""
import numpy as np
import pytest
import torch

import fragment_cases as fc
import remux_cases as rc
from hlsjs_p2p_wrapper_amd.net import new_event_loop
from hlsjs_p2p_wrapper_amd.net.origin import StaticOrigin
from hlsjs_p2p_wrapper_amd.ops import fragment, remux, tsdemux
from hlsjs_p2p_wrapper_amd.player import Hls, MediaElement, fmp4
from hlsjs_p2p_wrapper_amd.player.transmux import MediaPipeline, TransmuxJob
from test_esindex import _mixed_jobs, fresh  # noqa: F401  (fixture)

# job n of the mixed batch (two encrypted, two clear: each group holds one that asks and one that does not)
PARAMS = {0: dict(sequence_number=11, time_base=1000, time_ref=-1),
          3: dict(sequence_number=2 ** 32 + 12, time_ref=5 * 90000, anchor=True)}


def run_pipeline(device, ask):
    pipe = MediaPipeline(torch.device(device), new_event_loop("virtual"))
    out = {}
    jobs = _mixed_jobs()
    for n, (_, payload, key, iv) in enumerate(jobs):
        kw = dict(fragment=True, **PARAMS[n]) if ask and n in PARAMS else dict(remux=n == 1)
        pipe.submit(TransmuxJob(torch.from_numpy(np.array(payload)), key, iv, lambda r, n=n: out.__setitem__(n, r),
                                **kw))
    pipe.flush()
    return out


def check_pipeline(device):
    out = run_pipeline(device, True)
    plain = run_pipeline(device, False)
    for n in range(4):
        assert out[n].get("error") is None and out[n]["status"] == 0
        assert ("fmp4" in out[n]) == (n != 2) and ("fmp4" in plain[n]) == (n == 1)
    # a job that asked for the remux alone, in a group with a job that asked for the boxes: what it
    # got before, but for the larger A0 that the group's layout implies
    a, b = out[1]["fmp4"], plain[1]["fmp4"]
    assert a.keys() == b.keys() and "time_base" not in a.keys() and a.get("time_base") is None
    gap = fragment.frag_audio_gap(remux.DEFAULT_MAX_AFRAMES)
    for k in remux.RINFO:
        assert a[k] == b[k] + (gap if k == "audio_box_offset" else 0), k
    for t in ("video", "audio"):
        assert a[t].keys() == b[t].keys() and "fragment" not in a[t].keys() and a[t].get("tfdt") is None
        assert torch.equal(a[t]["mdat"], b[t]["mdat"]) and torch.equal(a[t]["samples"], b[t]["samples"])
        assert a[t]["moof"](5) == b[t]["moof"](5) and a[t]["base"] == b[t]["base"]
    assert dict(out[2]).keys() == dict(plain[2]).keys()
    # the jobs that asked
    for n, p in PARAMS.items():
        f = out[n]["fmp4"]
        assert f["video"]["fragment"].device.type == torch.device(device).type
        rate = f["audio"]["timescale"]
        vdts, apts = f["video_base_dts"], f["audio_base_pts"]
        if p.get("anchor"):
            base = min(vdts, apts) - p["time_ref"]
        else:
            base = p["time_base"]
        assert f["time_base"] == base
        want = {"video": vdts - base, "audio": fc.ref_rescale(apts - base, rate)}
        for t in ("video", "audio"):
            track = f[t]
            assert {"fragment", "moof_view", "tfdt"} <= set(track.keys()) and track["tfdt"] == want[t]
            moof, mdat, whole = track["moof_view"], track["mdat"], track["fragment"]
            assert moof.untyped_storage().data_ptr() == mdat.untyped_storage().data_ptr()
            assert moof.data_ptr() + moof.numel() == mdat.data_ptr()  # adjacent: one byte range
            assert whole.data_ptr() == moof.data_ptr() and whole.numel() == moof.numel() + mdat.numel()
            box = fc.walk_fragment(whole.cpu().numpy().tobytes())
            assert box["sequence_number"] == p["sequence_number"] & 0xFFFFFFFF and box["base"] == want[t]
            assert box["count"] == track["nb"] and len(box["mdat_payload"]) == mdat.numel() - 8
            # but for the time, the box the host packer builds
            rows = track["samples"].cpu().numpy()
            host = (fmp4.video_moof(p["sequence_number"], vdts - base, rows) if t == "video" else
                    fmp4.audio_moof(p["sequence_number"], apts - base, rate, rows))
            assert moof.cpu().numpy().tobytes() == host
    return out


def test_pipeline_writes_the_boxes_of_the_jobs_that_ask():
    check_pipeline("cpu")
    with pytest.raises(ValueError, match="time_ref"):
        TransmuxJob(b"", None, None, print, fragment=True, anchor=True)
    j = TransmuxJob(b"", None, None, print, fragment=True)
    assert j.remux and j.index and (j.sequence_number, j.time_base, j.time_ref, j.anchor) == (0, 0, -1, False)


@pytest.mark.gpu
def test_pipeline_on_the_device_equals_the_cpu_pipeline(cuda):
    dev, cpu = check_pipeline(cuda), check_pipeline("cpu")
    for n in PARAMS:
        a, b = dev[n]["fmp4"], cpu[n]["fmp4"]
        assert a["time_base"] == b["time_base"] and [a[k] for k in remux.RINFO] == [b[k] for k in remux.RINFO]
        for t in ("video", "audio"):
            assert a[t]["tfdt"] == b[t]["tfdt"] and torch.equal(a[t]["fragment"].cpu(), b[t]["fragment"])


# ---------------------------------------------------------------- the player
ROLL = 2 ** 33 / 90000.0  # seconds
# (start_time of the packager, seed): two segments, a discontinuity, two segments whose stamps are
# unrelated to the first side's and cross the 33-bit rollover between them
# (the packager's first stamp lies 10 s behind its start_time)
SIDES = (((1000.0, 1), (1002.0, 2)), ((ROLL - 11.5, 3), (ROLL - 9.5, 4)))


def play(config, want=4):
    lines = ["#EXTM3U", "#EXT-X-VERSION:3", "#EXT-X-TARGETDURATION:2", "#EXT-X-MEDIA-SEQUENCE:7"]
    res = {}
    for side, segs in enumerate(SIDES):
        if side:
            lines.append("#EXT-X-DISCONTINUITY")
        for k, (start, seed) in enumerate(segs):
            seg, _ = tsdemux.mux_segment(duration=2.0, target_bytes=188 * 300, seed=seed, sn=2 * side + k,
                                         start_time=start)
            lines += ["#EXTINF:2.0,", f"s{side}{k}.ts"]
            res[f"s{side}{k}.ts"] = np.frombuffer(bytes(seg), np.uint8).copy()
    res["media.m3u8"] = "\n".join(lines + ["#EXT-X-ENDLIST", ""])
    res["master.m3u8"] = "#EXTM3U\n#EXT-X-STREAM-INF:BANDWIDTH=300000,RESOLUTION=640x360\nmedia.m3u8\n"
    StaticOrigin("http://cdn.frag/vod/", res)
    loop = new_event_loop("virtual")
    hls = Hls(dict(config, transmuxDevice="cpu"))
    media_el = MediaElement()
    events, errors = [], []
    E = Hls.Events
    for name in (E.FRAG_PARSING_INIT_SEGMENT, E.FRAG_PARSING_DATA, E.FRAG_PARSED, E.FRAG_BUFFERED):
        hls.on(name, lambda e, d: events.append((e, d)))
    hls.on(E.ERROR, lambda e, d: errors.append(d))
    hls.loadSource("http://cdn.frag/vod/master.m3u8")
    hls.attachMedia(media_el)
    hls.on(E.MANIFEST_PARSED, lambda e, d: media_el.play())
    assert loop.run_until(lambda: sum(e == E.FRAG_BUFFERED for e, _ in events) >= want or errors, timeout_ms=60_000)
    init_pts = dict(hls.streamController._init_pts)
    hls.destroy()
    assert not errors
    return events, init_pts


def test_player_places_fragments_across_a_discontinuity(fresh):  # noqa: F811
    events, init_pts = play({"fmp4Fragments": True})
    data = [d for e, d in events if e == Hls.Events.FRAG_PARSING_DATA]
    assert len(data) == 8 and [d["frag"].cc for d in data] == [0, 0, 0, 0, 1, 1, 1, 1]
    assert sorted(init_pts) == [0, 1]  # one initPTS per discontinuity counter ...
    # ... the first side's is its first stamp (its playlist start is 0), the second side's lies 4 s before its own
    assert init_pts[0] == min(data[0]["pts"][0], data[1]["pts"][0])
    assert init_pts[1] == min(data[4]["pts"][0], data[5]["pts"][0]) - 4 * 90000
    frame = 1 / 25.0
    for d in data:
        frag, moof, mdat, whole = d["frag"], d["data1"], d["data2"], d["fragment"]
        assert frag.start == 2.0 * (frag.sn - 7)
        assert isinstance(moof, torch.Tensor) and moof.untyped_storage().data_ptr() == mdat.untyped_storage().data_ptr()
        assert moof.data_ptr() + moof.numel() == mdat.data_ptr()
        assert whole.data_ptr() == moof.data_ptr() and whole.numel() == moof.numel() + mdat.numel()
        box = fc.walk_fragment(whole.numpy().tobytes())
        scale = 90000 if d["type"] == "video" else 48000
        assert abs(box["base"] / scale - frag.start) <= frame, (frag.sn, d["type"], box["base"] / scale)
        assert d["startDTS"] == box["base"] / scale and d["endDTS"] > d["startDTS"]
        assert abs(d["endDTS"] - (frag.start + 2.0)) <= 2 * frame
        assert box["sequence_number"] == frag.sn and box["count"] == d["nb"] > 0
    # the second side crossed the rollover: its last fragment's raw stamps are small again
    raw = [d["pts"][0] for d in data if d["type"] == "video"]
    assert raw[3] < raw[2] and raw[2] > 2 ** 33 - 2 * 90000


def test_player_with_the_key_off_emits_what_it_did(fresh):  # noqa: F811
    """Without ``fmp4Fragments`` the events are those of ``remuxFmp4``, byte for byte: host moof bytes in
    ``data1`` with the raw stamp, no ``fragment``; and without both keys those of the plain player."""
    def plain(events):
        out = []
        for e, d in events:
            row = {}
            for k, v in d.items():
                if k in ("samples", "tracks", "stats"):
                    row[k] = sorted(v.keys()) if hasattr(v, "keys") else None
                else:
                    row[k] = v.sn if k == "frag" else v.numpy().tobytes() if isinstance(v, torch.Tensor) else v
            out.append((e, row))
        return out

    off, _ = play({"remuxFmp4": True, "fmp4Fragments": False})
    default, pts = play({"remuxFmp4": True})
    assert plain(off) == plain(default) and pts == {}
    data = [d for e, d in off if e == Hls.Events.FRAG_PARSING_DATA]
    assert all(isinstance(d["data1"], bytes) and "fragment" not in d for d in data)
    video = [d for d in data if d["type"] == "video"]
    for d in video:  # the raw stamp: the first DTS, one frame in front of the first PTS
        base = rc.parse_moof(d["data1"])["base"]
        assert base == d["pts"][0] - 3600 and d["startDTS"] == base / 90000
    bare, _ = play({})
    assert all(set(d) == {"frag", "type", "startPTS", "endPTS", "data1", "nb", "pts"}
               for e, d in bare if e == Hls.Events.FRAG_PARSING_DATA)
    on, _ = play({"fmp4Fragments": True})  # the key alone implies the remux
    assert [(e, sorted(d)) for e, d in on if e != Hls.Events.FRAG_PARSING_DATA] == \
        [(e, sorted(d)) for e, d in off if e != Hls.Events.FRAG_PARSING_DATA]
