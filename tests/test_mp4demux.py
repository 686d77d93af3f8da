"""``ops.mp4_demux_batch`` on the host implementation against the independent reference of
``mp4_cases.py``: all ten tensors bit for bit, the source unchanged between its canaries, every
output inside its tensor, the layout names pinned to the runtime's exports, and ``caption_batch``
on the ``as_demux()`` / ``as_index()`` views of an fMP4 batch."""
import numpy as np
import pytest
import torch

import captions_cases as cc
import mp4_cases as mc
from hlsjs_p2p_wrapper_amd.ops import captions, esindex, mp4demux, tsdemux
from hlsjs_p2p_wrapper_amd.ops._native import runtime

PAD = 64  # canary elements behind each output of a raw call
S = mp4demux.MSTATUS


def shapes(B, lim):
    P, N = lim["max_pes"], lim["max_nal"]
    return {"minfo": ((B, 18), np.int64), "msamples": ((B, 2, P, 4), np.int32),
            "runs": ((B, lim["max_run"], 16), np.int64),
            "emsg": ((B, lim["max_emsg"], 12), np.int64), "info": ((B, 24), np.int64), "pes": ((B, 3, P, 3), np.int64),
            "nal": ((B, N, 4), np.int32), "au": ((B, P, 4), np.int32), "aframes": ((B, P, 2), np.int32),
            "sinfo": ((B, 8), np.int64)}


def run_raw(buf, offs, lens, tracks, lim):
    """The runtime's ``mp4_demux_batch`` on outputs with ``PAD`` canary elements behind each."""
    B = len(offs)
    sh = shapes(B, lim)
    flat = {k: np.full(int(np.prod(s)) + PAD, 0x5A, dt) for k, (s, dt) in sh.items()}
    runtime().mp4_demux_batch(buf.numpy(), np.asarray(offs, np.int64), np.asarray(lens, np.int64),
                              mp4demux.pack_tracks(tracks, B), lim["max_pes"], lim["max_nal"], lim["max_moof"],
                              lim["max_run"], lim["max_emsg"], *(flat[k] for k in mc.NAMES))
    for k in sh:
        assert (flat[k][-PAD:] == 0x5A).all(), k
    return {k: flat[k][:-PAD].reshape(s) for k, (s, _) in sh.items()}


@pytest.fixture(scope="module")
def batches():
    out = {}
    for name in mc.CASES:
        buf, offs, lens, tracks, lim = mc.batch(name)
        out[name] = (buf, offs, lens, tracks, lim, mc.ref_batch(buf, offs, lens, tracks, lim))
    return out


def test_layout_names_equal_the_runtime_exports(rt):
    m = mp4demux
    assert m.TRACK == dict(rt.MP4_TRACK) and m.KIND == dict(rt.MP4_KIND) and m.MINFO == dict(rt.MP4_MINFO)
    assert m.MINFO_TRACK == dict(rt.MP4_MINFO_TRACK) and m.MSTATUS == dict(rt.MP4_STATUS)
    assert m.MSAMPLE == dict(rt.MP4_MSAMPLE) and m.RUN == dict(rt.MP4_RUN) and m.EMSG == dict(rt.MP4_EMSG)
    assert (m.TRACKS, m.TRACK_WORDS, m.MINFO_WORDS, m.MINFO_TRACK0, m.MINFO_TRACK_WORDS) == \
        (rt.MP4_TRACKS, rt.MP4_TRACK_WORDS, rt.MP4_MINFO_WORDS, rt.MP4_MINFO_TRACK0, rt.MP4_MINFO_TRACK_WORDS) == \
        (2, 8, 18, 6, 6)
    assert (m.MSAMPLE_WORDS, m.RUN_WORDS, m.EMSG_WORDS, m.MAX_BOX_ROWS) == \
        (rt.MP4_MSAMPLE_WORDS, rt.MP4_RUN_WORDS, rt.MP4_EMSG_WORDS, rt.MP4_MAX_BOX_ROWS) == (4, 16, 12, 256)
    assert (m.DEFAULT_MAX_MOOF, m.DEFAULT_MAX_RUN, m.DEFAULT_MAX_EMSG) == \
        (rt.MP4_DEFAULT_MAX_MOOF, rt.MP4_DEFAULT_MAX_RUN, rt.MP4_DEFAULT_MAX_EMSG) == (64, 128, 16)
    assert sorted(m.MINFO.values()) == list(range(m.MINFO_TRACK0))
    assert sorted(m.MINFO_TRACK.values()) == list(range(m.MINFO_TRACK_WORDS))
    assert m.MINFO_TRACK0 + m.TRACKS * m.MINFO_TRACK_WORDS == m.MINFO_WORDS
    assert sorted(m.MSAMPLE.values()) == list(range(m.MSAMPLE_WORDS)) and max(m.RUN.values()) < m.RUN_WORDS
    assert max(m.EMSG.values()) < m.EMSG_WORDS and max(m.TRACK.values()) < m.TRACK_WORDS
    assert tuple(S[k] for k in ("bad_box", "moof_overflow", "emsg_overflow", "run_overflow", "no_tfdt",
                                "sample_out_of_range", "sample_overflow", "nal_error", "bad_timestamps")) == \
        (mc.BAD_BOX, mc.MOOF_OVERFLOW, mc.EMSG_OVERFLOW, mc.RUN_OVERFLOW, mc.NO_TFDT, mc.OUT_OF_RANGE,
         mc.SAMPLE_OVERFLOW, mc.NAL_ERROR, mc.BAD_TS)
    assert (mc.NAL_OVERFLOW, mc.UNSUPPORTED_VIDEO) == (esindex.SSTATUS["nal_overflow"],
                                                       esindex.SSTATUS["unsupported_video"])
    assert (mc.LIMITS["max_pes"], mc.LIMITS["max_nal"]) == (tsdemux.DEFAULT_MAX_PES, esindex.DEFAULT_MAX_NAL)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_host_equals_the_reference(batches, name):
    buf, offs, lens, tracks, lim, ref = batches[name]
    before = buf.clone()
    got = mp4demux.mp4_demux_batch(buf, offs, lens, tracks, **lim)
    mc.assert_equal(got, ref)
    mc.assert_equal(run_raw(buf, offs, lens, tracks, lim), ref)
    assert torch.equal(buf, before)
    assert got.minfo.device == buf.device and got.msamples.dtype == torch.int32 and got.pes.dtype == torch.int64
    # a length tensor with host caps: lengths beyond the cap and below zero are clamped
    n = torch.tensor(lens, dtype=torch.int64)
    mc.assert_equal(mp4demux.mp4_demux_batch(buf, offs, n + 5, tracks, caps=lens, **lim), ref)


def test_the_cases_hold_what_they_claim(batches):
    """The reference's own figures on the hand-built segments: a builder that planted nothing
    would make every comparison pass."""
    M, T0 = mp4demux.MINFO, mp4demux.MINFO_TRACK0
    h = batches["headers"][5]["minfo"]
    # a box ending at n, at n - 1, one past it; size 0; a 64-bit size; 2^31; size 7; styp; prft + sidx + unknown
    assert h[:9, M["status"]].tolist() == [0, 1, 1, 0, 0, 1, 1, 0, 0]
    assert h[:9, M["n_moof"]].tolist() == [1, 1, 1, 1, 1, 0, 0, 1, 1]
    assert h[:9, T0].tolist() == [2, 2, 2, 2, 2, 0, 0, 2, 2]
    assert (h[9:16, M["status"]] == 1).all() and (h[9:16, T0] == 2).all()       # 1..7 trailing bytes
    assert (h[16:32, M["status"]] == 0).all() and (h[16:32, T0] == 2).all()     # a moof at every offset mod 16
    entries = batches["headers"][5]["runs"][16:32, 0, mp4demux.RUN["entries"]]
    assert sorted(set(o % 16 for o in entries)) == list(range(16))
    assert h[32:37, M["status"]].tolist() == [0, 1, 0, 1, 1] and h[32:37, M["n_moof"]].tolist() == [0, 0, 0, 0, 0]
    f = batches["fields"][5]
    # tfhd subsets: the size comes from tfhd (5) or trex (4), the duration from tfhd (512) or trex (1001)
    ms = f["msamples"][:32, 0, 0]
    assert [int(x) for x in ms[:, 1]] == [512 if m & 4 else 1001 for m in range(32)]
    assert [int(x) for x in f["msamples"][:32, 0, 1, 3]] == [0x10000 if m & 16 else 0x01010000 for m in range(32)]
    assert f["minfo"][32:35, T0 + 1].tolist() == [0xFFFFFFFF, (1 << 32) + 77, -(1 << 63) + 5]
    assert (f["minfo"][:99, M["status"]] & ~(S["sample_out_of_range"] | S["nal_error"]) == 0).all()
    v0, v1 = f["msamples"][101, 0, :3, 2].tolist(), f["msamples"][102, 0, :3, 2].tolist()
    assert v0 == v1 == [-25, -(1 << 31), (1 << 31) - 1]                         # cts is signed in both versions
    assert f["minfo"][103:108, T0].tolist() == [2, 2, 2, 2, 1] and (f["minfo"][103:108, 0] & 1 == 1).all()
    r = batches["runs"][5]
    A = T0 + 6
    assert r["minfo"][3:11, A].tolist() == [5] * 8
    # two trafs in one moof and in two: tfdt on both, missing on the first, on the second, on both
    assert [r["pes"][i, 1, 2, 2] for i in (3, 5, 7, 9)] == [500, 500, 130, 30]
    assert [r["pes"][i, 1, 2, 2] for i in (4, 6, 8, 10)] == [500, 500, 130, 30]
    assert [int(r["minfo"][i, 0]) & 16 for i in range(3, 11)] == [0, 0, 16, 16, 16, 16, 16, 16]
    assert r["minfo"][11, M["n_other_traf"]] == 1 and r["minfo"][11, T0] == 4 and r["minfo"][11, A] == 3
    assert r["minfo"][12:19, A].tolist() == [63, 64, 65, 255, 256, 257, 600]
    assert r["minfo"][18, 0] == S["sample_overflow"] and r["minfo"][12, A + 1] == 1 << 33
    assert r["minfo"][20:23, M["n_run"]].tolist() == [127, 128, 129] and r["minfo"][20:23, 0].tolist() == [0, 0, 8]
    assert r["minfo"][23:26, M["n_moof"]].tolist() == [63, 64, 65] and r["minfo"][23:26, 0].tolist() == [16, 16, 18]
    assert r["minfo"][26, 0] == S["bad_timestamps"]
    assert r["pes"][26, 1, 5, 2] == (1 << 32) - 5 + 3 * 0x7FFFFFFF + (1 << 31) + 0xFFFFFFFF
    k = batches["nal"][5]
    assert k["sinfo"][:5, 1].tolist() == [15, 15, 15, 0, 0] and k["sinfo"][3:5, 0].tolist() == [4, 4]
    assert sorted(set(int(o) % 16 for o in k["pes"][5, 0, :33, 0])) == list(range(16)) and k["sinfo"][5, 1] == 33
    assert k["minfo"][6, 0] == S["nal_error"] and k["sinfo"][6, 1] == 6
    assert k["au"][6, :6, 1].tolist() == [3, 0, 1, 0, 2, 0]
    assert k["sinfo"][7:10, 1].tolist() == [2047, 2048, 2049] and k["sinfo"][7:10, 0].tolist() == [0, 0, 1]
    assert k["nal"][10, :8, 2].tolist() == [35, 33, 34, 39, 19, 1, 21, 40]
    assert k["au"][10, :8, 2].tolist() == [8, 2, 4, 0, 1, 0, 1, 0]
    # 300 samples of seven NAL units: two rounds of the NAL pass, the table full inside the second
    assert k["sinfo"][11, :5].tolist() == [1, 2100, 300, 3, 0] and k["minfo"][11, 0] == 0
    assert k["au"][11, 255:258, 0].tolist() == [1785, 1792, 1799] and k["au"][11, 291:294, :2].tolist() == \
        [[2037, 7], [2044, 4], [-1, 0]]
    assert k["nal"][11, 2047].tolist()[2:] == [1, 292] and k["au"][11, 299, 2] == 0 and k["au"][11, 200, 2] == 1
    buf, offs, lens = batches["nal"][:3]
    assert offs[-1] + lens[-1] > buf.numel() - 4  # the last sample of the last segment ends the buffer
    e = batches["emsg"][5]
    E = mp4demux.EMSG
    assert e["minfo"][:, M["n_emsg"]].tolist() == [14, 17, 1] and e["minfo"][:, 0].tolist() == [1, 4, 0]
    assert e["emsg"][0, :14, E["is_id3"]].tolist() == [1, 1, 0, 0, 0, 0, 0, -1, -1, -1, -1, -1, -1, 1]
    assert e["emsg"][0, 1, E["time"]] == (1 << 40) + 9 and e["emsg"][0, 0, E["time_is_delta"]] == 1
    assert (e["emsg"][1, :, E["id"]] == np.arange(16)).all()


def test_captions_run_on_the_views_unchanged(batches):
    buf, offs, lens, tracks, lim, ref = batches["captions"]
    got = mp4demux.mp4_demux_batch(buf, offs, lens, tracks, **lim)
    res, ix = got.as_demux(), got.as_index()
    assert res.es.data_ptr() == buf.data_ptr() and ix.nal.data_ptr() == got.nal.data_ptr()
    caps = captions.caption_batch(res, ix, lens, max_cc=8)
    cc.assert_captions_equal(caps, cc.ref_batch(res, ix, lens, 8))
    for i in range(2):
        seg = caps.segment(i)
        assert seg["n_samples"] == 5 and seg["status"] == 0
        # presentation order follows dts + cts, in the track's timescale
        assert [s["pts"] for s in seg["samples"]] == sorted(90000 + 3000 * a + c for a, c in
                                                            ((0, 0), (1, 6000), (2, -3000), (4, 0), (5, 9000)))
        assert [len(s["bytes"]) for s in sorted(seg["samples"], key=lambda s: s["au"])] == [5, 8, 11, 17, 20]
    view = got.segment(0)
    assert view["video"]["n_samples"] == 6 and view["audio"]["n_samples"] == 3 and view["video"]["first_sync"] == 0
    assert view["video"]["base_time"] == 90000 and view["audio"]["duration"] == 3 * 1024 and view["emsg"] == []


def test_track_rows_are_what_the_reference_builds():
    """``pack_tracks`` against the reference's own rows: slot order and word layout."""
    hevc = (mc.AUDIO, mc.Mp4Track(9, "video", 0x24, 2, 11, 22, 33))
    for tracks, B in ((mc.AV, 3), (hevc, 1), ([mc.AV, hevc, (mc.AUDIO,)], 3)):
        assert np.array_equal(mp4demux.pack_tracks(tracks, B), mc.track_rows(tracks, B))
    assert mc.track_rows(hevc, 1)[0].tolist() == [[9, 1, 0x24, 2, 11, 22, 33, 0], [2, 2, 0x0F, 0, 0, 0, 0, 0]]


def test_arguments_are_checked():
    buf, offs, lens, tracks, lim = mc.batch("small")
    bad = [dict(max_pes=0), dict(max_run=257), dict(max_moof=0), dict(max_emsg=300), dict(max_nal=-1)]
    for kw in bad:
        with pytest.raises(ValueError, match="max_"):
            mp4demux.mp4_demux_batch(buf, offs, lens, tracks, **{**lim, **kw})
    with pytest.raises(ValueError, match="out of bounds"):
        mp4demux.mp4_demux_batch(buf, offs, [buf.numel()] * 3, tracks, **lim)
    with pytest.raises(ValueError, match="negative"):
        mp4demux.mp4_demux_batch(buf, [-16, 0, 0], lens, tracks, **lim)
    with pytest.raises(ValueError, match="caps"):
        mp4demux.mp4_demux_batch(buf, offs, torch.tensor(lens), tracks, **lim)
    for tk in ((mc.VIDEO, mc.VIDEO), (mc.Mp4Track(1, "video", 0x1B, 3),), (mc.Mp4Track(1, "video", 0x02),),
               (mc.Mp4Track(0, "audio"),), (mc.VIDEO, mc.Mp4Track(1, "audio")), [mc.AV, mc.AV]):
        with pytest.raises(ValueError):
            mp4demux.mp4_demux_batch(buf, offs, lens, tk, **lim)
    empty = mp4demux.mp4_demux_batch(buf, [], [], mc.AV, **lim)
    assert empty.minfo.shape == (0, 18) and empty.pes.shape == (0, 3, 8, 3) and empty.runs.shape == (0, 4, 16)
    one = mp4demux.mp4_demux_batch(buf, offs[:1], lens[:1], [mc.AV], **lim)
    mc.assert_equal(one, {k: v[:1] for k, v in mc.ref_batch(buf, offs, lens, tracks, lim).items()})
