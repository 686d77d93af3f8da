"""Remux to fMP4 samples and mdat boxes on the host (``runtime/remux.cpp``): the three tables and
every byte of the output buffer equal the independent sequential reference
(``tests/remux_cases.py``) on the hand-built cases; the conditions those cases exist for are
counted on the reference; the result round-trips to the kept NALs and frame bodies; damaged
rows write nothing outside the tables and regions; the ``moof`` parses; the layout names equal
the runtime's exports."""
import struct

import numpy as np
import pytest
import torch

import remux_cases as rc
from esindex_cases import INFO, SC
from hlsjs_p2p_wrapper_amd.ops import esindex, remux, tsdemux
from hlsjs_p2p_wrapper_amd.ops._native import runtime
from hlsjs_p2p_wrapper_amd.player import fmp4

R = remux.RINFO


@pytest.fixture(scope="module")
def ran():
    """Every case once, on the host."""
    return {name: rc.run_case(name, rc.TILE) for name in rc.CASES}


@pytest.mark.parametrize("case", sorted(rc.CASES))
def test_hand_built_cases_match_the_reference(case, ran):
    _, _, _, _, rx, ref = ran[case]
    rc.assert_remux_equal(rx, ref)


def kept_rows(ix_seg, vtype, m):
    keep = (lambda t: t in rc.H264_KEPT) if vtype == 0x1B else (lambda t: t >= 0 and t not in rc.HEVC_DROPPED)
    return [(int(s), int(ln)) for s, ln, t, a in ix_seg["nal"] if 0 <= a < m and ln > 0 and keep(int(t))]


def test_alignment_walk_meets_every_alignment(ran):
    """Counted on the reference: a NAL body starts at every output residue mod 16 from every
    source residue mod 4, and a length prefix starts 1, 2 and 3 bytes before a 16-byte edge."""
    _, res, _, ix, _, ref = ran["alignment"]
    rows = kept_rows(ix.segment(0), 0x1B, 6)
    assert [ln for _, ln in rows] == [1 + k % 40 for k in range(240)]
    combos, prefixes, d = set(), set(), 8
    for s, ln in rows:
        prefixes.add(d % 16)
        combos.add(((d + 4) % 16, (int(res.es_offs[0]) + s) % 4))
        d += 4 + ln
    assert combos == {(a, b) for a in range(16) for b in range(4)}
    assert {13, 14, 15} <= prefixes
    assert d == 8 + int(ref[0][0, R["video_payload_bytes"]])


def test_tile_edge_bodies_begin_and_end_around_the_tile(ran):
    T = rc.TILE
    _, _, _, ix, _, ref = ran["tile_edges"]
    begins, ends, totals = set(), set(), []
    for i in range(6):
        d = 8
        for s, ln in kept_rows(ix.segment(i), 0x1B, 2):
            begins.add(d + 4)
            ends.add(d + 4 + ln)
            d += 4 + ln
        totals.append(d)
        assert d == 8 + int(ref[0][i, R["video_payload_bytes"]])
    assert {T - 1, T, T + 1} <= begins and {T - 1, T, T + 1} <= ends
    assert totals == [2 * T + 40] * 5 + [2 * T + 41]
    assert (totals[0] - 8) % 16 == 0 and (totals[5] - 8) % 16 == 1


def test_dropped_nals_leave_rows_and_offsets_in_order(ran):
    _, _, _, ix, rx, _ = ran["dropping"]
    s = rx.segment(0)
    nal = ix.segment(0)["nal"]
    assert nal[0, 3] == -1 and nal[1, 3] == -1  # in front of the first PES
    v = s["vsamples"]
    assert s["n_vsamples"] == 5 and s["status"] == 0
    assert v[:, 1].tolist() == [4 * 3 + 9 + 4 + 50, 0, 4 + 33, 4 + 1, 4 * 2 + 7 + 21]
    assert v[:, 0].tolist() == np.concatenate([[0], np.cumsum(v[:-1, 1])]).tolist()
    assert v[:, 4].tolist() == [rc.SYNC] + [rc.NON_SYNC] * 4
    assert s["video_payload_bytes"] == int(v[:, 1].sum())


def test_codecs(ran):
    _, _, _, _, rx, _ = ran["codecs"]
    avc, hevc, mpeg2 = (rx.segment(i) for i in range(3))
    assert avc["status"] == 0 and hevc["status"] == 0 and mpeg2["status"] == remux.RSTATUS["unsupported_video"]
    # H.264 reads the nine header bytes as types 6 0 2 4 6 | 8 10 12 2; HEVC keeps all but 35..38
    assert avc["vsamples"][:, 1].tolist() == [4 + 5 + 4 + 17, 4 + 8]
    assert hevc["vsamples"][:, 1].tolist() == [4 * 4 + 5 + 8 + 11 + 14, 4 + 11]
    assert hevc["vsamples"][0, 4] == rc.SYNC and avc["vsamples"][0, 4] == rc.NON_SYNC
    assert mpeg2["video_mdat"] == struct.pack(">I4s", 8, b"mdat") and mpeg2["n_vsamples"] == 0
    assert mpeg2["n_aframes"] == 3 and mpeg2["audio_mdat"] == avc["audio_mdat"] and len(avc["audio_mdat"]) > 8


def test_overflow_bits(ran):
    _, _, _, _, rx, _ = ran["nal_overflow"]
    assert rx.rinfo[:, R["status"]].tolist() == [1, 1, 0, 0]
    _, _, _, _, rx, _ = ran["audio_overflow"]
    assert rx.rinfo[:, R["status"]].tolist() == [0, 0, 2, 2]
    assert rx.rinfo[:, R["n_aframes"]].tolist() == [3, 4, 5, 9]
    assert [len(rx.segment(i)["asamples"]) for i in range(4)] == [3, 4, 4, 4]


def test_timestamps(ran):
    _, _, _, _, rx, _ = ran["timestamps"]
    reorder, early, back, wide, one, none = (rx.segment(i) for i in range(6))
    assert reorder["status"] == 0 and reorder["vsamples"][:, 2].tolist() == [3600] * 5
    assert reorder["vsamples"][:, 3].tolist() == [3600, 3 * 3600, 0, 0, 3600]
    assert early["vsamples"][:, 3].tolist() == [-1500] * 5 and early["status"] == 0
    assert back["status"] == remux.RSTATUS["bad_timestamps"]
    assert back["vsamples"][:, 2].tolist() == [3000, 6000, 0, 6000, 6000]
    assert wide["status"] == remux.RSTATUS["bad_timestamps"]
    assert wide["vsamples"][:, 2].tolist() == [1, 0, 1, 1, 1] and wide["vsamples"][:, 3].tolist()[:3] == [0, 0, 0]
    assert one["n_vsamples"] == 1 and one["vsamples"][0, 2:4].tolist() == [0, 7] and one["video_base_dts"] == 900000
    assert none["n_vsamples"] == 0 and none["video_base_dts"] == -1 and none["video_payload_bytes"] == 0


def test_audio_payload_is_the_counted_frames(ran):
    segs, _, _, ix, rx, _ = ran["adts"]
    for i, s in enumerate(segs):
        got, idx = rx.segment(i), ix.segment(i)
        want_frames = idx["n_adts_frames"] if s["atype"] == 0x0F else 0
        assert got["n_aframes"] == want_frames == len(got["asamples"])
        bodies, audio = b"", s["audio"]
        if s["atype"] == 0x0F:
            starts = s["apes"][:4]
            for k, (frames, _) in enumerate(idx["aframes"]):
                q = starts[k]
                for _ in range(frames):
                    ln = ((audio[q + 3] & 3) << 11) | (audio[q + 4] << 3) | (audio[q + 5] >> 5)
                    bodies += audio[q + (7 if audio[q + 1] & 1 else 9):q + ln]
                    q += ln
        assert got["audio_mdat"] == struct.pack(">I4s", 8 + len(bodies), b"mdat") + bodies
    assert [rx.segment(i)["n_aframes"] for i in range(len(segs))] == [6, 4, 3, 2, 2, 4, 0, 5]


@pytest.mark.parametrize("case", ["alignment", "dropping", "codecs", "nal_overflow", "adts", "mixed"])
def test_round_trip(case, ran):
    """On the result itself: a sample's length-prefixed units joined by start codes are the kept
    NALs' bytes of the video ES, and the asamples ranges are the audio box's payload."""
    segs, res, caps, ix, rx, _ = ran[case]
    es = res.es.numpy()
    for i, s in enumerate(segs):
        got, idx = rx.segment(i), ix.segment(i)
        V = es[int(res.es_offs[i]):int(res.es_offs[i]) + caps[i]].tobytes()
        m = got["n_vsamples"]
        payload = got["video_mdat"][8:]
        assert int(got["vsamples"][:, 1].sum()) == len(payload)
        for a in range(m):
            off, size = (int(x) for x in got["vsamples"][a, :2])
            units, p = [], off
            while p < off + size:
                ln = struct.unpack_from(">I", payload, p)[0]
                units.append(payload[p + 4:p + 4 + ln])
                p += 4 + ln
            assert p == off + size
            rows = [] if s["vtype"] not in (0x1B, 0x24) else \
                [(st, ln) for st, ln, t, unit in idx["nal"] if unit == a and ln > 0 and
                 (t in rc.H264_KEPT if s["vtype"] == 0x1B else t not in rc.HEVC_DROPPED)]
            assert SC.join(units) == SC.join(V[st:st + ln] for st, ln in rows)
        body = got["audio_mdat"][8:]
        assert b"".join(body[o:o + n] for o, n in got["asamples"].tolist()) == body


# ---------------------------------------------------------------- damaged rows
def test_fuzzed_rows_stay_inside_tables_and_regions():
    """Random ES bytes with random, partly damaged ``pes`` / ``info`` rows through the host index
    and the host remux with sentinels around every output: nothing outside changes, and the
    sample sizes add up to the payload."""
    rng = np.random.default_rng(31)
    rt = runtime()
    max_pes, max_nal, max_af, guard = 6, 24, 5, 64
    for _ in range(300):
        cap = int(rng.integers(0, 400))
        es = rng.integers(0, 256, cap, dtype=np.uint8)
        if cap:
            es[rng.random(cap) < 0.5] = 0
            es[rng.random(cap) < 0.15] = 1
            es[rng.random(cap) < 0.05] = 0xFF
        wild = lambda n: rng.choice([-1, 0, 1, cap // 2, cap, cap + 1, 2 ** 31, -2 ** 40, 2 ** 62],  # noqa: E731
                                    size=n).astype(np.int64)
        info = np.zeros((1, tsdemux.INFO_WORDS), np.int64)
        info[0] = wild(tsdemux.INFO_WORDS)
        info[0, INFO["video_type"]] = rng.choice([0x1B, 0x24, 0x02])
        info[0, INFO["audio_type"]] = rng.choice([0x0F, 0x0F, 0x03])
        if rng.random() < 0.7:
            info[0, INFO["video_bytes"]] = rng.integers(0, cap + 1)
            info[0, INFO["audio_es_offset"]] = info[0, INFO["video_bytes"]]
            info[0, INFO["audio_bytes"]] = cap - info[0, INFO["video_bytes"]]
            info[0, INFO["n_video_pes"]] = rng.integers(0, max_pes + 3)
            info[0, INFO["n_audio_pes"]] = rng.integers(0, max_pes + 3)
        pes = np.sort(rng.integers(0, cap + 2, (1, 3, max_pes, 3)), axis=2).astype(np.int64)
        damaged = rng.random(pes.shape) < 0.2
        pes[damaged] = wild(int(damaged.sum()))
        eo, caps = np.zeros(1, np.int64), np.array([cap], np.int64)
        nal, au = np.empty((1, max_nal, 4), np.int32), np.empty((1, max_pes, 4), np.int32)
        af, sinfo = np.empty((1, max_pes, 2), np.int32), np.empty((1, 8), np.int64)
        rt.index_batch(es, eo, caps, info, pes, max_pes, max_nal, nal, au, af, sinfo)
        region = rc.out_bytes(cap, max_nal)

        def guarded(n, dtype):
            return np.full(n + 2 * guard, 0x5A5A5A5A5A5A5A5A if dtype == np.int64 else 0x5A5A5A5A if dtype == np.int32
                           else 0x5A, dtype)

        vs, asamp, rinfo = guarded(max_pes * 5, np.int32), guarded(max_af * 2, np.int32), guarded(8, np.int64)
        out = guarded(region, np.uint8)
        rt.remux_batch(es, eo, caps, info, pes, max_pes, max_nal, nal, au, af, sinfo, max_af, vs[guard:-guard],
                       asamp[guard:-guard], rinfo[guard:-guard], out, np.array([guard], np.int64))
        for t in (vs, asamp, rinfo, out):
            assert (t[:guard] == t[0]).all() and (t[-guard:] == t[0]).all() and t[0] == t[-1]
        ri = rinfo[guard:-guard]
        P, m, A0, Q = (int(ri[R[k]]) for k in ("video_payload_bytes", "n_vsamples", "audio_box_offset",
                                                "audio_payload_bytes"))
        rows = vs[guard:-guard].reshape(max_pes, 5)
        assert int(rows[:m, 1].sum()) == P and 0 <= m <= max_pes
        assert A0 == (8 + P + 15) // 16 * 16 and A0 + 8 + Q <= region
        body = out[guard:guard + region]
        assert body[:8].tobytes() == struct.pack(">I4s", 8 + P, b"mdat")
        assert body[A0:A0 + 8].tobytes() == struct.pack(">I4s", 8 + Q, b"mdat")
        assert (body[8 + P:A0] == 0x5A).all() and (body[A0 + 8 + Q:] == 0x5A).all()
        arows = asamp[guard:-guard].reshape(max_af, 2)
        n_rec = int((arows[:, 0] >= 0).sum())
        assert int(arows[:n_rec, 1].sum()) == Q


# ---------------------------------------------------------------- moof
def test_video_moof(ran):
    _, _, _, _, rx, _ = ran["timestamps"]
    for i, seq in ((0, 7), (1, 8), (4, 2 ** 32 - 1), (5, 1)):
        s = rx.segment(i)
        data = fmp4.video_moof(seq, s["video_base_dts"], s["vsamples"])
        f = rc.parse_moof(data)
        assert f["sequence_number"] == seq and f["track"] == 1 and f["tfhd_flags"] == 0x020000
        assert f["base"] == max(s["video_base_dts"], 0) and f["trun_version"] == 1
        assert f["count"] == s["n_vsamples"] and f["data_offset"] == len(data) + 8
        assert sum(r["size"] for r in f["samples"]) == len(s["video_mdat"]) - 8
        assert [r["cts"] for r in f["samples"]] == s["vsamples"][:, 3].tolist()
        assert [r["duration"] for r in f["samples"]] == s["vsamples"][:, 2].tolist()
        assert [r["flags"] for r in f["samples"]] == ([rc.SYNC] + [rc.NON_SYNC] * 4)[:s["n_vsamples"]]
    assert [r["cts"] for r in rc.parse_moof(fmp4.video_moof(1, 0, rx.segment(1)["vsamples"]))["samples"]] == [-1500] * 5


def test_audio_moof(ran):
    _, _, _, ix, rx, _ = ran["adts"]
    for i, rate in ((0, 48000), (1, 44100)):
        s = rx.segment(i)
        assert ix.segment(i)["audio_sample_rate"] == rate
        data = fmp4.audio_moof(3, s["audio_base_pts"], rate, s["asamples"])
        f = rc.parse_moof(data)
        assert f["track"] == 2 and f["default_duration"] == 1024 and f["default_flags"] == rc.SYNC
        assert f["base"] == round(s["audio_base_pts"] * rate / 90000) and s["audio_base_pts"] == 90000
        assert f["count"] == len(s["asamples"]) and f["data_offset"] == len(data) + 8
        assert sum(r["size"] for r in f["samples"]) == len(s["audio_mdat"]) - 8
        assert set(f["samples"][0]) == {"size"}
    assert fmp4.audio_base(90001, 44100) == 44100 and fmp4.audio_base(12345678, 44100) == round(12345678 * 0.49)
    assert rc.parse_moof(fmp4.audio_moof(1, -1, 0, np.zeros((0, 2), np.int32)))["count"] == 0


# ---------------------------------------------------------------- layout
def test_layout_names_equal_the_runtime_exports():
    rt = runtime()
    assert remux.RINFO == dict(rt.ES_RINFO) and remux.RINFO_WORDS == rt.ES_RINFO_WORDS
    assert remux.RSTATUS == dict(rt.ES_RSTATUS) and remux.SAMPLE_FLAGS == dict(rt.ES_SAMPLE_FLAGS)
    assert remux.DEFAULT_MAX_AFRAMES == rt.ES_DEFAULT_MAX_AFRAMES and remux.OUT_ALIGN == rt.ES_OUT_ALIGN
    assert rc.TILE == rt.ES_REMUX_TILE
    for cap, max_nal, max_af, n in ((0, 1, 1, 1), (3_000_000, 2048, 1024, 64), (77, 5, 3, 0)):
        assert remux.remux_out_bytes(cap, max_nal) == int(rt.remux_out_bytes(cap, max_nal)) == cap + max_nal + 32
        assert remux.remux_scratch_words(n, max_nal, max_af) == rt.remux_scratch_words(n, max_nal, max_af)
    caps = np.array([0, 1000, 255, 4096])
    offs, size = remux.layout_out(caps, 64)
    assert (offs % 256 == 0).all() and offs[0] == 0
    assert (np.diff(np.append(offs, size)) >= remux.remux_out_bytes(caps, 64)).all()


def test_region_holds_the_real_output_of_every_case(ran):
    for name, (_, _, caps, ix, _, ref) in ran.items():
        rinfo = ref[0]
        for i, cap in enumerate(caps):
            used = int(rinfo[i, R["audio_box_offset"]] + 8 + rinfo[i, R["audio_payload_bytes"]])
            assert remux.remux_out_bytes(cap, ix.nal.shape[1]) >= used, (name, i)


def test_rejections_on_the_host():
    segs, max_pes, max_nal, _ = rc.CASES["dropping"](rc.TILE)
    res, caps, ix = rc.build(segs, max_pes, max_nal)
    offs, size = remux.layout_out(caps, max_nal)
    out = torch.zeros(size, dtype=torch.uint8)
    with pytest.raises(ValueError, match="out of bounds"):
        remux.remux_batch(res, ix, caps, out[:int(offs[-1]) + caps[-1] + max_nal + 31], offs)
    res2, caps2, ix2 = rc.build(segs + segs, max_pes, max_nal)
    with pytest.raises(ValueError, match="overlap"):
        remux.remux_batch(res2, ix2, caps2, torch.zeros(2 * size, dtype=torch.uint8), [0, 256])
    with pytest.raises(ValueError, match="max_aframes"):
        remux.remux_batch(res, ix, caps, out, offs, max_aframes=0)
    with pytest.raises(ValueError, match="uint8"):
        remux.remux_batch(res, ix, caps, out.to(torch.int32), offs)
    other = esindex.index_batch(res, caps, max_nal=16)
    with pytest.raises(ValueError, match="out of bounds"):
        remux.remux_batch(res, other, caps, out[:caps[0] + 16 + 31], [0])


# ---------------------------------------------------------------- pipeline and player
def run_pipeline(device, ask):
    """One mixed encrypted / clear batch through a pipeline; ``ask[n]``: job n wants the remux."""
    from hlsjs_p2p_wrapper_amd.net.event_loop import new_event_loop
    from hlsjs_p2p_wrapper_amd.player.transmux import MediaPipeline, TransmuxJob
    from test_esindex import _mixed_jobs

    pipe = MediaPipeline(torch.device(device), new_event_loop("virtual"))
    out = {}
    jobs = _mixed_jobs()
    for n, (_, payload, key, iv) in enumerate(jobs):
        pipe.submit(TransmuxJob(torch.from_numpy(np.array(payload)), key, iv, lambda r, n=n: out.__setitem__(n, r),
                                remux=ask[n]))
    pipe.flush()
    return jobs, out


def check_fmp4(jobs, out, ask):
    """The jobs that asked carry the reference's boxes and rows; the others carry no ``fmp4``."""
    from hlsjs_p2p_wrapper_amd.player.transmux import Fmp4
    from test_esindex import _demux_cpu

    for n, (seg, _, _, _) in enumerate(jobs):
        r = out[n]
        assert r.get("error") is None and r["status"] == 0
        assert ("fmp4" in r) == ask[n] and ("samples" in r) == ask[n]
        if not ask[n]:
            continue
        res, lens = _demux_cpu([seg])
        ix = esindex.index_batch(res, lens)
        tables = (t[0].numpy() for t in (ix.nal, ix.au, ix.aframes, ix.sinfo))
        rinfo, vs, asamp, region = rc.ref_segment(res.es[:lens[0]].numpy().tobytes(), lens[0], res.info[0].numpy(),
                                                  res.pes[0].numpy(), *tables, 1024)
        f = r["fmp4"]
        assert isinstance(f, Fmp4) and [f[k] for k in remux.RINFO] == rinfo.tolist() and f.get("nope") is None
        P, A0, Q = (int(rinfo[R[k]]) for k in ("video_payload_bytes", "audio_box_offset", "audio_payload_bytes"))
        v, a = f["video"], f["audio"]
        assert v["mdat"].cpu().numpy().tobytes() == region[:8 + P] and P > 0
        assert a["mdat"].cpu().numpy().tobytes() == region[A0:A0 + 8 + Q] and Q > 0
        assert v["nb"] == 20 and np.array_equal(v["samples"].cpu().numpy(), vs[:20])
        n_af = int(rinfo[R["n_aframes"]])
        assert a["nb"] == n_af and np.array_equal(a["samples"].cpu().numpy(), asamp[:n_af])
        mv, ma = rc.parse_moof(v["moof"](n + 1)), rc.parse_moof(a["moof"](n + 1))
        assert v["moof"](n + 1) is v["moof"](n + 1) and mv["sequence_number"] == n + 1
        assert mv["base"] == rinfo[R["video_base_dts"]] == v["base"] and mv["count"] == 20
        assert sum(s["size"] for s in mv["samples"]) == P and sum(s["size"] for s in ma["samples"]) == Q
        rate = int(ix.sinfo[0, esindex.SINFO["audio_sample_rate"]])
        assert ma["base"] == fmp4.audio_base(int(rinfo[R["audio_base_pts"]]), rate) == a["base"] and rate > 0
        assert a["timescale"] == rate and v["timescale"] == 90000 and a["duration"] == 1024 * n_af
        assert v["duration"] == int(vs[:20, 2].sum())
        with pytest.raises(TypeError):
            f["video"] = None  # read-only


def test_pipeline_remuxes_only_the_jobs_that_ask():
    ask = [True, False, False, True]
    jobs, out = run_pipeline("cpu", ask)
    check_fmp4(jobs, out, ask)
    _, plain = run_pipeline("cpu", [False] * 4)
    for n in (1, 2):  # jobs that did not ask: the result a pipeline without the feature gives
        a, b = out[n], plain[n]
        assert dict(a).keys() == dict(b).keys()
        assert a["status"] == b["status"] and a["plain_bytes"] == b["plain_bytes"] and a["index"] == b["index"]
        assert a["info"].to_dict() == b["info"].to_dict()
        assert torch.equal(a["video"], b["video"]) and torch.equal(a["audio"], b["audio"])


from test_esindex import fresh  # noqa: E402,F401  (fixture)


def test_controller_emits_fmp4_only_under_remuxFmp4(fresh):  # noqa: F811
    from hlsjs_p2p_wrapper_amd.agent import set_current_node
    from hlsjs_p2p_wrapper_amd.net import clear_origins
    from test_esindex import _play

    def plain(events):
        return [{k: (v.sn if k == "frag" else v.numpy().tobytes() if k == "data1" else v) for k, v in d.items()}
                for d in events]

    before, parsed_before = _play({})
    clear_origins()
    set_current_node(None)
    off, parsed_off = _play({"remuxFmp4": False})
    assert plain(off) == plain(before) and [set(d) for d in parsed_off] == [set(d) for d in parsed_before]
    assert all(set(d) == {"frag", "type", "startPTS", "endPTS", "data1", "nb", "pts"} for d in off)
    clear_origins()
    set_current_node(None)
    on, parsed = _play({"remuxFmp4": True})
    assert len(on) >= 4 and [d["type"] for d in on[:2]] == ["video", "audio"]
    for d, raw in zip(on, off):
        f = rc.parse_moof(d["data1"])
        assert isinstance(d["data1"], bytes) and f["sequence_number"] == d["frag"].sn & 0xFFFFFFFF
        assert f["track"] == (1 if d["type"] == "video" else 2) and f["count"] == d["nb"] > 0
        head = d["data2"][:8].numpy().tobytes()
        assert head[4:] == b"mdat" and struct.unpack(">I", head[:4])[0] == d["data2"].numel()
        assert sum(s["size"] for s in f["samples"]) == d["data2"].numel() - 8
        assert d["endDTS"] > d["startDTS"] >= 0 and "samples" in d
        assert d["startPTS"] == raw["startPTS"] and d["pts"] == raw["pts"]
    assert all(d["independent"] is True for d in parsed)
