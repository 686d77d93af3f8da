"""The packed-audio demux on the host (``runtime/packedaudio.cpp``): all seven tensors equal the
independent reference of ``packedaudio_cases.py`` bit for bit, and the ops behind it (remux, codec
configuration, fragment) give for a packed segment what they give for an audio-only MPEG-TS of the
same frames and stamps.  ``test_packedaudio_gpu.py`` runs the same cases on the device."""
import pytest
import torch

import packedaudio_cases as pc
from hlsjs_p2p_wrapper_amd.ops import codecconfig, esindex, fragment, packedaudio, remux, tsdemux

PA, ST = packedaudio.PAINFO, packedaudio.PASTATUS


def test_python_tables_equal_the_runtime_exports(rt):
    assert packedaudio.PAINFO == dict(rt.ES_PAINFO) and packedaudio.PAINFO_WORDS == rt.ES_PAINFO_WORDS
    assert packedaudio.PASTATUS == dict(rt.ES_PASTATUS) and packedaudio.FATAL == rt.ES_PACKED_FATAL
    assert sorted(packedaudio.PAINFO.values()) == list(range(packedaudio.PAINFO_WORDS))
    assert packedaudio.FRAMES_PER_PES == rt.ES_PACKED_FRAMES_PER_PES == pc.G
    assert packedaudio.NAL_ROWS == rt.ES_PACKED_NAL_ROWS and packedaudio.MAX_PES_LIMIT == rt.ES_PACKED_MAX_PES_LIMIT
    assert packedaudio.tile_bytes() == rt.ES_PACKED_TILE == 32768
    assert (rt.ES_PACKED_MAX_TAGS, rt.ES_PACKED_MAX_ID3_FRAMES) == (8, 32)
    assert dict(rt.ES_PASTATUS) == {"no_timestamp": pc.NO_TIMESTAMP, "bad_id3": pc.BAD_ID3, "no_frame": pc.NO_FRAME,
                                    "trailing_bytes": pc.TRAILING, "pes_overflow": pc.OVERFLOW, "bad_rate": pc.BAD_RATE}


def test_hand_built_segments_give_what_they_must():
    """What the builder plants, stated by hand: a reference and a demux that both found nothing
    could not pass."""
    f = pc.frames(9, 1, rate_index=3, channels=2)
    head = pc.ts_tag((1 << 32) + 5)
    buf, offs, lens = pc.layout([head + b"".join(f), b"".join(f[:4]), head + b"".join(f) + b"zz"])
    got = packedaudio.packed_audio_batch(buf, offs, lens, max_pes=2)
    T = len(head)
    assert T == 10 + 10 + 53
    pa = got.painfo.numpy()
    assert pa[0].tolist() == [ST["pes_overflow"], T, 1, (1 << 32) + 5, 9, lens[0], 48000, 2]
    assert pa[1].tolist() == [ST["no_timestamp"], 0, 0, -1, 4, lens[1], 48000, 2]
    assert pa[2].tolist() == [ST["pes_overflow"] | ST["trailing_bytes"], T, 1, (1 << 32) + 5, 9, lens[2] - 2, 48000, 2]
    sizes = [len(x) for x in f]
    assert got.pes[0, 1].tolist() == [[0, (1 << 32) + 5, (1 << 32) + 5],
                                      [sum(sizes[:4]), (1 << 32) + 5 + 7680, (1 << 32) + 5 + 7680]]
    assert got.pes[0, 2, 0].tolist() == [0, (1 << 32) + 5, (1 << 32) + 5] and (got.pes[0, 0] == -1).all()
    assert got.aframes[0].tolist() == [[4, sum(sizes[:4])], [4, sum(sizes[4:8])]]
    assert got.aframes[1].tolist() == [[4, lens[1]], [-1, -1]] and (got.pes[1, 2] == -1).all()
    I = tsdemux.INFO
    info = got.info.numpy()
    assert info[0, I["status"]] == tsdemux.STATUS["pes_overflow"] and info[1, I["status"]] == 0
    assert info[0, I["n_audio_pes"]] == 3 and info[0, I["audio_es_offset"]] == T
    assert info[0, I["audio_bytes"]] == lens[0] - T
    assert info[0, I["audio_type"]] == 0x0F and info[0, I["video_type"]] == 0 and info[0, I["video_pid"]] == -1
    assert info[0, I["id3_bytes"]] == T and info[0, I["n_id3_pes"]] == 1 and info[1, I["n_id3_pes"]] == 0
    S = esindex.SINFO
    assert got.sinfo[:, S["status"]].tolist() == [0, 0, esindex.SSTATUS["adts_error"]]
    assert got.sinfo[0].tolist() == [0, 0, 0, 0, -1, 9, 48000, 2]
    assert (got.nal == -1).all() and (got.au == -1).all() and tuple(got.nal.shape) == (3, 1, 4)
    seg = got.segment(2)
    assert seg["status_names"] == ["trailing_bytes", "pes_overflow"] and seg["n_frames"] == 9 and len(seg["pes"]) == 2
    pc.assert_equal(got, pc.ref_batch(buf, offs, lens, 2))


def test_the_case_builders_plant_what_they_name():
    ref = {name: pc.ref_batch(*pc.batch(name)[:3], pc.batch(name)[3])["painfo"] for name in ("counts", "overflow",
                                                                                         "align", "tiles", "tags")}
    assert ref["counts"][:, PA["n_frames"]].tolist() == [0, 1, 3, 4, 5, 0, 5]
    assert ref["overflow"][:, PA["n_frames"]].tolist() == [16, 17, 21, 3]
    assert [int(s) & pc.OVERFLOW for s in ref["overflow"][:, PA["status"]]] == [0, 16, 16, 0]
    assert sorted(int(t) % 16 for t in ref["align"][:, PA["id3_bytes"]]) == list(range(16))
    assert (ref["align"][:, PA["status"]] == 0).all() and (ref["tiles"][:, PA["status"]] == 0).all()
    tile = pc.tile_bytes()
    segs, _ = pc.case_tiles()
    T = int(ref["tiles"][0, PA["id3_bytes"]])
    for c in range(8):  # a frame starts c bytes in front of the first tile's end
        starts, q = [], T
        while q < len(segs[c]):
            starts.append(q)
            q += pc._frame_at(segs[c], q, len(segs[c]))
        assert (T & ~15) + tile - c in starts
    assert len(segs[8]) > 2 * tile + T
    st = ref["tags"][:, PA["status"]]
    assert int(st[0]) == pc.NO_TIMESTAMP and int(st[2]) == 0 and int(ref["tags"][5, PA["timestamp"]]) == pc.TS0 + 3
    assert int(ref["tags"][6, PA["timestamp"]]) == pc.TS0 + 4
    assert int(st[8]) == pc.NO_TIMESTAMP | pc.NO_FRAME and int(ref["tags"][8, PA["n_tags"]]) == 8 and int(st[9]) == 0
    assert int(st[10]) == pc.BAD_ID3 | pc.NO_TIMESTAMP and int(st[11]) == pc.BAD_ID3
    assert [int(s) for s in st[12:17]] == [pc.NO_TIMESTAMP] * 5
    assert int(ref["tags"][17, PA["timestamp"]]) == (1 << 32) + 12345
    assert int(ref["tags"][18, PA["timestamp"]]) == pc.TS0
    assert int(ref["tags"][19, PA["timestamp"]]) == (1 << 33) - 1
    assert [int(s) for s in st[20:23]] == [pc.NO_TIMESTAMP] * 3
    assert int(st[28]) == pc.NO_TIMESTAMP and int(st[29]) == 0


@pytest.mark.parametrize("name", list(pc.CASES))
def test_cases_match_the_reference(name):
    buf, offs, lens, max_pes = pc.batch(name)
    before = buf.clone()
    got = packedaudio.packed_audio_batch(buf, offs, lens, max_pes=max_pes)
    pc.assert_equal(got, pc.ref_batch(buf, offs, lens, max_pes))
    assert torch.equal(buf, before)
    assert buf.numel() < 1_000_000


def test_breaks_stop_the_chain_where_they_are():
    buf, offs, lens, max_pes = pc.batch("breaks")
    pa = packedaudio.packed_audio_batch(buf, offs, lens, max_pes=max_pes).painfo.numpy()
    assert pa[:, PA["n_frames"]].tolist() == [5, 1, 3, 3, 2, 2, 4, 0, 5, 5, 5, 4]
    want = [pc.TRAILING] * 7 + [pc.NO_FRAME, pc.BAD_RATE, pc.BAD_RATE, pc.TRAILING, 0]
    assert pa[:, PA["status"]].tolist() == want


def test_lengths_as_a_tensor_with_host_caps():
    buf, offs, lens, max_pes = pc.batch("counts")
    n = torch.tensor(lens, dtype=torch.int64)
    ref = pc.ref_batch(buf, offs, lens, max_pes)
    pc.assert_equal(packedaudio.packed_audio_batch(buf, offs, n + 9, caps=lens, max_pes=max_pes), ref)
    cut = [lens[0], -3] + [v - 5 for v in lens[2:]]
    want = pc.ref_batch(buf, offs, [max(v, 0) for v in cut], max_pes)
    pc.assert_equal(packedaudio.packed_audio_batch(buf, offs, torch.tensor(cut), caps=lens, max_pes=max_pes), want)
    assert want["painfo"][4, PA["status"]] & pc.TRAILING


def test_default_limit_views_and_empty_batch():
    buf, offs, lens, _ = pc.batch("mixed")
    got = packedaudio.packed_audio_batch(buf, offs, lens)
    pc.assert_equal(got, pc.ref_batch(buf, offs, lens, tsdemux.DEFAULT_MAX_PES))
    res, ix = got.as_demux(), got.as_index()
    assert res.es.data_ptr() == buf.data_ptr() and res.info.data_ptr() == got.info.data_ptr()
    assert ix.aframes.data_ptr() == got.aframes.data_ptr() and ix.sinfo.data_ptr() == got.sinfo.data_ptr()
    empty = packedaudio.packed_audio_batch(buf, [], [], max_pes=4)
    assert empty.painfo.shape == (0, 8) and empty.pes.shape == (0, 3, 4, 3) and empty.nal.shape == (0, 1, 4)


def test_bad_arguments_are_rejected():
    buf, offs, lens, _ = pc.batch("one")
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="max_pes"):
            packedaudio.packed_audio_batch(buf, offs, lens, max_pes=bad)
    with pytest.raises(ValueError):
        packedaudio.packed_audio_batch(buf, offs, [buf.numel() + 1])
    with pytest.raises(ValueError):
        packedaudio.packed_audio_batch(buf, [-16], lens)
    with pytest.raises(ValueError, match="caps"):
        packedaudio.packed_audio_batch(buf, offs, torch.tensor(lens))
    with pytest.raises(ValueError, match="uint8"):
        packedaudio.packed_audio_batch(buf.to(torch.int32), offs, lens)


# ---------------------------------------------------------------- equivalence with the TS path
MAX_PES, MAX_AF = 8, 32


def equivalence_inputs():
    """Per segment ``(frames, stamp, rate)``: one to thirty frames, both header sizes, three rates."""
    out = []
    for i, (count, idx) in enumerate(((1, 3), (4, 4), (9, 3), (13, 11), (30, 4))):
        out.append((pc.frames(count, 40 + i, rate_index=idx, channels=1 + i % 2, lo=1, hi=300), pc.TS0 + 977 * i,
                    pc.RATES[idx]))
    return out


def chain(res, ix, caps, seqs):
    """remux -> codec configuration -> fragment, as the pipeline calls them; the host views of every segment."""
    max_nal = int(ix.nal.shape[1])
    hr, gap = fragment.frag_headroom(MAX_PES), fragment.frag_audio_gap(MAX_AF)
    oo, size = remux.layout_out(caps, max_nal, headroom=hr, audio_gap=gap)
    out = torch.zeros(size, dtype=torch.uint8, device=res.es.device)
    rx = remux.remux_batch(res, ix, caps, out, oo, max_aframes=MAX_AF, audio_gap=gap, headroom=hr)
    cfg = codecconfig.config_batch(res, ix, caps)
    fr = fragment.fragment_batch(rx, ix, seqs)
    views = []
    for i in range(len(caps)):
        r, f = rx.segment(i), fr.segment(i)
        cinfo = cfg.cinfo[i].cpu().numpy()
        views.append({"asamples": r["asamples"].tolist(), "audio_mdat": r["audio_mdat"],
                      "rinfo": [r[k] for k in ("audio_box_offset", "audio_payload_bytes", "n_aframes",
                                               "audio_base_pts")],
                      "config": cinfo[16:19].tolist() + [int(cinfo[0]) & codecconfig.CSTATUS["no_audio_config"]],
                      "moof": f["audio"][:f["audio_moof_bytes"]], "audio": f["audio"],
                      "finfo": [f[k] for k in ("audio_moof_bytes", "audio_tfdt", "time_base")]})
    return views


def packed_and_ts_views(dev):
    inputs = equivalence_inputs()
    seqs = list(range(7, 7 + len(inputs)))
    buf, offs, lens = pc.layout([pc.ts_tag(ts) + b"".join(f) for f, ts, _ in inputs], dev)
    pa = packedaudio.packed_audio_batch(buf, offs, lens, max_pes=MAX_PES)
    packed = chain(pa.as_demux(), pa.as_index(), lens, seqs)
    tbuf, toffs, tlens = pc.layout([pc.audio_ts(f, ts, rate) for f, ts, rate in inputs], dev)
    res = tsdemux.demux_batch(tbuf, toffs, tlens, torch.zeros_like(tbuf), toffs, max_pes=MAX_PES)
    ts = chain(res, esindex.index_batch(res, tlens, max_nal=4), tlens, seqs)
    return inputs, pa, res, packed, ts


def check_equivalence(dev):
    inputs, pa, res, packed, ts = packed_and_ts_views(dev)
    I = tsdemux.INFO
    for i, (f, stamp, rate) in enumerate(inputs):
        assert packed[i] == ts[i], (i, [k for k in ts[i] if packed[i][k] != ts[i][k]])
        bodies = b"".join(x[9 if not x[1] & 1 else 7:] for x in f)
        assert packed[i]["audio_mdat"][8:] == bodies and packed[i]["rinfo"][2] == len(f)
        assert packed[i]["rinfo"][3] == stamp and len(packed[i]["moof"]) == 96 + 4 * len(f)
        assert packed[i]["config"] == [2, pc.RATES.index(rate), 1 + i % 2, 0]
    # the demux rows themselves: what the TS demux found for the same frames
    groups = [(len(f) + 3) // 4 for f, _, _ in inputs]
    pi, ti = pa.info.cpu().numpy(), res.info.cpu().numpy()
    for k in ("n_audio_pes", "audio_first_pts", "audio_last_pts", "audio_type", "video_type", "n_video_pes",
              "video_bytes", "video_first_pts", "video_last_pts", "video_pid", "status"):
        assert pi[:, I[k]].tolist() == ti[:, I[k]].tolist(), k
    assert pi[:, I["n_audio_pes"]].tolist() == groups
    for i, g in enumerate(groups):
        assert torch.equal(pa.pes[i, 1, :g].cpu(), res.pes[i, 1, :g].cpu())


def test_the_ops_behind_give_what_an_audio_only_ts_gives():
    check_equivalence("cpu")
