"""The moof boxes of ``ops/fragment.py`` on the host implementation (``runtime/fragment.cpp``)
against the independent reference of ``fragment_cases.py``: every byte of ``out`` (a canary fill
shows what must stay untouched: the unused head of the headroom and of the gap, both ``mdat``
boxes, the slack between segments), the ``finfo`` rows, the time cases as literals, the gap
variant of the remux against the plain one, the host-side errors and fuzzed rows."""
import dataclasses

import numpy as np
import pytest
import torch

import fragment_cases as fc
import remux_cases as rc
from hlsjs_p2p_wrapper_amd.ops import fragment, remux
from hlsjs_p2p_wrapper_amd.player import fmp4


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_host_equals_the_reference(name):
    b = fc.build_batch(name)
    rx, fr = fc.run_batch(b)
    fc.assert_batch_equal(rx, fr, fc.expected(name))
    assert list(b.offs) == sorted(b.offs, reverse=True)  # out_offs does not ascend


def test_counts_cover_every_lane_grouping():
    want_m = {0, 1, 3, 63, 64, 65, 255, 256, 257, 512, 300}
    want_n = {0, 1, 2, 3, 4, 5, 255, 256, 257, 1024, 12, 10}
    got_m, got_n, overflowed = set(), set(), set()
    for name in fc.CASES:
        ref = fc.expected(name)
        got_m |= set(ref[0][:, remux.RINFO["n_vsamples"]].tolist())
        got_n |= set(ref[4][:, fragment.FINFO["n_asamples"]].tolist())
        over = ref[0][:, remux.RINFO["status"]] & remux.RSTATUS["aframe_overflow"] != 0
        overflowed |= {(ref[2].shape[1], int(t)) for t in ref[0][over, remux.RINFO["n_aframes"]]}
    assert want_m <= got_m and want_n <= got_n
    assert {(1024, 1027), (12, 15), (10, 13)} <= overflowed  # max_aframes + 3 frames: the table keeps max_aframes
    assert fc.build_batch("one").offs.shape == (1,) and fc.build_batch("counts").offs.shape == (9,)


def test_time_cases_as_literals():
    b = fc.build_batch("times")
    _, fr = fc.run_batch(b)
    _, want = fc.time_segments()
    F = fragment.FINFO
    got = fr.finfo.numpy()
    for i, w in enumerate(want):
        assert (int(got[i, F["status"]]), int(got[i, F["video_tfdt"]]), int(got[i, F["audio_tfdt"]]),
                int(got[i, F["time_base"]])) == w, i
    # the rollover case: the reference time plus the seven ticks since the wrap
    assert int(got[3, F["video_tfdt"]]) == 900007
    assert fragment.FSTATUS == {"time_clamped": 1, "no_rate": 2}
    seg0 = fr.segment(0)
    assert fc.walk_fragment(seg0["video"])["sequence_number"] == 5  # 2^32 + 5, modulo 2^32


def test_time_rules_of_the_runtime(rt):
    for x, base, ref in ((7, 2 ** 33 - 900000, 900000), (900000, 450000, -1), (5, 10, -1), (5, 10, 0),
                         (2 ** 33 - 1, 0, 5), (100, 0, 2 ** 40), (0, 2 ** 33 + 7, 3 * 2 ** 33)):
        assert rt.time_rel(x, base, ref) == fc.ref_time_rel(x, base, ref), (x, base, ref)
    for t, rate in ((900300, 48000), (1, 44100), (2 ** 34, 96000), (0, 8000), (89999, 7350)):
        assert rt.audio_rescale(t, rate) == fc.ref_rescale(t, rate) == fmp4.audio_base(t, rate)


@pytest.mark.parametrize("name", ["counts", "rows300_10"])
def test_default_times_equal_the_host_packer(name):
    """With the default time arguments both boxes are what ``player/fmp4.py`` packs, byte for byte."""
    b = fc.build_batch(name)
    rx, fr = fc.run_batch(b)
    for i, p in enumerate(b.params):
        s, f = rx.segment(i), fr.segment(i)
        rate = int(b.ix.sinfo[i, 6])
        vmoof = fmp4.video_moof(p["seq"], s["video_base_dts"], s["vsamples"])
        amoof = fmp4.audio_moof(p["seq"], s["audio_base_pts"], rate, s["asamples"])
        assert f["video"] == vmoof + s["video_mdat"] and f["audio"] == amoof + s["audio_mdat"], i
        assert (f["video_moof_bytes"], f["audio_moof_bytes"]) == (len(vmoof), len(amoof))
        for track, count in (("video", len(s["vsamples"])), ("audio", len(s["asamples"]))):
            box = fc.walk_fragment(f[track])
            assert box["count"] == count and len(box["mdat_payload"]) == s[f"{track}_payload_bytes"]
        assert torch.equal(fr.video(i), rx.out[int(b.offs[i]) - len(vmoof):int(b.offs[i]) + len(s["video_mdat"])])


def test_box_sizes_and_layout_exports(rt):
    rows = np.zeros((7, 5), np.int32)
    for m in (0, 1, 7):
        assert fragment.moof_video_bytes(m) == len(fmp4.video_moof(1, 0, rows[:m])) == 88 + 16 * m
        assert fragment.moof_audio_bytes(m) == len(fmp4.audio_moof(1, 0, 48000, rows[:m, :2])) == 96 + 4 * m
        assert len(fc.ref_video_moof(1, 0, rows[:m])) == 88 + 16 * m
        assert len(fc.ref_audio_moof(1, 0, rows[:m])) == 96 + 4 * m
    assert [fragment.frag_headroom(p) for p in (1, 10, 11, 512)] == [256, 256, 512, 8448]
    assert [fragment.frag_audio_gap(n) for n in (10, 12, 1024)] == [144, 144, 4192]
    assert fragment.FINFO == dict(rt.ES_FINFO) and fragment.FINFO_WORDS == rt.ES_FINFO_WORDS == 8
    assert sorted(fragment.FINFO.values()) == list(range(fragment.FINFO_WORDS))
    assert fragment.FSTATUS == dict(rt.ES_FSTATUS)
    assert fragment.FPARAM == dict(rt.ES_FPARAM) and fragment.FPARAM_WORDS == rt.ES_FPARAM_WORDS
    assert rt.ES_OUT_ALIGN == 256


@pytest.mark.parametrize("name", ["mixed", "audio_overflow", "timestamps"])
def test_remux_with_a_gap_is_the_plain_remux_shifted(name):
    T, g = rc.TILE, 48
    segs, max_pes, max_nal, max_aframes = rc.CASES[name](T)
    res, caps, ix = rc.build(segs, max_pes, max_nal)
    offs, size = remux.layout_out(caps, max_nal)
    plain = remux.remux_batch(res, ix, caps, torch.full((size,), rc.FILL, dtype=torch.uint8), offs,
                              max_aframes=max_aframes)
    goffs, gsize = remux.layout_out(caps, max_nal, headroom=512, audio_gap=g)
    assert np.array_equal(goffs % 256, np.zeros_like(goffs)) and goffs[0] == 512
    gapped = remux.remux_batch(res, ix, caps, torch.full((gsize,), rc.FILL, dtype=torch.uint8), goffs,
                               max_aframes=max_aframes, audio_gap=g, headroom=512)
    assert (gapped.headroom, gapped.audio_gap) == (512, g) and (plain.headroom, plain.audio_gap) == (0, 0)
    A0 = remux.RINFO["audio_box_offset"]
    want = plain.rinfo.clone()
    want[:, A0] += g
    assert torch.equal(gapped.rinfo, want)
    assert torch.equal(gapped.vsamples, plain.vsamples) and torch.equal(gapped.asamples, plain.asamples)
    expect = np.full(gsize, rc.FILL, np.uint8)
    src = plain.out.numpy()
    for i in range(len(caps)):
        P, a0, Q = (int(plain.rinfo[i, remux.RINFO[k]]) for k in ("video_payload_bytes", "audio_box_offset",
                                                                  "audio_payload_bytes"))
        o, go = int(offs[i]), int(goffs[i])
        expect[go:go + 8 + P] = src[o:o + 8 + P]
        expect[go + a0 + g:go + a0 + g + 8 + Q] = src[o + a0:o + a0 + 8 + Q]
    fc.assert_equal("out", gapped.out, expect)


def test_host_errors():
    b = fc.build_batch("one")
    out = torch.zeros(b.size, dtype=torch.uint8)
    seq = [1]
    with pytest.raises(ValueError, match="multiple of 16"):
        remux.remux_batch(b.res, b.ix, b.caps, out, b.offs, max_aframes=b.max_aframes, audio_gap=b.gap + 8)
    with pytest.raises(ValueError, match="multiple of 16"):
        remux.layout_out(b.caps, fc.MAX_NAL, audio_gap=24)
    with pytest.raises(ValueError, match="multiple of align"):
        remux.layout_out(b.caps, fc.MAX_NAL, headroom=128)
    short_gap = remux.remux_batch(b.res, b.ix, b.caps, out, b.offs, max_aframes=b.max_aframes, audio_gap=b.gap - 16,
                                  headroom=b.headroom)
    with pytest.raises(ValueError, match="audio_gap"):
        fragment.fragment_batch(short_gap, b.ix, seq)
    short_head = remux.remux_batch(b.res, b.ix, b.caps, out, b.offs, max_aframes=b.max_aframes, audio_gap=b.gap,
                                   headroom=b.headroom - 256)
    with pytest.raises(ValueError, match="headroom"):
        fragment.fragment_batch(short_head, b.ix, seq)
    plain = remux.remux_batch(b.res, b.ix, b.caps, out, b.offs, max_aframes=b.max_aframes)
    with pytest.raises(ValueError, match="headroom"):
        fragment.fragment_batch(plain, b.ix, seq)
    rx = remux.remux_batch(b.res, b.ix, b.caps, out, b.offs, max_aframes=b.max_aframes, audio_gap=b.gap,
                           headroom=b.headroom)
    with pytest.raises(ValueError, match="anchored"):
        fragment.fragment_batch(rx, b.ix, seq, anchor=[True])
    with pytest.raises(ValueError, match="anchored"):
        fragment.fragment_batch(rx, b.ix, seq, anchor=[True], time_ref=[-1])
    with pytest.raises(ValueError, match="one value per segment"):
        fragment.fragment_batch(rx, b.ix, [1, 2])
    # a headroom that the buffer does not hold, or that is another segment's region
    with pytest.raises(ValueError, match="outside out"):
        fragment.fragment_batch(dataclasses.replace(rx, out_offs=b.offs - 256, headroom=b.headroom), b.ix, seq)
    two = fc.build_batch("rows300_12")
    stride = int(two.offs[0] - two.offs[1])  # a headroom one slot longer, with room for it in front of the first
    out2 = torch.zeros(two.size + stride, dtype=torch.uint8)
    rx2 = remux.remux_batch(two.res, two.ix, two.caps, out2, two.offs + stride, max_aframes=two.max_aframes,
                            audio_gap=two.gap, headroom=two.headroom)
    fragment.fragment_batch(rx2, two.ix, [0] * 9)
    with pytest.raises(ValueError, match="overlaps"):
        fragment.fragment_batch(dataclasses.replace(rx2, headroom=two.headroom + stride), two.ix, [0] * 9)
    fragment.fragment_batch(rx, b.ix, seq, anchor=[True], time_ref=[0])  # and the valid call passes


def test_fuzzed_rows_stay_behind_the_canaries():
    """Garbage in ``rinfo`` / ``vsamples`` / ``asamples``: the boxes equal the reference's clamped
    reading, and no byte outside the segment's headroom and region changes; where the audio box
    offset is as the remux wrote it, no byte outside the headroom and the gap."""
    b = fc.build_batch("rows300_10")
    rx, _ = fc.run_batch(b)
    before = rx.out.numpy().copy()
    fz, (rinfo, vs, asamp) = fc.fuzz_tables(rx)
    seq, base, ref, anchor = fc.param_arrays(b.params)
    fr = fragment.fragment_batch(fz, b.ix, seq, time_base=base, time_ref=ref, anchor=anchor)
    want = before.copy()
    regions = np.asarray(b.caps, np.int64) + fc.MAX_NAL + 32 + b.gap
    finfo = fc.apply_moofs(want, b.offs, rinfo, vs, asamp, b.ix.sinfo.numpy()[:, 6], b.params, regions, b.gap)
    fc.assert_equal("out", fz.out, want)
    fc.assert_equal("finfo", fr.finfo, finfo)
    assert {0, 300} <= set(finfo[:, 1] // 16 - 5) and {0, 10} <= set((finfo[:, 2] - 96) // 4)  # empty and full tables
    changed = np.flatnonzero(fz.out.numpy() != before)
    for i, o in enumerate(b.offs):
        o = int(o)
        mine = changed[(changed >= o - b.headroom) & (changed < o + regions[i])]
        if i % 3 != 2:  # the remux's own A0: only the headroom and the gap
            P, a0 = int(rx.rinfo[i, 1]), int(rx.rinfo[i, 3])
            assert np.all((mine < o) | ((mine >= o + 8 + P) & (mine < o + a0))), i
        changed = np.setdiff1d(changed, mine)
    assert not len(changed)
