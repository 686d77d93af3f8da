"""``ops.caption_batch`` on the host implementation against the independent reference of
``captions_cases.py``: all five tensors bit for bit, the ES unchanged between its canaries, every
output inside its tensor, and the layout names pinned to the runtime's exports."""
import numpy as np
import pytest
import torch

import captions_cases as cc
import esindex_cases as esc
from hlsjs_p2p_wrapper_amd.ops import captions, esindex
from hlsjs_p2p_wrapper_amd.ops._native import runtime

PAD = 64  # canary elements behind each output of a raw call


def run_raw(res, ix, caps, max_cc, enable=None):
    """The runtime's ``caption_batch`` on outputs with ``PAD`` canary elements behind each: the five
    arrays as a dict, after checking the canaries."""
    B, max_pes, max_nal = len(caps), int(res.pes.shape[2]), int(ix.nal.shape[1])
    shapes = {"ccsamples": ((B, max_cc, 8), np.int32), "ccpts": ((B, max_cc), np.int64),
              "ccbytes": ((B, max_cc, cc.SLOT), np.uint8), "cc608": ((B, max_cc, 2, cc.FIELD), np.uint8),
              "ccinfo": ((B, 8), np.int64)}
    flat = {k: np.full(int(np.prod(s)) + PAD, 0x5A, dt) for k, (s, dt) in shapes.items()}
    en = np.ones(B, np.uint8) if enable is None else np.asarray(enable, np.uint8)
    runtime().caption_batch(res.es.numpy(), np.asarray(res.es_offs, np.int64), np.asarray(caps, np.int64),
                            res.info.numpy(), res.pes.numpy(), max_pes, max_nal, ix.nal.numpy(), ix.au.numpy(),
                            ix.aframes.numpy(), ix.sinfo.numpy(), en, max_cc, *(flat[k] for k in cc.NAMES))
    for k, (s, _) in shapes.items():
        assert (flat[k][-PAD:] == 0x5A).all(), k
    return {k: flat[k][:-PAD].reshape(s) for k, (s, _) in shapes.items()}


@pytest.fixture(scope="module")
def batches():
    out = {}
    for name in cc.CASES:
        res, caps, ix, max_cc = cc.batch(name)
        out[name] = (res, caps, ix, max_cc, cc.ref_batch(res, ix, caps, max_cc))
    return out


def test_layout_names_equal_the_runtime_exports(rt):
    assert captions.CCINFO == dict(rt.ES_CCINFO) and captions.CCINFO_WORDS == rt.ES_CCINFO_WORDS
    assert captions.CCROW == dict(rt.ES_CCROW) and captions.CCROW_WORDS == rt.ES_CCROW_WORDS
    assert captions.CCSTATUS == dict(rt.ES_CCSTATUS)
    assert sorted(captions.CCINFO.values()) == list(range(captions.CCINFO_WORDS))
    assert sorted(captions.CCROW.values()) == list(range(captions.CCROW_WORDS))
    assert (captions.CC_SLOT_BYTES, captions.CC_FIELD_BYTES, captions.CC_NAL_BYTES) == \
        (rt.ES_CC_SLOT_BYTES, rt.ES_CC_FIELD_BYTES, rt.ES_CC_NAL_BYTES) == (cc.SLOT, cc.FIELD, cc.NAL_BYTES)
    assert (captions.DEFAULT_MAX_CC, captions.MAX_CC_LIMIT) == (rt.ES_CC_DEFAULT_MAX, rt.ES_CC_MAX_LIMIT) == (512, 2048)
    assert (cc.TRUNCATED, cc.UNSUPPORTED, cc.OVERFLOW, cc.CLIPPED) == tuple(
        captions.CCSTATUS[k] for k in ("truncated", "unsupported_video", "cc_overflow", "sei_clipped"))


@pytest.mark.parametrize("name", list(cc.CASES))
def test_host_equals_the_reference(batches, name):
    res, caps, ix, max_cc, ref = batches[name]
    before = res.es.clone()
    got = captions.caption_batch(res, ix, caps, max_cc=max_cc)
    cc.assert_captions_equal(got, ref)
    cc.assert_captions_equal(run_raw(res, ix, caps, max_cc), ref)
    assert torch.equal(res.es, before)
    assert got.ccinfo.device == res.es.device and got.ccsamples.dtype == torch.int32


def test_the_cases_hold_what_they_claim(batches):
    """The reference's own totals on the hand-built segments: a builder that planted nothing would
    make every comparison pass."""
    info = batches["main"][4][4]
    S = captions.CCINFO
    # headers, near misses, emulation prevention, clip: candidates walked, samples found
    assert info[:4, S["n_sei"]].tolist() == [16, 8, 9, 7]
    assert info[:4, S["n_samples"]].tolist() == [10, 3, 9, 4]
    assert info[:4, S["status"]].tolist() == [0, 0, 0, cc.CLIPPED]
    samples = batches["main"][4][0]
    assert samples[1, :3, captions.CCROW["cc_count"]].tolist() == [3, 2, 1]  # walked on; the first of two wins
    assert samples[0, :, captions.CCROW["cc_count"]].max() == 31 and 0 in samples[0, :10, captions.CCROW["cc_count"]]
    # placement: all 40, and the candidate at the ES's last byte with and without audio behind it
    assert info[4:7, S["n_samples"]].tolist() == [40, 1, 1]
    # rows: the matches on the edges of the rounds, the candidate of a row without an access unit is none
    rows = samples[7, :, captions.CCROW["nal"]]
    assert [r for r in rows if r >= 0] == [5, 255, 256, 257, 300, 511, 512, 600, 601]
    assert info[7, S["n_sei"]] == 9  # row 0 has au == -1
    # order and pairs
    o = samples[8, :8]
    assert o[:, captions.CCROW["order"]].tolist() == [2, 7, 3, 5, 6, 0, 4, 1]
    assert o[:5, captions.CCROW["field1_pairs"]].tolist() == [1, 1, 31, 6, 0]
    assert o[:5, captions.CCROW["field2_pairs"]].tolist() == [1, 0, 0, 6, 31]
    assert o[:5, captions.CCROW["flags"]].tolist() == [1, 1, 1, 1, 0]
    assert (info[8, S["first_pts"]], info[8, S["last_pts"]]) == (-1, 10800)
    # HEVC: 39 and not 40 nor H.264's 6; 0x24 over H.264 bytes; MPEG-2 video with and without bytes
    assert info[9:14, S["n_samples"]].tolist() == [2, 0, 0, 0, 0]
    assert info[9:14, S["status"]].tolist() == [0, 0, cc.UNSUPPORTED, 0, 0]
    small = batches["small"][4][4]
    assert small[:, S["status"]].tolist() == [cc.OVERFLOW, cc.TRUNCATED | cc.OVERFLOW, 0]
    assert small[:, S["n_samples"]].tolist() == [6, 8, 3]
    long_ = batches["long"][4][4]
    assert long_[0, S["status"]] == cc.CLIPPED and long_[0, S["n_samples"]] == 2 and batches["long"][1][0] > 70000


def test_segment_view_is_in_presentation_order(batches):
    res, caps, ix, max_cc, ref = batches["main"]
    view = captions.caption_batch(res, ix, caps, max_cc=max_cc).segment(8)
    assert view["n_samples"] == 8 and [s["pts"] for s in view["samples"]] == [-1, -1, 0, 3600, 3600, 7200, 7200, 10800]
    assert [s["nal"] for s in view["samples"]] == [11, 15, 1, 5, 13, 7, 9, 3]
    first = view["samples"][2]
    assert first["type"] == 3 and first["au"] == 0 and first["bytes"][:2] == b"\x44\xff" and len(first["bytes"]) == 14
    assert (0, 0x14, 0x20) in view["field1"] and (0, 0x15, 0x2C) in view["field2"]
    assert [p for p, _, _ in view["field1"]] == sorted(p for p, _, _ in view["field1"])
    assert len(view["field1"]) == view["field1_pairs"] and len(view["field2"]) == view["field2_pairs"]


@pytest.mark.parametrize("mask", [[1, 0, 1], [0, 0, 0], [0, 1, 0]])
def test_enable_masks(batches, mask):
    res, caps, ix, max_cc, _ = batches["small"]
    ref = cc.ref_batch(res, ix, caps, max_cc, enable=mask)
    got = captions.caption_batch(res, ix, caps, max_cc=max_cc, enable=mask)
    cc.assert_captions_equal(got, ref)
    for i, on in enumerate(mask):
        if not on:
            assert not got.ccinfo[i].any() and (got.ccsamples[i] == -1).all() and (got.ccpts[i] == -1).all()
            assert not got.ccbytes[i].any() and not got.cc608[i].any()


def test_default_and_extreme_max_cc(batches):
    res, caps, ix, _, _ = batches["small"]
    for max_cc in (1, 512, 2048):
        got = captions.caption_batch(res, ix, caps, **({} if max_cc == 512 else {"max_cc": max_cc}))
        assert got.ccsamples.shape == (3, max_cc, 8)
        cc.assert_captions_equal(got, cc.ref_batch(res, ix, caps, max_cc))


def test_empty_batch():
    res, caps = esc.hand_batch([], "cpu")
    ix = esindex.index_batch(res, caps, max_nal=8)
    got = captions.caption_batch(res, ix, caps, max_cc=4)
    assert got.ccinfo.shape == (0, 8) and got.ccsamples.shape == (0, 4, 8) and got.ccpts.shape == (0, 4)
    assert got.ccbytes.shape == (0, 4, 96) and got.cc608.shape == (0, 4, 2, 64)


def test_host_side_checks(batches):
    res, caps, ix, max_cc, _ = batches["small"]
    for bad in (0, -1, 2049):
        with pytest.raises(ValueError, match="max_cc"):
            captions.caption_batch(res, ix, caps, max_cc=bad)
    with pytest.raises(ValueError, match="enable"):
        captions.caption_batch(res, ix, caps, enable=[True])
    with pytest.raises(ValueError, match="ES"):
        captions.caption_batch(res, ix, [res.es.numel() + 1] * 3)
    other = esindex.index_batch(*esc.hand_batch([esc.seg(b"")], "cpu"), max_nal=16)
    with pytest.raises(ValueError, match="does not belong"):
        captions.caption_batch(res, other, caps)


def damaged_batch():
    """The main batch with rows that lie (``captions_cases.damage``)."""
    res, caps, ix, max_cc = cc.batch("main")
    cc.damage(res, caps, ix)
    return res, caps, ix, max_cc


def test_damaged_rows_stay_in_bounds():
    res, caps, ix, max_cc = damaged_batch()
    before = res.es.clone()
    got = run_raw(res, ix, caps, max_cc)  # checks the canaries behind each output
    assert torch.equal(res.es, before)
    ref = cc.ref_batch(res, ix, caps, max_cc)
    cc.assert_captions_equal(got, ref)
    assert ref[4][:, captions.CCINFO["n_sei"]].sum() > 500  # the damage left work to do
