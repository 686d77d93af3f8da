"""``ops.cbcs_decrypt_batch`` on the host (``runtime/cbcs.cpp``) against the independent reference of
``cbcs_cases.py``: the decrypted bytes, ``ranges`` and ``cinfo`` bit for bit, the source unchanged,
for every pattern, range length, IV form, subsample table, box placement, alignment and tile edge,
for damaged bytes, for the limits and the enable masks; what the builders must give; and the host
checks."""
import numpy as np
import pytest
import torch

import cbcs_cases as cc
import mp4_cases as mc
from hlsjs_p2p_wrapper_amd.ops import cbcs, mp4demux
from hlsjs_p2p_wrapper_amd.ops._native import runtime

ALL = list(cc.CASES)


def copies(cb, lens):
    """The bytes of every segment's copy (the buffer between them is not written)."""
    return [cb.buf[int(o):int(o) + n].numpy().tobytes() for o, n in zip(cb.offs, lens)]


def test_the_builders_give_protected_segments_that_decrypt_to_their_clear_twins():
    """The packager planted what the cases claim: the reference turns every sound segment into its
    clear twin, ``protect`` wrote the stated number of cipher blocks and changed at least 15 of
    every 16 bytes of them (a block that encrypts to itself in more than one byte is a 2^-16 event
    per byte pair; the seeds are fixed)."""
    total = 0
    for name in ALL:
        b = cc.batch(name)
        _, outs, _, cinfo = cc.ref_batch(b)
        for i, clear in enumerate(b.clear):
            if clear is None:
                continue
            o, n = b.offs[i], b.lens[i]
            prot = b.buf[o:o + n].numpy().tobytes()
            assert outs[i] == clear and len(prot) == len(clear), (name, i)
            changed = sum(x != y for x, y in zip(prot, clear))
            assert changed >= 15 * b.blocks[i] and b.blocks[i] == cinfo[i, 4] + cinfo[i, 5], (name, i, changed)
            total += b.blocks[i]
    assert total > 2000


def test_the_pattern_counts_that_the_rules_state():
    assert [len(cc.cipher_positions(n, 1, 9)) for n in cc.LENGTHS] == list(cc.BLOCKS_1_9)
    assert [len(cc.cipher_positions(n, 2, 8)) for n in cc.LENGTHS] == list(cc.BLOCKS_2_8)
    assert cc.cipher_positions(192, 2, 8) == [0, 16, 160, 176] and cc.cipher_positions(176, 1, 9) == [0, 160]
    b = cc.batch("patterns")
    _, cb = cc.run(b)
    for i, want in ((0, cc.BLOCKS_1_9), (3, cc.BLOCKS_2_8)):
        seg = cb.segment(i)
        video = [r for r in seg["ranges"] if r[2] >> 30 == 0]
        sizes = {int(r[2]) & 0x3FFFFFFF: int(r[1]) for r in video}
        ranks = [int(r[3]) for r in video] + [seg["video_blocks"]]
        got = {k: ranks[j + 1] - ranks[j] for j, k in enumerate(sizes)}
        assert [got.get(k, 0) for k in range(len(cc.LENGTHS))] == list(want)
        assert seg["video_blocks"] == sum(want) and seg["video_samples"] == sum(1 for w in want if w)


@pytest.mark.parametrize("name", ALL)
def test_cases_match_the_reference(name):
    b = cc.batch(name)
    before = b.buf.clone()
    ref = cc.ref_batch(b)
    md, cb = cc.run(b)
    mc.assert_equal(md, ref[0])
    cc.assert_equal(b, cb, ref)
    assert torch.equal(b.buf, before)  # the source is only read
    assert cb.md.buf is cb.buf and cb.md.nal is md.nal and np.array_equal(cb.md.offs, cb.offs)


def test_statuses_of_the_subsample_and_placement_cases():
    ref = cc.ref_batch(cc.batch("subsamples"))[3]
    st = ref[:, 0].tolist()
    assert st[:7] == [0] * 7 and st[7] == st[8] == cc.BAD_SENC  # sums beyond the sample
    assert all(s & cc.BAD_SENC and s & cc.NO_SENC for s in st[9:14]) and st[14] == cc.BAD_SENC | cc.NO_SENC
    assert st[15:19] == [cc.NO_SENC, cc.NO_SENC, 0, 0] and st[19] == cc.NO_SENC
    assert ref[15, 1] == 0 and ref[16, 2] == 2 and ref[19, 6] == 0 and ref[0, 6] == 1
    ref = cc.ref_batch(cc.batch("placement"))[3]
    assert ref[:, 0].tolist() == [0] * 9 and ref[7, 6] == 3 and ref[4, 6] == 2 and ref[6, 6] == 1
    ref = cc.ref_batch(cc.batch("overlap"))[3]
    assert ref[:, 0].tolist() == [cc.OVERLAP, 0] and ref[0, 3] == 2 and ref[1, 3] == 4
    ref = cc.ref_batch(cc.batch("limits"))[3]
    assert ref[:, 0].tolist() == [cc.RANGE_OVERFLOW] * 3 and ref[:, 1].tolist() == [6] * 3
    assert cc.ref_batch(cc.batch("tiles"))[3][:, 1].tolist() == [1, 300, 300]


def test_enable_masks_leave_disabled_rows_alone_and_an_empty_batch_is_empty():
    for mask in ([True, False, True], [False, False, False], [False, True, False]):
        b = cc.batch("limits", enable=mask)
        ref = cc.ref_batch(b)
        _, cb = cc.run(b, max_range=8)
        b.max_range = 8
        cc.assert_equal(b, cb, cc.ref_batch(b))
        assert [o >= 0 for o in cb.offs.tolist()] == mask and ref[3][~np.array(mask)].sum() == 0
    b = cc.batch("limits")
    md = mp4demux.mp4_demux_batch(b.buf, [], [], b.tracks[0], max_pes=4)
    cb = cbcs.cbcs_decrypt_batch(md, b.tracks[0], [], max_range=4)
    assert cb.cinfo.shape == (0, 8) and cb.ranges.shape == (0, 4, 4) and len(cb.offs) == 0


def test_one_track_set_for_all_segments_and_an_init_segment():
    from hlsjs_p2p_wrapper_amd.player.mp4init import parse_init

    b = cc.batch("limits")
    md, cb = cc.run(b)
    same = cbcs.cbcs_decrypt_batch(md, b.tracks[0], b.keys, b.ivs, max_range=b.max_range)
    assert torch.equal(same.cinfo, cb.cinfo) and copies(same, b.lens) == copies(cb, b.lens)
    init = parse_init(cc.cbcs_init(audio=False))
    assert init.video.protection == b.tracks[0][0].protection
    same = cbcs.cbcs_decrypt_batch(md, init, b.keys, b.ivs, max_range=b.max_range)
    assert torch.equal(same.ranges, cb.ranges) and copies(same, b.lens) == copies(cb, b.lens)


def test_host_checks():
    b = cc.batch("limits")
    md, _ = cc.run(b)
    v = b.tracks[0][0]

    def track(**kw):
        return (mp4demux.Mp4Track(1, "video", 0x1B, 4, protection=cbcs.Mp4Protection(**{
            **dict(scheme="cbcs", crypt_byte_block=1, skip_byte_block=9, per_sample_iv_size=0, constant_iv=bytes(16),
                   kid=cc.KID), **kw})),)
    assert track() == (mp4demux.Mp4Track(1, "video", 0x1B, 4, protection=track()[0].protection),) and v.protection
    for bad, what in ((track(scheme="cenc"), "cenc"), (track(per_sample_iv_size=4), "IV"),
                      (track(constant_iv=bytes(5)), "IV"), (track(crypt_byte_block=0), "crypt_byte_block")):
        with pytest.raises(ValueError, match=what):
            cbcs.cbcs_decrypt_batch(md, bad, b.keys)
    with pytest.raises(ValueError, match="16 bytes"):
        cbcs.cbcs_decrypt_batch(md, b.tracks, [b"short"] * 3)
    with pytest.raises(ValueError, match="16 bytes"):
        cbcs.cbcs_decrypt_batch(md, b.tracks, b.keys, [b"short"] * 3)
    for n in (0, 65537):
        with pytest.raises(ValueError, match="max_range"):
            cbcs.cbcs_decrypt_batch(md, b.tracks, b.keys, max_range=n)
    with pytest.raises(ValueError, match="one key"):
        cbcs.cbcs_decrypt_batch(md, b.tracks, b.keys[:2])
    other = mp4demux.mp4_demux_batch(b.buf, b.offs[:2], b.lens[:2], b.tracks[:2], **b.limits)
    other.offs = md.offs  # tables of two segments, offsets of three
    with pytest.raises(ValueError, match="does not belong"):
        cbcs.cbcs_decrypt_batch(other, b.tracks, b.keys)


def test_layout_constants_agree_with_the_native_ones():
    rt = runtime()
    assert (cbcs.PROT, cbcs.CINFO) == (rt.CBCS_PROT, rt.CBCS_CINFO)
    assert (cbcs.CSTATUS, cbcs.RANGE) == (rt.CBCS_STATUS, rt.CBCS_RANGE)
    assert (cbcs.PROT_WORDS, cbcs.CINFO_WORDS, cbcs.RANGE_WORDS, cbcs.AUX_WORDS, cbcs.TRACK_SHIFT, cbcs.MAX_RANGE_LIMIT,
            cbcs.DEFAULT_MAX_RANGE) == (rt.CBCS_PROT_WORDS, rt.CBCS_CINFO_WORDS, rt.CBCS_RANGE_WORDS, rt.CBCS_AUX_WORDS,
                                        rt.CBCS_TRACK_SHIFT, rt.CBCS_MAX_RANGE_LIMIT, rt.CBCS_DEFAULT_MAX_RANGE)
    assert cbcs.CSTATUS == {"range_overflow": cc.RANGE_OVERFLOW, "no_senc": cc.NO_SENC, "bad_senc": cc.BAD_SENC,
                            "demux_damaged": cc.DEMUX_DAMAGED, "overlap": cc.OVERLAP}
