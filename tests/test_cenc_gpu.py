"""The cenc decrypt on the MI355X (``kernels/cenc.hip``): the cases of ``test_cenc.py`` through the
same builders.  The decrypted bytes, ``ranges`` and ``cinfo`` equal the independent reference and
the host implementation bit for bit; through the raw op the copy, ``ranges``, ``cinfo`` and the
scratch sit behind canaries and the bytes between the segments' copies keep theirs; the source is
unchanged; ``caption_batch`` runs on the decrypted views; the dispatcher op agrees with the pybind
entry.  The largest batch is 160 KB."""
import numpy as np
import pytest
import torch

import captions_cases as cap
import cenc_cases as ce
import mp4_cases as mc
from hlsjs_p2p_wrapper_amd.ops import aes, captions, cenc, mp4demux
from hlsjs_p2p_wrapper_amd.ops._native import device

pytestmark = pytest.mark.gpu
PAD = 64  # canary elements behind each output of a raw call


def run_raw(op, b, md, cuda, max_range=None, short=None):
    """``cenc_decrypt`` through ``op`` on a destination laid out here, canaries between the copies
    and ``PAD`` canary elements behind ``ranges``, ``cinfo`` and the scratch: (bytes per segment,
    ranges, cinfo) after checking every canary."""
    B, max_range = len(b.offs), max_range or b.max_range
    max_pes, max_run = md.pes.shape[2], md.runs.shape[1]
    en = np.ones(B, np.uint8) if b.enable is None else np.asarray(b.enable, np.uint8)
    raw, offs, lens = mc.layout([bytes(n) for n in b.lens])
    dst = torch.from_numpy(np.frombuffer(raw, np.uint8).copy())
    src = b.buf.cpu()
    for i in np.flatnonzero(en):
        dst[offs[i]:offs[i] + lens[i]] = src[b.offs[i]:b.offs[i] + lens[i]]
    planted = dst.clone()
    dst = dst.to(cuda)
    prot, civ = cenc.pack_protection(b.tracks, B, "cenc_decrypt", "cenc")
    erk = np.stack([aes.enc_round_keys_le(k) for k in b.keys]) if B else np.zeros((0, 44), np.uint32)
    iv = np.frombuffer(b"".join(b.ivs), np.uint8)
    sizes = {"scratch": B * 2 * max_pes * 4, "ranges": B * max_range * 8, "cinfo": B * 8}
    out = {k: torch.full((n + (PAD if k != short else -1),), 0x5A, dtype=torch.int64 if k == "cinfo" else torch.int32,
                         device=cuda) for k, n in sizes.items()}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    tel, sbox = aes.device_enc_tables(cuda)
    i64 = lambda a: dev(np.asarray(a, np.int64))  # noqa: E731
    op(b.buf, i64(b.offs), i64(b.lens), dst, i64(offs), md.info, md.pes, md.minfo, md.msamples, md.runs, max_pes,
       max_run, dev(prot.reshape(-1)), dev(civ.reshape(-1)),
       dev(iv.copy()), dev(erk.view(np.int32).reshape(-1)), dev(en), tel, sbox, max_range, max(b.lens),
       out["scratch"], out["ranges"], out["cinfo"])
    torch.cuda.synchronize()
    for k in sizes:
        assert (out[k][-PAD:] == 0x5A).all(), k
    got = dst.cpu()
    keep = torch.ones(got.numel(), dtype=torch.bool)
    for i in np.flatnonzero(en):
        keep[offs[i]:offs[i] + lens[i]] = False
    assert torch.equal(got[keep], planted[keep])  # canaries and disabled segments
    segs = [got[o:o + n].numpy().tobytes() if en[i] else None for i, (o, n) in enumerate(zip(offs, lens))]
    return (segs, out["ranges"][:-PAD].cpu().numpy().reshape(B, max_range, 8),
            out["cinfo"][:-PAD].cpu().numpy().reshape(B, 8))


@pytest.mark.parametrize("name", list(ce.CASES))
def test_cases_match_the_reference_and_the_host(name, cuda):
    b = ce.batch(name, cuda)
    before = b.buf.cpu()
    ref = ce.ref_of(name)
    md, cb = ce.run(b)
    assert cb.buf.is_cuda and cb.cinfo.is_cuda and cb.ranges.is_cuda
    mc.assert_equal(md, ref[0])
    ce.assert_equal(b, cb, ref)
    segs, ranges, cinfo = run_raw(device().cenc_decrypt, b, md, cuda)  # behind canaries
    assert segs == ref[1] and np.array_equal(ranges, ref[2]) and np.array_equal(cinfo, ref[3])
    assert torch.equal(b.buf.cpu(), before)  # the source is only read
    host = ce.batch(name)
    _, hb = ce.run(host)
    assert torch.equal(cb.cinfo.cpu(), hb.cinfo) and torch.equal(cb.ranges.cpu(), hb.ranges)
    assert np.array_equal(cb.offs, hb.offs)
    for i, n in enumerate(b.lens):
        o = int(cb.offs[i])
        if o >= 0:
            assert torch.equal(cb.buf[o:o + n].cpu(), hb.buf[o:o + n]), i


def test_the_known_answer_is_the_nist_plaintext(cuda):
    b = ce.batch("known", cuda)
    _, cb = ce.run(b)
    for i in range(2):
        o = int(cb.offs[i])
        assert cb.buf[o + b.lens[i] - 64:o + b.lens[i]].cpu().numpy().tobytes() == ce.NIST_PLAIN


def test_the_grid_walk_has_more_pairs_than_workgroups(cuda):
    b = ce.batch("grid", cuda)
    assert len(b.offs) > device().device_cus(b.buf) and ce.TILE == cenc.TILE_UNITS


def test_enable_masks_and_an_empty_batch(cuda):
    for mask in ([True, False, True], [False, False, False]):
        b = ce.batch("limits", cuda, enable=mask)
        md, cb = ce.run(b)
        ref = ce.ref_batch(b)
        ce.assert_equal(b, cb, ref)
        segs, ranges, cinfo = run_raw(device().cenc_decrypt, b, md, cuda)
        assert segs == ref[1] and np.array_equal(ranges, ref[2]) and np.array_equal(cinfo, ref[3])
    b = ce.batch("limits", cuda)
    md = mp4demux.mp4_demux_batch(b.buf, [], [], b.tracks[0], max_pes=4)
    cb = cenc.cenc_decrypt_batch(md, b.tracks[0], [], max_range=4)
    assert cb.cinfo.shape == (0, 8) and cb.ranges.shape == (0, 4, 8) and cb.cinfo.is_cuda


def caption_twins(dev):
    """The caption case's video samples packaged again under cenc with 8-byte per-sample IVs and a
    subsample per NAL unit (SEI units included): (clear buffer, protected buffer, offsets, lengths,
    tracks, limits, key)."""
    buf, offs, lens, tracks, lim = mc.batch("captions")
    md = mp4demux.mp4_demux_batch(buf, offs, lens, tracks, **lim)
    raw, nal, au, key, twins, vt = buf.numpy(), md.nal.numpy(), md.au.numpy(), ce.key_of(3), [], []
    for i, o in enumerate(offs):
        hdr = 2 if tracks[i][0].codec_type == 0x24 else 1
        samples, subs = [], []
        for a in range(int(md.sinfo[i, 2])):
            q, z = int(md.pes[i, 0, a, 0]), int(md.msamples[i, 0, a, 0])
            samples.append(raw[o + q:o + q + z].tobytes())
            subs.append([(4 + hdr, int(nal[i, k, 1]) - hdr) for k in range(au[i, a, 0], au[i, a, 0] + au[i, a, 1])])
        twins.append(ce.protect([ce.Traf(1, 90000, samples, (0, 0), subs, iv_mode="per8")], key))
        vt.append((mp4demux.Mp4Track(1, "video", tracks[i][0].codec_type, 4,
                                     protection=cenc.Mp4Protection("cenc", 0, 0, 8, b"", ce.KID)),))
    clear, offs2, lens2 = mc.layout([t[0] for t in twins])
    prot = mc.layout([t[1] for t in twins])[0]
    assert sum(t[2] for t in twins) > 0 and clear != prot
    to = lambda x: torch.from_numpy(np.frombuffer(x, np.uint8).copy()).to(dev)  # noqa: E731
    return to(clear), to(prot), offs2, lens2, vt, lim, key


def test_captions_run_on_the_decrypted_views(cuda):
    clear, prot, offs, lens, tracks, lim, key = caption_twins(cuda)
    plain = mp4demux.mp4_demux_batch(clear, offs, lens, tracks, **lim)
    want = captions.caption_batch(plain.as_demux(), plain.as_index(), lens, max_cc=8)
    md = mp4demux.mp4_demux_batch(prot, offs, lens, tracks, **lim)
    cb = cenc.cenc_decrypt_batch(md, tracks, [key] * 2)
    assert cb.cinfo[:, 0].tolist() == [0, 0] and (cb.cinfo[:, 4] > 0).all()
    res, ix = cb.md.as_demux(), cb.md.as_index()
    assert res.es.data_ptr() == cb.buf.data_ptr() and ix.nal.data_ptr() == md.nal.data_ptr()
    got = captions.caption_batch(res, ix, lens, max_cc=8)
    cap.assert_captions_equal(got, cap.ref_batch(plain.as_demux(), plain.as_index(), lens, 8))
    assert torch.equal(got.ccinfo, want.ccinfo) and got.ccinfo[:, captions.CCINFO["n_samples"]].tolist() == [5, 5]
    for i, n in enumerate(lens):
        o = int(cb.offs[i])
        assert torch.equal(cb.buf[o:o + n], clear[offs[i]:offs[i] + n]), i


def test_dispatcher_op_agrees_with_the_pybind_entry(cuda):
    b = ce.batch("placement", cuda)
    md, _ = ce.run(b)
    ref = ce.ref_of("placement")
    for op in (device().cenc_decrypt, torch.ops.hlsp2p.cenc_decrypt):
        segs, ranges, cinfo = run_raw(op, b, md, cuda)
        assert segs == ref[1] and np.array_equal(ranges, ref[2]) and np.array_equal(cinfo, ref[3])


def test_short_outputs_and_misaligned_offsets_are_rejected_on_the_host(cuda):
    b = ce.batch("limits", cuda)
    md, _ = ce.run(b)
    for short in ("scratch", "ranges", "cinfo"):
        with pytest.raises(RuntimeError, match=f"{short} too small"):
            run_raw(device().cenc_decrypt, b, md, cuda, short=short)
    with pytest.raises(RuntimeError, match="1 to 65536"):
        run_raw(device().cenc_decrypt, b, md, cuda, max_range=65537)
    md.offs = md.offs + 8
    with pytest.raises(ValueError, match="16-byte aligned"):
        cenc.cenc_decrypt_batch(md, b.tracks, b.keys)
