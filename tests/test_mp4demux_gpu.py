"""The fragmented-MP4 demux on the MI355X (``kernels/mp4_demux.hip``): the cases of
``test_mp4demux.py`` through the same builders.  All ten tensors equal the independent reference
and the host implementation bit for bit; the source is unchanged between its canaries; damaged
bytes leave every output inside its tensor; ``caption_batch`` runs on the views; the dispatcher op
agrees with the pybind entry; misaligned offsets and short outputs are rejected on the host.  The
largest batch is 55 KB."""
import numpy as np
import pytest
import torch

import captions_cases as cc
import mp4_cases as mc
from hlsjs_p2p_wrapper_amd.ops import captions, mp4demux
from hlsjs_p2p_wrapper_amd.ops._native import device
from test_mp4demux import shapes

pytestmark = pytest.mark.gpu
PAD = 64  # canary elements behind each output of a raw call


def run_raw(op, buf, offs, lens, tracks, lim, cuda, short=None):
    """``mp4_demux`` through ``op`` on outputs with ``PAD`` canary elements behind each (``short``:
    that one an element short instead): the ten arrays as a dict, after checking the canaries."""
    B = len(offs)
    sh = shapes(B, lim)
    dt = {np.int64: torch.int64, np.int32: torch.int32}
    flat = {k: torch.full((int(np.prod(s)) + (PAD if k != short else -1),), 0x5A, dtype=dt[t], device=cuda)
            for k, (s, t) in sh.items()}
    dev = lambda a: torch.from_numpy(np.asarray(a, np.int64)).to(cuda)  # noqa: E731
    op(buf, dev(offs), dev(lens), dev(lens), dev(mp4demux.pack_tracks(tracks, B).reshape(-1)), lim["max_pes"],
       lim["max_nal"], lim["max_moof"], lim["max_run"], lim["max_emsg"], *(flat[k] for k in mc.NAMES))
    torch.cuda.synchronize()
    for k in sh:
        assert (flat[k][-PAD:] == 0x5A).all(), k
    return {k: flat[k][:-PAD].cpu().numpy().reshape(sh[k][0]) for k in mc.NAMES}


@pytest.mark.parametrize("name", list(mc.CASES))
def test_cases_match_the_reference_and_the_host(name, cuda):
    buf, offs, lens, tracks, lim = mc.batch(name, cuda)
    before = buf.cpu()
    ref = mc.ref_batch(buf, offs, lens, tracks, lim)
    got = mp4demux.mp4_demux_batch(buf, offs, lens, tracks, **lim)
    assert got.minfo.is_cuda and got.nal.is_cuda and got.emsg.is_cuda
    mc.assert_equal(got, ref)
    mc.assert_equal(run_raw(device().mp4_demux, buf, offs, lens, tracks, lim, cuda), ref)  # behind canaries
    assert torch.equal(buf.cpu(), before)
    host = mp4demux.mp4_demux_batch(before, offs, lens, tracks, **lim)
    for field in mc.NAMES:
        assert torch.equal(getattr(got, field).cpu(), getattr(host, field)), field
    assert ref["minfo"][:, mp4demux.MINFO["n_moof"]].sum() > 0


def test_device_lengths_with_host_caps(cuda):
    """``lens`` as the decrypt leaves it: a device tensor; values beyond the cap and below zero are clamped."""
    buf, offs, lens, tracks, lim = mc.batch("small", cuda)
    ref = mc.ref_batch(buf, offs, lens, tracks, lim)
    n = torch.tensor(lens, dtype=torch.int64, device=cuda)
    mc.assert_equal(mp4demux.mp4_demux_batch(buf, offs, n + 9, tracks, caps=lens, **lim), ref)
    cut = [lens[0] - 1, -3, lens[2]]
    want = mc.ref_batch(buf, offs, [lens[0] - 1, 0, lens[2]], tracks, lim)
    mc.assert_equal(mp4demux.mp4_demux_batch(buf, offs, torch.tensor(cut, device=cuda), tracks, caps=lens, **lim), want)


def test_captions_run_on_the_views_unchanged(cuda):
    buf, offs, lens, tracks, lim = mc.batch("captions", cuda)
    got = mp4demux.mp4_demux_batch(buf, offs, lens, tracks, **lim)
    res, ix = got.as_demux(), got.as_index()
    assert res.es.data_ptr() == buf.data_ptr() and ix.nal.data_ptr() == got.nal.data_ptr()
    caps = captions.caption_batch(res, ix, lens, max_cc=8)
    cc.assert_captions_equal(caps, cc.ref_batch(res, ix, lens, 8))
    assert caps.ccinfo[:, captions.CCINFO["n_samples"]].tolist() == [5, 5]


def test_default_limits_and_empty_batch(cuda):
    buf, offs, lens, tracks, _ = mc.batch("small", cuda)
    mc.assert_equal(mp4demux.mp4_demux_batch(buf, offs, lens, tracks), mc.ref_batch(buf, offs, lens, tracks, mc.LIMITS))
    ones = dict(max_moof=1, max_run=1, max_emsg=1, max_pes=1, max_nal=1)
    one = mp4demux.mp4_demux_batch(buf, offs[:1], lens[:1], tracks, **ones)
    mc.assert_equal(one, mc.ref_batch(buf, offs[:1], lens[:1], tracks, ones))
    empty = mp4demux.mp4_demux_batch(buf, [], [], tracks, max_pes=4)
    assert empty.minfo.shape == (0, 18) and empty.pes.shape == (0, 3, 4, 3) and empty.minfo.is_cuda


def test_dispatcher_op_agrees_with_the_pybind_entry(cuda):
    buf, offs, lens, tracks, lim = mc.batch("small", cuda)
    ref = mc.ref_batch(buf, offs, lens, tracks, lim)
    for op in (device().mp4_demux, torch.ops.hlsp2p.mp4_demux):
        mc.assert_equal(run_raw(op, buf, offs, lens, tracks, lim, cuda), ref)


def test_misaligned_offsets_and_short_outputs_are_rejected_on_the_host(cuda):
    buf, offs, lens, tracks, lim = mc.batch("small", cuda)
    for short in ("minfo", "runs", "pes", "nal", "aframes"):
        with pytest.raises(RuntimeError, match=f"{short} too small"):
            run_raw(device().mp4_demux, buf, offs, lens, tracks, lim, cuda, short=short)
    with pytest.raises(RuntimeError, match="1 to 256"):
        run_raw(device().mp4_demux, buf, offs, lens, tracks, {**lim, "max_run": 257}, cuda)
    with pytest.raises(ValueError, match="16-byte aligned"):
        mp4demux.mp4_demux_batch(buf, [o + 8 for o in offs], lens, tracks, **lim)
    with pytest.raises(ValueError, match="partial dword"):
        i = next(i for i in range(len(offs)) if (offs[i] + lens[i]) % 4)  # a segment that ends inside a dword
        mp4demux.mp4_demux_batch(buf[:offs[i] + lens[i]], offs[:i + 1], lens[:i + 1], tracks, **lim)
    with pytest.raises(ValueError, match="lens"):
        mp4demux.mp4_demux_batch(buf, offs, torch.tensor(lens), tracks, caps=lens, **lim)
