"""``kernels/fragment.hip`` against the independent reference of ``fragment_cases.py`` and, bit
for bit, against the host implementation: the batches of ``test_fragment.py`` (every byte of a
canary-filled ``out``), fuzzed rows, the dispatcher op, the gap variant of the remux kernels, and
the pipeline on the device against the pipeline on the host."""
import numpy as np
import pytest
import torch

import fragment_cases as fc
import remux_cases as rc
from hlsjs_p2p_wrapper_amd.ops import fragment, remux
from hlsjs_p2p_wrapper_amd.ops._native import device
from hlsjs_p2p_wrapper_amd.ops.desc import pack_to_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_kernel_equals_the_reference_and_the_host(cuda, name):
    b = fc.build_batch(name, cuda)
    rx, fr = fc.run_batch(b)
    fc.assert_batch_equal(rx, fr, fc.expected(name))
    hrx, hfr = fc.run_batch(fc.build_batch(name))
    fc.assert_batch_equal(rx, fr, tuple(t.numpy() for t in (hrx.rinfo, hrx.vsamples, hrx.asamples, hrx.out,
                                                             hfr.finfo)))
    i = len(b.segs) - 1
    seg = fr.segment(i)
    assert seg == hfr.segment(i) and fr.video(i).device.type == "cuda"
    assert fr.video(i).untyped_storage().data_ptr() == rx.out.untyped_storage().data_ptr()
    for track in ("video", "audio"):
        fc.walk_fragment(seg[track])


def test_fuzzed_rows_on_the_device(cuda):
    """The garbage tables of ``test_fragment.py``: the kernel's bytes and rows equal the host's and
    the reference's clamped reading, and nothing outside the headrooms and regions changes."""
    hb = fc.build_batch("rows300_10")
    hrx, _ = fc.run_batch(hb)
    hfz, (rinfo, vs, asamp) = fc.fuzz_tables(hrx)
    b = fc.build_batch("rows300_10", cuda)
    rx, _ = fc.run_batch(b)
    before = rx.out.cpu().numpy()
    fz, _ = fc.fuzz_tables(rx)
    assert np.array_equal(fz.rinfo.cpu().numpy(), rinfo)  # the same seed: the same garbage
    seq, base, ref, anchor = fc.param_arrays(b.params)
    fr = fragment.fragment_batch(fz, b.ix, seq, time_base=base, time_ref=ref, anchor=anchor)
    hfr = fragment.fragment_batch(hfz, hb.ix, seq, time_base=base, time_ref=ref, anchor=anchor)
    want = before.copy()
    regions = np.asarray(b.caps, np.int64) + fc.MAX_NAL + 32 + b.gap
    finfo = fc.apply_moofs(want, b.offs, rinfo, vs, asamp, hb.ix.sinfo.numpy()[:, 6], b.params, regions, b.gap)
    fc.assert_equal("out", fz.out, want)
    fc.assert_equal("finfo", fr.finfo, finfo)
    fc.assert_equal("host out", fz.out, hfz.out.numpy())
    fc.assert_equal("host finfo", fr.finfo, hfr.finfo.numpy())


def test_dispatcher_op(cuda):
    """``torch.ops.hlsp2p.fragment_moof`` on the raw tensors, and its host-side checks."""
    device()
    b = fc.build_batch("rows300_12", cuda)
    out = torch.full((b.size,), fc.FILL, dtype=torch.uint8, device=cuda)
    rx = remux.remux_batch(b.res, b.ix, b.caps, out, b.offs, max_aframes=b.max_aframes, audio_gap=b.gap,
                           headroom=b.headroom)
    seq, base, ref, anchor = fc.param_arrays(b.params)
    B = len(b.caps)
    fp = np.zeros((B, fragment.FPARAM_WORDS), np.int64)
    fp[:, 0], fp[:, 1], fp[:, 2], fp[:, 3], fp[:, 4], fp[:, 5] = b.offs, rx.region, seq, base, ref, anchor
    d = pack_to_device({"fp": fp.reshape(-1)}, cuda)
    finfo = torch.full((B, fragment.FINFO_WORDS), -7, dtype=torch.int64, device=cuda)
    args = [rx.rinfo, rx.vsamples, rx.asamples, b.ix.sinfo, d["fp"], 300, b.max_aframes, b.headroom, b.gap, out, finfo]
    for bad, value, match in ((7, b.headroom - 256, "headroom"), (8, b.gap - 16, "audio_gap"),
                              (8, b.gap + 8, "audio_gap"), (5, 301, "vsamples too small"),
                              (6, b.max_aframes + 1, "audio_gap|asamples too small")):
        wrong = list(args)
        wrong[bad] = value
        with pytest.raises(RuntimeError, match=match):
            torch.ops.hlsp2p.fragment_moof(*wrong)
    torch.cuda.synchronize()
    assert (finfo.cpu() == -7).all() and torch.equal(out.cpu(), rx.out.cpu())
    torch.ops.hlsp2p.fragment_moof(*args)
    ref_ = fc.expected("rows300_12")
    fc.assert_equal("out", out, ref_[3])
    fc.assert_equal("finfo", finfo, ref_[4])
    schema = str(torch.ops.hlsp2p.fragment_moof.default._schema)
    assert "Tensor(a!) out" in schema and "Tensor(b!) finfo" in schema


def test_a_row_outside_out_is_left_alone(cuda):
    """The kernel's own guard: an fparams row whose headroom or region does not lie inside ``out``
    writes nothing (the Python wrapper rejects such a row before any launch)."""
    b = fc.build_batch("one", cuda)
    rx, fr = fc.run_batch(b)
    want_out, want_finfo = rx.out.clone(), fr.finfo.clone()
    rx.out[:int(b.offs[0])] = fc.FILL  # the video moof gone
    for off, region in ((b.headroom - 256, int(rx.region[0])), (int(b.offs[0]), rx.out.numel()),
                        (int(b.offs[0]) + 8, int(rx.region[0])), (int(b.offs[0]), 16)):
        fp = np.zeros((1, fragment.FPARAM_WORDS), np.int64)
        fp[0, :3] = off, region, 7
        fp[0, 4] = -1
        d = pack_to_device({"fp": fp.reshape(-1)}, cuda)
        before = rx.out.clone()
        finfo = torch.full((1, fragment.FINFO_WORDS), -7, dtype=torch.int64, device=cuda)
        device().fragment_moof(rx.rinfo, rx.vsamples, rx.asamples, b.ix.sinfo, d["fp"], 8, b.max_aframes, b.headroom,
                               b.gap, rx.out, finfo)
        assert torch.equal(rx.out, before) and (finfo == -7).all(), (off, region)
    seq, base, ref, anchor = fc.param_arrays(b.params)
    again = fragment.fragment_batch(rx, b.ix, seq, time_base=base, time_ref=ref, anchor=anchor)
    assert torch.equal(rx.out, want_out) and torch.equal(again.finfo, want_finfo)


@pytest.mark.parametrize("name", ["mixed", "tile_edges", "audio_overflow"])
def test_remux_kernels_with_a_gap_equal_the_host(cuda, name):
    T, g = device().remux_tile_bytes(), 4192
    segs, max_pes, max_nal, max_aframes = rc.CASES[name](T)
    outs = []
    for dev in ("cpu", cuda):
        res, caps, ix = rc.build(segs, max_pes, max_nal, dev)
        offs, size = remux.layout_out(caps, max_nal, headroom=256, audio_gap=g)
        out = torch.full((size,), rc.FILL, dtype=torch.uint8, device=res.es.device)
        outs.append(remux.remux_batch(res, ix, caps, out, offs, max_aframes=max_aframes, audio_gap=g, headroom=256))
    host, dev = outs
    for name_ in ("rinfo", "vsamples", "asamples", "out"):
        fc.assert_equal(name_, getattr(dev, name_), getattr(host, name_).numpy())
    A0, P = remux.RINFO["audio_box_offset"], remux.RINFO["video_payload_bytes"]
    assert torch.equal(host.rinfo[:, A0], (8 + host.rinfo[:, P] + g + 15) // 16 * 16)
