"""Remux on the MI355X (``kernels/remux.hip``): the kernels' three tables and every byte of the
output buffer equal the independent sequential reference (``tests/remux_cases.py``) on the
hand-built cases -- every output alignment against every source alignment, NAL bodies around
the copy tile's edges, dropped NALs, codecs, table overflows, timestamps, ADTS walks, empty
and mixed batches --, nothing is written outside the tables, the scratch and the payloads, the
result equals the host implementation on demuxed segments, and it reaches the pipeline's
results with the batch's event as the only wait."""
import numpy as np
import pytest
import torch

import remux_cases as rc
from hlsjs_p2p_wrapper_amd.ops import esindex, remux, tsdemux
from hlsjs_p2p_wrapper_amd.ops._native import device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tile(cuda):
    return device().remux_tile_bytes()


@pytest.mark.parametrize("case", sorted(rc.CASES))
def test_hand_built_cases_match_the_reference(case, cuda, tile):
    _, _, _, _, rx, ref = rc.run_case(case, tile, cuda)
    assert rx.rinfo.is_cuda and rx.vsamples.is_cuda and rx.asamples.is_cuda and rx.out.is_cuda
    rc.assert_remux_equal(rx, ref)


def raw_call(cuda, name, scratch_short=0, op=None):
    """One case through the raw binding (or the dispatcher op) with 4 sentinel elements behind
    every output tensor and behind a scratch of exactly the exported size."""
    segs, max_pes, max_nal, max_af = rc.CASES[name](device().remux_tile_bytes())
    res, caps, ix = rc.build(segs, max_pes, max_nal, cuda)
    B, T = len(segs), device().remux_tile_bytes()
    cap = np.asarray(caps, np.int64)
    offs, size = remux.layout_out(caps, max_nal)
    tp = np.zeros(B + 1, np.int64)
    np.cumsum((remux.remux_out_bytes(cap, max_nal) + T - 1) // T, out=tp[1:])

    def guarded(n, dtype, fill):
        return torch.full((n + 4,), fill, dtype=dtype, device=cuda)

    scratch = guarded(device().remux_scratch_words(B, max_nal, max_af) - scratch_short, torch.int32, 0x5A5A5A5A)
    vs = guarded(B * max_pes * 5, torch.int32, 0x5A5A5A5A)
    asamp = guarded(B * max_af * 2, torch.int32, 0x5A5A5A5A)
    rinfo = guarded(B * 8, torch.int64, 0x5A5A5A5A)
    out = guarded(size, torch.uint8, rc.FILL)
    dev = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    call = op or device().remux
    given = scratch[:len(scratch) - 4] if scratch_short else scratch
    args = (res.es, dev(res.es_offs), dev(cap), dev(tp), int(tp[-1]), res.info, res.pes, max_pes, max_nal, ix.nal,
            ix.au, ix.aframes, ix.sinfo, max_af, given, vs, asamp, rinfo, out, dev(offs))
    ref = rc.ref_batch(res, ix, caps, offs, size + 4, max_af)
    return call, args, (scratch, vs, asamp, rinfo, out), ref, (B, max_pes, max_af)


def check_raw(tensors, ref, dims):
    scratch, vs, asamp, rinfo, out = tensors
    B, max_pes, max_af = dims
    for t in (scratch, vs, asamp, rinfo):
        assert (t[-4:] == 0x5A5A5A5A).all()
    assert np.array_equal(rinfo[:-4].cpu().numpy().reshape(B, 8), ref[0])
    assert np.array_equal(vs[:-4].cpu().numpy().reshape(B, max_pes, 5), ref[1])
    assert np.array_equal(asamp[:-4].cpu().numpy().reshape(B, max_af, 2), ref[2])
    assert np.array_equal(out.cpu().numpy(), ref[3])  # the sentinels and all slack included


def test_no_byte_is_written_outside_the_tables_or_the_region(cuda):
    call, args, tensors, ref, dims = raw_call(cuda, "mixed")
    call(*args)
    check_raw(tensors, ref, dims)


def test_a_short_scratch_is_rejected_before_any_launch(cuda):
    call, args, tensors, _, _ = raw_call(cuda, "dropping", scratch_short=1)
    with pytest.raises(RuntimeError, match="scratch too small"):
        call(*args)
    torch.cuda.synchronize()
    assert (tensors[3] == 0x5A5A5A5A).all()


def test_the_dispatcher_op_equals_the_binding(cuda):
    assert hasattr(torch.ops.hlsp2p, "remux")
    call, args, tensors, ref, dims = raw_call(cuda, "codecs", op=torch.ops.hlsp2p.remux)
    call(*args)
    check_raw(tensors, ref, dims)
    _, args2, tensors2, _, _ = raw_call(cuda, "codecs")
    device().remux(*args2)
    for a, b in zip(tensors[1:], tensors2[1:]):
        assert torch.equal(a, b)


def test_unaligned_offsets_and_small_regions_are_rejected(cuda):
    segs, max_pes, max_nal, _ = rc.CASES["dropping"](0)
    res, caps, ix = rc.build(segs, max_pes, max_nal, cuda)
    offs, size = remux.layout_out(caps, max_nal)
    out = torch.zeros(size + 256, dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError, match="256-byte aligned"):
        remux.remux_batch(res, ix, caps, out, offs + 16)
    with pytest.raises(ValueError, match="out of bounds"):
        remux.remux_batch(res, ix, caps, out[:caps[0] + max_nal + 31], offs)
    with pytest.raises(ValueError, match="one device"):
        remux.remux_batch(res, ix, caps, out.cpu(), offs)


def test_remux_matches_the_host_implementation_on_demuxed_segments(cuda):
    """The index test's four segment shapes through demux, index and remux on both devices:
    everything equal, byte for byte."""
    segs = []
    for i, (tb, id3) in enumerate([(400_000, False), (400_000, True), (1_000_000, False), (188 * 300, True)]):
        seg, _ = tsdemux.mux_segment(target_bytes=tb, with_id3=id3, seed=11 + i, sn=i, start_time=4.0 * i)
        segs.append(seg)
    offs, pos = [], 0
    for s in segs:
        offs.append(pos)
        pos += (len(s) + 255) // 256 * 256
    buf = np.zeros(pos + 256, np.uint8)
    for o, s in zip(offs, segs):
        buf[o:o + len(s)] = s
    lens = [len(s) for s in segs]
    cpu = tsdemux.demux_batch(torch.from_numpy(buf), offs, lens, torch.zeros(pos + 256, dtype=torch.uint8), offs)
    gpu = tsdemux.demux_batch(torch.from_numpy(buf).to(cuda), offs, lens,
                              torch.zeros(pos + 256, dtype=torch.uint8, device=cuda), offs)
    hi, gi = esindex.index_batch(cpu, lens), esindex.index_batch(gpu, lens)
    oo, size = remux.layout_out(lens, hi.nal.shape[1])
    hr = remux.remux_batch(cpu, hi, lens, torch.full((size,), rc.FILL, dtype=torch.uint8), oo)
    gr = remux.remux_batch(gpu, gi, lens, torch.full((size,), rc.FILL, dtype=torch.uint8, device=cuda), oo)
    for name in ("rinfo", "vsamples", "asamples", "out"):
        assert torch.equal(getattr(gr, name).cpu(), getattr(hr, name)), name
    R = remux.RINFO
    assert hr.rinfo[:, R["status"]].tolist() == [0] * 4 and hr.rinfo[:, R["n_vsamples"]].tolist() == [100] * 4
    assert (hr.rinfo[:, R["video_payload_bytes"]] > 0).all() and (hr.rinfo[:, R["audio_payload_bytes"]] > 0).all()


def test_pipeline_remuxes_on_the_gpu_with_one_wait(cuda, monkeypatch):
    """A batch of encrypted and clear fragments through ``MediaPipeline`` with ``remux=True`` on
    some: their ``fmp4`` equals the reference, the others have none, and the batch's event is
    the only host wait (no device-wide or stream sync, no blocking copy, between launch and the
    callbacks)."""
    from test_remux import check_fmp4, run_pipeline

    waits = []
    real = torch.cuda.Event.synchronize
    monkeypatch.setattr(torch.cuda.Event, "synchronize", lambda self: (waits.append("event"), real(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: waits.append("device"))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: waits.append("stream"))
    ask = [True, False, True, True]
    jobs, out = run_pipeline(cuda, ask)
    assert waits == ["event"], waits
    monkeypatch.undo()
    check_fmp4(jobs, out, ask)
    assert out[0]["fmp4"]["video"]["mdat"].is_cuda and out[0]["fmp4"]["audio"]["samples"].is_cuda
