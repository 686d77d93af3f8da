"""Sample index on the MI355X (``kernels/es_index.hip``): the kernels' four tensors equal the
independent sequential reference (``tests/esindex_cases.py``) exactly on the hand-built edge
cases -- start codes on every lane, wave, iteration and tile edge, the end of the video ES,
zero runs, table overflow, access-unit mapping, ADTS walks -- equal the host implementation
on demuxed segments, and reach the pipeline's results with the batch's event as the only wait."""
import numpy as np
import pytest
import torch

from esindex_cases import CASES, assert_index_equal, boundary_segments, hand_batch, ref_batch
from hlsjs_p2p_wrapper_amd.ops import esindex, tsdemux
from hlsjs_p2p_wrapper_amd.ops._native import device
from test_esindex import check_samples, run_pipeline

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tile(cuda):
    return device().es_index_tile_bytes()


@pytest.mark.parametrize("case", sorted(CASES))
def test_hand_built_cases_match_the_reference(case, cuda, tile):
    segs, max_pes, max_nal = CASES[case](tile)
    res, caps = hand_batch(segs, cuda, max_pes)
    ix = esindex.index_batch(res, caps, max_nal=max_nal)
    assert ix.sinfo.is_cuda and ix.nal.is_cuda and ix.au.is_cuda and ix.aframes.is_cuda
    assert_index_equal(ix, ref_batch(res, caps, max_nal))


def test_boundary_batch_finds_every_planted_start_code(cuda, tile):
    """Counted on the result itself: every planted position but ``n - 3`` (no header byte
    inside the ES) is a NAL start, in offset order, and nothing else is."""
    segs, groups = boundary_segments(tile)
    n = 2 * tile + 40
    res, caps = hand_batch(segs, cuda)
    ix = esindex.index_batch(res, caps)
    full = [i for i, s in enumerate(segs) if len(s["video"]) == n]
    assert len(full) == len(groups) + 1
    for i, g in zip(full, groups):
        want = [p + 3 for p in g if p + 3 < n]
        assert ix.segment(i)["nal"][:, 0].tolist() == want, g
    s = ix.segment(full[-1])  # the 4-byte forms: the NAL before each one loses exactly one byte
    assert s["nal"][:, 0].tolist() == [4, tile + 2, 2 * tile + 3]
    assert s["nal"][:, 1].tolist() == [tile - 2 - 4, 2 * tile - 1 - (tile + 2), n - (2 * tile + 3)]
    sizes = {len(x["video"]): i for i, x in enumerate(segs)}
    assert [int(ix.sinfo[sizes[k], 1]) for k in (0, 1, 3, 4)] == [0, 0, 0, 1]


def test_no_row_is_written_past_the_tables(cuda):
    """65 and 200 NALs into tables of 64 rows through the raw binding, with sentinel rows behind
    every output and behind the scratch."""
    segs, max_pes, max_nal = CASES["overflow"](0)
    res, caps = hand_batch(segs, cuda, max_pes)
    B, T = len(segs), device().es_index_tile_bytes()
    cap = np.asarray(caps, np.int64)
    tp = np.zeros(B + 1, np.int64)
    np.cumsum((cap + T - 1) // T, out=tp[1:])
    total = int(tp[-1])

    def guarded(n, dtype):
        return torch.full((n + 4,), 0x5A5A5A5A, dtype=dtype, device=cuda)

    scratch = guarded(2 * total + B * (max_nal + 1), torch.int32)
    nal, au = guarded(B * max_nal * 4, torch.int32), guarded(B * max_pes * 4, torch.int32)
    af, sinfo = guarded(B * max_pes * 2, torch.int32), guarded(B * 8, torch.int64)
    dev = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    device().es_index(res.es, dev(res.es_offs), dev(cap), dev(tp), total, res.info, res.pes, max_pes, max_nal, scratch,
                      nal, au, af, sinfo)
    for t in (scratch, nal, au, af, sinfo):
        assert (t[-4:] == 0x5A5A5A5A).all()
    ref = ref_batch(res, caps, max_nal)
    assert np.array_equal(nal[:-4].cpu().numpy().reshape(B, max_nal, 4), ref[0])
    assert np.array_equal(sinfo[:-4].cpu().numpy().reshape(B, 8), ref[3])
    assert sinfo[:-4].view(B, 8)[:, 1].tolist() == [65, 200, 64, 63]


def test_unaligned_offsets_are_rejected(cuda):
    res, caps = hand_batch(CASES["zero_runs"](0)[0], cuda)
    res.es_offs = res.es_offs + 8
    with pytest.raises(ValueError, match="16-byte aligned"):
        esindex.index_batch(res, caps)


def test_index_matches_the_host_implementation_on_demuxed_segments(cuda):
    """The demux test's four segment shapes (the 3 MB one cut to 400 KB) through demux and
    index on both devices: everything equal."""
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
    for name in ("sinfo", "nal", "au", "aframes"):
        assert torch.equal(getattr(gi, name).cpu(), getattr(hi, name)), name
    S = esindex.SINFO
    assert hi.sinfo[:, S["status"]].tolist() == [0] * 4 and hi.sinfo[:, S["n_au"]].tolist() == [100] * 4
    assert hi.sinfo[:, S["n_nal"]].tolist() == [4 + 2 * 99] * 4


def test_pipeline_indexes_on_the_gpu_with_one_wait(cuda, monkeypatch):
    """A batch of encrypted and clear fragments through ``MediaPipeline`` with ``index=True`` on
    some: their ``samples`` equal the reference, and the batch's event is the only host wait
    (no device-wide or stream sync, no blocking copy, between launch and the callbacks)."""
    waits = []
    real = torch.cuda.Event.synchronize
    monkeypatch.setattr(torch.cuda.Event, "synchronize", lambda self: (waits.append("event"), real(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: waits.append("device"))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", lambda self: waits.append("stream"))
    ask = [True, False, True, True]
    jobs, out = run_pipeline(cuda, ask)
    assert waits == ["event"], waits
    monkeypatch.undo()
    check_samples(jobs, out, ask)
    assert out[0]["samples"]["nal"].is_cuda
