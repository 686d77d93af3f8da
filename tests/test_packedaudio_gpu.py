"""The packed-audio demux on the MI355X (``kernels/packed_audio.hip``): the cases of
``test_packedaudio.py`` through the same builders.  All seven tensors equal the independent
reference and the host implementation bit for bit, for the walk through LDS tiles and for the one
through global memory; the source is unchanged; the outputs of a raw call sit behind canaries; the
dispatcher op agrees with the pybind entry; misaligned offsets and short outputs are rejected on
the host; the ops behind give what an audio-only MPEG-TS of the same frames gives.  The largest
batch is about 370 KB."""
import numpy as np
import pytest
import torch

import packedaudio_cases as pc
from hlsjs_p2p_wrapper_amd.ops import packedaudio
from hlsjs_p2p_wrapper_amd.ops._native import device
from test_packedaudio import check_equivalence

pytestmark = pytest.mark.gpu
PAD = 64  # canary elements behind each output of a raw call


def shapes(B, max_pes):
    return {"info": ((B, 24), torch.int64), "pes": ((B, 3, max_pes, 3), torch.int64), "nal": ((B, 1, 4), torch.int32),
            "au": ((B, max_pes, 4), torch.int32), "aframes": ((B, max_pes, 2), torch.int32),
            "sinfo": ((B, 8), torch.int64), "painfo": ((B, 8), torch.int64)}


def run_raw(op, buf, offs, lens, max_pes, cuda, short=None, **kw):
    """``packed_audio`` through ``op`` on outputs with ``PAD`` canary elements behind each (``short``:
    that one an element short instead): the seven arrays as a dict, after checking the canaries."""
    sh = shapes(len(offs), max_pes)
    flat = {k: torch.full((int(np.prod(s)) + (PAD if k != short else -1),), 0x5A, dtype=t, device=cuda)
            for k, (s, t) in sh.items()}
    dev = lambda a: torch.from_numpy(np.asarray(a, np.int64)).to(cuda)  # noqa: E731
    op(buf, dev(offs), dev(lens), dev(lens), max_pes, *(flat[k] for k in pc.NAMES), **kw)
    torch.cuda.synchronize()
    for k in sh:
        assert (flat[k][-PAD:] == 0x5A).all(), k
    return {k: flat[k][:-PAD].cpu().numpy().reshape(sh[k][0]) for k in pc.NAMES}


@pytest.mark.parametrize("name", list(pc.CASES))
def test_cases_match_the_reference_and_the_host(name, cuda):
    buf, offs, lens, max_pes = pc.batch(name, cuda)
    before = buf.cpu()
    ref = pc.ref_batch(before, offs, lens, max_pes)
    got = packedaudio.packed_audio_batch(buf, offs, lens, max_pes=max_pes)
    assert got.info.is_cuda and got.painfo.is_cuda and got.aframes.is_cuda
    pc.assert_equal(got, ref)
    pc.assert_equal(run_raw(device().packed_audio, buf, offs, lens, max_pes, cuda), ref)  # behind canaries
    pc.assert_equal(run_raw(device().packed_audio, buf, offs, lens, max_pes, cuda, staged=False), ref)
    assert torch.equal(buf.cpu(), before)
    host = packedaudio.packed_audio_batch(before, offs, lens, max_pes=max_pes)
    for field in pc.NAMES:
        assert torch.equal(getattr(got, field).cpu(), getattr(host, field)), field


def test_device_lengths_with_host_caps(cuda):
    """``lens`` as the decrypt leaves it: a device tensor; values beyond the cap and below zero are clamped."""
    buf, offs, lens, max_pes = pc.batch("counts", cuda)
    ref = pc.ref_batch(buf, offs, lens, max_pes)
    n = torch.tensor(lens, dtype=torch.int64, device=cuda)
    pc.assert_equal(packedaudio.packed_audio_batch(buf, offs, n + 9, caps=lens, max_pes=max_pes), ref)
    cut = [lens[0], -3] + [v - 5 for v in lens[2:]]
    want = pc.ref_batch(buf, offs, [max(v, 0) for v in cut], max_pes)
    n = torch.tensor(cut, device=cuda)
    pc.assert_equal(packedaudio.packed_audio_batch(buf, offs, n, caps=lens, max_pes=max_pes), want)


def test_default_limit_the_largest_and_empty_batch(cuda):
    buf, offs, lens, _ = pc.batch("overflow", cuda)
    for max_pes in (512, 1, packedaudio.MAX_PES_LIMIT):
        got = packedaudio.packed_audio_batch(buf, offs, lens, max_pes=max_pes)
        pc.assert_equal(got, pc.ref_batch(buf, offs, lens, max_pes))
    empty = packedaudio.packed_audio_batch(buf, [], [], max_pes=4)
    assert empty.painfo.shape == (0, 8) and empty.pes.shape == (0, 3, 4, 3) and empty.painfo.is_cuda


def test_dispatcher_op_agrees_with_the_pybind_entry(cuda):
    buf, offs, lens, max_pes = pc.batch("tags", cuda)
    ref = pc.ref_batch(buf, offs, lens, max_pes)
    for op in (device().packed_audio, torch.ops.hlsp2p.packed_audio):
        pc.assert_equal(run_raw(op, buf, offs, lens, max_pes, cuda), ref)
    assert device().packed_audio_tile_bytes() == packedaudio.tile_bytes()


def test_misaligned_offsets_and_short_outputs_are_rejected_on_the_host(cuda):
    buf, offs, lens, max_pes = pc.batch("counts", cuda)
    for short in pc.NAMES:
        with pytest.raises(RuntimeError, match=f"{short} too small"):
            run_raw(device().packed_audio, buf, offs, lens, max_pes, cuda, short=short)
    with pytest.raises(RuntimeError, match="1 to 4096"):
        run_raw(device().packed_audio, buf, offs, lens, 4097, cuda)
    with pytest.raises(ValueError, match="16-byte aligned"):
        packedaudio.packed_audio_batch(buf, [o + 8 for o in offs], lens, max_pes=max_pes)
    with pytest.raises(ValueError, match="partial dword"):
        i = next(i for i in range(len(offs)) if (offs[i] + lens[i]) % 4)  # a segment that ends inside a dword
        packedaudio.packed_audio_batch(buf[:offs[i] + lens[i]], offs[:i + 1], lens[:i + 1], max_pes=max_pes)
    with pytest.raises(ValueError, match="lens"):
        packedaudio.packed_audio_batch(buf, offs, torch.tensor(lens), caps=lens, max_pes=max_pes)


def test_the_ops_behind_give_what_an_audio_only_ts_gives(cuda):
    check_equivalence(cuda)
