"""Caption extraction on the MI355X (``kernels/captions.hip``): the cases of ``test_captions.py``
through the same builders.  All five tensors equal the independent reference and the host
implementation bit for bit; the ES is unchanged between its canaries; damaged rows leave every
output inside its tensor; the dispatcher op agrees with the pybind entry; misaligned offsets are
rejected on the host.  The largest batch is 71 KB."""
import numpy as np
import pytest
import torch

import captions_cases as cc
import esindex_cases as esc
from hlsjs_p2p_wrapper_amd.ops import captions, esindex
from hlsjs_p2p_wrapper_amd.ops._native import device

pytestmark = pytest.mark.gpu
PAD = 64  # canary elements behind each output and the scratch of a raw call


def run_raw(op, res, ix, caps, max_cc, cuda, enable=None, short=None):
    """``cc_extract`` through ``op`` on outputs with ``PAD`` canary elements behind each (``short``:
    that one an element short instead): the five arrays as a dict, after checking the canaries."""
    B, max_pes, max_nal = len(caps), int(res.pes.shape[2]), int(ix.nal.shape[1])
    shapes = {"ccsamples": ((B, max_cc, 8), torch.int32), "ccpts": ((B, max_cc), torch.int64),
              "ccbytes": ((B, max_cc, cc.SLOT), torch.uint8), "cc608": ((B, max_cc, 2, cc.FIELD), torch.uint8),
              "ccinfo": ((B, 8), torch.int64), "scratch": ((device().cc_scratch_words(B, max_nal),), torch.int32)}
    flat = {k: torch.full((int(np.prod(s)) + (PAD if k != short else -1),), 0x5A, dtype=dt, device=cuda)
            for k, (s, dt) in shapes.items()}
    dev = lambda a, dt: torch.from_numpy(np.asarray(a, dt)).to(cuda)  # noqa: E731
    en = np.ones(B, np.uint8) if enable is None else enable
    op(res.es, dev(res.es_offs, np.int64), dev(caps, np.int64), res.info, res.pes, max_pes, max_nal, ix.nal, ix.au,
       ix.aframes, ix.sinfo, dev(en, np.uint8), max_cc, flat["scratch"], *(flat[k] for k in cc.NAMES))
    torch.cuda.synchronize()
    for k in shapes:
        assert (flat[k][-PAD:] == 0x5A).all(), k
    return {k: flat[k][:-PAD].cpu().numpy().reshape(shapes[k][0]) for k in cc.NAMES}


@pytest.mark.parametrize("name", list(cc.CASES))
def test_cases_match_the_reference_and_the_host(name, cuda):
    res, caps, ix, max_cc = cc.batch(name, cuda)
    before = res.es.cpu()
    got = captions.caption_batch(res, ix, caps, max_cc=max_cc)
    assert got.ccinfo.is_cuda and got.cc608.is_cuda
    ref = cc.ref_batch(res, ix, caps, max_cc)
    cc.assert_captions_equal(got, ref)
    assert torch.equal(res.es.cpu(), before)
    hres, hcaps, hix, _ = cc.batch(name)
    assert torch.equal(ix.nal.cpu(), hix.nal) and torch.equal(ix.sinfo.cpu(), hix.sinfo)
    host = captions.caption_batch(hres, hix, hcaps, max_cc=max_cc)
    for field in cc.NAMES:
        assert torch.equal(getattr(got, field).cpu(), getattr(host, field)), field
    assert ref[4][:, captions.CCINFO["n_samples"]].sum() > 0


@pytest.mark.parametrize("mask", [[1, 0, 1], [0, 0, 0]])
def test_enable_masks(mask, cuda):
    res, caps, ix, max_cc = cc.batch("small", cuda)
    got = captions.caption_batch(res, ix, caps, max_cc=max_cc, enable=mask)
    cc.assert_captions_equal(got, cc.ref_batch(res, ix, caps, max_cc, enable=mask))


def test_default_and_extreme_max_cc(cuda):
    res, caps, ix, _ = cc.batch("small", cuda)
    for max_cc in (1, 512, 2048):
        got = captions.caption_batch(res, ix, caps, **({} if max_cc == 512 else {"max_cc": max_cc}))
        cc.assert_captions_equal(got, cc.ref_batch(res, ix, caps, max_cc))


def test_empty_batch(cuda):
    res, caps = esc.hand_batch([], cuda)
    got = captions.caption_batch(res, esindex.index_batch(res, caps, max_nal=8), caps, max_cc=4)
    assert got.ccinfo.shape == (0, 8) and got.ccbytes.shape == (0, 4, 96) and got.ccinfo.is_cuda


def test_damaged_rows_stay_in_bounds(cuda):
    res, caps, ix, max_cc = cc.batch("main", cuda)
    cc.damage(res, caps, ix)
    before = res.es.cpu()
    got = run_raw(device().cc_extract, res, ix, caps, max_cc, cuda)  # checks the canaries behind each output
    assert torch.equal(res.es.cpu(), before)
    cc.assert_captions_equal(got, cc.ref_batch(res, ix, caps, max_cc))


def test_dispatcher_op_agrees_with_the_pybind_entry(cuda):
    res, caps, ix, max_cc = cc.batch("small", cuda)
    ref = cc.ref_batch(res, ix, caps, max_cc)
    for op in (device().cc_extract, torch.ops.hlsp2p.cc_extract):
        cc.assert_captions_equal(run_raw(op, res, ix, caps, max_cc, cuda), ref)


def test_misaligned_offsets_and_short_outputs_are_rejected_on_the_host(cuda):
    res, caps, ix, max_cc = cc.batch("small", cuda)
    for short in ("scratch", "ccbytes", "ccinfo"):
        with pytest.raises(RuntimeError, match=f"{short} too small"):
            run_raw(device().cc_extract, res, ix, caps, max_cc, cuda, short=short)
    res.es_offs = res.es_offs + 8
    with pytest.raises(ValueError, match="16-byte aligned"):
        captions.caption_batch(res, ix, caps, max_cc=max_cc)
    res.es_offs = res.es_offs - 8
    with pytest.raises(ValueError, match="one device"):
        captions.caption_batch(res, cc.batch("small")[2], caps, max_cc=max_cc)
    with pytest.raises(ValueError, match="max_cc"):
        captions.caption_batch(res, ix, caps, max_cc=4096)
