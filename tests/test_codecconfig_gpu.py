"""Codec configuration on the MI355X (``kernels/codec_config.hip``): ``cinfo`` and ``ps`` equal, bit
for bit, the independent sequential reference (``tests/codec_cases.py``) and the host
implementation on every hand-built case, the fuzz batch and the 64-segment mix; the dispatcher op
agrees with the pybind entry; nothing is written behind the two outputs; a short output is
rejected on the host; and the pipeline's init segments equal the CPU pipeline's."""
import numpy as np
import pytest
import torch

import codec_cases as cc
from hlsjs_p2p_wrapper_amd.ops import codecconfig
from hlsjs_p2p_wrapper_amd.ops._native import device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_cases_match_the_reference_and_the_host(name, cuda):
    case = cc.CASES[name]()
    res, ix, caps = cc.build(case, cuda)
    cfg = codecconfig.config_batch(res, ix, caps, case.max_ps)
    assert cfg.cinfo.is_cuda and cfg.ps.is_cuda
    cc.assert_config_equal(cfg, cc.ref_batch(res, ix, caps, case.max_ps))
    hres, hix, _ = cc.build(case, "cpu")
    host = codecconfig.config_batch(hres, hix, caps, case.max_ps)
    assert torch.equal(cfg.cinfo.cpu(), host.cinfo) and torch.equal(cfg.ps.cpu(), host.ps)


def raw_call(cuda, name, short=None, op=None):
    """One case through the raw binding (or the dispatcher op) with 4 sentinel elements behind both
    outputs (``short``: that output one element short of its size, and no sentinels behind it)."""
    case = cc.CASES[name]()
    res, ix, caps = cc.build(case, cuda)
    B, max_ps = len(case.segs), case.max_ps
    sizes = {"cinfo": B * 19, "ps": B * 2 * max_ps}
    extra = {k: (-1 if k == short else 4) for k in sizes}
    cinfo = torch.full((sizes["cinfo"] + extra["cinfo"],), 0x5A5A5A5A, dtype=torch.int32, device=cuda)
    ps = torch.full((sizes["ps"] + extra["ps"],), 0x5A, dtype=torch.uint8, device=cuda)
    dev = lambda a: torch.from_numpy(np.asarray(a, np.int64)).to(cuda)  # noqa: E731
    args = (res.es, dev(res.es_offs), dev(caps), res.info, res.pes, case.max_pes, case.max_nal, ix.nal, ix.au,
            ix.aframes, ix.sinfo, max_ps, cinfo, ps)
    return (op or device().codec_config), args, (cinfo, ps), cc.ref_batch(res, ix, caps, max_ps), sizes


@pytest.mark.parametrize("name", ["mixed", "copy_16"])
def test_dispatcher_op_agrees_with_the_pybind_entry_and_writes_nothing_behind(name, cuda):
    outs = []
    for op in (None, torch.ops.hlsp2p.codec_config):
        call, args, (cinfo, ps), ref, sizes = raw_call(cuda, name, op=op)
        call(*args)
        assert (cinfo[sizes["cinfo"]:].cpu() == 0x5A5A5A5A).all() and (ps[sizes["ps"]:].cpu() == 0x5A).all()
        assert np.array_equal(cinfo[:sizes["cinfo"]].cpu().numpy().reshape(ref[0].shape), ref[0])
        assert np.array_equal(ps[:sizes["ps"]].cpu().numpy().reshape(ref[1].shape), ref[1])
        outs.append((cinfo.cpu(), ps.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("short", ["cinfo", "ps"])
def test_a_short_output_is_rejected_on_the_host(short, cuda):
    call, args, (cinfo, ps), _, _ = raw_call(cuda, "other", short=short)
    with pytest.raises(RuntimeError, match=f"{short} too small"):
        call(*args)
    torch.cuda.synchronize()
    assert (cinfo.cpu() == 0x5A5A5A5A).all() and (ps.cpu() == 0x5A).all()
    call, args, _, _, _ = raw_call(cuda, "other")
    with pytest.raises(RuntimeError, match="max_ps"):
        call(*args[:11], 24, *args[12:])


def test_pipeline_init_segments_equal_the_cpu_pipelines(cuda):
    from test_codecconfig import check_config, run_pipeline

    ask = [True, False, True, True]
    jobs, out = run_pipeline(cuda, ask)
    check_config(jobs, out, ask)
    _, host = run_pipeline("cpu", ask)
    for n in (0, 2, 3):
        for track in ("video", "audio"):
            assert out[n]["fmp4"][track]["init"] == host[n]["fmp4"][track]["init"] is not None
            assert out[n]["fmp4"][track]["codec"] == host[n]["fmp4"][track]["codec"]
        assert dict(out[n]["fmp4"]["config"]) == dict(host[n]["fmp4"]["config"])
