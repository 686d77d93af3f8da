"""HEVC configuration on the MI355X (``kernels/hevc_config.hip``): ``hinfo`` and ``hps`` equal, bit
for bit, the independent sequential reference (``tests/hevc_cases.py``) and the host implementation
on every hand-built case (rows 255 / 256 of the search, escapes at SPS bytes 63 / 64 and 255 / 256
with ``max_ps`` 512 among them), the fuzz batch and the 64-segment mix; the dispatcher op agrees
with the pybind entry; nothing is written behind the two outputs; short outputs and mixed devices
are rejected on the host; and the pipeline's HEVC init segments equal the CPU pipeline's."""
import numpy as np
import pytest
import torch

import hevc_cases as hc
from hlsjs_p2p_wrapper_amd.ops import hevcconfig
from hlsjs_p2p_wrapper_amd.ops._native import device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_cases_match_the_reference_and_the_host(name, cuda):
    case = hc.CASES[name]()
    assert len(case.segs) <= 256  # a few KB each: the test runs in seconds
    res, ix, caps = hc.build(case, cuda)
    cfg = hevcconfig.hevc_config_batch(res, ix, caps, case.max_ps)
    assert cfg.hinfo.is_cuda and cfg.hps.is_cuda
    hc.assert_hevc_equal(cfg, hc.ref_batch(res, ix, caps, case.max_ps))
    hres, hix, _ = hc.build(case, "cpu")
    host = hevcconfig.hevc_config_batch(hres, hix, caps, case.max_ps)
    assert torch.equal(cfg.hinfo.cpu(), host.hinfo) and torch.equal(cfg.hps.cpu(), host.hps)


def test_the_kernels_own_edges_are_in_the_cases(cuda):
    """Stated on the kernel's results: the three types on both sides of a 256-row round, and an
    escape on both sides of a wave's 64 bytes and of a 256-byte unescape round."""
    case = hc.search_cases()
    res, ix, caps = hc.build(case, cuda)
    cfg = hevcconfig.hevc_config_batch(res, ix, caps, case.max_ps)
    cols = [hevcconfig.HINFO[k] for k in ("status", "vps_nal", "sps_nal", "pps_nal")]
    got = cfg.hinfo[:, cols].cpu().tolist()
    assert got[1] == [0, 255, 256, 257] and got[2] == [0, 254, 255, 256] and got[3] == [0, 256, 257, 258]
    assert got[4] == [0, 511, 512, 513] and got[9] == [hevcconfig.HSTATUS["no_pps"], 518, 519, -1]
    case = hc.unescape_cases()
    assert case.max_ps == 512
    res, ix, caps = hc.build(case, cuda)
    cfg = hevcconfig.hevc_config_batch(res, ix, caps, case.max_ps)
    segs = [cfg.segment(i) for i in range(len(case.segs))]
    last = [hc.escape_positions(s["sps"])[-1] for s in segs[8:19]]
    assert last == [62, 63, 64, 65, 127, 128, 254, 255, 256, 257, 511]
    for s in segs[8:19]:
        assert s["status"] == 0 and (s["width"], s["height"]) == (1920, 1080)
        assert s["sps_rbsp_bytes"] == s["sps_bytes"] - 2 - len(hc.escape_positions(s["sps"]))
    moving = set()
    for i, s in enumerate(segs[20:]):
        moving |= set(hc.escape_positions(s["sps"]))
        assert (s["status"], s["width"], s["height"]) == (0, 1280 + i, 720 - 2 * i)
    assert {63, 64} <= moving


def raw_call(cuda, name, short=None, op=None):
    """One case through the raw binding (or the dispatcher op) with 4 sentinel elements behind both
    outputs (``short``: that output one element short of its size, and no sentinels behind it)."""
    case = hc.CASES[name]()
    res, ix, caps = hc.build(case, cuda)
    B, max_ps = len(case.segs), case.max_ps
    sizes = {"hinfo": B * 22, "hps": B * 3 * max_ps}
    extra = {k: (-1 if k == short else 4) for k in sizes}
    hinfo = torch.full((sizes["hinfo"] + extra["hinfo"],), 0x5A5A5A5A, dtype=torch.int32, device=cuda)
    hps = torch.full((sizes["hps"] + extra["hps"],), 0x5A, dtype=torch.uint8, device=cuda)
    dev = lambda a: torch.from_numpy(np.asarray(a, np.int64)).to(cuda)  # noqa: E731
    args = (res.es, dev(res.es_offs), dev(caps), res.info, res.pes, case.max_pes, case.max_nal, ix.nal, ix.au,
            ix.aframes, ix.sinfo, max_ps, hinfo, hps)
    return (op or device().hevc_config), args, (hinfo, hps), hc.ref_batch(res, ix, caps, max_ps), sizes


@pytest.mark.parametrize("name", ["mixed", "copy_16", "other"])
def test_dispatcher_op_agrees_with_the_pybind_entry_and_writes_nothing_behind(name, cuda):
    outs = []
    for op in (None, torch.ops.hlsp2p.hevc_config):
        call, args, (hinfo, hps), ref, sizes = raw_call(cuda, name, op=op)
        call(*args)
        assert (hinfo[sizes["hinfo"]:].cpu() == 0x5A5A5A5A).all() and (hps[sizes["hps"]:].cpu() == 0x5A).all()
        assert np.array_equal(hinfo[:sizes["hinfo"]].cpu().numpy().reshape(ref[0].shape), ref[0])
        assert np.array_equal(hps[:sizes["hps"]].cpu().numpy().reshape(ref[1].shape), ref[1])
        outs.append((hinfo.cpu(), hps.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("short", ["hinfo", "hps"])
def test_a_short_output_is_rejected_on_the_host(short, cuda):
    call, args, (hinfo, hps), _, _ = raw_call(cuda, "other", short=short)
    with pytest.raises(RuntimeError, match=f"{short} too small"):
        call(*args)
    torch.cuda.synchronize()
    assert (hinfo.cpu() == 0x5A5A5A5A).all() and (hps.cpu() == 0x5A).all()
    call, args, _, _, _ = raw_call(cuda, "other")
    with pytest.raises(RuntimeError, match="max_ps"):
        call(*args[:11], 24, *args[12:])


def test_mixed_devices_are_rejected_on_the_host(cuda):
    res, ix, caps = hc.build(hc.other_cases())
    _, ix_dev, _ = hc.build(hc.other_cases(), cuda)
    with pytest.raises(ValueError, match="one device"):
        hevcconfig.hevc_config_batch(res, ix_dev, caps)
    call, args, (hinfo, hps), _, _ = raw_call(cuda, "other")
    for slot, match in ((12, "hinfo must be a GPU tensor"), (13, "hps must be a GPU tensor"),
                        (7, "nal must be a GPU tensor")):
        moved = list(args)
        moved[slot] = args[slot].cpu()
        with pytest.raises(RuntimeError, match=match):
            call(*moved)
    torch.cuda.synchronize()
    assert (hinfo.cpu() == 0x5A5A5A5A).all() and (hps.cpu() == 0x5A).all()


def test_pipeline_hevc_init_segments_equal_the_cpu_pipelines(cuda):
    from test_hevcconfig import check_pipeline, hevc_jobs, run_pipeline

    jobs = hevc_jobs()
    out = run_pipeline(cuda, jobs)
    check_pipeline(jobs, out)
    host = run_pipeline("cpu", jobs)
    for n in range(len(jobs)):
        for track in ("video", "audio"):
            assert out[n]["fmp4"][track]["init"] == host[n]["fmp4"][track]["init"] is not None
            assert out[n]["fmp4"][track]["codec"] == host[n]["fmp4"][track]["codec"]
        assert dict(out[n]["fmp4"]["hevc"]) == dict(host[n]["fmp4"]["hevc"])
        assert dict(out[n]["fmp4"]["config"]) == dict(host[n]["fmp4"]["config"])
