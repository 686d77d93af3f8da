"""AC-3 / E-AC-3 behind the remux on the MI355X (``kernels/ac3_audio.hip``): the batches of
``test_ac3audio.py`` through the same builders.  The six outputs equal the independent reference
and the host implementation bit for bit: the walk cases, the header cases, the mixed batches with
and without the MPEG audio op in front, the overflow, damaged PES rows, the fuzz, all 16 residues of
the audio ES start, 255 / 256 / 257 audio PES (the carry between rounds of the workgroup) and
payloads around one and two 16 KiB tiles.  The outputs of a raw call sit behind canaries, the
dispatcher op agrees with the pybind entry, short or misaligned arguments are rejected on the host,
and ``fragment_moof`` with the ``Ac3Audio`` equals the host.  The largest batch is about 34 KB of ES."""
import numpy as np
import pytest
import torch

import ac3audio_cases as ac
import remux_cases as rc
from hlsjs_p2p_wrapper_amd.ops import ac3audio, fragment, remux
from hlsjs_p2p_wrapper_amd.ops._native import device
from hlsjs_p2p_wrapper_amd.ops.desc import pack_to_device

pytestmark = pytest.mark.gpu
PAD = 64  # canary elements behind each output of a raw call
OUTS = ("scratch", "dframes", "ac3info", "mpainfo", "asamples", "rinfo", "out")


@pytest.mark.parametrize("name", sorted(ac.BATCHES))
def test_batches_match_the_reference_and_the_host(name, cuda):
    r = ac.run(name, cuda)
    assert r.da.dframes.is_cuda and r.da.ac3info.is_cuda and r.da.mpainfo.is_cuda
    got = r.got()
    ac.assert_equal(got, ac.expected(name))
    ac.assert_equal(got, ac.host(name).got())
    assert np.array_equal(r.res.es.cpu().numpy(), r.es_before)  # the ES is only read
    if r.with_mpa:
        assert np.array_equal(r.ma.mpainfo.cpu().numpy(), r.mpa_before)  # the MpegAudio's own tensor is never written


def raw_args(r, cuda, short=None, oo_shift=0):
    """The raw call's arguments for batch ``r`` (a CPU run: what the ops in front left is taken from
    it), every output with ``PAD`` canary elements behind it (``short``: that one an element short)."""
    B = len(r.caps)
    region = np.asarray(r.rx.region, np.int64)
    tile = device().ac3_audio_tile_bytes()
    tp = np.zeros(B + 1, np.int64)
    np.cumsum((region + tile - 1) // tile, out=tp[1:])
    d = pack_to_device({"eo": np.asarray(r.res.es_offs, np.int64), "cap": np.asarray(r.caps, np.int64), "tp": tp,
                        "rg": region, "oo": np.asarray(r.offs, np.int64) + oo_shift}, cuda)
    outs = {"scratch": np.zeros(device().mpa_scratch_words(B, r.max_pes), np.int32),
            "dframes": np.zeros(B * r.max_pes * 2, np.int32), "ac3info": np.zeros(B * 16, np.int64),
            "mpainfo": np.zeros(B * 8, np.int64), "asamples": r.before["asamples"].reshape(-1),
            "rinfo": r.before["rinfo"].reshape(-1), "out": r.before["out"]}
    assert tuple(outs) == OUTS
    flat = {}
    for k, a in outs.items():
        canary = 0x3C if k == "out" else -77
        body = a if k != short else a[:-1]
        tail = np.full(PAD if k != short else 0, canary, a.dtype)
        flat[k] = torch.from_numpy(np.concatenate([body, tail])).to(cuda)
    mpa_in = None if r.mpa_before is None else torch.from_numpy(r.mpa_before.reshape(-1).copy()).to(cuda)
    args = (r.res.es.to(cuda), d["eo"], d["cap"], d["tp"], int(tp[-1]), r.res.info.to(cuda), r.res.pes.to(cuda),
            r.max_pes, d["rg"], r.max_aframes, *(flat[k] for k in outs), d["oo"], mpa_in)
    return args, flat


@pytest.mark.parametrize("name", ["walk", "walk_header", "damaged", "fuzz1", "overflow", "tile_p2", "mixed_mpa"])
def test_canaries_and_the_dispatcher_op(name, cuda):
    r, want = ac.host(name), ac.expected(name)
    for op in (device().ac3_audio, torch.ops.hlsp2p.ac3_audio):
        args, flat = raw_args(r, cuda)
        op(*args)
        torch.cuda.synchronize()
        for k in ac.NAMES:
            canary = 0x3C if k == "out" else -77
            got = flat[k].cpu().numpy()
            assert (got[-PAD:] == canary).all(), k
            assert np.array_equal(got[:-PAD], want[k].reshape(-1)), k
        assert (flat["scratch"][-PAD:] == -77).all()
        if args[-1] is not None:
            assert np.array_equal(args[-1].cpu().numpy(), r.mpa_before.reshape(-1))
    schema = str(torch.ops.hlsp2p.ac3_audio.default._schema)
    for name_ in OUTS:
        assert f"!) {name_}" in schema, schema
    assert "Tensor? mpa_in=None" in schema


def test_short_or_misaligned_arguments_are_rejected_on_the_host(cuda):
    r = ac.host("mixed_mpa")
    for short in ("scratch", "dframes", "ac3info", "mpainfo", "asamples", "rinfo"):
        args, _ = raw_args(r, cuda, short=short)
        with pytest.raises(RuntimeError, match=f"{short} too small"):
            device().ac3_audio(*args)
    args, flat = raw_args(r, cuda)
    wrong = list(args)
    wrong[-1] = args[-1][:-1]
    with pytest.raises(RuntimeError, match="mpa_in too small"):
        device().ac3_audio(*wrong)
    wrong = list(args)
    wrong[16] = flat["out"][1:]  # out: not 16-byte aligned
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        device().ac3_audio(*wrong)
    wrong = list(args)
    wrong[7] = 0
    with pytest.raises(RuntimeError, match="out of range"):
        device().ac3_audio(*wrong)
    torch.cuda.synchronize()
    for k, words in (("ac3info", 16), ("mpainfo", 8)):
        assert (flat[k].cpu() == torch.cat([torch.zeros(len(r.caps) * words, dtype=torch.int64),
                                            torch.full((PAD,), -77)])).all()  # nothing was launched
    d = ac.run("mixed_mpa", cuda)
    shifted = remux.Remuxed(d.rx.rinfo, d.rx.vsamples, d.rx.asamples, d.rx.out, d.rx.out_offs + 16, d.rx.headroom,
                            d.rx.audio_gap, d.rx.region)
    with pytest.raises(ValueError, match="256-byte aligned"):
        ac3audio.ac3_audio_batch(d.res, shifted, d.caps)
    with pytest.raises(ValueError, match="one device"):
        ac3audio.ac3_audio_batch(d.res, r.rx, d.caps)
    with pytest.raises(ValueError, match="mpeg_audio does not belong"):
        ac3audio.ac3_audio_batch(d.res, d.rx, d.caps, mpeg_audio=r.ma)  # a host tensor
    empty = ac.Run([], 4, 8, True, cuda)
    assert empty.da.ac3info.shape == (0, 16) and empty.da.mpainfo.shape == (0, 8)
    assert empty.da.dframes.shape == (0, 4, 2) and empty.da.ac3info.is_cuda


@pytest.mark.parametrize("name", ["mixed_mpa", "walk"])
def test_fragment_moof_with_the_ac3_audio_equals_the_host(name, cuda):
    results = []
    for dev in (cuda, "cpu"):
        segs, max_pes, max_aframes, with_mpa = ac.BATCHES[name]()
        r = ac.Run(segs, max_pes, max_aframes, with_mpa, dev)
        seqs = np.arange(3, 3 + len(r.caps))
        fr = fragment.fragment_batch(r.rx, r.ix, seqs, mpeg_audio=r.da)
        plain = ac.Run(segs, max_pes, max_aframes, with_mpa, dev)
        fr0 = fragment.fragment_batch(plain.rx, plain.ix, seqs)
        results.append((fr.finfo.cpu().numpy(), r.out.cpu().numpy(), fr0.finfo.cpu().numpy(), plain.out.cpu().numpy()))
        if dev == "cpu":
            continue
        for i in range(len(r.caps)):  # the audio tfhd duration is 1536, the tfdt in units of the row's rate
            m, rx, f = r.da.segment(i), r.rx.segment(i), fr.segment(i)
            if not m["has_config"]:
                continue
            p = rc.parse_moof(f["audio"][:f["audio_moof_bytes"]])
            assert p["default_duration"] == 1536 and p["count"] == len(rx["asamples"])
            assert f["audio_tfdt"] == p["base"] == (rx["audio_base_pts"] * m["sample_rate"] + 45000) // 90000
    for got, want in zip(*results):
        assert np.array_equal(got, want)
    assert not np.array_equal(results[0][1], results[0][3])  # the argument changes the audio tfhd and tfdt
