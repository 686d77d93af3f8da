"""MPEG audio behind the remux on the MI355X (``kernels/mpeg_audio.hip``): the batches of
``test_mpegaudio.py`` through the same builders.  The five outputs equal the independent reference
and the host implementation bit for bit: the walk cases, the mixed batch, the overflow, damaged
PES rows, the fuzz, all 16 residues of the audio ES start, 255 / 256 / 257 audio PES (the carry
between rounds of the workgroup) and payloads around one and two 16 KiB tiles.  The outputs of a
raw call sit behind canaries, the dispatcher op agrees with the pybind entry, short or misaligned
arguments are rejected on the host, and ``fragment_moof`` with the new argument equals the host.
The largest batch is about 35 KB of ES."""
import numpy as np
import pytest
import torch

import mpegaudio_cases as mc
from hlsjs_p2p_wrapper_amd.ops import fragment, mpegaudio, remux
from hlsjs_p2p_wrapper_amd.ops._native import device
from hlsjs_p2p_wrapper_amd.ops.desc import pack_to_device

pytestmark = pytest.mark.gpu
PAD = 64  # canary elements behind each output of a raw call


@pytest.mark.parametrize("name", sorted(mc.BATCHES))
def test_batches_match_the_reference_and_the_host(name, cuda):
    r = mc.run(name, cuda)
    assert r.ma.mframes.is_cuda and r.ma.mpainfo.is_cuda
    got = r.got()
    mc.assert_equal(got, mc.expected(name))
    mc.assert_equal(got, mc.host(name).got())
    assert np.array_equal(r.res.es.cpu().numpy(), r.es_before)  # the ES is only read


def raw_args(r, cuda, short=None, oo_shift=0):
    """The raw call's arguments for batch ``r`` (a CPU run: what the remux left is taken from it),
    every output with ``PAD`` canary elements behind it (``short``: that one an element short)."""
    B = len(r.caps)
    region = np.asarray(r.rx.region, np.int64)
    tile = device().mpeg_audio_tile_bytes()
    tp = np.zeros(B + 1, np.int64)
    np.cumsum((region + tile - 1) // tile, out=tp[1:])
    d = pack_to_device({"eo": np.asarray(r.res.es_offs, np.int64), "cap": np.asarray(r.caps, np.int64), "tp": tp,
                        "rg": region, "oo": np.asarray(r.offs, np.int64) + oo_shift}, cuda)
    outs = {"scratch": np.zeros(device().mpa_scratch_words(B, r.max_pes), np.int32),
            "mframes": np.zeros(B * r.max_pes * 2, np.int32), "mpainfo": np.zeros(B * 8, np.int64),
            "asamples": r.before["asamples"].reshape(-1), "rinfo": r.before["rinfo"].reshape(-1),
            "out": r.before["out"]}
    flat = {}
    for k, a in outs.items():
        canary = 0x3C if k == "out" else -77
        body = a if k != short else a[:-1]
        tail = np.full(PAD if k != short else 0, canary, a.dtype)
        flat[k] = torch.from_numpy(np.concatenate([body, tail])).to(cuda)
    args = (r.res.es.to(cuda), d["eo"], d["cap"], d["tp"], int(tp[-1]), r.res.info.to(cuda), r.res.pes.to(cuda),
            r.max_pes, d["rg"], r.max_aframes, *(flat[k] for k in outs), d["oo"])
    return args, flat


@pytest.mark.parametrize("name", ["walk", "damaged", "fuzz1", "overflow", "tile_p1"])
def test_canaries_and_the_dispatcher_op(name, cuda):
    r, want = mc.host(name), mc.expected(name)
    for op in (device().mpeg_audio, torch.ops.hlsp2p.mpeg_audio):
        args, flat = raw_args(r, cuda)
        op(*args)
        torch.cuda.synchronize()
        for k in mc.NAMES:
            canary = 0x3C if k == "out" else -77
            got = flat[k].cpu().numpy()
            assert (got[-PAD:] == canary).all(), k
            assert np.array_equal(got[:-PAD], want[k].reshape(-1)), k
        assert (flat["scratch"][-PAD:] == -77).all()
    schema = str(torch.ops.hlsp2p.mpeg_audio.default._schema)
    for name_ in ("scratch", "mframes", "mpainfo", "asamples", "rinfo", "out"):
        assert f"!) {name_}" in schema, schema


def test_short_or_misaligned_arguments_are_rejected_on_the_host(cuda):
    r = mc.host("mixed")
    for short in ("scratch", "mframes", "mpainfo", "asamples", "rinfo"):
        args, _ = raw_args(r, cuda, short=short)
        with pytest.raises(RuntimeError, match=f"{short} too small"):
            device().mpeg_audio(*args)
    args, flat = raw_args(r, cuda)
    wrong = list(args)
    wrong[15] = flat["out"][1:]  # out: not 16-byte aligned
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        device().mpeg_audio(*wrong)
    wrong = list(args)
    wrong[7] = 0
    with pytest.raises(RuntimeError, match="out of range"):
        device().mpeg_audio(*wrong)
    torch.cuda.synchronize()
    assert (flat["mpainfo"].cpu() == torch.cat([torch.zeros(len(r.caps) * 8, dtype=torch.int64),
                                                torch.full((PAD,), -77)])).all()  # nothing was launched
    d = mc.run("mixed", cuda)
    shifted = remux.Remuxed(d.rx.rinfo, d.rx.vsamples, d.rx.asamples, d.rx.out, d.rx.out_offs + 16, d.rx.headroom,
                            d.rx.audio_gap, d.rx.region)
    with pytest.raises(ValueError, match="256-byte aligned"):
        mpegaudio.mpeg_audio_batch(d.res, shifted, d.caps)
    with pytest.raises(ValueError, match="one device"):
        mpegaudio.mpeg_audio_batch(d.res, r.rx, d.caps)
    empty = mc.Run([], 4, 8, cuda)
    assert empty.ma.mpainfo.shape == (0, 8) and empty.ma.mframes.shape == (0, 4, 2) and empty.ma.mpainfo.is_cuda


@pytest.mark.parametrize("name", ["mixed", "walk"])
def test_fragment_moof_with_the_new_argument_equals_the_host(name, cuda):
    seqs = None
    results = []
    for dev in (cuda, "cpu"):
        segs, max_pes, max_aframes = mc.BATCHES[name]()
        r = mc.Run(segs, max_pes, max_aframes, dev)
        seqs = np.arange(3, 3 + len(r.caps))
        fr = fragment.fragment_batch(r.rx, r.ix, seqs, mpeg_audio=r.ma)
        plain = mc.Run(segs, max_pes, max_aframes, dev)
        fr0 = fragment.fragment_batch(plain.rx, plain.ix, seqs)
        results.append((fr.finfo.cpu().numpy(), r.out.cpu().numpy(), fr0.finfo.cpu().numpy(), plain.out.cpu().numpy()))
    for got, want in zip(*results):
        assert np.array_equal(got, want)
    assert not np.array_equal(results[0][1], results[0][3])  # the argument changes the audio tfhd and tfdt
