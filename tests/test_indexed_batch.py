"""What every op on a demuxed and indexed batch checks of the batch itself, once per layer.

On the CPU the five Python ops (``ops.esindex.IndexedBatch``): an index of another batch, a strided
``es`` and caps past ``es`` are rejected with the op's name in front, and nothing is touched.  On the
MI355X the six ``_C`` entry points (``es_batch`` in ``kernels/bindings.cpp``): a ``nal`` or ``es`` that
is not 16-byte aligned, a descriptor left on the host and one on another GPU are rejected by the host
check, before any launch, and every output keeps its sentinel.  One batch throughout: a segment with
three planted NAL units and an empty one."""
import numpy as np
import pytest
import torch

from esindex_cases import background, hand_batch, plant, seg
from hlsjs_p2p_wrapper_amd.ops import aes, captions, codecconfig, esindex, hevcconfig, remux, sampleaes, tsdemux
from hlsjs_p2p_wrapper_amd.ops._native import device

MAX_PES, MAX_NAL, MAX_PS, MAX_CC, MAX_AF = 4, 6, 16, 4, 8
KEY, IV = bytes(range(16)), bytes(range(16, 32))


def batch(dev="cpu"):
    v = background(np.random.default_rng(12), 200)
    for p in (0, 60, 130):
        plant(v, p)
    res, caps = hand_batch([seg(v, vpes=[0]), seg(b"")], dev, max_pes=MAX_PES)
    return res, caps, esindex.index_batch(res, caps, max_nal=MAX_NAL)


def _remux(res, ix, caps):
    offs, size = remux.layout_out([256] * len(res.es_offs), MAX_NAL)  # room for any cap the batch can hold
    return remux.remux_batch(res, ix, caps, torch.zeros(size, dtype=torch.uint8), offs, max_aframes=MAX_AF)


def _decrypt(res, ix, caps):
    n = len(res.es_offs)
    return sampleaes.sample_decrypt_batch(res, ix, caps, [KEY] * n, [IV] * n)


OPS = {"remux_batch": _remux,
       "config_batch": lambda res, ix, caps: codecconfig.config_batch(res, ix, caps, MAX_PS),
       "hevc_config_batch": lambda res, ix, caps: hevcconfig.hevc_config_batch(res, ix, caps, MAX_PS),
       "sample_decrypt_batch": _decrypt,
       "caption_batch": lambda res, ix, caps: captions.caption_batch(res, ix, caps, max_cc=MAX_CC)}


def snapshot(res, ix):
    return [t.clone() for t in (res.es, res.info, res.pes, ix.nal, ix.au, ix.aframes, ix.sinfo)]


def assert_untouched(res, ix, before):
    for t, b in zip((res.es, res.info, res.pes, ix.nal, ix.au, ix.aframes, ix.sinfo), before):
        assert torch.equal(t, b)


@pytest.mark.parametrize("name", sorted(OPS))
def test_the_batch_is_accepted_as_it_is(name):
    res, caps, ix = batch()
    assert ix.sinfo[:, esindex.SINFO["n_nal"]].tolist() == [3, 0]
    OPS[name](res, ix, caps)


@pytest.mark.parametrize("name", sorted(OPS))
def test_an_index_of_another_batch_is_rejected(name):
    res, caps, ix = batch()
    one, one_caps = hand_batch([seg(b"")], "cpu", max_pes=MAX_PES)
    other = esindex.index_batch(one, one_caps, max_nal=MAX_NAL)
    before = snapshot(res, ix)
    with pytest.raises(ValueError, match=rf"^{name}: .*does not belong"):
        OPS[name](res, other, caps)
    assert_untouched(res, ix, before)


@pytest.mark.parametrize("name", sorted(OPS))
def test_a_strided_es_is_rejected(name):
    res, caps, ix = batch()
    wide = torch.zeros(2 * res.es.numel(), dtype=torch.uint8)
    wide[::2] = res.es
    strided = tsdemux.DemuxResult(res.info, res.pes, wide[::2], res.es_offs)
    assert torch.equal(strided.es, res.es) and not strided.es.is_contiguous()
    before, wide_before = snapshot(res, ix), wide.clone()
    with pytest.raises(ValueError, match=rf"^{name}: .*contiguous"):
        OPS[name](strided, ix, caps)
    assert_untouched(res, ix, before)
    assert torch.equal(wide, wide_before)


@pytest.mark.parametrize("name", sorted(OPS))
def test_caps_past_es_are_rejected(name):
    res, caps, ix = batch()
    before = snapshot(res, ix)
    with pytest.raises(ValueError, match=rf"^{name}: ES range out of bounds"):
        OPS[name](res, ix, [caps[0], res.es.numel() - int(res.es_offs[1]) + 1])
    assert_untouched(res, ix, before)


# ---------------------------------------------------------------- the six _C entry points
ENTRIES = ("es_index", "remux", "codec_config", "hevc_config", "sample_aes_decrypt", "cc_extract")


def entry(name, cuda, **swap):
    """``(call, args, outputs)`` of one ``_C`` entry point on the batch, every output (and the scratch)
    of exactly its exported size and filled with a sentinel; ``swap[k]`` replaces shared tensor ``k``
    by what it returns of it."""
    C = device()
    res, caps, ix = batch(cuda)
    B, cap = len(caps), np.asarray(caps, np.int64)
    dev = lambda a, dt=np.int64: torch.from_numpy(np.asarray(a, dt)).to(cuda)  # noqa: E731
    full = lambda n, dt: torch.full((int(n),), 0x5A, dtype=dt, device=cuda)  # noqa: E731
    s = {"es": res.es, "es_off": dev(res.es_offs), "cap": dev(cap), "info": res.info, "pes": res.pes, "nal": ix.nal,
         "au": ix.au, "aframes": ix.aframes, "sinfo": ix.sinfo}
    if name == "es_index":  # the four tables are its outputs
        s.update({k: torch.full_like(s[k], 0x5A) for k in ("nal", "au", "aframes", "sinfo")})
    s.update({k: f(s[k]) for k, f in swap.items()})
    head, mid = (s["es"], s["es_off"], s["cap"]), (s["info"], s["pes"], MAX_PES, MAX_NAL)
    tables = (s["nal"], s["au"], s["aframes"], s["sinfo"])

    def tiles(sized, T):
        tp = np.zeros(B + 1, np.int64)
        np.cumsum((sized + T - 1) // T, out=tp[1:])
        return dev(tp), int(tp[-1])

    if name == "es_index":
        tp, total = tiles(cap, C.es_index_tile_bytes())
        outs = (full(C.es_index_scratch_words(total, B, MAX_NAL), torch.int32), *tables)
        return C.es_index, (*head, tp, total, *mid, *outs), outs
    if name == "remux":
        offs, size = remux.layout_out(caps, MAX_NAL)
        tp, total = tiles(remux.remux_out_bytes(cap, MAX_NAL), C.remux_tile_bytes())
        outs = (full(C.remux_scratch_words(B, MAX_NAL, MAX_AF), torch.int32), full(B * MAX_PES * 5, torch.int32),
                full(B * MAX_AF * 2, torch.int32), full(B * remux.RINFO_WORDS, torch.int64), full(size, torch.uint8))
        return C.remux, (*head, tp, total, *mid, *tables, MAX_AF, *outs, dev(offs)), outs
    if name == "codec_config":
        outs = (full(B * codecconfig.CINFO_WORDS, torch.int32), full(B * 2 * MAX_PS, torch.uint8))
        return C.codec_config, (*head, *mid, *tables, MAX_PS, *outs), outs
    if name == "hevc_config":
        outs = (full(B * hevcconfig.HINFO_WORDS, torch.int32), full(B * hevcconfig.HPS_ROWS * MAX_PS, torch.uint8))
        return C.hevc_config, (*head, *mid, *tables, MAX_PS, *outs), outs
    if name == "sample_aes_decrypt":  # rewrites es and nal as well
        drk = dev(np.stack([aes.round_keys_le(KEY)] * B).view(np.int32), np.int32)
        iv = dev(np.frombuffer(IV * B, np.uint8).reshape(B, 16).copy(), np.uint8)
        outs = (full(B * sampleaes.SAINFO_WORDS, torch.int64), s["es"], s["nal"])
        return (C.sample_aes_decrypt,
                (*head, *mid, *tables, drk, iv, dev(np.ones(B), np.uint8), *aes.device_tables(cuda), outs[0]), outs)
    outs = (full(C.cc_scratch_words(B, MAX_NAL), torch.int32), full(B * MAX_CC * captions.CCROW_WORDS, torch.int32),
            full(B * MAX_CC, torch.int64), full(B * MAX_CC * captions.CC_SLOT_BYTES, torch.uint8),
            full(B * MAX_CC * 2 * captions.CC_FIELD_BYTES, torch.uint8), full(B * captions.CCINFO_WORDS, torch.int64))
    return C.cc_extract, (*head, *mid, *tables, dev(np.ones(B), np.uint8), MAX_CC, *outs), outs


def offset_by_one_element(t):
    """``t``'s values in a contiguous view that starts one element into its allocation."""
    return torch.cat([t.new_zeros(1), t.flatten()])[1:].view(t.shape)


def rejected(name, cuda, match, **swap):
    call, args, outs = entry(name, cuda, **swap)
    before = [t.cpu() for t in outs]
    with pytest.raises(RuntimeError, match=match):
        call(*args)
    torch.cuda.synchronize()
    for t, b in zip(outs, before):
        assert torch.equal(t.cpu(), b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENTRIES)
def test_entry_point_takes_the_batch_as_it_is(name, cuda):
    call, args, outs = entry(name, cuda)
    before = [t.cpu() for t in outs]
    call(*args)
    torch.cuda.synchronize()
    assert not all(torch.equal(t.cpu(), b) for t, b in zip(outs, before))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENTRIES)
def test_entry_point_rejects_a_misaligned_nal_or_es(name, cuda):
    rejected(name, cuda, "nal must be 16-byte aligned", nal=offset_by_one_element)
    rejected(name, cuda, "es must be 16-byte aligned", es=offset_by_one_element)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENTRIES)
def test_entry_point_rejects_a_descriptor_on_the_host(name, cuda):
    rejected(name, cuda, "es_off must be a GPU tensor", es_off=lambda t: t.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENTRIES)
def test_entry_point_rejects_a_descriptor_on_another_gpu(name, cuda):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU")
    rejected(name, cuda, "different devices", cap=lambda t: t.to("cuda:1"))
