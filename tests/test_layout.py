"""One owner per layout fact (``ops/csrc/shared/layout.hpp``): the Python tables of
``ops/tsdemux.py`` / ``ops/esindex.py`` equal what ``_runtime`` exports from the shared enums,
and the device bindings accept workspaces sized exactly by the exported size functions and
reject, in their host-side checks, anything one element short."""
import zlib

import numpy as np
import pytest
import torch

from esindex_cases import background, hand_batch, plant, seg
from hlsjs_p2p_wrapper_amd.ops import crc, esindex, remux, tsdemux
from hlsjs_p2p_wrapper_amd.ops._native import device
from hlsjs_p2p_wrapper_amd.ops.desc import pack_to_device


def test_python_tables_equal_the_runtime_exports(rt):
    assert tsdemux.INFO == dict(rt.TS_INFO) and tsdemux.INFO_WORDS == rt.TS_INFO_WORDS
    assert tsdemux.STATUS == dict(rt.TS_STATUS) and tsdemux.PACKET == rt.TS_PACKET
    assert len(tsdemux.CLASSES) == rt.TS_CLASSES
    assert esindex.SINFO == dict(rt.ES_SINFO) and esindex.SINFO_WORDS == rt.ES_SINFO_WORDS
    assert esindex.SSTATUS == dict(rt.ES_STATUS) and esindex.AU_FLAGS == dict(rt.ES_AU_FLAGS)
    assert esindex.DEFAULT_MAX_NAL == rt.ES_DEFAULT_MAX_NAL
    assert max(tsdemux.INFO.values()) < tsdemux.INFO_WORDS and len(set(tsdemux.INFO.values())) == len(tsdemux.INFO)
    assert sorted(esindex.SINFO.values()) == list(range(esindex.SINFO_WORDS))
    assert remux.RINFO == dict(rt.ES_RINFO) and remux.RINFO_WORDS == rt.ES_RINFO_WORDS
    assert sorted(remux.RINFO.values()) == list(range(remux.RINFO_WORDS))
    assert remux.RSTATUS == dict(rt.ES_RSTATUS) and remux.SAMPLE_FLAGS == dict(rt.ES_SAMPLE_FLAGS)
    assert remux.DEFAULT_MAX_AFRAMES == rt.ES_DEFAULT_MAX_AFRAMES and remux.OUT_ALIGN == rt.ES_OUT_ALIGN
    # the row widths are the shapes the two batch calls return
    res, caps = hand_batch([seg(b"\x00\x00\x01\x65\x11", vpes=[0]), seg(b"")], "cpu", max_pes=4)
    assert tuple(res.pes.shape) == (2, rt.TS_CLASSES, 4, rt.TS_PES_WORDS)
    ix = esindex.index_batch(res, caps, max_nal=6)
    assert tuple(ix.nal.shape) == (2, 6, rt.ES_NAL_WORDS) and tuple(ix.au.shape) == (2, 4, rt.ES_AU_WORDS)
    assert tuple(ix.aframes.shape) == (2, 4, rt.ES_APES_WORDS) and tuple(ix.sinfo.shape) == (2, rt.ES_SINFO_WORDS)
    offs, size = remux.layout_out(caps, 6)
    rx = remux.remux_batch(res, ix, caps, torch.zeros(size, dtype=torch.uint8), offs, max_aframes=3)
    assert tuple(rx.vsamples.shape) == (2, 4, rt.ES_VSAMPLE_WORDS) and tuple(rx.rinfo.shape) == (2, rt.ES_RINFO_WORDS)
    assert tuple(rx.asamples.shape) == (2, 3, rt.ES_ASAMPLE_WORDS)
    assert (rt.TS_PES_WORDS, rt.ES_NAL_WORDS, rt.ES_AU_WORDS, rt.ES_APES_WORDS) == (3, 4, 4, 2)
    assert (rt.ES_VSAMPLE_WORDS, rt.ES_ASAMPLE_WORDS) == (5, 2)


def test_per_class_info_slots_are_base_plus_class():
    I = tsdemux.INFO
    for c, name in enumerate(tsdemux.CLASSES):
        assert I[f"{name}_pid"] == I["video_pid"] + c
        assert I[f"{name}_bytes"] == I["video_bytes"] + c
        assert I[f"n_{name}_pes"] == I["n_video_pes"] + c
        assert I[f"{name}_first_pts"] == I["video_first_pts"] + c
        assert I[f"{name}_last_pts"] == I["video_last_pts"] + c


def _demux_case(cuda):
    """Caps of 1 and 257 packets: blocks 1 and 2, so the aux partition has a block boundary
    and a segment boundary.  Returns the raw binding's arguments and the CPU result."""
    C = device()
    ts, _ = tsdemux.mux_segment(target_bytes=300 * 188, seed=3)
    ts = np.frombuffer(ts, np.uint8)
    lens = [188, 257 * 188]
    offs = [0, 256]
    buf = np.zeros(256 + lens[1] + 256, np.uint8)
    buf[:188] = ts[:188]
    buf[256:256 + lens[1]] = ts[:lens[1]]
    max_pes = 64
    cpu = tsdemux.demux_batch(torch.from_numpy(buf), offs, lens, torch.zeros(len(buf), dtype=torch.uint8), offs,
                              max_pes=max_pes)
    blocks = C.ts_demux_blocks(np.asarray(lens, np.int64))
    assert blocks.tolist() == [1, 2] and C.ts_demux_blocks(0) == 0
    bp = np.concatenate([[0], np.cumsum(blocks)]).astype(np.int64)
    d = pack_to_device({"o": np.asarray(offs, np.int64), "n": np.asarray(lens, np.int64), "bp": bp}, cuda)
    return torch.from_numpy(buf).to(cuda), d, int(bp[-1]), max_pes, offs, cpu


def _demux_args(cuda, case, short=None):
    """The raw binding's arguments, workspaces sized by ``ts_demux_workspace`` (``short``: that
    one an element less), outputs filled with -7."""
    buf, d, total, max_pes, _, _ = case
    sizes = dict(zip(("meta", "pts_dts", "aux"), device().ts_demux_workspace(total, 2)))
    if short:
        sizes[short] -= 1
    meta = torch.empty(sizes["meta"], dtype=torch.int32, device=cuda)
    pts = torch.empty(sizes["pts_dts"], dtype=torch.int64, device=cuda)
    aux = torch.empty(sizes["aux"], dtype=torch.int32, device=cuda)
    es = torch.zeros(buf.numel(), dtype=torch.uint8, device=cuda)
    info = torch.full((2, tsdemux.INFO_WORDS), -7, dtype=torch.int64, device=cuda)
    pes = torch.full((2, 3, max_pes, 3), -7, dtype=torch.int64, device=cuda)
    return (buf, d["o"], d["n"], d["bp"], total, meta, pts, aux, es, d["o"], pes, max_pes, info), info, pes, es


@pytest.mark.gpu
def test_demux_runs_in_a_workspace_of_exactly_the_exported_size(cuda):
    case = _demux_case(cuda)
    assert device().ts_demux_workspace(3, 2) == (3 * 256, 3 * 256 * 2, 3 * 12 + 2 * 7)
    args, info, pes, es = _demux_args(cuda, case)
    device().ts_demux(*args)
    cpu, offs = case[-1], case[-2]
    assert torch.equal(info.cpu(), cpu.info) and torch.equal(pes.cpu(), cpu.pes)
    ci = cpu.info.numpy()
    assert ci[1, tsdemux.INFO["payload_bytes"]] > 0 and ci[1, tsdemux.INFO["status"]] == 0
    for i, o in enumerate(offs):
        n = int(ci[i, tsdemux.INFO["payload_bytes"]])
        assert torch.equal(es[o:o + n].cpu(), cpu.es[o:o + n])


@pytest.mark.gpu
@pytest.mark.parametrize("short", ["aux", "meta"])
def test_demux_rejects_a_workspace_one_element_short(cuda, short):
    """In the host-side check: the PSI kernel, the first launch, would rewrite the info rows."""
    args, info, _, _ = _demux_args(cuda, _demux_case(cuda), short=short)
    with pytest.raises(RuntimeError, match=f"{short} too small"):
        device().ts_demux(*args)
    assert (info.cpu() == -7).all()


def _index_case(tile, dev):
    """Caps of one tile + 16 bytes and of 0: two tiles and none."""
    v = background(np.random.default_rng(4), tile + 16)
    for p in (0, tile - 2, tile + 9):  # the second start code straddles the tile edge
        plant(v, p)
    return hand_batch([seg(v, vpes=[0, tile]), seg(b"")], dev, max_pes=4)


def _index_args(cuda, tile, max_nal, short=0):
    res, caps = _index_case(tile, cuda)
    assert caps == [tile + 16, 0]
    max_pes = 4
    tp = np.array([0, 2, 2], np.int64)
    d = pack_to_device({"eo": res.es_offs, "cap": np.asarray(caps, np.int64), "tp": tp}, cuda)
    words = device().es_index_scratch_words(2, 2, max_nal)
    assert words == 2 * 2 + 2 * (max_nal + 1)
    scratch = torch.empty(words - short, dtype=torch.int32, device=cuda)
    nal = torch.empty((2, max_nal, 4), dtype=torch.int32, device=cuda)
    au = torch.empty((2, max_pes, 4), dtype=torch.int32, device=cuda)
    af = torch.empty((2, max_pes, 2), dtype=torch.int32, device=cuda)
    sinfo = torch.full((2, esindex.SINFO_WORDS), -7, dtype=torch.int64, device=cuda)
    args = (res.es, d["eo"], d["cap"], d["tp"], 2, res.info, res.pes, max_pes, max_nal, scratch, nal, au, af, sinfo)
    return args, esindex.EsIndex(nal, au, af, sinfo)


@pytest.mark.gpu
def test_index_runs_in_a_scratch_of_exactly_the_exported_size(cuda):
    tile, max_nal = device().es_index_tile_bytes(), 6
    args, ix = _index_args(cuda, tile, max_nal)
    device().es_index(*args)
    res, caps = _index_case(tile, "cpu")
    ref = esindex.index_batch(res, caps, max_nal=max_nal)
    for name in ("nal", "au", "aframes", "sinfo"):
        assert torch.equal(getattr(ix, name).cpu(), getattr(ref, name)), name
    assert ref.sinfo[:, esindex.SINFO["n_nal"]].tolist() == [3, 0]


@pytest.mark.gpu
def test_index_rejects_a_scratch_one_element_short(cuda):
    """In the host-side check: the prefix kernel would write the sinfo rows."""
    args, ix = _index_args(cuda, device().es_index_tile_bytes(), 6, short=1)
    with pytest.raises(RuntimeError, match="scratch too small"):
        device().es_index(*args)
    assert (ix.sinfo.cpu() == -7).all()


@pytest.mark.gpu
def test_crc_needs_the_whole_shift_table(cuda, rt):
    """Segments of 257 bytes (two groups, one tile) and 0 bytes.  The combine kernel reads
    P_0..P_39 and Q_0..Q_11: 52 Ki words; a table cut to 48 Ki words is rejected on the host."""
    C = device()
    assert (C.CRC_GROUP_BYTES, C.CRC_TILE_GROUPS) == (256, 32)
    data = np.random.default_rng(2).integers(0, 256, 512, dtype=np.uint8)
    buf = torch.from_numpy(data).to(cuda)
    o, n = np.array([0, 272], np.int64), np.array([257, 0], np.int64)
    w, tables = crc._device_consts(cuda, "fp4")
    assert tables.numel() == (rt.CRC_NUM_P + rt.CRC_NUM_Q) * 1024 == 52 * 1024
    want = [zlib.crc32(data[:257].tobytes()), zlib.crc32(b"")]
    got, _ = C.crc32_launch(buf, o, n, w, tables)
    assert got.cpu().numpy().view(np.uint32).tolist() == want
    got, _ = crc._crc32_batch_py(buf, o, n, None, None, None, None)
    assert got.cpu().numpy().view(np.uint32).tolist() == want
    cut = tables[:48 * 1024].clone()
    with pytest.raises(ValueError, match="tables"):
        C.crc32_launch(buf, o, n, w, cut)
    d = pack_to_device({"o": o, "n": n, "tp": np.array([0, 1, 1], np.int64), "ro": np.array([0, 2], np.int64)}, cuda)
    residues = torch.empty(2, dtype=torch.int32, device=cuda)
    out = torch.full((2,), -7, dtype=torch.int32, device=cuda)
    with pytest.raises(RuntimeError, match="tables too small"):
        C.crc32_batch(buf, d["o"], d["n"], d["tp"], d["ro"], w, cut, residues, out, None, None, 1)
    torch.cuda.synchronize()
    assert out.tolist() == [-7, -7]
