"""Per-kernel microbenchmark on one bench round's batch: 64 x ~3 MB AES-128 TS segments
(the 1080p 6 Mb/s config).  Times AES-CBC decrypt, TS demux (psi+scan+gather), the sample
index over the demuxed ES, the remux to fMP4 samples, the codec configuration for the init segments
(H.264 and HEVC) and the MFMA CRC with HIP events and reports us / GB/s of input.
Checks results against the host oracles once.

    PYTHONPATH=. python tools/kernel_bench.py [--segs 64] [--iters 20]
"""
import argparse
import json

import numpy as np
import torch

from hlsjs_p2p_wrapper_amd.net.origin import PRESET_1080P_6M, SyntheticHlsOrigin
from hlsjs_p2p_wrapper_amd.ops import aes, codecconfig, crc, esindex, hevcconfig, remux, segment, tsdemux


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segs", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda")
    origin = SyntheticHlsOrigin("http://cdn.kb/", renditions=PRESET_1080P_6M, num_segments=args.segs,
                                encrypted=True, pool_size=args.segs, pin_memory=True, seed=3)
    pool = origin.pools[0]
    offs = [int(o) for o in pool.offsets[:args.segs]]
    lens = [int(n) for n in pool.lengths[:args.segs]]
    src = pool.data.to(dev)
    total = sum(lens)
    keys = [origin.key] * args.segs
    ivs = [origin.iv] * args.segs
    dec = torch.empty_like(src)
    res = {}
    out_len = aes.cbc_decrypt_batch(src, offs, lens, keys, ivs, dec, offs)
    res["aes_us"] = timed(lambda: aes.cbc_decrypt_batch(src, offs, lens, keys, ivs, dec, offs), args.iters)
    # correctness vs host (first segment)
    ref = aes.cbc_decrypt(origin.key, origin.iv, pool.data[offs[0]:offs[0] + lens[0]].numpy())
    assert dec[offs[0]:offs[0] + len(ref)].cpu().numpy().tobytes() == ref.tobytes(), "AES mismatch"
    es = torch.empty_like(src)
    caps = lens
    r = tsdemux.demux_batch(dec, offs, out_len, es, offs, caps=caps)
    res["demux_us"] = timed(lambda: tsdemux.demux_batch(dec, offs, out_len, es, offs, caps=caps), args.iters)
    cpu = tsdemux.demux_batch(torch.from_numpy(ref.copy()), [0], [len(ref)], torch.empty(len(ref) + 256,
                                                                                           dtype=torch.uint8), [0])
    g, c = r.segment(0), cpu.segment(0)
    assert g["video_bytes"] == c["video_bytes"] and torch.equal(g["video"]["es"].cpu(), c["video"]["es"]), \
        "demux mismatch"
    # the sample index over the ES the demux just wrote (count + prefix + emit + finish)
    ix = esindex.index_batch(r, caps)
    res["esindex_us"] = timed(lambda: esindex.index_batch(r, caps), args.iters)
    hx = esindex.index_batch(cpu, [len(ref)])
    assert all(torch.equal(getattr(ix, k)[0].cpu(), getattr(hx, k)[0]) for k in ("sinfo", "nal", "au", "aframes")), \
        "esindex mismatch"
    # the remux of the indexed ES into mdat boxes and sample tables (plan + copy)
    oo, size = remux.layout_out(caps, ix.nal.shape[1])
    boxes = torch.empty(size, dtype=torch.uint8, device=dev)
    rx = remux.remux_batch(r, ix, caps, boxes, oo)
    res["remux_us"] = timed(lambda: remux.remux_batch(r, ix, caps, boxes, oo), args.iters)
    ho, hsize = remux.layout_out([len(ref)], hx.nal.shape[1])
    hr = remux.remux_batch(cpu, hx, [len(ref)], torch.empty(hsize, dtype=torch.uint8), ho)
    assert all(torch.equal(getattr(rx, k)[0].cpu(), getattr(hr, k)[0]) for k in ("rinfo", "vsamples", "asamples")), \
        "remux mismatch"
    used = int(hr.rinfo[0, remux.RINFO["audio_box_offset"]] + 8 + hr.rinfo[0, remux.RINFO["audio_payload_bytes"]])
    vend = 8 + int(hr.rinfo[0, remux.RINFO["video_payload_bytes"]])
    a0 = int(hr.rinfo[0, remux.RINFO["audio_box_offset"]])
    for lo, hi in ((0, vend), (a0, used)):  # both boxes; the bytes between and behind them belong to nobody
        assert torch.equal(boxes[int(oo[0]) + lo:int(oo[0]) + hi].cpu(), hr.out[lo:hi]), "remux mismatch"
    # the codec configuration of the indexed ES for the init segments (one workgroup per segment)
    cfg = codecconfig.config_batch(r, ix, caps)
    res["codecconfig_us"] = timed(lambda: codecconfig.config_batch(r, ix, caps), args.iters)
    hc = codecconfig.config_batch(cpu, hx, [len(ref)])
    assert all(torch.equal(getattr(cfg, k)[0].cpu(), getattr(hc, k)[0]) for k in ("cinfo", "ps")), \
        "codecconfig mismatch"
    # the HEVC configuration launched behind it: on this H.264 batch every workgroup exits at once,
    # which is what the launch adds to a remuxFmp4 group ...
    hv = hevcconfig.hevc_config_batch(r, ix, caps)
    res["hevcconfig_us"] = timed(lambda: hevcconfig.hevc_config_batch(r, ix, caps), args.iters)
    hh = hevcconfig.hevc_config_batch(cpu, hx, [len(ref)])
    assert all(torch.equal(getattr(hv, k)[0].cpu(), getattr(hh, k)[0]) for k in ("hinfo", "hps")), \
        "hevcconfig mismatch"
    # ... and with the same bytes declared HEVC and indexed as such: the row search runs over every
    # recorded NAL of a segment that holds no parameter set, the longest path the kernel has
    r24 = tsdemux.DemuxResult(r.info.clone(), r.pes, r.es, r.es_offs)
    r24.info[:, tsdemux.INFO["video_type"]] = 0x24
    ix24 = esindex.index_batch(r24, caps)
    hv = hevcconfig.hevc_config_batch(r24, ix24, caps)
    res["hevcconfig_search_us"] = timed(lambda: hevcconfig.hevc_config_batch(r24, ix24, caps), args.iters)
    cpu24 = tsdemux.DemuxResult(cpu.info.clone(), cpu.pes, cpu.es, cpu.es_offs)
    cpu24.info[:, tsdemux.INFO["video_type"]] = 0x24
    hh = hevcconfig.hevc_config_batch(cpu24, esindex.index_batch(cpu24, [len(ref)]), [len(ref)])
    assert all(torch.equal(getattr(hv, k)[0].cpu(), getattr(hh, k)[0]) for k in ("hinfo", "hps")), \
        "hevcconfig (HEVC) mismatch"
    res["crc_us"] = timed(lambda: crc.crc32_batch(src, offs, lens), args.iters)
    got = crc.crc32_batch(src, offs, lens)[0].cpu().numpy().view(np.uint32)
    assert int(got[0]) == crc.crc32(pool.data[offs[0]:offs[0] + lens[0]].numpy()), "CRC mismatch"
    # byte-moving rooflines on the same bytes: the batched K4 segment copy and torch's copy_
    cp = torch.empty_like(src)
    res["copy_us"] = timed(lambda: segment.copy_segments(src, cp, offs, offs, lens), args.iters)
    assert torch.equal(cp[offs[5]:offs[5] + lens[5]], src[offs[5]:offs[5] + lens[5]]), "copy mismatch"
    res["torch_copy_us"] = timed(lambda: cp.copy_(src), args.iters)
    for k in ("aes", "demux", "esindex", "remux", "codecconfig", "hevcconfig", "hevcconfig_search", "crc", "copy",
              "torch_copy"):
        res[f"{k}_GBps"] = round(total / (res[f"{k}_us"] * 1e-6) / 1e9, 1)
        res[f"{k}_us"] = round(res[f"{k}_us"], 1)
    res["bytes"] = total
    print(json.dumps(res))


if __name__ == "__main__":
    main()
