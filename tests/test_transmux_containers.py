"""The three containers of the transmux pipeline in one batch: MPEG-TS, fragmented MP4 and packed
audio jobs of every kind that reaches a different branch, interleaved, with the three error classes
of each container.  A job's result in the mixed batch is what it gets in a batch of its own container
alone; the callbacks come container by container; the counters count what they count; every device
op is called once per group that has a row asking; a stage that fails in one container reaches only
that container's jobs; and the device pipeline gives what the CPU pipeline gives."""
import functools
from collections import Counter
from collections.abc import Mapping

import numpy as np
import pytest
import torch

import cbcs_cases as cc
import test_cbcs_pipeline as cp
import test_cenc_pipeline as ce
import test_mp4_pipeline as mp
import test_packedaudio_pipeline as pp
import test_sampleaes_pipeline as sp
from hlsjs_p2p_wrapper_amd.ops import aes, tsdemux
from hlsjs_p2p_wrapper_amd.player.mp4init import parse_init
from hlsjs_p2p_wrapper_amd.player.transmux import CaptionData, MediaPipeline, Samples, TransmuxJob, _View

KEY, IV = bytes(range(16)), bytes(range(16, 32))
SKEY, SIV = cc.key_of(5), cc.iv_of(9)  # what the cbcs / cenc twins are packaged with


def errors_of(plain: bytes):
    """The three error classes of an AES-128 payload: ``16k - 3`` bytes, none at all, and a ciphertext
    whose last block decrypts to a padding byte of zero."""
    cipher = bytearray(aes.cbc_encrypt(KEY, IV, np.frombuffer(plain, np.uint8)))
    assert len(cipher) >= 32 and len(cipher) % 16 == 0
    bad = bytearray(cipher)
    bad[-17] ^= 16 - len(plain) % 16  # CBC: flips the same bits of the last plaintext byte, the padding length
    return bytes(cipher[:-3]), np.zeros(0, np.uint8), bytes(bad)


@functools.lru_cache(maxsize=None)
def specs():
    """``(name, container, payload, key, iv, kwargs)`` of the mixed batch, in submit order."""
    ts = bytes(tsdemux.mux_segment(target_bytes=40 * 188, seed=5)[0])
    ts_sa = sp.twin_streams()[0]
    clear_init, cbcs_init, cenc_init = parse_init(mp.INIT), parse_init(cp.INIT), parse_init(ce.INIT)
    frags = mp.fragments()
    cbcs, cenc = cp.twins()[0][1], ce.twins()[0][1]
    (_, _, s0), (_, _, s1) = pp.segment(0), pp.segment(1, 7)
    enc = lambda b: bytes(aes.cbc_encrypt(KEY, IV, np.frombuffer(b, np.uint8)))  # noqa: E731
    t_odd, t_empty, t_bad = errors_of(ts)
    m_odd, m_empty, m_bad = errors_of(frags[1])
    p_odd, p_empty, p_bad = errors_of(s1)
    m, p = dict(mp4=clear_init), dict(packed_audio=True)
    return [
        ("ts_clear", "ts", ts, None, None, {}),
        ("mp4_clear", "mp4", frags[0], None, None, dict(m, captions=True)),
        ("aac_clear", "aac", s0, None, None, dict(p, fragment=True, sequence_number=9)),
        ("ts_enc", "ts", enc(ts), KEY, IV, {}),
        ("mp4_enc", "mp4", enc(frags[1]), KEY, IV, m),
        ("aac_enc", "aac", enc(s1), KEY, IV, dict(p, remux=True)),
        ("ts_sample", "ts", ts_sa, None, None, dict(sample_key=sp.KEY, sample_iv=sp.IV, index=True)),
        ("mp4_cbcs", "mp4", cbcs, None, None, dict(mp4=cbcs_init, sample_key=SKEY, sample_iv=SIV, captions=True)),
        ("aac_plain", "aac", s1, None, None, p),
        ("ts_frag", "ts", ts, None, None, dict(fragment=True, sequence_number=3, time_base=1000)),
        ("mp4_cenc", "mp4", cenc, None, None, dict(mp4=cenc_init, sample_key=SKEY, sample_iv=SIV)),
        ("ts_odd", "ts", t_odd, KEY, IV, {}),
        ("mp4_odd", "mp4", m_odd, KEY, IV, m),
        ("aac_odd", "aac", p_odd, KEY, IV, p),
        ("ts_empty", "ts", t_empty, KEY, IV, {}),
        ("mp4_empty", "mp4", m_empty, KEY, IV, m),
        ("aac_empty", "aac", p_empty, KEY, IV, p),
        ("ts_pad", "ts", t_bad, KEY, IV, {}),
        ("mp4_pad", "mp4", m_bad, KEY, IV, m),
        ("aac_pad", "aac", p_bad, KEY, IV, p),
    ]


def run(device, chosen, extra=()):
    """One batch of ``chosen`` (and ``extra`` jobs behind them): (results by name, names in callback
    order, the pipeline)."""
    pipe = MediaPipeline(torch.device(device))
    pipe.auto_flush = False
    out, order = {}, []

    def put(name):
        def cb(r):
            out[name] = r
            order.append(name)
        return cb

    for name, _, payload, key, iv, kw in chosen:
        pipe.submit(TransmuxJob(payload, key, iv, put(name), **kw))
    for name, payload, kw in extra:
        pipe.submit(TransmuxJob(payload, None, None, put(name), **kw))
    pipe.complete(pipe.launch())
    return out, order, pipe


def plain(x, devices=None):
    """A result value as plain comparable data: a tensor as its shape and bytes (its device noted in
    ``devices``), a view or mapping by key, without the callables; of ``samples`` and ``captions`` the
    scalar fields."""
    if isinstance(x, torch.Tensor):
        if devices is not None:
            devices.append(x.device.type)
        return (tuple(x.shape), str(x.dtype), x.cpu().contiguous().numpy().tobytes())
    if isinstance(x, np.ndarray):
        return (x.shape, str(x.dtype), x.tobytes())
    if isinstance(x, (Samples, CaptionData)):
        return {k: x[k] for k in x.keys() if not isinstance(x[k], torch.Tensor) and not callable(x[k])}
    if isinstance(x, (Mapping, _View)) or hasattr(x, "to_dict"):
        items = x.to_dict().items() if hasattr(x, "to_dict") else ((k, x[k]) for k in x.keys())
        return {k: plain(v, devices) for k, v in items if not callable(v)}
    if isinstance(x, (list, tuple)):
        return [plain(v, devices) for v in x]
    if isinstance(x, BaseException):
        return (type(x).__name__, str(x))
    return x


def digest(r, devices=None):
    d = {"keys": sorted(dict.keys(r))}  # what is stored; the ES views of an MPEG-TS shaped result come on access
    for k in ("status", "plain_bytes", "container", "index", "verify_failed"):
        d[k] = r.get(k)
    d["init"] = id(r.get("init"))  # one Mp4Init object per init segment serves every batch of this module
    for k in ("info", "error", "emsg", "data", "samples", "captions", "fmp4", "cbcs", "cenc", "sample_aes",
              "packed_audio"):
        if k in r:
            d[k] = plain(r[k], devices)
    for k in ("video", "audio", "id3"):
        if "info" in r and (k != "id3" or r.get("container") != "mp4"):
            d[k] = plain(r[k], devices)
    return d


@functools.lru_cache(maxsize=None)
def mixed_cpu():
    """The mixed batch on CPU, computed once: (digests by name, callback order, the three counters)."""
    out, order, pipe = run("cpu", specs())
    return {k: digest(r) for k, r in out.items()}, order, (pipe.segments, pipe.bytes_in, pipe.batches)


def of(container):
    return [s for s in specs() if s[1] == container]


def test_a_job_in_the_mixed_batch_gets_what_it_gets_in_a_batch_of_its_own_container():
    mixed, order, counters = mixed_cpu()
    names = [s[0] for s in specs()]
    assert sorted(mixed) == sorted(names) and len(names) == 20
    # every branch is reached: no error but the nine asked for, and each kind's own keys
    want_errors = {"odd": "ValueError: encrypted payload is not a multiple of 16 bytes",
                   "empty": "ValueError: encrypted payload is not a multiple of 16 bytes",
                   "pad": "ValueError: decryption failed (bad PKCS#7 padding)"}
    for name in names:
        kind = name.split("_")[1]
        err = mixed[name].get("error")
        assert (": ".join(err) if err else None) == want_errors.get(kind), name
        assert mixed[name]["container"] == {"ts": None, "mp4": "mp4", "aac": "aac"}[name.split("_")[0]]
    assert mixed["ts_odd"]["keys"] == ["error", "status"] and mixed["mp4_odd"]["keys"] == mixed["aac_empty"]["keys"] \
        == ["container", "error", "status"]
    assert all(mixed[name]["plain_bytes"] < 0 for name in ("ts_pad", "mp4_pad", "aac_pad"))
    assert "sample_aes" in mixed["ts_sample"] and "samples" in mixed["ts_sample"] and "fmp4" not in mixed["ts_sample"]
    assert mixed["ts_frag"]["fmp4"]["time_base"] == 1000 and "fragment" in mixed["ts_frag"]["fmp4"]["video"]
    assert "captions" in mixed["mp4_clear"] and "cbcs" in mixed["mp4_cbcs"] and "cenc" in mixed["mp4_cenc"]
    assert mixed["mp4_cbcs"]["data"] == mixed["mp4_cenc"]["data"] != mixed["mp4_clear"]["data"]  # the clear twin
    assert "fragment" in mixed["aac_clear"]["fmp4"]["audio"] and "fragment" not in mixed["aac_enc"]["fmp4"]["audio"]
    assert "fmp4" not in mixed["aac_plain"] and mixed["aac_plain"]["audio"] == mixed["aac_enc"]["audio"]
    for container in ("ts", "mp4", "aac"):
        out, alone_order, pipe = run("cpu", of(container))
        for name, r in out.items():
            assert digest(r) == mixed[name], name
        assert alone_order == [s[0] for s in of(container)]
        # segments and bytes_in count every job, batches the MPEG-TS core alone
        assert (pipe.segments, pipe.batches) == ({"ts": 7, "mp4": 7, "aac": 6}[container], int(container == "ts"))
        assert pipe.bytes_in == BYTES[container] == sum(len(s[2]) for s in of(container))
    # all fragmented-MP4 jobs in submit order, then all packed-audio jobs, then all MPEG-TS jobs
    assert order == [s[0] for s in of("mp4")] + [s[0] for s in of("aac")] + [s[0] for s in of("ts")]
    assert counters == (20, 452537 + 3529 + 7559, 1)


# the payload bytes of the mixed batch, per container (the case modules' segments have fixed sizes): MPEG-TS
# 2 x 89864 clear + 89872 encrypted + 3196 SAMPLE-AES + 89869 odd + 0 + 89872 bad padding, and likewise
BYTES = {"ts": 452537, "mp4": 574 + 432 + 831 + 831 + 429 + 0 + 432, "aac": 1872 + 1424 + 1418 + 1421 + 0 + 1424}

OPS = {"aes": ["cbc_decrypt_batch"], "tsdemux": ["demux_batch"], "mp4demux": ["mp4_demux_batch"],
       "packedaudio": ["packed_audio_batch"], "esindex": ["index_batch"], "sampleaes": ["sample_decrypt_batch"],
       "captions": ["caption_batch"], "remux": ["remux_batch"], "fragment": ["fragment_batch"],
       "codecconfig": ["config_batch"], "hevcconfig": ["hevc_config_batch"], "cbcs": ["cbcs_decrypt_batch"],
       "cenc": ["cenc_decrypt_batch"]}


def test_every_op_is_called_once_per_group_that_has_a_row_asking(monkeypatch):
    import importlib

    calls = Counter()
    depth = [0]  # an op that calls another op of the list is one call of the pipeline's

    def counted(name, fn):
        def wrapper(*a, **kw):
            if not depth[0]:
                calls[name] += 1
            depth[0] += 1
            try:
                return fn(*a, **kw)
            finally:
                depth[0] -= 1
        return wrapper

    for mod, names in OPS.items():
        module = importlib.import_module(f"hlsjs_p2p_wrapper_amd.ops.{mod}")
        for name in names:
            monkeypatch.setattr(module, name, counted(name, getattr(module, name)))
    out, _, _ = run("cpu", specs())
    assert {k: digest(r) for k, r in out.items()} == mixed_cpu()[0]
    # The groups of the batch, per container the accepted encrypted rows, then the clear ones:
    #   MPEG-TS  {ts_enc, ts_pad}  {ts_clear, ts_sample, ts_frag}
    #   mp4      {mp4_enc, mp4_pad}  {mp4_clear}  {mp4_cbcs}  {mp4_cenc}
    #   aac      {aac_enc, aac_pad}  {aac_clear, aac_plain}
    assert dict(calls) == {
        "cbc_decrypt_batch": 3,      # one per container: each has encrypted rows
        "demux_batch": 2,            # the two MPEG-TS groups
        "mp4_demux_batch": 4,
        "packed_audio_batch": 2,
        "index_batch": 1,            # the clear MPEG-TS group (ts_sample, ts_frag); packed audio brings its own index
        "sample_decrypt_batch": 1,   # ts_sample's group
        "caption_batch": 2,          # mp4_clear's group and mp4_cbcs's
        "remux_batch": 3,            # ts_frag's group, aac_enc's, aac_clear's
        "fragment_batch": 2,         # ts_frag's group, aac_clear's
        "config_batch": 3,           # behind every remux
        "hevc_config_batch": 3,
        "cbcs_decrypt_batch": 1,
        "cenc_decrypt_batch": 1,
    }


@pytest.mark.parametrize("container", ["ts", "mp4", "aac"])
def test_a_stage_that_fails_reaches_the_jobs_of_its_container_only(container):
    kw = {"ts": {}, "mp4": dict(mp4=parse_init(mp.INIT)), "aac": dict(packed_audio=True)}[container]
    out, order, pipe = run("cpu", specs(), extra=[("unstageable", 3.5, kw)])
    mixed = mixed_cpu()[0]
    hit = [s[0] for s in of(container)] + ["unstageable"]
    for name in hit:
        r = out[name]
        assert isinstance(r["error"], TypeError) and "unsupported payload type" in str(r["error"])
        if container == "ts":
            assert dict(r) == {"error": r["error"]}
        else:
            assert dict(r) == {"error": r["error"], "status": -1, "container": container}
    assert len({id(out[name]["error"]) for name in hit}) == 1  # the one exception of the stage
    for name in mixed:
        if name not in hit:
            assert digest(out[name]) == mixed[name], name
    assert len(order) == 21 and sorted(order[:8] if container == "mp4" else order[-8:] if container == "ts"
                                       else order[7:14]) == sorted(hit)


@pytest.mark.gpu
def test_the_mixed_batch_on_the_device_equals_the_cpu_pipeline(cuda):
    out, order, pipe = run(cuda, specs())
    devices = []
    dev = {k: digest(r, devices) for k, r in out.items()}
    cpu, cpu_order, counters = mixed_cpu()
    for name in cpu:
        assert dev[name] == cpu[name], name
    assert order == cpu_order and (pipe.segments, pipe.bytes_in, pipe.batches) == counters
    assert devices and set(devices) == {"cuda"}
