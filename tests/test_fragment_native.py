"""The host moof writer under AddressSanitizer and UndefinedBehaviorSanitizer, as a plain
executable: ``runtime/fragment.cpp`` and ``tests/native/fragment_main.cpp`` built with
``g++ -fsanitize=address,undefined``, fed the fuzzed-row batch of ``test_fragment.py`` and the time
cases, every segment's headroom and region in one heap buffer of exactly their size.  Its output
equals the in-process result and the independent reference."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fragment_cases as fc
from hlsjs_p2p_wrapper_amd.ops import fragment

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "hlsjs_p2p_wrapper_amd" / "ops" / "csrc"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ to build the stand-alone driver with")
    exe = tmp_path_factory.mktemp("fragment_native") / "fragment_main"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", f"-I{CSRC / 'shared'}", f"-I{CSRC / 'runtime'}",
           str(CSRC / "runtime" / "fragment.cpp"), str(REPO / "tests" / "native" / "fragment_main.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0:
        if "asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr:
            pytest.skip("the sanitizer runtime cannot be linked here: " + built.stderr.strip().splitlines()[-1])
        pytest.fail(built.stderr)
    return exe


def run(driver, tmp_path, rx, ix, params, gap):
    """``(finfo, [bytes per segment])`` of the driver on the tables of ``rx`` and the bytes of
    ``rx.out`` as they are: per segment ``frag_headroom(max_pes)`` bytes and the region."""
    rinfo, vs, asamp = (t.numpy() for t in (rx.rinfo, rx.vsamples, rx.asamples))
    B, max_pes, max_aframes = rinfo.shape[0], vs.shape[1], asamp.shape[1]
    head = fragment.frag_headroom(max_pes)
    out, rates = rx.out.numpy(), ix.sinfo.numpy()[:, 6]
    parts = [np.array([B, max_pes, max_aframes, gap], "<i8").tobytes()]
    for i in range(B):
        o, region, p = int(rx.out_offs[i]), int(rx.region[i]), params[i]
        fp = np.array([o, region, p["seq"], p["base"], p["ref"], int(p["anchor"]), 0, 0], "<i8")
        parts += [rinfo[i].tobytes(), vs[i].tobytes(), asamp[i].tobytes(), np.array([rates[i]], "<i8").tobytes(),
                  fp.tobytes(), out[o - head:o + region].tobytes()]
    src, dst = tmp_path / "batch.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(parts))
    ran = subprocess.run([str(driver), str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr, ran.stderr[-3000:]
    data, p, finfo, regions = dst.read_bytes(), 0, [], []
    for i in range(B):
        finfo.append(np.frombuffer(data, "<i8", 8, p))
        p += 64
        n = head + int(rx.region[i])
        regions.append(data[p:p + n])
        p += n
    assert p == len(data)
    return np.stack(finfo), regions


def check(got, rx_after, finfo_after, want_out, want_finfo, head):
    finfo, regions = got
    assert np.array_equal(finfo, want_finfo) and np.array_equal(finfo, finfo_after.numpy())
    after = rx_after.out.numpy()
    for i, r in enumerate(regions):
        o = int(rx_after.out_offs[i])
        assert r == after[o - head:o + len(r) - head].tobytes(), i
        assert r == want_out[o - head:o + len(r) - head].tobytes(), i


def test_sanitized_driver_on_fuzzed_rows(driver, tmp_path):
    b = fc.build_batch("rows300_10")
    rx = fc.remux_only(b)
    fz, (rinfo, vs, asamp) = fc.fuzz_tables(rx)
    got = run(driver, tmp_path, fz, b.ix, b.params, b.gap)  # on the bytes as they are before the in-process call
    want = rx.out.numpy().copy()
    regions = np.asarray(b.caps, np.int64) + fc.MAX_NAL + 32 + b.gap
    finfo = fc.apply_moofs(want, b.offs, rinfo, vs, asamp, b.ix.sinfo.numpy()[:, 6], b.params, regions, b.gap)
    seq, base, ref, anchor = fc.param_arrays(b.params)
    fr = fragment.fragment_batch(fz, b.ix, seq, time_base=base, time_ref=ref, anchor=anchor)
    check(got, fz, fr.finfo, want, finfo, fragment.frag_headroom(300))
    assert b.headroom == fragment.frag_headroom(300)  # the driver's buffers are the batch's own room, to the byte


@pytest.mark.parametrize("name", ["times", "full"])
def test_sanitized_driver_on_the_cases(driver, tmp_path, name):
    b = fc.build_batch(name)
    rx = fc.remux_only(b)
    ref = fc.expected(name)
    got = run(driver, tmp_path, rx, b.ix, b.params, b.gap)  # on the bytes the remux left
    seq, base, ref_time, anchor = fc.param_arrays(b.params)
    fr = fragment.fragment_batch(rx, b.ix, seq, time_base=base, time_ref=ref_time, anchor=anchor)
    check(got, rx, fr.finfo, ref[3], ref[4], fragment.frag_headroom(rx.vsamples.shape[1]))
