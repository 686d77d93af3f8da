"""The host cenc decrypt under AddressSanitizer and UndefinedBehaviorSanitizer, as a plain
executable: ``runtime/cenc.cpp``, ``runtime/mp4.cpp`` and ``runtime/aes_host.cpp`` as shipped and
``tests/native/cenc_main.cpp``, which also runs the same ``cenc_segment_with`` over a reader of its
own without a range test (so a rule that asked for a byte outside the segment would be seen) and
compares the two, built with ``g++ -fsanitize=address,undefined``, fed the damaged batch and the
edge cases of ``cenc_cases.py``, every segment and every copy in a heap buffer of exactly ``n``
bytes.  Its output equals the in-process result and the independent reference.  Nothing loaded into
Python runs under a sanitizer; no sanitizer runs on the GPU."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cenc_cases as ce
from hlsjs_p2p_wrapper_amd.ops import cenc, mp4demux

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "hlsjs_p2p_wrapper_amd" / "ops" / "csrc"
SANITIZE = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The sanitized driver.  The package itself is built with ``g++``, so its absence is a failure;
    whether the sanitizer runtimes can be linked is probed with a trivial program before any of the
    code under test is compiled, and only that probe may skip.  A failed build of the runtime files
    or of the driver fails the test."""
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is what the package is built with"
    tmp = tmp_path_factory.mktemp("cenc_native")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([gxx, *SANITIZE, str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if probed.returncode != 0 or subprocess.run([str(tmp / "probe")]).returncode != 0:
        why = (probed.stderr.strip().splitlines() or ["the probe did not run"])[-1]
        pytest.skip("the sanitizer runtimes cannot be linked here: " + why)
    exe = tmp / "cenc_main"
    built = subprocess.run([gxx, *SANITIZE, f"-I{CSRC / 'shared'}", f"-I{CSRC / 'runtime'}",
                            *(str(CSRC / "runtime" / f) for f in ("cenc.cpp", "mp4.cpp", "aes_host.cpp")),
                            str(REPO / "tests" / "native" / "cenc_main.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    return exe


@pytest.mark.parametrize("name", ["damaged", "subsamples", "placement", "lengths", "straddles", "counter", "known",
                                  "limits", "overlap"])
def test_sanitized_driver_equals_the_in_process_result(driver, tmp_path, name):
    b = ce.batch(name)
    raw, B, lim = b.buf.numpy().tobytes(), len(b.offs), b.limits
    tk = mp4demux.pack_tracks(b.tracks, B)
    prot, civ = cenc.pack_protection(b.tracks, B, "cenc_decrypt_batch", "cenc")
    limits = [lim[k] for k in ("max_pes", "max_nal", "max_moof", "max_run", "max_emsg")]
    parts = [np.array([B, *limits, b.max_range], "<i8").tobytes()]
    for i, (o, n) in enumerate(zip(b.offs, b.lens)):
        parts += [np.array([n], "<i8").tobytes(), tk[i].astype("<i8").tobytes(), prot[i].astype("<i8").tobytes(),
                  civ[i].tobytes(), b.ivs[i], b.keys[i], raw[o:o + n]]
    src, dst = tmp_path / "batch.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(parts))
    ran = subprocess.run([str(driver), str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr, ran.stderr[-3000:]
    _, here = ce.run(b)
    _, outs, ranges, cinfo = ce.ref_of(name)
    data, p = dst.read_bytes(), 0
    for i, (o, n) in enumerate(zip(b.offs, b.lens)):
        rg = np.frombuffer(data, "<i4", b.max_range * 8, p).reshape(b.max_range, 8)
        p += rg.nbytes
        ci = np.frombuffer(data, "<i8", 8, p)
        p += ci.nbytes
        assert np.array_equal(rg, here.ranges[i].numpy()) and np.array_equal(ci, here.cinfo[i].numpy()), i
        assert np.array_equal(rg, ranges[i]) and np.array_equal(ci, cinfo[i]), i
        at = int(here.offs[i])
        assert data[p:p + n] == here.buf[at:at + n].numpy().tobytes() == outs[i], i
        p += n
        assert data[p:p + n] == raw[o:o + n]  # the segment is only read
        p += n
    assert p == len(data)
