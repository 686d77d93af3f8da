"""The host AC-3 / E-AC-3 op under AddressSanitizer and UndefinedBehaviorSanitizer, as a plain
executable: ``runtime/ac3audio.cpp`` as shipped and ``tests/native/ac3audio_main.cpp``, built with
``g++ -fsanitize=address,undefined``, fed the fuzz, walk, damaged, overflow and mixed batches of
``ac3audio_cases.py``, every segment's ES in a heap buffer of exactly ``cap`` bytes and its output
region in one of exactly ``region`` bytes.  Its output equals the independent reference.  Nothing
loaded into Python runs under a sanitizer; no sanitizer runs on the GPU."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ac3audio_cases as ac

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "hlsjs_p2p_wrapper_amd" / "ops" / "csrc"
SANITIZE = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The sanitized driver.  The package itself is built with ``g++``, so its absence is a failure;
    whether the sanitizer runtimes can be linked is probed with a trivial program before any of the
    code under test is compiled, and only that probe may skip.  A failed build of
    ``runtime/ac3audio.cpp`` or of the driver fails the test."""
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is what the package is built with"
    tmp = tmp_path_factory.mktemp("ac3audio_native")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([gxx, *SANITIZE, str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if probed.returncode != 0 or subprocess.run([str(tmp / "probe")]).returncode != 0:
        why = (probed.stderr.strip().splitlines() or ["the probe did not run"])[-1]
        pytest.skip("the sanitizer runtimes cannot be linked here: " + why)
    exe = tmp / "ac3audio_main"
    built = subprocess.run([gxx, *SANITIZE, f"-I{CSRC / 'shared'}", f"-I{CSRC / 'runtime'}",
                            str(CSRC / "runtime" / "ac3audio.cpp"),
                            str(REPO / "tests" / "native" / "ac3audio_main.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    return exe


@pytest.mark.parametrize("name", ["fuzz0", "fuzz1", "fuzz2", "walk", "walk_acmod", "walk_header", "damaged", "overflow",
                                  "mixed", "mixed_mpa"])
def test_sanitized_driver_equals_the_reference(driver, tmp_path, name):
    r, want = ac.host(name), ac.expected(name)
    B = len(r.caps)
    es, info, pes = r.es_before, r.res.info.numpy(), r.res.pes.numpy()
    parts = [np.array([B, r.max_pes, r.max_aframes, int(r.with_mpa)], "<i8").tobytes()]
    for i in range(B):
        o, cap, oo, region = int(r.res.es_offs[i]), int(r.caps[i]), int(r.offs[i]), int(r.rx.region[i])
        parts += [np.array([cap, region], "<i8").tobytes(), es[o:o + cap].tobytes(), info[i].tobytes(),
                  pes[i].tobytes(), r.before["rinfo"][i].tobytes(), r.before["asamples"][i].tobytes(),
                  r.before["out"][oo:oo + region].tobytes()]
        if r.with_mpa:
            parts.append(r.mpa_before[i].tobytes())
    src, dst = tmp_path / "batch.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(parts))
    ran = subprocess.run([str(driver), str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr, ran.stderr[-3000:]
    data, p = dst.read_bytes(), 0
    shapes = {"dframes": ((r.max_pes, 2), np.int32), "ac3info": ((16,), np.int64), "mpainfo": ((8,), np.int64),
              "asamples": ((r.max_aframes, 2), np.int32), "rinfo": ((8,), np.int64)}
    for i in range(B):
        for k, (shape, dtype) in shapes.items():
            a = np.frombuffer(data, dtype, int(np.prod(shape)), p).reshape(shape)
            p += a.nbytes
            assert np.array_equal(a, want[k][i]), (k, i)
        oo, region = int(r.offs[i]), int(r.rx.region[i])
        assert data[p:p + region] == want["out"][oo:oo + region].tobytes(), i
        p += region
    assert p == len(data)
