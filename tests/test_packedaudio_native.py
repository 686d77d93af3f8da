"""The host packed-audio demux under AddressSanitizer and UndefinedBehaviorSanitizer, as a plain
executable: ``runtime/packedaudio.cpp`` as shipped and ``tests/native/packedaudio_main.cpp``, which
also runs the same passes over a reader of its own without a range test (so a rule that asked for a
byte outside the segment would be seen) and compares the two, built with
``g++ -fsanitize=address,undefined``, fed the fuzz batches and the tag and break cases of
``packedaudio_cases.py``, every segment in a heap buffer of exactly ``cap`` bytes.  Its output
equals the independent reference.  Nothing loaded into Python runs under a sanitizer; no sanitizer
runs on the GPU."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import packedaudio_cases as pc
from test_packedaudio_gpu import shapes

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "hlsjs_p2p_wrapper_amd" / "ops" / "csrc"
SANITIZE = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-fno-omit-frame-pointer"]
DTYPES = {"info": np.int64, "pes": np.int64, "nal": np.int32, "au": np.int32, "aframes": np.int32, "sinfo": np.int64,
          "painfo": np.int64}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The sanitized driver.  The package itself is built with ``g++``, so its absence is a failure;
    whether the sanitizer runtimes can be linked is probed with a trivial program before any of the
    code under test is compiled, and only that probe may skip.  A failed build of
    ``runtime/packedaudio.cpp`` or of the driver fails the test."""
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is what the package is built with"
    tmp = tmp_path_factory.mktemp("packedaudio_native")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([gxx, *SANITIZE, str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if probed.returncode != 0 or subprocess.run([str(tmp / "probe")]).returncode != 0:
        why = (probed.stderr.strip().splitlines() or ["the probe did not run"])[-1]
        pytest.skip("the sanitizer runtimes cannot be linked here: " + why)
    exe = tmp / "packedaudio_main"
    built = subprocess.run([gxx, *SANITIZE, f"-I{CSRC / 'shared'}", f"-I{CSRC / 'runtime'}",
                            str(CSRC / "runtime" / "packedaudio.cpp"),
                            str(REPO / "tests" / "native" / "packedaudio_main.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    return exe


@pytest.mark.parametrize("name", ["random", "mutated", "tags", "breaks", "counts"])
def test_sanitized_driver_equals_the_reference(driver, tmp_path, name):
    buf, offs, lens, max_pes = pc.batch(name)
    raw, B = buf.numpy().tobytes(), len(offs)
    parts = [np.array([B, max_pes], "<i8").tobytes()]
    for o, n in zip(offs, lens):
        parts += [np.array([n], "<i8").tobytes(), raw[o:o + n]]
    src, dst = tmp_path / "batch.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(parts))
    ran = subprocess.run([str(driver), str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr, ran.stderr[-3000:]
    data, p, rows = dst.read_bytes(), 0, {k: [] for k in pc.NAMES}
    sh = shapes(1, max_pes)
    for o, n in zip(offs, lens):
        for k in pc.NAMES:
            shape = sh[k][0]
            a = np.frombuffer(data, DTYPES[k], int(np.prod(shape)), p).reshape(shape[1:])
            p += a.nbytes
            rows[k].append(a)
        assert data[p:p + n] == raw[o:o + n]  # the segment is only read
        p += n
    assert p == len(data)
    pc.assert_equal({k: np.stack(v) for k, v in rows.items()}, pc.ref_batch(buf, offs, lens, max_pes))
