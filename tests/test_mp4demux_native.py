"""The host fragmented-MP4 demux under AddressSanitizer and UndefinedBehaviorSanitizer, as a plain
executable: ``runtime/mp4.cpp`` as shipped and ``tests/native/mp4_main.cpp``, which also runs the same
``demux_segment_with`` over a reader of its own without a range test (so a rule that asked for a
byte outside the segment would be seen) and compares the two, built with
``g++ -fsanitize=address,undefined``, fed the damaged-byte batches and the field cases of
``mp4_cases.py``, every segment in a heap buffer of exactly ``n`` bytes.  Its output equals the
independent reference.  Nothing loaded into Python runs under a sanitizer; no sanitizer runs on
the GPU."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mp4_cases as mc
from hlsjs_p2p_wrapper_amd.ops import mp4demux
from test_mp4demux import shapes

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "hlsjs_p2p_wrapper_amd" / "ops" / "csrc"


SANITIZE = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The sanitized driver.  The package itself is built with ``g++``, so its absence is a failure;
    whether the sanitizer runtimes can be linked is probed with a trivial program before any of the
    code under test is compiled, and only that probe may skip.  A failed build of ``runtime/mp4.cpp``
    or of the driver fails the test."""
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is what the package is built with"
    tmp = tmp_path_factory.mktemp("mp4_native")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([gxx, *SANITIZE, str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if probed.returncode != 0 or subprocess.run([str(tmp / "probe")]).returncode != 0:
        why = (probed.stderr.strip().splitlines() or ["the probe did not run"])[-1]
        pytest.skip("the sanitizer runtimes cannot be linked here: " + why)
    exe = tmp / "mp4_main"
    built = subprocess.run([gxx, *SANITIZE, f"-I{CSRC / 'shared'}", f"-I{CSRC / 'runtime'}",
                            str(CSRC / "runtime" / "mp4.cpp"), str(REPO / "tests" / "native" / "mp4_main.cpp"), "-o",
                            str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    return exe


@pytest.mark.parametrize("name", ["random", "mutated", "fields", "headers", "nal", "emsg"])
def test_sanitized_driver_equals_the_reference(driver, tmp_path, name):
    buf, offs, lens, tracks, lim = mc.batch(name)
    raw, B = buf.numpy().tobytes(), len(offs)
    tk = mp4demux.pack_tracks(tracks, B)
    limits = [lim[k] for k in ("max_pes", "max_nal", "max_moof", "max_run", "max_emsg")]
    parts = [np.array([B, *limits], "<i8").tobytes()]
    for i, (o, n) in enumerate(zip(offs, lens)):
        parts += [np.array([n], "<i8").tobytes(), tk[i].astype("<i8").tobytes(), raw[o:o + n]]
    src, dst = tmp_path / "batch.bin", tmp_path / "out.bin"
    src.write_bytes(b"".join(parts))
    ran = subprocess.run([str(driver), str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr, ran.stderr[-3000:]
    data, p, rows = dst.read_bytes(), 0, {k: [] for k in mc.NAMES}
    sh = shapes(1, lim)
    for o, n in zip(offs, lens):
        for k in mc.NAMES:
            shape, dt = sh[k]
            a = np.frombuffer(data, dt, int(np.prod(shape)), p).reshape(shape[1:])
            p += a.nbytes
            rows[k].append(a)
        assert data[p:p + n] == raw[o:o + n]  # the segment is only read
        p += n
    assert p == len(data)
    mc.assert_equal({k: np.stack(v) for k, v in rows.items()}, mc.ref_batch(buf, offs, lens, tracks, lim))
