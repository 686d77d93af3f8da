"""The host HEVC SPS parser under AddressSanitizer and UndefinedBehaviorSanitizer, as a plain
executable: ``runtime/hevc.cpp`` and ``tests/native/hevc_main.cpp`` built with
``g++ -fsanitize=address,undefined``, fed every hand-built SPS plus 20,000 random blobs, its
printed rows equal to the reference parser's (``tests/hevc_cases.py``)."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import hevc_cases as hc

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "hlsjs_p2p_wrapper_amd" / "ops" / "csrc"


def random_blobs(count: int, seed: int = 71) -> list:
    """Blobs of 0..120 bytes: random bytes with runs of zeros and planted ``00 00 03``, two in five
    on top of a valid head (the header and a cut of a sub-layered SPS), a plausible first RBSP byte
    in every third of the rest."""
    rng = np.random.default_rng(seed)
    heads = [hc.SPS_A, hc.sps_nal(L=3, sub=[(1, 0), (0, 1), (1, 1)], window=(1, 2, 3, 4)),
             hc.sps_nal(L=6, sub=[(1, 1)] * 6, sub_fill=0)]
    out = []
    for i in range(count):
        n = int(rng.integers(0, 81))
        b = rng.integers(0, 256, n, dtype=np.uint8)
        b[rng.random(n) < 0.25] = 0
        if n >= 3 and i % 2:
            j = int(rng.integers(0, n - 2))
            b[j:j + 3] = (0, 0, 3)
        if n >= 3 and i % 3 == 0:
            b[2] = int(rng.integers(0, 16))  # vps id 0, a sub-layer count and the nesting flag
        if i % 5 in (0, 1):
            head = heads[i % len(heads)]
            k = int(rng.integers(0, len(head) + 1))
            tail = b if i % 5 == 0 else b[:int(rng.integers(0, 4))]
            b = np.concatenate([np.frombuffer(head[:k], np.uint8), tail])
        out.append(b.tobytes())
    return out


@pytest.fixture(scope="module")
def parser(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ to build the stand-alone parser with")
    exe = tmp_path_factory.mktemp("hevc_native") / "hevc_main"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", f"-I{CSRC / 'shared'}", f"-I{CSRC / 'runtime'}",
           str(CSRC / "runtime" / "hevc.cpp"), str(REPO / "tests" / "native" / "hevc_main.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0:
        if "asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr:
            pytest.skip("the sanitizer runtime cannot be linked here: " + built.stderr.strip().splitlines()[-1])
        pytest.fail(built.stderr)
    return exe


def test_sanitized_parser_equals_the_reference(parser, tmp_path):
    blobs = hc.all_sps_blobs() + random_blobs(20_000)
    assert len(blobs) > 20_500
    path = tmp_path / "blobs.bin"
    path.write_bytes(b"".join(struct.pack("<I", len(b)) + b for b in blobs))
    ran = subprocess.run([str(parser), str(path)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr, ran.stderr[-2000:]
    got = np.array([line.split() for line in ran.stdout.splitlines()], dtype=np.int64)
    assert got.shape == (len(blobs), 16)
    want = np.empty_like(got)
    for i, b in enumerate(blobs):
        f = hc.ref_parse_sps(b)
        want[i] = [int(f["ok"]), f["sps_rbsp_bytes"]] + [f[k] for k in hc.PARSED]
    bad = np.argwhere(got != want)
    assert not len(bad), f"blob {bad[0][0]} ({blobs[bad[0][0]].hex()}): got {got[bad[0][0]]}, want {want[bad[0][0]]}"
    random_ok = int(want[-20_000:, 0].sum())
    # both outcomes, among the random ones too
    assert 100 < random_ok < 20_000 and 100 < int(want[:, 0].sum()) < len(blobs)
    assert int((want[:, 1] < np.array([max(len(b) - 2, 0) for b in blobs])).sum()) > 1000  # escapes were dropped
