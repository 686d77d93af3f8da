"""The host SPS parser under AddressSanitizer and UndefinedBehaviorSanitizer, as a plain
executable: ``runtime/codec.cpp`` and ``tests/native/codec_main.cpp`` built with
``g++ -fsanitize=address,undefined``, fed every SPS of the hand-built cases plus 20,000 random
blobs, its printed rows equal to the reference parser's (``tests/codec_cases.py``)."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import codec_cases as cc

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "hlsjs_p2p_wrapper_amd" / "ops" / "csrc"
FIELDS = cc.NAMES[6:16]


def random_blobs(count: int, seed: int = 41) -> list:
    """Blobs of 0..80 bytes: random bytes with runs of zeros and planted ``00 00 03``, some on top of a
    valid head, a high profile in every third."""
    rng = np.random.default_rng(seed)
    head = cc.sps_nal(**cc.HIGH_1080)
    out = []
    for i in range(count):
        n = int(rng.integers(0, 81))
        b = rng.integers(0, 256, n, dtype=np.uint8)
        b[rng.random(n) < 0.25] = 0
        if n >= 3 and i % 2:
            j = int(rng.integers(0, n - 2))
            b[j:j + 3] = (0, 0, 3)
        if n >= 2 and i % 3 == 0:
            b[1] = cc.HIGH_PROFILES[i % len(cc.HIGH_PROFILES)]
        if i % 5 == 0:
            k = int(rng.integers(0, len(head)))
            b = np.concatenate([np.frombuffer(head[:k], np.uint8), b])
        out.append(b.tobytes())
    return out


@pytest.fixture(scope="module")
def parser(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ to build the stand-alone parser with")
    exe = tmp_path_factory.mktemp("codec_native") / "codec_main"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", f"-I{CSRC / 'shared'}", f"-I{CSRC / 'runtime'}",
           str(CSRC / "runtime" / "codec.cpp"), str(REPO / "tests" / "native" / "codec_main.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0:
        if "asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr:
            pytest.skip("the sanitizer runtime cannot be linked here: " + built.stderr.strip().splitlines()[-1])
        pytest.fail(built.stderr)
    return exe


def test_sanitized_parser_equals_the_reference(parser, tmp_path):
    blobs = cc.all_sps_blobs() + random_blobs(20_000)
    assert len(blobs) > 20_300
    path = tmp_path / "blobs.bin"
    path.write_bytes(b"".join(struct.pack("<I", len(b)) + b for b in blobs))
    ran = subprocess.run([str(parser), str(path)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr, ran.stderr[-2000:]
    got = np.array([line.split() for line in ran.stdout.splitlines()], dtype=np.int64)
    assert got.shape == (len(blobs), 12)
    want = np.empty_like(got)
    for i, b in enumerate(blobs):
        f = cc.ref_parse_sps(b)
        want[i] = [int(f["ok"]), f["sps_rbsp_bytes"]] + [f[k] for k in FIELDS]
    bad = np.argwhere(got != want)
    assert not len(bad), f"blob {bad[0][0]} ({blobs[bad[0][0]].hex()}): got {got[bad[0][0]]}, want {want[bad[0][0]]}"
    assert 100 < int(want[:, 0].sum()) < len(blobs)  # both outcomes
