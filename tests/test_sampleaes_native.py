"""The host SAMPLE-AES decrypt under AddressSanitizer and UndefinedBehaviorSanitizer, as a plain
executable: ``runtime/sampleaes.cpp``, ``runtime/aes_host.cpp`` and
``tests/native/sampleaes_main.cpp`` built with ``g++ -fsanitize=address,undefined``, fed the
damaged-row batch of ``test_sampleaes.py`` and the ``long`` case (a NAL of 70,000 bytes), every
segment's ES in a heap buffer of exactly ``cap`` bytes.  Its output equals the in-process result
and, on the undamaged case, the independent reference."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sampleaes_cases as sc
from hlsjs_p2p_wrapper_amd.ops import sampleaes
from test_sampleaes import damaged_batch

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "hlsjs_p2p_wrapper_amd" / "ops" / "csrc"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ to build the stand-alone driver with")
    exe = tmp_path_factory.mktemp("sampleaes_native") / "sampleaes_main"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", f"-I{CSRC / 'shared'}", f"-I{CSRC / 'runtime'}",
           str(CSRC / "runtime" / "sampleaes.cpp"), str(CSRC / "runtime" / "aes_host.cpp"),
           str(REPO / "tests" / "native" / "sampleaes_main.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0:
        if "asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr:
            pytest.skip("the sanitizer runtime cannot be linked here: " + built.stderr.strip().splitlines()[-1])
        pytest.fail(built.stderr)
    return exe


def serialize(res, caps, ix, keys, ivs) -> bytes:
    es = res.es.numpy()
    out = [np.array([len(caps), res.pes.shape[2], ix.nal.shape[1]], "<i8").tobytes()]
    for i, c in enumerate(caps):
        o = int(res.es_offs[i])
        out += [np.array([c], "<i8").tobytes(), es[o:o + c].tobytes(), keys[i], ivs[i]]
        out += [t[i].numpy().tobytes() for t in (res.info, res.pes, ix.nal, ix.au, ix.aframes, ix.sinfo)]
    return b"".join(out)


def run(driver, tmp_path, res, caps, ix, keys, ivs):
    """The driver's ``(es, nal, sainfo)`` per segment."""
    src, dst = tmp_path / "batch.bin", tmp_path / "out.bin"
    src.write_bytes(serialize(res, caps, ix, keys, ivs))
    ran = subprocess.run([str(driver), str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr, ran.stderr[-3000:]
    data, p, out = dst.read_bytes(), 0, []
    max_nal = ix.nal.shape[1]
    for c in caps:
        es = np.frombuffer(data, np.uint8, c, p)
        nal = np.frombuffer(data, "<i4", max_nal * 4, p + c).reshape(max_nal, 4)
        sainfo = np.frombuffer(data, "<i8", sampleaes.SAINFO_WORDS, p + c + max_nal * 16)
        out.append((es, nal, sainfo))
        p += c + max_nal * 16 + 8 * sampleaes.SAINFO_WORDS
    assert p == len(data)
    return out


def compare(got, res, caps, nal, sainfo):
    es = res.es.numpy() if hasattr(res.es, "numpy") else res.es
    for i, (c, (ges, gnal, gsa)) in enumerate(zip(caps, got)):
        o = int(res.es_offs[i])
        assert np.array_equal(ges, es[o:o + c]), i
        assert np.array_equal(gnal, nal[i]) and np.array_equal(gsa, sainfo[i]), i


def test_sanitized_driver_on_damaged_rows(driver, tmp_path):
    res, caps, ix, keys, ivs, _ = damaged_batch()
    got = run(driver, tmp_path, res, caps, ix, keys, ivs)
    sa = sampleaes.sample_decrypt_batch(res, ix, caps, keys, ivs)  # in place, after the driver read the batch
    compare(got, res, caps, ix.nal.numpy(), sa.sainfo.numpy())
    assert sa.sainfo[:, sampleaes.SAINFO["protected_nals"]].sum() > 20  # the damage left work to do


def test_sanitized_driver_on_the_long_case(driver, tmp_path):
    _, (res, caps, ix), keys, ivs, _, _ = sc.batch("long")
    assert max(caps) > 70000
    got = run(driver, tmp_path, res, caps, ix, keys, ivs)
    want_es, want_nal, want_sainfo = sc.ref_batch(res, ix, caps, keys, ivs)
    res.es = want_es
    compare(got, res, caps, want_nal, want_sainfo)
