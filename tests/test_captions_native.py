"""The host caption extraction under AddressSanitizer and UndefinedBehaviorSanitizer, as a plain
executable: ``runtime/captions.cpp`` and ``tests/native/captions_main.cpp`` built with
``g++ -fsanitize=address,undefined``, fed the damaged-row batch of ``test_captions.py`` and the
``long`` case (an SEI of 70,000 bytes), every segment's ES in a heap buffer of exactly ``cap``
bytes.  Its output equals the in-process result and the independent reference."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import captions_cases as cc
from hlsjs_p2p_wrapper_amd.ops import captions
from test_captions import damaged_batch

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "hlsjs_p2p_wrapper_amd" / "ops" / "csrc"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ to build the stand-alone driver with")
    exe = tmp_path_factory.mktemp("captions_native") / "captions_main"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", f"-I{CSRC / 'shared'}", f"-I{CSRC / 'runtime'}",
           str(CSRC / "runtime" / "captions.cpp"), str(REPO / "tests" / "native" / "captions_main.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0:
        if "asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr:
            pytest.skip("the sanitizer runtime cannot be linked here: " + built.stderr.strip().splitlines()[-1])
        pytest.fail(built.stderr)
    return exe


def serialize(res, caps, ix, max_cc) -> bytes:
    es = res.es.numpy()
    out = [np.array([len(caps), res.pes.shape[2], ix.nal.shape[1], max_cc], "<i8").tobytes()]
    for i, c in enumerate(caps):
        o = int(res.es_offs[i])
        out += [np.array([c], "<i8").tobytes(), es[o:o + c].tobytes()]
        out += [t[i].numpy().tobytes() for t in (res.info, res.pes, ix.nal, ix.au, ix.aframes, ix.sinfo)]
    return b"".join(out)


def run(driver, tmp_path, res, caps, ix, max_cc):
    """The driver's five tables stacked like ``Captions``, after checking that it left the ES alone."""
    src, dst = tmp_path / "batch.bin", tmp_path / "out.bin"
    src.write_bytes(serialize(res, caps, ix, max_cc))
    ran = subprocess.run([str(driver), str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and not ran.stderr, ran.stderr[-3000:]
    data, p, out = dst.read_bytes(), 0, []
    parts = (("<i4", (max_cc, 8)), ("<i8", (max_cc,)), ("u1", (max_cc, cc.SLOT)), ("u1", (max_cc, 2, cc.FIELD)),
             ("<i8", (8,)))
    es = res.es.numpy()
    for i, c in enumerate(caps):
        seg = []
        for dt, shape in parts:
            a = np.frombuffer(data, dt, int(np.prod(shape)), p).reshape(shape)
            p += a.nbytes
            seg.append(a)
        o = int(res.es_offs[i])
        assert data[p:p + c] == es[o:o + c].tobytes(), i
        p += c
        out.append(seg)
    assert p == len(data)
    return tuple(np.stack([seg[j] for seg in out]) for j in range(5))


def compare(got, cap_obj, ref):
    for name, g, want in zip(cc.NAMES, got, ref):
        assert np.array_equal(g, want), name
        assert np.array_equal(g, getattr(cap_obj, name).numpy()), name


def test_sanitized_driver_on_damaged_rows(driver, tmp_path):
    res, caps, ix, max_cc = damaged_batch()
    got = run(driver, tmp_path, res, caps, ix, max_cc)
    compare(got, captions.caption_batch(res, ix, caps, max_cc=max_cc), cc.ref_batch(res, ix, caps, max_cc))
    assert got[4][:, captions.CCINFO["n_sei"]].sum() > 500  # the damage left work to do


def test_sanitized_driver_on_the_long_case(driver, tmp_path):
    res, caps, ix, max_cc = cc.batch("long")
    assert max(caps) > 70000
    got = run(driver, tmp_path, res, caps, ix, max_cc)
    compare(got, captions.caption_batch(res, ix, caps, max_cc=max_cc), cc.ref_batch(res, ix, caps, max_cc))
    assert got[4][0, captions.CCINFO["status"]] == cc.CLIPPED
