"""``bench.py --dump-outputs DIR``: the arrays the last timed step delivered, in an order and
with contents that depend on the arguments only (so two builds can be compared array for
array), and ``--full`` is accepted.  The smallest stream, 8 packaged segments.

``golden/bench_outputs_hostcost_micro.npz`` holds the six arrays as the host kernels deliver
them (``bench.py --cpu --players 0`` with the arguments of ``_bench``, saved with
``numpy.savez_compressed``): the in-process player, the fleet and the gfx950 kernels must all
deliver exactly these."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]
GOLDEN = Path(__file__).resolve().parent / "golden" / "bench_outputs_hostcost_micro.npz"
NAMES = {"segment", "info", "plain_bytes", "pes", "es_checksum", "es_sample"}


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _bench(out: Path, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--config", "hostcost-micro",
                        "--steps", "3", "--warmup", "1", "--pool", "8", "--inflight", "8", "--dump-outputs", str(out),
                        *extra], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["errors"] == 0
    return rec, {f.stem: np.load(f) for f in sorted(out.glob("*.npy"))}


def _same(got, golden):
    assert set(got) == NAMES == set(golden)
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    for k in sorted(NAMES):
        assert got[k].dtype == golden[k].dtype and got[k].shape == golden[k].shape, k
        assert np.array_equal(got[k], golden[k]), k


def test_golden_is_a_clean_batch(golden):
    # one row per packaged segment of the pool, in pool order, every one demuxed cleanly
    assert golden["segment"].tolist() == [[0.0, float(i)] for i in range(8)]
    assert (golden["info"][:, 0] == 0).all() and (golden["plain_bytes"] > 0).all()
    assert (golden["es_checksum"][:, :2] > 0).all() and (golden["es_sample"][:, :2] >= 0).all()


def test_dump_outputs_cpu_in_process_player(tmp_path, golden):
    _, got = _bench(tmp_path, "--cpu", "--players", "0", "--full")
    _same(got, golden)


def test_dump_outputs_cpu_fleet(tmp_path, golden):
    rec, got = _bench(tmp_path, "--cpu", "--players", "2")
    assert rec["config"]["player_processes"] is True
    _same(got, golden)


@pytest.mark.gpu
def test_dump_outputs_gpu_fleet(tmp_path, golden):
    """The flagship path (fleet players, columnar batches, the gfx950 decrypt + demux kernels)."""
    rec, got = _bench(tmp_path, "--players", "2")
    assert rec["config"]["device"] == "MI355X"
    _same(got, golden)
