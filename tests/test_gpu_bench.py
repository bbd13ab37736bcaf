"""bench.py on the GPU: a plain run with --dump-outputs writes what its last
timed step returned, and that is the round the arguments determine."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from conftest import assert_bitexact
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_steps_grad_and_residual(tmp_path):
    """N = 1, 32 MiB bucket (8 Mi elements: above Runner.DUMP_ELEMS, so the seeded sample is what is
    written), 3 timed steps after 2: the last step is the fifth, its input the generator's bucket
    SEED + 4, its grad that bucket bit for bit (n == 1: a copy) and its residual zero.  The line is
    the plain one: no check, no leg."""
    steps, warmup, mib = 3, 2, 32
    elems = mib << 18
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "ONO_BENCH_DEADLINE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--bucket-mib", str(mib), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["roofline"]["launches"] == steps
    assert "check" not in line and "host_fed" not in line and "cpu_baseline" not in line
    assert sorted(os.listdir(tmp_path)) == ["grad.npy", "residual.npy"]
    grad, res = np.load(tmp_path / "grad.npy"), np.load(tmp_path / "residual.npy")
    n = bench.Runner.DUMP_ELEMS
    assert grad.dtype == res.dtype == np.float32 and grad.shape == res.shape == (n,)
    idx = np.sort(np.random.default_rng(bench.SEED).integers(0, elems, n, dtype=np.int64))
    assert_bitexact(grad, O.synth(elems, bench.SEED + steps + warmup - 1, 0)[idx], "grad sample")
    assert not res.view(np.uint32).any()
