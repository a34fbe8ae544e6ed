"""GPU: a plain `bench.py` run times exactly --steps steps, leaves the --full legs out of its line, and with --dump-outputs
writes what its last timed step computed (losses + a seeded sample of the updated weights) in float32 / float64."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "1",
           "--height", "192", "--width", "256", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-9)  # batch 1
    for k in ("roofline", "other_mode", "sparse_backward", "value_dense_backward", "cpu_baseline", "inference", "p16_audit"):
        assert line[k] is None, k
    assert sorted(os.listdir(str(out))) == ["losses.npy", "weights.npy"]
    losses, weights = np.load(str(out / "losses.npy")), np.load(str(out / "weights.npy"))
    assert losses.dtype == np.float64 and losses.tolist() == [line["losses"][k] for k in bench.LOSS_KEYS]
    assert weights.dtype == np.float32 and weights.shape == (bench.DUMP_WEIGHTS,) and np.isfinite(weights).all()
    assert losses.nbytes + weights.nbytes <= 64 << 20
