"""bench.py as the driver runs it, at a tiny shape: a plain run prints the headline line without the --full measurements, and
--dump-outputs writes the last timed step's losses."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_the_last_ones_outputs(tmp_path):
    out_dir = str(tmp_path / "outputs")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--hidden", "64",
           "--seq-len", "8", "--voices", "2", "--latent", "16", "--batch", "16", "--prewarm-max", "0", "--dump-outputs", out_dir]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    line = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "windows/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert not {"cpu_baseline", "other_configs", "fit_e2e"} & set(line) and "elbo_gpu" not in line["elbo"]
    files = sorted(os.listdir(out_dir))
    assert "metric.loss.npy" in files and "metric.kl.npy" in files and "metric.notes_loss.npy" in files
    assert all(f.startswith("metric.") and (f.endswith("_loss.npy") or f in ("metric.loss.npy", "metric.kl.npy")) for f in files)
    loss = np.load(os.path.join(out_dir, "metric.loss.npy"))
    assert loss.dtype == np.float64 and loss.tolist() == [line["elbo"]["loss_final"]]
