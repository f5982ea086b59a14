"""bench.py as the measurement of every change runs it: a plain run (the headline line only, exactly --steps timed steps) with
--dump-outputs, whose files are what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import wdsr_numpy as on
from probav_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_timed_step(dev, tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PROBAV_FORCE_DP"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2", "--batch", "8",
                          "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-1500:]
    line = json.loads(lines[0])
    assert line["steps"] == 4 and line["step_ms"]["n"] == 4 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert abs(line["value"] - 8 * 1e3 / line["ms_per_step"]) < 1e-3 * line["value"]
    for leg in ("roofline", "kernel_classes", "sustained_mfma", "fp32_mfma_path", "power", "other_configs", "cpu_baseline", "dp"):
        assert leg not in line, leg
    pred, loss, grad = (np.load(str(tmp_path / (n + ".npy"))) for n in ("pred", "loss", "grad_flat"))
    assert pred.dtype == loss.dtype == grad.dtype == np.float32
    assert pred.shape == (8, 48, 48, 1) and grad.shape == (535267,) and np.isfinite(grad).all() and np.abs(grad).max() > 0
    assert float(loss) == line["config"]["loss"]
    # the dumped prediction is the one the loss was taken of: the step's inputs are bench.py's seeded synthetic batch
    _, hr, mask = synth.synth_batch(8, seed=1234, numImgLR=9)
    assert abs(on.shift_l1_loss(hr, mask, pred.astype(np.float64)) - float(loss)) < 1e-5 * float(loss)
