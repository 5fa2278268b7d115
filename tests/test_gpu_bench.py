"""bench.py on the GPU: a plain run prints the headline figure from its timed steps and writes --dump-outputs, and
measures nothing that takes runs of its own (that is --full's)."""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_plain_run_prints_the_headline_and_nothing_more(tmp_path):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TORCHELASTIC_RUN_ID")}
    dump = tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--dump-outputs", str(dump)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["unit"] == "detector-samples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["flags"] == 0
    per_step = line["config"]["n_det_total"] * line["config"]["n_samples"]
    assert abs(line["value"] / (per_step / (line["ms_per_step"] * 1e-3)) - 1) < 1e-6
    assert 0.0 < line["gpu_ms_per_step"] <= line["ms_per_step"] * 1.01
    for key in ("roofline", "second_kernel", "cpu_baseline", "frontend"):
        assert key not in line, key
    assert "serial_breakdown" not in line["stage_ms"]
    assert sorted(os.listdir(dump)) == ["screens.npy", "tod.npy", "tod_rows.npy"]
    assert {n: list(np.load(dump / f"{n}.npy").shape) for n in line["dump_outputs"]["arrays"]} == line["dump_outputs"]["arrays"]
    assert np.isfinite(np.load(dump / "tod.npy")).all()
