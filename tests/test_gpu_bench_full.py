"""`bench.py` plain and with `--full`: a plain run prints the headline line and nothing that needs runs of its own (no sustained region,
no per-launch profile or rooflines, no sub-records, no CPU baseline); `--full` adds the sustained region and the per-launch records."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "4", "--warmup", "2", "--repeats", "2"]
FULL_ONLY = ("schedule", "roofline", "roofline_end_to_end", "kernel_time_table", "step_breakdown", "loss_curve_deviation", "parity_mode",
             "other_configs", "cpu_baseline")


def _bench(extra):
    p = subprocess.run([sys.executable, "bench.py"] + ARGS + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    return json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])


def test_plain_run_prints_the_headline_only(cuda):
    out = _bench([])
    assert out["metric"] == "DDPG update steps/sec (batch 2048, frame 10, emb 128)" and out["unit"] == "steps/s"
    assert out["higher_is_better"] is True and out["dtype"] == "bf16" and out["steps"] == 4 and out["warmup"] == 2
    assert len(out["ms_per_step_samples"]) == 2 and out["ms_per_step"] > 0
    assert abs(out["value"] - 1e3 / out["ms_per_step"]) <= 1e-6 * out["value"]
    assert out["sustained"] is None
    assert not set(FULL_ONLY) & set(out), sorted(set(FULL_ONLY) & set(out))


def test_full_run_adds_the_sustained_region_and_per_launch_records(cuda):
    out = _bench(["--full", "--no-traffic", "--no-extras", "--no-cpu-baseline"])
    assert out["ms_per_step"] > 0 and len(out["ms_per_step_samples"]) == 2
    assert out["sustained"]["steps"] == 2000 and out["sustained"]["ms_per_step"] > 0
    assert out["schedule"] in ("fused", "cycle") and out["roofline"]["kernel"] and out["kernel_time_table"]
    assert out["step_breakdown"]["launches"] and out["roofline_end_to_end"]["tflops"] > 0
