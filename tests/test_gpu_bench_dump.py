"""`bench.py --dump-outputs DIR`: what the timed path computed in its last timed step -- the losses and every network's parameters --
lands in DIR as float32 / float64 .npy files, and two runs with the same arguments write the same arrays (the inputs are seeded and the
engine sums in a fixed order), so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "4", "--warmup", "2", "--repeats", "1", "--no-extras", "--no-cpu-baseline", "--no-traffic"]


def _bench(out_dir):
    p = subprocess.run([sys.executable, "bench.py"] + ARGS + ["--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    out = json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])
    return out, {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir)) if f.endswith(".npy")}


def test_bench_dumps_the_last_timed_step_reproducibly(cuda, tmp_path):
    out, a = _bench(tmp_path / "a")
    assert out["steps"] == 4 and out["ms_per_step"] > 0
    assert set(a) >= {"loss_value", "loss_policy"}
    for k in ("loss_value", "loss_policy"):
        assert a[k].dtype == np.float64 and a[k].shape == (1,) and np.isfinite(a[k]).all()
    H, state, emb = 256, 1290, 128
    for net, (inp, o) in {"policy_net": (state, emb), "target_policy_net": (state, emb), "value_net": (state + emb, 1),
                          "target_value_net": (state + emb, 1)}.items():
        shapes = {"w1": (H, inp), "b1": (H,), "w2": (H, H), "b2": (H,), "w3": (o, H), "b3": (o,)}
        for p, want in shapes.items():
            x = a[f"{net}.{p}"]
            assert x.dtype == np.float32 and x.shape == want and np.isfinite(x).all(), (net, p, x.dtype, x.shape)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    _, b = _bench(tmp_path / "b")
    assert set(b) == set(a)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
