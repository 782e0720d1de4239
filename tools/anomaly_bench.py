#!/usr/bin/env python3
"""AnomalyDetector timings (csrc/anomaly.hip): eval rec_error at 27,278 rows (ML-20M's movie count) and 100,000 rows, and one
training step at 15,000 rows (forward + MSE + backward + recnn_amd.optim.Adam, the training notebook's batch).  The same calls
through eager torch on the same GPU are timed for comparison only.  Device-event timing after warm-up; FLOPs from the shapes
(40,960 per row forward, backward twice that, the input gradient not taken) against the fp32-MFMA floor.  Kernel times come
from a separate `rocprofv3 --kernel-trace --stats -- python tools/anomaly_bench.py` run.  Prints one JSON object.
usage: python tools/anomaly_bench.py [--iters 50] [--warmup 10] [--no-torch]"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

FWD_FLOP_PER_ROW = 2 * (128 * 64 + 64 * 32 + 32 * 64 + 64 * 128)   # 40,960
FP32_MATRIX_TFLOPS = 155.0                                           # measured fp32 MFMA rate


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters        # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    from recnn_amd.nn.models import AnomalyDetector
    from recnn_amd.optim import Adam
    dev = torch.device("cuda")
    torch.manual_seed(0)
    ad = AnomalyDetector().to(dev)
    eager = copy.deepcopy(ad.ae)
    res = {"device": torch.cuda.get_device_name(0), "fp32_matrix_tflops_assumed": FP32_MATRIX_TFLOPS}

    def floor_us(flop):
        return flop / (FP32_MATRIX_TFLOPS * 1e12) * 1e6

    for rows in (27278, 100000):
        x = torch.rand(rows, 128, device=dev)
        ad.eval()
        eager.eval()
        with torch.no_grad():
            us = timed(lambda: ad.rec_error(x), a.iters, a.warmup)
            flop = FWD_FLOP_PER_ROW * rows
            r = {"hip_us": round(us, 2), "gflop": round(flop / 1e9, 3), "floor_us": round(floor_us(flop), 2),
                 "share_of_floor": round(floor_us(flop) / us, 3)}
            if not a.no_torch:
                r["torch_us"] = round(timed(lambda: torch.sum((x - eager(x)) ** 2, 1), a.iters, a.warmup), 2)
        res[f"eval_rec_error_{rows}"] = r

    rows = 15000
    x = torch.rand(rows, 128, device=dev)
    crit = nn.MSELoss()
    ad.train()
    opt = Adam(ad.parameters(), lr=1e-3)

    def step():
        opt.zero_grad()
        loss = crit(ad(x), x)
        loss.backward()
        opt.step()
    us = timed(step, a.iters, a.warmup)
    flop = 3 * FWD_FLOP_PER_ROW * rows
    r = {"hip_us": round(us, 2), "gflop": round(flop / 1e9, 3), "floor_us": round(floor_us(flop), 2),
         "share_of_floor": round(floor_us(flop) / us, 3)}
    if not a.no_torch:
        eager.train()
        opt_t = torch.optim.Adam(eager.parameters(), lr=1e-3)

        def step_t():
            opt_t.zero_grad()
            loss = crit(eager(x), x)
            loss.backward()
            opt_t.step()
        r["torch_us"] = round(timed(step_t, a.iters, a.warmup), 2)
    res["train_step_15000"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
