#!/usr/bin/env python3
"""Next-item training (csrc/logprob_bwd.hip): forward + backward of the full-softmax cross-entropy over the
catalogue at B = 2048 rows and N = 100,000 items, K in {128, 256}, in the fp32 and the bf16 catalogue mode, each timed beside the
materialising route on the same inputs in the same process:
  fused          `functional.catalogue_cross_entropy(x, W, c, a).backward()`
  materialising  eager `torch.nn.functional.cross_entropy(torch.addmm(c, x, W.T), a).backward()` (fp32 whatever the row's dtype)
Every time is the median of 5 device-event windows of back-to-back calls after a warm-up call, in microseconds per call (DESIGN.md
section 20's method, tools/ope_bench.py's code); the fused route is timed before and after the materialising one (`fused_again_us`:
the spread of the run).  `*_peak_bytes` is the rise of torch's peak allocated memory during one forward + backward, gradients
included.  `mfma_share` is the fused route's 8 B N K FLOP (the logits once forward and once in each backward kernel, and the two
gradient products) over `fused_us` over the MFMA peak of the operand type (157.3 TFLOP/s fp32, 2516 TFLOP/s bf16): a whole-call
rate, not a kernel's.  `max_rel_diff` compares the two routes' gradients (largest difference over the largest magnitude, per
gradient).  Kernel times: a separate `rocprofv3 --kernel-trace --stats -- python tools/xent_bench.py --quick` run.
Prints one JSON object and writes it to profiles/xent_bench.json.
usage: python tools/xent_bench.py [--quick] [--out profiles/xent_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from ope_bench import PEAK_TFLOPS, device_us, peak_rise  # noqa: E402

B, N = 2048, 100_000
KS = (128, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="short windows (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xent_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("xent_bench.py measures on the GPU and none is visible")
    from recnn_amd.nn import functional as F
    dev = torch.device("cuda")
    torch.manual_seed(0)
    window = 0.05 if a.quick else 0.5
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "xent_bench", "B": B, "n_items": N, "device": torch.cuda.get_device_name(0),
           "arch": getattr(props, "gcnArchName", "unknown"), "window_s": window, "matrix_bytes": 4 * B * N, "cases": []}
    for K in KS:
        x = torch.randn(B, K, device=dev, requires_grad=True)
        W = (torch.randn(N, K, device=dev) / K ** 0.5).requires_grad_(True)
        c = torch.randn(N, device=dev, requires_grad=True)
        acts = torch.randint(0, N, (B,), device=dev)

        def grads(loss):
            return torch.autograd.grad(loss, (x, W, c))

        def old():
            return grads(torch.nn.functional.cross_entropy(torch.addmm(c, x, W.T), acts))
        for dtype in ("fp32", "bf16"):
            def fused():
                return grads(F.catalogue_cross_entropy(x, W, c, acts, dtype=dtype))
            fused_us, n_f = device_us(fused, window)
            old_us, n_o = device_us(old, window)
            again_us, _ = device_us(fused, window)
            fwd_us, _ = device_us(lambda: F.catalogue_log_prob(x, W, c, acts, dtype=dtype), window)
            diffs = [float((p - q).abs().max() / q.abs().max()) for p, q in zip(fused(), old())]
            flop = 8.0 * B * N * K
            out["cases"].append({
                "dtype": dtype, "K": K, "fused_us": round(fused_us, 1), "fused_again_us": round(again_us, 1),
                "materialise_us": round(old_us, 1), "forward_only_us": round(fwd_us, 1), "iters": [n_f, n_o],
                "materialise_over_fused": round(old_us / fused_us, 3),
                "fused_peak_bytes": peak_rise(fused), "materialise_peak_bytes": peak_rise(old),
                "items_per_slice_bwd": F.catalogue_bwd_items_per_slice(B, N, K),
                "fused_tflops": round(flop / fused_us / 1e6, 1), "mfma_share": round(flop / fused_us / 1e6 / PEAK_TFLOPS[dtype], 4),
                "max_rel_diff": {"dx": diffs[0], "dW": diffs[1], "dc": diffs[2]}})
            print(json.dumps(out["cases"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
