#!/usr/bin/env python3
"""Sampled-softmax next-item training (csrc/sampled.hip): forward + backward from Python at B = 2048 rows,
K in {128, 256}, N in {100,000, 1,000,000} items, S in {1024, 4096, 16384} shared negatives, fp32 and bf16, beside two other routes on
the same inputs in the same process:
  sampled        `functional.sampled_cross_entropy(x, W, c, a, neg, target_log_q=, negative_log_q=)` + backward, dense dW [N, K]
  sampled sparse the same with `sparse_grad=True` (compact rows, no scatter launch for W; the bias gradient stays dense)
  eager          `Ws = W[neg]; cross_entropy(cat([z_t - tq, x @ Ws.T + c[neg] - nq], 1), 0)` + backward (fp32 whatever the row's dtype;
                 torch's index backward makes the dense dW)
  full           `functional.catalogue_cross_entropy(x, W, c, a)` + backward, the fused full softmax of section 27 (N = 100,000 only)
Every time is the median of 5 device-event windows of back-to-back calls after a warm-up call, in microseconds per call (DESIGN.md
section 20's method, tools/ope_bench.py's code); the sampled route is timed before and after the eager one (`sampled_again_us`: the
spread of the run).  `*_peak_bytes` is the rise of torch's peak allocated memory during one forward + backward, gradients included.
`max_rel_diff` compares the sampled and the eager gradients with accidental hits left in (the eager route does not remove them).
Prints one JSON object and writes it to profiles/sampled_bench.json.
usage: python tools/sampled_bench.py [--quick] [--out profiles/sampled_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from ope_bench import device_us, peak_rise  # noqa: E402

B = 2048
KS = (128, 256)
NS = (100_000, 1_000_000)
SS = (1024, 4096, 16384)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="short windows, the smallest case of each K only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampled_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sampled_bench.py measures on the GPU and none is visible")
    from recnn_amd.nn import NegativeSampler
    from recnn_amd.nn import functional as F
    dev = torch.device("cuda")
    torch.manual_seed(0)
    window = 0.05 if a.quick else 0.5
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "sampled_bench", "B": B, "device": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", "unknown"),
           "window_s": window, "cases": []}
    for K in KS:
        for N in NS[:1] if a.quick else NS:
            x = torch.randn(B, K, device=dev, requires_grad=True)
            W = (torch.randn(N, K, device=dev) / K ** 0.5).requires_grad_(True)
            c = torch.randn(N, device=dev, requires_grad=True)
            acts = torch.randint(0, N, (B,), device=dev)
            sampler = NegativeSampler(N, seed=1, device=dev)
            tq = sampler.log_q(acts)

            def grads(loss):
                return torch.autograd.grad(loss, (x, W, c))
            full = {}
            if N == NS[0]:
                for dtype in ("fp32", "bf16"):
                    def full_fn():
                        return grads(F.catalogue_cross_entropy(x, W, c, acts, dtype=dtype))
                    full[dtype] = (device_us(full_fn, window)[0], peak_rise(full_fn))
            for S in SS[:1] if a.quick else SS:
                neg, nq = sampler.sample(S)

                def eager():
                    zt = (x * W[acts]).sum(1, keepdim=True) + (c[acts] - tq)[:, None]
                    z = torch.addmm((c[neg] - nq)[None], x, W[neg].T)
                    return grads(torch.nn.functional.cross_entropy(torch.cat([zt, z], 1), torch.zeros(B, dtype=torch.int64, device=dev)))
                for dtype in ("fp32", "bf16"):
                    def sampled(hits=True, sparse=False):
                        return grads(F.sampled_cross_entropy(x, W, c, acts, neg, target_log_q=tq, negative_log_q=nq, dtype=dtype,
                                                             remove_accidental_hits=hits, sparse_grad=sparse))
                    s_us, n_s = device_us(sampled, window)
                    e_us, n_e = device_us(eager, window)
                    again_us, _ = device_us(sampled, window)
                    sp_us, _ = device_us(lambda: sampled(sparse=True), window)
                    diffs = [float((p - q).abs().max() / q.abs().max()) for p, q in zip(sampled(hits=False), eager())]
                    case = {"dtype": dtype, "K": K, "n_items": N, "S": S, "sampled_us": round(s_us, 1), "sampled_again_us": round(again_us, 1),
                            "sampled_sparse_us": round(sp_us, 1), "eager_us": round(e_us, 1), "iters": [n_s, n_e],
                            "eager_over_sampled": round(e_us / s_us, 3), "sampled_peak_bytes": peak_rise(sampled),
                            "sampled_sparse_peak_bytes": peak_rise(lambda: sampled(sparse=True)), "eager_peak_bytes": peak_rise(eager),
                            "max_rel_diff": {"dx": diffs[0], "dW": diffs[1], "dc": diffs[2]}}
                    if dtype in full:
                        case.update({"full_us": round(full[dtype][0], 1), "full_over_sampled": round(full[dtype][0] / s_us, 2),
                                     "full_peak_bytes": full[dtype][1], "n_over_s_plus_1": round(N / (S + 1), 1)})
                    out["cases"].append(case)
                    print(json.dumps(case), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
