#!/usr/bin/env python3
"""Off-policy evaluation (csrc/logprob.hip): the log-probability of one logged action per row at B = 2048 rows
and N = 100,000 items, for the two heads the package has -- the policy head of `DiscreteActor` (state 1290 -> hidden 2048 ->
catalogue, K = 2048) and `Beta` (state 1290 -> catalogue, K = 1290) -- in the fp32 and the bf16 catalogue mode, each timed beside the
route that existed before `log_prob`, on the same inputs in the same process:
  policy   fused `actor.log_prob(state, a)`            materialising `actor._act(state, actions=a)`
  beta     fused `beta.log_prob(state, a)`             materialising `beta(state)` + `functional.categorical(p, actions=a)`
`head_only_us` is `functional.catalogue_log_prob` alone on a ready hidden layer (the policy row) or state (the beta row): the fused
launch and its merge, padding included.  Every time is the median of 5 device-event windows of back-to-back calls after a warm-up
call, in microseconds per call; the fused route is timed before and after the materialising one (`fused_again_us`: the spread of
the run).  `*_peak_bytes` is the rise of torch's peak allocated memory during one call.  `mfma_share` is the head's
2 B N K' FLOP (K' the padded contraction length) over `head_only_us` over the MFMA peak of the operand type (157.3 TFLOP/s fp32,
2516 TFLOP/s bf16): a whole-call rate, not a kernel's; `floor_us` is the larger of that FLOP count over the peak and one read of W
over 6.3 TB/s, and `floor_from` says which of the two gives it -- the floor's source, not a finding about what limits the launch.  `max_abs_diff` compares the two routes' log-probs where the materialising route's clamp
(log p >= -15.9) is not active.  Kernel times: a separate `rocprofv3 --kernel-trace --stats -- python tools/ope_bench.py --quick` run.
Prints one JSON object and writes it to profiles/ope_bench.json.
usage: python tools/ope_bench.py [--quick] [--out profiles/ope_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

B, N, STATE, HIDDEN = 2048, 100_000, 1290, 2048
PEAK_TFLOPS = {"fp32": 157.3, "bf16": 2516.0}
HBM_TBS = 6.3


def device_us(fn, window_s):
    """Median over 5 device-event windows of back-to-back calls (each about `window_s` long), after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    iters = int(max(1, min(2000, window_s / max(time.perf_counter() - t, 1e-6))))
    times = []
    for _ in range(5):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) * 1e3 / iters)
    return statistics.median(times), iters


def peak_rise(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - start
    del out
    return int(rise)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="short windows (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ope_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ope_bench.py measures on the GPU and none is visible")
    import recnn_amd
    from recnn_amd.nn import functional as F
    dev = torch.device("cuda")
    torch.manual_seed(0)
    window = 0.05 if a.quick else 0.5
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "ope_bench", "B": B, "n_items": N, "device": torch.cuda.get_device_name(0),
           "arch": getattr(props, "gcnArchName", "unknown"), "window_s": window, "matrix_bytes": 4 * B * N,
           "items_per_slice": F.default_items_per_slice(B, N), "cases": []}
    actor = recnn_amd.nn.DiscreteActor(STATE, N, HIDDEN).to(dev)
    beta = recnn_amd.nn.Beta(STATE, N).to(dev)
    state = torch.randn(B, STATE, device=dev)
    acts = torch.randint(0, N, (B,), device=dev)
    with torch.no_grad():
        hidden = torch.relu(state @ actor.linear1.weight.T + actor.linear1.bias)

    def old_policy():
        with torch.no_grad():
            return actor._act(state, actions=acts)[2]

    def old_beta():
        return F.categorical(beta(state), actions=acts)[1]

    heads = (("policy", HIDDEN, lambda: actor.log_prob(state, acts)[0], old_policy,
              lambda: F.catalogue_log_prob(hidden, actor.linear2.weight, actor.linear2.bias, acts)[0]),
             ("beta", STATE, lambda: beta.log_prob(state, acts)[0], old_beta,
              lambda: F.catalogue_log_prob(state, beta.net[0].weight, beta.net[0].bias, acts)[0]))
    for dtype in ("fp32", "bf16"):
        F.set_catalogue_dtype(dtype)
        for name, K, fused, old, head in heads:
            Kp = (K + 127) // 128 * 128 if dtype == "bf16" else (K + 63) // 64 * 64
            fused_us, n_f = device_us(fused, window)
            old_us, n_o = device_us(old, window)
            again_us, _ = device_us(fused, window)
            head_us, n_h = device_us(head, window)
            new_lp, old_lp = fused().float(), old().float()
            free = old_lp > -15.0
            diff = (new_lp - old_lp)[free].abs().max().item() if bool(free.any()) else float("nan")
            flop = 2.0 * B * N * Kp
            t_flop = flop / (PEAK_TFLOPS[dtype] * 1e12) * 1e6
            t_bytes = N * Kp * (2 if dtype == "bf16" else 4) / (HBM_TBS * 1e12) * 1e6
            out["cases"].append({
                "head": name, "dtype": dtype, "K": K, "K_padded": Kp,
                "fused_us": round(fused_us, 1), "fused_again_us": round(again_us, 1), "materialise_us": round(old_us, 1),
                "head_only_us": round(head_us, 1), "iters": [n_f, n_o, n_h],
                "materialise_over_fused": round(old_us / fused_us, 3),
                "fused_peak_bytes": peak_rise(fused), "materialise_peak_bytes": peak_rise(old),
                "head_tflops": round(flop / head_us / 1e6, 1), "mfma_share": round(flop / head_us / 1e6 / PEAK_TFLOPS[dtype], 4),
                "floor_us": round(max(t_flop, t_bytes), 1), "floor_from": "mfma" if t_flop >= t_bytes else "hbm",
                "rows_unclamped": int(free.sum()), "max_abs_diff": diff})
            print(json.dumps(out["cases"][-1]), file=sys.stderr, flush=True)
    F.set_catalogue_dtype("fp32")
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
