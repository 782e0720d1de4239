#!/usr/bin/env python3
"""Offline ranking evaluation (csrc/rank.hip, csrc/topk.hip, csrc/evalrank.hip): `FlatIndex.rank_of` at
N = 26,744 items (the ML-20M catalogue), B = 2048 and B = 25 actions, under L2, IP and one VALU metric (cityblock), each timed beside
two yardsticks on the same inputs in the same run:
  search_us       `FlatIndex.search(k=10)`: the top-K selection the rank replaces when the question is "where is the target";
  materialise_us  the [B, N] matrix and torch comparisons: `cdist` for cityblock, `torch.matmul` for IP / L2, then
                  `((d < d_t) | ((d == d_t) & (id < g))).sum(1)`;
and the full evaluation loop `policy(state) -> rank_of -> RankingMeter.update` (an Actor of the benchmark's shape, L2).
Every figure is the median of 5 device-event windows of back-to-back calls after one warm-up call, in microseconds per call.
`agree` is the share of rows on which the materialising route gives the same rank (1.0 for cityblock, whose matrix is bit-equal;
torch.matmul rounds differently, so near-ties may swap).  Kernel times: a separate
`rocprofv3 --kernel-trace --stats -- python tools/eval_bench.py --quick` run.
Prints one JSON object and writes it to profiles/eval_bench.json.
usage: python tools/eval_bench.py [--quick] [--out profiles/eval_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

E, N, FRAME = 128, 26744, 10


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


def rank_from_matrix(key, targets, larger_is_better):
    ids = torch.arange(key.shape[1], device=key.device)[None, :]
    g = targets[:, None]
    kt = key.gather(1, g)
    first = key > kt if larger_is_better else key < kt
    return (first | ((key == kt) & (ids < g))).sum(1).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="B = 2048 only, short windows (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_bench.py measures on the GPU and none is visible")
    import recnn_amd
    from recnn_amd.retrieval import FlatIndex, RankingMeter, cdist
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    table = torch.randn(N, E, generator=gen).to(dev)
    norms = (table * table).sum(1)
    window = 0.02 if a.quick else 0.1
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "eval_bench", "n_items": N, "device": torch.cuda.get_device_name(0),
           "arch": getattr(props, "gcnArchName", "unknown"), "window_s": window, "cases": [], "loop": []}
    index = {m: FlatIndex(table, m) for m in ("L2", "IP", "cityblock")}
    actor = recnn_amd.nn.Actor(FRAME * (E + 1), E, 256).to(dev).eval()

    def matrix_route(metric, q, targets):
        if metric == "cityblock":
            return rank_from_matrix(cdist(q, table, "cityblock"), targets, False)
        s = torch.matmul(q, table.T)
        return rank_from_matrix(s if metric == "IP" else 2.0 * s - norms[None, :], targets, True)

    for B in ((2048,) if a.quick else (2048, 25)):
        q = (torch.randn(B, E, generator=gen) * 0.7).to(dev)
        targets = torch.randint(0, N, (B,), generator=gen).to(dev)
        for metric in ("L2", "IP", "cityblock"):
            idx = index[metric]
            rank_us, n_r = device_us(lambda: idx.rank_of(q, targets), window)
            search_us, n_s = device_us(lambda: idx.search(q, 10), window)
            mat_us, n_m = device_us(lambda: matrix_route(metric, q, targets), window)
            agree = (idx.rank_of(q, targets) == matrix_route(metric, q, targets)).float().mean().item()
            if metric == "cityblock":
                assert agree == 1.0, "rank_of and the cdist matrix disagree"
            out["cases"].append({"metric": metric, "B": B, "rank_of_us": round(rank_us, 2), "search_k10_us": round(search_us, 2),
                                 "materialise_us": round(mat_us, 2), "iters": [n_r, n_s, n_m],
                                 "rank_over_search": round(rank_us / search_us, 3),
                                 "materialise_over_rank": round(mat_us / rank_us, 2), "agree": round(agree, 5),
                                 "matrix_bytes": 4 * B * N})
        state = torch.randn(B, FRAME * (E + 1), generator=gen).to(dev)
        meter = RankingMeter(ks=(1, 10, 100), device=dev)

        def loop():
            with torch.no_grad():
                meter.update(index["L2"].rank_of(actor(state), targets))

        def policy():
            with torch.no_grad():
                actor(state)

        loop_us, n_l = device_us(loop, window)
        policy_us, n_p = device_us(policy, window)
        r = index["L2"].rank_of(q, targets)
        update_us, n_u = device_us(lambda: meter.update(r), window)
        out["loop"].append({"B": B, "policy_rank_update_us": round(loop_us, 2), "policy_us": round(policy_us, 2),
                            "update_us": round(update_us, 2), "iters": [n_l, n_p, n_u]})
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
