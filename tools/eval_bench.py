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
`--seen` adds to each row the same `rank_of` and `search(k=10)` calls with a per-row exclusion mask: one list
per query row, its length drawn like the synthetic store's histories (clip(round(lognormal(4.22, 1.22)), 20, 9254)),
its ids uniform over the catalogue, all lists slices of one id array.  `mask_build_us` is `SeenItems.mask` alone (the cache
emptied before each call), `*_excl_us` the call with the mask already built (what a second call on the same batch costs),
`rank_of_excl_first_us` the first call (build + rank).  Every ratio is against the plain call of the same row in the same run.
With `--seen` the default output is profiles/eval_bench_seen.json.
usage: python tools/eval_bench.py [--quick] [--seen] [--out profiles/eval_bench.json]"""
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
    ap.add_argument("--seen", action="store_true", help="also time rank_of / search with a per-row exclusion mask")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "eval_bench_seen.json" if a.seen else "eval_bench.json")
    if not torch.cuda.is_available():
        sys.exit("eval_bench.py measures on the GPU and none is visible")
    import recnn_amd
    from recnn_amd.retrieval import FlatIndex, RankingMeter, SeenItems, cdist
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
        if a.seen:
            import numpy as np
            rng = np.random.default_rng(0)
            lens = np.clip(np.round(rng.lognormal(4.22, 1.22, size=B)), 20, 9254).astype(np.int64)
            starts = np.cumsum(lens) - lens
            seen = SeenItems(torch.from_numpy(rng.integers(0, N, size=int(lens.sum())).astype(np.int32)).to(dev),
                             torch.from_numpy(starts), torch.from_numpy(lens), keep=targets)

            def build_mask():
                seen._masks.clear()
                return seen.mask(N)

            mask_us, n_b = device_us(build_mask, window)
            excluded = int(sum(bin(w & (2 ** 64 - 1)).count("1") for w in seen.mask(N).words.flatten().tolist()))
            out.setdefault("seen", []).append({"B": B, "ids": int(lens.sum()), "longest": int(lens.max()),
                                               "excluded_bits": excluded, "mask_bytes": 8 * seen.mask(N).words.numel(),
                                               "mask_build_us": round(mask_us, 2), "iters": n_b})
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
            if a.seen:
                def first_call():
                    seen._masks.clear()
                    return idx.rank_of(q, targets, exclude=seen)

                first_us, n_f = device_us(first_call, window)
                rank_x_us, n_rx = device_us(lambda: idx.rank_of(q, targets, exclude=seen), window)
                search_x_us, n_sx = device_us(lambda: idx.search(q, 10, exclude=seen), window)
                # the plain calls again, after the excluding ones: the spread of the baseline within this run
                rank2_us, _ = device_us(lambda: idx.rank_of(q, targets), window)
                search2_us, _ = device_us(lambda: idx.search(q, 10), window)
                assert (idx.rank_of(q, targets, exclude=seen) <= idx.rank_of(q, targets)).all()
                out["cases"][-1].update({"rank_of_excl_us": round(rank_x_us, 2), "rank_of_excl_first_us": round(first_us, 2),
                                         "search_k10_excl_us": round(search_x_us, 2), "rank_of_again_us": round(rank2_us, 2),
                                         "search_k10_again_us": round(search2_us, 2),
                                         "rank_excl_over_rank": round(rank_x_us / rank_us, 3),
                                         "search_excl_over_search": round(search_x_us / search_us, 3),
                                         "iters_excl": [n_f, n_rx, n_sx]})
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
