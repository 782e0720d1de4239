#!/usr/bin/env python3
"""Top-K diversity statistics (csrc/divstats.hip): what the reference's diversity / distances notebooks do with a search result,
timed three ways on the same [B, k] distances and ids, at B = 65,536 (every state of a test set) and at the notebooks' B = 50,
k = 20, N = 26,744 (the ML-20M catalogue):
  (a) stats_us:  `recnn_amd.retrieval.topk_stats` accumulating into preallocated counts / totals (two launches);
  (b) copy_us:   a device-to-device copy of the same dist + ids bytes (12 B k in, 12 B k out): the floor of any pass over them;
  (c) host_us:   the notebooks' route: `.cpu().numpy()` of both, `np.unique(ids, return_counts=True)`, `D.mean(axis=1).mean()`,
                 `D.std(axis=1).mean()` (host clock around work that starts on synchronised device data).
(a) and (b) are device-event times over enough repeats to fill the window after warm-up; (c) is a host wall time, repeated.
Kernel times: a separate `rocprofv3 --kernel-trace --stats -- python tools/diversity_bench.py --quick` run.
Prints one JSON line.
usage: python tools/diversity_bench.py [--quick] [--window-s 1.0]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

E, N, K = 128, 26744, 20


def device_us(fn, window_s, max_iters=20000):
    """Microseconds per call from device events, over about `window_s` of back-to-back calls after warm-up."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    est = (time.perf_counter() - t) / 10
    iters = int(max(20, min(max_iters, window_s / max(est, 1e-7))))
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters, iters


def host_us(fn, window_s, max_iters=2000):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    est = time.perf_counter() - t
    iters = int(max(5, min(max_iters, window_s / max(est, 1e-7))))
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t) * 1e6 / iters, iters


def notebook_route(dist, ids):
    D, topK = dist.cpu().numpy(), ids.cpu().numpy()
    uniques, counts = np.unique(topK, return_counts=True)
    return uniques, counts, D.mean(axis=1).mean(), D.std(axis=1).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="B = 65,536 only, short window (for a profiler run)")
    ap.add_argument("--window-s", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("diversity_bench.py measures on the GPU and none is visible")
    from recnn_amd.retrieval import FlatIndex, topk_stats
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    index = FlatIndex(torch.randn(N, E, generator=gen).to(dev), "L2")
    window = 0.2 if a.quick else a.window_s
    out = {"tool": "diversity_bench", "k": K, "n_items": N, "device": torch.cuda.get_device_name(0), "cases": []}
    for B in ((65536,) if a.quick else (65536, 50)):
        q = (torch.randn(B, E, generator=gen) * 0.7).to(dev)
        found = [index.search(q[r:r + 8192], K) for r in range(0, B, 8192)]
        dist, ids = torch.cat([d for d, _ in found]), torch.cat([i for _, i in found])
        counts = torch.zeros(N, dtype=torch.int32, device=dev)
        totals = torch.zeros(4, dtype=torch.float64, device=dev)
        dist2, ids2 = torch.empty_like(dist), torch.empty_like(ids)

        def copy():
            dist2.copy_(dist)
            ids2.copy_(ids)

        stats_us, n_a = device_us(lambda: topk_stats(dist, ids, N, False, counts, totals), window)
        copy_us, n_b = device_us(copy, window)
        nb_us, n_c = host_us(lambda: notebook_route(dist, ids), window)
        # the routes computed the same thing
        st = topk_stats(dist, ids, N)
        u, c, m, s = notebook_route(dist, ids)
        t = st.totals.tolist()
        assert np.array_equal(np.flatnonzero(st.counts.cpu().numpy()), u) and abs(t[0] / t[2] - m) <= 1e-4 * abs(m) \
            and abs(t[1] / t[2] - s) <= 1e-4 * abs(s)                      # the notebooks' D is float32: a sanity check only
        bytes_in = 12 * B * K
        out["cases"].append({"B": B, "stats_us": round(stats_us, 2), "copy_us": round(copy_us, 2), "host_us": round(nb_us, 1),
                             "iters": [n_a, n_b, n_c], "bytes_in": bytes_in,
                             "stats_GBps_in": round(bytes_in / stats_us * 1e-3, 1),
                             "copy_GBps_in_plus_out": round(2 * bytes_in / copy_us * 1e-3, 1),
                             "host_over_stats": round(nb_us / stats_us, 1), "stats_over_copy": round(stats_us / copy_us, 2)})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
