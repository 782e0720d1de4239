#!/usr/bin/env python3
"""Ranking under scipy's metrics (csrc/rank.hip): `FlatIndex(table, metric).search(actions, k=10)` for every metric at
B in {1, 50, 2048} actions x N in {26,744, 100,000} items.  Device-event timing after warm-up.  Reported per case: microseconds
per call (and of the [B, N] matrix launch alone), pair-elements per second (B * N * 128 / time), the share of the metric's VALU issue floor (DESIGN.md section 11:
VALU slots per pair-element from the inner loop's instruction count, over 1024 SIMDs x 2.4 GHz x 16 lanes per clock), and an
eager-torch baseline on the same GPU: torch.cdist(q, t, p) + topk for the p-norm metrics, normalised rows + one matmul for
cosine / correlation, and a chunked broadcast restatement for canberra / braycurtis.  For context, scipy's per-item loop of the
reference for one action at N = 26,744 on the host.  Kernel times: a separate
`rocprofv3 --kernel-trace --stats -- python tools/rank_bench.py --quick` run.
Prints one JSON object per case, then a markdown table.
usage: python tools/rank_bench.py [--quick] [--no-torch] [--no-scipy]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

E = 128
CASES = [("sqeuclidean", None), ("euclidean", None), ("cityblock", None), ("chebyshev", None), ("minkowski", 3.0),
         ("canberra", None), ("braycurtis", None), ("cosine", None), ("correlation", None)]
# VALU issue slots per pair-element (one slot = one 64-lane f32 instruction at 4 cycles; packed add / mul / fma do two
# elements per slot; transcendentals take two slots): DESIGN.md section 11
SLOTS = {"sqeuclidean": 1.0, "euclidean": 1.0, "cityblock": 1.5, "chebyshev": 1.5, "minkowski": 5.5, "canberra": 7.0,
         "braycurtis": 3.0, "cosine": 0.5, "correlation": 0.5}
LANE_OPS_PER_S = 1024 * 2.4e9 * 16          # SIMDs x clock x lanes per clock of one unpacked f32 VALU stream


def timed(fn, budget_s=0.3, max_iters=200):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    est = time.perf_counter() - t
    iters = int(max(3, min(max_iters, budget_s / max(est, 1e-6))))
    for _ in range(min(iters, 5)):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters        # microseconds per call


def torch_rank(q, t, metric, p, k):
    """Eager restatement of the same ranking on the GPU (distances ascending, first k)."""
    if metric in ("sqeuclidean", "euclidean", "cityblock", "chebyshev", "minkowski"):
        pp = {"cityblock": 1.0, "chebyshev": math.inf, "minkowski": p}.get(metric, 2.0)
        return torch.topk(torch.cdist(q, t, p=pp), k, dim=1, largest=False)
    if metric in ("cosine", "correlation"):
        if metric == "correlation":
            q, t = q - q.mean(1, keepdim=True), t - t.mean(1, keepdim=True)
        c = torch.nn.functional.normalize(q, dim=1) @ torch.nn.functional.normalize(t, dim=1).T
        return torch.topk(1.0 - c.clamp(-1.0, 1.0), k, dim=1, largest=False)
    out = torch.empty(q.shape[0], t.shape[0], device=q.device)
    step = max(1, (256 << 20) // (q.shape[0] * E * 4))
    for c0 in range(0, t.shape[0], step):
        a, b = q[:, None, :], t[None, c0:c0 + step, :]
        if metric == "canberra":
            den = a.abs() + b.abs()
            out[:, c0:c0 + step] = torch.where(den > 0, (a - b).abs() / den, torch.zeros_like(den)).sum(-1)
        else:
            out[:, c0:c0 + step] = (a - b).abs().sum(-1) / (a + b).abs().sum(-1)
    return torch.topk(out, k, dim=1, largest=False)


def cdist_into(q, t, metric, p, aux, out):
    """recnn_dist_matrix into a preallocated [B, N] (the scoring loop with the store epilogue)."""
    import ctypes as C
    from recnn_amd import _lib as L
    from recnn_amd.retrieval import DIST_METRICS, minkowski_p
    ws = L.workspace("recnn_dist_workspace_bytes", q.shape[0], t.shape[0], DIST_METRICS[metric], 0, device=q.device)
    L.call("recnn_dist_matrix", L.ptr(q), q.stride(0), q.shape[0], L.ptr(t), t.shape[0], t.shape[1], DIST_METRICS[metric],
           C.c_double(minkowski_p(metric, p)), L.ptr(aux), L.ptr(out), t.shape[0], L.ptr(ws), L.current_stream())


def scipy_loop_us(table, action, metric, p):
    """The reference's `rank`: one scipy call per item, sorted, first 10 (host)."""
    from scipy.spatial import distance
    fn = getattr(distance, metric)
    kw = {} if p is None else {"p": p}
    t0 = time.perf_counter()
    scores = [[i, fn(table[i], action, **kw)] for i in range(table.shape[0])]
    sorted(scores, key=lambda x: x[1])[:10]
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="B = 2048, N = 26,744 only")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    from recnn_amd.retrieval import FlatIndex
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    tables = {n: torch.randn(n, E, generator=gen).to(dev) for n in (26744, 100000)}
    actions = (torch.randn(2048, E, generator=gen) * 0.7).to(dev)
    shapes = [(2048, 26744)] if a.quick else [(b, n) for b in (1, 50, 2048) for n in (26744, 100000)]
    rows = []
    for metric, p in CASES:
        for B, N in shapes:
            idx = FlatIndex(tables[N], metric, p)
            q = actions[:B]
            us = timed(lambda: idx.search(q, 10))
            out = torch.empty(B, N, device=dev)
            matrix_us = timed(lambda: cdist_into(q, tables[N], metric, p, idx.aux, out))
            elems = B * N * E
            floor_us = elems * SLOTS[metric] / LANE_OPS_PER_S * 1e6
            r = {"metric": metric if p is None else f"{metric}(p={p:g})", "B": B, "N": N, "us": round(us, 2),
                 "pair_elem_per_s": float(f"{elems / us * 1e6:.4g}"), "floor_us": round(floor_us, 2),
                 "share_of_floor": round(floor_us / us, 3), "matrix_us": round(matrix_us, 2)}
            if not a.no_torch:
                r["torch_us"] = round(timed(lambda: torch_rank(q, tables[N], metric, p, 10), budget_s=0.5), 2)
                r["speedup"] = round(r["torch_us"] / us, 2)
            if not a.no_scipy and B == 1 and N == 26744:
                try:
                    r["scipy_loop_us"] = round(scipy_loop_us(tables[N].cpu().double().numpy(),
                                                             q[0].cpu().double().numpy(), metric, p), 0)
                except ImportError:
                    pass
            print(json.dumps(r), flush=True)
            rows.append(r)
    print("\n| metric | B | N | search us | matrix us | pair-elem/s | floor us | share of floor | torch us | speedup | scipy loop us |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        print(f"| {r['metric']} | {r['B']} | {r['N']} | {r['us']} | {r['matrix_us']} | {r['pair_elem_per_s']:.3g} | {r['floor_us']} | "
              f"{r['share_of_floor']} | {r.get('torch_us', '')} | {r.get('speedup', '')} | {r.get('scipy_loop_us', '')} |")


if __name__ == "__main__":
    main()
