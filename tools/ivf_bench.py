#!/usr/bin/env python3
"""IVF-Flat search (csrc/ivf.hip): `IVFFlatIndex.search(queries, k, nprobe)` at nprobe in {1, 4, 16, 64} beside
`FlatIndex.search(queries, k)` on the same table and queries in the same run, with the recall@k of the IVF result against the flat
one (the mean share of the flat top k that the IVF top k contains) and the mean share of the table a query's probed lists hold.
Shapes: N = 26,744 (the ML-20M catalogue, nlist = 256) and N = 100,000 (nlist = 1024), width 128, L2; B in {25, 2048}; k in {10, 64}.
Two synthetic tables per N, because recall is a property of the data:
  gaussian  i.i.d. normal rows, queries 0.7 * normal: no cluster structure at all, the worst case for an inverted file;
  mixture   N rows around 500 unit-normal centres with noise 0.3 per coordinate, queries = random table rows + noise 0.3.
`train_ms` is the wall time of the constructor (10 Lloyd iterations, the final assignment, the lists and the rows in list order),
synchronised before and after.  Every search figure is the median of 5 device-event windows of back-to-back calls after one warm-up
call, in microseconds per call from Python, allocations included (the method of tools/eval_bench.py).
Prints one JSON object and writes it to profiles/ivf_bench.json.
usage: python tools/ivf_bench.py [--quick] [--out profiles/ivf_bench.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from eval_bench import device_us  # noqa: E402

D = 128
SHAPES = ((26744, 256), (100000, 1024))
NPROBES = (1, 4, 16, 64)


def make_data(kind, N, gen):
    if kind == "gaussian":
        return torch.randn(N, D, generator=gen), lambda B: torch.randn(B, D, generator=gen) * 0.7
    centres = torch.randn(500, D, generator=gen)
    table = centres[torch.randint(0, 500, (N,), generator=gen)] + 0.3 * torch.randn(N, D, generator=gen)
    return table, lambda B: table[torch.randint(0, N, (B,), generator=gen)] + 0.3 * torch.randn(B, D, generator=gen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="N = 26,744, the mixture table and B = 25 only, short windows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ivf_bench.py measures on the GPU and none is visible")
    from recnn_amd.retrieval import FlatIndex, IVFFlatIndex
    dev = torch.device("cuda")
    window = 0.02 if a.quick else 0.05
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "ivf_bench", "dim": D, "metric": "L2", "niter": 10, "device": torch.cuda.get_device_name(0),
           "arch": getattr(props, "gcnArchName", "unknown"), "window_s": window, "cases": []}
    IVFFlatIndex(torch.randn(2000, D).to(dev), 8, niter=1).search(torch.randn(4, D).to(dev), 4, 2)     # loads the library
    for N, nlist in (SHAPES[:1] if a.quick else SHAPES):
        for kind in (("mixture",) if a.quick else ("gaussian", "mixture")):
            gen = torch.Generator().manual_seed(0)
            table, make_queries = make_data(kind, N, gen)
            table = table.to(dev)
            flat = FlatIndex(table, "L2")
            torch.cuda.synchronize()
            t = time.perf_counter()
            ivf = IVFFlatIndex(table, nlist, "L2", niter=10, seed=0)
            torch.cuda.synchronize()
            train_ms = (time.perf_counter() - t) * 1e3
            sizes = (ivf.list_start[1:] - ivf.list_start[:-1]).to(torch.float32)
            case = {"n_items": N, "nlist": nlist, "data": kind, "train_ms": round(train_ms, 1), "empty_lists": int((sizes == 0).sum()),
                    "longest_list": int(sizes.max()), "searches": []}
            for B in ((25,) if a.quick else (25, 2048)):
                q = make_queries(B).to(dev)
                for k in (10, 64):
                    flat_us, n_f = device_us(lambda: flat.search(q, k), window)
                    want = flat.search(q, k)[1]
                    row = {"B": B, "k": k, "flat_us": round(flat_us, 1), "flat_iters": n_f, "ivf": []}
                    for nprobe in NPROBES:
                        us, n_i = device_us(lambda: ivf.search(q, k, nprobe), window)
                        got = ivf.search(q, k, nprobe)[1]
                        recall = ((got[:, :, None] == want[:, None, :]) & (got[:, :, None] >= 0)).any(2).float().mean().item()
                        scored = sizes[ivf.probe(q, nprobe)[1]].sum(1).mean().item() / N
                        row["ivf"].append({"nprobe": nprobe, "us": round(us, 1), "iters": n_i, "flat_over_ivf": round(flat_us / us, 2),
                                           "recall": round(recall, 4), "share_scored": round(scored, 4)})
                    case["searches"].append(row)
            out["cases"].append(case)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
