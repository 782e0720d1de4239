#!/usr/bin/env python3
"""LSTM state encoder over whole user histories (csrc/seq.hip): `recnn_amd.nn.functional.lstm_encode` against `torch.nn.LSTM`
on the same GPU, at the reference SeqEnv's defaults (U = 25 users, H = 256, E = 128, T = 1000 steps) and at U = 256.
  hip_fused_ms / hip_chunked_ms   one lstm_encode call (every launch of it), input projection fused into the step / projected per
                                  chunk of steps by a grid-wide launch; both gather the item rows through the replay store
  torch_ms                        torch.nn.LSTM(E + 1, H, batch_first=True) on the already MATERIALISED [U, T, E + 1] input (building
                                  that input is not timed: the comparison favours the eager route)
Device-event times around the whole Python call, median of `--repeats` calls after one warm-up call: the HIP figures include the call's
host work (a pageable upload of the slots, the workspace and the three output allocations), microseconds against tens of milliseconds.
Also reports max |hip - torch| over h.  Prints one JSON line.
usage: python tools/seq_bench.py [--quick] [--repeats 5] [--out profiles/seq_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def median_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return float(np.median(times))


def case(U, T, E, H, repeats, dev):
    from recnn_amd.data.store import ReplayStore
    from recnn_amd.nn import functional as F
    rng = np.random.default_rng(U)
    n_items = 26744
    lens = rng.integers(T + 1, T + 50, size=U)
    off = np.zeros(U + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    items = rng.integers(0, n_items, size=int(off[-1])).astype(np.int32)
    ratings = (2.0 * (rng.integers(1, 11, size=int(off[-1])) * 0.5 - 2.5)).astype(np.float32)
    store = ReplayStore.from_arrays(items, ratings, off, dev)
    table = torch.from_numpy(rng.standard_normal((n_items, E)).astype(np.float32)).to(dev)
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(E + 1, H, batch_first=True).to(dev)
    slots = np.arange(U, dtype=np.int32)
    idx = torch.from_numpy(np.stack([items[off[u]:off[u] + T] for u in range(U)]).astype(np.int64)).to(dev)
    rts = torch.from_numpy(np.stack([ratings[off[u]:off[u] + T] for u in range(U)])).to(dev)
    x = torch.cat([table[idx], rts[..., None]], 2).contiguous()
    res = {"U": U, "T": T, "E": E, "H": H}
    out = {}
    for variant in ("fused", "chunked"):
        F.set_lstm_variant(variant)
        res[f"hip_{variant}_ms"] = median_ms(lambda: out.__setitem__(variant, F.lstm_encode(lstm, store, table, slots, T)[0]), repeats)
    F.set_lstm_variant("chunked")
    with torch.no_grad():
        res["torch_ms"] = median_ms(lambda: out.__setitem__("torch", lstm(x)[0]), repeats)
    res["max_abs_diff_vs_torch"] = float((out["chunked"] - out["torch"]).abs().max())
    res["variants_bit_equal"] = bool(torch.equal(out["fused"], out["chunked"]))
    best = min(res["hip_fused_ms"], res["hip_chunked_ms"])
    res["torch_over_hip"] = res["torch_ms"] / best
    res["hip_us_per_step"] = 1e3 * best / T
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="T = 100 instead of 1000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    T = 100 if a.quick else 1000
    res = {"tool": "seq_bench", "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName,      # (the marketing name may read generic; the arch does not)
           "lib": os.environ.get("RECNN_HIP_LIB", "in-tree"), "cases": [case(U, T, 128, 256, a.repeats, dev) for U in (25, 256)]}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
