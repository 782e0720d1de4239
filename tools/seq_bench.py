#!/usr/bin/env python3
"""LSTM state encoder over whole user histories (csrc/lstm.hip, csrc/seq_chain.h): `recnn_amd.nn.functional.lstm_encode` against `torch.nn.LSTM`
on the same GPU, at the reference SeqEnv's defaults (U = 25 users, H = 256, E = 128, T = 1000 steps) and at U = 256.
  hip_fused_ms / hip_chunked_ms   one lstm_encode call (every launch of it), input projection fused into the step / projected per
                                  chunk of steps by a grid-wide launch; both gather the item rows through the replay store
  torch_ms                        torch.nn.LSTM(E + 1, H, batch_first=True) on the already MATERIALISED [U, T, E + 1] input (building
                                  that input is not timed: the comparison favours the eager route)
Device-event times around the whole Python call, median of `--repeats` calls after one warm-up call: the HIP figures include the call's
host work (a pageable upload of the slots, the workspace and the three output allocations), microseconds against tens of milliseconds.
Also reports max |hip - torch| over h.  Prints one JSON line.
  --backward   training instead (csrc/seq_bwd.h): `lstm_encode_train` forward + backward of the loss h.sum() (every
               step live) against torch.nn.LSTM forward + backward of the same loss, the training forward alone against the inference
               encode, and max |hip - torch| relative to max |torch| per weight gradient.  Same shapes, same timing method.
  --backward --table-grad   the embedding table trained as well: `lstm_encode_train(..., train_table=True)` forward +
               backward with `table.requires_grad` against the same call with the table frozen, and against eager torch.nn.LSTM
               over `table[idx]` with `table.requires_grad` on the same GPU (here the gather IS timed: it is part of the graph);
               max |hip - torch| of the table gradient relative to max |torch|, and how many table rows the batch touches.
               Default --out: profiles/seq_table_grad_bench.json.
  --cell gru   the same columns for the GRU encoder (csrc/gru.hip): `gru_encode` / `gru_encode_train` against
               torch.nn.GRU on the same GPU.  --cell both runs the LSTM and the GRU in one invocation and also prints, per case, the
               GRU's times beside the LSTM's ("gru_beside_lstm": every *_ms column as [gru, lstm, gru / lstm]).
usage: python tools/seq_bench.py [--quick] [--repeats 5] [--cell lstm|gru|both] [--backward [--table-grad]] [--out profiles/seq_bench.json]"""
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


def cell_of(name):
    """(torch module class, inference encode, training encode) of the cell `name`."""
    from recnn_amd.nn import functional as F
    return {"lstm": (torch.nn.LSTM, F.lstm_encode, F.lstm_encode_train), "gru": (torch.nn.GRU, F.gru_encode, F.gru_encode_train)}[name]


def case(U, T, E, H, repeats, dev, backward=False, table_grad=False, cell="lstm"):
    from recnn_amd.data.store import ReplayStore
    from recnn_amd.nn import functional as F
    module, encode, encode_train = cell_of(cell)
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
    lstm = module(E + 1, H, batch_first=True).to(dev)
    slots = np.arange(U, dtype=np.int32)
    idx = torch.from_numpy(np.stack([items[off[u]:off[u] + T] for u in range(U)]).astype(np.int64)).to(dev)
    rts = torch.from_numpy(np.stack([ratings[off[u]:off[u] + T] for u in range(U)])).to(dev)
    x = torch.cat([table[idx], rts[..., None]], 2).contiguous()
    res = {"U": U, "T": T, "E": E, "H": H}
    out = {}
    if table_grad:
        return table_grad_case(res, lstm, store, table, slots, idx, rts, T, repeats, encode_train)
    if backward:
        return backward_case(res, lstm, store, table, slots, x, T, repeats, encode, encode_train)
    for variant in ("fused", "chunked"):
        F.set_lstm_variant(variant)
        res[f"hip_{variant}_ms"] = median_ms(lambda: out.__setitem__(variant, encode(lstm, store, table, slots, T)[0]), repeats)
    F.set_lstm_variant("chunked")
    with torch.no_grad():
        res["torch_ms"] = median_ms(lambda: out.__setitem__("torch", lstm(x)[0]), repeats)
    res["max_abs_diff_vs_torch"] = float((out["chunked"] - out["torch"]).abs().max())
    res["variants_bit_equal"] = bool(torch.equal(out["fused"], out["chunked"]))
    best = min(res["hip_fused_ms"], res["hip_chunked_ms"])
    res["torch_over_hip"] = res["torch_ms"] / best
    res["hip_us_per_step"] = 1e3 * best / T
    return res


def backward_case(res, lstm, store, table, slots, x, T, repeats, encode, encode_train):
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    grads = {}

    def hip_step():
        lstm.zero_grad(set_to_none=True)
        encode_train(lstm, store, table, slots, T)[0].sum().backward()
        grads["hip"] = [getattr(lstm, n).grad for n in names]

    def torch_step():
        lstm.zero_grad(set_to_none=True)
        lstm(x)[0].sum().backward()
        grads["torch"] = [getattr(lstm, n).grad for n in names]

    res["hip_train_fwd_bwd_ms"] = median_ms(hip_step, repeats)
    res["torch_fwd_bwd_ms"] = median_ms(torch_step, repeats)
    res["hip_train_fwd_ms"] = median_ms(lambda: encode_train(lstm, store, table, slots, T), repeats)
    res["hip_infer_fwd_ms"] = median_ms(lambda: encode(lstm, store, table, slots, T), repeats)
    with torch.no_grad():
        res["torch_fwd_ms"] = median_ms(lambda: lstm(x), repeats)
    res["hip_bwd_ms"] = res["hip_train_fwd_bwd_ms"] - res["hip_train_fwd_ms"]       # a difference of two medians
    res["torch_over_hip_fwd_bwd"] = res["torch_fwd_bwd_ms"] / res["hip_train_fwd_bwd_ms"]
    res["train_fwd_over_infer_fwd"] = res["hip_train_fwd_ms"] / res["hip_infer_fwd_ms"]
    res["hip_bwd_us_per_step"] = 1e3 * res["hip_bwd_ms"] / T
    res["grad_rel_diff_vs_torch"] = {n: float((a - b).abs().max() / b.abs().max()) for n, a, b in zip(names, grads["hip"], grads["torch"])}
    return res


def table_grad_case(res, lstm, store, table, slots, idx, rts, T, repeats, encode_train):
    P = table.clone().requires_grad_(True)
    grads = {}

    def hip_step(tbl):
        lstm.zero_grad(set_to_none=True)
        P.grad = None
        encode_train(lstm, store, tbl, slots, T, train_table=tbl.requires_grad)[0].sum().backward()
        grads["hip"] = P.grad

    def torch_step():
        lstm.zero_grad(set_to_none=True)
        P.grad = None
        lstm(torch.cat([P[idx], rts[..., None]], 2))[0].sum().backward()
        grads["torch"] = P.grad

    res["hip_fwd_bwd_table_frozen_ms"] = median_ms(lambda: hip_step(table), repeats)
    res["hip_fwd_bwd_table_grad_ms"] = median_ms(lambda: hip_step(P), repeats)
    res["torch_fwd_bwd_table_grad_ms"] = median_ms(torch_step, repeats)
    res["table_grad_added_ms"] = res["hip_fwd_bwd_table_grad_ms"] - res["hip_fwd_bwd_table_frozen_ms"]   # a difference of two medians
    res["table_grad_added_fraction"] = res["table_grad_added_ms"] / res["hip_fwd_bwd_table_frozen_ms"]
    res["torch_over_hip_fwd_bwd_table_grad"] = res["torch_fwd_bwd_table_grad_ms"] / res["hip_fwd_bwd_table_grad_ms"]
    res["table_grad_rel_diff_vs_torch"] = float((grads["hip"] - grads["torch"]).abs().max() / grads["torch"].abs().max())
    res["table_rows_touched"] = int((grads["hip"].abs().amax(1) > 0).sum())
    res["n_items"] = int(table.shape[0])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="T = 100 instead of 1000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--backward", action="store_true", help="time the training forward + backward (DESIGN.md 15)")
    ap.add_argument("--table-grad", action="store_true", help="with --backward: train the embedding table as well (DESIGN.md 18)")
    ap.add_argument("--cell", choices=("lstm", "gru", "both"), default="lstm", help="the encoder's cell (DESIGN.md 19)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.table_grad and not a.backward:
        ap.error("--table-grad goes with --backward")
    if a.table_grad and a.out is None:
        a.out = os.path.join(ROOT, "profiles", "seq_table_grad_bench.json")
    dev = torch.device("cuda")
    T = 100 if a.quick else 1000
    tool = "seq_bench --backward --table-grad" if a.table_grad else "seq_bench --backward" if a.backward else "seq_bench"
    if a.cell != "lstm":
        tool += f" --cell {a.cell}"
    run = lambda cell: [case(U, T, 128, 256, a.repeats, dev, a.backward, a.table_grad, cell) for U in (25, 256)]
    res = {"tool": tool, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName,      # (the marketing name may read generic; the arch does not)
           "lib": os.environ.get("RECNN_HIP_LIB", "in-tree"), "cases": run("gru" if a.cell == "gru" else "lstm")}
    if a.cell == "both":
        res["gru_cases"] = run("gru")
        res["gru_beside_lstm"] = [dict({k: g[k] for k in ("U", "T", "E", "H")},
                                       **{k: [g[k], l[k], g[k] / l[k]] for k in g if k.endswith("_ms")})
                                  for g, l in zip(res["gru_cases"], res["cases"])]
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
