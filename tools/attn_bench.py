#!/usr/bin/env python3
"""The causal self-attention state encoder (csrc/attn.hip): `attn_encode` / `attn_encode_train` at the reference
SeqEnv's shape (E = 128, H = 256, 4 heads, T = 1000 steps) for U = 25 and 256 users, with no window and with window = 200, against two
yardsticks timed in the same run on the same GPU:

  eager_*   the eager route in fp32: gather [U, T, 129] from the table, F.linear, scaled_dot_product_attention under an explicit
            additive mask (causal, window, ALiBi; built once, outside the timed region), F.linear -- and its autograd backward.  Which
            SDPA backends torch has enabled is recorded, and which one a forced single-backend call accepts for these arguments.
  lstm_* / gru_*   `lstm_encode` / `gru_encode` (and `_train`) at the same U and T: what the new encoder costs beside the old ones.

What is timed: forward; forward + backward of the loss h.sum(); the latter with `train_table=True`.  Every figure is the median of 5
device-event windows of back-to-back calls after one warm-up call (the method of tools/eval_bench.py), in milliseconds per call,
allocations included.  Also reports max |hip - eager| over h and per gradient, relative to max |eager|.
usage: python tools/attn_bench.py [--quick] [--window-s 0.3] [--only-hip-train U] [--out profiles/attn_bench.json]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402

E, H, HEADS, N_ITEMS = 128, 256, 4, 26744


def device_ms(fn, window_s):
    """Median over 5 device-event windows of back-to-back calls (each about `window_s` long), after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    iters = int(max(1, min(200, window_s / max(time.perf_counter() - t, 1e-6))))
    times = []
    for _ in range(5):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) / iters)
    return statistics.median(times)


def make_case(U, T, dev):
    from recnn_amd.data.store import ReplayStore
    rng = np.random.default_rng(U)
    lens = rng.integers(T + 1, T + 50, size=U)
    off = np.zeros(U + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    items = rng.integers(0, N_ITEMS, size=int(off[-1])).astype(np.int32)
    ratings = (2.0 * (rng.integers(1, 11, size=int(off[-1])) * 0.5 - 2.5)).astype(np.float32)
    store = ReplayStore.from_arrays(items, ratings, off, dev)
    table = torch.from_numpy(rng.standard_normal((N_ITEMS, E)).astype(np.float32)).to(dev)
    idx = torch.from_numpy(np.stack([items[off[u]:off[u] + T] for u in range(U)]).astype(np.int64)).to(dev)
    rts = torch.from_numpy(np.stack([ratings[off[u]:off[u] + T] for u in range(U)])).to(dev)
    return store, table, np.arange(U, dtype=np.int32), idx, rts


def additive_mask(T, window, dev):
    t = torch.arange(T, device=dev)
    dist = (t[:, None] - t[None, :]).float()
    slopes = torch.tensor([2.0 ** (-8.0 * (a + 1) / HEADS) for a in range(HEADS)], device=dev)
    keep = (dist >= 0) if window is None else (dist >= 0) & (dist < window)
    return torch.where(keep[None], -slopes[:, None, None] * dist[None], torch.full((), -math.inf, device=dev))[None].contiguous()


def eager(enc, table, idx, rts, mask):
    U, T = idx.shape
    x = torch.cat([table[idx], rts[..., None]], 2)
    q, k, v = (t.reshape(U, T, HEADS, H // HEADS).transpose(1, 2) for t in TF.linear(x, enc.in_proj_weight, enc.in_proj_bias).split(H, 2))
    o = TF.scaled_dot_product_attention(q, k, v, attn_mask=mask)
    return enc.out_proj(o.transpose(1, 2).reshape(U, T, H))


def sdpa_backends(dev):
    """The enabled SDPA backends, and which single backend accepts fp32 q, k, v with a float additive mask at this shape."""
    out = {"flash_enabled": torch.backends.cuda.flash_sdp_enabled(), "mem_efficient_enabled": torch.backends.cuda.mem_efficient_sdp_enabled(),
           "math_enabled": torch.backends.cuda.math_sdp_enabled()}
    try:
        from torch.nn.attention import SDPBackend, sdpa_kernel
        q = torch.randn(2, HEADS, 128, H // HEADS, device=dev)
        m = additive_mask(128, None, dev)
        accepts = {}
        for name, b in (("flash", SDPBackend.FLASH_ATTENTION), ("mem_efficient", SDPBackend.EFFICIENT_ATTENTION), ("math", SDPBackend.MATH)):
            try:
                with sdpa_kernel([b]):
                    TF.scaled_dot_product_attention(q, q, q, attn_mask=m)
                torch.cuda.synchronize()
                accepts[name] = True
            except RuntimeError:
                accepts[name] = False
        out["accepts_these_arguments"] = accepts
        out["picked"] = next((n for n in ("flash", "mem_efficient", "math") if accepts[n] and out[f"{n}_enabled"]), None)   # torch's priority order
    except ImportError:
        out["picked"] = "unknown (torch.nn.attention missing)"
    return out


def case(U, T, window, window_s, dev, yardsticks=True):
    from recnn_amd.nn import AttentionEncoder
    from recnn_amd.nn import functional as F
    store, table, slots, idx, rts = make_case(U, T, dev)
    torch.manual_seed(0)
    enc = AttentionEncoder(E + 1, H, HEADS, window=window, alibi=True).to(dev)
    P = table.clone().requires_grad_(True)
    res = {"U": U, "T": T, "E": E, "H": H, "heads": HEADS, "window": window}
    keep = {}

    def hip_step(tbl):
        enc.zero_grad(set_to_none=True)
        P.grad = None
        F.attn_encode_train(enc, store, tbl, slots, T, train_table=tbl.requires_grad).sum().backward()
        keep["hip"] = {n: p.grad for n, p in enc.named_parameters()}
        keep["hip"]["table"] = P.grad

    res["hip_fwd_ms"] = device_ms(lambda: keep.__setitem__("h", F.attn_encode(enc, store, table, slots, T)), window_s)
    res["hip_fwd_bwd_ms"] = device_ms(lambda: hip_step(table), window_s)
    res["hip_fwd_bwd_table_ms"] = device_ms(lambda: hip_step(P), window_s)
    if not yardsticks:
        return res
    mask = additive_mask(T, window, dev)

    def eager_step(tbl):
        enc.zero_grad(set_to_none=True)
        P.grad = None
        eager(enc, tbl, idx, rts, mask).sum().backward()
        keep["eager"] = {n: p.grad for n, p in enc.named_parameters()}
        keep["eager"]["table"] = P.grad

    with torch.no_grad():
        res["eager_fwd_ms"] = device_ms(lambda: keep.__setitem__("he", eager(enc, table, idx, rts, mask)), window_s)
    res["eager_fwd_bwd_ms"] = device_ms(lambda: eager_step(table), window_s)
    res["eager_fwd_bwd_table_ms"] = device_ms(lambda: eager_step(P), window_s)
    res["max_rel_diff_h"] = float((keep["h"] - keep["he"]).abs().max() / keep["he"].abs().max())
    res["max_rel_diff_grads"] = {n: float((keep["hip"][n] - g).abs().max() / g.abs().max()) for n, g in keep["eager"].items()}
    for k in ("fwd", "fwd_bwd", "fwd_bwd_table"):
        res[f"eager_over_hip_{k}"] = res[f"eager_{k}_ms"] / res[f"hip_{k}_ms"]
    if window is None:                                   # the recurrent encoders do not know a window: once per U
        for name, mod, fwd, train in (("lstm", torch.nn.LSTM, F.lstm_encode, F.lstm_encode_train),
                                      ("gru", torch.nn.GRU, F.gru_encode, F.gru_encode_train)):
            torch.manual_seed(0)
            cell = mod(E + 1, H).to(dev)

            def cell_step():
                cell.zero_grad(set_to_none=True)
                train(cell, store, table, slots, T)[0].sum().backward()
            res[f"{name}_fwd_ms"] = device_ms(lambda: fwd(cell, store, table, slots, T), window_s)
            res[f"{name}_fwd_bwd_ms"] = device_ms(cell_step, window_s)
            res[f"{name}_over_attn_fwd"] = res[f"{name}_fwd_ms"] / res["hip_fwd_ms"]
            res[f"{name}_over_attn_fwd_bwd"] = res[f"{name}_fwd_bwd_ms"] / res["hip_fwd_bwd_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="T = 100 instead of 1000")
    ap.add_argument("--window-s", type=float, default=0.3, help="length of one timing window in seconds")
    ap.add_argument("--only-hip-train", type=int, default=None, metavar="U",
                    help="a few forward + backward calls of the HIP encoder at this U and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    T = 100 if a.quick else 1000
    if a.only_hip_train is not None:
        print(json.dumps(case(a.only_hip_train, T, None, 0.05, dev, yardsticks=False)))
        return
    res = {"tool": "attn_bench", "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "torch": torch.__version__, "sdpa": sdpa_backends(dev),
           "cases": [case(U, T, w, a.window_s, dev) for U in (25, 256) for w in (None, 200)]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
