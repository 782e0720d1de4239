#!/usr/bin/env python3
"""The transformer state encoder (csrc/block.hip): `transformer_encode` / `transformer_encode_train` at the reference
SeqEnv's shape (E = 128, H = 256, 4 heads, T = 1000 steps, L = 2 blocks) for F = 256 and 1024, U = 25 and 256 users, with no window
and with window = 200, against the eager fp32 route of the same model, timed in the same run on the same GPU:

  eager_*   gather [U, T, 129] from the table, F.linear, then per block F.layer_norm, F.linear, scaled_dot_product_attention under an
            explicit additive mask (causal, window, ALiBi; built once, outside the timed region), F.linear, the residual,
            F.layer_norm, F.linear, relu, F.linear, the residual; F.layer_norm at the end -- and its autograd backward.

What is timed: the encode; forward + backward of the loss (h * g).sum() for a fixed random g (h.sum() has no gradient to speak of below
a LayerNorm); the latter with `train_table=True`.  Every figure is the median of 5
device-event windows of back-to-back calls after one warm-up call (the method of tools/attn_bench.py), in milliseconds per call,
allocations included.  Also the peak of torch's allocator over one forward + backward of each route, and max |hip - eager| over h and
per gradient, relative to max |eager|.
usage: python tools/transformer_bench.py [--quick] [--window-s 0.3] [--activation relu|gelu] [--only-hip U] [--out profiles/transformer_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402

from attn_bench import E, H, HEADS, additive_mask, device_ms, make_case  # noqa: E402

LAYERS = 2


def eager(enc, table, idx, rts, mask):
    U, T = idx.shape
    d = H // HEADS
    x = enc.embed(torch.cat([table[idx], rts[..., None]], 2))
    for blk in enc.layers:
        sa = blk.self_attn
        n = TF.layer_norm(x, (H,), blk.norm1.weight, blk.norm1.bias, enc.eps)
        q, k, v = (t.reshape(U, T, HEADS, d).transpose(1, 2) for t in TF.linear(n, sa.in_proj_weight, sa.in_proj_bias).split(H, 2))
        o = TF.scaled_dot_product_attention(q, k, v, attn_mask=mask)
        x = x + sa.out_proj(o.transpose(1, 2).reshape(U, T, H))
        n = TF.layer_norm(x, (H,), blk.norm2.weight, blk.norm2.bias, enc.eps)
        x = x + blk.linear2((torch.relu if enc.activation == "relu" else TF.gelu)(blk.linear1(n)))
    return TF.layer_norm(x, (H,), enc.norm.weight, enc.norm.bias, enc.eps)


def case(U, T, F_, window, window_s, dev, yardstick=True, act="relu"):
    from recnn_amd.nn import TransformerStateEncoder
    from recnn_amd.nn import functional as F
    store, table, slots, idx, rts = make_case(U, T, dev)
    torch.manual_seed(0)
    enc = TransformerStateEncoder(E + 1, H, HEADS, num_layers=LAYERS, dim_feedforward=F_, activation=act, window=window, alibi=True).to(dev)
    P = table.clone().requires_grad_(True)
    res = {"U": U, "T": T, "E": E, "H": H, "heads": HEADS, "L": LAYERS, "F": F_, "activation": act, "window": window}
    g = torch.randn(U, T, H, device=dev, generator=torch.Generator(dev).manual_seed(1))
    keep = {}

    def step(route, fwd, tbl):
        enc.zero_grad(set_to_none=True)
        P.grad = None
        (fwd(tbl) * g).sum().backward()
        keep[route] = {n: p.grad for n, p in enc.named_parameters()}
        keep[route]["table"] = P.grad

    def peak_mb(fn):
        keep.clear()
        enc.zero_grad(set_to_none=True)
        P.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    hip_train = lambda tbl: F.transformer_encode_train(enc, store, tbl, slots, T, train_table=tbl.requires_grad)
    res["hip_fwd_ms"] = device_ms(lambda: keep.__setitem__("h", F.transformer_encode(enc, store, table, slots, T)), window_s)
    res["hip_fwd_bwd_ms"] = device_ms(lambda: step("hip", hip_train, table), window_s)
    res["hip_fwd_bwd_table_ms"] = device_ms(lambda: step("hip", hip_train, P), window_s)
    h_hip, g_hip = keep["h"], keep["hip"]
    res["hip_fwd_peak_mb"] = peak_mb(lambda: F.transformer_encode(enc, store, table, slots, T))
    res["hip_fwd_bwd_table_peak_mb"] = peak_mb(lambda: step("hip", hip_train, P))
    if not yardstick:
        return res
    mask = additive_mask(T, window, dev)
    eager_fwd = lambda tbl: eager(enc, tbl, idx, rts, mask)
    with torch.no_grad():
        res["eager_fwd_ms"] = device_ms(lambda: keep.__setitem__("he", eager_fwd(table)), window_s)
    res["eager_fwd_bwd_ms"] = device_ms(lambda: step("eager", eager_fwd, table), window_s)
    res["eager_fwd_bwd_table_ms"] = device_ms(lambda: step("eager", eager_fwd, P), window_s)
    res["max_rel_diff_h"] = float((h_hip - keep["he"]).abs().max() / keep["he"].abs().max())
    res["max_rel_diff_grads"] = {n: float((g_hip[n] - ge).abs().max() / ge.abs().max()) for n, ge in keep["eager"].items()}
    with torch.no_grad():
        res["eager_fwd_peak_mb"] = peak_mb(lambda: eager_fwd(table))
    res["eager_fwd_bwd_table_peak_mb"] = peak_mb(lambda: step("eager", eager_fwd, P))
    for k in ("fwd", "fwd_bwd", "fwd_bwd_table"):
        res[f"eager_over_hip_{k}"] = res[f"eager_{k}_ms"] / res[f"hip_{k}_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="T = 100 instead of 1000")
    ap.add_argument("--window-s", type=float, default=0.3, help="length of one timing window in seconds")
    ap.add_argument("--only-hip", type=int, default=None, metavar="U",
                    help="a few calls of the HIP encoder at this U, F = 1024, no window, and nothing else (for a kernel trace)")
    ap.add_argument("--activation", default="relu", choices=("relu", "gelu"),
                    help="gelu has no kink: the two fp32 routes then agree in every gradient (with relu a pre-activation within rounding "
                         "of 0 has its mask flipped between them, which moves the gradients below it)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    T = 100 if a.quick else 1000
    if a.only_hip is not None:
        print(json.dumps(case(a.only_hip, T, 1024, None, 0.05, dev, yardstick=False)))
        return
    res = {"tool": "transformer_bench", "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "torch": torch.__version__,
           "cases": [case(U, T, F_, w, a.window_s, dev, act=a.activation) for U in (25, 256) for F_ in (256, 1024) for w in (None, 200)]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
