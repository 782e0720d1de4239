#!/usr/bin/env python3
"""Serving the transformer state encoder step by step (csrc/attn_dev.h): one `transformer_append` of n = 1 at position P
of every session, at the reference SeqEnv's model (E = 128, H = 256, 4 heads, L = 2 blocks) for F = 256 and 1024, no window and
window = 200, 25 / 256 / 2048 sessions, P = 64 / 200 / 1000, against the two other routes to the same row, timed in the same run on
the same GPU:

  reencode_ms  `transformer_encode` of the P + 1 steps through a ReplayStore -- the only route without the cache;
  eager_ms     the same model in eager fp32 torch with cached keys and values: embedding of the new step, per block F.layer_norm,
               F.linear, torch.cat of the cached K / V with the new row, scaled_dot_product_attention for the one query under an
               additive bias (ALiBi; built once, outside the timed region; under a window the cached K / V hold the last w - 1
               positions), F.linear, the residual, the feed-forward, the residual; F.layer_norm at the end.

Also a prefill of 960 positions in 15 appends of 64 against one whole-history call of 960 steps (256 sessions).  Every figure is the
median of 5 device-event windows of back-to-back calls after one warm-up call (the method of tools/attn_bench.py), in milliseconds
per call, allocations and the upload of the rows' positions included.  `append_equals_reencode` is the comparison of bits;
`max_rel_diff_eager` is max |append - eager| / max |eager|.  `kv_read_mb` is what the append's attention launches read from the cache
(both blocks): the rows up to P of the key tiles the new row's block stages, [k | v] of one head each, over all sessions and heads.
usage: python tools/kv_cache_bench.py [--quick] [--window-s 0.2] [--only-append S P] [--out profiles/kv_cache_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402

from attn_bench import E, H, HEADS, device_ms, make_case  # noqa: E402
from transformer_bench import LAYERS  # noqa: E402

CHUNK = 64


def setup(S, T, F_, window, dev):
    from recnn_amd.nn import KVCache, TransformerStateEncoder
    store, table, slots, idx, rts = make_case(S, T, dev)
    torch.manual_seed(0)
    enc = TransformerStateEncoder(E + 1, H, HEADS, num_layers=LAYERS, dim_feedforward=F_, activation="relu", window=window, alibi=True).to(dev)
    cap = (T + CHUNK + 63) // 64 * 64 if window is None else KVCache.min_capacity(window, CHUNK)
    return store, table, slots, idx.to(torch.int32), rts, enc, KVCache(enc, S, cap, max_append=CHUNK)


def prefill(enc, cache, table, idx, rts, P):
    from recnn_amd.nn import functional as F
    cache.reset()
    h = None
    for at in range(0, P, CHUNK):
        h = F.transformer_append(enc, cache, table, idx[:, at:min(P, at + CHUNK)], rts[:, at:min(P, at + CHUNK)])
    return h


def eager_cache(cache, P, window):
    """Per block (K, V) [S, heads, kept, d] of the positions before P, read out of the prefilled cache (outside the timed region),
    and the additive bias of the one query at position P over the kept + 1 keys."""
    S, d, dev = cache.n_sessions, H // HEADS, cache.device
    kept = P if window is None else min(P, window - 1)
    slot = torch.arange(P - kept, P, device=dev) % cache.capacity
    out = []
    for layer in range(LAYERS):
        kv = cache.kv[layer][:, slot]
        out.append(tuple(z.reshape(S, kept, HEADS, d).transpose(1, 2).contiguous() for z in kv.split(H, 2)))
    slopes = torch.tensor([2.0 ** (-8.0 * (a + 1) / HEADS) for a in range(HEADS)], device=dev)
    bias = (-slopes[:, None] * torch.arange(kept, -1, -1, device=dev).float()[None])[None, :, None, :].contiguous()
    return out, bias


def eager_step(enc, table, item, rating, kvs, bias):
    S, d = item.shape[0], H // HEADS
    x = enc.embed(torch.cat([table[item.long()], rating[:, None]], 1))
    for blk, (Kc, Vc) in zip(enc.layers, kvs):
        sa = blk.self_attn
        n = TF.layer_norm(x, (H,), blk.norm1.weight, blk.norm1.bias, enc.eps)
        q, k, v = (z.reshape(S, HEADS, 1, d) for z in TF.linear(n, sa.in_proj_weight, sa.in_proj_bias).split(H, 1))
        o = TF.scaled_dot_product_attention(q, torch.cat([Kc, k], 2), torch.cat([Vc, v], 2), attn_mask=bias)
        x = x + sa.out_proj(o.reshape(S, H))
        n = TF.layer_norm(x, (H,), blk.norm2.weight, blk.norm2.bias, enc.eps)
        x = x + blk.linear2(torch.relu(blk.linear1(n)))
    return TF.layer_norm(x, (H,), enc.norm.weight, enc.norm.bias, enc.eps)


def staged_rows(P, window):
    """Cache rows the attention of one new row at position P reads: from the first key tile of 64 its block's window reaches to P."""
    q0 = P // 64 * 64
    lo = 0 if window is None else max(0, q0 - window + 1) // 64
    return P + 1 - 64 * lo


def case(S, P, F_, window, window_s, dev, yardstick=True):
    from recnn_amd.nn import functional as F
    store, table, slots, idx, rts, enc, cache = setup(S, P + 1, F_, window, dev)
    res = {"sessions": S, "P": P, "E": E, "H": H, "heads": HEADS, "L": LAYERS, "F": F_, "window": window, "capacity": cache.capacity}
    prefill(enc, cache, table, idx, rts, P)
    keep = {}

    def step():
        cache.lengths[:] = P
        keep["h"] = F.transformer_append(enc, cache, table, idx[:, P:P + 1], rts[:, P:P + 1])
    res["append_ms"] = device_ms(step, window_s)
    res["kv_read_mb"] = LAYERS * S * HEADS * staged_rows(P, window) * 2 * (H // HEADS) * 4 / 2 ** 20
    if not yardstick:
        return res
    res["reencode_ms"] = device_ms(lambda: keep.__setitem__("w", F.transformer_encode(enc, store, table, slots, P + 1)), window_s)
    res["append_equals_reencode"] = bool(torch.equal(keep["h"].view(torch.int32), keep["w"][:, P:].contiguous().view(torch.int32)))
    with torch.no_grad():
        kvs, bias = eager_cache(cache, P, window)
        res["eager_ms"] = device_ms(lambda: keep.__setitem__("e", eager_step(enc, table, idx[:, P], rts[:, P], kvs, bias)), window_s)
    res["max_rel_diff_eager"] = float((keep["h"][:, 0] - keep["e"]).abs().max() / keep["e"].abs().max())
    res["reencode_over_append"] = res["reencode_ms"] / res["append_ms"]
    res["eager_over_append"] = res["eager_ms"] / res["append_ms"]
    return res


def prefill_case(S, P, F_, window, window_s, dev):
    from recnn_amd.nn import functional as F
    store, table, slots, idx, rts, enc, cache = setup(S, P, F_, window, dev)
    res = {"sessions": S, "P": P, "F": F_, "window": window, "appends": (P + CHUNK - 1) // CHUNK, "n": CHUNK}
    keep = {}
    res["prefill_appends_ms"] = device_ms(lambda: keep.__setitem__("h", prefill(enc, cache, table, idx, rts, P)), window_s)
    res["whole_history_ms"] = device_ms(lambda: keep.__setitem__("w", F.transformer_encode(enc, store, table, slots, P)), window_s)
    last = P - (P - 1) // CHUNK * CHUNK
    res["last_append_equals_whole"] = bool(torch.equal(keep["h"].view(torch.int32), keep["w"][:, P - last:].contiguous().view(torch.int32)))
    res["appends_over_whole"] = res["prefill_appends_ms"] / res["whole_history_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="25 and 256 sessions, P = 64 and 200 only")
    ap.add_argument("--window-s", type=float, default=0.2, help="length of one timing window in seconds")
    ap.add_argument("--only-append", type=int, nargs=2, default=None, metavar=("S", "P"),
                    help="a few appends of n = 1 at these sessions and position, F = 1024, no window, and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    if a.only_append is not None:
        print(json.dumps(case(a.only_append[0], a.only_append[1], 1024, None, 0.02, dev, yardstick=False)))
        return
    sessions, hist = ((25, 256), (64, 200)) if a.quick else ((25, 256, 2048), (64, 200, 1000))
    res = {"tool": "kv_cache_bench", "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "torch": torch.__version__,
           "cases": [case(S, P, F_, w, a.window_s, dev) for F_ in (256, 1024) for w in (None, 200) for S in sessions for P in hist],
           "prefill": [prefill_case(256, 192 if a.quick else 960, F_, w, a.window_s, dev) for F_ in (256, 1024) for w in (None, 200)]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
