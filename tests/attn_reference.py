"""Host restatement of the causal self-attention state encoder (test infrastructure, not an oracle file): the layer of
recnn_amd.nn.AttentionEncoder written out in plain torch on the CPU, in float64 and float32, over the materialised [U, T, E + 1] inputs
of tests/seq_reference.py (`lstm_inputs`), its autograd gradients, and the bounds every attention test uses:

  forward    max(4 max |h32cpu - h64cpu|, 1e-6)                                             (the rule of tests/test_gpu_seq.py)
  gradients  per tensor G: max(4 max |G32cpu - G64cpu|, 2^-23 max(8, sqrt(U T)) max |G64|)  (seq_grad_reference.grad_bounds)

tests/test_attn_cpu.py pins `attn_cpu` in float64 to torch's scaled_dot_product_attention under an explicit additive mask."""
import math

import numpy as np
import torch

PARAMS = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")


def params_of(enc, dtype):
    """The four parameters of `enc` as detached CPU copies in `dtype`, in the order of PARAMS."""
    return [p.detach().cpu().to(dtype).clone() for p in (enc.in_proj_weight, enc.in_proj_bias, enc.out_proj.weight, enc.out_proj.bias)]


def slopes(num_heads, alibi, dtype):
    return torch.tensor([2.0 ** (-8.0 * (a + 1) / num_heads) if alibi else 0.0 for a in range(num_heads)], dtype=dtype)


def attn_layer(x, w_in, b_in, w_o, b_o, num_heads, window, alibi, causal=True):
    """h [U, T, H] of the layer for x [U, T, E + 1], every step written out: scores, the recency bias, the mask as a select, softmax,
    the weighted sum, the out-projection.  `causal=False` removes the mask altogether (a sensitivity probe, not a mode of the layer)."""
    U, T, _ = x.shape
    H = w_o.shape[0]
    d = H // num_heads
    qkv = x @ w_in.T + b_in
    q, k, v = (t.reshape(U, T, num_heads, d).transpose(1, 2) for t in qkv.split(H, dim=2))       # [U, heads, T, d]
    t_idx = torch.arange(T)
    dist = (t_idx[:, None] - t_idx[None, :]).to(x.dtype)                                           # t - j
    s = q @ k.transpose(2, 3) / math.sqrt(d) - slopes(num_heads, alibi, x.dtype)[None, :, None, None] * dist
    if causal:
        keep = dist >= 0
        if window is not None:
            keep = keep & (dist < window)
        s = torch.where(keep, s, torch.full_like(s, -math.inf))
    o = (torch.softmax(s, dim=3) @ v).transpose(1, 2).reshape(U, T, H)
    return o @ w_o.T + b_o


def attn_cpu(enc, x, dtype=torch.float64, **override):
    """h of a CPU copy of `enc` in `dtype`; `override` replaces window / alibi / causal for the sensitivity probes."""
    kw = dict(window=enc.window, alibi=enc.alibi, causal=True)
    kw.update(override)
    with torch.no_grad():
        return attn_layer(x.to(dtype), *params_of(enc, dtype), enc.num_heads, **kw)


def fp32_bound(enc, x):
    """(bound, h64): max(4 max |h32cpu - h64cpu|, 1e-6) and the float64 result."""
    h64 = attn_cpu(enc, x, torch.float64)
    h32 = attn_cpu(enc, x, torch.float32)
    return max(4.0 * float((h32.double() - h64).abs().max()), 1e-6), h64


def loss_weights(U, T, H, seed, rows=None):
    """The cotangent g_h [U, T, H] of the loss sum(h * g_h): random, or zero except at `rows` (user, step) pairs -- what
    seq_collect_rows sends back."""
    g = torch.randn(U, T, H, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    if rows is not None:
        keep = torch.zeros(U, T, 1, dtype=torch.float64)
        for u, t in rows:
            keep[u, t] = 1.0
        g = g * keep
    return g


def cpu_grads(enc, table, idx, rts, g_h, dtype):
    """{name: gradient} of sum(h * g_h) over a CPU copy of `enc` in `dtype`, the inputs being cat([table[idx], rating]) with the
    table requiring grad: the four parameters and "table" [n_items, E]."""
    ps = [p.requires_grad_(True) for p in params_of(enc, dtype)]
    tb = table.detach().cpu().to(dtype).clone().requires_grad_(True)
    x = torch.cat([tb[idx], rts.to(dtype)[..., None]], 2)
    h = attn_layer(x, *ps, enc.num_heads, enc.window, enc.alibi)
    (h * g_h.to(dtype)).sum().backward()
    g = {n: p.grad for n, p in zip(PARAMS, ps)}
    g["table"] = tb.grad
    return g


def grad_bounds(enc, table, idx, rts, g_h):
    """(bounds, float64 gradients) under the rule of seq_grad_reference.grad_bounds."""
    U, T = idx.shape
    g64 = cpu_grads(enc, table, idx, rts, g_h, torch.float64)
    g32 = cpu_grads(enc, table, idx, rts, g_h, torch.float32)
    floor = 2.0 ** -23 * max(8.0, math.sqrt(U * T))
    return {n: max(4.0 * float((g32[n].double() - g64[n]).abs().max()), floor * float(g64[n].abs().max())) for n in g64}, g64


def positions(items, ratings, T, t0=0):
    """(idx int64 [U, T], ratings float32 [U, T]) of steps t0 .. t0 + T - 1 of every user."""
    idx = torch.from_numpy(np.stack([np.asarray(i[t0:t0 + T], dtype=np.int64) for i in items]))
    rts = torch.from_numpy(np.stack([np.asarray(r[t0:t0 + T], dtype=np.float32) for r in ratings]))
    return idx, rts


def make_encoder(E, H, heads, window, alibi, seed, bias_scale=0.1):
    """An AttentionEncoder(E + 1, H, heads) on the CPU with non-zero biases (the module initialises them to zero, which would leave
    the bias paths untested) and in-projection rows scaled up so that the softmax is far from uniform."""
    from recnn_amd.nn import AttentionEncoder
    torch.manual_seed(seed)
    enc = AttentionEncoder(E + 1, H, heads, window=window, alibi=alibi)
    with torch.no_grad():
        enc.in_proj_weight[: 2 * H] *= 3.0
        enc.in_proj_bias.normal_(0.0, bias_scale)
        enc.out_proj.bias.normal_(0.0, bias_scale)
    return enc
