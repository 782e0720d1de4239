"""Host restatement of the transformer state encoder (test infrastructure, not an oracle file): the model of
recnn_amd.nn.TransformerStateEncoder written out in plain torch on the CPU, in float64 and float32, over the materialised
[U, T, E + 1] inputs of tests/seq_reference.py (`lstm_inputs`), its autograd gradients, and the bounds every transformer test uses:

  forward    max(4 max |h32cpu - h64cpu|, 1e-6)                                             (attn_reference.fp32_bound's rule)
  gradients  per tensor G: max(4 max |G32cpu - G64cpu|, 2^-23 max(8, sqrt(U T)) max |G64|)  (attn_reference.grad_bounds' rule)

tests/test_transformer_cpu.py pins `block` in float64 to torch.nn.TransformerEncoderLayer(norm_first=True, dropout=0) under a causal
mask.  The attention inside a block is attn_reference.attn_layer, which tests/test_attn_cpu.py pins to scaled_dot_product_attention."""
import math

import torch

import attn_reference as A

BLOCK_PARAMS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
                "norm2.bias")


def layer_norm(z, gamma, beta, eps):
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    return (z - mean) / torch.sqrt(var + eps) * gamma + beta


def activation(a, name):
    if name == "relu":
        return torch.where(a > 0, a, torch.zeros_like(a))
    if name == "gelu":
        return 0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0)))
    raise ValueError(name)


def block(x, p, num_heads, window, alibi, act, eps, causal=True, norms=True, ffn=True, residual=True, pre=None):
    """One pre-LN block on x [U, T, H]; p: {name of BLOCK_PARAMS: tensor}.  `causal`, `norms`, `ffn` and `residual` switch a piece off
    (sensitivity probes, not modes of the model); `pre`, a list, receives the feed-forward's pre-activation."""
    ln = layer_norm if norms else (lambda z, g, b, e: z)
    a = A.attn_layer(ln(x, p["norm1.weight"], p["norm1.bias"], eps), p["self_attn.in_proj_weight"], p["self_attn.in_proj_bias"],
                     p["self_attn.out_proj.weight"], p["self_attn.out_proj.bias"], num_heads, window, alibi, causal=causal)
    u = x + a if residual else a
    if not ffn:
        return u
    a1 = ln(u, p["norm2.weight"], p["norm2.bias"], eps) @ p["linear1.weight"].T + p["linear1.bias"]
    if pre is not None:
        pre.append(a1)
    f = activation(a1, act) @ p["linear2.weight"].T + p["linear2.bias"]
    return u + f if residual else f


def model(x_in, params, enc, pre=None, **probe):
    """h [U, T, H] for x_in [U, T, E + 1]; params: {name: tensor} under the module's own parameter names."""
    kw = dict(window=enc.window, alibi=enc.alibi, act=enc.activation, causal=True, norms=True, ffn=True, residual=True)
    kw.update(probe)
    norms = kw["norms"]
    x = x_in @ params["embed.weight"].T + params["embed.bias"]
    for i in range(enc.num_layers):
        p = {n: params[f"layers.{i}.{n}"] for n in BLOCK_PARAMS}
        x = block(x, p, enc.num_heads, kw["window"], kw["alibi"], kw["act"], enc.eps, causal=kw["causal"], norms=norms, ffn=kw["ffn"],
                  residual=kw["residual"], pre=pre)
    return layer_norm(x, params["norm.weight"], params["norm.bias"], enc.eps) if norms else x


def params_of(enc, dtype):
    """{name: detached CPU copy in `dtype`} of the module's parameters."""
    return {n: p.detach().cpu().to(dtype).clone() for n, p in enc.named_parameters()}


def model_cpu(enc, x, dtype=torch.float64, pre=None, **probe):
    with torch.no_grad():
        return model(x.to(dtype), params_of(enc, dtype), enc, pre=pre, **probe)


def fp32_bound(enc, x):
    """(bound, h64): max(4 max |h32cpu - h64cpu|, 1e-6) and the float64 result."""
    h64 = model_cpu(enc, x, torch.float64)
    h32 = model_cpu(enc, x, torch.float32)
    return max(4.0 * float((h32.double() - h64).abs().max()), 1e-6), h64


def smallest_preactivation(enc, x):
    """The smallest |a_1| of the float64 reference over all blocks: how far relu's kink is from every pre-activation."""
    pre = []
    model_cpu(enc, x, torch.float64, pre=pre)
    return min(float(a.abs().min()) for a in pre)


def cpu_grads(enc, table, idx, rts, g_h, dtype):
    """{name: gradient} of sum(h * g_h) over a CPU copy of `enc` in `dtype`, the inputs being cat([table[idx], rating]) with the table
    requiring grad: every parameter of the module and "table" [n_items, E]."""
    ps = {n: p.requires_grad_(True) for n, p in params_of(enc, dtype).items()}
    tb = table.detach().cpu().to(dtype).clone().requires_grad_(True)
    x = torch.cat([tb[idx], rts.to(dtype)[..., None]], 2)
    h = model(x, ps, enc)
    (h * g_h.to(dtype)).sum().backward()
    g = {n: p.grad for n, p in ps.items()}
    g["table"] = tb.grad
    return g


def grad_bounds(enc, table, idx, rts, g_h):
    """(bounds, float64 gradients) under the rule of attn_reference.grad_bounds."""
    U, T = idx.shape
    g64 = cpu_grads(enc, table, idx, rts, g_h, torch.float64)
    g32 = cpu_grads(enc, table, idx, rts, g_h, torch.float32)
    floor = 2.0 ** -23 * max(8.0, math.sqrt(U * T))
    return {n: max(4.0 * float((g32[n].double() - g64[n]).abs().max()), floor * float(g64[n].abs().max())) for n in g64}, g64


def make_encoder(E, H, heads, F, L, activation, window, alibi, seed, bias_scale=0.1):
    """A TransformerStateEncoder(E + 1, H, heads, L, F) on the CPU with non-zero biases, non-trivial gamma and beta (the module
    initialises them to 0, 1 and 0, which would leave those paths untested) and the q, k rows of every in-projection scaled by 3 so
    that the softmax is far from uniform."""
    from recnn_amd.nn import TransformerStateEncoder
    torch.manual_seed(seed)
    enc = TransformerStateEncoder(E + 1, H, heads, num_layers=L, dim_feedforward=F, activation=activation, window=window, alibi=alibi)
    with torch.no_grad():
        for blk in enc.layers:
            blk.self_attn.in_proj_weight[: 2 * H] *= 3.0
            blk.self_attn.in_proj_bias.normal_(0.0, bias_scale)
            blk.self_attn.out_proj.bias.normal_(0.0, bias_scale)
            for norm in (blk.norm1, blk.norm2):
                norm.weight.normal_(1.0, 0.2)
                norm.bias.normal_(0.0, bias_scale)
        enc.norm.weight.normal_(1.0, 0.2)
        enc.norm.bias.normal_(0.0, bias_scale)
    return enc
