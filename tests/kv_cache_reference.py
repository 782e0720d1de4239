"""Host restatement of the step-by-step path of the attention encoders (test infrastructure, not an oracle file): the float64 model
of tests/transformer_reference.py written incrementally -- K and V kept per layer and per session, appended to, and the new steps
attending to them -- and the tile walk of the append's attention kernel restated as a set of positions, for the ring-size checks.

`IncrementalModel.append(x_new)` must give rows P .. P + n - 1 of `transformer_reference.model_cpu` over the P + n steps so far
(tests/test_kv_cache_cpu.py holds the two together within 1e-12)."""
import math

import torch

import attn_reference as A
import transformer_reference as TR

TILE = 64


class IncrementalModel:
    """The transformer of `transformer_reference.model` for U sessions, fed n steps at a time: per layer the keys and values of
    every step so far (under a window w only the last w - 1 + n are ever attended to, and only those are kept)."""

    def __init__(self, enc, dtype=torch.float64):
        self.enc, self.dtype = enc, dtype
        self.p = TR.params_of(enc, dtype)
        self.k = [None] * enc.num_layers
        self.v = [None] * enc.num_layers
        self.first = 0          # the position of row 0 of k / v
        self.length = 0

    def _attend(self, layer, xn, P):
        """Attention of the new rows xn [U, n, H] (already normalised) at positions P .. P + n - 1 over the layer's cache."""
        enc, p = self.enc, self.p
        H, heads = enc.hidden_size, enc.num_heads
        d = H // heads
        U, n, _ = xn.shape
        qkv = xn @ p[f"layers.{layer}.self_attn.in_proj_weight"].T + p[f"layers.{layer}.self_attn.in_proj_bias"]
        q, k, v = qkv.split(H, dim=2)
        self.k[layer] = k if self.k[layer] is None else torch.cat([self.k[layer], k], 1)
        self.v[layer] = v if self.v[layer] is None else torch.cat([self.v[layer], v], 1)
        K, V = self.k[layer], self.v[layer]
        S = K.shape[1]
        qh = q.reshape(U, n, heads, d).transpose(1, 2)
        kh = K.reshape(U, S, heads, d).transpose(1, 2)
        vh = V.reshape(U, S, heads, d).transpose(1, 2)
        tq = torch.arange(P, P + n)
        tk = torch.arange(self.first, self.first + S)
        dist = (tq[:, None] - tk[None, :]).to(self.dtype)
        s = qh @ kh.transpose(2, 3) / math.sqrt(d) - A.slopes(heads, enc.alibi, self.dtype)[None, :, None, None] * dist
        keep = dist >= 0
        if enc.window is not None:
            keep = keep & (dist < enc.window)
        s = torch.where(keep, s, torch.full_like(s, -math.inf))
        o = (torch.softmax(s, dim=3) @ vh).transpose(1, 2).reshape(U, n, H)
        return o @ p[f"layers.{layer}.self_attn.out_proj.weight"].T + p[f"layers.{layer}.self_attn.out_proj.bias"]

    def append(self, x_new):
        """h [U, n, H] of the new steps x_new [U, n, E + 1]."""
        enc, p = self.enc, self.p
        P = self.length
        with torch.no_grad():
            x = x_new.to(self.dtype) @ p["embed.weight"].T + p["embed.bias"]
            for i in range(enc.num_layers):
                pre = f"layers.{i}."
                u = x + self._attend(i, TR.layer_norm(x, p[pre + "norm1.weight"], p[pre + "norm1.bias"], enc.eps), P)
                a1 = TR.layer_norm(u, p[pre + "norm2.weight"], p[pre + "norm2.bias"], enc.eps) @ p[pre + "linear1.weight"].T \
                    + p[pre + "linear1.bias"]
                x = u + TR.activation(a1, enc.activation) @ p[pre + "linear2.weight"].T + p[pre + "linear2.bias"]
            self.length = P + x_new.shape[1]
            if enc.window is not None:          # what no later step can reach is dropped
                drop = max(0, self.length - (enc.window - 1) - self.first)
                self.k = [k[:, drop:] for k in self.k]
                self.v = [v[:, drop:] for v in self.v]
                self.first += drop
            return TR.layer_norm(x, p["norm.weight"], p["norm.bias"], enc.eps)


def run_split(enc, x, sizes, dtype=torch.float64):
    """h [U, sum(sizes), H]: x fed to an `IncrementalModel` in appends of `sizes` steps."""
    m, out, at = IncrementalModel(enc, dtype), [], 0
    for n in sizes:
        out.append(m.append(x[:, at:at + n]))
        at += n
    return torch.cat(out, 1)


def staged_positions(pos, n, window):
    """The positions the append kernel reads from the cache for an append of n steps at position `pos` under `window` (None: no
    window): per 64-aligned query block q0 that [pos, pos + n) touches, the key tiles from the one that holds max(0, q0 - w + 1) up
    to the block's own, their rows below pos + n."""
    end = pos + n
    out = set()
    for qb in range(pos // TILE, (end - 1) // TILE + 1):
        q0 = qb * TILE
        lo = 0 if window is None else max(0, q0 - window + 1) // TILE
        for kt in range(lo, qb + 1):
            out.update(t for t in range(kt * TILE, (kt + 1) * TILE) if t < end)
    return out


def ring_is_safe(pos, n, window, capacity):
    """Whether, in a ring of `capacity` slots, the staged positions and the positions the append writes all lie in different slots
    -- and every staged position is one of the last `capacity` written (so its slot still holds it)."""
    live = staged_positions(pos, n, window) | set(range(pos, pos + n))
    return len({t % capacity for t in live}) == len(live) and min(live) > pos + n - 1 - capacity
