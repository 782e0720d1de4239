"""The parameter container of the causal self-attention state encoder (csrc/attn.hip)."""
import torch
import torch.nn as nn


class AttentionEncoder(nn.Module):
    """One layer of causal multi-head self-attention over a user's history, as a state encoder beside torch.nn.LSTM and torch.nn.GRU:
    for step t of a call, with x_t = [table[item_t] | rating_t] (width `input_size` = E + 1),

        [q_t | k_t | v_t] = in_proj_weight x_t + in_proj_bias                      in_proj_weight [3H, E + 1], order q, k, v
        s_a(t, j) = (q_t^a . k_j^a) / sqrt(head_dim) - m_a (t - j)                  j in [max(0, t - window + 1), t], head a
        h_t = out_proj(sum_j softmax_j(s_a)(t, j) v_j^a)                            out_proj: Linear(H, H)

    m_a = 2^(-8 (a + 1) / num_heads) with `alibi` (a recency bias without parameters or a maximum length), else 0; `window=None`
    attends to every earlier step of the call.  No residual, LayerNorm or feed-forward block: `TransformerStateEncoder`
    (nn/transformer.py) is this layer inside pre-LN blocks with all three.  Initialised as torch.nn.MultiheadAttention is (xavier_uniform_ weights, zero biases).

    The module only holds the parameters, as a torch.nn.LSTM does for `lstm_encode`: the layer runs in
    `recnn_amd.nn.functional.attn_encode` / `attn_encode_train` (or `state_encode`, or a `SeqEnv`), which read the store."""

    def __init__(self, input_size, hidden_size, num_heads, window=None, alibi=True):
        super().__init__()
        self.input_size, self.hidden_size, self.num_heads = int(input_size), int(hidden_size), int(num_heads)
        if self.num_heads < 1 or self.hidden_size % self.num_heads:
            raise ValueError(f"AttentionEncoder: hidden_size={hidden_size} is not a multiple of num_heads={num_heads}")
        if window is not None and int(window) < 1:
            raise ValueError(f"AttentionEncoder: window={window} must be at least 1 (or None)")
        self.head_dim = self.hidden_size // self.num_heads
        self.window = None if window is None else int(window)
        self.alibi = bool(alibi)
        self.in_proj_weight = nn.Parameter(torch.empty(3 * self.hidden_size, self.input_size))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * self.hidden_size))
        self.out_proj = nn.Linear(self.hidden_size, self.hidden_size)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.xavier_uniform_(self.out_proj.weight)
        nn.init.zeros_(self.in_proj_bias)
        nn.init.zeros_(self.out_proj.bias)

    def extra_repr(self):
        return (f"input_size={self.input_size}, hidden_size={self.hidden_size}, num_heads={self.num_heads}, window={self.window}, "
                f"alibi={self.alibi}")

    def forward(self, *args, **kwargs):
        raise RuntimeError("AttentionEncoder holds parameters only: encode with recnn_amd.nn.functional.attn_encode(enc, store, table, "
                           "slots, T) or attn_encode_train (state_encode and SeqEnv dispatch to them)")
