"""The parameter containers of the transformer state encoder (csrc/block.hip)."""
import torch
import torch.nn as nn

ACTIVATIONS = {"relu": 0, "gelu": 1}


class _SelfAttention(nn.Module):
    """The parameters of a block's attention under the names torch.nn.MultiheadAttention gives them."""

    def __init__(self, hidden_size):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * hidden_size, hidden_size))
        self.in_proj_bias = nn.Parameter(torch.empty(3 * hidden_size))
        self.out_proj = nn.Linear(hidden_size, hidden_size)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.in_proj_bias)
        nn.init.zeros_(self.out_proj.bias)


class TransformerBlock(nn.Module):
    """One pre-LN block, u = x + out_proj(Attn(norm1(x))), y = u + linear2(act(linear1(norm2(u)))): the parameters only, under the
    keys and shapes of torch.nn.TransformerEncoderLayer (`load_state_dict` works strictly in both directions) and initialised as
    that layer is."""

    def __init__(self, hidden_size, dim_feedforward, eps=1e-5):
        super().__init__()
        self.self_attn = _SelfAttention(hidden_size)
        self.linear1 = nn.Linear(hidden_size, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, hidden_size)
        self.norm1 = nn.LayerNorm(hidden_size, eps=eps)
        self.norm2 = nn.LayerNorm(hidden_size, eps=eps)

    def forward(self, *args, **kwargs):
        raise RuntimeError("TransformerBlock holds parameters only: it runs inside recnn_amd.nn.functional.transformer_encode")


class TransformerStateEncoder(nn.Module):
    """A stack of pre-LN transformer blocks over a user's history, as a state encoder beside torch.nn.LSTM, torch.nn.GRU and
    `AttentionEncoder` (SASRec's encoder): for step t of a call, with [table[item_t] | rating_t] of width `input_size` = E + 1,

        x^0_t   = embed([table[item_t] | rating_t])                                  embed: Linear(E + 1, H)
        u       = x^l + out_proj(Attn_l(norm1(x^l)))                                 Attn: AttentionEncoder's layer on a dense input
        x^l+1   = u + linear2(act(linear1(norm2(u))))                                linear1: Linear(H, F), linear2: Linear(F, H)
        h_t     = norm(x^L_t)                                                        LayerNorm(H), eps

    for l = 0 .. num_layers - 1, with the causal mask, `window` and ALiBi slopes of `AttentionEncoder` in every block; `act` is
    "relu" or "gelu" (the exact erf form, torch's default); `dim_feedforward=None` means `hidden_size` (SASRec's choice).  One
    block with alibi=False, window=None is torch.nn.TransformerEncoderLayer(H, heads, F, dropout=0, norm_first=True,
    batch_first=True) under a causal mask, and `layers[i]` exchanges state dicts with it.

    Not covered: dropout, learned positional embeddings, a KV cache across calls, bf16 or split-bf16 arithmetic.

    The module only holds the parameters: the stack runs in `recnn_amd.nn.functional.transformer_encode` /
    `transformer_encode_train` (or `state_encode`, or a `SeqEnv`), which read the store."""

    def __init__(self, input_size, hidden_size, num_heads, num_layers=2, dim_feedforward=None, activation="relu", window=None,
                 alibi=True, eps=1e-5):
        super().__init__()
        self.input_size, self.hidden_size, self.num_heads = int(input_size), int(hidden_size), int(num_heads)
        self.num_layers = int(num_layers)
        self.dim_feedforward = self.hidden_size if dim_feedforward is None else int(dim_feedforward)
        if self.num_heads < 1 or self.hidden_size % self.num_heads:
            raise ValueError(f"TransformerStateEncoder: hidden_size={hidden_size} is not a multiple of num_heads={num_heads}")
        if window is not None and int(window) < 1:
            raise ValueError(f"TransformerStateEncoder: window={window} must be at least 1 (or None)")
        if self.num_layers < 1:
            raise ValueError(f"TransformerStateEncoder: num_layers={num_layers} must be at least 1")
        if activation not in ACTIVATIONS:
            raise ValueError(f"TransformerStateEncoder: activation={activation!r} is not one of {sorted(ACTIVATIONS)}")
        if self.dim_feedforward % 16 or not 16 <= self.dim_feedforward <= 1024:
            raise ValueError(f"TransformerStateEncoder: dim_feedforward={self.dim_feedforward} must be a multiple of 16 in 16 .. 1024")
        if not float(eps) > 0:
            raise ValueError(f"TransformerStateEncoder: eps={eps} must be positive")
        self.head_dim = self.hidden_size // self.num_heads
        self.window = None if window is None else int(window)
        self.alibi = bool(alibi)
        self.activation = activation
        self.eps = float(eps)
        self.embed = nn.Linear(self.input_size, self.hidden_size)
        self.layers = nn.ModuleList(TransformerBlock(self.hidden_size, self.dim_feedforward, self.eps) for _ in range(self.num_layers))
        self.norm = nn.LayerNorm(self.hidden_size, eps=self.eps)

    def extra_repr(self):
        return (f"input_size={self.input_size}, hidden_size={self.hidden_size}, num_heads={self.num_heads}, "
                f"num_layers={self.num_layers}, dim_feedforward={self.dim_feedforward}, activation={self.activation}, "
                f"window={self.window}, alibi={self.alibi}, eps={self.eps}")

    def forward(self, *args, **kwargs):
        raise RuntimeError("TransformerStateEncoder holds parameters only: encode with recnn_amd.nn.functional.transformer_encode(enc, "
                           "store, table, slots, T) or transformer_encode_train (state_encode and SeqEnv dispatch to them)")
