"""The transformer state encoder without a GPU: the float64 reference block of tests/transformer_reference.py is pinned to
torch.nn.TransformerEncoderLayer, the module exchanges state dicts with that layer, the host-only workspace query does not depend on
the feed-forward width, and every refusal is made on the host."""
import ctypes as C

import numpy as np
import pytest
import torch

import transformer_reference as TR
from helpers import csr, make_store


@pytest.mark.parametrize("act", ("relu", "gelu"))
@pytest.mark.parametrize("dims", ((16, 1, 16), (48, 3, 80), (256, 4, 1024)), ids=lambda d: "H%d-heads%d-F%d" % d)
def test_reference_block_is_torchs_pre_ln_encoder_layer(dims, act):
    H, heads, F = dims
    torch.manual_seed(H + F)
    layer = torch.nn.TransformerEncoderLayer(H, heads, F, dropout=0.0, activation=act, norm_first=True, batch_first=True).double()
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if n.endswith("bias") or n.startswith("norm"):
                p.add_(0.1 * torch.randn_like(p))
    U, T = 3, 37
    x = torch.randn(U, T, H, dtype=torch.float64)
    mask = torch.triu(torch.full((T, T), -np.inf, dtype=torch.float64), diagonal=1)
    with torch.no_grad():
        layer.train()                                                     # (the plain path: dropout is 0)
        want = layer(x, src_mask=mask)
        p = {n: v.detach().clone() for n, v in layer.state_dict().items()}
        got = TR.block(x, p, heads, None, False, act, layer.norm1.eps)
    err = float((got - want).abs().max())
    print(f"reference block {dims} {act}: max |difference| to torch's layer {err:.3e}, max |y| {float(want.abs().max()):.3e}")
    assert err <= 1e-12 and float(want.abs().max()) > 0.1
    # and the probes are real: every piece moves the result
    for probe in (dict(causal=False), dict(norms=False), dict(ffn=False), dict(residual=False)):
        moved = float((TR.block(x, p, heads, None, False, act, 1e-5, **probe) - want).abs().max())
        assert moved > 1e-3, probe


def test_state_dict_round_trip_with_torchs_layer():
    from recnn_amd.nn import TransformerStateEncoder
    enc = TransformerStateEncoder(25, 48, 3, num_layers=2, dim_feedforward=80, activation="gelu")
    layer = torch.nn.TransformerEncoderLayer(48, 3, 80, dropout=0.0, activation="gelu", norm_first=True, batch_first=True)
    want = {k: tuple(v.shape) for k, v in layer.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in enc.layers[0].state_dict().items()} == want
    with torch.no_grad():
        for p in layer.parameters():
            p.normal_()
    enc.layers[1].load_state_dict(layer.state_dict(), strict=True)
    assert all(torch.equal(enc.layers[1].state_dict()[k], v) for k, v in layer.state_dict().items())
    other = torch.nn.TransformerEncoderLayer(48, 3, 80, dropout=0.0, norm_first=True, batch_first=True)
    other.load_state_dict(enc.layers[1].state_dict(), strict=True)
    assert all(torch.equal(other.state_dict()[k], v) for k, v in layer.state_dict().items())
    # the attributes, the defaults and the initialisation of torch's layer
    assert isinstance(enc.embed, torch.nn.Linear) and tuple(enc.embed.weight.shape) == (48, 25)
    assert isinstance(enc.layers, torch.nn.ModuleList) and len(enc.layers) == 2 and isinstance(enc.norm, torch.nn.LayerNorm)
    assert (enc.hidden_size, enc.input_size, enc.num_heads, enc.num_layers, enc.dim_feedforward) == (48, 25, 3, 2, 80)
    assert TransformerStateEncoder(9, 32, 2).dim_feedforward == 32 and TransformerStateEncoder(9, 32, 2).num_layers == 2
    sa = enc.layers[0].self_attn
    assert not sa.in_proj_bias.any() and not sa.out_proj.bias.any() and float(sa.in_proj_weight.detach().abs().max()) <= (6.0 / (4 * 48)) ** 0.5
    assert bool((enc.layers[0].norm1.weight == 1).all()) and not enc.layers[0].norm1.bias.any()


def test_block_workspace_does_not_depend_on_the_feed_forward_width():
    """The no-grad encode keeps the [U T, F] activation in LDS: the workspace query has no F argument at all, the training forward's
    `saved` grows by exactly the pre-activation, and both grow with U T."""
    from recnn_amd import _lib as L
    lib = L.load()
    assert len(L.SIGNATURES["recnn_block_workspace_bytes"][1]) == 5      # n_users, T, hidden, n_heads, bytes
    a, b, s16, s1024, bw = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    assert lib.recnn_block_workspace_bytes(25, 100, 256, 4, C.byref(a)) == 0
    assert lib.recnn_block_workspace_bytes(50, 100, 256, 4, C.byref(b)) == 0
    assert 0 < a.value < b.value and a.value >= 25 * 100 * 256 * 4 * 5
    assert lib.recnn_block_train_workspace_bytes(25, 100, 256, 4, 16, C.byref(s16), C.byref(bw)) == 0
    assert lib.recnn_block_train_workspace_bytes(25, 100, 256, 4, 1024, C.byref(s1024), C.byref(bw)) == 0
    assert s16.value - a.value == 25 * 100 * 16 * 4 and s1024.value - a.value == 25 * 100 * 1024 * 4
    # refusals of the host-only queries
    assert lib.recnn_block_workspace_bytes(25, 100, 250, 5, C.byref(a)) != 0 and b"hidden" in lib.recnn_last_error()
    assert lib.recnn_block_train_workspace_bytes(25, 100, 256, 4, 24, C.byref(s16), C.byref(bw)) != 0
    assert b"dim_feedforward" in lib.recnn_last_error()
    assert lib.recnn_block_train_workspace_bytes(25, 100, 256, 4, 2048, C.byref(s16), C.byref(bw)) != 0


def _store(E=8):
    from recnn_amd.data.store import ReplayStore
    items, ratings, table = make_store(4, 40, E, 12, 14, seed=1)
    return ReplayStore.from_arrays(*csr(items, ratings), torch.device("cpu")), torch.from_numpy(table)


def test_forward_raises_and_a_cpu_module_is_refused():
    from recnn_amd import _lib as L
    from recnn_amd.nn import TransformerStateEncoder, functional as F
    enc = TransformerStateEncoder(9, 16, 1)
    with pytest.raises(RuntimeError, match="transformer_encode"):
        enc(torch.zeros(2, 3, 9))
    with pytest.raises(RuntimeError, match="parameters only"):
        enc.layers[0](torch.zeros(2, 3, 16))
    st, table = _store()
    for fn in (F.transformer_encode, F.transformer_encode_train):
        with pytest.raises(L.RecnnHipError, match="needs a GPU module"):
            fn(enc, st, table, [0, 1], 4)
    with pytest.raises(L.RecnnHipError, match="needs a GPU module"):
        F.state_encode(enc, st, table, [0, 1], 4)


def test_host_side_refusals():
    from recnn_amd import _lib as L
    from recnn_amd.nn import AttentionEncoder, TransformerStateEncoder, functional as F
    st, table = _store()
    ok = lambda **kw: TransformerStateEncoder(9, 16, 1, **kw)
    # at construction
    for kw in (dict(num_layers=0), dict(dim_feedforward=24), dict(dim_feedforward=2048), dict(dim_feedforward=0),
               dict(activation="tanh"), dict(eps=0.0), dict(eps=-1e-5), dict(window=0)):
        with pytest.raises(ValueError):
            ok(**kw)
    with pytest.raises(ValueError):
        TransformerStateEncoder(9, 16, 3)
    # at the call, by argument name, whatever happened to the module since
    def refused(enc, match, tbl=table, T=4, t0=0, exc=L.RecnnHipError):
        for fn in (F.transformer_encode, F.transformer_encode_train):
            with pytest.raises(exc, match=match):
                fn(enc, st, tbl, [0, 1], T, t0=t0)
    enc = ok()
    enc.dim_feedforward = 24
    refused(enc, "dim_feedforward")
    enc = ok()
    enc.num_layers = 0
    refused(enc, "num_layers")
    enc = ok()
    enc.activation = "tanh"
    refused(enc, "activation")
    enc = ok()
    enc.eps = 0.0
    refused(enc, "eps")
    enc = ok()
    enc.window = 0
    refused(enc, "window")
    refused(AttentionEncoder(9, 16, 1), "TransformerStateEncoder")
    refused(torch.nn.LSTM(9, 16), "TransformerStateEncoder")
    refused(ok().double(), "embed.weight must be a contiguous float32")
    refused(TransformerStateEncoder(10, 16, 1), "input_size")
    refused(TransformerStateEncoder(9, 128, 1), "head_dim")
    refused(TransformerStateEncoder(9, 24, 1, dim_feedforward=32), "head_dim")
    refused(TransformerStateEncoder(13, 16, 1), "multiple of 8", tbl=torch.zeros(40, 12))
    enc = ok()
    enc.layers[1].linear1 = torch.nn.Linear(16, 32)
    refused(enc, "shapes")
    refused(ok(), "history", T=40, exc=ValueError)
    refused(ok(), "T >= 1", T=0, exc=ValueError)
    with pytest.raises(L.RecnnHipError, match="train_table"):
        F.transformer_encode_train(ok(), st, table.clone().requires_grad_(True), [0, 1], 4)
    # SeqEnv and state_encode name the new module among what they accept
    from recnn_amd.data.env import SeqEnv
    with pytest.raises(TypeError, match="TransformerStateEncoder"):
        SeqEnv(None, torch.nn.RNN(9, 16))
    with pytest.raises(L.RecnnHipError, match="TransformerStateEncoder"):
        F.state_encode(torch.nn.RNN(9, 16), st, table, [0, 1], 4)
