"""The causal self-attention state encoder without a GPU: the float64 reference of tests/attn_reference.py pinned to torch's
scaled_dot_product_attention under an explicit additive mask, the parameter container, every host refusal of `attn_encode` /
`attn_encode_train`, the host-only workspace queries against their layouts written out, and `SeqEnv` accepting the type."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import attn_reference as A
import seq_reference as R
from helpers import csr, make_store


# ---------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("alibi", (True, False))
@pytest.mark.parametrize("window", (None, 1, 5))
@pytest.mark.parametrize("heads", (1, 3, 4))
def test_float64_reference_equals_sdpa_under_an_explicit_mask(heads, window, alibi):
    E, H, U, T = 8, 48, 3, 19
    enc = A.make_encoder(E, H, heads, window, alibi, seed=heads)
    x = torch.randn(U, T, E + 1, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    got = A.attn_cpu(enc, x, torch.float64)
    w_in, b_in, w_o, b_o = A.params_of(enc, torch.float64)
    d = H // heads
    q, k, v = (t.reshape(U, T, heads, d).transpose(1, 2) for t in TF.linear(x, w_in, b_in).split(H, dim=2))
    mask = torch.zeros(heads, T, T, dtype=torch.float64)
    for a in range(heads):
        m_a = 2.0 ** (-8.0 * (a + 1) / heads) if alibi else 0.0
        for t in range(T):
            for j in range(T):
                seen = j <= t and (window is None or t - j < window)
                mask[a, t, j] = -m_a * (t - j) if seen else -math.inf
    o = TF.scaled_dot_product_attention(q, k, v, attn_mask=mask[None])
    want = TF.linear(o.transpose(1, 2).reshape(U, T, H), w_o, b_o)
    err = float((got - want).abs().max())
    print(f"heads={heads} window={window} alibi={alibi}: max |reference - sdpa| = {err:.3e}")
    assert err <= 1e-12
    # the probes of the GPU tests change what they say they change
    if window is not None and window < T:
        assert float((A.attn_cpu(enc, x, window=None) - got).abs().max()) > 1e-6
    assert float((A.attn_cpu(enc, x, causal=False) - got).abs().max()) > 1e-6
    assert float((A.attn_cpu(enc, x, alibi=not alibi) - got).abs().max()) > (1e-6 if window != 1 else -1.0)


# ---------------------------------------------------------------------------------------------------- the module
def test_module_parameters_names_and_initialisation():
    import recnn_amd
    from recnn_amd.nn import AttentionEncoder
    assert recnn_amd.nn.AttentionEncoder is AttentionEncoder
    enc = AttentionEncoder(25, 48, 3, window=7, alibi=False)
    assert isinstance(enc, torch.nn.Module)
    assert (enc.input_size, enc.hidden_size, enc.num_heads, enc.head_dim, enc.window, enc.alibi) == (25, 48, 3, 16, 7, False)
    shapes = {n: tuple(p.shape) for n, p in enc.named_parameters()}
    assert shapes == {"in_proj_weight": (144, 25), "in_proj_bias": (144,), "out_proj.weight": (48, 48), "out_proj.bias": (48,)}
    assert list(enc.state_dict().keys()) == ["in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"]
    assert float(enc.in_proj_bias.detach().abs().max()) == 0.0 and float(enc.out_proj.bias.detach().abs().max()) == 0.0
    bound = math.sqrt(6.0 / (144 + 25))                    # xavier_uniform_, as torch.nn.MultiheadAttention initialises
    top = float(enc.in_proj_weight.detach().abs().max())
    assert 0.9 * bound < top <= bound
    assert float(enc.out_proj.weight.detach().abs().max()) <= math.sqrt(6.0 / 96)
    dflt = AttentionEncoder(9, 16, 1)
    assert dflt.window is None and dflt.alibi is True
    with pytest.raises(RuntimeError, match="attn_encode"):
        enc(torch.zeros(1, 2, 25))
    with pytest.raises(ValueError, match="num_heads"):
        AttentionEncoder(9, 48, 5)
    with pytest.raises(ValueError, match="window"):
        AttentionEncoder(9, 48, 3, window=0)


# ---------------------------------------------------------------------------------------------------- host refusals
@pytest.fixture(scope="module")
def cpu_store():
    from recnn_amd.data.store import ReplayStore
    items, ratings, table = make_store(6, 40, 8, 12, 20, seed=3)
    return ReplayStore.from_arrays(*csr(items, ratings), torch.device("cpu")), torch.from_numpy(table)


def test_host_refusals_by_name(cpu_store):
    from recnn_amd import _lib as L
    from recnn_amd.nn import AttentionEncoder
    from recnn_amd.nn import functional as F
    st, table = cpu_store
    fns = (F.attn_encode, F.attn_encode_train)
    ok = AttentionEncoder(9, 32, 2)
    for fn in fns:
        with pytest.raises(L.RecnnHipError, match="in_proj_weight.device"):                         # a CPU module, all else in order
            fn(ok, st, table, [0, 1], 4)
        for other, word in ((torch.nn.LSTM(9, 16), "LSTM.*lstm_encode"), (torch.nn.GRU(9, 16), "GRU.*gru_encode"),
                            (torch.nn.Linear(9, 16), "Linear")):
            with pytest.raises(L.RecnnHipError, match=word):
                fn(other, st, table, [0, 1], 4)
        bad = AttentionEncoder(9, 32, 2)
        bad.in_proj_weight.data = bad.in_proj_weight.data.double()
        with pytest.raises(L.RecnnHipError, match="in_proj_weight"):
            fn(bad, st, table, [0, 1], 4)
        bad = AttentionEncoder(9, 32, 2)
        bad.out_proj.weight.data = torch.zeros(32, 64)[:, ::2]
        with pytest.raises(L.RecnnHipError, match=r"out_proj\.weight.*strided"):
            fn(bad, st, table, [0, 1], 4)
        with pytest.raises(L.RecnnHipError, match="input_size=10"):
            fn(AttentionEncoder(10, 32, 2), st, table, [0, 1], 4)
        bad = AttentionEncoder(9, 32, 2)
        bad.num_heads = 3
        with pytest.raises(L.RecnnHipError, match="num_heads=3"):
            fn(bad, st, table, [0, 1], 4)
        for H, heads, word in ((32, 4, "head_dim=8"), (256, 2, "head_dim=128"), (48, 1, "head_dim=48")):
            with pytest.raises(L.RecnnHipError, match=word):
                fn(AttentionEncoder(9, H, heads), st, table, [0, 1], 4)
        with pytest.raises(L.RecnnHipError, match="hidden_size=320"):
            fn(AttentionEncoder(9, 320, 5), st, table, [0, 1], 4)
        for E in (4, 12, 136):
            with pytest.raises(L.RecnnHipError, match=f"E={E}"):
                fn(AttentionEncoder(E + 1, 32, 2), st, torch.zeros(40, E), [0, 1], 4)
        bad = AttentionEncoder(9, 32, 2)
        bad.window = 0
        with pytest.raises(L.RecnnHipError, match="window=0"):
            fn(bad, st, table, [0, 1], 4)
        shortest = int(st.lengths[[0, 1]].min())
        with pytest.raises(ValueError, match="history"):
            fn(ok, st, table, [0, 1], shortest + 1)
        with pytest.raises(ValueError, match="history"):
            fn(ok, st, table, [0, 1], shortest, t0=1)
        with pytest.raises(ValueError, match=r"2\^31"):
            fn(ok, st, table, [0] * 60000, 40000)
    with pytest.raises(L.RecnnHipError, match="table.requires_grad"):
        F.attn_encode_train(ok, st, table.clone().requires_grad_(True), [0, 1], 4)
    with pytest.raises(L.RecnnHipError, match="in_proj_weight.device"):                             # asked for: reaches the same checks
        F.attn_encode_train(ok, st, table.clone().requires_grad_(True), [0, 1], 4, train_table=True)
    with pytest.raises(L.RecnnHipError, match="in_proj_weight.device"):
        F.state_encode(ok, st, table, [0, 1], 4)
    with pytest.raises(L.RecnnHipError, match="RNN"):
        F.state_encode(torch.nn.RNN(9, 16), st, table, [0, 1], 4)


def test_seq_env_accepts_the_encoder_and_refuses_other_modules_by_name():
    from recnn_amd.data.env import SeqEnv
    from recnn_amd.nn import AttentionEncoder
    tbl, user_dict, users, _ = R.seq_env_data()
    env = SeqEnv.from_user_dict(tbl, user_dict, users, state_encoder=AttentionEncoder(9, 16, 1), batch_size=5, max_buf_size=20,
                                device="cpu")
    assert isinstance(env.state_encoder, AttentionEncoder)
    assert [tuple(s) for s in env.buffer_layout] == [(20, 16), (20, 8), (20, 1), (20, 16)]
    with pytest.raises(TypeError, match=r"torch\.nn\.modules\.rnn\.RNN"):
        SeqEnv.from_user_dict(tbl, user_dict, users, state_encoder=torch.nn.RNN(9, 16), batch_size=5, max_buf_size=20, device="cpu")
    with pytest.raises(TypeError, match="Linear"):
        SeqEnv(None, torch.nn.Linear(9, 16))


# ---------------------------------------------------------------------------------------------------- workspace queries
def _r256(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("U,T,H,heads,E,n_items", ((1, 1, 16, 1, 8, 5), (3, 700, 256, 4, 8, 50), (17, 65, 48, 3, 24, 300), (33, 130, 256, 16, 128, 1000),
                                                   (25, 1000, 256, 4, 128, 5000)))
def test_workspace_queries_against_their_layouts(U, T, H, heads, E, n_items):
    from recnn_amd import _lib as L
    lib = L.load()
    n, s, b = C.c_int64(), C.c_int64(), C.c_int64()
    keep = _r256(12 * U * T * H) + _r256(4 * U * T * H) + _r256(8 * U * heads * T)          # qkv, o, (m, l) of the log-sum-exp
    assert lib.recnn_attn_workspace_bytes(U, T, H, heads, C.byref(n)) == 0 and n.value == keep
    assert lib.recnn_attn_train_workspace_bytes(U, T, H, E, heads, C.byref(s), C.byref(b)) == 0
    assert s.value == keep
    nsplit = min(64, max(1, -(-U * T // 1024)))
    assert b.value == _r256(4 * H * H) + _r256(4 * U * T * H) + _r256(4 * U * heads * T) + _r256(12 * U * T * H) \
        + _r256(4 * nsplit * max(3 * H * (E + 2), H * (H + 1)))
    assert lib.recnn_attn_table_grad_workspace_bytes(U, T, H, E, n_items, C.byref(n)) == 0
    assert n.value == _r256(12 * E * H) + 2 * _r256(4 * U * T * E) + _r256(4 * n_items) + _r256(4 * (n_items + 1)) + 3 * _r256(4 * U * T)
    g = C.c_int64()
    assert lib.recnn_gru_table_grad_workspace_bytes(U, T, H, E, n_items, C.byref(g)) == 0 and g.value == n.value


def test_workspace_queries_and_entry_points_refuse_with_a_message():
    from recnn_amd import _lib as L
    lib = L.load()
    n, s, b = C.c_int64(), C.c_int64(), C.c_int64()
    assert lib.recnn_attn_workspace_bytes(4, 8, 32, 2, None) != 0 and b"null" in lib.recnn_last_error()
    for H, heads, word in ((24, 1, b"hidden"), (272, 17, b"hidden"), (48, 5, b"n_heads"), (32, 4, b"head_dim"), (256, 2, b"head_dim"),
                           (32, 0, b"n_heads")):
        assert lib.recnn_attn_workspace_bytes(4, 8, H, heads, C.byref(n)) != 0
        err = lib.recnn_last_error()
        assert b"attn_workspace_bytes" in err and word in err, err
        assert lib.recnn_attn_train_workspace_bytes(4, 8, H, 8, heads, C.byref(s), C.byref(b)) != 0
        assert b"attn_train_workspace_bytes" in lib.recnn_last_error() and word in lib.recnn_last_error()
    for E in (4, 12, 136):
        assert lib.recnn_attn_train_workspace_bytes(4, 8, 32, E, 2, C.byref(s), C.byref(b)) != 0
        assert b"emb_dim" in lib.recnn_last_error()
        assert lib.recnn_attn_table_grad_workspace_bytes(4, 8, 32, E, 50, C.byref(n)) != 0
        assert b"attn_table_grad_workspace_bytes" in lib.recnn_last_error() and b"emb_dim" in lib.recnn_last_error()
    assert lib.recnn_attn_workspace_bytes(65535, 40000, 32, 2, C.byref(n)) != 0 and b"2^31" in lib.recnn_last_error()
    assert lib.recnn_attn_table_grad_workspace_bytes(65535, 40000, 32, 8, 50, C.byref(n)) != 0 and b"2^31" in lib.recnn_last_error()
    assert lib.recnn_attn_table_grad_workspace_bytes(4, 8, 32, 8, 0, C.byref(n)) != 0 and b"n_items" in lib.recnn_last_error()
    # the launching entry points check their pointers first and the shapes next, both before any launch
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    head = lambda E, H, heads, window=0: (p, p, p, p, 4, 0, 3, p, 10, E, H, heads, window, 1)
    for E, H, heads, word in ((12, 32, 2, b"emb_dim"), (8, 24, 1, b"hidden"), (8, 48, 5, b"n_heads"), (8, 32, 4, b"head_dim")):
        for fn, name in ((lib.recnn_attn_encode, b"attn_encode"), (lib.recnn_attn_encode_train, b"attn_encode_train")):
            assert fn(*head(E, H, heads), p, p, p, p, p, p, None) != 0
            assert name in lib.recnn_last_error() and word in lib.recnn_last_error()
        assert lib.recnn_attn_backward(*head(E, H, heads), p, p, p, None, None, None, None, p, None) != 0
        assert b"attn_backward" in lib.recnn_last_error() and word in lib.recnn_last_error()
    assert lib.recnn_attn_encode(*head(8, 32, 2, window=-1), p, p, p, p, p, p, None) != 0 and b"window" in lib.recnn_last_error()
    assert lib.recnn_attn_encode(*([None] * 4), 4, 0, 3, None, 10, 8, 32, 2, 0, 1, *([None] * 7)) != 0
    assert b"attn_encode" in lib.recnn_last_error() and b"null" in lib.recnn_last_error()
    assert lib.recnn_attn_backward(*([None] * 4), 4, 0, 3, None, 10, 8, 32, 2, 0, 1, *([None] * 9)) != 0
    assert b"attn_backward" in lib.recnn_last_error() and b"null" in lib.recnn_last_error()
    assert lib.recnn_attn_backward_table(*head(8, 32, 2), p, p, p, p, None, None, None, None, None, p, p, None) != 0
    assert b"d_table" in lib.recnn_last_error()
