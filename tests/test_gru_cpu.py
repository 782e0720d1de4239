"""The GRU state encoder, host side (no GPU): the hand-written BPTT of the equations the reverse chain of csrc/gru.hip is written from
against float64 autograd of torch.nn.GRU, the host-only workspace queries against the layouts include/recnn_hip.h documents, the
refused shapes, and the refusals by name of the Python layer."""
import ctypes as C
import warnings

import pytest
import torch

import gru_reference as G
import seq_reference as R
from helpers import make_store


@pytest.mark.parametrize("E,H,U,T", [(8, 16, 5, 37), (24, 48, 3, 5)])
def test_hand_written_bptt_matches_float64_autograd(E, H, U, T):
    items, ratings, table = make_store(U, 40, E, T + 1, T + 3, seed=2)
    torch.manual_seed(2)
    gru = torch.nn.GRU(E + 1, H)
    x = R.lstm_inputs(torch.from_numpy(table), items, ratings, T)
    h0 = torch.randn(U, H, generator=torch.Generator().manual_seed(7)) * 0.5
    Rw = G.loss_weights(U, T, H, seed=3)
    ref = G.cpu_grads(gru, x, h0, Rw, torch.float64)
    hand = G.bptt_by_hand(gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0, x, h0, Rw)
    assert set(ref) == set(G.NAMES) == set(hand)
    for n in G.NAMES:
        err, scale = float((hand[n] - ref[n]).abs().max()), float(ref[n].abs().max())
        print(f"hand BPTT vs float64 autograd {n}: err {err:.3e} of {scale:.3e}")
        assert scale > 0 and err <= 1e-10 * scale
    # b_hn sits inside the reset product: the two bias gradients part in their last third
    assert torch.equal(hand["bias_ih_l0"][:2 * H], hand["bias_hh_l0"][:2 * H])
    assert not torch.equal(hand["bias_ih_l0"][2 * H:], hand["bias_hh_l0"][2 * H:])
    bounds, g64 = G.grad_bounds(gru, x, h0, Rw)
    assert all(bounds[n] > 0 for n in G.NAMES) and all(torch.equal(g64[n], ref[n]) for n in G.NAMES)


def test_training_case_is_chosen_on_the_float64_restatement():
    *_, lr, losses = G.training_case()
    print(f"GRU training case: lr {lr}, float64 loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert len(losses) == G.TRAIN_SGD_STEPS + 1 and losses[-1] <= 0.9 * losses[0] and lr > 0


def test_env_loop_keeps_the_same_steps_for_either_encoder():
    """The kept steps depend on the draws alone: the GRU run of the SeqEnv loop hands out buffers of 20, 17 and 20 rows, as the
    LSTM run does."""
    import numpy as np
    table, user_dict, users, gru = G.gru_env_data()
    np.random.seed(R.SEQ_ENV_SEED)
    out, bound = G.gru_env_batches(table, user_dict, users, gru, 5, 20, 3)
    assert [b["meta"]["rows"] for b in out] == [20, 17, 20] and bound >= 1e-6
    np.random.seed(R.SEQ_ENV_SEED)
    lstm_out, _ = R.seq_env_batches(table, user_dict, users, R.seq_env_data()[3], 5, 20, 3)
    assert [b["meta"]["step"] for b in out] == [b["meta"]["step"] for b in lstm_out]
    assert all(np.array_equal(a["action"], b["action"]) for a, b in zip(out, lstm_out))
    assert not np.array_equal(out[0]["state"], lstm_out[0]["state"])


def _round(n, to):
    return (n + to - 1) // to * to


@pytest.mark.parametrize("E,H", [(8, 16), (40, 96), (128, 256)])
def test_workspace_queries_give_the_documented_layouts(E, H):
    """include/recnn_hip.h, written out (tiles = ceil(U / 16), Tc = min(T, 32)):
      pre       [user tile][Tc][H / 16][r, z, nx][64 lanes] 16-byte vectors (variant 1; nothing for variant 0)
      saved     [user tile][T][H / 16][r, z, n, hn][64 lanes] 16-byte vectors
      backward  W_hh^T (H x 3H floats), dh (U x H floats, rounded up to 16 bytes), one chunk of the panel
                ([user tiles x 16 rows][Tc][4H] floats)
      table     packed W_ih^T (E x 3H floats), dX and the piece partials (U T E floats each), the inverted index (n_items,
                n_items + 1 and three times U T ints), every part rounded up to 256 bytes
    An undersized workspace would be an out-of-bounds write on the GPU."""
    from recnn_amd import _lib as L
    lib = L.load()
    n, s, b = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    n_items = 300
    for U, T in ((5, 1), (25, 37), (33, 70)):
        tiles, Tc = (U + 15) // 16, min(T, 32)
        assert lib.recnn_gru_workspace_bytes(U, T, H, 0, C.byref(n)) == 0 and n.value == 0
        assert lib.recnn_gru_workspace_bytes(U, T, H, 1, C.byref(n)) == 0
        assert n.value == tiles * Tc * (H // 16) * 3 * 64 * 16, (U, T, n.value)
        for variant in (0, 1):
            assert lib.recnn_gru_train_workspace_bytes(U, T, H, E, variant, C.byref(s), C.byref(b)) == 0
            assert s.value == tiles * T * (H // 16) * 4 * 64 * 16, (U, T, s.value)
            assert b.value == 12 * H * H + _round(4 * U * H, 16) + tiles * 16 * Tc * 4 * H * 4, (U, T, b.value)
        assert lib.recnn_gru_table_grad_workspace_bytes(U, T, H, E, n_items, C.byref(n)) == 0
        want = _round(12 * E * H, 256) + 2 * _round(4 * U * T * E, 256) + _round(4 * n_items, 256) + _round(4 * (n_items + 1), 256) \
            + 3 * _round(4 * U * T, 256)
        assert n.value == want, (U, T, n.value, want)


def test_unsupported_shapes_are_refused_with_a_message():
    from recnn_amd import _lib as L
    lib = L.load()
    n, s, b = C.c_int64(), C.c_int64(), C.c_int64()
    for E in (4, 12, 136):
        assert lib.recnn_gru_train_workspace_bytes(33, 70, 144, E, 1, C.byref(s), C.byref(b)) != 0
        err = lib.recnn_last_error()
        assert b"gru_train_workspace_bytes" in err and b"emb_dim" in err and str(E).encode() in err
        assert lib.recnn_gru_table_grad_workspace_bytes(33, 70, 144, E, 50, C.byref(n)) != 0
        err = lib.recnn_last_error()
        assert b"gru_table_grad_workspace_bytes" in err and b"emb_dim" in err and str(E).encode() in err
    for H in (8, 24, 272):
        assert lib.recnn_gru_workspace_bytes(33, 70, H, 1, C.byref(n)) != 0
        assert b"gru_workspace_bytes" in lib.recnn_last_error() and b"hidden" in lib.recnn_last_error()
        assert lib.recnn_gru_train_workspace_bytes(33, 70, H, 72, 1, C.byref(s), C.byref(b)) != 0
        err = lib.recnn_last_error()
        assert b"gru_train_workspace_bytes" in err and b"hidden" in err and str(H).encode() in err
    # the launching entry points check their pointers first and the shapes next, both before any launch
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for E, H, word in ((12, 16, b"emb_dim"), (136, 16, b"emb_dim"), (8, 24, b"hidden"), (8, 272, b"hidden")):
        for train in (False, True):
            fn = lib.recnn_gru_encode_train if train else lib.recnn_gru_encode
            tail = (0, None, p, None) if train else (0, None, None)
            assert fn(p, p, p, p, 4, 0, 3, p, 10, E, H, p, p, p, p, None, p, p, *tail) != 0
            err = lib.recnn_last_error()
            assert b"gru_encode" in err and word in err, err
        assert lib.recnn_gru_backward(p, p, p, p, 4, 0, 3, p, 10, E, H, p, p, p, None, None, None, *([None] * 5), p, None) != 0
        assert b"gru_backward" in lib.recnn_last_error() and word in lib.recnn_last_error()
    assert lib.recnn_gru_encode(*([None] * 4), 4, 0, 3, None, 10, 8, 16, *([None] * 7), 0, None, None) != 0
    assert b"gru_encode" in lib.recnn_last_error() and b"null" in lib.recnn_last_error()
    assert lib.recnn_gru_backward(*([None] * 4), 4, 0, 3, None, 10, 8, 16, *([None] * 13)) != 0
    assert b"gru_backward" in lib.recnn_last_error() and b"null" in lib.recnn_last_error()
    assert lib.recnn_gru_backward_table(p, p, p, p, 4, 0, 3, p, 10, 8, 16, *([p] * 5), *([None] * 8), p, p, None) != 0
    assert b"d_table" in lib.recnn_last_error()


def test_host_refusals_by_name():
    from recnn_amd import _lib as L
    from recnn_amd.data.env import SeqEnv
    from recnn_amd.nn import functional as F
    table = torch.zeros(20, 8)
    with pytest.raises(L.RecnnHipError, match="weight_ih_l0.device"):                      # a CPU module
        F.gru_encode(torch.nn.GRU(9, 16), None, table, [0, 1], 4)
    with pytest.raises(L.RecnnHipError, match="weight_ih_l0.device"):
        F.gru_encode_train(torch.nn.GRU(9, 16), None, table, [0, 1], 4)
    for kw, attr in ((dict(num_layers=2), "num_layers"), (dict(bidirectional=True), "bidirectional"), (dict(bias=False), "bias"),
                     (dict(num_layers=1, dropout=0.5), "dropout")):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            bad = torch.nn.GRU(9, 16, **kw)
        for fn in (F.gru_encode, F.gru_encode_train):
            with pytest.raises(L.RecnnHipError, match=attr):
                fn(bad, None, table, [0, 1], 4)
    # the other cell: the same attribute names, another number of weight rows -- refused by type, pointing at the right call
    for fn in (F.lstm_encode, F.lstm_encode_train):
        with pytest.raises(L.RecnnHipError, match=r"torch\.nn\.modules\.rnn\.GRU.*gru_encode"):
            fn(torch.nn.GRU(9, 16), None, table, [0, 1], 4)
    for fn in (F.gru_encode, F.gru_encode_train):
        with pytest.raises(L.RecnnHipError, match=r"torch\.nn\.modules\.rnn\.LSTM.*lstm_encode"):
            fn(torch.nn.LSTM(9, 16), None, table, [0, 1], 4)
        with pytest.raises(L.RecnnHipError, match="RNN"):
            fn(torch.nn.RNN(9, 16), None, table, [0, 1], 4)
    with pytest.raises(L.RecnnHipError, match="table.requires_grad"):
        F.gru_encode_train(torch.nn.GRU(9, 16), None, table.clone().requires_grad_(True), [0, 1], 4)
    tbl, user_dict, users, _ = R.seq_env_data()
    with pytest.raises(TypeError, match=r"torch\.nn\.modules\.rnn\.RNN"):
        SeqEnv.from_user_dict(tbl, user_dict, users, state_encoder=torch.nn.RNN(9, 16), batch_size=5, max_buf_size=20, device="cpu")
    with pytest.raises(TypeError, match="Linear"):
        SeqEnv(None, torch.nn.Linear(9, 16))
