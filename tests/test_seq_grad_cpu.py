"""Training the LSTM state encoder, host side (no GPU): the no-fallback refusals of the new entry points, the host-only
workspace query of csrc/lstm.hip, and the reference helper's float64 autograd gradients against a hand-written BPTT of the
equations the reverse-chain kernel is written from."""
import ctypes as C

import numpy as np
import pytest
import torch

import seq_grad_reference as G
import seq_reference as R
from helpers import csr, make_store


def test_hand_written_bptt_matches_float64_autograd():
    E, H, U, T = 8, 16, 3, 5
    items, ratings, table = make_store(U, 40, E, T + 1, T + 3, seed=2)
    torch.manual_seed(2)
    lstm = torch.nn.LSTM(E + 1, H)
    x = R.lstm_inputs(torch.from_numpy(table), items, ratings, T)
    g = torch.Generator().manual_seed(7)
    h0c0 = (torch.randn(U, H, generator=g) * 0.5, torch.randn(U, H, generator=g) * 0.5)
    Rw = G.loss_weights(U, T, H, seed=3)
    ref = G.cpu_grads(lstm, x, h0c0, Rw, torch.float64)
    hand = G.bptt_by_hand(lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, x, *h0c0, Rw)
    assert set(ref) == set(G.NAMES) == set(hand)
    for n in G.NAMES:
        err, scale = float((hand[n] - ref[n]).abs().max()), float(ref[n].abs().max())
        print(f"hand BPTT vs float64 autograd {n}: err {err:.3e} of {scale:.3e}")
        assert scale > 0 and err <= 1e-12 * max(scale, 1.0)         # two float64 evaluations of the same sums
    bounds, g64 = G.grad_bounds(lstm, x, h0c0, Rw)
    assert all(bounds[n] > 0 for n in G.NAMES) and all(torch.equal(g64[n], ref[n]) for n in G.NAMES)


def test_training_case_is_chosen_on_the_float64_restatement():
    *_, lr, losses = G.training_case()
    assert len(losses) == G.TRAIN_SGD_STEPS + 1 and losses[-1] <= 0.9 * losses[0] and lr > 0


def test_train_workspace_query_is_host_only_and_validates():
    from recnn_amd import _lib as L
    lib = L.load()
    s, b = C.c_int64(-1), C.c_int64(-1)
    assert lib.recnn_lstm_train_workspace_bytes(25, 37, 256, 128, 1, C.byref(s), C.byref(b)) == 0
    assert s.value == 5 * 32 * 37 * 256 * 4                           # i, f, g, o, c per (user of two 16-user tiles, step, unit)
    assert b.value == 4 * (256 * 1024 + 2 * 25 * 256 + 32 * 32 * 1024)  # W_hh^T, dh and dc, one 32-step chunk of da
    s2, b2 = C.c_int64(), C.c_int64()
    assert lib.recnn_lstm_train_workspace_bytes(5, 1, 16, 8, 0, C.byref(s2), C.byref(b2)) == 0
    assert s2.value == 5 * 16 * 1 * 16 * 4 and b2.value == 4 * (16 * 64 + 2 * 5 * 16 + 16 * 1 * 64)
    assert lib.recnn_lstm_train_workspace_bytes(0, 0, 16, 8, 0, C.byref(s2), C.byref(b2)) == 0 and s2.value == 0
    for bad in ((25, 37, 250, 128, 1), (25, 37, 256, 130, 1), (25, 37, 512, 128, 1), (-1, 37, 256, 128, 1), (25, -1, 256, 128, 0),
                (25, 37, 256, 128, 2)):
        assert lib.recnn_lstm_train_workspace_bytes(*bad, C.byref(s2), C.byref(b2)) != 0
        assert b"lstm_train_workspace_bytes" in lib.recnn_last_error()
    assert lib.recnn_lstm_train_workspace_bytes(25, 37, 256, 128, 1, None, C.byref(b2)) != 0
    assert b"null" in lib.recnn_last_error()


def test_train_workspaces_at_the_in_between_shapes():
    """Both training workspaces against the layouts seq_chain.h (`saved`) and seq_bwd.h (`bwd_ws`) document, written out, at the
    shapes tests/test_gpu_seq_shapes.py launches.  An undersized workspace would be an out-of-bounds write on the GPU.
      saved     [user tile][T][H / 16][i, f, g, o, c][64 lanes] 16-byte vectors
      backward  W_hh^T (H x 4H floats), dh and dc (U x H floats each, rounded up to 16 bytes), one chunk of da
                ([user tiles x 16 rows][min(T, 32) steps][4H] floats)"""
    from recnn_amd import _lib as L
    lib = L.load()
    s, b = C.c_int64(-1), C.c_int64(-1)
    for E, H in R.SWEEP_SHAPES:
        for U, T, _ in R.SWEEP_CASES:
            tiles = (U + 15) // 16
            state = (4 * U * H + 15) // 16 * 16                       # dh or dc: U x H floats, rounded up to 16 bytes
            for variant in (0, 1):
                assert lib.recnn_lstm_train_workspace_bytes(U, T, H, E, variant, C.byref(s), C.byref(b)) == 0
                assert s.value == tiles * T * (H // 16) * 5 * 64 * 16, (E, H, U, T, s.value)
                assert b.value == 16 * H * H + 2 * state + tiles * 16 * min(T, 32) * 16 * H, (E, H, U, T, b.value)
    for E in (4, 12, 136):
        assert lib.recnn_lstm_train_workspace_bytes(33, 70, 144, E, 1, C.byref(s), C.byref(b)) != 0
        err = lib.recnn_last_error()
        assert b"lstm_train_workspace_bytes" in err and b"emb_dim" in err and str(E).encode() in err
    for H in (8, 24, 272):
        assert lib.recnn_lstm_train_workspace_bytes(33, 70, H, 72, 1, C.byref(s), C.byref(b)) != 0
        err = lib.recnn_last_error()
        assert b"lstm_train_workspace_bytes" in err and b"hidden" in err and str(H).encode() in err


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    from recnn_amd import _lib as L
    lib = L.load()
    assert lib.recnn_lstm_encode_train(*([None] * 4), 4, 0, 3, None, 10, 8, 16, *([None] * 9), 0, None, None, None) != 0
    assert b"lstm_encode_train" in lib.recnn_last_error() and b"null" in lib.recnn_last_error()
    assert lib.recnn_lstm_backward(*([None] * 4), 4, 0, 3, None, 10, 8, 16, *([None] * 15)) != 0
    assert b"lstm_backward" in lib.recnn_last_error() and b"null" in lib.recnn_last_error()
    assert lib.recnn_seq_collect_bwd(None, None, 4, 5, 16, None, 2, None, None) != 0
    assert b"seq_collect_bwd" in lib.recnn_last_error()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    steps = C.cast((C.c_int32 * 2)(1, 2), C.c_void_p)
    assert lib.recnn_seq_collect_bwd(None, None, 4, 5, 6, steps, 2, p, None) != 0 and b"multiple of 4" in lib.recnn_last_error()
    off = C.c_void_p(p.value + 4)
    assert lib.recnn_seq_collect_bwd(off, None, 4, 5, 16, steps, 2, p, None) != 0 and b"align" in lib.recnn_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_training_entry_points_fail_loudly_without_a_gpu():
    from recnn_amd import _lib as L
    from recnn_amd.data.env import SeqEnv
    from recnn_amd.data.store import ReplayStore
    from recnn_amd.nn import functional as F
    items, ratings, table = make_store(4, 30, 8, 12, 14, seed=1)
    lstm = torch.nn.LSTM(9, 16)
    try:
        store = ReplayStore.from_arrays(*csr(items, ratings), torch.device("cpu"))
    except L.RecnnHipError:
        store = None                                              # (a store that refuses the CPU is as loud)
    with pytest.raises(L.RecnnHipError):
        F.lstm_encode_train(lstm, store, torch.from_numpy(table), [0, 1], 4)
    with pytest.raises(L.RecnnHipError):
        F.seq_collect_rows(torch.zeros(2, 5, 16, requires_grad=True), [1, 2], store, torch.from_numpy(table), [0, 1])
    tbl, user_dict, users, enc = R.seq_env_data()
    with pytest.raises(L.RecnnHipError):
        env = SeqEnv.from_user_dict(tbl, user_dict, users, state_encoder=enc, batch_size=5, max_buf_size=20, device="cpu")
        env.user_batch(users[:5], [3, 4, 9])
