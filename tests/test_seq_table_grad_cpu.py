"""The embedding-table gradient of the LSTM state encoder, host side (no GPU): the reference helper's float64 autograd gradient
against the hand-written index_add of da . W_ih[:, :E], the host-only workspace query of the table gradient against its layout
written out by hand, and the default call's refusal of a table that requires grad."""
import ctypes as C

import pytest
import torch

import seq_grad_reference as G
import seq_table_grad_reference as TG
from helpers import make_store


def test_hand_written_table_gradient_matches_float64_autograd():
    E, H, U, T = 8, 16, 3, 5
    items, ratings, table = make_store(U, 40, E, T + 1, T + 3, seed=2)
    torch.manual_seed(2)
    lstm = torch.nn.LSTM(E + 1, H)
    tbl = TG.extended_table(table, seed=2)
    idx, rts = TG.positions(items, ratings, T)
    g = torch.Generator().manual_seed(7)
    h0c0 = (torch.randn(U, H, generator=g) * 0.5, torch.randn(U, H, generator=g) * 0.5)
    Rw = G.loss_weights(U, T, H, seed=3)
    ref = TG.cpu_table_grads(lstm, tbl, idx, rts, h0c0, Rw, torch.float64)
    hand = TG.table_grad_by_hand(lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, tbl, idx, rts, *h0c0, Rw)
    err, scale = float((hand - ref["table"]).abs().max()), float(ref["table"].abs().max())
    print(f"hand table gradient vs float64 autograd: err {err:.3e} of {scale:.3e}")
    assert ref["table"].shape == tbl.shape and scale > 0
    assert err <= 1e-13 * max(scale, 1.0)                             # two float64 evaluations of the same sums
    assert bool((ref["table"][-TG.EXTRA_ROWS:] == 0).all()) and bool((hand[-TG.EXTRA_ROWS:] == 0).all())
    # the weights' gradients are those of the helper this one extends
    x = torch.cat([tbl[idx], rts[..., None]], 2)
    old = G.cpu_grads(lstm, x, h0c0, Rw, torch.float64)
    assert all(torch.equal(old[n], ref[n]) for n in G.NAMES)
    bounds, g64, d32 = TG.table_grad_bounds(lstm, tbl, idx, rts, h0c0, Rw)
    assert bounds["table"] > 0 and torch.equal(g64["table"], ref["table"]) and bounds["table"] >= 4.0 * d32["table"]


def test_training_case_with_table_is_chosen_on_the_float64_restatement():
    *_, lr, losses = TG.training_case_with_table()
    assert len(losses) == G.TRAIN_SGD_STEPS + 1 and losses[-1] <= 0.9 * losses[0] and lr > 0
    assert all(b < a for a, b in zip(losses, losses[1:]))


def _by_hand(U, T, H, E, n_items):
    """The table gradient's workspace, written out: the packed transpose of W_ih[:, 0:E] (E x 4H floats), dX of the whole call
    (U T E floats), the inverted index (counts [n_items], starts [n_items + 1], and three int arrays of U T: arrival slots, lists in
    arrival order, lists in contribution order), the piece partials (U T E floats); each rounded up to 256 bytes."""
    r = lambda b: (b + 255) // 256 * 256
    M = U * T
    return r(4 * E * 4 * H) + r(4 * M * E) + r(4 * n_items) + r(4 * (n_items + 1)) + 3 * r(4 * M) + r(4 * M * E)


def test_table_grad_workspace_query_is_host_only_and_validates():
    from recnn_amd import _lib as L
    lib = L.load()
    b = C.c_int64(-1)
    for E, H, U, T, n in ((8, 16, 5, 37, 312), (24, 48, 33, 70, 312), (72, 144, 17, 65, 312), (128, 256, 25, 37, 312),
                          (120, 128, 20, 40, 312), (128, 256, 256, 1000, 26744), (8, 16, 1, 1, 1), (8, 16, 0, 0, 5)):
        assert lib.recnn_lstm_table_grad_workspace_bytes(U, T, H, E, n, C.byref(b)) == 0
        assert b.value == _by_hand(U, T, H, E, n), (E, H, U, T, n, b.value)
    assert lib.recnn_lstm_table_grad_workspace_bytes(256, 1000, 256, 128, 26744, C.byref(b)) == 0
    assert b.value >= 2 * 4 * 256 * 1000 * 128                        # dX and the partials: 131 MB each at this shape
    for E in (12, 136):
        assert lib.recnn_lstm_table_grad_workspace_bytes(33, 70, 144, E, 312, C.byref(b)) != 0
        err = lib.recnn_last_error()
        assert b"lstm_table_grad_workspace_bytes" in err and b"emb_dim" in err and str(E).encode() in err
    for H in (24, 272):
        assert lib.recnn_lstm_table_grad_workspace_bytes(33, 70, H, 72, 312, C.byref(b)) != 0
        err = lib.recnn_last_error()
        assert b"lstm_table_grad_workspace_bytes" in err and b"hidden" in err and str(H).encode() in err
    for bad in ((-1, 70, 144, 72, 312), (33, -1, 144, 72, 312), (33, 70, 144, 72, 0), (1 << 16, 1 << 15, 144, 72, 312)):
        assert lib.recnn_lstm_table_grad_workspace_bytes(*bad, C.byref(b)) != 0
        assert b"lstm_table_grad_workspace_bytes" in lib.recnn_last_error()
    assert lib.recnn_lstm_table_grad_workspace_bytes(33, 70, 144, 72, 312, None) != 0
    assert b"null" in lib.recnn_last_error()


def test_backward_table_refuses_bad_arguments_before_any_launch():
    from recnn_amd import _lib as L
    lib = L.load()
    assert lib.recnn_lstm_backward_table(*([None] * 4), 4, 0, 3, None, 10, 8, 16, *([None] * 18)) != 0
    assert b"lstm_backward_table" in lib.recnn_last_error() and b"null" in lib.recnn_last_error()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    # d_table set, everything else missing: the shared checks of recnn_lstm_backward answer
    assert lib.recnn_lstm_backward_table(*([None] * 4), 4, 0, 3, None, 10, 8, 16, *([None] * 14), p, None, None, None) != 0
    assert b"lstm_backward" in lib.recnn_last_error() and b"null" in lib.recnn_last_error()


def test_default_call_still_refuses_a_table_that_requires_grad():
    from recnn_amd import _lib as L
    from recnn_amd.nn import functional as F
    _, _, table = make_store(4, 30, 8, 12, 14, seed=1)
    with pytest.raises(L.RecnnHipError, match="table.requires_grad"):
        F.lstm_encode_train(torch.nn.LSTM(9, 16), None, torch.from_numpy(table).requires_grad_(True), [0, 1], 4)
    with pytest.raises(L.RecnnHipError, match="train_table=True"):
        F.lstm_encode_train(torch.nn.LSTM(9, 16), None, torch.from_numpy(table).requires_grad_(True), [0, 1], 4, train_table=False)
