"""Dynamic-length path, host side (no GPU): padder, ReplayBuffer, the recnn shim, the no-fallback refusals and the error paths of
the C ABI of csrc/seq.hip and csrc/lstm.hip (which return before any launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

from seq_reference import SWEEP_CASES, SWEEP_SHAPES, padder_ref


def _users(lengths, seed=0):
    rng = np.random.default_rng(seed)
    return [{"items": rng.integers(1, 90, size=L).astype(np.int64), "rates": rng.standard_normal(L), "sizes": L, "users": 100 + i}
            for i, L in enumerate(lengths)]


def test_padder_matches_pad_sequence():
    from recnn_amd.data import utils
    x = _users([11, 12, 30, 11])
    got, ref = utils.padder(x), padder_ref(x)
    assert got["items"].dtype == torch.int64 and got["ratings"].dtype == torch.float32 and got["sizes"].dtype == torch.float32
    assert got["items"].shape == (4, 30) and got["ratings"].shape == (4, 30)
    assert torch.equal(got["items"], ref["items"]) and torch.equal(got["ratings"], ref["ratings"])
    assert torch.equal(got["sizes"], torch.tensor([11., 12., 30., 11.])) and got["users"] == [100, 101, 102, 103]
    assert got["items"].device.type == "cpu"
    for i, L in enumerate([11, 12, 30, 11]):
        assert not got["items"][i, L:].any() and not got["ratings"][i, L:].any()
        assert torch.equal(got["items"][i, :L], torch.from_numpy(x[i]["items"]))


def test_replay_buffer_on_cpu():
    from recnn_amd.data.utils import ReplayBuffer
    layout = [torch.Size([10, 4]), torch.Size([10, 2]), torch.Size([10, 1]), torch.Size([10, 4])]
    buf = ReplayBuffer(10, layout, device="cpu")
    assert buf.len() == 0 and buf.meta["step"] == []
    mk = lambda n, v: {"state": torch.full((n, 4), v), "action": torch.full((n, 2), v + 1), "reward": torch.full((n, 1), v + 2),
                       "next_state": torch.full((n, 4), v + 3), "step": int(v)}
    buf.append(mk(3, 1.0))
    buf.append(mk(4, 5.0))
    assert buf.len() == 7 and buf.meta["step"] == [1, 5]
    g = buf.get()
    assert set(g) == {"state", "action", "reward", "next_state", "meta"} and g["meta"] is buf.meta
    assert [tuple(g[k].shape) for k in ("state", "action", "reward", "next_state")] == [(10, 4), (10, 2), (10, 1), (10, 4)]
    assert (g["state"][:3] == 1).all() and (g["state"][3:7] == 5).all() and not g["state"][7:].any()
    assert (g["action"][3:7] == 6).all() and (g["reward"][:3] == 3).all() and (g["next_state"][3:7] == 8).all()
    assert not g["action"][7:].any() and not g["reward"][7:].any() and not g["next_state"][7:].any()
    with pytest.raises(ValueError, match=r"4 rows .* 7 of 10"):
        buf.append(mk(4, 9.0))
    assert buf.len() == 7
    buf.append(mk(3, 9.0))
    assert buf.len() == 10
    buf.flush()
    assert buf.len() == 0 and buf.meta["step"] == [] and not buf.get()["state"].any()
    assert (g["state"][7:] == 9).all()          # a batch handed out before the flush keeps its rows
    lazy = ReplayBuffer(10, layout)             # no device: the first appended batch decides
    lazy.append(mk(2, 1.0))
    assert lazy.get()["state"].device.type == "cpu" and lazy.len() == 2


def test_recnn_shim_serves_the_new_names():
    import recnn
    import recnn_amd
    assert recnn.data.utils.padder is recnn_amd.data.utils.padder
    assert recnn.data.utils.prepare_batch_dynamic_size is recnn_amd.data.utils.prepare_batch_dynamic_size
    assert recnn.data.utils.ReplayBuffer is recnn_amd.data.utils.ReplayBuffer
    assert recnn.data.env.SeqEnv is recnn_amd.data.env.SeqEnv


def test_cpu_inputs_are_refused_not_emulated():
    from recnn_amd import _lib as L
    from recnn_amd.data import utils
    from recnn_amd.nn import functional as F
    batch = utils.padder(_users([11, 12]))
    with pytest.raises(L.RecnnHipError):
        utils.prepare_batch_dynamic_size(batch, torch.zeros(100, 8))
    with pytest.raises(L.RecnnHipError, match="weight_ih_l0.device"):
        F.lstm_encode(torch.nn.LSTM(9, 16), None, torch.zeros(100, 8), [0], 4)


def test_seq_abi_error_paths_launch_nothing():
    from recnn_amd import _lib as L
    lib = L.load()
    p = C.c_void_p(4096)                       # any non-null, aligned address: the checks return before it is looked at
    assert lib.recnn_seq_gather(None, None, None, None, 4, 8, None, 10, 8, None, None, None, None) != 0
    assert b"seq_gather" in lib.recnn_last_error() and b"null" in lib.recnn_last_error()
    assert lib.recnn_seq_gather_idx(None, 8, None, 10, 8, None, None) != 0
    assert b"null" in lib.recnn_last_error()
    assert lib.recnn_seq_collect(None, 4, 8, 16, None, 1, None, None, None, None, None, 10, 8, None, None, None, None, None) != 0
    assert b"null" in lib.recnn_last_error()
    enc = lambda E, H, w=p: lib.recnn_lstm_encode(p, p, p, p, 4, 0, 8, p, 10, E, H, w, p, p, p, None, None, p, p, p, 0, None, None)
    assert enc(8, 16, None) != 0 and b"null" in lib.recnn_last_error()
    assert enc(8, 24) != 0 and b"hidden" in lib.recnn_last_error() and b"24" in lib.recnn_last_error()
    assert enc(12, 16) != 0 and b"emb_dim" in lib.recnn_last_error() and b"12" in lib.recnn_last_error()
    assert enc(136, 16) != 0 and enc(8, 272) != 0
    n = C.c_int64(-1)
    assert lib.recnn_lstm_workspace_bytes(25, 1000, 256, 0, C.byref(n)) == 0 and n.value == 0
    assert lib.recnn_lstm_workspace_bytes(25, 1000, 256, 1, C.byref(n)) == 0 and n.value == 2 * 32 * 1024 * 16 * 4
    assert lib.recnn_lstm_workspace_bytes(25, 1000, 24, 1, C.byref(n)) != 0


def test_encode_workspace_at_the_in_between_shapes():
    """The projection workspace against the layout seq_chain.h documents for `pre`, written out: [user tile][min(T, 32) steps][H / 16
    hidden tiles][4 gates][64 lanes] 16-byte vectors.  An undersized workspace would be an out-of-bounds write on the GPU."""
    from recnn_amd import _lib as L
    lib = L.load()
    n = C.c_int64(-1)
    for _, H in SWEEP_SHAPES:
        for U, T, _ in SWEEP_CASES:
            tiles = (U + 15) // 16
            assert lib.recnn_lstm_workspace_bytes(U, T, H, 1, C.byref(n)) == 0
            assert n.value == tiles * min(T, 32) * (H // 16) * 4 * 64 * 16, (U, T, H, n.value)
            assert lib.recnn_lstm_workspace_bytes(U, T, H, 0, C.byref(n)) == 0 and n.value == 0
    for H in (8, 24, 272):                     # (this query takes no embedding width: the training query's, which does, refuses E by name too)
        assert lib.recnn_lstm_workspace_bytes(33, 70, H, 1, C.byref(n)) != 0
        assert b"lstm_workspace_bytes" in lib.recnn_last_error() and b"hidden" in lib.recnn_last_error()


def _tiny_env(**kw):
    from recnn_amd.data.env import SeqEnv
    rng = np.random.default_rng(0)
    user_dict = {u: {"items": rng.integers(0, 20, size=12).astype(np.int64), "ratings": rng.standard_normal(12).astype(np.float32)}
                 for u in range(4)}
    return SeqEnv.from_user_dict(torch.zeros(20, 8), user_dict, [0, 1, 2, 3], state_encoder=torch.nn.LSTM(9, 16), batch_size=2,
                                 max_buf_size=10, **kw)


def test_seq_env_refuses_a_layout_that_does_not_fit_encoder_and_table():
    """The collect kernel writes rows of H, E, 1, H floats: the reference's hard-coded 256 / 128 layout over an H = 16, E = 8 env, or
    tensors of unequal row counts, are refused at construction with the sizes named."""
    n = 10
    with pytest.raises(ValueError, match=r"256.*hidden_size = 16, embedding width = 8"):
        _tiny_env(layout=[torch.Size([n, 256]), torch.Size([n, 128]), torch.Size([n, 1]), torch.Size([n, 256])])
    with pytest.raises(ValueError, match="layout"):
        _tiny_env(layout=[torch.Size([n, 16]), torch.Size([n, 8]), torch.Size([n - 1, 1]), torch.Size([n, 16])])
    with pytest.raises(ValueError, match="layout"):
        _tiny_env(layout=[torch.Size([n, 16]), torch.Size([n, 4]), torch.Size([n, 1]), torch.Size([n, 16])])
    env = _tiny_env(layout=[torch.Size([n, 16]), torch.Size([n, 8]), torch.Size([n]), torch.Size([n, 16])])
    assert env.train_buffer.capacity == n
    assert [tuple(i) for i in _tiny_env().buffer_layout] == [(10, 16), (10, 8), (10, 1), (10, 16)]


def test_seq_collect_checks_its_destinations_before_anything_else():
    from recnn_amd.nn import functional as F
    U, T, H, E = 3, 6, 16, 8
    h, table = torch.zeros(U, T, H), torch.zeros(20, E)
    good = lambda rows=2 * U: [torch.zeros(rows, H), torch.zeros(rows, E), torch.zeros(rows, 1), torch.zeros(rows, H)]
    cases = {"state": (0, torch.zeros(2 * U, 256)), "action": (1, torch.zeros(2 * U, 4)), "reward": (2, torch.zeros(2 * U - 1, 1)),
             "next_state": (3, torch.zeros(2 * U, H, dtype=torch.float64)), "action ": (1, torch.zeros(2 * U, 2 * E)[:, ::2])}
    for name, (i, bad) in cases.items():
        views = good()
        views[i] = bad
        with pytest.raises(ValueError, match=rf"seq_collect: {name.strip()} .*2 steps x 3 users, H = 16, E = 8"):
            F.seq_collect(h, [1, 4], None, table, [0, 1, 2], views)
    with pytest.raises(ValueError, match="rows|shape"):
        F.seq_collect(h, [1, 4], None, table, [0, 1, 2], good(rows=U))           # rows for one step, two asked
    with pytest.raises(ValueError, match="steps must lie"):
        F.seq_collect(h, [0, 4], None, table, [0, 1, 2], good())
    with pytest.raises(ValueError, match="slots"):
        F.seq_collect(h, [1, 4], None, table, [0, 1], good())


def test_replay_buffer_capacity_is_the_shortest_tensor():
    from recnn_amd.data.utils import ReplayBuffer
    buf = ReplayBuffer(10, [torch.Size([10, 4]), torch.Size([10, 2]), torch.Size([6, 1]), torch.Size([10, 4])], device="cpu")
    assert buf.capacity == 6 and buf.room(6) and not buf.room(7)
    with pytest.raises(ValueError, match="7 rows .* 0 of 6"):
        buf.reserve(7)


def test_seq_env_generators_refuse_an_empty_dataset():
    env = _tiny_env()                      # from_user_dict: test_users defaults to ()
    with pytest.raises(ValueError, match="empty"):
        next(env.test_batch())


def test_slots_are_range_checked_on_the_host():
    from recnn_amd.data.store import ReplayStore
    off = np.array([0, 4, 9, 12], dtype=np.int64)
    st = ReplayStore.from_arrays(np.arange(12), np.zeros(12), off, torch.device("cpu"))
    assert st.checked_slots([2, 0], "t").dtype == np.int32
    for bad in ([-1, 0], [0, 3], [[0, 1]], [0.5]):
        with pytest.raises(ValueError, match="slots"):
            st.checked_slots(bad, "t")
    with pytest.raises(ValueError, match="lives on"):
        st.checked_slots([0], "t", torch.device("cuda:0"))
