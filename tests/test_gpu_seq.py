"""Dynamic-length path on the GPU (csrc/seq.hip, csrc/lstm.hip): padded gathers, the LSTM encode against torch.nn.LSTM in float64 on the CPU, and
SeqEnv end to end against the same loop over that reference (tests/seq_reference.py).

The encode bound comes from the reference alone: 4 x max |LSTM_fp32_cpu - LSTM_fp64_cpu| on the same inputs, floored at 1e-6
(seq_reference.fp32_bound).  Every test prints its measured error next to the bound before it asserts."""
import numpy as np
import pytest
import torch

import seq_reference as R
from helpers import csr, make_store

pytestmark = pytest.mark.gpu

T_MAX = 37


def _store(cuda, items, ratings):
    from recnn_amd.data.store import ReplayStore
    return ReplayStore.from_arrays(*csr(items, ratings), cuda)


@pytest.fixture(scope="module")
def seq_data():
    """Per E: 25 users with at least T_MAX + 1 elements, their table and an LSTM(E + 1, H) (CPU master copies)."""
    out = {}
    for E, H in ((8, 16), (128, 256)):
        items, ratings, table = make_store(25, 300, E, T_MAX + 1, T_MAX + 9, seed=E)
        torch.manual_seed(E)
        out[(E, H)] = (items, ratings, torch.from_numpy(table), torch.nn.LSTM(E + 1, H))
    return out


def _on_gpu(cuda, data):
    items, ratings, table, lstm = data
    gl = torch.nn.LSTM(lstm.input_size, lstm.hidden_size).to(cuda)
    gl.load_state_dict(lstm.state_dict())
    return _store(cuda, items, ratings), table.to(cuda), gl


# ---------------------------------------------------------------------------------------------------- padded gather
@pytest.mark.parametrize("E", [8, 128])
def test_padded_gather_is_a_bit_exact_copy(cuda, E):
    from recnn_amd.data import utils
    from recnn_amd.data.env import UserDataset
    items, ratings, table = make_store(5, 200, E, 5, 20, seed=3)
    items[1], ratings[1] = items[1][:7], ratings[1][:7]
    lmax = 21                                               # odd, not a multiple of 4
    items[3] = np.resize(items[3], lmax)
    ratings[3] = np.resize(ratings[3], lmax)
    assert max(len(i) for i in items) == lmax and min(len(i) for i in items) < lmax
    user_dict = {u: {"items": items[u], "ratings": ratings[u]} for u in range(5)}
    order = [3, 0, 4, 1, 2]
    ds = UserDataset(order, user_dict)
    x = [ds[i] for i in range(5)]
    tbl = torch.from_numpy(table)
    ref = R.dynamic_ref(R.padder_ref(x), tbl)
    # the collate: padder on the host, rows through the pre-padded-index kernel
    got = utils.prepare_batch_dynamic_size(utils.padder(x), tbl.to(cuda))
    assert got["items"].is_cuda and got["items"].shape == (5, lmax, E)
    assert torch.equal(got["items"].cpu(), ref["items"]) and torch.equal(got["ratings"], ref["ratings"])
    assert torch.equal(got["sizes"], ref["sizes"]) and got["users"] == order
    # straight from the CSR store
    st = _store(cuda, items, ratings)
    ids, rts, rows = utils.gather_padded(st, tbl.to(cuda), np.asarray(order, dtype=np.int32))
    pad = R.padder_ref(x)
    assert ids.dtype == torch.int64 and torch.equal(ids.cpu(), pad["items"])
    assert torch.equal(rts.cpu(), pad["ratings"]) and torch.equal(rows.cpu(), ref["items"])
    assert torch.equal(rows, got["items"])
    for i, u in enumerate(order):
        L = len(items[u])
        if L < lmax:
            assert torch.equal(rows[i, L:].cpu(), tbl[0].expand(lmax - L, E))


# ---------------------------------------------------------------------------------------------------- encode
@pytest.mark.parametrize("U", [1, 16, 17, 25])
@pytest.mark.parametrize("EH", [(8, 16), (128, 256)])
def test_encode_against_float64(cuda, seq_data, EH, U):
    from recnn_amd.nn import functional as F
    items, ratings, table, lstm = seq_data[EH]
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    slots = np.arange(25 - U, 25, dtype=np.int32)           # not the first users: slots are looked up, not assumed
    cases = [(T, None) for T in (1, 2, T_MAX)]
    g = torch.Generator().manual_seed(U)
    cases.append((T_MAX, (torch.randn(U, EH[1], generator=g) * 0.5, torch.randn(U, EH[1], generator=g) * 0.5)))
    for T, hc in cases:
        x = R.lstm_inputs(table, [items[s] for s in slots], [ratings[s] for s in slots], T)
        bounds, ref = R.fp32_bound(lstm, x, hc)
        res = {}
        for variant in ("fused", "chunked"):
            F.set_lstm_variant(variant)
            try:
                h, (hT, cT) = F.lstm_encode(gl, st, tbl, slots, T, None if hc is None else tuple(t.to(cuda) for t in hc))
            finally:
                F.set_lstm_variant("chunked")
            res[variant] = (h.cpu(), hT.cpu(), cT.cpu())
            assert h.shape == (U, T, EH[1]) and hT.shape == (U, EH[1]) and torch.equal(h[:, -1], hT)
            errs = [float((a.double() - b).abs().max()) for a, b in zip(res[variant], ref)]
            print(f"encode E,H={EH} U={U} T={T} h0={'set' if hc else 'zero'} {variant}: err h/hT/cT "
                  + " ".join(f"{e:.3e}" for e in errs) + " bounds " + " ".join(f"{b:.3e}" for b in bounds))
            for e, b in zip(errs, bounds):
                assert e <= b, (variant, T, errs, bounds)
        for a, b in zip(res["fused"], res["chunked"]):
            assert torch.equal(a, b)                        # the two schedules sum in the same fixed order


def test_carry_independence_and_live_weights(cuda, seq_data):
    from recnn_amd.nn import functional as F
    EH = (128, 256)
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    slots = np.arange(17, dtype=np.int32)
    h, (hT, cT) = F.lstm_encode(gl, st, tbl, slots, T_MAX)
    # carry: 37 steps in one call == 20 + 17 with (h, c) carried over, bit for bit
    ha, hca = F.lstm_encode(gl, st, tbl, slots, 20)
    hb, (hTb, cTb) = F.lstm_encode(gl, st, tbl, slots, 17, hca, t0=20)
    assert torch.equal(torch.cat([ha, hb], 1), h) and torch.equal(hTb, hT) and torch.equal(cTb, cT)
    # independence: a permutation of the users permutes h; a user alone equals its row in the batch
    perm = np.random.default_rng(0).permutation(17)
    hp, (hTp, cTp) = F.lstm_encode(gl, st, tbl, slots[perm], T_MAX)
    pt = torch.from_numpy(perm).to(cuda)
    assert torch.equal(hp, h[pt]) and torch.equal(hTp, hT[pt]) and torch.equal(cTp, cT[pt])
    h1, (hT1, cT1) = F.lstm_encode(gl, st, tbl, slots[16:17], T_MAX)
    assert torch.equal(h1[0], h[16]) and torch.equal(hT1[0], hT[16]) and torch.equal(cT1[0], cT[16])
    # live weights: an in-place change of weight_hh_l0 shows in the next call
    with torch.no_grad():
        gl.weight_hh_l0.mul_(0.5)
    h2, _ = F.lstm_encode(gl, st, tbl, slots, T_MAX)
    assert torch.equal(h2[:, 0], h[:, 0]) and not torch.equal(h2[:, 1:], h[:, 1:])      # h_{-1} = 0: step 0 does not see W_hh
    with pytest.raises(ValueError, match="history"):
        F.lstm_encode(gl, st, tbl, slots, 60)


@pytest.mark.parametrize("kw,attr", [(dict(num_layers=2), "num_layers"), (dict(bidirectional=True), "bidirectional"),
                                     (dict(proj_size=8), "proj_size"), (dict(num_layers=1, dropout=0.5), "dropout"),
                                     (dict(bias=False), "bias")])
def test_unsupported_lstms_are_refused_by_name(cuda, seq_data, kw, attr):
    import warnings
    from recnn_amd import _lib as L
    from recnn_amd.nn import functional as F
    st, tbl, _ = _on_gpu(cuda, seq_data[(8, 16)])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lstm = torch.nn.LSTM(9, 16, **kw).to(cuda)
    with pytest.raises(L.RecnnHipError, match=attr):
        F.lstm_encode(lstm, st, tbl, [0, 1], 4)


# ---------------------------------------------------------------------------------------------------- SeqEnv
@pytest.fixture(scope="module")
def seq_env_case():
    table, user_dict, users, lstm = R.seq_env_data()
    np.random.seed(R.SEQ_ENV_SEED)
    ref, bound = R.seq_env_batches(table, user_dict, users, lstm, batch_size=5, max_buf_size=20, n_batches=3, max_epochs=2)
    return table, user_dict, users, lstm, ref, bound


def _env(cuda, case):
    from recnn_amd.data.env import SeqEnv
    table, user_dict, users, lstm = case[:4]
    gl = torch.nn.LSTM(lstm.input_size, lstm.hidden_size).to(cuda)
    gl.load_state_dict(lstm.state_dict())
    return SeqEnv.from_user_dict(table, user_dict, users, state_encoder=gl, batch_size=5, max_buf_size=20, device=cuda)


def test_seq_env_matches_the_reference_loop(cuda, seq_env_case):
    from recnn_amd.nn import functional as F
    ref, bound = seq_env_case[4:]
    assert len(ref) == 3 and all(len(r["meta"]["step"]) >= 1 for r in ref)      # the chosen seed keeps steps in every buffer
    assert any(r["meta"]["rows"] < 20 for r in ref)                                # ... and one is handed out because 5 more do not fit
    env = _env(cuda, seq_env_case)
    assert [tuple(s) for s in env.buffer_layout] == [(20, 16), (20, 8), (20, 1), (20, 16)]
    np.random.seed(R.SEQ_ENV_SEED)
    gen = env.train_batch()
    for k, want in enumerate(ref):
        got = next(gen)
        assert set(got) == {"state", "action", "reward", "next_state", "done", "meta"}
        m = got["meta"]
        assert m["step"] == want["meta"]["step"] and m["rows"] == want["meta"]["rows"] and list(m["users"]) == want["meta"]["users"]
        assert m["sizes"].cpu().tolist() == [float(s) for s in want["meta"]["sizes"]]
        rows = m["rows"]
        assert torch.equal(got["action"].cpu(), torch.from_numpy(want["action"]))
        assert torch.equal(got["reward"].cpu(), torch.from_numpy(want["reward"]))
        for key in ("state", "next_state"):
            err = float((got[key].cpu().double() - torch.from_numpy(want[key])).abs().max())
            print(f"SeqEnv batch {k} {key}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound
        for key in ("state", "action", "reward", "next_state", "done"):
            assert got[key].shape[0] == 20 and not got[key][rows:].any()
        assert not got["done"].any()
        # state of a kept step == next_state of the step before it, from a direct encode of that user batch (a buffer handed out
        # at 20 rows ends with rows of the users in meta; one handed out early already names the batch that did not fit)
        if rows < 20:
            continue
        U = len(m["users"])
        t = m["step"][-1]
        h, _ = F.lstm_encode(env.state_encoder, env.store, env.table, env.store.slots(m["users"]), t + 1)
        assert torch.equal(got["state"][rows - U:rows], h[:, t - 1]) and torch.equal(got["next_state"][rows - U:rows], h[:, t])


def test_seq_loader_yields_the_dynamic_collate(cuda, seq_env_case):
    from recnn_amd.data.env import UserDataset
    table, user_dict, users = seq_env_case[:3]
    env = _env(cuda, seq_env_case)
    assert len(env.train_dataloader) == 3
    ds = UserDataset(users, user_dict)
    for k, got in enumerate(env.train_dataloader):
        x = [ds[i] for i in range(5 * k, min(5 * k + 5, len(users)))]
        ref = R.dynamic_ref(R.padder_ref(x), table)
        assert torch.equal(got["items"].cpu(), ref["items"]) and torch.equal(got["ratings"].cpu(), ref["ratings"])
        assert torch.equal(got["sizes"], ref["sizes"]) and got["users"] == ref["users"]
        wrapped = env.prepare_batch_wrapper(x)
        assert torch.equal(wrapped["items"], got["items"])


def test_ddpg_update_runs_on_a_seq_env_batch(cuda, seq_env_case):
    import recnn
    env = _env(cuda, seq_env_case)
    np.random.seed(R.SEQ_ENV_SEED)
    batch = next(env.train_batch())
    torch.manual_seed(0)
    nets = {"value_net": recnn.nn.Critic(16, 8, 32).to(cuda), "target_value_net": recnn.nn.Critic(16, 8, 32).to(cuda).eval(),
            "policy_net": recnn.nn.Actor(16, 8, 32).to(cuda), "target_policy_net": recnn.nn.Actor(16, 8, 32).to(cuda).eval()}
    optimizer = {"policy_optimizer": torch.optim.Adam(nets["policy_net"].parameters(), lr=1e-4),
                 "value_optimizer": torch.optim.Adam(nets["value_net"].parameters(), lr=1e-4)}
    params = {"gamma": 0.99, "min_value": -10, "max_value": 10, "policy_step": 1, "soft_tau": 0.001}
    loss = recnn.nn.ddpg_update(batch, params, nets, optimizer, device=cuda, learn=True, step=0)
    assert np.isfinite(float(loss["value"])) and np.isfinite(float(loss["policy"]))
