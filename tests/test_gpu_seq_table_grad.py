"""Training the item embeddings through the LSTM state encoder on the GPU (csrc/seq_bwd.h, csrc/seq_grad.h): the table gradient of
`lstm_encode_train(..., train_table=True)` against torch.nn.LSTM under autograd in float64 on the CPU over cat([table[idx], rating])
(tests/seq_table_grad_reference.py), what must stay bit-equal, the carry across calls, `SeqEnv.user_batch(..., table=P)`, one
`ddpg_update` with P in the policy optimizer, and one small problem on which encoder AND table must actually learn.

The bound of a gradient tensor G comes from the reference alone: max(4 max |G32cpu - G64cpu|, 2^-23 max(8, sqrt(U T)) max |G64|).
Every case first asserts its preconditions from the float64 reference (rows nothing reaches, rows that are real sums, touched rows
far above the bound) and prints its measured error next to the bound before it asserts.

Measured on an MI355X, `d_table` err / bound per case: small 1.5e-7 / 1.7e-6, tiles 6.7e-7 / 1.3e-5, one_step_chunk 7.2e-7 / 6.0e-6,
wide 1.3e-6 / 6.1e-6, t0 6.7e-7 / 1.2e-5, e120 9.8e-7 / 5.7e-6, hot 8.0e-6 / 2.0e-4, hot_wide 1.4e-5 / 2.9e-4, ends 1.5e-7 / 1.7e-6,
carry 1.3e-6 / 6.1e-6 (worst ratio 0.21); smallest touched-row max |G| / bound 2.2e4.  No case misses its bound."""
import copy

import numpy as np
import pytest
import torch

import seq_grad_reference as G
import seq_reference as R
import seq_table_grad_reference as TG
from helpers import csr, make_store

pytestmark = pytest.mark.gpu

HOT = 7
# name -> (E, H, U, T, t0, kind).  (24, 48, 33, 70): three user tiles, the last with one live row; chunks of 32 + 32 + 6.
# (72, 144, 17, 65): the last chunk is one step.  E = 120: the last column tile of dX is half empty.  hot: every position of every
# user holds item 7, one destination with U T = 2310 contributions (the rank pass's bitmap path, 145 pieces).
CASES = {
    "small": (8, 16, 5, 37, 0, None),
    "tiles": (24, 48, 33, 70, 0, None),
    "one_step_chunk": (72, 144, 17, 65, 0, None),
    "wide": (128, 256, 25, 37, 0, None),
    "t0": (24, 48, 33, 70, 3, None),
    "e120": (120, 128, 20, 40, 0, None),
    "hot": (24, 48, 33, 70, 0, "hot"),
    "hot_wide": (128, 256, 33, 70, 0, "hot"),
    "ends": (8, 16, 5, 37, 0, "ends"),
}


def _case_data(name):
    E, H, U, T, t0, kind = CASES[name]
    items, ratings, table = make_store(U, 300, E, T + 1 + t0, T + 9 + t0, seed=E)
    if kind == "hot":
        items = [np.full(len(i), HOT, dtype=np.int64) for i in items]
    if kind == "ends":                                                 # the first and the last id a store of 300 items can hold
        items[0][0], items[1][5] = 0, 299
    torch.manual_seed(E)
    lstm = torch.nn.LSTM(E + 1, H)
    g = torch.Generator().manual_seed(U)
    hc = (torch.randn(U, H, generator=g) * 0.5, torch.randn(U, H, generator=g) * 0.5)
    return dict(E=E, H=H, U=U, T=T, t0=t0, kind=kind, items=items, ratings=ratings, table=TG.extended_table(table, seed=E),
                lstm=lstm, hc=hc, Rw=G.loss_weights(U, T, H, seed=T + U))


@pytest.fixture(scope="module")
def cases():
    """Case data and float64 / float32 CPU references, computed once per case and shared (never modified)."""
    store = {}

    def get(name):
        if name not in store:
            c = _case_data(name)
            c["idx"], c["rts"] = TG.positions(c["items"], c["ratings"], c["T"], c["t0"])
            c["bounds"], c["g64"], c["d32"] = TG.table_grad_bounds(c["lstm"], c["table"], c["idx"], c["rts"], c["hc"], c["Rw"])
            store[name] = c
        return store[name]
    return get


def _on_gpu(cuda, c):
    from recnn_amd.data.store import ReplayStore
    gl = torch.nn.LSTM(c["E"] + 1, c["H"]).to(cuda)
    gl.load_state_dict(c["lstm"].state_dict())
    return ReplayStore.from_arrays(*csr(c["items"], c["ratings"]), cuda), gl


def _gpu_grads(cuda, c, st, gl, train_table=True, with_h0=True, frozen=False):
    """{name: gradient on the CPU} of the loss over lstm_encode_train; "table" when train_table."""
    from recnn_amd.nn import functional as F
    gl.zero_grad(set_to_none=True)
    for p in gl.parameters():
        p.requires_grad_(not frozen)
    tbl = c["table"].to(cuda).requires_grad_(train_table)
    hcg = tuple(t.to(cuda).requires_grad_(with_h0 and not frozen) for t in c["hc"])
    slots = np.arange(c["U"], dtype=np.int32)
    h, (hT, cT) = F.lstm_encode_train(gl, st, tbl, slots, c["T"], hcg, t0=c["t0"], train_table=train_table)
    G.loss_of(h, hT, cT, c["Rw"]).backward()
    out = {} if frozen else {n: getattr(gl, n).grad.cpu() for n in G.PARAMS}
    if with_h0 and not frozen:
        out["h0"], out["c0"] = hcg[0].grad.cpu(), hcg[1].grad.cpu()
    if train_table:
        out["table"] = tbl.grad.cpu()
    for p in gl.parameters():
        p.requires_grad_(True)
    return out


def _check_table(tag, got, c, touched):
    err = float((got.double() - c["g64"]["table"]).abs().max())
    bound = c["bounds"]["table"]
    print(f"{tag} table: err {err:.3e} bound {bound:.3e} err/bound {err / bound:.3f} max|G32-G64| {c['d32']['table']:.3e} "
          f"max|G| {float(c['g64']['table'].abs().max()):.3e}")
    assert bool((got[~touched] == 0).all()), f"{tag}: a row nothing reaches is not exactly zero"
    assert bool((got[touched].abs().amax(1) > 0).all())
    assert err <= bound, (tag, err, bound)


# ---------------------------------------------------------------------------------------------------- versus float64
@pytest.mark.parametrize("name", list(CASES))
def test_table_gradient_against_float64(cuda, cases, name):
    c = cases(name)
    hot = c["U"] * c["T"] if c["kind"] == "hot" else None
    touched, _ = TG.check_preconditions(name, c["g64"]["table"], c["idx"], c["bounds"]["table"], hot=hot)
    if c["kind"] == "hot":
        assert hot == 2310 and int(torch.nonzero(touched)[0]) == HOT
    if c["kind"] == "ends":
        assert bool(touched[0]) and bool(touched[299])
    st, gl = _on_gpu(cuda, c)
    got = _gpu_grads(cuda, c, st, gl)
    assert got["table"].shape == c["table"].shape
    _check_table(name, got["table"], c, touched)
    for n in G.NAMES:                                                 # the other gradients of the same call stay within theirs
        err = float((got[n].double() - c["g64"][n]).abs().max())
        print(f"{name} {n}: err {err:.3e} bound {c['bounds'][n]:.3e}")
        assert err <= c["bounds"][n], (name, n, err, c["bounds"][n])


# ---------------------------------------------------------------------------------------------------- exact checks
@pytest.mark.parametrize("name", ["tiles", "wide"])
def test_bit_exact_properties(cuda, cases, name):
    from recnn_amd.nn import functional as F
    c = cases(name)
    st, gl = _on_gpu(cuda, c)
    a = _gpu_grads(cuda, c, st, gl)
    b = _gpu_grads(cuda, c, st, gl)
    assert torch.equal(a["table"], b["table"])                        # two runs, the same bits
    plain = _gpu_grads(cuda, c, st, gl, train_table=False)
    for n in G.NAMES:                                                 # the old outputs keep their bits
        assert torch.equal(a[n], plain[n]), n
    only = _gpu_grads(cuda, c, st, gl, frozen=True)                   # no weight gradient wanted: the chain still writes da
    assert set(only) == {"table"} and torch.equal(only["table"], a["table"])
    # the forward is lstm_encode's, bit for bit, under both variants
    slots = np.arange(c["U"], dtype=np.int32)
    hc = tuple(t.to(cuda) for t in c["hc"])
    for variant in ("fused", "chunked"):
        F.set_lstm_variant(variant)
        try:
            h, (hT, cT) = F.lstm_encode(gl, st, c["table"].to(cuda), slots, c["T"], hc)
            tbl = c["table"].to(cuda).requires_grad_(True)
            ht, (hTt, cTt) = F.lstm_encode_train(gl, st, tbl, slots, c["T"], hc, train_table=True)
        finally:
            F.set_lstm_variant("chunked")
        assert ht.requires_grad and torch.equal(ht, h) and torch.equal(hTt, hT) and torch.equal(cTt, cT), variant
    # a second backward on a fresh graph accumulates into table.grad
    tbl = c["table"].to(cuda).requires_grad_(True)
    for k in (1, 2):
        h, (hT, cT) = F.lstm_encode_train(gl, st, tbl, slots, c["T"], hc, train_table=True)
        G.loss_of(h, hT, cT, c["Rw"]).backward()
        assert torch.equal(tbl.grad.cpu(), a["table"] * k)
    # a table that does not require grad: train_table=True is today's call; under no_grad nothing is recorded
    ht, _ = F.lstm_encode_train(gl, st, c["table"].to(cuda), slots, c["T"], hc, train_table=True)
    assert ht.requires_grad and torch.equal(ht, h)
    with torch.no_grad():
        hn, _ = F.lstm_encode_train(gl, st, tbl, slots, 3, train_table=True)
    assert not hn.requires_grad and hn.grad_fn is None
    for p in gl.parameters():
        p.requires_grad_(False)
    hf, _ = F.lstm_encode_train(gl, st, c["table"].to(cuda), slots, 3, train_table=True)
    assert not hf.requires_grad
    hl, _ = F.lstm_encode_train(gl, st, tbl, slots, 3, train_table=True)     # the table alone counts as live
    assert hl.requires_grad and torch.equal(hl, hf)


# ---------------------------------------------------------------------------------------------------- carry
def test_carry_across_calls(cuda, cases):
    """37 steps as one call against 20 + 17 with (h_T, c_T) carried and requiring grad: the two calls' table gradients are summed
    by autograd."""
    from recnn_amd.nn import functional as F
    c = cases("wide")
    touched, _ = TG.check_preconditions("carry", c["g64"]["table"], c["idx"], c["bounds"]["table"])
    st, gl = _on_gpu(cuda, c)
    one = _gpu_grads(cuda, c, st, gl)
    gl.zero_grad(set_to_none=True)
    slots = np.arange(c["U"], dtype=np.int32)
    tbl = c["table"].to(cuda).requires_grad_(True)
    hcg = tuple(t.to(cuda).requires_grad_(True) for t in c["hc"])
    ha, hca = F.lstm_encode_train(gl, st, tbl, slots, 20, hcg, train_table=True)
    hb, (hT, cT) = F.lstm_encode_train(gl, st, tbl, slots, 17, hca, t0=20, train_table=True)
    G.loss_of(torch.cat([ha, hb], 1), hT, cT, c["Rw"]).backward()
    assert torch.equal(hcg[0].grad.cpu(), one["h0"]) and torch.equal(hcg[1].grad.cpu(), one["c0"])
    _check_table("carry 20 + 17 vs float64", tbl.grad.cpu(), c, touched)
    diff = float((tbl.grad.cpu().double() - one["table"].double()).abs().max())
    print(f"carry 20 + 17 vs one call table: diff {diff:.3e} bound {c['bounds']['table']:.3e}")


# ---------------------------------------------------------------------------------------------------- SeqEnv.user_batch
def _env(cuda, table, user_dict, users, lstm, batch_size=5):
    from recnn_amd.data.env import SeqEnv
    gl = torch.nn.LSTM(lstm.input_size, lstm.hidden_size).to(cuda)
    gl.load_state_dict(lstm.state_dict())
    return SeqEnv.from_user_dict(table, user_dict, users, state_encoder=gl, batch_size=batch_size, max_buf_size=4 * batch_size,
                                 device=cuda)


def test_user_batch_with_a_table(cuda):
    table, user_dict, users, lstm = R.seq_env_data()
    env = _env(cuda, table, user_dict, users, lstm)
    ids, steps = [0, 1, 2, 3, 4], [3, 4, 9, 30]
    today = env.user_batch(ids, steps)
    none = env.user_batch(ids, steps, table=None)
    keys = ("state", "action", "reward", "next_state")
    assert all(torch.equal(none[k], today[k]) for k in keys) and none["state"].requires_grad
    for params_live in (True, False):
        for p in env.state_encoder.parameters():
            p.requires_grad_(params_live)
        for table_live in (True, False):
            P = env.table.clone().requires_grad_(table_live)
            batch = env.user_batch(ids, steps, table=P)
            want = params_live or table_live
            assert batch["state"].requires_grad == want and batch["next_state"].requires_grad == want, (params_live, table_live)
            assert not batch["action"].requires_grad and not batch["reward"].requires_grad
            assert all(torch.equal(batch[k], today[k]) for k in keys)
            with torch.no_grad():
                assert not env.user_batch(ids, steps, table=P)["state"].requires_grad
    # another table is really read: state, next_state and action follow it
    P2 = (env.table * 0.5).contiguous()
    other = env.user_batch(ids, steps, table=P2)
    assert torch.equal(other["action"], today["action"] * 0.5) and not torch.equal(other["state"], today["state"])
    assert torch.equal(other["reward"], today["reward"])
    # a loss on next_state reaches P.grad: touched rows only
    P = env.table.clone().requires_grad_(True)
    batch = env.user_batch(ids, steps, table=P)
    batch["next_state"].pow(2).sum().backward()
    touched = torch.zeros(P.shape[0], dtype=torch.bool)
    for u in ids:
        touched[torch.as_tensor(user_dict[u]["items"][:steps[-1] + 1], dtype=torch.long)] = True
    g = P.grad.cpu()
    assert torch.isfinite(g).all() and bool((g[~touched] == 0).all()) and bool((g[touched].abs().amax(1) > 0).all())
    for bad in (env.table.cpu(), env.table.double(), env.table[:-1].contiguous(), env.table.t().contiguous().t()):
        with pytest.raises(ValueError, match="table"):
            env.user_batch(ids, steps, table=bad)


# ---------------------------------------------------------------------------------------------------- ddpg_update
PARAMS = {"gamma": 0.99, "min_value": -10, "max_value": 10, "policy_step": 2, "soft_tau": 0.01}


def test_ddpg_update_trains_the_table(cuda):
    """One ddpg_update(learn=True) at a policy step on a batch attached to P, P in the policy optimizer (plain SGD, no weight decay)."""
    import recnn
    from recnn_amd.nn import fused
    keep = dict(fused.DEFAULTS)
    fused.set_defaults(dtype="fp32", mask_mode="hash", seed=11)
    try:
        table, user_dict, users, lstm = R.seq_env_data()
        ids, steps = [0, 1, 2, 3, 4], [3, 7, 20]
        torch.manual_seed(3)
        pol, val = recnn.nn.Actor(16, 8, 16, 6e-1), recnn.nn.Critic(16, 8, 16, 54e-2)
        nets = {"policy_net": pol, "value_net": val, "target_policy_net": copy.deepcopy(pol), "target_value_net": copy.deepcopy(val)}
        nets = {k: v.to(cuda).eval() for k, v in nets.items()}
        env = _env(cuda, table, user_dict, users, lstm)
        P = env.table.clone().requires_grad_(True)
        before = P.detach().clone()
        popt = torch.optim.SGD(list(nets["policy_net"].parameters()) + list(env.state_encoder.parameters()) + [P], lr=1e-2)
        vopt = torch.optim.SGD(nets["value_net"].parameters(), lr=1e-2)
        batch = env.user_batch(ids, steps, table=P)
        assert batch["state"].requires_grad
        loss = recnn.nn.update.ddpg_update(batch, PARAMS, nets, {"policy_optimizer": popt, "value_optimizer": vopt}, learn=True, step=0)
        assert np.isfinite(loss["value"]) and np.isfinite(loss["policy"])
        touched = torch.zeros(P.shape[0], dtype=torch.bool)
        for u in ids:
            touched[torch.as_tensor(user_dict[u]["items"][:steps[-1] + 1], dtype=torch.long)] = True
        assert 0 < int(touched.sum()) < P.shape[0]
        g = P.grad.cpu()
        print(f"ddpg_update: P.grad max {float(g.abs().max()):.3e}, touched rows {int(touched.sum())} of {P.shape[0]}, "
              f"smallest touched-row max {float(g[touched].abs().amax(1).min()):.3e}")
        assert torch.isfinite(g).all()
        assert bool((g[touched].abs().amax(1) > 0).all()) and bool((g[~touched] == 0).all())
        moved = (P.detach() != before).any(1).cpu()
        assert bool(moved.any()) and not bool(moved[~touched].any())   # only touched rows of P change
        for n in G.PARAMS:
            assert getattr(env.state_encoder, n).grad is not None
    finally:
        fused.set_defaults(**keep)


# ---------------------------------------------------------------------------------------------------- training works
def test_training_works_with_the_table(cuda):
    """Plain SGD on encoder and table through user_batch(table=P): the GPU run's relative fall of the loss is at least half of the
    float64 CPU restatement's (which falls by at least 10 % at the learning rate the helper chose on it) -- the tolerance of
    tests/test_gpu_seq_grad.py::test_training_works --, every loss of the GPU curve lies within 1e-4 (relative) of the float64
    curve's, and the table really moved."""
    table, user_dict, users, lstm, steps, (w_read, b_read), lr, ref_losses = TG.training_case_with_table()
    env = _env(cuda, table, user_dict, list(range(12)), lstm)
    P = env.table.clone().requires_grad_(True)
    before = P.detach().clone()
    opt = torch.optim.SGD(list(env.state_encoder.parameters()) + [P], lr=lr)
    w, b = w_read.to(cuda), b_read.to(cuda)
    losses = []
    for _ in range(G.TRAIN_SGD_STEPS + 1):
        batch = env.user_batch(users, steps, table=P)                  # rows k * U + u
        loss = ((batch["next_state"] @ w + b) - batch["reward"]).pow(2).mean()
        losses.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    fall, ref_fall = 1.0 - losses[-1] / losses[0], 1.0 - ref_losses[-1] / ref_losses[0]
    worst = max(abs(a - r) / r for a, r in zip(losses, ref_losses))
    print(f"training with the table: lr {lr} float64 loss {ref_losses[0]:.6f} -> {ref_losses[-1]:.6f} (fall {ref_fall:.4f}), "
          f"GPU loss {losses[0]:.6f} -> {losses[-1]:.6f} (fall {fall:.4f}), worst relative distance of the curves {worst:.3e}")
    assert ref_fall >= 0.1 and np.isfinite(losses).all()
    assert fall >= 0.5 * ref_fall
    # the curves themselves: a step's float32 gradient lies within 1.6e-6 of its largest entry (the floor of this file's float64 rule at
    # U T = 5 * 36: 2^-23 sqrt(180)), the errors of the 20 steps add at most linearly along a monotone descent,
    # and the rule's factor 4 allows for other summation orders: 20 * 4 * 1.6e-6 = 1.3e-4, rounded down.  Not taken from the
    # measurement (1.9e-7 on an MI355X).
    assert worst <= 1e-4, worst
    assert float((P.detach() - before).abs().max()) > 0
