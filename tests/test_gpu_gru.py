"""The GRU state encoder on the GPU (csrc/gru.hip): `gru_encode` and `gru_encode_train` against torch.nn.GRU in float64 on the CPU
(tests/gru_reference.py), both schedules and the carry across calls bit for bit, the gradients of the four weights, of h0 and of the
embedding table, `SeqEnv` with a GRU as its state encoder, one small problem on which the encoder must actually learn, and
`ddpg_update` / `td3_update` training the GRU through an attached `user_batch`.

Bounds come from the references alone.  Forward: 4 max |fp32 CPU - fp64 CPU|, floored at 1e-6 (gru_reference.fp32_bound).  A gradient
tensor G: max(4 max |G32cpu - G64cpu|, 2^-23 max(8, sqrt(U T)) max |G64|) (gru_reference.grad_bounds).  Every test prints its measured
error next to the bound before it asserts.

Shapes (E, H): (8, 16) -- 3H = 48 is below one 64-row dW tile; (40, 96) -- a half-empty last k block of x and 3H = 288 off the 64
grid; (128, 256) -- two hidden tiles per wave.  U = 5 and 25 (one full tile of 16 users plus a partly filled one), T = 1 and 37 (37
crosses the 32-step chunk)."""
import copy

import numpy as np
import pytest
import torch

import gru_reference as G
import seq_reference as R
from helpers import csr, make_store

pytestmark = pytest.mark.gpu

T_MAX = 37
SHAPES = ((8, 16), (40, 96), (128, 256))
EXTRA_ROWS = 12            # table rows past the ids the store can hold: no position reaches them


@pytest.fixture(scope="module")
def seq_data():
    """Per (E, H): 25 users with at least T_MAX + 1 elements, their table and a GRU(E + 1, H) (CPU master copies)."""
    out = {}
    for E, H in SHAPES:
        items, ratings, table = make_store(25, 300, E, T_MAX + 1, T_MAX + 9, seed=E)
        torch.manual_seed(E)
        out[(E, H)] = (items, ratings, torch.from_numpy(table), torch.nn.GRU(E + 1, H))
    return out


@pytest.fixture(scope="module")
def references():
    """Float64 / float32 CPU results and bounds, computed once per case and shared (never modified)."""
    return {}


@pytest.fixture
def variants():
    from recnn_amd.nn import functional as F
    yield F
    F.set_lstm_variant("chunked")


def _gpu_gru(cuda, gru):
    gl = torch.nn.GRU(gru.input_size, gru.hidden_size).to(cuda)
    gl.load_state_dict(gru.state_dict())
    return gl


def _on_gpu(cuda, data):
    from recnn_amd.data.store import ReplayStore
    items, ratings, table, gru = data
    return ReplayStore.from_arrays(*csr(items, ratings), cuda), table.to(cuda), _gpu_gru(cuda, gru)


def _h0(U, H, seed):
    return torch.randn(U, H, generator=torch.Generator().manual_seed(seed)) * 0.5


def _inputs(seq_data, EH, slots, T, t0=0):
    items, ratings, table, _ = seq_data[EH]
    return R.lstm_inputs(table, [items[s] for s in slots], [ratings[s] for s in slots], T, t0)


def _reference(references, seq_data, EH, slots, T, with_h0, use="all"):
    key = (EH, tuple(int(s) for s in slots), T, with_h0, use)
    if key not in references:
        U = len(slots)
        h0 = _h0(U, EH[1], U) if with_h0 else None
        Rw = G.loss_weights(U, T, EH[1], seed=T + U)
        references[key] = (h0, Rw) + G.grad_bounds(seq_data[EH][3], _inputs(seq_data, EH, slots, T), h0, Rw, use)
    return references[key]


def _gpu_grads(cuda, gl, st, tbl, slots, T, h0, Rw, use="all", **kw):
    """{name: gradient on the CPU} of the loss over gru_encode_train."""
    from recnn_amd.nn import functional as F
    gl.zero_grad(set_to_none=True)
    h0g = None if h0 is None else h0.to(cuda).requires_grad_(True)
    h, hT = F.gru_encode_train(gl, st, tbl, slots, T, h0g, **kw)
    G.loss_of(h, hT, Rw, use).backward()
    out = {n: getattr(gl, n).grad.cpu() for n in G.PARAMS if getattr(gl, n).grad is not None}
    if h0g is not None:
        out["h0"] = h0g.grad.cpu()
    return out


def _check(tag, got, g64, bounds):
    worst = []
    for n in g64:
        err = float((got[n].double() - g64[n]).abs().max())
        print(f"{tag} {n}: err {err:.3e} bound {bounds[n]:.3e} max|G| {float(g64[n].abs().max()):.3e}")
        if not err <= bounds[n]:
            worst.append((n, err, bounds[n]))
    assert not worst, (tag, worst)


# ---------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("EH", SHAPES)
def test_forward_against_float64_and_between_variants(cuda, seq_data, variants, EH):
    F = variants
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    for U in (5, 25):
        slots = np.arange(25 - U, 25, dtype=np.int32)
        for T in (1, T_MAX):
            x = _inputs(seq_data, EH, slots, T)
            for h0 in (None, _h0(U, EH[1], U)):
                bound, (h64, hT64) = G.fp32_bound(seq_data[EH][3], x, h0)
                h0g = None if h0 is None else h0.to(cuda)
                got = {}
                for variant in ("fused", "chunked"):
                    F.set_lstm_variant(variant)
                    got[variant] = F.gru_encode(gl, st, tbl, slots, T, h0g)
                    ht, hTt = F.gru_encode_train(gl, st, tbl, slots, T, h0g)
                    assert ht.requires_grad and hTt.requires_grad and not got[variant][0].requires_grad
                    assert torch.equal(ht, got[variant][0]) and torch.equal(hTt, got[variant][1]), (U, T, variant)
                h, hT = got["chunked"]
                assert torch.equal(h, got["fused"][0]) and torch.equal(hT, got["fused"][1]), (U, T)
                assert h.shape == (U, T, EH[1]) and torch.equal(hT, h[:, -1])
                errs = float((h.cpu().double() - h64).abs().max()), float((hT.cpu().double() - hT64).abs().max())
                print(f"forward E,H={EH} U={U} T={T} h0={'zero' if h0 is None else 'set'}: h err {errs[0]:.3e} bound {bound[0]:.3e}, "
                      f"h_T err {errs[1]:.3e} bound {bound[1]:.3e}")
                assert errs[0] <= bound[0] and errs[1] <= bound[1]
    with torch.no_grad():                                            # the inference path: no graph, nothing saved
        ht, _ = F.gru_encode_train(gl, st, tbl, slots, 3)
    assert not ht.requires_grad and ht.grad_fn is None


@pytest.mark.parametrize("EH", SHAPES)
def test_forward_carry_and_batch_independence(cuda, seq_data, variants, EH):
    F = variants
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    slots = np.arange(25, dtype=np.int32)
    h0 = _h0(25, EH[1], 3).to(cuda)
    for variant in ("fused", "chunked"):
        F.set_lstm_variant(variant)
        h, hT = F.gru_encode(gl, st, tbl, slots, T_MAX, h0)
        ha, hTa = F.gru_encode(gl, st, tbl, slots, 20, h0)
        hb, hTb = F.gru_encode(gl, st, tbl, slots, 17, hTa, t0=20)
        assert torch.equal(torch.cat([ha, hb], 1), h) and torch.equal(hTb, hT), variant
        # a user's bits do not depend on its row in the tile or on the other users of the batch
        some = np.array([19, 3, 24], dtype=np.int32)
        hs, hTs = F.gru_encode(gl, st, tbl, some, T_MAX, h0[torch.from_numpy(some).long().to(cuda)])
        assert torch.equal(hs, h[some]) and torch.equal(hTs, hT[some]), variant


# ---------------------------------------------------------------------------------------------------- gradients
@pytest.mark.parametrize("U", [5, 25])
@pytest.mark.parametrize("EH", SHAPES)
def test_gradients_against_float64(cuda, seq_data, references, EH, U):
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    slots = np.arange(25 - U, 25, dtype=np.int32)
    H = EH[1]
    for T, with_h0 in ((T_MAX, True), (T_MAX, False), (1, True)):
        h0, Rw, bounds, g64 = _reference(references, seq_data, EH, slots, T, with_h0)
        got = _gpu_grads(cuda, gl, st, tbl, slots, T, h0, Rw)
        assert set(got) == set(g64)
        # b_hn sits inside the reset product: two tensors, equal in r and z, different in n
        assert torch.equal(got["bias_ih_l0"][:2 * H], got["bias_hh_l0"][:2 * H])
        assert not torch.equal(got["bias_ih_l0"][2 * H:], got["bias_hh_l0"][2 * H:])
        _check(f"grad E,H={EH} U={U} T={T} h0={'set' if with_h0 else 'zero'}", got, g64, bounds)


@pytest.mark.parametrize("use", ["final", "head"])
@pytest.mark.parametrize("EH", SHAPES)
def test_partial_losses(cuda, seq_data, references, EH, use):
    """"final": only h_T is used, the gradient of h is absent; "head": only h[:, :20], later steps carry zeros."""
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    slots = np.arange(25, dtype=np.int32)
    h0, Rw, bounds, g64 = _reference(references, seq_data, EH, slots, T_MAX, True, use)
    got = _gpu_grads(cuda, gl, st, tbl, slots, T_MAX, h0, Rw, use)
    _check(f"partial loss {use} E,H={EH}", got, g64, bounds)


@pytest.mark.parametrize("EH", [(40, 96), (128, 256)])
def test_carry_across_calls_with_grad(cuda, seq_data, references, EH):
    """37 steps as one call against 20 + 17 with h_T carried and requiring grad."""
    from recnn_amd.nn import functional as F
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    slots = np.arange(8, 25, dtype=np.int32)
    h0, Rw, bounds, g64 = _reference(references, seq_data, EH, slots, T_MAX, True)
    one = _gpu_grads(cuda, gl, st, tbl, slots, T_MAX, h0, Rw)
    gl.zero_grad(set_to_none=True)
    h0g = h0.to(cuda).requires_grad_(True)
    ha, hTa = F.gru_encode_train(gl, st, tbl, slots, 20, h0g)
    assert hTa.requires_grad
    hb, hT = F.gru_encode_train(gl, st, tbl, slots, 17, hTa, t0=20)
    G.loss_of(torch.cat([ha, hb], 1), hT, Rw).backward()
    two = {n: getattr(gl, n).grad.cpu() for n in G.PARAMS}
    two["h0"] = h0g.grad.cpu()
    assert torch.equal(two["h0"], one["h0"])
    _check(f"carry 20 + 17 vs float64 E,H={EH}", two, g64, bounds)
    for n in G.PARAMS:                                               # the grouping of the sums differs across the cut
        err = float((two[n].double() - one[n].double()).abs().max())
        print(f"carry 20 + 17 vs one call {n}: diff {err:.3e} bound {bounds[n]:.3e}")
        assert err <= bounds[n]


@pytest.mark.parametrize("EH", [(8, 16), (128, 256)])
def test_run_to_run_and_user_permutation(cuda, seq_data, references, EH):
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    slots = np.arange(8, 25, dtype=np.int32)
    h0, Rw, _, _ = _reference(references, seq_data, EH, slots, T_MAX, True)
    a = _gpu_grads(cuda, gl, st, tbl, slots, T_MAX, h0, Rw)
    b = _gpu_grads(cuda, gl, st, tbl, slots, T_MAX, h0, Rw)
    for n in G.NAMES:
        assert torch.equal(a[n], b[n]), n
    perm = np.random.default_rng(0).permutation(len(slots))
    pt = torch.from_numpy(perm)
    p = _gpu_grads(cuda, gl, st, tbl, slots[perm], T_MAX, h0[pt], tuple(r[pt] for r in Rw))
    assert torch.equal(p["h0"], a["h0"][pt])


# ---------------------------------------------------------------------------------------------------- table gradient
def _table_case(references, seq_data, EH, U, T, with_h0):
    key = ("table", EH, U, T, with_h0)
    if key not in references:
        items, ratings, table, gru = seq_data[EH]
        slots = np.arange(25 - U, 25, dtype=np.int32)
        extra = np.random.default_rng(1000 + EH[0]).standard_normal((EXTRA_ROWS, EH[0])).astype(np.float32)
        big = torch.cat([table, torch.from_numpy(extra)], 0)
        idx, rts = G.positions([items[s] for s in slots], [ratings[s] for s in slots], T)
        h0 = _h0(U, EH[1], U) if with_h0 else None
        Rw = G.loss_weights(U, T, EH[1], seed=T + U)
        references[key] = (slots, big, idx, h0, Rw) + G.table_grad_bounds(gru, big, idx, rts, h0, Rw)
    return references[key]


@pytest.mark.parametrize("U,T,with_h0", [(25, T_MAX, True), (5, T_MAX, False), (5, 1, True)])
@pytest.mark.parametrize("EH", SHAPES)
def test_table_gradient(cuda, seq_data, references, EH, U, T, with_h0):
    st, _, gl = _on_gpu(cuda, seq_data[EH])
    slots, big, idx, h0, Rw, bounds, g64 = _table_case(references, seq_data, EH, U, T, with_h0)
    counts = torch.bincount(idx.reshape(-1), minlength=big.shape[0])
    touched = counts > 0
    n_touched, n_untouched = int(touched.sum()), int((~touched).sum())
    print(f"table E,H={EH} U={U} T={T}: touched rows {n_touched}, untouched {n_untouched}, most hits {int(counts.max())}")
    assert n_touched > 0 and n_untouched >= EXTRA_ROWS and bool((g64["table"][~touched] == 0).all())
    tb = big.to(cuda).requires_grad_(True)
    got = _gpu_grads(cuda, gl, st, tb, slots, T, h0, Rw, train_table=True)
    got["table"] = tb.grad.cpu()
    assert set(got) == set(g64)
    _check(f"table grad E,H={EH} U={U} T={T}", got, g64, bounds)
    assert bool((got["table"][~touched] == 0).all()) and bool((got["table"][touched].abs().amax(1) > 0).all())
    # the frozen-table call gives the same bits in what the two share
    frozen = _gpu_grads(cuda, gl, st, big.to(cuda), slots, T, h0, Rw)
    for n in frozen:
        assert torch.equal(frozen[n], got[n]), n
    # every encoder parameter frozen: the table alone
    for p in gl.parameters():
        p.requires_grad_(False)
    tb2 = big.to(cuda).requires_grad_(True)
    alone = _gpu_grads(cuda, gl, st, tb2, slots, T, None if h0 is None else h0.clone(), Rw, train_table=True)
    assert not any(n in alone for n in G.PARAMS)
    assert torch.equal(tb2.grad.cpu(), got["table"])                  # ... and run to run
    if h0 is not None:
        assert torch.equal(alone["h0"], got["h0"])


# ---------------------------------------------------------------------------------------------------- SeqEnv
def _env(cuda, table, user_dict, users, gru, batch_size=5):
    from recnn_amd.data.env import SeqEnv
    return SeqEnv.from_user_dict(table, user_dict, users, state_encoder=_gpu_gru(cuda, gru), batch_size=batch_size,
                                 max_buf_size=4 * batch_size, device=cuda)


def test_seq_env_generator_matches_the_reference_loop(cuda):
    table, user_dict, users, gru = G.gru_env_data()
    np.random.seed(R.SEQ_ENV_SEED)
    ref, bound = G.gru_env_batches(table, user_dict, users, gru, 5, 20, 3)
    env = _env(cuda, table, user_dict, users, gru)
    assert [tuple(s) for s in env.buffer_layout] == [(20, 16), (20, 8), (20, 1), (20, 16)]
    np.random.seed(R.SEQ_ENV_SEED)
    gen = env.train_batch()
    compared = []
    for k, want in enumerate(ref):
        got = next(gen)
        assert set(got) == {"state", "action", "reward", "next_state", "done", "meta"}
        m = got["meta"]
        assert m["step"] == want["meta"]["step"] and m["rows"] == want["meta"]["rows"] and list(m["users"]) == want["meta"]["users"]
        assert torch.equal(got["action"].cpu(), torch.from_numpy(want["action"]))
        assert torch.equal(got["reward"].cpu(), torch.from_numpy(want["reward"]))
        for key in ("state", "next_state"):
            err = float((got[key].cpu().double() - torch.from_numpy(want[key])).abs().max())
            print(f"SeqEnv (GRU) batch {k} {key}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound
            assert got[key][:m["rows"]].abs().max() > 0 and not got[key][m["rows"]:].any()
        compared.append(m["rows"])
    assert compared == [20, 17, 20]                                   # an empty comparison must not pass


def test_user_batch(cuda):
    from recnn_amd.nn import functional as F
    table, user_dict, users, gru = G.gru_env_data()
    env = _env(cuda, table, user_dict, users, gru)
    ids, steps = [0, 1, 2, 3, 4], [3, 4, 9, 30]
    batch = env.user_batch(ids, steps)
    assert batch["meta"]["step"] == steps and batch["meta"]["users"] == ids and batch["meta"]["rows"] == 20
    slots = env.store.slots(ids)
    h, _ = F.gru_encode(env.state_encoder, env.store, env.table, slots, steps[-1] + 1)
    views = (torch.empty(20, 16, device=cuda), torch.empty(20, 8, device=cuda), torch.empty(20, 1, device=cuda),
             torch.empty(20, 16, device=cuda))
    F.seq_collect(h, steps, env.store, env.table, slots, views)
    for key, want in zip(("state", "action", "reward", "next_state"), views):
        assert torch.equal(batch[key], want), key
    assert batch["state"].requires_grad and batch["next_state"].requires_grad and not batch["action"].requires_grad
    # state.requires_grad holds exactly when an encoder parameter requires grad or the table does
    with torch.no_grad():
        assert not env.user_batch(ids, steps)["state"].requires_grad
    for p in env.state_encoder.parameters():
        p.requires_grad_(False)
    frozen = env.user_batch(ids, steps)
    assert not frozen["state"].requires_grad and not frozen["next_state"].requires_grad
    assert torch.equal(frozen["state"], views[0]) and torch.equal(frozen["next_state"], views[3])
    tb = env.table.detach().clone().requires_grad_(True)
    with_table = env.user_batch(ids, steps, table=tb)
    assert with_table["state"].requires_grad and torch.equal(with_table["state"], views[0])
    with_table["next_state"].sum().backward()
    assert tb.grad is not None and tb.grad.abs().max() > 0
    env.state_encoder.bias_hh_l0.requires_grad_(True)
    assert env.user_batch(ids, steps)["state"].requires_grad


def test_training_works(cuda):
    """Plain SGD on the GRU through user_batch: the GPU run's relative fall of the loss is at least half of the float64 CPU
    restatement's (which falls by at least 10 % at the learning rate the helper chose on it)."""
    table, user_dict, users, gru, steps, (w_read, b_read), lr, ref_losses = G.training_case()
    env = _env(cuda, table, user_dict, list(range(12)), gru)
    opt = torch.optim.SGD(env.state_encoder.parameters(), lr=lr)
    w, b = w_read.to(cuda), b_read.to(cuda)
    losses = []
    for _ in range(G.TRAIN_SGD_STEPS + 1):
        batch = env.user_batch(users, steps)                         # rows k * U + u
        loss = ((batch["next_state"] @ w + b) - batch["reward"]).pow(2).mean()
        losses.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    fall, ref_fall = 1.0 - losses[-1] / losses[0], 1.0 - ref_losses[-1] / ref_losses[0]
    print(f"GRU training: lr {lr} float64 loss {ref_losses[0]:.6f} -> {ref_losses[-1]:.6f} (fall {ref_fall:.4f}), "
          f"GPU loss {losses[0]:.6f} -> {losses[-1]:.6f} (fall {fall:.4f})")
    assert ref_fall >= 0.1 and np.isfinite(losses).all()
    assert fall >= 0.5 * ref_fall


# ---------------------------------------------------------------------------------------------------- ddpg_update / td3_update
DDPG_PARAMS = {"gamma": 0.99, "min_value": -10, "max_value": 10, "policy_step": 2, "soft_tau": 0.01}
TD3_PARAMS = {"gamma": 0.99, "noise_std": 0.5, "noise_clip": 0.7, "soft_tau": 0.01, "policy_update": 2}
# The encoder sits in the policy optimizer, a plain SGD stepped by torch.  What is measured is (p_before - p_after) / lr, and the fp32
# subtraction p - lr g rounds by up to 2^-24 (|p| + lr |g|), that is 2^-24 (|p| / lr + |g|) of the gradient: the learning rate is a power
# of two (the division is exact) and large enough, 16, that the |p| / lr term (|p| <= 0.25 at H = 16) stays well below the bound's floor
# 2^-23 * 8 max |G|.  The actor moves by 16 times its clipped gradient in the same step; nothing after the step is looked at.
UPDATE_LR = 16.0
UPDATE_IDS, UPDATE_STEPS = [0, 1, 2, 3, 4], [3, 4, 9, 30]


@pytest.fixture
def defaults(cuda):
    """fused.DEFAULTS as the update tests need them, put back afterwards."""
    from recnn_amd.nn import fused
    keep = dict(fused.DEFAULTS)
    fused.set_defaults(dtype="fp32", mask_mode="none", seed=11)
    yield fused
    fused.set_defaults(**keep)


def _nets(recnn, cuda, algo):
    torch.manual_seed(3)
    pol = recnn.nn.Actor(16, 8, 32, 6e-1)
    nets = {"policy_net": pol, "target_policy_net": copy.deepcopy(pol)}
    for k in (("value_net",) if algo == "ddpg" else ("value_net1", "value_net2")):
        nets[k] = recnn.nn.Critic(16, 8, 32, 54e-2)
        nets["target_" + k] = copy.deepcopy(nets[k])
    return {k: v.to(cuda).eval() for k, v in nets.items()}


def _update(recnn, fused, cuda, algo, env, step, attached):
    """One update call on the GRU user batch (attached) or on its detached rows, from the same fresh networks and the same noise.
    Returns (losses, gradients as they arrived at batch["state"], GRU parameters before the call)."""
    nets = _nets(recnn, cuda, algo)
    par = lambda n: list(nets[n].parameters())
    enc = list(env.state_encoder.parameters())
    optimizer = {"policy_optimizer": torch.optim.SGD(par("policy_net") + (enc if attached else []), lr=UPDATE_LR)}
    for k in nets:
        if k.startswith("value_net"):
            optimizer[k.replace("net", "optimizer")] = torch.optim.SGD(par(k), lr=1e-2)
    batch = env.user_batch(UPDATE_IDS, UPDATE_STEPS)
    assert batch["state"].requires_grad
    seen = []
    if attached:
        batch["state"].register_hook(lambda t: seen.append(t.detach().clone()))
    else:
        batch = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in batch.items()}
    before = {n: getattr(env.state_encoder, n).detach().clone() for n in G.PARAMS}
    if algo == "ddpg":
        loss = recnn.nn.update.ddpg_update(batch, DDPG_PARAMS, nets, optimizer, learn=True, step=step)
    else:
        noise = torch.randn(20, 8, generator=torch.Generator().manual_seed(17)) * TD3_PARAMS["noise_std"]
        with fused.external_randomness(nets, noise=noise, algo="td3"):
            loss = recnn.nn.update.td3_update(batch, TD3_PARAMS, nets, optimizer, learn=True, step=step)
    return loss, seen, before


@pytest.mark.parametrize("algo", ["ddpg", "td3"])
def test_updates_train_the_gru_through_an_attached_state(cuda, defaults, algo):
    import recnn
    table, user_dict, users, gru = G.gru_env_data()
    U, T = len(UPDATE_IDS), UPDATE_STEPS[-1] + 1
    x = R.lstm_inputs(table, [user_dict[u]["items"] for u in UPDATE_IDS], [user_dict[u]["ratings"] for u in UPDATE_IDS], T)
    prev = [t - 1 for t in UPDATE_STEPS]

    # ---- a policy step: policy_optimizer.zero_grad() precedes the last arrival, so the step applies that arrival's BPTT alone
    env = _env(cuda, table, user_dict, users, gru)
    loss, seen, before = _update(recnn, defaults, cuda, algo, env, 0, True)
    assert len(seen) == 2 and seen[-1].shape == (20, 16) and bool(torch.isfinite(seen[-1]).all()) and float(seen[-1].abs().max()) > 0
    g = seen[-1].cpu().view(len(UPDATE_STEPS), U, 16).transpose(0, 1)             # rows k U + u -> [U, K, H]

    def grads(dtype):
        ref = G.cpu_copy(gru, dtype)
        out, _ = ref(x.to(dtype))
        (out[:, prev] * g.to(dtype)).sum().backward()                             # state rows are h_{t - 1} of the kept steps
        return {n: getattr(ref, n).grad for n in G.PARAMS}

    g64, g32 = grads(torch.float64), grads(torch.float32)
    bounds = G._bounds(g32, g64, U, T)
    got = {n: ((before[n] - getattr(env.state_encoder, n).detach()) / UPDATE_LR).cpu() for n in G.PARAMS}
    _check(f"{algo} policy step: GRU parameter change / -lr", got, g64, bounds)
    assert all(float(g64[n].abs().max()) > 0 for n in G.PARAMS)
    print(f"{algo} step 0 losses attached {loss}")
    detached_loss, _, _ = _update(recnn, defaults, cuda, algo, _env(cuda, table, user_dict, users, gru), 0, False)
    print(f"{algo} step 0 losses detached {detached_loss}")
    assert loss == detached_loss and all(np.isfinite(v) for v in loss.values())

    # ---- not a policy step: the policy optimizer is not stepped, the GRU stays where it was
    env = _env(cuda, table, user_dict, users, gru)
    loss, seen, before = _update(recnn, defaults, cuda, algo, env, 1, True)
    assert len(seen) == 1
    for n in G.PARAMS:
        assert torch.equal(getattr(env.state_encoder, n).detach(), before[n]), n
        assert getattr(env.state_encoder, n).grad is not None                     # the value loss's BPTT did arrive
    detached_loss, _, _ = _update(recnn, defaults, cuda, algo, _env(cuda, table, user_dict, users, gru), 1, False)
    print(f"{algo} step 1 losses attached {loss} detached {detached_loss}")
    assert loss == detached_loss


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_by_name(cuda, seq_data):
    import warnings
    from recnn_amd import _lib as L
    from recnn_amd.data.env import SeqEnv
    from recnn_amd.nn import functional as F
    st, tbl, gl = _on_gpu(cuda, seq_data[(8, 16)])
    with pytest.raises(L.RecnnHipError, match="table.requires_grad"):
        F.gru_encode_train(gl, st, tbl.clone().requires_grad_(True), [0, 1], 4)
    with pytest.raises(L.RecnnHipError, match="weight_ih_l0.device"):
        F.gru_encode_train(torch.nn.GRU(9, 16), st, tbl, [0, 1], 4)
    for kw, attr in ((dict(num_layers=2), "num_layers"), (dict(bidirectional=True), "bidirectional"),
                     (dict(num_layers=1, dropout=0.5), "dropout"), (dict(bias=False), "bias")):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            bad = torch.nn.GRU(9, 16, **kw).to(cuda)
        for fn in (F.gru_encode, F.gru_encode_train):
            with pytest.raises(L.RecnnHipError, match=attr):
                fn(bad, st, tbl, [0, 1], 4)
    with pytest.raises(L.RecnnHipError, match="input_size"):
        F.gru_encode(torch.nn.GRU(10, 16).to(cuda), st, tbl, [0, 1], 4)
    strided = _gpu_gru(cuda, seq_data[(8, 16)][3])
    strided.weight_hh_l0.data = strided.weight_hh_l0.data.t().contiguous().t()
    with pytest.raises(L.RecnnHipError, match="weight_hh_l0"):
        F.gru_encode(strided, st, tbl, [0, 1], 4)
    with pytest.raises(L.RecnnHipError, match="weight_ih_l0"):
        F.gru_encode(_gpu_gru(cuda, seq_data[(8, 16)][3]).double(), st, tbl, [0, 1], 4)
    # the other cell, on the GPU: refused by type before any kernel reads 4H rows of a 3H matrix
    lstm = torch.nn.LSTM(9, 16).to(cuda)
    for fn in (F.lstm_encode, F.lstm_encode_train):
        with pytest.raises(L.RecnnHipError, match="GRU.*gru_encode"):
            fn(gl, st, tbl, [0, 1], 4)
    for fn in (F.gru_encode, F.gru_encode_train):
        with pytest.raises(L.RecnnHipError, match="LSTM.*lstm_encode"):
            fn(lstm, st, tbl, [0, 1], 4)
    table, user_dict, users, _ = G.gru_env_data()
    with pytest.raises(TypeError, match="RNN"):
        SeqEnv.from_user_dict(table, user_dict, users, state_encoder=torch.nn.RNN(9, 16).to(cuda), batch_size=5, device=cuda)
    h, _ = F.gru_encode_train(gl, st, tbl, [0, 1], 4)
    # a loss whose gradient with respect to h itself depends on h: only then does the first backward hand out a graph to refuse
    (g,) = torch.autograd.grad((h * h).sum(), gl.weight_hh_l0, create_graph=True)
    assert g.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
