"""The DDPG step's input gradient on the GPU (csrc/state_grad.hip, recnn_engine_state_grads) and the route of `ddpg_update` that hands
it to autograd, so that the DDPG losses train an LSTM state encoder in front of the networks.

Kernel tests compare with the float64 product of the very buffers the launch read; the bound per element is
(n + 4) 2^-24 (|dz| |W|)[r, s], n the contraction length -- the worst case of any fp32 summation order.  End-to-end tests compare the
encoder's gradients with the reference update in float64 on the CPU (tests/state_grad_reference.py) in relative Frobenius error, bound
max(4 ||G32cpu - G64|| / ||G64||, 2^-23 max(8, sqrt(U T))).  Every test prints its figures before it asserts."""
import copy

import numpy as np
import pytest
import torch

import seq_reference as R
import state_grad_reference as SG
from helpers import fro_err, make_store
from oracle import recnn_oracle as O

pytestmark = pytest.mark.gpu

PARAMS = {"gamma": 0.99, "min_value": -10, "max_value": 10, "policy_step": 2, "soft_tau": 0.01}


@pytest.fixture
def defaults(cuda):
    """fused.DEFAULTS as this file needs them, put back afterwards."""
    from recnn_amd.nn import fused
    keep = dict(fused.DEFAULTS)
    fused.set_defaults(dtype="fp32", mask_mode="hash", seed=11)
    yield fused
    fused.set_defaults(**keep)


# ---------------------------------------------------------------------------------------------------- 1, 2: the launch itself
def _mk(gen, H, inp, out):
    return {"w1": torch.randn(H, inp, generator=gen) * 0.2, "b1": torch.randn(H, generator=gen) * 0.1,
            "w2": torch.randn(H, H, generator=gen) * 0.2, "b2": torch.randn(H, generator=gen) * 0.1,
            "w3": torch.randn(out, H, generator=gen) * 0.3, "b3": torch.randn(out, generator=gen) * 0.3}


def _w_seen(w, dtype):
    return (w.bfloat16() if dtype == "bf16" else w).double().cpu()


def _check_product(tag, got, terms, n):
    """got [rows, S] against sum of dz @ W over `terms` = [(dz, W)] in float64; returns (worst error / bound, reference)."""
    ref = sum(dz.double().cpu() @ w for dz, w in terms)
    bound = (n + 4) * 2.0 ** -24 * sum(dz.double().cpu().abs() @ w.abs() for dz, w in terms)
    err = (got.double().cpu() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{tag}: max err {float(err.max()):.3e}, max err / bound {ratio:.3f}, max |ref| {float(ref.abs().max()):.3e}")
    return ratio, ref, bound


# (rows, S, A, H).  The two ends of the range, then what lies between them:
#   (65, 27, 8, 16)       a second row tile with one live row: tile_m and the m0 offset into dz, the seeds and out are non-zero
#   (130, 1290, 128, 256) the notebook's state width: 21 column tiles, the last 10 wide, three row tiles, the scalar tail store at n = 1288
#   (100, 70, 8, 40)      K = 40 ends 8 into the second 32-wide stage; S = 70 leaves a second column tile 6 wide, and the bf16 16-byte W
#                         chunk at columns 64 .. 71 crosses S.  No seeds here: the engine leaves unit backward tensors only on its
#                         fused bf16 path (A = 128, H in 136 .. 256), so TD3's which = 3 is the plain two-segment launch at this shape
#   (70, 70, 128, 232)    the fused bf16 path with K % 32 != 0: seeded rows (the epilogue's seed here, TD3's FOLD at which = 3) whose
#                         segments end 8 into their eighth stage, in a second row tile (m0 = 64) and a second column tile 6 wide
KERNEL_SHAPES = [(37, 27, 8, 16), (50, 256, 128, 256), (65, 27, 8, 16), (130, 1290, 128, 256), (100, 70, 8, 40), (70, 70, 128, 232)]


def seeded(shape, dtype):
    """Whether the engine leaves unit backward tensors (dz / d, the per-row seed applied by the launch) at this shape: its fused bf16
    path, which needs A = 128 and H rounded up to 128 equal to 256."""
    return dtype == "bf16" and shape[2] == 128 and 128 < shape[3] <= 256


def check_vector_store_tail(cuda, eng, rows, which, plain):
    """A second `out=` whose rows take the 16-byte store path (row stride a multiple of 4 floats on a 16-byte-aligned base), so the
    vectorised store meets the n + 3 >= S tail in whichever column tile S ends in: bit for bit the plain result, sentinels untouched."""
    S = plain.shape[1]
    ld = (S + 3) // 4 * 4 + 4
    out = torch.full((rows, ld), 7.0, device=cuda)
    assert out.data_ptr() % 16 == 0 and out.stride(0) % 4 == 0
    eng.state_grads(rows, which, out=out)
    return torch.equal(out[:, :S], plain) and bool((out[:, S:] == 7.0).all())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_kernel_against_its_own_buffers(cuda, shape, dtype):
    from recnn_amd import _lib as L
    from recnn_amd.nn.engine import StepEngine
    rows, S, A, H = shape
    gen = torch.Generator().manual_seed(S)
    actor, critic = _mk(gen, H, S, A), _mk(gen, H, S + A, 1)
    batch = [torch.randn(rows, S, generator=gen), torch.randn(rows, A, generator=gen), torch.randn(rows, generator=gen),
             torch.randn(rows, S, generator=gen), (torch.rand(rows, generator=gen) < 0.1).float()]
    masks = [(torch.rand(rows, H, generator=gen) < 0.5).to(torch.uint8) for _ in range(6)]
    eng = StepEngine("ddpg", S, A, H, max(rows, 64), dtype=dtype, mask_mode="external", device=cuda)
    for ni, p in ((L.NET_POLICY, actor), (L.NET_TARGET_POLICY, actor), (L.NET_VALUE1, critic), (L.NET_TARGET_VALUE1, critic)):
        eng.load_params(ni, p)
    eng.set_hyper(policy_every=1, policy_opt=dict(lr=1e-3), value_opt=dict(lr=0.1))
    eng.set_counters()
    eng.pack_batch(*batch)
    eng.set_external(masks=masks)
    with pytest.raises(L.RecnnHipError, match="value_grads"):           # nothing to read yet
        eng.state_grads(rows, 0)

    # ---- which = 0, against the critic as it is BEFORE its step
    eng.value_grads(rows, True)
    unit = int(eng.lib.recnn_engine_unit_backward(eng.handle))
    print(f"{shape} {dtype}: unit backward tensors (the per-row seed in the launch's epilogue): {unit}")
    assert unit == int(seeded(shape, dtype))                              # the seeded cases are really seeded
    w1c_old = _w_seen(eng.param_views(L.NET_VALUE1)["w1"][:, :S].clone(), dtype)
    gv = eng.state_grads(rows, 0)
    assert torch.equal(gv, eng.state_grads(rows, 0))                      # two launches, the same bits
    wide = torch.full((rows, S + 5), 7.0, device=cuda)
    eng.state_grads(rows, 0, out=wide)
    assert torch.equal(wide[:, :S], gv) and bool((wide[:, S:] == 7.0).all())
    assert check_vector_store_tail(cuda, eng, rows, 0, gv)
    dzc1 = eng.buffer("critic1_dz1", rows)
    assert float(dzc1.abs().max()) > 0
    rv, _, _ = _check_product(f"gV {shape} {dtype}", gv, [(dzc1, w1c_old)], H)
    with pytest.raises(L.RecnnHipError, match="policy_grads"):
        eng.state_grads(rows, 1)

    # ---- the value step (Adam, lr 0.1: every weight moves by about 0.1), then which = 1 against the UPDATED critic
    eng.value_apply(False)
    with pytest.raises(L.RecnnHipError, match="value_grads"):           # the pre-step critic is gone
        eng.state_grads(rows, 0)
    eng.policy_grads(rows, True)
    gp = eng.state_grads(rows, 1)
    assert torch.equal(gp, eng.state_grads(rows, 1))
    assert check_vector_store_tail(cuda, eng, rows, 1, gp)
    w1c_new = _w_seen(eng.param_views(L.NET_VALUE1)["w1"][:, :S].clone(), dtype)
    w1a = _w_seen(eng.param_views(L.NET_POLICY)["w1"].clone(), dtype)
    assert float((w1c_new - w1c_old).abs().mean()) > 0.05
    dze1, dzp1 = eng.buffer("dze1", rows), eng.buffer("dzp1", rows)
    assert float(dze1.abs().max()) > 0 and float(dzp1.abs().max()) > 0
    rp, _, _ = _check_product(f"gP {shape} {dtype}", gp, [(dze1, w1c_new), (dzp1, w1a)], 2 * H)
    # the other critic in either place misses by orders of magnitude
    r_old, _, _ = _check_product(f"gP with the pre-step critic {shape} {dtype}", gp, [(dze1, w1c_old), (dzp1, w1a)], 2 * H)
    r_new, _, _ = _check_product(f"gV with the updated critic {shape} {dtype}", gv, [(dzc1, w1c_new)], H)
    eng.finish(rows, True, False)

    # ---- one row
    eng.value_grads(1, True)
    g1 = eng.state_grads(1, 0)
    w_now = _w_seen(eng.param_views(L.NET_VALUE1)["w1"][:, :S].clone(), dtype)
    r1, _, _ = _check_product(f"gV rows=1 {shape} {dtype}", g1, [(eng.buffer("critic1_dz1", 1), w_now)], H)
    eng.finish(1, False, False)
    torch.cuda.synchronize()
    assert rv <= 1.0 and rp <= 1.0 and r1 <= 1.0
    assert r_old > 100.0 and r_new > 100.0


def test_refusals(cuda, defaults):
    import recnn
    from recnn_amd import _lib as L
    from recnn_amd.nn.engine import StepEngine
    eng = StepEngine("td3", 27, 8, 16, 64, dtype="fp32", mask_mode="none", device=cuda)
    with pytest.raises(L.RecnnHipError, match="TD3"):
        eng.state_grads(4, 0)
    defaults.set_defaults(dtype="bf16x3", mask_mode="none")
    torch.manual_seed(0)
    nets = _nets(recnn, cuda, 32, 32, 32)
    opt = {"policy_optimizer": torch.optim.SGD(nets["policy_net"].parameters(), lr=1e-2),
           "value_optimizer": torch.optim.SGD(nets["value_net"].parameters(), lr=1e-2)}
    g = torch.Generator().manual_seed(1)
    batch = {"state": torch.randn(6, 32, generator=g).to(cuda).requires_grad_(True), "action": torch.randn(6, 32, generator=g).to(cuda),
             "reward": torch.randn(6, generator=g).to(cuda), "next_state": torch.randn(6, 32, generator=g).to(cuda),
             "done": torch.zeros(6, device=cuda)}
    with pytest.raises(L.RecnnHipError, match="bf16x3"):
        recnn.nn.update.ddpg_update(batch, PARAMS, nets, opt, learn=True, step=0)
    assert batch["state"].grad is None


# ---------------------------------------------------------------------------------------------------- 3, 4: end to end
def _nets(recnn, cuda, S, A, H):
    pol, val = recnn.nn.Actor(S, A, H, 6e-1), recnn.nn.Critic(S, A, H, 54e-2)
    nets = {"policy_net": pol, "value_net": val, "target_policy_net": copy.deepcopy(pol).eval(), "target_value_net": copy.deepcopy(val).eval()}
    return {k: v.to(cuda) for k, v in nets.items()}


def _snapshot(nets):
    return {k: O.params_from_module(nets[k]) for k in SG.NET_KEYS}


def _env(cuda, table, user_dict, users, lstm, batch_size):
    from recnn_amd.data.env import SeqEnv
    gl = torch.nn.LSTM(lstm.input_size, lstm.hidden_size).to(cuda)
    gl.load_state_dict(lstm.state_dict())
    return SeqEnv.from_user_dict(table, user_dict, users, state_encoder=gl, batch_size=batch_size, max_buf_size=4 * batch_size, device=cuda)


def _small_case():
    table, user_dict, users, lstm = R.seq_env_data()
    return dict(table=table, user_dict=user_dict, users=users, lstm=lstm, dims=(16, 8, 16), ids=[0, 1, 2, 3, 4], steps=[3, 7, 20])


def _wide_case():
    items, ratings, table = make_store(25, 300, 128, 8, 12, seed=7)
    user_dict = {u: {"items": items[u], "ratings": ratings[u].astype(np.float32)} for u in range(25)}
    torch.manual_seed(7)
    return dict(table=torch.from_numpy(table), user_dict=user_dict, users=list(range(25)), lstm=torch.nn.LSTM(129, 256),
                dims=(256, 128, 256), ids=list(range(25)), steps=[2, 5])


def _sgd(pol, enc, val):
    return torch.optim.SGD(pol + enc, lr=1e-2), torch.optim.SGD(val, lr=1e-2)


def _reference(case, snap, masks, step, make_opts=_sgd):
    """{dtype: (encoder gradients, parameters after the update)} of one reference update on the case's user batch."""
    out = {}
    for dt in (torch.float64, torch.float32):
        ref = SG.RefDDPG(dt, case["table"], case["user_dict"], case["lstm"], snap, make_opts, PARAMS)
        ref.update(ref.batch(case["ids"], case["steps"]), masks, step)
        out[dt] = (ref.encoder_grads(), {n: {k: v.detach().double() for k, v in ref.nets[n].items()} for n in SG.NET_KEYS})
    return out


def _check_encoder_grads(tag, enc, ref, U, T):
    bad = []
    for n in SG.LSTM_PARAMS:
        g = getattr(enc, n).grad
        assert g is not None, f"{tag}: {n}.grad is None -- the update sent no gradient into the state"
        g64, g32 = ref[torch.float64][0][n], ref[torch.float32][0][n]
        err, bound = SG.fro(g.cpu(), g64), SG.grad_bound(g32, g64, U, T)
        print(f"{tag} {n}: rel Frobenius err {err:.3e} bound {bound:.3e} ||G64|| {float(g64.norm()):.3e}")
        assert float(g64.norm()) > 0
        if not err <= bound:
            bad.append((n, err, bound))
    assert not bad, (tag, bad)


def _check_nets(tag, nets, ref64):
    for n in SG.NET_KEYS:
        got = O.params_from_module(nets[n])
        for k in O.PARAM_ORDER:
            e = fro_err(got[k], ref64[n][k])
            assert e < 3e-3, (tag, n, k, e)       # the bound tests/test_gpu_api.py holds the networks to


def _run_update(recnn, fused, cuda, case, train, step):
    S, A, H = case["dims"]
    torch.manual_seed(3)
    nets = _nets(recnn, cuda, S, A, H)
    if not train:
        for m in nets.values():
            m.eval()
    snap = _snapshot(nets)
    env = _env(cuda, case["table"], case["user_dict"], case["users"], case["lstm"], len(case["ids"]))
    rows = len(case["ids"]) * len(case["steps"])
    g = torch.Generator().manual_seed(17)
    masks = [(torch.rand(rows, H, generator=g) < 0.5).to(torch.uint8) for _ in range(6)] if train else None
    popt, vopt = _sgd(list(nets["policy_net"].parameters()), list(env.state_encoder.parameters()), list(nets["value_net"].parameters()))
    batch = env.user_batch(case["ids"], case["steps"])
    assert batch["state"].requires_grad
    seen = {"state": [], "next_state": []}
    batch["state"].register_hook(lambda t: seen["state"].append(t.clone()))
    # (a tensor hook of an output the backward pass has no gradient for may still be called, with None: what counts is that no
    # gradient TENSOR ever arrives at next_state)
    batch["next_state"].register_hook(lambda t: seen["next_state"].append(t.clone()) if t is not None else None)
    optimizer = {"policy_optimizer": popt, "value_optimizer": vopt}
    if train:
        with fused.external_randomness(nets, masks=masks):
            loss = recnn.nn.update.ddpg_update(batch, PARAMS, nets, optimizer, learn=True, step=step)
    else:
        loss = recnn.nn.update.ddpg_update(batch, PARAMS, nets, optimizer, learn=True, step=step)
    return nets, env, snap, masks, seen, loss


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_end_to_end_small(cuda, defaults, mode):
    import recnn
    case = _small_case()
    U, T = len(case["ids"]), case["steps"][-1] + 1
    # ---- a policy step: the encoder's .grad is the BPTT of the policy loss's gradient alone
    nets, env, snap, masks, seen, loss = _run_update(recnn, defaults, cuda, case, mode == "train", 0)
    ref = _reference(case, snap, masks, 0)
    _check_encoder_grads(f"small {mode} step 0", env.state_encoder, ref, U, T)
    _check_nets(f"small {mode} step 0", nets, ref[torch.float64][1])
    assert len(seen["state"]) == 2 and not seen["next_state"]
    assert np.isfinite(loss["value"]) and np.isfinite(loss["policy"])
    # ---- no policy step: exactly the value loss's BPTT stays in .grad, the actor is not touched
    nets, env, snap, masks, seen, _ = _run_update(recnn, defaults, cuda, case, mode == "train", 1)
    ref = _reference(case, snap, masks, 1)
    _check_encoder_grads(f"small {mode} step 1", env.state_encoder, ref, U, T)
    _check_nets(f"small {mode} step 1", nets, ref[torch.float64][1])
    assert len(seen["state"]) == 1 and not seen["next_state"]
    assert torch.equal(O.params_from_module(nets["policy_net"])["w1"], snap["policy_net"]["w1"])


def test_no_gradient_without_learn_or_grad_mode(cuda, defaults):
    import recnn
    case = _small_case()
    torch.manual_seed(3)
    nets = _nets(recnn, cuda, *case["dims"])
    env = _env(cuda, case["table"], case["user_dict"], case["users"], case["lstm"], 5)
    popt, vopt = _sgd(list(nets["policy_net"].parameters()), list(env.state_encoder.parameters()), list(nets["value_net"].parameters()))
    optimizer = {"policy_optimizer": popt, "value_optimizer": vopt}
    recnn.nn.update.ddpg_update(env.user_batch(case["ids"], case["steps"]), PARAMS, nets, optimizer, learn=False, step=0)
    assert all(p.grad is None for p in env.state_encoder.parameters())
    with torch.no_grad():
        recnn.nn.update.ddpg_update(env.user_batch(case["ids"], case["steps"]), PARAMS, nets, optimizer, learn=True, step=0)
    assert all(p.grad is None for p in env.state_encoder.parameters())
    batch = env.user_batch(case["ids"], case["steps"])
    recnn.nn.update.ddpg_update(dict(batch, state=batch["state"].detach()), PARAMS, nets, optimizer, learn=True, step=0)
    assert all(p.grad is None for p in env.state_encoder.parameters())


def test_end_to_end_notebook_widths(cuda, defaults):
    import recnn
    case = _wide_case()
    nets, env, snap, masks, seen, _ = _run_update(recnn, defaults, cuda, case, False, 0)
    ref = _reference(case, snap, masks, 0)
    _check_encoder_grads("wide eval step 0", env.state_encoder, ref, len(case["ids"]), case["steps"][-1] + 1)
    _check_nets("wide eval step 0", nets, ref[torch.float64][1])
    assert len(seen["state"]) == 2 and not seen["next_state"]


# ---------------------------------------------------------------------------------------------------- 5: route coherence
def test_routes_alternate_coherently(cuda, defaults):
    """recnn_amd.optim.Adam in both slots; updates 0 and 2 on a detached batch (Adam inside the engine), 1 and 3 on an attached one (the
    optimizers' own step() between the phases): one Adam state, one parameter trajectory, against the reference's four steps."""
    import recnn
    from recnn_amd.optim import Adam
    case = _small_case()
    U, T = len(case["ids"]), case["steps"][-1] + 1
    P = dict(PARAMS, policy_step=1)
    torch.manual_seed(3)
    nets = _nets(recnn, cuda, *case["dims"])
    for m in nets.values():
        m.eval()
    snap = _snapshot(nets)
    env = _env(cuda, case["table"], case["user_dict"], case["users"], case["lstm"], 5)
    optimizer = {"policy_optimizer": Adam(list(nets["policy_net"].parameters()) + list(env.state_encoder.parameters()), lr=1e-3),
                 "value_optimizer": Adam(nets["value_net"].parameters(), lr=1e-3)}
    # a second pair of contexts that only ever see detached batches: one stepped in between the attached updates, one afterwards
    frozen_batch = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in env.user_batch(case["ids"], case["steps"]).items()}

    def detached_only():
        torch.manual_seed(4)
        n = _nets(recnn, cuda, *case["dims"])
        for m in n.values():
            m.eval()
        return n, {"policy_optimizer": Adam(n["policy_net"].parameters(), lr=1e-3), "value_optimizer": Adam(n["value_net"].parameters(), lr=1e-3)}

    side, side_opt = detached_only()
    for step in range(4):
        if step % 2 == 0:
            with torch.no_grad():
                batch = env.user_batch(case["ids"], case["steps"])
            assert not batch["state"].requires_grad
        else:
            batch = env.user_batch(case["ids"], case["steps"])
            assert batch["state"].requires_grad
        recnn.nn.update.ddpg_update(batch, P, nets, optimizer, learn=True, step=step)
        recnn.nn.update.ddpg_update(frozen_batch, P, side, side_opt, learn=True, step=step)
    st = optimizer["value_optimizer"].state[nets["value_net"].linear1.weight]
    assert int(st["step"]) == 4 and int(optimizer["policy_optimizer"].state[env.state_encoder.weight_hh_l0]["step"]) == 2

    refs = {}
    for dt in (torch.float64, torch.float32):
        ref = SG.RefDDPG(dt, case["table"], case["user_dict"], case["lstm"], snap,
                         lambda pol, enc, val: (torch.optim.Adam(pol + enc, lr=1e-3), torch.optim.Adam(val, lr=1e-3)), P)
        for step in range(4):
            ref.update(ref.batch(case["ids"], case["steps"], attached=step % 2 == 1), None, step)
        refs[dt] = ({n: {k: v.detach().double() for k, v in ref.nets[n].items()} for n in SG.NET_KEYS},
                    {n: getattr(ref.lstm, n).detach().double() for n in SG.LSTM_PARAMS})
    bad = []
    for n in SG.NET_KEYS:
        got = O.params_from_module(nets[n])
        for k in O.PARAM_ORDER:
            err = SG.fro(got[k], refs[torch.float64][0][n][k])
            bound = SG.grad_bound(refs[torch.float32][0][n][k], refs[torch.float64][0][n][k], U, T)
            print(f"routes {n}.{k}: rel Frobenius err {err:.3e} bound {bound:.3e}")
            if not err <= bound:
                bad.append((n, k, err, bound))
    for n in SG.LSTM_PARAMS:
        err = SG.fro(getattr(env.state_encoder, n).detach().cpu(), refs[torch.float64][1][n])
        bound = SG.grad_bound(refs[torch.float32][1][n], refs[torch.float64][1][n], U, T)
        print(f"routes encoder {n}: rel Frobenius err {err:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append(("encoder", n, err, bound))
        assert not torch.equal(getattr(env.state_encoder, n).detach().cpu(), getattr(case["lstm"], n).detach())    # it was trained
    # the detached-only context: the same four calls with no attached update anywhere near give the same bits
    after, after_opt = detached_only()
    for step in range(4):
        recnn.nn.update.ddpg_update(frozen_batch, P, after, after_opt, learn=True, step=step)
    for n in SG.NET_KEYS:
        for a, b in zip(side[n].parameters(), after[n].parameters()):
            assert torch.equal(a, b), n
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- 6: bf16 plumbing
def test_bf16_route_hands_autograd_the_launch_output(cuda, defaults):
    """bf16 engine, eval mode: the two gradients `ddpg_update` hands to autograd are bit for bit what recnn_engine_state_grads gives when the
    same phases are run by hand on a second, identical context.  (No accuracy claim for bf16 end to end: DESIGN.md 16 has the figures.)"""
    import recnn
    from recnn_amd import _lib as L
    defaults.set_defaults(dtype="bf16", mask_mode="none")
    case = _small_case()
    nets, env, snap, _, seen, _ = _run_update(recnn, defaults, cuda, case, False, 0)
    assert len(seen["state"]) == 2
    # by hand: fresh copies of the same networks, the same (detached) rows, the same SGD step between the phases
    torch.manual_seed(3)
    twin = _nets(recnn, cuda, *case["dims"])
    for m in twin.values():
        m.eval()
    env2 = _env(cuda, case["table"], case["user_dict"], case["users"], case["lstm"], 5)
    with torch.no_grad():
        batch = env2.user_batch(case["ids"], case["steps"])
    vopt = torch.optim.SGD(twin["value_net"].parameters(), lr=1e-2)
    ctx = defaults.context_for("ddpg", twin)
    assert ctx.dtype == "bf16"
    ctx.ensure(twin, batch["state"].shape[0])
    rows = ctx.load_batch(batch)
    ctx.set_hyper(PARAMS, None, None)
    ctx.apply_external(rows)
    eng = ctx.engine
    eng.value_grads(rows, True)
    gv = eng.state_grads(rows, 0)
    ctx.attach_grads(L.NET_VALUE1)
    vopt.step()
    ctx.refresh_stepped(L.NET_VALUE1)
    eng.policy_grads(rows, True)
    gp = eng.state_grads(rows, 1)
    eng.finish(rows, False, False)
    assert float(gv.abs().max()) > 0 and float(gp.abs().max()) > 0
    assert torch.equal(seen["state"][0], gv) and torch.equal(seen["state"][1], gp)
    # information only: the bf16 route's encoder gradients against the float64 reference
    ref = _reference(case, snap, None, 0)
    for n in SG.LSTM_PARAMS:
        print(f"bf16 route {n}: rel Frobenius err vs float64 {SG.fro(getattr(env.state_encoder, n).grad.cpu(), ref[torch.float64][0][n]):.3e}")
