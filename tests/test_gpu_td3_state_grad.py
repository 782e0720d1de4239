"""The TD3 step's input gradients on the GPU (csrc/state_grad.hip with per-segment seeds, recnn_engine_state_grads which = 0..3 on a
TD3 engine) and the route of `td3_update` that hands them to autograd, so that the TD3 losses train an LSTM state encoder.

Bounds and helpers are those of tests/test_gpu_state_grad.py: kernel tests compare with the float64 product of the very buffers the
launch read, bound (n + 4) 2^-24 (|dz| |W|)[r, s] per element with n the contraction length (H for one critic, 2 H for the merged
launch and the policy loss's); end-to-end tests compare the encoder's gradients with the reference update in float64 on the CPU
(tests/td3_state_grad_reference.py: two separate value backwards) in relative Frobenius error, bound
max(4 ||G32cpu - G64|| / ||G64||, 2^-23 max(8, sqrt(U T))).  Every test prints its figures before it asserts."""
import copy

import numpy as np
import pytest
import torch

import td3_state_grad_reference as TG
from helpers import fro_err
from oracle import recnn_oracle as O
from test_gpu_state_grad import (KERNEL_SHAPES, _check_product, _env, _mk, _small_case, _w_seen, _wide_case,  # noqa: F401
                                 check_vector_store_tail, defaults, seeded)

pytestmark = pytest.mark.gpu

PARAMS = {"gamma": 0.99, "noise_std": 0.5, "noise_clip": 0.7, "soft_tau": 0.01, "policy_update": 2}


# ---------------------------------------------------------------------------------------------------- 1: the launch itself
def _td3_engine(cuda, shape, dtype, algo="td3"):
    from recnn_amd import _lib as L
    from recnn_amd.nn.engine import StepEngine
    rows, S, A, H = shape
    gen = torch.Generator().manual_seed(S + 1)
    actor, critic1, critic2 = _mk(gen, H, S, A), _mk(gen, H, S + A, 1), _mk(gen, H, S + A, 1)
    batch = [torch.randn(rows, S, generator=gen), torch.randn(rows, A, generator=gen), torch.randn(rows, generator=gen),
             torch.randn(rows, S, generator=gen), (torch.rand(rows, generator=gen) < 0.1).float()]
    td3 = algo == "td3"
    masks = [(torch.rand(rows, H, generator=gen) < 0.5).to(torch.uint8) for _ in range(8 if td3 else 6)]
    noise = torch.randn(rows, A, generator=gen) * 0.5
    eng = StepEngine(algo, S, A, H, max(rows, 64), dtype=dtype, mask_mode="external", device=cuda)
    loads = [(L.NET_POLICY, actor), (L.NET_TARGET_POLICY, actor), (L.NET_VALUE1, critic1), (L.NET_TARGET_VALUE1, critic1)]
    if td3:
        loads += [(L.NET_VALUE2, critic2), (L.NET_TARGET_VALUE2, critic2)]
    for ni, p in loads:
        eng.load_params(ni, p)
    eng.set_hyper(policy_every=1, policy_opt=dict(lr=1e-3), value_opt=dict(lr=0.1))
    eng.set_counters()
    eng.pack_batch(*batch)
    eng.set_external(masks=masks, noise=noise if td3 else None)
    return eng


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES)          # (70, 70, 128, 232) bf16: the fold's segments each end 8 into a 32-wide stage
def test_kernel_against_its_own_buffers(cuda, shape, dtype):
    from recnn_amd import _lib as L
    rows, S, A, H = shape
    eng = _td3_engine(cuda, shape, dtype)
    for which in (0, 2, 3):
        with pytest.raises(L.RecnnHipError, match="value_grads"):       # nothing to read yet
            eng.state_grads(rows, which)

    # ---- which = 0, 2, 3 against the critics as they are BEFORE their steps
    eng.value_grads(rows, True)
    unit = int(eng.lib.recnn_engine_unit_backward(eng.handle))
    print(f"{shape} {dtype}: unit backward tensors (per-segment seeds in the merged launch): {unit}")
    assert unit == int(seeded(shape, dtype))      # the cases that cover the seeded fold really fold (K = 256, and K = 232: a partly masked last stage)
    w_old = [_w_seen(eng.param_views(ni)["w1"][:, :S].clone(), dtype) for ni in (L.NET_VALUE1, L.NET_VALUE2)]
    g0, g2, g3 = eng.state_grads(rows, 0), eng.state_grads(rows, 2), eng.state_grads(rows, 3)
    dz = [eng.buffer("critic1_dz1", rows), eng.buffer("critic2_dz1", rows)]
    assert float(dz[0].abs().max()) > 0 and float(dz[1].abs().max()) > 0 and not torch.equal(dz[0], dz[1])
    r0, _, b0 = _check_product(f"gV1 {shape} {dtype}", g0, [(dz[0], w_old[0])], H)
    r2, _, b2 = _check_product(f"gV2 {shape} {dtype}", g2, [(dz[1], w_old[1])], H)
    r3, _, b3 = _check_product(f"gV1+gV2 {shape} {dtype}", g3, [(dz[0], w_old[0]), (dz[1], w_old[1])], 2 * H)
    same_bits = torch.equal(g3, eng.state_grads(rows, 3))                 # two launches, the same bits
    rsum = float(((g3.double().cpu() - (g0.double().cpu() + g2.double().cpu())).abs() / (b0 + b2 + b3).clamp_min(1e-300)).max())
    print(f"|g3 - (g0 + g2)| / (sum of the three bounds) {shape} {dtype}: {rsum:.3f}")
    wide = torch.full((rows, S + 5), 7.0, device=cuda)
    eng.state_grads(rows, 3, out=wide)
    pad_ok = torch.equal(wide[:, :S], g3) and bool((wide[:, S:] == 7.0).all())
    vec_ok = all(check_vector_store_tail(cuda, eng, rows, which, g) for which, g in ((0, g0), (2, g2), (3, g3)))
    with pytest.raises(L.RecnnHipError, match="policy_grads"):
        eng.state_grads(rows, 1)

    # ---- the value steps (Adam, lr 0.1: every weight moves by about 0.1): the pre-step critics are gone
    eng.value_apply(False)
    for which in (0, 2, 3):
        with pytest.raises(L.RecnnHipError, match="value_grads"):
            eng.state_grads(rows, which)
    eng.policy_grads(rows, True)
    gp = eng.state_grads(rows, 1)
    assert torch.equal(gp, eng.state_grads(rows, 1))
    vec_ok = vec_ok and check_vector_store_tail(cuda, eng, rows, 1, gp)
    w_new = [_w_seen(eng.param_views(ni)["w1"][:, :S].clone(), dtype) for ni in (L.NET_VALUE1, L.NET_VALUE2)]
    w1a = _w_seen(eng.param_views(L.NET_POLICY)["w1"].clone(), dtype)
    assert float((w_new[0] - w_old[0]).abs().mean()) > 0.05 and float((w_new[1] - w_old[1]).abs().mean()) > 0.05
    dze1, dzp1 = eng.buffer("dze1", rows), eng.buffer("dzp1", rows)
    assert float(dze1.abs().max()) > 0 and float(dzp1.abs().max()) > 0
    rp, _, _ = _check_product(f"gP {shape} {dtype}", gp, [(dze1, w_new[0]), (dzp1, w1a)], 2 * H)
    # the other critic in either place misses by orders of magnitude
    r_old, _, _ = _check_product(f"gP with the pre-step critic 1 {shape} {dtype}", gp, [(dze1, w_old[0]), (dzp1, w1a)], 2 * H)
    r_new, _, _ = _check_product(f"gV1+gV2 with the updated critics {shape} {dtype}", g3, [(dz[0], w_new[0]), (dz[1], w_new[1])], 2 * H)
    eng.finish(rows, True, False)

    # ---- one row
    eng.value_grads(1, True)
    g1 = eng.state_grads(1, 3)
    w_now = [_w_seen(eng.param_views(ni)["w1"][:, :S].clone(), dtype) for ni in (L.NET_VALUE1, L.NET_VALUE2)]
    r1, _, _ = _check_product(f"gV1+gV2 rows=1 {shape} {dtype}", g1,
                              [(eng.buffer("critic1_dz1", 1), w_now[0]), (eng.buffer("critic2_dz1", 1), w_now[1])], 2 * H)
    eng.finish(1, False, False)
    torch.cuda.synchronize()
    assert r0 <= 1.0 and r2 <= 1.0 and r3 <= 1.0 and rp <= 1.0 and r1 <= 1.0
    assert same_bits and pad_ok and vec_ok
    assert rsum <= 1.0
    assert r_old > 100.0 and r_new > 100.0


# ---------------------------------------------------------------------------------------------------- 2: refusals
def _nets(recnn, cuda, S, A, H):
    pol = recnn.nn.Actor(S, A, H, 6e-1)
    v1, v2 = recnn.nn.Critic(S, A, H, 54e-2), recnn.nn.Critic(S, A, H, 54e-2)
    nets = {"policy_net": pol, "value_net1": v1, "value_net2": v2, "target_policy_net": copy.deepcopy(pol).eval(),
            "target_value_net1": copy.deepcopy(v1).eval(), "target_value_net2": copy.deepcopy(v2).eval()}
    return {k: v.to(cuda) for k, v in nets.items()}


def _sgd(pol, enc, v1, v2):
    return torch.optim.SGD(pol + enc, lr=1e-2), torch.optim.SGD(v1, lr=1e-2), torch.optim.SGD(v2, lr=1e-2)


def _opt_dict(opts):
    return dict(zip(("policy_optimizer", "value_optimizer1", "value_optimizer2"), opts))


def test_refusals(cuda, defaults):
    import recnn
    from recnn_amd import _lib as L
    eng = _td3_engine(cuda, (37, 27, 8, 16), "fp32", algo="ddpg")
    eng.value_grads(37, True)
    eng.state_grads(37, 0)
    for which in (2, 3):
        with pytest.raises(L.RecnnHipError, match="DDPG"):
            eng.state_grads(37, which)
    eng.finish(37, False, False)
    with pytest.raises(KeyError):
        eng.buffer("critic2_dz1", 4)
    eng = _td3_engine(cuda, (37, 27, 8, 16), "fp32")
    eng.value_grads(37, True)
    with pytest.raises(L.RecnnHipError, match="which"):
        eng.state_grads(37, 4)
    eng.finish(37, False, False)

    # a bf16x3 context with an attached state
    defaults.set_defaults(dtype="bf16x3", mask_mode="none")
    torch.manual_seed(0)
    nets = _nets(recnn, cuda, 32, 32, 32)
    par = lambda n: list(nets[n].parameters())
    opt = _opt_dict(_sgd(par("policy_net"), [], par("value_net1"), par("value_net2")))
    g = torch.Generator().manual_seed(1)
    batch = {"state": torch.randn(6, 32, generator=g).to(cuda).requires_grad_(True), "action": torch.randn(6, 32, generator=g).to(cuda),
             "reward": torch.randn(6, generator=g).to(cuda), "next_state": torch.randn(6, 32, generator=g).to(cuda),
             "done": torch.zeros(6, device=cuda)}
    with pytest.raises(L.RecnnHipError, match="bf16x3"):
        recnn.nn.update.td3_update(batch, PARAMS, nets, opt, learn=True, step=0)
    assert batch["state"].grad is None

    # a value optimizer that also holds the encoder: refused before anything is launched or changed
    defaults.set_defaults(dtype="fp32", mask_mode="none")
    torch.manual_seed(0)
    nets = _nets(recnn, cuda, 32, 32, 32)
    enc = torch.nn.Linear(32, 32).to(cuda)
    par = lambda n: list(nets[n].parameters())
    opt = {"policy_optimizer": torch.optim.Adam(par("policy_net"), lr=1e-2), "value_optimizer1": torch.optim.Adam(par("value_net1"), lr=1e-2),
           "value_optimizer2": torch.optim.Adam(par("value_net2") + list(enc.parameters()), lr=1e-2)}
    batch["state"] = enc(batch["state"].detach())
    before = {k: [p.detach().clone() for p in m.parameters()] for k, m in nets.items()}
    enc_before = [p.detach().clone() for p in enc.parameters()]
    with pytest.raises(L.RecnnHipError, match="value_optimizer2"):
        recnn.nn.update.td3_update(batch, PARAMS, nets, opt, learn=True, step=0)
    assert all(torch.equal(a, b) for k, m in nets.items() for a, b in zip(before[k], m.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(enc_before, enc.parameters())) and all(p.grad is None for p in enc.parameters())
    assert all(len(o.state) == 0 for o in opt.values())
    # ... and the same call is taken once the encoder sits in the policy optimizer
    opt = {"policy_optimizer": torch.optim.Adam(par("policy_net") + list(enc.parameters()), lr=1e-2),
           "value_optimizer1": torch.optim.Adam(par("value_net1"), lr=1e-2), "value_optimizer2": torch.optim.Adam(par("value_net2"), lr=1e-2)}
    recnn.nn.update.td3_update(batch, PARAMS, nets, opt, learn=True, step=0)
    assert not torch.equal(enc_before[0], enc.weight)


# ---------------------------------------------------------------------------------------------------- 3, 4: end to end
def _snapshot(nets):
    return {k: O.params_from_module(nets[k]) for k in TG.NET_KEYS}


def _reference(case, snap, masks, noise, step, make_opts=_sgd):
    """{dtype: (encoder gradients, parameters after the update)} of one reference update on the case's user batch."""
    out = {}
    for dt in (torch.float64, torch.float32):
        ref = TG.RefTD3(dt, case["table"], case["user_dict"], case["lstm"], snap, make_opts, PARAMS)
        ref.update(ref.batch(case["ids"], case["steps"]), masks, noise, step)
        out[dt] = (ref.encoder_grads(), ref.net_params())
    return out


def _check_encoder_grads(tag, enc, ref, U, T):
    bad = []
    for n in TG.LSTM_PARAMS:
        g = getattr(enc, n).grad
        assert g is not None, f"{tag}: {n}.grad is None -- the update sent no gradient into the state"
        g64, g32 = ref[torch.float64][0][n], ref[torch.float32][0][n]
        err, bound = TG.fro(g.cpu(), g64), TG.grad_bound(g32, g64, U, T)
        print(f"{tag} {n}: rel Frobenius err {err:.3e} bound {bound:.3e} ||G64|| {float(g64.norm()):.3e}")
        assert float(g64.norm()) > 0
        if not err <= bound:
            bad.append((n, err, bound))
    assert not bad, (tag, bad)


def _check_nets(tag, nets, ref64):
    for n in TG.NET_KEYS:
        got = O.params_from_module(nets[n])
        for k in O.PARAM_ORDER:
            e = fro_err(got[k], ref64[n][k])
            assert e < 3e-3, (tag, n, k, e)       # the bound tests/test_gpu_api.py holds the networks to


def _run_update(recnn, fused, cuda, case, train, step):
    S, A, H = case["dims"]
    fused.set_defaults(mask_mode="hash" if train else "none")
    torch.manual_seed(3)
    nets = _nets(recnn, cuda, S, A, H)
    if not train:
        for m in nets.values():
            m.eval()
    snap = _snapshot(nets)
    env = _env(cuda, case["table"], case["user_dict"], case["users"], case["lstm"], len(case["ids"]))
    rows = len(case["ids"]) * len(case["steps"])
    g = torch.Generator().manual_seed(17)
    masks = [(torch.rand(rows, H, generator=g) < 0.5).to(torch.uint8) for _ in range(8)] if train else None
    noise = torch.randn(rows, A, generator=g) * PARAMS["noise_std"]
    par = lambda n: list(nets[n].parameters())
    optimizer = _opt_dict(_sgd(par("policy_net"), list(env.state_encoder.parameters()), par("value_net1"), par("value_net2")))
    batch = env.user_batch(case["ids"], case["steps"])
    assert batch["state"].requires_grad
    seen = {"state": [], "next_state": []}
    batch["state"].register_hook(lambda t: seen["state"].append(t.clone()))
    batch["next_state"].register_hook(lambda t: seen["next_state"].append(t.clone()) if t is not None else None)
    with fused.external_randomness(nets, masks=masks, noise=noise, algo="td3"):
        loss = recnn.nn.update.td3_update(batch, PARAMS, nets, optimizer, learn=True, step=step)
    return nets, env, snap, masks, noise, seen, loss


def _bits(nets, name):
    return {k: v.clone() for k, v in O.params_from_module(nets[name]).items()}


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_end_to_end_small(cuda, defaults, mode):
    import recnn
    case = _small_case()
    U, T = len(case["ids"]), case["steps"][-1] + 1
    # ---- a policy step: the encoder's .grad is the BPTT of the policy loss's gradient alone; the target policy net never moves
    nets, env, snap, masks, noise, seen, loss = _run_update(recnn, defaults, cuda, case, mode == "train", 0)
    ref = _reference(case, snap, masks, noise, 0)
    _check_encoder_grads(f"td3 small {mode} step 0", env.state_encoder, ref, U, T)
    _check_nets(f"td3 small {mode} step 0", nets, ref[torch.float64][1])
    assert len(seen["state"]) == 2 and not seen["next_state"]
    assert all(np.isfinite(loss[k]) for k in ("value1", "value2", "policy"))
    assert all(torch.equal(v, snap["target_policy_net"][k]) for k, v in _bits(nets, "target_policy_net").items())
    assert not torch.equal(_bits(nets, "policy_net")["w1"], snap["policy_net"]["w1"])
    assert not torch.equal(_bits(nets, "target_value_net2")["w1"], snap["target_value_net2"]["w1"])
    # ---- no policy step: exactly the sum of the two value losses' BPTT stays in .grad, the actor is not touched
    nets, env, snap, masks, noise, seen, _ = _run_update(recnn, defaults, cuda, case, mode == "train", 1)
    ref = _reference(case, snap, masks, noise, 1)
    _check_encoder_grads(f"td3 small {mode} step 1", env.state_encoder, ref, U, T)
    _check_nets(f"td3 small {mode} step 1", nets, ref[torch.float64][1])
    assert len(seen["state"]) == 1 and not seen["next_state"]
    for name in ("policy_net", "target_policy_net"):
        assert all(torch.equal(v, snap[name][k]) for k, v in _bits(nets, name).items()), name


def test_end_to_end_notebook_widths(cuda, defaults):
    import recnn
    case = _wide_case()
    nets, env, snap, masks, noise, seen, _ = _run_update(recnn, defaults, cuda, case, False, 0)
    ref = _reference(case, snap, masks, noise, 0)
    _check_encoder_grads("td3 wide eval step 0", env.state_encoder, ref, len(case["ids"]), case["steps"][-1] + 1)
    _check_nets("td3 wide eval step 0", nets, ref[torch.float64][1])
    assert len(seen["state"]) == 2 and not seen["next_state"]


# ---------------------------------------------------------------------------------------------------- 5: bf16 plumbing
def test_bf16_route_hands_autograd_the_launch_output(cuda, defaults):
    """bf16 engine, eval mode: the two gradients `td3_update` hands to autograd are bit for bit what recnn_engine_state_grads gives when
    the same phases are run by hand on a second, identical context.  (No accuracy claim for bf16 end to end: DESIGN.md 17.)"""
    import recnn
    from recnn_amd import _lib as L
    defaults.set_defaults(dtype="bf16")
    case = _small_case()
    nets, env, snap, _, noise, seen, _ = _run_update(recnn, defaults, cuda, case, False, 0)
    assert len(seen["state"]) == 2
    torch.manual_seed(3)
    twin = _nets(recnn, cuda, *case["dims"])
    for m in twin.values():
        m.eval()
    env2 = _env(cuda, case["table"], case["user_dict"], case["users"], case["lstm"], 5)
    with torch.no_grad():
        batch = env2.user_batch(case["ids"], case["steps"])
    vopts = [torch.optim.SGD(twin[n].parameters(), lr=1e-2) for n in ("value_net1", "value_net2")]
    ctx = defaults.context_for("td3", twin)
    assert ctx.dtype == "bf16"
    ctx.ensure(twin, batch["state"].shape[0])
    rows = ctx.load_batch(batch)
    ctx.set_hyper(PARAMS, None, None)
    ctx.external = (None, noise)
    ctx.apply_external(rows)
    eng = ctx.engine
    eng.value_grads(rows, True)
    gv = eng.state_grads(rows, 3)
    for ni, o in zip((L.NET_VALUE1, L.NET_VALUE2), vopts):
        ctx.attach_grads(ni)
        o.step()
        ctx.refresh_stepped(ni)
    eng.policy_grads(rows, True)
    gp = eng.state_grads(rows, 1)
    eng.finish(rows, False, False)
    assert float(gv.abs().max()) > 0 and float(gp.abs().max()) > 0
    ref = _reference(case, snap, None, noise, 0)
    for n in TG.LSTM_PARAMS:
        print(f"td3 bf16 route {n}: rel Frobenius err vs float64 {TG.fro(getattr(env.state_encoder, n).grad.cpu(), ref[torch.float64][0][n]):.3e}")
    assert torch.equal(seen["state"][0], gv) and torch.equal(seen["state"][1], gp)


# ---------------------------------------------------------------------------------------------------- 6: route coherence
def test_routes_alternate_coherently(cuda, defaults):
    """recnn_amd.optim.Adam in all three slots; updates 0 and 2 on a detached batch (Adam inside the engine), 1 and 3 on an attached one
    (the optimizers' own step() between the phases): one Adam state, one parameter trajectory, against the reference's four steps."""
    import recnn
    from recnn_amd.optim import Adam
    case = _small_case()
    U, T = len(case["ids"]), case["steps"][-1] + 1
    P = dict(PARAMS, policy_update=1)
    defaults.set_defaults(mask_mode="none")
    torch.manual_seed(3)
    nets = _nets(recnn, cuda, *case["dims"])
    for m in nets.values():
        m.eval()
    snap = _snapshot(nets)
    env = _env(cuda, case["table"], case["user_dict"], case["users"], case["lstm"], 5)
    optimizer = {"policy_optimizer": Adam(list(nets["policy_net"].parameters()) + list(env.state_encoder.parameters()), lr=1e-3),
                 "value_optimizer1": Adam(nets["value_net1"].parameters(), lr=1e-3),
                 "value_optimizer2": Adam(nets["value_net2"].parameters(), lr=1e-3)}
    rows, A = U * len(case["steps"]), case["dims"][1]
    g = torch.Generator().manual_seed(23)
    noises = [torch.randn(rows, A, generator=g) * P["noise_std"] for _ in range(4)]
    for step in range(4):
        if step % 2 == 0:
            with torch.no_grad():
                batch = env.user_batch(case["ids"], case["steps"])
            assert not batch["state"].requires_grad
        else:
            batch = env.user_batch(case["ids"], case["steps"])
            assert batch["state"].requires_grad
        with defaults.external_randomness(nets, noise=noises[step], algo="td3"):
            recnn.nn.update.td3_update(batch, P, nets, optimizer, learn=True, step=step)
    steps_seen = {k: int(optimizer[k].state[nets[n].linear1.weight]["step"]) for k, n in
                  (("value_optimizer1", "value_net1"), ("value_optimizer2", "value_net2"), ("policy_optimizer", "policy_net"))}
    enc_steps = int(optimizer["policy_optimizer"].state[env.state_encoder.weight_hh_l0]["step"])
    counters = defaults.context_for("td3", nets).engine.counters()
    print(f"routes: optimizer steps {steps_seen}, encoder steps {enc_steps}, engine counters (step, policy, value1, value2) {counters}")

    refs = {}
    for dt in (torch.float64, torch.float32):
        mk = lambda pol, enc, v1, v2: (torch.optim.Adam(pol + enc, lr=1e-3), torch.optim.Adam(v1, lr=1e-3), torch.optim.Adam(v2, lr=1e-3))
        ref = TG.RefTD3(dt, case["table"], case["user_dict"], case["lstm"], snap, mk, P)
        for step in range(4):
            ref.update(ref.batch(case["ids"], case["steps"], attached=step % 2 == 1), None, noises[step], step)
        refs[dt] = (ref.net_params(), {n: getattr(ref.lstm, n).detach().double() for n in TG.LSTM_PARAMS})
    bad = []
    for n in TG.NET_KEYS:
        got = O.params_from_module(nets[n])
        for k in O.PARAM_ORDER:
            err = TG.fro(got[k], refs[torch.float64][0][n][k])
            bound = TG.grad_bound(refs[torch.float32][0][n][k], refs[torch.float64][0][n][k], U, T)
            print(f"routes {n}.{k}: rel Frobenius err {err:.3e} bound {bound:.3e}")
            if not err <= bound:
                bad.append((n, k, err, bound))
    for n in TG.LSTM_PARAMS:
        err = TG.fro(getattr(env.state_encoder, n).detach().cpu(), refs[torch.float64][1][n])
        bound = TG.grad_bound(refs[torch.float32][1][n], refs[torch.float64][1][n], U, T)
        print(f"routes encoder {n}: rel Frobenius err {err:.3e} bound {bound:.3e}")
        if not err <= bound:
            bad.append(("encoder", n, err, bound))
        assert not torch.equal(getattr(env.state_encoder, n).detach().cpu(), getattr(case["lstm"], n).detach())    # it was trained
    assert steps_seen == {"value_optimizer1": 4, "value_optimizer2": 4, "policy_optimizer": 4} and enc_steps == 2
    assert counters[1:] == (4, 4, 4)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- 7: nothing leaks
def test_no_gradient_without_learn_or_grad_mode(cuda, defaults):
    """learn=False, torch.no_grad() and a detached state each give the losses and parameters of a run on state.detach(), bit for bit,
    and leave no .grad on the encoder."""
    import recnn
    case = _small_case()
    defaults.set_defaults(mask_mode="none")
    rows, A = len(case["ids"]) * len(case["steps"]), case["dims"][1]
    noise = torch.randn(rows, A, generator=torch.Generator().manual_seed(5)) * PARAMS["noise_std"]

    def run(kind):
        torch.manual_seed(3)
        nets = _nets(recnn, cuda, *case["dims"])
        for m in nets.values():
            m.eval()
        env = _env(cuda, case["table"], case["user_dict"], case["users"], case["lstm"], 5)
        par = lambda n: list(nets[n].parameters())
        optimizer = _opt_dict(_sgd(par("policy_net"), list(env.state_encoder.parameters()), par("value_net1"), par("value_net2")))
        batch = env.user_batch(case["ids"], case["steps"])
        learn = not kind.startswith("test")
        if kind in ("detached", "baseline", "test_baseline"):
            batch = dict(batch, state=batch["state"].detach())
        with defaults.external_randomness(nets, noise=noise, algo="td3"):
            if kind == "no_grad":
                with torch.no_grad():
                    loss = recnn.nn.update.td3_update(batch, PARAMS, nets, optimizer, learn=learn, step=0)
            else:
                loss = recnn.nn.update.td3_update(batch, PARAMS, nets, optimizer, learn=learn, step=0)
        assert all(p.grad is None for p in env.state_encoder.parameters()), kind
        return loss, {n: _bits(nets, n) for n in TG.NET_KEYS}

    base, test_base = run("baseline"), run("test_baseline")
    for kind, want in (("detached", base), ("no_grad", base), ("test_attached", test_base)):
        loss, params = run(kind)
        print(f"{kind}: losses {loss}")
        assert loss == want[0], (kind, loss, want[0])
        for n in TG.NET_KEYS:
            assert all(torch.equal(params[n][k], want[1][n][k]) for k in O.PARAM_ORDER), (kind, n)
