"""The optimizer passes held to float64, ELEMENT BY ELEMENT: csrc/optim_dev.h apply_body (apply_kernel / apply_gather_kernel; Adam or
Ranger, the L1 clip quirk, the soft target update, the shadow rewrite with column rotation, split-bf16 and pair stores), the dW
epilogue of csrc/dwadam.hip that shares its element arithmetic, and the flat passes of csrc/optim.hip.

The arenas (params, grads, adam_m, adam_v, slow) are caller-owned tensors, recnn_engine_set_counters sets t and the phase API applies
whatever gradient lies in the bound arena: chosen inputs go in and every output element is compared with tests/optim_reference.py,
whose values carry a derived first-order fp32 error bound.  The assertion everywhere is |gpu - ref| <= 2 bound (no measured
constant; tests/test_optim_cpu.py shows the bound is tight enough to reject the reference's mutants).  Shadows are compared bit for bit
with the stored fp32 parameter.  The largest err / bound seen per operation is printed when the module ends (pytest -s)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import optim_reference as R
from tests.helpers import x3_pack_ref

pytestmark = pytest.mark.gpu
H = 64
TAU = 0.05
NAMES = {0: "policy", 1: "target_policy", 2: "value1", 3: "target_value1", 4: "value2", 5: "target_value2"}
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
RANGER = dict(lr=1e-3, beta1=0.95, beta2=0.999, eps=1e-5, alpha=0.5, k=6)
_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("largest err / bound per operation:", json.dumps(_RATIOS, sort_keys=True))


def _np(t):
    return t.detach().cpu().numpy()


def _hold(name, got, ref, ctx=None):
    """|got - ref| <= 2 bound on every element; records the largest err / bound under `name`"""
    got = _np(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    assert np.all(np.isfinite(got)), (name, ctx)
    r = R.ratio(got.reshape(ref.v.shape), ref)
    _RATIOS[name] = max(_RATIOS.get(name, 0.0), r)
    assert r <= 2.0, (name, ctx, r)


def _same_bits(a, b, tag):
    a = a if isinstance(a, torch.Tensor) else torch.from_numpy(a)
    b = b if isinstance(b, torch.Tensor) else torch.from_numpy(b)
    assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32)), tag


# ------------------------------------------------------------------------------------------------ 3a: the engine pass on written arenas
def _engine(algo, S, dtype, value_opt=None, policy_opt=None):
    from recnn_amd.nn.engine import StepEngine
    A = 32 if dtype == "bf16x3" else 8
    eng = StepEngine(algo, S, A, H, 64, dtype=dtype, mask_mode="none")
    eng.set_hyper(soft_tau=TAU, policy_opt=policy_opt, value_opt=value_opt)
    return eng


def _fill(eng, seed, zero_grad=False):
    """every arena of every network from optim_reference.make_inputs (targets: their own parameters), shadows refreshed; returns the host copies"""
    host = {}
    for ni in eng.nets:
        x = R.make_inputs(eng.params[ni].numel(), 1000 * seed + ni)
        if zero_grad:
            x["g"][:] = 0
        eng.params[ni].copy_(torch.from_numpy(x["p"]))
        if ni in eng.grads:
            eng.grads[ni].copy_(torch.from_numpy(x["g"]))
            eng.adam_m[ni].copy_(torch.from_numpy(x["m"]))
            eng.adam_v[ni].copy_(torch.from_numpy(x["v"]))
        if ni in eng.slow:
            eng.slow[ni].copy_(torch.from_numpy(x["slow"]))
        host[ni] = x
        eng.refresh(ni)
    return host


def _check_shadows(eng, ni, ctx):
    """W1 / W2 / (actor) W3 shadow of net `ni` == the stored fp32 parameter: the value (fp32), round-to-nearest-even (bf16), hi / lo
    (split bf16); a critic's W1 at column (c + A) mod cols; padding columns zero.  Bit for bit."""
    views = eng.param_views(ni)
    critic = ni >= 2
    for w in ("w1", "w2") + (() if critic else ("w3",)):
        raw = eng.buffer(f"{NAMES[ni]}_{w}_shadow", raw=True).cpu()
        W = views[w].detach().cpu()
        if critic and w == "w1":
            W = torch.roll(W, eng.A, dims=1)
        rows, cols = W.shape
        assert raw.shape[0] == rows and raw.shape[1] >= cols
        if eng.dtype == "bf16x3":
            want = x3_pack_ref(W, raw.shape[1])
        else:
            want = torch.zeros(rows, raw.shape[1], dtype=raw.dtype)
            want[:, :cols] = W.to(raw.dtype)
        it = torch.int32 if raw.dtype == torch.float32 else torch.int16
        bad = (raw.view(it) != want.view(it)).nonzero()
        assert bad.numel() == 0, (ctx, NAMES[ni], w, bad[:4].tolist())


def _untouched(eng, host, nets, ctx, keys=("p", "g", "m", "v", "slow")):
    arenas = dict(p=eng.params, g=eng.grads, m=eng.adam_m, v=eng.adam_v, slow=eng.slow)
    for ni in nets:
        for k in keys:
            if ni in arenas[k]:
                _same_bits(arenas[k][ni], host[ni][k], (ctx, NAMES[ni], k, "must be bit-unchanged"))


SHAPES = [(dt, S) for dt in ("fp32", "bf16", "bf16x3") for S in (29, 30, 32)]


@pytest.mark.parametrize("algo", ["ddpg", "td3"])
@pytest.mark.parametrize("dtype,S", SHAPES)
def test_value_apply_adam(cuda, dtype, S, algo):
    eng = _engine(algo, S, dtype)
    seed = 0
    for wd in (0.0, 1e-2):
        eng.set_hyper(soft_tau=TAU, value_opt=dict(kind="adam", weight_decay=wd, **ADAM))
        for t in (1, 2, 1000, 100000):
            for soft in (True, False):
                for gs in (1.0, 0.5):
                    seed += 1
                    ctx = (dtype, S, algo, wd, t, soft, gs)
                    host = _fill(eng, seed)
                    eng.set_counters(policy_t=3, value1_t=t - 1, value2_t=t - 1)
                    eng.value_apply(soft, gs)
                    torch.cuda.synchronize()
                    for ni in eng.value_nets():
                        x = host[ni]
                        ref = R.adam(x["p"], x["g"], x["m"], x["v"], wd=wd, t=t, gs=gs, **ADAM)
                        _hold("engine/adam/p", eng.params[ni], ref["p"], ctx)
                        _hold("engine/adam/m", eng.adam_m[ni], ref["m"], ctx)
                        _hold("engine/adam/v", eng.adam_v[ni], ref["v"], ctx)
                        _untouched(eng, host, [ni], ctx, keys=("g",))
                        if soft:
                            _hold("engine/soft/target_p", eng.params[ni + 1], R.soft(host[ni + 1]["p"], ref["p"], TAU), ctx)
                        else:
                            _untouched(eng, host, [ni + 1], ctx)
                        _check_shadows(eng, ni, ctx)
                        _check_shadows(eng, ni + 1, ctx)
                    _untouched(eng, host, [0, 1], ctx)


@pytest.mark.parametrize("algo", ["ddpg", "td3"])
@pytest.mark.parametrize("dtype,S", SHAPES)
def test_value_apply_ranger(cuda, dtype, S, algo):
    wd = 1e-2
    eng = _engine(algo, S, dtype, value_opt=dict(kind="ranger", weight_decay=wd, **RANGER))
    seed = 100
    for t in (4, 5, 6, 7, 12):
        for soft, gs in ((True, 1.0), (False, 0.5)):
            seed += 1
            ctx = (dtype, S, algo, t, soft, gs)
            host = _fill(eng, seed)
            eng.set_counters(value1_t=t - 1, value2_t=t - 1)
            eng.value_apply(soft, gs)
            torch.cuda.synchronize()
            for ni in eng.value_nets():
                x = host[ni]
                ref = R.ranger(x["p"], x["g"], x["m"], x["v"], x["slow"], wd=wd, t=t, gs=gs, **RANGER)
                assert ref["sync"] == (t in (6, 12)) and ref["rect"] == (t >= 6)
                _hold("engine/ranger/p", eng.params[ni], ref["p"], ctx)
                _hold("engine/ranger/m", eng.adam_m[ni], ref["m"], ctx)
                _hold("engine/ranger/v", eng.adam_v[ni], ref["v"], ctx)
                if ref["sync"]:
                    _hold("engine/ranger/slow", eng.slow[ni], ref["slow"], ctx)
                    _same_bits(eng.slow[ni], eng.params[ni], (ctx, "p = slow after a sync"))
                else:
                    _untouched(eng, host, [ni], ctx, keys=("slow",))
                _untouched(eng, host, [ni], ctx, keys=("g",))
                if soft:
                    _hold("engine/soft/target_p", eng.params[ni + 1], R.soft(host[ni + 1]["p"], ref["p"], TAU), ctx)
                else:
                    _untouched(eng, host, [ni + 1], ctx)
                _check_shadows(eng, ni, ctx)
                _check_shadows(eng, ni + 1, ctx)
            _untouched(eng, host, [0, 1], ctx)


def _actor_blocks(eng):
    """workgroups of the actor's optimizer layout (optim.h opt_blocks): 64 elements per workgroup up to 1024 elements, else 1024"""
    sizes = [H * eng.S, H, H * H, H, eng.A * H, eng.A]
    return sum((n + 63) // 64 if n <= 1024 else (n + 1023) // 1024 for n in sizes)


@pytest.mark.parametrize("algo", ["ddpg", "td3"])
@pytest.mark.parametrize("dtype,S", SHAPES)
def test_policy_apply_clip_quirk(cuda, dtype, S, algo):
    wd = 1e-2
    eng = _engine(algo, S, dtype)
    depth = R.engine_l1_depth(_actor_blocks(eng))
    others = [ni for ni in eng.nets if ni >= 2]
    seed = 200
    for kind, t, gs, zero in (("adam", 1, 1.0, False), ("adam", 1000, 0.5, False), ("adam", 2, 1.0, True), ("ranger", 6, 1.0, False),
                              ("ranger", 5, 0.5, False)):
        seed += 1
        ctx = (dtype, S, algo, kind, t, gs, zero)
        hp = ADAM if kind == "adam" else RANGER
        eng.set_hyper(soft_tau=TAU, policy_opt=dict(kind=kind, weight_decay=wd, **hp))
        host = _fill(eng, seed, zero_grad=zero)
        x = host[0]
        eng.set_counters(policy_t=t - 1, value1_t=77, value2_t=78)
        eng.policy_apply(True, gs)
        torch.cuda.synchronize()
        coef = _np(eng.buffer("clip_coef")).reshape(())
        assert coef.dtype == np.float32
        _hold("engine/clip/coef", coef, R.quirk_clip_coef(R.l1_sum(x["g"], depth), gs), ctx)
        if zero:
            assert abs(float(coef) + 1e6) < 1.0, coef       # -1 / (0 + 1e-6f)
        gs_eff = R.host(gs) * R.exact(coef)                 # the kernel's own coefficient: gs *= coef
        if kind == "adam":
            ref = R.adam(x["p"], x["g"], x["m"], x["v"], wd=wd, t=t, gs=gs_eff, **ADAM)
        else:
            ref = R.ranger(x["p"], x["g"], x["m"], x["v"], x["slow"], wd=wd, t=t, gs=gs_eff, **RANGER)
            if ref["sync"]:
                _hold("engine/clip+ranger/slow", eng.slow[0], ref["slow"], ctx)
            else:
                _untouched(eng, host, [0], ctx, keys=("slow",))
        for k, arena in (("p", eng.params), ("m", eng.adam_m), ("v", eng.adam_v)):
            _hold(f"engine/clip+{kind}/{k}", arena[0], ref[k], ctx)
        _untouched(eng, host, [0], ctx, keys=("g",))
        if algo == "ddpg":
            _hold("engine/soft/target_p", eng.params[1], R.soft(host[1]["p"], ref["p"], TAU), ctx)
        else:                                               # TD3 never soft-updates the target policy
            _untouched(eng, host, [1], ctx)
        _check_shadows(eng, 0, ctx)
        _check_shadows(eng, 1, ctx)
        _untouched(eng, host, others, ctx)


@pytest.mark.parametrize("dtype,S", SHAPES)
def test_clip_policy_grads_and_soft_update_alone(cuda, dtype, S):
    from recnn_amd import _lib as L
    eng = _engine("ddpg", S, dtype)
    depth = R.engine_l1_depth(_actor_blocks(eng))
    for i, gs in enumerate((1.0, 0.5)):
        ctx = (dtype, S, gs)
        host = _fill(eng, 300 + i)
        L.call("recnn_engine_clip_policy_grads", eng.handle, gs, L.current_stream())
        torch.cuda.synchronize()
        coef = R.quirk_clip_coef(R.l1_sum(host[0]["g"], depth), gs)
        _hold("engine/clip_policy_grads/g", eng.grads[0], R.exact(host[0]["g"]) * (R.host(gs) * coef), ctx)
        _untouched(eng, host, eng.nets, ctx, keys=("p", "m", "v"))
        _untouched(eng, host, [2], ctx, keys=("g",))
    for i, (ni, tau) in enumerate(((0, 0.001), (2, TAU), (2, 0.5))):
        ctx = (dtype, S, ni, tau)
        host = _fill(eng, 310 + i)
        L.call("recnn_engine_soft_update", eng.handle, ni, ni + 1, tau, L.current_stream())
        torch.cuda.synchronize()
        _hold("engine/soft_update/target_p", eng.params[ni + 1], R.soft(host[ni + 1]["p"], host[ni]["p"], tau), ctx)
        _untouched(eng, host, [n for n in eng.nets if n != ni + 1], ctx)
        _check_shadows(eng, ni, ctx)
        _check_shadows(eng, ni + 1, ctx)


# ------------------------------------------------------------------------------------------------ 3b: the routes a real step takes
S_, A_, H_ = 1290, 128, 256


def _snapshot(eng):
    snap = {}
    for ni in eng.nets:
        snap[ni] = dict(p=_np(eng.params[ni]).copy())
        if ni in eng.grads:
            snap[ni].update(m=_np(eng.adam_m[ni]).copy(), v=_np(eng.adam_v[ni]).copy())
        if ni in eng.slow:
            snap[ni]["slow"] = _np(eng.slow[ni]).copy()
    return snap


def _ref_update(kind, x, g, t, gs, wd):
    if kind == "adam":
        return R.adam(x["p"], g, x["m"], x["v"], wd=wd, t=t, gs=gs, **ADAM)
    return R.ranger(x["p"], g, x["m"], x["v"], x["slow"], wd=wd, t=t, gs=gs, **RANGER)


@pytest.mark.parametrize("dtype,B,fuse,kind,critic_launch", [("bf16", 1024, 1, "adam", "dwadam_critic"), ("bf16", 1024, 0, "adam", "adam_critic"),
                                                             ("bf16x3", 1024, 1, "adam", "dwadam_critic"), ("fp32", 333, 1, "adam", "adam_critic"),
                                                             ("bf16", 1024, 1, "ranger", "dwadam_critic"), ("bf16", 1024, 0, "ranger", "adam_critic")])
def test_real_step_routes(cuda, dtype, B, fuse, kind, critic_launch):
    """A policy step (critic pass with the soft update fused in, actor pass behind the clip quirk, DDPG's target actor) and an ordinary
    step, conditioned on the gradient the step itself consumed: both the slab-summing pass and the dW epilogue leave it in eng.grads."""
    from recnn_amd import _lib as L
    from tests.test_gpu_engine import _engine as mk, _init_nets, _rand_batch
    wd = 1e-2
    actor, critics = _init_nets(8, S_, A_, H_, 1)
    eng = mk("ddpg", S_, A_, H_, B, dtype, mask_mode="hash", seed=17)
    if dtype != "fp32":
        eng.set_tuning(split_fwd=2, dw_fuse=fuse)
    for ni, p in ((0, actor), (1, actor), (2, critics[0]), (3, critics[0])):
        eng.load_params(ni, p)
    hp = ADAM if kind == "adam" else RANGER
    o = dict(kind=kind, weight_decay=wd, **hp)
    eng.set_hyper(policy_opt=dict(o), value_opt=dict(o), policy_every=2, soft_tau=TAU)
    for ni in (0, 2):          # running moments (and slow weights) of a run under way; a gradient-sized scale
        x = R.make_inputs(eng.params[ni].numel(), 400 + ni)
        eng.adam_m[ni].copy_(torch.from_numpy(x["m"] * np.float32(1e-2)))
        eng.adam_v[ni].copy_(torch.from_numpy(x["v"] * np.float32(1e-4)))
        if ni in eng.slow:
            eng.slow[ni].add_(torch.from_numpy(x["slow"] - x["p"]).to(eng.slow[ni].device))
    t0 = 5 if kind == "ranger" else 0      # Ranger: the policy step is the Lookahead sync at t = 6
    eng.set_counters(policy_t=t0, value1_t=t0, value2_t=t0, step=0)
    gen = torch.Generator().manual_seed(31)
    with R.underflow_allowed():        # the gradients are the step's own: nothing keeps g * g in the normal range
        for step in (0, 1):
            pol = step == 0
            ctx = (dtype, B, fuse, kind, "policy step" if pol else "ordinary step")
            snap = _snapshot(eng)
            batch = _rand_batch(B, S_, A_, gen)
            eng.pack_batch(batch["state"], batch["action"], batch["reward"], batch["next_state"], batch["done"])
            eng.step(B, True, step)
            torch.cuda.synchronize()
            tag = f"step/{critic_launch}/{dtype}/{kind}"
            t = t0 + 1 + step
            ref = _ref_update(kind, snap[2], _np(eng.grads[2]), t, 1.0, wd)
            _hold(tag + "/p", eng.params[2], ref["p"], ctx)
            _hold(tag + "/m", eng.adam_m[2], ref["m"], ctx)
            _hold(tag + "/v", eng.adam_v[2], ref["v"], ctx)
            if kind == "ranger":
                assert ref["sync"] == pol
                if pol:
                    _hold(tag + "/slow", eng.slow[2], ref["slow"], ctx)
                else:
                    _same_bits(eng.slow[2], snap[2]["slow"], (ctx, "critic slow"))
            if pol:
                _hold(tag + "/target_p", eng.params[3], R.soft(snap[3]["p"], ref["p"], TAU), ctx)
                coef = _np(eng.buffer("clip_coef")).reshape(())
                aref = _ref_update(kind, snap[0], _np(eng.grads[0]), t0 + 1, R.host(1.0) * R.exact(coef), wd)
                atag = f"step/adam_actor/{dtype}/{kind}"
                _hold(atag + "/p", eng.params[0], aref["p"], ctx)
                _hold(atag + "/m", eng.adam_m[0], aref["m"], ctx)
                _hold(atag + "/v", eng.adam_v[0], aref["v"], ctx)
                if kind == "ranger":
                    _hold(atag + "/slow", eng.slow[0], aref["slow"], ctx)
                _hold(atag + "/target_p", eng.params[1], R.soft(snap[1]["p"], aref["p"], TAU), ctx)
            else:
                for ni in (0, 1, 3):
                    _same_bits(eng.params[ni], snap[ni]["p"], (ctx, NAMES[ni], "untouched on an ordinary step"))
            for ni in eng.nets:
                _check_shadows(eng, ni, ctx)
    prof = [n for n, _, _ in eng.profile(B, policy=False, n_steps=1)]
    assert critic_launch in prof, prof


# ------------------------------------------------------------------------------------------------ 3c: the flat passes
SIZES = [1, 3, 4, 5, 1027, 600_001]       # 600,001 > 2048 workgroups x 256: the 4-byte form wraps its grid


def _dev(x, off, cuda):
    """a device copy of x that starts `off` floats into a 16-byte aligned allocation"""
    base = torch.zeros(x.size + 4, device=cuda)
    assert base.data_ptr() % 16 == 0
    view = base[off:off + x.size]
    view.copy_(torch.from_numpy(x))
    return view


def _flat_inputs(n, off, cuda, seed):
    x = R.make_inputs(n, seed)
    return x, {k: _dev(v, off, cuda) for k, v in x.items()}


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_flat_adam(cuda, n, off):
    from recnn_amd import _lib as L
    wd, gs = 1e-2, 0.5
    for t in (1, 1000):
        x, d = _flat_inputs(n, off, cuda, 500 + t)
        L.call("recnn_adam_flat", L.ptr(d["p"]), L.ptr(d["g"]), L.ptr(d["m"]), L.ptr(d["v"]), n, ADAM["lr"], ADAM["beta1"], ADAM["beta2"],
               ADAM["eps"], wd, t, gs, L.current_stream())
        torch.cuda.synchronize()
        ref = R.adam(x["p"], x["g"], x["m"], x["v"], wd=wd, t=t, gs=gs, **ADAM)
        for k in ("p", "m", "v"):
            _hold("flat/adam/" + k, d[k], ref[k], (n, off, t))
        _same_bits(d["g"], x["g"], "g")
    # the count on the device plus step_add
    x, d = _flat_inputs(n, off, cuda, 520)
    cnt = torch.tensor([993], dtype=torch.int32, device=cuda)
    L.call("recnn_adam_flat_at", L.ptr(d["p"]), L.ptr(d["g"]), L.ptr(d["m"]), L.ptr(d["v"]), n, ADAM["lr"], ADAM["beta1"], ADAM["beta2"],
           ADAM["eps"], 0.0, L.ptr(cnt), 7, 1.0, L.current_stream())
    torch.cuda.synchronize()
    ref = R.adam(x["p"], x["g"], x["m"], x["v"], wd=0.0, t=1000, gs=1.0, **ADAM)
    for k in ("p", "m", "v"):
        _hold("flat/adam_at/" + k, d[k], ref[k], (n, off))
    assert int(cnt.item()) == 993


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_flat_ranger_radam_soft_clip(cuda, n, off):
    from recnn_amd import _lib as L
    wd = 1e-2
    for t in (5, 6):
        x, d = _flat_inputs(n, off, cuda, 600 + t)
        L.call("recnn_ranger_flat", L.ptr(d["p"]), L.ptr(d["g"]), L.ptr(d["m"]), L.ptr(d["v"]), L.ptr(d["slow"]), n, RANGER["lr"],
               RANGER["beta1"], RANGER["beta2"], RANGER["eps"], wd, RANGER["alpha"], RANGER["k"], 5.0, t, 0.5, L.current_stream())
        torch.cuda.synchronize()
        ref = R.ranger(x["p"], x["g"], x["m"], x["v"], x["slow"], wd=wd, t=t, gs=0.5, **RANGER)
        assert ref["sync"] == (t == 6) and ref["rect"] == (t == 6)
        for k in ("p", "m", "v", "slow"):
            _hold("flat/ranger/" + k, d[k], ref[k], (n, off, t))
        if not ref["sync"]:
            _same_bits(d["slow"], x["slow"], "slow without a sync")
        for norm in (None, 25.0):
            x, d = _flat_inputs(n, off, cuda, 610 + t)
            nd = None if norm is None else torch.tensor([norm], device=cuda)
            L.call("recnn_radam_flat", L.ptr(d["p"]), L.ptr(d["g"]), L.ptr(d["m"]), L.ptr(d["v"]), n, ADAM["lr"], ADAM["beta1"],
                   ADAM["beta2"], ADAM["eps"], wd, t, L.ptr(nd), 1.0, L.current_stream())
            torch.cuda.synchronize()
            ref = R.radam(x["p"], x["g"], x["m"], x["v"], wd=wd, t=t, norm=None if norm is None else np.float32(norm), max_norm=1.0, **ADAM)
            assert ref["rect"] == (t == 6)
            for k in ("p", "m", "v"):
                _hold("flat/radam/" + k, d[k], ref[k], (n, off, t, norm))
            if norm is None:
                _same_bits(d["g"], x["g"], "g without a clip norm")
            else:
                _hold("flat/radam/g", d["g"], ref["g"], (n, off, t, norm))
    x, d = _flat_inputs(n, off, cuda, 630)
    L.call("recnn_soft_update_flat", L.ptr(d["tgt"]), L.ptr(d["p"]), n, TAU, L.current_stream())
    scratch, out = torch.zeros(1024, device=cuda), torch.zeros(1, device=cuda)
    L.call("recnn_l1_norm_flat", L.ptr(d["g"]), n, L.ptr(scratch), L.ptr(out), L.current_stream())
    torch.cuda.synchronize()
    _hold("flat/soft_update", d["tgt"], R.soft(x["tgt"], x["p"], TAU), (n, off))
    _same_bits(d["p"], x["p"], "p")
    _hold("flat/l1_norm", out, R.l1_sum(x["g"], R.flat_l1_depth(n)), (n, off))
    norm = _np(out).reshape(())
    L.call("recnn_dqn_clip", L.ptr(d["g"]), n, L.ptr(out), 0.5, L.current_stream())
    torch.cuda.synchronize()
    _hold("flat/dqn_clip", d["g"], R.exact(x["g"]) * R.norm_clip_coef(norm, 0.5), (n, off))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("cols", [5, 6, 8])
def test_flat_shadow_copies(cuda, cols, bf16, off):
    """recnn_adam_flat_shadow / recnn_ranger_flat_shadow: element by element (5 columns), as pairs (6) and as one store per quad (8) --
    the copy is the new parameter bit for bit (bf16: rounded to nearest even), its padding untouched; p, m, v held to float64."""
    from recnn_amd import _lib as L
    rows, ld, wd = 129, cols + 4, 1e-2
    n = rows * cols
    dt = torch.bfloat16 if bf16 else torch.float32
    for kind, t in (("adam", 1), ("adam", 1000), ("ranger", 5), ("ranger", 6)):
        x, d = _flat_inputs(n, off, cuda, 700 + t)
        copy = torch.full((rows + 1, ld), 7.0, dtype=dt, device=cuda)
        sh = L.ShadowOut(copy.data_ptr(), cols, ld, int(bf16))
        if kind == "adam":
            L.call("recnn_adam_flat_shadow", L.ptr(d["p"]), L.ptr(d["g"]), L.ptr(d["m"]), L.ptr(d["v"]), n, ADAM["lr"], ADAM["beta1"],
                   ADAM["beta2"], ADAM["eps"], wd, t, 1.0, C.byref(sh), L.current_stream())
            ref = R.adam(x["p"], x["g"], x["m"], x["v"], wd=wd, t=t, gs=1.0, **ADAM)
        else:
            L.call("recnn_ranger_flat_shadow", L.ptr(d["p"]), L.ptr(d["g"]), L.ptr(d["m"]), L.ptr(d["v"]), L.ptr(d["slow"]), n, RANGER["lr"],
                   RANGER["beta1"], RANGER["beta2"], RANGER["eps"], wd, RANGER["alpha"], RANGER["k"], 5.0, t, 1.0, C.byref(sh),
                   L.current_stream())
            ref = R.ranger(x["p"], x["g"], x["m"], x["v"], x["slow"], wd=wd, t=t, gs=1.0, **RANGER)
        torch.cuda.synchronize()
        for k in ("p", "m", "v"):
            _hold(f"flat/{kind}_shadow/{k}", d[k], ref[k], (cols, bf16, off, t))
        assert torch.equal(copy[:rows, :cols], d["p"].view(rows, cols).to(dt)), (kind, cols, bf16, off, t)
        assert bool((copy[:rows, cols:] == 7).all()) and bool((copy[rows:] == 7).all()), (kind, cols, bf16, off, t)
