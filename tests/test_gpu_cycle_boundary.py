"""The seam between policy cycles in the bf16 cycle schedule (csrc/engine_graph.hip): two tuning knobs that change which bytes are stored and
where run graphs are cut, and nothing that is computed:

  frozen_acts_policy_only  the cycle-batched actor launch (csrc/mlpf.hip) stores h1 / h2 only for the policy step's batch
  run_align                long requests are composed of run graphs that end on a policy step (recnn_run_plan)

Everything that is computed is equal BIT FOR BIT under every setting, and equal to the eager step loop.

Shapes as tests/test_gpu_frozen_window.py: 128 rows per batch (64- and 128-row workgroup forms), users of 11-14 items, so user ends fall
inside panels and across batches; policy period 3.  run(7) from step 5 as ONE made-to-order graph = segments of 2 + 3 + 2 steps in
alternating copies of the cycle arrays: with cycle_min_seg 2 a batched segment that ends on its policy step with the policy batch as
the second of two (its first batch's activations are not stored), one whose policy batch is the third of three, and one without a policy
step (no activations stored); with cycle_min_seg 3 the 2-step segments step through the fused forward around the batched one."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS, UPB, PE = 128, 128, 3
SEED = 977
FIRST, N = 5, 7
KNOBS = ("frozen_acts_policy_only", "run_align")
ALL_OFF = {k: 0 for k in KNOBS}
# all on, and each one off alone
SETTINGS = [{k: 1 for k in KNOBS}] + [{k: int(k != off) for k in KNOBS} for off in KNOBS]
LONG = 200                    # 3 x 63-step aligned graphs + 3 aligned cycles (from step 2 behind a step and the policy step)


def _env(recnn_amd, cuda, n_users, seed=11, n_items=500):
    rng = np.random.default_rng(seed)
    lens = rng.integers(11, 15, size=n_users).astype(np.int64)          # 1..4 windows per user
    off = np.zeros(n_users + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    items = rng.integers(0, n_items, size=total, dtype=np.int32)
    ratings = (2.0 * (rng.integers(1, 11, size=total) * 0.5 - 2.5)).astype(np.float32)
    table = torch.randn(n_items, 128, generator=torch.Generator().manual_seed(seed))
    return recnn_amd.data.env.FrameEnv.from_store(table, items, ratings, off, frame_size=10, batch_size=25, device=cuda,
                                                  test_fraction=0.0, rows_per_batch=ROWS)


def _make(recnn_amd, cuda, env, algo):
    from recnn_amd.nn import fused
    fused.set_defaults(dtype="bf16", mask_mode="hash", seed=SEED)
    torch.manual_seed(31)
    nn = recnn_amd.nn
    if algo == "ddpg":
        a = nn.DDPG(nn.Actor(1290, 128, 256, 6e-1), nn.Critic(1290, 128, 256, 54e-2)).to(cuda)
        a.params["policy_step"] = PE
    else:
        a = nn.TD3(nn.Actor(1290, 128, 256, 6e-1), nn.Critic(1290, 128, 256, 54e-2), nn.Critic(1290, 128, 256, 54e-2)).to(cuda)
        a.params["policy_update"] = PE
    torch.manual_seed(57)                                  # the epoch permutation comes from the CPU generator
    a.attach_env(env, rows_per_batch=ROWS, users_per_batch=UPB)
    return a


def _state(a):
    """Master parameters of every network and the optimizers' moments (the engine's flat arenas), cloned."""
    eng = a._fused_ctx.engine
    out = {n: {k: v.detach().clone() for k, v in m.state_dict().items()} for n, m in a.nets.items()}
    out["adam"] = {ni: (eng.adam_m[ni].detach().clone(), eng.adam_v[ni].detach().clone()) for ni in sorted(eng.adam_m)}
    return out


def _assert_state_equal(x, y, what):
    assert x.keys() == y.keys()
    for net, sd in x.items():
        if net == "adam":
            assert sd.keys() == y[net].keys() and len(sd) >= 2
            for ni, (m, v) in sd.items():
                assert torch.equal(m, y[net][ni][0]) and torch.equal(v, y[net][ni][1]), (what, "adam", ni)
        else:
            for k, v in sd.items():
                assert torch.equal(v, y[net][k]), (what, net, k)


def _cycle_array(eng, name):
    r, c, ld, f = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
    p = eng.lib.recnn_engine_buffer(eng.handle, name.encode(), C.byref(r), C.byref(c), C.byref(ld), C.byref(f))
    assert p, name
    esz = 4 if f.value else 2

    class Span:
        __cuda_array_interface__ = {"shape": (r.value * ld.value * esz,), "typestr": "|u1", "data": (int(p), False), "version": 2}
    raw = torch.as_tensor(Span(), device=eng.device)
    return raw.view(torch.float32 if f.value else torch.bfloat16).view(r.value, ld.value)[:, :c.value].clone()


def _tuned(fields):
    from recnn_amd._tune import set_default_tuning
    set_default_tuning(**fields)
    return lambda: set_default_tuning(**{k: None for k in fields})


def _run_short(recnn_amd, cuda, env, algo, knobs, min_seg):
    undo = _tuned({**knobs, "cycle_min_len": 2, "cycle_min_seg": min_seg})
    try:
        a = _make(recnn_amd, cuda, env, algo)
        eng = a._fused_ctx.engine
        assert all(getattr(eng.tuning, k) == v for k, v in knobs.items()) and eng.tuning.cycle_min_seg == min_seg
        _, hist = a.run(FIRST, history=True)
        a.prepare_run(N, first_step=FIRST)                 # ONE made-to-order run graph: segments of 2 + 3 + 2 steps
        _, h = a.run(N, history=True)
        torch.cuda.synchronize()
        # the batched 3-step segment ends on policy step 9: its batch is rows 2 ROWS .. 3 ROWS of the cycle arrays, and nothing wrote
        # those rows afterwards (the last segment has two batches)
        acts = [_cycle_array(eng, f"cycle_actor_h{l}")[2 * ROWS:3 * ROWS] for l in (1, 2)]
        return {"hist": hist + h, "state": _state(a), "acts": acts}
    finally:
        undo()


def _loop(recnn_amd, cuda, env, algo, n, snaps=()):
    a = _make(recnn_amd, cuda, env, algo)
    perm = a._fused_ctx.perm.cpu().numpy()
    hist, states = [], {}
    for i in range(n):
        batch = env.collate_users([int(u) for u in perm[i * UPB:(i + 1) * UPB]])
        assert batch["state"].shape[0] == ROWS
        hist.append(dict(a.update(batch, learn=True)))
        a.step()
        if i + 1 in snaps:
            torch.cuda.synchronize()
            states[i + 1] = _state(a)
    return hist, states


def _assert_hist_close(hist, lhist, algo):
    """losses of the graph replay against the eager loop's: to summation order (as tests/test_gpu_bench_shape.py)"""
    keys = ("value1", "value2", "policy") if algo == "td3" else ("value", "policy")
    assert len(hist) == len(lhist)
    for x, y in zip(hist, lhist):
        assert x["step"] == y["step"]
        for k in keys:
            assert np.isfinite(x[k]) and abs(x[k] - y[k]) <= 1e-5 * max(abs(y[k]), 1.0), (k, x, y)


_SHARED = {}


def _shared(recnn_amd, cuda, algo):
    """The env and the eager-loop reference of one algorithm, computed once: the parameters after FIRST + N steps (the short request) and
    after 2 + LONG and 3 + LONG steps (the long ones)."""
    if algo not in _SHARED:
        env = _env(recnn_amd, cuda, n_users=(3 + LONG + 5) * UPB)
        n = FIRST + N if algo == "td3" else 3 + LONG
        _SHARED[algo] = (env,) + _loop(recnn_amd, cuda, env, algo, n, snaps=(FIRST + N, 2 + LONG, 3 + LONG))
    return _SHARED[algo]


@pytest.mark.parametrize("min_seg", [2, 3])
@pytest.mark.parametrize("algo", ["ddpg", "td3"])
def test_every_knob_setting_equals_all_off_and_the_eager_loop(cuda, algo, min_seg):
    import recnn_amd
    env, lhist, lstates = _shared(recnn_amd, cuda, algo)
    off = _run_short(recnn_amd, cuda, env, algo, ALL_OFF, min_seg)
    # ---- all off == the eager step loop: parameters and moments bit for bit, losses to summation order
    _assert_state_equal(lstates[FIRST + N], off["state"], "eager loop")
    _assert_hist_close(off["hist"], lhist[:FIRST + N], algo)
    for h in off["acts"]:
        assert float(h.float().abs().max()) > 0
    # ---- every setting == all off, bit for bit
    for knobs in SETTINGS:
        on = _run_short(recnn_amd, cuda, env, algo, knobs, min_seg)
        assert on["hist"] == off["hist"], knobs
        _assert_state_equal(off["state"], on["state"], knobs)
        # the policy step's batch of the actor's activations: what its backward read (stored under either setting of the store knob)
        for x, y in zip(on["acts"], off["acts"]):
            assert torch.equal(x, y), knobs


def _run_long(recnn_amd, cuda, env, first, align):
    undo = _tuned({"run_align": align, "cycle_min_len": 2, "cycle_min_seg": 2})
    try:
        a = _make(recnn_amd, cuda, env, "ddpg")
        eng = a._fused_ctx.engine
        assert eng.tuning.run_align == align and eng.tuning.frozen_acts_policy_only == 1
        _, hist = a.run(first, history=True)
        _, h = a.run(LONG, history=True)                   # no made-to-order graph: composed from the family (recnn_run_plan)
        torch.cuda.synchronize()
        return {"hist": hist + h, "state": _state(a)}
    finally:
        undo()


@pytest.mark.parametrize("first", [2, 3])                  # behind a policy step's successor / ON a policy step
def test_long_request_on_aligned_run_graphs(cuda, first):
    import recnn_amd
    from recnn_amd import _lib as L
    env, lhist, lstates = _shared(recnn_amd, cuda, "ddpg")
    # what the aligned composition of this request is: the 63-step aligned graph three times, then three aligned cycles
    fam = L.RunFamily()
    assert L.load().recnn_run_family_init(PE, -1, 1, C.byref(fam)) == 0
    kinds, lens = (C.c_int * 64)(), (C.c_int * 64)()
    n = L.load().recnn_run_plan(PE, C.byref(fam), first, LONG, 1, kinds, lens, 64)
    pieces = [(kinds[i], lens[i]) for i in range(n)]
    assert pieces.count((L.RUN_ALIGNED_MULTI, 63)) == 3 and (L.RUN_ALIGNED_CYCLE, 3) in pieces and (L.RUN_MULTI, 63) not in pieces
    on, off = _run_long(recnn_amd, cuda, env, first, 1), _run_long(recnn_amd, cuda, env, first, 0)
    # What is COMPUTED is equal bit for bit: every parameter and optimizer moment after first + LONG steps.  The REPORTED policy loss of
    # an ordinary step is summed by whichever launch carries its forward -- the next step's launches inside a run graph, the step's own
    # at a graph's last step -- in that launch's order, so where the two compositions cut differently a reported loss may differ in its
    # last bits (as between any two cuts of a request, and against the eager loop): 128 fp32 terms, |error| <= 128 * 2^-24 < 1e-5 relative.
    _assert_hist_close(on["hist"], off["hist"], "ddpg")
    _assert_state_equal(off["state"], on["state"], "run_align 1 / 0")
    _assert_state_equal(lstates[first + LONG], on["state"], "eager loop")
    _assert_hist_close(on["hist"], lhist[:first + LONG], "ddpg")
