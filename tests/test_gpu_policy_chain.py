"""The policy step's own launches behind tuning.policy_fused (include/recnn_hip.h; RECNN_POLICY_FUSED), a bit set that changes which
kernels run and nothing that is computed:

  bit 0  layer 1 of the policy-loss critic on the per-step tiled kernel (csrc/l1gemm.hip) instead of the generic GEMM launch
  bit 1  the actor's three weight gradients by ONE launch that sums the batch slices on chip and writes the flat gradient arena
         (csrc/dwadam.hip dw_grad_kernel), the clip quirk's |g| partial sums by l1_blocks_kernel from that arena -- instead of
         gemm_dw_dma_kernel's slabs + grad_reduce_kernel.  The tile plan fits batches of 1024, 2048, ... rows; below, both launches stay.

0 issues the generic launches exactly.  Everything that is computed is equal BIT FOR BIT under every value of the knob: the parameters and
optimizer moments of every network, the actor's flat gradient and the |g| partial sums of the clip quirk (recnn/nn/update/ddpg.py:86-100).

The REPORTED policy loss of a policy step is -(sum of rows per-row Q) / rows in fp32.  A schedule may sum those rows terms in another order:
two orders of n fp32 additions differ by at most 2 (n - 1) 2^-24 sum |Q_r| in the sum, so |d loss| <= 2 rows 2^-24 (sum |Q_r|) / rows.  No
launch behind the knob today sums the loss (the layer-2 launch does under every value), and sum |Q_r| >= |sum Q_r| = rows |loss|: the tests
hold the reported loss to 2 rows 2^-24 |loss|, which is never wider than the bound above."""
import numpy as np
import pytest
import torch

from tests.test_gpu_engine import _engine, _init_nets, _rand_batch

pytestmark = pytest.mark.gpu
S, A, H = 1290, 128, 256
PE = 10


def _loss_bound(rows, loss):
    return 2.0 * rows * 2.0 ** -24 * abs(loss)


def _state(eng, nets):
    return dict(p={ni: eng.params[ni].clone() for ni, _ in nets}, m={ni: eng.adam_m[ni].clone() for ni in sorted(eng.adam_m)},
                v={ni: eng.adam_v[ni].clone() for ni in sorted(eng.adam_v)})


def _assert_state_equal(a, b, what):
    for key in ("p", "m", "v"):
        assert a[key].keys() == b[key].keys() and len(a[key]) >= 2
        for ni in a[key]:
            assert torch.equal(a[key][ni], b[key][ni]), (what, key, ni, int((a[key][ni] != b[key][ni]).sum()))


def _eager(L, B, knob, steps, policy_every, grads_at=()):
    """`steps` eager steps of a DDPG engine on the split forward (so that the step's learning critics run on the tiled layer-1 kernel, as
    they do inside the cycle schedule's run graphs); the state after the last step, every step's losses, and after the steps in
    `grads_at` the actor's flat gradient and the clip quirk's partial sums."""
    actor, critics = _init_nets(8, S, A, H, 1)
    eng = _engine("ddpg", S, A, H, B, "bf16", mask_mode="hash", seed=17)
    eng.set_tuning(split_fwd=2, policy_fused=knob)
    assert eng.tuning.policy_fused == knob
    nets = [(L.NET_POLICY, actor), (L.NET_TARGET_POLICY, actor), (L.NET_VALUE1, critics[0]), (L.NET_TARGET_VALUE1, critics[0])]
    for ni, p in nets:
        eng.load_params(ni, p)
    o = dict(kind="adam", lr=1e-3, weight_decay=1e-2)
    eng.set_hyper(policy_opt=dict(o), value_opt=dict(o), policy_every=policy_every, soft_tau=0.05)
    eng.set_counters()
    gen = torch.Generator().manual_seed(31)
    losses, grads = [], {}
    for t in range(steps):
        batch = _rand_batch(B, S, A, gen)
        eng.pack_batch(batch["state"], batch["action"], batch["reward"], batch["next_state"], batch["done"])
        eng.step(B, True, t)
        losses.append(eng.losses())
        if t in grads_at:
            torch.cuda.synchronize()
            grads[t] = (eng.grads[L.NET_POLICY].clone(), eng.buffer("actor_l1part").clone())
    torch.cuda.synchronize()
    return dict(state=_state(eng, nets), losses=losses, grads=grads), eng


@pytest.mark.parametrize("B", [64, 96])
def test_eager_steps_knob_on_equal_knob_off(cuda, B):
    """21 eager steps, policy period 10: the policy steps 0, 10 and 20.  Every parameter and Adam moment of all networks byte-equal; the
    reported losses within the summation-order bound (equal, in fact)."""
    from recnn_amd import _lib as L
    off, _ = _eager(L, B, 0, 21, PE)
    on, eng = _eager(L, B, 3, 21, PE)
    prof = [n for n, _, _ in eng.profile(B, policy=True, n_steps=1)]
    assert "l1_pcritic" in prof and "fwd_l1_pcritic" not in prof and "bwd_chain_policy" in prof, prof
    assert "dwgrad_actor" not in prof and "dw_actor" in prof and "grad_reduce_actor" in prof, prof      # below the tile plan
    _assert_state_equal(off["state"], on["state"], B)
    for t, (x, y) in enumerate(zip(off["losses"], on["losses"])):
        assert x["value"] == y["value"], (t, x, y)
        assert np.isfinite(y["policy"]) and abs(x["policy"] - y["policy"]) <= _loss_bound(B, x["policy"]), (t, x, y)


@pytest.mark.parametrize("B", [64, 96, 1024, 2048])
def test_actor_gradient_without_slabs_equals_dw_launch_plus_slab_reduction(cuda, B):
    """Policy steps 0 and 2 of three steps: the actor's flat gradient and the clip quirk's |g| partial sums as the policy step left them,
    bit 1 on against off, byte for byte; filled with a sentinel by neither path -- every element of both arrays is written by every policy
    step, so a stale or unwritten element shows as a difference at step 2 (the parameters moved in between).  1024 rows: eight batch
    slices for each matrix (one per consumer wave); 2048 rows: sixteen for W2 and W3 (two per wave); 64 and 96 rows: below the tile plan,
    the engine keeps the two launches on its own."""
    from recnn_amd import _lib as L
    off, _ = _eager(L, B, 0, 3, 2, grads_at=(0, 2))
    on, eng = _eager(L, B, 2, 3, 2, grads_at=(0, 2))
    prof = [n for n, _, _ in eng.profile(B, policy=True, n_steps=1)]
    if B >= 1024:
        assert "dwgrad_actor" in prof and "l1_norm_actor" in prof and "dw_actor" not in prof and "grad_reduce_actor" not in prof, prof
    else:
        assert "dwgrad_actor" not in prof and "dw_actor" in prof and "grad_reduce_actor" in prof, prof
    assert "fwd_l1_pcritic" in prof and "l1_pcritic" not in prof, prof      # bit 0 is off
    for t in (0, 2):
        (g0, l0), (g1, l1) = off["grads"][t], on["grads"][t]
        assert float(g0.abs().max()) > 0 and float(l0.abs().min()) >= 0 and float(l0.sum()) > 0
        assert torch.equal(g0, g1), (t, int((g0 != g1).sum()), float((g0 - g1).abs().max()))
        assert torch.equal(l0, l1), (t, int((l0 != l1).sum()))
    _assert_state_equal(off["state"], on["state"], B)
    assert off["losses"] == on["losses"]


# ---- inside run graphs (the cycle schedule the benchmark replays): an algorithm object on a FrameEnv, as tests/test_gpu_cycle_boundary.py
def _env(recnn_amd, cuda, rows, n_batches, seed=11, n_items=500):
    rng = np.random.default_rng(seed)
    lens = rng.integers(11, 15, size=n_batches * rows).astype(np.int64)
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    items = rng.integers(0, n_items, size=total, dtype=np.int32)
    ratings = (2.0 * (rng.integers(1, 11, size=total) * 0.5 - 2.5)).astype(np.float32)
    table = torch.randn(n_items, 128, generator=torch.Generator().manual_seed(seed))
    return recnn_amd.data.env.FrameEnv.from_store(table, items, ratings, off, frame_size=10, batch_size=25, device=cuda,
                                                  test_fraction=0.0, rows_per_batch=rows)


def _graph_run(recnn_amd, cuda, env, rows, knob, n):
    from recnn_amd._tune import set_default_tuning
    from recnn_amd.nn import fused
    set_default_tuning(policy_fused=knob, cycle_min_len=2, cycle_min_seg=2)
    try:
        fused.set_defaults(dtype="bf16", mask_mode="hash", seed=977)
        torch.manual_seed(31)
        nn = recnn_amd.nn
        a = nn.DDPG(nn.Actor(S, A, H, 6e-1), nn.Critic(S, A, H, 54e-2)).to(cuda)
        a.params["policy_step"] = PE
        torch.manual_seed(57)
        a.attach_env(env, rows_per_batch=rows, users_per_batch=rows)
        eng = a._fused_ctx.engine
        assert eng.tuning.policy_fused == knob
        a.prepare_run(n, first_step=0)                     # ONE made-to-order run graph
        _, hist = a.run(n, history=True)
        torch.cuda.synchronize()
        state = {k: {kk: v.detach().clone() for kk, v in m.state_dict().items()} for k, m in a.nets.items()}
        adam = {ni: (eng.adam_m[ni].detach().clone(), eng.adam_v[ni].detach().clone()) for ni in sorted(eng.adam_m)}
        return hist, state, adam
    finally:
        set_default_tuning(policy_fused=None, cycle_min_len=None, cycle_min_seg=None)


@pytest.mark.parametrize("rows", [64, 96])
def test_one_run_graph_knob_on_equals_knob_off(cuda, rows):
    """21 steps as one run graph in cycle mode, policy period 10: every parameter and Adam moment of all networks byte-equal, the
    reported losses within the summation-order bound."""
    import recnn_amd
    env = _env(recnn_amd, cuda, rows, 21 + 5)
    h0, s0, m0 = _graph_run(recnn_amd, cuda, env, rows, 0, 21)
    h1, s1, m1 = _graph_run(recnn_amd, cuda, env, rows, 3, 21)
    assert s0.keys() == s1.keys() and m0.keys() == m1.keys() and len(m0) >= 2
    for net, sd in s0.items():
        for k, v in sd.items():
            assert torch.equal(v, s1[net][k]), (net, k)
    for ni, (m, v) in m0.items():
        assert torch.equal(m, m1[ni][0]) and torch.equal(v, m1[ni][1]), ni
    assert len(h0) == len(h1) == 21
    for x, y in zip(h0, h1):
        assert x["step"] == y["step"] and x["value"] == y["value"], (x, y)
        assert np.isfinite(y["policy"]) and abs(x["policy"] - y["policy"]) <= _loss_bound(rows, x["policy"]), (x, y)
