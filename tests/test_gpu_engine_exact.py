"""One step of the bf16 StepEngine at lattice parameters against the float64 step, with plain equality.

The per-step kernels of the bf16 engine -- the fused whole-network forward (mlp_fwd_nets, csrc/mlps.hip), the split forward (the tiled
layer-1 GEMM l1gemm.hip + the row-panel tail mlpt.hip: l1_actors / tail_actors, l1_target_critic / tail_target_critic, l1_critic /
tail_critic), the TD head, the critic's backward chain, the policy step's chain and the weight-gradient launches (dw_critic, the fused
dwadam_critic, dwgrad_actor) -- are elsewhere compared with each other bit for bit and with the fp32 oracle at bf16 bounds.  Here the
networks, the batch, the external dropout masks and the TD3 noise come from the lattice of tests/mlp_exact_reference.py (engine_case):
every stage the engine holds in bf16 is representable and every fp32 sum is exact (tests/test_mlp_exact_cpu.py asserts it for each
case of CASES below), so every compared tensor must EQUAL the float64 chain of oracle/recnn_oracle.py's ddpg_step / td3_step.

set_hyper: gamma 0.5, no clamp of the TD target, and learning rates of zero -- the optimizer launches run, their gradients are
compared, and the critic the policy half of the step sees is still the lattice one, so pc_h1, pc_h2, q_pi, dact and the actor's gradient
meet the float64 chain itself.  (Parameters after Adam are not exact by nature; tests/test_gpu_dwadam.py and test_gpu_engine.py cover them.)

Forward, every case: next_action, target_q, expected, q1 (TD3: q2), gen_action, critic1_h1 / h2, actor_h1 / h2, pc_h1 / h2.
Where 2 / B is a power of two (64 and 1024 rows) also: the value loss mean((q1 - expected)^2) and the policy loss -mean(q_pi) as the
engine reports them (a learning step sums q_pi into the loss and stores no per-row q_pi); critic1_dz2 / dz1 and all six tensors of the
value network's gradient arena; dact, dzp2 / dzp1 and all six tensors of the actor's gradient arena.
Each case asserts from eng.profile which launches computed what it compared."""
import pytest
import torch

from tests import mlp_exact_reference as R

pytestmark = pytest.mark.gpu

SPLIT = {"l1_actors", "tail_actors", "l1_target_critic", "tail_target_critic", "l1_critic", "tail_critic"}
FORWARD = ("next_action", "target_q", "expected", "q1", "q2", "gen_action", "critic1_h1", "critic1_h2", "actor_h1", "actor_h2", "pc_h1", "pc_h2")
BACKWARD = ("critic1_dz2", "critic1_dz1", "dact", "dzp2", "dzp1")
CASES = R.ENGINE_CASES       # (algo, rows, split_fwd, dw_fuse, policy_fused)


def _differs(got, want, what):
    got, want = got.detach().cpu().double().reshape(want.shape), want.double()
    if torch.equal(got, want):
        return None
    bad = (got != want).nonzero()
    i = tuple(int(x) for x in bad[0])
    return f"{what}: {len(bad)} of {want.numel()} elements differ, first at {i}: got {float(got[i])!r}, want {float(want[i])!r}"


@pytest.mark.parametrize("algo,B,split,dw_fuse,policy_fused", CASES, ids=lambda v: str(v))
def test_step_equals_float64(cuda, algo, B, split, dw_fuse, policy_fused):
    from recnn_amd import _lib as L
    from recnn_amd.nn.engine import StepEngine
    td3 = algo == "td3"
    batch, masks, noise, ref = R.engine_case(B, algo)
    backward = B & (B - 1) == 0
    assert R.engine_inadmissible(ref, B, backward) == {}
    nets = R.engine_nets()
    eng = StepEngine(algo, R.ES, R.EA, R.EH, B, dtype="bf16", mask_mode="external", seed=0)
    eng.set_tuning(split_fwd=split, dw_fuse=dw_fuse, policy_fused=policy_fused)
    load = [(L.NET_POLICY, "actor"), (L.NET_TARGET_POLICY, "actor"), (L.NET_VALUE1, "critic1"), (L.NET_TARGET_VALUE1, "critic1")]
    if td3:
        load += [(L.NET_VALUE2, "critic2"), (L.NET_TARGET_VALUE2, "critic2")]
    for ni, name in load:
        eng.load_params(ni, {k: v.float() for k, v in nets[name].items()})
    eng.set_hyper(gamma=R.GAMMA, min_value=-2.0 ** 20, max_value=2.0 ** 20, soft_tau=0.0, policy_every=1, noise_std=0.5, noise_clip=3.0,
                  policy_opt=dict(lr=0.0), value_opt=dict(lr=0.0))
    eng.set_counters()
    eng.pack_batch(batch["state"], batch["action"], batch["reward"], batch["next_state"], batch["done"])
    eng.set_external(masks=masks, noise=noise)
    eng.step(B, True, 0)
    torch.cuda.synchronize()

    wrong = []
    for name in FORWARD + (BACKWARD if backward else ()):
        if name in ref:
            wrong.append(_differs(eng.buffer(name, B), ref[name], name))
    if backward:
        lo = eng.losses()
        delta = ref["q1"] - ref["expected"]
        for key, want in (("value1" if td3 else "value", float((delta * delta).mean())), ("policy", float(-ref["q_pi"].mean()))):
            print(f"{algo} B={B} loss {key}: got {lo[key]!r}, want {want!r}")
            if lo[key] != want:
                wrong.append(f"loss {key}: got {lo[key]!r}, want {want!r}")
        for ni, tag in ((L.NET_VALUE1, "value_grads"), (L.NET_POLICY, "policy_grads")):
            got = eng.param_views(ni, eng.grads[ni])
            for k, want in ref[tag].items():
                wrong.append(_differs(got[k], want, f"{tag}.{k}"))
    # the critic's optimizer launch ran on a learning rate of zero: the parameters are the lattice's, bit for bit
    for k, v in eng.param_views(L.NET_VALUE1).items():
        wrong.append(_differs(v, nets["critic1"][k], f"critic1.{k} after the step"))
    wrong = [w for w in wrong if w]
    assert not wrong, "\n".join(wrong)

    # ---- which launches these numbers came from
    names = {n for n, _, _ in eng.profile(B, policy=True, n_steps=1)}
    if split == 2:
        assert SPLIT <= names and "mlp_fwd_nets" not in names, names
    else:
        assert "mlp_fwd_nets" in names and not (SPLIT & names), names
    # the critic's dW with Adam in its epilogue: the split forward's backward tensors at 1024 rows, dw_fuse on; else dW slabs + a reduction
    assert ("dwadam_critic" in names) == bool(B >= 1024 and split == 2 and dw_fuse), names
    if policy_fused == 0 or B < 1024:            # the actor's dW as batch slabs + a reduction, or (1024 rows on the split forward) without slabs
        assert "dwgrad_actor" not in names and "dw_actor" in names, names
    elif split == 2:
        assert "dwgrad_actor" in names and "dw_actor" not in names, names
