#!/usr/bin/env python3
"""The DDPG step's input-gradient launch (csrc/state_grad.hip, `recnn_engine_state_grads`) against eager torch on the
same GPU, and what the attached route of `ddpg_update` costs.

Per shape (rows, S, A, H) and compute type (fp32, bf16), on an engine that has just run the phase the launch reads from:
  value_ms / policy_ms              one `StepEngine.state_grads(rows, 0 | 1)` call: gV = dz_c1 W1c[:, state] (one contraction segment) /
                                    gP = dz_e1 W1c[:, state] + dz_p1 W1a (two)
  torch_value_ms / torch_policy_ms  torch.matmul on fp32 copies of the same buffers: one matmul / two matmuls and an add
  value_bytes / policy_bytes        rows K sizeof(dz) + K S sizeof(W) + rows S 4 with K = H per segment: what the launch must move
  max_abs_diff_*                    max |hip - torch| (information; tests/test_gpu_state_grad.py holds the launch to its derived bound)
Whole update: `ddpg_update` on a `SeqEnv.user_batch` of U = 25 users, 2 kept steps, T = 40 encoder steps (Actor / Critic 256-128-256,
LSTM(129, 256), recnn_amd.optim.Adam, fp32), with the state attached to the encoder's graph against the same rows detached, on a
policy step and on an ordinary one.  Every timed call builds its batch (`user_batch`: the encode, recorded for the attached one) and
runs the update; the attached figures also contain the backward passes through the encoder (one per loss).
Device-event times around the Python call, median of `--repeats` calls after one warm-up call.  Writes one JSON file and prints it.

--algo td3 times, on a TD3 engine and per shape and compute type,
  merged_ms                         one `state_grads(rows, 3)`: gV1 + gV2, two contraction segments (per-segment seeds where the fused bf16
                                    forward left unit backward tensors: `unit_backward`)
  split_ms                          `state_grads(rows, 0)` + `state_grads(rows, 2)` + a torch add of the two outputs
  torch_merged_ms                   two torch.matmul and an add on fp32 copies of the same buffers
and a whole `td3_update` on the same user batch as above (three recnn_amd.optim.Adam; the encoder in the policy optimizer), attached
against detached, on a policy step and on an ordinary one.  Its figures go under the "td3" key of the same JSON file; what the file
already holds is kept.
usage: python tools/state_grad_bench.py [--algo ddpg|td3] [--repeats 5] [--out profiles/state_grad_bench.json]"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = ((50, 256, 128, 256), (1000, 256, 128, 256), (2048, 1290, 128, 256))


def median_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return float(np.median(times))


def launch_case(rows, S, A, H, dtype, repeats, dev):
    from recnn_amd import _lib as L
    from recnn_amd.nn.engine import StepEngine
    gen = torch.Generator().manual_seed(rows)

    def mk(inp, out):
        return {"w1": torch.randn(H, inp, generator=gen) * 0.03, "b1": torch.randn(H, generator=gen) * 0.1,
                "w2": torch.randn(H, H, generator=gen) * 0.06, "b2": torch.randn(H, generator=gen) * 0.1,
                "w3": torch.randn(out, H, generator=gen) * 0.3, "b3": torch.randn(out, generator=gen) * 0.3}
    actor, critic = mk(S, A), mk(S + A, 1)
    eng = StepEngine("ddpg", S, A, H, rows, dtype=dtype, mask_mode="hash", seed=1, device=dev)
    for ni, p in ((L.NET_POLICY, actor), (L.NET_TARGET_POLICY, actor), (L.NET_VALUE1, critic), (L.NET_TARGET_VALUE1, critic)):
        eng.load_params(ni, p)
    eng.set_hyper(policy_every=1, policy_opt=dict(lr=1e-3), value_opt=dict(lr=1e-3))
    eng.set_counters()
    eng.pack_batch(torch.randn(rows, S, generator=gen), torch.randn(rows, A, generator=gen), torch.randn(rows, generator=gen),
                   torch.randn(rows, S, generator=gen), (torch.rand(rows, generator=gen) < 0.1).float())
    esz = 4 if dtype == "fp32" else 2
    seen = (lambda w: w.bfloat16().float()) if dtype == "bf16" else (lambda w: w.float())
    res = {"rows": rows, "S": S, "A": A, "H": H, "dtype": dtype, "workgroups": ((rows + 63) // 64) * ((S + 63) // 64)}
    out = torch.empty(rows, S, device=dev)

    eng.value_grads(rows, True)
    res["value_ms"] = median_ms(lambda: eng.state_grads(rows, 0, out=out), repeats)
    dz = eng.buffer("critic1_dz1", rows).float().contiguous()
    w = seen(eng.param_views(L.NET_VALUE1)["w1"][:, :S]).contiguous()
    res["torch_value_ms"] = median_ms(lambda: torch.matmul(dz, w), repeats)
    res["max_abs_diff_value"] = float((out - torch.matmul(dz, w)).abs().max())
    res["value_bytes"] = rows * H * esz + H * S * esz + rows * S * 4

    eng.value_apply(False)
    eng.policy_grads(rows, True)
    res["policy_ms"] = median_ms(lambda: eng.state_grads(rows, 1, out=out), repeats)
    de, dp = eng.buffer("dze1", rows).float().contiguous(), eng.buffer("dzp1", rows).float().contiguous()
    wc = seen(eng.param_views(L.NET_VALUE1)["w1"][:, :S]).contiguous()
    wa = seen(eng.param_views(L.NET_POLICY)["w1"]).contiguous()
    res["torch_policy_ms"] = median_ms(lambda: torch.matmul(de, wc) + torch.matmul(dp, wa), repeats)
    res["max_abs_diff_policy"] = float((out - (torch.matmul(de, wc) + torch.matmul(dp, wa))).abs().max())
    res["policy_bytes"] = 2 * (rows * H * esz + H * S * esz) + rows * S * 4
    eng.finish(rows, True, False)
    torch.cuda.synchronize()
    return res


def launch_case_td3(rows, S, A, H, dtype, repeats, dev):
    from recnn_amd import _lib as L
    from recnn_amd.nn.engine import StepEngine
    gen = torch.Generator().manual_seed(rows)

    def mk(inp, out):
        return {"w1": torch.randn(H, inp, generator=gen) * 0.03, "b1": torch.randn(H, generator=gen) * 0.1,
                "w2": torch.randn(H, H, generator=gen) * 0.06, "b2": torch.randn(H, generator=gen) * 0.1,
                "w3": torch.randn(out, H, generator=gen) * 0.3, "b3": torch.randn(out, generator=gen) * 0.3}
    actor, critic1, critic2 = mk(S, A), mk(S + A, 1), mk(S + A, 1)
    eng = StepEngine("td3", S, A, H, rows, dtype=dtype, mask_mode="hash", seed=1, device=dev)
    for ni, p in ((L.NET_POLICY, actor), (L.NET_TARGET_POLICY, actor), (L.NET_VALUE1, critic1), (L.NET_TARGET_VALUE1, critic1),
                  (L.NET_VALUE2, critic2), (L.NET_TARGET_VALUE2, critic2)):
        eng.load_params(ni, p)
    eng.set_hyper(policy_every=1, policy_opt=dict(lr=1e-3), value_opt=dict(lr=1e-3))
    eng.set_counters()
    eng.pack_batch(torch.randn(rows, S, generator=gen), torch.randn(rows, A, generator=gen), torch.randn(rows, generator=gen),
                   torch.randn(rows, S, generator=gen), (torch.rand(rows, generator=gen) < 0.1).float())
    esz = 4 if dtype == "fp32" else 2
    seen = (lambda w: w.bfloat16().float()) if dtype == "bf16" else (lambda w: w.float())
    res = {"rows": rows, "S": S, "A": A, "H": H, "dtype": dtype, "workgroups": ((rows + 63) // 64) * ((S + 63) // 64)}
    out, o0, o2 = (torch.empty(rows, S, device=dev) for _ in range(3))

    eng.value_grads(rows, True)
    res["unit_backward"] = int(eng.lib.recnn_engine_unit_backward(eng.handle))
    res["merged_ms"] = median_ms(lambda: eng.state_grads(rows, 3, out=out), repeats)

    def split():
        eng.state_grads(rows, 0, out=o0)
        eng.state_grads(rows, 2, out=o2)
        return o0 + o2
    res["split_ms"] = median_ms(split, repeats)
    dz = [eng.buffer(f"critic{c}_dz1", rows).float().contiguous() for c in (1, 2)]
    w = [seen(eng.param_views(ni)["w1"][:, :S]).contiguous() for ni in (L.NET_VALUE1, L.NET_VALUE2)]
    ref = lambda: torch.matmul(dz[0], w[0]) + torch.matmul(dz[1], w[1])
    res["torch_merged_ms"] = median_ms(ref, repeats)
    res["max_abs_diff_merged"] = float((out - ref()).abs().max())
    res["max_abs_diff_merged_vs_split"] = float((out - split()).abs().max())
    res["merged_bytes"] = 2 * (rows * H * esz + H * S * esz) + rows * S * 4 + (2 * rows * 4 if res["unit_backward"] else 0)
    eng.finish(rows, False, False)
    torch.cuda.synchronize()
    return res


def update_case_td3(repeats, dev):
    import recnn_amd as recnn
    from recnn_amd.data.env import SeqEnv
    from recnn_amd.nn import fused
    from recnn_amd.optim import Adam
    U, E, H, T, steps = 25, 128, 256, 40, [20, 39]
    rng = np.random.default_rng(0)
    user_dict = {u: {"items": rng.integers(0, 3000, size=T + 2).astype(np.int64),
                     "ratings": (2.0 * (rng.integers(1, 11, size=T + 2) * 0.5 - 2.5)).astype(np.float32)} for u in range(U)}
    table = torch.from_numpy(rng.standard_normal((3000, E)).astype(np.float32))
    fused.set_defaults(dtype="fp32", mask_mode="hash", seed=3)
    torch.manual_seed(0)
    pol = recnn.nn.Actor(H, E, 256, 6e-1)
    v1, v2 = recnn.nn.Critic(H, E, 256, 54e-2), recnn.nn.Critic(H, E, 256, 54e-2)
    nets = {"policy_net": pol, "value_net1": v1, "value_net2": v2, "target_policy_net": copy.deepcopy(pol).eval(),
            "target_value_net1": copy.deepcopy(v1).eval(), "target_value_net2": copy.deepcopy(v2).eval()}
    nets = {k: v.to(dev) for k, v in nets.items()}
    env = SeqEnv.from_user_dict(table, user_dict, list(range(U)), state_encoder=torch.nn.LSTM(E + 1, H).to(dev), batch_size=U,
                                max_buf_size=2 * U, device=dev)
    optimizer = {"policy_optimizer": Adam(list(pol.parameters()) + list(env.state_encoder.parameters()), lr=1e-5),
                 "value_optimizer1": Adam(v1.parameters(), lr=1e-5), "value_optimizer2": Adam(v2.parameters(), lr=1e-5)}
    params = {"gamma": 0.99, "noise_std": 0.5, "noise_clip": 3, "soft_tau": 0.001, "policy_update": 2}
    ids = list(range(U))

    def detached_update(step):
        with torch.no_grad():
            batch = env.user_batch(ids, steps)
        recnn.nn.update.td3_update(batch, params, nets, optimizer, learn=True, step=step)

    def attached_update(step):       # (a fresh batch per call: the update steps the encoder, which invalidates the previous graph)
        recnn.nn.update.td3_update(env.user_batch(ids, steps), params, nets, optimizer, learn=True, step=step)

    res = {"U": U, "kept_steps": len(steps), "T": steps[-1] + 1, "rows": U * len(steps), "S": H, "A": E, "H": 256, "dtype": "fp32"}
    for name, step in (("policy_step", 0), ("ordinary_step", 1)):
        res[f"{name}_detached_ms"] = median_ms(lambda: detached_update(step), repeats)
        res[f"{name}_attached_ms"] = median_ms(lambda: attached_update(step), repeats)
    return res


def update_case(repeats, dev):
    import recnn_amd as recnn
    from recnn_amd.data.env import SeqEnv
    from recnn_amd.nn import fused
    from recnn_amd.optim import Adam
    U, E, H, T, steps = 25, 128, 256, 40, [20, 39]
    rng = np.random.default_rng(0)
    user_dict = {u: {"items": rng.integers(0, 3000, size=T + 2).astype(np.int64),
                     "ratings": (2.0 * (rng.integers(1, 11, size=T + 2) * 0.5 - 2.5)).astype(np.float32)} for u in range(U)}
    table = torch.from_numpy(rng.standard_normal((3000, E)).astype(np.float32))
    fused.set_defaults(dtype="fp32", mask_mode="hash", seed=3)
    torch.manual_seed(0)
    pol, val = recnn.nn.Actor(H, E, 256, 6e-1), recnn.nn.Critic(H, E, 256, 54e-2)
    nets = {"policy_net": pol, "value_net": val, "target_policy_net": copy.deepcopy(pol).eval(), "target_value_net": copy.deepcopy(val).eval()}
    nets = {k: v.to(dev) for k, v in nets.items()}
    env = SeqEnv.from_user_dict(table, user_dict, list(range(U)), state_encoder=torch.nn.LSTM(E + 1, H).to(dev), batch_size=U,
                                max_buf_size=2 * U, device=dev)
    optimizer = {"policy_optimizer": Adam(list(pol.parameters()) + list(env.state_encoder.parameters()), lr=1e-5),
                 "value_optimizer": Adam(val.parameters(), lr=1e-5)}
    params = {"gamma": 0.99, "min_value": -10, "max_value": 10, "policy_step": 2, "soft_tau": 0.001}
    ids = list(range(U))

    def detached_update(step):
        with torch.no_grad():
            batch = env.user_batch(ids, steps)
        recnn.nn.update.ddpg_update(batch, params, nets, optimizer, learn=True, step=step)

    def attached_update(step):       # (a fresh batch per call: the update steps the encoder, which invalidates the previous graph)
        recnn.nn.update.ddpg_update(env.user_batch(ids, steps), params, nets, optimizer, learn=True, step=step)

    def encode_detached():
        with torch.no_grad():
            env.user_batch(ids, steps)

    res = {"U": U, "kept_steps": len(steps), "T": steps[-1] + 1, "rows": U * len(steps), "S": H, "A": E, "H": 256, "dtype": "fp32",
           "user_batch_detached_ms": median_ms(encode_detached, repeats),
           "user_batch_attached_ms": median_ms(lambda: env.user_batch(ids, steps), repeats)}
    for name, step in (("policy_step", 0), ("ordinary_step", 1)):
        res[f"{name}_detached_ms"] = median_ms(lambda: detached_update(step), repeats)
        res[f"{name}_attached_ms"] = median_ms(lambda: attached_update(step), repeats)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", choices=("ddpg", "td3"), default="ddpg")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_grad_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "state_grad_bench needs a GPU"
    dev = torch.device("cuda")
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    launch, update = (launch_case, update_case) if args.algo == "ddpg" else (launch_case_td3, update_case_td3)
    res = {"arch": arch, "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "launch": [launch(*shape, dtype, args.repeats, dev) for shape in SHAPES for dtype in ("fp32", "bf16")],
           "update": update(args.repeats, dev)}
    out = {}
    if os.path.exists(args.out):            # one file for both algorithms: keep what the other run wrote
        with open(args.out) as f:
            out = json.load(f)
    if args.algo == "td3":
        out["td3"] = res
    else:
        out = dict(res, **({"td3": out["td3"]} if "td3" in out else {}))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
