"""Launch plans and bit-level results of the step engine over its schedules, as one JSON: the A/B record of a scheduling change.

A change to the step planner (csrc/engine_plan.hip) that is meant to keep every schedule as it is shows that by producing the same file
before and after; one that is meant to change a schedule shows exactly which launches moved.  Per configuration:

  * plan:   eng.profile(rows, policy, n_steps=1) for policy False and True (cycle configurations: policy=2), as ["name flops"];
  * losses: float.hex() of every loss of four eager steps (steps 0-3, policy_every=2, Adam, fixed seeds) -- cycle configurations: of a
            24-step run replayed as run graphs (cycle_min_len=2, cycle_min_seg=2: the batched frozen networks and the deferred
            policy-loss critic under capture; "run" configurations: the same run outside cycle mode, where the deferred critic rides in
            the fused forward / the split-bf16 launches);
  * sha256: of every bound network's parameters, both moments and gradient arena after the last step (a shard's file keeps one per
            arena; the merged file one digest of them per configuration, and stores equal plans and equal records once: _pack).

    python tools/plan_dump.py --list                      # the configuration names
    python tools/plan_dump.py --shard 0/4 --out a0.json   # every 4th configuration, starting at the first
    python tools/plan_dump.py --merge a0.json a1.json a2.json a3.json --out profiles/plan_dump.json
    python tools/plan_dump.py --diff old.json new.json    # names of the configurations that differ (exit status 1 if any)

Needs a GPU for --shard; the engines are built with the suite's own helpers (tests/test_gpu_engine.py, tests/test_gpu_bench_shape.py)."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BIG, SMALL = (1290, 128, 256), (27, 8, 16)
# one field at a time against the defaults (frozen_gemm only matters without the fused frozen launches)
TUNINGS = [("split_fwd", 0), ("split_fwd", 2), ("fused_mlp", 0), ("fused_mlp", 2), ("chain_target_critic", 0), ("bwd_panel", 1), ("bwd_panel", 0),
           ("policy_chain", 0), ("tail_half", 0), ("x3_tail", 0), ("frozen_fused", 0, "frozen_gemm", 1), ("frozen_fused", 0, "frozen_gemm", 0)]
CYCLE_TUNINGS = [(), ("frozen_window", 0), ("frozen_fused", 0), ("frozen_fused", 0, "frozen_gemm", 0)]
# run graphs outside cycle mode: the deferred policy-loss critic in the fused forward (bf16) and in the split-bf16 launches
RUN_CONFIGS = [("bf16", ("split_fwd", 0)), ("bf16x3", ())]
CYCLE_STEPS = 24


def _tname(t):
    return "+".join(f"{t[i]}={t[i + 1]}" for i in range(0, len(t), 2)) or "defaults"


def configs():
    """[(name, kind, fields)]: algorithm x dtype x rows x {hash, none} x {defaults, each tuning}, external masks once per dtype."""
    out = []
    for algo in ("ddpg", "td3"):
        for dtype in ("fp32", "bf16", "bf16x3"):
            for rows in (128, 80):       # 80: no multiple of 32 or 128 -- half panels off, no frozen search
                for mask in ("hash", "none"):
                    for t in [()] + TUNINGS:
                        if t and t[0] == "x3_tail" and dtype != "bf16x3":
                            continue
                        out.append((f"{algo}/{dtype}/big/r{rows}/{mask}/{_tname(t)}", "eager", dict(algo=algo, dtype=dtype, shape=BIG, rows=rows, mask=mask, tuning=t)))
            out.append((f"{algo}/{dtype}/big/r128/external/defaults", "eager", dict(algo=algo, dtype=dtype, shape=BIG, rows=128, mask="external", tuning=())))
        for rows in (128, 80):           # the generic GEMM path
            for mask in ("hash", "none"):
                out.append((f"{algo}/fp32/small/r{rows}/{mask}/defaults", "eager", dict(algo=algo, dtype="fp32", shape=SMALL, rows=rows, mask=mask, tuning=())))
        for t in CYCLE_TUNINGS:
            out.append((f"{algo}/bf16/cycle/{_tname(t)}", "cycle", dict(algo=algo, tuning=t)))
        for dtype, t in RUN_CONFIGS:
            out.append((f"{algo}/{dtype}/run/{_tname(t)}", "cycle", dict(algo=algo, tuning=t, dtype=dtype, cycle=False)))
    return out


def _plan(eng, rows, policy):
    return [f"{name} {flops!r}" for name, _, flops in eng.profile(rows, policy, n_steps=1)]


def _digests(eng):
    import torch
    torch.cuda.synchronize()
    out = {}
    for ni in eng.nets:
        for key, arena in (("p", eng.params), ("m", eng.adam_m), ("v", eng.adam_v), ("g", eng.grads)):
            if ni in arena:
                out[f"{key}{ni}"] = hashlib.sha256(arena[ni].detach().cpu().numpy().tobytes()).hexdigest()
    return out


def _hex(losses):
    return {k: float(v).hex() for k, v in losses.items() if k != "step"}


def run_eager(algo, dtype, shape, rows, mask, tuning):
    import torch
    from recnn_amd import _lib as L
    from tests.test_gpu_engine import _engine, _init_nets, _rand_batch
    S, A, H = shape
    td3 = algo == "td3"
    actor, critics = _init_nets(8, S, A, H, 2 if td3 else 1)
    eng = _engine(algo, S, A, H, rows, dtype, mask_mode=mask, seed=17)
    if tuning:
        eng.set_tuning(**dict(zip(tuning[::2], tuning[1::2])))
    nets = [(L.NET_POLICY, actor), (L.NET_TARGET_POLICY, actor), (L.NET_VALUE1, critics[0]), (L.NET_TARGET_VALUE1, critics[0])]
    if td3:
        nets += [(L.NET_VALUE2, critics[1]), (L.NET_TARGET_VALUE2, critics[1])]
    for ni, p in nets:
        eng.load_params(ni, p)
    o = dict(kind="adam", lr=1e-3, weight_decay=1e-2)
    eng.set_hyper(policy_opt=dict(o), value_opt=dict(o), policy_every=2, soft_tau=0.05)
    eng.set_counters()
    gen = torch.Generator().manual_seed(31)
    losses = []
    for t in range(4):
        b = _rand_batch(rows, S, A, gen)
        eng.pack_batch(b["state"], b["action"], b["reward"], b["next_state"], b["done"])
        if mask == "external":
            eng.set_external(masks=[(torch.rand(rows, H, generator=gen) < 0.5).to(torch.uint8) for _ in range(eng.n_masks)])
        eng.step(rows, True, t)
        losses.append(_hex(eng.losses()))
    rec = {"losses": losses, "sha256": _digests(eng)}
    rec["plan"] = {"value_step": _plan(eng, rows, False), "policy_step": _plan(eng, rows, True)}      # (profile() steps the engine: last)
    return rec


_ENV = {}


def run_cycle(algo, tuning, dtype="bf16", cycle=True):
    import torch
    import recnn_amd
    from recnn_amd._tune import set_default_tuning
    from recnn_amd.nn import fused
    from tests import test_gpu_bench_shape as B
    cuda = torch.device("cuda:0")
    if "env" not in _ENV:
        _ENV["env"] = B._bench_env(recnn_amd, cuda, n_users=(CYCLE_STEPS + 2) * B.UPB)[0]
    fields = dict(zip(tuning[::2], tuning[1::2]), cycle_min_len=2, cycle_min_seg=2)
    set_default_tuning(**fields)
    try:
        if algo == "ddpg":
            a = B._make_algo(recnn_amd, cuda, _ENV["env"], dtype)
        else:
            nn = recnn_amd.nn
            fused.set_defaults(dtype=dtype, mask_mode="hash", seed=B.SEED)
            torch.manual_seed(12)
            a = nn.TD3(nn.Actor(1290, 128, 256, 6e-1), nn.Critic(1290, 128, 256, 54e-2), nn.Critic(1290, 128, 256, 54e-2)).to(cuda)
            torch.manual_seed(99)
            a.attach_env(_ENV["env"], rows_per_batch=B.ROWS, users_per_batch=B.UPB)
        eng = a._fused_ctx.engine
        assert all(getattr(eng.tuning, k) == v for k, v in fields.items())
        _, hist = a.run(CYCLE_STEPS, history=True)
        rec = {"losses": [_hex(h) for h in hist], "sha256": _digests(eng)}
        if cycle:
            rec["plan"] = {"cycle": _plan(eng, B.ROWS, 2)}
        else:
            rec["plan"] = {"value_step": _plan(eng, B.ROWS, False), "policy_step": _plan(eng, B.ROWS, True)}
        return rec
    finally:
        set_default_tuning(**{k: None for k in fields})


def _key(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()[:10]


def _pack(doc):
    """The merged file is kept small: many configurations share a launch plan or a whole record, so plans and records are stored once
    under a key made of their content; the arenas' digests of a configuration become one digest of them; losses lose their names
    (sorted by name: policy, value / policy, value1, value2)."""
    out = {"configs": {}, "records": {}, "plans": {}}
    for name in sorted(doc):
        r = doc[name]
        plans = {}
        for which, plan in r["plan"].items():
            plans[which] = _key(plan)
            out["plans"][plans[which]] = plan
        rec = {"plan": plans, "losses": [[step[k] for k in sorted(step)] for step in r["losses"]],
               "sha256": hashlib.sha256("".join(f"{k}:{v}\n" for k, v in sorted(r["sha256"].items())).encode()).hexdigest()}
        out["configs"][name] = _key(rec)
        out["records"][out["configs"][name]] = rec
    return out


def _load(path):
    """A shard's file or a merged one, as {configuration: record} with the plans written out."""
    d = json.load(open(path))
    if "configs" not in d:
        d = _pack(d)
    return {name: dict(d["records"][k], plan={w: d["plans"][p] for w, p in d["records"][k]["plan"].items()}) for name, k in d["configs"].items()}


def _write(path, doc):
    with open(path, "w") as f:       # one entry per line, sorted: the file diffs line by line
        f.write("{\n" + ",\n".join(f"{json.dumps(s)}: {{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(doc[s][k], sort_keys=True)}" for k in sorted(doc[s])) + "\n}"
                                   for s in sorted(doc)) + "\n}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--shard", default=None, metavar="I/N")
    ap.add_argument("--merge", nargs="+", default=None, metavar="JSON")
    ap.add_argument("--diff", nargs=2, default=None, metavar="JSON")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfgs = configs()
    if args.list:
        print("\n".join(name for name, _, _ in cfgs))
        return 0
    if args.diff:
        a, b = (_load(p) for p in args.diff)
        bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        for k in bad:
            what = [f for f in ("plan", "losses", "sha256") if (a.get(k) or {}).get(f) != (b.get(k) or {}).get(f)]
            print(f"differs: {k} ({', '.join(what)})")
        print(f"{len(bad)} of {len(set(a) | set(b))} configurations differ")
        return 1 if bad else 0
    if args.merge:
        doc = {}
        for p in args.merge:
            doc.update(json.load(open(p)))
        missing = [name for name, _, _ in cfgs if name not in doc]
        assert not missing, f"configurations missing from the merge: {missing}"
        _write(args.out, _pack(doc))
        return 0
    i, n =(int(x) for x in args.shard.split("/"))
    doc = {}
    for name, kind, fields in cfgs[i::n]:
        doc[name] = run_eager(**fields) if kind == "eager" else run_cycle(**fields)
        print(name, flush=True)
    with open(args.out, "w") as f:       # (a shard keeps every arena's own digest, for looking into a difference)
        json.dump(doc, f, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
