#!/usr/bin/env python3
"""bench.py -- DDPG update steps/sec (batch 2048 transition rows, frame 10, emb 128) on N MI355X.

One "step" = the whole hot path of BASELINE.json's north_star on one batch of synthetic ML20M-shaped data:
  replay sampler (row plan) -> embedding gather -> target/actor/critic forward -> critic backward -> Adam ->
  policy loss through the updated critic -> [every 10th step: actor backward, L1 clip quirk, Adam, soft update]
all inside librecnn_hip.so (hipGraph replay), inputs resident in HBM.  Nothing is skipped inside the timed region.

Contract (driver): python bench.py --gpus N --steps K --warmup W  -> ONE JSON line on rank 0.
value = total update steps/s over all ranks (weak scaling: every rank runs its own B=2048 step on its own shard
of the replay users; gradients are all-reduced over RCCL when N > 1).

A plain run does only what that line's headline needs: set up, warm up, time the `--repeats` regions of K steps, write
--dump-outputs, print.  --full adds everything else the line has carried: the sustained 2000-step region, the per-launch
profile and rooflines (with two rocprofv3 child runs for PMC traffic), the sub-records (parity mode, other configs, loss-curve
deviation from the CPU oracle), the CPU baseline and, for N > 1, the timing of both collectives; --no-traffic / --no-extras /
--no-cpu-baseline then leave out their part of it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

B_ROWS, FRAME, EMB, HIDDEN = 2048, 10, 128, 256
STATE = FRAME * EMB + FRAME
N_USERS, N_ITEMS = 138_493, 26_744           # ML20M as processed by the reference
USERS_PER_BATCH = 256                        # >= 2048 rows guaranteed (every user has >= 10 windows)
GATHER_BYTES_PER_ROW = {"fp32": 16_604,       # 5,632 + 132 read, 10,840 written (fp32 rows)
                        "bf16": 11_192,       # same reads, 5,428 written (bf16 rows): what the bf16 engine materialises
                        "bf16x3": 16_620}     # split-bf16 rows (hi + lo = 4 bytes per value: 10,856 written incl. the reward / done floats)
HBM_PEAK_GBS = 8000.0                        # MI355X_MICROARCH.md
# dense MFMA peaks the ALGORITHMIC flops are priced against; "bf16x3" (split bf16: three bf16 MFMAs per product, fp32-grade
# results) executes 3x its algorithmic flops on the bf16 pipe, so its ceiling is a third of the bf16 peak
MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3, "bf16x3": 2500.0 / 3}


def synthetic_store(seed=0):
    """ML20M-shaped replay store: lognormal history lengths (>= 20), uniform item ids, ratings in {-4..5}."""
    rng = np.random.default_rng(seed)
    lens = np.clip(np.round(rng.lognormal(4.22, 1.22, N_USERS)), 20, 9254).astype(np.int64)
    off = np.zeros(N_USERS + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    items = rng.integers(0, N_ITEMS, size=total, dtype=np.int32)
    ratings = (2.0 * (rng.integers(1, 11, size=total) * 0.5 - 2.5)).astype(np.float32)
    return items, ratings, off, lens


def init_nets(seed=0):
    """Actor(1290,128,256,6e-1), Critic(1290,128,256,54e-2) with the reference's constructor RNG order."""
    torch.manual_seed(seed)

    def mk(inp, out, init_w):
        l1, l2, l3 = torch.nn.Linear(inp, HIDDEN), torch.nn.Linear(HIDDEN, HIDDEN), torch.nn.Linear(HIDDEN, out)
        l3.weight.data.uniform_(-init_w, init_w)
        l3.bias.data.uniform_(-init_w, init_w)
        return {"w1": l1.weight.data, "b1": l1.bias.data, "w2": l2.weight.data, "b2": l2.bias.data,
                "w3": l3.weight.data, "b3": l3.bias.data}
    critic = mk(STATE + EMB, 1, 54e-2)
    actor = mk(STATE, EMB, 6e-1)
    return actor, critic


def cpu_baseline(items, ratings, off, table, budget_s=12.0):
    """The CPU restatement of the reference (oracle/, validated against the real reference in the build container)
    timed on this host: collate (windows + gather) + ddpg_update with Adam, fp32, all cores."""
    from oracle import recnn_oracle as O
    actor, critic = init_nets(0)
    st = O.DDPGState.create(O.clone_params(actor), O.clone_params(critic), O.AdamState(lr=1e-5, weight_decay=1e-2),
                            O.AdamState(lr=1e-5, weight_decay=1e-2))
    rng = np.random.default_rng(1)
    tab = table.numpy()

    def one(step):
        users = rng.integers(0, N_USERS, size=USERS_PER_BATCH)
        ui = [items[off[u]:off[u + 1]].astype(np.int64) for u in users]
        ur = [ratings[off[u]:off[u + 1]].astype(np.float64) for u in users]
        # only as many users as the 2048 rows need (the reference collates whole users)
        need, k = 0, 0
        while need < B_ROWS:
            need += len(ui[k]) - FRAME
            k += 1
        b = O.frame_batch(ui[:k], ur[:k], tab, FRAME, rows=B_ROWS)
        masks = O.draw_dropout_masks(6, B_ROWS, HIDDEN)
        O.ddpg_step(st, b, masks, step=step, learn=True)
    # pick the intra-op thread count that runs this step fastest on this host (many-core hosts lose badly
    # to oversubscription at these GEMM sizes), then time a bounded sample with it
    ncpu = os.cpu_count() or 1
    best, best_t = 1, None
    for nt in sorted({min(ncpu, c) for c in (8, 16, 32, 64)}):
        torch.set_num_threads(nt)
        one(0)
        t0 = time.perf_counter()
        for k in range(3):               # three steps per candidate: one step's time moves by more than the candidates differ
            one(1 + k)
        dt = time.perf_counter() - t0
        if best_t is None or dt < best_t:
            best, best_t = nt, dt
    torch.set_num_threads(best)
    t0 = time.perf_counter()
    n = 0
    while True:
        one(n + 4)
        n += 1
        el = time.perf_counter() - t0
        if el > budget_s and n >= 3:
            break
    # cores = the threads actually used (the contract's definition); host_cpu_count = what the box has
    return {"value": n / el, "unit": "steps/s", "cores": torch.get_num_threads(), "threads": torch.get_num_threads(),
            "host_cpu_count": ncpu, "kind": "port",
            "sample": f"{n} DDPG steps of B={B_ROWS} (collate + update, fp32, Adam) in {el:.1f}s with {torch.get_num_threads()} "
                      f"intra-op threads (fastest of 8/16/32/64 on this {ncpu}-core host)"}


# launch-slot name (recnn_engine_profile) -> substring of the kernel symbol rocprofv3 reports
KERNEL_OF_SLOT = {"mlp_fwd_nets": "mlps_fwd_kernel", "mlp_fwd_critic": "mlps_fwd_kernel", "l1_critic": "l1_gemm_kernel", "tail_critic": "mlp_tail_kernel",
                  "frozen_actors": "mlp_frozen_kernel", "frozen_target_critics": "mlp_frozen_kernel",
                  "frame_gather": "frame_gather_kernel", "dw_critic": "gemm_dw_dma_kernel",
                  "adam_critic": "apply_kernel", "adam_critic+gather": "apply_gather_kernel",
                  "fwd_l1": "x3_fwd_ws_kernel<2, 2, 2, 4, 4, 3", "x3_tail": "x3_tail_kernel",   # (the 64 x 128-tile instance: the grouped layer-1 launch)
                  "dwadam_critic": "dw_adam_kernel", "dw_actor": "gemm_dw_dma_kernel", "adam_actor": "apply_kernel",
                  "frame_gather_cycle": "frame_gather_multi_kernel", "bwd_chain_policy": "bwd_chain_kernel",
                  "grad_reduce_actor": "grad_reduce_kernel", "grad_reduce_critic": "grad_reduce_kernel",
                  "fwd_l1_pcritic": "gemm_fwd_dma_kernel", "fwd_l2_pcritic": "gemm_fwd_dma_kernel"}
PARAMS = {"critic": 429_313, "actor": 429_184}      # parameters per network


FROZEN_SLOTS = ("frame_gather_cycle", "td3_noise", "frozen_actors", "frozen_target_critics", "l1_frozen_actors", "l2_frozen_actors",
                "l3_frozen_actors", "tail_frozen_actors", "l1_frozen_target_critic", "l2_frozen_target_critic",
                "q_frozen_target_critic", "tail_frozen_target_critic")    # launches of the cycle schedule that serve a whole policy cycle


def pick_dominant(launches, policy_every):
    """launches: [(slot name, mean ms per launch, algorithmic flops per launch)] of the schedule the timed region replayed.
    Returns (flop-dominant launch, time-dominant launch, per-step flops of a launch, per-step ms of a launch): the dominant kernel of an
    MFMA roofline is the launch that carries the largest share of the step's ALGORITHMIC FLOPS -- fused schedule: the row-panel forward of
    all networks (also the longest launch: rounds 1-4's choice); cycle schedule: the batched frozen-network launch.  By TIME per step the
    cycle schedule's longest MFMA launch is the learning critic's tail (a dependent latency chain of 0.5 GFLOP): reported beside it.
    Launches in FROZEN_SLOTS run once per policy cycle and count 1 / policy_every per step.  No MFMA launch at all: the longest launch."""
    per_step = lambda r, v: v / policy_every if r[0] in FROZEN_SLOTS else v
    flops_per_step = lambda r: per_step(r, r[2])
    share = lambda r: per_step(r, r[1])
    cand = [r for r in launches if r[2] > 0]
    if not cand:
        dom = max(launches, key=lambda r: r[1])
        return dom, dom, flops_per_step, share
    return max(cand, key=flops_per_step), max(cand, key=share), flops_per_step, share


PCRITIC_SLOTS = ("fwd_l1_pcritic", "fwd_l2_pcritic", "mlp_fwd_pcritic")     # the policy-loss forward through the updated critic
PCRITIC_HOST = {"fwd_l1_pcritic": ("l1_critic", "mlp_fwd_nets"), "fwd_l2_pcritic": ("tail_critic", "mlp_fwd_nets"),
                "mlp_fwd_pcritic": ("mlp_fwd_nets",)}


def kernel_table(used, prof, prof_pol, policy_every, deferred=False):
    """Per KERNEL SYMBOL of the schedule the timed region replayed: us per step summed over all its launches -- what
    `rocprofv3 --kernel-trace --stats` of the same command lists (profiles/rNN_cycle_stats.txt), so that `roofline` can be re-derived
    from that file: flops per launch / average duration / peak for the kernel at its top.
    used: [(slot, ms per launch, flops per launch)] of an ordinary step of that schedule (cycle schedule: + the launches that serve a whole
    policy cycle, FROZEN_SLOTS, counted 1 / policy_every per step); a policy step's EXTRA launches (prof_pol minus prof, as multisets of
    slot names: the actor's backward chain, dW, L1 norm, optimizer) are counted 1 / policy_every per step as well.
    deferred (run graphs): the policy-loss forward of an ordinary step rides as one more problem on the NEXT step's forward launch(es) --
    its own launches then run on policy steps only (1 / policy_every per step) and its flops are credited to the launch that carries it."""
    names = {n for n, _, _ in used}
    rows = []
    for n, ms, fl in used:
        w = (1.0 / policy_every) if n in FROZEN_SLOTS else 1.0
        if deferred and n in PCRITIC_SLOTS:
            host = next((h for h in PCRITIC_HOST[n] if h in names), None)
            if host:
                rows.append((host, 0.0, fl * (1.0 - 1.0 / policy_every), 0.0))   # flops only: the host launch's time already has it in-graph
                w = 1.0 / policy_every
        rows.append((n, ms, fl, w))
    left = {}
    for n, _, _ in (prof or []):
        left[n] = left.get(n, 0) + 1
    for n, ms, fl in (prof_pol or []):
        if left.get(n, 0) > 0:
            left[n] -= 1
        else:
            rows.append((n, ms, fl, 1.0 / policy_every))
    tab = {}
    for n, ms, fl, w in rows:
        k = KERNEL_OF_SLOT.get(n, n)
        t = tab.setdefault(k, {"kernel": k, "slots": [], "ms_per_step": 0.0, "flops_per_step": 0.0, "launches_per_step": 0.0})
        if n not in t["slots"]:
            t["slots"].append(n)
        t["ms_per_step"] += ms * w
        t["flops_per_step"] += fl * (w if w > 0 else 1.0)
        t["launches_per_step"] += w
    out = sorted(tab.values(), key=lambda t: -t["ms_per_step"])
    total = sum(t["ms_per_step"] for t in out) or 1.0
    for t in out:
        t["avg_ms"] = t["ms_per_step"] / t["launches_per_step"]
        t["flops_per_launch"] = t["flops_per_step"] / t["launches_per_step"]
        t["share_of_step_time"] = t["ms_per_step"] / total
    return out


class ChildTrace:
    """What the two `rocprofv3 --pmc X --kernel-trace` child runs of this benchmark saw, per kernel symbol: launches, total duration, and the
    mean FETCH_SIZE / WRITE_SIZE counter values (KB).  Kernels are looked up by a substring of their symbol."""

    def __init__(self, note=None):
        self.calls, self.total_ns, self.ctr = {}, {}, {"FETCH_SIZE": {}, "WRITE_SIZE": {}}
        self.note = note

    def names(self, sub):
        return [k for k in self.calls if sub in k]

    def graph_ms(self, sub):
        ks = self.names(sub)
        n = sum(self.calls[k] for k in ks)
        return sum(self.total_ns[k] for k in ks) / n * 1e-6 if n else None

    def traffic(self, sub):
        """(HBM bytes per launch or None, note): FETCH_SIZE doubled (gfx950 tallies 128-byte read requests at 64 B), WRITE_SIZE as is."""
        if self.note:
            return None, self.note
        m = {}
        for ctr, d in self.ctr.items():
            v = [x for k, xs in d.items() if sub in k for x in xs]
            if v:
                m[ctr] = sum(v) / len(v)
        if len(m) < 2:
            return None, f"no counter rows for {sub}"
        return (m["FETCH_SIZE"] * 1024.0 * 2.0 + m["WRITE_SIZE"] * 1024.0,
                "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes) on a child run of this command, mean per "
                f"launch of {sub}: fetch 2 x {m['FETCH_SIZE'] * 1024:.0f} B + write {m['WRITE_SIZE'] * 1024:.0f} B")

    def table(self, steps):
        """[(short symbol, us per step, calls per step, average us)] of every kernel, by time per step: the `--stats` ranking."""
        rows = []
        for k, n in self.calls.items():
            short = k.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
            rows.append((short, k, self.total_ns[k] / 1e3 / steps, n / steps, self.total_ns[k] / 1e3 / n))
        return sorted(rows, key=lambda r: -r[2])


def measure_traffic(argv_tail, timeout_s=300):
    """HBM bytes per launch from the PMC counters, collected as MI355X_MICROARCH.md (HBM / rocprofv3 sections) prescribes: FETCH_SIZE and
    WRITE_SIZE in SEPARATE `rocprofv3 --pmc X --kernel-trace` passes over a child run of this same benchmark (`--child-trace`: the timed
    regions only), counter unit KB; the FETCH pass's kernel trace is also the in-graph duration of every kernel.  Returns a ChildTrace."""
    import csv
    import shutil
    import subprocess
    import tempfile
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.isfile(rocprof):
        return ChildTrace("rocprofv3 not found")
    if any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ):
        return ChildTrace("already running under a profiler")
    ct = ChildTrace()
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix=f"recnn_pmc_{ctr}_", dir="/tmp")
        cmd = [rocprof, "--pmc", ctr, "--kernel-trace", "-d", d, "-o", "p", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__)] + argv_tail
        try:
            subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s,
                           env=dict(os.environ, TMPDIR="/tmp"), cwd="/tmp")
            for root, _, files in os.walk(d):
                for f in files:
                    if f.endswith("kernel_trace.csv") and ctr == "FETCH_SIZE":
                        for r in csv.DictReader(open(os.path.join(root, f))):
                            try:
                                dt = float(r["End_Timestamp"]) - float(r["Start_Timestamp"])
                            except (KeyError, ValueError):
                                continue
                            k = r.get("Kernel_Name", "?")
                            ct.calls[k] = ct.calls.get(k, 0) + 1
                            ct.total_ns[k] = ct.total_ns.get(k, 0.0) + dt
                    if f.endswith("counter_collection.csv"):
                        for r in csv.DictReader(open(os.path.join(root, f))):
                            if r.get("Counter_Name", ctr) != ctr:
                                continue
                            ct.ctr[ctr].setdefault(r["Kernel_Name"], []).append(float(r["Counter_Value"]))
        except Exception as ex:                                    # profiler unavailable on this box: report null
            return ChildTrace(f"{ctr} pass failed: {type(ex).__name__}")
        finally:
            shutil.rmtree(d, ignore_errors=True)
    if not ct.calls:
        ct.note = "the child run left no kernel trace"
    return ct


FLOP_PER_ROW = {"ddpg": 5.401e6, "td3": 8.106e6}    # algorithmic MLP flops per transition row, averaged over a policy cycle


def _make_algo(recnn_amd, algo_name, dtype, dev, seed):
    """Actor / Critic / facade exactly as the headline run builds them, in compute type `dtype`."""
    from recnn_amd.nn import fused
    fused.set_defaults(dtype=dtype, mask_mode="hash", seed=seed)
    torch.manual_seed(0)
    value_net = recnn_amd.nn.Critic(STATE, EMB, HIDDEN, 54e-2)
    policy_net = recnn_amd.nn.Actor(STATE, EMB, HIDDEN, 6e-1)
    if algo_name == "td3":
        return recnn_amd.nn.TD3(policy_net, value_net, recnn_amd.nn.Critic(STATE, EMB, HIDDEN, 54e-2)).to(dev)
    return recnn_amd.nn.DDPG(policy_net, value_net).to(dev)


def timed_subrun(recnn_amd, env, dev, stream, algo_name, dtype, rows, steps, warmup, reps):
    """A second engine on the same replay store, timed like the headline (made-to-order run graphs, `reps` regions of `steps`
    steps bracketed by synchronize, median): the sub-records of the JSON line (parity mode, configs[2])."""
    algo = _make_algo(recnn_amd, algo_name, dtype, dev, 1234)
    torch.manual_seed(100)
    algo.attach_env(env, rows_per_batch=rows)
    samples = []
    with torch.cuda.stream(stream):
        t_build = time.perf_counter()
        if 2 <= steps <= 64:
            for r in range(reps):
                algo.prepare_run(steps, first_step=warmup + r * steps)
        torch.cuda.synchronize(dev)
        build_s = time.perf_counter() - t_build
        algo.run(warmup)
        for r in range(reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            algo.run(steps)
            torch.cuda.synchronize(dev)
            samples.append(time.perf_counter() - t0)
    el = float(np.median(samples))
    losses = algo._fused_ctx.engine.losses()
    peak = MFMA_PEAK_TFLOPS[dtype]
    tfl = FLOP_PER_ROW[algo_name] * rows / (el / steps) / 1e12
    return {"algo": algo_name, "dtype": dtype, "rows": rows, "value": steps / el, "unit": "steps/s", "ms_per_step": el / steps * 1e3,
            "steps": steps, "warmup": warmup, "repeats": reps, "spread": (max(samples) - min(samples)) / el,
            "ms_per_step_samples": [round(x / steps * 1e3, 6) for x in samples], "graph_setup_s": round(build_s, 4),
            "end_to_end": {"tflops": tfl, "peak": peak, "frac": tfl / peak}, "final_losses": losses}


def loss_curve_deviation(recnn_amd, env, dev, dtype, n_steps=12, seed=4242):
    """Worst relative deviation of the DDPG loss curve of compute type `dtype` from the CPU oracle over `n_steps` update steps on
    the SAME batches (2048 rows of the synthetic store) and the SAME dropout masks (the engine's hash masks, dumped) -- the
    quantity north_star bounds by 1e-4.  The oracle is the checker here, not the thing measured (cf. cpu_baseline)."""
    from oracle import recnn_oracle as O
    from recnn_amd import _lib as L
    algo = _make_algo(recnn_amd, "ddpg", dtype, dev, seed)
    ost = O.DDPGState.create(O.params_from_module(algo.nets["policy_net"]), O.params_from_module(algo.nets["value_net"]),
                             O.AdamState(lr=1e-5, weight_decay=1e-2), O.AdamState(lr=1e-5, weight_decay=1e-2))
    rng = np.random.default_rng(5)
    slots = env.store.slots(env.base.train_user_dataset.users)
    worst = {"value": 0.0, "policy": 0.0}
    for i in range(n_steps):
        pick = rng.choice(slots, size=USERS_PER_BATCH, replace=False)
        batch = env.collate_slots(pick, rows_per_batch=B_ROWS)
        assert batch["state"].shape[0] == B_ROWS
        got = algo.update(batch, learn=True)
        masks = []
        for stream_id in range(6):
            m = torch.zeros(B_ROWS, HIDDEN, dtype=torch.uint8, device=dev)
            L.call("recnn_hash_mask_dump", seed, i, stream_id, B_ROWS, HIDDEN, L.ptr(m), L.current_stream())
            masks.append(m)
        torch.cuda.synchronize(dev)
        ref = O.ddpg_step(ost, {k: batch[k].float().cpu() for k in ("state", "action", "reward", "next_state", "done")},
                          [m.cpu() for m in masks], step=i, learn=True)
        algo.step()
        for k in worst:
            worst[k] = max(worst[k], abs(float(got[k]) - ref[k]) / (abs(ref[k]) + 1e-6))
    return {"steps": n_steps, "worst_rel_dev": worst, "bound": 1e-4, "within_bound": max(worst.values()) <= 1e-4}


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves, exactly as the driver would
    (`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...`), and pass
    rank 0's JSON line through.  RECNN_BENCH_SINGLE_DEVICE=1 puts every rank on GPU 0 over gloo (functional test of the
    N>1 path on a one-GPU box)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), RECNN_BENCH_SPAWNED="1")
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def reinforce_subrun():
    """BASELINE configs[4] on ONE GPU (the 8-GPU form is unmeasured): REINFORCE with Top-K off-policy correction at a 100k-item
    catalogue, the notebook's Beta behaviour policy learning inside every step, bf16 catalogue GEMMs (tools/reinforce_bench.py;
    SURVEY 8 row f1).  update iterations / s over two whole policy cycles (31 steps, 3 policy updates)."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "reinforce_bench.py")
    spec = importlib.util.spec_from_file_location("reinforce_bench", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import recnn_amd
    from recnn_amd.nn import functional as F_hip
    try:
        rec = mod.run(dtype="bf16")
    finally:
        F_hip.set_catalogue_dtype("fp32")
        recnn_amd.nn.algo.set_default_optimizer("adam")      # (main()'s setting: north_star's optimizer for the headline)
        torch.cuda.empty_cache()
    rec.update(algo="reinforce_topk", unit="update iterations/s", value=rec["it_per_s"])
    return rec


def reinforce_main(args, world, rank):
    """`python bench.py --algo reinforce --gpus N`: BASELINE configs[4] -- REINFORCE with Top-K off-policy correction at a 100k-item
    catalogue, learned Beta, bf16 catalogue GEMMs, batches from a discrete-action FrameEnv; for N > 1 the catalogue dimension of the
    actor's head and of the critic's first layer is sharded over the ranks (recnn_amd/parallel.py).  One JSON line from rank 0."""
    import importlib.util
    path = os.path.join(ROOT, "tools", "reinforce_bench.py")
    spec = importlib.util.spec_from_file_location("reinforce_bench", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    dtype = "bf16" if args.dtype == "bf16" else "fp32"
    steps = args.steps if 11 <= args.steps <= 2000 else 31
    # (RECNN_REINFORCE_ITEMS / _HIDDEN: smaller shapes for the functional tests of this entry point; the benchmark is the default)
    rec = mod.run(dtype=dtype, world=world, steps=steps, items=int(os.environ.get("RECNN_REINFORCE_ITEMS", "100000")),
                  hidden=int(os.environ.get("RECNN_REINFORCE_HIDDEN", "2048")))
    if rank == 0:
        cyc = steps - 11 if steps >= 31 else steps - 1
        out = {"metric": "REINFORCE Top-K update iterations/sec (100k-item catalogue, 256 rows, hidden 2048, learned Beta)",
               "value": rec["it_per_s"], "unit": "update iterations/s", "n_gpus": world, "steps": min(cyc, 20) if steps >= 31 else cyc,
               "warmup": 11 if steps >= 31 else 1, "ms_per_step": round(1e3 / rec["it_per_s"], 4), "higher_is_better": True,
               "scaling": "strong", "vs_baseline": None, "dtype": dtype, "data": "synthetic",
               "config": {"workload": "configs[4]: REINFORCE with Top-K off-policy correction, 100,000-item catalogue, 256 transition rows per step "
                                      "(the SAME batch on every rank), DiscreteActor / Critic hidden 2048, the notebook's Beta trained inside every "
                                      "step, fused Ranger, policy update every 10th step; catalogue dimension sharded over the ranks",
                          "parallelism": "single" if world == 1 else f"vocab-parallel x{world}"},
               "detail": rec}
        print(json.dumps(out))
    return 0


def dump_outputs(out_dir, eng):
    """--dump-outputs: what the timed path hands its caller after its last step -- that step's losses (float64) and the fp32 master
    parameters of every network (float32, the whole tensors: ~7 MB for DDPG, ~10 MB for TD3) -- as out_dir/<name>.npy."""
    from recnn_amd.nn.engine import NET_NAMES_DDPG, NET_NAMES_TD3
    os.makedirs(out_dir, exist_ok=True)
    for k, v in eng.losses().items():                     # (synchronises the engine's stream)
        np.save(os.path.join(out_dir, f"loss_{k}.npy"), np.array([v], dtype=np.float64))
    torch.cuda.synchronize()
    for net, ni in (NET_NAMES_TD3 if eng.td3 else NET_NAMES_DDPG).items():
        for p, t in eng.param_views(ni).items():
            np.save(os.path.join(out_dir, f"{net}.{p}.npy"), t.detach().float().cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "bf16x3"])
    ap.add_argument("--algo", default="ddpg", choices=["ddpg", "td3", "reinforce"],
                    help="td3 --rows 4096 = BASELINE.json configs[2]; reinforce = configs[4]: Top-K REINFORCE at a 100k-item catalogue, the catalogue "
                         "dimension sharded over --gpus ranks (tools/reinforce_bench.py)")
    ap.add_argument("--rows", type=int, default=B_ROWS, help="transition rows per step per GPU")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: sustained region, per-launch profile and rooflines, PMC traffic child runs, sub-records "
                         "(parity_mode, other_configs, loss-curve deviation), CPU baseline, N > 1 collective A/B")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--no-traffic", action="store_true", help="(--full) skip the two rocprofv3 --pmc child runs behind roofline.traffic")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: every rank steps on its own --rows rows (headline); strong: the GLOBAL batch is --rows rows, "
                         "each rank takes rows/N of it")
    ap.add_argument("--overlap", action="store_true", help="data parallel: overlap the critic all-reduce with the actor forward")
    ap.add_argument("--collective", default="peer", choices=["peer", "rccl"],
                    help="data parallel: in-graph two-shot all-reduce over peer-mapped buffers (default; falls back to rccl when "
                         "the peers cannot be mapped) or host-issued RCCL all-reduces")
    ap.add_argument("--force-dp", action="store_true", help="run the data-parallel stepper even with one rank (tests the N>1 path)")
    ap.add_argument("--repeats", type=int, default=5, help="timed regions of `--steps` steps each; value = their median")
    ap.add_argument("--no-extras", action="store_true", help="(--full) skip the sub-records (parity_mode, other_configs, loss-curve deviation)")
    ap.add_argument("--child-trace", action="store_true",
                    help="(internal: the rocprofv3 child runs behind roofline.traffic) the timed regions only -- no eager per-launch profile, no "
                         "sustained region, no sub-records: the child's kernel trace then holds the replayed schedule and nothing else")
    ap.add_argument("--preflight", action="store_true",
                    help="N > 1 diagnostics instead of the benchmark: one JSON object per stage (tools/multigpu_preflight.py)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed regions, write what the last timed step computed (its losses, every network's parameters) "
                         "as DIR/<name>.npy (rank 0; ddpg / td3)")
    args = ap.parse_args()
    if args.dump_outputs and args.algo == "reinforce":
        raise SystemExit("--dump-outputs: supported for --algo ddpg / td3")

    if args.preflight:
        if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
            spawn_ranks(args)                             # (does not return)
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import multigpu_preflight
        raise SystemExit(multigpu_preflight.main())
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args)                                 # no launcher around us: be the launcher (does not return)
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started {world} ranks (WORLD_SIZE={world})")
    if args.algo == "reinforce":
        raise SystemExit(reinforce_main(args, world, rank))
    if os.environ.get("RECNN_BENCH_SINGLE_DEVICE"):      # functional test of the N>1 path on a 1-GPU box (gloo)
        local_rank = 0
        os.environ.setdefault("RECNN_BENCH_BACKEND", "gloo")
        os.environ.setdefault("RECNN_COMM_WORKGROUPS", "32")   # the ranks' collective launches wait for each other: all resident at once
        os.environ.setdefault("RECNN_COMM_FUSED", "0")         # (... which the 420-workgroup optimizer launches of two ranks are not)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    rows = args.rows
    if args.scaling == "strong":
        if rows % world:
            raise SystemExit(f"--scaling strong: {rows} rows do not split over {world} ranks")
        rows //= world
    use_dp = world > 1 or args.force_dp
    preflight = None
    if use_dp:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29531")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        backend = os.environ.get("RECNN_BENCH_BACKEND", "nccl")
        if world > 1 and not os.environ.get("RECNN_BENCH_NO_PREFLIGHT"):
            # the N > 1 path has never run on more than one GPU (README): walk it stage by stage FIRST (tools/multigpu_preflight.py:
            # one JSON line per stage, so a hang is attributed), keep its process group, embed its summary in the JSON line
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import multigpu_preflight
            try:
                multigpu_preflight.main(keep_group=True, quick=True)
                preflight = multigpu_preflight.LAST_SUMMARY
            except Exception as ex:       # diagnostic only: the benchmark still runs
                preflight = {"ok": False, "error": f"{type(ex).__name__}: {ex}"[:300]}
        if not dist.is_initialized():
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=dev)
            else:
                dist.init_process_group(backend)
        if preflight is not None:
            # the choice of collective is made by ALL ranks together: a preflight that failed, or raised, on one rank only
            # must not send that rank down the RCCL path while its peers enter PeerComm.create's gathers
            peer_ok = bool(preflight.get("ok")) or all(preflight.get("stages", {}).get(k, False) for k in ("peer_connect", "peer_self_test"))
            votes = [None] * world
            dist.all_gather_object(votes, int(peer_ok and "error" not in preflight))
            preflight["peer_votes"] = votes
            if not min(votes):
                args.collective = "rccl"          # the device collective did not pass on every rank: host-issued RCCL all-reduces

    from recnn_amd import _lib as L
    from recnn_amd._tune import apply_env_knobs
    apply_env_knobs()            # RECNN_* tuning knobs for A/B runs from the shell (recnn_amd/_tune.py)

    import recnn_amd
    from recnn_amd.nn import fused
    items, ratings, off, lens = synthetic_store(0)
    gen = torch.Generator().manual_seed(0)
    table = torch.randn(N_ITEMS, EMB, generator=gen)
    # ---- the reference's objects: FrameEnv (device-resident replay store) + Actor/Critic + DDPG/TD3 facade
    env = recnn_amd.data.env.FrameEnv.from_store(table, items, ratings, off, frame_size=FRAME, batch_size=25, device=dev,
                                                 test_fraction=0.0)
    fused.set_defaults(dtype=args.dtype, mask_mode="hash", seed=1234 + rank)
    recnn_amd.nn.algo.set_default_optimizer("adam")        # north_star: fused Adam (the facades default to Ranger, as the reference)
    torch.manual_seed(0)                                   # same seed on every rank: replicas start identical
    value_net = recnn_amd.nn.Critic(STATE, EMB, HIDDEN, 54e-2)
    policy_net = recnn_amd.nn.Actor(STATE, EMB, HIDDEN, 6e-1)
    if args.algo == "td3":
        value_net2 = recnn_amd.nn.Critic(STATE, EMB, HIDDEN, 54e-2)
        algo = recnn_amd.nn.TD3(policy_net, value_net, value_net2).to(dev)
    else:
        algo = recnn_amd.nn.DDPG(policy_net, value_net).to(dev)   # optimizers: fused Adam(lr=1e-5, wd=1e-2)
    torch.manual_seed(100 + rank)                                 # epoch permutations differ per rank
    # dense epochs (round 4): the windows of the shuffled users concatenated and cut into `rows`-row batches -- every window of every
    # user once per epoch, as the reference's whole-user batches (recnn/data/utils.py:161-187); RECNN_SAMPLER_DENSE=0: round 1-3's
    # "256 users per batch, keep the first 2048 rows"
    dense = os.environ.get("RECNN_SAMPLER_DENSE", "1") != "0"
    algo.attach_env(env, rows_per_batch=rows, users_per_batch=None if dense else max(USERS_PER_BATCH, -(-rows // 10)), shard=(rank, world))
    ctx = algo._fused_ctx
    eng = ctx.engine

    stream = torch.cuda.Stream(device=dev)
    if not use_dp:
        def run(first, n):
            algo.run(n)                                   # hipGraph replays; ends with one loss read-back
    else:
        from recnn_amd.parallel import DataParallelStepper, PeerComm
        with torch.cuda.stream(stream):
            # the gradient exchange: recnn_dp_allreduce_flat launches inside the run graphs (peer buffers over hipIpc / xGMI,
            # csrc/comm.hip) when every rank can map its peers, else RCCL all-reduces issued by the host between phase graphs
            comm = None
            if args.collective == "peer" and not args.overlap:
                comm = PeerComm.create(PeerComm.floats_for(eng))
            collective = "peer" if comm is not None else "rccl"
            dp = DataParallelStepper(eng, rows, always_reduce=args.force_dp, overlap=args.overlap, comm=comm)

        if os.environ.get("RECNN_BENCH_SINGLE_DEVICE") and comm is not None:
            # ranks sharing ONE GPU are time-sliced, not co-scheduled: a collective launch that waits for its peer inside a
            # long run graph only proceeds when the slice ends (seconds per step, measured).  One-step graphs with a host
            # sync in between let the queues go idle and alternate: a functional check of the N > 1 path, not a measurement.
            def run(first, n):
                for t in range(first, first + n):
                    dp.step(t)
                    torch.cuda.synchronize(dev)
        else:
            def run(first, n):
                dp.run(first, n)

    def barrier():
        torch.cuda.synchronize(dev)
        if use_dp:
            dist.barrier()
            torch.cuda.synchronize(dev)

    # Timed regions: `--repeats` (default 5) regions of EXACTLY `--steps` steps, each bracketed by barrier + synchronize on both
    # sides; every region's time is the MAX over ranks; `value` is computed from the MEDIAN region, the spread is reported
    # (one 20-step region is ~1.3 ms: a single sample of that moves +-8 % from box to box and call to call).
    reps = max(1, args.repeats)
    samples = []
    graph_setup = {"made_to_order_graphs": 0, "build_s": 0.0}
    with torch.cuda.stream(stream):
        t_build = time.perf_counter()
        if use_dp and comm is not None and 2 <= args.steps <= 64:
            for r in range(reps):
                eng.graph_prepare(args.warmup + r * args.steps, args.steps)
            graph_setup["made_to_order_graphs"] = len({(args.warmup + r * args.steps) % int(eng.policy_every) for r in range(reps)})
        if not use_dp and 2 <= args.steps <= 64:
            # setup, like the rest of the graph family: every timed `run(steps)` call gets a run graph made to order for
            # (first step mod policy_step, steps), i.e. ONE graph launch instead of [ordinary stretch][cycles][policy + tail].
            # OUTSIDE the timed regions -- a capture, like building the graph family -- and its cost is reported (graph_setup)
            for r in range(reps):
                algo.prepare_run(args.steps, first_step=args.warmup + r * args.steps)
            graph_setup["made_to_order_graphs"] = len({(args.warmup + r * args.steps) % int(eng.policy_every) for r in range(reps)})
        torch.cuda.synchronize(dev)
        graph_setup["build_s"] = round(time.perf_counter() - t_build, 4)
        graph_setup["note"] = ("run graphs captured for exactly (first step mod policy_every, --steps) of each timed region, outside the timer; "
                               "0 graphs = the request is served by the standing graph family")
        run(0, args.warmup)
        if use_dp and comm is not None:
            # the warm-up steps were the first to run the exchange INSIDE the optimizer launches (PeerComm's own self-test covers the
            # stand-alone collective): if any rank saw a wait run out, every rank goes back to RCCL issued by the host
            torch.cuda.synchronize(dev)
            ok = 1
            try:
                comm.check()
            except L.RecnnHipError:
                ok = 0
            votes = [None] * world
            dist.all_gather_object(votes, ok)
            if not min(votes):
                eng.set_comm(None)
                comm = None
                collective = "rccl (the peer collective timed out in the warm-up)"
                dp = DataParallelStepper(eng, rows, always_reduce=args.force_dp, overlap=args.overlap)

                def run(first, n):
                    dp.run(first, n)
                run(args.warmup, 2)
        for r in range(reps):
            barrier()
            t0 = time.perf_counter()
            run(args.warmup + r * args.steps, args.steps)
            barrier()
            samples.append(time.perf_counter() - t0)
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, eng)
    # the same path over ONE long region (whole policy cycles per run graph): the short timed regions above carry ~100 us of fixed cost each
    # (graph launch, loss read-back), which a 20-step region does not amortise -- with --full both figures go into the line
    sustained = None
    if args.full and not use_dp and args.steps < 2000 and not args.child_trace:
        with torch.cuda.stream(stream):
            first = args.warmup + reps * args.steps
            run(first, 200)
            barrier()
            t0 = time.perf_counter()
            run(first + 200, 2000)
            barrier()
            el_s = time.perf_counter() - t0
        sustained = {"steps": 2000, "ms_per_step": el_s / 2000 * 1e3, "value": 2000 / el_s, "unit": "steps/s",
                     "note": "one 2000-step region after the timed regions (not `value`: the contract times exactly --steps steps)"}
    if use_dp:
        t = torch.tensor(samples, device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        samples = [float(x) for x in t.tolist()]
    elapsed = float(np.median(samples))
    losses = eng.losses()
    collective_ab = None
    if args.full and use_dp and world > 1 and not args.child_trace:
        # ---- ONE run decides between the collectives: per-collective latency at the two gradient sizes, and the
        # same data-parallel steps with the OTHER exchange (host-issued RCCL all-reduces between phase graphs), timed like the headline
        single = bool(os.environ.get("RECNN_BENCH_SINGLE_DEVICE"))
        n_ab = 6 if single else 200
        collective_ab = {"steps": n_ab, "latency_us": {}}
        with torch.cuda.stream(stream):
            gpu_backend = dist.get_backend() == "nccl"

            def rccl_all_reduce(t):
                if gpu_backend:
                    dist.all_reduce(t)
                else:                       # gloo stand-in on a 1-GPU box: through the host
                    h = t.cpu()
                    dist.all_reduce(h)
                    t.copy_(h)
            for n_fl in (429_312, 858_496):              # ~ one network's gradient arena; two (the communicator's capacity for DDPG)
                row = {}
                for name, fn in (("peer", comm.all_reduce if comm is not None else None), ("rccl", rccl_all_reduce)):
                    if fn is None:
                        continue
                    x = torch.randn((n_fl + 3) // 4 * 4, device=dev)
                    for _ in range(2):
                        fn(x)
                    barrier()
                    t0 = time.perf_counter()
                    for _ in range(3 if single else 20):
                        fn(x)
                    torch.cuda.synchronize(dev)
                    row[name] = round((time.perf_counter() - t0) / (3 if single else 20) * 1e6, 2)
                collective_ab["latency_us"][str(n_fl)] = row
            if comm is not None:
                comm.check()
                # the other exchange: detach the device communicator, step the same engine through the host-collective path
                eng.set_comm(None)
                dp_b = DataParallelStepper(eng, rows, always_reduce=args.force_dp, overlap=False)
                first = args.warmup + reps * args.steps
                dp_b.run(first, 2)
                barrier()
                t0 = time.perf_counter()
                dp_b.run(first + 2, n_ab)
                barrier()
                tb = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
                dist.all_reduce(tb, op=dist.ReduceOp.MAX)
                collective_ab["rccl"] = {"ms_per_step": float(tb[0]) / n_ab * 1e3, "rank_steps_per_s": world * n_ab / float(tb[0])}
                collective_ab["peer"] = {"ms_per_step": elapsed / args.steps * 1e3, "rank_steps_per_s": world * args.steps / elapsed,
                                         "note": f"the headline's {args.steps}-step regions"}
                collective_ab["faster"] = "peer" if collective_ab["peer"]["ms_per_step"] <= collective_ab["rccl"]["ms_per_step"] else "rccl"
                comm = None
            else:
                collective_ab["rccl"] = {"ms_per_step": elapsed / args.steps * 1e3, "rank_steps_per_s": world * args.steps / elapsed,
                                         "note": "the headline's regions (the peer collective was not available on every rank)"}
        collective_ab["note"] = ("latency: host-timed back-to-back collectives incl. launch overhead; rates: weak scaling, MAX over ranks"
                                 + ("; ranks share ONE GPU: functional only" if single else ""))
    if use_dp and comm is not None:
        # the per-launch profile below replays steps on rank 0 ONLY: with the communicator attached its collectives would wait
        # (4 s each, then report) for peers that are not stepping
        torch.cuda.synchronize(dev)
        comm.check()
        dist.barrier()
        eng.set_comm(None)
    assert os.environ.get("RECNN_MLP_PROBE") or all(np.isfinite(v) for v in losses.values()), losses

    if args.child_trace:
        if rank == 0:
            print(json.dumps({"child_trace": True, "ms_per_step": elapsed / args.steps * 1e3}), flush=True)
        return
    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        out = {
            "metric": "DDPG update steps/sec (batch 2048, frame 10, emb 128)" if (args.algo, rows) == ("ddpg", B_ROWS)
                      else f"{args.algo.upper()} update steps/sec (batch {rows}, frame 10, emb 128)",
            # weak scaling: every rank completes `steps` updates on its own `rows`-row batch -> N x steps batch-updates;
            # strong scaling: the ranks share ONE `args.rows`-row batch per step -> `steps` updates in total
            "value": (world if args.scaling == "weak" else 1) * args.steps / elapsed, "unit": "steps/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
            "repeats": reps, "ms_per_step_samples": [round(x / args.steps * 1e3, 6) for x in samples], "graph_setup": graph_setup,
            "spread": (max(samples) - min(samples)) / elapsed,     # (slowest - fastest region) / median region
            "sustained": sustained,
            "scaling": args.scaling,
            # synchronised optimizer updates per second (one per step whatever N is) and transition rows consumed per second
            "global_updates_per_s": args.steps / elapsed, "rows_per_s": world * rows * args.steps / elapsed,
            # N > 1: `value` counts RANK-steps (weak scaling: N ranks x steps / time -- what BASELINE's "steps/sec at 1/2/4/8 GPU" and
            # north_star's 50,000 target are read against, every rank-step being one 2048-row DDPG update's worth of work); the number
            # of SYNCHRONISED optimizer updates per second is global_updates_per_s
            "value_is": "rank-steps/s (n_gpus x steps / time)" if (world > 1 and args.scaling == "weak") else "optimizer updates/s",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": ("configs[1]: DDPG" if args.algo == "ddpg" else "configs[2]: TD3 (twin critics, delayed actor)")
                                   + f", {rows} transition rows/step/GPU ({args.scaling} scaling), frame_size 10, emb_dim 128, "
                                   "Actor/Critic hidden 256, Adam, policy+soft update every 10th step, synthetic ML20M-shaped "
                                   "replay store (138,493 users, 26,744 items, ~20M ratings), " + ("dense epochs: every window of every user once" if dense else "256 users per batch, first rows kept"),
                       "rows_per_step_per_gpu": rows, "parallelism": (f"dp{world}" if world > 1 else "single") + (f" ({collective} collective)" if use_dp else ""),
                       "final_losses": losses},
        }
        if use_dp:
            out["multi_gpu"] = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "collective": collective,
                                "collective_requested": args.collective,
                                "decision": ("in-graph two-shot all-reduce over hipIpc peer buffers (csrc/comm.hip): every rank mapped its peers and "
                                             "passed the self-test" if comm is not None else
                                             "host-issued all-reduces between phase graphs (torch.distributed backend above)"),
                                "ranks_share_one_gpu": bool(os.environ.get("RECNN_BENCH_SINGLE_DEVICE")),
                                "global_updates_per_s": args.steps / elapsed, "rank_steps_per_s": world * args.steps / elapsed,
                                "preflight": preflight, "collective_ab": collective_ab}
            if world > 1:
                out["config"]["workload"] += (f"; N = {world}: value = rank-steps/s (every rank steps on its own {rows}-row batch, one gradient "
                                              "all-reduce per optimizer step), global_updates_per_s = synchronised updates/s")
    if rank == 0 and args.full:
        # ---- per-launch times, measured live with HIP events around every launch (eager replays of the same steps on the stream
        # the kernels run on), and the rooflines they imply.  Two schedules exist and agree bit for bit (profiles/NOTES_r01_r05.md 5c):
        #   "fused": one row-panel launch for all networks of a step (csrc/mlps.hip) -- eager steps and run graphs shorter than
        #            the cycle-mode threshold (20 steps since round 5; 30 before, when the driver's `--steps 20` replayed THIS one);
        #   "cycle": a policy cycle's batches gathered at once, the frozen networks applied to all of them (csrc/mlpf.hip), the
        #            per-step launches carry the learning critics only (csrc/l1gemm.hip + csrc/mlpt.hip) -- run graphs >= 20 steps (the driver's command).
        peak = MFMA_PEAK_TFLOPS[args.dtype]
        pe = int(eng.policy_every)
        with torch.cuda.stream(stream):
            prof = eng.profile(rows, policy=False, n_steps=50)
            prof_pol = eng.profile(rows, policy=True, n_steps=10)
            try:
                prof_cyc = eng.profile(rows, policy=2, n_steps=20) if args.dtype == "bf16" else None
            except L.RecnnHipError:
                prof_cyc = None
        cyc_min = int(os.environ.get("RECNN_CYCLE_MIN_LEN", "20"))       # (the library default, include/recnn_hip.h)
        split_knob = int(os.environ.get("RECNN_SPLIT_FWD", "1"))
        # (data parallel with the device collective replays the same run graphs; the host-collective path steps phase graphs on
        # the fused forward)
        run_graphs = not use_dp or comm is not None
        schedule = "cycle" if (prof_cyc and run_graphs and split_knob >= 1 and (args.steps >= cyc_min or split_knob >= 2)) else "fused"

        def roof(name, ms, fl, per_step=1.0):
            ach = fl / (ms * 1e-3) / 1e12
            return {"kernel": name, "bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
                    "avg_ms": ms, "flops_per_launch": fl, "launches_per_step": per_step}
        FROZEN = FROZEN_SLOTS
        used = prof_cyc if schedule == "cycle" else prof
        cand = [r for r in used if r[2] > 0]
        # `roofline` = the kernel with the largest us per step in the schedule the timed region replayed (all its launches summed, as a
        # `rocprofv3 --stats` listing of this command ranks them); the launch with the largest share of the algorithmic flops is
        # reported beside it as `roofline_flop_dominant` (rounds 1-4 and 6: the time-dominant one is `roofline`; round 5 had them swapped)
        ktab = kernel_table(used, prof, prof_pol, pe, deferred=run_graphs)
        top = ktab[0]
        dom, _, flops_per_step, share = pick_dominant(used, pe)
        dom_k = KERNEL_OF_SLOT.get(dom[0], dom[0])
        # A child run of this very command under rocprofv3 (N = 1 only; two passes, one counter each): HBM bytes per launch from the PMC
        # counters, and -- from its kernel trace -- what every kernel of the REPLAYED schedule took inside the run graphs
        tr = None
        if world == 1 and not args.no_traffic and not use_dp:
            c_steps, c_reps = min(args.steps, 2000), (reps if args.steps <= 200 else 1)
            tail = ["--steps", str(c_steps), "--warmup", str(min(args.warmup, 200)), "--repeats", str(c_reps), "--child-trace", "--no-cpu-baseline",
                    "--no-traffic", "--no-extras", "--dtype", args.dtype, "--algo", args.algo, "--rows", str(args.rows)]
            tr = measure_traffic(tail)
            child_steps = min(args.warmup, 200) + c_reps * c_steps
        traffic_of = lambda k: tr.traffic(k) if tr else (None, "skipped")
        gather_traffic, gather_note = traffic_of("frame_gather_kernel")
        gather_multi_traffic = traffic_of("frame_gather_multi_kernel")[0]
        out["schedule"] = schedule
        # SURVEY.md 8(d)'s end-to-end figure: algorithmic MLP flops of a step / measured time per step / dense MFMA peak
        e2e = FLOP_PER_ROW[args.algo] * rows / (ms_per_step * 1e-3) / 1e12
        out["roofline_end_to_end"] = {"flops_per_step": FLOP_PER_ROW[args.algo] * rows, "tflops": e2e, "peak": peak, "frac": e2e / peak,
                                      "note": "north_star asks >= 0.40 MFMA utilisation; this is flops / wall time of the whole step"}
        # algorithmic HBM bytes per launch of the kernels that do no matrix work: optimizer 28 B / parameter, gather per row
        f32_rows = args.dtype == "fp32" or os.environ.get("RECNN_SAMPLER_F32") == "1"
        per_row = GATHER_BYTES_PER_ROW["fp32" if f32_rows else args.dtype]
        hbm_bytes = {"apply_kernel": 28.0 * PARAMS["critic"], "apply_gather_kernel": 28.0 * PARAMS["critic"] + per_row * rows,
                     "frame_gather_kernel": float(per_row * rows), "frame_gather_multi_kernel": float(per_row * rows * pe),
                     "grad_reduce_kernel": 8.0 * PARAMS["actor"]}
        # `roofline`: the kernel at the top of the replayed schedule's time ranking.  With the child trace: ranked by what the kernels took
        # INSIDE the run graphs (the `rocprofv3 --stats` order of this command); else by HIP events around eager launches of the same steps
        gtab = tr.table(child_steps) if tr and tr.calls else []
        if gtab:
            g_short, g_full, g_us, g_lps, g_avg = gtab[0]
            kt = next((t for t in ktab if t["kernel"] in g_full), None)
            g_total = sum(r[2] for r in gtab)
            src = (f"kernel trace of a child run of this command under rocprofv3 ({child_steps} replayed steps, counter pass): all launches of "
                   f"the kernel summed = {g_us:.2f} us/step of {g_total:.2f} us/step of kernel time")
            rec = {"kernel": g_short, "avg_ms": g_avg * 1e-3, "launches_per_step": g_lps, "us_per_step": g_us, "share_of_step_time": g_us / g_total,
                   "selected_by": src}
            t_traffic, t_note = tr.traffic(g_short)
            fl_step = kt["flops_per_step"] if kt else 0.0
            if fl_step > 0:
                ach = fl_step / (g_us * 1e-6) / 1e12
                rec.update(bound="mfma", achieved=ach, peak=peak, unit="TFLOP/s", frac=ach / peak, flops_per_launch=fl_step / g_lps, slots=kt["slots"],
                           eager={"avg_ms": kt["avg_ms"], "launches_per_step": kt["launches_per_step"]})
            else:
                nbytes = next((v for k, v in hbm_bytes.items() if k in g_full), None)
                gbs = nbytes / (g_avg * 1e-6) / 1e9 if nbytes else None
                rec.update(bound="hbm", achieved=gbs, peak=HBM_PEAK_GBS, unit="GB/s", frac=gbs / HBM_PEAK_GBS if gbs else None, bytes_per_launch=nbytes)
            rec.update(traffic=t_traffic, traffic_source=t_note)
            out["roofline"] = rec
            out["kernel_time_table_in_graph"] = [{"kernel": r[0], "us_per_step": round(r[2], 3), "launches_per_step": round(r[3], 3),
                                                  "avg_us": round(r[4], 3)} for r in gtab if r[2] > 0.05]
        else:
            sel = ("largest us per step of the replayed schedule, all launches of the kernel summed (HIP events around eager launches): %.2f "
                   "us/step = %.0f %% of the step's kernel time (%.2f launches per step)"
                   % (top["ms_per_step"] * 1e3, 100 * top["share_of_step_time"], top["launches_per_step"]))
            t_traffic, t_note = traffic_of(top["kernel"])
            if top["flops_per_launch"] > 0:
                ach = top["flops_per_launch"] / (top["avg_ms"] * 1e-3) / 1e12
                out["roofline"] = {"kernel": top["kernel"], "slots": top["slots"], "bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s",
                                   "frac": ach / peak, "avg_ms": top["avg_ms"], "flops_per_launch": top["flops_per_launch"],
                                   "launches_per_step": top["launches_per_step"], "share_of_step_time": top["share_of_step_time"],
                                   "traffic": t_traffic, "traffic_source": t_note, "selected_by": sel}
            else:
                nbytes = hbm_bytes.get(top["kernel"])
                gbs = nbytes / (top["avg_ms"] * 1e-3) / 1e9 if nbytes else None
                out["roofline"] = {"kernel": top["kernel"], "slots": top["slots"], "bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                   "frac": gbs / HBM_PEAK_GBS if gbs else None, "avg_ms": top["avg_ms"], "bytes_per_launch": nbytes,
                                   "launches_per_step": top["launches_per_step"], "share_of_step_time": top["share_of_step_time"],
                                   "traffic": t_traffic, "traffic_source": t_note, "selected_by": sel}
        out["kernel_time_table"] = [{"kernel": t["kernel"], "us_per_step": round(t["ms_per_step"] * 1e3, 3), "avg_us": round(t["avg_ms"] * 1e3, 3),
                                     "launches_per_step": round(t["launches_per_step"], 3), "gflop_per_launch": round(t["flops_per_launch"] / 1e9, 4),
                                     "share_of_step_time": round(t["share_of_step_time"], 4)} for t in ktab]
        if dom[2] > 0:
            traffic, traffic_note = traffic_of(dom_k)
            out["roofline_flop_dominant"] = dict(roof(dom[0], dom[1], dom[2], 1.0 / pe if dom[0] in FROZEN else 1.0), traffic=traffic,
                                   traffic_source=traffic_note,
                                   dominant_by="algorithmic flops per step: this launch %.0f %% of the schedule's MFMA flops in %.0f %% of its MFMA launch "
                                               "time" % (100 * flops_per_step(dom) / sum(flops_per_step(r) for r in cand),
                                                         100 * share(dom) / sum(share(r) for r in cand)))
            if dom[0] in ("frozen_actors", "frozen_target_critics"):
                out["roofline_flop_dominant"]["traffic_covers"] = "mean over the two launches of mlp_frozen_kernel per policy cycle (actors; target critics)"
        # every MFMA launch of both schedules (the per-step forward AND the cycle-batched frozen-network launch)
        out["roofline_kernels"] = {
            "fused": [roof(n, ms, fl) for n, ms, fl in prof if fl > 0],
            "cycle": [roof(n, ms, fl, 1.0 / pe if n in FROZEN else 1.0) for n, ms, fl in (prof_cyc or []) if fl > 0]}
        g = [r for r in prof if r[0] == "frame_gather"]
        if g:
            gbs = per_row * rows / (g[0][1] * 1e-3) / 1e9
            # the fraction is taken on MEASURED HBM bytes (PMC) when there are any: consecutive windows of a user share embedding
            # lines, so the algorithmic byte count (every line counted per use) over-states what the kernel has to move
            t_gbs = gather_traffic / (g[0][1] * 1e-3) / 1e9 if gather_traffic else None
            out["roofline_gather"] = {"kernel": "frame_gather", "bound": "hbm", "achieved": t_gbs if t_gbs else gbs, "peak": HBM_PEAK_GBS,
                                      "unit": "GB/s", "frac": (t_gbs if t_gbs else gbs) / HBM_PEAK_GBS,
                                      "basis": "PMC traffic" if t_gbs else "algorithmic bytes (no PMC data)",
                                      "algorithmic": {"bytes_per_launch": per_row * rows, "achieved": gbs, "frac": gbs / HBM_PEAK_GBS},
                                      "traffic": gather_traffic, "traffic_source": gather_note, "avg_ms": g[0][1],
                                      "bytes_per_launch": per_row * rows,
                                      "rows_dtype": "fp32+bf16" if (f32_rows and args.dtype == "bf16") else args.dtype}
            gc = [r for r in (prof_cyc or []) if r[0] == "frame_gather_cycle"]
            if gc:       # the cycle's batches in one launch: `pe` batches of `rows` rows
                gbs_c = per_row * rows * pe / (gc[0][1] * 1e-3) / 1e9
                t_c = gather_multi_traffic / (gc[0][1] * 1e-3) / 1e9 if gather_multi_traffic else None
                # (no frac on the algorithmic bytes: the windows of a batch share lines, the count exceeds what moves -- 1.07 "of peak")
                out["roofline_gather"]["cycle_launch"] = {"batches": pe, "avg_ms": gc[0][1], "traffic": gather_multi_traffic,
                                                          "achieved": t_c, "frac": t_c / HBM_PEAK_GBS if t_c else None,
                                                          "algorithmic": {"bytes_per_launch": per_row * rows * pe, "achieved": gbs_c}}
        gemm_fl = sum(r[2] for r in prof)
        gemm_ms = sum(r[1] for r in prof if r[2] > 0)
        out["step_breakdown"] = {"launches": [{"name": n, "ms": round(ms, 5), "gflop": round(fl / 1e9, 4)} for n, ms, fl in prof],
                                 "sum_kernel_ms": sum(r[1] for r in prof), "gemm_tflops": gemm_fl / (gemm_ms * 1e-3) / 1e12,
                                 "policy_step_sum_kernel_ms": sum(r[1] for r in prof_pol), "policy_step_launches": len(prof_pol)}
        if prof_cyc:
            out["step_breakdown"]["cycle_mode"] = {
                "launches": [{"name": n, "ms": round(ms, 5), "gflop": round(fl / 1e9, 4), "per_step": (round(1.0 / pe, 4) if n in FROZEN else 1)}
                             for n, ms, fl in prof_cyc],
                "sum_kernel_ms_per_step": sum(share(r) for r in prof_cyc)}
        if world == 1 and not use_dp and not args.no_extras and (args.algo, rows) == ("ddpg", B_ROWS):
            # ---- driver-timed sub-records: the 1e-4-parity compute type, BASELINE configs[2], and the loss-curve
            # deviation of both compute types from the CPU oracle measured in THIS run
            try:
                out["loss_curve_deviation"] = {args.dtype: loss_curve_deviation(recnn_amd, env, dev, args.dtype)}
                if args.dtype != "bf16x3":
                    pm = timed_subrun(recnn_amd, env, dev, stream, "ddpg", "bf16x3", B_ROWS, min(args.steps, 2000), min(args.warmup, 100), reps)
                    pm["loss_curve_deviation"] = loss_curve_deviation(recnn_amd, env, dev, "bf16x3")
                    pm["what"] = ("split-bf16 compute (hi + lo bf16 planes, 3 MFMAs per product, fp32 accumulate): the configuration that "
                                  "meets north_star's 1e-4 loss-curve parity, timed like the headline")
                    out["parity_mode"] = pm
                out["other_configs"] = {"configs[2]": timed_subrun(recnn_amd, env, dev, stream, "td3", args.dtype, 4096, min(args.steps, 60),
                                                                    min(args.warmup, 20), reps)}
                out["other_configs"]["configs[4] (1 GPU)"] = reinforce_subrun()
            except L.RecnnHipError as ex:
                out["extras_error"] = str(ex)
        if world == 1 and not args.no_cpu_baseline and (args.algo, rows) == ("ddpg", B_ROWS):
            out["cpu_baseline"] = cpu_baseline(items, ratings, off, table)
    if use_dp:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # RCCL prints a version banner through C stdio; flush it first so that the JSON line is the LAST line of stdout
        import ctypes
        sys.stdout.flush()
        ctypes.CDLL(None).fflush(None)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
