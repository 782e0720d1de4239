"""Times one learn step of the embeddings notebook's dueling DQN (`dqn_update`) against the notebook's eager-torch step
on the same GPU, after warm-up, with device events.

  python tools/dqn_bench.py                 # B in {256, 2048} x N in {26,744, 100,000}, fp32 and bf16
  python tools/dqn_bench.py --quick         # B = 2048, N = 26,744, fp32 only (for a kernel trace:
                                            #   rocprofv3 --kernel-trace --stats -d <dir> -- python tools/dqn_bench.py --quick)

Floors: the target head's catalogue GEMM (2 B 128 N flop) at the MFMA peak (fp32 157.3 TF/s, bf16 2.5 PF/s dense), and the two RAdam
passes (28 B per parameter: p, g, m, v read, p, m, v written) at 6.3 TB/s.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, E, H = 10, 128, 128
PEAK = {"fp32": 157.3e12, "bf16": 2.5e15}
HBM = 6.3e12


class EagerDuelDQN(nn.Module):
    def __init__(self, input_dim, action_dim):
        super().__init__()
        self.feature = nn.Sequential(nn.Linear(input_dim, H), nn.ReLU())
        self.advantage = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, action_dim))
        self.value = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 1))

    def forward(self, x):
        x = self.feature(x)
        a = self.advantage(x)
        return self.value(x) + a - a.mean()


def make_batch(B, N, dev, seed):
    g = torch.Generator().manual_seed(seed)
    it = (torch.rand(B, F + 1, generator=g) ** 3 * N).long().clamp_(max=N - 1)      # skewed popularity
    r = torch.randn(B, F + 1, generator=g)
    done = (torch.rand(B, generator=g) < 0.05).float()
    b = [it[:, :-1], it[:, 1:], r[:, :-1], r[:, 1:], it[:, -1], r[:, -1], done]
    return [t.to(dev) for t in b]


def eager_step(batch, dqn, target, emb, vo, eo, gamma=0.99):
    items, next_items, ratings, next_ratings, action, reward, done = batch
    B = items.size(0)
    state = torch.cat([emb(items).view(B, -1), ratings], 1)
    next_state = torch.cat([emb(next_items).view(B, -1), next_ratings], 1)
    q_values = dqn(state)
    with torch.no_grad():
        next_q_values = target(next_state)
    q = q_values.gather(1, action.unsqueeze(1)).squeeze(1)
    y = reward + gamma * next_q_values.max(1)[0] * (1 - done)
    loss = (q - y).pow(2).mean()
    eo.zero_grad()
    vo.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(dqn.parameters(), -1, 1)
    eo.step()
    vo.step()
    return loss.item()


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def run(B, N, dtype, steps, warmup, eager=True):
    from recnn_amd.nn import DuelDQN, functional as Fh
    from recnn_amd.nn.update import dqn_update
    from recnn_amd.optim import RAdam
    dev = torch.device("cuda")
    torch.manual_seed(0)
    dqn, target = DuelDQN(F * (E + 1), N).to(dev), DuelDQN(F * (E + 1), N).to(dev)
    target.load_state_dict(dqn.state_dict())
    emb = nn.Embedding(N, E).to(dev)
    nets = {"dqn": dqn, "target_dqn": target, "embeddings": emb}
    opts = {"value_optimizer": RAdam(dqn.parameters(), lr=1e-5), "embeddings_optimizer": RAdam(emb.parameters(), lr=1e-5)}
    batch = make_batch(B, N, dev, 1)
    Fh.set_catalogue_dtype(dtype)
    try:
        ours = timed(lambda: dqn_update(batch, {"gamma": 0.99}, nets, opts), steps, warmup)
    finally:
        Fh.set_catalogue_dtype("fp32")
    n_params = sum(p.numel() for p in dqn.parameters()) + emb.weight.numel()
    gemm_floor = 2 * B * H * N / PEAK[dtype] * 1e6
    radam_floor = 28 * n_params / HBM * 1e6
    rec = {"B": B, "N": N, "dtype": dtype, "step_us": round(ours, 1), "target_gemm_floor_us": round(gemm_floor, 1),
           "radam_floor_us": round(radam_floor, 1), "floor_us": round(gemm_floor + radam_floor, 1), "params": n_params}
    if eager:
        edqn, etgt = EagerDuelDQN(F * (E + 1), N).to(dev), EagerDuelDQN(F * (E + 1), N).to(dev)
        edqn.load_state_dict(dqn.state_dict())
        etgt.load_state_dict(dqn.state_dict())
        eemb = nn.Embedding(N, E).to(dev)
        vo, eo = torch.optim.RAdam(edqn.parameters(), lr=1e-5), torch.optim.RAdam(eemb.parameters(), lr=1e-5)
        rec["eager_us"] = round(timed(lambda: eager_step(batch, edqn, etgt, eemb, vo, eo), steps, warmup), 1)
        rec["speedup"] = round(rec["eager_us"] / ours, 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the records to this JSON file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dqn_bench needs a GPU"
    from recnn_amd import _lib
    _lib.load()
    shapes = [(2048, 26744, "fp32")] if a.quick else [(B, N, d) for d in ("fp32", "bf16") for B in (256, 2048) for N in (26744, 100000)]
    recs = []
    for B, N, d in shapes:
        r = run(B, N, d, a.steps, a.warmup)
        recs.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
