#!/usr/bin/env python3
"""Two-stage recommendation (csrc/qcand.hip): `TwoStageIndex.search(action, state, k=10)` with 64 candidates at
N = 26,744 items (the ML-20M catalogue), S = 1290, H = 256, B = 2048 states, timed beside, on the same inputs in the same run:
  flat_search_us   the first stage alone: `FlatIndex(L2).search(action, 64)`;
  rerank_us        the second stage alone: `CriticIndex.rerank(state, candidates, 10)` (layer 1 of the states, then one launch);
  q_of_us          the same without the sort: `CriticIndex.q_of(state, candidates)`;
  eager_us         the route without the kernel, on the same candidates: `table[ids]` gather, `Critic.candidates(state, actions, 64)`,
                   `torch.sort` (`eager_q_us` is the gather and `Critic.candidates` alone);
  critic_search_us the whole catalogue by value: `CriticIndex.search(state, 10)`, the offline yardstick.
`pair_tflops` counts 2 B 64 H^2 flops of `q_of_us` (which contains layer 1 of the states) and `peak_share` sets it against the
157 TFLOP/s fp32 matrix peak.  Every figure is the median of 5 device-event windows of back-to-back calls after one warm-up call, in
microseconds per call from Python, allocations included (the method of tools/eval_bench.py).  `top1_agree` is the share of rows on
which the eager route picks the same best candidate (its GEMMs round in another order, so near-ties may swap); `overlap10` the mean
share of the whole-catalogue top 10 that the two-stage top 10 contains (random weights: a property of the inputs, not of the code).
Prints one JSON object and writes it to profiles/two_stage_bench.json.
usage: python tools/two_stage_bench.py [--quick] [--out profiles/two_stage_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from eval_bench import device_us  # noqa: E402

A, N, S, H = 128, 26744, 1290, 256
N_CAND, TOP = 64, 10
PEAK_FP32_MATRIX = 157e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="B = 25 only, short windows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_stage_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("two_stage_bench.py measures on the GPU and none is visible")
    import recnn_amd
    from recnn_amd.retrieval import CriticIndex, FlatIndex, TwoStageIndex
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    table = torch.randn(N, A, generator=gen).to(dev)
    critic = recnn_amd.nn.Critic(S, A, H).to(dev).eval()
    with torch.no_grad():
        critic.linear3.weight.mul_(1e4)
    index, flat = CriticIndex(critic, table), FlatIndex(table, "L2")
    two = TwoStageIndex(flat, index, N_CAND)
    window = 0.02 if a.quick else 0.05
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "two_stage_bench", "n_items": N, "state_dim": S, "hidden": H, "n_candidates": N_CAND, "k": TOP,
           "device": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", "unknown"), "window_s": window, "cases": []}

    def eager_q(state, cand):
        actions = table[cand.reshape(-1)]
        return critic.candidates(state, actions, N_CAND).view(-1, N_CAND)

    for B in ((25,) if a.quick else (2048, 25)):
        state = torch.randn(B, S, generator=gen).to(dev)
        action = (torch.randn(B, A, generator=gen) * 0.7).to(dev)
        cand = flat.search(action, N_CAND)[1]
        assert (cand >= 0).all()
        two_us, n_t = device_us(lambda: two.search(action, state, TOP), window)
        flat_us, n_f = device_us(lambda: flat.search(action, N_CAND), window)
        rerank_us, n_r = device_us(lambda: index.rerank(state, cand, TOP), window)
        q_of_us, n_q = device_us(lambda: index.q_of(state, cand), window)
        eager_q_us, n_eq = device_us(lambda: eager_q(state, cand), window)
        eager_us, n_e = device_us(lambda: torch.sort(eager_q(state, cand), 1, descending=True), window)
        critic_us, n_c = device_us(lambda: index.search(state, TOP), window)
        q, ids = two.search(action, state, TOP)
        rows = min(B, 64)                                  # the bits of the whole-catalogue kernel, on as many rows as is cheap
        same = torch.equal(index.q_of(state[:rows], cand[:rows]).view(torch.int32),
                           index.q_values(state[:rows]).gather(1, cand[:rows]).view(torch.int32))
        assert same, "q_of and q_values disagree"
        eq, eo = torch.sort(eager_q(state, cand), 1, descending=True)
        agree = (cand.gather(1, eo[:, :1])[:, 0] == ids[:, 0]).float().mean().item()
        top = index.search(state, TOP)[1]
        overlap = (ids[:, :, None] == top[:, None, :]).any(2).float().mean().item()
        flops = 2.0 * B * N_CAND * H * H
        out["cases"].append({"B": B, "two_stage_search_us": round(two_us, 1), "flat_search_us": round(flat_us, 1),
                             "rerank_us": round(rerank_us, 1), "q_of_us": round(q_of_us, 1), "eager_q_us": round(eager_q_us, 1),
                             "eager_us": round(eager_us, 1), "critic_search_us": round(critic_us, 1),
                             "iters": [n_t, n_f, n_r, n_q, n_eq, n_e, n_c], "eager_over_rerank": round(eager_us / rerank_us, 2),
                             "critic_search_over_two_stage": round(critic_us / two_us, 1),
                             "pair_tflops": round(flops / q_of_us / 1e6, 2),
                             "peak_share": round(flops / (q_of_us * 1e-6) / PEAK_FP32_MATRIX, 4),
                             "top1_agree": round(agree, 5), "overlap10": round(overlap, 4)})
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
