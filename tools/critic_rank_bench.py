#!/usr/bin/env python3
"""The catalogue ranked by the critic's value (csrc/qrank.hip, csrc/scoresel.hip): `CriticIndex.rank_of` and
`CriticIndex.search(k=10)` at N = 26,744 items (the ML-20M catalogue), S = 1290, H = 256, B = 2048 and B = 25 states, each timed
beside, on the same inputs in the same run:
  chunked_us      the route without the fused kernel: a loop of `Critic.candidates` over item chunks (the chunk's embeddings repeated
                  per state row, as that call wants them) into a [B, N] matrix, then torch comparisons for the rank
                  (`chunked_q_us` is the loop alone);
  flat_l2_us      `FlatIndex(L2).rank_of` on B actions, for scale: what ranking by geometry costs;
  q_values_us     the pair kernel alone (`CriticIndex.q_values`: layer 1 of the states, then one launch).
`peak_share` counts 2 B N H^2 flops of `q_values_us` against the 157 TFLOP/s fp32 matrix peak DESIGN.md section 20 uses.
Every figure is the median of 5 device-event windows of back-to-back calls after one warm-up call, in microseconds per call (the
method of tools/eval_bench.py).  `agree` is the share of rows on which the chunked route gives the same rank (its GEMMs round in
another order, so near-ties may swap).  Prints one JSON object and writes it to profiles/critic_rank_bench.json.
usage: python tools/critic_rank_bench.py [--quick] [--out profiles/critic_rank_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from eval_bench import device_us, rank_from_matrix  # noqa: E402

A, N, S, H = 128, 26744, 1290, 256
PEAK_FP32_MATRIX = 157e12
CHUNK_ROWS = 1 << 18           # candidate rows per `Critic.candidates` call of the chunked route (3 x 256 MiB of activations)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="B = 25 only, short windows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "critic_rank_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("critic_rank_bench.py measures on the GPU and none is visible")
    import recnn_amd
    from recnn_amd.retrieval import CriticIndex, FlatIndex
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    table = torch.randn(N, A, generator=gen).to(dev)
    critic = recnn_amd.nn.Critic(S, A, H).to(dev).eval()
    with torch.no_grad():
        critic.linear3.weight.mul_(1e4)
    index, flat = CriticIndex(critic, table), FlatIndex(table, "L2")
    window = 0.02 if a.quick else 0.05
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "critic_rank_bench", "n_items": N, "state_dim": S, "hidden": H, "device": torch.cuda.get_device_name(0),
           "arch": getattr(props, "gcnArchName", "unknown"), "window_s": window, "block_rows": index.block_rows, "cases": []}

    def chunked_q(state):
        B = state.shape[0]
        n = max(1, CHUNK_ROWS // B)
        q = torch.empty(B, N, device=dev)
        for c0 in range(0, N, n):
            c = min(n, N - c0)
            q[:, c0:c0 + c] = critic.candidates(state, table[c0:c0 + c].repeat(B, 1), c).view(B, c)
        return q

    for B in ((25,) if a.quick else (2048, 25)):
        state = torch.randn(B, S, generator=gen).to(dev)
        actions = (torch.randn(B, A, generator=gen) * 0.7).to(dev)
        targets = torch.randint(0, N, (B,), generator=gen).to(dev)
        rank_us, n_r = device_us(lambda: index.rank_of(state, targets), window)
        search_us, n_s = device_us(lambda: index.search(state, 10), window)
        q_us, n_q = device_us(lambda: index.q_values(state), window)
        chunk_q_us, n_cq = device_us(lambda: chunked_q(state), window)
        chunk_us, n_c = device_us(lambda: rank_from_matrix(chunked_q(state), targets, True), window)
        flat_us, n_f = device_us(lambda: flat.rank_of(actions, targets), window)
        agree = (index.rank_of(state, targets) == rank_from_matrix(chunked_q(state), targets, True)).float().mean().item()
        same = (index.rank_of(state, targets) == rank_from_matrix(index.q_values(state), targets, True)).all().item()
        assert same, "rank_of and the comparisons on q_values disagree"
        flops = 2.0 * B * N * H * H
        out["cases"].append({"B": B, "rank_of_us": round(rank_us, 1), "search_k10_us": round(search_us, 1),
                             "q_values_us": round(q_us, 1), "chunked_q_us": round(chunk_q_us, 1), "chunked_us": round(chunk_us, 1),
                             "flat_l2_us": round(flat_us, 1), "iters": [n_r, n_s, n_q, n_cq, n_c, n_f],
                             "chunked_over_rank_of": round(chunk_us / rank_us, 2), "rank_of_over_flat_l2": round(rank_us / flat_us, 1),
                             "pair_tflops": round(flops / q_us / 1e6, 1), "peak_share": round(flops / (q_us * 1e-6) / PEAK_FP32_MATRIX, 3),
                             "agree": round(agree, 5), "q_block_bytes": 4 * min(B, index.block_rows) * N})
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
