#!/usr/bin/env python3
"""Slate diversification (csrc/slate.hip): `SlateDiversifier(table, "COS")` over K = 64 candidates per row,
k = 10 picks, N = 26,744 items (the ML-20M catalogue), B = 2048 and 25 rows, timed beside, on the same inputs in the same run:
  rerank_us          `rerank(q, ids, 10, lam=0.5, normalize=True)`: gather, Gram matrix, similarity and the ten greedy picks, one launch;
  similarity_us      `similarity(ids)`: the same up to S, written out as [B, 64, 64];
  ild_us / ild10_us  `ild(ids)` over the 64 candidates / over a slate of 10;
  torch_us           the route without the kernel: `table[ids]`, `torch.bmm`, the cosine scaling, then k rounds of torch ops that
                     implement the same rule (`torch_sim_us`: up to S alone).  Its ties go to the smaller slot, not the smaller id,
                     and its sums round in another order; `torch_agree` is the share of rows on which it picks the same ten slots;
  two_stage_us       `TwoStageIndex.search(action, state, 10)` as it was, and `two_stage_div_us` the same with `diversify=0.5`.
The candidates are the 64 items nearest to an action and the relevance is the critic's value of them, as in `TwoStageIndex.search`.
The table is clustered (groups of 16 items around a common centre, as near-duplicates in a catalogue are), so that the nearest
candidates are alike and a diversifying rerank has something to do.  `quality` reports, for lam = 0.3 / 0.5 / 0.7, the mean
intra-list cosine distance of the ten most valuable candidates (`ild_before`) and of the ten picked (`ild_after`), and the mean
relevance given up: the drop of the slate's mean min-max-normalised value.
`gather_gbs` sets the 32 KiB a row gathers against `rerank_us`.  Every time is the median of 5 device-event windows of back-to-back
calls after one warm-up call, in microseconds per call from Python, allocations included (the method of tools/eval_bench.py).
Prints one JSON object and writes it to profiles/slate_bench.json.
usage: python tools/slate_bench.py [--quick] [--out profiles/slate_bench.json]"""
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
K, TOP = 64, 10
GROUP = 16


def torch_similarity(table, ids):
    """Cosine S [B, K, K] by gather, bmm and scaling; entries of empty slots and of zero rows are 0."""
    ok = (ids >= 0) & (ids < table.shape[0])
    X = table[ids.clamp(0, table.shape[0] - 1)] * ok[:, :, None]
    G = torch.bmm(X, X.transpose(1, 2))
    root = torch.diagonal(G, dim1=1, dim2=2).sqrt()
    den = root[:, :, None] * root[:, None, :]
    return torch.where(den > 0, G / den, torch.zeros_like(G)), ok


def torch_rerank(table, rel, ids, k, lam):
    """The rule of `SlateDiversifier.rerank(normalize=True)` in k rounds of torch ops: (ids [B, k], slots [B, k])."""
    sim, ok = torch_similarity(table, ids)
    fin = ok & torch.isfinite(rel)
    mn = torch.where(fin, rel, torch.full_like(rel, float("inf"))).min(1, keepdim=True)[0]
    mx = torch.where(fin, rel, torch.full_like(rel, float("-inf"))).max(1, keepdim=True)[0]
    r = torch.where(fin, torch.where(mx > mn, (rel - mn) / (mx - mn), torch.zeros_like(rel)), rel)
    lam32 = torch.tensor(lam, dtype=torch.float32).item()
    lr, mu = lam32 * r, 1.0 - lam32
    left, m, slots = ok.clone(), None, []
    for _ in range(k):
        score = lr if m is None else lr - mu * m
        s = torch.where(left & ~torch.isnan(score), score, torch.full_like(score, float("-inf"))).argmax(1, keepdim=True)
        slots.append(s)
        left.scatter_(1, s, False)
        row = sim.gather(1, s[:, :, None].expand(-1, 1, sim.shape[2]))[:, 0]
        m = row if m is None else torch.maximum(m, row)
    slots = torch.cat(slots, 1)
    return ids.gather(1, slots), slots


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="B = 25 only, short windows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slate_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("slate_bench.py measures on the GPU and none is visible")
    import recnn_amd
    from recnn_amd.retrieval import CriticIndex, FlatIndex, SlateDiversifier, TwoStageIndex
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    centres = torch.randn((N + GROUP - 1) // GROUP, A, generator=gen)
    table = (centres.repeat_interleave(GROUP, 0)[:N] + 0.35 * torch.randn(N, A, generator=gen))[torch.randperm(N, generator=gen)].to(dev)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)                                           # the same critic, so the same slates, in every run
        critic = recnn_amd.nn.Critic(S, A, H).to(dev).eval()
    with torch.no_grad():
        critic.linear3.weight.mul_(1e4)
    index, flat = CriticIndex(critic, table), FlatIndex(table, "L2")
    two = TwoStageIndex(flat, index, K)
    div = SlateDiversifier(table, "COS")
    window = 0.02 if a.quick else 0.05
    props = torch.cuda.get_device_properties(0)
    out = {"tool": "slate_bench", "n_items": N, "state_dim": S, "hidden": H, "n_candidates": K, "k": TOP, "similarity": "COS",
           "group": GROUP, "device": torch.cuda.get_device_name(0), "arch": getattr(props, "gcnArchName", "unknown"),
           "window_s": window, "cases": []}

    for B in ((25,) if a.quick else (2048, 25)):
        state = torch.randn(B, S, generator=gen).to(dev)
        pick = torch.randint(0, N, (B,), generator=gen).to(dev)
        action = table[pick] + 0.2 * torch.randn(B, A, generator=gen).to(dev)
        cand = flat.search(action, K)[1]
        assert (cand >= 0).all()
        q, ids = index.rerank(state, cand)                             # the candidates by value, as TwoStageIndex hands them on
        top10 = ids[:, :TOP].contiguous()
        rerank_us, n_r = device_us(lambda: div.rerank(q, ids, TOP, 0.5, True), window)
        sim_us, n_s = device_us(lambda: div.similarity(ids), window)
        ild_us, n_i = device_us(lambda: div.ild(ids), window)
        ild10_us, n_i10 = device_us(lambda: div.ild(top10), window)
        torch_us, n_t = device_us(lambda: torch_rerank(table, q, ids, TOP, 0.5), window)
        torch_sim_us, n_ts = device_us(lambda: torch_similarity(table, ids), window)
        two_us, n_2 = device_us(lambda: two.search(action, state, TOP), window)
        two_div_us, n_2d = device_us(lambda: two.search(action, state, TOP, diversify=0.5), window)
        _, got, slots = div.rerank(q, ids, TOP, 0.5, True)
        t_ids, t_slots = torch_rerank(table, q, ids, TOP, 0.5)
        agree = (slots.long() == t_slots).all(1).float().mean().item()
        sim_err = (div.similarity(ids) - torch_similarity(table, ids)[0]).abs().max().item()
        qn = (q - q.min(1, keepdim=True)[0]) / (q.max(1, keepdim=True)[0] - q.min(1, keepdim=True)[0])
        quality = []
        for lam in (0.3, 0.5, 0.7):
            _, chosen, sl = div.rerank(q, ids, TOP, lam, True)
            quality.append({"lam": lam, "ild_before": round(div.ild(top10).mean().item(), 4),
                            "ild_after": round(div.ild(chosen).mean().item(), 4),
                            "relevance_given_up": round((qn[:, :TOP].mean(1) - qn.gather(1, sl.long()).mean(1)).mean().item(), 4)})
        out["cases"].append({"B": B, "rerank_us": round(rerank_us, 1), "similarity_us": round(sim_us, 1), "ild_us": round(ild_us, 1),
                             "ild10_us": round(ild10_us, 1), "torch_us": round(torch_us, 1), "torch_sim_us": round(torch_sim_us, 1),
                             "two_stage_us": round(two_us, 1), "two_stage_div_us": round(two_div_us, 1),
                             "iters": [n_r, n_s, n_i, n_i10, n_t, n_ts, n_2, n_2d],
                             "torch_over_rerank": round(torch_us / rerank_us, 2),
                             "torch_sim_over_similarity": round(torch_sim_us / sim_us, 2),
                             "gather_gbs": round(B * K * A * 4 / rerank_us / 1e3, 1),
                             "torch_agree": round(agree, 5), "similarity_max_abs_diff_vs_torch": sim_err, "quality": quality})
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
