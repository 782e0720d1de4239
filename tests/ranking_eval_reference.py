"""numpy reference of the offline ranking evaluation (recnn_amd.retrieval: FlatIndex.rank_of, RankingMeter).

The order is the one `FlatIndex.search` uses: key ascending for the scipy metrics, descending for IP / L2 / COS' internal key; +0 and
-0 are one value, every NaN is one value after all numbers, ties go to the smaller id.
"""
import math

import numpy as np


def ranks_from_keys(keys, targets, larger_is_better=False):
    """int64 [B]: per row the number of items i != target that come before the target, from a [B, N] key or distance matrix;
    -1 for a target outside [0, N)."""
    keys = np.asarray(keys)
    targets = np.asarray(targets, dtype=np.int64)
    B, N = keys.shape
    out = np.full(B, -1, dtype=np.int64)
    ids = np.arange(N)
    for b in range(B):
        g = int(targets[b])
        if not 0 <= g < N:
            continue
        k, kg = keys[b], keys[b, g]
        nan, nan_g = np.isnan(k), bool(np.isnan(kg))
        if nan_g:
            strictly = ~nan
            equal = nan
        else:
            with np.errstate(invalid="ignore"):
                strictly = ~nan & ((k > kg) if larger_is_better else (k < kg))
                equal = ~nan & (k == kg)
        before = strictly | (equal & (ids < g))
        before[g] = False
        out[b] = int(before.sum())
    return out


def meter_reference(ranks, mask, ks):
    """What RankingMeter accumulates, in float64, integer fields as Python ints: {"hits": {K: int}, "ndcg_sum": {K: float},
    "mrr_sum", "rank_sum", "rows", "invalid"} and the derived "hit_rate", "ndcg", "mrr", "mean_rank" (None without rows)."""
    ranks = np.asarray(ranks, dtype=np.int64)
    keep = np.ones(len(ranks), dtype=bool) if mask is None else np.asarray(mask) != 0
    r = ranks[keep]
    invalid = int((r < 0).sum())
    r = r[r >= 0]
    rows = int(len(r))
    out = {"rows": rows, "invalid": invalid, "rank_sum": int(r.sum()),
           "mrr_sum": math.fsum(1.0 / (float(x) + 1.0) for x in r),
           "hits": {int(k): int((r < k).sum()) for k in ks},
           "ndcg_sum": {int(k): math.fsum(1.0 / math.log2(float(x) + 2.0) for x in r[r < k]) for k in ks}}
    if rows:
        out["hit_rate"] = {k: h / rows for k, h in out["hits"].items()}
        out["ndcg"] = {k: v / rows for k, v in out["ndcg_sum"].items()}
        out["mrr"] = out["mrr_sum"] / rows
        out["mean_rank"] = out["rank_sum"] / rows
    return out
