"""float64 numpy restatement of recnn_amd.retrieval.topk_stats (csrc/divstats.hip), written from its formulas: per-item counts of a
[B, k] id matrix and the per-row mean and population standard deviation of the [B, k] distances (their square roots when asked).
`gamma(k)` is the summation constant k u / (1 - k u), u = 2^-53, of the tests' derived bounds."""
import numpy as np

U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


def topk_stats(dist, ids, n_items, sqrt=False):
    """(counts int64 [n_items], row_mean float64 [B], row_std float64 [B], x float64 [B, k])"""
    x = np.asarray(dist, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        x = np.sqrt(x) if sqrt else x
        return np.bincount(np.asarray(ids).ravel(), minlength=n_items), x.mean(axis=1), x.std(axis=1), x
