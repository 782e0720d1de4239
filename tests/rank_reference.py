"""float64 numpy restatement of scipy.spatial.distance.cdist (scipy 1.15) for the nine metrics of recnn_amd.retrieval, and
of the reference's `rank` (examples/streamlit_demo.py:207-231): every item's distance, sorted ascending, first k.

No scipy import: the GPU tests use this module.  Degenerate rows follow scipy: cosine against a zero row and correlation
against a constant row give NaN, braycurtis(0, 0) is NaN, a 0/0 canberra term counts 0.  `rank` orders by distance, NaN
after every number, ties to the smaller id (the stable `sorted` over item order of the reference).
"""
import numpy as np

METRICS = ("sqeuclidean", "euclidean", "cityblock", "chebyshev", "minkowski", "canberra", "braycurtis", "cosine", "correlation")


def _pairs(q, t, fn, chunk):
    """fn(q[:, None, :], t[None, c0:c1, :]) -> [B, c], over item chunks of at most `chunk` B * c * E elements."""
    B, N = q.shape[0], t.shape[0]
    out = np.empty((B, N), dtype=np.float64)
    step = max(1, chunk // max(1, B * q.shape[1]))
    for c0 in range(0, N, step):
        out[:, c0:c0 + step] = fn(q[:, None, :], t[None, c0:c0 + step, :])
    return out


def _cosine(q, t):
    # scipy's C kernel: dot / (|u| |v|), clipped to [-1, 1], then 1 - cos; a zero norm gives NaN
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (q @ t.T) / (np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(t, axis=1)[None, :])
    c = np.where(np.abs(c) > 1.0, np.sign(c), c)
    return 1.0 - c


def cdist(q, t, metric, p=None, chunk=1 << 24):
    """float64 [B, N] distance matrix of the rows of q [B, E] and t [N, E] (any float dtype)."""
    q = np.asarray(q, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    if metric == "minkowski":
        p = 2.0 if p is None else float(p)
        if p == np.inf:
            metric = "chebyshev"
        elif p == 1.0:
            metric = "cityblock"
    if metric == "sqeuclidean":
        return _pairs(q, t, lambda a, b: np.square(a - b).sum(-1), chunk)
    if metric == "euclidean":
        return np.sqrt(cdist(q, t, "sqeuclidean", chunk=chunk))
    if metric == "cityblock":
        return _pairs(q, t, lambda a, b: np.abs(a - b).sum(-1), chunk)
    if metric == "chebyshev":
        return _pairs(q, t, lambda a, b: np.abs(a - b).max(-1), chunk)
    if metric == "minkowski":
        return _pairs(q, t, lambda a, b: np.power(np.power(np.abs(a - b), p).sum(-1), 1.0 / p), chunk)
    if metric == "canberra":
        def canb(a, b):
            den = np.abs(a) + np.abs(b)
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.where(den > 0, np.abs(a - b) / den, 0.0).sum(-1)
        return _pairs(q, t, canb, chunk)
    if metric == "braycurtis":
        def bray(a, b):
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.abs(a - b).sum(-1) / np.abs(a + b).sum(-1)
        return _pairs(q, t, bray, chunk)
    if metric == "cosine":
        return _cosine(q, t)
    if metric == "correlation":
        return _cosine(q - q.mean(axis=1, keepdims=True), t - t.mean(axis=1, keepdims=True))
    raise ValueError(f"unknown metric {metric!r}")


def rank_matrix(d, k):
    """(dist [B, k], ids [B, k]) of a distance matrix: ascending, NaN last, ties to the smaller id."""
    ids = np.argsort(d, axis=1, kind="stable")[:, :k]       # numpy sorts NaN after every number; stable keeps id order
    return np.take_along_axis(d, ids, 1), ids


def rank(q, t, metric, k, p=None):
    return rank_matrix(cdist(q, t, metric, p), k)
