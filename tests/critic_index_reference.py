"""numpy reference of the catalogue ranked by the critic's value (recnn_amd.retrieval: CriticIndex, topk_of_scores, rank_in_scores).

    S1[b] = state[b] . W1[:, :S]^T + b1,   E1[n] = table[n] . W1[:, S:]^T,   Q[b, n] = w3 . relu(W2 . relu(S1[b] + E1[n]) + b2) + b3

in float64 (`q_values`) and in int64 for integer operands (`q_values_int`, with the largest absolute partial sum any evaluation order
can meet).  The order of a score row: larger score first, -0 == +0, every NaN after all numbers, ties (NaN among NaN too) to the smaller
id; excluded items do not exist for their row; short rows are padded with id -1 at -inf.  `topk` sorts, `ranks` counts with plain
comparisons: two statements of the same order, checked against each other and against a pairwise comparator in the CPU tests.
"""
import numpy as np


def _chunks(n, step):
    return [(c, min(n, c + step)) for c in range(0, n, step)]


def _forward(state, table, w1, b1, w2, b2, w3, b3, dtype, chunk=256):
    state, table = np.asarray(state, dtype=dtype), np.asarray(table, dtype=dtype)
    w1, b1, w2, b2 = (np.asarray(x, dtype=dtype) for x in (w1, b1, w2, b2))
    w3, b3 = np.asarray(w3, dtype=dtype).reshape(-1), np.asarray(b3, dtype=dtype).reshape(())
    S = state.shape[1]
    s1 = state @ w1[:, :S].T + b1
    e1 = table @ w1[:, S:].T
    out = np.empty((state.shape[0], table.shape[0]), dtype=dtype)
    for c0, c1 in _chunks(table.shape[0], chunk):
        h1 = np.maximum(s1[:, None, :] + e1[None, c0:c1, :], 0)
        h2 = np.maximum(h1 @ w2.T + b2, 0)
        out[:, c0:c1] = h2 @ w3 + b3
    return out


def q_values(state, table, w1, b1, w2, b2, w3, b3):
    """float64 [B, N]."""
    return _forward(state, table, w1, b1, w2, b2, w3, b3, np.float64)


def q_values_int(state, table, w1, b1, w2, b2, w3, b3):
    """(int64 [B, N], bound): the exact values for integer operands, and the largest sum of absolute values of the terms of any
    partial sum of the three layers (every intermediate of every evaluation order is at most this in magnitude).  The integers are
    carried in float64, where sums below 2^53 are exact in any order (asserted on the bound); the result is returned as int64."""
    args = [np.asarray(x) for x in (state, table, w1, b1, w2, b2, w3, b3)]
    assert all(np.array_equal(x, np.rint(x)) for x in args), "integer operands only"
    a = [np.abs(x).astype(np.float64) for x in args]
    S = a[0].shape[1]
    s1, e1 = a[0] @ a[2][:, :S].T + a[3], a[1] @ a[2][:, S:].T
    bound = 0.0
    for c0, c1 in _chunks(e1.shape[0], 256):
        l1 = s1[:, None, :] + e1[None, c0:c1, :]                                  # >= |h1| and every partial sum of layer 1
        l2 = l1 @ a[4].T + a[5]                                                    # >= |h2| ...
        l3 = l2 @ a[6].reshape(-1) + a[7].reshape(())
        bound = max(bound, l1.max(), l2.max(), l3.max())
    assert bound < 2.0 ** 53
    q = _forward(*args, np.float64)
    return np.rint(q).astype(np.int64), int(bound)


def _gone(excluded, b, N):
    gone = np.zeros(N, dtype=bool)
    if excluded is not None:
        ids = np.asarray([i for i in excluded[b] if 0 <= i < N], dtype=np.int64)
        gone[ids] = True
    return gone


def order(row, gone=None):
    """The ids of one score row, best first, without the excluded ones."""
    row = np.asarray(row, dtype=np.float64)
    N = row.shape[0]
    nan = np.isnan(row)
    neg = np.where(nan, 0.0, -row) + 0.0                    # (-0.0) + 0.0 == +0.0: one zero
    ids = np.lexsort((np.arange(N), neg, nan))              # last key first: NaN last, score descending, id ascending
    return ids if gone is None else ids[~gone[ids]]


def topk(scores, k, excluded=None):
    """(values float64 [B, k], ids int64 [B, k]); `excluded`: one list of ids per row (ids outside [0, N) are ignored)."""
    scores = np.asarray(scores)
    B, N = scores.shape
    vals = np.full((B, k), -np.inf, dtype=np.float64)
    ids = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        o = order(scores[b], _gone(excluded, b, N))[:k]
        ids[b, :len(o)] = o
        vals[b, :len(o)] = scores[b, o]
    return vals, ids


def ranks(scores, targets, excluded=None):
    """int64 [B]: items other than the target, not excluded, that come before it; -1 for a target outside [0, N).  The target's own
    exclusion is not consulted."""
    scores = np.asarray(scores)
    targets = np.asarray(targets, dtype=np.int64)
    B, N = scores.shape
    out = np.full(B, -1, dtype=np.int64)
    idx = np.arange(N)
    for b in range(B):
        g = int(targets[b])
        if not 0 <= g < N:
            continue
        row = scores[b].astype(np.float64)
        nan = np.isnan(row)
        if nan[g]:
            before = ~nan | (idx < g)
        else:
            with np.errstate(invalid="ignore"):
                before = ~nan & ((row > row[g]) | ((row == row[g]) & (idx < g)))
        before &= ~_gone(excluded, b, N)
        before[g] = False
        out[b] = int(before.sum())
    return out
