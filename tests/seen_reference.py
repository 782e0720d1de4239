"""numpy reference of the per-row exclusion (recnn_amd.retrieval: SeenItems, SeenMask, FlatIndex.search / rank_of with `exclude`).

A row's exclusion list is a sequence of ids: unordered, duplicates allowed, ids outside [0, N) ignored.
"""
import numpy as np

import ranking_eval_reference as R


def excluded_set(ids, N):
    """The distinct ids of a list that lie in [0, N)."""
    return sorted({int(i) for i in ids if 0 <= int(i) < N})


def mask_words(lists, N, keep=None):
    """uint64 [B, ceil(N / 64)]: bit (i & 63) of word (i >> 6) of row b set when i is in lists[b] (and is not keep[b]); the tail bits
    above N are zero."""
    B, W = len(lists), (N + 63) // 64
    bits = np.zeros((B, W * 64), dtype=np.uint8)
    for b, ids in enumerate(lists):
        bits[b, excluded_set(ids, N)] = 1
        if keep is not None and 0 <= int(keep[b]) < N:
            bits[b, int(keep[b])] = 0
    packed = np.packbits(bits, axis=1, bitorder="little")               # byte j holds items 8j .. 8j + 7, item 8j in bit 0
    return np.ascontiguousarray(packed).view("<u8").reshape(B, W)


def ranks_from_keys_excluding(keys, targets, lists, larger_is_better=False):
    """`ranking_eval_reference.ranks_from_keys` with the excluded columns of each row removed from `before`: the rank of the target
    among the items that are not excluded in its row.  The target's own membership is not consulted."""
    keys = np.asarray(keys)
    targets = np.asarray(targets, dtype=np.int64)
    B, N = keys.shape
    out = np.full(B, -1, dtype=np.int64)
    for b in range(B):
        g = int(targets[b])
        if not 0 <= g < N:
            continue
        cols = np.ones(N, dtype=bool)
        cols[excluded_set(lists[b], N)] = False
        cols[g] = True
        kept = np.flatnonzero(cols)                                     # ascending: id order, and so tie order, is preserved
        sub_target = int(np.searchsorted(kept, g))
        out[b] = R.ranks_from_keys(keys[b:b + 1, kept], [sub_target], larger_is_better)[0]
    return out


def filter_order(order_row, excluded, k):
    """The first k ids of a best-first order after the excluded ids are removed, padded with -1."""
    ex = {int(i) for i in excluded}
    left = [int(i) for i in order_row if int(i) not in ex][:k]
    return left + [-1] * (k - len(left))
