"""numpy reference of the two-stage recommendation (recnn_amd.retrieval: CriticIndex.q_of / rerank, TwoStageIndex): the critic's
value over per-row candidate lists, the list sorted by it, the position of a target in it and the two-stage rank.

A slot of a list is (score, id, slot index); a slot whose id is outside [0, N) is empty.  Order of a row: larger score first,
-0 == +0, ties to the smaller id, equal ids to the smaller slot, every NaN after all numbers in (id, slot) order, empty slots last
in slot order, reported as id -1 at -inf.  The values come from tests/critic_index_reference.py: `q_of` looks the listed ids up in
its whole-catalogue matrix."""
import numpy as np

import critic_index_reference as R


def q_of(q_matrix, ids):
    """float64 [B, K]: `q_matrix[b, ids[b, j]]`, -inf for an id outside [0, N)."""
    q_matrix, ids = np.asarray(q_matrix), np.asarray(ids, dtype=np.int64)
    N = q_matrix.shape[1]
    ok = (ids >= 0) & (ids < N)
    out = np.take_along_axis(q_matrix.astype(np.float64), np.where(ok, ids, 0), axis=1)
    return np.where(ok, out, -np.inf)


def q_of_int(state, table, params, ids):
    """`q_of` over the exact integer values of `critic_index_reference.q_values_int`."""
    q, _ = R.q_values_int(state, table, *params)
    return q_of(q, ids)


def slot_order(q_row, id_row, N):
    """The slot indices of one row in the stated order (all of them: the empty slots are the tail)."""
    q_row = np.asarray(q_row, dtype=np.float64)
    id_row = np.asarray(id_row, dtype=np.int64)
    K = q_row.shape[0]
    empty = (id_row < 0) | (id_row >= N)
    nan = np.isnan(q_row) & ~empty
    cls = np.where(empty, 2, np.where(nan, 1, 0))
    neg = np.where(cls == 0, -q_row, 0.0) + 0.0                  # (-0.0) + 0.0 == +0.0: one zero; NaN and empty slots carry no score
    key_id = np.where(empty, 0, id_row)                          # empty slots order by slot alone
    return np.lexsort((np.arange(K), key_id, neg, cls))          # last key first


def rerank(q, ids, N, k=None):
    """(values float64 [B, k], ids int64 [B, k]): the first k slots of every row in the stated order; empty slots as -1 at -inf."""
    q, ids = np.asarray(q), np.asarray(ids, dtype=np.int64)
    B, K = ids.shape
    k = K if k is None else k
    vals = np.full((B, k), -np.inf, dtype=np.float64)
    out = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        o = slot_order(q[b], ids[b], N)[:k]
        full = (ids[b, o] >= 0) & (ids[b, o] < N)
        out[b, :len(o)] = np.where(full, ids[b, o], -1)
        vals[b, :len(o)] = np.where(full, q[b, o].astype(np.float64), -np.inf)
    return vals, out


def pos(q, ids, N, targets):
    """int64 [B]: the number of non-empty slots before the first slot (in the stated order) that holds `targets[b]`; -1 if no slot
    holds it or it is outside [0, N)."""
    q, ids = np.asarray(q), np.asarray(ids, dtype=np.int64)
    targets = np.asarray(targets, dtype=np.int64)
    out = np.full(ids.shape[0], -1, dtype=np.int64)
    for b in range(ids.shape[0]):
        g = int(targets[b])
        if not 0 <= g < N:
            continue
        o = slot_order(q[b], ids[b], N)
        hit = np.nonzero(ids[b, o] == g)[0]
        if len(hit):
            out[b] = int(hit[0])                                  # every slot before a non-empty one is non-empty
    return out


def two_stage_rank(position, flat_rank, filled):
    """int64 [B]: `position` where it is >= 0, else max(flat_rank, filled); -1 where flat_rank is -1 (a target outside [0, N))."""
    position, flat_rank, filled = (np.asarray(x, dtype=np.int64) for x in (position, flat_rank, filled))
    return np.where(position >= 0, position, np.where(flat_rank < 0, -1, np.maximum(flat_rank, filled)))
