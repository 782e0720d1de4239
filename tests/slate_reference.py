"""numpy reference of the slate diversifier (recnn_amd.retrieval.SlateDiversifier, csrc/slate.hip), generic
over the dtype the arithmetic runs in (np.float32: the kernel's own operations, one correctly rounded operation each; np.float64:
the yardstick).

A row is a list of K slots (id, relevance); a slot whose id is outside [0, N) is empty.  With G = X X^T over the gathered table rows
and n_i = G_ii:  IP  S_ij = G_ij;  COS  S_ij = G_ij / (sqrt(n_i) sqrt(n_j)), 0 where a norm is 0;  L2  S_ij = -max((n_i + n_j) - 2
G_ij, 0).  Entries of an empty slot are 0.  (numpy's float32 matrix product sums in its own order, so the float32 `similarity` has
the kernel's bits on exactly representable data only; the selection and `ild` are stated over a given S.)

Selection: lam32 = float32(lam), mu32 = float32(1) - lam32; step 1 scores slot j as lam32 * r_j, step t > 1 as (lam32 * r_j) -
(mu32 * m_j) with m_j the largest S_js over the chosen s (the first chosen s sets it; a later one replaces it where S_js > m_j); the
slot chosen is the first not-yet-chosen slot of `two_stage_reference.slot_order` over (score, id, slot)."""
import math

import numpy as np

import two_stage_reference as T

KINDS = ("IP", "COS", "L2")


def _empty(ids, N):
    ids = np.asarray(ids, dtype=np.int64)
    return (ids < 0) | (ids >= N)


def gather(table, ids, dtype=np.float64):
    """[B, K, E]: the table rows of the slots in `dtype`, zeros for the empty ones."""
    table, ids = np.asarray(table), np.asarray(ids, dtype=np.int64)
    empty = _empty(ids, table.shape[0])
    X = table[np.where(empty, 0, ids)].astype(dtype)
    X[empty] = 0
    return X


def similarity(table, ids, kind, dtype=np.float64):
    """`dtype` [B, K, K]."""
    assert kind in KINDS
    X = gather(table, ids, dtype)
    empty = _empty(ids, np.asarray(table).shape[0])
    G = np.matmul(X, X.transpose(0, 2, 1))
    n = np.einsum("bii->bi", G)
    ni, nj = n[:, :, None], n[:, None, :]
    with np.errstate(all="ignore"):
        if kind == "IP":
            S = G.copy()
        elif kind == "COS":
            S = np.where((ni == 0) | (nj == 0), dtype(0), G / (np.sqrt(ni) * np.sqrt(nj)))
        else:
            S = dtype(0) - np.maximum((ni + nj) - dtype(2) * G, dtype(0))
    S[empty[:, :, None] | empty[:, None, :]] = 0
    assert S.dtype == dtype
    return S


def relevance(rel, ids, N, normalize, dtype=np.float32):
    """`dtype` [B, K]: r_j.  With `normalize`, (rel_j - mn) / (mx - mn) over the row's non-empty slots of finite relevance (mn and mx
    with one zero: -0 counts as +0), 0 for them when mx == mn; everything else passes through."""
    rel = np.array(rel, dtype=dtype)
    if not normalize:
        return rel
    empty = _empty(ids, N)
    out = rel.copy()
    for b in range(rel.shape[0]):
        fin = ~empty[b] & np.isfinite(rel[b])
        if not fin.any():
            continue
        mn, mx = rel[b, fin].min() + dtype(0), rel[b, fin].max() + dtype(0)
        with np.errstate(all="ignore"):
            out[b, fin] = dtype(0) if mx == mn else (rel[b, fin] - mn) / (mx - mn)
    assert out.dtype == dtype
    return out


def mmr(S, rel, ids, N, k=None, lam=0.5, normalize=False, dtype=np.float32, gaps=False):
    """(score `dtype` [B, k], ids int64 [B, k], slots int64 [B, k]) of the greedy selection over a given S [B, K, K]; once the
    non-empty slots run out: -inf, -1, -1.  With `gaps` a fourth element float64 [B]: the smallest difference, over the steps, of
    the best and the second-best score among the slots still to choose from (inf where there was no second one)."""
    S, ids = np.asarray(S), np.asarray(ids, dtype=np.int64)
    B, K = ids.shape
    k = K if k is None else k
    lam32 = np.float32(lam)
    lam_t, mu_t = dtype(lam32), dtype(np.float32(1) - lam32)
    r = relevance(rel, ids, N, normalize, dtype)
    empty = _empty(ids, N)
    score = np.full((B, k), -np.inf, dtype=dtype)
    out = np.full((B, k), -1, dtype=np.int64)
    slots = np.full((B, k), -1, dtype=np.int64)
    gap = np.full(B, np.inf)
    with np.errstate(all="ignore"):
        for b in range(B):
            lr = lam_t * r[b]
            left = np.where(empty[b], -1, ids[b])                  # the id while the slot can still be chosen
            m = None
            for t in range(k):
                sc = lr if m is None else lr - mu_t * m
                assert sc.dtype == dtype
                o = T.slot_order(sc, left, N)
                s = int(o[0])
                if left[s] < 0:
                    break
                if K > 1 and left[o[1]] >= 0:
                    gap[b] = min(gap[b], float(sc[s]) - float(sc[o[1]]))
                score[b, t], out[b, t], slots[b, t] = sc[s], ids[b, s], s
                left[s] = -1
                row = S[b, s].astype(dtype)
                m = row.copy() if m is None else np.where(row > m, row, m)
    return (score, out, slots, gap) if gaps else (score, out, slots)


def distances(S, kind, dtype=np.float32):
    """`dtype`: D_ij formed from S_ij in `dtype`."""
    S = np.asarray(S).astype(dtype)
    with np.errstate(all="ignore"):
        return dtype(1) - S if kind == "COS" else np.sqrt(-S) if kind == "L2" else -S


def ild(S, ids, N, kind, dtype=np.float32):
    """(mean float64 [B], sum of |D| float64 [B], pairs int64 [B]): the mean over unordered pairs of non-empty slots of D_ij, formed
    in `dtype` and summed exactly in float64 (math.fsum), rounded once by the division; NaN with fewer than two non-empty slots."""
    ids = np.asarray(ids, dtype=np.int64)
    B, K = ids.shape
    D = distances(S, kind, dtype).astype(np.float64)
    empty = _empty(ids, N)
    mean, mass, pairs = np.full(B, np.nan), np.zeros(B), np.zeros(B, dtype=np.int64)
    iu = np.triu_indices(K, 1)
    for b in range(B):
        keep = ~empty[b][iu[0]] & ~empty[b][iu[1]]
        d = D[b][iu][keep]
        pairs[b] = len(d)
        if len(d):
            mean[b] = math.fsum(d.tolist()) / len(d)
            mass[b] = math.fsum(np.abs(d).tolist())
    return mean, mass, pairs
