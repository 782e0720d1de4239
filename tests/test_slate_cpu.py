"""CPU checks of the slate diversifier: the identities of tests/slate_reference.py itself, and the refusals
that need no GPU: the argument checks of csrc/slate.hip's entry points (made before any HIP call) and of SlateDiversifier."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import slate_reference as SR
import two_stage_reference as T

NAN, INF = float("nan"), float("inf")
N = 200


def _rows(rng, B, K, lo=-3, hi=3):
    """Integer data with repeats and empties: (table, ids, rel)."""
    table = rng.integers(lo, hi + 1, size=(N, 128)).astype(np.float32)
    ids = rng.integers(0, N, size=(B, K))
    ids[:, K // 2:] = np.where(rng.random((B, K - K // 2)) < 0.4, ids[:, :1], ids[:, K // 2:])
    hit = rng.random((B, K)) < 0.125
    ids[hit] = np.array([-1, N, N + 5])[rng.integers(0, 3, size=int(hit.sum()))]
    rel = rng.integers(-8, 9, size=(B, K)).astype(np.float32)
    return table, ids, rel


def test_a_hand_made_slate():
    table = np.zeros((N, 128), dtype=np.float32)
    table[1, 0] = 1.0                       # items 1 and 2 point the same way, item 3 is orthogonal to them, item 4 is the zero row
    table[2, 0] = 2.0
    table[3, 1] = 3.0
    ids = np.array([[1, 2, 3, -1, 4]])
    cos = SR.similarity(table, ids, "COS")[0]
    assert cos[:3, :3].tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 1]] and not cos[3].any() and not cos[:, 3].any() and not cos[4].any()
    assert SR.similarity(table, ids, "IP")[0][:3, :3].tolist() == [[1, 2, 0], [2, 4, 0], [0, 0, 9]]
    l2 = SR.similarity(table, ids, "L2", np.float32)[0]
    assert l2[:3, :3].tolist() == [[0, -1, -10], [-1, 0, -13], [-10, -13, 0]] and l2[4, :3].tolist() == [-1, -4, -9]
    assert not np.signbit(np.diag(l2)).any() and l2.dtype == np.float32
    rel = np.array([[1.0, 0.9, 0.5, 7.0, 0.1]], dtype=np.float32)
    # relevance alone: 1, 2, 3, 4; then the empty slot as padding
    score, out, slots = SR.mmr(cos[None], rel, ids, N, lam=1.0)
    assert out[0].tolist() == [1, 2, 3, 4, -1] and slots[0].tolist() == [0, 1, 2, 4, -1]
    assert score[0].tolist() == [1.0, np.float32(0.9), 0.5, np.float32(0.1), -INF]
    # lam = 0.5: after item 1, its twin 2 scores 0.45 - 0.5 and the orthogonal 3 scores 0.25 - 0
    score, out, slots = SR.mmr(cos[None], rel, ids, N, k=3, lam=0.5)
    assert out[0].tolist() == [1, 3, 4] and slots[0].tolist() == [0, 2, 4]
    assert score[0].tolist() == [0.5, 0.25, np.float32(np.float32(0.5) * np.float32(0.1))]
    # normalize: (rel - 0.1) / 0.9 over the non-empty slots; the empty slot's 7.0 does not count
    r = SR.relevance(rel, ids, N, True)
    assert r[0, 0] == 1.0 and r[0, 4] == 0.0 and r[0, 3] == 7.0
    assert r[0, 1] == np.float32(np.float32(0.9) - np.float32(0.1)) / (np.float32(1.0) - np.float32(0.1))
    # ild: pairs of the four non-empty slots; the zero row is at cosine distance 1 from everything
    mean, mass, pairs = SR.ild(cos[None], ids, N, "COS")
    assert pairs[0] == 6 and mean[0] == (0 + 1 + 1 + 1 + 1 + 1) / 6 and mass[0] == 5
    mean, _, pairs = SR.ild(l2[None], ids, N, "L2")
    assert pairs[0] == 6 and mean[0] == math.fsum([1, float(np.sqrt(np.float32(10))), 1, float(np.sqrt(np.float32(13))), 2, 3]) / 6
    mean, _, pairs = SR.ild(cos[None][:, :2, :2], np.array([[1, -1]]), N, "COS")
    assert np.isnan(mean[0]) and pairs[0] == 0


@pytest.mark.parametrize("K", [1, 7, 64])
def test_lam_one_without_normalize_is_the_two_stage_rerank(K):
    rng = np.random.default_rng(K)
    table, ids, rel = _rows(rng, 20, K)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    hit = rng.random(rel.shape) < 0.3
    rel[hit] = special[rng.integers(0, 5, size=int(hit.sum()))]
    S = SR.similarity(table, ids, "L2", np.float32)
    for k in sorted({1, min(10, K), K}):
        score, out, slots = SR.mmr(S, rel, ids, N, k=k, lam=1.0)
        vals, want = T.rerank(rel, ids, N, k)
        assert np.array_equal(out, want) and np.array_equal(score.astype(np.float64), vals, equal_nan=True)
        for b in range(20):
            assert slots[b].tolist() == [int(s) if 0 <= ids[b, s] < N else -1 for s in T.slot_order(rel[b], ids[b], N)[:k]]


def test_float32_and_float64_forms_agree_on_integer_data():
    rng = np.random.default_rng(0)
    table, ids, rel = _rows(rng, 100, 17)
    for kind in ("IP", "L2"):
        S32, S64 = SR.similarity(table, ids, kind, np.float32), SR.similarity(table, ids, kind, np.float64)
        assert S32.dtype == np.float32 and np.array_equal(S32.astype(np.float64), S64)
        assert np.array_equal(S64, S64.transpose(0, 2, 1)) and np.abs(S64).max() < 2 ** 24
        for lam in (0.25, 0.5):
            a = SR.mmr(S32, rel, ids, N, lam=lam, dtype=np.float32)
            b = SR.mmr(S64, rel, ids, N, lam=lam, dtype=np.float64)
            assert a[0].dtype == np.float32 and b[0].dtype == np.float64
            assert np.array_equal(a[0].astype(np.float64), b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # ties are everywhere on such data: in most rows several slots of different ids share the best relevance
    filled = (ids >= 0) & (ids < N)
    best = np.where(filled, rel, -np.inf).max(1, keepdims=True)
    tied = [len(set(ids[r][filled[r] & (rel[r] == best[r])].tolist())) > 1 for r in range(len(ids))]
    assert sum(tied) > len(ids) // 4


def test_outputs_are_padded_once_the_slots_run_out():
    rng = np.random.default_rng(3)
    table, ids, rel = _rows(rng, 6, 9)
    ids[0] = -1                                                  # nothing
    ids[1, 1:] = N                                               # one item
    ids[2, :] = 5                                                # nine slots of one item: all are chosen, by slot
    S = SR.similarity(table, ids, "IP", np.float32)
    rel[2] = 1.0
    for normalize in (False, True):
        score, out, slots = SR.mmr(S, rel, ids, N, lam=0.5, normalize=normalize)
        assert (out[0] == -1).all() and (slots[0] == -1).all() and np.isneginf(score[0]).all()
        assert out[1].tolist() == [ids[1, 0]] + [-1] * 8 and slots[1].tolist() == [0] + [-1] * 8 and np.isneginf(score[1, 1:]).all()
        assert out[2].tolist() == [5] * 9 and slots[2].tolist() == list(range(9))
        filled = (ids >= 0) & (ids < N)
        assert ((out >= 0).sum(1) == filled.sum(1)).all()
        for b in range(6):
            picked = slots[b][slots[b] >= 0]
            assert len(set(picked.tolist())) == len(picked) and filled[b, picked].all()
            assert np.array_equal(out[b, : len(picked)], ids[b, picked])
    # normalize: a row whose finite relevances are all equal scores 0; -0 and +0 are one minimum
    r = SR.relevance([[2.0, 2.0, INF, NAN, 2.0]], [[1, 2, 3, 4, -1]], N, True)
    assert r[0, :2].tolist() == [0.0, 0.0] and r[0, 2] == INF and np.isnan(r[0, 3]) and r[0, 4] == 2.0
    a = SR.relevance([[-0.0, 0.0, 1.0]], [[1, 2, 3]], N, True)
    b = SR.relevance([[0.0, -0.0, 1.0]], [[2, 1, 3]], N, True)
    assert a.tolist() == [[-0.0, 0.0, 1.0]] and np.signbit(a[0, 0]) and not np.signbit(a[0, 1])
    assert np.signbit(b[0, 1]) and not np.signbit(b[0, 0])


# ---------------------------------------------------------------- refusals

def _aligned(buf):
    p = C.cast(C.byref(buf, 0), C.c_void_p)
    return C.c_void_p((p.value + 15) & ~15)


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    from recnn_amd import _lib as L
    lib = L.load()
    buf = (C.c_float * 1024)()
    p = _aligned(buf)
    odd = C.c_void_p(p.value + 2)

    def rerank(K=10, k=5, lam=0.5, kind=2, ids64=1, ld_ids=10, ld_rel=10, normalize=0, table=p, rel=p, n_rows=2, n_items=100):
        return lib.recnn_slate_rerank(table, n_items, p, ld_ids, n_rows, K, ids64, kind, rel, ld_rel, lam, normalize, k, p, p, p, None)
    for K in (65, 0, -1):
        assert rerank(K=K, k=1) != 0 and b"n_candidates must be from 1 to 64" in lib.recnn_last_error()
    for k in (0, 11, -1):
        assert rerank(k=k) != 0 and b"1 <= k <= n_candidates" in lib.recnn_last_error()
    for lam in (-0.25, 1.5, NAN, INF):
        assert rerank(lam=lam) != 0 and b"lam must be in [0, 1]" in lib.recnn_last_error()
    for kind in (-1, 3):
        assert rerank(kind=kind) != 0 and b"kind must be 0 (IP), 1 (L2) or 2 (COS)" in lib.recnn_last_error()
    assert rerank(ids64=2) != 0 and b"ids_are_int64" in lib.recnn_last_error()
    assert rerank(ld_ids=9) != 0 and b"ld_ids" in lib.recnn_last_error()
    assert rerank(ld_rel=9) != 0 and b"ld_rel" in lib.recnn_last_error()
    assert rerank(rel=odd) != 0 and b"rel" in lib.recnn_last_error()
    assert rerank(normalize=2) != 0 and b"normalize" in lib.recnn_last_error()
    assert rerank(table=None) != 0 and b"slate_rerank: null pointer" in lib.recnn_last_error()
    assert rerank(rel=None) != 0 and b"slate_rerank: null pointer" in lib.recnn_last_error()
    assert rerank(table=C.c_void_p(p.value + 4)) != 0 and b"table must be 16-byte aligned" in lib.recnn_last_error()
    assert rerank(n_items=0) != 0 and b"n_items > 0" in lib.recnn_last_error()
    assert rerank(n_rows=-1) != 0 and b"n_rows >= 0" in lib.recnn_last_error()
    for fn, name in ((lib.recnn_slate_similarity, b"slate_similarity"), (lib.recnn_slate_ild, b"slate_ild")):
        assert fn(p, 100, p, 70, 2, 65, 1, 2, p, None) != 0 and name + b": n_candidates must be from 1 to 64" in lib.recnn_last_error()
        assert fn(p, 100, p, 10, 2, 10, 1, 7, p, None) != 0 and name + b": kind" in lib.recnn_last_error()
        assert fn(p, 100, p, 10, 2, 10, 1, 2, None, None) != 0 and name + b": out" in lib.recnn_last_error()
        assert fn(p, 100, p, 10, 2, 10, 1, 2, odd, None) != 0 and name + b": out" in lib.recnn_last_error()
        assert fn(p, 100, odd, 10, 2, 10, 0, 2, p, None) != 0 and b"ids must be aligned" in lib.recnn_last_error()
        assert fn(p, 100, None, 10, 0, 10, 1, 2, None, None) == 0                     # zero rows launch nothing, need no storage
    assert lib.recnn_slate_rerank(p, 100, None, 10, 0, 10, 1, 2, None, 10, 0.5, 0, 3, None, None, None, None) == 0


def _shell(table, kind="COS"):
    """A SlateDiversifier without its constructor (which wants the table on the GPU)."""
    from recnn_amd import retrieval as RT
    o = object.__new__(RT.SlateDiversifier)
    o.table, o.kind = table, kind
    o.n_items, o.dim = table.shape
    return o


def test_slate_diversifier_refuses_by_name_and_fails_loudly_on_cpu_tensors():
    import recnn
    from recnn_amd import _lib as L
    from recnn_amd import retrieval as RT
    assert "SlateDiversifier" in RT.__all__ and recnn.retrieval.SlateDiversifier is RT.SlateDiversifier
    table = torch.zeros(N, 128)
    for kind in ("cos", "L1", None, 2):
        with pytest.raises(ValueError, match=r"similarity must be one of \['COS', 'IP', 'L2'\]"):
            RT.SlateDiversifier(table, kind)
    for bad in (torch.zeros(N, 64), torch.zeros(128), torch.zeros(0, 128)):
        with pytest.raises(ValueError, match=r"item table must be \[N, 128\]"):
            RT.SlateDiversifier(bad)
    with pytest.raises(L.RecnnHipError, match="no CPU fallback"):
        RT.SlateDiversifier(table, "L2")

    d = _shell(table)
    ids = torch.zeros(4, 10, dtype=torch.int64)
    rel = torch.zeros(4, 10)
    calls = (lambda i: d.similarity(i), lambda i: d.ild(i), lambda i: d.rerank(torch.zeros(i.shape[0], i.shape[-1]), i))
    for call in calls:
        with pytest.raises(ValueError, match="ids must be an integer tensor"):
            call(ids.float())
        with pytest.raises(ValueError, match=r"ids must be \[B, K\]"):
            call(ids[0])
        with pytest.raises(ValueError, match="ids holds K = 65 candidates per row; a slate takes at most 64"):
            call(torch.zeros(2, 65, dtype=torch.int32))
        with pytest.raises(ValueError, match="the ids live on meta, the index on cpu"):
            call(torch.zeros(4, 10, dtype=torch.int64, device="meta"))
        with pytest.raises(L.RecnnHipError, match="no CPU fallback"):           # everything in order, but nothing is on the GPU
            call(ids)
    with pytest.raises(ValueError, match="ids must be an integer tensor"):
        d.similarity([[1, 2]])
    for k in (0, 11, -1, 2.5):
        with pytest.raises(ValueError, match="k must be an integer from 1 to the 10 candidates"):
            d.rerank(rel, ids, k)
    for lam in (-0.1, 1.01, NAN):
        with pytest.raises(ValueError, match=r"lam must be in \[0, 1\]"):
            d.rerank(rel, ids, 5, lam)
    with pytest.raises(ValueError, match="3 rows of relevance but ids of 4 rows"):
        d.rerank(rel[:3], ids)
    with pytest.raises(ValueError, match=r"relevance is \(4, 9\) but ids \(4, 10\)"):
        d.rerank(rel[:, :9], ids)
    with pytest.raises(ValueError, match="relevance must be a floating-point tensor"):
        d.rerank(ids, ids)
    with pytest.raises(ValueError, match="the relevance lives on meta"):
        d.rerank(torch.zeros(4, 10, device="meta"), ids)


def test_two_stage_search_takes_diversify_and_the_policy_passes_it_on():
    import inspect

    import recnn_amd
    from recnn_amd import retrieval as RT
    sig = inspect.signature(RT.TwoStageIndex.search).parameters
    assert sig["diversify"].default is None and sig["similarity"].default == "COS"
    assert inspect.signature(recnn_amd.nn.WolpertingerPolicy.recommend).parameters["diversify"].default is None
