"""CPU checks of the two-stage recommendation: the reference order of tests/two_stage_reference.py on
hand-made cases and against a pairwise comparator, the two-stage rank identity, and the refusals that need no GPU: the argument
checks of csrc/qcand.hip's entry points (made before any HIP call) and of TwoStageIndex / WolpertingerPolicy."""
import functools
import math

import numpy as np
import pytest
import torch

import two_stage_reference as T

NAN, INF = float("nan"), float("inf")


def test_reference_order_on_a_hand_made_row():
    N = 10
    #       slot  0    1    2     3    4    5    6     7    8    9    10
    ids = [[3,   7,   3,   -1,   9,   10,  2,   5,    0,   7,   2]]
    q = [[1.0, NAN, 1.0, 99.0, 0.0, 5.0, -0.0, INF, -INF, NAN, 0.0]]
    # numbers: inf(5) > 1.0 (id 3: slot 0 then slot 2) > zeros (id 2 slot 6, id 2 slot 10, id 9 slot 4: -0 == +0, id first) > -inf(0);
    # then the NaN of id 7 (slot 1, slot 9); then the empty slots 3 (id -1) and 5 (id 10 = N) in slot order
    assert T.slot_order(q[0], ids[0], N).tolist() == [7, 0, 2, 6, 10, 4, 8, 1, 9, 3, 5]
    vals, out = T.rerank(q, ids, N)
    assert out[0].tolist() == [5, 3, 3, 2, 2, 9, 0, 7, 7, -1, -1]
    assert np.array_equal(vals[0], [INF, 1.0, 1.0, 0.0, 0.0, 0.0, -INF, NAN, NAN, -INF, -INF], equal_nan=True)
    vals, out = T.rerank(q, ids, N, k=3)
    assert out[0].tolist() == [5, 3, 3] and vals[0].tolist() == [INF, 1.0, 1.0]
    # pos: first slot of a repeated id; a NaN candidate still has a place; absent; out of range (even though slot 5 holds "10")
    assert T.pos(q * 6, ids * 6, N, [5, 3, 2, 7, 4, 10]).tolist() == [0, 1, 3, 7, -1, -1]
    assert T.pos(q, ids, N, [-1]).tolist() == [-1]
    # rows that are all empty, and with one non-empty slot in the middle
    vals, out = T.rerank([[1.0, 2.0, 3.0]], [[-1, N, N + 5]], N)
    assert out[0].tolist() == [-1, -1, -1] and np.isneginf(vals[0]).all()
    vals, out = T.rerank([[1.0, 2.0, 3.0]], [[-1, 4, N]], N)
    assert out[0].tolist() == [4, -1, -1] and vals[0].tolist() == [2.0, -INF, -INF]
    assert T.pos([[1.0, 2.0, 3.0]], [[-1, 4, N]], N, [4]).tolist() == [0]


def _cmp(a, b):
    """The order stated pair by pair for slots (score, id, slot, empty)."""
    (sa, ia, ja, ea), (sb, ib, jb, eb) = a, b
    if ea != eb:
        return 1 if ea else -1
    if ea:
        return -1 if ja < jb else 1
    na, nb = math.isnan(sa), math.isnan(sb)
    if na != nb:
        return 1 if na else -1
    if not na and sa != sb:
        return -1 if sa > sb else 1
    return -1 if (ia, ja) < (ib, jb) else 1


@pytest.mark.parametrize("K", [1, 7, 64])
def test_reference_order_against_a_pairwise_sort(K):
    N = 12
    rng = np.random.default_rng(K)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    for _ in range(20):
        q = rng.integers(-2, 3, size=K).astype(np.float32)
        hit = rng.random(K) < 0.3
        q[hit] = special[rng.integers(0, 5, size=int(hit.sum()))]
        ids = rng.integers(-2, N + 2, size=K)
        slots = [(float(q[j]), int(ids[j]), j, not 0 <= ids[j] < N) for j in range(K)]
        want = [s[2] for s in sorted(slots, key=functools.cmp_to_key(_cmp))]
        assert T.slot_order(q, ids, N).tolist() == want
        g = int(rng.integers(0, N))
        holds = [n for n, j in enumerate(want) if ids[j] == g]
        assert T.pos(q[None], ids[None], N, [g]).tolist() == [holds[0] if holds else -1]


def test_q_of_looks_the_ids_up_and_two_stage_rank_identity():
    qm = np.arange(12, dtype=np.float64).reshape(2, 6)
    got = T.q_of(qm, [[5, 0, -1, 6], [2, 2, 11, 1]])
    assert np.array_equal(got, [[5.0, 0.0, -INF, -INF], [8.0, 8.0, -INF, 7.0]])
    # position where the target is a candidate; else the flat rank, but never before the candidates; -1 stays -1
    assert T.two_stage_rank([3, -1, -1, -1], [9, 70, 2, -1], [64, 64, 5, 64]).tolist() == [3, 70, 5, -1]


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    import ctypes as C
    from recnn_amd import _lib as L
    lib = L.load()
    buf = (C.c_float * 1024)()
    p = C.cast(C.byref(buf, 0), C.c_void_p)                       # 16-byte alignment is not promised for a ctypes array: find it
    p = C.c_void_p((p.value + 15) & ~15)
    common = (p, 64, 2, p, 64, 10, 64, p, p, p, 0.0, p, 70)

    def rerank(n_cand, k, targets=None, pos=None, fallback=None, ids64=1):
        return lib.recnn_qcand_rerank(*common, n_cand, ids64, k, p, p, targets, pos, fallback, None)
    assert rerank(65, 10) != 0 and b"at most 64 candidates" in lib.recnn_last_error()
    for k in (0, 11, -1):
        assert rerank(10, k) != 0 and b"1 <= k <= n_candidates" in lib.recnn_last_error()
    assert rerank(10, 5, targets=p) != 0 and b"targets and out_pos go together" in lib.recnn_last_error()
    assert rerank(10, 5, fallback=p) != 0 and b"fallback_rank" in lib.recnn_last_error()
    assert rerank(10, 5, ids64=2) != 0 and b"ids_are_int64" in lib.recnn_last_error()
    assert rerank(0, 1) != 0 and b"n_candidates > 0" in lib.recnn_last_error()
    assert lib.recnn_qcand_rerank(None, 64, 2, p, 64, 10, 64, p, p, p, 0.0, p, 70, 10, 1, 5, p, p, None, None, None, None) != 0
    assert b"qcand_rerank: null pointer" in lib.recnn_last_error()

    def scores(hp=64, ld_ids=70, n_cand=10, ld_out=10, ld_e1=64):
        return lib.recnn_qcand_scores(p, 64, 2, p, ld_e1, 10, hp, p, p, p, 0.0, p, ld_ids, n_cand, 0, p, ld_out, None)
    assert scores(hp=320) != 0 and b"up to 256" in lib.recnn_last_error()
    assert scores(hp=48) != 0 and scores(ld_e1=32) != 0
    assert scores(ld_ids=9) != 0 and b"row stride of at least n_candidates" in lib.recnn_last_error()
    assert scores(ld_out=9) != 0 and b"ld_out" in lib.recnn_last_error()
    assert scores(n_cand=65535 * 64 + 1, ld_ids=1 << 23, ld_out=1 << 23) != 0 and b"candidates per row" in lib.recnn_last_error()
    # zero rows launch nothing and need no storage
    assert lib.recnn_qcand_scores(None, 64, 0, p, 64, 10, 64, p, p, p, 0.0, None, 10, 10, 0, None, 10, None) == 0
    assert lib.recnn_qcand_rerank(None, 64, 0, p, 64, 10, 64, p, p, p, 0.0, None, 10, 10, 0, 3, None, None, None, None, None, None) == 0


def _shell(cls, **attrs):
    """An index object without its constructor (which wants the GPU): the attributes `TwoStageIndex` checks."""
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_two_stage_index_and_policy_refuse_by_name():
    import recnn_amd
    from recnn_amd import _lib as L
    from recnn_amd import retrieval as RT
    table = torch.zeros(100, 128)
    flat = _shell(RT.FlatIndex, n_items=100, table=table)
    critic = _shell(RT.CriticIndex, n_items=100, table=table)
    with pytest.raises(TypeError, match="FlatIndex and a CriticIndex.*CriticIndex and FlatIndex"):
        RT.TwoStageIndex(critic, flat)
    with pytest.raises(TypeError, match="FlatIndex and a CriticIndex"):
        RT.TwoStageIndex(flat, table)
    for n in (0, 65, 2.5, -1):
        with pytest.raises(ValueError, match="n_candidates must be an integer from 1 to 64"):
            RT.TwoStageIndex(flat, critic, n)
    with pytest.raises(ValueError, match="same table.*100 items.*99"):
        RT.TwoStageIndex(flat, _shell(RT.CriticIndex, n_items=99, table=table))
    with pytest.raises(ValueError, match="lives on cpu.*meta"):
        RT.TwoStageIndex(flat, _shell(RT.CriticIndex, n_items=100, table=torch.zeros(100, 128, device="meta")))
    with pytest.raises(ValueError, match="holds only 40 items"):
        RT.TwoStageIndex(_shell(RT.FlatIndex, n_items=40, table=table), _shell(RT.CriticIndex, n_items=40, table=table), 64)
    two = RT.TwoStageIndex(flat, critic, 32)
    assert two.n_candidates == 32 and two.ntotal == 100
    # no CPU fallback: the policy's indexes want the table on the GPU
    with pytest.raises(L.RecnnHipError):
        recnn_amd.nn.WolpertingerPolicy(recnn_amd.nn.Actor(20, 128, 16), recnn_amd.nn.Critic(20, 128, 16), table)
    assert recnn_amd.nn.WolpertingerPolicy is recnn_amd.nn.policy.WolpertingerPolicy
    import recnn
    assert recnn.nn.WolpertingerPolicy is recnn_amd.nn.WolpertingerPolicy and recnn.retrieval.TwoStageIndex is RT.TwoStageIndex
