"""CPU checks of the value-ranking stack: the reference order of tests/critic_index_reference.py against a
pairwise comparator, argument validation of CriticIndex / topk_of_scores / rank_in_scores, no CPU fallback, and the host-only size
queries of csrc/qrank.hip and csrc/scoresel.hip."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import critic_index_reference as R


def _cmp(a, b):
    """The order stated pair by pair: (score, id) a before b -> -1."""
    (sa, ia), (sb, ib) = a, b
    na, nb = math.isnan(sa), math.isnan(sb)
    if na != nb:
        return 1 if na else -1
    if not na and sa != sb:                                  # -0.0 == 0.0 here, as the order wants
        return -1 if sa > sb else 1
    return -1 if ia < ib else (1 if ia > ib else 0)


def _brute(row, gone):
    items = [(float(s), i) for i, s in enumerate(row) if i not in gone]
    return [i for _, i in sorted(items, key=functools.cmp_to_key(_cmp))]


def _rows(seed, B, N):
    rng = np.random.default_rng(seed)
    s = rng.integers(-3, 4, size=(B, N)).astype(np.float32)              # heavy ties
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    hit = rng.random((B, N)) < 0.3
    s[hit] = special[rng.integers(0, 5, size=int(hit.sum()))]
    if B > 1:
        s[1] = np.nan                                                     # a row of NaN orders by id
    if B > 2:
        s[2] = -0.0
        s[2, ::2] = 0.0                                                   # one value: orders by id
    return s


@pytest.mark.parametrize("B,N", [(1, 1), (3, 7), (4, 65), (5, 200)])
def test_reference_order_against_a_pairwise_sort(B, N):
    s = _rows(B * 1000 + N, B, N)
    rng = np.random.default_rng(7)
    excluded = [rng.integers(-2, N + 2, size=int(rng.integers(0, N + 1))).tolist() for _ in range(B)]
    for ex in (None, excluded):
        for k in (1, 10, 64):
            vals, ids = R.topk(s, k, ex)
            for b in range(B):
                want = _brute(s[b], set() if ex is None else set(ex[b]))[:k]
                assert ids[b, :len(want)].tolist() == want and (ids[b, len(want):] == -1).all()
                assert np.array_equal(vals[b, :len(want)], s[b, want].astype(np.float64), equal_nan=True)
                assert np.isneginf(vals[b, len(want):]).all()
        targets = rng.integers(0, N, size=B)
        got = R.ranks(s, targets, ex)
        for b in range(B):
            gone = (set() if ex is None else set(ex[b])) - {int(targets[b])}     # the target's own bit is not consulted
            assert got[b] == _brute(s[b], gone).index(int(targets[b]))
    assert R.ranks(s, np.full(B, N), None).tolist() == [-1] * B and R.ranks(s, np.full(B, -1), None).tolist() == [-1] * B


def test_reference_values_int_and_float_agree_on_integers():
    rng = np.random.default_rng(3)
    S, A, H, B, N = 5, 4, 8, 3, 6
    draw = lambda *sh: rng.integers(-1, 2, size=sh)
    args = (draw(B, S), draw(N, A), draw(H, S + A), draw(H), draw(H, H), draw(H), draw(1, H), draw(1))
    q, bound = R.q_values_int(*args)
    assert q.dtype == np.int64 and bound <= H * (H * (S + A + 1) + 1) + 1
    assert np.array_equal(q.astype(np.float64), R.q_values(*args))
    # one pair by hand
    x = np.concatenate([args[0][1], args[1][4]])
    h1 = np.maximum(args[2] @ x + args[3], 0)
    h2 = np.maximum(args[4] @ h1 + args[5], 0)
    assert q[1, 4] == int(args[6][0] @ h2 + args[7][0])


def test_size_queries_are_host_arithmetic_and_refuse_bad_arguments():
    from recnn_amd import _lib as L
    lib = L.load()
    n, r, hp = C.c_int64(), C.c_int64(), C.c_int()
    for h, want in ((1, 64), (24, 64), (64, 64), (65, 128), (192, 192), (256, 256)):
        assert lib.recnn_qrank_hidden_padded(h, C.byref(hp)) == 0 and hp.value == want
    assert lib.recnn_qrank_hidden_padded(257, C.byref(hp)) != 0 and b"256" in lib.recnn_last_error()
    assert lib.recnn_qrank_hidden_padded(0, C.byref(hp)) != 0 and lib.recnn_qrank_hidden_padded(8, None) != 0
    # whole 16-row tiles of [rows, n_items] float32 within the limit, never less than one tile
    assert lib.recnn_qrank_block_rows(1000, 128_000, C.byref(r)) == 0 and r.value == 32
    assert lib.recnn_qrank_block_rows(1000, 191_999, C.byref(r)) == 0 and r.value == 32
    assert lib.recnn_qrank_block_rows(1000, 192_000, C.byref(r)) == 0 and r.value == 48
    assert lib.recnn_qrank_block_rows(1000, 1, C.byref(r)) == 0 and r.value == 16
    assert lib.recnn_qrank_block_rows(26_744, 256 << 20, C.byref(r)) == 0 and r.value == 2496 and r.value >= 2048
    assert lib.recnn_qrank_block_rows(0, 1 << 20, C.byref(r)) != 0 and b"qrank_block_rows" in lib.recnn_last_error()
    assert lib.recnn_qrank_block_rows(10, 0, C.byref(r)) != 0 and lib.recnn_qrank_block_rows(10, 100, None) != 0
    assert lib.recnn_scores_topk_workspace_bytes(33, 10, C.byref(n)) == 0 and n.value == 33 * 8 * 10 * 8
    assert lib.recnn_scores_topk_workspace_bytes(0, 1, C.byref(n)) == 0 and n.value == 0
    for bad in ((33, 0), (33, 65), (-1, 10)):
        assert lib.recnn_scores_topk_workspace_bytes(*bad, C.byref(n)) != 0
    assert b"k <= 64" in lib.recnn_last_error() and lib.recnn_scores_topk_workspace_bytes(1, 1, None) != 0
    a, b = C.c_int64(), C.c_int64()
    assert lib.recnn_scores_rank_workspace_bytes(33, 1000, C.byref(a)) == 0 and a.value == 33 * 3 * 4      # 3 splits of 384 items
    assert lib.recnn_scores_rank_workspace_bytes(33, 70_001, C.byref(b)) == 0 and b.value == 33 * 8 * 4
    assert lib.recnn_scores_rank_workspace_bytes(4096, 70_001, C.byref(b)) == 0 and b.value == 4096 * 4
    assert lib.recnn_scores_rank_workspace_bytes(0, 5, C.byref(b)) == 0 and b.value == 0
    assert lib.recnn_scores_rank_workspace_bytes(5, 0, C.byref(b)) != 0 and lib.recnn_scores_rank_workspace_bytes(5, 5, None) != 0
    # the launching entry points check their arguments before any HIP call
    assert lib.recnn_scores_topk(None, 10, 2, 10, 3, None, None, None, None, None, 0) != 0 and b"scores_topk" in lib.recnn_last_error()
    assert lib.recnn_scores_rank(None, 10, 2, 10, None, None, None, None, None, 0) != 0
    assert lib.recnn_qrank_scores(None, 256, 2, None, 256, 10, 256, None, None, None, 0.0, None, 10, None) != 0
    assert lib.recnn_qrank_layer1(None, 16, 2, 16, None, 16, None, 64, None, 64, None) != 0


def test_cpu_tensors_are_refused_without_a_fallback():
    import recnn_amd
    from recnn_amd import _lib as L
    from recnn_amd import retrieval as RT
    with pytest.raises(L.RecnnHipError):
        RT.topk_of_scores(torch.zeros(2, 5), 2)
    with pytest.raises(L.RecnnHipError):
        RT.rank_in_scores(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(L.RecnnHipError):
        RT.CriticIndex(recnn_amd.nn.Critic(20, 128, 16), torch.zeros(9, 128))


def test_critic_index_refuses_other_modules_and_shapes_by_name():
    """The module and the shapes are checked before the table's device, so CPU tensors reach every refusal."""
    import recnn_amd
    from recnn_amd import retrieval as RT
    Critic, Actor = recnn_amd.nn.Critic, recnn_amd.nn.Actor
    table = torch.zeros
    with pytest.raises(TypeError, match="three-layer recnn_amd.nn.Critic.*Actor"):
        RT.CriticIndex(Actor(20, 128, 16), table(9, 128))
    with pytest.raises(TypeError, match="Critic"):
        RT.CriticIndex(torch.nn.Linear(4, 4), table(9, 128))
    broken = Critic(20, 128, 16)
    broken.linear2 = torch.nn.Identity()
    with pytest.raises(TypeError, match="three-layer"):
        RT.CriticIndex(broken, table(9, 128))
    with pytest.raises(ValueError, match=r"\[N, 128\]"):
        RT.CriticIndex(Critic(20, 64, 16), table(9, 64))
    with pytest.raises(ValueError, match="limit of 256"):
        RT.CriticIndex(Critic(20, 128, 320), table(9, 128))
    with pytest.raises(ValueError, match=r"S \+ 128 inputs"):
        RT.CriticIndex(Critic(20, 100, 16), table(9, 128))            # linear1 takes 120 inputs: no state part is left
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        RT.CriticIndex(Critic(20, 128, 16), table(9, 128), max_workspace_bytes=0)
