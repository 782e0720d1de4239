"""CPU: the numpy reference of the per-row exclusion (tests/seen_reference.py) against brute-force loops, the identity the GPU
tests lean on, SeenItems' argument refusals and the host-only size query of csrc/seen.hip."""
import ctypes as C

import numpy as np
import pytest
import torch

import ranking_eval_reference as R
import seen_reference as S


def _lists(rng, B, N, longest):
    out = []
    for _ in range(B):
        ids = rng.integers(-2, N + 2, size=int(rng.integers(0, longest + 1))).tolist()
        out.append(ids + ids[:1] + [-1, N, 2 ** 31 + 5])                # a duplicate and the out-of-range values
    return out


@pytest.mark.parametrize("N", [1, 63, 64, 65, 129, 200])
def test_mask_words_against_a_loop(N):
    rng = np.random.default_rng(N)
    lists = _lists(rng, 4, N, 2 * N) + [[], list(range(N))]
    keep = [0, N - 1, -1, N, lists[4][0] if lists[4] else 0, N // 2]
    for kp in (None, keep):
        got = S.mask_words(lists, N, kp)
        assert got.dtype == np.uint64 and got.shape == (6, (N + 63) // 64)
        for b, ids in enumerate(lists):
            want = {i for i in ids if 0 <= i < N}
            if kp is not None:
                want.discard(kp[b])
            for i in range(got.shape[1] * 64):
                assert (int(got[b, i >> 6]) >> (i & 63)) & 1 == (i in want), (N, b, i)


def _rank_loop(keys, g, excluded, larger_is_better):
    """The definition, item by item: NaN after every number, ties to the smaller id."""
    def before(i, j):
        a, b = keys[i], keys[j]
        if np.isnan(a):
            return bool(np.isnan(b)) and i < j
        if np.isnan(b):
            return True
        if a != b:
            return a > b if larger_is_better else a < b
        return i < j
    return sum(1 for i in range(len(keys)) if i != g and i not in excluded and before(i, g))


@pytest.mark.parametrize("larger_is_better", [False, True])
def test_ranks_from_keys_excluding_against_a_loop(larger_is_better):
    rng = np.random.default_rng(3)
    B, N = 7, 40
    keys = rng.integers(0, 6, size=(B, N)).astype(np.float64)          # many ties
    keys[rng.random((B, N)) < 0.1] = np.nan
    lists = _lists(rng, B, N, 30)
    lists[2] = list(range(N))                                           # everything excluded
    lists[3] = []
    targets = np.array([0, N - 1, 5, 7, -1, N, 13])
    lists[6] = lists[6] + [13]                                          # an excluded target is still ranked
    got = S.ranks_from_keys_excluding(keys, targets, lists, larger_is_better)
    for b in range(B):
        g = int(targets[b])
        want = _rank_loop(keys[b], g, set(S.excluded_set(lists[b], N)), larger_is_better) if 0 <= g < N else -1
        assert got[b] == want, (b, got[b], want)
    assert got[2] == 0 and got[4] == -1 and got[5] == -1
    # no exclusion: the existing reference
    assert S.ranks_from_keys_excluding(keys, targets, [[]] * B, larger_is_better).tolist() == \
        R.ranks_from_keys(keys, targets, larger_is_better).tolist()


def test_filter_order():
    assert S.filter_order([4, 2, 9, 0, 7], [2, 7, 100, -1], 2) == [4, 9]
    assert S.filter_order([4, 2, 9, 0, 7], [2, 7, 2], 5) == [4, 9, 0, -1, -1]
    assert S.filter_order([4, 2], [4, 2], 3) == [-1, -1, -1]
    assert S.filter_order([4, 2], [], 2) == [4, 2]


def _order_before(keys, i, g, larger_is_better):
    return R.ranks_from_keys(keys[None, [i, g]], [1], larger_is_better)[0] == 1


@pytest.mark.parametrize("larger_is_better", [False, True])
def test_filtered_rank_is_unfiltered_rank_minus_excluded_items_in_front(larger_is_better):
    """filtered rank = unfiltered rank - #{distinct excluded e != g that come before g}: the identity test_gpu_seen.py checks with
    the unfiltered rank_of on the excluded ids themselves."""
    rng = np.random.default_rng(8)
    B, N = 9, 150
    keys = rng.standard_normal((B, N))
    keys[:, 100:] = keys[:, :50]                                        # exact ties, decided by id
    lists = _lists(rng, B, N, 60)
    targets = rng.integers(0, N, size=B)
    targets[:3] = [0, 120, N - 1]
    plain = R.ranks_from_keys(keys, targets, larger_is_better)
    filtered = S.ranks_from_keys_excluding(keys, targets, lists, larger_is_better)
    for b in range(B):
        g = int(targets[b])
        in_front = sum(1 for e in S.excluded_set(lists[b], N) if e != g and _order_before(keys[b], e, g, larger_is_better))
        assert filtered[b] == plain[b] - in_front
        # "e comes before g" is "rank of g with only {e, g} present is 1", and also "rank(e) < rank(g)"
        ranks_e = R.ranks_from_keys(np.repeat(keys[b:b + 1], N, 0), np.arange(N), larger_is_better)
        assert in_front == sum(1 for e in S.excluded_set(lists[b], N) if e != g and ranks_e[e] < ranks_e[g])


def test_seen_items_refuses_bad_arguments_by_name():
    from recnn_amd import _lib as L
    from recnn_amd.retrieval import SeenItems
    ids = torch.arange(10, dtype=torch.int32)
    ok = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="ids must be a 1-D integer tensor"):
        SeenItems(ids.float(), ok, ok)
    with pytest.raises(ValueError, match="ids must be a 1-D integer tensor"):
        SeenItems(ids[None], ok, ok)
    with pytest.raises(ValueError, match="starts must be a 1-D integer tensor"):
        SeenItems(ids, ok.float(), ok)
    with pytest.raises(ValueError, match="starts must be a 1-D integer tensor"):
        SeenItems(ids, ok[None], ok)
    with pytest.raises(ValueError, match="lengths must be a 1-D integer tensor"):
        SeenItems(ids, ok, ok.bool())
    with pytest.raises(ValueError, match="3 starts but 2 lengths"):
        SeenItems(ids, ok, ok[:2])
    with pytest.raises(ValueError, match="keep must be a 1-D integer tensor"):
        SeenItems(ids, ok, ok, keep=ok.double())
    with pytest.raises(ValueError, match="3 starts but 4 keep"):
        SeenItems(ids, ok, ok, keep=torch.zeros(4, dtype=torch.int32))
    if not torch.cuda.is_available():
        with pytest.raises(L.RecnnHipError, match="GPU"):                # no CPU fallback
            SeenItems(ids, ok, ok)
        with pytest.raises(L.RecnnHipError, match="GPU"):
            SeenItems.from_lists([[1, 2], []], device="cpu")


def test_seen_mask_size_query_is_host_only_and_validates():
    from recnn_amd import _lib as L
    lib = L.load()
    n = C.c_int64(-1)
    for items, words in ((1, 1), (64, 1), (65, 2), (26744, 418), (1 << 20, 16384)):
        assert lib.recnn_seen_mask_words(items, C.byref(n)) == 0 and n.value == words
    assert lib.recnn_seen_mask_words((1 << 20) + 1, C.byref(n)) != 0
    assert b"1048576" in lib.recnn_last_error() and b"seen_mask_words" in lib.recnn_last_error()
    assert lib.recnn_seen_mask_words(0, C.byref(n)) != 0
    assert lib.recnn_seen_mask_words(5, None) != 0
    assert n.value == 16384                                             # a refused query writes nothing
    # the build refuses bad arguments before any HIP call
    assert lib.recnn_seen_mask_build(None, 0, None, None, None, 3, 10, None, None) != 0
    assert b"seen_mask_build" in lib.recnn_last_error()
    assert lib.recnn_seen_mask_build(None, 0, None, None, None, 0, (1 << 20) + 1, None, None) != 0
    assert b"1048576" in lib.recnn_last_error()
    assert lib.recnn_seen_mask_build(None, 0, None, None, None, 0, 10, None, None) == 0      # no rows: nothing to do
