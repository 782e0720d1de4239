"""Serving the attention encoders step by step (recnn_amd/nn/kv_cache.py, csrc/attn_dev.h): `attn_append` and
`transformer_append` over a `KVCache` against the whole-history calls `attn_encode` / `transformer_encode`, BIT FOR BIT -- under
every split of the history, in a ring of exactly `min_capacity` slots, from ragged positions, for a subset of the rows, over a cache
full of NaN -- and, once per shape, directly against the float64 model within transformer_reference.fp32_bound.

The whole-history calls are held to float64 by tests/test_gpu_attn.py and tests/test_gpu_transformer.py; equality of bits carries
their bounds over to every appended row.  The inputs of an append are read from the arrays the store was built from.  Query blocks and
key tiles are 64 positions: the splits cut at, before and after a multiple of 64."""
import copy

import numpy as np
import pytest
import torch

import attn_reference as A
import seq_reference as R
import transformer_reference as TR
from helpers import csr, make_store

pytestmark = pytest.mark.gpu

T_SHAPES = ((8, 16, 1, 16, 1), (24, 48, 3, 80, 2), (128, 256, 4, 256, 2))      # (E, H, heads, F, L)
A_SHAPES = ((8, 16, 1), (72, 64, 2))                                           # (E, H, heads)
N_USERS, N_ITEMS, LEN_MIN = 17, 300, 200
SPLITS = ((130,), (64, 66), (63, 1, 1, 65), (1, 129), (1,) * 130)
LARGE_SPLITS = SPLITS[1:3]


def _sid(s):
    return ("E%d-H%d-heads%d-F%d-L%d" if len(s) == 5 else "attn-E%d-H%d-heads%d") % s


@pytest.fixture(scope="module")
def seq_data():
    """Per E: 17 users with at least 200 elements and their table (CPU)."""
    return {E: make_store(N_USERS, N_ITEMS, E, LEN_MIN, LEN_MIN + 8, seed=E) for E in sorted({s[0] for s in T_SHAPES + A_SHAPES})}


@pytest.fixture(scope="module")
def gpu_data(cuda, seq_data):
    from recnn_amd.data.store import ReplayStore
    return {E: (ReplayStore.from_arrays(*csr(items, ratings), cuda), torch.from_numpy(table).to(cuda))
            for E, (items, ratings, table) in seq_data.items()}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _make(shape, cuda, window=None, alibi=True, act="gelu"):
    """(encoder on the GPU, its whole-history call, its append call)."""
    from recnn_amd.nn import functional as F
    if len(shape) == 5:
        E, H, heads, Ff, L = shape
        enc = TR.make_encoder(E, H, heads, Ff, L, act, window, alibi, seed=E + H + heads + Ff)
        return enc.to(cuda), F.transformer_encode, F.transformer_append
    E, H, heads = shape
    return A.make_encoder(E, H, heads, window, alibi, seed=E + H + heads).to(cuda), F.attn_encode, F.attn_append


def _inputs(seq_data, E, users, T, cuda):
    """(items int64 [U, T], ratings float32 [U, T]) on the GPU, from the arrays the store was built from."""
    items, ratings, _ = seq_data[E]
    idx, rts = A.positions([items[u] for u in users], [ratings[u] for u in users], T)
    return idx.to(cuda), rts.to(cuda)


def _feed(append, enc, cache, tbl, idx, rts, sizes, rows=None):
    """h [R, sum(sizes), H]: the columns of idx / rts appended in pieces of `sizes`."""
    out, at = [], 0
    for n in sizes:
        out.append(append(enc, cache, tbl, idx[:, at:at + n], rts[:, at:at + n], rows))
        at += n
    return torch.cat(out, 1)


# ---------------------------------------------------------------------------------------------------- 1. splits
@pytest.mark.parametrize("sessions", (1, 17))
@pytest.mark.parametrize("alibi", (True, False))
@pytest.mark.parametrize("shape", T_SHAPES + A_SHAPES, ids=_sid)
def test_every_split_gives_the_whole_history_call(cuda, seq_data, gpu_data, shape, alibi, sessions):
    from recnn_amd.nn import KVCache
    T, E, H = 130, shape[0], shape[1]
    st, tbl = gpu_data[E]
    enc, encode, append = _make(shape, cuda, None, alibi)
    users = list(range(sessions))
    idx, rts = _inputs(seq_data, E, users, T, cuda)
    whole = encode(enc, st, tbl, users, T)
    assert bool(torch.isfinite(whole).all()) and float(whole.abs().max()) > 0
    for sizes in (LARGE_SPLITS if H == 256 else SPLITS):
        cache = KVCache(enc, sessions, 192, max_append=max(sizes))
        at = 0
        for n in sizes:
            h = append(enc, cache, tbl, idx[:, at:at + n], rts[:, at:at + n])
            assert h.shape == (sessions, n, H) and h.dtype == torch.float32 and not h.requires_grad
            assert _same_bits(h, whole[:, at:at + n]), (sizes[:4], at)
            at += n
            if len(sizes) <= 4:                            # and the shorter whole-history call of the steps so far
                assert _same_bits(h, encode(enc, st, tbl, users, at)[:, at - n:]), (sizes, at)
        assert (cache.lengths == T).all()


@pytest.mark.parametrize("shape", T_SHAPES[:2], ids=_sid)
def test_both_feed_forward_kernels_of_the_append_give_the_same_bits(cuda, seq_data, gpu_data, shape):
    """Up to 4096 rows (R n) a block's feed-forward runs the 16-row kernel, above it the whole-history call's 64-row kernel: 64 and 65
    sessions times 64 steps lie on the two sides.  Session i replays user i % 17."""
    from recnn_amd.nn import KVCache
    E, T = shape[0], 66
    st, tbl = gpu_data[E]
    enc, encode, append = _make(shape, cuda)
    whole = encode(enc, st, tbl, list(range(N_USERS)), T)
    for sessions in (64, 65):
        users = [i % N_USERS for i in range(sessions)]
        idx, rts = _inputs(seq_data, E, users, T, cuda)
        got = _feed(append, enc, KVCache(enc, sessions, 128), tbl, idx, rts, (64, 2))
        assert _same_bits(got, whole[users]), sessions


# ---------------------------------------------------------------------------------------------------- 2. window and ring
@pytest.mark.parametrize("n", (1, 7))
@pytest.mark.parametrize("window", (1, 5, 70))
@pytest.mark.parametrize("shape", T_SHAPES[:2] + A_SHAPES[:1], ids=_sid)
def test_a_ring_of_min_capacity_gives_the_whole_history_call(cuda, seq_data, gpu_data, shape, window, n):
    from recnn_amd.nn import KVCache
    T, E, U = 200, shape[0], 3
    st, tbl = gpu_data[E]
    enc, encode, append = _make(shape, cuda, window, True, act="relu")
    idx, rts = _inputs(seq_data, E, range(U), T, cuda)
    whole = encode(enc, st, tbl, list(range(U)), T)
    cap = KVCache.min_capacity(window, n)
    assert cap < T or window == 70
    sizes = (n,) * (T // n) + ((T % n,) if T % n else ())
    got = [_feed(append, enc, KVCache(enc, U, c, max_append=n), tbl, idx, rts, sizes) for c in (cap, cap + 64)]
    assert _same_bits(got[0], whole) and _same_bits(got[1], whole)
    assert bool(torch.isfinite(whole).all())


# ---------------------------------------------------------------------------------------------------- 3. ragged positions
@pytest.mark.parametrize("shape", T_SHAPES + A_SHAPES[:1], ids=_sid)
def test_ragged_positions_in_one_append(cuda, seq_data, gpu_data, shape):
    from recnn_amd.nn import KVCache
    P, n, E = (0, 1, 63, 64, 65, 100), 3, shape[0]
    st, tbl = gpu_data[E]
    enc, encode, append = _make(shape, cuda)
    users = list(range(len(P)))
    idx, rts = _inputs(seq_data, E, users, max(P) + n, cuda)
    whole = encode(enc, st, tbl, users, max(P) + n)
    cache = KVCache(enc, len(P), 128, max_append=100)
    for i, p in enumerate(P):
        if p:
            append(enc, cache, tbl, idx[i:i + 1, :p], rts[i:i + 1, :p], [i])
    assert list(cache.lengths) == list(P)
    new = torch.stack([idx[i, p:p + n] for i, p in enumerate(P)]), torch.stack([rts[i, p:p + n] for i, p in enumerate(P)])
    h = append(enc, cache, tbl, *new)
    for i, p in enumerate(P):
        assert _same_bits(h[i], whole[i, p:p + n]), (i, p)
    assert list(cache.lengths) == [p + n for p in P]


# ---------------------------------------------------------------------------------------------------- 4. row subsets
@pytest.mark.parametrize("shape", (T_SHAPES[1], A_SHAPES[0]), ids=_sid)
def test_a_subset_of_the_rows_leaves_the_others_alone(cuda, seq_data, gpu_data, shape):
    from recnn_amd.nn import KVCache
    E, rows, sizes = shape[0], [5, 2, 9], (70, 3)
    st, tbl = gpu_data[E]
    enc, encode, append = _make(shape, cuda)
    idx, rts = _inputs(seq_data, E, range(3), sum(sizes), cuda)
    big, small = KVCache(enc, 12, 128, max_append=70), KVCache(enc, 3, 128, max_append=70)
    big.kv.normal_()
    before = big.kv.clone()
    got = _feed(append, enc, big, tbl, idx, rts, sizes, rows)
    assert _same_bits(got, _feed(append, enc, small, tbl, idx, rts, sizes))
    assert _same_bits(got, encode(enc, st, tbl, [0, 1, 2], sum(sizes)))
    others = [r for r in range(12) if r not in rows]
    assert _same_bits(big.kv[:, others], before[:, others])
    assert not _same_bits(big.kv[:, rows], before[:, rows])
    assert list(big.lengths[others]) == [0] * 9 and list(big.lengths[rows]) == [73] * 3
    # a session's k and v do not depend on the row it lives in
    assert _same_bits(big.kv[:, rows, :73], small.kv[:, :, :73])


# ---------------------------------------------------------------------------------------------------- 5. poison
@pytest.mark.parametrize("window,n", ((None, 64), (5, 7), (70, 1)))
@pytest.mark.parametrize("shape", (T_SHAPES[1], A_SHAPES[0]), ids=_sid)
def test_a_cache_full_of_nan_changes_nothing(cuda, seq_data, gpu_data, shape, window, n):
    from recnn_amd.nn import KVCache
    T, E, U = 200, shape[0], 3
    st, tbl = gpu_data[E]
    enc, encode, append = _make(shape, cuda, window)
    idx, rts = _inputs(seq_data, E, range(U), T, cuda)
    whole = encode(enc, st, tbl, list(range(U)), T)
    cap = 256 if window is None else KVCache.min_capacity(window, n)
    sizes = (n,) * (T // n) + ((T % n,) if T % n else ())
    cache = KVCache(enc, U, cap, max_append=n)
    cache.kv.fill_(float("nan"))
    got = _feed(append, enc, cache, tbl, idx, rts, sizes)
    assert bool(torch.isfinite(got).all()) and _same_bits(got, whole)
    # a reset row is a fresh session: user 2's history into row 0, over user 0's stale keys
    cache.reset([0])
    assert list(cache.lengths) == [0, T, T]
    again = _feed(append, enc, cache, tbl, idx[2:3], rts[2:3], sizes, [0])
    assert _same_bits(again, whole[2:3])


# ---------------------------------------------------------------------------------------------------- 6. float64, directly
@pytest.mark.parametrize("shape", T_SHAPES, ids=_sid)
def test_appended_rows_against_float64(cuda, seq_data, gpu_data, shape):
    from recnn_amd.nn import KVCache
    T, E, U = 130, shape[0], 3
    items, ratings, table = seq_data[E]
    _, tbl = gpu_data[E]
    enc = TR.make_encoder(*shape[:5], "gelu", None, True, seed=sum(shape))
    x = R.lstm_inputs(table, items[:U], ratings[:U], T)
    bound, h64 = TR.fp32_bound(enc, x)
    ge = copy.deepcopy(enc).to(cuda)
    from recnn_amd.nn import functional as F
    idx, rts = _inputs(seq_data, E, range(U), T, cuda)
    h = _feed(F.transformer_append, ge, KVCache(ge, U, 192, max_append=65), tbl, idx, rts, (63, 1, 1, 65))
    err = float((h.cpu().double() - h64).abs().max())
    print(f"transformer_append {shape} split (63, 1, 1, 65): err {err:.3e} bound {bound:.3e} ratio {err / bound:.2f} "
          f"max|h| {float(h64.abs().max()):.3e}")
    assert err <= bound


# ---------------------------------------------------------------------------------------------------- 7. bad ids
@pytest.mark.parametrize("shape", (T_SHAPES[1], A_SHAPES[0]), ids=_sid)
def test_an_id_outside_the_table(cuda, seq_data, gpu_data, shape):
    """Session u gets an id past the table at step j = 70.  Appended as (64, 66) the second append walks the tiles the whole-history
    call walks for steps 64 .. 129, and the isnan pattern is that call's (steps 64 .. 69 included: they share j's key tile, and
    0 * NaN is NaN).  Appended one step at a time, the steps before j were returned before j arrived and keep the clean run's
    bits; from j on the pattern is again the whole-history call's.  Every other session keeps its bits throughout."""
    from recnn_amd.data.store import ReplayStore
    from recnn_amd.nn import KVCache
    T, E, U, u, j = 130, shape[0], 5, 3, 70
    items, ratings, _ = seq_data[E]
    st, tbl = gpu_data[E]
    enc, encode, append = _make(shape, cuda)
    idx, rts = _inputs(seq_data, E, range(U), T, cuda)
    clean = encode(enc, st, tbl, list(range(U)), T)
    others = [v for v in range(U) if v != u]
    for bad in (N_ITEMS, -1, 2 ** 31 - 1, 2 ** 40):
        idx2 = idx.clone()
        idx2[u, j] = bad
        items2 = [i.copy() for i in items[:U]]
        items2[u][j] = bad if bad < 2 ** 31 else -1          # (the store holds int32 ids)
        whole = encode(enc, ReplayStore.from_arrays(*csr(items2, ratings[:U]), cuda), tbl, list(range(U)), T)
        assert bool(torch.isnan(whole[u, j:]).all())
        got = _feed(append, enc, KVCache(enc, U, 192, max_append=66), tbl, idx2, rts, (64, 66))
        assert torch.equal(torch.isnan(got), torch.isnan(whole))
        assert _same_bits(got[others], clean[others]) and _same_bits(got[u, :64], clean[u, :64])
        if bad == N_ITEMS:
            ones = _feed(append, enc, KVCache(enc, U, 192), tbl, idx2, rts, (1,) * T)
            assert torch.equal(torch.isnan(ones[:, j:]), torch.isnan(whole[:, j:])) and bool(torch.isnan(ones[u, j:]).all())
            assert _same_bits(ones[others], clean[others]) and _same_bits(ones[u, :j], clean[u, :j])
    # int32 ids go down the same path
    got = _feed(append, enc, KVCache(enc, U, 192, max_append=66), tbl, idx.to(torch.int32), rts, (64, 66))
    assert _same_bits(got, clean)


# ---------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_name_the_argument_and_leave_the_cache_alone(cuda, seq_data, gpu_data):
    from recnn_amd import _lib as L
    from recnn_amd.nn import KVCache, functional as F
    E = 24
    _, tbl = gpu_data[E]
    enc, _, _ = _make(T_SHAPES[1], cuda, None)
    wenc, _, _ = _make(T_SHAPES[1], cuda, 5)
    aenc, _, _ = _make((24, 48, 3), cuda)
    idx, rts = _inputs(seq_data, E, range(4), 80, cuda)
    for p in enc.parameters():
        assert p.requires_grad
    cache = KVCache(enc, 4, 128, max_append=64)
    h = F.transformer_append(enc, cache, tbl, idx[:, :60], rts[:, :60])
    assert not h.requires_grad
    acache = KVCache(aenc, 4, 128)
    assert not F.attn_append(aenc, acache, tbl, idx[:, :60], rts[:, :60]).requires_grad
    kv0, len0 = cache.kv.clone(), cache.lengths.copy()
    ok = dict(enc=enc, cache=cache, table=tbl, items=idx[:, 60:64], ratings=rts[:, 60:64], rows=None)

    def refused(err, word, fn=F.transformer_append, **change):
        kw = dict(ok, **change)
        with pytest.raises(err) as e:
            fn(kw["enc"], kw["cache"], kw["table"], kw["items"], kw["ratings"], kw["rows"])
        assert word in str(e.value), (word, str(e.value))
        assert type(e.value) is err
        assert _same_bits(cache.kv, kv0) and np.array_equal(cache.lengths, len0)

    H = L.RecnnHipError
    refused(H, "AttentionEncoder", enc=aenc)                                   # the encoder's type, both ways
    refused(H, "TransformerStateEncoder", fn=F.attn_append)
    refused(H, "torch.nn.modules.rnn.LSTM", enc=torch.nn.LSTM(25, 48).to(cuda))
    refused(H, "cache", cache=None)
    refused(H, "window", enc=wenc)                                             # a cache built for another window
    refused(H, "the cache was built for", cache=KVCache(_make(T_SHAPES[0], cuda)[0], 4, 128))      # ... or another shape
    refused(H, "the cache was built for", fn=F.attn_append, enc=aenc)          # ... or another number of layers
    refused(H, "table", table=tbl.cpu())
    refused(H, "items", items=idx[:, 60:64].cpu())
    refused(H, "ratings", ratings=rts[:, 60:64].cpu())
    refused(H, "table", table=tbl.double())
    refused(H, "items", items=idx[:, 60:64].float())
    refused(H, "ratings", ratings=rts[:, 60:64].double())
    refused(H, "input_size", table=tbl[:, :16].contiguous())
    cpu_kv = copy.copy(cache)
    cpu_kv.kv = cache.kv.cpu()
    refused(H, "cache.kv", cache=cpu_kv)
    refused(ValueError, "ratings", ratings=rts[:, 60:65])
    refused(ValueError, "items", items=idx[0, 60:64])
    refused(ValueError, "n = ", items=idx[:, :0], ratings=rts[:, :0])
    refused(ValueError, "max_append", items=idx[:, :65], ratings=rts[:, :65])
    refused(ValueError, "rows", rows=[0, 1, 1, 2])
    refused(ValueError, "rows", rows=[0, 1, 2, 4])
    refused(ValueError, "rows", rows=[0, 1, -1, 2])
    refused(ValueError, "rows", rows=[0, 1])
    big = KVCache(enc, 4, 128, max_append=128)                                 # no window: 60 + 69 positions do not fit 128
    big.lengths[:] = 60
    with pytest.raises(ValueError, match="capacity"):
        F.transformer_append(enc, big, tbl, idx[:, :69], rts[:, :69])
    assert (big.lengths == 60).all()
    # the cache's own refusals
    for bad, word in ((dict(capacity=100), "capacity"), (dict(capacity=0), "capacity"), (dict(max_append=0), "max_append"),
                      (dict(n_sessions=0), "n_sessions"), (dict(capacity=64, max_append=65), "max_append")):
        with pytest.raises(ValueError, match=word):
            KVCache(enc, **dict(dict(n_sessions=4, capacity=128), **bad))
    with pytest.raises(ValueError, match="min_capacity"):
        KVCache(wenc, 4, KVCache.min_capacity(5, 64) - 64)
    KVCache(wenc, 4, KVCache.min_capacity(5, 64))
    # and the call still works afterwards, from the untouched state
    h2 = F.transformer_append(enc, cache, tbl, idx[:, 60:64], rts[:, 60:64])
    assert (cache.lengths == 64).all() and bool(torch.isfinite(h2).all())


# ---------------------------------------------------------------------------------------------------- 9. the session wrapper
def test_encoder_session_serves_states(cuda, seq_data, gpu_data):
    import recnn_amd
    from recnn_amd import _lib as L
    from recnn_amd.nn import EncoderSession, functional as F
    shape, T, U = T_SHAPES[2], 70, 5
    E, H = shape[0], shape[1]
    st, tbl = gpu_data[E]
    enc, _, _ = _make(shape, cuda)
    idx, rts = _inputs(seq_data, E, range(U), T, cuda)
    ses = EncoderSession(enc, tbl, U, 128)
    with pytest.raises(ValueError, match="nothing has been appended"):
        ses.state()
    ses.append(idx[:, :64], rts[:, :64])
    for t in range(64, T):
        ses.append(idx[:, t:t + 1], rts[:, t:t + 1])
    want = F.state_encode(enc, st, tbl, list(range(U)), T)[:, -1]
    assert _same_bits(ses.state(), want) and _same_bits(ses.state([3, 1]), want[[3, 1]])
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3)
        actor = recnn_amd.nn.Actor(H, 128, 64).to(cuda)
        critic = recnn_amd.nn.Critic(H, 128, 64).to(cuda)
    policy = recnn_amd.nn.WolpertingerPolicy(actor, critic, tbl, n_candidates=64)
    q, ids = policy.recommend(ses.state(), 10)
    q2, ids2 = policy.recommend(want, 10)
    assert tuple(ids.shape) == (U, 10) and torch.equal(ids, ids2) and _same_bits(q, q2)
    ses.reset([1])
    assert list(ses.cache.lengths) == [T, 0, T, T, T]
    h = ses.append(idx[3:4, :5], rts[3:4, :5], [1])
    assert _same_bits(h, F.state_encode(enc, st, tbl, [3], 5)) and _same_bits(ses.state([1]), h[:, -1])
    # the attention encoder goes through the same wrapper; a recurrent encoder is refused by name
    aenc, encode, _ = _make(A_SHAPES[0], cuda)
    ast, atbl = gpu_data[A_SHAPES[0][0]]
    aidx, arts = _inputs(seq_data, A_SHAPES[0][0], range(2), 9, cuda)
    ases = EncoderSession(aenc, atbl, 2, 64)
    ases.append(aidx, arts)
    assert _same_bits(ases.state(), encode(aenc, ast, atbl, [0, 1], 9)[:, -1])
    with pytest.raises(L.RecnnHipError, match="torch.nn.modules.rnn.LSTM.*lstm_encode / gru_encode"):
        EncoderSession(torch.nn.LSTM(E + 1, H).to(cuda), tbl, U, 128)
