"""GPU: the catalogue ranked by the critic's Q-value (csrc/qrank.hip, csrc/scoresel.hip): CriticIndex,
topk_of_scores and rank_in_scores against tests/critic_index_reference.py.

Ids, ranks and the integer-data values are compared without a tolerance.  The real-valued values are held to 8 x the error of a plain
float32 evaluation of the same formula with torch on the CPU, both against float64 (the issue's bound: two fp32 contractions of the
same lengths that differ in summation order only).  Measured on an MI355X, max-norm error over max |Q|, kernel / float32 torch /
ratio: (S, H) = (1290, 256): 9.1e-07 / 4.7e-07 / 1.95;  (50, 64): 3.0e-07 / 3.2e-07 / 0.94;  (50, 24): 3.6e-07 / 3.6e-07 / 1.00."""
import numpy as np
import pytest
import torch

import critic_index_reference as R
import ranking_eval_reference as E
from helpers import make_store

pytestmark = pytest.mark.gpu

A = 128
INT_SHAPES = [(1, 1), (3, 200), (5, 129), (33, 1000)]


@pytest.fixture(scope="module")
def RT(cuda):
    from recnn_amd import retrieval
    return retrieval


def _critic(S, H, cuda, params=None):
    import recnn_amd
    c = recnn_amd.nn.Critic(S, A, H)
    if params is not None:
        with torch.no_grad():
            for p, v in zip((c.linear1.weight, c.linear1.bias, c.linear2.weight, c.linear2.bias, c.linear3.weight, c.linear3.bias),
                            params):
                p.copy_(torch.as_tensor(v, dtype=torch.float32))
    return c.to(cuda)


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _targets(B, N, seed):
    """Target vectors of length B that together hold ids 0, N - 1, 63 / 64 and 127 / 128 where they exist, the rest random."""
    rng = np.random.default_rng(seed)
    special = sorted({i for i in (0, N - 1, 63, 64, 127, 128) if i < N})
    return [np.array(special[o:o + B] + rng.integers(0, N, size=B - len(special[o:o + B])).tolist(), dtype=np.int64)
            for o in range(0, len(special), B)]


def _lists(B, N, seed, longest=30):
    """One exclusion list per row: ids 0, 63, 64, 127, 128, N - 1 where they exist, random ids, a duplicate, ids out of range."""
    rng = np.random.default_rng(seed)
    special = [i for i in (0, 63, 64, 127, 128, N - 1) if i < N]
    out = []
    for _ in range(B):
        ids = special + rng.integers(0, N, size=int(rng.integers(0, longest + 1))).tolist()
        ids = ids + [ids[0], -1, N, 2 ** 31 + 5]
        out.append([ids[i] for i in rng.permutation(len(ids))])
    return out


# ---------------------------------------------------------------- integer data: exact values, and the order under heavy ties

@pytest.fixture(scope="module")
def int_case(cuda):
    """S = 50, H = 256, everything drawn from {-1, 0, 1}, for the largest shape; the smaller shapes are its leading rows."""
    S, H, B, N = 50, 256, 33, 1000
    rng = np.random.default_rng(11)
    draw = lambda *sh: rng.integers(-1, 2, size=sh)
    state, table = draw(B, S), draw(N, A)
    params = (draw(H, S + A), draw(H), draw(H, H), draw(H), draw(1, H), draw(1))
    q, bound = R.q_values_int(state, table, *params)
    # every partial sum of every order is an integer below 2^24: each fp32 operation is exact
    assert bound <= 256 * (256 * 179 + 1) + 1 < 2 ** 24
    return {"S": S, "H": H, "state": state, "table": table, "params": params, "q": q, "critic": _critic(S, H, cuda, params)}


@pytest.mark.parametrize("B,N", INT_SHAPES)
def test_integer_data_is_exact_and_pins_search_and_rank_of(RT, cuda, int_case, B, N):
    c = int_case
    state = torch.from_numpy(c["state"][:B]).float().to(cuda)
    index = RT.CriticIndex(c["critic"], torch.from_numpy(c["table"][:N]).float().to(cuda))
    want = c["q"][:B, :N]
    got = index.q_values(state)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, N)
    assert np.array_equal(got.cpu().numpy().astype(np.float64), want.astype(np.float64))
    assert len(np.unique(want)) < want.size or want.size == 1          # the data ties (where there is more than one value)
    for k in (1, 10, 64):
        q, ids = index.search(state, k)
        wv, wi = R.topk(want, k)
        assert ids.dtype == torch.int64 and np.array_equal(ids.cpu().numpy(), wi)
        assert np.array_equal(q.cpu().numpy().astype(np.float64), wv)
    for t in _targets(B, N, seed=B + N):
        r = index.rank_of(state, torch.from_numpy(t))
        assert r.dtype == torch.int32 and np.array_equal(r.cpu().numpy(), R.ranks(want, t))


# ---------------------------------------------------------------- real-valued data against float64

@pytest.mark.parametrize("S,H", [(1290, 256), (50, 64), (50, 24)])
def test_real_data_within_eight_times_a_float32_evaluation(RT, cuda, S, H):
    B, N = 33, 1000
    g = torch.Generator().manual_seed(S + H)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    state, table = rn(B, S), rn(N, A)
    params = (rn(H, S + A) / (S + A) ** 0.5, rn(H) / (S + A) ** 0.5, rn(H, H) / H ** 0.5, rn(H) / H ** 0.5, rn(1, H) / H ** 0.5,
              rn(1) / H ** 0.5)
    ref = R.q_values(state.numpy(), table.numpy(), *(p.numpy() for p in params))
    w1, b1, w2, b2, w3, b3 = params
    h1 = torch.relu((state @ w1[:, :S].T + b1)[:, None, :] + (table @ w1[:, S:].T)[None])       # plain float32, torch on the CPU
    plain = (torch.relu(h1 @ w2.T + b2) @ w3[0] + b3).numpy()
    assert plain.dtype == np.float32
    got = RT.CriticIndex(_critic(S, H, cuda, params), table.to(cuda)).q_values(state.to(cuda)).cpu().numpy()
    scale = np.abs(ref).max()
    e_kernel, e_plain = np.abs(got - ref).max() / scale, np.abs(plain - ref).max() / scale
    print(f"(S, H) = ({S}, {H}): kernel {e_kernel:.3e}, float32 torch {e_plain:.3e}, ratio {e_kernel / e_plain:.2f}")
    assert e_plain > 0 and e_kernel <= 8 * e_plain


# ---------------------------------------------------------------- position independence

def test_a_pair_has_the_same_bits_wherever_it_sits(RT, cuda):
    S, H, N = 1290, 256, 1000
    g = torch.Generator().manual_seed(5)
    state = torch.randn(130, S, generator=g).to(cuda)
    low = torch.randn(N // 2, A, generator=g)
    table = torch.cat([low, low]).to(cuda)                            # rows [low; low]: every item has a twin N / 2 further on
    critic = _critic(S, H, cuda)
    with torch.no_grad():
        critic.linear3.weight.mul_(1e4)                               # (the initial last layer is tiny; any scale will do)
    index = RT.CriticIndex(critic, table)
    blocked = RT.CriticIndex(critic, table, max_workspace_bytes=32 * N * 4)
    assert blocked.block_rows == 32 and index.block_rows >= 130
    rng = np.random.default_rng(5)
    targets = torch.from_numpy(rng.integers(0, N, size=130))
    full = {"q": index.q_values(state), "ids": index.search(state, 10)[1], "rank": index.rank_of(state, targets)}
    for row in (0, 17, 129):
        for rows, ix in ((slice(row, row + 1), index), (slice(row, row + 1), blocked), (slice(0, 33) if row < 33 else None, index),
                         (slice(0, 130), blocked)):
            if rows is None:
                continue
            r = row - rows.start
            assert np.array_equal(_bits(ix.q_values(state[rows])[r]), _bits(full["q"][row]))
            assert torch.equal(ix.search(state[rows], 10)[1][r], full["ids"][row])
            assert int(ix.rank_of(state[rows], targets[rows])[r]) == int(full["rank"][row])
    # twins have equal bits, so the upper one ranks exactly one after the lower one
    q = full["q"]
    assert np.array_equal(_bits(q[:, :N // 2]), _bits(q[:, N // 2:]))
    lower = torch.from_numpy(rng.integers(0, N // 2, size=130))
    assert torch.equal(index.rank_of(state, lower + N // 2), index.rank_of(state, lower) + 1)
    assert torch.equal(blocked.rank_of(state, lower + N // 2), index.rank_of(state, lower) + 1)


# ---------------------------------------------------------------- search / rank_of against the selection from q_values

@pytest.fixture(scope="module")
def real_case(RT, cuda):
    S, H, B, N = 50, 24, 33, 1000
    g = torch.Generator().manual_seed(9)
    critic = _critic(S, H, cuda)
    with torch.no_grad():
        critic.linear3.weight.mul_(1e4)
    index = RT.CriticIndex(critic, torch.randn(N, A, generator=g).to(cuda))
    state = torch.randn(B, S, generator=g).to(cuda)
    return {"index": index, "critic": critic, "state": state, "q": index.q_values(state), "B": B, "N": N}


def test_search_and_rank_of_are_the_selection_from_q_values(RT, cuda, real_case):
    c = real_case
    index, state, q, B, N = c["index"], c["state"], c["q"], c["B"], c["N"]
    ex = RT.SeenItems.from_lists(_lists(B, N, seed=3), device=cuda)
    for exclude in (None, ex):
        for k in (1, 10, 64):
            v, ids = index.search(state, k, exclude=exclude)
            sv, sids = RT.topk_of_scores(q, k, exclude=exclude)
            assert torch.equal(ids, sids) and np.array_equal(_bits(v), _bits(sv))
        t = torch.from_numpy(_targets(B, N, seed=1)[0])
        assert torch.equal(index.rank_of(state, t, exclude=exclude), RT.rank_in_scores(q, t, exclude=exclude))
        v, ids = index.search(state, 64, exclude=exclude)
        for j in (0, 1, 9, 63):                                       # the item at position j has rank j
            assert index.rank_of(state, ids[:, j], exclude=exclude).tolist() == [j] * B
        assert np.array_equal(_bits(v), _bits(torch.gather(q, 1, ids)))   # and the reported value is the matrix entry


# ---------------------------------------------------------------- the selection kernels on their own

def _planted(B, N, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((B, N)).astype(np.float32)
    s[rng.random((B, N)) < 0.3] = 1.5                                  # ties
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    hit = rng.random((B, N)) < 0.05 if N > 1 else np.ones((B, N), dtype=bool)
    s[hit] = special[rng.integers(0, 5, size=int(hit.sum()))]
    if B > 2:
        s[1] = np.nan                                                  # constant rows: order by id
        s[2] = 0.0
        s[2, ::3] = -0.0
        s[3] = -np.inf
        s[4] = 7.25
    return s


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 129, 1000, 70_001])
def test_selection_from_a_score_matrix_is_exact(RT, cuda, B, N):
    s = _planted(B, N, seed=B * 100_003 + N)
    wide = torch.full((B, N + 37), float("nan"), device=cuda)          # a non-contiguous row stride
    wide[:, :N] = torch.from_numpy(s).to(cuda)
    wv64, wi64 = R.topk(s, 64)                                         # the first k of the first 64
    for scores in (torch.from_numpy(s).to(cuda), wide[:, :N]):
        for k in (1, 10, 64):                                          # k > N where N is small
            v, ids = RT.topk_of_scores(scores, k)
            wv, wi = wv64[:, :k], wi64[:, :k]
            assert tuple(ids.shape) == (B, k) and np.array_equal(ids.cpu().numpy(), wi)
            assert np.array_equal(v.cpu().numpy().astype(np.float64), wv, equal_nan=True)
        for t in _targets(B, N, seed=N) + [np.array(([-1, N, 2 ** 31 + 5, -2 ** 40] * B)[:B], dtype=np.int64)]:
            r = RT.rank_in_scores(scores, torch.from_numpy(t))
            assert r.dtype == torch.int32 and np.array_equal(r.cpu().numpy(), R.ranks(s, t))
    assert not scores.is_contiguous() or B == 1


@pytest.mark.parametrize("B,N", [(1, 1), (5, 129), (33, 1000), (33, 70_001)])
def test_selection_with_exclusion(RT, cuda, B, N):
    s = _planted(B, N, seed=B + N)
    lists = _lists(B, N, seed=N)
    if N >= 129:
        lists[0] = [i for i in range(N) if i % 40 != 7][: N - 3] if N < 2000 else lists[0]     # a short row: at most a few items left
    scores = torch.from_numpy(s).to(cuda)
    ex = RT.SeenItems.from_lists(lists, device=cuda)
    wv64, wi64 = R.topk(s, 64, lists)
    for exclude in (ex, ex.mask(N)):
        for k in (1, 10, 64):
            v, ids = RT.topk_of_scores(scores, k, exclude=exclude)
            wv, wi = wv64[:, :k], wi64[:, :k]
            assert np.array_equal(ids.cpu().numpy(), wi) and np.array_equal(v.cpu().numpy().astype(np.float64), wv, equal_nan=True)
            for b in range(B):                                         # excluded items never appear; short rows end in -1 / -inf
                assert not set(ids[b].tolist()) & {i for i in lists[b] if 0 <= i < N}
        for t in _targets(B, N, seed=N + 1):
            assert np.array_equal(RT.rank_in_scores(scores, torch.from_numpy(t), exclude=exclude).cpu().numpy(), R.ranks(s, t, lists))
        t = np.array([lists[b][0] if 0 <= lists[b][0] < N else 0 for b in range(B)], dtype=np.int64)   # excluded targets are still ranked
        assert np.array_equal(RT.rank_in_scores(scores, torch.from_numpy(t), exclude=exclude).cpu().numpy(), R.ranks(s, t, lists))
    if N == 1000:
        left = N - len({i for i in lists[0] if 0 <= i < N})
        v, ids = RT.topk_of_scores(scores, 64, exclude=ex)
        assert 0 < left < 64 and (ids[0, left:] == -1).all() and torch.isneginf(v[0, left:]).all() and (ids[0, :left] >= 0).all()


def test_refusals(RT, cuda, real_case):
    c = real_case
    index, state, q, B, N = c["index"], c["state"], c["q"], c["B"], c["N"]
    good = RT.SeenItems.from_lists([[1]] * B, device=cuda)
    other_rows = RT.SeenItems.from_lists([[1]] * (B + 1), device=cuda)
    other_n = good.mask(N + 64)
    t = torch.zeros(B, dtype=torch.int64)
    for bad in (other_rows, other_n):
        for call in (lambda: index.search(state, 5, exclude=bad), lambda: index.rank_of(state, t, exclude=bad),
                     lambda: RT.topk_of_scores(q, 5, exclude=bad), lambda: RT.rank_in_scores(q, t, exclude=bad)):
            with pytest.raises(ValueError, match="exclusion"):
                call()
    with pytest.raises(TypeError, match="SeenItems"):
        index.search(state, 5, exclude=[[1]] * B)
    for k in (0, 65, 2.5):
        with pytest.raises(ValueError, match="k must be"):
            index.search(state, k)
        with pytest.raises(ValueError, match="k must be"):
            RT.topk_of_scores(q, k)
    with pytest.raises(ValueError, match="targets"):
        index.rank_of(state, torch.zeros(B + 1, dtype=torch.int64))
    with pytest.raises(ValueError, match="targets"):
        RT.rank_in_scores(q, torch.zeros(B))
    with pytest.raises(ValueError, match=r"\[B, 50\]"):
        index.q_values(state[:, :40])
    with pytest.raises(ValueError, match="scores must be"):
        RT.topk_of_scores(q[0], 3)
    from recnn_amd import _lib as L
    for call in (lambda: index.q_values(state.cpu()), lambda: index.search(state.cpu()), lambda: index.rank_of(state.cpu(), t)):
        with pytest.raises(L.RecnnHipError):
            call()
    # an empty batch returns empty tensors
    e = state[:0]
    assert tuple(index.q_values(e).shape) == (0, N)
    v, ids = index.search(e, 7)
    assert tuple(v.shape) == (0, 7) and tuple(ids.shape) == (0, 7) and ids.dtype == torch.int64
    assert tuple(index.rank_of(e, t[:0]).shape) == (0,)
    v, ids = RT.topk_of_scores(q[:0], 7)
    assert tuple(v.shape) == (0, 7) and tuple(RT.rank_in_scores(q[:0], t[:0]).shape) == (0,)


def test_refresh_rereads_the_weights(RT, cuda, real_case):
    c = real_case
    index, critic, state, q = c["index"], c["critic"], c["state"], c["q"]
    saved = [p.detach().clone() for p in critic.parameters()]
    try:
        with torch.no_grad():
            for p in critic.parameters():
                p.add_(0.01)
        assert np.array_equal(_bits(index.q_values(state)), _bits(q))      # the snapshot, not the module
        index.refresh()
        moved = index.q_values(state)
        assert not np.array_equal(_bits(moved), _bits(q))
        w = [p.detach().cpu().numpy() for p in critic.parameters()]
        ref = R.q_values(state.cpu().numpy(), index.table.cpu().numpy(), *w)
        assert np.abs(moved.cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()
    finally:
        with torch.no_grad():
            for p, s in zip(critic.parameters(), saved):
                p.copy_(s)
        index.refresh()
    assert np.array_equal(_bits(index.q_values(state)), _bits(q))


# ---------------------------------------------------------------- the whole path once

def test_frame_env_critic_and_policy_ranks_feed_the_meter(RT, cuda):
    from recnn_amd.data.env import FrameEnv
    n_users, n_items, F = 12, 500, 10
    items, ratings, table = make_store(n_users=n_users, n_items=n_items, emb_dim=128, min_len=25, max_len=40, seed=6)
    user_dict = {100 + 3 * u: {"items": items[u], "ratings": ratings[u]} for u in range(n_users)}
    ids = list(user_dict)
    env = FrameEnv.from_user_dict(torch.from_numpy(table), user_dict, ids[:6], ids[6:], frame_size=F, batch_size=4, device=cuda)
    critic = _critic(1290, 256, cuda)
    with torch.no_grad():
        critic.linear3.weight.mul_(1e4)
    index = RT.CriticIndex(critic, env.table)
    batch = env.test_batch()
    state, targets, seen = batch["state"], env.target_items(batch), env.seen_items(batch)
    ranks = index.rank_of(state, targets, exclude=seen)
    # the reference order over the values the index reports (their accuracy is the subject of the tests above)
    st, ln = seen.starts.cpu().numpy(), seen.lengths.cpu().numpy()
    store_items = env.store.items.cpu().numpy()
    tg = targets.cpu().numpy()
    lists = [[i for i in store_items[s:s + n].tolist() if i != tg[b]] for b, (s, n) in enumerate(zip(st, ln))]
    want = R.ranks(index.q_values(state).cpu().numpy(), tg, lists)
    assert np.array_equal(ranks.cpu().numpy(), want) and (want >= 0).all()
    ks = (1, 5, 10, 50)
    # a DiscreteActor-shaped matrix: one probability per (row, item)
    probs = torch.softmax(torch.randn(state.shape[0], n_items, generator=torch.Generator().manual_seed(2)), 1).to(cuda)
    policy_ranks = RT.rank_in_scores(probs, targets, exclude=seen)
    policy_want = R.ranks(probs.cpu().numpy(), tg, lists)
    assert np.array_equal(policy_ranks.cpu().numpy(), policy_want)
    for got, ref_ranks in ((ranks, want), (policy_ranks, policy_want)):
        meter = RT.RankingMeter(ks, device=cuda)
        meter.update(got)
        ref = E.meter_reference(ref_ranks, None, ks)
        assert meter.rows == ref["rows"] and meter.hits() == ref["hits"]
        for k in ks:
            assert abs(meter.ndcg()[k] - ref["ndcg"][k]) <= 1e-12 and abs(meter.hit_rate()[k] - ref["hit_rate"][k]) <= 1e-12
        assert abs(meter.mrr - ref["mrr"]) <= 1e-12 and abs(meter.mean_rank - ref["mean_rank"]) <= 1e-12
