"""GPU: two-stage recommendation (csrc/qcand.hip): CriticIndex.q_of / rerank, TwoStageIndex and
WolpertingerPolicy against tests/two_stage_reference.py and against the whole-catalogue CriticIndex.

Every comparison is exact: values as bit patterns (or as integers on the integer data), ids and ranks as integers."""
import numpy as np
import pytest
import torch

import critic_index_reference as R
import ranking_eval_reference as E
import two_stage_reference as T
from helpers import make_store

pytestmark = pytest.mark.gpu

A = 128
N = 1000
KS = (1, 15, 16, 17, 64, 65, 130)


@pytest.fixture(scope="module")
def RT(cuda):
    from recnn_amd import retrieval
    return retrieval


def _critic(S, H, cuda, params=None, scale3=None):
    import recnn_amd
    c = recnn_amd.nn.Critic(S, A, H)
    with torch.no_grad():
        if params is not None:
            for p, v in zip((c.linear1.weight, c.linear1.bias, c.linear2.weight, c.linear2.bias, c.linear3.weight, c.linear3.bias),
                            params):
                p.copy_(torch.as_tensor(v, dtype=torch.float32))
        if scale3 is not None:
            c.linear3.weight.mul_(scale3)                               # (the initial last layer is tiny; any scale will do)
    return c.to(cuda)


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _ids(rng, B, K, empties=True):
    """Random ids with repeats; about one slot in eight holds -1, N or N + 5."""
    ids = rng.integers(0, N, size=(B, K))
    ids[:, K // 2:] = np.where(rng.random((B, K - K // 2)) < 0.5, ids[:, :1], ids[:, K // 2:])       # repeats of the row's first id
    if empties:
        hit = rng.random((B, K)) < 0.125
        hit[0, K - 1] = True                                            # at least one, also at K = 1
        ids[hit] = np.array([-1, N, N + 5])[rng.integers(0, 3, size=int(hit.sum()))]
    return ids


# ---------------------------------------------------------------- 1. the bits of the whole-catalogue kernel

@pytest.fixture(scope="module", params=[(50, 24), (50, 64), (1290, 256)], ids=lambda p: f"S{p[0]}-H{p[1]}")
def real_case(request, RT, cuda):
    S, H = request.param
    g = torch.Generator().manual_seed(S + H)
    index = RT.CriticIndex(_critic(S, H, cuda, scale3=1e4), torch.randn(N, A, generator=g).to(cuda))
    state = torch.randn(33, S, generator=g).to(cuda)
    return {"index": index, "state": state, "q": index.q_values(state), "S": S, "H": H}


@pytest.mark.parametrize("B", [1, 5, 33])
def test_q_of_has_the_bits_of_q_values(RT, cuda, real_case, B):
    c = real_case
    index, state, full = c["index"], c["state"][:B], c["q"][:B]
    rng = np.random.default_rng(B)
    for K in KS:
        ids = _ids(rng, B, K)
        ok = (ids >= 0) & (ids < N)
        assert (~ok).any()
        want = torch.gather(full, 1, torch.from_numpy(np.where(ok, ids, 0)).to(cuda))
        want = torch.where(torch.from_numpy(ok).to(cuda), want, torch.full_like(want, float("-inf")))
        for dtype in (torch.int32, torch.int64):
            t = torch.from_numpy(ids).to(cuda, dtype)
            wide = torch.full((B, K + 7), 3, dtype=dtype, device=cuda)
            wide[:, 3:3 + K] = t
            for arg in (t, wide[:, 3:3 + K]):
                got = index.q_of(state, arg)
                assert got.dtype == torch.float32 and tuple(got.shape) == (B, K)
                assert np.array_equal(_bits(got), _bits(want)), (K, dtype)
        assert torch.isneginf(got[torch.from_numpy(~ok).to(cuda)]).all()
        # row 0 alone and inside the batch
        alone = index.q_of(c["state"][:1], torch.from_numpy(ids[:1]).to(cuda))
        assert np.array_equal(_bits(alone[0]), _bits(got[0]))
        if K <= 64:                                                       # and the sorted form reports the same bits
            v, sid = index.rerank(state, t)
            filled = sid >= 0
            assert np.array_equal(_bits(v[filled]), _bits(torch.gather(full, 1, sid.clamp_min(0))[filled]))


# ---------------------------------------------------------------- 2. integer data: exact values, ties

@pytest.fixture(scope="module")
def int_case(cuda):
    """DESIGN.md section 22's construction: S = 50, H = 256, everything drawn from {-1, 0, 1}."""
    S, H, B = 50, 256, 33
    rng = np.random.default_rng(11)
    draw = lambda *sh: rng.integers(-1, 2, size=sh)
    state, table = draw(B, S), draw(N, A)
    params = (draw(H, S + A), draw(H), draw(H, H), draw(H), draw(1, H), draw(1))
    q, bound = R.q_values_int(state, table, *params)
    assert bound <= 256 * (256 * 179 + 1) + 1 < 2 ** 24          # every partial sum of every order: each fp32 operation is exact
    return {"state": state, "table": table, "q": q, "critic": _critic(S, H, cuda, params)}


@pytest.mark.parametrize("K", [1, 16, 17, 64])
def test_integer_data_is_exact_and_pins_the_tie_rules(RT, cuda, int_case, K):
    c = int_case
    index = RT.CriticIndex(c["critic"], torch.from_numpy(c["table"]).float().to(cuda))
    state = torch.from_numpy(c["state"]).float().to(cuda)
    rng = np.random.default_rng(K)
    ids = _ids(rng, 33, K, empties=K > 1)
    want = T.q_of(c["q"], ids)
    t = torch.from_numpy(ids).to(cuda)
    got = index.q_of(state, t)
    assert np.array_equal(got.cpu().numpy().astype(np.float64), want)
    if K > 1:
        filled = want[np.isfinite(want)]
        assert len(np.unique(filled)) < filled.size                      # the data ties
        assert any(len(set(r[r >= 0].tolist())) < (r >= 0).sum() for r in ids)       # and ids repeat within a row
    for k in sorted({1, min(10, K), K}):
        v, sid = index.rerank(state, t, k)
        wv, wi = T.rerank(want, ids, N, k)
        assert sid.dtype == torch.int64 and tuple(sid.shape) == (33, k) and np.array_equal(sid.cpu().numpy(), wi)
        assert np.array_equal(v.cpu().numpy().astype(np.float64), wv)
    g = np.where(ids[:, 0] >= 0, ids[:, 0], 5)                           # the row's first id is repeated further on
    pos = index.rerank(state, t, 1, torch.from_numpy(g))[2]
    assert pos.dtype == torch.int32 and np.array_equal(pos.cpu().numpy(), T.pos(want, ids, N, g))


# ---------------------------------------------------------------- 3. the sort is the stated order; +inf and NaN through the data

def _plain_f32(state, table, params):
    """The formula in plain float32 with torch on the CPU."""
    w1, b1, w2, b2, w3, b3 = (torch.as_tensor(p, dtype=torch.float32) for p in params)
    S = state.shape[1]
    h1 = torch.relu((state @ w1[:, :S].T + b1)[:, None, :] + (table @ w1[:, S:].T)[None])
    return torch.relu(h1 @ w2.T + b2) @ w3[0] + b3


@pytest.fixture(scope="module", params=["inf", "nan"])
def planted_case(request, RT, cuda):
    S, H, B, hot = 50, 24, 33, 7
    g = torch.Generator().manual_seed(21)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    state, table = rn(B, S), rn(N, A)
    table[hot] *= 1e30                                                   # E1[hot] ~ 1e30: layer 2 reaches ~1e36, the head's products overflow
    w3 = rn(1, H).abs() * 1e4 + 1.0
    if request.param == "nan":
        w3[0, ::2] *= -1.0                                               # +inf and -inf meet in the head's sum
    params = (rn(H, S + A) * 0.1, rn(H) * 0.1, rn(H, H).abs() * 1e5 + 1.0, rn(H).abs(), w3, rn(1))
    plain = _plain_f32(state, table, params)
    special = torch.isposinf if request.param == "inf" else torch.isnan
    assert special(plain[:, hot]).all() and torch.isfinite(plain[:, :hot]).all() and torch.isfinite(plain[:, hot + 1:]).all()
    index = RT.CriticIndex(_critic(S, H, cuda, [p.numpy() for p in params]), table.to(cuda))
    return {"index": index, "state": state.to(cuda), "hot": hot, "special": special, "B": B}


@pytest.mark.parametrize("K", [1, 17, 64])
def test_rerank_is_the_stated_order_of_q_of(RT, cuda, planted_case, K):
    c = planted_case
    index, state, hot, B = c["index"], c["state"], c["hot"], c["B"]
    rng = np.random.default_rng(K + 100)
    ids = _ids(rng, B, K)
    ids[1] = np.array([-1, N, N + 5])[rng.integers(0, 3, size=K)]       # a row that is all empty
    ids[2] = -1
    ids[2, K // 3] = 123                                                 # one non-empty slot
    ids[3, K // 4: K // 2] = N                                           # empty slots in the middle
    for b in range(4, B, 3):                                             # the planted item, some rows twice
        ids[b, rng.integers(0, K)] = hot
        ids[b, rng.integers(0, K)] = hot
    t = torch.from_numpy(ids).to(cuda)
    q = index.q_of(state, t)
    at_hot = torch.from_numpy(ids == hot).to(cuda)
    assert at_hot.any() and c["special"](q[at_hot]).all() and torch.isfinite(q[~at_hot & (t >= 0) & (t < N)]).all()
    qn = q.cpu().numpy()
    for k in sorted({1, min(10, K), K}):
        for arg in (t, t.to(torch.int32)):
            v, sid = index.rerank(state, arg, k)
            wv, wi = T.rerank(qn, ids, N, k)
            assert np.array_equal(sid.cpu().numpy(), wi)
            assert np.array_equal(_bits(v), wv.astype(np.float32).view(np.int32))       # the GPU's own values, bit for bit
    v, sid = index.rerank(state, t)                                      # k defaults to K
    assert tuple(sid.shape) == (B, K) and (sid[1] == -1).all() and torch.isneginf(v[1]).all()
    assert sid[2].tolist() == [123] + [-1] * (K - 1) and torch.isneginf(v[2, 1:]).all()
    # pos: the first slot's id, the last slot's id, a repeated id (the row's first id), absent, out of range
    absent = np.array([next(i for i in range(N) if i not in set(ids[b].tolist())) for b in range(B)])
    twice = np.array([next((i for i in r.tolist() if (r == i).sum() > 1), r[0]) for r in ids])
    for g in (ids[:, 0], ids[:, K - 1], twice, absent,
              np.array(([-1, N, 2 ** 31 + 5, -2 ** 40] * B)[:B]), np.full(B, hot)):
        out = index.rerank(state, t, 1, torch.from_numpy(np.asarray(g, dtype=np.int64)))
        assert len(out) == 3 and out[2].dtype == torch.int32
        assert np.array_equal(out[2].cpu().numpy(), T.pos(qn, ids, N, g))
    assert (index.rerank(state, t, 1, torch.from_numpy(absent))[2] == -1).all()


# ---------------------------------------------------------------- 4. two-stage identities

@pytest.fixture(scope="module")
def small_case(RT, cuda):
    S, H, B = 50, 24, 33
    g = torch.Generator().manual_seed(31)
    return {"critic": _critic(S, H, cuda, scale3=1e4), "table": torch.randn(N, A, generator=g).to(cuda),
            "state": torch.randn(B, S, generator=g).to(cuda), "action": torch.randn(B, A, generator=g).to(cuda), "B": B}


@pytest.mark.parametrize("metric", ["L2", "IP"])
@pytest.mark.parametrize("n", [1, 40, 64])
def test_candidates_that_are_the_whole_catalogue_give_the_critic_index(RT, cuda, small_case, n, metric):
    c = small_case
    state, action, B = c["state"], c["action"], c["B"]
    critic_index = RT.CriticIndex(c["critic"], c["table"][:n])
    two = RT.TwoStageIndex(RT.FlatIndex(c["table"][:n], metric), critic_index, n_candidates=n)
    for k in sorted({1, min(10, n), n}):
        q, ids = two.search(action, state, k)
        wq, wi = critic_index.search(state, k)
        assert torch.equal(ids, wi) and np.array_equal(_bits(q), _bits(wq))
    rng = np.random.default_rng(n)
    for t in (rng.integers(0, n, size=B), np.array(([-1, n, 2 ** 31 + 5, 0] * B)[:B])):
        t = torch.from_numpy(t)
        r = two.rank_of(action, state, t)
        assert r.dtype == torch.int32 and torch.equal(r, critic_index.rank_of(state, t))


def test_the_whole_catalogue_reached_through_exclusion(RT, cuda, small_case):
    c = small_case
    left = [0, 1, 30, 64, 64, 30, 1, 0]
    B = len(left)
    state, action = c["state"][:B], c["action"][:B]
    rng = np.random.default_rng(4)
    keep = [sorted(rng.choice(N, size=n, replace=False).tolist()) for n in left]
    lists = [[i for i in range(N) if i not in set(kp)] + [-1, N, 2 ** 31 + 5] for kp in keep]
    ex = RT.SeenItems.from_lists(lists, device=cuda)
    critic_index = RT.CriticIndex(c["critic"], c["table"])
    two = RT.TwoStageIndex(RT.FlatIndex(c["table"], "L2"), critic_index, n_candidates=64)
    for k in (1, 10, 64):
        q, ids = two.search(action, state, k, exclude=ex)
        wq, wi = critic_index.search(state, k, exclude=ex)
        assert torch.equal(ids, wi) and np.array_equal(_bits(q), _bits(wq))
        for b, n in enumerate(left):
            assert (ids[b, :min(n, k)] >= 0).all() and (ids[b, n:] == -1).all() and torch.isneginf(q[b, n:]).all()
            assert set(ids[b, :min(n, k)].tolist()) <= set(keep[b])
    rows = [b for b, n in enumerate(left) if n]
    t = torch.tensor([keep[b][-1] if keep[b] else 0 for b in range(B)])
    got, want = two.rank_of(action, state, t, exclude=ex), critic_index.rank_of(state, t, exclude=ex)
    assert torch.equal(got[rows], want[rows])


def test_rank_of_is_the_position_among_the_candidates_then_the_flat_rank(RT, cuda, small_case):
    c = small_case
    state, action, B = c["state"], c["action"], c["B"]
    flat = RT.FlatIndex(c["table"], "L2")
    two = RT.TwoStageIndex(flat, RT.CriticIndex(c["critic"], c["table"]), n_candidates=64)
    rng = np.random.default_rng(8)
    lists = [rng.integers(0, N, size=int(rng.integers(0, 40))).tolist() + [-1, N] for _ in range(B)]
    for ex in (None, RT.SeenItems.from_lists(lists, device=cuda)):
        q, ids = two.search(action, state, 64, exclude=ex)
        assert (ids >= 0).all()
        cand = flat.search(action, 64, exclude=ex)[1]
        assert torch.equal(ids.sort(1)[0], cand.sort(1)[0])            # the same 64 items, reordered
        assert (q[:, :-1] >= q[:, 1:]).all()
        for j in range(64):
            assert two.rank_of(action, state, ids[:, j], exclude=ex).tolist() == [j] * B
        if ex is not None:
            for b in range(B):
                assert not set(ids[b].tolist()) & set(lists[b])
        inside = [set(r) for r in ids.tolist()]
        gone = [set(l) for l in lists] if ex is not None else [set()] * B
        for _ in range(50):
            t = torch.tensor([next(i for i in rng.permutation(N).tolist() if i not in inside[b] and i not in gone[b])
                              for b in range(B)])
            r = two.rank_of(action, state, t, exclude=ex)
            assert torch.equal(r, flat.rank_of(action, t, exclude=ex)) and (r >= 64).all()


# ---------------------------------------------------------------- 5. the policy

@pytest.fixture(scope="module")
def policy_case(RT, cuda):
    import recnn_amd
    from recnn_amd.data.env import FrameEnv
    n_users, n_items, F = 12, 500, 10
    items, ratings, table = make_store(n_users=n_users, n_items=n_items, emb_dim=128, min_len=25, max_len=40, seed=6)
    user_dict = {100 + 3 * u: {"items": items[u], "ratings": ratings[u]} for u in range(n_users)}
    ids = list(user_dict)
    env = FrameEnv.from_user_dict(torch.from_numpy(table), user_dict, ids[:6], ids[6:], frame_size=F, batch_size=4, device=cuda)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3)
        actor = recnn_amd.nn.Actor(1290, 128, 256).to(cuda)
        critic = _critic(1290, 256, cuda, scale3=1e4)
    policy = recnn_amd.nn.WolpertingerPolicy(actor, critic, env.table, n_candidates=64)
    return {"env": env, "actor": actor, "critic": critic, "policy": policy, "batch": env.test_batch(), "n_items": n_items}


def test_policy_act_is_the_best_candidate_its_row_and_its_value(RT, cuda, policy_case):
    c = policy_case
    policy, actor, critic, state = c["policy"], c["actor"], c["critic"], c["batch"]["state"]
    B = state.shape[0]
    actor.eval()
    ids, actions, q = policy.act(state)
    rq, rids = policy.recommend(state, 1)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (B,) and tuple(actions.shape) == (B, 128) and tuple(q.shape) == (B,)
    assert torch.equal(ids, rids[:, 0]) and np.array_equal(_bits(q), _bits(rq[:, 0])) and (ids >= 0).all()
    assert np.array_equal(_bits(actions), _bits(policy.table[ids]))
    full = policy.critic_index.q_values(state)
    assert np.array_equal(_bits(q), _bits(full.gather(1, ids[:, None])[:, 0]))
    # the best of the 64 items nearest to the actor's eval-mode action
    cand = policy.flat.search(policy.proto_action(state), 64)[1]
    assert torch.equal(q, full.gather(1, cand).max(1)[0])
    actor.train()                                                        # eval semantics whatever the module says
    try:
        ids2, actions2, q2 = policy.act(state)
    finally:
        actor.eval()
    assert torch.equal(ids2, ids) and np.array_equal(_bits(q2), _bits(q)) and np.array_equal(_bits(actions2), _bits(actions))
    # a row with nothing left
    ex = RT.SeenItems.from_lists([list(range(c["n_items"]))] + [[]] * (B - 1), device=cuda)
    ids3, actions3, q3 = policy.act(state, exclude=ex)
    assert int(ids3[0]) == -1 and (actions3[0] == 0).all() and torch.isneginf(q3[0])
    assert torch.equal(ids3[1:], ids[1:]) and np.array_equal(_bits(actions3[1:]), _bits(actions[1:]))
    # refresh() picks up an in-place change of the last layer
    saved = critic.linear3.weight.detach().clone()
    try:
        with torch.no_grad():
            critic.linear3.weight.mul_(-1.0)
        assert np.array_equal(_bits(policy.act(state)[2]), _bits(q))     # the snapshot, not the module
        policy.refresh()
        ids4, _, q4 = policy.act(state)
        assert not np.array_equal(_bits(q4), _bits(q))
        assert np.array_equal(_bits(q4), _bits(policy.critic_index.q_values(state).gather(1, ids4[:, None])[:, 0]))
    finally:
        with torch.no_grad():
            critic.linear3.weight.copy_(saved)
        policy.refresh()
    assert np.array_equal(_bits(policy.act(state)[2]), _bits(q))


def test_frame_env_policy_ranks_feed_the_meter(RT, cuda, policy_case):
    c = policy_case
    env, policy, batch = c["env"], c["policy"], c["batch"]
    n_items = c["n_items"]
    state, targets, seen = batch["state"], env.target_items(batch), env.seen_items(batch)
    ranks = policy.rank_of(state, targets, exclude=seen)
    assert ranks.dtype == torch.int32
    # the reference: positions by the numpy order over the values q_of reports, the rest by the flat index's rank
    proto = policy.proto_action(state)
    cand = policy.flat.search(proto, 64, exclude=seen)[1]
    qn, cn, tg = policy.critic_index.q_of(state, cand).cpu().numpy(), cand.cpu().numpy(), targets.cpu().numpy()
    flat_rank = policy.flat.rank_of(proto, targets, exclude=seen).cpu().numpy()
    want = T.two_stage_rank(T.pos(qn, cn, n_items, tg), flat_rank, (cn >= 0).sum(1))
    assert np.array_equal(ranks.cpu().numpy(), want) and (want >= 0).all()
    ks = (1, 5, 10, 50)
    meter = RT.RankingMeter(ks, device=cuda)
    meter.update(ranks)
    ref = E.meter_reference(want, None, ks)
    assert meter.rows == ref["rows"] and meter.hits() == ref["hits"]
    assert abs(meter.hit_rate()[10] - ref["hit_rate"][10]) <= 1e-12 and abs(meter.ndcg()[10] - ref["ndcg"][10]) <= 1e-12


# ---------------------------------------------------------------- 6. refusals

def test_refusals(RT, cuda, small_case):
    c = small_case
    state, action, B = c["state"], c["action"], c["B"]
    index = RT.CriticIndex(c["critic"], c["table"])
    flat = RT.FlatIndex(c["table"], "L2")
    ids = torch.zeros(B, 10, dtype=torch.int64, device=cuda)
    for call in (index.q_of, index.rerank):
        with pytest.raises(ValueError, match="integer tensor"):
            call(state, ids.float())
        with pytest.raises(ValueError, match="integer tensor"):
            call(state, ids.bool())
        with pytest.raises(ValueError, match="integer tensor"):
            call(state, [[0] * 10] * B)
        with pytest.raises(ValueError, match="live on cpu"):
            call(state, ids.cpu())
        with pytest.raises(ValueError, match=f"{B} states but ids of {B + 1} rows"):
            call(state, torch.zeros(B + 1, 10, dtype=torch.int64, device=cuda))
        with pytest.raises(ValueError, match=r"\[B, K\]"):
            call(state, ids[0])
    with pytest.raises(ValueError, match="at most 64 candidates"):
        index.rerank(state, torch.zeros(B, 65, dtype=torch.int64, device=cuda))
    for k in (0, 11, 2.5, -1):
        with pytest.raises(ValueError, match="k must be an integer from 1 to the 10 candidates"):
            index.rerank(state, ids, k)
    with pytest.raises(ValueError, match="targets"):
        index.rerank(state, ids, 1, torch.zeros(B + 1, dtype=torch.int64))
    with pytest.raises(ValueError, match="targets"):
        index.rerank(state, ids, 1, torch.zeros(B))
    with pytest.raises(ValueError, match="same table"):
        RT.TwoStageIndex(RT.FlatIndex(c["table"][:500], "L2"), index)
    for n in (0, 65):
        with pytest.raises(ValueError, match="n_candidates must be"):
            RT.TwoStageIndex(flat, index, n)
    with pytest.raises(TypeError, match="FlatIndex and a CriticIndex"):
        RT.TwoStageIndex(index, flat)
    two = RT.TwoStageIndex(flat, index, 20)
    with pytest.raises(ValueError, match="k must be an integer from 1 to the 20 candidates"):
        two.search(action, state, 21)
    with pytest.raises(ValueError, match="exclusion"):
        two.search(action, state, 5, exclude=RT.SeenItems.from_lists([[1]] * (B + 1), device=cuda))
    with pytest.raises(ValueError, match="targets"):
        two.rank_of(action, state, torch.zeros(B + 1, dtype=torch.int64))
    # small integer dtypes are widened; an empty batch returns empty tensors
    assert np.array_equal(_bits(index.q_of(state, ids.to(torch.int16))), _bits(index.q_of(state, ids)))
    e = state[:0]
    assert tuple(index.q_of(e, ids[:0]).shape) == (0, 10)
    v, sid = index.rerank(e, ids[:0], 3)
    assert tuple(v.shape) == (0, 3) and tuple(sid.shape) == (0, 3) and sid.dtype == torch.int64
