"""GPU: the rank of a target item under all twelve orders of FlatIndex (csrc/rank.hip, csrc/topk.hip), RankingMeter
(csrc/evalrank.hip) and FrameEnv.target_items, against tests/ranking_eval_reference.py.

The ranks are integers and are compared without a tolerance: against the reference's count on the matrix `cdist` returns (which is
bit-equal to what `search` reports), against an int64 reference on integer-valued data for IP / L2, and against `search` itself.
Only RankingMeter's float64 sums carry a bound: 1e-12 relative, for at most a few thousand terms of magnitude <= 1."""
import numpy as np
import pytest
import torch

import ranking_eval_reference as R
from helpers import make_store

pytestmark = pytest.mark.gpu

SCIPY_CASES = [("sqeuclidean", None), ("euclidean", None), ("cityblock", None), ("chebyshev", None), ("minkowski", None),
               ("canberra", None), ("braycurtis", None), ("cosine", None), ("correlation", None), ("minkowski", 3.0)]
SHAPES = [(1, 1), (3, 200), (5, 129), (33, 1000)]


@pytest.fixture(scope="module")
def RT(cuda):
    from recnn_amd import retrieval
    return retrieval


def _normal(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 128, generator=g), torch.randn(N, 128, generator=g)


def _target_sets(B, N, seed):
    """Target vectors of length B that together hold ids 0, N - 1, 63 / 64 and 127 / 128 where they exist, the rest random."""
    rng = np.random.default_rng(seed)
    special = sorted({i for i in (0, N - 1, 63, 64, 127, 128) if i < N})
    sets = []
    for o in range(0, len(special), B):
        head = special[o:o + B]
        sets.append(np.array(head + rng.integers(0, N, size=B - len(head)).tolist(), dtype=np.int64))
    return sets


def _check_against_matrix(RT, cuda, q, t, metric, p, target_sets):
    index = RT.FlatIndex(t.to(cuda), metric, p)
    d = RT.cdist(q.to(cuda), t.to(cuda), metric, p).cpu().numpy()
    for targets in target_sets:
        got = index.rank_of(q.to(cuda), torch.from_numpy(targets))
        assert got.dtype == torch.int32 and got.device.type == "cuda" and got.shape == (q.shape[0],)
        ref = R.ranks_from_keys(d, targets)
        assert got.cpu().numpy().tolist() == ref.tolist(), (metric, p, targets.tolist())


@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("metric,p", SCIPY_CASES)
def test_scipy_metrics_exact_against_the_matrix(RT, cuda, metric, p, B, N):
    q, t = _normal(B, N, seed=B * 7 + N)
    _check_against_matrix(RT, cuda, q, t, metric, p, _target_sets(B, N, seed=N))


@pytest.mark.parametrize("metric", ["euclidean", "cosine", "L2", "IP"])
def test_twin_rows_rank_next_to_each_other(RT, cuda, metric):
    """The upper half of the table repeats the lower half, so a target in the upper half ties with its lower twin and ranks right
    after it -- unless the target's key is not, bit for bit, what the stream computes for that pair."""
    H = 100
    _, low = _normal(1, H, seed=5)
    t = torch.cat([low, low]).to(cuda)
    rows = [0, 1, 63, 64, 99, 100, 163, 199, 17]
    q = t[rows]                                           # queries from the table: the query's own twins tie at the best key
    lower = torch.tensor([0, 5, 63, 64, 99, 0, 63, 98, 17])
    index = RT.FlatIndex(t, metric)
    r_low = index.rank_of(q, lower).cpu()
    r_up = index.rank_of(q, lower + H).cpu()
    assert (r_low >= 0).all() and torch.equal(r_up, r_low + 1), (metric, r_low.tolist(), r_up.tolist())
    own = index.rank_of(q, torch.tensor(rows) % H).cpu()  # the query's own lower twin
    if metric != "IP":                                   # nothing is nearer than the row itself (IP has no such property)
        assert own.tolist() == [0] * len(rows)


def test_nan_distances_rank_last_in_id_order(RT, cuda):
    q, t = _normal(6, 150, seed=9)
    t[[0, 64, 100, 149]] = 0.0                            # zero rows: cosine against them is NaN
    q[2] = 0.0                                            # a zero query: its whole row is NaN
    targets = [np.array([0, 64, 100, 149, 7, 130]), np.array([5, 0, 64, 3, 149, 100]), np.array([149, 148, 1, 0, 64, 99])]
    _check_against_matrix(RT, cuda, q, t, "cosine", None, targets)
    d = RT.cdist(q.to(cuda), t.to(cuda), "cosine").cpu().numpy()
    assert np.isnan(d[2]).all() and np.isnan(d[:, 64]).all() and not np.isnan(d[0, 1])
    # braycurtis: only the zero query against a zero row is NaN (0 / 0)
    _check_against_matrix(RT, cuda, q, t, "braycurtis", None, targets)
    d = RT.cdist(q.to(cuda), t.to(cuda), "braycurtis").cpu().numpy()
    assert np.isnan(d[2, [0, 64, 100, 149]]).all() and np.isnan(d).sum() == 4


def _integer_data(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-3, 4, (B, 128), generator=g).float(), torch.randint(-3, 4, (N, 128), generator=g).float())


TOPK_SHAPES = [(1, 1), (64, 64), (65, 65), (130, 520), (7, 1100)]


def _topk_targets(B, N, seed):
    rng = np.random.default_rng(seed)
    targets = rng.integers(0, N, size=B)
    special = sorted({i for i in (0, N - 1, 63, 64) if i < N})[:B]
    targets[:len(special)] = special
    return targets.astype(np.int64)


@pytest.mark.parametrize("B,N", TOPK_SHAPES)
def test_ip_and_l2_exact_on_integer_data(RT, cuda, B, N):
    """Entries in -3..3: every key of IP and L2 is an integer below 2^24, so fp32 is exact and ties are frequent."""
    q, t = _integer_data(B, N, seed=B + N)
    qi, ti = q.numpy().astype(np.int64), t.numpy().astype(np.int64)
    targets = _topk_targets(B, N, seed=N)
    ip = qi @ ti.T
    l2 = (qi * qi).sum(1)[:, None] - 2 * ip + (ti * ti).sum(1)[None, :]
    got_ip = RT.FlatIndex(t.to(cuda), "IP").rank_of(q.to(cuda), torch.from_numpy(targets)).cpu().numpy()
    got_l2 = RT.FlatIndex(t.to(cuda), "L2").rank_of(q.to(cuda), torch.from_numpy(targets)).cpu().numpy()
    assert got_ip.tolist() == R.ranks_from_keys(ip, targets, larger_is_better=True).tolist()
    assert got_l2.tolist() == R.ranks_from_keys(l2, targets).tolist()


@pytest.mark.parametrize("B,N", TOPK_SHAPES)
@pytest.mark.parametrize("data", ["integer", "normal"])
@pytest.mark.parametrize("metric", ["IP", "L2", "COS"])
def test_rank_agrees_with_search(RT, cuda, metric, data, B, N):
    """rank < k: the target sits at that position of the search result; rank >= k: it is not in it.  N <= 64 pins every rank."""
    q, t = (_integer_data if data == "integer" else _normal)(B, N, seed=3 * B + N)
    index = RT.FlatIndex(t.to(cuda), metric)
    k = min(64, N)
    _, ids = index.search(q.to(cuda), k)
    ids = ids.cpu().numpy()
    for targets in (_topk_targets(B, N, seed=1), ids[:, k // 2].copy(), ids[:, k - 1].copy()):
        rank = index.rank_of(q.to(cuda), torch.from_numpy(targets)).cpu().numpy()
        assert ((rank >= 0) & (rank < N)).all()
        for b in range(B):
            if rank[b] < k:
                assert ids[b, rank[b]] == targets[b], (metric, b, int(rank[b]))
            else:
                assert targets[b] not in ids[b], (metric, b, int(rank[b]))


@pytest.mark.parametrize("metric", ["cityblock", "cosine", "L2", "COS"])
def test_rank_does_not_depend_on_batch_or_split(RT, cuda, metric):
    q, t = _normal(130, 1000, seed=21)
    q, t = q.to(cuda), t.to(cuda)
    targets = torch.from_numpy(np.random.default_rng(4).integers(0, 1000, size=130)).to(cuda)
    index = RT.FlatIndex(t, metric)
    in130 = index.rank_of(q, targets)
    in33 = index.rank_of(q[:33], targets[:33])
    alone = torch.cat([index.rank_of(q[b:b + 1], targets[b:b + 1]) for b in range(33)])
    assert torch.equal(in33, in130[:33]) and torch.equal(alone, in33)
    assert torch.equal(index.rank_of(q, targets), in130)
    assert torch.equal(RT.target_ranks(q, t, targets, metric), in130)


@pytest.mark.parametrize("metric", ["euclidean", "correlation", "IP", "L2", "COS"])
def test_bad_targets_give_minus_one(RT, cuda, metric):
    q, t = _normal(9, 300, seed=2)
    q, t = q.to(cuda), t.to(cuda)
    index = RT.FlatIndex(t, metric)
    good = torch.tensor([0, 299, 5, 64, 7, 100, 200, 250, 3])
    ref = index.rank_of(q, good).cpu()
    bad = good.clone()
    bad[1], bad[4], bad[8] = -1, 300, 2 ** 40
    got = index.rank_of(q, bad).cpu()
    keep = torch.tensor([0, 2, 3, 5, 6, 7])
    assert got[[1, 4, 8]].tolist() == [-1, -1, -1] and torch.equal(got[keep], ref[keep]) and (ref >= 0).all()
    assert torch.equal(index.rank_of(q, good.to(torch.int32)).cpu(), ref)                             # int32 targets are cast
    empty = index.rank_of(q[:0], good[:0])
    assert empty.shape == (0,) and empty.dtype == torch.int32 and empty.device.type == "cuda"
    with pytest.raises(ValueError, match="9.*8|8.*9"):
        index.rank_of(q, good[:8])
    with pytest.raises(ValueError):
        index.rank_of(q, good.float())


# ---------------------------------------------------------------- RankingMeter

KS = (1, 10, 100, 1000)


def _handmade_ranks():
    rng = np.random.default_rng(11)
    r = np.concatenate([np.arange(0, 12), [99, 100, 101, 999, 1000, 1001, 4999, 5000, -1, -1],
                        rng.integers(0, 5001, size=2500), [-1], rng.integers(0, 30, size=700)]).astype(np.int32)
    mask = (rng.random(len(r)) < 0.7).astype(np.uint8)
    return r, mask


def _state(m):
    torch.cuda.synchronize()
    return m.counts.cpu().tolist(), m.sums.cpu().numpy().copy()


def _assert_matches(m, ref, ks=KS):
    counts, sums = _state(m)
    assert counts[:len(ks)] == [ref["hits"][k] for k in ks]
    assert counts[len(ks):] == [ref["rank_sum"], ref["rows"], ref["invalid"]]
    for got, want in zip(sums, [ref["ndcg_sum"][k] for k in ks] + [ref["mrr_sum"]]):
        assert got == pytest.approx(want, rel=1e-12)


def test_ranking_meter_against_the_reference(RT, cuda):
    r, mask = _handmade_ranks()
    assert len(r) > 3 * 1024 and (r == -1).sum() == 3
    ranks = torch.from_numpy(r).to(cuda)
    m = RT.RankingMeter(ks=KS, device=cuda)
    m.update(ranks)
    ref = R.meter_reference(r, None, KS)
    _assert_matches(m, ref)
    assert m.invalid == 3
    for read in (lambda: m.rows, m.hit_rate, m.ndcg, lambda: m.mrr, lambda: m.mean_rank, m.hits):
        with pytest.raises(ValueError, match="3"):
            read()
    # masking the invalid rows out makes the meter readable
    ok = torch.from_numpy((r >= 0).astype(np.uint8)).to(cuda)
    m.reset()
    m.update(ranks, ok)
    ref = R.meter_reference(r, r >= 0, KS)
    _assert_matches(m, ref)
    assert m.rows == ref["rows"] and m.invalid == 0 and m.hits() == ref["hits"]
    assert m.hit_rate() == {k: ref["hits"][k] / ref["rows"] for k in KS}
    for k in KS:
        assert m.ndcg()[k] == pytest.approx(ref["ndcg"][k], rel=1e-12)
    assert m.mrr == pytest.approx(ref["mrr"], rel=1e-12) and m.mean_rank == pytest.approx(ref["mean_rank"], rel=1e-12)
    # a mask of any dtype: non-zero keeps the row
    m.reset()
    both = mask * (r >= 0)
    m.update(ranks, torch.from_numpy(both.astype(np.float32)).to(cuda))
    _assert_matches(m, R.meter_reference(r, both, KS))


def test_ranking_meter_accumulates_and_repeats_bit_for_bit(RT, cuda):
    r, mask = _handmade_ranks()
    ranks, msk = torch.from_numpy(r).to(cuda), torch.from_numpy(mask).to(cuda)
    cuts = [0, 5, 1500, len(r)]

    def three_calls():
        m = RT.RankingMeter(ks=KS, device=cuda)
        for a, b in zip(cuts, cuts[1:]):
            m.update(ranks[a:b], msk[a:b])
        return m

    one = RT.RankingMeter(ks=KS, device=cuda)
    one.update(ranks, msk)
    (c3, f3), (c1, f1) = _state(three_calls()), _state(one)
    assert c3 == c1
    np.testing.assert_allclose(f3, f1, rtol=1e-12, atol=0)
    _assert_matches(one, R.meter_reference(r, mask, KS))
    c3b, f3b = _state(three_calls())
    assert c3b == c3 and f3b.tobytes() == f3.tobytes()
    # an empty meter cannot be read, an empty update changes nothing
    m = RT.RankingMeter(ks=(5,), device=cuda)
    m.update(ranks[:0])
    assert m.rows == 0
    with pytest.raises(ValueError):
        m.mrr
    m.update(torch.tensor([4, 5], dtype=torch.int32, device=cuda))
    assert m.hit_rate() == {5: 0.5} and m.mean_rank == 4.5
    with pytest.raises(ValueError):
        m.update(ranks.long())


# ---------------------------------------------------------------- the whole path once

@pytest.mark.parametrize("rows_per_batch", [None, 37])
def test_frame_env_targets_rank_first_under_their_own_action(RT, cuda, rows_per_batch):
    from recnn_amd.data.env import FrameEnv
    n_users = 12
    items, ratings, table = make_store(n_users=n_users, n_items=500, emb_dim=128, min_len=25, max_len=40, seed=6)
    user_dict = {100 + 3 * u: {"items": items[u], "ratings": ratings[u]} for u in range(n_users)}
    ids = list(user_dict)
    env = FrameEnv.from_user_dict(torch.from_numpy(table), user_dict, ids[:6], ids[6:], frame_size=10, batch_size=4, device=cuda,
                                  rows_per_batch=rows_per_batch)
    index = RT.FlatIndex(env.table, "L2")
    meter = RT.RankingMeter(ks=(1, 10), device=cuda)
    sl = env.store.slots(ids[7:10])
    # (batch, its users, slots to pass): a collate_slots batch made without user ids records its slots as the users
    cases = [(env.test_batch(), None, None), (env.collate_users(ids[2:5]), ids[2:5], None),
             (env.collate_slots(sl, ids[7:10]), ids[7:10], None), (env.collate_slots(sl), ids[7:10], sl)]
    for batch, users, slots in cases:
        rows = batch["action"].shape[0]
        assert rows == 37 if rows_per_batch else rows > 0
        targets = env.target_items(batch) if slots is None else env.target_items(batch, slots=slots)
        assert targets.dtype == torch.int64 and targets.shape == (rows,) and targets.device.type == "cuda"
        users = batch["meta"]["users"].tolist() if users is None else users
        want = np.concatenate([user_dict[u]["items"][10:] for u in users])[:rows]
        assert targets.cpu().numpy().tolist() == want.tolist()
        assert torch.equal(env.table[targets], batch["action"])                  # the gather is a copy
        rank = index.rank_of(batch["action"], targets)
        assert rank.cpu().tolist() == [0] * rows
        meter.update(rank)
    assert meter.hit_rate()[1] == 1.0 and meter.mrr == 1.0 and meter.mean_rank == 0.0 and meter.ndcg()[10] == 1.0
    batch = cases[1][0]
    with pytest.raises(ValueError):
        env.target_items({"action": batch["action"], "meta": {"users": batch["meta"]["users"], "sizes": batch["meta"]["sizes"] + 1}})
    with pytest.raises(ValueError):
        env.target_items(cases[3][0])                    # its users are slots, which are not user ids of this store
