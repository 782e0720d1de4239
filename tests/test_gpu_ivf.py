"""GPU: the IVF-Flat index (csrc/ivf.hip) against `FlatIndex` and tests/ivf_reference.py.

Every comparison is exact -- ids and list contents as integers, distances and centroids as bit patterns -- except the float k-means
of test 7, whose bound is the sequential-summation bound stated there."""
import types

import numpy as np
import pytest
import torch

import ivf_reference as R

pytestmark = pytest.mark.gpu

N, D = 1000, 128
PLANTED = (0, 1, 63, 64, 65, 300, 507)                # list lengths: the chunk boundaries of the scan, and an empty list
EMPTY, SINGLE = 0, 1
BS, KS = (1, 5, 65, 130), (1, 10, 64)


@pytest.fixture(scope="module")
def RT(cuda):
    from recnn_amd import retrieval
    return retrieval


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _same(got, want):
    return torch.equal(got[1], want[1]) and np.array_equal(_bits(got[0]), _bits(want[0]))


def planted_assignment(seed=0):
    a = np.repeat(np.arange(len(PLANTED)), PLANTED)
    np.random.default_rng(seed).shuffle(a)
    return a


def integer_case(seed=30):
    """Test 5's data: integer values in [-8, 8]; centroid 13 repeats centroid 4."""
    rng = np.random.default_rng(seed)
    table = rng.integers(-8, 9, size=(N, D))
    cent = table[rng.permutation(N)[:20]].copy()
    cent[13] = cent[4]
    return table, cent


def blob_case(seed=7):
    """Test 7's data: 12 Gaussian blobs of 125 rows, unit-variance centres, noise 0.1, rows shuffled; one initial centroid per blob."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((12, D))
    label = rng.permutation(np.repeat(np.arange(12), 125))
    table = (centres[label] + 0.1 * rng.standard_normal((len(label), D))).astype(np.float32)
    first = np.array([int(np.nonzero(label == c)[0][0]) for c in range(12)])
    return table, table[first].copy()


@pytest.fixture(scope="module")
def data(RT, cuda):
    g = torch.Generator().manual_seed(0)
    table = torch.randn(N, D, generator=g)
    dup = table.clone()
    dup[500:540] = dup[100:140]                                          # 40 duplicated rows: ties decided by id
    queries = torch.randn(130, D, generator=g)
    queries[7] = dup[110]                                                # a query that sits on a duplicated pair
    wide = torch.zeros(130, 200)
    wide[:, 8:8 + D] = queries
    d = {"table": table.to(cuda), "dup": dup.to(cuda), "q": queries.to(cuda), "wide": wide.to(cuda), "flat": {}, "RT": RT}
    return d


def _queries(data, B, layout):
    return data["q"][:B] if layout == "contiguous" else data["wide"][:B, 8:8 + D]


def _flat(data, which, metric, B, k):
    """FlatIndex.search on the contiguous queries: computed once, shared."""
    key = (which, metric, B, k)
    if key not in data["flat"]:
        index = data["flat"].setdefault((which, metric), data["RT"].FlatIndex(data[which], metric))
        data["flat"][key] = index.search(data["q"][:B], k)
    return data["flat"][key]


# ---------------------------------------------------------------- 1. lists as planted

def test_lists_are_the_stable_sort_of_the_assignment(RT, cuda, data):
    a = planted_assignment()
    cent = torch.randn(len(PLANTED), D, generator=torch.Generator().manual_seed(1)).to(cuda)
    for arg in (torch.from_numpy(a), torch.from_numpy(a).to(cuda, torch.int32)):
        index = RT.IVFFlatIndex.from_assignment(data["table"], cent, arg, "L2")
        start, ids = R.build_lists(a, len(PLANTED))
        assert index.list_start.dtype == torch.int32 and index.list_ids.dtype == torch.int32 and index.assignment.dtype == torch.int32
        assert np.array_equal(index.list_start.cpu().numpy(), start) and np.diff(start).tolist() == list(PLANTED)
        assert np.array_equal(index.list_ids.cpu().numpy(), ids)
        assert np.array_equal(index.assignment.cpu().numpy(), a)
        assert np.array_equal(_bits(index.centroids), _bits(cent))
        assert (index.ntotal, index.dim, index.nlist, index.metric) == (N, D, len(PLANTED), "L2")
    with pytest.raises(ValueError, match=r"list ids in \[0, 7\)"):
        RT.IVFFlatIndex.from_assignment(data["table"], cent, torch.from_numpy(a + 1), "L2")


# ---------------------------------------------------------------- 2. exhaustive equals flat

def _index(RT, cuda, table, nlist, metric):
    if nlist == len(PLANTED):                                            # planted lists, one of them empty
        cent = torch.randn(nlist, D, generator=torch.Generator().manual_seed(2)).to(cuda)
        return RT.IVFFlatIndex.from_assignment(table, cent, torch.from_numpy(planted_assignment(3)), metric)
    return RT.IVFFlatIndex(table, nlist, metric, niter=2, seed=nlist)


@pytest.mark.parametrize("metric", ["L2", "IP"])
@pytest.mark.parametrize("nlist", [1, 7, 20])
def test_every_list_probed_is_the_flat_search(RT, cuda, data, nlist, metric):
    for which in ("table", "dup"):
        index = _index(RT, cuda, data[which], nlist, metric)
        assert int(index.list_start[-1]) == N
        for B in BS:
            for k in KS:
                want = _flat(data, which, metric, B, k)
                for layout in ("contiguous", "slice"):
                    q = _queries(data, B, layout)
                    got = index.search(q, k, nprobe=nlist if k != 10 else 64)
                    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and tuple(got[1].shape) == (B, k)
                    assert _same(got, want), (which, B, k, layout)
    if metric == "L2":                                                   # the duplicated pair: equal distance, smaller id first
        ids = index.search(data["q"][7:8], 2, nprobe=64)[1][0].tolist()
        assert ids == [110, 510]


# ---------------------------------------------------------------- 3. restricted equals flat with exclusion

@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_restricted_search_is_the_flat_search_without_the_other_lists(RT, cuda, data, metric):
    B = 70
    table, q = data["table"], data["q"][:B]
    a = planted_assignment(4)
    cent = table[torch.randperm(N, generator=torch.Generator().manual_seed(5))[:len(PLANTED)].to(cuda)].clone()
    scale = 1.0 if metric == "L2" else 10.0                             # row 0 lands on the empty list, row 1 on the one-item list
    cent[EMPTY], cent[SINGLE] = scale * q[0], scale * q[1]
    index = RT.IVFFlatIndex.from_assignment(table, cent, torch.from_numpy(a), metric)
    flat = RT.FlatIndex(table, metric)
    rng = np.random.default_rng(6)
    user = [rng.integers(0, N, size=30).tolist() + [-1, N] for _ in range(B)]
    user[1] = list(range(N))                                             # with the user's exclusion on top: a row with nothing left
    for nprobe in (1, 3):
        lists = index.probe(q, nprobe)[1]
        assert tuple(lists.shape) == (B, nprobe) and int(lists[0, 0]) == EMPTY and int(lists[1, 0]) == SINGLE
        reach = R.probed_items(lists.cpu().numpy(), a)
        others = [np.nonzero(~reach[b])[0].tolist() for b in range(B)]
        ex = RT.SeenItems.from_lists(others, device=cuda)
        both = RT.SeenItems.from_lists([o + u for o, u in zip(others, user)], device=cuda)
        for k in (10, 64):
            got = index.search(q, k, nprobe)
            assert _same(got, flat.search(q, k, exclude=ex)), (nprobe, k)
            n_reach = reach.sum(1)
            for b in np.nonzero(n_reach < k)[0]:
                assert (got[1][b, n_reach[b]:] == -1).all() and (got[1][b, :n_reach[b]] >= 0).all()
                assert torch.isinf(got[0][b, n_reach[b]:]).all()
            if nprobe == 1:
                assert (got[1][0] == -1).all() and got[1][1].tolist() == [int(np.nonzero(a == SINGLE)[0][0])] + [-1] * (k - 1)
                assert (got[0][0] == (float("inf") if metric == "L2" else float("-inf"))).all()
            with_user = index.search(q, k, nprobe, exclude=RT.SeenItems.from_lists(user, device=cuda))
            assert _same(with_user, flat.search(q, k, exclude=both)), (nprobe, k)
            assert (with_user[1][1] == -1).all()
            mask = RT.SeenItems.from_lists(user, device=cuda).mask(N)    # a SeenMask is taken as it is
            assert _same(index.search(q, k, nprobe, exclude=mask), with_user)


# ---------------------------------------------------------------- 4. probe

@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_probe_is_the_flat_search_over_the_centroids(RT, cuda, data, metric):
    index = RT.IVFFlatIndex(data["table"], 20, metric, niter=1, seed=1)
    flat = RT.FlatIndex(index.centroids, metric)
    for nprobe, p in ((1, 1), (5, 5), (20, 20), (64, 20)):
        for layout in ("contiguous", "slice"):
            got = index.probe(_queries(data, 65, layout), nprobe)
            assert tuple(got[1].shape) == (65, p) and got[1].dtype == torch.int64
            assert _same(got, flat.search(data["q"][:65], p))


# ---------------------------------------------------------------- 5. one k-means iteration, exact

def test_one_iteration_on_integer_data_is_exact(RT, cuda):
    table_i, cent_i = integer_case()
    assert R.sq_dists(table_i, cent_i).max() < 2 ** 24 and np.abs(table_i).sum(0).max() < 2 ** 24     # every partial sum is exact
    table = torch.from_numpy(table_i).float().to(cuda)
    cent = torch.from_numpy(cent_i).float()
    a0 = R.assign(table_i, cent_i)
    assert not (a0 == 13).any() and (a0 == 4).any()                      # the tie goes to the smaller id: list 13 is empty
    lists_only = RT.IVFFlatIndex(table, 20, "L2", niter=0, centroids=cent)
    assert np.array_equal(lists_only.assignment.cpu().numpy(), a0)
    assert np.array_equal(_bits(lists_only.centroids), cent.numpy().view(np.int32))
    a1, means = R.kmeans_iteration(table_i, cent_i)
    assert np.array_equal(a1, a0) and np.array_equal(means[13], cent_i[13])
    rounded = means.astype(np.float32).astype(np.float64)                # the centroids the final assignment is taken against
    assert R.fp32_assignment_margin(table_i, rounded) > 0                # the reference's precondition: no fp32 order can differ
    for metric in ("L2", "IP"):                                          # training is L2 for both metrics
        index = RT.IVFFlatIndex(table, 20, metric, niter=1, centroids=cent)
        got = index.centroids.cpu().numpy()
        # an exact integer sum divided once, correctly rounded: the float64 quotient rounded to fp32
        assert np.array_equal(got.view(np.int32), means.astype(np.float32).view(np.int32))
        assert np.array_equal(index.assignment.cpu().numpy(), R.assign(table_i.astype(np.float64), rounded))
        start, ids = R.build_lists(index.assignment.cpu().numpy(), 20)
        assert np.array_equal(index.list_start.cpu().numpy(), start) and np.array_equal(index.list_ids.cpu().numpy(), ids)
    assert np.array_equal(cent.numpy(), cent_i)                          # the caller's centroids are not written


# ---------------------------------------------------------------- 6. composition and determinism

def _state(index):
    return [_bits(index.centroids), index.assignment.cpu().numpy(), index.list_start.cpu().numpy(), index.list_ids.cpu().numpy()]


def _equal_state(x, y):
    return all(np.array_equal(p, q) for p, q in zip(_state(x), _state(y)))


def test_iterations_compose_and_construction_is_deterministic(RT, cuda, data):
    table = data["table"]
    nlist = 20
    c0 = table[torch.randperm(N, generator=torch.Generator().manual_seed(9))[:nlist].to(cuda)].clone()
    three = RT.IVFFlatIndex(table, nlist, "L2", niter=3, centroids=c0)
    step = RT.IVFFlatIndex(table, nlist, "L2", niter=1, centroids=c0)
    assert not np.array_equal(_bits(step.centroids), _bits(c0))
    for _ in range(2):
        step = RT.IVFFlatIndex(table, nlist, "L2", niter=1, centroids=step.centroids)
    assert _equal_state(three, step)
    assert _equal_state(three, RT.IVFFlatIndex(table, nlist, "L2", niter=3, centroids=c0))
    # the seeded start is the documented one, and the same seed gives the same index
    seeded = RT.IVFFlatIndex(table, nlist, "IP", niter=3, seed=9)
    assert _equal_state(seeded, three) and _equal_state(seeded, RT.IVFFlatIndex(table, nlist, "IP", niter=3, seed=9))
    assert not _equal_state(seeded, RT.IVFFlatIndex(table, nlist, "IP", niter=3, seed=10))
    q = data["q"][:33]
    assert _same(three.search(q, 10, 4), step.search(q, 10, 4))


# ---------------------------------------------------------------- 7. float data against float64

def test_float_kmeans_against_float64(RT, cuda):
    table_f, cent_f = blob_case()
    want_a, want_c, gap = R.kmeans(table_f, cent_f, 3, min_gap=0.5)     # the reference's own precondition
    index = RT.IVFFlatIndex(torch.from_numpy(table_f).to(cuda), 12, "L2", niter=3, centroids=torch.from_numpy(cent_f))
    assert np.array_equal(index.assignment.cpu().numpy(), want_a)
    assert np.bincount(want_a, minlength=12).tolist() == [125] * 12
    got = index.centroids.cpu().numpy().astype(np.float64)
    worst = 0.0
    for c in range(12):
        rows = table_f[want_a == c]
        bound = (len(rows) + 1) * 2.0 ** -24 * np.abs(rows).max()      # sequential summation, any order, and the division
        err = np.abs(got[c] - want_c[c]).max()
        worst = max(worst, err / bound)
        assert err <= bound, (c, err, bound)
    print(f"float k-means: relative gap {gap:.3f}, worst centroid error {worst:.3f} of its bound")


# ---------------------------------------------------------------- 8. db_con

def test_db_con_builds_the_ivf_index_and_honours_nprobe(RT, cuda, data):
    from recnn_amd.data import db_con
    env = types.SimpleNamespace(base=types.SimpleNamespace(embeddings=data["table"]))
    q = data["q"][:33]
    for metric in (db_con.MetricType.L2, db_con.MetricType.IP):
        con = db_con.MilvusConnection(env, "movies", param={"metric_type": metric, "index_type": "IVF_FLAT", "nlist": 16})
        assert isinstance(con.index, RT.IVFFlatIndex) and con.index.nlist == 16 and con.index.metric == metric.name
        for param, nprobe in (({"nprobe": 2}, 2), (None, 16), ({}, 16), ({"nprobe": 64}, 64)):
            res = con.search(q, topk=10, search_param=param)
            assert _same((res.dist(cuda), res.id(cuda)), con.index.search(q, 10, nprobe))
        res = con.client.search("movies", q, 10, params={"nprobe": 2})[1]
        assert _same((res.dist(cuda), res.id(cuda)), con.index.search(q, 10, 2))
        assert not torch.equal(con.index.search(q, 10, 2)[1], con.index.search(q, 10, 16)[1])
        # without index_type nothing changes: a FlatIndex, nprobe ignored
        plain = db_con.MilvusConnection(env, "movies", param={"metric_type": metric})
        assert isinstance(plain.index, RT.FlatIndex)
        res = plain.search(q, topk=10, search_param={"nprobe": 1})
        assert _same((res.dist(cuda), res.id(cuda)), RT.FlatIndex(data["table"], metric.name).search(q, 10))


# ---------------------------------------------------------------- 9. two-stage

def test_two_stage_takes_an_ivf_first_stage(RT, cuda, data):
    import recnn_amd
    S, H, B, nlist = 50, 24, 33, 20
    g = torch.Generator().manual_seed(31)
    critic = recnn_amd.nn.Critic(S, D, H)
    with torch.no_grad():
        critic.linear3.weight.mul_(1e4)
    critic = critic.to(cuda)
    state, action = torch.randn(B, S, generator=g).to(cuda), data["q"][:B]
    critic_index = RT.CriticIndex(critic, data["table"])
    rng = np.random.default_rng(3)
    ex = RT.SeenItems.from_lists([rng.integers(0, N, size=25).tolist() for _ in range(B)], device=cuda)
    for metric in ("L2", "IP"):
        ivf = RT.IVFFlatIndex(data["table"], nlist, metric, niter=2)
        two = RT.TwoStageIndex(ivf, critic_index, 64)
        want = RT.TwoStageIndex(RT.FlatIndex(data["table"], metric), critic_index, 64)
        for k in (1, 10, 64):
            assert _same(two.search(action, state, k, nprobe=nlist), want.search(action, state, k))
            assert _same(two.search(action, state, k, ex, nprobe=64), want.search(action, state, k, ex))
        near = two.search(action, state, 10)                             # 16 probes by default
        assert _same(near, critic_index.rerank(state, ivf.search(action, 64, 16)[1], 10))
        with pytest.raises(ValueError, match="rank_of: refused with an IVFFlatIndex first stage"):
            two.rank_of(action, state, torch.zeros(B, dtype=torch.int64))


def test_wolpertinger_policy_with_an_ivf_first_stage(RT, cuda, data):
    import recnn_amd
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3)
        actor = recnn_amd.nn.Actor(1290, 128, 256).to(cuda)
        critic = recnn_amd.nn.Critic(1290, 128, 256).to(cuda)
    state = torch.randn(8, 1290, generator=torch.Generator().manual_seed(4)).to(cuda)
    flat = recnn_amd.nn.WolpertingerPolicy(actor, critic, data["table"])
    ivf = recnn_amd.nn.WolpertingerPolicy(actor, critic, data["table"], index="ivf", nlist=12, nprobe=12)
    assert isinstance(ivf.flat, RT.IVFFlatIndex)
    assert _same(ivf.recommend(state, 10), flat.recommend(state, 10))
    ids, actions, q = ivf.act(state)
    want = flat.act(state)
    assert torch.equal(ids, want[0]) and np.array_equal(_bits(actions), _bits(want[1])) and np.array_equal(_bits(q), _bits(want[2]))
    with pytest.raises(ValueError, match="rank_of: refused"):
        ivf.rank_of(state, torch.zeros(8, dtype=torch.int64))
