"""GPU: per-row exclusion of already-seen items (csrc/seen.hip and the excluding epilogues of csrc/topk.hip, csrc/rank.hip;
DESIGN.md section 21): SeenItems / SeenMask, FlatIndex.search / rank_of with `exclude`, FrameEnv.seen_items, against
tests/seen_reference.py.

Everything here is compared without a tolerance: mask words bit for bit, ranks as integers, ids as integers, distances by their bit
patterns against what the search without `exclude` (the code that was there before) reports for the same pair."""
import numpy as np
import pytest
import torch

import seen_reference as S
from helpers import make_store

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 200), (5, 129), (64, 64), (65, 65), (33, 1000), (130, 1000)]
SCIPY_CASES = [("sqeuclidean", None), ("euclidean", None), ("cityblock", None), ("chebyshev", None), ("minkowski", None),
               ("canberra", None), ("braycurtis", None), ("cosine", None), ("correlation", None), ("minkowski", 3.0)]
# the twelve orders: faiss's three and scipy's nine (minkowski with an exponent that has a kernel of its own)
ORDERS = [("IP", None), ("L2", None), ("COS", None)] + [c for c in SCIPY_CASES if c != ("minkowski", None)]
OUT_OF_RANGE = [-1, 2 ** 31 + 5]


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


def _lists(B, N, seed, longest=30):
    """One exclusion list per row: ids 0, 63, 64, 127, 128 and N - 1 where they exist, random ids, a duplicate, and the
    out-of-range values -1, N and 2^31 + 5, shuffled."""
    rng = np.random.default_rng(seed)
    special = [i for i in (0, 63, 64, 127, 128, N - 1) if i < N]
    out = []
    for _ in range(B):
        ids = special + rng.integers(0, N, size=int(rng.integers(0, longest + 1))).tolist()
        ids = ids + [ids[0]] + OUT_OF_RANGE + [N]
        out.append([ids[i] for i in rng.permutation(len(ids))])
    return out


def _words(mask):
    return mask.words.cpu().numpy().view(np.uint64)


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _index(RT, cuda, t, metric, p):
    return RT.FlatIndex(t.to(cuda), metric, p)


def _descending(metric):
    return metric in ("IP", "COS")


# ---------------------------------------------------------------- the mask

@pytest.mark.parametrize("B,N", SHAPES)
def test_mask_equals_the_reference_bit_for_bit(RT, cuda, B, N):
    lists = _lists(B, N, seed=B + N)
    if B >= 3:
        lists[1] = []                                                    # a row of length 0 amid others
        lists[2] = np.random.default_rng(1).permutation(N).tolist()      # the whole catalogue
    inside = [next((i for i in ids if 0 <= i < N), 0) for ids in lists]
    outside = [next((i for i in range(N) if i not in set(ids)), N) for ids in lists]           # N: nothing is left to keep
    keeps = [None, inside, outside, [(-1, N, 2 ** 40)[b % 3] for b in range(B)]]
    for keep in keeps:
        seen = RT.SeenItems.from_lists(lists, cuda, keep=None if keep is None else torch.tensor(keep))
        m = seen.mask(N)
        assert m.rows == B and m.n_items == N and m.words.dtype == torch.int64 and m.words.shape == (B, (N + 63) // 64)
        assert seen.mask(N) is m                                         # built once per n_items
        assert np.array_equal(_words(m), S.mask_words(lists, N, keep)), (B, N, keep)
    empty = RT.SeenItems.from_lists([[]] * B, cuda)
    assert not _words(empty.mask(N)).any()
    # the same lists read over a smaller and a larger catalogue: ids outside [0, n_items) are ignored
    for n in (max(N - 1, 1), N + 70):
        assert np.array_equal(_words(RT.SeenItems.from_lists(lists, cuda).mask(n)), S.mask_words(lists, n))


def test_mask_ignores_positions_outside_the_id_array(RT, cuda):
    N, n_ids = 300, 50
    ids = np.random.default_rng(2).integers(0, N, size=n_ids)
    big = 2 ** 62
    rows = [(-5, 10), (n_ids - 3, 10), (n_ids + 7, 5), (-10, 5), (4, -3), (-big, big + 3), (big, big), (0, 2 ** 63 - 1), (7, 0),
            (n_ids, 1), (n_ids - 1, 1), (-1, 1), (-1, 2), (3, 20), (-2 ** 63, 2 ** 63 - 1)]
    starts = torch.tensor([r[0] for r in rows], dtype=torch.int64)
    lengths = torch.tensor([r[1] for r in rows], dtype=torch.int64)
    lists = [ids[max(s, 0):max(min(s + n, n_ids), 0)].tolist() if n > 0 else [] for s, n in rows]
    assert [len(x) for x in lists] == [5, 3, 0, 0, 0, 3, 0, n_ids, 0, 0, 1, 0, 1, 20, 0]
    for dtype in (torch.int32, torch.int64, torch.int16):
        seen = RT.SeenItems(torch.from_numpy(ids).to(cuda, dtype), starts, lengths)
        assert np.array_equal(_words(seen.mask(N)), S.mask_words(lists, N))
    # an id array without elements: every row is empty
    none = RT.SeenItems(torch.zeros(0, dtype=torch.int32, device=cuda), starts, lengths)
    assert not _words(none.mask(N)).any()
    # int32 ids are used as they are; a wider dtype is converted once, values that do not fit become -1
    own = torch.from_numpy(ids.astype(np.int32)).to(cuda)
    assert RT.SeenItems(own, starts, lengths).ids.data_ptr() == own.data_ptr()
    wide = torch.tensor([5, 2 ** 31 + 5, -2 ** 31 - 1, 2 ** 32 + 7, 9], device=cuda)
    assert RT.SeenItems(wide, starts[:1], lengths[:1]).ids.tolist() == [5, -1, -1, -1, 9]


def test_mask_of_the_largest_catalogue_and_the_refusal_above_it(RT, cuda):
    N = 1 << 20
    rng = np.random.default_rng(5)
    lists = [rng.integers(0, N, size=5000).tolist() + [0, 63, 64, N - 1, N - 1, -1, N, 2 ** 31 + 5],
             rng.integers(N - 200, N + 50, size=300).tolist()]
    keep = [N - 1, 5]
    seen = RT.SeenItems.from_lists(lists, cuda, keep=torch.tensor(keep))
    assert np.array_equal(_words(seen.mask(N)), S.mask_words(lists, N, keep))
    from recnn_amd import _lib as L
    with pytest.raises(L.RecnnHipError, match="1048576"):
        seen.mask(N + 1)


# ---------------------------------------------------------------- rank_of

@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("metric,p", SCIPY_CASES)
def test_rank_of_scipy_metrics_exact_against_the_matrix(RT, cuda, metric, p, B, N):
    q, t = _normal(B, N, seed=B * 7 + N)
    index = _index(RT, cuda, t, metric, p)
    d = RT.cdist(q.to(cuda), t.to(cuda), metric, p).cpu().numpy()
    lists = _lists(B, N, seed=N + 1)
    seen = RT.SeenItems.from_lists(lists, cuda)
    for targets in _target_sets(B, N, seed=N):
        got = index.rank_of(q.to(cuda), torch.from_numpy(targets), exclude=seen)
        assert got.dtype == torch.int32 and got.device.type == "cuda" and got.shape == (B,)
        ref = S.ranks_from_keys_excluding(d, targets, lists)
        assert got.cpu().numpy().tolist() == ref.tolist(), (metric, p, targets.tolist())
    assert torch.equal(RT.target_ranks(q.to(cuda), t.to(cuda), torch.from_numpy(targets), metric, p, exclude=seen), got)


@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("metric,p", ORDERS)
def test_rank_of_is_the_plain_rank_minus_the_excluded_items_in_front(RT, cuda, metric, p, B, N):
    """filtered rank = unfiltered rank - #{distinct excluded e != g that come before g}; "e comes before g" is decided by the
    unfiltered rank_of on e itself, the query repeated per excluded id (tests/test_seen_cpu.py checks the identity)."""
    q, t = _normal(B, N, seed=B * 5 + N)
    q = q.to(cuda)
    index = _index(RT, cuda, t, metric, p)
    lists = _lists(B, N, seed=N + 2)
    targets = _target_sets(B, N, seed=N + 3)[0]
    lists[0] = lists[0] + [int(targets[0])]                              # an excluded target is ranked among the rest all the same
    plain = index.rank_of(q, torch.from_numpy(targets)).cpu().numpy()
    got = index.rank_of(q, torch.from_numpy(targets), exclude=RT.SeenItems.from_lists(lists, cuda)).cpu().numpy()
    ex = [[e for e in S.excluded_set(ids, N) if e != int(targets[b])] for b, ids in enumerate(lists)]
    owner = np.repeat(np.arange(B), [len(e) for e in ex])
    flat = np.array([e for row in ex for e in row], dtype=np.int64)
    in_front = np.zeros(B, dtype=np.int64)
    if len(flat):
        rank_e = index.rank_of(q[torch.from_numpy(owner).to(cuda)], torch.from_numpy(flat)).cpu().numpy()
        np.add.at(in_front, owner, rank_e < plain[owner])
    assert got.tolist() == (plain - in_front).tolist(), (metric, p)


@pytest.mark.parametrize("metric", ["euclidean", "cosine", "L2", "IP"])
def test_excluding_the_lower_twin_moves_the_upper_twin_up_by_one(RT, cuda, metric):
    """The upper half of the table repeats the lower half: a target in the upper half ties with its lower twin and ranks right after
    it.  With the lower twin excluded the tie is gone and the rank is exactly one less."""
    H = 100
    _, low = _normal(1, H, seed=5)
    t = torch.cat([low, low]).to(cuda)
    rows = [0, 1, 63, 64, 99, 100, 163, 199, 17]
    q = t[rows]
    lower = torch.tensor([0, 5, 63, 64, 99, 0, 63, 98, 17])
    index = RT.FlatIndex(t, metric)
    r_low = index.rank_of(q, lower).cpu()
    r_up = index.rank_of(q, lower + H).cpu()
    assert torch.equal(r_up, r_low + 1)
    seen = RT.SeenItems.from_lists([[int(i)] for i in lower], cuda)
    assert torch.equal(index.rank_of(q, lower + H, exclude=seen).cpu(), r_up - 1)
    assert torch.equal(index.rank_of(q, lower, exclude=seen).cpu(), r_low)          # the target's own bit is not consulted
    upper = RT.SeenItems.from_lists([[int(i) + H] for i in lower], cuda)
    assert torch.equal(index.rank_of(q, lower, exclude=upper).cpu(), r_low)          # the upper twin was behind it anyway


# ---------------------------------------------------------------- search

@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("metric,p", ORDERS)
def test_search_filters_exactly_within_the_head(RT, cuda, metric, p, B, N):
    q, t = _normal(B, N, seed=B * 3 + N)
    q = q.to(cuda)
    index = _index(RT, cuda, t, metric, p)
    k0 = min(64, N)
    d0, i0 = index.search(q, k0)
    if k0 > 4:
        drop = sorted({0, 2, 5, k0 - 1})
        keep = [j for j in range(k0) if j not in drop]
        lists = [i0[b, drop].tolist() + [int(i0[b, 0])] + OUT_OF_RANGE + [N] for b in range(B)]
        d, i = index.search(q, k0 - 4, exclude=RT.SeenItems.from_lists(lists, cuda))
        assert d.shape == (B, k0 - 4) and i.dtype == torch.int64 and d.dtype == torch.float32
        assert torch.equal(i, i0[:, keep]) and np.array_equal(_bits(d), _bits(d0[:, keep])), (metric, p)
    if N <= 64:                                                          # the complete order is known: arbitrary subsets
        rng = np.random.default_rng(B)
        sizes = [0, N, 1, N - 1] + rng.integers(0, N + 1, size=B).tolist()
        lists = [rng.permutation(N)[:sizes[b]].tolist() + OUT_OF_RANGE + [N] for b in range(B)]
        d, i = index.search(q, N, exclude=RT.SeenItems.from_lists(lists, cuda))
        pad = -np.inf if _descending(metric) else np.inf
        order, dist = i0.cpu().numpy(), d0.cpu().numpy()
        for b in range(B):
            want = S.filter_order(order[b], lists[b], N)
            assert i[b].tolist() == want, (metric, p, b)
            by_id = dict(zip(order[b].tolist(), dist[b]))
            want_d = np.array([by_id[j] if j >= 0 else pad for j in want], dtype=np.float32)
            assert np.array_equal(_bits(d[b]), want_d.view(np.int32)), (metric, p, b)


@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("metric", ["IP", "L2", "COS", "cityblock", "cosine"])
def test_search_is_consistent_with_rank_of(RT, cuda, metric, B, N):
    """Every item at position j of an excluding search has excluding rank j; a padding slot's id -1 is no target."""
    q, t = _normal(B, N, seed=B * 11 + N)
    q = q.to(cuda)
    index = _index(RT, cuda, t, metric, None)
    lists = _lists(B, N, seed=N + 4)
    k = min(64, N)
    _, ids = index.search(q, k, exclude=RT.SeenItems.from_lists(lists, cuda))
    left = [N - len(S.excluded_set(x, N)) for x in lists]
    assert [(row >= 0).sum().item() for row in ids] == [min(k, n) for n in left]
    rep = RT.SeenItems.from_lists([x for x in lists for _ in range(k)], cuda)
    rank = index.rank_of(q.repeat_interleave(k, 0), ids.flatten(), exclude=rep).reshape(B, k)
    want = torch.where(ids >= 0, torch.arange(k, device=cuda)[None, :], -1)
    assert torch.equal(rank.long(), want), metric


@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("metric,p", ORDERS)
def test_short_rows_end_in_minus_one(RT, cuda, metric, p, B):
    """Rows with 3 items left, none, all, 20 and 1 (k = 10): the items that are left in their order, then id -1 at +inf where
    distances ascend and -inf where scores descend."""
    N, k = 200, 10
    q, t = _normal(B, N, seed=B)
    q = q.to(cuda)
    index = _index(RT, cuda, t, metric, p)
    d0, i0 = index.search(q, 64)
    order, dist = i0.cpu().numpy(), d0.cpu().numpy()
    picks = [[3, 17, 40], [], None, list(range(5, 64, 3)), [63]][:B]     # positions of the head that stay; None: nothing excluded
    lists = [[] if pk is None else sorted(set(range(N)) - set(order[b, pk].tolist())) + [N, -1] for b, pk in enumerate(picks)]
    seen = RT.SeenItems.from_lists(lists, cuda)
    d, i = index.search(q, k, exclude=seen)
    pad = -np.inf if _descending(metric) else np.inf
    for b, pk in enumerate(picks):
        want = S.filter_order(order[b], lists[b], k)
        assert i[b].tolist() == want and want.count(-1) == (0 if pk is None else max(k - len(pk), 0)), (metric, b)
        by_id = dict(zip(order[b].tolist(), dist[b]))
        want_d = np.array([by_id[j] if j >= 0 else pad for j in want], dtype=np.float32)
        assert np.array_equal(_bits(d[b]), want_d.view(np.int32)), (metric, b)
    # everything excluded (row 1): any valid target ranks first, a bad one gives -1
    targets = torch.tensor([5, 199, 0, 7, 64][:B])
    rank = index.rank_of(q, targets, exclude=seen).cpu()
    assert rank[1] == 0
    bad = targets.clone()
    bad[1] = N
    assert index.rank_of(q, bad, exclude=seen).cpu()[1] == -1
    bad[1] = -1
    assert index.rank_of(q, bad, exclude=seen).cpu()[1] == -1


@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("metric,p", ORDERS)
def test_an_empty_exclusion_gives_the_plain_answer(RT, cuda, metric, p, B, N):
    q, t = _normal(B, N, seed=B + 2 * N)
    q = q.to(cuda)
    index = _index(RT, cuda, t, metric, p)
    seen = RT.SeenItems.from_lists([[]] * B, cuda)
    k = min(10, N)
    d0, i0 = index.search(q, k)
    d, i = index.search(q, k, exclude=seen)
    assert torch.equal(i, i0) and np.array_equal(_bits(d), _bits(d0))
    d, i = index.search(q, k, exclude=seen.mask(N))                      # a SeenMask is taken as well
    assert torch.equal(i, i0) and np.array_equal(_bits(d), _bits(d0))
    for targets in _target_sets(B, N, seed=N):
        tg = torch.from_numpy(targets)
        assert torch.equal(index.rank_of(q, tg, exclude=seen), index.rank_of(q, tg))


@pytest.mark.parametrize("metric", ["cityblock", "cosine", "L2", "COS", "IP"])
def test_results_do_not_depend_on_batch_or_split(RT, cuda, metric):
    q, t = _normal(130, 1000, seed=21)
    q, t = q.to(cuda), t.to(cuda)
    targets = torch.from_numpy(np.random.default_rng(4).integers(0, 1000, size=130)).to(cuda)
    lists = _lists(130, 1000, seed=6, longest=200)
    index = RT.FlatIndex(t, metric)

    def run(rows):
        seen = RT.SeenItems.from_lists([lists[b] for b in rows], cuda)
        sel = torch.tensor(list(rows), device=cuda)
        d, i = index.search(q[sel], 64, exclude=seen)
        return index.rank_of(q[sel], targets[sel], exclude=seen), d, i       # (one mask serves both calls)

    r130, d130, i130 = run(range(130))
    r33, d33, i33 = run(range(33))
    assert torch.equal(r33, r130[:33]) and torch.equal(i33, i130[:33]) and np.array_equal(_bits(d33), _bits(d130[:33]))
    for b in (0, 1, 31, 32):
        r1, d1, i1 = run([b])
        assert torch.equal(r1, r130[b:b + 1]) and torch.equal(i1, i130[b:b + 1]) and np.array_equal(_bits(d1), _bits(d130[b:b + 1]))
    r130b, d130b, i130b = run(range(130))
    assert torch.equal(r130b, r130) and torch.equal(i130b, i130) and np.array_equal(_bits(d130b), _bits(d130))


def test_refusals_by_name(RT, cuda):
    q, t = _normal(9, 300, seed=2)
    q, t = q.to(cuda), t.to(cuda)
    targets = torch.arange(9)
    for metric in ("L2", "cityblock"):
        index = RT.FlatIndex(t, metric)
        seen8 = RT.SeenItems.from_lists([[1]] * 8, cuda)
        with pytest.raises(ValueError, match="9 queries but an exclusion of 8 rows"):
            index.search(q, 5, exclude=seen8)
        with pytest.raises(ValueError, match="9 queries but an exclusion of 8 rows"):
            index.rank_of(q, targets, exclude=seen8.mask(300))
        other = RT.SeenItems.from_lists([[1]] * 9, cuda).mask(301)
        with pytest.raises(ValueError, match="n_items = 301"):
            index.search(q, 5, exclude=other)
        with pytest.raises(ValueError, match="n_items = 301"):
            index.rank_of(q, targets, exclude=other)
        with pytest.raises(TypeError, match="SeenItems or a SeenMask"):
            index.search(q, 5, exclude=[[1]] * 9)
        # an empty batch: empty results, nothing launched
        none = RT.SeenItems.from_lists([], cuda)
        d, i = index.search(q[:0], 5, exclude=none)
        assert d.shape == (0, 5) and i.shape == (0, 5) and i.dtype == torch.int64
        r = index.rank_of(q[:0], targets[:0], exclude=none)
        assert r.shape == (0,) and r.dtype == torch.int32
    ids = torch.arange(10, dtype=torch.int32, device=cuda)
    with pytest.raises(ValueError, match="starts must be a 1-D integer tensor"):
        RT.SeenItems(ids, torch.zeros(9), torch.ones(9, dtype=torch.int64))
    with pytest.raises(ValueError, match="9 starts but 8 lengths"):
        RT.SeenItems(ids, torch.zeros(9, dtype=torch.int64), torch.ones(8, dtype=torch.int64))


# ---------------------------------------------------------------- the whole path once

@pytest.mark.parametrize("rows_per_batch", [None, 37])
def test_frame_env_seen_items(RT, cuda, rows_per_batch):
    from recnn_amd.data.env import FrameEnv
    n_users, n_items, F = 12, 500, 10
    items, ratings, table = make_store(n_users=n_users, n_items=n_items, emb_dim=128, min_len=25, max_len=40, seed=6)
    user_dict = {100 + 3 * u: {"items": items[u], "ratings": ratings[u]} for u in range(n_users)}
    ids = list(user_dict)
    env = FrameEnv.from_user_dict(torch.from_numpy(table), user_dict, ids[:6], ids[6:], frame_size=F, batch_size=4, device=cuda,
                                  rows_per_batch=rows_per_batch)
    index = RT.FlatIndex(env.table, "L2")
    sl = env.store.slots(ids[7:10])
    cases = [(env.test_batch(), None, None), (env.collate_users(ids[2:5]), ids[2:5], None),
             (env.collate_slots(sl, ids[7:10]), ids[7:10], None), (env.collate_slots(sl), ids[7:10], sl)]
    store_items = env.store.items.cpu().numpy()
    for batch, users, slots in cases:
        rows = batch["action"].shape[0]
        assert rows == 37 if rows_per_batch else rows > 0
        kw = {} if slots is None else {"slots": slots}
        targets = env.target_items(batch, **kw)
        assert torch.equal(env.table[targets], batch["action"])
        users = batch["meta"]["users"].tolist() if users is None else users
        # per row: its user's history before its target (row r of a user targets position F + r)
        want = [user_dict[u]["items"][:F + r].tolist() for u in users for r in range(len(user_dict[u]["items"]) - F)][:rows]
        for keep_targets in (True, False):
            seen = env.seen_items(batch, keep_targets=keep_targets, **kw)
            assert isinstance(seen, RT.SeenItems) and seen.rows == rows
            assert seen.ids.data_ptr() == env.store.items.data_ptr()     # the store's items themselves: no copy
            st, ln = seen.starts.cpu().numpy(), seen.lengths.cpu().numpy()
            assert [store_items[s:s + n].tolist() for s, n in zip(st, ln)] == want
            assert (seen.keep is None) == (not keep_targets)
            tg = targets.cpu().numpy()
            words = _words(seen.mask(n_items))
            assert np.array_equal(words, S.mask_words(want, n_items, tg if keep_targets else None))
            for b in range(rows):                                        # every window item is set, except a kept target
                for i in want[b][-F:]:
                    assert (int(words[b, i >> 6]) >> (i & 63)) & 1 == (0 if keep_targets and i == tg[b] else 1)
            assert index.rank_of(batch["action"], targets, exclude=seen).cpu().tolist() == [0] * rows
            _, found = index.search(batch["action"], 10, exclude=seen)
            found = found.cpu().numpy()
            for b in range(rows):
                gone = set(want[b]) - ({int(tg[b])} if keep_targets else set())
                assert not gone & set(found[b].tolist()) and (found[b] >= 0).all()
                if keep_targets:
                    assert found[b, 0] == tg[b]                          # L2 under its own action: the target is nearest
    with pytest.raises(ValueError):
        env.seen_items(cases[3][0])                      # its users are slots, which are not user ids of this store
    batch = cases[1][0]
    with pytest.raises(ValueError):
        env.seen_items({"action": batch["action"], "meta": {"users": batch["meta"]["users"], "sizes": batch["meta"]["sizes"] + 1}})
