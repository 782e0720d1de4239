"""GPU: the slate diversifier (csrc/slate.hip): SlateDiversifier.similarity / rerank / ild, and the `diversify`
stage of TwoStageIndex.search and WolpertingerPolicy.recommend, against tests/slate_reference.py.

The similarity is held to float64 within a derived bound; the selection is held to the stated rule over the kernel's own S bit for
bit; integer data is exact end to end."""
import numpy as np
import pytest
import torch

import slate_reference as SR

pytestmark = pytest.mark.gpu

N = 200
ZERO_ROW = 7                       # a planted zero row of the Gaussian table
BS = (1, 5, 33)
KS = (1, 2, 16, 17, 63, 64)
LAMS = (0.0, 0.25, 0.5, 0.7, 1.0)
U = 2.0 ** -24                     # fp32 unit roundoff
G128 = 128 * U / (1 - 128 * U)     # gamma_128: a chain of 128 fused multiply-adds (Higham, Accuracy and Stability, section 3.1)


@pytest.fixture(scope="module")
def RT(cuda):
    from recnn_amd import retrieval
    return retrieval


@pytest.fixture(scope="module")
def gauss(RT, cuda):
    rng = np.random.default_rng(25)
    table = rng.standard_normal((N, 128)).astype(np.float32)
    table[ZERO_ROW] = 0
    dev = torch.from_numpy(table).to(cuda)
    return {"table": table, "dev": dev, "div": {kind: RT.SlateDiversifier(dev, kind) for kind in SR.KINDS}}


def _bits(t):
    """Bit patterns, every NaN as one (the payload and sign of a NaN differ between arithmetic units and mean nothing)."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a = a.astype(np.float32, copy=True)
    a[np.isnan(a)] = np.nan
    return a.view(np.int32)


def _ids(rng, B, K, empties=True):
    """Random ids with repeats (of the row's first id), the zero row now and then, and about one slot in eight empty (-1, N, N + 5)."""
    ids = rng.integers(0, N, size=(B, K))
    ids[:, K // 2:] = np.where(rng.random((B, K - K // 2)) < 0.4, ids[:, :1], ids[:, K // 2:])
    ids[rng.random((B, K)) < 0.05] = ZERO_ROW
    if empties:
        hit = rng.random((B, K)) < 0.125
        if K > 1:
            hit[0, K - 1] = True
        ids[hit] = np.array([-1, N, N + 5])[rng.integers(0, 3, size=int(hit.sum()))]
    return ids


def _rel(rng, B, K):
    """Gaussian relevance with planted NaN, +-inf and +-0."""
    rel = rng.standard_normal((B, K)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    hit = rng.random((B, K)) < 0.15
    rel[hit] = special[rng.integers(0, 5, size=int(hit.sum()))]
    return rel


def sim_bound(table, ids, kind):
    """float64 [B, K, K]: how far the kernel's S may be from the float64 S.

    G is a chain of 128 fused multiply-adds in fp32: |G^ - G| <= gamma_128 * A_ij with A = |X| |X|^T (so n^_i = n_i (1 + d),
    |d| <= gamma_128, as A_ii = n_i).  Every later step is one correctly rounded operation (relative error <= u = 2^-24).
      IP   gamma_128 A_ij
      COS  the two roots carry (1 + gamma_128)^(1/2) (1 + u) each, their product one more u: the denominator is off by a relative
           gamma_128 + 3 u, the quotient adds u:  gamma_128 A_ij / den + |S_ij| (gamma_128 + 4 u)
      L2   n_i + n_j is off by gamma_128 (n_i + n_j) and rounded once (u (n_i + n_j)), 2 G is off by 2 gamma_128 A_ij, the
           difference d is rounded once (u |d|); max(., 0) and the negation add nothing:
           gamma_128 (n_i + n_j + 2 A_ij) + u (n_i + n_j) + u |d_ij|
    each times 1.01 for the second-order terms left out (they are of relative size gamma_128 < 1e-5)."""
    X = SR.gather(table, ids, np.float64)
    G = np.matmul(X, X.transpose(0, 2, 1))
    A = np.matmul(np.abs(X), np.abs(X).transpose(0, 2, 1))
    n = np.einsum("bii->bi", G)
    ni, nj = n[:, :, None], n[:, None, :]
    if kind == "IP":
        return 1.01 * G128 * A
    if kind == "COS":
        den = np.sqrt(ni) * np.sqrt(nj)
        S = SR.similarity(table, ids, "COS", np.float64)
        with np.errstate(all="ignore"):
            return np.where(den > 0, 1.01 * (G128 * A / den + np.abs(S) * (G128 + 4 * U)), 0.0)
    d = (ni + nj) - 2 * G
    return 1.01 * (G128 * (ni + nj + 2 * A) + U * (ni + nj) + U * np.abs(d))


# ---------------------------------------------------------------- 1. the similarity matrix

@pytest.mark.parametrize("kind", SR.KINDS)
@pytest.mark.parametrize("K", KS)
def test_similarity_against_float64_and_its_bits_are_row_local(RT, cuda, gauss, kind, K):
    d, table = gauss["div"][kind], gauss["table"]
    rng = np.random.default_rng(K)
    ids = _ids(rng, 33, K)
    if K > 1:
        ids[1, :2] = (ZERO_ROW, 3)
    empty = (ids < 0) | (ids >= N)
    want, bound = SR.similarity(table, ids, kind, np.float64), sim_bound(table, ids, kind)
    full = None
    for B in reversed(BS):
        t = torch.from_numpy(ids[:B]).to(cuda)
        S = d.similarity(t)
        assert S.dtype == torch.float32 and tuple(S.shape) == (B, K, K)
        got = S.cpu().numpy()
        err = np.abs(got.astype(np.float64) - want[:B])
        assert (err <= bound[:B]).all(), (kind, K, B, float((err - bound[:B]).max()))
        assert np.array_equal(_bits(got), _bits(got.transpose(0, 2, 1)))                 # bitwise symmetric
        assert not got[empty[:B]].any() and not got.transpose(0, 2, 1)[empty[:B]].any()   # empty slots
        if kind == "COS":
            z = ids[:B] == ZERO_ROW
            assert not got[z].any() and not got.transpose(0, 2, 1)[z].any()               # the zero row
        if kind == "L2":
            diag = np.einsum("bii->bi", got)
            assert not diag.any() and not np.signbit(diag).any()
        if full is None:
            full = got                                                                    # B = 33
        else:
            assert np.array_equal(_bits(got), _bits(full[:B]))                            # the same rows in a smaller batch
        # int32 ids, and an id matrix with a row stride, give the same bits
        wide = torch.full((B, K + 7), 3, dtype=torch.int32, device=cuda)
        wide[:, 3:3 + K] = t
        assert np.array_equal(_bits(d.similarity(t.to(torch.int32))), _bits(got))
        assert np.array_equal(_bits(d.similarity(wide[:, 3:3 + K])), _bits(got))
    for b in (0, 17, 32):                                                                 # a row alone
        assert np.array_equal(_bits(d.similarity(torch.from_numpy(ids[b:b + 1]).to(cuda))[0]), _bits(full[b]))
    # one pair of table rows, one bit pattern: whatever the row, the slots or the tile that holds it
    key = (np.where(empty, N, ids)[:, :, None] * (N + 1) + np.where(empty, N, ids)[:, None, :]).ravel()
    order = np.argsort(key, kind="stable")
    key, bits = key[order], _bits(full).ravel()[order]
    same = key[1:] == key[:-1]
    assert same.any() or K == 1
    assert (bits[1:][same] == bits[:-1][same]).all()


# ---------------------------------------------------------------- 2. the selection is the stated rule over the kernel's own S

@pytest.mark.parametrize("kind", SR.KINDS)
@pytest.mark.parametrize("K", KS)
def test_selection_is_the_stated_rule_over_the_kernels_own_similarity(RT, cuda, gauss, kind, K):
    d = gauss["div"][kind]
    rng = np.random.default_rng(100 + K)
    ids, rel = _ids(rng, 33, K), _rel(rng, 33, K)
    rel[2, : min(K, 3)] = (np.nan, -0.0, 0.0)[: min(K, 3)]
    t, r = torch.from_numpy(ids).to(cuda), torch.from_numpy(rel).to(cuda)
    S = d.similarity(t).cpu().numpy()
    wide = torch.zeros(33, K + 5, device=cuda)
    wide[:, 2:2 + K] = r
    for lam in LAMS:
        for normalize in (False, True):
            want = SR.mmr(S, rel, ids, N, K, lam, normalize, np.float32)                  # the first k picks do not depend on k
            for k in sorted({1, min(10, K), K}):
                for B in BS:
                    score, out, slots = d.rerank(r[:B], t[:B], k, lam, normalize)
                    assert score.dtype == torch.float32 and out.dtype == torch.int64 and slots.dtype == torch.int32
                    assert tuple(score.shape) == tuple(out.shape) == tuple(slots.shape) == (B, k)
                    where = (kind, K, lam, normalize, k, B)
                    assert np.array_equal(out.cpu().numpy(), want[1][:B, :k]), where
                    assert np.array_equal(slots.cpu().numpy(), want[2][:B, :k]), where
                    assert np.array_equal(_bits(score), _bits(want[0][:B, :k])), where
            # k defaults to K; a relevance with a row stride and in float64 is taken as well
            for arg in (wide[:, 2:2 + K], r.double()):
                got = d.rerank(arg, t, lam=lam, normalize=normalize)
                assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[2].cpu().numpy(), want[2])
    assert (want[1] == -1).any() or K == 1                                                # some row ran out of slots


# ---------------------------------------------------------------- 3. integer data: exact end to end, ties everywhere

@pytest.mark.parametrize("kind", ["IP", "L2"])
@pytest.mark.parametrize("K", KS)
def test_integer_data_is_exact_end_to_end(RT, cuda, kind, K):
    rng = np.random.default_rng(200 + K)
    table = rng.integers(-3, 4, size=(N, 128)).astype(np.float32)
    d = RT.SlateDiversifier(torch.from_numpy(table).to(cuda), kind)
    ids = _ids(rng, 33, K)
    rel = rng.integers(-8, 9, size=(33, K)).astype(np.float32)
    t, r = torch.from_numpy(ids).to(cuda), torch.from_numpy(rel).to(cuda)
    S64 = SR.similarity(table, ids, kind, np.float64)
    assert np.abs(S64).max() < 2 ** 24                                                    # every partial sum is an integer below 2^24
    assert np.array_equal(d.similarity(t).cpu().numpy().astype(np.float64), S64)
    for lam in (0.25, 0.5):
        want = SR.mmr(S64, rel, ids, N, K, lam, False, np.float64)
        for k in sorted({1, min(10, K), K}):
            for B in BS:
                score, out, slots = d.rerank(r[:B], t[:B], k, lam)
                assert np.array_equal(out.cpu().numpy(), want[1][:B, :k]), (kind, K, lam, k, B)
                assert np.array_equal(slots.cpu().numpy(), want[2][:B, :k])
                assert np.array_equal(score.cpu().numpy().astype(np.float64), want[0][:B, :k])
    mean, _, pairs = SR.ild(S64, ids, N, kind, np.float64)
    got = d.ild(t).cpu().numpy()
    if kind == "IP":                                                                      # integers again: the mean is one division
        assert np.array_equal(got, mean, equal_nan=True)
    assert np.array_equal(np.isnan(got), pairs == 0)


# ---------------------------------------------------------------- 4. end to end on Gaussian data against float64

def test_end_to_end_on_gaussian_data_against_float64(RT, cuda, gauss):
    d, table = gauss["div"]["COS"], gauss["table"]
    B, K, k, lam = 33, 64, 10, 0.5
    rng = np.random.default_rng(4)
    ids = np.stack([rng.permutation(N)[:K] for _ in range(B)])
    rel = rng.standard_normal((B, K)).astype(np.float32)
    S64 = SR.similarity(table, ids, "COS", np.float64)
    score64, out64, slots64, gap = SR.mmr(S64, rel, ids, N, k, lam, False, np.float64, gaps=True)
    # lam = mu = 1/2: both products are exact, m_j is off by at most the largest similarity bound of the row, and the difference,
    # at most max|rel| / 2 + max|S| / 2 in size, is rounded once
    err = 0.5 * sim_bound(table, ids, "COS").max(axis=(1, 2)) + U * (0.5 * np.abs(rel).max(axis=1) + 0.5)
    keep = gap >= 2 * err
    assert (~keep).sum() <= 0.02 * B, (gap, err)
    score, out, slots = d.rerank(torch.from_numpy(rel).to(cuda), torch.from_numpy(ids).to(cuda), k, lam)
    assert np.array_equal(out.cpu().numpy()[keep], out64[keep]) and np.array_equal(slots.cpu().numpy()[keep], slots64[keep])
    assert (np.abs(score.cpu().numpy().astype(np.float64) - score64)[keep] <= err[keep, None]).all()
    # the slate got more diverse than the ten most relevant items, and gave relevance up for it
    top = torch.from_numpy(ids).to(cuda).gather(1, torch.from_numpy(rel).to(cuda).topk(k, dim=1)[1])
    assert float(d.ild(out).mean()) > float(d.ild(top).mean())


# ---------------------------------------------------------------- 5. lam = 1 is the existing rerank

@pytest.mark.parametrize("K", [1, 17, 64])
def test_lam_one_is_critic_index_rerank_bit_for_bit(RT, cuda, gauss, K):
    import recnn_amd
    S_, H = 50, 64
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(K)
        critic = recnn_amd.nn.Critic(S_, 128, H)
        with torch.no_grad():
            critic.linear3.weight.mul_(1e4)                              # (the initial last layer is tiny; any scale will do)
        state = torch.randn(33, S_).to(cuda)
    index = RT.CriticIndex(critic.to(cuda), gauss["dev"])
    t = torch.from_numpy(_ids(np.random.default_rng(K), 33, K)).to(cuda)
    q = index.q_of(state, t)
    for kind in SR.KINDS:
        for k in sorted({1, min(10, K), K}):
            score, out, _ = gauss["div"][kind].rerank(q, t, k, lam=1.0, normalize=False)
            want_q, want_ids = index.rerank(state, t, k)
            assert torch.equal(out, want_ids) and np.array_equal(_bits(score), _bits(want_q))


# ---------------------------------------------------------------- 6. intra-list distance

@pytest.mark.parametrize("kind", SR.KINDS)
def test_ild_is_the_float64_mean_of_the_kernels_own_distances(RT, cuda, gauss, kind):
    d = gauss["div"][kind]
    for K in KS:
        rng = np.random.default_rng(300 + K)
        ids = _ids(rng, 33, K)
        if K > 1:
            ids[3] = -1                                                  # no slot
            ids[4, 1:] = N                                               # one slot
        t = torch.from_numpy(ids).to(cuda)
        S = d.similarity(t).cpu().numpy()
        mean, mass, pairs = SR.ild(S, ids, N, kind, np.float32)          # the kernel's own D_ij, summed exactly, divided once
        for B in BS:
            got = d.ild(t[:B])
            assert got.dtype == torch.float64 and tuple(got.shape) == (B,)
            got = got.cpu().numpy()
            assert np.array_equal(np.isnan(got), pairs[:B] == 0), (kind, K, B)
            ok = pairs[:B] > 0
            # a float64 sum of `pairs` terms in any order is within pairs * 2^-53 * sum|D| of the exact one; then one division
            bound = (pairs[:B] * 2.0 ** -53 * mass[:B]) / np.maximum(pairs[:B], 1) + 2.0 ** -52 * np.abs(mean[:B])
            assert (np.abs(got - mean[:B])[ok] <= bound[ok]).all(), (kind, K, B)
        assert K == 1 or (np.isnan(got[3]) and np.isnan(got[4]))
        assert K > 1 or np.isnan(got).all()


# ---------------------------------------------------------------- 7. TwoStageIndex.search(diversify=), WolpertingerPolicy.recommend

@pytest.fixture(scope="module")
def policy_case(RT, cuda, gauss):
    import recnn_amd
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7)
        actor = recnn_amd.nn.Actor(1290, 128, 256).to(cuda)
        critic = recnn_amd.nn.Critic(1290, 128, 256)
        with torch.no_grad():
            critic.linear3.weight.mul_(1e4)
        state = torch.randn(5, 1290).to(cuda)
    policy = recnn_amd.nn.WolpertingerPolicy(actor, critic.to(cuda), gauss["dev"], n_candidates=64)
    return {"policy": policy, "state": state}


def test_diversify_is_the_calls_composed_by_hand(RT, cuda, gauss, policy_case):
    policy, state = policy_case["policy"], policy_case["state"]
    two, B = policy.index, state.shape[0]
    action = policy.proto_action(state)
    # row 0 has three items left, fewer than k
    ex = RT.SeenItems.from_lists([list(range(3, N))] + [[1, 2, 3]] * (B - 1), device=cuda)
    for exclude in (None, ex):
        cand = two.flat.search(action, 64, exclude)[1]
        q_all, ids_all = two.critic_index.rerank(state, cand)
        today = two.critic_index.rerank(state, cand, 10)
        got = two.search(action, state, 10, exclude)
        assert torch.equal(got[1], today[1]) and np.array_equal(_bits(got[0]), _bits(today[0]))       # diversify=None: as before
        got = policy.recommend(state, 10, exclude)
        assert torch.equal(got[1], today[1]) and np.array_equal(_bits(got[0]), _bits(today[0]))
        for similarity in ("COS", "L2"):
            for lam in (0.3, 1.0):
                _, ids, slots = RT.SlateDiversifier(gauss["dev"], similarity).rerank(q_all, ids_all, 10, lam, normalize=True)
                q = torch.where(slots >= 0, q_all.gather(1, slots.clamp_min(0).long()), torch.full_like(q_all[:, :10], float("-inf")))
                got = two.search(action, state, 10, exclude, diversify=lam, similarity=similarity)
                assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64
                assert torch.equal(got[1], ids) and np.array_equal(_bits(got[0]), _bits(q)), (similarity, lam)
                if similarity == "COS":
                    rec = policy.recommend(state, 10, exclude, diversify=lam)
                    assert torch.equal(rec[1], ids) and np.array_equal(_bits(rec[0]), _bits(q))
                if lam == 1.0:                                           # relevance alone: today's order
                    assert torch.equal(got[1], today[1]) and np.array_equal(_bits(got[0]), _bits(today[0]))
        if exclude is not None:
            assert set(got[1][0, :3].tolist()) == {0, 1, 2} and got[1][0, 3:].tolist() == [-1] * 7
            assert torch.isneginf(got[0][0, 3:]).all() and torch.isfinite(got[0][0, :3]).all()
    assert two.diversifier("COS") is two.diversifier("COS") and two.diversifier("COS").kind == "COS"  # built once and kept
    with pytest.raises(ValueError, match="k must be an integer from 1 to the 64 candidates"):
        two.search(action, state, 65, diversify=0.5)
    with pytest.raises(ValueError, match=r"lam must be in \[0, 1\]"):
        two.search(action, state, 10, diversify=1.5)
    with pytest.raises(ValueError, match="similarity must be one of"):
        two.search(action, state, 10, diversify=0.5, similarity="L1")


# ---------------------------------------------------------------- 8. refusals, empty batches, more rows than one launch takes

def test_refusals_name_the_argument(RT, cuda, gauss):
    d = gauss["div"]["COS"]
    ids = torch.zeros(4, 10, dtype=torch.int64, device=cuda)
    rel = torch.zeros(4, 10, device=cuda)
    with pytest.raises(ValueError, match="K = 65 candidates per row; a slate takes at most 64"):
        d.similarity(torch.zeros(2, 65, dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError, match="K = 65"):
        d.rerank(torch.zeros(2, 65, device=cuda), torch.zeros(2, 65, dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError, match="K = 65"):
        d.ild(torch.zeros(2, 65, dtype=torch.int64, device=cuda))
    for k in (0, 11, -1, 2.5):
        with pytest.raises(ValueError, match="k must be an integer from 1 to the 10 candidates"):
            d.rerank(rel, ids, k)
    for lam in (-0.1, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"lam must be in \[0, 1\]"):
            d.rerank(rel, ids, 5, lam)
    with pytest.raises(ValueError, match="similarity must be one of"):
        RT.SlateDiversifier(gauss["dev"], "cosine")
    with pytest.raises(ValueError, match="ids must be an integer tensor"):
        d.similarity(ids.float())
    with pytest.raises(ValueError, match="the ids live on cpu, the index on cuda"):
        d.ild(ids.cpu())
    with pytest.raises(ValueError, match="the relevance lives on cpu"):
        d.rerank(rel.cpu(), ids)
    with pytest.raises(ValueError, match="3 rows of relevance but ids of 4 rows"):
        d.rerank(rel[:3], ids)
    from recnn_amd import _lib as L
    with pytest.raises(L.RecnnHipError, match="no CPU fallback"):
        RT.SlateDiversifier(gauss["dev"].cpu())
    # B = 0: empty tensors, no launch
    none = ids[:0]
    assert tuple(d.similarity(none).shape) == (0, 10, 10) and tuple(d.ild(none).shape) == (0,)
    score, out, slots = d.rerank(rel[:0], none, 3)
    assert tuple(score.shape) == tuple(out.shape) == tuple(slots.shape) == (0, 3)


def test_more_rows_than_one_launch_takes(RT, cuda, gauss):
    """2^20 rows go into one launch; the call loops above that.  K = 2, lam = 1: the more relevant of the two slots first."""
    d = gauss["div"]["IP"]
    B = (1 << 20) + 37
    g = torch.Generator(device="cpu").manual_seed(1)
    ids = torch.randint(0, N, (B, 2), generator=g, dtype=torch.int32).to(cuda)
    ids[::5, 1] = -1
    rel = torch.rand(B, 2, generator=g)
    rel[:, 1] = rel[:, 0] + torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0)      # no ties
    rel = rel.to(cuda)
    score, out, slots = d.rerank(rel, ids, 2, lam=1.0)
    first = (rel[:, 1] > rel[:, 0]) & (ids[:, 1] >= 0)
    want_slots = torch.stack([first.int(), 1 - first.int()], 1)
    want_slots[:, 1] = torch.where(ids[:, 1] >= 0, want_slots[:, 1], torch.full_like(want_slots[:, 1], -1))
    assert torch.equal(slots, want_slots)
    want_ids = torch.where(want_slots >= 0, ids.long().gather(1, want_slots.clamp_min(0).long()), torch.full_like(want_slots, -1).long())
    assert torch.equal(out, want_ids)
    want_score = torch.where(want_slots >= 0, rel.gather(1, want_slots.clamp_min(0).long()), torch.full_like(rel, float("-inf")))
    assert torch.equal(score, want_score)
    ild = d.ild(ids)
    assert torch.equal(torch.isnan(ild), ids[:, 1] < 0)
    tail = slice(B - 40, B)                                              # rows of the second launch
    assert torch.equal(torch.nan_to_num(ild[tail]), torch.nan_to_num(d.ild(ids[tail])))
    assert torch.equal(d.similarity(ids)[tail], d.similarity(ids[tail]))
