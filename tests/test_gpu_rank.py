"""GPU: ranking under scipy's metrics (csrc/rank.hip via recnn_amd.retrieval.cdist / FlatIndex) against the float64
restatement of scipy in tests/rank_reference.py.

Value bounds are those derived in DESIGN.md section 11 (REL below; 2e-6 absolute for cosine / correlation); NaN exactly
where the reference has NaN.  `search` must report the bits `cdist` stores for the same pair, so its ids are checked exactly against the float32
matrix, and against the float64 reference wherever neighbouring ranks are separated by more than the bound."""
import numpy as np
import pytest
import torch

import rank_reference as R

pytestmark = pytest.mark.gpu

CASES = [("sqeuclidean", None), ("euclidean", None), ("cityblock", None), ("chebyshev", None), ("canberra", None),
         ("braycurtis", None), ("cosine", None), ("correlation", None), ("minkowski", 1.5), ("minkowski", 3.0)]
IDS = [m if p is None else f"{m}-{p}" for m, p in CASES]


# The bounds derived in DESIGN.md section 11 (u = 2^-24): sums of 128 non-negative terms <= (127 + term error) u relative,
# chebyshev one rounding, braycurtis a quotient of two such sums, minkowski's log2 / exp2 at 1 ulp each; cosine / correlation
# absolute.  Each is no looser than what the issue allows: 2e-5 relative, 1e-4 relative for minkowski, 2e-6 absolute.
REL = {"sqeuclidean": 1e-5, "euclidean": 1e-5, "cityblock": 1e-5, "chebyshev": 1e-6, "canberra": 1e-5, "braycurtis": 2e-5,
       "minkowski": 2e-5}


def bound(metric, p, ref):
    """Largest allowed |gpu - reference| per entry."""
    if metric in ("cosine", "correlation"):
        return np.full_like(ref, 2e-6)
    return REL[metric] * np.abs(ref)


def data(seed, B, N):
    rng = np.random.default_rng(seed)
    q = (rng.standard_normal((B, 128)) * 0.7).astype(np.float32)
    t = rng.standard_normal((N, 128)).astype(np.float32)
    if N > 8:
        t[2] = 0.0                          # zero row: cosine / correlation NaN, braycurtis NaN against a zero query
        t[5] = 0.25                         # constant row: correlation NaN
        t[7] = t[3]                         # duplicate: ties go to the smaller id
    if B > 8:
        q[1] = 0.0
        q[4] = -1.5
        q[6] = t[min(9, N - 1)]             # a query equal to an item
    return q, t


def check_values(got, ref, metric, p):
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    err = np.abs(got.astype(np.float64) - ref)
    b = bound(metric, p, ref)
    assert (err[~nan] <= b[~nan]).all(), float((err[~nan] / np.maximum(b[~nan], 1e-30)).max())


def f32_order(D, k):
    """top-k ids of float32 rows: ascending, NaN last, ties to the smaller id."""
    return np.argsort(D, axis=1, kind="stable")[:, :k]


def check_search(dist, ids, D, q, t, rows, metric, p, k):
    """dist / ids of `search` for query rows `rows` against the GPU matrix D (float32) and the float64 reference."""
    dist, ids, D = dist[rows], ids[rows], D[rows]
    assert np.array_equal(ids, f32_order(D, k))                                     # exact: the same bits rank the same
    assert np.array_equal(dist.view(np.uint32), np.take_along_axis(D, ids, 1).view(np.uint32))
    ref = R.cdist(q[rows], t, metric, p)
    d_ref, i_ref = R.rank_matrix(ref, k)
    true = np.take_along_axis(ref, ids, 1)
    b = bound(metric, p, d_ref)
    fin = ~np.isnan(d_ref)
    assert np.array_equal(np.isnan(true), ~fin)
    assert (np.abs(true - d_ref)[fin] <= 2 * b[fin]).all()                          # inside a tie the distance is right
    # ranks whose neighbours are apart by more than both bounds: the float32 order must be the float64 order.  NaN ranks
    # too: NaN sits at the same entries in both, and both order NaN by id.
    gap_ok = np.ones_like(i_ref, dtype=bool)
    with np.errstate(invalid="ignore"):
        gap = np.abs(np.diff(d_ref, axis=1)) > b[:, 1:] + b[:, :-1]
        nxt = np.sort(ref, axis=1)[:, k] if ref.shape[1] > k else np.full(ref.shape[0], np.inf)
        last = (np.abs(nxt - d_ref[:, -1]) > 2 * b[:, -1]) | (ref.shape[1] <= k)
    gap_ok[:, 1:] &= gap | ~fin[:, 1:]
    gap_ok[:, :-1] &= gap | ~fin[:, 1:]
    gap_ok[:, -1] &= last | np.isnan(nxt)
    gap_ok |= ~fin
    assert np.array_equal(ids[gap_ok], i_ref[gap_ok])
    plain = ~np.isin(rows, [1, 4, 6])                    # the fraction over rows that are not degenerate by construction
    return gap_ok[plain].mean()


@pytest.mark.parametrize("metric,p", CASES, ids=IDS)
@pytest.mark.parametrize("B,N", [(1, 1), (1, 63), (65, 65), (2048, 63), (1, 100001), (65, 26744), (2048, 26744)])
def test_cdist_and_search_match_reference(cuda, metric, p, B, N):
    from recnn_amd.retrieval import FlatIndex, cdist
    q, t = data(B * 7 + N, B, N)
    qg, tg = torch.from_numpy(q).to(cuda), torch.from_numpy(t).to(cuda)
    D = cdist(qg, tg, metric, p).cpu().numpy()
    rows = np.arange(B) if B * N <= 2_000_000 else np.r_[0:8, np.random.default_rng(0).choice(np.arange(8, B), 16, replace=False)]
    check_values(D[rows], R.cdist(q[rows], t, metric, p), metric, p)
    k = min(10, N)
    dist, ids = FlatIndex(tg, metric, p).search(qg, k)
    frac = check_search(dist.cpu().numpy(), ids.cpu().numpy(), D, q, t, rows, metric, p, k)
    if N >= 1000 and len(rows) * k >= 200:
        assert frac > 0.95                                                          # the exact-id comparison is not vacuous


@pytest.mark.parametrize("metric,p", CASES, ids=IDS)
def test_same_bits_at_any_batch_position_and_call(cuda, metric, p):
    from recnn_amd.retrieval import FlatIndex, cdist
    q, t = data(3, 2048, 26744)
    tg = torch.from_numpy(t).to(cuda)
    idx = FlatIndex(tg, metric, p)
    x = q[1500]
    outs = []
    for B, pos in ((1, 0), (65, 37), (2048, 1500)):
        qq = q[:B].copy()
        qq[pos] = x
        qg = torch.from_numpy(qq).to(cuda)
        d, i = idx.search(qg, 16)
        D = cdist(qg, tg, metric, p)
        outs.append((d[pos].cpu().numpy().view(np.uint32), i[pos].cpu().numpy(), D[pos].cpu().numpy().view(np.uint32)))
        if B == 2048:
            d2, i2 = idx.search(qg, 16)                                             # a second call: the same bits
            assert torch.equal(d2.view(torch.int32), d.view(torch.int32)) and torch.equal(i2, i)
            assert torch.equal(cdist(qg, tg, metric, p).view(torch.int32), D.view(torch.int32))
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("p,same", [(1, "cityblock"), (2, "euclidean"), (np.inf, "chebyshev")])
def test_minkowski_special_p_is_bit_identical(cuda, p, same):
    from recnn_amd.retrieval import FlatIndex, cdist
    q, t = data(4, 65, 5000)
    qg, tg = torch.from_numpy(q).to(cuda), torch.from_numpy(t).to(cuda)
    a, b = cdist(qg, tg, "minkowski", p), cdist(qg, tg, same)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    (da, ia), (db, ib) = FlatIndex(tg, "minkowski", p).search(qg, 10), FlatIndex(tg, same).search(qg, 10)
    assert torch.equal(da.view(torch.int32), db.view(torch.int32)) and torch.equal(ia, ib)


@pytest.mark.parametrize("metric,p", CASES, ids=IDS)
def test_limits_and_duplicates(cuda, metric, p):
    from recnn_amd.retrieval import FlatIndex, cdist
    q, t = data(5, 65, 3000)
    qg, tg = torch.from_numpy(q).to(cuda), torch.from_numpy(t).to(cuda)
    D = cdist(qg, tg, metric, p).cpu().numpy()
    def scipy_like(u, v):                                                           # stands in for scipy.spatial.distance.<metric>
        raise AssertionError("never called")
    scipy_like.__name__ = metric
    idx = FlatIndex(tg, scipy_like, p)                                              # a callable resolves by its name
    for k in (1, 64):
        d, i = idx.search(qg, k)
        assert np.array_equal(i.cpu().numpy(), f32_order(D, k))
        assert np.array_equal(d.cpu().numpy().view(np.uint32), np.take_along_axis(D, i.cpu().numpy(), 1).view(np.uint32))
    for N in (1, 50, 64):                                                           # k = N <= 64
        d, i = FlatIndex(tg[:N], metric, p).search(qg, N)
        assert np.array_equal(i.cpu().numpy(), f32_order(D[:, :N], N))
    d, i = idx.search(qg[:0], 5)                                                    # B = 0 is a no-op
    assert d.shape == (0, 5) and i.shape == (0, 5) and cdist(qg[:0], tg, metric, p).shape == (0, 3000)
    dup = np.repeat(t[:7], 100, axis=0)                                             # 100 copies of each of 7 rows
    dup = dup[np.random.default_rng(6).permutation(700)]
    qd = q[8:]                                           # random queries: their distances to the 7 rows are far apart
    d, i = FlatIndex(torch.from_numpy(dup).to(cuda), metric, p).search(torch.from_numpy(qd).to(cuda), 12)
    d_ref, i_ref = R.rank(qd, dup, metric, 12, p)
    assert np.array_equal(i.cpu().numpy(), i_ref)                                   # duplicates: the smaller id first


def test_existing_l2_index_is_unchanged(cuda):
    from oracle import retrieval_oracle as O
    from recnn_amd.retrieval import FlatIndex
    q, t = data(8, 100, 5000)
    idx = FlatIndex(torch.from_numpy(t).to(cuda), "L2")
    assert idx.aux.shape == (5000,)                                                 # the |t|^2 array of topk.hip, not rank.hip's
    d, i = idx.search(torch.from_numpy(q).to(cuda), 10)
    d, i = d.cpu().numpy().astype(np.float64), i.cpu().numpy()
    d_ref, i_ref = O.topk(q, t, "L2", 10)
    tol = 1e-5 * np.abs(d_ref).max()
    assert np.abs(d - d_ref).max() <= tol                                           # squared distances, as faiss reports
    gap_ok = np.ones_like(i_ref, dtype=bool)
    gap = np.diff(d_ref, axis=1) > 4 * tol
    gap_ok[:, 1:] &= gap
    gap_ok[:, :-1] &= gap
    assert np.array_equal(i[gap_ok], i_ref[gap_ok]) and gap_ok.mean() > 0.9
