"""GPU: recnn.data.db_con (the reference's MilvusConnection over FlatIndex) and the top-K statistics of csrc/divstats.hip
(`recnn_amd.retrieval.topk_stats`, `DiversityMeter`) against the numpy restatement in tests/diversity_reference.py.

The search must be bit-equal to `FlatIndex.search` (itself held to the oracle by tests/test_gpu_retrieval.py).  Counts are exact.
Row statistics: kernel and numpy are both two-pass float64 computations on the same float32 inputs; with u = 2^-53 and
gamma = k u / (1 - k u) each side's mean is within gamma max|x| and each side's standard deviation within about
2 gamma (max|x| + std) of the exact value, so per row |row_mean - ref| <= 4 gamma max|x_row| and
|row_std - ref| <= 8 gamma (max|x_row| + ref_std), x the (square rooted) row.  The bounds are derived, not measured."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import diversity_reference as R

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 37), (50, 20, 26744), (2048, 10, 5000), (4099, 64, 26744)]          # (B, k, N)


def _table(N, cuda, seed=0):
    return torch.randn(N, 128, generator=torch.Generator().manual_seed(seed + N)).to(cuda)


def _queries(B, seed=1):
    return torch.randn(B, 128, generator=torch.Generator().manual_seed(seed + B)) * 0.7


def _env_like(table):
    return SimpleNamespace(base=SimpleNamespace(embeddings=table))


def _search(B, k, N, cuda, metric="L2"):
    from recnn_amd.retrieval import FlatIndex
    return FlatIndex(_table(N, cuda), metric).search(_queries(B).to(cuda), k)


def _check_rows(st, dist, k, sqrt, label):
    """row_mean / row_std of a TopkStats against numpy within the derived per-row bounds; prints the worst used share."""
    _, m_ref, s_ref, x = R.topk_stats(dist.cpu().numpy(), np.zeros(dist.shape, np.int64), 1, sqrt)
    m, s = st.row_mean.cpu().numpy(), st.row_std.cpu().numpy()
    assert m.dtype == np.float64 and s.dtype == np.float64 and m.shape == m_ref.shape == s.shape
    nan = np.isnan(m_ref)                                                   # NaN where numpy's are, bounded elsewhere
    assert np.array_equal(np.isnan(m), nan) and np.array_equal(np.isnan(s), np.isnan(s_ref)) and np.array_equal(np.isnan(s_ref), nan)
    m, s, m_ref, s_ref, x = m[~nan], s[~nan], m_ref[~nan], s_ref[~nan], x[~nan]
    if m.size == 0:
        return m, s
    g, mx = R.gamma(k), np.abs(x).max(axis=1)
    b_mean, b_std = 4 * g * mx, 8 * g * (mx + s_ref)
    e_mean, e_std = np.abs(m - m_ref), np.abs(s - s_ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"{label}: mean err / bound max {np.max(np.where(b_mean > 0, e_mean / b_mean, 0.0)):.3f}, "
              f"std err / bound max {np.max(np.where(b_std > 0, e_std / b_std, 0.0)):.3f}")
    assert np.all(e_mean <= b_mean), (label, float((e_mean - b_mean).max()))
    assert np.all(e_std <= b_std), (label, float((e_std - b_std).max()))
    return m, s


def _check_overall(mean, std, dist, k, sqrt):
    """`DiversityMeter.mean / std` (or totals / rows) against numpy's D.mean(axis=1).mean() / D.std(axis=1).mean(): the sum of B
    doubles is allowed 4 B u max|row value|, on top of the largest per-row bound of `_check_rows`."""
    _, m_ref, s_ref, x = R.topk_stats(dist.cpu().numpy(), np.zeros(dist.shape, np.int64), 1, sqrt)
    B, g, mx = len(m_ref), R.gamma(k), np.abs(x).max()
    assert abs(mean - m_ref.mean()) <= 4 * B * R.U * np.abs(m_ref).max() + 4 * g * mx
    assert abs(std - s_ref.mean()) <= 4 * B * R.U * s_ref.max() + 8 * g * (mx + s_ref.max())


@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_search_through_the_references_interface(cuda, metric):
    from recnn.data.db_con import MetricType, MilvusConnection, SearchResult
    from recnn_amd import _lib as L
    from recnn_amd.retrieval import FlatIndex
    for N in (37, 5000, 26744):
        table = _table(N, cuda)
        name = f"movies_{metric}"
        con = MilvusConnection(_env_like(table), name=name, param={"metric_type": MetricType[metric]})
        assert con.name == name and con.statuses["created_collection"].OK() and con.get_log() is con.statuses
        assert con.client.has_collection(name)[1] is True and con.client.has_collection("other")[1] is False
        index = FlatIndex(table, metric)
        for B in (1, 50, 2048):
            q = _queries(B)
            for topk in (1, 10, 20, 64):
                if topk > N:                                               # topk.hip's existing limit, with its existing error
                    with pytest.raises(L.RecnnHipError):
                        index.search(q.to(cuda), topk)
                    with pytest.raises(L.RecnnHipError):
                        con.search(q.numpy(), topk)
                    continue
                d_ref, i_ref = index.search(q.to(cuda), topk)
                forms = {"numpy": q.numpy(), "cpu tensor": q, "gpu tensor": q.to(cuda), "list": q.numpy().tolist()}
                if B == 2048 and topk != 20:
                    del forms["list"]                                      # a 2048 x 128 nested list once is enough
                for form, vecs in forms.items():
                    res = con.search(vecs, topk=topk)
                    assert isinstance(res, SearchResult) and con.statuses["last_search"].OK()
                    ids, dist = res.id(cuda), res.dist(cuda)
                    assert ids.dtype == torch.int64 and dist.dtype == torch.float32 and ids.is_cuda and dist.is_cuda
                    assert tuple(ids.shape) == (B, topk) == tuple(dist.shape)
                    assert torch.equal(ids, i_ref), (N, B, topk, form)
                    assert torch.equal(dist.view(torch.int32), d_ref.view(torch.int32)), (N, B, topk, form)
                    assert res.id(cuda).data_ptr() == ids.data_ptr()       # already there: no copy
                if B <= 50:
                    assert res.id_array == i_ref.tolist() and res.distance_array == d_ref.tolist()
                    assert res.id("cpu").device.type == "cpu" and torch.equal(res.id("cpu"), i_ref.cpu())
                    status, results = con.client.search(collection_name=name, query_records=q.numpy(), top_k=topk,
                                                        params={"nprobe": 16})
                    assert status.OK()
                    assert results.id_array == i_ref.tolist() and results.distance_array == d_ref.tolist()
        one = con.search(q[0].numpy(), topk=5, search_param={"nprobe": 32})   # a single [dim] vector
        assert torch.equal(one.id(cuda), index.search(q[:1].to(cuda), 5)[1])
    # the table is moved to the GPU once and the environment is left alone
    cpu_table = _table(5000, cuda).cpu()
    env = _env_like(cpu_table)
    con = MilvusConnection(env, param={"metric_type": metric, "dimension": 128})
    assert env.base.embeddings is cpu_table and not cpu_table.is_cuda
    assert torch.equal(con.search(_queries(50)).id(cuda), FlatIndex(cpu_table.to(cuda), metric).search(_queries(50).to(cuda), 10)[1])


def _adversarial(B, k, N, cuda):
    same = torch.arange(N - k, N, dtype=torch.int64).flip(0).repeat(B, 1).to(cuda)       # k items get B each
    last = torch.full((B, k), N - 1, dtype=torch.int64, device=cuda)                     # one item gets B k
    return {"identical rows": same, "all N-1": last}


@pytest.mark.parametrize("B,k,N", CASES)
def test_counts_are_exact(cuda, B, k, N):
    from recnn_amd.retrieval import DiversityMeter, topk_stats
    dist, real = _search(B, k, N, cuda)
    for label, ids in {"search": real, **_adversarial(B, k, N, cuda)}.items():
        h = ids.cpu().numpy()
        ref = np.bincount(h.ravel(), minlength=N)
        st = topk_stats(dist, ids, N)
        assert st.counts.dtype == torch.int32 and tuple(st.counts.shape) == (N,)
        assert np.array_equal(st.counts.cpu().numpy(), ref), label
        assert st.totals.cpu().numpy()[2:].tolist() == [B, 0]
        meter = DiversityMeter(N)
        meter.update(dist, ids)
        u, c = meter.recommended()
        u_ref, c_ref = np.unique(h, return_counts=True)
        assert u.dtype == np.int64 and c.dtype == np.int64
        assert np.array_equal(u, u_ref) and np.array_equal(c, c_ref), label
        n, how_many = meter.counts_of_counts()
        n_ref, how_ref = np.unique(ref[ref > 0], return_counts=True)
        assert np.array_equal(n, n_ref) and np.array_equal(how_many, how_ref), label
        assert meter.rows == B
    if B * k > 1:
        assert len(np.unique(real.cpu().numpy())) > 1


@pytest.mark.parametrize("B,k,N", CASES)
def test_row_statistics_within_the_derived_bounds(cuda, B, k, N):
    from recnn_amd.retrieval import topk_stats
    for metric, sqrt in (("L2", False), ("L2", True), ("IP", False)):
        dist, ids = _search(B, k, N, cuda, metric)
        if sqrt:
            assert float(dist.min()) >= 0.0                                 # topk.hip clamps L2 at 0: no NaN from rounding
        st = topk_stats(dist, ids, N, sqrt=sqrt)
        m, s = _check_rows(st, dist, k, sqrt, f"B={B} k={k} N={N} {metric} sqrt={sqrt}")
        if k == 1:
            assert np.all(s == 0.0)
            if not sqrt:
                assert np.array_equal(m, dist.cpu().numpy().astype(np.float64)[:, 0])
        tot = st.totals.cpu().numpy()
        for got, rows in ((tot[0], m), (tot[1], s)):                        # the sum of B doubles
            assert abs(got / B - rows.mean()) <= 4 * B * R.U * np.abs(rows).max()
        _check_overall(tot[0] / tot[2], tot[1] / tot[2], dist, k, sqrt)


def test_equal_distances_have_zero_std(cuda):
    from recnn_amd.retrieval import FlatIndex, topk_stats
    table = np.zeros((700, 128), dtype=np.float32)
    table[:, 0] = np.arange(700) % 7                                        # 100 exact duplicates of each of 7 rows
    q = np.zeros((3, 128), dtype=np.float32)
    q[:, 0] = [1.0, -1.0, 0.5]
    k = 12
    for metric in ("L2", "IP"):
        d, i = FlatIndex(torch.from_numpy(table).to(cuda), metric).search(torch.from_numpy(q).to(cuda), k)
        h = d.cpu().numpy()
        assert np.all(h == h[:, :1])                                        # k duplicates: one distance per row
        for sqrt in ((False, True) if metric == "L2" else (False,)):
            st = topk_stats(d, i, 700, sqrt=sqrt)
            assert np.all(st.row_std.cpu().numpy() == 0.0), (metric, sqrt)
            x = np.sqrt(h[:, 0].astype(np.float64)) if sqrt else h[:, 0].astype(np.float64)
            assert np.array_equal(st.row_mean.cpu().numpy(), x)             # 0, 1, 0.25 and their roots: every sum is exact
    # a constant row of a value whose multiples are not representable in float32 still has std 0 (the sums run in double)
    d = torch.full((5, 64), 0.1, dtype=torch.float32, device=cuda)
    st = topk_stats(d, torch.zeros(5, 64, dtype=torch.int64, device=cuda), 3)
    assert np.all(st.row_std.cpu().numpy() == 0.0) and np.all(st.row_mean.cpu().numpy() == float(np.float32(0.1)))


def test_nan_rows(cuda):
    from recnn_amd.retrieval import FlatIndex, topk_stats
    N, B = 40, 33
    table = _table(N, cuda).clone()
    table[7] = 0.0                                                          # cosine against a zero row is NaN, ranked last
    dist, ids = FlatIndex(table, "cosine").search(_queries(B).to(cuda), N)
    h = dist.cpu().numpy()
    assert np.isnan(h[:, -1]).all() and not np.isnan(h[:, :-1]).any() and (ids[:, -1] == 7).all()
    mixed = dist.clone()
    mixed[::2, -1] = 1.0                                                    # every other row finite again
    for d in (dist, mixed):
        st = topk_stats(d, ids, N)
        c_ref, m_ref, s_ref, _ = R.topk_stats(d.cpu().numpy(), ids.cpu().numpy(), N)
        assert np.isnan(m_ref).sum() == np.isnan(s_ref).sum() == (B if d is dist else B // 2)
        m, _ = _check_rows(st, d, N, False, f"cosine k=N={N}, {int(np.isnan(m_ref).sum())} NaN rows")
        assert m.size == B - np.isnan(m_ref).sum() and np.isnan(st.row_mean.cpu().numpy()).sum() == np.isnan(m_ref).sum()
        assert np.array_equal(st.counts.cpu().numpy(), c_ref) and np.all(c_ref == B)


def test_accumulation_and_determinism(cuda):
    from recnn_amd.retrieval import DiversityMeter, topk_stats
    sizes, k, N = [700, 129, 64, 300, 1], 20, 5000
    B = sum(sizes)
    dist, ids = _search(B, k, N, cuda)
    for sqrt in (False, True):
        meters = [DiversityMeter(N, sqrt=sqrt), DiversityMeter(N, sqrt=sqrt)]
        rows = [[], []]
        for w, meter in enumerate(meters):
            r0 = 0
            for n in sizes:
                st = meter.update(dist[r0:r0 + n], ids[r0:r0 + n])
                rows[w].append((st.row_mean, st.row_std))
                r0 += n
        whole = topk_stats(dist, ids, N, sqrt=sqrt)
        assert torch.equal(meters[0].counts, whole.counts)
        m_all = torch.cat([m for m, _ in rows[0]]).cpu().numpy()
        s_all = torch.cat([s for _, s in rows[0]]).cpu().numpy()
        assert np.array_equal(m_all, whole.row_mean.cpu().numpy())          # a row's arithmetic does not depend on its batch
        assert np.array_equal(s_all, whole.row_std.cpu().numpy())
        assert meters[0].rows == B
        assert abs(meters[0].mean - np.mean(m_all)) <= 4 * B * R.U * np.abs(m_all).max()
        assert abs(meters[0].std - np.mean(s_all)) <= 4 * B * R.U * np.abs(s_all).max()
        assert np.array_equal(meters[0].counts.cpu().numpy(), R.topk_stats(dist.cpu().numpy(), ids.cpu().numpy(), N, sqrt)[0])
        _check_overall(meters[0].mean, meters[0].std, dist, k, sqrt)
        # two meters fed the same batches: the same bits
        assert torch.equal(meters[0].totals.view(torch.int64), meters[1].totals.view(torch.int64))
        for (m0, s0), (m1, s1) in zip(*rows):
            assert torch.equal(m0.view(torch.int64), m1.view(torch.int64)) and torch.equal(s0.view(torch.int64), s1.view(torch.int64))
        assert torch.equal(meters[0].counts, meters[1].counts)
        meters[0].reset()
        assert not meters[0].counts.any() and not meters[0].totals.any()
        assert meters[0].recommended()[0].size == 0


def test_bad_ids_are_reported_not_counted(cuda):
    from recnn_amd.retrieval import DiversityMeter
    B, k, N = 50, 20, 5000
    dist, ids = _search(B, k, N, cuda)
    ids = ids.clone()
    ids[3, 4] = N
    ids[49, 19] = -1
    meter = DiversityMeter(N)
    meter.update(dist, ids)
    assert int(meter.counts.sum()) == B * k - 2
    assert meter.totals.cpu().numpy()[2:].tolist() == [B, 2]
    for read in (lambda: meter.mean, lambda: meter.std, meter.recommended, meter.counts_of_counts):
        with pytest.raises(ValueError, match="2"):
            read()
    meter.reset()
    meter.update(dist, _search(B, k, N, cuda)[1])
    assert np.isfinite(meter.mean)


def test_whole_path_once(cuda):
    """Actor -> MilvusConnection.search -> DiversityMeter, the notebooks' flow with every state of the batch."""
    from recnn.data.db_con import MetricType, MilvusConnection
    from recnn_amd.nn import Actor
    from recnn_amd.retrieval import DiversityMeter
    torch.manual_seed(0)
    N, B, k = 26744, 2048, 20
    actor = Actor(1290, 128, 256).to(cuda).eval()
    state = torch.randn(B, 1290, generator=torch.Generator().manual_seed(3)).to(cuda)
    with torch.no_grad():
        actions = actor(state)
    con = MilvusConnection(_env_like(_table(N, cuda)), name="movies_L2", param={"metric_type": MetricType.L2})
    result = con.search(actions, topk=k)
    for sqrt in (False, True):
        meter = DiversityMeter(N, sqrt=sqrt)
        st = meter.update(result.dist(cuda), result.id(cuda))
        _check_rows(st, result.dist(cuda), k, sqrt, f"whole path sqrt={sqrt}")
        c_ref = R.topk_stats(result.dist("cpu").numpy(), result.id("cpu").numpy(), N, sqrt)[0]
        _check_overall(meter.mean, meter.std, result.dist(cuda), k, sqrt)
        u, c = meter.recommended()
        u_ref, c_ref2 = np.unique(result.id("cpu").numpy(), return_counts=True)
        assert np.array_equal(u, u_ref) and np.array_equal(c, c_ref2) and int(c.sum()) == B * k
        assert np.array_equal(meter.counts.cpu().numpy(), c_ref)
