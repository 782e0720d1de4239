"""CPU: the ranking helper (tests/rank_reference.py) against scipy, metric-name parsing of recnn_amd.retrieval, and the
argument checks of the recnn_dist_* entry points (include/recnn_hip.h section 7), which run before any HIP call."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.spatial import distance

import rank_reference as R

CASES = [("sqeuclidean", None), ("euclidean", None), ("cityblock", None), ("chebyshev", None), ("canberra", None),
         ("braycurtis", None), ("cosine", None), ("correlation", None), ("minkowski", 1.0), ("minkowski", 1.5),
         ("minkowski", 3.0), ("minkowski", np.inf), ("minkowski", None)]


def _data(seed, B=9, N=40):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((B, 128)).astype(np.float32)
    t = rng.standard_normal((N, 128)).astype(np.float32)
    q[1] = 0.0                       # zero query row
    t[3] = 0.0                       # zero item row: with q[1] a zero pair
    t[5] = 0.1                       # constant rows
    q[2] = 3.0
    t[7] = t[8]                      # duplicated items
    q[4] = t[11]                     # a query equal to an item
    return q, t


def _scipy(q, t, metric, p):
    kw = {} if p is None else {"p": p}
    with np.errstate(divide="ignore", invalid="ignore"):
        return distance.cdist(q.astype(np.float64), t.astype(np.float64), metric, **kw)


@pytest.mark.parametrize("metric,p", CASES)
def test_helper_equals_scipy_cdist(metric, p):
    q, t = _data(0)
    ref = _scipy(q, t, metric, p)
    got = R.cdist(q, t, metric, p)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.allclose(got[ok], ref[ok], rtol=1e-12, atol=1e-12)
    # small chunks give the same values
    assert np.array_equal(R.cdist(q, t, metric, p, chunk=300), got, equal_nan=True)


def test_helper_degenerate_rows_follow_scipy():
    q, t = _data(1)
    cos = R.cdist(q, t, "cosine")
    assert np.isnan(cos[1]).all() and np.isnan(cos[:, 3]).all()           # zero rows
    cor = R.cdist(q, t, "correlation")
    assert np.isnan(cor[2]).all() and np.isnan(cor[:, 5]).all() and np.isnan(cor[:, 3]).all()   # constant rows (0 is one)
    assert np.isnan(R.cdist(q, t, "braycurtis")[1, 3])                   # braycurtis(0, 0)
    assert R.cdist(q, t, "canberra")[1, 3] == 0.0                          # canberra(0, 0)
    assert np.isfinite(R.cdist(q, t, "braycurtis")[1, :3]).all()
    for m in ("cosine", "correlation"):                                     # scipy's clip to [0, 2]
        d = R.cdist(q, t, m)
        assert np.nanmin(d) >= 0.0 and np.nanmax(d) <= 2.0
        assert R.cdist(q[4:5], t[11:12], m)[0, 0] == pytest.approx(0.0, abs=1e-12)


@pytest.mark.parametrize("metric,p", CASES)
def test_rank_equals_the_reference_loop(metric, p):
    """The reference's `rank`: `scores.append([i, metric(emb[i], action)])`, `sorted(..., key=x[1])[:k]` with the scipy
    callable (rows without NaN distances: the reference's sort does not define an order for NaN)."""
    q, t = _data(2)
    q = q[[0, 3, 4, 5, 6]]
    t = np.delete(t, [3, 5], axis=0)
    fn = getattr(distance, metric)
    kw = {} if p is None else {"p": p}
    k = 10
    d, ids = R.rank(q, t, metric, k, p)
    for b in range(q.shape[0]):
        scores = [[i, fn(t[i].astype(np.float64), q[b].astype(np.float64), **kw)] for i in range(t.shape[0])]
        top = sorted(scores, key=lambda x: x[1])[:k]
        assert ids[b].tolist() == [i for i, _ in top], (metric, b)
        assert np.allclose(d[b], [s for _, s in top], rtol=1e-12, atol=1e-12)


def test_rank_nan_last_and_ties_to_smaller_id():
    d = np.array([[0.5, np.nan, 0.2, 0.5, np.nan, 0.2]])
    dist, ids = R.rank_matrix(d, 6)
    assert ids.tolist() == [[2, 5, 0, 3, 1, 4]]
    assert np.isnan(dist[0, 4:]).all()


def test_metric_names_and_scipy_callables():
    from recnn_amd import retrieval as RT
    for name in R.METRICS:
        assert RT.metric_name(name) == name
        assert RT.metric_name(getattr(distance, name)) == name
    for name in ("IP", "L2", "COS"):
        assert RT.metric_name(name) == name
    for bad in ("hamming", "Euclidean", distance.jaccard, None, 3):
        with pytest.raises(ValueError):
            RT.metric_name(bad)
    assert RT.minkowski_p("minkowski", None) == 2.0
    assert RT.minkowski_p("minkowski", 1.5) == 1.5 and RT.minkowski_p("minkowski", math.inf) == math.inf
    for bad in (0.5, math.nan, -1.0):
        with pytest.raises(ValueError):
            RT.minkowski_p("minkowski", bad)
    with pytest.raises(ValueError):
        RT.minkowski_p("canberra", 3.0)


def test_unknown_metric_still_raises_value_error():
    import torch
    from recnn_amd.retrieval import FlatIndex, cdist
    t = torch.zeros(4, 128)
    with pytest.raises(ValueError):
        FlatIndex(t, "hamming")
    with pytest.raises(ValueError):
        cdist(t, t, "L2")


def test_dist_entry_points_reject_bad_arguments():
    from recnn_amd import _lib as L
    lib = L.load()
    buf = (C.c_float * (130 * 128 + 8))()
    base = C.addressof(buf)
    a16 = (base + 15) // 16 * 16
    ids = (C.c_int64 * 64)()
    P = C.c_void_p
    q, t, out = P(a16), P(a16), P(a16)
    nb = C.c_int64()

    def mat(metric=0, p=0.0, q=q, ld=128, B=2, t=t, N=4, E=128, aux=None, out=out, ldo=4, ws=P(a16)):
        return lib.recnn_dist_matrix(q, ld, B, t, N, E, metric, p, aux, out, ldo, ws, None)

    def topk(metric=0, p=0.0, k=3, B=2, N=4, aux=None, ws=P(a16), od=out):
        return lib.recnn_dist_topk(q, 128, B, t, N, 128, metric, p, aux, k, od, ids, ws, None)

    bad = [mat(metric=9), mat(metric=-1), mat(metric=4, p=0.5), mat(metric=4, p=math.nan), mat(q=None), mat(t=None),
           mat(out=None), mat(metric=7), mat(metric=8), mat(E=64), mat(ld=130), mat(q=P(a16 + 4)), mat(t=P(a16 + 8)),
           mat(ldo=3), mat(N=0), mat(B=-1),
           topk(metric=9), topk(metric=4, p=math.nan), topk(k=0), topk(k=65, N=100), topk(k=5), topk(metric=7),
           topk(ws=None), topk(od=None), topk(ws=P(a16 + 4)),
           lib.recnn_dist_item_aux(t, 4, 128, 0, out, None), lib.recnn_dist_item_aux(None, 4, 128, 7, out, None),
           lib.recnn_dist_item_aux(t, 4, 128, 7, None, None), lib.recnn_dist_item_aux(t, 4, 64, 8, out, None),
           lib.recnn_dist_workspace_bytes(2, 4, 9, 0, C.byref(nb)), lib.recnn_dist_workspace_bytes(2, 4, 0, 65, C.byref(nb)),
           lib.recnn_dist_workspace_bytes(2, 4, 0, 1, None), lib.recnn_dist_item_aux_floats(4, 128, 12, C.byref(nb))]
    assert all(rc == -1 for rc in bad), bad
    assert b"dist_" in lib.recnn_last_error()
    # the sizes of what a call needs
    assert lib.recnn_dist_item_aux_floats(10, 128, 7, C.byref(nb)) == 0 and nb.value == 1280
    assert lib.recnn_dist_item_aux_floats(10, 128, 5, C.byref(nb)) == 0 and nb.value == 0
    assert lib.recnn_dist_workspace_bytes(3, 1000, 0, 0, C.byref(nb)) == 0 and nb.value == 0
    assert lib.recnn_dist_workspace_bytes(3, 1000, 8, 0, C.byref(nb)) == 0 and nb.value >= 3 * 128 * 4
    assert lib.recnn_dist_workspace_bytes(3, 1000, 0, 10, C.byref(nb)) == 0 and nb.value >= 3 * 10 * 8
    # an empty batch is a no-op that needs no rows, outputs or workspace
    assert lib.recnn_dist_workspace_bytes(0, 1000, 8, 10, C.byref(nb)) == 0 and nb.value == 0
    assert lib.recnn_dist_matrix(None, 128, 0, t, 4, 128, 0, 0.0, None, None, 4, None, None) == 0
    assert lib.recnn_dist_topk(None, 128, 0, t, 4, 128, 2, 0.0, None, 3, None, None, None, None) == 0
