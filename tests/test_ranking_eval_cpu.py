"""CPU: the ranking-evaluation helper (tests/ranking_eval_reference.py) against a stable sort, the argument checks of the target-rank
and rank-metrics entry points (include/recnn_hip.h section 11), which run before any HIP call, and the no-GPU behaviour of
FlatIndex.rank_of / target_ranks / RankingMeter."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ranking_eval_reference as R


@pytest.mark.parametrize("larger", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ranks_from_keys_equals_position_in_a_stable_sort(seed, larger):
    rng = np.random.default_rng(seed)
    B, N = 7, 23
    keys = rng.integers(-3, 4, size=(B, N)).astype(np.float32)            # few values: many ties
    keys[rng.random((B, N)) < 0.15] = np.nan
    keys[0, :] = np.nan                                                    # a row of NaNs: ordered by id
    keys[1, ::2] = 0.0
    keys[1, 1::4] = -0.0                                                   # -0 counts as +0
    keys[2, 5] = np.inf
    keys[2, 6] = -np.inf
    targets = rng.integers(0, N, size=B)
    targets[3], targets[4] = 0, N - 1
    got = R.ranks_from_keys(keys, targets, larger_is_better=larger)
    for b in range(B):
        k = keys[b].astype(np.float64) + 0.0                               # -0 + 0 = +0
        nan = np.isnan(k)
        filled = np.where(nan, 0.0, -k if larger else k)
        order = np.lexsort((np.arange(N), filled, nan))                    # NaN last, then the key, then the id
        assert got[b] == int(np.nonzero(order == targets[b])[0][0]), (b, targets[b])
    bad = R.ranks_from_keys(keys, np.array([-1, N, 0, 1, 2, 3, 4]), larger)
    assert bad[0] == -1 and bad[1] == -1 and (bad[2:] >= 0).all()


def test_meter_reference_by_hand():
    ref = R.meter_reference([0, 1, 9, 10, -1, 5000], None, (1, 10, 100))
    assert ref["rows"] == 5 and ref["invalid"] == 1 and ref["rank_sum"] == 5020
    assert ref["hits"] == {1: 1, 10: 3, 100: 4}
    assert ref["mrr_sum"] == pytest.approx(1 + 1 / 2 + 1 / 10 + 1 / 11 + 1 / 5001, rel=1e-15)
    assert ref["ndcg_sum"][10] == pytest.approx(1 + 1 / math.log2(3) + 1 / math.log2(11), rel=1e-15)
    masked = R.meter_reference([0, 1, 9, 10, -1, 5000], [1, 0, 1, 1, 0, 1], (1, 10, 100))
    assert masked["rows"] == 4 and masked["invalid"] == 0 and masked["hits"] == {1: 1, 10: 2, 100: 3}
    assert masked["hit_rate"][10] == 0.5 and masked["mean_rank"] == 5019 / 4


def test_target_rank_entry_points_reject_bad_arguments():
    from recnn_amd import _lib as L
    lib = L.load()
    buf = (C.c_float * (130 * 128 + 8))()
    a16 = (C.addressof(buf) + 15) // 16 * 16
    P = C.c_void_p
    q, t, out, ws = P(a16), P(a16), P(a16), P(a16)
    tg = (C.c_int64 * 8)()
    nb = C.c_int64()

    def dist(metric=0, p=0.0, q=q, ld=128, B=2, t=t, N=4, E=128, aux=None, tg=tg, out=out, ws=ws):
        return lib.recnn_dist_target_rank(q, ld, B, t, N, E, metric, p, aux, tg, out, ws, None)

    def topk(metric=0, q=q, ld=128, B=2, t=t, N=4, E=128, aux=None, tg=tg, out=out, ws=ws):
        return lib.recnn_topk_target_rank(q, ld, B, t, N, E, metric, aux, tg, out, ws, None)

    bad = [dist(q=None), dist(t=None), dist(tg=None), dist(out=None), dist(ws=None), dist(E=64), dist(metric=9), dist(metric=-1),
           dist(metric=4, p=0.5), dist(metric=4, p=math.nan), dist(ld=130), dist(metric=7), dist(metric=8), dist(N=0), dist(B=-1),
           dist(q=P(a16 + 4)), dist(ws=P(a16 + 4)),
           topk(q=None), topk(t=None), topk(tg=None), topk(out=None), topk(ws=None), topk(E=64), topk(metric=3), topk(metric=-1),
           topk(ld=130), topk(metric=1), topk(metric=2), topk(N=0), topk(B=-1), topk(q=P(a16 + 4)),
           lib.recnn_dist_target_rank_workspace_bytes(2, 4, 9, C.byref(nb)), lib.recnn_dist_target_rank_workspace_bytes(2, 4, 0, None),
           lib.recnn_dist_target_rank_workspace_bytes(2, 0, 0, C.byref(nb)), lib.recnn_topk_target_rank_workspace_bytes(2, 4, None),
           lib.recnn_topk_target_rank_workspace_bytes(-1, 4, C.byref(nb)), lib.recnn_topk_target_rank_workspace_bytes(2, 0, C.byref(nb))]
    assert all(rc == -1 for rc in bad), bad
    assert b"target_rank" in lib.recnn_last_error()
    # sizes: one int32 per (row, split), plus the prepared query rows of cosine / correlation
    assert lib.recnn_dist_target_rank_workspace_bytes(3, 1000, 0, C.byref(nb)) == 0 and nb.value >= 3 * 4
    assert lib.recnn_dist_target_rank_workspace_bytes(3, 1000, 7, C.byref(nb)) == 0 and nb.value >= 3 * 128 * 4 + 3 * 4
    assert lib.recnn_topk_target_rank_workspace_bytes(3, 1000, C.byref(nb)) == 0 and nb.value >= 3 * 4
    assert lib.recnn_topk_target_rank_workspace_bytes(2048, 26744, C.byref(nb)) == 0 and 2048 * 4 <= nb.value <= 2048 * 4 * 64
    # an empty batch is a no-op that needs no rows, outputs or workspace
    assert lib.recnn_dist_target_rank_workspace_bytes(0, 1000, 8, C.byref(nb)) == 0 and nb.value == 0
    assert lib.recnn_topk_target_rank_workspace_bytes(0, 1000, C.byref(nb)) == 0 and nb.value == 0
    assert lib.recnn_dist_target_rank(None, 128, 0, t, 4, 128, 0, 0.0, None, None, None, None, None) == 0
    assert lib.recnn_topk_target_rank(None, 128, 0, t, 4, 128, 0, None, None, None, None, None) == 0


def test_rank_metrics_rejects_bad_arguments():
    from recnn_amd import _lib as L
    lib = L.load()
    buf = (C.c_double * 64)()
    P = C.c_void_p
    a = P(C.addressof(buf))
    nb = C.c_int64()

    def ks(*v):
        return (C.c_int32 * max(len(v), 1))(*v)

    def met(ranks=a, mask=None, n=4, k=ks(1, 5, 10), n_ks=3, f=a, i=a, ws=a):
        return lib.recnn_rank_metrics(ranks, mask, n, k, n_ks, f, i, ws, None)

    bad = [met(ranks=None), met(k=None), met(f=None), met(i=None), met(ws=None), met(n=-1), met(n_ks=0),
           met(k=ks(*range(1, 10)), n_ks=9), met(k=ks(5, 5, 10)), met(k=ks(10, 5, 20)), met(k=ks(0, 5, 10)), met(k=ks(-3), n_ks=1),
           met(ws=P(C.addressof(buf) + 4)), lib.recnn_rank_metrics_workspace_bytes(4, None),
           lib.recnn_rank_metrics_workspace_bytes(-1, C.byref(nb))]
    assert all(rc == -1 for rc in bad), bad
    assert b"rank_metrics" in lib.recnn_last_error()
    assert lib.recnn_rank_metrics_workspace_bytes(1, C.byref(nb)) == 0 and nb.value > 0
    small = nb.value
    assert lib.recnn_rank_metrics_workspace_bytes(100_000, C.byref(nb)) == 0 and nb.value > small
    assert lib.recnn_rank_metrics_workspace_bytes(0, C.byref(nb)) == 0 and nb.value == 0
    assert lib.recnn_rank_metrics(None, None, 0, ks(1, 1000), 2, a, a, None, None) == 0      # cutoffs are not limited to 64


@pytest.mark.parametrize("ks", [(), tuple(range(1, 10)), (5, 5), (10, 5), (0, 5), (-1,), (1.5, 3)])
def test_ranking_meter_refuses_bad_cutoffs(ks):
    from recnn_amd.retrieval import RankingMeter
    with pytest.raises(ValueError):
        RankingMeter(ks=ks)


def test_ranking_eval_fails_loudly_without_a_gpu():
    from recnn_amd import _lib as L
    from recnn_amd import retrieval as RT
    assert {"target_ranks", "RankingMeter"} <= set(RT.__all__) and hasattr(RT.FlatIndex, "rank_of")
    with pytest.raises(L.RecnnHipError):
        RT.RankingMeter(ks=(1, 10), device="cpu")
    t, tg = torch.zeros(4, 128), torch.zeros(4, dtype=torch.int64)
    for metric in ("L2", "IP", "COS", "cityblock", "cosine"):
        with pytest.raises(L.RecnnHipError):                 # the table must live on the GPU, as for search / cdist
            RT.target_ranks(t, t, tg, metric)
    with pytest.raises(ValueError):
        RT.target_ranks(t, t, tg, "hamming")
    if torch.cuda.is_available():
        return
    with pytest.raises(L.RecnnHipError):
        RT.RankingMeter(ks=(1, 10))
