"""CPU checks of the IVF-Flat index: the numpy reference of tests/ivf_reference.py against itself where two
routes must agree, the host-only workspace queries of csrc/ivf.hip, and the refusals that need no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import ivf_reference as R


@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_restricted_search_with_every_list_probed_is_the_brute_force_search(metric):
    rng = np.random.default_rng(1)
    N, D, nlist, B = 200, 16, 9, 11
    table = rng.standard_normal((N, D))
    table[50:60] = table[10:20]                                          # ties, decided by id
    queries = rng.standard_normal((B, D))
    centroids = table[rng.permutation(N)[:nlist]]
    assignment = R.assign(table, centroids)
    assignment[assignment == 4] = 5                                      # an empty list
    for k in (1, 10, 64):
        want = R.search(queries, table, k, metric)
        for nprobe in (nlist, 64):
            got = R.ivf_search(queries, table, centroids, assignment, k, nprobe, metric)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    # and a restricted search reports only items of the probed lists, fewer than k where they run out
    lists = R.probe(queries, centroids, 2, metric)
    dist, ids = R.ivf_search(queries, table, centroids, assignment, 64, 2, metric)
    for b in range(B):
        reach = np.nonzero(np.isin(assignment, lists[b]))[0]
        n = min(64, len(reach))
        assert set(ids[b, :n].tolist()) <= set(reach.tolist()) and (ids[b, n:] == -1).all()
        assert np.isinf(dist[b, n:]).all()


def test_lists_are_the_stable_sort():
    a = np.array([2, 0, 2, 1, 0, 2, 4])
    start, ids = R.build_lists(a, 5)
    assert start.tolist() == [0, 2, 3, 6, 6, 7] and ids.tolist() == [1, 4, 3, 0, 2, 5, 6]


def test_one_iteration_on_integer_data_gives_the_same_means_in_either_summation_order():
    rng = np.random.default_rng(2)
    N, D, nlist = 300, 128, 12
    table = rng.integers(-8, 9, size=(N, D))
    centroids = table[rng.permutation(N)[:nlist]].copy()
    centroids[9] = centroids[2]                                          # the tie goes to list 2; list 9 stays empty
    a_up, m_up = R.kmeans_iteration(table, centroids)
    a_down, m_down = R.kmeans_iteration(table, centroids, descending=True)
    assert np.array_equal(a_up, a_down) and np.array_equal(m_up, m_down)
    assert not (a_up == 9).any() and np.array_equal(m_up[9], centroids[9])
    counts = np.bincount(a_up, minlength=nlist)
    for c in np.nonzero(counts)[0]:                                      # exact: an integer sum divided once
        assert np.array_equal(m_up[c], table[a_up == c].sum(0) / counts[c])
    assert R.sq_dists(table, centroids).dtype == np.int64


def test_workspace_queries_are_host_arithmetic_and_refuse_bad_sizes():
    from recnn_amd import _lib as L
    lib = L.load()

    def lists(n, nlist):
        out = C.c_int64(-1)
        return lib.recnn_ivf_lists_workspace_bytes(n, nlist, C.byref(out)), out.value

    def search(B, nprobe, nlist, k):
        out = C.c_int64(-1)
        return lib.recnn_ivf_search_workspace_bytes(B, nprobe, nlist, k, C.byref(out)), out.value

    rc, small = lists(1000, 20)
    assert rc == 0 and small >= 2 * 4 * 1000
    assert lists(100000, 20)[1] > small and lists(1000, 1000)[1] > small
    for n, nlist in ((0, 1), (10, 0), (10, 11), (-5, 1)):
        assert lists(n, nlist)[0] != 0 and b"1 <= nlist <= n_items" in lib.recnn_last_error()
    rc, base = search(25, 4, 100, 10)
    assert rc == 0 and base >= 25 * 4 * 10 * 8
    assert search(2048, 4, 100, 10)[1] > base and search(25, 16, 100, 10)[1] > base and search(25, 4, 100, 64)[1] > base
    assert search(0, 4, 100, 10)[0] == 0
    for nprobe, nlist in ((0, 100), (65, 100), (8, 7)):
        assert search(25, nprobe, nlist, 10)[0] != 0 and b"nprobe" in lib.recnn_last_error()
    for k in (0, 65):
        assert search(25, 4, 100, k)[0] != 0 and b"1 <= k <= 64" in lib.recnn_last_error()
    assert search(-1, 4, 100, 10)[0] != 0 and b"n_queries" in lib.recnn_last_error()
    assert search(1 << 20, 64, 100, 10)[0] != 0 and b"n_queries * nprobe" in lib.recnn_last_error()
    assert lib.recnn_ivf_search_workspace_bytes(25, 4, 100, 10, None) != 0 and b"null pointer" in lib.recnn_last_error()
    # the scan refuses before any HIP call, and zero queries launch nothing
    buf = (C.c_float * 1024)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    scan = lambda B=2, ld=128, nlist=4, n=10, metric=1, nprobe=2, k=5, aux=p: lib.recnn_ivf_scan(
        p, ld, B, p, aux, p, p, nlist, n, metric, p, nprobe, k, p, p, p, None, None, 0)
    assert scan(nprobe=5) != 0 and b"nprobe" in lib.recnn_last_error()
    assert scan(k=65) != 0 and b"1 <= k <= 64" in lib.recnn_last_error()
    assert scan(metric=2) != 0 and b"metric" in lib.recnn_last_error()
    assert scan(aux=None) != 0 and b"metric" in lib.recnn_last_error()
    assert scan(ld=64) != 0 and b"ld_q" in lib.recnn_last_error()
    assert scan(nlist=11) != 0 and b"nlist" in lib.recnn_last_error()
    assert lib.recnn_ivf_scan(None, 128, 0, p, p, p, p, 4, 10, 1, None, 2, 5, None, None, None, None, None, 0) == 0


def _shell(cls, **attrs):
    """An index object without its constructor (which wants the GPU): the attributes `search` checks before anything else."""
    o = object.__new__(cls)
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def test_refusals_fire_without_a_gpu():
    from recnn_amd import _lib as L
    from recnn_amd import retrieval as RT
    table = torch.zeros(100, 128)
    for metric in ("COS", "cosine", "euclidean", None):
        with pytest.raises(ValueError, match="metric must be \"L2\" or \"IP\""):
            RT.IVFFlatIndex(table, 10, metric)
    for nlist in (101, 0, -3):
        with pytest.raises(ValueError, match="nlist must be an integer from 1 to 100"):
            RT.IVFFlatIndex(table, nlist)
    with pytest.raises(TypeError, match="nlist must be an integer"):
        RT.IVFFlatIndex(table, 2.5)
    with pytest.raises(ValueError, match=r"table must be \[N, 128\]"):
        RT.IVFFlatIndex(torch.zeros(100, 64), 10)
    with pytest.raises(ValueError, match=r"table must be \[N, 128\]"):
        RT.IVFFlatIndex(torch.zeros(128), 1)
    with pytest.raises(TypeError, match="table must be a float32 tensor"):
        RT.IVFFlatIndex(np.zeros((100, 128), dtype=np.float32), 10)
    with pytest.raises(ValueError, match="niter"):
        RT.IVFFlatIndex(table, 10, niter=-1)
    with pytest.raises(ValueError, match=r"centroids must be a float32 tensor \[10, 128\]"):
        RT.IVFFlatIndex(table, 10, centroids=torch.zeros(9, 128))
    with pytest.raises(ValueError, match="centroids must be a float32 tensor"):
        RT.IVFFlatIndex(table, 10, centroids=torch.zeros(10, 128, dtype=torch.float64))
    with pytest.raises(ValueError, match="assignment must be a 1-D integer tensor of 100 entries"):
        RT.IVFFlatIndex.from_assignment(table, torch.zeros(10, 128), torch.zeros(99, dtype=torch.int64))
    with pytest.raises(ValueError, match="assignment must be a 1-D integer tensor"):
        RT.IVFFlatIndex.from_assignment(table, torch.zeros(10, 128), torch.zeros(100))
    # no CPU fallback: a CPU table raises as FlatIndex does
    with pytest.raises(L.RecnnHipError, match="must live on the GPU"):
        RT.IVFFlatIndex(table, 10)
    with pytest.raises(L.RecnnHipError, match="must live on the GPU"):
        RT.IVFFlatIndex.from_assignment(table, torch.zeros(10, 128), torch.zeros(100, dtype=torch.int64))
    # search and probe check k and nprobe before they touch the index
    index = _shell(RT.IVFFlatIndex, n_items=100, nlist=10, dim=128)
    q = torch.zeros(3, 128)
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match="k must be an integer from 1 to 64"):
            index.search(q, k)
    for nprobe in (0, 65):
        with pytest.raises(ValueError, match="nprobe must be an integer from 1 to 64"):
            index.search(q, 10, nprobe)
        with pytest.raises(ValueError, match="nprobe must be an integer from 1 to 64"):
            index.probe(q, nprobe)
    with pytest.raises(TypeError, match="nprobe must be an integer"):
        index.search(q, 10, "16")
    with pytest.raises(ValueError, match="holds only 30 items"):
        _shell(RT.IVFFlatIndex, n_items=30, nlist=10).search(q, 31)
    assert index.ntotal == 100 and RT.DEFAULT_NPROBE == 16
    # the two-stage index takes it as a first stage and refuses rank_of by name
    critic = _shell(RT.CriticIndex, n_items=100, table=table)
    two = RT.TwoStageIndex(_shell(RT.IVFFlatIndex, n_items=100, nlist=10, table=table), critic, 32)
    with pytest.raises(ValueError, match="rank_of: refused with an IVFFlatIndex first stage.*head of the flat index's order"):
        two.rank_of(q, q, torch.zeros(3, dtype=torch.int64))
    flat_two = RT.TwoStageIndex(_shell(RT.FlatIndex, n_items=100, table=table), critic, 32)
    with pytest.raises(ValueError, match="nprobe applies to an IVFFlatIndex first stage"):
        flat_two.search(q, q, 5, nprobe=4)
    import recnn_amd
    with pytest.raises(ValueError, match="index=\"ivf\" needs nlist"):
        recnn_amd.nn.WolpertingerPolicy(None, None, table, index="ivf")
    with pytest.raises(ValueError, match="nlist and nprobe apply to index=\"ivf\""):
        recnn_amd.nn.WolpertingerPolicy(None, None, table, nprobe=4)


def test_db_con_refuses_an_unknown_index_type_without_a_gpu():
    import types
    from recnn_amd.data import db_con
    env = types.SimpleNamespace(base=types.SimpleNamespace(embeddings=torch.zeros(10, 128)))
    with pytest.raises(ValueError, match="index_type"):
        db_con.MilvusConnection(env, param={"index_type": "HNSW"})
    with pytest.raises(ValueError, match="needs param\\['nlist'\\]"):
        db_con.MilvusConnection(env, param={"index_type": "IVF_FLAT"})
