"""CPU: the import surface of recnn.data.db_con (the reference's MilvusConnection over FlatIndex), its argument checks, the
no-GPU failure, and the host-side argument checks of the top-K statistics entry points (csrc/divstats.hip)."""
import ctypes as C
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env_like(n=37, width=128):
    return SimpleNamespace(base=SimpleNamespace(embeddings=torch.randn(n, width, generator=torch.Generator().manual_seed(0))))


def test_one_module_under_both_names_and_a_cheap_import():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import recnn.data.db_con\n"
            "import recnn_amd.data.db_con\n"
            "from recnn.data.db_con import MilvusConnection, MetricType, SearchResult\n"
            "assert recnn.data.db_con is recnn_amd.data.db_con and recnn.data.db_con is sys.modules['recnn.data.db_con']\n"
            "assert MetricType.L2.name == 'L2' and MetricType.IP.name == 'IP' and MetricType.L2 is not MetricType.IP\n"
            "assert 'milvus' not in sys.modules and 'oracle' not in sys.modules\n"
            "from recnn_amd import _lib\n"
            "assert _lib._lib is None, 'importing db_con loaded the HIP library'\n"
            "print('ok')\n") % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
    src = open(os.path.join(ROOT, "recnn_amd", "data", "db_con.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(milvus|pymilvus|oracle)\b", src, flags=re.M)
    assert not os.path.exists(os.path.join(ROOT, "milvus")) and not os.path.exists(os.path.join(ROOT, "milvus.py"))


def _construct(param):
    """The connection, or None where no GPU is visible (then the failure must be the package's own error, after the checks)."""
    from recnn_amd import _lib as L
    from recnn.data.db_con import MilvusConnection
    try:
        return MilvusConnection(_env_like(), name="movies_IP", param=param)
    except L.RecnnHipError:
        assert not torch.cuda.is_available()
        return None


def test_metric_type_spellings_and_argument_checks():
    from recnn.data.db_con import MetricType, MilvusConnection, metric_type_name
    foreign = SimpleNamespace(name="IP", value=2)                      # what pymilvus' MetricType.IP looks like
    for spelling in (foreign, "IP", MetricType.IP):
        assert metric_type_name(spelling) == "IP"
        con = _construct({"metric_type": spelling, "dimension": 128, "index_file_size": 1024})
        assert con is None or (con.metric == "IP" and con.name == "movies_IP")
    assert metric_type_name(MetricType.L2) == "L2" and metric_type_name("L2") == "L2"
    # refused before anything touches the GPU: a ValueError with or without one
    for bad in ("HAMMING", SimpleNamespace(name="JACCARD"), 7, None):
        with pytest.raises(ValueError, match="metric_type"):
            MilvusConnection(_env_like(), param={"metric_type": bad})
    with pytest.raises(ValueError, match="dimension"):
        MilvusConnection(_env_like(), param={"dimension": 64})
    with pytest.raises(ValueError, match="dimension"):
        MilvusConnection(_env_like(width=64), "movies_L2", "19530", {"metric_type": MetricType.L2, "dimension": 128})


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_gpu_means_the_packages_error_not_numpy():
    from recnn_amd import _lib as L
    from recnn.data.db_con import MetricType, MilvusConnection
    with pytest.raises(L.RecnnHipError):
        MilvusConnection(_env_like())
    with pytest.raises(L.RecnnHipError):
        MilvusConnection(_env_like(), name="movies_IP", param={"metric_type": MetricType.IP})
    from recnn_amd.retrieval import DiversityMeter, topk_stats
    with pytest.raises(L.RecnnHipError):
        topk_stats(torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int64), 5)
    with pytest.raises(L.RecnnHipError):
        DiversityMeter(5)


def test_new_names_are_exported():
    from recnn_amd import _lib as L
    from recnn_amd import retrieval
    lib = L.load()
    for name in ("recnn_topk_stats_workspace_bytes", "recnn_topk_stats"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "recnn_hip.h")).read()
    assert "recnn_topk_stats(" in hdr and "recnn_topk_stats_workspace_bytes(" in hdr
    assert "topk_stats" in retrieval.__all__ and "DiversityMeter" in retrieval.__all__


def test_stats_argument_checks_are_host_only():
    """Error codes and an error string, before any GPU call: this runs with no GPU present."""
    from recnn_amd import _lib as L
    lib = L.load()
    n = C.c_int64(-1)
    assert lib.recnn_topk_stats_workspace_bytes(65536, 20, C.byref(n)) == 0 and n.value > 0
    big = n.value
    assert lib.recnn_topk_stats_workspace_bytes(50, 20, C.byref(n)) == 0 and 0 < n.value < big
    assert lib.recnn_topk_stats_workspace_bytes(0, 1, C.byref(n)) == 0 and n.value == 0
    for bad in ((10, 0), (10, 65), (-1, 5)):
        assert lib.recnn_topk_stats_workspace_bytes(bad[0], bad[1], C.byref(n)) != 0
        assert b"topk_stats_workspace_bytes" in lib.recnn_last_error()
    assert lib.recnn_topk_stats_workspace_bytes(10, 5, None) != 0

    B, k, N = 4, 3, 9                                                   # host buffers: never dereferenced by a failing call
    dist, ids = np.zeros((B, 64), np.float32), np.zeros((B, 64), np.int64)
    counts, rm, rs, tot, ws = np.zeros(N, np.int32), np.zeros(B), np.zeros(B), np.zeros(4), np.zeros(8)

    def call(dist_p, k_, n_items, n_queries=B):
        p = [C.c_void_p(a.ctypes.data) for a in (ids, counts, rm, rs, tot, ws)]
        return lib.recnn_topk_stats(dist_p, p[0], n_queries, k_, n_items, 0, p[1], p[2], p[3], p[4], p[5], None)

    d = C.c_void_p(dist.ctypes.data)
    for args, word in (((d, 0, N), b"k <= 64"), ((d, 65, N), b"k <= 64"), ((d, k, 0), b"n_items"), ((None, k, N), b"null"),
                       ((d, k, N, -1), b"n_queries")):
        assert call(*args) != 0
        msg = lib.recnn_last_error()
        assert b"topk_stats" in msg and word in msg, msg
    assert not counts.any() and not tot.any()
