"""The reference's `recnn/data/db_con.py` (`MilvusConnection`, `SearchResult`) without a server: a "collection" is a
`recnn_amd.retrieval.FlatIndex` over `env.base.embeddings`, searched exactly on the GPU (csrc/topk.hip), or, when `param` asks for
`index_type="IVF_FLAT"`, a `recnn_amd.retrieval.IVFFlatIndex` (csrc/ivf.hip) whose search honours `nprobe`.

The evaluation notebooks (`examples/[Results]/2. Diversity Test (Indexes).ipynb`, `3. Distances Test.ipynb`) and the demo's
"Test Diversity" page run against it as written, except that without pymilvus installed their import line becomes
`from recnn.data.db_con import MilvusConnection, MetricType`.  Nothing here imports `milvus`, opens a
socket, loads the HIP library or touches the GPU at import time.

Conventions:
* `MetricType.L2` reports SQUARED distances, ascending; `MetricType.IP` inner products, descending.  That is what
  `FlatIndex("L2")` / `FlatIndex("IP")` and faiss report, and what the demo assumes when it takes `D ** 0.5`
  ("l2 -> euclidean").  Whether a Milvus server reports the squared value as well has not been checked (pymilvus and a server
  were not available when this was written).
* Without `index_type` the search is exact: `nprobe` and every other search parameter is accepted and ignored.  Ties go to the
  smaller id.  With `param={"index_type": "IVF_FLAT", "nlist": n}` the collection is an inverted-file index of n k-means lists and
  a search scores the `search_param["nprobe"]` nearest lists (default 16, what the reference passes); other keys are still ignored.
* Ids are rows of `env.base.embeddings` (the reference inserts the rows with `ids=range(N)`).
* `topk` <= 64 and an embedding width of 128 are the limits of csrc/topk.hip and are reported with its errors.
* No CPU fallback: without a GPU the constructor raises `recnn_amd._lib.RecnnHipError`.
"""
import enum

import numpy as np
import torch

from .. import _lib as L
from ..retrieval import DEFAULT_NPROBE, FlatIndex, IVFFlatIndex


class MetricType(enum.Enum):
    """The two metric types the reference's notebooks use (pymilvus' names and values)."""
    L2 = 1
    IP = 2


def metric_type_name(metric_type):
    """"L2" / "IP" from a `MetricType`, the string itself, or any object whose `.name` is one of them (pymilvus' enum)."""
    name = metric_type if isinstance(metric_type, str) else getattr(metric_type, "name", None)
    if name not in MetricType.__members__:
        raise ValueError(f"metric_type must be MetricType.L2 or MetricType.IP (or their names), got {metric_type!r}")
    return name


class Status:
    """What the client calls return first: `.OK()` is True (a failure raises instead)."""

    def __init__(self, message="OK"):
        self.code, self.message = 0, message

    def OK(self):
        return True

    def __repr__(self):
        return f"Status(code={self.code}, message={self.message!r})"


class SearchResult:
    """Ids int64 [B, k] and distances float32 [B, k] of one search, best first, kept where the search left them."""

    def __init__(self, dist, ids):
        self._dist, self._ids = dist, ids
        self._id_array = self._distance_array = None

    def id(self, device):
        return self._ids.to(device)

    def dist(self, device):
        return self._dist.to(device)

    @property
    def id_array(self):
        """Nested lists [B][k], as the Milvus client's result has them (built on first access)."""
        if self._id_array is None:
            self._id_array = self._ids.tolist()
        return self._id_array

    @property
    def distance_array(self):
        if self._distance_array is None:
            self._distance_array = self._dist.tolist()
        return self._distance_array

    @property
    def shape(self):
        return tuple(self._ids.shape)

    def __len__(self):
        return self._ids.shape[0]


class _Client:
    """The part of the Milvus client the notebooks call directly (`get_err_l2_dist` / `get_err_ip_dist`)."""

    def __init__(self, connection):
        self._con = connection

    def has_collection(self, collection_name):
        return Status(), collection_name == self._con.name

    def search(self, collection_name, query_records, top_k, params=None, **_ignored):
        if collection_name != self._con.name:
            raise ValueError(f"collection {collection_name!r} is not this connection's ({self._con.name!r})")
        return Status(), self._con._search(query_records, top_k, params)


class MilvusConnection:
    """`MilvusConnection(env, name, port, param)` of the reference: `param` may carry `metric_type` (default L2) and `dimension`
    (must equal the table's width), and `index_type="IVF_FLAT"` with `nlist` (an `IVFFlatIndex` instead of the `FlatIndex`);
    `port`, `index_file_size` and other keys are accepted and ignored."""

    def __init__(self, env, name="movies_L2", port="19530", param=None):
        param = {"collection_name": name, "metric_type": MetricType.L2, **(param or {})}
        self.metric = metric_type_name(param["metric_type"])
        table = env.base.embeddings
        if not torch.is_tensor(table) or table.dim() != 2:
            raise ValueError("env.base.embeddings must be a [n_items, width] tensor")
        if param.get("dimension") is not None and int(param["dimension"]) != table.shape[1]:
            raise ValueError(f"param['dimension'] = {param['dimension']} but env.base.embeddings is {table.shape[1]} wide")
        index_type = param.get("index_type")
        index_type = getattr(index_type, "name", index_type)           # pymilvus' IndexType enum, or the name
        if index_type not in (None, "FLAT", "IVF_FLAT", "IVFLAT"):
            raise ValueError(f"param['index_type'] must be \"FLAT\" or \"IVF_FLAT\" (or absent), got {param['index_type']!r}")
        self.ivf = index_type in ("IVF_FLAT", "IVFLAT")
        if self.ivf and "nlist" not in param:
            raise ValueError("param['index_type'] = \"IVF_FLAT\" needs param['nlist']")
        self.name = name
        self.statuses = {}
        if not table.is_cuda:
            if not torch.cuda.is_available():
                raise L.RecnnHipError("MilvusConnection searches on the GPU and none is visible (no CPU fallback)")
            table = table.detach().to("cuda")           # once; env.base.embeddings itself stays where it is
        self.index = IVFFlatIndex(table, param["nlist"], self.metric) if self.ivf else FlatIndex(table, self.metric)
        self.client = _Client(self)
        self.statuses["created_collection"] = Status(f"{name}: {self.index.ntotal} x {self.index.dim}, {self.metric}")

    def _search(self, search_vecs, topk, search_param=None):
        if isinstance(search_vecs, (list, tuple)) and len(search_vecs) and torch.is_tensor(search_vecs[0]):
            search_vecs = torch.stack(list(search_vecs))
        if not torch.is_tensor(search_vecs):
            search_vecs = torch.from_numpy(np.asarray(search_vecs, dtype=np.float32))
        q = search_vecs.detach()
        if q.dim() == 1:
            q = q[None]
        if q.dim() != 2 or q.shape[1] != self.index.dim:
            raise ValueError(f"search vectors must be [B, {self.index.dim}] or [{self.index.dim}], got {tuple(search_vecs.shape)}")
        if self.ivf:
            dist, ids = self.index.search(q, int(topk), (search_param or {}).get("nprobe", DEFAULT_NPROBE))
        else:
            dist, ids = self.index.search(q, int(topk))
        return SearchResult(dist, ids)

    def search(self, search_vecs, topk=10, search_param=None):
        result = self._search(search_vecs, topk, search_param)
        self.statuses["last_search"] = Status()
        return result

    def get_log(self):
        return self.statuses


__all__ = ["MetricType", "MilvusConnection", "SearchResult", "Status", "metric_type_name"]
