"""Exact batched nearest-item search on the GPU: the retrieval step that turns generated actions into item ids.

`FlatIndex(table, metric)` mirrors how the reference's demo uses faiss (`examples/streamlit_demo.py:190-204`:
IndexFlatL2 / IndexFlatIP / IndexFlatIP over L2-normalised rows) and `MilvusConnection.search`
(`recnn/data/db_con.py:45-56`): `search(queries, k)` returns `(distances[B, k], ids[B, k])`, best first.
SURVEY.md 8 row f2 ("next"); kernel in csrc/topk.hip.

It also takes the metrics of the reference's per-item scipy ranking loop (`examples/streamlit_demo.py:207-231`, `rank`;
`examples/[Results]/1. Ranking.ipynb`): the names of `scipy.spatial.distance.cdist` in `DIST_METRICS`, or the scipy
functions themselves (`distance.canberra`).  `cdist(queries, table, metric)` gives the whole distance matrix.  Kernel in
csrc/rank.hip; DESIGN.md section 11.
"""
import ctypes as C

import torch

from . import _lib as L

METRICS = {"IP": 0, "L2": 1, "COS": 2}
# scipy.spatial.distance.cdist names -> include/recnn_hip.h RECNN_DIST_*
DIST_METRICS = {"sqeuclidean": 0, "euclidean": 1, "cityblock": 2, "chebyshev": 3, "minkowski": 4, "canberra": 5,
                "braycurtis": 6, "cosine": 7, "correlation": 8}


def metric_name(metric):
    """A metric name as given, or the `__name__` of a scipy distance function (`distance.canberra` -> "canberra")."""
    name = metric if isinstance(metric, str) else getattr(metric, "__name__", None)
    if name not in METRICS and name not in DIST_METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS) + sorted(DIST_METRICS)} or a scipy distance function, "
                         f"got {metric!r}")
    return name


def minkowski_p(name, p):
    """The exponent passed to the kernel: scipy's default p = 2 for minkowski; p is an error for the other metrics."""
    if name != "minkowski":
        if p is not None:
            raise ValueError(f"p applies to minkowski only, not {name}")
        return 0.0
    p = 2.0 if p is None else float(p)
    if not p >= 1.0:
        raise ValueError(f"minkowski needs p >= 1 (got {p})")
    return p


def _on_gpu(t, what):
    if not t.is_cuda:
        raise L.RecnnHipError(f"{what} must live on the GPU (no CPU fallback)")


def _queries(queries, device):
    q = queries.detach().to(device, torch.float32)
    if q.dim() == 1:
        q = q[None]
    if q.stride(-1) != 1 or q.stride(0) % 4 or q.stride(0) < q.shape[1] or q.data_ptr() % 16:
        q = q.contiguous()
    return q


def _item_aux(table, name):
    n, dim = table.shape
    nf = C.c_int64()
    L.call("recnn_dist_item_aux_floats", n, dim, DIST_METRICS[name], C.byref(nf))
    if nf.value == 0:
        return None
    aux = torch.empty(nf.value, dtype=torch.float32, device=table.device)
    L.call("recnn_dist_item_aux", L.ptr(table), n, dim, DIST_METRICS[name], L.ptr(aux), L.current_stream())
    return aux


def _workspace(B, n, name, k, device):
    nbytes = C.c_int64()
    L.call("recnn_dist_workspace_bytes", B, n, DIST_METRICS[name], k, C.byref(nbytes))
    return torch.empty(max(int(nbytes.value), 16), dtype=torch.uint8, device=device)


class FlatIndex:
    """Exact search over the rows of `table` (float32 [N, 128] on the GPU).

    metric "IP" / "L2" / "COS" are faiss's indexes: IP and COS (q.t / |t|) report scores descending, L2 squared distances
    ascending.  Any name of `DIST_METRICS` (or the scipy function of that name; `p` is minkowski's exponent, default 2)
    reports scipy's distances ascending, as the reference's `rank` does; NaN distances (cosine against a zero row,
    correlation against a constant row, braycurtis of two zero rows) come last, ties go to the smaller id.

    Ids are table row ids.  For the reference's environments, whose item embeddings are indexed by
    `env.base.key_to_id` (row 0 is the padding item), `env.base.id_to_key[i]` turns row id i into the item key; to leave
    the padding item out, as the notebooks do, index `table[1:]` and add 1 to the ids, or ask for k + 1 and drop id 0.
    """

    def __init__(self, table: torch.Tensor, metric="L2", p=None):
        self.metric = metric_name(metric)
        _on_gpu(table, "FlatIndex: the item table")
        self.p = minkowski_p(self.metric, p) if self.metric in DIST_METRICS else None
        if self.metric in METRICS and p is not None:
            raise ValueError("p applies to minkowski only")
        self.table = table.detach().to(torch.float32).contiguous()
        self.n_items, self.dim = self.table.shape
        self.aux = None
        if self.metric in DIST_METRICS:
            self.aux = _item_aux(self.table, self.metric)
        elif self.metric != "IP":
            self.aux = torch.empty(self.n_items, dtype=torch.float32, device=table.device)
            L.call("recnn_topk_item_aux", L.ptr(self.table), self.n_items, self.dim, METRICS[self.metric], L.ptr(self.aux),
                   L.current_stream())

    @property
    def ntotal(self):
        return self.n_items

    def search(self, queries: torch.Tensor, k: int = 10):
        """(distances float32[B, k], ids int64[B, k]); L2 -> squared distances ascending, IP / COS -> scores descending,
        scipy metrics -> distances ascending."""
        if self.metric in DIST_METRICS:
            _on_gpu(queries, "FlatIndex.search: the queries")
        q = _queries(queries, self.table.device)
        B = q.shape[0]
        dist = torch.empty(B, k, dtype=torch.float32, device=q.device)
        ids = torch.empty(B, k, dtype=torch.int64, device=q.device)
        if self.metric in DIST_METRICS:
            ws = _workspace(B, self.n_items, self.metric, k, q.device)
            L.call("recnn_dist_topk", L.ptr(q), q.stride(0), B, L.ptr(self.table), self.n_items, self.dim,
                   DIST_METRICS[self.metric], self.p, L.ptr(self.aux), k, L.ptr(dist), L.ptr(ids), L.ptr(ws), L.current_stream())
            return dist, ids
        nbytes = C.c_int64()
        L.call("recnn_topk_workspace_bytes", B, k, C.byref(nbytes))
        ws = torch.empty(max(int(nbytes.value), 16), dtype=torch.uint8, device=q.device)
        L.call("recnn_topk_search", L.ptr(q), q.stride(0), B, L.ptr(self.table), self.n_items, self.dim, METRICS[self.metric],
               L.ptr(self.aux), k, L.ptr(dist), L.ptr(ids), L.ptr(ws), L.current_stream())
        return dist, ids


def cdist(queries: torch.Tensor, table: torch.Tensor, metric="euclidean", p=None):
    """float32 [B, N] matrix of scipy's `cdist(queries, table, metric)` on the GPU (table: [N, 128]; metric: a name of
    `DIST_METRICS` or the scipy function).  Each entry is bit-identical to what `FlatIndex(table, metric).search` reports
    for that pair."""
    name = metric_name(metric)
    if name not in DIST_METRICS:
        raise ValueError(f"cdist takes the scipy metrics {sorted(DIST_METRICS)}, not {name}")
    pp = minkowski_p(name, p)
    _on_gpu(table, "cdist: the item table")
    _on_gpu(queries, "cdist: the queries")
    t = table.detach().to(torch.float32).contiguous()
    q = _queries(queries, t.device)
    B, (N, dim) = q.shape[0], t.shape
    aux = _item_aux(t, name)
    out = torch.empty(B, N, dtype=torch.float32, device=t.device)
    ws = _workspace(B, N, name, 0, t.device)
    L.call("recnn_dist_matrix", L.ptr(q), q.stride(0), B, L.ptr(t), N, dim, DIST_METRICS[name], pp, L.ptr(aux), L.ptr(out), N,
           L.ptr(ws), L.current_stream())
    return out


__all__ = ["FlatIndex", "cdist", "METRICS", "DIST_METRICS", "metric_name", "minkowski_p"]
