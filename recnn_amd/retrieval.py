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

    def search(self, queries: torch.Tensor, k: int = 10, exclude=None):
        """(distances float32[B, k], ids int64[B, k]); L2 -> squared distances ascending, IP / COS -> scores descending,
        scipy metrics -> distances ascending.

        `exclude` (a `SeenItems` or `SeenMask` of B rows): the items excluded in a row do not exist for it.  A row with fewer
        than k items left ends in id -1 with distance +inf (L2, scipy metrics) or -inf (IP, COS), faiss's convention."""
        if self.metric in DIST_METRICS:
            _on_gpu(queries, "FlatIndex.search: the queries")
        q = _queries(queries, self.table.device)
        B = q.shape[0]
        dist = torch.empty(B, k, dtype=torch.float32, device=q.device)
        ids = torch.empty(B, k, dtype=torch.int64, device=q.device)
        if exclude is not None:
            m = self._exclusion(exclude, B, "FlatIndex.search")
            if B == 0:
                return dist, ids
            if self.metric in DIST_METRICS:
                ws = L.workspace("recnn_dist_workspace_bytes", B, self.n_items, DIST_METRICS[self.metric], k, device=q.device)
                L.call("recnn_dist_topk_excluding", L.ptr(q), q.stride(0), B, L.ptr(self.table), self.n_items, self.dim,
                       DIST_METRICS[self.metric], self.p, L.ptr(self.aux), k, L.ptr(dist), L.ptr(ids), L.ptr(ws),
                       L.current_stream(), L.ptr(m.words), m.words.shape[1])
            else:
                ws = L.workspace("recnn_topk_workspace_bytes", B, k, device=q.device)
                L.call("recnn_topk_search_excluding", L.ptr(q), q.stride(0), B, L.ptr(self.table), self.n_items, self.dim,
                       METRICS[self.metric], L.ptr(self.aux), k, L.ptr(dist), L.ptr(ids), L.ptr(ws), L.current_stream(),
                       L.ptr(m.words), m.words.shape[1])
            return dist, ids
        if self.metric in DIST_METRICS:
            ws = L.workspace("recnn_dist_workspace_bytes", B, self.n_items, DIST_METRICS[self.metric], k, device=q.device)
            L.call("recnn_dist_topk", L.ptr(q), q.stride(0), B, L.ptr(self.table), self.n_items, self.dim,
                   DIST_METRICS[self.metric], self.p, L.ptr(self.aux), k, L.ptr(dist), L.ptr(ids), L.ptr(ws), L.current_stream())
            return dist, ids
        ws = L.workspace("recnn_topk_workspace_bytes", B, k, device=q.device)
        L.call("recnn_topk_search", L.ptr(q), q.stride(0), B, L.ptr(self.table), self.n_items, self.dim, METRICS[self.metric],
               L.ptr(self.aux), k, L.ptr(dist), L.ptr(ids), L.ptr(ws), L.current_stream())
        return dist, ids

    def _exclusion(self, exclude, B, what):
        """The `SeenMask` of an `exclude` argument, checked against this index and a batch of B rows."""
        if not isinstance(exclude, (SeenItems, SeenMask)):
            raise TypeError(f"{what}: exclude must be a SeenItems or a SeenMask, got {type(exclude).__name__}")
        if exclude.rows != B:
            raise ValueError(f"{what}: {B} queries but an exclusion of {exclude.rows} rows")
        m = exclude.mask(self.n_items) if isinstance(exclude, SeenItems) else exclude
        if m.n_items != self.n_items:
            raise ValueError(f"{what}: the exclusion mask was built for n_items = {m.n_items}, the index holds {self.n_items}")
        if m.words.device != self.table.device:
            raise ValueError(f"{what}: the exclusion mask lives on {m.words.device}, the index on {self.table.device}")
        return m

    def rank_of(self, queries: torch.Tensor, targets: torch.Tensor, exclude=None):
        """int32 [B]: for each query row, how many items come before item `targets[b]` in the order `search` uses (0 = the
        target is the best item); -1 for a target id outside [0, n_items).  The whole table is counted: no limit of 64.

        `exclude` (a `SeenItems` or `SeenMask` of B rows): the items excluded in a row are not counted.  The target's own bit is
        not consulted: an excluded target is still ranked among the rest."""
        if self.metric in DIST_METRICS:
            _on_gpu(queries, "FlatIndex.rank_of: the queries")
        q = _queries(queries, self.table.device)
        B = q.shape[0]
        t = _targets(targets, B, q.device, "FlatIndex.rank_of")
        rank = torch.empty(B, dtype=torch.int32, device=q.device)
        if exclude is not None:
            m = self._exclusion(exclude, B, "FlatIndex.rank_of")
            if B == 0:
                return rank
            if self.metric in DIST_METRICS:
                ws = L.workspace("recnn_dist_target_rank_workspace_bytes", B, self.n_items, DIST_METRICS[self.metric],
                                 device=q.device)
                L.call("recnn_dist_target_rank_excluding", L.ptr(q), q.stride(0), B, L.ptr(self.table), self.n_items, self.dim,
                       DIST_METRICS[self.metric], self.p, L.ptr(self.aux), L.ptr(t), L.ptr(rank), L.ptr(ws), L.current_stream(),
                       L.ptr(m.words), m.words.shape[1])
            else:
                ws = L.workspace("recnn_topk_target_rank_workspace_bytes", B, self.n_items, device=q.device)
                L.call("recnn_topk_target_rank_excluding", L.ptr(q), q.stride(0), B, L.ptr(self.table), self.n_items, self.dim,
                       METRICS[self.metric], L.ptr(self.aux), L.ptr(t), L.ptr(rank), L.ptr(ws), L.current_stream(),
                       L.ptr(m.words), m.words.shape[1])
            return rank
        if B == 0:                                                       # an empty batch has no storage to point at
            return rank
        if self.metric in DIST_METRICS:
            ws = L.workspace("recnn_dist_target_rank_workspace_bytes", B, self.n_items, DIST_METRICS[self.metric], device=q.device)
            L.call("recnn_dist_target_rank", L.ptr(q), q.stride(0), B, L.ptr(self.table), self.n_items, self.dim,
                   DIST_METRICS[self.metric], self.p, L.ptr(self.aux), L.ptr(t), L.ptr(rank), L.ptr(ws), L.current_stream())
            return rank
        ws = L.workspace("recnn_topk_target_rank_workspace_bytes", B, self.n_items, device=q.device)
        L.call("recnn_topk_target_rank", L.ptr(q), q.stride(0), B, L.ptr(self.table), self.n_items, self.dim, METRICS[self.metric],
               L.ptr(self.aux), L.ptr(t), L.ptr(rank), L.ptr(ws), L.current_stream())
        return rank


def _targets(targets, B, device, what):
    t = torch.as_tensor(targets)
    if t.dtype.is_floating_point or t.dtype == torch.bool or t.dim() != 1:
        raise ValueError(f"{what}: targets must be a 1-D integer tensor, got {t.dtype} {tuple(t.shape)}")
    if t.shape[0] != B:
        raise ValueError(f"{what}: {B} queries but {t.shape[0]} targets")
    return t.detach().to(device, torch.int64).contiguous()


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
    ws = L.workspace("recnn_dist_workspace_bytes", B, N, DIST_METRICS[name], 0, device=t.device)
    L.call("recnn_dist_matrix", L.ptr(q), q.stride(0), B, L.ptr(t), N, dim, DIST_METRICS[name], pp, L.ptr(aux), L.ptr(out), N,
           L.ptr(ws), L.current_stream())
    return out


__all__ = ["FlatIndex", "cdist", "METRICS", "DIST_METRICS", "metric_name", "minkowski_p"]


# ---- statistics of a search result (csrc/divstats.hip): what the reference's diversity and distances
# notebooks compute on the host from `[B, k]` ids and distances, kept on the GPU and accumulated over the test loader's batches.

class TopkStats:
    """Device tensors of one `topk_stats` call: `row_mean`, `row_std` (float64 [B]), `counts` (int32 [n_items]) and `totals`
    (float64 [4]: sum of row_mean, sum of row_std, rows seen, ids outside [0, n_items))."""
    __slots__ = ("row_mean", "row_std", "counts", "totals")

    def __init__(self, row_mean, row_std, counts, totals):
        self.row_mean, self.row_std, self.counts, self.totals = row_mean, row_std, counts, totals


def _dense16(t, dtype, what):
    _on_gpu(t, what)
    if t.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, got {t.dtype}")
    t = t.detach().contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def topk_stats(dist, ids, n_items, sqrt=False, counts=None, totals=None):
    """Per-row mean and population std (float64, `np.sqrt` of the distances first when `sqrt`) of `dist` float32 [B, k], and
    how often each item of [0, n_items) appears in `ids` int64 [B, k]: one pass over what `FlatIndex.search` or
    `SearchResult.dist / id` returned, on the GPU.  `counts` and `totals` are accumulated into when given (else fresh zeros);
    ids out of range are not counted but tallied in `totals[3]`."""
    dist, ids = _dense16(dist, torch.float32, "topk_stats: dist"), _dense16(ids, torch.int64, "topk_stats: ids")
    if dist.dim() != 2 or dist.shape != ids.shape:
        raise ValueError(f"topk_stats: dist and ids must both be [B, k], got {tuple(dist.shape)} and {tuple(ids.shape)}")
    B, k = dist.shape
    dev = dist.device
    if counts is None:
        counts = torch.zeros(n_items, dtype=torch.int32, device=dev)
    if totals is None:
        totals = torch.zeros(4, dtype=torch.float64, device=dev)
    for t, dtype, shape, what in ((counts, torch.int32, (n_items,), "counts"), (totals, torch.float64, (4,), "totals")):
        _on_gpu(t, f"topk_stats: {what}")
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"topk_stats: {what} must be a contiguous {dtype} tensor of shape {shape}")
    row_mean = torch.empty(B, dtype=torch.float64, device=dev)
    row_std = torch.empty(B, dtype=torch.float64, device=dev)
    ws = L.workspace("recnn_topk_stats_workspace_bytes", B, k, device=dev)     # (also refuses a k the kernel cannot take)
    if B == 0:                                                       # an empty batch has no storage to point at
        return TopkStats(row_mean, row_std, counts, totals)
    L.call("recnn_topk_stats", L.ptr(dist), L.ptr(ids), B, k, n_items, int(bool(sqrt)), L.ptr(counts), L.ptr(row_mean),
           L.ptr(row_std), L.ptr(totals), L.ptr(ws), L.current_stream())
    return TopkStats(row_mean, row_std, counts, totals)


class DiversityMeter:
    """Accumulates `topk_stats` over any number of `update(dist, ids)` calls (one per batch of the test loader).

    `mean` / `std` are the notebooks' `D.mean(axis=1).mean()` / `D.std(axis=1).mean()` over all rows seen, `recommended()`
    what `np.unique(ids, return_counts=True)` gives, `counts_of_counts()` what `pd.Series(counts).value_counts()` holds.
    Reading any of them synchronises once and raises ValueError if an id was outside [0, n_items).  That includes the id -1 a
    `search(..., exclude=...)` reports for a row with fewer than k items left: such a row has no k recommendations to take
    statistics of, and raising is the right answer for it."""

    def __init__(self, n_items, sqrt=False, device="cuda"):
        self.n_items, self.sqrt = int(n_items), bool(sqrt)
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise L.RecnnHipError("DiversityMeter: the accumulators live on the GPU (no CPU fallback)")
        self.counts = torch.zeros(self.n_items, dtype=torch.int32, device=device)
        self.totals = torch.zeros(4, dtype=torch.float64, device=device)

    def update(self, dist, ids):
        """Adds one batch; returns its `TopkStats` (the per-row tensors of this batch, the shared accumulators)."""
        return topk_stats(dist, ids, self.n_items, self.sqrt, self.counts, self.totals)

    def reset(self):
        self.counts.zero_()
        self.totals.zero_()

    def _totals(self):
        t = self.totals.tolist()
        if t[3] != 0:
            raise ValueError(f"DiversityMeter: {int(t[3])} ids were outside [0, {self.n_items}) and were not counted")
        return t

    @property
    def rows(self):
        return int(self._totals()[2])

    @property
    def mean(self):
        t = self._totals()
        return t[0] / t[2]

    @property
    def std(self):
        t = self._totals()
        return t[1] / t[2]

    def recommended(self):
        """(uniques, counts) as numpy int64 arrays: the ids with a non-zero count, ascending, and their counts."""
        self._totals()
        uniques = torch.nonzero(self.counts).flatten()
        return uniques.cpu().numpy(), self.counts[uniques].to(torch.int64).cpu().numpy()

    def counts_of_counts(self):
        """(n_recommended, how_many_items) as numpy int64 arrays, sorted by n_recommended, over the recommended items."""
        self._totals()
        n, how_many = torch.unique(self.counts[self.counts > 0], return_counts=True)
        return n.to(torch.int64).cpu().numpy(), how_many.cpu().numpy()


__all__ += ["topk_stats", "DiversityMeter"]


# ---- offline ranking evaluation (csrc/rank.hip, csrc/topk.hip, csrc/evalrank.hip): the rank of the item the
# user took next under the generated action, and hit rate / NDCG / MRR accumulated over the test loader's batches.

def target_ranks(queries, table, targets, metric="L2", p=None, exclude=None):
    """`FlatIndex(table, metric, p).rank_of(queries, targets, exclude)` in one call, as `cdist` is for the matrix."""
    index = FlatIndex(table, metric, p)
    return index.rank_of(queries, targets) if exclude is None else index.rank_of(queries, targets, exclude)


MAX_CUTOFFS = 8


class RankingMeter:
    """Accumulates the ranking metrics of `update(ranks)` calls (one per batch of the test loader), one relevant item per row.

    `ranks` is what `FlatIndex.rank_of` returns (int32 [B] on the GPU); `mask` (optional, [B]) keeps the rows where it is
    non-zero.  `hit_rate()[K]` is the share of rows with rank < K, `ndcg()[K]` the mean of 1 / log2(rank + 2) over rows with
    rank < K counted against all rows (IDCG = 1), `mrr` the mean of 1 / (rank + 1), `mean_rank` the mean rank.  Cutoffs: up to 8,
    ascending, of any size.  Reading synchronises once; it raises ValueError if a rank was negative (a target outside the table)
    and not masked out, or if no row was counted."""

    def __init__(self, ks=(1, 5, 10), device="cuda"):
        ks = tuple(ks)
        if not 1 <= len(ks) <= MAX_CUTOFFS:
            raise ValueError(f"RankingMeter: need 1 to {MAX_CUTOFFS} cutoffs, got {len(ks)}")
        if any(int(k) != k or k < 1 or k >= 2 ** 31 for k in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
            raise ValueError(f"RankingMeter: cutoffs must be integers >= 1 in strictly ascending order, got {ks}")
        self.ks = tuple(int(k) for k in ks)
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise L.RecnnHipError("RankingMeter: the accumulators live on the GPU (no CPU fallback)")
        self._ks = (C.c_int32 * len(self.ks))(*self.ks)
        self.sums = torch.zeros(len(self.ks) + 1, dtype=torch.float64, device=device)     # ndcg per cutoff, mrr
        self.counts = torch.zeros(len(self.ks) + 3, dtype=torch.int64, device=device)     # hits per cutoff, rank sum, rows, invalid

    def update(self, ranks, mask=None):
        """Adds one batch of ranks (int32 [B] on the GPU)."""
        _on_gpu(ranks, "RankingMeter.update: ranks")
        if ranks.dtype != torch.int32 or ranks.dim() != 1:
            raise ValueError(f"RankingMeter.update: ranks must be int32 [B], got {ranks.dtype} {tuple(ranks.shape)}")
        ranks = ranks.detach().contiguous()
        n = ranks.shape[0]
        if mask is not None:
            _on_gpu(mask, "RankingMeter.update: mask")
            if mask.shape != ranks.shape:
                raise ValueError(f"RankingMeter.update: {n} ranks but a mask of shape {tuple(mask.shape)}")
            mask = (mask.detach() != 0).to(torch.uint8).contiguous()
        if n == 0:
            return
        ws = L.workspace("recnn_rank_metrics_workspace_bytes", n, device=ranks.device)
        L.call("recnn_rank_metrics", L.ptr(ranks), L.ptr(mask), n, self._ks, len(self.ks), L.ptr(self.sums), L.ptr(self.counts),
               L.ptr(ws), L.current_stream())

    def reset(self):
        self.sums.zero_()
        self.counts.zero_()

    def _read(self, need_rows=True):
        c = self.counts.tolist()                          # the one synchronisation; sums follow on the same stream
        if c[-1] != 0:
            raise ValueError(f"RankingMeter: {c[-1]} rows had a negative rank (a target outside the table) and were not counted")
        if need_rows and c[-2] == 0:
            raise ValueError("RankingMeter: no rows counted yet")
        return c, self.sums.tolist()

    @property
    def rows(self):
        return self._read(need_rows=False)[0][-2]

    @property
    def invalid(self):
        return int(self.counts[-1])

    def hits(self):
        """{K: rows with rank < K} as Python ints."""
        c, _ = self._read(need_rows=False)
        return dict(zip(self.ks, c))

    def hit_rate(self):
        c, _ = self._read()
        return {k: h / c[-2] for k, h in zip(self.ks, c)}

    def ndcg(self):
        c, f = self._read()
        return {k: v / c[-2] for k, v in zip(self.ks, f)}

    @property
    def mrr(self):
        c, f = self._read()
        return f[-1] / c[-2]

    @property
    def mean_rank(self):
        c, _ = self._read()
        return c[-3] / c[-2]


__all__ += ["target_ranks", "RankingMeter"]


# ---- per-row exclusion (csrc/seen.hip): what a user has already consumed is left out of `search` and
# `rank_of`, as the usual offline protocol does before hit@K / NDCG / MRR.

class SeenMask:
    """One bit per (query row, item): `words` int64 [rows, ceil(n_items / 64)] on the GPU, bit (i & 63) of word (i >> 6) of row b
    set when item i is excluded for row b (the int64 holds the uint64 bit pattern).  Made by `SeenItems.mask`."""
    __slots__ = ("words", "n_items", "rows")

    def __init__(self, words, n_items):
        self.words, self.n_items, self.rows = words, int(n_items), words.shape[0]


def _row_ints(t, B, what, name):
    t = torch.as_tensor(t)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool or t.dim() != 1:
        raise ValueError(f"{what}: {name} must be a 1-D integer tensor, got {t.dtype} {tuple(t.shape)}")
    if B is not None and t.shape[0] != B:
        raise ValueError(f"{what}: {B} starts but {t.shape[0]} {name}")
    return t


class SeenItems:
    """Per query row, a list of item ids that do not exist for that row: row b's list is `ids[starts[b] : starts[b] + lengths[b]]`.

    `ids` is one integer tensor on the GPU that the rows' lists are slices of (a replay store's `items`, used as it is when it is
    int32; another integer dtype is converted once, values that do not fit int32 become -1).  `starts`, `lengths` and the optional
    `keep` are 1-D integer tensors of one length B.  Lists are unordered and may repeat ids; ids outside the catalogue and
    positions outside `ids` are ignored by the kernel, so nothing here synchronises to validate device data.  `keep[b]` (a row
    id, typically the row's target) is taken out of row b's list again.  `FrameEnv.seen_items` builds one from a batch."""

    def __init__(self, ids, starts, lengths, keep=None):
        what = "SeenItems"
        ids = torch.as_tensor(ids)
        if ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool or ids.dim() != 1:
            raise ValueError(f"{what}: ids must be a 1-D integer tensor, got {ids.dtype} {tuple(ids.shape)}")
        starts = _row_ints(starts, None, what, "starts")
        B = starts.shape[0]
        lengths = _row_ints(lengths, B, what, "lengths")
        if keep is not None:
            keep = _row_ints(keep, B, what, "keep")
        _on_gpu(ids, "SeenItems: ids")
        ids = ids.detach()
        if ids.dtype != torch.int32:
            if ids.dtype not in (torch.int8, torch.uint8, torch.int16):      # the rest can hold values int32 cannot
                wide = ids.to(torch.int64)
                ids = torch.where((wide >= -2 ** 31) & (wide < 2 ** 31), wide, -1)
            ids = ids.to(torch.int32)
        ids = ids.contiguous()
        self.ids = ids.clone() if ids.data_ptr() % 4 else ids
        dev = ids.device
        self.starts = starts.detach().to(dev, torch.int64).contiguous()
        self.lengths = lengths.detach().to(dev, torch.int64).contiguous()
        self.keep = None if keep is None else keep.detach().to(dev, torch.int64).contiguous()
        self.rows = B
        self._masks = {}

    @classmethod
    def from_lists(cls, lists, device="cuda", keep=None):
        """From one Python sequence of ids per row (for callers without a CSR)."""
        rows = [[int(i) for i in row] for row in lists]
        lengths = torch.tensor([len(r) for r in rows], dtype=torch.int64)
        starts = torch.cumsum(lengths, 0) - lengths
        flat = [i if -2 ** 63 <= i < 2 ** 63 else -1 for r in rows for i in r]
        ids = torch.tensor(flat, dtype=torch.int64).to(device)
        return cls(ids, starts, lengths, keep)

    def mask(self, n_items):
        """The `SeenMask` of these rows over a catalogue of `n_items` items: one launch, cached per `n_items`."""
        n_items = int(n_items)
        m = self._masks.get(n_items)
        if m is None:
            if not 0 < n_items < 2 ** 31:
                raise ValueError(f"SeenItems.mask: n_items must be positive and below 2^31, got {n_items}")
            nw = C.c_int64()
            L.call("recnn_seen_mask_words", n_items, C.byref(nw))          # refuses a catalogue above the LDS limit, by name
            words = torch.empty(self.rows, nw.value, dtype=torch.int64, device=self.ids.device)
            if self.rows:
                L.call("recnn_seen_mask_build", L.ptr(self.ids), self.ids.shape[0], L.ptr(self.starts), L.ptr(self.lengths),
                       L.ptr(self.keep), self.rows, n_items, L.ptr(words), L.current_stream())
            m = self._masks[n_items] = SeenMask(words, n_items)
        return m


__all__ += ["SeenItems", "SeenMask"]
