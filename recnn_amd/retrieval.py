"""Exact batched nearest-item search on the GPU: the retrieval step that turns generated actions into item ids.

`FlatIndex(table, metric)` mirrors how the reference's demo uses faiss (`examples/streamlit_demo.py:190-204`:
IndexFlatL2 / IndexFlatIP / IndexFlatIP over L2-normalised rows) and `MilvusConnection.search`
(`recnn/data/db_con.py:45-56`): `search(queries, k)` returns `(distances[B, k], ids[B, k])`, best first.
SURVEY.md 8 row f2 ("next"); kernel in csrc/topk.hip.

It also takes the metrics of the reference's per-item scipy ranking loop (`examples/streamlit_demo.py:207-231`, `rank`;
`examples/[Results]/1. Ranking.ipynb`): the names of `scipy.spatial.distance.cdist` in `DIST_METRICS`, or the scipy
functions themselves (`distance.canberra`).  `cdist(queries, table, metric)` gives the whole distance matrix.  Kernel in
csrc/rank.hip; DESIGN.md section 11.

`IVFFlatIndex(table, nlist, metric)` is the inverted-file counterpart (faiss's IndexIVFFlat, Milvus's IVF_FLAT): k-means lists and a
search that scores only the `nprobe` nearest of them.  Kernels in csrc/ivf.hip; DESIGN.md section 24.
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
        suffix, mask = ("", ()) if exclude is None else ("_excluding", (L.ptr(m.words), m.words.shape[1]))
        head = (L.ptr(q), q.stride(0), B, L.ptr(self.table), self.n_items, self.dim)
        if self.metric in DIST_METRICS:
            ws = L.workspace("recnn_dist_workspace_bytes", B, self.n_items, DIST_METRICS[self.metric], k, device=q.device)
            L.call("recnn_dist_topk" + suffix, *head, DIST_METRICS[self.metric], self.p, L.ptr(self.aux), k, L.ptr(dist), L.ptr(ids),
                   L.ptr(ws), L.current_stream(), *mask)
        else:
            ws = L.workspace("recnn_topk_workspace_bytes", B, k, device=q.device)
            L.call("recnn_topk_search" + suffix, *head, METRICS[self.metric], L.ptr(self.aux), k, L.ptr(dist), L.ptr(ids), L.ptr(ws),
                   L.current_stream(), *mask)
        return dist, ids

    def _exclusion(self, exclude, B, what):
        """The `SeenMask` of an `exclude` argument, checked against this index and a batch of B rows."""
        return _exclusion(exclude, B, self.n_items, self.table.device, what)

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
        if B == 0:                                                       # an empty batch has no storage to point at
            return rank
        suffix, mask = ("", ()) if exclude is None else ("_excluding", (L.ptr(m.words), m.words.shape[1]))
        head = (L.ptr(q), q.stride(0), B, L.ptr(self.table), self.n_items, self.dim)
        tail = (L.ptr(self.aux), L.ptr(t), L.ptr(rank))
        if self.metric in DIST_METRICS:
            ws = L.workspace("recnn_dist_target_rank_workspace_bytes", B, self.n_items, DIST_METRICS[self.metric], device=q.device)
            L.call("recnn_dist_target_rank" + suffix, *head, DIST_METRICS[self.metric], self.p, *tail, L.ptr(ws), L.current_stream(), *mask)
        else:
            ws = L.workspace("recnn_topk_target_rank_workspace_bytes", B, self.n_items, device=q.device)
            L.call("recnn_topk_target_rank" + suffix, *head, METRICS[self.metric], *tail, L.ptr(ws), L.current_stream(), *mask)
        return rank


def _exclusion(exclude, B, n_items, device, what):
    """The `SeenMask` of an `exclude` argument, checked against a catalogue of `n_items` on `device` and a batch of B rows."""
    if not isinstance(exclude, (SeenItems, SeenMask)):
        raise TypeError(f"{what}: exclude must be a SeenItems or a SeenMask, got {type(exclude).__name__}")
    if exclude.rows != B:
        raise ValueError(f"{what}: {B} queries but an exclusion of {exclude.rows} rows")
    m = exclude.mask(n_items) if isinstance(exclude, SeenItems) else exclude
    if m.n_items != n_items:
        raise ValueError(f"{what}: the exclusion mask was built for n_items = {m.n_items}, the index holds {n_items}")
    if m.words.device != device:
        raise ValueError(f"{what}: the exclusion mask lives on {m.words.device}, the index on {device}")
    return m


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


# ---- the catalogue ranked by value (csrc/qrank.hip, csrc/scoresel.hip): selection from a score matrix that
# already exists, and the critic's Q-value of every (state, item) pair as that matrix.

MAX_K = 64


def _scores(scores, what):
    _on_gpu(scores, f"{what}: scores")
    if scores.dim() != 2 or scores.shape[1] < 1:
        raise ValueError(f"{what}: scores must be [B, N] with N >= 1, got {tuple(scores.shape)}")
    s = scores.detach()
    if s.dtype != torch.float32:
        s = s.to(torch.float32)
    if s.stride(1) != 1 or (s.shape[0] > 1 and s.stride(0) < s.shape[1]) or s.data_ptr() % 4:
        s = s.contiguous()
    return s


def _ld(s):
    return s.stride(0) if s.shape[0] > 1 else s.shape[1]


def _mask_rows(m, r0, r1):
    """(pointer, words per row) of rows [r0, r1) of a `SeenMask`, or (NULL, 0)."""
    if m is None:
        return None, 0
    return C.c_void_p(m.words.data_ptr() + r0 * m.words.stride(0) * 8), m.words.shape[1]


def _check_k(k, what):
    if int(k) != k or not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k must be an integer from 1 to {MAX_K}, got {k}")
    return int(k)


def _select_topk(s, ld, B, N, k, out_s, out_i, m, r0):
    ws = L.workspace("recnn_scores_topk_workspace_bytes", B, k, device=out_s.device)
    mp, W = _mask_rows(m, r0, r0 + B)
    L.call("recnn_scores_topk", s, ld, B, N, k, L.ptr(out_s), L.ptr(out_i), L.ptr(ws), L.current_stream(), mp, W)


def _select_rank(s, ld, B, N, t, out_r, m, r0):
    ws = L.workspace("recnn_scores_rank_workspace_bytes", B, N, device=out_r.device)
    mp, W = _mask_rows(m, r0, r0 + B)
    L.call("recnn_scores_rank", s, ld, B, N, L.ptr(t), L.ptr(out_r), L.ptr(ws), L.current_stream(), mp, W)


def topk_of_scores(scores, k, exclude=None):
    """(values float32[B, k], ids int64[B, k]) of a float32 score matrix [B, N] on the GPU (any row stride): larger score first,
    ties to the smaller id (-0 == +0), NaN after every number in id order.  `exclude` (a `SeenItems` or `SeenMask` of B rows): the
    items excluded in a row do not exist for it.  k <= 64 and may exceed N; a row with fewer than k items left ends in id -1 with
    score -inf.  N is not limited by k or by 16-bit ids: `DiscreteActor`'s probabilities over a whole catalogue are such a matrix."""
    what = "topk_of_scores"
    s = _scores(scores, what)
    k = _check_k(k, what)
    B, N = s.shape
    m = None if exclude is None else _exclusion(exclude, B, N, s.device, what)
    out_s = torch.empty(B, k, dtype=torch.float32, device=s.device)
    out_i = torch.empty(B, k, dtype=torch.int64, device=s.device)
    if B:
        _select_topk(L.ptr(s), _ld(s), B, N, k, out_s, out_i, m, 0)
    return out_s, out_i


def rank_in_scores(scores, targets, exclude=None):
    """int32 [B]: per row of a float32 score matrix [B, N] on the GPU, how many items come before item `targets[b]` in the order of
    `topk_of_scores` (0 = the target has the best score); -1 for a target outside [0, N).  Excluded items are not counted; the
    target's own bit is not consulted.  Feeds `RankingMeter.update` as `FlatIndex.rank_of` does."""
    what = "rank_in_scores"
    s = _scores(scores, what)
    B, N = s.shape
    t = _targets(targets, B, s.device, what)
    m = None if exclude is None else _exclusion(exclude, B, N, s.device, what)
    rank = torch.empty(B, dtype=torch.int32, device=s.device)
    if B:
        _select_rank(L.ptr(s), _ld(s), B, N, t, rank, m, 0)
    return rank


ITEM_DIM = 128            # the embedding width of every index of this module
MAX_HIDDEN = 256          # the pair kernel keeps all hidden columns of its pair rows in accumulators
# One block of Q is [rows, N] float32.  256 MiB holds the 2048-row evaluation batch of the reference's catalogue (2048 x 26,744 x 4 =
# 209 MiB) in one block, so a batch is one pair launch and one selection; more buys nothing (the pair kernel's grid is full from a
# few hundred rows on) and less only adds launches.  Results do not depend on it.
DEFAULT_WORKSPACE_BYTES = 256 << 20


def _id_matrix(ids, device, what, B=None, rows_of=None):
    """A candidate id matrix as the kernels take it: int32 or int64 [B, K] with unit column stride, any row stride, on `device`;
    with `B`, of that many rows (the rows of the `rows_of` it goes with)."""
    if not isinstance(ids, torch.Tensor) or ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
        raise ValueError(f"{what}: ids must be an integer tensor [B, K], got "
                         f"{ids.dtype if isinstance(ids, torch.Tensor) else type(ids).__name__}")
    if ids.dim() != 2 or ids.shape[1] < 1:
        raise ValueError(f"{what}: ids must be [B, K] with K >= 1, got {tuple(ids.shape)}")
    if ids.device != device:
        raise ValueError(f"{what}: the ids live on {ids.device}, the index on {device}")
    if B is not None and ids.shape[0] != B:
        raise ValueError(f"{what}: {B} {rows_of} but ids of {ids.shape[0]} rows")
    t = ids.detach()
    if t.dtype not in (torch.int32, torch.int64):
        t = t.to(torch.int64)
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


class CriticIndex:
    """The catalogue ranked by a critic's Q-value: `Q[b, n] = critic(state[b], table[n])` for every item, eval semantics (no
    dropout, whatever `critic.training` says), without the [B N, H] activations ever reaching memory (csrc/qrank.hip).

    `critic` is a `recnn_amd.nn.Critic` (three linear layers, one output) with hidden size <= 256 whose `linear1` takes
    S + 128 inputs; `table` float32 [N, 128] on the GPU.  The constructor snapshots the weights and computes the items' share of
    layer 1, as `FlatIndex` snapshots its table; call `refresh()` after training steps.  fp32 only.

    `search` and `rank_of` compute Q for a block of state rows at a time into a workspace of at most `max_workspace_bytes`
    (default 256 MiB: the reference's 2048 x 26,744 evaluation batch in one block; never less than 16 rows) and select from it
    (csrc/scoresel.hip).  The bits of `Q[b, n]` depend on that pair alone, so no result depends on the batch or the block size."""

    def __init__(self, critic, table, max_workspace_bytes=None):
        from .nn.models import Critic
        lin = [getattr(critic, n, None) for n in ("linear1", "linear2", "linear3")]
        if not isinstance(critic, Critic) or any(not isinstance(l, torch.nn.Linear) for l in lin):
            raise TypeError(f"CriticIndex: critic must be a three-layer recnn_amd.nn.Critic, got {type(critic).__name__}")
        if table.dim() != 2 or table.shape[1] != ITEM_DIM or table.shape[0] < 1:
            raise ValueError(f"CriticIndex: the item table must be [N, {ITEM_DIM}] (the embedding width is {ITEM_DIM}), got "
                             f"{tuple(table.shape)}")
        l1, l2, l3 = lin
        H = l1.out_features
        if H > MAX_HIDDEN:
            raise ValueError(f"CriticIndex: hidden size {H} is above the pair kernel's limit of {MAX_HIDDEN}")
        if l1.in_features <= ITEM_DIM or l2.in_features != H or l2.out_features != H or l3.in_features != H or l3.out_features != 1:
            raise ValueError(f"CriticIndex: Critic.linear1 must take S + {ITEM_DIM} inputs (S >= 1) and the layers must be "
                             f"[H, S + {ITEM_DIM}], [H, H], [1, H]; got linear1 {tuple(l1.weight.shape)}, linear2 "
                             f"{tuple(l2.weight.shape)}, linear3 {tuple(l3.weight.shape)}")
        if max_workspace_bytes is None:
            max_workspace_bytes = DEFAULT_WORKSPACE_BYTES
        if int(max_workspace_bytes) != max_workspace_bytes or max_workspace_bytes < 1:
            raise ValueError(f"CriticIndex: max_workspace_bytes must be a positive integer, got {max_workspace_bytes}")
        _on_gpu(table, "CriticIndex: the item table")
        self.critic = critic
        self.table = table.detach().to(torch.float32).contiguous()
        self.n_items, self.dim = self.table.shape
        self.state_dim, self.hidden = l1.in_features - ITEM_DIM, H
        hp = C.c_int()
        L.call("recnn_qrank_hidden_padded", H, C.byref(hp))
        self._hp = hp.value
        rows = C.c_int64()
        L.call("recnn_qrank_block_rows", self.n_items, int(max_workspace_bytes), C.byref(rows))
        self.block_rows = rows.value
        self.refresh()

    @property
    def ntotal(self):
        return self.n_items

    def refresh(self):
        """Re-reads the critic's weights (after training steps) and recomputes the items' share of layer 1."""
        c, dev, hp, S = self.critic, self.table.device, self._hp, self.state_dim
        sp = (S + 15) // 16 * 16

        def pad(t, rows, cols):
            out = torch.zeros(rows, cols, dtype=torch.float32, device=dev)
            out[: t.shape[0], : t.shape[1]] = t.detach().to(dev, torch.float32)
            return out
        w1 = c.linear1.weight
        self._w1s = pad(w1[:, :S], hp, sp)
        self._w1a = pad(w1[:, S:], hp, ITEM_DIM)
        self._b1 = pad(c.linear1.bias[None], 1, hp)[0]
        self._w2 = pad(c.linear2.weight, hp, hp)
        self._b2 = pad(c.linear2.bias[None], 1, hp)[0]
        self._w3 = pad(c.linear3.weight, 1, hp)[0]
        self._b3 = float(c.linear3.bias.detach().to(torch.float32).item())
        self._e1 = torch.empty(self.n_items, hp, dtype=torch.float32, device=dev)
        L.call("recnn_qrank_layer1", L.ptr(self.table), ITEM_DIM, self.n_items, ITEM_DIM, L.ptr(self._w1a), ITEM_DIM, None, hp,
               L.ptr(self._e1), hp, L.current_stream())

    def _s1(self, state, what):
        """S1 = state W1[:, :S]^T + b1 for every row, [B, hidden padded]."""
        _on_gpu(state, f"{what}: the states")
        st = state.detach().to(torch.float32)
        if st.dim() == 1:
            st = st[None]
        if st.dim() != 2 or st.shape[1] != self.state_dim:
            raise ValueError(f"{what}: the states must be [B, {self.state_dim}], got {tuple(st.shape)}")
        if st.device != self.table.device:
            raise ValueError(f"{what}: the states live on {st.device}, the index on {self.table.device}")
        B, sp = st.shape[0], self._w1s.shape[1]
        if sp != self.state_dim or not st.is_contiguous() or st.data_ptr() % 16:
            x = torch.zeros(B, sp, dtype=torch.float32, device=st.device)
            x[:, : self.state_dim] = st
            st = x
        s1 = torch.empty(B, self._hp, dtype=torch.float32, device=st.device)
        if B:
            L.call("recnn_qrank_layer1", L.ptr(st), sp, B, sp, L.ptr(self._w1s), sp, L.ptr(self._b1), self._hp, L.ptr(s1), self._hp,
                   L.current_stream())
        return s1

    def _pairs(self, s1, r0, rows, out, ld_out):
        L.call("recnn_qrank_scores", C.c_void_p(s1.data_ptr() + r0 * self._hp * 4), self._hp, rows, L.ptr(self._e1), self._hp,
               self.n_items, self._hp, L.ptr(self._w2), L.ptr(self._b2), L.ptr(self._w3), self._b3, L.ptr(out), ld_out,
               L.current_stream())

    def q_values(self, state):
        """float32 [B, N]: the critic's value of every item for every state row (the counterpart of `cdist`).  Each entry is
        bit-identical to what `search` reports for that pair."""
        s1 = self._s1(state, "CriticIndex.q_values")
        B = s1.shape[0]
        out = torch.empty(B, self.n_items, dtype=torch.float32, device=s1.device)
        step = 65535 * 16                                  # one pair launch's rows
        for r0 in range(0, B, step):
            self._pairs(s1, r0, min(step, B - r0), out[r0:], self.n_items)
        return out

    def _blocks(self, B):
        rows = min(self.block_rows, B)
        ws = torch.empty(rows, self.n_items, dtype=torch.float32, device=self.table.device)
        return ws, [(r0, min(rows, B - r0)) for r0 in range(0, B, rows)]

    def search(self, state, k=10, exclude=None):
        """(q float32[B, k] descending, ids int64[B, k]): the k items of highest value per state row, ties to the smaller id.
        `exclude` as in `FlatIndex.search`; a row with fewer than k items left ends in id -1 with value -inf."""
        what = "CriticIndex.search"
        k = _check_k(k, what)
        s1 = self._s1(state, what)
        B = s1.shape[0]
        m = None if exclude is None else _exclusion(exclude, B, self.n_items, self.table.device, what)
        q = torch.empty(B, k, dtype=torch.float32, device=s1.device)
        ids = torch.empty(B, k, dtype=torch.int64, device=s1.device)
        if B == 0:
            return q, ids
        ws, blocks = self._blocks(B)
        for r0, rows in blocks:
            self._pairs(s1, r0, rows, ws, self.n_items)
            _select_topk(L.ptr(ws), self.n_items, rows, self.n_items, k, q[r0:r0 + rows], ids[r0:r0 + rows], m, r0)
        return q, ids

    def rank_of(self, state, targets, exclude=None):
        """int32 [B]: how many items the critic values above item `targets[b]` in state b (ties to the smaller id; 0 = the target
        is the critic's first choice), -1 for a target outside [0, n_items).  `exclude` as in `FlatIndex.rank_of`.  Feeds
        `RankingMeter.update` unchanged."""
        what = "CriticIndex.rank_of"
        s1 = self._s1(state, what)
        B = s1.shape[0]
        t = _targets(targets, B, s1.device, what)
        m = None if exclude is None else _exclusion(exclude, B, self.n_items, self.table.device, what)
        rank = torch.empty(B, dtype=torch.int32, device=s1.device)
        if B == 0:
            return rank
        ws, blocks = self._blocks(B)
        for r0, rows in blocks:
            self._pairs(s1, r0, rows, ws, self.n_items)
            _select_rank(L.ptr(ws), self.n_items, rows, self.n_items, t[r0:r0 + rows], rank[r0:r0 + rows], m, r0)
        return rank

    # ---- per-row candidate lists (csrc/qcand.hip)

    def _ids(self, ids, B, what):
        """The id matrix as the kernel takes it: int32 or int64 [B, K] with unit column stride, any row stride."""
        return _id_matrix(ids, self.table.device, what, B, "states")

    def _cand_args(self, s1, t):
        B, K = t.shape
        return (L.ptr(s1), self._hp, B, L.ptr(self._e1), self._hp, self.n_items, self._hp, L.ptr(self._w2), L.ptr(self._b2),
                L.ptr(self._w3), self._b3, L.ptr(t), t.stride(0) if B > 1 else K, K, int(t.dtype == torch.int64))

    def q_of(self, state, ids):
        """float32 [B, K]: `Q[b, j] = critic(state[b], table[ids[b, j]])` for an integer id matrix [B, K] (int32 or int64, any row
        stride, any K >= 1), one launch after layer 1 of the states.  Each entry has the bits of `q_values(state)[b, ids[b, j]]`;
        a slot whose id is outside [0, n_items) (the -1 `FlatIndex.search` pads with) reads nothing and gives -inf."""
        what = "CriticIndex.q_of"
        s1 = self._s1(state, what)
        B = s1.shape[0]
        t = self._ids(ids, B, what)
        out = torch.empty(B, t.shape[1], dtype=torch.float32, device=s1.device)
        if B:
            L.call("recnn_qcand_scores", *self._cand_args(s1, t), L.ptr(out), t.shape[1], L.current_stream())
        return out

    def rerank(self, state, ids, k=None, targets=None, _fallback=None):
        """(q float32 [B, k], ids int64 [B, k]): the candidates `ids` [B, K <= 64] of every row sorted by the critic's value, the
        first k of them (default K), in the launch that computes the values.  Order: larger Q first, ties to the smaller id, a
        repeated id to the smaller slot, -0 == +0, NaN after every number in id order; empty slots (ids outside [0, n_items)) come
        last as id -1 at -inf.  With `targets` (integer [B]) a third element `pos` int32 [B]: the number of non-empty slots before
        the first slot that holds `targets[b]`, -1 if no slot holds it or it is outside [0, n_items)."""
        what = "CriticIndex.rerank"
        s1 = self._s1(state, what)
        B = s1.shape[0]
        t = self._ids(ids, B, what)
        K = t.shape[1]
        if K > MAX_K:
            raise ValueError(f"{what}: the sorted form takes at most {MAX_K} candidates per row, got {K} (q_of takes any number)")
        if k is None:
            k = K
        if int(k) != k or not 1 <= k <= K:
            raise ValueError(f"{what}: k must be an integer from 1 to the {K} candidates per row, got {k}")
        k = int(k)
        tg = None if targets is None else _targets(targets, B, s1.device, what)
        q = torch.empty(B, k, dtype=torch.float32, device=s1.device)
        out = torch.empty(B, k, dtype=torch.int64, device=s1.device)
        pos = None if tg is None else torch.empty(B, dtype=torch.int32, device=s1.device)
        if B:
            L.call("recnn_qcand_rerank", *self._cand_args(s1, t), k, L.ptr(q), L.ptr(out), L.ptr(tg), L.ptr(pos), L.ptr(_fallback),
                   L.current_stream())
        return (q, out) if tg is None else (q, out, pos)


__all__ += ["topk_of_scores", "rank_in_scores", "CriticIndex"]


# ---- a diversifying rerank of a candidate slate (csrc/slate.hip): greedy maximal marginal relevance
# (Carbonell & Goldstein 1998) over the similarity matrix of a row's candidates, and the slate's intra-list distance.

class SlateDiversifier:
    """Similarity, greedy MMR selection and intra-list distance of per-row candidate lists `ids` [B, K <= 64] (int32 or int64, any
    row stride) over the rows of `table` (float32 [N, 128] on the GPU, snapshotted as the indexes do), one launch each.

    `similarity` "IP" / "COS" / "L2": with G = X X^T over a row's gathered table rows and n_i = G_ii, S_ij = G_ij, G_ij / (sqrt(n_i)
    sqrt(n_j)) (0 where a norm is 0), or -max((n_i + n_j) - 2 G_ij, 0).  A slot whose id is outside [0, N) (the -1 `search` pads
    with) is empty: its entries of S are 0, and no selection picks it.  S is bitwise symmetric and S_ij depends on the two table
    rows alone, not on B, K or the slots."""

    def __init__(self, table, similarity="COS"):
        what = "SlateDiversifier"
        if similarity not in METRICS:
            raise ValueError(f"{what}: similarity must be one of {sorted(METRICS)}, got {similarity!r}")
        if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.shape[1] != ITEM_DIM or table.shape[0] < 1:
            raise ValueError(f"{what}: the item table must be [N, {ITEM_DIM}] (the embedding width is {ITEM_DIM}), got "
                             f"{tuple(table.shape) if isinstance(table, torch.Tensor) else type(table).__name__}")
        _on_gpu(table, f"{what}: the item table")
        self.kind = similarity
        self.table = table.detach().to(torch.float32).contiguous()
        self.n_items, self.dim = self.table.shape

    @property
    def ntotal(self):
        return self.n_items

    def _lists(self, ids, what, B=None):
        """The id matrix checked: `_id_matrix` with K <= 64."""
        t = _id_matrix(ids, self.table.device, what, B, "rows of relevance")
        if t.shape[1] > MAX_K:
            raise ValueError(f"{what}: ids holds K = {t.shape[1]} candidates per row; a slate takes at most {MAX_K}")
        return t

    def _args(self, t, what):
        """The arguments every entry point begins with."""
        _on_gpu(t, f"{what}: ids")
        B, K = t.shape
        return (L.ptr(self.table), self.n_items, L.ptr(t), t.stride(0) if B > 1 else K, B, K, int(t.dtype == torch.int64),
                METRICS[self.kind])

    def similarity(self, ids):
        """float32 [B, K, K]: S of every row's candidates."""
        what = "SlateDiversifier.similarity"
        t = self._lists(ids, what)
        args = self._args(t, what)
        B, K = t.shape
        out = torch.empty(B, K, K, dtype=torch.float32, device=t.device)
        if B:
            L.call("recnn_slate_similarity", *args, L.ptr(out), L.current_stream())
        return out

    def rerank(self, relevance, ids, k=None, lam=0.5, normalize=False):
        """(score float32 [B, k], ids int64 [B, k], slots int32 [B, k]): k (default K) slots of every row picked greedily.  With
        lam32 = float32(lam) and mu32 = 1 - lam32, step 1 scores slot j as lam32 * r_j and step t > 1 as (lam32 * r_j) - (mu32 *
        m_j), m_j the largest S_js over the slots chosen so far, each operation rounded to fp32; the slot picked is the first not
        yet chosen in the order of `CriticIndex.rerank` (larger score first, ties to the smaller id, a repeated id to the smaller
        slot, -0 == +0, NaN after every number, empty slots last).  `relevance` float32 [B, K], larger is better; r_j is the
        relevance itself, or with `normalize` (rel_j - mn) / (mx - mn) over the row's non-empty slots of finite relevance (0 when
        mx == mn; a non-finite relevance passes through).  `score` is the score at the moment of the pick, `slots` the picked
        slot's index in the list; once the non-empty slots run out: score -inf, id -1, slot -1.  lam = 1 sorts by relevance,
        lam = 0 spreads the slate regardless of it."""
        what = "SlateDiversifier.rerank"
        if not isinstance(relevance, torch.Tensor) or not relevance.dtype.is_floating_point or relevance.dim() != 2:
            raise ValueError(f"{what}: relevance must be a floating-point tensor [B, K], got "
                             f"{(relevance.dtype, tuple(relevance.shape)) if isinstance(relevance, torch.Tensor) else type(relevance).__name__}")
        t = self._lists(ids, what, relevance.shape[0])
        B, K = t.shape
        if relevance.shape[1] != K:
            raise ValueError(f"{what}: relevance is {tuple(relevance.shape)} but ids {tuple(t.shape)}")
        if relevance.device != t.device:
            raise ValueError(f"{what}: the relevance lives on {relevance.device}, the ids on {t.device}")
        if k is None:
            k = K
        if isinstance(k, bool) or int(k) != k or not 1 <= k <= K:
            raise ValueError(f"{what}: k must be an integer from 1 to the {K} candidates per row, got {k}")
        k = int(k)
        lam = float(lam)
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"{what}: lam must be in [0, 1], got {lam}")
        args = self._args(t, what)
        r = relevance.detach().to(torch.float32)
        if r.stride(1) != 1 or (B > 1 and r.stride(0) < K) or r.data_ptr() % 4:
            r = r.contiguous()
        score = torch.empty(B, k, dtype=torch.float32, device=t.device)
        out = torch.empty(B, k, dtype=torch.int64, device=t.device)
        slots = torch.empty(B, k, dtype=torch.int32, device=t.device)
        if B:
            L.call("recnn_slate_rerank", *args, L.ptr(r), r.stride(0) if B > 1 else K, lam, int(bool(normalize)), k, L.ptr(score),
                   L.ptr(out), L.ptr(slots), L.current_stream())
        return score, out, slots

    def ild(self, ids):
        """float64 [B]: the slate's intra-list distance, the mean over unordered pairs of non-empty slots of D_ij = 1 - S_ij (COS),
        sqrt(-S_ij) (L2: the distance) or -S_ij (IP), formed in fp32 and summed in float64; NaN with fewer than two non-empty
        slots."""
        what = "SlateDiversifier.ild"
        t = self._lists(ids, what)
        args = self._args(t, what)
        out = torch.empty(t.shape[0], dtype=torch.float64, device=t.device)
        if t.shape[0]:
            L.call("recnn_slate_ild", *args, L.ptr(out), L.current_stream())
        return out


__all__ += ["SlateDiversifier"]


# ---- retrieve, then rerank (csrc/qcand.hip): the actor's proto-action picks the candidates by geometry, the
# critic orders them by value -- the Wolpertinger policy of Dulac-Arnold et al. (2015).

class TwoStageIndex:
    """`flat` (a `FlatIndex`) retrieves the `n_candidates` <= 64 items nearest to an action, `critic_index` (a `CriticIndex` over
    the same table) sorts them by Q(state, item).  `search` is the flat search's launches, layer 1 of the states and one rerank
    launch; the whole-catalogue `CriticIndex.search` stays the offline yardstick.

    `flat` may be an `IVFFlatIndex`: the candidates are then the nearest items of the `nprobe` lists `search` probes, and
    `rank_of` is refused (its identity needs the candidates to be the head of the flat order)."""

    def __init__(self, flat, critic_index, n_candidates=MAX_K):
        if not isinstance(flat, (FlatIndex, IVFFlatIndex)) or not isinstance(critic_index, CriticIndex):
            raise TypeError(f"TwoStageIndex: need a FlatIndex and a CriticIndex, got {type(flat).__name__} and "
                            f"{type(critic_index).__name__}")
        if int(n_candidates) != n_candidates or not 1 <= n_candidates <= MAX_K:
            raise ValueError(f"TwoStageIndex: n_candidates must be an integer from 1 to {MAX_K}, got {n_candidates}")
        if flat.n_items != critic_index.n_items:
            raise ValueError(f"TwoStageIndex: the two indexes must hold the same table; the flat index holds {flat.n_items} items, "
                             f"the critic index {critic_index.n_items}")
        if flat.table.device != critic_index.table.device:
            raise ValueError(f"TwoStageIndex: the flat index lives on {flat.table.device}, the critic index on "
                             f"{critic_index.table.device}")
        if n_candidates > flat.n_items:
            raise ValueError(f"TwoStageIndex: n_candidates = {n_candidates} but the table holds only {flat.n_items} items")
        self.flat, self.critic_index, self.n_candidates = flat, critic_index, int(n_candidates)
        self.n_items = flat.n_items
        self._diversifiers = {}

    @property
    def ntotal(self):
        return self.n_items

    def refresh(self):
        """Re-reads the critic's weights (`CriticIndex.refresh`)."""
        self.critic_index.refresh()

    def search(self, action, state, k=10, exclude=None, nprobe=None, diversify=None, similarity="COS"):
        """(q float32 [B, k] descending, ids int64 [B, k]): the k <= n_candidates candidates of highest value among the
        n_candidates items nearest to `action[b]`.  `exclude` as in `FlatIndex.search`; a row with fewer than k items left ends in
        id -1 at -inf.  `nprobe` (an `IVFFlatIndex` first stage only; default 16): the lists the first stage scores.

        `diversify=lam` (0 <= lam <= 1; default None: no such stage): the n_candidates retrieved items, sorted by the critic, are
        re-ranked by a `SlateDiversifier(flat.table, similarity)` with `normalize=True` (Q has no fixed scale), built on first use
        and kept per similarity.  q is then the critic's value of the k chosen items in the order of their choice -- no longer
        descending -- and -inf where the row ran out of items."""
        if isinstance(self.flat, IVFFlatIndex):
            cand = self.flat.search(action, self.n_candidates, DEFAULT_NPROBE if nprobe is None else nprobe, exclude)[1]
        else:
            if nprobe is not None:
                raise ValueError("TwoStageIndex.search: nprobe applies to an IVFFlatIndex first stage; this one is a FlatIndex")
            cand = self.flat.search(action, self.n_candidates, exclude)[1]
        if diversify is None:
            return self.critic_index.rerank(state, cand, k)
        if int(k) != k or not 1 <= k <= self.n_candidates:
            raise ValueError(f"TwoStageIndex.search: k must be an integer from 1 to the {self.n_candidates} candidates per row, got {k}")
        q, ids = self.critic_index.rerank(state, cand)
        _, out, slots = self.diversifier(similarity).rerank(q, ids, int(k), diversify, normalize=True)
        picked = torch.gather(q, 1, slots.clamp_min(0).to(torch.int64))
        return picked.masked_fill_(slots < 0, float("-inf")), out

    def diversifier(self, similarity="COS"):
        """The `SlateDiversifier` over `flat.table` that `search(diversify=)` uses, built once per similarity."""
        if similarity not in self._diversifiers:
            self._diversifiers[similarity] = SlateDiversifier(self.flat.table, similarity)
        return self._diversifiers[similarity]

    def rank_of(self, action, state, targets, exclude=None):
        """int32 [B]: the rank of item `targets[b]` in the order "the retrieved candidates by value, then every other item in the
        flat index's order": its position among the candidates if it is one, else `max(flat.rank_of, candidates retrieved)`;
        -1 for a target outside [0, n_items).  Feeds `RankingMeter.update` unchanged."""
        if isinstance(self.flat, IVFFlatIndex):
            raise ValueError("TwoStageIndex.rank_of: refused with an IVFFlatIndex first stage: the rank identity needs the "
                             "candidates to be the head of the flat index's order, and the items of the probed lists are not")
        cand = self.flat.search(action, self.n_candidates, exclude)[1]
        behind = self.flat.rank_of(action, targets, exclude)
        return self.critic_index.rerank(state, cand, 1, targets, _fallback=behind)[2]


__all__ += ["TwoStageIndex"]


# ---- IVF-Flat (csrc/ivf.hip): a k-means coarse quantiser over the table, the items stored per nearest
# centroid, and a search that scores only the `nprobe` nearest lists: faiss's IndexIVFFlat, Milvus's IVF_FLAT.

MAX_PROBE = 64
DEFAULT_NPROBE = 16       # what the reference's MilvusConnection.search passes on every call
IVF_METRICS = ("L2", "IP")


def _check_count(v, lo, hi, what, name, why=""):
    try:
        whole = not isinstance(v, bool) and int(v) == v
    except (TypeError, ValueError):
        whole = False
    if not whole:
        raise TypeError(f"{what}: {name} must be an integer, got {v!r}")
    if not lo <= v <= hi:
        raise ValueError(f"{what}: {name} must be an integer from {lo} to {hi}{why}, got {v}")
    return int(v)


class IVFFlatIndex:
    """Inverted-file search over the rows of `table` (float32 [N, 128] on the GPU): `nlist` k-means centroids, every item stored in
    the list of its nearest centroid, and `search(queries, k, nprobe)` scoring only the items of the `nprobe` lists whose centroids
    are nearest to (L2) or have the largest inner product with (IP) the query.  With `nprobe >= nlist` it is `FlatIndex.search`,
    bit for bit; with fewer probes it is that search restricted to the probed lists, each (query, item) score still with
    `FlatIndex`'s bits.  metric "L2" or "IP".

    Training is Lloyd's k-means under L2 for both metrics, as in faiss: `niter` rounds of (assign every item to its nearest centroid,
    ties to the smaller centroid id: `FlatIndex(centroids, "L2").search(table, 1)`; move every centroid to the fp32 mean of its list),
    then one final assignment that defines the lists.  Initial centroids: `centroids` (float32 [nlist, 128]) if given, else the
    table rows `torch.randperm(N, generator=<CPU generator seeded with seed>)[:nlist]`.  Deterministic: no float atomics, the order
    of every sum is fixed by the item ids.  A list with no items keeps its previous centroid; faiss re-splits a large cluster
    instead, this index does not.  `niter=0` with `centroids=` only builds the lists.

    `centroids` float32 [nlist, 128], `assignment` int32 [N] (the list of every item), `list_start` int32 [nlist + 1] (CSR over the
    lists), `list_ids` int32 [N] (item ids list by list, ascending id inside a list).  Items cannot be added or removed."""

    def __init__(self, table, nlist, metric="L2", niter=10, centroids=None, seed=0):
        what = "IVFFlatIndex"
        nlist = self._check_table(table, nlist, metric, what)
        niter = _check_count(niter, 0, 2 ** 31 - 1, what, "niter")
        seed = _check_count(seed, -2 ** 63, 2 ** 63 - 1, what, "seed")
        if centroids is not None:
            centroids = self._check_centroids(centroids, nlist, what)
        _on_gpu(table, f"{what}: the item table")
        self._set_table(table, nlist, metric)
        if centroids is None:
            rows = torch.randperm(self.n_items, generator=torch.Generator().manual_seed(seed))[:nlist]
            cent = self.table[rows.to(self.table.device)].contiguous()
        else:
            cent = centroids.detach().to(self.table.device, torch.float32).contiguous().clone()
        for _ in range(niter):
            _, start, ids = self._build_lists(self._nearest_centroid(cent))
            L.call("recnn_ivf_update_centroids", L.ptr(self.table), self.n_items, L.ptr(start), L.ptr(ids), nlist, L.ptr(cent),
                   L.current_stream())
        self._finish(cent, self._nearest_centroid(cent))

    @classmethod
    def from_assignment(cls, table, centroids, assignment, metric="L2"):
        """The index whose lists are `assignment` (integer [N], values in [0, nlist)) and whose centroids are `centroids`
        (float32 [nlist, 128]) as given: no training."""
        what = "IVFFlatIndex.from_assignment"
        if not isinstance(centroids, torch.Tensor) or centroids.dim() != 2:
            raise ValueError(f"{what}: centroids must be a float32 tensor [nlist, {ITEM_DIM}]")
        self = object.__new__(cls)
        nlist = self._check_table(table, centroids.shape[0], metric, what)
        centroids = self._check_centroids(centroids, nlist, what)
        a = torch.as_tensor(assignment)
        if a.dtype.is_floating_point or a.dtype.is_complex or a.dtype == torch.bool or a.dim() != 1 or a.shape[0] != table.shape[0]:
            raise ValueError(f"{what}: assignment must be a 1-D integer tensor of {table.shape[0]} entries, got {a.dtype} "
                             f"{tuple(a.shape)}")
        _on_gpu(table, f"{what}: the item table")
        self._set_table(table, nlist, metric)
        a = a.detach().to(self.table.device, torch.int64).contiguous()
        lo, hi = int(a.min()), int(a.max())
        if lo < 0 or hi >= nlist:
            raise ValueError(f"{what}: assignment must hold list ids in [0, {nlist}), got values from {lo} to {hi}")
        self._finish(centroids.detach().to(self.table.device, torch.float32).contiguous().clone(), a)
        return self

    # ---- construction
    @staticmethod
    def _check_table(table, nlist, metric, what):
        try:
            name = metric_name(metric)
        except ValueError:
            name = None
        if name not in IVF_METRICS:
            raise ValueError(f"{what}: metric must be \"L2\" or \"IP\", got {metric!r} (COS and the scipy metrics are FlatIndex's)")
        if not isinstance(table, torch.Tensor):
            raise TypeError(f"{what}: table must be a float32 tensor [N, {ITEM_DIM}], got {type(table).__name__}")
        if table.dim() != 2 or table.shape[1] != ITEM_DIM or table.shape[0] < 1:
            raise ValueError(f"{what}: table must be [N, {ITEM_DIM}] (the embedding width is {ITEM_DIM}), got {tuple(table.shape)}")
        if table.shape[0] >= 2 ** 31:
            raise ValueError(f"{what}: table holds {table.shape[0]} rows, the limit is 2^31 - 1")
        return _check_count(nlist, 1, table.shape[0], what, "nlist", " (the number of table rows)")

    @staticmethod
    def _check_centroids(centroids, nlist, what):
        if not isinstance(centroids, torch.Tensor) or centroids.dtype != torch.float32 or tuple(centroids.shape) != (nlist, ITEM_DIM):
            got = f"{centroids.dtype} {tuple(centroids.shape)}" if isinstance(centroids, torch.Tensor) else type(centroids).__name__
            raise ValueError(f"{what}: centroids must be a float32 tensor [{nlist}, {ITEM_DIM}] (nlist rows), got {got}")
        return centroids

    def _set_table(self, table, nlist, metric):
        self.metric = metric if isinstance(metric, str) else metric.__name__
        self.table = table.detach().to(torch.float32).contiguous()
        self.n_items, self.dim = self.table.shape
        self.nlist = nlist

    def _nearest_centroid(self, cent):
        """int64 [N]: the centroid of smallest squared L2 distance to every table row, ties to the smaller id."""
        return FlatIndex(cent, "L2").search(self.table, 1)[1].view(-1)

    def _build_lists(self, assign):
        dev, N = self.table.device, self.n_items
        assignment = torch.empty(N, dtype=torch.int32, device=dev)
        start = torch.empty(self.nlist + 1, dtype=torch.int32, device=dev)
        ids = torch.empty(N, dtype=torch.int32, device=dev)
        ws = L.workspace("recnn_ivf_lists_workspace_bytes", N, self.nlist, device=dev)
        L.call("recnn_ivf_build_lists", L.ptr(assign), N, self.nlist, L.ptr(assignment), L.ptr(start), L.ptr(ids), L.ptr(ws),
               L.current_stream())
        return assignment, start, ids

    def _finish(self, cent, assign):
        self.centroids = cent
        self.assignment, self.list_start, self.list_ids = self._build_lists(assign)
        # the table rows and the L2 |t|^2 term in list order: a list is one contiguous stream
        self._rows = torch.empty_like(self.table)
        L.call("recnn_ivf_gather_rows", L.ptr(self.table), self.n_items, L.ptr(self.list_ids), L.ptr(self._rows), L.current_stream())
        self._aux = None
        if self.metric == "L2":
            self._aux = torch.empty(self.n_items, dtype=torch.float32, device=self.table.device)
            L.call("recnn_topk_item_aux", L.ptr(self._rows), self.n_items, self.dim, METRICS["L2"], L.ptr(self._aux), L.current_stream())
        self.quantizer = FlatIndex(self.centroids, self.metric)

    # ---- search
    @property
    def ntotal(self):
        return self.n_items

    def _nprobe(self, nprobe, what):
        return min(_check_count(nprobe, 1, MAX_PROBE, what, "nprobe"), self.nlist)

    def _ivf_queries(self, queries, what):
        if not isinstance(queries, torch.Tensor):
            raise TypeError(f"{what}: queries must be a tensor [B, {ITEM_DIM}], got {type(queries).__name__}")
        if queries.dim() not in (1, 2) or queries.shape[-1] != ITEM_DIM:
            raise ValueError(f"{what}: queries must be [B, {ITEM_DIM}] or [{ITEM_DIM}], got {tuple(queries.shape)}")
        return _queries(queries, self.table.device)

    def probe(self, queries, nprobe):
        """(score float32 [B, p], lists int64 [B, p]), p = min(nprobe, nlist): the lists a search of `nprobe` probes scores, nearest
        centroid first under L2 (squared distances), largest inner product first under IP.  It is
        `FlatIndex(centroids, metric).search(queries, p)`."""
        what = "IVFFlatIndex.probe"
        p = self._nprobe(nprobe, what)
        return self.quantizer.search(self._ivf_queries(queries, what), p)

    def search(self, queries, k=10, nprobe=DEFAULT_NPROBE, exclude=None):
        """(distances float32 [B, k], ids int64 [B, k]) over the items of each query's `min(nprobe, nlist)` probed lists, in
        `FlatIndex.search`'s order and conventions: L2 squared distances ascending, IP scores descending, ties to the smaller id.
        k <= 64, nprobe <= 64.  `exclude` (a `SeenItems` or `SeenMask` of B rows) as in `FlatIndex.search`.  A row with fewer than k
        items in reach ends in id -1 with distance +inf (L2) or -inf (IP)."""
        what = "IVFFlatIndex.search"
        k = _check_count(k, 1, MAX_K, what, "k")
        if k > self.n_items:
            raise ValueError(f"{what}: k = {k} but the index holds only {self.n_items} items")
        p = self._nprobe(nprobe, what)
        q = self._ivf_queries(queries, what)
        B, dev = q.shape[0], q.device
        m = None if exclude is None else _exclusion(exclude, B, self.n_items, dev, what)
        dist = torch.empty(B, k, dtype=torch.float32, device=dev)
        ids = torch.empty(B, k, dtype=torch.int64, device=dev)
        if B == 0:
            return dist, ids
        lists = self.quantizer.search(q, p)[1]
        ws = L.workspace("recnn_ivf_search_workspace_bytes", B, p, self.nlist, k, device=dev)
        L.call("recnn_ivf_scan", L.ptr(q), q.stride(0), B, L.ptr(self._rows), L.ptr(self._aux), L.ptr(self.list_start),
               L.ptr(self.list_ids), self.nlist, self.n_items, METRICS[self.metric], L.ptr(lists), p, k, L.ptr(dist), L.ptr(ids),
               L.ptr(ws), L.current_stream(), None if m is None else L.ptr(m.words), 0 if m is None else m.words.shape[1])
        return dist, ids


__all__ += ["IVFFlatIndex"]
