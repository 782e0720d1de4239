"""Reference for the IVF-Flat index (csrc/ivf.hip) in numpy, float64 / int64 throughout.

Lists: the stable sort of an assignment.  K-means: Lloyd's iterations under squared L2, ties to the smaller centroid id, the mean of
a list in float64, an empty list keeps its centroid.  Search: every item scored in float64, ordered by (score, id); the restricted
search is the same order over the items of the probed lists.  Nothing here imports torch or the package under test."""
import numpy as np

INF = float("inf")


def build_lists(assignment, nlist):
    """(list_start int64 [nlist + 1], list_ids int64 [N]): item ids list by list, ascending id inside a list."""
    a = np.asarray(assignment, dtype=np.int64)
    ids = np.argsort(a, kind="stable")
    start = np.zeros(nlist + 1, dtype=np.int64)
    start[1:] = np.cumsum(np.bincount(a, minlength=nlist))
    return start, ids


def sq_dists(x, c):
    """[len(x), len(c)] squared L2 distances, in int64 when both are integer arrays (exact), else float64."""
    x, c = np.asarray(x), np.asarray(c)
    if np.issubdtype(x.dtype, np.integer) and np.issubdtype(c.dtype, np.integer):
        x, c = x.astype(np.int64), c.astype(np.int64)
    else:
        x, c = x.astype(np.float64), c.astype(np.float64)
    return ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1)


def assign(table, centroids):
    """int64 [N]: the centroid of smallest squared distance, ties to the smaller id (np.argmin takes the first)."""
    return np.argmin(sq_dists(table, centroids), axis=1).astype(np.int64)


def relative_gap(table, centroids):
    """The smallest (d2 - d1) / d2 over the rows, d1 <= d2 the two smallest centroid distances: how far the assignment is from a
    near-tie that fp32 and float64 could decide differently."""
    d = np.sort(sq_dists(table, centroids), axis=1)
    return float(((d[:, 1] - d[:, 0]) / d[:, 1]).min())


def fp32_assignment_margin(table, centroids):
    """How safely an fp32 scorer reproduces `assign`: the smallest, over the rows, of (d2 - d1) - (e1 + e2), with d1 <= d2 the two
    smallest centroid distances and e the error bound of the fp32 key 2 t.c - |c|^2 for that pair.  The bound holds for any
    summation order: a K-term fp32 sum of products errs by at most g = K u / (1 - K u) times the sum of the absolute products
    (u = 2^-24), so the dot product contributes 2 g sum|t_k c_k|, |c|^2 contributes g |c|^2, and the final subtraction one rounding
    u |key|.  Positive: no fp32 evaluation can order a row's two nearest centroids the other way round."""
    t, c = np.asarray(table, dtype=np.float64), np.asarray(centroids, dtype=np.float64)
    u = 2.0 ** -24
    g = t.shape[1] * u / (1 - t.shape[1] * u)
    cn = (c ** 2).sum(1)
    err = 2 * g * (np.abs(t) @ np.abs(c).T) + g * cn[None, :] + u * np.abs(2 * (t @ c.T) - cn[None, :])
    d = sq_dists(t, c)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]
    rows = np.arange(len(t))
    d1, d2 = d[rows, order[:, 0]], d[rows, order[:, 1]]
    return float(((d2 - d1) - (err[rows, order[:, 0]] + err[rows, order[:, 1]])).min())


def list_means(table, centroids, start, ids, descending=False):
    """float64 [nlist, D]: the mean of every list, summed row after row in list order (or in the opposite order); an empty list
    keeps its centroid."""
    t = np.asarray(table, dtype=np.float64)
    out = np.asarray(centroids, dtype=np.float64).copy()
    for c in range(len(start) - 1):
        rows = ids[start[c]:start[c + 1]]
        if len(rows) == 0:
            continue
        if descending:
            rows = rows[::-1]
        total = np.zeros(t.shape[1], dtype=np.float64)
        for r in rows:
            total = total + t[r]
        out[c] = total / len(rows)
    return out


def kmeans_iteration(table, centroids, descending=False):
    """(assignment, new centroids float64) of one Lloyd iteration."""
    a = assign(table, centroids)
    start, ids = build_lists(a, len(centroids))
    return a, list_means(table, centroids, start, ids, descending)


def kmeans(table, centroids, niter, min_gap=None):
    """(final assignment, centroids float64, smallest relative gap seen): `niter` iterations and the final assignment.  With
    `min_gap` the precondition is asserted at every assignment: every row's two nearest centroids differ by more than that share."""
    cent = np.asarray(centroids, dtype=np.float64)
    gap = INF
    for _ in range(niter):
        gap = min(gap, relative_gap(table, cent))
        _, cent = kmeans_iteration(table, cent)
    gap = min(gap, relative_gap(table, cent))
    if min_gap is not None:
        assert gap > min_gap, f"the reference's precondition fails: relative gap {gap} <= {min_gap}"
    return assign(table, cent), cent, gap


def scores(queries, table, metric):
    """float64 [B, N] keys, smaller = better: squared distance (L2) or minus the inner product (IP)."""
    q, t = np.asarray(queries, dtype=np.float64), np.asarray(table, dtype=np.float64)
    if metric == "L2":
        return ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1)
    assert metric == "IP"
    return -(q @ t.T)


def search(queries, table, k, metric, allowed=None):
    """(dist float64 [B, k], ids int64 [B, k]): the k best items per row in (score, id) order, L2 squared distances ascending, IP
    scores descending.  `allowed` (bool [B, N]): the items that exist for each row; a short row ends in id -1 at +inf / -inf."""
    key = scores(queries, table, metric)
    B, N = key.shape
    ids = np.full((B, k), -1, dtype=np.int64)
    dist = np.full((B, k), INF if metric == "L2" else -INF)
    for b in range(B):
        live = np.arange(N) if allowed is None else np.nonzero(allowed[b])[0]
        order = live[np.lexsort((live, key[b, live]))][:k]
        ids[b, :len(order)] = order
        dist[b, :len(order)] = key[b, order] if metric == "L2" else -key[b, order]
    return dist, ids


def probe(queries, centroids, nprobe, metric):
    """int64 [B, p]: the p = min(nprobe, nlist) lists of every row, nearest centroid (L2) / largest inner product (IP) first."""
    return search(queries, centroids, min(nprobe, len(centroids)), metric)[1]


def probed_items(lists, assignment):
    """bool [B, N]: whether item n is in one of row b's probed lists."""
    a = np.asarray(assignment)
    return (a[None, :, None] == np.asarray(lists)[:, None, :]).any(-1)


def ivf_search(queries, table, centroids, assignment, k, nprobe, metric):
    """The restricted search: `search` over the items of the probed lists."""
    return search(queries, table, k, metric, probed_items(probe(queries, centroids, nprobe, metric), assignment))
