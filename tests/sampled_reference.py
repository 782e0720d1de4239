"""numpy float64 reference for csrc/sampled.hip (sampled softmax with negatives shared by the batch) and the error bound its tests hold
the kernels to.  Extends tests/xent_reference.py / tests/ope_reference.py: same u, gamma_j, L and the same delta / rho construction,
with ln N -> ln(S + 1): a row's softmax runs over its target and the S negatives.

The function.  Targets a [B], negatives n [S] (one list for every row, repeats allowed), corrections tq [B], nq [S]:

    z_t[b] = x_b . W[a_b] + c[a_b] - tq[b]         z[b, s] = x_b . W[n_s] + c[n_s] - nq[s]
    lse[b] = log(exp z_t[b] + sum_s exp z[b, s])   lp[b] = min(z_t[b] - lse[b], 0)

A negative outside [0, N) is absent (z = -inf) in every row; with remove_hits a negative equal to the row's target is absent in that
row.  A target outside [0, N): lp = NaN, lse over the negatives, g_lp taken as 0.  The closed-form gradient, gd = g_lse - g_lp,
p = exp(z - lse):

    D[b, s] = gd_b p[b, s]          D_t[b] = gd_b p_t[b] + g_lp[b]
    dx = D W[n] + D_t W[a]          dWs[s] = sum_b D[b, s] x_b       dcs[s] = sum_b D[b, s]          (compact, one row per negative)
    dW[i] = sum_{s: n_s = i} dWs[s] + sum_{b: a_b = i} D_t[b] x_b    dc[i] likewise                   (dense, scatter-summed by id)

The bound.  Per row b, E_b = gamma_{K+2} max over the row's live columns (sum_k |x_bk W_nk| + |c_n| + |q|): K products accumulated in
fp32, the bias and the correction.  d is the forward's chain depth (`chain_depth`):

    allowed(lp, lse) = 2 E_b + u (128 + d + (L + 1) ln(S + 1) + 2 |lse_b| + 2 |lp_b|)                       (ope_reference.allowed)
    delta_b = 2 E_b + u (128 + d + (L + 1) ln(S + 1) + 2 |lse_b| + 2 max_live |z - lse_b|)
    rho_b   = expm1(delta_b) + (L + 1) u
    |dD_bs| <= |gd_b| p_bs (rho_b + 3 u) + 2 u |D_bs|  (+ 2^-8 |D_bs| in bf16 mode: D is rounded before the second product)
    |dD_t,b| <= |gd_b| p_t,b (rho_b + 3 u) + 2 u |D_t,b|      (D_t is never rounded to bf16)

Chains of INEXACT additions, as the kernels are built:
  dx   c1 = min(S, items_per_slice) + slices + 2: at most one add per negative of a slice (absent columns and columns past S enter as
       exact zeros), one per further slice in the merge, then the target term D_t W[a] (one fused multiply-add; 2 allows an unfused one);
  dWs  c2 = rows of a chunk + chunks + 2: one accumulator over the chunk's row tiles in row order, one add per further chunk; dcs adds a
       lane's values of every row tile (rows / 4) and 2 across the lane groups, then the chunks -- below the same c2;
  a dense row: one add per contribution to that id (a wave adds a run of the sorted list in order, the pieces of a list in order):
       tol(dW[i]) = sum of its contributions' own tolerances + gamma_{cnt_i} sum |contributions|, and a target's contribution
       D_t[b] x_b carries |dD_t| |x_b| + u |D_t x_b| for its product.
bf16 mode: the reference first rounds x and W to bf16 and is the gradient of that rounded function (xent_reference's convention).
The bound is derived from the formats and the kernels' structure; nothing in it is fitted to a measured error.
"""
import math

import numpy as np

import ope_reference as R

U, L_ULP, gamma = R.U, R.L_ULP, R.gamma

SHAPES = ((1, 1, 2, 32), (127, 130, 300, 40), (129, 128, 1000, 128), (200, 257, 5000, 160), (300, 1500, 2000, 256))   # (B, S, N, K)


def fwd_items_per_slice(B, S):
    return R.default_items_per_slice(B, S)


def bwd_items_per_slice(B, S, K):
    """functional.catalogue_bwd_items_per_slice over the negatives."""
    row_tiles = max(1, (B + 127) // 128)
    tiles = (S + R.TILE - 1) // R.TILE
    slices = max(1, min(tiles, (512 if K <= 128 else 256) // row_tiles))
    return (tiles + slices - 1) // slices * R.TILE


def chunks_of(B, S):
    """(chunks, row tiles per chunk) of the dWs / dcs kernel: csrc/sampled.hip chunks_of."""
    row_tiles, item_tiles = (B + 127) // 128, (S + 127) // 128
    want = max(1, min(row_tiles, 256 // max(1, item_tiles)))
    tpc = max(1, (row_tiles + want - 1) // want)
    return max(1, (row_tiles + tpc - 1) // tpc), tpc


def chain_depth(S, items_per_slice):
    """Forward: 7 in the lane + 4 across lanes + tiles per slice + slices + the target's term."""
    tiles = (S + R.TILE - 1) // R.TILE
    per = min(items_per_slice // R.TILE, tiles)
    slices = (S + items_per_slice - 1) // items_per_slice
    return 12 + per + slices


def chain_dx(S, items_per_slice):
    return min(S, items_per_slice) + (S + items_per_slice - 1) // items_per_slice + 2


def chain_dw(B, S):
    chunks, tpc = chunks_of(B, S)
    return min(B, 128 * tpc) + chunks + 2


def run(x, W, c, targets, negatives, tq=None, nq=None, g_lp=None, g_lse=None, remove_hits=True, bf16=False, d=None, c1=None, c2=None):
    """dict in float64: lp, lse, tol_f (for lp and lse), dx, dWs, dcs, dW, dc, Dt and tol_dx, tol_dWs, tol_dcs, tol_dW, tol_dc.
    c None: zeros; tq / nq / g_lp / g_lse None: zeros.  d, c1, c2 default to the loosest chains (S + 64, S + 64, B + 64)."""
    x, W = np.asarray(x, dtype=np.float64), np.asarray(W, dtype=np.float64)
    if bf16:
        x, W = R.to_bf16(x), R.to_bf16(W)
    B, K = x.shape
    N = W.shape[0]
    a = np.asarray(targets, dtype=np.int64)
    n = np.asarray(negatives, dtype=np.int64)
    S = len(n)
    c = np.zeros(N) if c is None else np.asarray(c, dtype=np.float64)
    tq = np.zeros(B) if tq is None else np.asarray(tq, dtype=np.float64)
    nq = np.zeros(S) if nq is None else np.asarray(nq, dtype=np.float64)
    g_lp = np.zeros(B) if g_lp is None else np.asarray(g_lp, dtype=np.float64)
    g_lse = np.zeros(B) if g_lse is None else np.asarray(g_lse, dtype=np.float64)
    d = S + 64 if d is None else d
    c1 = S + 64 if c1 is None else c1
    c2 = B + 64 if c2 is None else c2
    ok = (a >= 0) & (a < N)
    live_n = (n >= 0) & (n < N)
    g_lp = np.where(ok, g_lp, 0.0)
    ac, nc = np.where(ok, a, 0), np.where(live_n, n, 0)
    Wn, Wa = W[nc], W[ac]

    live = np.broadcast_to(live_n[None, :], (B, S)).copy()
    if remove_hits:
        live &= ~(ok[:, None] & (n[None, :] == a[:, None]))
    z = np.where(live, x @ Wn.T + (c[nc] - nq)[None, :], -np.inf)
    zt = np.where(ok, (x * Wa).sum(1) + c[ac] - tq, -np.inf)
    allz = np.concatenate([zt[:, None], z], 1)
    m = allz.max(1)
    ms = np.where(np.isinf(m), 0.0, m)
    with np.errstate(divide="ignore"):
        lse = ms + np.log(np.exp(allz - ms[:, None]).sum(1))
    lsef = np.where(np.isinf(lse), 0.0, lse)
    p = np.exp(z - lsef[:, None])
    pt = np.where(ok, np.exp(zt - lsef), 0.0)
    lp = np.where(ok, np.minimum(zt - lse, 0.0), np.nan)
    gd = g_lse - g_lp
    D = gd[:, None] * p
    Dt = gd * pt + g_lp

    mag = np.where(live, np.abs(x) @ np.abs(Wn).T + (np.abs(c[nc]) + np.abs(nq))[None, :], 0.0)
    magt = np.where(ok, (np.abs(x) * np.abs(Wa)).sum(1) + np.abs(c[ac]) + np.abs(tq), 0.0)
    E = gamma(K + 2) * np.maximum(mag.max(1), magt)
    lnS = math.log(S + 1)
    lp0 = np.where(np.isnan(lp), 0.0, lp)
    tol_f = 2.0 * E + U * (128.0 + d + (L_ULP + 1) * lnS + 2.0 * np.abs(lsef) + 2.0 * np.abs(lp0))
    dev = np.where(np.isinf(allz), 0.0, np.abs(allz - lsef[:, None])).max(1)
    delta = 2.0 * E + U * (128.0 + d + (L_ULP + 1) * lnS + 2.0 * np.abs(lsef) + 2.0 * dev)
    rho = np.expm1(delta) + (L_ULP + 1) * U
    aD, aDt = np.abs(D), np.abs(Dt)
    dD = np.abs(gd)[:, None] * p * (rho + 3.0 * U)[:, None] + 2.0 * U * aD
    if bf16:
        dD = dD + 2.0 ** -8 * aD
    dDt = np.abs(gd) * pt * (rho + 3.0 * U) + 2.0 * U * aDt
    aWn, aWa, ax = np.abs(Wn) * live_n[:, None], np.abs(Wa) * ok[:, None], np.abs(x)

    out = {"lp": lp, "lse": lse, "tol_f": tol_f, "Dt": Dt, "D": D,
           "dx": D @ (Wn * live_n[:, None]) + Dt[:, None] * (Wa * ok[:, None]),
           "tol_dx": dD @ aWn + dDt[:, None] * aWa + gamma(c1) * (aD @ aWn + aDt[:, None] * aWa),
           "dWs": D.T @ x, "tol_dWs": dD.T @ ax + gamma(c2) * (aD.T @ ax),
           "dcs": D.sum(0), "tol_dcs": dD.sum(0) + gamma(c2) * aD.sum(0)}
    # dense: contributions by id
    ids = np.concatenate([n[live_n], a[ok]])
    cnt = np.bincount(ids, minlength=N).astype(np.float64)
    rows = np.concatenate([out["dWs"][live_n], (Dt[:, None] * x)[ok]])
    tol_rows = np.concatenate([out["tol_dWs"][live_n], (dDt[:, None] * ax + U * np.abs(Dt[:, None] * x))[ok]])
    sc = np.concatenate([out["dcs"][live_n], Dt[ok]])
    tol_sc = np.concatenate([out["tol_dcs"][live_n], dDt[ok]])
    dW, tW, aW = np.zeros((N, K)), np.zeros((N, K)), np.zeros((N, K))
    dc, tc, ac_ = np.zeros(N), np.zeros(N), np.zeros(N)
    np.add.at(dW, ids, rows)
    np.add.at(tW, ids, tol_rows)
    np.add.at(aW, ids, np.abs(rows))
    np.add.at(dc, ids, sc)
    np.add.at(tc, ids, tol_sc)
    np.add.at(ac_, ids, np.abs(sc))
    g = gamma(cnt)
    out.update({"dW": dW, "tol_dW": tW + g[:, None] * aW, "dc": dc, "tol_dc": tc + g * ac_, "count": cnt})
    return out


def worst_ratio(got, ref, name, tol=None):
    """max |got - ref| / tol over the elements of output `name`; an element with zero tolerance must be exact.  NaN must meet NaN."""
    got = np.asarray(got, dtype=np.float64)
    want = ref[name]
    tol = ref["tol_" + name] if tol is None else tol
    nan = np.isnan(want)
    if (np.isnan(got) != nan).any():
        return math.inf
    inf = np.isinf(want) & ~nan
    if (got[inf] != want[inf]).any():
        return math.inf
    fin = ~(nan | inf)
    err = np.abs(got[fin] - want[fin])
    tol = np.broadcast_to(tol, want.shape)[fin]
    if not np.isfinite(err).all():
        return math.inf
    exact = tol == 0
    if (err[exact] != 0).any():
        return math.inf
    return float((err[~exact] / tol[~exact]).max()) if (~exact).any() else 0.0


def torch_autograd(x, W, c, targets, negatives, tq, nq, g_lp, g_lse, remove_hits=True, dtype=None):
    """The materialised formulation through torch autograd on the CPU (float64 by default): (lp, lse, dx, dW dense, dc dense)."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    T = lambda v: torch.as_tensor(np.asarray(v), dtype=dtype)      # noqa: E731
    x, W, c = T(x).requires_grad_(), T(W).requires_grad_(), T(c).requires_grad_()
    a, n = torch.as_tensor(np.asarray(targets)), torch.as_tensor(np.asarray(negatives))
    N = W.shape[0]
    ok, live_n = (a >= 0) & (a < N), (n >= 0) & (n < N)
    ac, nc = a.clamp(0, N - 1), n.clamp(0, N - 1)
    z = x @ W[nc].T + (c[nc] - T(nq))[None]
    dead = ~live_n[None, :].expand_as(z)
    if remove_hits:
        dead = dead | (ok[:, None] & (n[None, :] == a[:, None]))
    z = z.masked_fill(dead, -math.inf)
    zt = (x * W[ac]).sum(1) + c[ac] - T(tq)
    zt_m = zt.masked_fill(~ok, -math.inf)
    lse = torch.logsumexp(torch.cat([zt_m[:, None], z], 1), 1)
    lp = torch.where(ok, zt - lse, torch.zeros_like(lse))
    glp = torch.where(ok, T(g_lp), torch.zeros_like(lse))
    fin = torch.isfinite(lse)
    (glp * lp + torch.where(fin, T(g_lse) * lse.masked_fill(~fin, 0.0), torch.zeros_like(lse))).sum().backward()
    lp = torch.where(ok, lp, torch.full_like(lp, math.nan))
    return tuple(t.detach().numpy().astype(np.float64) for t in (lp, lse, x.grad, W.grad, c.grad))
