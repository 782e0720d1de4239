"""numpy float64 reference for csrc/logprob_bwd.hip (the backward of the catalogue log-prob) and the error bound its tests hold the
kernels to.  Extends tests/ope_reference.py: same u, gamma_j and L.

The function.  z = x W^T + c, lse_b = logsumexp_n z_bn, lp_b = z_{b, a_b} - lse_b.  With upstream gradients g_lp, g_lse (g_lp taken
as 0 in a row whose action lies outside [0, N)):

    p_bn = exp(z_bn - lse_b)       D_bn = (g_lse_b - g_lp_b) p_bn + g_lp_b [n == a_b]
    dx = D W       dW = D^T x       dc_n = sum_b D_bn

The bound.  Per row b, with E_b = gamma_{K+1} max_n (sum_k |x_bk W_nk| + |c_n|) the error of a logit and d the forward's chain depth
(ope_reference.chain_depth; d <= N):

    delta_b = 2 E_b + u (128 + d + (L + 1) ln N + 2 |lse_b| + 2 max_n |z_bn - lse_b|)     error of the exponent z_bn - lse_b: the
                                                                                          recomputed logit, the forward's lse
    rho_b   = expm1(delta_b) + (L + 1) u                                                  relative error of p_bn (expf: L ulp)
    |dD_bn| <= |g_lse - g_lp|_b p_bn (rho_b + 3 u) + 2 u |D_bn|                           the subtraction, the product, the add

    tol(dx_bk) = sum_n |dD_bn| |W_nk| + gamma_{c1} sum_n |D_bn| |W_nk|
    tol(dW_nk) = sum_b |dD_bn| |x_bk| + gamma_{c2} sum_b |D_bn| |x_bk|
    tol(dc_n)  = sum_b |dD_bn|        + gamma_{c2} sum_b |D_bn|

c1 and c2 are the longest chains of INEXACT additions an output element passes through in the kernels as built:
  c1 = min(N, items_per_slice) + slices   (dx: the MFMA steps of a slice's tiles run one after the other into one accumulator, each
       adding 4 (fp32) or 32 (bf16) products -- at most one addition per item of the slice; items past N enter as exact zeros; then
       one addition per further slice in the merge kernel);
  c2 = B + 2   (dW: one accumulator over every row tile in row order, at most one addition per row, rows past B are exact zeros;
       dc: a lane adds its 32 values of every row tile, B / 4 in all, then 2 additions across the four lane groups -- below B + 2).
A product of the second matrix multiplication is exact in the fp32 accumulator's input (fp32 MFMA rounds once per addition; that
rounding is what gamma counts).

bf16 mode: the reference first rounds x and W to bf16 and is the gradient of that rounded function; the kernel also rounds D to bf16
before the second product, for which dD gains 2^-8 |D_bn|.
"""
import math

import numpy as np

import ope_reference as R

U, L_ULP, gamma = R.U, R.L_ULP, R.gamma

SHAPES = ((1, 1, 32), (127, 130, 32), (129, 200, 128), (200, 1000, 160), (300, 1500, 256))     # (B, N, K)


def bwd_items_per_slice(B, N, K):
    """What functional.catalogue_bwd_items_per_slice documents: about 256 workgroups of 128 rows x slice (512 where K <= 128),
    slices of whole tiles."""
    row_tiles = max(1, (B + 127) // 128)
    tiles = (N + R.TILE - 1) // R.TILE
    slices = max(1, min(tiles, (512 if K <= 128 else 256) // row_tiles))
    return (tiles + slices - 1) // slices * R.TILE


def chain_dx(N, items_per_slice):
    """c1: items of a slice + slices."""
    return min(N, items_per_slice) + (N + items_per_slice - 1) // items_per_slice


def chain_dw(B):
    """c2: rows + 2."""
    return B + 2


def backward(x, W, c, actions, g_lp, g_lse, bf16=False, d=None, c1=None, c2=None):
    """dict(dx, dW, dc, tol_dx, tol_dW, tol_dc, lp, lse, D) in float64.  g_lp / g_lse None mean zeros.  d defaults to N, c1 to
    N + 64 and c2 to B + 64 (the loosest chains)."""
    x, W, c = (np.asarray(t, dtype=np.float64) for t in (x, W, c))
    if bf16:
        x, W = R.to_bf16(x), R.to_bf16(W)
    a = np.asarray(actions, dtype=np.int64)
    B, K = x.shape
    N = W.shape[0]
    d = N if d is None else d
    c1 = N + 64 if c1 is None else c1
    c2 = B + 64 if c2 is None else c2
    g_lp = np.zeros(B) if g_lp is None else np.asarray(g_lp, dtype=np.float64)
    g_lse = np.zeros(B) if g_lse is None else np.asarray(g_lse, dtype=np.float64)
    ok = (a >= 0) & (a < N)
    g_lp = np.where(ok, g_lp, 0.0)
    z = x @ W.T + c
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    p = np.exp(z - lse[:, None])
    gd = g_lse - g_lp
    D = gd[:, None] * p
    rows = np.nonzero(ok)[0]
    D[rows, a[rows]] += g_lp[rows]
    lp = np.full(B, np.nan)
    lp[rows] = z[rows, a[rows]] - lse[rows]

    E = gamma(K + 1) * (np.abs(x) @ np.abs(W).T + np.abs(c)).max(1)
    delta = 2.0 * E + U * (128.0 + d + (L_ULP + 1) * math.log(N) + 2.0 * np.abs(lse) + 2.0 * np.abs(z - lse[:, None]).max(1))
    rho = np.expm1(delta) + (L_ULP + 1) * U
    aD = np.abs(D)
    dD = np.abs(gd)[:, None] * p * (rho + 3.0 * U)[:, None] + 2.0 * U * aD
    if bf16:
        dD = dD + 2.0 ** -8 * aD
    aW, ax = np.abs(W), np.abs(x)
    return {"dx": D @ W, "dW": D.T @ x, "dc": D.sum(0), "lp": lp, "lse": lse, "D": D,
            "tol_dx": dD @ aW + gamma(c1) * (aD @ aW),
            "tol_dW": dD.T @ ax + gamma(c2) * (aD.T @ ax),
            "tol_dc": dD.sum(0) + gamma(c2) * aD.sum(0)}


def worst_ratio(got, ref, name):
    """max |got - ref| / tol over the elements of output `name` ('dx', 'dW', 'dc'); an element with zero tolerance must be exact."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref[name])
    tol = ref["tol_" + name]
    if not np.isfinite(err).all():
        return math.inf
    exact = tol == 0
    if (err[exact] != 0).any():
        return math.inf
    return float((err[~exact] / tol[~exact]).max()) if (~exact).any() else 0.0
