"""numpy float64 references for csrc/logprob.hip and csrc/ope.hip, and the error bound the GPU tests hold the log-prob kernel to.

The bound.  With u = 2^-24, gamma_j = j u / (1 - j u), K the contraction length and N the catalogue size, per row b

    E_b     = gamma_{K+1} max_n ( sum_k |x_bk W_nk| + |c_n| )          a logit: K products accumulated in fp32, plus c_n
    R_b     = u (128 + d + (L + 1) ln N + 2 |lse_b| + 2 |lp_b|)        the log-sum-exp around it
    allowed = 2 E_b + R_b

2 E_b because the picked logit and the log-sum-exp each carry one logit error.  In R_b, d is the longest chain of additions a
term of s = sum exp(z - m) passes through in the kernel as built (`chain_depth`: 7 in the lane, 4 across the 16 lanes of a row,
one per tile of the slice, one per slice), (L + 1) ln N pays for the rescaling s exp(m - m') at the expected number of times the
running maximum moves, the 2 |.| terms for the roundings of m + log s and z_a - lse, and 128 for the constant number of expf / logf
results on a term's path.  L is the error of expf and logf in ulp: no document installed next to the compiler states ocml's
figure, so L = 3, the OpenCL full-profile limit for exp and log, is assumed.  d <= N always.

bf16 mode: the reference first rounds x and W to bf16; products of two bf16 numbers are exact in fp32, so what is left is the
fp32 accumulation the formula already describes.

The estimators follow csrc/ope.hip's definitions in float64, batch after batch; next to every sum the reference keeps the sum of
the absolute values of its terms, which is what the tests scale their tolerance with.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
L_ULP = 3          # expf / logf: OpenCL full-profile limit (assumed; see above)
TILE = 128        # items per tile of logprob.hip: items_per_slice is a multiple of it


def gamma(j):
    return j * U / (1.0 - j * U)


def to_bf16(a):
    """float64 copy of `a` rounded to bfloat16 (nearest even)."""
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def chain_depth(N, items_per_slice):
    """Longest chain of additions a term of s passes through in logprob.hip: 7 + 4 + tiles per slice + slices."""
    tiles = (N + TILE - 1) // TILE
    per = min(items_per_slice // TILE, tiles)
    slices = (N + items_per_slice - 1) // items_per_slice
    return min(N, 11 + per + slices)


def default_items_per_slice(B, N):
    """What functional.default_items_per_slice documents: about 512 workgroups of 128 rows x slice, slices of whole tiles."""
    row_tiles = max(1, (B + 127) // 128)
    tiles = (N + TILE - 1) // TILE
    slices = max(1, min(tiles, 512 // row_tiles))
    return (tiles + slices - 1) // slices * TILE


def log_prob(x, W, c, actions, bf16=False):
    """(logprob, lse, E) in float64: E_b = gamma_{K+1} max_n (sum_k |x_bk W_nk| + |c_n|).  Invalid actions give NaN in logprob."""
    x, W, c = (np.asarray(t, dtype=np.float64) for t in (x, W, c))
    if bf16:
        x, W = to_bf16(x), to_bf16(W)
    a = np.asarray(actions, dtype=np.int64)
    B, K = x.shape
    N = W.shape[0]
    z = x @ W.T + c
    m = z.max(1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(1))
    ok = (a >= 0) & (a < N)
    lp = np.full(B, np.nan)
    lp[ok] = np.minimum(z[np.nonzero(ok)[0], a[ok]] - lse[ok], 0.0)
    E = gamma(K + 1) * (np.abs(x) @ np.abs(W).T + np.abs(c)).max(1)
    return lp, lse, E


def allowed(E, lp, lse, N, d, L=L_ULP):
    lp = np.where(np.isnan(lp), 0.0, lp)
    return 2.0 * E + U * (128.0 + d + (L + 1) * math.log(N) + 2.0 * np.abs(lse) + 2.0 * np.abs(lp))


def pow_int(b, e):
    """b^e by squaring."""
    b = np.array(b)
    r = np.ones_like(b)
    while e:
        if e & 1:
            r = r * b
        b = b * b
        e >>= 1
    return r


def _lambda_k(lp_pi, k):
    return k * pow_int(-np.expm1(lp_pi), k - 1)


def lambda_k(lp_pi, k):
    """K (1 - pi)^(K - 1) of the top-K off-policy correction; 1 - exp(lp) evaluated as -expm1(lp)."""
    return _lambda_k(np.asarray(lp_pi, dtype=np.longdouble), k).astype(np.float64)


def weights(lp_pi, lp_beta, top_k=0):
    """The importance weights, evaluated in extended precision and rounded to float64 once: the reference's own error stays
    out of the comparison (the kernel works in float64 throughout)."""
    lp_pi, lp_beta = np.asarray(lp_pi, dtype=np.longdouble), np.asarray(lp_beta, dtype=np.longdouble)
    w = np.exp(lp_pi - lp_beta)
    if top_k >= 1:
        w = w * _lambda_k(lp_pi, top_k)
    return w.astype(np.float64)


SUMS = ("w", "w2", "wr", "wc", "wcr", "r", "dr")


class Meter:
    """OffPolicyMeter in numpy float64.  `sums[k]` and `abs_sums[k]` (the sum of |terms|) for k in SUMS, `max_w`, counts."""

    def __init__(self, cap=math.inf, top_k=0):
        self.cap, self.top_k = float(cap), int(top_k)
        self.reset()

    def reset(self):
        self.sums = dict.fromkeys(SUMS, 0.0)
        self.abs_sums = dict.fromkeys(SUMS, 0.0)
        self.max_w = 0.0
        self.rows = self.invalid = self.capped = 0
        self.n_batch = 0

    def update(self, lp_pi, lp_beta, reward, mask=None, q_logged=None, v_dm=None):
        lp_pi, lp_beta, r = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (lp_pi, lp_beta, reward))
        keep = np.ones(len(r), dtype=bool) if mask is None else np.asarray(mask) != 0
        bad = keep & (np.isnan(lp_pi) | np.isnan(lp_beta))
        keep = keep & ~bad
        self.invalid += int(bad.sum())
        self.rows += int(keep.sum())
        self.n_batch = max(self.n_batch, len(r))
        lp_pi, lp_beta, r = lp_pi[keep], lp_beta[keep], r[keep]
        w = weights(lp_pi, lp_beta, self.top_k)
        wc = np.minimum(w, self.cap)
        self.capped += int((w > self.cap).sum())
        terms = {"w": w, "w2": w * w, "wr": w * r, "wc": wc, "wcr": wc * r, "r": r}
        if q_logged is not None:
            q = np.asarray(q_logged, dtype=np.float32).astype(np.float64)[keep]
            v = np.asarray(v_dm, dtype=np.float32).astype(np.float64)[keep]
            terms["dr"] = v + w * (r - q)       # r - q is exact: both are fp32 values
        for k, t in terms.items():
            self.sums[k] += float(t.sum()) if len(t) else 0.0
            self.abs_sums[k] += float(np.abs(t).sum()) if len(t) else 0.0
        if len(w):
            self.max_w = max(self.max_w, float(w.max()))

    def sum_tol(self, k):
        """(n + 16) 2^-53 sum |terms|: n roundings of the additions (any order) and 16 for the few roundings inside a term
        (two exponentials, the power's products, the products with r), n the rows of the largest update."""
        return (self.n_batch + 16) * 2.0 ** -53 * self.abs_sums[k]

    def readouts(self):
        """{name: (value, tolerance)}.  A mean over rows is sum / rows and carries (n + 16) 2^-53 sum |terms| / rows, the terms
        being those of the mean's sum, nothing added.  snips and ess are quotients of two sums, for which "the terms" are not
        defined; they carry the two sums' tolerances propagated to first order: (tol_a + |a / b| tol_b) / |b|, and for the square
        (sum w)^2 twice |sum w| tol_w."""
        s, n = self.sums, self.rows
        t = {k: self.sum_tol(k) for k in SUMS}

        def mean(k):
            return s[k] / n, t[k] / n

        def ratio(a, ta, b, tb):
            v = a / b
            return v, (ta + abs(v) * tb) / abs(b)
        out = {"ips": mean("wr"), "capped_ips": mean("wcr"), "mean_weight": mean("w"), "logged_mean": mean("r"),
               "snips": ratio(s["wr"], t["wr"], s["w"], t["w"]),
               "ess": ratio(s["w"] * s["w"], 2.0 * abs(s["w"]) * t["w"], s["w2"], t["w2"]),
               "max_weight": (self.max_w, 16 * 2.0 ** -53 * self.max_w),
               "capped_share": (self.capped / n, 0.0), "rows": (n, 0), "invalid": (self.invalid, 0)}
        if self.abs_sums["dr"] or self.sums["dr"]:
            out["dr"] = mean("dr")
        return out
