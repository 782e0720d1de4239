"""Float64 restatements of the optimizer arithmetic (csrc/optim.h opt_elem / soft_elem, csrc/optim_dev.h quirk_clip_coef, csrc/optim.hip
adam_elem / ranger_elem / radam_elem / norm_clip_coef / the L1 sums), each value carrying a running FIRST-ORDER bound on the distance
of the fp32 kernel result from it.  Plain numpy, no GPU.

Error model (nothing in it is measured; u = 2^-24, the fp32 unit round-off):
  * fp32 tensors handed to a kernel are exact;
  * a host double rounded to float on its way into a kernel is off by at most u |c| (0 when the double is a float already: 1.0, 0.5);
    a scalar that is rounded twice (lr -> float, then lr / bc1 -> float) is charged 2 u |c|.  Host scalars are computed here from the
    Python doubles the user wrote (beta2 = 0.999, not float32(0.999)): recnn_snap7 makes the kernels do the same;
  * every fp32 operation adds u |result| and propagates its operands' bounds: add / sub ea + eb; mul |a| eb + |b| ea;
    div ea / |b| + |a / b| eb / |b|; sqrt ea / (2 sqrt a), or sqrt(ea) at a = 0;
  * sums of non-negative terms: depth u sum|g|, depth = per-thread serial length + tree levels, read from the summation trees as written
    (wave_sum: 6 levels; block_sum256: 6 + 2).
The tests assert |gpu - value| <= 2 bound; the factor 2 covers the second-order terms.

Division and square root: the library is built with -O3 and without fast-math flags.  In the gfx950 device assembly of optim.hip every
fp32 `/` is the v_div_scale / v_rcp / v_fma refinement / v_div_fmas / v_div_fixup sequence and every sqrtf is v_sqrt followed by the
+-1 ulp residual correction (two v_fma + v_cndmask, with the 2^-96 input scaling) -- the correctly rounded forms, not a bare v_rcp /
v_sqrt (the only bare v_rcp_f32 belongs to a 64-bit INTEGER division).  Both are therefore charged u like every other operation.
(Read once by hand from `hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S optim.hip`; no test looks at assembly.)

Every fp32 intermediate of a restatement must be a normal number (or exactly 0), so that flush-to-zero behaviour is not under test: asserted
in every operation (make_inputs keeps |g| either 0 or >= 1e-9) -- except under `underflow_allowed()`, for a real step's own gradient.

MUTANTS: the Adam / Ranger / soft-update restatements take `mutant=`, one of ADAM_MUTANTS / RANGER_MUTANTS / SOFT_MUTANTS -- plausible wrong
formulas the assertions must reject (tests/test_optim_cpu.py shows that they do)."""
import contextlib
import math

import numpy as np

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126

ADAM_MUTANTS = ("eps_in_sqrt", "no_bc2", "decoupled_wd")
RANGER_MUTANTS = ("eps_in_sqrt", "l2_wd", "rect_early", "la_no_slow")
SOFT_MUTANTS = ("tau_swapped",)


_UNDERFLOW = [False]


@contextlib.contextmanager
def underflow_allowed():
    """For gradients the test does not choose (a real step's own): an intermediate below the normal range is charged FLT_MIN, which
    holds with or without flush-to-zero, instead of being refused."""
    _UNDERFLOW[0] = True
    try:
        yield
    finally:
        _UNDERFLOW[0] = False


class F:
    """float64 value(s) `v` with the bound `e` >= |fp32 result - v| (first order).  The operators are fp32 operations."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.asarray(e, dtype=np.float64)

    @staticmethod
    def _op(v, e):
        a = np.abs(v)
        assert bool(np.all(np.isfinite(v)))
        if _UNDERFLOW[0]:       # below the normal range the result is off by at most FLT_MIN, flushed to zero or not
            return F(v, e + U * a + np.where(a < FLT_MIN, FLT_MIN, 0.0))
        assert bool(np.all((a == 0) | (a >= FLT_MIN))), "a subnormal fp32 intermediate: flush-to-zero would be under test"
        return F(v, e + U * a)

    def __add__(self, o):
        return F._op(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return F._op(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return F._op(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    def __truediv__(self, o):
        q = self.v / o.v
        return F._op(q, self.e / np.abs(o.v) + np.abs(q) * o.e / np.abs(o.v))

    def __neg__(self):          # a sign flip does not round
        return F(-self.v, self.e)

    def sqrt(self):
        r = np.sqrt(self.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(self.v > 0, self.e / (2 * r), np.sqrt(self.e))
        return F._op(r, e)

    def fmin(self, c):
        """fminf(x, c) with an exactly representable c"""
        return F(np.where(self.v <= c, self.v, c), np.where(self.v <= c, self.e, 0.0))

    def bound(self):
        return np.broadcast_to(self.e, self.v.shape)


def exact(x):
    """an fp32 tensor (or an exactly representable constant) as the kernel reads it; an F passes through"""
    return x if isinstance(x, F) else F(np.asarray(x, dtype=np.float64), 0.0)


def host(c, roundings=1):
    """a host double that reaches the kernel rounded to float `roundings` times"""
    c = float(c)
    if roundings == 1 and float(np.float32(c)) == c:
        return F(c, 0.0)
    return F(c, roundings * U * abs(c))


def _scalar(x):
    return x if isinstance(x, F) else host(x)


# ------------------------------------------------------------------------------------------------ step scalars (double, as the hosts compute them)
def adam_scalars(lr, beta1, beta2, t):
    """opt_scalars_at / recnn_adam_flat_shadow: step_size = (float)((double)(float)lr / bc1), bc2_sqrt = (float)sqrt(bc2)"""
    bc1 = -math.expm1(t * math.log(beta1))
    bc2 = -math.expm1(t * math.log(beta2))
    return dict(step_size=host(lr / bc1, 2), bc2_sqrt=host(math.sqrt(bc2)), omb1=host(1.0 - beta1), omb2=host(1.0 - beta2),
                beta1=host(beta1), beta2=host(beta2))


def radam_step(t, beta1, beta2, nsma_thr=5.0, rect=None):
    """optim.h radam_scalars: (rectified?, step factor as a double, N_sma)"""
    b2t, b1t = math.exp(t * math.log(beta2)), math.exp(t * math.log(beta1))
    n_max = 2.0 / (1.0 - beta2) - 1.0
    n_sma = n_max - 2.0 * t * b2t / (1.0 - b2t)
    if rect is None:
        rect = n_sma > nsma_thr
    r = math.sqrt((1.0 - b2t) * (n_sma - 4.0) / (n_max - 4.0) * (n_sma - 2.0) / n_sma * n_max / (n_max - 2.0)) if rect else 1.0
    return bool(rect), r / (1.0 - b1t), n_sma


# ------------------------------------------------------------------------------------------------ element arithmetic
def adam(p, g, m, v, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, t, gs=1.0, mutant=None):
    """opt_elem's Adam branch == adam_elem (torch.optim.Adam: L2 decay folded into the gradient, eps outside the root, both bias corrections)."""
    assert mutant is None or mutant in ADAM_MUTANTS
    p, g, m, v, gs = exact(p), exact(g), exact(m), exact(v), _scalar(gs)
    s = adam_scalars(lr, beta1, beta2, t)
    bc2_sqrt = exact(1.0) if mutant == "no_bc2" else s["bc2_sqrt"]
    gj = g * gs
    if wd != 0 and mutant != "decoupled_wd":
        gj = gj + host(wd) * p
    m = m + s["omb1"] * (gj - m)
    v = s["beta2"] * v + (s["omb2"] * gj) * gj
    if mutant == "eps_in_sqrt":
        denom = (v + host(eps)).sqrt() / bc2_sqrt
    else:
        denom = v.sqrt() / bc2_sqrt + host(eps)
    if wd != 0 and mutant == "decoupled_wd":
        p = p - (host(lr) * host(wd)) * p
    p = p - s["step_size"] * (m / denom)
    return dict(p=p, m=m, v=v)


def ranger(p, g, m, v, slow, *, lr, beta1=0.95, beta2=0.999, eps=1e-5, wd=0.0, alpha=0.5, k=6, nsma_thr=5.0, t, gs=1.0, mutant=None):
    """opt_elem's Ranger branch == ranger_elem + the Lookahead sync of ranger_flat_kernel: RAdam with DECOUPLED decay, the rectified
    (N_sma > thr) and the unrectified update, every k-th step slow += alpha (p - slow); p = slow.  Returns also sync / rect."""
    assert mutant is None or mutant in RANGER_MUTANTS
    p, g, m, v, slow, gs = exact(p), exact(g), exact(m), exact(v), exact(slow), _scalar(gs)
    rect, step, _ = radam_step(t, beta1, beta2, nsma_thr)
    if mutant == "rect_early":
        rect, step, _ = radam_step(t, beta1, beta2, nsma_thr, rect=radam_step(t + 1, beta1, beta2, nsma_thr)[0])
    sl_lr = host(step) * host(lr)
    gj = g * gs
    if wd != 0 and mutant == "l2_wd":
        gj = gj + host(wd) * p
    v = host(beta2) * v + (host(1.0 - beta2) * gj) * gj
    m = host(beta1) * m + host(1.0 - beta1) * gj
    if wd != 0 and mutant != "l2_wd":
        p = p + (-host(wd) * host(lr)) * p
    if rect:
        den = (v + host(eps)).sqrt() if mutant == "eps_in_sqrt" else v.sqrt() + host(eps)
        p = p + (-sl_lr) * (m / den)
    else:
        p = p + (-sl_lr) * m
    sync = k > 0 and t % k == 0
    if sync:
        sl = slow + host(alpha) * (p - slow)
        p = sl
        if mutant != "la_no_slow":
            slow = sl
    return dict(p=p, m=m, v=v, slow=slow, sync=sync, rect=rect)


def radam_scalars_flat(lr, beta1, beta2, t):
    """recnn_radam_flat's host scalars (torch.optim.RAdam, foreach form): rect, S, U"""
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    rho_inf = 2.0 / (1.0 - beta2) - 1.0
    rho_t = rho_inf - 2.0 * t * beta2 ** t / bc2
    rect = rho_t > 5.0
    S = U_ = 0.0
    if rect:
        r = math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))
        S = math.sqrt(bc2) * (lr * r / bc1) * -1.0
    else:
        U_ = (lr * 1.0 / bc1) * -1.0
    return rect, S, U_


def norm_clip_coef(norm, max_norm):
    """optim.hip norm_clip_coef: fminf(max_norm / (norm + 1e-6f), 1); norm is an fp32 device value"""
    return (host(max_norm) / (exact(norm) + host(1e-6))).fmin(1.0)


def radam(p, g, m, v, *, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, t, norm=None, max_norm=1.0):
    """radam_flat_kernel + radam_elem; with a clip norm the scaled gradient is written back (returned as `g`)."""
    p, g, m, v = exact(p), exact(g), exact(m), exact(v)
    rect, S, U_ = radam_scalars_flat(lr, beta1, beta2, t)
    if norm is not None:
        g = g * norm_clip_coef(norm, max_norm)
    gi = g
    if wd != 0:
        gi = gi + host(wd) * p
    m = m + host(1.0 - beta1) * (gi - m)
    v = v * host(beta2) + (host(1.0 - beta2) * gi) * gi
    if rect:
        step = exact(1.0) / ((v.sqrt() + host(eps)) / host(S, 2))
    else:
        step = host(U_, 2)
    p = p + step * m
    return dict(p=p, g=g, m=m, v=v, rect=rect)


def soft(tp, p, tau, mutant=None):
    """soft_elem: target * (1 - tau) + param * tau, that operand order (1 - tau is an fp32 subtraction in the kernel)"""
    assert mutant is None or mutant in SOFT_MUTANTS
    tp, p, tau = exact(tp), exact(p), host(tau)
    keep = exact(1.0) - tau
    if mutant == "tau_swapped":
        keep, tau = tau, keep
    return tp * keep + p * tau


# ------------------------------------------------------------------------------------------------ sums and clip coefficients
def l1_sum(g, depth):
    s = float(np.abs(np.asarray(g, dtype=np.float64)).sum())
    return F(s, depth * U * s)


def engine_l1_depth(nblk):
    """l1_blocks_kernel (<= 4 serial adds per thread, block_sum256: 6 + 2 levels), then quirk_clip_coef over the nblk partials
    (ceil(nblk / 256) serial adds, block_sum256)"""
    return 4 + 8 + (nblk + 255) // 256 + 8


def flat_l1_depth(n):
    """recnn_l1_norm_flat: l1_part_kernel on grid = min(ceil(n / 256), 1024) workgroups, l1_final_kernel over their partials"""
    grid = max(1, min((n + 255) // 256, 1024))
    return (n + grid * 256 - 1) // (grid * 256) + 8 + (grid + 255) // 256 + 8


def quirk_clip_coef(l1, grad_scale):
    """quirk_clip_coef: clip_grad_norm_(max_norm=-1, norm_type=1): min(-1 / (sum|g| gs + 1e-6), 1)"""
    total = exact(l1) * _scalar(grad_scale)
    return (exact(-1.0) / (total + host(1e-6))).fmin(1.0)


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(n, seed):
    """fp32 arrays p ~ 0.1 N(0, 1); |g| log-uniform in [1e-9, 1e-1] with a random sign (1 in 128 exactly 0); a quarter of the elements with
    m = v = 0, the others with m and sqrt(v) of the gradient's magnitude; slow weights near p; a target."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    p = (0.1 * rng.standard_normal(n)).astype(f32)
    mag = 10.0 ** rng.uniform(-9.0, -1.0, n)
    g = (mag * rng.choice([-1.0, 1.0], n)).astype(f32)
    g[rng.random(n) < 1.0 / 128] = 0
    fresh = rng.random(n) < 0.25
    m = (mag * rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(f32)
    v = ((mag * rng.uniform(0.5, 2.0, n)) ** 2).astype(f32)
    m[fresh] = 0
    v[fresh] = 0
    slow = (p.astype(np.float64) + 0.01 * rng.standard_normal(n)).astype(f32)
    tgt = (0.1 * rng.standard_normal(n)).astype(f32)
    a = np.abs(g.astype(np.float64))
    assert bool(np.all((a == 0) | (a >= 1e-15)))
    return dict(p=p, g=g, m=m, v=v, slow=slow, tgt=tgt)


def ratio(got, ref):
    """max |got - ref.v| / ref.e over the elements (0 / 0 counts as 0): the assertion is ratio <= 2"""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref.v)
    e = ref.bound()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / e)
    return float(r.max()) if r.size else 0.0
