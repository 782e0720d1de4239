"""Float64 references, derived fp32 bounds and the shared input sets of the categorical policy-head kernels (csrc/policy.hip).

Everything here runs on the CPU.  tests/test_gpu_policy_head.py compares the kernels with it element by element;
tests/test_policy_head_cpu.py pins it to torch's float64 autograd and checks that every input set moves its reference by at least
100 bounds when the option it exists for is removed.

Bounds are counts of the kernel's fp32 roundings times u = 2^-24, taken from the float64 reference alone.  A result that may
flush to zero gets one smallest normal (2^-126) of absolute floor.  HIP's expf is good to 1 ulp = 2 u, a division and an
addition to u.

categorical_kernel<SOFTMAX>, one 1024-thread workgroup per row, thread t owning the float4 groups t, t + 1024, ... (K of them):
  p_i    = fl(fl(expf(fl(x_i - max))) * fl(1 / denom))
           the subtraction moves the argument by u |x_i - max| and so the exponential by that much, relatively;
           expf 2 u, the reciprocal u, the product u:                       u (|x_i - max| + 4) + the denominator's error
  denom  = sum over threads of s_t expf(m_t - max), where s_t is the online sum of the thread's groups.  One term exp(x_j - max) is
           made of up to K + 1 exponentials (its own, a rescale at each later group, the last against the row's max: 2 u each), whose
           arguments add up to x_j - max, and K products; it then sits under 3 adds inside its float4, K adds of the running sum,
           6 DPP steps of the wave sum and 16 adds over the waves:          u (sum_j p_j |x_j - max| + 4 K + 27), relatively
  sum p  = (v.x + v.y) + (v.z + v.w), K adds of the running sum, 6 + 16 adds: u (K + 24), plus the errors of the p_i themselves
"""
import functools
import hashlib

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126                        # smallest normal fp32
PT = 1024                                 # threads of a row's workgroup, each loading float4s
CAT_EPS = float(torch.finfo(torch.float32).eps)
NS = (1, 3, 4, 5, 1021, 1024, 1025, 4095, 4096, 4097, 4100, 8195)
ROWS = (1, 31, 32, 33, 65)
INF = float("inf")


def round4(n):
    return (n + 3) // 4 * 4


def groups(n):
    """float4 groups the first thread of a 1024-thread row workgroup visits"""
    return max(1, -(-(round4(n) // 4) // PT))


def _gen(*seed):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) % (2 ** 31)) + 11)


def ulp32(v):
    """one unit in the last place of fp32 at |v| (float64 tensor in, float64 out)"""
    a = v.abs().clamp_min(TINY)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


# ---------------------------------------------------------------------------------------------------- softmax and log-prob
def softmax64(x):
    """x [R, N] (-inf allowed) -> max, sum exp(x - max), p, x - max; all float64"""
    x = x.double()
    mx = x.max(1, keepdim=True).values
    d = x - mx
    e = torch.exp(d)
    den = e.sum(1, keepdim=True)
    return mx[:, 0], den[:, 0], e / den, d


def softmax_bounds(x, c_num, c_den, c_sum):
    """reference and bounds of a softmax kernel: c_num roundings of a numerator beside its argument's, c_den of the denominator beside
    its terms' arguments, c_sum adds of the longest chain under sum p"""
    mx, den, p, d = softmax64(x)
    ad = torch.where(torch.isinf(d), torch.zeros_like(d), d.abs())
    spread = (p * ad).sum(1, keepdim=True)                     # sum_j p_j |x_j - max|
    rel_den = U * (spread + c_den)
    rel = U * (ad + c_num) + rel_den
    bound = rel * p + TINY
    return dict(max=mx, den=den, p=p, rel=rel, rel_den=rel_den[:, 0], bound=bound, masked=torch.isinf(d) & (d < 0),
                sum_bound=bound.sum(1) + U * c_sum)


def categorical_bounds(x):
    k = groups(x.shape[1])
    return softmax_bounds(x, 4, 4 * k + 27, k + 24)


def logprob64(p, actions):
    """log(clamp(p[a], eps, 1 - eps)) and whether the clamp was active; NaN and False for an action outside [0, N)"""
    R, N = p.shape
    ok = (actions >= 0) & (actions < N)
    q = p.double().gather(1, actions.clamp(0, N - 1).view(-1, 1))[:, 0]
    clamped = ((q < CAT_EPS) | (q > 1.0 - CAT_EPS)) & ok
    lp = torch.log(q.clamp(CAT_EPS, 1.0 - CAT_EPS))
    return torch.where(ok, lp, torch.full_like(lp, float("nan"))), clamped


def _pick_actions(p, gen, finite=None):
    """a random item of each row, the least likely (finite) one where the draw's probability is above 0.3: p <= 1/2 and |log p| >= 1/2
    then, so the quotient's rounding (u, absolute, in the logarithm) is at most one ulp of the result"""
    R, N = p.shape
    w = torch.ones(R, N, dtype=torch.float64) if finite is None else finite.double()
    a = torch.multinomial(w, 1, generator=gen)[:, 0]
    least = torch.where(w > 0, p, torch.full_like(p, INF)).argmin(1)
    return torch.where(p.gather(1, a.view(-1, 1))[:, 0] > 0.3, least, a)


def _not_borderline(p, actions):
    ok = (actions >= 0) & (actions < p.shape[1])
    q = p.gather(1, actions.clamp(0, p.shape[1] - 1).view(-1, 1))[:, 0][ok]
    assert bool(((q - CAT_EPS).abs() > 0.01 * CAT_EPS).all()) and bool(((q == 1.0) | (q < 1.0 - 100 * CAT_EPS)).all())


SOFTMAX_ROWS = ("randn3",) * 3 + ("+1000",) * 3 + ("-1000",) * 3 + ("range120", "clamped", "action=N", "action=-1")


@functools.lru_cache(maxsize=None)
def softmax_case(N):
    """the 13 rows of section 1 at width N: (fp32 logits [13, N], actions [13])"""
    g = _gen(1, N)
    z = torch.randn(3, N, generator=g) * 3.0
    wide = -120.0 * torch.rand(1, N, generator=g)
    wide[0, 0] = 0.0
    if N > 1:
        wide[0, N - 1] = -120.0
    low = z[:1].clone()
    x = torch.cat([z, z + 1000.0, z - 1000.0, wide, low, z[1:2], z[2:3]])
    p = softmax64(x)[2]
    a = _pick_actions(p, g)
    if N > 1:                                                 # p < eps on the chosen item: 40 below the row's largest logit
        a[10] = int(x[10].argmin())
        x[10, a[10]] = x[10].max() - 40.0
    a[11], a[12] = N, -1
    _not_borderline(softmax64(x)[2], a)
    return x, a


@functools.lru_cache(maxsize=None)
def masked_case(N):
    """section 2 at width N: a random third at -inf (rows 0-2), items 0..3 (row 3), items 4092..4095 (row 4), everything but the last
    item (row 5), row 0 again with a masked item as the action (row 6).  (logits [7, N], actions [7], names)"""
    g = _gen(2, N)
    z = torch.randn(7, N, generator=g) * 3.0
    mask = torch.zeros(7, N, dtype=torch.bool)
    mask[:3] = torch.rand(3, N, generator=g) < 1.0 / 3.0
    mask[torch.arange(3), torch.randint(0, N, (3,), generator=g)] = False          # one finite item at least
    names = ["third"] * 3 + ["plain", "plain", "last only", "masked action"]
    if N > 4:
        mask[3, :4] = True
        names[3] = "items 0..3"
    if N > 4096:
        mask[4, 4092:4096] = True
        names[4] = "items 4092..4095"
    mask[5, :N - 1] = True
    z[6], mask[6] = z[0], mask[0]
    x = z.masked_fill(mask, -INF)
    p = softmax64(x)[2]
    a = _pick_actions(p, g, finite=~mask)
    a[5] = N - 1
    if bool(mask[6].any()):
        a[6] = int(mask[6].nonzero()[0])
    _not_borderline(p, a)
    return x, a, tuple(names)


def unmask(x):
    """-inf logits replaced by the largest finite logit of their row (the mask removed)"""
    top = torch.where(torch.isinf(x), torch.full_like(x, -3e38), x).max(1, keepdim=True).values
    return torch.where(torch.isinf(x), top.expand_as(x), x)


def assert_probes(probes):
    """each (name, moved, bound): the reference moves by at least 100 bounds when the option is removed"""
    for name, moved, bound in probes:
        print(f"  probe {name}: reference moves by {moved:.3e} = {moved / bound:.3g} bounds")
        assert moved >= 100 * bound, (name, moved, bound)


def _moved(a, b, bound):
    """(largest |a - b| / bound, as moved and bound of the element where it is reached)"""
    r = (a - b).abs() / bound
    r = torch.where(torch.isnan(r), torch.full_like(r, INF), r)
    i = int(r.argmax())
    return float((a - b).abs().reshape(-1)[i]) if np.isfinite(float(r.reshape(-1)[i])) else INF, float(bound.reshape(-1)[i])


def softmax_probes(N):
    x, a = softmax_case(N)
    ref = categorical_bounds(x)
    out = []
    naive = torch.exp(x.double()) / torch.exp(x.double()).sum(1, keepdim=True)      # no max subtraction: inf / inf and 0 / 0
    for rows, name in ((slice(3, 6), "+1000"), (slice(6, 9), "-1000")):
        out.append((f"max subtraction, {name}", INF if not bool(torch.isfinite(naive[rows]).all()) else 0.0, 1.0))
    if N > 1:
        lp, clamped = logprob64(ref["p"], a)
        assert bool(clamped[10])
        free = float(torch.log(ref["p"][10, a[10]]))
        out.append(("clamp", abs(free - float(lp[10])), 4 * float(ulp32(lp[10:11]))))
    return out


def masked_probes(N):
    x, a, names = masked_case(N)
    ref = categorical_bounds(x)
    open_ = softmax64(unmask(x))[2]
    out = []
    for r in range(x.shape[0]):
        if bool(ref["masked"][r].any()):
            out.append((f"mask of row {r} ({names[r]})",) + _moved(open_[r], ref["p"][r], ref["bound"][r]))
    return out


# ---------------------------------------------------------------------------------------------------- the two backwards
def logprob_bwd64(p, actions, g, sum_p, clamped, old=None):
    """g (onehot(a) - p / sum p), zero for clamped rows and for g = None, plus `old` when accumulating; (result, bound).
    The kernel rounds 1 / sum p, -g times it and the product with p (3 u of |g p / sum p|), then the sum with g at the action's
    column and the sum with `old` (u of each result)."""
    R, N = p.shape
    gv = torch.zeros(R, dtype=torch.float64) if g is None else g.double()
    gv = torch.where(clamped, torch.zeros_like(gv), gv)[:, None]
    t = gv * p.double() / sum_p.double()[:, None]
    hit = torch.zeros(R, N, dtype=torch.float64)
    hit[torch.arange(R), actions] = 1.0
    o = hit * gv - t
    bound = U * (3 * t.abs() + hit * o.abs())
    if old is not None:
        o = o + old.double()
        bound = bound + U * o.abs()
    return o, bound + TINY


def softmax_bwd64(p, dp):
    """p (dp - sum_j p_j dp_j); (result, bound).  The dot: a product and ceil(N / 1024) adds per thread, 6 + 16 over the workgroup, each
    within u of sum |p dp|; then a subtraction and a product, u of the result each."""
    p, dp = p.double(), dp.double()
    N = p.shape[1]
    dot = (p * dp).sum(1, keepdim=True)
    dot_err = U * (-(-N // PT) + 1 + 22) * (p * dp).abs().sum(1, keepdim=True)
    o = p * (dp - dot)
    return o, p * dot_err + 2 * U * o.abs() + TINY


def shard_logprob_bwd64(p, local, g):
    """-g p, plus g at the row's action where 0 <= local < n; (result, bound): a product and, at that column, an addition"""
    R, n = p.shape
    own = (local >= 0) & (local < n)
    hit = torch.zeros(R, n, dtype=torch.float64)
    hit[torch.arange(R)[own], local[own]] = 1.0
    t = g.double()[:, None] * p.double()
    o = hit * g.double()[:, None] - t
    return o, U * (t.abs() + hit * o.abs()) + TINY


@functools.lru_cache(maxsize=None)
def logprob_bwd_case(R, N):
    """fp32 probabilities (unnormalised: each row times a factor in [0.5, 2]), actions in the last real column and in every lane of the
    ragged last float4, g, rowstat (sum p; clamped on every fifth row), an `old` output that bf16 holds exactly"""
    gen = _gen(3, R, N)
    scale = 0.5 + 1.5 * torch.rand(R, 1, generator=gen, dtype=torch.float64)
    p = (torch.softmax(torch.randn(R, N, generator=gen, dtype=torch.float64) * 2.0, 1) * scale).float()
    a = torch.randint(0, N, (R,), generator=gen)
    for r in range(min(R, 5)):
        a[r] = max(0, N - 1 - (r % 4)) if r < 4 else (N - 1) // 4 * 4
    g = torch.randn(R, generator=gen)
    stat = torch.zeros(R, 4)
    stat[:, 2] = p.double().sum(1).float()
    stat[4::5, 3] = 1.0
    old = torch.randn(R, N, generator=gen).to(torch.bfloat16).float()
    return dict(p=p, actions=a, g=g, stat=stat, old=old)


def logprob_bwd_probes(R, N):
    c = logprob_bwd_case(R, N)
    sp, cl = c["stat"][:, 2], c["stat"][:, 3] != 0
    full, b = logprob_bwd64(c["p"], c["actions"], c["g"], sp, cl)
    acc, b_acc = logprob_bwd64(c["p"], c["actions"], c["g"], sp, cl, c["old"])
    flat = torch.zeros(R, dtype=torch.float64)
    out = [("accumulate",) + _moved(full, acc, b_acc),
           ("1 / sum p",) + _moved(logprob_bwd64(c["p"], c["actions"], c["g"], flat + 1.0, cl)[0], full, b)]
    if N > 1:                              # (one item: p / sum p = 1 on the action's column, the gradient is zero whatever g is)
        out.append(("g",) + _moved(logprob_bwd64(c["p"], c["actions"], None, sp, cl)[0], full, b))
        out.append(("the action's column",) + _moved(logprob_bwd64(c["p"], (c["actions"] + 1) % N, c["g"], sp, cl)[0], full, b))
    if bool(cl.any()) and N > 1:
        out.append(("clamped rows",) + _moved(logprob_bwd64(c["p"], c["actions"], c["g"], sp, cl & False)[0], full, b))
    return out


@functools.lru_cache(maxsize=None)
def softmax_bwd_case(N, R=3):
    """fp32 probabilities and a dp whose entry (r, (7 r) % N) is 1e4 times the rest"""
    gen = _gen(4, N)
    p = torch.softmax(torch.randn(R, N, generator=gen, dtype=torch.float64) * 2.0, 1).float()
    dp = torch.randn(R, N, generator=gen)
    for r in range(R):
        dp[r, (7 * r) % N] = 1e4 * (1.0 + r)
    return p, dp


def softmax_bwd_probes(N):
    p, dp = softmax_bwd_case(N)
    o, b = softmax_bwd64(p, dp)
    return [("the dot",) + _moved(p.double() * dp.double(), o, b)]


# ---------------------------------------------------------------------------------------------------- sharded softmax
SHARD_NS = (1025, 4100, 8195)


def shard_cuts(N, parts):
    """column ranges of `parts` shards of unequal width whose inner cuts are odd (inside a float4)"""
    cuts = [0, (N // 3) | 1, N] if parts == 2 else [0, (N // 5) | 1, (7 * N // 10) | 1, N]
    assert all(c % 4 for c in cuts[1:-1]) and len(set(np.diff(cuts).tolist())) == parts
    return list(zip(cuts[:-1], cuts[1:]))


@functools.lru_cache(maxsize=None)
def shard_case(N, parts):
    """rows: randn * 3, + 1000, range 120, a third masked, the first shard at -inf throughout, the last shard at -inf throughout;
    actions on the first and last column of shards"""
    sx, _ = softmax_case(N)
    mx, _, _ = masked_case(N)
    cuts = shard_cuts(N, parts)
    x = torch.cat([sx[0:1], sx[3:4], sx[9:10], mx[0:1], sx[1:2], sx[2:3]]).clone()
    x[3, N - 1] = 0.5                      # (row 3's action: not a masked item)
    x[4, cuts[0][0]:cuts[0][1]] = -INF
    x[5, cuts[-1][0]:cuts[-1][1]] = -INF
    a = torch.tensor([0, cuts[0][1] - 1, cuts[1][0], N - 1, cuts[1][1] - 1, cuts[-1][0]])
    return x, a, cuts


def shard_bounds(x, cuts):
    """pass 1 stores fl(expf(fl(x - max))), pass 2 divides by the sum: 2 + 1 roundings beside the argument's.  The sum: terms of one
    exponential each, (v.x + v.y) + (v.z + v.w), one add per group of the widest shard, 6 + 16 over the workgroup, one per further
    shard on the host."""
    k = max(groups(hi - lo) for lo, hi in cuts)
    return softmax_bounds(x, 3, 2 + 2 + k + 22 + len(cuts) - 1, 0)


def shard_softmax64(x, cuts):
    """the three passes in float64 with the two all-reduces between them; equals softmax64(x)[2]"""
    x = x.double()
    m = torch.stack([x[:, lo:hi].max(1).values for lo, hi in cuts]).max(0).values
    e = [torch.exp(x[:, lo:hi] - m[:, None]) for lo, hi in cuts]
    s = torch.stack([t.sum(1) for t in e]).sum(0)
    return torch.cat([t / s[:, None] for t in e], 1)


def shard_probes(N, parts):
    x, a, cuts = shard_case(N, parts)
    ref = shard_bounds(x, cuts)
    lo, hi = cuts[0]
    alone = x.clone()                      # without the all-reduces the first shard is a softmax of its own
    alone[:, hi:] = -INF
    p_alone = softmax64(alone[:4])[2]
    return [("the all-reduces",) + _moved(p_alone[:, lo:hi], ref["p"][:4, lo:hi], ref["bound"][:4, lo:hi])]


@functools.lru_cache(maxsize=None)
def shard_bwd_case(R, n):
    """a shard's probabilities (padding zero, like pass 2 leaves it), local action indices inside, below and above the shard, g"""
    gen = _gen(5, R, n)
    p = (torch.softmax(torch.randn(R, n, generator=gen, dtype=torch.float64) * 2.0, 1) * 0.4).float()
    local = torch.randint(-n, 2 * n, (R,), generator=gen)
    local[0], local[1], local[R - 1], local[256] = 0, n - 1, n - 1, (n - 1) // 4 * 4
    return p, local, torch.randn(R, generator=gen)


def shard_bwd_probes(R, n):
    p, local, g = shard_bwd_case(R, n)
    o, b = shard_logprob_bwd64(p, local, g)
    rolled = shard_logprob_bwd64(p, local, g.roll(256))[0]          # a row loop that strides wrongly reads another row's g
    return [("g of the row",) + _moved(rolled, o, b), ("the owned action",) + _moved(shard_logprob_bwd64(p, local * 0 - 1, g)[0], o, b)]


# ---------------------------------------------------------------------------------------------------- the sampler
SAMPLER_NS = (5, 4097, 8195)
SAMPLER_TOTAL = 4096
SAMPLER_KEYS = ((7, 3), (123456789, 40))            # (seed, step)


def thread_major_order(n):
    """the item order of the sampler's inverse CDF: thread t of 1024 owns items 4 (t + 1024 k) + c, k = 0, 1, ..., c = 0..3, and the
    threads follow each other; a permutation of range(n)"""
    item = np.arange(n)
    group = item // 4
    return np.lexsort((item % 4, group // PT, group % PT))


def interval_lookup(weights, targets):
    """weights: non-negative integers [n]; targets: integers in [0, sum).  The item whose interval of the thread-major cumulative sum
    holds each target (an item of weight zero has an empty interval)"""
    order = thread_major_order(len(weights))
    cum = np.cumsum(np.asarray(weights, dtype=np.int64)[order])
    return order[np.searchsorted(cum, np.asarray(targets, dtype=np.int64), side="right")]


@functools.lru_cache(maxsize=None)
def sampler_weights(n):
    """integer weights summing to 4096 with zeros, weight on item 0, on item n - 1 and (where they exist) on items 4096..4099 and
    8192.., the second and third float4 group of thread 0"""
    w = np.zeros(n, dtype=np.int64)
    if n == 5:
        w[:] = (1000, 0, 2000, 0, 1096)
        return w
    special = {0: 300, 3: 1, 4: 7, 4095: 200, 4096: 150, n - 1: 90}
    if n > 4100:
        special.update({4097: 50, 4099: 70, 8192: 60, 8188: 33, 2044: 21})
    for i, v in special.items():
        w[i] = v
    rng = np.random.default_rng(n)
    others = rng.choice(np.setdiff1d(np.arange(n), np.fromiter(special, dtype=np.int64)), 150, replace=False)
    w[others] = rng.multinomial(SAMPLER_TOTAL - int(w.sum()), np.full(150, 1.0 / 150))
    assert int(w.sum()) == SAMPLER_TOTAL and int((w == 0).sum()) > n // 2
    return w


def sampler_probes(n):
    """the thread-major order matters: read in index order the same targets give other items for at least a tenth of them"""
    w = sampler_weights(n)
    t = np.arange(SAMPLER_TOTAL)
    plain = np.searchsorted(np.cumsum(w), t, side="right")
    differ = int((plain != interval_lookup(w, t)).sum())
    return [] if n <= 4 * PT else [("thread-major order (targets that land elsewhere)", float(differ), 1.0)]      # identity up to 4096


@functools.lru_cache(maxsize=None)
def masked_sampling_case(n=4100, bins=64):
    """one logit row with a third at -inf, its float64 probabilities summed over `bins` contiguous-index bins"""
    gen = _gen(6, n)
    x = torch.randn(n, generator=gen) * 1.5
    mask = torch.rand(n, generator=gen) < 1.0 / 3.0
    x = x.masked_fill(mask, -INF)
    p = softmax64(x[None])[2][0]
    which = torch.arange(n) * bins // n
    return x, mask, which, torch.zeros(bins, dtype=torch.float64).index_add_(0, which, p)


def digest(tensors):
    """sha256 over the bytes of the tensors in order"""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()
