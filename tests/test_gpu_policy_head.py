"""The eleven kernels of csrc/policy.hip, called through the C ABI and held to the float64 references of tests/policy_head_reference.py
element by element: the softmax / log-prob / sampling head (`recnn_categorical_rows`), `recnn_logprob_bwd` with its column sums, its
accumulate flag and its bf16 output, `recnn_softmax_bwd`, `recnn_colsum_rows`, `recnn_onehot_rows`, the three sharded-softmax passes
and `recnn_shard_logprob_bwd`.

Every bound is a count of the kernel's roundings times 2^-24 taken from the reference alone (derivations in policy_head_reference);
every comparison prints its worst error / bound before it asserts; where a case exists for an option the reference is probed first:
without the option it must move by at least 100 bounds (tests/test_policy_head_cpu.py runs the same probes without a GPU).

Every output has a pitch wider than round4(N) and one row more than it needs, prefilled with a NaN sentinel: columns [N, round4(N))
must be exact zeros, everything beyond keeps the sentinel.  Input padding holds NaN where the kernel's contract says it does not
matter, 7.0 where `logprob_bwd` loads whole float4s of p, and the zeros pass 2 leaves where `shard_logprob_bwd` multiplies them.

A row's workgroup is 1024 threads x 4 floats, the backward kernels take 256 float4s per workgroup and 32 rows per slab: N runs over
1, 3, 4, 5, 1021, 1024, 1025, 4095, 4096, 4097, 4100, 8195 and the slabbed kernels over 1, 31, 32, 33, 65 rows.

-inf logits are masked items: exact zero probability, never sampled.  (Before the fix of the online max / sum loop a thread whose
first float4 was four -inf logits and which met a finite one later -- N > 4096 -- turned the whole row into NaN.)"""
import math

import numpy as np
import pytest
import torch

import policy_head_reference as P

pytestmark = pytest.mark.gpu

SENT32 = 0x7FC05A5A         # a NaN fp32 pattern
SENT16 = 0x7FC1             # a NaN bf16 pattern
ACT_SENT = -0x5A5A5A5A5A


def _lib():
    from recnn_amd import _lib as L
    L.load()
    return L


def _sentinel(rows, ld, bf16=False):
    if bf16:
        return torch.full((rows, ld), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return torch.full((rows, ld), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)


def _place(x, ld, pad=None):
    """[R, N] -> [R + 1, ld] on the device: x inside, `pad` (default: the sentinel) in the padding columns, the sentinel in the last row"""
    R, N = x.shape
    buf = _sentinel(R + 1, ld)
    buf[:R, :N] = x.to("cuda")
    if pad is not None:
        buf[:R, N:] = pad
    return buf


def _kept(buf, R, W, what):
    """the sentinel still stands everywhere outside [R, W]"""
    bits = buf.view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32).clone()
    sent = SENT16 if buf.dtype == torch.bfloat16 else SENT32
    bits[:R, :W] = sent
    bad = (bits != sent).nonzero()
    assert bad.numel() == 0, (what, "written outside", (R, W), "at", bad[:4].tolist())


def _zero_pad(buf, R, N, what):
    """columns [N, round4(N)) are exact zeros, the rest outside [R, round4(N)) is the sentinel"""
    assert not (buf[:R, N:P.round4(N)] != 0).any(), (what, "padding columns are not zero")
    _kept(buf, R, P.round4(N), what)


def _check(what, got, want, bound):
    err = (got.double() - want).abs()
    ratio = err / bound
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    i = int(ratio.argmax())
    worst = float(ratio.reshape(-1)[i])
    print(f"{what}: worst error / bound = {worst:.3f} (error {float(err.reshape(-1)[i]):.3e}, bound {float(bound.reshape(-1)[i]):.3e}, "
          f"reference {float(want.reshape(-1)[i]):.3e}, element {i})")
    assert worst <= 1.0, (what, worst)
    return worst


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---------------------------------------------------------------------------------------------------- recnn_categorical_rows
def _categorical(x, flags, actions=None, seed=1, step=1, what="", nan_row=None):
    """x: [R, N] on either side.  -> dict(p, lp, stat, act) on the CPU (p: rows 0 and R - 1 only when x came from the device).
    nan_row: a row of -inf throughout, whose result (padding columns included) is NaN and is not looked at"""
    L = _lib()
    R, N = x.shape
    ld = P.round4(N) + 8
    buf = _place(x, ld)
    act = torch.full((R + 1,), ACT_SENT, dtype=torch.int64, device="cuda")
    if actions is not None:
        act[:R] = actions.to("cuda")
    lp, stat = _sentinel(1, R + 1)[0], _sentinel(R + 1, 4)
    L.call("recnn_categorical_rows", L.ptr(buf), ld, R, N, flags, seed, step, L.ptr(act), L.ptr(lp), L.ptr(stat), L.current_stream())
    torch.cuda.synchronize()
    if nan_row is not None:
        buf[nan_row, :P.round4(N)] = 0.0
    if flags & L.CAT_SOFTMAX:
        _zero_pad(buf, R, N, what)
    else:                                                                      # given probabilities are left untouched
        _kept(buf, R, N, what)
        assert torch.equal(_bits(buf[:R, :N]), _bits(x.to("cuda"))), (what, "the probabilities were written to")
    assert int(act[R]) == ACT_SENT and int(_bits(lp)[R]) == SENT32 and bool((_bits(stat[R]) == SENT32).all()), (what, "row R written")
    rows = slice(0, R) if not x.is_cuda else [0, R - 1]
    return dict(p=buf[rows, :N].cpu(), lp=lp[:R].cpu(), stat=stat[:R].cpu(), act=act[:R].cpu())


def _check_logprob(what, lp, p_at, sum_p, clamped_got, ref_p_at, ref_err, in_range):
    """lp against the logarithm of the kernel's own stored quotient (4 ulp of the result: logf is good to 3, the quotient's rounding is
    one more where |lp| >= 1/2), and against the float64 reference, whose probability and sum carry their own bounds (relative:
    absolute in the logarithm).  Out of range: NaN, written (not the sentinel), clamped = 0."""
    ok = in_range
    assert bool(torch.isnan(lp[~ok]).all()) and not (_bits(lp[~ok]) == SENT32).any() and not clamped_got[~ok].any(), what
    q = (p_at.double() / sum_p.double())[ok]
    own = torch.log(q.clamp(P.CAT_EPS, 1.0 - P.CAT_EPS))
    ulps = (lp[ok].double() - own).abs() / P.ulp32(own)
    print(f"{what}: logprob within {float(ulps.max()):.2f} ulp of log(stored p / stored sum) (bound 4)")
    assert float(ulps.max()) <= 4.0, (what, ulps)
    want_cl = (ref_p_at < P.CAT_EPS) | (ref_p_at > 1.0 - P.CAT_EPS)
    assert torch.equal(clamped_got[ok] != 0, want_cl[ok]), (what, "clamped flag")
    want = torch.log(ref_p_at.clamp(P.CAT_EPS, 1.0 - P.CAT_EPS))[ok]
    bound = 4 * P.ulp32(want) + torch.where(want_cl[ok], torch.zeros_like(want), ref_err[ok])
    return _check(what + " logprob", lp[ok], want, bound)


def _check_softmax_rows(what, out, x, actions):
    """p, max, sum exp, sum p, clamped and logprob of `out` against the float64 softmax of x"""
    ref = P.categorical_bounds(x)
    N = x.shape[1]
    _check(what + " p", out["p"], ref["p"], ref["bound"])
    assert not out["p"][ref["masked"]].any(), (what, "a masked item has a non-zero probability")
    stat = out["stat"]
    assert torch.equal(stat[:, 0].double(), ref["max"]), (what, "row max")
    _check(what + " sum exp", stat[:, 1], ref["den"], ref["rel_den"] * ref["den"])
    _check(what + " sum p", stat[:, 2], ref["p"].sum(1), ref["sum_bound"])
    ok = (actions >= 0) & (actions < N)
    ac = actions.clamp(0, N - 1).view(-1, 1)
    rel_at = ref["rel"].gather(1, ac)[:, 0] + ref["sum_bound"]
    _check_logprob(what, out["lp"], out["p"].gather(1, ac)[:, 0], stat[:, 2], stat[:, 3], ref["p"].gather(1, ac)[:, 0], rel_at, ok)


@pytest.fixture(scope="module")
def softmax_runs(cuda):
    """section 1's 13 rows at every N through CAT_SOFTMAX with the actions given, run once and shared"""
    L = _lib()
    return {N: _categorical(P.softmax_case(N)[0], L.CAT_SOFTMAX, P.softmax_case(N)[1], what=f"softmax N={N}") for N in P.NS}


@pytest.mark.parametrize("N", P.NS)
def test_softmax_and_logprob_against_float64(cuda, softmax_runs, N):
    """randn * 3, the same + 1000 and - 1000, a row of range 120 (probabilities down to 1e-45: zero or within the floor), a row clamped
    at p < eps (at N = 1 every row is clamped at p > 1 - eps), actions N and -1."""
    x, a = P.softmax_case(N)
    P.assert_probes(P.softmax_probes(N))
    out = softmax_runs[N]
    _check_softmax_rows(f"softmax N={N}", out, x, a)
    assert bool(torch.isfinite(out["p"]).all()) and bool((out["stat"][:, 3] != 0)[10])
    assert torch.equal(out["act"], a)                                          # given actions are not written to


def test_digest_of_the_finite_rows(cuda, softmax_runs):
    """prints one sha256 over p, logprob and rowstat of section 1 at every N: rows without -inf keep their bits across builds"""
    d = P.digest([t for N in P.NS for t in (softmax_runs[N]["p"], softmax_runs[N]["lp"], softmax_runs[N]["stat"])])
    print(f"policy head, finite rows: sha256 {d}")
    assert len(d) == 64


@pytest.mark.parametrize("N", P.NS)
def test_masked_logits_against_float64(cuda, N):
    """-inf logits: exact zeros there, section 1's bounds elsewhere.  A third of a row at random; items 0..3, and 4092..4095, whose
    thread meets finite logits only in a later float4 group (N > 4096); a row whose only finite logit is the last item; a masked
    item as the action (clamped, log eps)."""
    L = _lib()
    x, a, names = P.masked_case(N)
    P.assert_probes(P.masked_probes(N))
    out = _categorical(x, L.CAT_SOFTMAX, a, what=f"masked N={N}")
    for r, name in enumerate(names):                                           # name the rows a NaN took before comparing
        assert bool(torch.isfinite(out["p"][r]).all()), (f"N={N} row {r} ({name})", "non-finite probabilities",
                                                          int(torch.isnan(out["p"][r]).sum()), "NaN of", N)
    _check_softmax_rows(f"masked N={N}", out, x, a)
    assert float(out["p"][5, N - 1]) == 1.0 and bool(out["stat"][5, 3] != 0)


@pytest.mark.parametrize("N", (5, 4097, 8195))
def test_a_row_of_minus_inf_leaves_the_other_rows_their_bits(cuda, N):
    """a row that is -inf throughout is NaN in torch too; nothing is asserted of it"""
    L = _lib()
    x, a, _ = P.masked_case(N)
    alone = _categorical(x, L.CAT_SOFTMAX, a, what=f"N={N}")
    x2 = torch.cat([x[:3], torch.full((1, N), -P.INF), x[3:]])
    a2 = torch.cat([a[:3], a[:1], a[3:]])
    both = _categorical(x2, L.CAT_SOFTMAX, a2, what=f"N={N} with a row of -inf", nan_row=3)
    keep = [0, 1, 2, 4, 5, 6, 7]
    for k in ("p", "lp", "stat"):
        assert torch.equal(_bits(both[k][keep]), _bits(alone[k])), (N, k)


# ---------------------------------------------------------------------------------------------------- recnn_logprob_bwd
def _logprob_bwd(c, flags, with_g=True, old=None, what=""):
    """-> (d [R, N] fp32 or bf16, column sums [N]) on the CPU"""
    L = _lib()
    R, N = c["p"].shape
    n4r, slabs = P.round4(N), (R + 31) // 32
    bf16 = bool(flags & L.LPB_BF16)
    ldp, ldd = n4r + 4, n4r + 8
    p = _place(c["p"], ldp, pad=7.0)                                           # whole float4s of p are loaded
    d = _sentinel(R + 1, ldd, bf16)
    if old is not None:
        d[:R, :N] = old.to("cuda").to(d.dtype)
    cs, scratch = _sentinel(1, n4r + 8), _sentinel(slabs + 1, n4r)
    g = c["g"].to("cuda") if with_g else None
    a, stat = c["actions"].to("cuda"), c["stat"].to("cuda")                  # (named: they must outlive the launch)
    L.call("recnn_logprob_bwd", L.ptr(p), ldp, R, N, L.ptr(a), L.ptr(g), L.ptr(stat), L.ptr(d), ldd, flags, L.ptr(cs), L.ptr(scratch),
           L.current_stream())
    torch.cuda.synchronize()
    _zero_pad(d, R, N, what)
    _kept(cs, 1, N, what + " colsum")
    _kept(scratch, slabs, n4r, what + " scratch")
    return d[:R, :N].cpu(), cs[0, :N].cpu()


def _check_colsum(what, cs, d, R):
    """the column sums equal the sum of the stored fp32 d: 32 row-ordered adds per slab, one add per slab"""
    total = d.double().sum(0)
    return _check(what + " colsum", cs, total, P.U * (32 + (R + 31) // 32) * d.double().abs().sum(0) + P.TINY)


@pytest.mark.parametrize("N", P.NS)
def test_logprob_bwd_against_float64(cuda, N):
    L = _lib()
    worst = 0.0
    for R in P.ROWS:
        c = P.logprob_bwd_case(R, N)
        P.assert_probes(P.logprob_bwd_probes(R, N))
        sp, cl = c["stat"][:, 2], c["stat"][:, 3] != 0
        what = f"logprob_bwd R={R} N={N}"
        runs = {}
        for name, flags, with_g, old in (("plain", 0, True, None), ("accumulate", L.LPB_ACCUMULATE, True, c["old"]),
                                         ("g=NULL", 0, False, None), ("g=NULL accumulate", L.LPB_ACCUMULATE, False, c["old"])):
            d, cs = _logprob_bwd(c, flags, with_g, old, what=f"{what} {name}")
            want, bound = P.logprob_bwd64(c["p"], c["actions"], c["g"] if with_g else None, sp, cl, old)
            worst = max(worst, _check(f"{what} {name}", d, want, bound), _check_colsum(f"{what} {name}", cs, d, R))
            assert not d[cl].any() or old is not None                          # clamped rows: exact zeros
            runs[name] = (d, cs)
        assert not runs["g=NULL"][0].any()
        # bf16 output: the fp32 result rounded to nearest even, the column sums taken before the rounding
        for name, flags, old in (("plain", L.LPB_BF16, None), ("accumulate", L.LPB_BF16 | L.LPB_ACCUMULATE, c["old"])):
            d16, cs16 = _logprob_bwd(c, flags, True, old, what=f"{what} bf16 {name}")
            d32, cs32 = runs[name]
            assert d16.dtype == torch.bfloat16 and torch.equal(_bits(d16), _bits(d32.to(torch.bfloat16))), (what, name, "bf16 output")
            assert torch.equal(_bits(cs16), _bits(cs32)), (what, name, "column sums of the bf16 mode")
    print(f"logprob_bwd N={N}: worst error / bound over rows {P.ROWS} = {worst:.3f}")


def test_logprob_bwd_without_column_sums(cuda):
    """colsum = NULL: no scratch needed, the same bits in d"""
    L = _lib()
    c = P.logprob_bwd_case(33, 1025)
    d, _ = _logprob_bwd(c, 0, what="with column sums")
    n4r = P.round4(1025)
    p, out = _place(c["p"], n4r + 4, pad=7.0), _sentinel(34, n4r + 8)
    a, g, stat = c["actions"].to("cuda"), c["g"].to("cuda"), c["stat"].to("cuda")
    L.call("recnn_logprob_bwd", L.ptr(p), n4r + 4, 33, 1025, L.ptr(a), L.ptr(g), L.ptr(stat), L.ptr(out), n4r + 8, 0, None, None,
           L.current_stream())
    torch.cuda.synchronize()
    _zero_pad(out, 33, 1025, "no column sums")
    assert torch.equal(_bits(out[:33, :1025].cpu()), _bits(d))


# ---------------------------------------------------------------------------------------------------- recnn_softmax_bwd
@pytest.mark.parametrize("N", P.NS)
def test_softmax_bwd_against_float64(cuda, N):
    """p and dp at odd pitches from addresses that are not 16-byte aligned (the kernel is scalar), one dp entry 1e4 times the rest"""
    L = _lib()
    p, dp = P.softmax_bwd_case(N)
    P.assert_probes(P.softmax_bwd_probes(N))
    R = p.shape[0]
    ldp = N + 3 if N % 2 == 0 else N + 4
    lddp, ldd = ldp + 2, P.round4(N) + 5
    assert ldp % 2 and lddp % 2
    views = []
    for t, ld in ((p, ldp), (dp, lddp)):
        flat = _sentinel(1, R * ld + 1)[0]
        v = flat[1:].view(R, ld)                                               # one float past the allocation's alignment
        v[:, :N] = t.to("cuda")
        assert v.data_ptr() % 16 == 4
        views.append(v)
    d = _sentinel(R + 1, ldd)
    L.call("recnn_softmax_bwd", L.ptr(views[0]), ldp, R, N, L.ptr(views[1]), lddp, L.ptr(d), ldd, L.current_stream())
    torch.cuda.synchronize()
    _zero_pad(d, R, N, f"softmax_bwd N={N}")
    want, bound = P.softmax_bwd64(p, dp)
    _check(f"softmax_bwd N={N}", d[:R, :N].cpu(), want, bound)


# ---------------------------------------------------------------------------------------------------- colsum_rows, onehot_rows
@pytest.mark.parametrize("N", P.NS)
def test_colsum_rows_is_exact_on_integers(cuda, N):
    L = _lib()
    for R in (0, 1, 33):
        x = torch.randint(-8, 9, (R, N), generator=torch.Generator().manual_seed(N + R)).float()
        ld = P.round4(N) + 4
        buf = _place(x, ld)                                                    # NaN in the padding: loaded, never stored
        out = _sentinel(1, P.round4(N) + 8)
        L.call("recnn_colsum_rows", L.ptr(buf), ld, R, N, L.ptr(out), L.current_stream())
        torch.cuda.synchronize()
        _kept(out, 1, N, f"colsum_rows R={R} N={N}")
        assert torch.equal(out[0, :N].cpu(), x.sum(0)), (R, N)
        _kept(buf, R, N, "colsum_rows input")


def test_onehot_rows_past_the_grid_limit(cuda):
    """65 537 rows: the grid's row dimension stops at 65 535 and the kernel strides; ids 0, n - 1; out of range: an all-zero row"""
    L = _lib()
    R, n, ld = 65537, 5, 8
    ids = torch.randint(0, n, (R,), generator=torch.Generator().manual_seed(3))
    ids[:6] = torch.tensor([0, n - 1, -1, n, 7, 2 ** 40])
    ids[65534:] = torch.tensor([n - 1, 0, n - 1])
    out, dev_ids = _sentinel(R + 1, ld), ids.to("cuda")
    L.call("recnn_onehot_rows", L.ptr(dev_ids), R, n, L.ptr(out), ld, L.current_stream())
    torch.cuda.synchronize()
    want = torch.zeros(R, ld)
    ok = (ids >= 0) & (ids < n)
    want[torch.arange(R)[ok], ids[ok]] = 1.0
    assert not want[2:6].any() and torch.equal(out[:R].cpu(), want)
    _kept(out, R, ld, "onehot")


@pytest.mark.parametrize("n", (1, 4, 1021, 1025))
def test_onehot_rows_widths(cuda, n):
    L = _lib()
    ld = P.round4(n) + 4
    ids = torch.tensor([0, n - 1, n // 2, n, -1])
    out, dev_ids = _sentinel(6, ld), ids.to("cuda")
    L.call("recnn_onehot_rows", L.ptr(dev_ids), 5, n, L.ptr(out), ld, L.current_stream())
    torch.cuda.synchronize()
    want = torch.zeros(5, ld)
    want[torch.arange(3), ids[:3]] = 1.0
    assert torch.equal(out[:5].cpu(), want)
    _kept(out, 5, ld, "onehot")


# ---------------------------------------------------------------------------------------------------- the sharded passes
@pytest.mark.parametrize("parts", (2, 3))
@pytest.mark.parametrize("N", P.SHARD_NS)
def test_sharded_softmax_passes_against_float64(cuda, N, parts):
    """passes 0 / 1 / 2 per column shard (unequal widths, cuts inside a float4), the max and sum all-reduces done here in torch; rows
    with a shard at -inf throughout; `pa` on the owning shard alone, actions on the first and last column of shards"""
    L = _lib()
    x, a, cuts = P.shard_case(N, parts)
    P.assert_probes(P.shard_probes(N, parts))
    R = x.shape[0]
    ref = P.shard_bounds(x, cuts)
    bufs = [_place(x[:, lo:hi], P.round4(hi - lo) + 8) for lo, hi in cuts]
    stream = L.current_stream()

    def one_pass(which, rowval_in=None):
        outs = []
        for (lo, hi), buf in zip(cuts, bufs):
            res = _sentinel(1, R + 1)[0]
            local = (a - lo).to("cuda")
            rowval = res if which == 0 else rowval_in
            L.call("recnn_shard_softmax_pass", L.ptr(buf), buf.shape[1], R, hi - lo, which, L.ptr(rowval), L.ptr(local) if which == 2 else None,
                   None if which == 0 else L.ptr(res), stream)
            torch.cuda.synchronize()
            assert int(_bits(res)[R]) == SENT32
            outs.append(res[:R].clone())
        return torch.stack(outs)

    m = one_pass(0)
    for (lo, hi), buf, got in zip(cuts, bufs, m.cpu()):
        assert torch.equal(got, x[:, lo:hi].max(1).values)                      # exact, -inf for a shard at -inf throughout
        _kept(buf, R, hi - lo, "pass 0 writes nothing")
    assert bool(torch.isinf(m[0, 4])) and bool(torch.isinf(m[-1, 5]))
    s = one_pass(1, m.max(0).values.contiguous())
    pa = one_pass(2, s.sum(0).contiguous()).cpu()
    for (lo, hi), buf in zip(cuts, bufs):
        _zero_pad(buf, R, hi - lo, f"shard [{lo}, {hi})")
    p = torch.cat([buf[:R, :hi - lo] for (lo, hi), buf in zip(cuts, bufs)], 1).cpu()
    _check(f"sharded softmax N={N} parts={parts} p", p, ref["p"], ref["bound"])
    assert not p[ref["masked"]].any()
    _check(f"sharded softmax N={N} parts={parts} sum exp", s.sum(0).cpu(), ref["den"], ref["rel_den"] * ref["den"])
    owner = torch.tensor([[lo <= int(v) < hi for v in a] for lo, hi in cuts])
    assert bool((owner.sum(0) == 1).all())
    assert not pa[~owner].any(), "pa is non-zero on a shard that does not own the action"
    stored = p.gather(1, a.view(-1, 1))[:, 0]
    assert torch.equal(_bits(pa.sum(0)), _bits(stored)) and bool((stored[[0, 1, 3, 4]] > 0).all()) and float(stored[5]) == 0.0


@pytest.mark.parametrize("R", (257, 300))
def test_shard_logprob_bwd_against_float64(cuda, R):
    """its row loop strides by 256: rows 256.. are the second trip"""
    L = _lib()
    n = 1025
    p, local, g = P.shard_bwd_case(R, n)
    P.assert_probes(P.shard_bwd_probes(R, n))
    ldp, ldd = P.round4(n) + 4, P.round4(n) + 8
    pb = _place(p, ldp)
    pb[:R, n:P.round4(n)] = 0.0                                                 # what pass 2 leaves there; the kernel multiplies it
    d, dev_local, dev_g = _sentinel(R + 1, ldd), local.to("cuda"), g.to("cuda")
    L.call("recnn_shard_logprob_bwd", L.ptr(pb), ldp, R, n, L.ptr(dev_local), L.ptr(dev_g), L.ptr(d), ldd, L.current_stream())
    torch.cuda.synchronize()
    _zero_pad(d, R, n, f"shard_logprob_bwd R={R}")
    want, bound = P.shard_logprob_bwd64(p, local, g)
    _check(f"shard_logprob_bwd R={R}", d[:R, :n].cpu(), want, bound)


# ---------------------------------------------------------------------------------------------------- the sampler
def test_sampler_draws_the_item_of_the_interval_exactly(cuda):
    """Integer weights summing to 4096 make every partial sum, the wave scan and u * sum p exact in fp32.  All weights 1 at N = 4096
    calibrates: thread-major order is the identity there, the draw is floor(4096 u_row).  With the same seed, step and rows every
    other distribution must draw, with zero tolerance, the item whose interval of the thread-major cumulative sum holds that
    number: the lane scan over 64 x 16 partials, the owning lane's walk and the owning thread's walk over its float4 groups."""
    L = _lib()
    R = 2048
    seen = []
    for seed, step in P.SAMPLER_KEYS:
        ones = torch.ones(R, 4096, device="cuda")
        cal = _categorical(ones, L.CAT_SAMPLE, seed=seed, step=step, what="calibration")
        target = cal["act"].numpy()
        assert target.min() >= 0 and target.max() < 4096 and len(np.unique(target)) > 1400          # ~1611 of 2048 uniform draws
        assert torch.equal(cal["act"], _categorical(ones, L.CAT_SAMPLE, seed=seed, step=step)["act"])
        _check_logprob("calibration", cal["lp"], torch.ones(R), cal["stat"][:, 2], cal["stat"][:, 3], torch.full((R,), 1.0 / 4096, dtype=torch.float64),
                       torch.zeros(R, dtype=torch.float64), torch.ones(R, dtype=torch.bool))
        seen.append(target)
        for N in P.SAMPLER_NS:
            P.assert_probes(P.sampler_probes(N))
            w = P.sampler_weights(N)
            rows = torch.from_numpy(w).float().to("cuda").expand(R, N)
            out = _categorical(rows, L.CAT_SAMPLE, seed=seed, step=step, what=f"sampler N={N}")
            want = P.interval_lookup(w, target)
            got = out["act"].numpy()
            wrong = int((got != want).sum())
            print(f"sampler seed={seed} step={step} N={N}: {wrong} of {R} draws off their interval; {len(np.unique(got))} distinct items")
            assert wrong == 0, (N, np.nonzero(got != want)[0][:5], got[got != want][:5], want[got != want][:5])
            assert bool((w[got] > 0).all())
            stat = out["stat"]
            assert bool((stat[:, 0] == 0).all()) and bool((stat[:, 1] == 1).all()) and bool((stat[:, 2] == 4096).all())
            q = torch.from_numpy(w[got] / 4096.0)
            _check_logprob(f"sampler N={N}", out["lp"], torch.from_numpy(w[got]).float(), stat[:, 2], stat[:, 3], q, torch.zeros(R, dtype=torch.float64),
                           torch.ones(R, dtype=torch.bool))
    assert not np.array_equal(seen[0], seen[1])


def test_masked_items_are_never_sampled(cuda):
    """CAT_SOFTMAX with a third of the logits at -inf, N = 4100, 20 000 rows of one distribution: no masked item is drawn, and the
    draws fit the float64 probabilities (chi-square over 64 contiguous-index bins, P < 1e-6; the seed is fixed)"""
    from scipy.stats import chi2 as chi2_dist
    L = _lib()
    R, N, bins = 20000, 4100, 64
    x, mask, which, expect = P.masked_sampling_case(N, bins)
    out = _categorical(x.to("cuda").expand(R, N), L.CAT_SOFTMAX | L.CAT_SAMPLE, seed=11, step=5, what="masked sampling")
    a = out["act"]
    assert int(a.min()) >= 0 and int(a.max()) < N
    assert not mask[a].any(), "a masked item was drawn"
    counts = torch.bincount(which[a], minlength=bins).double()
    chi2 = float(((counts - R * expect) ** 2 / (R * expect)).sum())
    limit = float(chi2_dist.isf(1e-6, bins - 1))
    print(f"masked sampling: chi-square {chi2:.1f} over {bins} bins (limit {limit:.1f}), {int(a.unique().numel())} distinct items")
    assert chi2 < limit
    ref = P.categorical_bounds(x[None])
    for row in range(2):                                                         # rows 0 and R - 1 of the probabilities
        _check(f"masked sampling p (row {row})", out["p"][row:row + 1], ref["p"], ref["bound"])
        assert not out["p"][row][mask].any()
    rel_at = ref["rel"][0][a] + ref["sum_bound"][0]
    _check("masked sampling logprob", out["lp"], torch.log(ref["p"][0][a].clamp(P.CAT_EPS, 1 - P.CAT_EPS)),
           4 * P.ulp32(torch.log(ref["p"][0][a])) + rel_at)
