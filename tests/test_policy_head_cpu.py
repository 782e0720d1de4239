"""The references of tests/policy_head_reference.py without a GPU: softmax, both backwards and the sharded composition against torch's
float64 autograd, the sampler's item order and interval lookup, and -- for every input set tests/test_gpu_policy_head.py uses -- the
probes that show the reference moving by at least 100 bounds when the option under test is removed."""
import numpy as np
import pytest
import torch

import policy_head_reference as P


def _logits(R, N, seed):
    return torch.randn(R, N, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 3.0


@pytest.mark.parametrize("N", P.NS)
def test_softmax_and_logprob_equal_torch(N):
    x = _logits(5, N, N)
    mx, den, p, _ = P.softmax64(x)
    assert torch.equal(mx, x.max(1).values)
    err = float((p - torch.softmax(x, 1)).abs().max())
    err_den = float((den - torch.exp(x - mx[:, None]).sum(1)).abs().max())
    print(f"N={N}: softmax {err:.3e}, denominator {err_den:.3e}")
    assert err <= 1e-12 and err_den <= 1e-12 * N
    # masked items: exact zeros, like torch
    xm = x.clone()
    xm[:, ::3] = -P.INF
    if N > 1:
        pm = P.softmax64(xm)[2]
        assert float((pm - torch.softmax(xm, 1)).abs().max()) <= 1e-12 and not pm[:, ::3].any()
    a = torch.randint(0, N, (5,), generator=torch.Generator().manual_seed(N))
    lp, clamped = P.logprob64(p, a)
    want = torch.distributions.Categorical(probs=p).log_prob(a)          # float64: its clamp is float64's eps, far below any p here
    free = ~clamped
    assert float((lp[free] - want[free]).abs().max() if bool(free.any()) else 0.0) <= 1e-12
    lp_bad, cl_bad = P.logprob64(p, torch.tensor([N, -1, N, -1, N]))
    assert bool(torch.isnan(lp_bad).all()) and not cl_bad.any()


@pytest.mark.parametrize("N", P.NS)
def test_logprob_backward_equals_autograd(N):
    R = 7
    gen = torch.Generator().manual_seed(N + 1)
    x = _logits(R, N, N + 2).requires_grad_(True)
    a = torch.randint(0, N, (R,), generator=gen)
    g = torch.randn(R, generator=gen, dtype=torch.float64)
    scale = 0.5 + torch.rand(R, generator=gen, dtype=torch.float64)
    (g * torch.log_softmax(x, 1).gather(1, a.view(-1, 1))[:, 0]).sum().backward()
    p = torch.softmax(x.detach(), 1) * scale[:, None]                   # unnormalised: the kernel divides by the row's sum
    none = torch.zeros(R, dtype=torch.bool)
    got, bound = P.logprob_bwd64(p, a, g, p.sum(1), none)
    assert float((got - x.grad).abs().max()) <= 1e-12 and bool((bound > 0).all())
    old = torch.randn(R, N, generator=gen, dtype=torch.float64)
    assert float((P.logprob_bwd64(p, a, g, p.sum(1), none, old)[0] - (x.grad + old)).abs().max()) <= 1e-12
    clamped = torch.arange(R) % 2 == 0
    got = P.logprob_bwd64(p, a, g, p.sum(1), clamped)[0]
    assert not got[clamped].any() and float((got[~clamped] - x.grad[~clamped]).abs().max()) <= 1e-12
    assert not P.logprob_bwd64(p, a, None, p.sum(1), none)[0].any()
    # a shard's share: the same gradient on the columns it holds, the action's term on the owner alone
    lo, hi = N // 3, N
    got = P.shard_logprob_bwd64(torch.softmax(x.detach(), 1)[:, lo:hi], a - lo, g)[0]
    assert float((got - x.grad[:, lo:hi]).abs().max()) <= 1e-12


@pytest.mark.parametrize("N", P.NS)
def test_softmax_backward_equals_autograd(N):
    x = _logits(4, N, N + 3).requires_grad_(True)
    dp = torch.randn(4, N, generator=torch.Generator().manual_seed(N + 4), dtype=torch.float64)
    dp[0, 0] = 1e4
    (torch.softmax(x, 1) * dp).sum().backward()
    got, _ = P.softmax_bwd64(torch.softmax(x.detach(), 1), dp)
    err = float((got - x.grad).abs().max())
    print(f"N={N}: softmax backward {err:.3e} of {float(x.grad.abs().max()):.3e}")
    assert err <= 1e-12 * max(1.0, float(x.grad.abs().max()))


@pytest.mark.parametrize("parts", (2, 3))
@pytest.mark.parametrize("N", P.SHARD_NS)
def test_sharded_composition_equals_the_whole_softmax(N, parts):
    x, a, cuts = P.shard_case(N, parts)
    assert cuts[0][0] == 0 and cuts[-1][1] == N and all(c[1] == d[0] for c, d in zip(cuts, cuts[1:]))
    assert float((P.shard_softmax64(x, cuts) - torch.softmax(x.double(), 1)).abs().max()) <= 1e-12
    assert set(a.tolist()) >= {0, N - 1, cuts[0][1] - 1, cuts[1][0]}
    P.assert_probes(P.shard_probes(N, parts))


@pytest.mark.parametrize("N", P.NS)
def test_thread_major_order_is_a_permutation(N):
    order = P.thread_major_order(N)
    assert np.array_equal(np.sort(order), np.arange(N))
    if N <= 4096:
        assert np.array_equal(order, np.arange(N))
    else:                                            # thread 0: items 0..3, then its second float4 group
        assert order[:5].tolist() == [0, 1, 2, 3, 4096]


def test_thread_major_order_written_out():
    """N = 8195: thread 0 owns 0..3, 4096..4099, 8192..8194; thread 1 follows with 4..7, 4100..4103; the last thread ends the order"""
    order = P.thread_major_order(8195).tolist()
    assert order[:11] == [0, 1, 2, 3, 4096, 4097, 4098, 4099, 8192, 8193, 8194]
    assert order[11:19] == [4, 5, 6, 7, 4100, 4101, 4102, 4103]
    assert order[-8:] == [4092, 4093, 4094, 4095, 8188, 8189, 8190, 8191]


@pytest.mark.parametrize("N", P.SAMPLER_NS + (4096,))
def test_interval_lookup_finds_point_masses(N):
    targets = np.array([0, 1, 2047, 4095])
    for item in sorted({0, N - 1, N // 2, min(N - 1, 4096)}):
        w = np.zeros(N, dtype=np.int64)
        w[item] = P.SAMPLER_TOTAL
        assert P.interval_lookup(w, targets).tolist() == [item] * 4
    # all weights one at N = 4096: the identity (the calibration of the GPU test)
    if N == 4096:
        assert np.array_equal(P.interval_lookup(np.ones(N, dtype=np.int64), np.arange(N)), np.arange(N))


@pytest.mark.parametrize("N", P.SAMPLER_NS)
def test_sampler_weights(N):
    w = P.sampler_weights(N)
    assert int(w.sum()) == P.SAMPLER_TOTAL and w.min() == 0 and w[0] > 0 and w[N - 1] > 0
    if N > 4096:
        assert w[4096] > 0
    if N > 4100:
        assert w[4097] > 0 and w[4098] == 0 and w[4099] > 0 and w[8192] > 0
    drawn = P.interval_lookup(w, np.arange(P.SAMPLER_TOTAL))
    assert np.array_equal(np.bincount(drawn, minlength=N), w)                 # every target once: each item as often as its weight
    P.assert_probes(P.sampler_probes(N))


def test_masked_sampling_case():
    x, mask, which, expect = P.masked_sampling_case()
    assert 0.3 < float(mask.double().mean()) < 0.37 and abs(float(expect.sum()) - 1.0) < 1e-12
    assert int(which.max()) == 63 and float(expect.min()) * 20000 >= 20           # every bin's expected count is far above 5


# ---------------------------------------------------------------------------------------------------- the GPU test's input sets
@pytest.mark.parametrize("N", P.NS)
def test_softmax_input_sets_probe(N):
    x, a = P.softmax_case(N)
    assert x.dtype == torch.float32 and x.shape == (len(P.SOFTMAX_ROWS), N)
    ref = P.categorical_bounds(x)
    lp, clamped = P.logprob64(ref["p"], a)
    assert bool(clamped[10]) and bool(torch.isnan(lp[11:]).all())
    if N == 1:
        assert bool(clamped[:11].all())                                            # p = 1 > 1 - eps
    else:
        assert float(x[9].max() - x[9].min()) == 120.0 and float(ref["p"][9].min()) < 1e-44
        assert float(lp[10]) == float(np.log(P.CAT_EPS))
    free = ~clamped & ~torch.isnan(lp)
    assert bool((lp[free].abs() >= 0.5).all())
    P.assert_probes(P.softmax_probes(N))


@pytest.mark.parametrize("N", P.NS)
def test_masked_input_sets_probe(N):
    x, a, names = P.masked_case(N)
    ref = P.categorical_bounds(x)
    assert bool(torch.isfinite(ref["p"]).all()) and not ref["p"][ref["masked"]].any()
    assert float((ref["p"].sum(1) - 1).abs().max()) < 1e-12
    if N >= 3:
        assert 0 < int(ref["masked"][:3].sum()) < 3 * N
    if N > 4096:
        assert names[3] == "items 0..3" and names[4] == "items 4092..4095"
        assert bool(torch.isinf(x[3, :4]).all()) and bool(torch.isfinite(x[3, 4:]).all())
        assert bool(torch.isinf(x[4, 4092:4096]).all()) and int(torch.isinf(x[4]).sum()) == 4
    assert int(torch.isfinite(x[5]).sum()) == 1 and bool(torch.isfinite(x[5, N - 1]))
    P.assert_probes(P.masked_probes(N))


@pytest.mark.parametrize("N", P.NS)
def test_backward_input_sets_probe(N):
    for R in P.ROWS:
        c = P.logprob_bwd_case(R, N)
        assert int(c["actions"][0]) == N - 1 and torch.equal(c["old"], c["old"].to(torch.bfloat16).float())
        if R >= 5 and N >= 4:
            assert sorted(int(v) % 4 for v in c["actions"][:4]) == [0, 1, 2, 3] or N % 4 == 0
            assert {int(v) // 4 for v in c["actions"][:4]} <= {(N - 1) // 4, (N - 1) // 4 - 1}
        P.assert_probes(P.logprob_bwd_probes(R, N))
    P.assert_probes(P.softmax_bwd_probes(N))


@pytest.mark.parametrize("R", (257, 300))
def test_shard_backward_input_sets_probe(R):
    P.assert_probes(P.shard_bwd_probes(R, 1025))
