"""No GPU: tests/sampled_reference.py's closed form against float64 torch autograd, the soundness of its bound on torch's own fp32
route, the host-only workspace queries and refusals of csrc/sampled.hip, and NegativeSampler on the CPU device."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import sampled_reference as SR


def _case(B, S, N, K, seed=0, hits=0, bad_neg=0, bad_tgt=0):
    g = torch.Generator().manual_seed(seed * 7919 + K * 1000 + N + B + 31 * S)
    x = torch.randn(B, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    c = torch.randn(N, generator=g)
    a = torch.randint(0, N, (B,), generator=g)
    n = torch.randint(0, N, (S,), generator=g)
    tq, nq = -torch.rand(B, generator=g) * 3, -torch.rand(S, generator=g) * 3
    g_lp, g_lse = torch.randn(B, generator=g), torch.randn(B, generator=g)
    n[:hits] = a[:hits]                      # accidental hits
    if S > 4:
        n[S // 2] = n[0]                     # a repeat
    for i in range(bad_neg):
        n[S - 1 - i] = -1 if i % 2 else N    # out-of-range negatives
    for i in range(bad_tgt):
        a[B - 1 - i] = -100 if i % 2 else N + 3      # ignored / invalid targets
    return [t.numpy() for t in (x, W, c, a, n, tq, nq, g_lp, g_lse)]


@pytest.mark.parametrize("remove_hits", (True, False))
@pytest.mark.parametrize("B,S,N,K,hits,bad_neg,bad_tgt", ((1, 1, 2, 4, 0, 0, 0), (9, 7, 5, 6, 3, 0, 0), (40, 33, 20, 12, 10, 4, 3),
                                                         (30, 30, 50, 8, 30, 2, 2)))
def test_closed_form_equals_autograd(B, S, N, K, hits, bad_neg, bad_tgt, remove_hits):
    """The float64 closed form (log_prob, lse, dx and the scatter-summed dW, dc) equals float64 torch autograd of the materialised
    formulation: hits, repeats, out-of-range negatives, invalid and ignored targets."""
    x, W, c, a, n, tq, nq, g_lp, g_lse = _case(B, S, N, K, seed=1, hits=hits, bad_neg=bad_neg, bad_tgt=bad_tgt)
    ref = SR.run(x, W, c, a, n, tq, nq, g_lp, g_lse, remove_hits=remove_hits)
    lp, lse, dx, dW, dc = SR.torch_autograd(x, W, c, a, n, tq, nq, g_lp, g_lse, remove_hits=remove_hits)
    ok = (a >= 0) & (a < N)
    assert np.array_equal(np.isnan(ref["lp"]), ~ok) and np.array_equal(np.isnan(lp), ~ok)
    np.testing.assert_allclose(ref["lp"][ok], np.minimum(lp[ok], 0.0), rtol=0, atol=1e-12)
    for got, name in ((lse, "lse"), (dx, "dx"), (dW, "dW"), (dc, "dc")):
        np.testing.assert_allclose(ref[name], got, rtol=0, atol=1e-12, err_msg=name)
    # compact rows: one per negative, zero for an absent one; targets separately
    live = (n >= 0) & (n < N)
    assert not ref["dWs"][~live].any() and not ref["dcs"][~live].any() and not ref["Dt"][~ok].any()


def test_bound_holds_for_torch_fp32_at_the_gpu_shapes():
    """Soundness: torch's own fp32 materialised route on the CPU (another summation order, another expf) stays inside the bound at
    every shape the GPU test uses.  (tests/xent_reference.py's stayed below 0.09.)"""
    worst = 0.0
    for B, S, N, K in SR.SHAPES:
        x, W, c, a, n, tq, nq, g_lp, g_lse = _case(B, S, N, K)
        ips_f, ips_b = SR.fwd_items_per_slice(B, S), SR.bwd_items_per_slice(B, S, K)
        ref = SR.run(x, W, c, a, n, tq, nq, g_lp, g_lse, d=SR.chain_depth(S, ips_f), c1=SR.chain_dx(S, ips_b), c2=SR.chain_dw(B, S))
        lp, lse, dx, dW, dc = SR.torch_autograd(x, W, c, a, n, tq, nq, g_lp, g_lse, dtype=torch.float32)
        for got, name in ((lp, "lp"), (lse, "lse"), (dx, "dx"), (dW, "dW"), (dc, "dc")):
            r = SR.worst_ratio(got, ref, name, tol=ref["tol_f"] if name in ("lp", "lse") else None)
            print(f"torch fp32 B={B} S={S} N={N} K={K} {name}: error / tolerance = {r:.3f}")
            worst = max(worst, r)
    print(f"torch fp32, worst error / tolerance over the GPU shapes = {worst:.3f}")
    assert worst <= 1.0


def test_chunks_and_chains():
    for B, S in ((1, 1), (127, 130), (2048, 4096), (2048, 1024), (300, 16384), (100000, 128)):
        chunks, tpc = SR.chunks_of(B, S)
        row_tiles, item_tiles = (B + 127) // 128, (S + 127) // 128
        assert chunks >= 1 and chunks * tpc >= row_tiles > (chunks - 1) * tpc
        assert chunks * item_tiles <= max(256, item_tiles) + item_tiles
    assert SR.chunks_of(2048, 4096) == (8, 2) and SR.chunks_of(300, 1500) == (3, 1)


@pytest.fixture(scope="module")
def lib():
    from recnn_amd import _lib
    return _lib.load()


def test_workspace_queries_are_host_only(lib):
    n = C.c_int64(-1)
    assert lib.recnn_sampled_logprob_workspace_bytes(300, 1500, 256, C.byref(n)) == 0 and n.value == 2 * 6 * 300 * 4
    assert lib.recnn_sampled_logprob_bwd_workspace_bytes(300, 1500, 256, 256, C.byref(n)) == 0
    r256 = lambda b: (b + 255) // 256 * 256      # noqa: E731
    assert n.value == r256(6 * 300 * 256 * 4) + r256(3 * 1500 * 256 * 4) + r256(3 * 1500 * 4)
    assert lib.recnn_sampled_logprob_bwd_workspace_bytes(100, 1500, 64, 512, C.byref(n)) == 0 and n.value == r256(3 * 100 * 64 * 4)
    assert lib.recnn_sampled_scatter_workspace_bytes(10, 20, 100, 64, C.byref(n)) == 0
    assert n.value == r256(400) + r256(404) + 3 * r256(120) + r256(30 * 64 * 4) + r256(120) + r256(12)
    for fn, args, word in ((lib.recnn_sampled_logprob_workspace_bytes, (4, 0, 128, C.byref(n)), b"S = 0"),
                           (lib.recnn_sampled_logprob_workspace_bytes, (4, 8, 100, C.byref(n)), b"multiple of 128"),
                           (lib.recnn_sampled_logprob_workspace_bytes, (-1, 8, 128, C.byref(n)), b"B >= 0"),
                           (lib.recnn_sampled_logprob_bwd_workspace_bytes, (4, 8, 320, 128, C.byref(n)), b"K = 320"),
                           (lib.recnn_sampled_logprob_bwd_workspace_bytes, (4, 0, 64, 128, C.byref(n)), b"S = 0"),
                           (lib.recnn_sampled_scatter_workspace_bytes, (4, 8, 0, 64, C.byref(n)), b"N >= 1"),
                           (lib.recnn_sampled_logprob_workspace_bytes, (4, 8, 128, None), b"null")):
        assert fn(*args) != 0 and word in lib.recnn_last_error(), word
    # the entry points refuse S = 0 and a padded K of 320 before touching any pointer or the device
    assert lib.recnn_sampled_logprob(None, 64, 4, 64, None, 64, 0, None, 10, None, None, 0, None, None, 1, 128, None, None, None, None,
                                     None) != 0 and b"S = 0" in lib.recnn_last_error()
    assert lib.recnn_sampled_logprob(None, 320, 4, 320, None, 320, 0, None, 10, None, None, 8, None, None, 1, 128, None, None, None, None,
                                     None) != 0 and b"K = 320" in lib.recnn_last_error()


def test_python_refusals_by_name(lib):
    from recnn_amd import _lib
    from recnn_amd.nn import functional as F
    x, W = torch.zeros(4, 32), torch.zeros(10, 32)
    a, n = torch.zeros(4, dtype=torch.int64), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(_lib.RecnnHipError, match="GPU"):
        F.sampled_log_prob_train(x, W, None, a, n)
    with pytest.raises(_lib.RecnnHipError, match="GPU"):
        F.sampled_cross_entropy(x, W, None, a, n)
    with pytest.raises(ValueError, match="320"):
        F.sampled_log_prob_train(torch.zeros(4, 300), torch.zeros(10, 300), None, a, n)
    with pytest.raises(ValueError, match="reduction"):
        F.sampled_cross_entropy(x, W, None, a, n, reduction="max")


# ------------------------------------------------------------------------------------------------------------ NegativeSampler

def _sampler(**kw):
    from recnn_amd.nn import NegativeSampler
    return NegativeSampler(device="cpu", **kw)


SAMPLER_SEED = 11      # chosen once; the 5-sigma check below holds for it


def test_negative_sampler_distribution():
    N = 50
    counts = torch.arange(N, dtype=torch.float64) ** 2          # skewed, with a zero count
    s = _sampler(n_items=N, counts=counts, power=0.75, smoothing=1.0, seed=SAMPLER_SEED)
    w = (counts + 1.0) ** 0.75
    q = w / w.sum()
    ids = torch.arange(N)
    assert torch.equal(s.log_q(ids), torch.log(q).float())
    assert s.log_q(torch.tensor([-1, N, 3])).tolist()[:2] == [0.0, 0.0]
    draws, lq = s.sample(200_000)
    assert draws.dtype == torch.int64 and lq.dtype == torch.float32 and torch.equal(lq, s.log_q(draws))
    assert int(draws.min()) >= 0 and int(draws.max()) < N
    freq = torch.bincount(draws, minlength=N).double() / 200_000
    sigma = torch.sqrt(q * (1 - q) / 200_000)
    z = ((freq - q).abs() / sigma).max()
    print(f"NegativeSampler: worst deviation {float(z):.2f} sigma")
    assert float(z) <= 5.0
    again, _ = _sampler(n_items=N, counts=counts, seed=SAMPLER_SEED).sample(1000)
    assert torch.equal(again, draws[:1000])
    other, _ = _sampler(n_items=N, counts=counts, seed=SAMPLER_SEED + 1).sample(1000)
    assert not torch.equal(other, again)
    # uniform
    u = _sampler(n_items=N, seed=0)
    assert torch.allclose(u.log_q(ids), torch.full((N,), -math.log(N)))
    # from_store counts the store's items
    store = type("Store", (), {"items": np.array([1, 1, 4, 49, 4, 1])})
    from recnn_amd.nn import NegativeSampler
    fs = NegativeSampler.from_store(store, N, smoothing=0.5, power=1.0, device="cpu")
    assert abs(math.exp(float(fs.log_q(torch.tensor([1])))) - 3.5 / (6 + 0.5 * N)) < 1e-6


def test_negative_sampler_refuses_zero_q():
    with pytest.raises(ValueError, match="q = 0"):
        _sampler(n_items=4, counts=[1, 0, 2, 3], smoothing=0.0)
    with pytest.raises(ValueError, match="counts"):
        _sampler(n_items=4, counts=[1, 2, 3])
    _sampler(n_items=4, counts=[1, 0, 2, 3], smoothing=1e-3)


# ------------------------------------------------------------------------------------------------------------ the end-to-end setup

def test_end_to_end_setup_drops_the_full_loss_in_float64():
    """What tests/test_gpu_sampled.py::test_next_item_update_with_a_sampler relies on, confirmed in float64 on the CPU: the 12-user
    data, a GRU with H = E = 16 over [embedding | rating], the table tied to the head, states h_{t-1} -> target item_t for 5 users x 4
    steps, a uniform sampler with n_negatives >= half the catalogue, 20 Adam steps at lr 1e-2.  The FULL cross-entropy of the batch
    drops by at least 10 %."""
    import seq_reference as S
    table, user_dict, users, _ = S.seq_env_data(E=16)
    ids, steps = [0, 1, 2, 3, 4], [3, 4, 9, 30]
    N, E = table.shape
    torch.manual_seed(0)
    gru = torch.nn.GRU(E + 1, E, batch_first=True).double()
    P = table.double().clone().requires_grad_(True)
    items = torch.as_tensor(np.stack([user_dict[u]["items"][:max(steps) + 1] for u in ids]))
    ratings = torch.as_tensor(np.stack([user_dict[u]["ratings"][:max(steps) + 1] for u in ids])).double()
    target = torch.cat([items[:, t] for t in steps])

    def states():
        h, _ = gru(torch.cat([P[items], ratings[..., None]], 2))
        return torch.cat([h[:, t - 1] for t in steps])
    full = lambda: float(torch.nn.functional.cross_entropy(states() @ P.T, target).detach())      # noqa: E731
    sampler = _sampler(n_items=N, seed=3)
    opt = torch.optim.Adam([P] + list(gru.parameters()), lr=1e-2)
    before = full()
    for _ in range(20):
        neg, nq = sampler.sample((N + 1) // 2 + 7)
        x = states()
        z = x @ P[neg].T - nq.double()[None]
        z = z.masked_fill(neg[None, :] == target[:, None], -math.inf)
        zt = (x * P[target]).sum(1) - sampler.log_q(target).double()
        loss = (torch.logsumexp(torch.cat([zt[:, None], z], 1), 1) - zt).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    after = full()
    print(f"float64 setup: full cross-entropy {before:.4f} -> {after:.4f}")
    assert after <= 0.9 * before
