"""GPU: the sampled softmax with shared negatives (csrc/sampled.hip), sampled_log_prob_train / sampled_cross_entropy, NegativeSampler,
NextItemHead.sampled_loss and next_item_update's sampler keys, against tests/sampled_reference.py (float64; the bound and its
derivation are stated there).  The worst measured error / tolerance per test is recorded in DESIGN.md section 28."""
import functools
import math

import numpy as np
import pytest
import torch

import sampled_reference as SR
import xent_reference as X
import ope_reference as R

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "bf16")
SLICINGS = (128, 256, None)
OUTS = ("lp", "lse", "dx", "dW", "dc")


@pytest.fixture(scope="module")
def F(cuda):
    from recnn_amd.nn import functional
    return functional


@functools.lru_cache(maxsize=None)
def _gauss(B, S, N, K, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + K * 1000 + N + B + 31 * S)
    x = torch.randn(B, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    c = torch.randn(N, generator=g)
    a = torch.randint(0, N, (B,), generator=g)
    n = torch.randint(0, N, (S,), generator=g)
    tq, nq = -torch.rand(B, generator=g) * 3, -torch.rand(S, generator=g) * 3
    return x, W, c, a, n, tq, nq, torch.randn(B, generator=g), torch.randn(B, generator=g)


def _chains(B, S, K, ips):
    fwd = SR.fwd_items_per_slice(B, S) if ips is None else ips
    bwd = SR.bwd_items_per_slice(B, S, K) if ips is None else ips
    return dict(d=SR.chain_depth(S, fwd), c1=SR.chain_dx(S, bwd), c2=SR.chain_dw(B, S))


def _run(F, cuda, x, W, c, a, n, tq, nq, g_lp, g_lse, dtype, ips, hits=True, need=(True, True, True), sparse=False):
    """(lp, lse, dx, dW, dc) on the CPU (None where not asked for) of one forward + backward."""
    xd = x.to(cuda).requires_grad_(need[0])
    Wd = W.to(cuda).requires_grad_(need[1])
    cd = None if c is None else c.to(cuda).requires_grad_(need[2])
    dv = lambda t: None if t is None else t.to(cuda)      # noqa: E731
    lp, lse = F.sampled_log_prob_train(xd, Wd, cd, a.to(cuda), n.to(cuda), target_log_q=dv(tq), negative_log_q=dv(nq),
                                       remove_accidental_hits=hits, dtype=dtype, items_per_slice=ips, sparse_grad=sparse)
    outs, grads = [], []
    if g_lp is not None:
        outs.append(lp), grads.append(g_lp.to(cuda))
    if g_lse is not None:
        outs.append(lse), grads.append(g_lse.to(cuda))
    if any(need) and outs:
        torch.autograd.backward(outs, grads)
    return tuple(None if t is None else t.detach().cpu() for t in (lp, lse, xd.grad, Wd.grad, None if cd is None else cd.grad))


def _ref(x, W, c, a, n, tq, nq, g_lp, g_lse, dtype, ips, hits=True):
    B, K = x.shape
    return SR.run(x, W, c, a, n, tq, nq, g_lp, g_lse, remove_hits=hits, bf16=dtype == "bf16", **_chains(B, len(n), K, ips))


def _bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(got, ref, what):
    """Every output that is there inside the bound; returns the worst error / tolerance."""
    worst = 0.0
    for name, t in zip(OUTS, got):
        if t is None:
            continue
        t = t.to_dense() if t.is_sparse else t
        r = SR.worst_ratio(t.numpy(), ref, name, tol=ref["tol_f"] if name in ("lp", "lse") else None)
        worst = max(worst, r)
        assert r <= 1.0, (what, name, r)
    return worst


@pytest.mark.parametrize("B,S,N,K", SR.SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gaussian_against_float64(F, cuda, B, S, N, K, dtype):
    """Gaussian inputs, random g_lp and g_lse, every slicing, with and without corrections and bias: log_prob, lse, dx, dW, dc inside
    the bound, and a second call gives the same bits."""
    x, W, c, a, n, tq, nq, g_lp, g_lse = _gauss(B, S, N, K)
    worst = 0.0
    for ips in SLICINGS:
        for cc, t, q in ((c, tq, nq), (None, None, None)) if ips != 256 else ((c, None, None),):
            got = _run(F, cuda, x, W, cc, a, n, t, q, g_lp, g_lse, dtype, ips)
            assert got[2].shape == (B, K) and got[3].shape == (N, K) and (cc is None or got[4].shape == (N,))
            worst = max(worst, _check(got, _ref(x, W, cc, a, n, t, q, g_lp, g_lse, dtype, ips), (ips, cc is None)))
            again = _run(F, cuda, x, W, cc, a, n, t, q, g_lp, g_lse, dtype, ips)
            assert all(_bits_equal(p, q_) for p, q_ in zip(got, again))
    print(f"gaussian B={B} S={S} N={N} K={K} {dtype}: worst error / tolerance = {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_accidental_hits(F, cuda, dtype):
    """Half the rows' targets planted among the negatives: removal on and off against the reference.  A row whose every negative is a
    hit: log_prob == 0 and dx = g_lse W[a] inside the bound."""
    B, S, N, K = 130, 200, 400, 64
    x, W, c, a, n, tq, nq, g_lp, g_lse = _gauss(B, S, N, K, seed=1)
    n = n.clone()
    n[:B // 2] = a[:B // 2]
    worst = 0.0
    for hits in (True, False):
        got = _run(F, cuda, x, W, c, a, n, tq, nq, g_lp, g_lse, dtype, None, hits=hits)
        worst = max(worst, _check(got, _ref(x, W, c, a, n, tq, nq, g_lp, g_lse, dtype, None, hits=hits), hits))
    on = _run(F, cuda, x, W, c, a, n, tq, nq, None, None, dtype, None, hits=True, need=(False,) * 3)
    off = _run(F, cuda, x, W, c, a, n, tq, nq, None, None, dtype, None, hits=False, need=(False,) * 3)
    assert bool((on[0][:B // 2] > off[0][:B // 2]).all())       # a removed hit takes its mass out of the denominator
    # every negative a hit
    a2 = torch.full((B,), 7)
    a2[1::2] = 9
    n2 = torch.full((S,), 7)
    got = _run(F, cuda, x, W, c, a2, n2, tq, None, g_lp, g_lse, dtype, None)
    ref = _ref(x, W, c, a2, n2, tq, None, g_lp, g_lse, dtype, None)
    worst = max(worst, _check(got, ref, "all hits"))
    rows = torch.arange(0, B, 2)
    assert bool((got[0][rows] == 0).all())
    Wr = torch.as_tensor(R.to_bf16(W.numpy())) if dtype == "bf16" else W.double()
    want = g_lse[rows].double()[:, None] * Wr[7][None]
    assert bool(((got[2][rows].double() - want).abs().numpy() <= ref["tol_dx"][rows.numpy()]).all())
    print(f"hits {dtype}: worst error / tolerance = {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_in_batch_negatives(F, cuda, dtype):
    """negatives = targets, with duplicate targets in the batch."""
    B, N, K = 150, 60, 48
    x, W, c, a, _, tq, _, g_lp, g_lse = _gauss(B, B, N, K, seed=2)
    assert len(set(a.tolist())) < B
    got = _run(F, cuda, x, W, c, a, a, tq, tq, g_lp, g_lse, dtype, None)
    worst = _check(got, _ref(x, W, c, a, a, tq, tq, g_lp, g_lse, dtype, None), "in-batch")
    print(f"in-batch {dtype}: worst error / tolerance = {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_full_catalogue_meets_catalogue_log_prob_train(F, cuda, dtype):
    """negatives = arange(N), hits removed: the full softmax.  Every output within the sum of the two kernels' bounds of
    catalogue_log_prob_train's on the same inputs."""
    B, N, K = 140, 700, 96
    x, W, c, a, _, _, _, g_lp, g_lse = _gauss(B, N, N, K, seed=3)
    n = torch.arange(N)
    got = _run(F, cuda, x, W, c, a, n, None, None, g_lp, g_lse, dtype, None)
    xd, Wd, cd = x.to(cuda).requires_grad_(), W.to(cuda).requires_grad_(), c.to(cuda).requires_grad_()
    lp, lse = F.catalogue_log_prob_train(xd, Wd, cd, a.to(cuda), dtype=dtype)
    torch.autograd.backward([lp, lse], [g_lp.to(cuda), g_lse.to(cuda)])
    full = [t.detach().cpu() for t in (lp, lse, xd.grad, Wd.grad, cd.grad)]
    ref = _ref(x, W, c, a, n, None, None, g_lp, g_lse, dtype, None)
    fwd, bwd = R.default_items_per_slice(B, N), X.bwd_items_per_slice(B, N, K)
    xr = X.backward(x, W, c, a, g_lp, g_lse, bf16=dtype == "bf16", d=R.chain_depth(N, fwd), c1=X.chain_dx(N, bwd), c2=X.chain_dw(B))
    lpx, lsex, Ex = R.log_prob(x, W, c, a, bf16=dtype == "bf16")
    tol = {"lp": ref["tol_f"] + R.allowed(Ex, lpx, lsex, N, R.chain_depth(N, fwd)), "dx": ref["tol_dx"] + xr["tol_dx"],
           "dW": ref["tol_dW"] + xr["tol_dW"], "dc": ref["tol_dc"] + xr["tol_dc"]}
    tol["lse"] = tol["lp"]
    worst = 0.0
    for name, g, f in zip(OUTS, got, full):
        err = (g.double() - f.double()).abs().numpy()
        ratio = float((err / tol[name]).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, ratio)
    print(f"full catalogue {dtype}: worst difference / summed tolerance = {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_scatter_long_list_padding_and_zeros(F, cuda, dtype):
    """One id 300 times among 600 negatives and the target of 40 rows (the long-list path of scatter_rank_kernel); negatives holding -1
    and N; untouched rows of dW and dc bitwise +0; the sparse gradient densifies to the same thing."""
    B, S, N, K = 200, 600, 900, 64
    x, W, c, a, n, tq, nq, g_lp, g_lse = _gauss(B, S, N, K, seed=4)
    a, n = a.clone(), n.clone()
    n[torch.randperm(S, generator=torch.Generator().manual_seed(5))[:300]] = 123
    a[:40] = 123
    n[-1], n[-2], n[5] = -1, N, -1
    ref = _ref(x, W, c, a, n, tq, nq, g_lp, g_lse, dtype, None, hits=False)
    got = _run(F, cuda, x, W, c, a, n, tq, nq, g_lp, g_lse, dtype, None, hits=False)
    worst = _check(got, ref, "scatter")
    untouched = torch.as_tensor(ref["count"] == 0)
    assert int(untouched.sum()) > 100
    assert bool((got[3][untouched].contiguous().view(torch.int32) == 0).all()) and bool((got[4][untouched].view(torch.int32) == 0).all())
    sp = _run(F, cuda, x, W, c, a, n, tq, nq, g_lp, g_lse, dtype, None, hits=False, sparse=True)
    assert sp[3].is_sparse and not sp[3].is_coalesced() and sp[3].shape == (N, K)
    live = (n >= 0) & (n < N)
    assert torch.equal(sp[3]._indices()[0], torch.cat([n[live], a]))
    worst = max(worst, _check(sp, ref, "sparse"))
    assert _bits_equal(sp[2], got[2]) and _bits_equal(sp[4], got[4])
    print(f"scatter {dtype}: worst error / tolerance = {worst:.3f}")


def test_sparse_grad_allocates_nothing_catalogue_sized(F, cuda):
    """N = 200,000, K = 128, S = 256, no bias: with sparse_grad the peak allocation of forward + backward stays far below one [N, K]
    fp32 matrix (102 MB), and SparseAdam takes the gradient."""
    B, S, N, K = 64, 256, 200_000, 128
    g = torch.Generator().manual_seed(6)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(cuda).requires_grad_()
    x = torch.randn(B, K, generator=g).to(cuda)
    a, n = torch.randint(0, N, (B,), generator=g).to(cuda), torch.randint(0, N, (S,), generator=g).to(cuda)
    opt = torch.optim.SparseAdam([W], lr=1e-3)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = F.sampled_cross_entropy(x, W, None, a, n, sparse_grad=True)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"sparse_grad: peak rise {rise} bytes; one [N, K] fp32 matrix {N * K * 4}")
    assert W.grad.is_sparse and W.grad._values().shape == (S + B, K)
    assert rise < N * K * 4 / 16
    before = W.detach()[a[0]].clone()
    opt.step()
    assert not torch.equal(W.detach()[a[0]], before)


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_independence_and_needs_input_grad(F, cuda, dtype):
    """With items_per_slice fixed, a row's log_prob, lse and dx bits are those of the reversed batch and of the row alone; every
    needs_input_grad combination gives the bits of the full call; bias=None."""
    B, S, N, K = 140, 300, 500, 96
    x, W, c, a, n, tq, nq, g_lp, g_lse = _gauss(B, S, N, K, seed=7)
    ips = 128
    full = _run(F, cuda, x, W, c, a, n, tq, nq, g_lp, g_lse, dtype, ips)
    rev = _run(F, cuda, x.flip(0), W, c, a.flip(0), n, tq.flip(0), nq, g_lp.flip(0), g_lse.flip(0), dtype, ips)
    for i in (0, 1, 2):
        assert _bits_equal(full[i], rev[i].flip(0)), i
    for b in (0, 77, B - 1):
        one = _run(F, cuda, x[b:b + 1], W, c, a[b:b + 1], n, tq[b:b + 1], nq, g_lp[b:b + 1], g_lse[b:b + 1], dtype, ips)
        for i in (0, 1, 2):
            assert _bits_equal(full[i][b:b + 1], one[i]), (b, i)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)):
        part = _run(F, cuda, x, W, c, a, n, tq, nq, g_lp, g_lse, dtype, ips, need=need)
        for i, want in zip((2, 3, 4), need):
            assert (part[i] is not None) == want and (not want or _bits_equal(part[i], full[i])), (need, i)
    only_lse = _run(F, cuda, x, W, c, a, n, tq, nq, None, g_lse, dtype, ips)
    _check(only_lse, _ref(x, W, c, a, n, tq, nq, None, g_lse, dtype, ips), "g_lse only")
    nob = _run(F, cuda, x, W, None, a, n, tq, nq, g_lp, g_lse, dtype, ips)
    assert nob[4] is None
    _check(nob, _ref(x, W, None, a, n, tq, nq, g_lp, g_lse, dtype, ips), "no bias")


def test_invalid_targets_and_empty_batch(F, cuda):
    B, S, N, K = 40, 50, 80, 32
    x, W, c, a, n, tq, nq, g_lp, g_lse = _gauss(B, S, N, K, seed=8)
    a = a.clone()
    a[3], a[17] = -1, N
    got = _run(F, cuda, x, W, c, a, n, tq, nq, g_lp, g_lse, "fp32", None)
    assert torch.isnan(got[0]).nonzero().flatten().tolist() == [3, 17]
    assert all(bool(torch.isfinite(t).all()) for t in got[1:])
    _check(got, _ref(x, W, c, a, n, tq, nq, g_lp, g_lse, "fp32", None), "invalid")
    # sampled_cross_entropy: ignore_index rows contribute nothing, other invalid targets are refused
    t = a.clone()
    t[3], t[17] = -100, -100
    Wd = W.to(cuda).requires_grad_()
    loss = F.sampled_cross_entropy(x.to(cuda), Wd, c.to(cuda), t.to(cuda), n.to(cuda), reduction="none")
    assert loss[3] == 0 and loss[17] == 0 and bool((loss >= 0).all())
    mean = F.sampled_cross_entropy(x.to(cuda), Wd, c.to(cuda), t.to(cuda), n.to(cuda))
    assert abs(float(mean) - float(loss.sum()) / (B - 2)) < 1e-5
    with pytest.raises(ValueError, match="outside"):
        F.sampled_cross_entropy(x.to(cuda), Wd, c.to(cuda), a.to(cuda), n.to(cuda))
    # an empty batch launches nothing and gives exact zeros
    e = _run(F, cuda, x[:0], W, c, a[:0], n, None, None, g_lp[:0], g_lse[:0], "fp32", None)
    assert e[0].shape == (0,) and e[2].shape == (0, K) and not e[3].any() and not e[4].any()


def test_refusals_on_the_gpu(F, cuda):
    x, W, c, a, n, tq, nq, _, _ = _gauss(8, 8, 20, 32, seed=9)
    dv = lambda t: t.to(cuda)      # noqa: E731
    with pytest.raises(ValueError, match="S = 0"):
        F.sampled_log_prob_train(dv(x), dv(W), None, dv(a), dv(n[:0]))
    with pytest.raises(ValueError, match="negative_log_q"):
        F.sampled_log_prob_train(dv(x), dv(W), None, dv(a), dv(n), negative_log_q=dv(nq[:3]))
    with pytest.raises(ValueError, match="target_log_q"):
        F.sampled_log_prob_train(dv(x), dv(W), None, dv(a), dv(n), target_log_q=dv(tq[:3]))
    with pytest.raises(ValueError, match="320"):
        F.sampled_log_prob_train(torch.zeros(8, 300, device=cuda), torch.zeros(20, 300, device=cuda), None, dv(a), dv(n))


# ------------------------------------------------------------------------------------------------------------ end to end

def _seq_env(cuda):
    import seq_reference as S
    from recnn_amd.data.env import SeqEnv
    table, user_dict, users, _ = S.seq_env_data(E=16)
    items = np.concatenate([user_dict[u]["items"] for u in users])
    ratings = np.concatenate([user_dict[u]["ratings"] for u in users])
    off = np.concatenate([[0], np.cumsum([len(user_dict[u]["items"]) for u in users])]).astype(np.int64)
    torch.manual_seed(0)
    E = table.shape[1]
    gru = torch.nn.GRU(E + 1, E).to(cuda)
    env = SeqEnv.from_store(table, items, ratings, off, state_encoder=gru, test_fraction=0.0, batch_size=5, max_buf_size=20, device=cuda)
    return env, items, gru


def test_next_item_update_with_a_sampler(cuda):
    """12-user SeqEnv, GRU with H = E = 16 and a tied table: 20 Adam steps of next_item_update with a uniform sampler and
    n_negatives >= half the catalogue lower the FULL cross-entropy of the training batch (tests/test_sampled_cpu.py confirms in
    float64 that this setup drops it by more than 10 %).  Without the new keys the update is the full-softmax one, bit for bit."""
    import recnn_amd
    from recnn_amd.nn import NegativeSampler
    env, items, gru = _seq_env(cuda)
    ids, steps = [0, 1, 2, 3, 4], [3, 4, 9, 30]
    P = env.table.clone().requires_grad_(True)
    N = P.shape[0]
    head = recnn_amd.nn.NextItemHead(P)

    def batch_of():
        batch = env.user_batch(ids, steps, table=P)
        batch["target"] = env.target_items(batch)
        return batch
    nets = {"head": head}
    full = lambda: float(recnn_amd.nn.next_item_update(batch_of(), {}, nets, None, learn=False)["loss"])      # noqa: E731
    before = full()
    sampler = NegativeSampler(N, seed=3, device=cuda)
    params = {"sampler": sampler, "n_negatives": (N + 1) // 2 + 7}
    opt = torch.optim.Adam([P] + list(gru.parameters()), lr=1e-2)
    for step in range(20):
        out = recnn_amd.nn.next_item_update(batch_of(), params, nets, {"optimizer": opt}, learn=True, step=step)
        assert math.isfinite(float(out["loss"]))
    after = full()
    print(f"sampled next_item_update: full cross-entropy {before:.4f} -> {after:.4f}")
    assert after < before
    # in-batch negatives, alone and joined with sampled ones, and a from_store sampler
    for prm in ({"in_batch": True}, {"in_batch": True, "sampler": NegativeSampler.from_store(type("S", (), {"items": items}), N, device=cuda),
                                     "n_negatives": 16}):
        out = recnn_amd.nn.next_item_update(batch_of(), prm, nets, {"optimizer": opt}, learn=True, step=0)
        assert math.isfinite(float(out["loss"]))

    # without the new keys: what head.loss gives, bit for bit, in the loss and in the stepped table
    def one_step(update):
        torch.manual_seed(1)
        Q = env.table.clone().requires_grad_(True)
        h = recnn_amd.nn.NextItemHead(Q)
        o = torch.optim.SGD([Q], lr=0.1)
        batch = env.user_batch(ids, steps)
        state, target = batch["state"].detach(), env.target_items(batch)
        if update:
            loss = recnn_amd.nn.next_item_update({"state": state, "target": target}, update, {"head": h}, {"optimizer": o})["loss"]
            loss = torch.tensor(float(loss))
        else:
            rows = h.loss(state, target, reduction="none")
            loss = rows.sum() / (target != -100).sum()
            o.zero_grad()
            loss.backward()
            o.step()
            loss = loss.detach().cpu()
        return loss, Q.detach().cpu()
    l0, q0 = one_step(None)
    for prm in ({"ignore_index": -100}, {"sampler": None, "in_batch": False}):
        l1, q1 = one_step(prm)
        assert float(l0) == float(l1) and _bits_equal(q0, q1)
