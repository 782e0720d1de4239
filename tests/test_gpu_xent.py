"""GPU: the backward of the catalogue log-prob (csrc/logprob_bwd.hip), catalogue_log_prob_train / catalogue_cross_entropy,
NextItemHead, SeqEnv.target_items and next_item_update, against tests/xent_reference.py (float64; the bound and its derivation are
stated there).  The worst measured error / tolerance per test is recorded in DESIGN.md section 27."""
import functools
import math

import numpy as np
import pytest
import torch

import ope_reference as R
import xent_reference as X

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "bf16")
SLICINGS = (128, 256, None)


@pytest.fixture(scope="module")
def F(cuda):
    from recnn_amd.nn import functional
    return functional


@functools.lru_cache(maxsize=None)
def _gauss(B, N, K, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + K * 1000 + N + B)
    x = torch.randn(B, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    c = torch.randn(N, generator=g)
    a = torch.randint(0, N, (B,), generator=g)
    return x, W, c, a, torch.randn(B, generator=g), torch.randn(B, generator=g)


def _chains(B, N, K, ips):
    """(d, c1, c2) of one call: the forward's chain depth and the backward's chains, for the slicing `ips` (None: the defaults)."""
    fwd = R.default_items_per_slice(B, N) if ips is None else ips
    bwd = X.bwd_items_per_slice(B, N, K) if ips is None else ips
    return R.chain_depth(N, fwd), X.chain_dx(N, bwd), X.chain_dw(B)


def _run(F, cuda, x, W, c, a, g_lp, g_lse, dtype, ips, need=(True, True, True)):
    """(lp, lse, dx, dW, dc) on the CPU (None where not asked for) of one forward + backward."""
    xd = x.to(cuda).requires_grad_(need[0])
    Wd = W.to(cuda).requires_grad_(need[1])
    cd = None if c is None else c.to(cuda).requires_grad_(need[2])
    lp, lse = F.catalogue_log_prob_train(xd, Wd, cd, a.to(cuda), dtype=dtype, items_per_slice=ips)
    outs, grads = [], []
    if g_lp is not None:
        outs.append(lp), grads.append(g_lp.to(cuda))
    if g_lse is not None:
        outs.append(lse), grads.append(g_lse.to(cuda))
    torch.autograd.backward(outs, grads)
    return tuple(None if t is None else t.detach().cpu() for t in (lp, lse, xd.grad, Wd.grad, None if cd is None else cd.grad))


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(got, ref, what):
    """Every gradient inside the bound; returns the worst error / tolerance."""
    worst = 0.0
    for name, t in zip(("dx", "dW", "dc"), got[2:]):
        r = X.worst_ratio(t.numpy(), ref, name)
        worst = max(worst, r)
        assert r <= 1.0, (what, name, r)
    return worst


@pytest.mark.parametrize("B,N,K", X.SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gaussian_against_float64(F, cuda, B, N, K, dtype):
    """Gaussian inputs, random g_lp and g_lse, every slicing: forward bits equal catalogue_log_prob's, dx / dW / dc inside the bound,
    and a second call gives the same bits."""
    x, W, c, a, g_lp, g_lse = _gauss(B, N, K)
    worst = 0.0
    for ips in SLICINGS:
        got = _run(F, cuda, x, W, c, a, g_lp, g_lse, dtype, ips)
        lp, lse = F.catalogue_log_prob(x.to(cuda), W.to(cuda), c.to(cuda), a.to(cuda), dtype=dtype, items_per_slice=ips)
        assert _bits_equal(got[0], lp.cpu()) and _bits_equal(got[1], lse.cpu()) and not lp.requires_grad
        assert got[2].shape == (B, K) and got[3].shape == (N, K) and got[4].shape == (N,)
        d, c1, c2 = _chains(B, N, K, ips)
        ref = X.backward(x, W, c, a, g_lp, g_lse, bf16=dtype == "bf16", d=d, c1=c1, c2=c2)
        worst = max(worst, _check(got, ref, (ips,)))
        again = _run(F, cuda, x, W, c, a, g_lp, g_lse, dtype, ips)
        assert all(_bits_equal(p, q) for p, q in zip(got, again))
    print(f"gaussian B={B} N={N} K={K} {dtype}: worst error / tolerance = {worst:.3f}")


@pytest.mark.parametrize("B,N,K", X.SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_weights(F, cuda, B, N, K, dtype):
    """W = 0, c = 0: p = 1 / N exactly, so dx = 0 exactly, dc[n] = sum_b g_b ([a_b = n] - 1 / N) and dW = D^T x to the bound: a
    dropped or double-counted item or row shows."""
    x, _, _, a, g_lp, _ = _gauss(B, N, K, seed=1)
    W, c = torch.zeros(N, K), torch.zeros(N)
    want_dc = np.zeros(N)
    np.add.at(want_dc, a.numpy(), g_lp.double().numpy())
    want_dc -= g_lp.double().sum().item() / N
    worst = 0.0
    for ips in SLICINGS:
        got = _run(F, cuda, x, W, c, a, g_lp, None, dtype, ips)
        assert bool((got[2] == 0).all())
        d, c1, c2 = _chains(B, N, K, ips)
        ref = X.backward(x, W, c, a, g_lp, None, bf16=dtype == "bf16", d=d, c1=c1, c2=c2)
        assert np.abs(ref["dc"] - want_dc).max() <= 1e-12
        worst = max(worst, _check(got, ref, (ips,)))
    print(f"zero weights B={B} N={N} K={K} {dtype}: worst error / tolerance = {worst:.3f}")


@pytest.mark.parametrize("B,N,K", X.SHAPES[1:])
@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_item(F, cuda, B, N, K, dtype):
    """W = 0, c = -200 except c_j = 0, every action j: p_j = 1 to rounding, so the gradient at the planted row is about 0 (inside the
    bound of a true value of 1e-85) -- and finite, like everything else."""
    x, _, _, _, g_lp, _ = _gauss(B, N, K, seed=2)
    W = torch.zeros(N, K)
    worst = 0.0
    for j in sorted({0, 127 % N, 128 % N, N - 1}):
        c = torch.full((N,), -200.0)
        c[j] = 0.0
        a = torch.full((B,), j, dtype=torch.int64)
        got = _run(F, cuda, x, W, c, a, g_lp, None, dtype, 128)
        assert all(bool(torch.isfinite(t).all()) for t in got)
        d, c1, c2 = _chains(B, N, K, 128)
        ref = X.backward(x, W, c, a, g_lp, None, bf16=dtype == "bf16", d=d, c1=c1, c2=c2)
        # the planted row against the bound; the true values elsewhere (about e^-200) lie below fp32's range, where the bound's
        # relative model does not apply: they must come out as (almost) nothing
        assert abs(ref["dc"][j]) < 1e-60 and abs(float(got[4][j])) <= ref["tol_dc"][j]
        assert bool((got[3][j].double().abs().numpy() <= ref["tol_dW"][j]).all())
        worst = max(worst, abs(float(got[4][j])) / ref["tol_dc"][j], float((got[3][j].double().abs().numpy() / ref["tol_dW"][j]).max()))
        rest = torch.arange(N) != j
        assert float(got[4][rest].abs().max()) <= 1e-30 and float(got[3][rest].abs().max()) <= 1e-30 and bool((got[2] == 0).all())
    print(f"planted B={B} N={N} K={K} {dtype}: worst error / tolerance at the planted row = {worst:.3f}")


@pytest.mark.parametrize("B,N,K", X.SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_lse_gradient_only(F, cuda, B, N, K, dtype):
    """g_lse only: D = g_lse p, every row of D sums to g_lse, hence sum_n dc_n = sum_b g_lse_b to the bound."""
    x, W, c, a, _, g_lse = _gauss(B, N, K, seed=3)
    worst = 0.0
    for ips in SLICINGS:
        got = _run(F, cuda, x, W, c, a, None, g_lse, dtype, ips)
        d, c1, c2 = _chains(B, N, K, ips)
        ref = X.backward(x, W, c, a, None, g_lse, bf16=dtype == "bf16", d=d, c1=c1, c2=c2)
        worst = max(worst, _check(got, ref, (ips,)))
        total, want = float(got[4].double().sum()), float(g_lse.double().sum())
        assert abs(ref["dc"].sum() - want) <= 1e-10 * max(1.0, float(g_lse.abs().sum()))
        assert abs(total - want) <= ref["tol_dc"].sum() + 1e-10 * float(g_lse.abs().sum())
    print(f"lse only B={B} N={N} K={K} {dtype}: worst error / tolerance = {worst:.3f}")


@pytest.mark.parametrize("B,N,K,ips", [(129, 200, 128, 128), (200, 1000, 160, 128), (200, 1000, 160, 256), (300, 1500, 256, 256)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_independence(F, cuda, B, N, K, ips, dtype):
    """With items_per_slice fixed: the rows of dx have the same bits in the reversed batch and for a row alone."""
    x, W, c, a, g_lp, g_lse = _gauss(B, N, K, seed=4)
    base = _run(F, cuda, x, W, c, a, g_lp, g_lse, dtype, ips, need=(True, False, False))[2]
    rev = _run(F, cuda, x.flip(0), W, c, a.flip(0), g_lp.flip(0), g_lse.flip(0), dtype, ips, need=(True, False, False))[2]
    assert _bits_equal(rev.flip(0), base)
    for b in (0, 1, 63, 127, 128, B - 1):
        alone = _run(F, cuda, x[b:b + 1], W, c, a[b:b + 1], g_lp[b:b + 1], g_lse[b:b + 1], dtype, ips, need=(True, False, False))[2]
        assert _bits_equal(alone, base[b:b + 1]), b


@pytest.mark.parametrize("dtype", DTYPES)
def test_invalid_and_ignored_rows(F, cuda, dtype):
    """An action outside [0, N): NaN in that row's log_prob only, its g_lp counts as 0 (the row's dx has the bits of the call with
    g_lp = 0 there), every other row's dx bits are those of the clean call, and no gradient holds a NaN -- also when the upstream
    g_lp of that row is NaN.  ignore_index rows of catalogue_cross_entropy: zero loss, zero dx, the other rows' bits unchanged."""
    B, N, K = 200, 1000, 160
    x, W, c, a, g_lp, g_lse = _gauss(B, N, K, seed=5)
    clean = _run(F, cuda, x, W, c, a, g_lp, g_lse, dtype, 256)
    bad, hit = a.clone(), torch.zeros(B, dtype=torch.bool)
    bad[0], bad[64], bad[129], bad[77] = -1, N, N + 5, -(2 ** 40)
    hit[[0, 64, 129, 77]] = True
    g_nan = g_lp.clone()
    g_nan[64] = float("nan")
    got = _run(F, cuda, x, W, c, bad, g_nan, g_lse, dtype, 256)
    assert bool(torch.isnan(got[0][hit]).all()) and _bits_equal(got[0][~hit], clean[0][~hit]) and _bits_equal(got[1], clean[1])
    assert all(bool(torch.isfinite(t).all()) for t in got[2:])
    assert _bits_equal(got[2][~hit], clean[2][~hit])
    zeroed = _run(F, cuda, x, W, c, a, torch.where(hit, torch.zeros(B), g_lp), g_lse, dtype, 256)
    assert _bits_equal(got[2][hit], zeroed[2][hit])
    d, c1, c2 = _chains(B, N, K, 256)
    ref = X.backward(x, W, c, bad, g_lp, g_lse, bf16=dtype == "bf16", d=d, c1=c1, c2=c2)
    _check(got, ref, "invalid")

    def xent(targets, **kw):
        xd, Wd, cd = x.to(cuda).requires_grad_(True), W.to(cuda).requires_grad_(True), c.to(cuda).requires_grad_(True)
        loss = F.catalogue_cross_entropy(xd, Wd, cd, targets.to(cuda), dtype=dtype, **kw)
        loss.sum().backward()
        return loss.detach().cpu(), xd.grad.cpu(), Wd.grad.cpu(), cd.grad.cpu()
    full = xent(a, reduction="none")
    ign = a.clone()
    ign[hit] = -100
    part = xent(ign, reduction="none")
    assert bool((part[0][hit] == 0).all()) and _bits_equal(part[0][~hit], full[0][~hit])
    assert bool((part[1][hit] == 0).all()) and _bits_equal(part[1][~hit], full[1][~hit])
    assert all(bool(torch.isfinite(t).all()) for t in part)
    # mean leaves the ignored rows out; sum is the sum; a custom ignore_index inside [0, N) works; any other bad id raises
    mean, total = xent(ign, reduction="mean")[0], xent(ign, reduction="sum")[0]
    assert float(total) == pytest.approx(float(part[0].double().sum()), rel=1e-5)
    assert float(mean) == pytest.approx(float(part[0].double().sum()) / int((~hit).sum()), rel=1e-5)
    ign7 = torch.where(hit, torch.full_like(a, 7), a)
    keep7 = ign7 != 7
    own = xent(ign7, reduction="none", ignore_index=7)
    assert bool((own[0][~keep7] == 0).all()) and _bits_equal(own[0][keep7], full[0][keep7])
    with pytest.raises(ValueError, match="outside"):
        xent(bad, reduction="mean")
    # torch's own cross_entropy agrees (fp32: 1e-4 relative on the mean is far above either route's error)
    if dtype == "fp32":
        want = torch.nn.functional.cross_entropy(torch.addmm(c, x, W.T), ign, ignore_index=-100)
        assert float(mean) == pytest.approx(float(want), rel=1e-4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_needs_input_grad(F, cuda, dtype):
    """Frozen weight, frozen x, bias=None: the gradients that are asked for have the bits of the full call, the others are None."""
    B, N, K = 129, 200, 128
    x, W, c, a, g_lp, g_lse = _gauss(B, N, K, seed=6)
    full = _run(F, cuda, x, W, c, a, g_lp, g_lse, dtype, 128)
    for need in ((True, False, False), (False, True, True), (False, True, False), (False, False, True), (True, True, False)):
        got = _run(F, cuda, x, W, c, a, g_lp, g_lse, dtype, 128, need=need)
        for i, on in enumerate(need):
            assert (got[2 + i] is not None and _bits_equal(got[2 + i], full[2 + i])) if on else got[2 + i] is None, (need, i)
    nobias = _run(F, cuda, x, W, None, a, g_lp, g_lse, dtype, 128)
    zero = _run(F, cuda, x, W, torch.zeros(N), a, g_lp, g_lse, dtype, 128)
    assert nobias[4] is None and all(_bits_equal(p, q) for p, q in zip(nobias[:4], zero[:4]))
    # nothing requires grad: no graph
    lp, _ = F.catalogue_log_prob_train(x.to(cuda), W.to(cuda), c.to(cuda), a.to(cuda), dtype=dtype)
    assert not lp.requires_grad


def test_refusals(F, cuda):
    from recnn_amd import _lib as L
    x, W, c, a, _, _ = _gauss(4, 10, 320)
    with pytest.raises(ValueError, match="256"):
        F.catalogue_log_prob_train(x.to(cuda), W.to(cuda), c.to(cuda), a.to(cuda))
    with pytest.raises(ValueError, match="256"):
        F.catalogue_cross_entropy(x.to(cuda), W.to(cuda), c.to(cuda), a.to(cuda))
    with pytest.raises(L.RecnnHipError, match="256"):
        lse = torch.zeros(4, device=cuda)
        out = torch.zeros(4, 320, device=cuda)
        L.call("recnn_catalogue_logprob_bwd", L.ptr(x.to(cuda)), 320, 4, 320, L.ptr(W.to(cuda)), 320, 0, L.ptr(c.to(cuda)), 10,
               L.ptr(a.to(cuda)), L.ptr(lse), L.ptr(lse), None, 128, L.ptr(out), 320, None, 320, None, L.ptr(out), L.current_stream())
    x, W, c, a, _, _ = _gauss(4, 10, 64)
    for args in ((x, W.to(cuda), c.to(cuda), a), (x.to(cuda), W, c, a)):
        with pytest.raises(L.RecnnHipError):
            F.catalogue_log_prob_train(*args)
        with pytest.raises(L.RecnnHipError):
            F.catalogue_cross_entropy(*args)
    with pytest.raises(L.RecnnHipError):
        F.catalogue_log_prob_train(x.to(cuda).requires_grad_(True), W.to(cuda), c.to(cuda), a.to(cuda), items_per_slice=100)


@pytest.mark.parametrize("dtype", DTYPES)
def test_operands_as_they_come(F, cuda, dtype):
    """x as a column slice of a wider tensor, a weight that is a view at an unaligned offset, K = 70 and N = 263 (padded inside):
    forward and gradients have the bits of the plain padded call, and the shapes of the operands."""
    B, N = 65, 263
    x, W, c, a, g_lp, g_lse = _gauss(B, N, 64, seed=7)
    base = _run(F, cuda, x, W, c, a, g_lp, g_lse, dtype, 128)
    wide = torch.randn(B, 192).to(cuda)
    wide[:, 64:128] = x.to(cuda)
    wide.requires_grad_(True)
    flat = torch.zeros(N * 64 + 1, device=cuda)
    flat[1:].view(N, 64).copy_(W)
    flat.requires_grad_(True)
    view = flat[1:].view(N, 64)
    assert view.data_ptr() % 16 != 0
    cd = c.to(cuda).requires_grad_(True)
    lp, lse = F.catalogue_log_prob_train(wide[:, 64:128], view, cd, a.to(cuda), dtype=dtype, items_per_slice=128)
    torch.autograd.backward([lp, lse], [g_lp.to(cuda), g_lse.to(cuda)])
    assert _bits_equal(lp.detach().cpu(), base[0]) and _bits_equal(lse.detach().cpu(), base[1])
    gw = wide.grad.cpu()
    assert _bits_equal(gw[:, 64:128], base[2]) and bool((gw[:, :64] == 0).all()) and bool((gw[:, 128:] == 0).all())
    assert _bits_equal(flat.grad[1:].view(N, 64).cpu(), base[3]) and float(flat.grad[0]) == 0.0 and _bits_equal(cd.grad.cpu(), base[4])
    x, W, c, a, g_lp, g_lse = _gauss(B, N, 70, seed=8)
    xp, Wp = torch.zeros(B, 128), torch.zeros(N, 128)
    xp[:, :70], Wp[:, :70] = x, W
    got, want = _run(F, cuda, x, W, c, a, g_lp, g_lse, dtype, 256), _run(F, cuda, xp, Wp, c, a, g_lp, g_lse, dtype, 256)
    assert got[2].shape == (B, 70) and got[3].shape == (N, 70)
    assert _bits_equal(got[2], want[2][:, :70]) and _bits_equal(got[3], want[3][:, :70]) and _bits_equal(got[4], want[4])
    assert bool((want[2][:, 70:] == 0).all()) and bool((want[3][:, 70:] == 0).all())


def test_empty_batch(F, cuda):
    """B = 0 launches nothing: empty dx, zero dW and dc."""
    W, c = torch.randn(200, 64).to(cuda).requires_grad_(True), torch.randn(200).to(cuda).requires_grad_(True)
    x = torch.zeros(0, 64, device=cuda, requires_grad=True)
    lp, lse = F.catalogue_log_prob_train(x, W, c, torch.zeros(0, dtype=torch.int64, device=cuda))
    (lp.sum() + lse.sum()).backward()
    assert x.grad.shape == (0, 64) and bool((W.grad == 0).all()) and bool((c.grad == 0).all())


def test_memory_stays_far_below_one_logits_matrix(F, cuda):
    """B = 2048, N = 20000, K = 128, fp32 (aligned: nothing is padded): during forward + backward the peak allocated memory rises by
    less than the three gradients plus a quarter of one B x N fp32 matrix (the dx partials, 16 slices of [B, K], are a tenth of it)."""
    B, N, K = 2048, 20000, 128
    x, W, c, a, _, _ = (t.to(cuda) if torch.is_tensor(t) else t for t in _gauss(B, N, K, seed=9))
    x.requires_grad_(True), W.requires_grad_(True), c.requires_grad_(True)
    F.catalogue_cross_entropy(x, W, c, a).backward()
    x.grad = W.grad = c.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    F.catalogue_cross_entropy(x, W, c, a).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - start
    grads = (B * K + N * K + N) * 4
    print(f"memory: peak rise {rise} bytes, gradients {grads}, one B x N fp32 matrix {B * N * 4}")
    assert rise < grads + B * N * 4 / 4


# ------------------------------------------------------------------------------------------------------------ end to end

def _seq_env(cuda):
    """The sequence tests' smallest data (seq_reference.seq_env_data: 12 users, 50 items; E = 16, the smallest hidden width the GRU kernels take)
    as CSR arrays, a GRU with H = E."""
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
    return env, user_dict, gru


def test_target_items(cuda):
    env, user_dict, _ = _seq_env(cuda)
    ids, steps = [0, 1, 2, 3, 4], [3, 4, 9, 30]
    batch = env.user_batch(ids, steps)
    got = env.target_items(batch).cpu()
    want = torch.tensor([int(user_dict[u]["items"][t]) for t in steps for u in ids])
    assert got.dtype == torch.int64 and torch.equal(got, want)
    assert torch.equal(batch["action"].cpu(), env.table.cpu()[want])
    batch["meta"]["step"] = steps[:-1]
    with pytest.raises(ValueError, match="rows"):
        env.target_items(batch)


def test_tied_table_gradient_and_training(cuda):
    """GRU with H = E and the table P as both the encoder's embeddings and the head's weights: after one backward, P.grad is the
    head-only gradient plus the encoder-only gradient (each obtained by detaching the other path) to one fp32 add per element; 20
    next_item_update Adam steps on one fixed batch lower the loss."""
    import recnn_amd
    env, _, gru = _seq_env(cuda)
    ids, steps = [0, 1, 2, 3, 4], [3, 4, 9, 30]
    P = env.table.clone().requires_grad_(True)
    head = recnn_amd.nn.NextItemHead(P)
    assert head.n_items == P.shape[0] and head.weight is P

    def grad_of(tie_head, tie_encoder):
        P.grad = None
        batch = env.user_batch(ids, steps, table=P)
        state = batch["state"] if tie_encoder else batch["state"].detach()
        h = head if tie_head else recnn_amd.nn.NextItemHead(P.detach())
        loss = h.loss(state, env.target_items(batch))
        loss.backward()
        return P.grad.clone(), float(loss.detach())
    both, l0 = grad_of(True, True)
    g_head, l1 = grad_of(True, False)
    g_enc, l2 = grad_of(False, True)
    assert l0 == l1 == l2 and float(g_head.abs().max()) > 0 and float(g_enc.abs().max()) > 0
    want = g_head.double() + g_enc.double()
    assert bool(((both.double() - want).abs() <= 2.0 ** -24 * want.abs() + 1e-45).all())

    with pytest.raises(ValueError, match="bias"):
        recnn_amd.nn.NextItemHead(P, torch.zeros(P.shape[0], device=cuda)).index()
    lp = head.log_prob(env.user_batch(ids, steps)["state"].detach(), env.target_items(env.user_batch(ids, steps)))[0]
    assert not lp.requires_grad and lp.shape == (20,)

    P.grad = None
    opt = torch.optim.Adam([P] + list(gru.parameters()), lr=1e-2)
    nets, optimizer = {"head": head}, {"optimizer": opt}
    losses = []
    for step in range(20):
        batch = env.user_batch(ids, steps, table=P)
        batch["target"] = env.target_items(batch)
        out = recnn_amd.nn.next_item_update(batch, {}, nets, optimizer, learn=True, step=step)
        assert out["step"] == step
        losses.append(float(out["loss"]))
    batch = env.user_batch(ids, steps, table=P)
    batch["target"] = env.target_items(batch)
    before = P.detach().clone()
    final = float(recnn_amd.nn.next_item_update(batch, {}, nets, optimizer, learn=False)["loss"])
    assert torch.equal(P.detach(), before)
    print(f"next_item_update: loss {losses[0]:.4f} -> {final:.4f}")
    assert all(math.isfinite(v) for v in losses) and final < losses[0] - 0.1
    # a projection in front of the head is applied and trained
    proj = torch.nn.Linear(P.shape[1], P.shape[1]).to(cuda)
    opt2 = torch.optim.Adam(proj.parameters(), lr=1e-2)
    w0 = proj.weight.detach().clone()
    recnn_amd.nn.next_item_update(batch, {}, {"head": head, "proj": proj}, {"optimizer": opt2}, learn=True, step=0)
    assert not torch.equal(proj.weight.detach(), w0)
