"""GPU: the fused catalogue log-prob (csrc/logprob.hip), the off-policy accumulators (csrc/ope.hip), DiscreteActor.log_prob /
Beta.log_prob and recnn_amd.ope, against tests/ope_reference.py (float64; the bound and its derivation are stated there).

Measured on an MI355X, worst |error| / allowed over every case: uniform 0.045, Gaussian 0.019 (fp32) / 0.017 (bf16), meter
readouts 0.59 (n = 1, top_k = 16); DESIGN.md section 26."""
import math

import numpy as np
import pytest
import torch

import ope_reference as R

pytestmark = pytest.mark.gpu

BS = (1, 63, 64, 65, 130)
KN = ((64, 1), (64, 63), (64, 64), (64, 65), (192, 200), (64, 1000), (1344, 130))
DTYPES = ("fp32", "bf16")
U = R.U


@pytest.fixture(scope="module")
def F(cuda):
    from recnn_amd.nn import functional
    return functional


def _slicings(N):
    """default, one tile, two tiles, all of N"""
    return (None, R.TILE, 2 * R.TILE, (N + R.TILE - 1) // R.TILE * R.TILE)


def _ips(B, N, ips):
    return R.default_items_per_slice(B, N) if ips is None else ips


def _run(F, cuda, x, W, c, a, dtype, ips):
    lp, lse = F.catalogue_log_prob(x.to(cuda), W.to(cuda), c.to(cuda), a.to(cuda), dtype=dtype, items_per_slice=ips)
    assert lp.dtype == torch.float32 and lp.shape == (x.shape[0],) and lse.shape == lp.shape and not lp.requires_grad
    return lp.cpu().numpy(), lse.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _gauss(B, K, N, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + K * 1000 + N)
    x = torch.randn(B, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    c = torch.randn(N, generator=g)
    a = torch.randint(0, N, (B,), generator=g)
    return x, W, c, a


@pytest.mark.parametrize("K,N", KN)
@pytest.mark.parametrize("dtype", DTYPES)
def test_uniform(F, cuda, K, N, dtype):
    """x = 0, c = 0: every logit is 0, logprob = -ln N within R_b (E_b = 0); N = 1 gives exactly 0.  A dropped or double-counted
    item moves this by about 1 / N."""
    worst = 0.0
    for B in BS:
        _, W, _, a = _gauss(B, K, N)
        x, c = torch.zeros(B, K), torch.zeros(N)
        for ips in _slicings(N):
            lp, lse = _run(F, cuda, x, W, c, a, dtype, ips)
            if N == 1:
                assert (lp == 0).all() and (lse == 0).all()
                continue
            want = -math.log(N)
            d = R.chain_depth(N, _ips(B, N, ips))
            tol = R.allowed(np.zeros(B), np.full(B, want), np.full(B, -want), N, d)
            worst = max(worst, float((np.abs(lp - want) / tol).max()), float((np.abs(lse + want) / tol).max()))
            assert (np.abs(lp - want) <= tol).all() and (np.abs(lse + want) <= tol).all(), (B, ips, lp[:4], want)
    print(f"uniform K={K} N={N} {dtype}: worst error / allowed = {worst:.3f}")


@pytest.mark.parametrize("K,N", KN)
@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_item(F, cuda, K, N, dtype):
    """x = 0, c = -200 except c_j = 0: logprob(a = j) in [-1e-6, 0]; logprob(a != j) = -200 within 800 u, finite, not clamped."""
    for B in BS:
        _, W, _, _ = _gauss(B, K, N)
        x = torch.zeros(B, K)
        for j in sorted({j for j in (0, 63, 64, 127, 128, N - 1) if 0 <= j < N}):
            c = torch.full((N,), -200.0)
            c[j] = 0.0
            rows = torch.arange(B)
            other = (j + 1 + rows) % N
            a = torch.where((rows % 2 == 0) | (other == j), torch.full((B,), j), other)
            for ips in _slicings(N):
                lp, _ = _run(F, cuda, x, W, c, a, dtype, ips)
                at = (a == j).numpy()
                assert ((lp[at] >= -1e-6) & (lp[at] <= 0)).all(), (B, j, ips, lp[at][:4])
                assert np.isfinite(lp).all() and (np.abs(lp[~at] + 200.0) <= 800 * U).all(), (B, j, ips, lp[~at][:4])


def _gauss_variants(B, K, N):
    x, W, c, a = _gauss(B, K, N, seed=1)
    yield "plain", x, W, c, a
    yield "x6", x * 6, W, c * 6, a
    # one logit of every row at +80 and one at -80 (items p and q: their W rows are zero, the bias carries the value); the action is
    # the maximum in even rows, the -80 item in odd rows (logprob ~ -160), where N has room for both
    W2, c2, a2 = W.clone(), c.clone(), a.clone()
    p, q = (N // 3) % N, (N // 3 + 1 + N // 2) % N
    W2[p], c2[p] = 0.0, 80.0
    a2[0::2] = p
    if q != p:
        W2[q], c2[q] = 0.0, -80.0
        a2[1::2] = q
    yield "pushed", x, W2, c2, a2


@pytest.mark.parametrize("K,N", KN)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gaussian_against_float64(F, cuda, K, N, dtype):
    worst = 0.0
    for B in BS:
        for name, x, W, c, a in _gauss_variants(B, K, N):
            ref_lp, ref_lse, E = R.log_prob(x, W, c, a, bf16=dtype == "bf16")
            for ips in _slicings(N):
                lp, lse = _run(F, cuda, x, W, c, a, dtype, ips)
                tol = R.allowed(E, ref_lp, ref_lse, N, R.chain_depth(N, _ips(B, N, ips)))
                assert np.isfinite(lp).all() and (lp <= 0).all(), (name, B, ips)
                worst = max(worst, float((np.abs(lp - ref_lp) / tol).max()), float((np.abs(lse - ref_lse) / tol).max()))
                assert (np.abs(lp - ref_lp) <= tol).all(), (name, B, ips, float((np.abs(lp - ref_lp) / tol).max()))
                assert (np.abs(lse - ref_lse) <= tol).all(), (name, B, ips, float((np.abs(lse - ref_lse) / tol).max()))
            if name == "pushed" and N >= 3 and B >= 2:
                assert (ref_lp[1::2] < -150).all() and (ref_lp[0::2] > -1e-3).all()
    print(f"gaussian K={K} N={N} {dtype}: worst error / allowed = {worst:.3f}")


@pytest.mark.parametrize("K,N,ips", [(192, 200, 128), (64, 1000, 128), (64, 1000, 256), (1344, 130, 128)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_independence(F, cuda, K, N, ips, dtype):
    """With items_per_slice fixed: the 130-row call, the same rows reversed and every row alone give equal bits per row; the same
    call twice gives equal bits."""
    B = 130
    x, W, c, a = _gauss(B, K, N, seed=2)
    xd, Wd, cd, ad = (t.to(cuda) for t in (x, W, c, a))
    lp, lse = F.catalogue_log_prob(xd, Wd, cd, ad, dtype=dtype, items_per_slice=ips)
    lp2, lse2 = F.catalogue_log_prob(xd, Wd, cd, ad, dtype=dtype, items_per_slice=ips)
    assert torch.equal(lp.view(torch.int32), lp2.view(torch.int32)) and torch.equal(lse.view(torch.int32), lse2.view(torch.int32))
    rlp, rlse = F.catalogue_log_prob(xd.flip(0), Wd, cd, ad.flip(0), dtype=dtype, items_per_slice=ips)
    assert torch.equal(rlp.flip(0).view(torch.int32), lp.view(torch.int32))
    assert torch.equal(rlse.flip(0).view(torch.int32), lse.view(torch.int32))
    alone = [F.catalogue_log_prob(xd[b:b + 1], Wd, cd, ad[b:b + 1], dtype=dtype, items_per_slice=ips) for b in range(B)]
    assert torch.equal(torch.cat([t[0] for t in alone]).view(torch.int32), lp.view(torch.int32))
    assert torch.equal(torch.cat([t[1] for t in alone]).view(torch.int32), lse.view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_invalid_actions(F, cuda, dtype):
    """Actions -1, N and N + 5 give NaN in their rows; every other row, and every lse, has the bits of the call without them."""
    for K, N in ((64, 65), (192, 200)):
        for ips in _slicings(N):
            x, W, c, a = _gauss(130, K, N, seed=3)
            lp, lse = _run(F, cuda, x, W, c, a, dtype, ips)
            bad = a.clone()
            bad[0], bad[64], bad[129], bad[77] = -1, N, N + 5, -(2 ** 40)
            blp, blse = _run(F, cuda, x, W, c, bad, dtype, ips)
            hit = (bad != a).numpy()
            assert hit.sum() == 4 and np.isnan(blp[hit]).all()
            assert (_bits(blp[~hit]) == _bits(lp[~hit])).all() and (_bits(blse) == _bits(lse)).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_layouts(F, cuda, dtype):
    """x as a column slice of a wider tensor, a hidden width of 70 (padded inside) and N not a multiple of 4 give the bits of the
    padded contiguous call."""
    B, N = 65, 263
    x, W, c, a = _gauss(B, 64, N, seed=4)
    base = _run(F, cuda, x, W, c, a, dtype, 128)
    wide = torch.randn(B, 192)
    wide[:, 64:128] = x
    got = F.catalogue_log_prob(wide.to(cuda)[:, 64:128], W.to(cuda), c.to(cuda), a.to(cuda), dtype=dtype, items_per_slice=128)
    assert (_bits(got[0].cpu().numpy()) == _bits(base[0])).all() and (_bits(got[1].cpu().numpy()) == _bits(base[1])).all()
    x, W, c, a = _gauss(B, 70, N, seed=5)
    xp, Wp = torch.zeros(B, 128), torch.zeros(N, 128)
    xp[:, :70], Wp[:, :70] = x, W
    for ips in (128, 256):
        got, want = _run(F, cuda, x, W, c, a, dtype, ips), _run(F, cuda, xp, Wp, c, a, dtype, ips)
        assert (_bits(got[0]) == _bits(want[0])).all() and (_bits(got[1]) == _bits(want[1])).all()
    ref_lp, ref_lse, E = R.log_prob(x, W, c, a, bf16=dtype == "bf16")
    assert (np.abs(got[0] - ref_lp) <= R.allowed(E, ref_lp, ref_lse, N, R.chain_depth(N, 256))).all()


def test_bad_arguments(F, cuda):
    from recnn_amd import _lib as L
    x, W, c, a = (t.to(cuda) for t in _gauss(4, 64, 10))
    with pytest.raises(L.RecnnHipError):
        F.catalogue_log_prob(x, W, c, a, items_per_slice=100)
    with pytest.raises(ValueError):
        F.catalogue_log_prob(x, W[:, :32], c, a)
    with pytest.raises(ValueError):
        F.catalogue_log_prob(x, W, c, a, dtype="fp16")
    with pytest.raises(L.RecnnHipError):
        F.catalogue_log_prob(x.cpu(), W, c, a)
    with pytest.raises(ValueError):
        F.catalogue_log_prob(x, W, c[:5], a)
    with pytest.raises(ValueError):
        F.action_ids(torch.zeros(4, device=cuda))
    assert torch.equal(F.action_ids(a[:, None]), a)


@pytest.mark.parametrize("dtype", DTYPES)
def test_operands_as_they_come(F, cuda, dtype):
    """A weight that is a view at an unaligned offset gives the bits of the plain call."""
    B, K, N = 65, 64, 200
    x, W, c, a = (t.to(cuda) for t in _gauss(B, K, N, seed=7))
    want = F.catalogue_log_prob(x, W, c, a, dtype=dtype, items_per_slice=128)
    flat = torch.zeros(N * K + 1, device=cuda)
    view = flat[1:].view(N, K)
    view.copy_(W)
    assert view.data_ptr() % 16 != 0
    got = F.catalogue_log_prob(x, view, c, a, dtype=dtype, items_per_slice=128)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ modules

def _hidden64(actor, state):
    """float64 hidden layer of a DiscreteActor and a bound on what the fp32 GEMM kernel's differs from it by:
    gamma_{K+2} (sum_k |x_k w_k| + |b|) for the accumulation and the bias, u |h| for nothing more than safety."""
    x = state.double().numpy()
    w1, b1 = actor.linear1.weight.detach().cpu().double().numpy(), actor.linear1.bias.detach().cpu().double().numpy()
    h = np.maximum(x @ w1.T + b1, 0.0)
    dh = R.gamma(x.shape[1] + 2) * (np.abs(x) @ np.abs(w1).T + np.abs(b1)) + U * h
    return h, dh


@pytest.mark.parametrize("dtype", DTYPES)
def test_modules(F, cuda, dtype):
    import recnn_amd
    torch.manual_seed(0)
    N, B = 200, 65
    actor = recnn_amd.nn.DiscreteActor(70, N, 64).to(cuda)
    beta = recnn_amd.nn.Beta(70, N).to(cuda)
    state = torch.randn(B, 70)
    ids = torch.randint(0, N, (B,))
    ids[:3] = torch.tensor([0, N - 1, 64])
    before = {k: v.clone() for m in (actor, beta) for k, v in m.state_dict().items()}
    versions = [p._version for m in (actor, beta) for p in m.parameters()]
    actor.forced_actions.append(torch.zeros(B, dtype=torch.int64))
    actor.saved_log_probs.append("kept")
    F.set_catalogue_dtype(dtype)
    try:
        sd, idd = state.to(cuda), ids.to(cuda)
        onehot = F.onehot_rows(idd, N)
        dense = torch.zeros(B, N, device=cuda)
        dense[torch.arange(B), idd] = 1.0
        for net in (actor, beta):
            a = net.log_prob(sd, idd)
            for enc in (onehot, dense):
                b = net.log_prob(sd, enc)
                assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        lp_pi, lp_beta = actor.log_prob(sd, idd)[0].cpu().numpy(), beta.log_prob(sd, idd)[0].cpu().numpy()
    finally:
        F.set_catalogue_dtype("fp32")
    bf16 = dtype == "bf16"
    d = R.chain_depth(N, R.default_items_per_slice(B, N))
    # Beta: one catalogue product over the state
    lin = beta.net[0]
    ref, lse, E = R.log_prob(state, lin.weight.detach().cpu(), lin.bias.detach().cpu(), ids, bf16=bf16)
    assert (np.abs(lp_beta - ref) <= R.allowed(E, ref, lse, N, d)).all()
    # DiscreteActor: the head over the hidden layer; the hidden layer's own error dh (and, in bf16 mode, its rounding to bf16,
    # 2^-9 |h|, which the reference does not replay) reaches a logit as sum_k dh_k |W_nk|, twice (picked logit and lse)
    h, dh = _hidden64(actor, state)
    w2, b2 = actor.linear2.weight.detach().cpu(), actor.linear2.bias.detach().cpu()
    w2r = R.to_bf16(w2) if bf16 else w2.double().numpy()
    if bf16:
        dh = dh + 2.0 ** -9 * h
    ref, lse, E = R.log_prob(h, w2r, b2, ids)
    extra = 2.0 * (dh @ np.abs(w2r).T).max(1)
    assert (np.abs(lp_pi - ref) <= R.allowed(E, ref, lse, N, d) + extra).all()
    # nothing was touched
    after = {k: v for m in (actor, beta) for k, v in m.state_dict().items()}
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert versions == [p._version for m in (actor, beta) for p in m.parameters()]
    assert beta.optim is None and beta.last_loss is None
    assert len(actor.forced_actions) == 1 and actor.saved_log_probs == ["kept"] and not actor.rewards and not actor.correction


# -------------------------------------------------------------------------------------------------------------------- meter

def _logged(n, seed, nan_rows=()):
    rng = np.random.default_rng(seed)
    lp_pi = -rng.uniform(0.0, 9.0, size=n).astype(np.float32)
    lp_beta = (lp_pi + rng.normal(scale=1.0, size=n)).clip(max=0).astype(np.float32)
    r = rng.normal(size=n).astype(np.float32)
    q = (r + rng.normal(scale=0.3, size=n)).astype(np.float32)
    v = rng.normal(size=n).astype(np.float32)
    mask = (rng.uniform(size=n) < 0.8).astype(np.uint8)
    for i, k in enumerate(nan_rows):
        (lp_pi if i % 2 else lp_beta)[k % n] = np.nan
    return lp_pi, lp_beta, r, mask, q, v


def _check_meter(m, ref):
    """Counts equal; every readout within the tolerance the reference derives for it.  Returns the worst error / tolerance."""
    want = ref.readouts()
    for k in ("rows", "invalid", "capped_share"):
        assert getattr(m, k) == want[k][0], k
    worst = 0.0
    for k, (val, tol) in want.items():
        if k in ("rows", "invalid", "capped_share"):
            continue
        err = abs(getattr(m, k) - val)
        worst = max(worst, err / tol if tol else 0.0)
        assert err <= tol, (k, getattr(m, k), val, tol)
    return worst


@pytest.mark.parametrize("n", (1, 255, 256, 257, 1025, 4097))
def test_meter(cuda, n):
    from recnn_amd.ope import OffPolicyMeter
    worst = 0.0
    for cap in (math.inf, 5.0, 0.5):
        for top_k in (0, 1, 16):
            m, ref = OffPolicyMeter(cap=cap, top_k=top_k, device=cuda), R.Meter(cap=cap, top_k=top_k)
            for use_mask, use_dm in ((False, False), (True, True)):
                m.reset()
                ref.reset()
                for batch in range(3):
                    nan_rows = (3, 17, 200) if (batch == 1 and n > 1) else ()
                    lp_pi, lp_beta, r, mask, q, v = _logged(n, 100 * n + batch, nan_rows)
                    kw = {}
                    if use_mask:
                        kw["mask"] = mask
                    if use_dm:
                        kw["q_logged"], kw["v_dm"] = q, v
                    ref.update(lp_pi, lp_beta, r, **kw)
                    m.update(torch.from_numpy(lp_pi).to(cuda), torch.from_numpy(lp_beta).to(cuda), torch.from_numpy(r).to(cuda),
                             **{k: torch.from_numpy(t).to(cuda) for k, t in kw.items()})
                if ref.rows == 0:
                    assert m.rows == 0
                    continue
                worst = max(worst, _check_meter(m, ref))
                if not use_mask and n > 1:
                    assert m.invalid == min(3, len({3 % n, 17 % n, 200 % n}))
    print(f"meter n={n}: worst error / allowed = {worst:.3f}")


def test_meter_top_k_1_is_plain_and_calls_repeat(cuda):
    from recnn_amd.ope import OffPolicyMeter
    lp_pi, lp_beta, r, mask, q, v = (torch.from_numpy(t).to(cuda) for t in _logged(4097, 5, (3, 9)))

    def run(top_k):
        m = OffPolicyMeter(cap=2.0, top_k=top_k, device=cuda)
        for _ in range(3):
            m.update(lp_pi, lp_beta, r, mask=mask, q_logged=q, v_dm=v)
        return m.sums.cpu().numpy().view(np.uint64).tolist(), m.counts.tolist()
    assert run(0) == run(1) == run(1)
    assert run(16) == run(16) and run(16) != run(0)


def test_meter_reset_and_errors(cuda):
    from recnn_amd.ope import OffPolicyMeter
    lp_pi, lp_beta, r, mask, q, v = (torch.from_numpy(t).to(cuda) for t in _logged(300, 6))
    m = OffPolicyMeter(device=cuda)
    with pytest.raises(ValueError):
        m.ips
    assert m.rows == 0
    m.update(lp_pi, lp_beta, r, mask=torch.zeros(300, device=cuda))
    with pytest.raises(ValueError):
        m.snips
    m.update(lp_pi, lp_beta, r)
    first = (m.ips, m.snips, m.ess, m.rows)
    with pytest.raises(ValueError):
        m.dr
    with pytest.raises(ValueError):
        m.update(lp_pi, lp_beta, r, q_logged=q, v_dm=v)
    with pytest.raises(ValueError):
        m.update(lp_pi, lp_beta, r, q_logged=q)
    with pytest.raises(ValueError):
        m.update(lp_pi, lp_beta[:10], r)
    assert (m.ips, m.snips, m.ess, m.rows) == first
    m.reset()
    assert m.rows == 0 and m.invalid == 0
    m.update(lp_pi, lp_beta, r, q_logged=q, v_dm=v)
    assert (m.ips, m.snips, m.ess, m.rows) == first and math.isfinite(m.dr)
    with pytest.raises(ValueError):
        m.update(lp_pi, lp_beta, r)
    with pytest.raises(ValueError):
        OffPolicyMeter(cap=0.0, device=cuda)
    with pytest.raises(ValueError):
        OffPolicyMeter(top_k=-1, device=cuda)


# ---------------------------------------------------------------------------------------------------------- evaluate_policy

def test_evaluate_policy(F, cuda):
    import recnn_amd
    from recnn_amd.ope import OffPolicyMeter, evaluate_policy
    torch.manual_seed(1)
    N = 200
    actor = recnn_amd.nn.DiscreteActor(70, N, 64).to(cuda)
    beta = recnn_amd.nn.Beta(70, N).to(cuda)
    g = torch.Generator().manual_seed(2)
    batches = []
    for B in (130, 64, 7):
        ids = torch.randint(0, N, (B,), generator=g).to(cuda)
        batches.append({"state": torch.randn(B, 70, generator=g).to(cuda), "action": F.onehot_rows(ids, N),
                        "reward": torch.randn(B, generator=g).to(cuda), "ids": ids})
    m = evaluate_policy(actor, beta, batches, cap=3.0, top_k=2)
    assert isinstance(m, OffPolicyMeter) and m.rows == 201 and m.invalid == 0
    # the same by hand: bit for bit; and the reference meter over the GPU's log-probs and over float64 ones
    by_hand, ref, ref64 = OffPolicyMeter(cap=3.0, top_k=2, device=cuda), R.Meter(cap=3.0, top_k=2), R.Meter(cap=3.0, top_k=2)
    for b in batches:
        lp_pi, lp_beta = actor.log_prob(b["state"], b["ids"])[0], beta.log_prob(b["state"], b["ids"])[0]
        by_hand.update(lp_pi, lp_beta, b["reward"])
        ref.update(lp_pi.cpu().numpy(), lp_beta.cpu().numpy(), b["reward"].cpu().numpy())
        h, _ = _hidden64(actor, b["state"].cpu())
        lp64 = R.log_prob(h, actor.linear2.weight.detach().cpu(), actor.linear2.bias.detach().cpu(), b["ids"].cpu())[0]
        lb64 = R.log_prob(b["state"].cpu(), beta.net[0].weight.detach().cpu(), beta.net[0].bias.detach().cpu(), b["ids"].cpu())[0]
        ref64.update(lp64, lb64, b["reward"].cpu().numpy())
    assert torch.equal(m.sums.view(torch.int64), by_hand.sums.view(torch.int64)) and torch.equal(m.counts, by_hand.counts)
    _check_meter(m, ref)
    # against float64 log-probs: a log-prob error e moves a weight by w e; e < 2e-5 here (test_modules holds it to the bound)
    for k, (val, _) in ref64.readouts().items():
        assert getattr(m, k) == pytest.approx(val, rel=2e-4, abs=1e-6), k
    # a behaviour policy that computes the same function: every weight is exactly 1
    twin = recnn_amd.nn.DiscreteActor(70, N, 64).to(cuda)
    twin.load_state_dict(actor.state_dict())
    m = evaluate_policy(actor, twin, batches)
    assert m.max_weight == 1.0 and m.mean_weight == 1.0 and m.ess == m.rows == 201
    assert m.ips == pytest.approx(m.logged_mean, rel=1e-15) and m.snips == pytest.approx(m.logged_mean, rel=1e-15)
    again = evaluate_policy(actor, twin, batches, meter=m)
    assert again is m and m.rows == 402
    from recnn_amd.parallel import VocabParallelDiscreteActor
    with pytest.raises(TypeError, match="VocabParallelDiscreteActor"):
        evaluate_policy(VocabParallelDiscreteActor(70, N, 64), beta, batches)


# ------------------------------------------------------------------------------------------------------------------- memory

def test_memory_stays_far_below_one_logits_matrix(F, cuda):
    """B = 256, N = 20000, K = 64, fp32 (aligned: nothing is padded): peak allocated memory rises during the call by less than a
    quarter of one B x N fp32 matrix."""
    B, N, K = 256, 20000, 64
    x, W, c, a = (t.to(cuda) for t in _gauss(B, K, N, seed=6))
    F.catalogue_log_prob(x, W, c, a, dtype="fp32")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    lp, lse = F.catalogue_log_prob(x, W, c, a, dtype="fp32")
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - start
    print(f"memory: peak rise {rise} bytes, one B x N fp32 matrix {B * N * 4}")
    assert rise < B * N * 4 / 4
    ref_lp, ref_lse, E = R.log_prob(x.cpu(), W.cpu(), c.cpu(), a.cpu())
    tol = R.allowed(E, ref_lp, ref_lse, N, R.chain_depth(N, R.default_items_per_slice(B, N)))
    assert (np.abs(lp.cpu().numpy() - ref_lp) <= tol).all()
