"""tests/optim_reference.py checked without a GPU.

  * An op-by-op float32 numpy emulation of every kernel formula (separate products, no FMA: the kernels have contraction off; numpy's
    float32 `/` and sqrt are correctly rounded, like the device's) stays within 1x the reference's bound -- the bound is a bound.
  * Non-vacuity, on the reference alone: the bound is a small fraction of what it guards (1e-3 of the parameter UPDATE, 1e-5 of the
    moments), so that a wrong formula cannot hide inside it.
  * Every mutant of optim_reference misses the asserted `<= 2 bound` on at least a quarter of the elements at a step where it differs:
    the GPU assertions of tests/test_gpu_optim_exact.py would fail for a kernel that computed it."""
import math

import numpy as np
import pytest

from tests import optim_reference as R

f32 = np.float32
N = 200_000
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
RHP = dict(lr=1e-3, beta1=0.95, beta2=0.999, eps=1e-5, alpha=0.5, k=6)


@pytest.fixture(scope="module")
def inp():
    return R.make_inputs(N, 7)


# ---- float32 emulations, in the kernels' operation order -------------------------------------------------------------------------
def emu_adam(x, lr, beta1, beta2, eps, wd, t, gs):
    p, g, m, v = x["p"], x["g"], x["m"], x["v"]
    bc1, bc2 = -math.expm1(t * math.log(beta1)), -math.expm1(t * math.log(beta2))
    step_size, bc2_sqrt = f32(float(f32(lr)) / bc1), f32(math.sqrt(bc2))
    omb1, omb2, b2, wdf = f32(1.0 - beta1), f32(1.0 - beta2), f32(beta2), f32(wd)
    gj = g * f32(gs)
    if wd != 0:
        gj = gj + wdf * p
    m = m + omb1 * (gj - m)
    v = b2 * v + (omb2 * gj) * gj
    denom = np.sqrt(v) / bc2_sqrt + f32(eps)
    p = p - step_size * (m / denom)
    return dict(p=p, m=m, v=v)


def emu_ranger(x, lr, beta1, beta2, eps, wd, alpha, k, t, gs):
    p, g, m, v, sl = x["p"], x["g"], x["m"], x["v"], x["slow"]
    rect, step, _ = R.radam_step(t, beta1, beta2)
    sl_lr = f32(step) * f32(lr)
    gj = g * f32(gs)
    v = f32(beta2) * v + (f32(1.0 - beta2) * gj) * gj
    m = f32(beta1) * m + f32(1.0 - beta1) * gj
    if wd != 0:
        p = p + (-f32(wd) * f32(lr)) * p
    if rect:
        p = p + (-sl_lr) * (m / (np.sqrt(v) + f32(eps)))
    else:
        p = p + (-sl_lr) * m
    if k > 0 and t % k == 0:
        sl = sl + f32(alpha) * (p - sl)
        p = sl
    return dict(p=p, m=m, v=v, slow=sl)


def emu_radam(x, lr, beta1, beta2, eps, wd, t, norm, max_norm):
    p, g, m, v = x["p"], x["g"], x["m"], x["v"]
    rect, S, U_ = R.radam_scalars_flat(float(f32(lr)), beta1, beta2, t)
    if norm is not None:
        g = g * min(f32(max_norm) / (f32(norm) + f32(1e-6)), f32(1.0))
    gi = g
    if wd != 0:
        gi = gi + f32(wd) * p
    m = m + f32(1.0 - beta1) * (gi - m)
    v = v * f32(beta2) + (f32(1.0 - beta2) * gi) * gi
    step = f32(1.0) / ((np.sqrt(v) + f32(eps)) / f32(S)) if rect else f32(U_)
    p = p + step * m
    return dict(p=p, g=g, m=m, v=v)


def emu_soft(tp, p, tau):
    return tp * (f32(1.0) - f32(tau)) + p * f32(tau)


def _all_f32(d):
    return all(v.dtype == np.float32 for v in d.values())


# ---- the bound is a bound ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("t", [1, 2, 7, 1000, 100000])
def test_adam_emulation_within_bound(inp, t, wd):
    for gs in (1.0, 0.5, 0.3):
        got = emu_adam(inp, wd=wd, t=t, gs=gs, **HP)
        assert _all_f32(got)
        ref = R.adam(inp["p"], inp["g"], inp["m"], inp["v"], wd=wd, t=t, gs=gs, **HP)
        for key in ("p", "m", "v"):
            assert R.ratio(got[key], ref[key]) <= 1.0, (key, t, wd, gs, R.ratio(got[key], ref[key]))


@pytest.mark.parametrize("t", [4, 5, 6, 7, 12])
def test_ranger_emulation_within_bound(inp, t):
    assert not R.radam_step(5, 0.95, 0.999)[0] and R.radam_step(6, 0.95, 0.999)[0]      # the cases bracket the N_sma > 5 switch
    for wd in (0.0, 1e-2):
        got = emu_ranger(inp, wd=wd, t=t, gs=1.0, **RHP)
        assert _all_f32(got)
        ref = R.ranger(inp["p"], inp["g"], inp["m"], inp["v"], inp["slow"], wd=wd, t=t, **RHP)
        assert ref["sync"] == (t in (6, 12)) and ref["rect"] == (t >= 6)
        for key in ("p", "m", "v", "slow"):
            assert R.ratio(got[key], ref[key]) <= 1.0, (key, t, wd, R.ratio(got[key], ref[key]))
        if not ref["sync"]:
            assert np.array_equal(got["slow"], inp["slow"]) and not np.any(ref["slow"].e)


@pytest.mark.parametrize("norm", [None, 0.37, 25.0])
@pytest.mark.parametrize("t", [5, 6])
def test_radam_emulation_within_bound(inp, t, norm):
    for wd in (0.0, 1e-2):
        got = emu_radam(inp, wd=wd, t=t, norm=norm, max_norm=1.0, **HP)
        ref = R.radam(inp["p"], inp["g"], inp["m"], inp["v"], wd=wd, t=t, norm=None if norm is None else f32(norm), max_norm=1.0, **HP)
        assert ref["rect"] == (t >= 6)
        for key in ("p", "g", "m", "v"):
            assert R.ratio(got[key], ref[key]) <= 1.0, (key, t, wd, norm, R.ratio(got[key], ref[key]))


def test_soft_and_clip_emulations_within_bound(inp):
    for tau in (0.001, 0.05, 0.5):
        assert R.ratio(emu_soft(inp["tgt"], inp["p"], tau), R.soft(inp["tgt"], inp["p"], tau)) <= 1.0
    g = inp["g"][:5000]
    # a float32 summation in ANY order of non-negative terms is within (terms - 1) u of the sum; the tree's depth is what the kernels' order earns
    s32 = f32(0)
    for blk in np.abs(g).reshape(-1, 8):
        s32 = s32 + ((blk[0] + blk[1]) + (blk[2] + blk[3])) + ((blk[4] + blk[5]) + (blk[6] + blk[7]))
    assert R.ratio(s32, R.l1_sum(g, 625 + 3)) <= 1.0
    for gs in (1.0, 0.5):
        l1 = R.l1_sum(g, R.engine_l1_depth(17))
        coef = min(f32(-1.0) / (f32(l1.v) * f32(gs) + f32(1e-6)), f32(1.0))
        assert R.ratio(coef, R.quirk_clip_coef(R.exact(f32(l1.v)), gs)) <= 1.0
    zero = R.quirk_clip_coef(R.l1_sum(np.zeros(8), 21), 1.0)
    assert abs(float(zero.v) + 1e6) < 1.0 and float(zero.e) < 1.0


# ---- the bound is small against what it guards ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("t", [1, 2, 7, 1000, 100000])
def test_adam_bounds_are_not_vacuous(inp, t, wd):
    ref = R.adam(inp["p"], inp["g"], inp["m"], inp["v"], wd=wd, t=t, **HP)
    upd = np.abs(ref["p"].v - inp["p"].astype(np.float64))
    frac_p = float(np.mean(2 * ref["p"].e < 1e-3 * upd))
    assert frac_p >= 0.95, (t, wd, frac_p)
    for key in ("m", "v"):
        frac = float(np.mean(2 * ref[key].e < 1e-5 * np.abs(ref[key].v)))
        assert frac >= 0.99, (key, t, wd, frac)


@pytest.mark.parametrize("t", [4, 5, 6, 7, 12])
def test_ranger_bounds_are_not_vacuous(inp, t):
    """The moments.  The parameter cannot meet Adam's 1e-3 criterion at these steps by the nature of the algorithm, whatever the bound: an
    unrectified step is p -= lr step m (momentum SGD: with |m| log-uniform down to 1e-9 most updates are below an ulp of p), and the
    first rectified steps are scaled by r_t ~ 1e-2, a 1e-5 update against an ulp of 6e-9.  What the parameter's bound still rejects is
    shown per mutant in test_ranger_mutants_are_caught; on a Lookahead sync the update is alpha (p - slow), far above the bound:"""
    ref = R.ranger(inp["p"], inp["g"], inp["m"], inp["v"], inp["slow"], wd=1e-2, t=t, **RHP)
    for key in ("m", "v"):
        frac = float(np.mean(2 * ref[key].e < 1e-5 * np.abs(ref[key].v)))
        assert frac >= 0.99, (key, t, frac)
    if ref["sync"]:
        for key, old in (("p", inp["p"]), ("slow", inp["slow"])):
            upd = np.abs(ref[key].v - old.astype(np.float64))
            frac_p = float(np.mean(2 * ref[key].e < 1e-3 * upd))
            assert frac_p >= 0.95, (key, t, frac_p)


# ---- every mutant is caught ---------------------------------------------------------------------------------------------------------
def _caught(ref, mut, keys):
    """largest fraction of elements, over the compared arrays, on which the mutant is more than 2 bound away from the reference"""
    return max(float(np.mean(np.abs(mut[k].v - ref[k].v) > 2 * ref[k].bound())) for k in keys)


@pytest.mark.parametrize("mutant,t,wd", [("eps_in_sqrt", 1, 0.0), ("eps_in_sqrt", 1000, 0.0), ("no_bc2", 1, 0.0), ("no_bc2", 2, 1e-2),
                                         ("decoupled_wd", 2, 1e-2), ("decoupled_wd", 1000, 1e-2)])
def test_adam_mutants_are_caught(inp, mutant, t, wd):
    a = (inp["p"], inp["g"], inp["m"], inp["v"])
    ref, mut = R.adam(*a, wd=wd, t=t, **HP), R.adam(*a, wd=wd, t=t, mutant=mutant, **HP)
    frac = _caught(ref, mut, ("p", "m", "v"))
    assert frac >= 0.25, (mutant, t, frac)


def test_no_bias_correction_is_invisible_late_as_it_must_be(inp):
    a = (inp["p"], inp["g"], inp["m"], inp["v"])
    ref, mut = R.adam(*a, t=100000, **HP), R.adam(*a, t=100000, mutant="no_bc2", **HP)
    assert _caught(ref, mut, ("p", "m", "v")) == 0.0


@pytest.mark.parametrize("mutant,t", [("eps_in_sqrt", 6), ("eps_in_sqrt", 7), ("l2_wd", 4), ("l2_wd", 7), ("rect_early", 5), ("la_no_slow", 6),
                                      ("la_no_slow", 12)])
def test_ranger_mutants_are_caught(inp, mutant, t):
    a = (inp["p"], inp["g"], inp["m"], inp["v"], inp["slow"])
    ref, mut = R.ranger(*a, wd=1e-2, t=t, **RHP), R.ranger(*a, wd=1e-2, t=t, mutant=mutant, **RHP)
    frac = _caught(ref, mut, ("p", "m", "v", "slow"))
    assert frac >= 0.25, (mutant, t, frac)


def test_soft_mutant_is_caught(inp):
    for tau in (0.001, 0.05):
        ref, mut = R.soft(inp["tgt"], inp["p"], tau), R.soft(inp["tgt"], inp["p"], tau, mutant="tau_swapped")
        assert float(np.mean(np.abs(mut.v - ref.v) > 2 * ref.bound())) >= 0.25


def test_mutants_fail_against_the_emulated_kernel(inp):
    """The same statement from the kernel's side: the float32 emulation of the RIGHT formula, held to a mutant reference with the
    assertion the GPU tests use, fails."""
    got = emu_adam(inp, wd=1e-2, t=2, gs=1.0, **HP)
    for mutant in R.ADAM_MUTANTS:
        mut = R.adam(inp["p"], inp["g"], inp["m"], inp["v"], wd=1e-2, t=2, mutant=mutant, **HP)
        assert max(R.ratio(got[k], mut[k]) for k in ("p", "m", "v")) > 2.0, mutant
    for mutant, t in (("eps_in_sqrt", 6), ("l2_wd", 6), ("rect_early", 5), ("la_no_slow", 6)):
        got = emu_ranger(inp, wd=1e-2, t=t, gs=1.0, **RHP)
        mut = R.ranger(inp["p"], inp["g"], inp["m"], inp["v"], inp["slow"], wd=1e-2, t=t, mutant=mutant, **RHP)
        assert max(R.ratio(got[k], mut[k]) for k in ("p", "m", "v", "slow")) > 2.0, mutant
    assert R.ratio(emu_soft(inp["tgt"], inp["p"], 0.05), R.soft(inp["tgt"], inp["p"], 0.05, mutant="tau_swapped")) > 2.0


def test_reference_refuses_subnormal_intermediates():
    x = R.make_inputs(16, 0)
    g = x["g"].copy()
    g[0] = 1e-25                      # g * g * (1 - beta2) is subnormal in fp32
    with pytest.raises(AssertionError):
        R.adam(x["p"], g, x["m"], np.zeros_like(x["v"]), t=1, **HP)
