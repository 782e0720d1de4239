"""CPU checks of off-policy evaluation: the float64 reference (tests/ope_reference.py) on examples worked by hand, the bound's
slack against fp32 log_softmax, and the native boundary of csrc/logprob.hip / csrc/ope.hip (declared, exported, signed; host-only
workspace queries; bad arguments refused; no CPU fallback)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import ope_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("recnn_catalogue_logprob_workspace_bytes", "recnn_catalogue_logprob", "recnn_ope_accumulate_workspace_bytes",
       "recnn_ope_accumulate")
GAUSSIAN_SHAPES = [(64, 1), (64, 63), (64, 64), (64, 65), (192, 200), (64, 1000), (1344, 130)]


def test_three_rows_by_hand():
    # pi = (1/2, 1/4, 1/8), beta = (1/4, 1/4, 1/2): w = (2, 1, 1/4); r = (1, 2, 4)
    lp_pi, lp_beta = np.log([0.5, 0.25, 0.125]), np.log([0.25, 0.25, 0.5])
    r = np.array([1.0, 2.0, 4.0])
    m = R.Meter(cap=1.5)
    m.update(lp_pi, lp_beta, r, q_logged=np.array([0.5, 2.0, 3.0]), v_dm=np.array([1.0, 1.0, 2.0]))
    out = {k: v[0] for k, v in m.readouts().items()}
    assert out["rows"] == 3 and out["invalid"] == 0
    assert out["ips"] == pytest.approx((2 * 1 + 1 * 2 + 0.25 * 4) / 3, rel=1e-6)                 # 5 / 3
    assert out["capped_ips"] == pytest.approx((1.5 * 1 + 1 * 2 + 0.25 * 4) / 3, rel=1e-6)        # 4.5 / 3
    assert out["capped_share"] == pytest.approx(1 / 3)
    assert out["snips"] == pytest.approx(5 / 3.25, rel=1e-6)
    assert out["ess"] == pytest.approx(3.25 ** 2 / (4 + 1 + 1 / 16), rel=1e-6)
    assert out["mean_weight"] == pytest.approx(3.25 / 3, rel=1e-6)
    assert out["max_weight"] == pytest.approx(2.0, rel=1e-6)
    assert out["logged_mean"] == pytest.approx(7 / 3, rel=1e-6)
    # dr terms: 1 + 2 (1 - 0.5) = 2;  1 + 1 (2 - 2) = 1;  2 + 0.25 (4 - 3) = 2.25
    assert out["dr"] == pytest.approx(5.25 / 3, rel=1e-6)


def test_masked_and_nan_rows():
    m = R.Meter()
    m.update([0.0, np.nan, -1.0, -1.0], [0.0, -1.0, np.nan, -1.0], [1.0, 5.0, 5.0, 3.0], mask=[1, 1, 1, 0])
    out = m.readouts()
    assert out["rows"][0] == 1 and out["invalid"][0] == 2 and out["ips"][0] == 1.0


def test_lambda_k_against_the_formula():
    lp = np.log(np.array([0.9, 0.5, 0.01, 1e-9]))
    for k in (1, 2, 5, 16):
        want = k * (1.0 - np.exp(lp)) ** (k - 1)
        assert np.allclose(R.lambda_k(lp, k), want, rtol=1e-12, atol=0)
    assert (R.lambda_k(lp, 1) == 1.0).all()
    assert (R.weights(lp, lp - 0.5, top_k=1) == R.weights(lp, lp - 0.5, top_k=0)).all()


def test_equal_policies_give_the_logged_mean():
    rng = np.random.default_rng(0)
    lp = np.float32(-rng.uniform(0.1, 12.0, size=1000))
    r = np.float32(rng.normal(size=1000))
    m = R.Meter()
    m.update(lp, lp, r)
    out = {k: v[0] for k, v in m.readouts().items()}
    assert out["ips"] == out["snips"] == out["logged_mean"]
    assert out["ess"] == out["rows"] == 1000 and out["max_weight"] == 1.0 and out["mean_weight"] == 1.0


@pytest.mark.parametrize("K,N", GAUSSIAN_SHAPES)
def test_bound_is_loose_for_fp32_log_softmax(K, N):
    """With d = N, torch's CPU fp32 log_softmax of the fp32 logits stays below 0.02 of the bound: the bound is loose by design,
    the structured GPU cases carry the sharpness."""
    g = torch.Generator().manual_seed(K * 1000 + N)
    B = 65
    x = torch.randn(B, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    c = torch.randn(N, generator=g)
    a = torch.randint(0, N, (B,), generator=g)
    for scale in (1.0, 6.0):
        lp, lse, E = R.log_prob(x * scale, W, c * scale, a)
        got = torch.log_softmax((x * scale) @ W.T + c * scale, 1).gather(1, a[:, None])[:, 0].double().numpy()
        ratio = np.abs(got - lp) / R.allowed(E, lp, lse, N, N)
        assert ratio.max() < 0.02, (K, N, scale, ratio.max())


def test_chain_depth_and_default_slices():
    assert R.chain_depth(200, 128) == 11 + 1 + 2 and R.chain_depth(1000, 256) == 11 + 2 + 4 and R.chain_depth(1, 128) == 1
    from recnn_amd.nn import functional as F
    for B, N in ((1, 1), (130, 200), (2048, 100_000), (256, 20_000), (100_000, 64)):
        ips = F.default_items_per_slice(B, N)
        assert ips == R.default_items_per_slice(B, N) and ips % R.TILE == 0 and ips >= R.TILE
    ips = F.default_items_per_slice(2048, 100_000)
    assert 256 <= 16 * ((100_000 + ips - 1) // ips) <= 512


def test_new_entry_points_are_declared_exported_and_signed():
    from recnn_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "recnn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(recnn_[a-z0-9_]+)\s*\(", src))
    lib = L.load()
    assert lib.recnn_abi_version() == 2
    for n in NEW:
        assert n in declared, f"{n} is not declared in include/recnn_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in L.SIGNATURES, f"{n} has no ctypes signature"
    mk = open(os.path.join(ROOT, "recnn_amd", "csrc", "Makefile")).read()
    assert "logprob.hip" in mk and "ope.hip" in mk


def test_workspace_queries_are_host_arithmetic():
    from recnn_amd import _lib as L
    lib = L.load()
    a, b = C.c_int64(0), C.c_int64(0)
    q = lib.recnn_catalogue_logprob_workspace_bytes
    assert q(64, 200, 128, C.byref(a)) == 0 and q(128, 200, 128, C.byref(b)) == 0 and 0 < a.value < b.value
    assert q(64, 1000, 128, C.byref(b)) == 0 and a.value < b.value           # more slices
    assert q(64, 200, 256, C.byref(b)) == 0 and b.value < a.value            # one slice
    assert a.value >= (2 * 2 + 1) * 64 * 4
    assert q(0, 200, 128, C.byref(b)) == 0 and b.value == 0
    for bad in ((-1, 200, 128), (64, 0, 128), (64, -5, 128), (64, 200, 0), (64, 200, -128), (64, 200, 64), (64, 200, 192)):
        assert q(*bad, C.byref(b)) == -1, bad
        assert b"catalogue_logprob_workspace_bytes" in lib.recnn_last_error()
    assert q(64, 200, 128, None) == -1
    q = lib.recnn_ope_accumulate_workspace_bytes
    assert q(1, C.byref(a)) == 0 and q(100_000, C.byref(b)) == 0 and 0 < a.value < b.value
    assert q(0, C.byref(b)) == 0 and b.value == 0
    assert q(-1, C.byref(b)) == -1 and b"ope_accumulate_workspace_bytes" in lib.recnn_last_error()
    assert q(5, None) == -1


def test_null_pointers_are_refused_with_a_message():
    from recnn_amd import _lib as L
    lib = L.load()
    assert lib.recnn_catalogue_logprob(None, 64, 4, 64, None, 64, 0, None, 10, None, 128, None, None, None, None) == -1
    assert b"catalogue_logprob: null pointer" in lib.recnn_last_error()
    assert lib.recnn_ope_accumulate(None, None, None, None, None, None, 4, math.inf, 0, None, None, None, None) == -1
    assert b"ope_accumulate: null pointer" in lib.recnn_last_error()
    # arguments checked before anything is launched: host buffers stand in for device ones
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.recnn_ope_accumulate(p, p, p, None, p, None, 4, math.inf, 0, p, p, p, None) == -1
    assert b"come together" in lib.recnn_last_error()
    assert lib.recnn_ope_accumulate(p, p, p, None, None, None, 4, 0.0, 0, p, p, p, None) == -1
    assert b"cap" in lib.recnn_last_error()
    assert lib.recnn_ope_accumulate(p, p, p, None, None, None, 4, math.inf, -1, p, p, p, None) == -1
    assert b"top_k" in lib.recnn_last_error()
    assert lib.recnn_catalogue_logprob(p, 64, 4, 48, p, 64, 0, p, 10, p, 128, p, p, p, None) == -1
    assert b"multiple of 32" in lib.recnn_last_error()
    assert lib.recnn_catalogue_logprob(p, 64, 4, 64, p, 64, 0, p, 10, p, 100, p, p, p, None) == -1
    assert b"items_per_slice" in lib.recnn_last_error()
    assert lib.recnn_catalogue_logprob(p, 32, 4, 64, p, 64, 0, p, 10, p, 128, p, p, p, None) == -1
    assert b"at least K long" in lib.recnn_last_error()


def test_cpu_tensors_mean_loud_failure_not_fallback():
    import recnn_amd
    from recnn_amd import _lib as L
    from recnn_amd.nn import functional as F
    with pytest.raises(L.RecnnHipError):
        F.catalogue_log_prob(torch.zeros(2, 64), torch.zeros(10, 64), torch.zeros(10), torch.zeros(2, dtype=torch.int64))
    if not torch.cuda.is_available():
        with pytest.raises(L.RecnnHipError):
            recnn_amd.ope.OffPolicyMeter()
    with pytest.raises(L.RecnnHipError):
        recnn_amd.ope.OffPolicyMeter(device="cpu")
    with pytest.raises(L.RecnnHipError):
        recnn_amd.nn.Beta(70, 20).log_prob(torch.zeros(2, 70), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(L.RecnnHipError):
        recnn_amd.nn.DiscreteActor(70, 20, 64).log_prob(torch.zeros(2, 70), torch.zeros(2, dtype=torch.int64))
    import recnn
    assert recnn.ope is recnn_amd.ope
