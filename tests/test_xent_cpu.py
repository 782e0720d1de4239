"""CPU: the error bound of tests/xent_reference.py is sound (torch's own fp32 autograd route stays inside it, with the chains the
kernels are built with), the backward's workspace query is host arithmetic that validates its arguments and never scales with
B x N, and the argument errors of NextItemHead / next_item_update / catalogue_cross_entropy that need no GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ope_reference as R
import xent_reference as X


def _case(B, N, K, scale, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + K * 1000 + N + B)
    x = torch.randn(B, K, generator=g)
    W = torch.randn(N, K, generator=g) * scale
    c = torch.randn(N, generator=g) * scale
    a = torch.randint(0, N, (B,), generator=g)
    return x, W, c, a, torch.randn(B, generator=g), torch.randn(B, generator=g)


@pytest.mark.parametrize("B,N,K", X.SHAPES)
def test_bound_holds_torch_fp32_autograd(B, N, K):
    """The fp32 route torch itself takes (materialised logits, log_softmax, autograd) against the float64 reference, with the
    kernels' chains (d for the default forward slicing, c1 for the shortest and the default dx slicing, c2 = B + 2): every element of
    dx, dW and dc inside the bound, with and without an lse gradient, at logit scales 0.1 and 0.5."""
    worst = 0.0
    for scale in (0.1, 0.5):
        x, W, c, a, g_lp, g_lse = _case(B, N, K, scale)
        for use_lse in (False, True):
            xt, Wt, ct = (t.clone().requires_grad_(True) for t in (x, W, c))
            z = torch.addmm(ct, xt, Wt.T)
            lse = torch.logsumexp(z, 1)
            lp = z.gather(1, a[:, None])[:, 0] - lse
            loss = (g_lp * lp).sum() + ((g_lse * lse).sum() if use_lse else 0.0)
            loss.backward()
            d = R.chain_depth(N, R.default_items_per_slice(B, N))
            for ips in (R.TILE, X.bwd_items_per_slice(B, N, K)):
                ref = X.backward(x, W, c, a, g_lp, g_lse if use_lse else None, d=d, c1=X.chain_dx(N, ips), c2=X.chain_dw(B))
                for name, got in (("dx", xt.grad), ("dW", Wt.grad), ("dc", ct.grad)):
                    r = X.worst_ratio(got.numpy(), ref, name)
                    worst = max(worst, r)
                    assert r <= 1.0, (name, scale, use_lse, ips, r)
    print(f"torch fp32 route B={B} N={N} K={K}: worst error / tolerance = {worst:.3f}")


def test_reference_matches_float64_autograd():
    """The reference's closed form is the gradient: float64 autograd agrees to 1e-12, invalid action rows included."""
    x, W, c, a, g_lp, g_lse = _case(37, 50, 32, 0.5)
    a[3] = 50
    ref = X.backward(x, W, c, a, g_lp, g_lse)
    xt, Wt, ct = (t.double().requires_grad_(True) for t in (x, W, c))
    z = xt @ Wt.T + ct
    lse = torch.logsumexp(z, 1)
    ok = a < 50
    lp = z.gather(1, a.clamp(max=49)[:, None])[:, 0] - lse
    ((g_lp.double() * lp)[ok].sum() + (g_lse.double() * lse).sum()).backward()
    for name, got in (("dx", xt.grad), ("dW", Wt.grad), ("dc", ct.grad)):
        assert np.abs(got.numpy() - ref[name]).max() < 1e-12, name
    assert math.isnan(ref["lp"][3]) and np.isfinite(np.delete(ref["lp"], 3)).all()


def test_workspace_query_is_host_only_and_validates():
    from recnn_amd import _lib as L
    lib = L.load()
    n = C.c_int64(-1)
    assert lib.recnn_catalogue_logprob_bwd_workspace_bytes(300, 1500, 256, 256, C.byref(n)) == 0
    assert n.value == 6 * 300 * 256 * 4          # one [B][K] fp32 partial per slice
    assert lib.recnn_catalogue_logprob_bwd_workspace_bytes(0, 1500, 64, 128, C.byref(n)) == 0 and n.value == 0
    for bad in ((-1, 10, 64, 128), (4, 0, 64, 128), (4, 10, 64, 100), (4, 10, 64, 0), (4, 10, 48, 128), (4, 10, 0, 128)):
        assert lib.recnn_catalogue_logprob_bwd_workspace_bytes(*bad, C.byref(n)) != 0, bad
        assert b"catalogue_logprob_bwd_workspace_bytes" in lib.recnn_last_error()
    assert lib.recnn_catalogue_logprob_bwd_workspace_bytes(4, 10, 64, 128, None) != 0
    assert lib.recnn_catalogue_logprob_bwd_workspace_bytes(4, 10, 320, 128, C.byref(n)) != 0
    assert b"256" in lib.recnn_last_error()
    # the entry point itself refuses K = 320 by name before any HIP call (no GPU is needed to get the error)
    assert lib.recnn_catalogue_logprob_bwd(None, 320, 0, 320, C.c_void_p(16), 320, 0, C.c_void_p(16), 10, None, None, None, None, 128,
                                           None, 320, None, 320, None, None, None) != 0
    assert b"256" in lib.recnn_last_error()


def test_memory_never_scales_with_rows_times_items():
    """B = 2048, N = 100000, K = 256, the default dx slicing.  Everything the backward allocates that a gradient's own shape does
    not dictate -- the workspace -- plus dx and dc stays below one eighth of one fp32 logits matrix (B N 4 / 8 = 102.4 MB), and so
    does the workspace for up to 48 slices.  dW is [N, K] fp32 whatever computes it: 100000 x 256 x 4 = 102,400,000 bytes, which at
    this shape EQUALS B N 4 / 8 (B / 8 = K), so a sum that includes dW cannot lie strictly below that figure for any
    implementation; it is printed, and held to one eighth of the matrix plus dW's own size."""
    from recnn_amd import _lib as L
    from recnn_amd.nn import functional as F
    lib = L.load()
    B, N, K = 2048, 100000, 256
    eighth = B * N * 4 // 8
    ips = F.catalogue_bwd_items_per_slice(B, N, K)
    assert ips == X.bwd_items_per_slice(B, N, K) and ips % 128 == 0
    n = C.c_int64()
    assert lib.recnn_catalogue_logprob_bwd_workspace_bytes(B, N, K, ips, C.byref(n)) == 0
    dx, dw, dc = B * K * 4, N * K * 4, N * 4
    print(f"workspace {n.value} + dx {dx} + dc {dc} = {n.value + dx + dc}; dW {dw}; one eighth of the logits matrix {eighth}")
    assert n.value + dx + dc < eighth
    assert n.value + dx + dc + dw < eighth + dw
    # slice-order partials: 48 slices fit
    ips48 = (((N + 127) // 128 + 47) // 48) * 128
    assert (N + ips48 - 1) // ips48 <= 48
    assert lib.recnn_catalogue_logprob_bwd_workspace_bytes(B, N, K, ips48, C.byref(n)) == 0 and n.value < eighth
    # and nothing grows with B x N: doubling N at a fixed slice count leaves the workspace alone
    m = C.c_int64()
    assert lib.recnn_catalogue_logprob_bwd_workspace_bytes(B, 2 * N, K, 2 * ips, C.byref(m)) == 0
    assert lib.recnn_catalogue_logprob_bwd_workspace_bytes(B, N, K, ips, C.byref(n)) == 0 and m.value == n.value


def test_slice_lengths_are_functions_of_the_shape():
    from recnn_amd.nn import functional as F
    for B, N, K in X.SHAPES + ((2048, 100000, 128), (12800, 100000, 256), (1, 100000, 64)):
        ips = F.catalogue_bwd_items_per_slice(B, N, K)
        assert ips == X.bwd_items_per_slice(B, N, K) and ips >= 128 and ips % 128 == 0
        assert (N + ips - 1) // ips * ((B + 127) // 128) <= max(512 if K <= 128 else 256, (B + 127) // 128)


def test_argument_errors_without_a_gpu():
    import recnn_amd
    from recnn_amd import _lib as L
    from recnn_amd.nn import functional as F
    nn = recnn_amd.nn
    assert nn.next_item_update is nn.update.next_item_update and "next_item_update" in nn.update.__all__
    w = torch.zeros(10, 32)
    with pytest.raises(L.RecnnHipError):
        nn.NextItemHead(w)                                   # not on the GPU
    with pytest.raises(ValueError):
        nn.NextItemHead(w.double())
    with pytest.raises(ValueError):
        nn.NextItemHead(w.t())
    with pytest.raises(ValueError):
        nn.NextItemHead(torch.zeros(10))
    with pytest.raises(TypeError, match="NextItemHead"):
        nn.next_item_update({"state": w, "target": torch.zeros(10, dtype=torch.int64)}, {}, {"head": torch.nn.Linear(32, 10)},
                            {"optimizer": None})
    with pytest.raises(TypeError, match="NextItemHead"):
        nn.next_item_update({}, {}, {}, {})
    with pytest.raises(L.RecnnHipError):
        F.catalogue_log_prob_train(w, w, None, torch.zeros(10, dtype=torch.int64))
    with pytest.raises(L.RecnnHipError):
        F.catalogue_cross_entropy(w, w, None, torch.zeros(10, dtype=torch.int64))
    with pytest.raises(ValueError, match="reduction"):
        F.catalogue_cross_entropy(w, w, None, torch.zeros(10, dtype=torch.int64), reduction="max")
    with pytest.raises(ValueError, match="256"):
        F.catalogue_log_prob_train(torch.zeros(4, 320), torch.zeros(10, 320), None, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="256"):
        F.catalogue_log_prob_train(torch.zeros(4, 257), torch.zeros(10, 257), None, torch.zeros(4, dtype=torch.int64), dtype="bf16")
