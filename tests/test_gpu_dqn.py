"""GPU: the dueling DQN of the embeddings notebook (csrc/dqn.hip, recnn_amd.nn.DuelDQN, recnn_amd.nn.update.dqn_update) against the
float64 restatement in tests/dqn_reference.py.

Bounds (u = 2^-24): fp32 values are held to 1e-4 of the largest magnitude of the compared tensor (the exact-f32 MFMA
products carry at most ~K u relative error of the absolute dot with K <= 1344 through three layers: 3e-4 worst case, 1e-5 typical);
the bf16 head to 2^-7 of sum_k |h_k W_nk| plus that.  Sums with a fixed order are checked bit for bit across calls."""
import copy

import numpy as np
import pytest
import torch

import dqn_reference as R

pytestmark = pytest.mark.gpu

SHAPES_B = [1, 65, 2048]
SHAPES_N = [1, 63, 65, 26744, 100001]


def _rel_err(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def _models(N, cuda, K=1290, seed=0):
    from recnn_amd.nn import DuelDQN
    torch.manual_seed(seed)
    m = DuelDQN(K, N).to(cuda)
    with torch.no_grad():
        for p in m.parameters():          # default init leaves the head near zero: spread it so that max / mean are not trivial
            p.mul_(3.0)
    ref = R.RefDuelDQN(K, N).double().to(cuda)
    ref.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    return m, ref


@pytest.mark.parametrize("B", SHAPES_B)
@pytest.mark.parametrize("N", SHAPES_N)
def test_forward(cuda, B, N):
    m, ref = _models(N, cuda)
    x = torch.randn(B, 1290, device=cuda, generator=torch.Generator(cuda).manual_seed(B * 7 + N))
    Q = m(x)
    assert Q.shape == (B, N) and Q.dtype == torch.float32
    with torch.no_grad():
        Q64 = ref(x.double())
    assert _rel_err(Q, Q64) < 1e-4


@pytest.mark.parametrize("B,N", [(1, 65), (65, 63), (65, 26744), (2048, 1), (2048, 1000)])
def test_backward(cuda, B, N):
    m, ref = _models(N, cuda, seed=1)
    gen = torch.Generator(cuda).manual_seed(3)
    x = torch.randn(B, 1290, device=cuda, generator=gen)
    dQ = torch.randn(B, N, device=cuda, generator=gen)
    x1 = x.clone().requires_grad_(True)
    (m(x1) * dQ).sum().backward()
    x2 = x.double().requires_grad_(True)
    (ref(x2) * dQ.double()).sum().backward()
    assert _rel_err(x1.grad, x2.grad) < 1e-4
    for (name, p), p2 in zip(m.named_parameters(), ref.parameters()):
        assert p.grad is not None, name
        assert _rel_err(p.grad, p2.grad) < 1e-4, name


def test_row_max_and_mean(cuda):
    from recnn_amd.nn import functional as Fh
    B, N = 65, 26744
    gen = torch.Generator(cuda).manual_seed(5)
    h = torch.relu(torch.randn(B, 256, device=cuda, generator=gen))
    W = torch.randn(N, 128, device=cuda, generator=gen) * 0.1
    c = torch.randn(N, device=cuda, generator=gen)
    A64 = h[:, :128].double() @ W.double().T + c.double()
    got = Fh.ord_to_float(Fh.dqn_head(h, W, c, rowmax=True))
    bound = 1e-5 * float((h[:, :128].double().abs() @ W.double().abs().T).max()) + 1e-6
    assert float((got.double() - A64.max(1)[0]).abs().max()) < bound
    sh, sw, sc = Fh.dqn_head_stats(h, B, W, c)
    mu = torch.empty(1, device=cuda)
    from recnn_amd import _lib as L
    L.call("recnn_dqn_mean", L.ptr(sh), L.ptr(sw), L.ptr(sc), B, N, L.ptr(mu), L.current_stream())
    assert abs(float(mu) - float(A64.mean())) < 1e-5 * float(A64.abs().mean()) + 1e-6
    # bf16 head: within 2^-7 of the absolute dot
    Fh.set_catalogue_dtype("bf16")
    try:
        got16 = Fh.ord_to_float(Fh.dqn_head(h, W, c, rowmax=True))
    finally:
        Fh.set_catalogue_dtype("fp32")
    assert float((got16.double() - A64.max(1)[0]).abs().max()) < 2 ** -7 * float((h[:, :128].double().abs() @ W.double().abs().T).max())


def _scatter(src, ids, per_row, n_dest, scale=None):
    import ctypes as C
    from recnn_amd import _lib as L
    rows = ids.shape[0]
    n = C.c_int64()
    L.call("recnn_dqn_scatter_workspace_bytes", rows * per_row, n_dest, C.byref(n))
    ws = torch.empty(n.value // 4 + 1, device=src.device)
    out = torch.full((n_dest, 128), float("nan"), device=src.device)
    out_s = torch.full((n_dest,), float("nan"), device=src.device)
    L.call("recnn_dqn_scatter_sum", L.ptr(src), src.stride(0), rows, per_row, L.ptr(ids), ids.stride(0), L.ptr(scale), n_dest, L.ptr(out),
           L.ptr(out_s), None, None, L.ptr(ws), L.current_stream())
    return out, out_s


def test_scatter_sum_exact_order_and_skew(cuda):
    B, F, n_dest = 2048, 10, 26744
    gen = torch.Generator(cuda).manual_seed(11)
    src = torch.randn(B, F * 128 + 64, device=cuda, generator=gen)
    # Zipf-like popularity plus one item in 3000 contributions (longer than many pieces)
    ids = (torch.rand(B, F, device=cuda, generator=gen) ** 4 * n_dest).long().clamp_(max=n_dest - 1)
    ids.view(-1)[torch.randperm(B * F, device=cuda, generator=gen)[:3000]] = 17
    scale = torch.randn(B, device=cuda, generator=gen)
    out, out_s = _scatter(src, ids, F, n_dest)
    ref = torch.zeros(n_dest, 128, dtype=torch.float64, device=cuda).index_add_(
        0, ids.reshape(-1), src[:, :F * 128].reshape(B * F, 128).double())
    cnt = torch.bincount(ids.reshape(-1), minlength=n_dest).double()
    absum = torch.zeros(n_dest, 128, dtype=torch.float64, device=cuda).index_add_(
        0, ids.reshape(-1), src[:, :F * 128].reshape(B * F, 128).double().abs())
    assert bool(((out.double() - ref).abs() <= cnt[:, None] * 2 ** -24 * absum + 1e-30).all())
    assert torch.equal(out_s.double(), cnt)
    out2, _ = _scatter(src, ids, F, n_dest)
    assert torch.equal(out, out2)
    # one contribution per row with a weight (the head's g_b h_b)
    a = ids[:, 0].contiguous()
    o1, s1 = _scatter(src, a, 1, n_dest, scale)
    r1 = torch.zeros(n_dest, 128, dtype=torch.float64, device=cuda).index_add_(0, a, scale.double()[:, None] * src[:, :128].double())
    assert float((o1.double() - r1).abs().max()) < 1e-5 * float(r1.abs().max())
    assert float((s1.double() - torch.zeros(n_dest, dtype=torch.float64, device=cuda).index_add_(0, a, scale.double())).abs().max()) < 1e-5


def _nets(cuda, N=300, F=10, seed=0, lr=1e-3, fused=True):
    from recnn_amd.nn import DuelDQN
    from recnn_amd.optim import RAdam
    torch.manual_seed(seed)
    dqn = DuelDQN(F * 129, N).to(cuda)
    target = DuelDQN(F * 129, N).to(cuda)
    target.load_state_dict(dqn.state_dict())
    with torch.no_grad():
        for p in target.parameters():
            p.add_(torch.randn_like(p) * 0.01)
    emb = torch.nn.Embedding(N, 128).to(cuda)
    Opt = RAdam if fused else torch.optim.RAdam
    nets = {"dqn": dqn, "target_dqn": target, "embeddings": emb}
    opts = {"value_optimizer": Opt(dqn.parameters(), lr=lr), "embeddings_optimizer": Opt(emb.parameters(), lr=lr)}
    return nets, opts


def _oracle(nets, lr=1e-3):
    dqn = R.RefDuelDQN(nets["dqn"].feature[0].in_features, nets["dqn"].advantage[2].out_features).double()
    dqn.load_state_dict({k: v.double().cpu() for k, v in nets["dqn"].state_dict().items()})
    target = copy.deepcopy(dqn)
    target.load_state_dict({k: v.double().cpu() for k, v in nets["target_dqn"].state_dict().items()})
    emb = torch.nn.Embedding(*nets["embeddings"].weight.shape).double()
    emb.weight.data.copy_(nets["embeddings"].weight.detach().double().cpu())
    return dqn, target, emb, torch.optim.RAdam(dqn.parameters(), lr=lr), torch.optim.RAdam(emb.parameters(), lr=lr)


def _batch(B, F, N, seed):
    b = R.make_batch(B, F, N, torch.Generator().manual_seed(seed))
    b["ratings"], b["next_ratings"], b["reward"] = b["ratings"].float(), b["next_ratings"].float(), b["reward"].float()
    b["done"] = b["done"].float()
    return b


def _b64(b):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in b.items()}


@pytest.mark.parametrize("fused", [True, False])
def test_learn_step_against_oracle(cuda, fused):
    from recnn_amd.nn.update import dqn_update
    nets, opts = _nets(cuda, fused=fused)
    dqn64, tgt64, emb64, vo64, eo64 = _oracle(nets)
    b = _batch(37, 10, 300, 1)
    out = dqn_update(b, {"gamma": 0.99}, nets, opts)
    loss64, _, _ = R.autograd_step(dqn64, tgt64, emb64, _b64(b), 0.99, vo64, eo64)
    assert out["step"] == -1
    assert abs(out["value"] - loss64) <= 1e-4 * abs(loss64)
    for (name, p), p64 in zip(nets["dqn"].named_parameters(), dqn64.parameters()):
        assert _rel_err(p.grad.cpu(), p64.grad) < 2e-4, name
        assert _rel_err(p.detach().cpu(), p64.detach()) < 1e-5, name
        st, st64 = opts["value_optimizer"].state[p], vo64.state[p64]
        assert _rel_err(st["exp_avg"].cpu(), st64["exp_avg"]) < 2e-4, name
        assert _rel_err(st["exp_avg_sq"].cpu(), st64["exp_avg_sq"]) < 4e-4, name
    assert _rel_err(nets["embeddings"].weight.grad.cpu(), emb64.weight.grad) < 1e-4
    assert _rel_err(nets["embeddings"].weight.detach().cpu(), emb64.weight.detach()) < 1e-5
    st = opts["embeddings_optimizer"].state[nets["embeddings"].weight]
    assert _rel_err(st["exp_avg"].cpu(), eo64.state[emb64.weight]["exp_avg"]) < 1e-4


def _loop(cuda, steps, dtype="fp32", seed=0, N=300):
    from recnn_amd.nn import functional as Fh
    from recnn_amd.nn.update import dqn_update
    from recnn_amd.utils import soft_update
    nets, opts = _nets(cuda, N=N, seed=seed)
    Fh.set_catalogue_dtype(dtype)
    losses = []
    try:
        for step in range(1, steps + 1):
            losses.append(dqn_update(_batch(64, 10, N, 100 + step), {"gamma": 0.99}, nets, opts, step=step)["value"])
            if step % 30:
                soft_update(nets["dqn"], nets["target_dqn"])
    finally:
        Fh.set_catalogue_dtype("fp32")
    return losses, nets


def _loop64(nets0, steps, N=300):
    dqn, target, emb, vo, eo = _oracle(nets0)
    losses = []
    for step in range(1, steps + 1):
        losses.append(R.autograd_step(dqn, target, emb, _b64(_batch(64, 10, N, 100 + step)), 0.99, vo, eo)[0])
        if step % 30:
            with torch.no_grad():
                for tp, p in zip(target.parameters(), dqn.parameters()):
                    tp.copy_(tp * (1.0 - 1e-2) + p * 1e-2)
    return losses


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_twenty_step_loop(cuda, dtype, tol):
    nets0, _ = _nets(cuda)
    ref = _loop64(nets0, 20)
    got, _ = _loop(cuda, 20, dtype)
    for s, (a, b) in enumerate(zip(got, ref)):
        assert abs(a - b) <= tol * abs(b), (s, a, b)


def test_two_runs_bit_identical(cuda):
    l1, n1 = _loop(cuda, 5)
    l2, n2 = _loop(cuda, 5)
    assert l1 == l2
    for k in ("dqn", "target_dqn", "embeddings"):
        for p, q in zip(n1[k].parameters(), n2[k].parameters()):
            assert torch.equal(p, q)


class _Writer:
    def __init__(self):
        self.calls = []

    def add_scalar(self, *a, **k):
        self.calls.append(("scalar",) + a)

    def add_histogram(self, *a, **k):
        self.calls.append(("histogram",) + a)


def test_learn_false_changes_nothing(cuda):
    from recnn_amd.nn.update import dqn_update
    nets, opts = _nets(cuda)
    before = {k: [p.detach().clone() for p in n.parameters()] for k, n in nets.items()}
    w = _Writer()
    b = _batch(33, 10, 300, 9)
    out = dqn_update(b, {"gamma": 0.99}, nets, opts, writer=w, learn=False, step=12)
    for k, n in nets.items():
        for p, q in zip(n.parameters(), before[k]):
            assert torch.equal(p, q) and p.grad is None
    assert [c[0] for c in w.calls] == ["histogram", "scalar"]
    assert w.calls[0][1] == "q_values" and w.calls[1][1] == "value/test" and w.calls[1][3] == 12
    hist = w.calls[0][2]
    assert hist.shape == (33, 300)
    dqn64, tgt64, emb64, _, _ = _oracle(nets)
    loss64, q64, _ = R.autograd_step(dqn64, tgt64, emb64, _b64(b), 0.99, learn=False)
    assert _rel_err(hist.cpu(), q64) < 1e-4
    assert abs(out["value"] - loss64) <= 1e-4 * abs(loss64)
    assert abs(w.calls[1][2] - out["value"]) == 0


def test_fused_radam_matches_torch(cuda):
    from recnn_amd.optim import RAdam
    from recnn_amd import _lib as L
    gen = torch.Generator(cuda).manual_seed(2)
    p0 = torch.randn(1000, 33, device=cuda, generator=gen)
    a = torch.nn.Parameter(p0.clone())
    b = torch.nn.Parameter(p0.clone())
    oa, ob = RAdam([a], lr=1e-2, weight_decay=0.01), torch.optim.RAdam([b], lr=1e-2, weight_decay=0.01)
    for t in range(10):            # across the rectification threshold (t = 6 with the default betas)
        g = torch.randn(1000, 33, device=cuda, generator=gen)
        a.grad, b.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
        assert _rel_err(a.detach(), b.detach()) < 1e-6, t
    assert _rel_err(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"]) < 1e-6
    # the device clip coefficient: -1 / (|g|_1 + 1e-6), gradient written back
    g = torch.randn(1000, 33, device=cuda, generator=gen)
    a.grad, b.grad = g.clone(), g.clone()
    norm = torch.empty(1, device=cuda)
    part = torch.empty(1024, device=cuda)
    L.call("recnn_l1_norm_flat", L.ptr(a.grad), a.numel(), L.ptr(part), L.ptr(norm), L.current_stream())
    oa.step_clipped(norm, -1.0)
    torch.nn.utils.clip_grad_norm_([b], -1, 1)
    ob.step()
    assert _rel_err(a.grad, b.grad) < 1e-6
    assert _rel_err(a.detach(), b.detach()) < 1e-6
