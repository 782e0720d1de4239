"""Training the LSTM state encoder on the GPU (csrc/lstm.hip, csrc/seq_bwd.h): the training forward against `lstm_encode` bit for bit, the
gradients of `lstm_encode_train` against torch.nn.LSTM under autograd in float64 on the CPU (tests/seq_grad_reference.py), the
differentiable collect, `SeqEnv.user_batch`, and one small problem on which the encoder must actually learn.

The bound of a gradient tensor G comes from the reference alone (seq_grad_reference.grad_bounds):
max(4 max |G32cpu - G64cpu|, 2^-23 max(8, sqrt(U T)) max |G64|).  Every test prints its measured error next to the bound before it
asserts."""
import numpy as np
import pytest
import torch

import seq_grad_reference as G
import seq_reference as R
from helpers import csr, make_store

pytestmark = pytest.mark.gpu

T_MAX = 37
SHAPES = ((8, 16), (128, 256))


@pytest.fixture(scope="module")
def seq_data():
    """Per (E, H): 25 users with at least T_MAX + 1 elements, their table and an LSTM(E + 1, H) (CPU master copies)."""
    out = {}
    for E, H in SHAPES:
        items, ratings, table = make_store(25, 300, E, T_MAX + 1, T_MAX + 9, seed=E)
        torch.manual_seed(E)
        out[(E, H)] = (items, ratings, torch.from_numpy(table), torch.nn.LSTM(E + 1, H))
    return out


@pytest.fixture(scope="module")
def references():
    """Float64 / float32 CPU gradients and bounds, computed once per case and shared (never modified)."""
    return {}


def _on_gpu(cuda, data):
    from recnn_amd.data.store import ReplayStore
    items, ratings, table, lstm = data
    gl = torch.nn.LSTM(lstm.input_size, lstm.hidden_size).to(cuda)
    gl.load_state_dict(lstm.state_dict())
    return ReplayStore.from_arrays(*csr(items, ratings), cuda), table.to(cuda), gl


def _h0c0(U, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(U, H, generator=g) * 0.5, torch.randn(U, H, generator=g) * 0.5


def _reference(references, seq_data, EH, slots, T, with_h0, use="all"):
    key = (EH, tuple(int(s) for s in slots), T, with_h0, use)
    if key not in references:
        items, ratings, table, lstm = seq_data[EH]
        U = len(slots)
        x = R.lstm_inputs(table, [items[s] for s in slots], [ratings[s] for s in slots], T)
        hc = _h0c0(U, EH[1], U) if with_h0 else None
        Rw = G.loss_weights(U, T, EH[1], seed=T + U)
        references[key] = (hc, Rw) + G.grad_bounds(lstm, x, hc, Rw, use)
    return references[key]


def _gpu_grads(cuda, gl, st, tbl, slots, T, hc, Rw, use="all"):
    """{name: gradient on the CPU} of the loss over lstm_encode_train."""
    from recnn_amd.nn import functional as F
    gl.zero_grad(set_to_none=True)
    hcg = None if hc is None else tuple(t.to(cuda).requires_grad_(True) for t in hc)
    h, (hT, cT) = F.lstm_encode_train(gl, st, tbl, slots, T, hcg)
    G.loss_of(h, hT, cT, Rw, use).backward()
    out = {n: getattr(gl, n).grad.cpu() for n in G.PARAMS}
    if hcg is not None:
        out["h0"], out["c0"] = hcg[0].grad.cpu(), hcg[1].grad.cpu()
    return out


def _check(tag, got, g64, bounds):
    worst = []
    for n in g64:
        err = float((got[n].double() - g64[n]).abs().max())
        print(f"{tag} {n}: err {err:.3e} bound {bounds[n]:.3e} max|G| {float(g64[n].abs().max()):.3e}")
        if not err <= bounds[n]:
            worst.append((n, err, bounds[n]))
    assert not worst, (tag, worst)


# ---------------------------------------------------------------------------------------------------- training forward
@pytest.mark.parametrize("EH", SHAPES)
def test_training_forward_equals_lstm_encode_bit_for_bit(cuda, seq_data, EH):
    from recnn_amd.nn import functional as F
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    for U in (5, 25):
        slots = np.arange(25 - U, 25, dtype=np.int32)
        for T in (1, T_MAX):
            for hc in (None, tuple(t.to(cuda) for t in _h0c0(U, EH[1], U))):
                for variant in ("fused", "chunked"):
                    F.set_lstm_variant(variant)
                    try:
                        h, (hT, cT) = F.lstm_encode(gl, st, tbl, slots, T, hc)
                        ht, (hTt, cTt) = F.lstm_encode_train(gl, st, tbl, slots, T, hc)
                    finally:
                        F.set_lstm_variant("chunked")
                    assert ht.requires_grad and hTt.requires_grad and cTt.requires_grad and not h.requires_grad
                    assert torch.equal(ht, h) and torch.equal(hTt, hT) and torch.equal(cTt, cT), (U, T, variant)
    with torch.no_grad():                                            # the inference path: no graph, nothing saved
        ht, _ = F.lstm_encode_train(gl, st, tbl, slots, 3)
    assert not ht.requires_grad and ht.grad_fn is None


# ---------------------------------------------------------------------------------------------------- gradients
@pytest.mark.parametrize("U", [5, 25])
@pytest.mark.parametrize("EH", SHAPES)
def test_gradients_against_float64(cuda, seq_data, references, EH, U):
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    slots = np.arange(25 - U, 25, dtype=np.int32)
    for T, with_h0 in ((T_MAX, True), (T_MAX, False), (1, True)):
        hc, Rw, bounds, g64 = _reference(references, seq_data, EH, slots, T, with_h0)
        got = _gpu_grads(cuda, gl, st, tbl, slots, T, hc, Rw)
        assert torch.equal(got["bias_ih_l0"], got["bias_hh_l0"])
        _check(f"grad E,H={EH} U={U} T={T} h0={'set' if with_h0 else 'zero'}", got, g64, bounds)


@pytest.mark.parametrize("use", ["final", "head"])
@pytest.mark.parametrize("EH", SHAPES)
def test_partial_losses(cuda, seq_data, references, EH, use):
    """"final": only h_T and c_T are used, the gradient of h is absent; "head": only h[:, :20], later steps carry zeros."""
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    slots = np.arange(25, dtype=np.int32)
    hc, Rw, bounds, g64 = _reference(references, seq_data, EH, slots, T_MAX, True, use)
    got = _gpu_grads(cuda, gl, st, tbl, slots, T_MAX, hc, Rw, use)
    _check(f"partial loss {use} E,H={EH}", got, g64, bounds)


def test_carry_across_calls(cuda, seq_data, references):
    """37 steps as one call against 20 + 17 with (h_T, c_T) carried and requiring grad."""
    from recnn_amd.nn import functional as F
    EH = (128, 256)
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    slots = np.arange(8, 25, dtype=np.int32)
    hc, Rw, bounds, g64 = _reference(references, seq_data, EH, slots, T_MAX, True)
    one = _gpu_grads(cuda, gl, st, tbl, slots, T_MAX, hc, Rw)
    gl.zero_grad(set_to_none=True)
    hcg = tuple(t.to(cuda).requires_grad_(True) for t in hc)
    ha, hca = F.lstm_encode_train(gl, st, tbl, slots, 20, hcg)
    assert hca[0].requires_grad and hca[1].requires_grad
    hb, (hT, cT) = F.lstm_encode_train(gl, st, tbl, slots, 17, hca, t0=20)
    G.loss_of(torch.cat([ha, hb], 1), hT, cT, Rw).backward()
    two = {n: getattr(gl, n).grad.cpu() for n in G.PARAMS}
    two["h0"], two["c0"] = hcg[0].grad.cpu(), hcg[1].grad.cpu()
    assert torch.equal(two["h0"], one["h0"]) and torch.equal(two["c0"], one["c0"])
    _check("carry 20 + 17 vs float64", two, g64, bounds)
    for n in G.PARAMS:                                               # the grouping of the sums differs across the cut
        err = float((two[n].double() - one[n].double()).abs().max())
        print(f"carry 20 + 17 vs one call {n}: diff {err:.3e} bound {bounds[n]:.3e}")
        assert err <= bounds[n]


def test_run_to_run_and_user_permutation(cuda, seq_data, references):
    EH = (128, 256)
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    slots = np.arange(8, 25, dtype=np.int32)
    hc, Rw, _, _ = _reference(references, seq_data, EH, slots, T_MAX, True)
    a = _gpu_grads(cuda, gl, st, tbl, slots, T_MAX, hc, Rw)
    b = _gpu_grads(cuda, gl, st, tbl, slots, T_MAX, hc, Rw)
    for n in G.NAMES:
        assert torch.equal(a[n], b[n]), n
    perm = np.random.default_rng(0).permutation(len(slots))
    pt = torch.from_numpy(perm)
    p = _gpu_grads(cuda, gl, st, tbl, slots[perm], T_MAX, tuple(t[pt] for t in hc), tuple(r[pt] for r in Rw))
    assert torch.equal(p["h0"], a["h0"][pt]) and torch.equal(p["c0"], a["c0"][pt])


# ---------------------------------------------------------------------------------------------------- collect
def test_seq_collect_rows(cuda, seq_data):
    from recnn_amd.nn import functional as F
    EH = (8, 16)
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    U, H, E, T = 7, 16, 8, 12
    slots = np.arange(3, 3 + U, dtype=np.int32)
    steps = [3, 4, 9]
    h, _ = F.lstm_encode(gl, st, tbl, slots, T)
    views = (torch.empty(3 * U, H, device=cuda), torch.empty(3 * U, E, device=cuda), torch.empty(3 * U, 1, device=cuda),
             torch.empty(3 * U, H, device=cuda))
    F.seq_collect(h, steps, st, tbl, slots, views)
    hg = h.clone().requires_grad_(True)
    rows = F.seq_collect_rows(hg, steps, st, tbl, slots)
    for got, want in zip(rows, views):
        assert got.shape == want.shape and torch.equal(got, want)
    assert rows[0].requires_grad and rows[3].requires_grad and not rows[1].requires_grad and not rows[2].requires_grad
    g = torch.Generator().manual_seed(1)
    gs, gn = torch.randn(3 * U, H, generator=g).to(cuda), torch.randn(3 * U, H, generator=g).to(cuda)
    ((rows[0] * gs).sum() + (rows[3] * gn).sum()).backward()
    idx = torch.tensor(steps, device=cuda)
    want = torch.zeros(U, T, H, device=cuda)
    want.index_add_(1, idx, gn.view(3, U, H).transpose(0, 1).contiguous())
    want.index_add_(1, idx - 1, gs.view(3, U, H).transpose(0, 1).contiguous())
    assert torch.equal(hg.grad, want)
    live = want.abs().sum((0, 2)).ne(0).cpu().tolist()
    assert [t for t, v in enumerate(live) if v] == [2, 3, 4, 8, 9]
    assert torch.equal(hg.grad[:, 3], gn.view(3, U, H)[0] + gs.view(3, U, H)[1])      # two contributions
    # one of the two gradients absent
    hg2 = h.clone().requires_grad_(True)
    (F.seq_collect_rows(hg2, steps, st, tbl, slots)[0] * gs).sum().backward()
    want2 = torch.zeros(U, T, H, device=cuda).index_add_(1, idx - 1, gs.view(3, U, H).transpose(0, 1).contiguous())
    assert torch.equal(hg2.grad, want2)
    for bad in ([4, 3, 9], [3, 3, 9]):
        with pytest.raises(ValueError, match="strictly increasing"):
            F.seq_collect_rows(hg, bad, st, tbl, slots)


# ---------------------------------------------------------------------------------------------------- SeqEnv.user_batch
def _env(cuda, table, user_dict, users, lstm):
    from recnn_amd.data.env import SeqEnv
    gl = torch.nn.LSTM(lstm.input_size, lstm.hidden_size).to(cuda)
    gl.load_state_dict(lstm.state_dict())
    return SeqEnv.from_user_dict(table, user_dict, users, state_encoder=gl, batch_size=5, max_buf_size=20, device=cuda)


def test_user_batch(cuda):
    import recnn
    from recnn_amd.nn import functional as F
    env = _env(cuda, *R.seq_env_data())
    ids, steps = [0, 1, 2, 3, 4], [3, 4, 9, 30]
    batch = env.user_batch(ids, steps)
    assert set(batch) == {"state", "action", "reward", "next_state", "done", "meta"}
    assert batch["meta"]["step"] == steps and batch["meta"]["users"] == ids and batch["meta"]["rows"] == 20
    slots = env.store.slots(ids)
    h, _ = F.lstm_encode(env.state_encoder, env.store, env.table, slots, steps[-1] + 1)
    views = (torch.empty(20, 16, device=cuda), torch.empty(20, 8, device=cuda), torch.empty(20, 1, device=cuda),
             torch.empty(20, 16, device=cuda))
    F.seq_collect(h, steps, env.store, env.table, slots, views)
    for key, want in zip(("state", "action", "reward", "next_state"), views):
        assert torch.equal(batch[key], want), key
    assert batch["state"].requires_grad and batch["next_state"].requires_grad and not batch["action"].requires_grad
    assert not batch["done"].any() and batch["done"].shape == (20,)
    # through an eval-mode critic: a squared TD-style loss reaches all four LSTM parameters
    torch.manual_seed(0)
    critic = recnn.nn.Critic(16, 8, 32).to(cuda).eval()
    q = critic(batch["state"], batch["action"])
    target = batch["reward"] + 0.99 * critic(batch["next_state"], batch["action"])
    (q - target.detach() + 0.1 * target).pow(2).mean().backward()
    for n in G.PARAMS:
        g = getattr(env.state_encoder, n).grad
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0, n
    # state.requires_grad holds exactly when an encoder parameter does
    with torch.no_grad():
        assert not env.user_batch(ids, steps)["state"].requires_grad
    for p in env.state_encoder.parameters():
        p.requires_grad_(False)
    frozen = env.user_batch(ids, steps)
    assert not frozen["state"].requires_grad and not frozen["next_state"].requires_grad
    assert torch.equal(frozen["state"], views[0]) and torch.equal(frozen["next_state"], views[3])
    env.state_encoder.bias_hh_l0.requires_grad_(True)
    assert env.user_batch(ids, steps)["state"].requires_grad
    for bad in ([0, 3], [3, 37], [4, 3]):
        with pytest.raises(ValueError):
            env.user_batch(ids, bad)


def test_training_works(cuda):
    """Plain SGD on the encoder through user_batch: the GPU run's relative fall of the loss is at least half of the float64 CPU
    restatement's (which falls by at least 10 % at the learning rate the helper chose on it)."""
    table, user_dict, users, lstm, steps, (w_read, b_read), lr, ref_losses = G.training_case()
    env = _env(cuda, table, user_dict, list(range(12)), lstm)
    opt = torch.optim.SGD(env.state_encoder.parameters(), lr=lr)
    w, b = w_read.to(cuda), b_read.to(cuda)
    losses = []
    for _ in range(G.TRAIN_SGD_STEPS + 1):
        batch = env.user_batch(users, steps)                         # rows k * U + u
        loss = ((batch["next_state"] @ w + b) - batch["reward"]).pow(2).mean()
        losses.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    fall, ref_fall = 1.0 - losses[-1] / losses[0], 1.0 - ref_losses[-1] / ref_losses[0]
    print(f"training: lr {lr} float64 loss {ref_losses[0]:.6f} -> {ref_losses[-1]:.6f} (fall {ref_fall:.4f}), "
          f"GPU loss {losses[0]:.6f} -> {losses[-1]:.6f} (fall {fall:.4f})")
    assert ref_fall >= 0.1 and np.isfinite(losses).all()
    assert fall >= 0.5 * ref_fall


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_by_name(cuda, seq_data):
    import warnings
    from recnn_amd import _lib as L
    from recnn_amd.nn import functional as F
    st, tbl, gl = _on_gpu(cuda, seq_data[(8, 16)])
    with pytest.raises(L.RecnnHipError, match="table.requires_grad"):
        F.lstm_encode_train(gl, st, tbl.clone().requires_grad_(True), [0, 1], 4)
    with pytest.raises(L.RecnnHipError, match="weight_ih_l0.device"):
        F.lstm_encode_train(torch.nn.LSTM(9, 16), st, tbl, [0, 1], 4)
    for kw, attr in ((dict(num_layers=2), "num_layers"), (dict(bidirectional=True), "bidirectional"), (dict(proj_size=8), "proj_size"),
                     (dict(num_layers=1, dropout=0.5), "dropout"), (dict(bias=False), "bias")):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            bad = torch.nn.LSTM(9, 16, **kw).to(cuda)
        with pytest.raises(L.RecnnHipError, match=attr):
            F.lstm_encode_train(bad, st, tbl, [0, 1], 4)
    h, _ = F.lstm_encode_train(gl, st, tbl, [0, 1], 4)
    # a loss whose gradient with respect to h itself depends on h: only then does the first backward hand out a graph to refuse
    (g,) = torch.autograd.grad((h * h).sum(), gl.weight_hh_l0, create_graph=True)
    assert g.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
