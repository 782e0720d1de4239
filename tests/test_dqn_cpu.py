"""CPU: the dueling DQN of the embeddings notebook -- the two float64 forms of tests/dqn_reference.py agree (clip sign and torch's
RAdam across its rectification threshold included), `batch_no_embeddings` and its use through `prepare_batch_static_size`,
DuelDQN's parameter layout, argument errors and the `recnn.*` names.  Nothing here needs a GPU."""
import copy

import numpy as np
import pytest
import torch

import dqn_reference as R


def _setup(seed=0, F=3, N=40, n_emb=30):
    torch.manual_seed(seed)
    dqn = R.RefDuelDQN(F * 129, N).double()
    target = R.RefDuelDQN(F * 129, N).double()
    emb = torch.nn.Embedding(n_emb, 128).double()
    return dqn, target, emb


def test_structured_forms_match_autograd():
    F, N, B = 3, 40, 37
    dqn, target, emb = _setup(F=F, N=N)
    batch = R.make_batch(B, F, 30, torch.Generator().manual_seed(1))
    batch["action"] = batch["action"] % N
    st = R.structured_grads(dqn, target, emb.weight.detach(), batch, 0.99)
    # autograd, gradients before the clip
    x = torch.cat([emb(batch["items"]).view(B, -1), batch["ratings"]], 1)
    xn = torch.cat([emb(batch["next_items"]).view(B, -1), batch["next_ratings"]], 1)
    qv = dqn(x)
    with torch.no_grad():
        nq_all = target(xn)
    q = qv.gather(1, batch["action"].unsqueeze(1)).squeeze(1)
    y = batch["reward"] + 0.99 * nq_all.max(1)[0] * (1 - batch["done"])
    loss = (q - y).pow(2).mean()
    loss.backward()
    assert abs(float(loss.detach()) - st["loss"]) <= 1e-12 * abs(st["loss"])
    with torch.no_grad():
        a = dqn.advantage(dqn.feature(x))
        assert abs(float(a.mean()) - st["mu"]) < 1e-13
        at = target.advantage(target.feature(xn))
        np.testing.assert_allclose(at.max(1)[0].numpy(), st["next_max"].numpy(), rtol=1e-13, atol=1e-13)
    for name, p in dqn.named_parameters():
        np.testing.assert_allclose(p.grad.numpy(), st["grads"][name].numpy(), rtol=1e-10, atol=1e-14, err_msg=name)
    np.testing.assert_allclose(emb.weight.grad.numpy(), st["emb"].numpy(), rtol=1e-10, atol=1e-14)


def test_clip_negates_and_normalises():
    dqn, target, emb = _setup()
    batch = R.make_batch(16, 3, 30, torch.Generator().manual_seed(2))
    st = R.structured_grads(dqn, target, emb.weight.detach(), batch, 0.9)
    clipped, norm = R.clip_l1(st["grads"])
    assert norm > 0
    total = sum(float(v.abs().sum()) for v in clipped.values())
    assert abs(total - norm / (norm + 1e-6)) < 1e-9
    for k in clipped:
        assert torch.all(torch.sign(clipped[k]) == -torch.sign(st["grads"][k]))
    # torch's own clip gives the same coefficient (max_norm -1, L1)
    ps = [torch.nn.Parameter(v.clone()) for v in st["grads"].values()]
    for p, v in zip(ps, st["grads"].values()):
        p.grad = v.clone()
    tn = float(torch.nn.utils.clip_grad_norm_(ps, -1, 1))
    assert abs(tn - norm) <= 1e-12 * norm
    for p, k in zip(ps, clipped):
        np.testing.assert_allclose(p.grad.numpy(), clipped[k].numpy(), rtol=1e-12, atol=0)


def test_learn_loop_structured_vs_torch_radam_across_threshold():
    """Eight notebook steps (torch RAdam: rectified from t = 6 on with betas (0.9, 0.999)) against the structured gradients, the L1
    clip and the restated RAdam."""
    F, N = 3, 40
    dqn, target, emb = _setup(seed=3, F=F, N=N)
    dqn2, target2, emb2 = copy.deepcopy(dqn), copy.deepcopy(target), copy.deepcopy(emb)
    vo = torch.optim.RAdam(dqn.parameters(), lr=1e-3)
    eo = torch.optim.RAdam(emb.parameters(), lr=1e-3)
    opts = {k: R.RAdamRef(1e-3) for k in dict(dqn2.named_parameters())}
    eopt = R.RAdamRef(1e-3)
    gen = torch.Generator().manual_seed(4)
    for t in range(8):
        batch = R.make_batch(21, F, 30, gen)
        batch["action"] = batch["action"] % N
        l1, _, _ = R.autograd_step(dqn, target, emb, batch, 0.99, vo, eo)
        st = R.structured_grads(dqn2, target2, emb2.weight.detach(), batch, 0.99)
        assert abs(l1 - st["loss"]) <= 1e-9 * abs(st["loss"]) + 1e-12, t
        clipped, _ = R.clip_l1(st["grads"])
        with torch.no_grad():
            emb2.weight.copy_(eopt.step(emb2.weight.detach(), st["emb"]))
            for name, p in dqn2.named_parameters():
                p.copy_(opts[name].step(p.detach(), clipped[name]))
    assert vo.state[dqn.feature[0].weight]["step"] == 8
    for (name, p), p2 in zip(dqn.named_parameters(), dqn2.parameters()):
        np.testing.assert_allclose(p.detach().numpy(), p2.detach().numpy(), rtol=1e-9, atol=1e-12, err_msg=name)
    np.testing.assert_allclose(emb.weight.detach().numpy(), emb2.weight.detach().numpy(), rtol=1e-9, atol=1e-12)


def _user_batch(sizes, seed=0, n_items=50):
    rng = np.random.default_rng(seed)
    return [{"items": rng.integers(0, n_items, s), "rates": rng.standard_normal(s).astype(np.float32), "sizes": s, "users": u}
            for u, s in enumerate(sizes)]


def test_batch_no_embeddings_layout():
    from recnn_amd.data import batch_no_embeddings, rolling_window
    F = 4
    users = _user_batch([7, 5, 9])
    items = np.concatenate([rolling_window(u["items"], F + 1) for u in users])
    rates = np.concatenate([rolling_window(u["rates"], F + 1) for u in users])
    sizes = torch.tensor([7, 5, 9])
    b = batch_no_embeddings({"items": torch.tensor(items), "ratings": torch.tensor(rates), "sizes": sizes, "users": torch.arange(3)}, F)
    assert set(b) == {"items", "next_items", "ratings", "next_ratings", "action", "reward", "done", "meta"}
    B = items.shape[0]
    assert B == (7 - F) + (5 - F) + (9 - F)
    assert tuple(b["items"].shape) == (B, F) and tuple(b["next_items"].shape) == (B, F)
    assert tuple(b["ratings"].shape) == (B, F) and tuple(b["next_ratings"].shape) == (B, F)
    assert torch.equal(b["items"], torch.tensor(items[:, :-1])) and torch.equal(b["next_items"], torch.tensor(items[:, 1:]))
    assert torch.equal(b["action"], torch.tensor(items[:, -1])) and torch.equal(b["reward"], torch.tensor(rates[:, -1]))
    expect = torch.zeros(B)
    expect[torch.cumsum(sizes - F, 0) - 1] = 1
    assert torch.equal(b["done"], expect)
    assert b["done"].nonzero().flatten().tolist() == [2, 3, 8]
    assert torch.equal(b["meta"]["sizes"], sizes)


def test_prepare_batch_static_size_with_batch_no_embeddings():
    from recnn_amd.data import batch_no_embeddings, prepare_batch_static_size
    users = _user_batch([13, 11, 12], seed=5)
    b = prepare_batch_static_size(users, None, frame_size=10, embed_batch=batch_no_embeddings)
    assert tuple(b["items"].shape) == (3 + 1 + 2, 10)
    assert torch.equal(b["next_items"][0], torch.as_tensor(users[0]["items"][1:11]))
    assert int(b["action"][0]) == int(users[0]["items"][10])
    assert b["done"].tolist() == [0, 0, 1, 1, 0, 1]


def test_duel_dqn_layout_and_notebook_state_dict():
    from recnn_amd.nn import DuelDQN
    torch.manual_seed(7)
    m = DuelDQN(1290, 300)
    torch.manual_seed(7)
    ref = R.RefDuelDQN(1290, 300)
    sd, rsd = m.state_dict(), ref.state_dict()
    assert list(sd) == ["feature.0.weight", "feature.0.bias", "advantage.0.weight", "advantage.0.bias", "advantage.2.weight",
                        "advantage.2.bias", "value.0.weight", "value.0.bias", "value.2.weight", "value.2.bias"]
    assert list(sd) == list(rsd)
    for k in sd:
        assert sd[k].shape == rsd[k].shape
        assert torch.equal(sd[k], rsd[k]), k          # torch's default init, same RNG consumption
    other = R.RefDuelDQN(1290, 300).state_dict()
    m.load_state_dict(other)
    for k in other:
        assert torch.equal(m.state_dict()[k], other[k])


def test_cpu_tensors_raise_recnn_hip_error():
    from recnn_amd import _lib as L
    from recnn_amd.nn import DuelDQN
    m = DuelDQN(1290, 20)
    with pytest.raises(L.RecnnHipError):
        m(torch.zeros(2, 1290))


def _nets(n=20, F=2, emb=None):
    from recnn_amd.nn import DuelDQN
    return {"dqn": DuelDQN(F * 129, n), "target_dqn": DuelDQN(F * 129, n),
            "embeddings": emb if emb is not None else torch.nn.Embedding(n, 128)}


def _opts(nets):
    return {"value_optimizer": torch.optim.RAdam(nets["dqn"].parameters()),
            "embeddings_optimizer": torch.optim.RAdam(nets["embeddings"].parameters())}


def _list_batch(B=4, F=2, n=20):
    b = R.make_batch(B, F, n, torch.Generator().manual_seed(0))
    return [b[k] for k in ("items", "next_items", "ratings", "next_ratings", "action", "reward", "done")]


@pytest.mark.parametrize("kw", [dict(padding_idx=0), dict(max_norm=1.0), dict(sparse=True)])
def test_dqn_update_refuses_embedding_options(kw):
    from recnn_amd.nn.update import dqn_update
    nets = _nets(emb=torch.nn.Embedding(20, 128, **kw))
    with pytest.raises(ValueError, match="not supported"):
        dqn_update(_list_batch(), {"gamma": 0.99}, nets, _opts(nets))


def test_dqn_update_argument_errors():
    from recnn_amd import _lib as L
    from recnn_amd.nn.update import dqn_update
    nets = _nets()
    with pytest.raises(ValueError, match="7-element"):
        dqn_update(_list_batch()[:5], {"gamma": 0.99}, nets, _opts(nets))
    with pytest.raises(KeyError):
        dqn_update({"items": torch.zeros(2, 2)}, {"gamma": 0.99}, nets, _opts(nets))
    with pytest.raises(ValueError, match="embedding_dim"):
        n2 = _nets(emb=torch.nn.Embedding(20, 64))
        dqn_update(_list_batch(), {"gamma": 0.99}, n2, _opts(n2))
    with pytest.raises(L.RecnnHipError):
        dqn_update(_list_batch(), {"gamma": 0.99}, nets, _opts(nets))


def test_recnn_shim_names():
    import recnn
    import recnn_amd
    assert recnn.data.batch_no_embeddings is recnn_amd.data.utils.batch_no_embeddings
    assert recnn.nn.DuelDQN is recnn_amd.nn.models.DuelDQN
    assert recnn.nn.models.DuelDQN is recnn_amd.nn.models.DuelDQN
    assert recnn.nn.update.dqn_update is recnn_amd.nn.update.dqn.dqn_update
    assert recnn.optim.RAdam is recnn_amd.optim.RAdam
    assert "DuelDQN" in recnn_amd.nn.models.__all__
    assert "batch_no_embeddings" in recnn_amd.data.utils.__all__
    assert "dqn_update" in recnn_amd.nn.update.__all__


def test_radam_refuses_cpu_parameters():
    from recnn_amd import _lib as L
    from recnn_amd.optim import RAdam
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(L.RecnnHipError):
        RAdam([p]).step()
