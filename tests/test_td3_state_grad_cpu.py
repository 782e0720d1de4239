"""The TD3 step's input gradients without a GPU: the restatement the GPU tests compare against (tests/td3_state_grad_reference.py)
against autograd, the one-backward identity the attached route of `td3_update` rests on, and next_state's missing gradient."""
import torch

import seq_reference as R
import td3_state_grad_reference as TG
from oracle import recnn_oracle as O

PARAMS = {"gamma": 0.99, "noise_std": 0.5, "noise_clip": 0.7, "soft_tau": 0.01, "policy_update": 2}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_closed_forms_equal_autograd_through_the_modules():
    """gV1 / gV2 / gP from the equations against autograd through the layers of recnn.nn.Critic / Actor in float64 (1e-12 relative),
    with keep-masks.  Critic 1 of the policy loss is "critic 1 after its step": just another critic."""
    import recnn
    S, A, H, B = 27, 8, 16, 5
    torch.manual_seed(5)
    actor = recnn.nn.Actor(S, A, H, 6e-1).double()
    c1, c2, c1u = (recnn.nn.Critic(S, A, H, 54e-2).double() for _ in range(3))
    g = torch.Generator().manual_seed(6)
    state = torch.randn(B, S, generator=g, dtype=torch.float64)
    action = torch.randn(B, A, generator=g, dtype=torch.float64)
    expected = torch.randn(B, 1, generator=g, dtype=torch.float64)
    masks = [(torch.rand(B, H, generator=g) < 0.5).to(torch.uint8) for _ in range(8)]

    def run(mod, x, m1, m2):
        h1 = torch.relu(mod.linear1(x)) * (m1.double() * 2.0)
        h2 = torch.relu(mod.linear2(h1)) * (m2.double() * 2.0)
        return mod.linear3(h2)

    auto = []
    for crit, (ma, mb) in ((c1, masks[0:2]), (c2, masks[2:4])):
        s = state.clone().requires_grad_(True)
        auto.append(torch.autograd.grad((run(crit, torch.cat([s, action], 1), ma, mb) - expected).pow(2).mean(), s)[0])
    s = state.clone().requires_grad_(True)
    policy_loss = -run(c1u, torch.cat([s, run(actor, s, masks[4], masks[5])], 1), masks[6], masks[7]).mean()
    auto.append(torch.autograd.grad(policy_loss, s)[0])

    as_p = lambda m: {k: v.double() for k, v in zip(O.PARAM_ORDER, (p.detach() for p in m.parameters()))}
    gV1, gV2, gP, dz = TG.input_grads(as_p(actor), as_p(c1), as_p(c2), as_p(c1u), state, action, expected, masks)
    errs = [_rel(a, b) for a, b in zip((gV1, gV2, gP), auto)]
    print("closed forms vs autograd (relative max): gV1 %.3e gV2 %.3e gP %.3e" % tuple(errs))
    assert all(float(t.abs().max()) > 0 for t in auto)
    assert not torch.equal(gV1, gV2)
    assert all(e <= 1e-12 for e in errs)
    # the forms as the launch computes them: layer-1 pre-activation gradients times the state columns
    assert _rel(dz["dz_c1"] @ as_p(c1)["w1"][:, :S] + dz["dz_c2"] @ as_p(c2)["w1"][:, :S], auto[0] + auto[1]) <= 1e-12


def _ref(dtype=torch.float64):
    table, user_dict, users, lstm = R.seq_env_data()
    torch.manual_seed(9)
    S, A, H = lstm.hidden_size, table.shape[1], 16
    mk = lambda i, o: {"w1": torch.randn(H, i) * 0.2, "b1": torch.randn(H) * 0.1, "w2": torch.randn(H, H) * 0.2, "b2": torch.randn(H) * 0.1,
                       "w3": torch.randn(o, H) * 0.3, "b3": torch.randn(o) * 0.3}
    pol, v1, v2 = mk(S, A), mk(S + A, 1), mk(S + A, 1)
    snap = {"policy_net": pol, "value_net1": v1, "value_net2": v2, "target_policy_net": pol, "target_value_net1": v1, "target_value_net2": v2}
    sgd = lambda p, e, a, b: (torch.optim.SGD(p + e, lr=1e-2), torch.optim.SGD(a, lr=1e-2), torch.optim.SGD(b, lr=1e-2))
    return TG.RefTD3(dtype, table, user_dict, lstm, snap, sgd, PARAMS), (S, A, H)


def test_one_backward_for_both_value_losses_equals_two():
    """The encoder's backward is linear in the gradient it is handed: gV1 + gV2 pushed through it once gives the encoder gradients
    of the reference's two separate value backwards (RefTD3 at a step that is no policy step), to 1e-12 relative."""
    ref, (S, A, H) = _ref()
    ids, steps = [0, 1, 2, 3, 4], [3, 7, 20]
    rows = len(ids) * len(steps)
    g = torch.Generator().manual_seed(2)
    masks = [(torch.rand(rows, H, generator=g) < 0.5).to(torch.uint8) for _ in range(8)]
    noise = torch.randn(rows, A, generator=g, dtype=torch.float64) * 0.5
    before = ref.net_params()
    batch = ref.batch(ids, steps)
    ref.update(batch, masks, noise, 1)
    two = ref.encoder_grads()

    again, _ = _ref()
    b2 = again.batch(ids, steps)
    with torch.no_grad():
        expected = TG.td_target(before["target_policy_net"], before["target_value_net1"], before["target_value_net2"], b2["next_state"],
                                b2["reward"], b2["done"], noise, PARAMS)
        gV1, gV2, _, _ = TG.input_grads(before["policy_net"], before["value_net1"], before["value_net2"], before["value_net1"],
                                        b2["state"].detach(), b2["action"], expected, masks)
    torch.autograd.backward([b2["state"]], [gV1 + gV2])
    one = again.encoder_grads()
    for n in TG.LSTM_PARAMS:
        e = _rel(one[n], two[n])
        print(f"one backward vs two, {n}: {e:.3e} (max |g| {float(two[n].abs().max()):.3e})")
        assert float(two[n].abs().max()) > 0 and e <= 1e-12


def test_next_state_gets_no_gradient():
    ref, (S, A, H) = _ref()
    batch = ref.batch([0, 1, 2], [3, 7])
    batch["state"] = batch["state"].detach().requires_grad_(True)
    batch["next_state"] = batch["next_state"].detach().requires_grad_(True)
    ref.update(batch, None, torch.zeros(6, A, dtype=torch.float64), 0)
    assert batch["next_state"].grad is None
    assert batch["state"].grad is not None and float(batch["state"].grad.abs().max()) > 0
