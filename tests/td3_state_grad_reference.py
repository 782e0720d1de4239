"""Host restatements for the TD3 step's input gradients (test infrastructure, not an oracle file).

`input_grads`: the three gradients of recnn/nn/update/td3.py:88-132 with respect to `state`, written from the equations
    gV1 = dz_c1[0] W1c1[:, state columns]                  (value loss 1, critic 1 BEFORE its step)
    gV2 = dz_c1[1] W1c2[:, state columns]                  (value loss 2, critic 2 BEFORE its step)
    gP  = dz_e1 W1c1'[:, state columns] + dz_p1 W1a        (policy loss, critic 1 AFTER its step, then the actor)
on the oracle's hand-written MLP forward / backward, through `state_grad_reference.input_grads`.

`RefTD3`: the reference's whole update with a torch.nn.LSTM state encoder in front, in plain torch autograd on the CPU in float64 or
float32, in td3.py's statement order with retain_graph=True: value_optimizer1.zero_grad / value_loss1.backward / step,
value_optimizer2.zero_grad / value_loss2.backward / step -- TWO separate backward passes through the encoder --, then on a policy step
policy_optimizer.zero_grad / policy_loss.backward / clip_grad_norm_(policy_net.parameters(), -1, 1) / step / soft updates of the two
target critics (the target policy net is never soft-updated)."""

import torch

from oracle import recnn_oracle as O
import state_grad_reference as SG
from state_grad_reference import LSTM_PARAMS, fro, grad_bound, _mlp  # noqa: F401  (re-exported for the tests)

NET_KEYS = ("policy_net", "value_net1", "value_net2", "target_policy_net", "target_value_net1", "target_value_net2")


def td_target(target_policy, target_value1, target_value2, next_state, reward, done, noise, params):
    """td3.py:73-86: noise is the UNCLIPPED draw; no clamp of the target."""
    na, _ = O.actor_forward(target_policy, next_state)
    na = na + torch.clamp(noise.to(na.dtype), -params["noise_clip"], params["noise_clip"])
    tq1, _ = O.critic_forward(target_value1, next_state, na)
    tq2, _ = O.critic_forward(target_value2, next_state, na)
    return reward.reshape(-1, 1) + (1.0 - done.reshape(-1, 1)) * params["gamma"] * torch.min(tq1, tq2)


def input_grads(actor, critic1, critic2, critic1_updated, state, action, expected, masks):
    """(gV1, gV2, gP, {dz_c1, dz_c2, dz_e1, dz_p1}).  masks: the eight keep-masks in the reference's consumption order
    (critic 1 L1, L2 | critic 2 L1, L2 | actor L1, L2 | critic 1 L1, L2), or None (eval mode)."""
    m = list(masks) if masks is not None else None
    pick = lambda idx: None if m is None else [m[i] for i in idx]
    gV1, gP, d1 = SG.input_grads(actor, critic1, critic1_updated, state, action, expected, pick((0, 1, 4, 5, 6, 7)))
    gV2, _, d2 = SG.input_grads(actor, critic2, critic2, state, action, expected, pick((2, 3, 4, 5, 6, 7)))
    return gV1, gV2, gP, {"dz_c1": d1["dz_c1"], "dz_c2": d2["dz_c1"], "dz_e1": d1["dz_e1"], "dz_p1": d1["dz_p1"]}


class RefTD3:
    """nets: {name: oracle param dict} (float32 masters) for the six networks; lstm: a torch.nn.LSTM; make_opts(policy_params,
    encoder_params, value1_params, value2_params) -> (policy_optimizer, value_optimizer1, value_optimizer2)."""

    def __init__(self, dtype, table, user_dict, lstm, nets, make_opts, params):
        self.dtype, self.params = dtype, dict(params)
        self.table, self.user_dict = torch.as_tensor(table), user_dict
        self.lstm = torch.nn.LSTM(lstm.input_size, lstm.hidden_size, batch_first=True)
        self.lstm.load_state_dict({k: v.detach().cpu() for k, v in lstm.state_dict().items()})
        self.lstm = self.lstm.to(dtype)
        self.nets = {n: {k: torch.nn.Parameter(v.detach().cpu().to(dtype).clone()) for k, v in nets[n].items()} for n in NET_KEYS}
        for n in NET_KEYS[3:]:
            for v in self.nets[n].values():
                v.requires_grad_(False)
        plist = lambda n: [self.nets[n][k] for k in O.PARAM_ORDER]
        self.popt, self.vopt1, self.vopt2 = make_opts(plist("policy_net"), list(self.lstm.parameters()), plist("value_net1"),
                                                      plist("value_net2"))

    batch = SG.RefDDPG.batch

    def update(self, batch, masks, noise, step):
        N, P = self.nets, self.params
        m = list(masks) if masks is not None else [None] * 8
        state, action = batch["state"], batch["action"]
        # td3.py:73-86 (the target actor runs outside no_grad there too; everything that uses its output is inside)
        next_action = _mlp(N["target_policy_net"], batch["next_state"], None, None)
        next_action = next_action + torch.clamp(noise.to(self.dtype), -P["noise_clip"], P["noise_clip"])
        with torch.no_grad():
            xn = torch.cat([batch["next_state"], next_action], 1)
            tq = torch.min(_mlp(N["target_value_net1"], xn, None, None), _mlp(N["target_value_net2"], xn, None, None))
            expected = batch["reward"].reshape(-1, 1) + (1.0 - batch["done"].reshape(-1, 1)) * P["gamma"] * tq
        q1 = _mlp(N["value_net1"], torch.cat([state, action], 1), m[0], m[1])
        q2 = _mlp(N["value_net2"], torch.cat([state, action], 1), m[2], m[3])
        value_loss1 = (q1 - expected).pow(2).mean()
        value_loss2 = (q2 - expected).pow(2).mean()
        self.vopt1.zero_grad()
        value_loss1.backward(retain_graph=True)
        self.vopt1.step()
        self.vopt2.zero_grad()
        value_loss2.backward(retain_graph=True)
        self.vopt2.step()
        gen = _mlp(N["policy_net"], state, m[4], m[5])
        policy_loss = -_mlp(N["value_net1"], torch.cat([state, gen], 1), m[6], m[7]).mean()
        if step % P["policy_update"] == 0:
            self.popt.zero_grad()
            policy_loss.backward(retain_graph=True)
            pol = [N["policy_net"][k] for k in O.PARAM_ORDER]
            coef = min(-1.0 / (sum(float(p.grad.abs().sum()) for p in pol) + 1e-6), 1.0)     # clip_grad_norm_(.., -1, 1)
            with torch.no_grad():
                for p in pol:
                    p.grad.mul_(coef)
            self.popt.step()
            with torch.no_grad():
                for net, tgt in (("value_net1", "target_value_net1"), ("value_net2", "target_value_net2")):
                    for k in O.PARAM_ORDER:
                        N[tgt][k].copy_(N[tgt][k] * (1.0 - P["soft_tau"]) + N[net][k] * P["soft_tau"])
        return {"value1": float(value_loss1.detach()), "value2": float(value_loss2.detach()), "policy": float(policy_loss.detach())}

    def encoder_grads(self):
        return {n: (None if getattr(self.lstm, n).grad is None else getattr(self.lstm, n).grad.detach().double().clone()) for n in LSTM_PARAMS}

    def net_params(self):
        """The six networks' parameters (after the updates so far), float64 copies."""
        return {n: {k: v.detach().double().clone() for k, v in self.nets[n].items()} for n in NET_KEYS}
