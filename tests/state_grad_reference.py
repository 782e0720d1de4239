"""Host restatements for the DDPG step's input gradient (test infrastructure, not an oracle file).

`input_grads`: the two gradients of recnn/nn/update/ddpg.py:58-104 with respect to `state`, written from the equations
    gV = dz_c1 W1c[:, state columns]                      (value loss, the critic BEFORE its step)
    gP = dz_e1 W1c'[:, state columns] + dz_p1 W1a          (policy loss, the critic AFTER its step, then the actor)
on the oracle's hand-written MLP forward / backward (explicit keep-masks, the x2 of Dropout(0.5)), in whatever dtype it is given.

`RefDDPG`: the reference's whole update with a torch.nn.LSTM state encoder in front, in plain torch autograd on the CPU in float64 or
float32 -- value_optimizer.zero_grad / value_loss.backward(retain_graph) / step, then on a policy step policy_optimizer.zero_grad /
policy_loss.backward(retain_graph) / clip_grad_norm_(policy_net.parameters(), -1, 1) / step / soft updates."""

import numpy as np
import torch

from oracle import recnn_oracle as O
import seq_reference as R

NET_KEYS = ("policy_net", "value_net", "target_policy_net", "target_value_net")
LSTM_PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def td_target(target_policy, target_value, next_state, reward, done, params):
    na, _ = O.actor_forward(target_policy, next_state)
    tv, _ = O.critic_forward(target_value, next_state, na)
    return torch.clamp(reward.reshape(-1, 1) + (1.0 - done.reshape(-1, 1)) * params["gamma"] * tv, params["min_value"], params["max_value"])


def input_grads(actor, critic_v, critic_p, state, action, expected, masks):
    """(gV, gP, {dz_c1, dz_e1, dz_p1}).  masks: the six keep-masks in the reference's consumption order, or None (eval mode)."""
    m = list(masks) if masks is not None else [None] * 6
    B, S = state.shape
    train = masks is not None
    value, vcache = O.critic_forward(critic_v, state, action, m[0], m[1])
    _, _, iv = O.mlp_backward(critic_v, vcache, (value - expected) * (2.0 / B), train=train, need_dw=False)
    gV = iv["dz1"] @ critic_v["w1"][:, :S]
    gen, pcache = O.actor_forward(actor, state, m[2], m[3])
    q, qcache = O.critic_forward(critic_p, state, gen, m[4], m[5])
    _, dxa, ie = O.mlp_backward(critic_p, qcache, torch.full_like(q, -1.0 / B), train=train, need_dx=True, need_dw=False)
    _, _, ip = O.mlp_backward(actor, pcache, dxa[:, S:], train=train, need_dw=False)
    gP = ie["dz1"] @ critic_p["w1"][:, :S] + ip["dz1"] @ actor["w1"]
    return gV, gP, {"dz_c1": iv["dz1"], "dz_e1": ie["dz1"], "dz_p1": ip["dz1"]}


def _mlp(p, x, m1, m2):
    drop = lambda h, m: h if m is None else h * (m.to(h.dtype) * 2.0)
    h1 = drop(torch.relu(x @ p["w1"].t() + p["b1"]), m1)
    h2 = drop(torch.relu(h1 @ p["w2"].t() + p["b2"]), m2)
    return h2 @ p["w3"].t() + p["b3"]


class RefDDPG:
    """nets: {name: oracle param dict} (float32 masters); lstm: a torch.nn.LSTM; make_opts(policy_params, encoder_params,
    value_params) -> (policy_optimizer, value_optimizer) over the torch Parameters it is handed."""

    def __init__(self, dtype, table, user_dict, lstm, nets, make_opts, params):
        self.dtype, self.params = dtype, dict(params)
        self.table, self.user_dict = torch.as_tensor(table), user_dict
        self.lstm = torch.nn.LSTM(lstm.input_size, lstm.hidden_size, batch_first=True)
        self.lstm.load_state_dict({k: v.detach().cpu() for k, v in lstm.state_dict().items()})
        self.lstm = self.lstm.to(dtype)
        self.nets = {n: {k: torch.nn.Parameter(v.detach().cpu().to(dtype).clone()) for k, v in nets[n].items()} for n in NET_KEYS}
        for n in ("target_policy_net", "target_value_net"):
            for v in self.nets[n].values():
                v.requires_grad_(False)
        pol = [self.nets["policy_net"][k] for k in O.PARAM_ORDER]
        val = [self.nets["value_net"][k] for k in O.PARAM_ORDER]
        self.popt, self.vopt = make_opts(pol, list(self.lstm.parameters()), val)

    def batch(self, ids, steps, attached=True):
        items = [self.user_dict[u]["items"] for u in ids]
        ratings = [self.user_dict[u]["ratings"] for u in ids]
        E = self.table.shape[1]
        x = R.lstm_inputs(self.table, items, ratings, steps[-1] + 1).to(self.dtype)
        with torch.enable_grad() if attached else torch.no_grad():
            h, _ = self.lstm(x)
            state = torch.cat([h[:, t - 1] for t in steps], 0)
            next_state = torch.cat([h[:, t] for t in steps], 0)
        return {"state": state, "next_state": next_state, "action": torch.cat([x[:, t, :E] for t in steps], 0),
                "reward": torch.cat([x[:, t, E] for t in steps], 0), "done": torch.zeros(len(ids) * len(steps), dtype=self.dtype)}

    def update(self, batch, masks, step):
        N, P = self.nets, self.params
        m = list(masks) if masks is not None else [None] * 6
        with torch.no_grad():
            expected = td_target(N["target_policy_net"], N["target_value_net"], batch["next_state"], batch["reward"], batch["done"], P)
        value = _mlp(N["value_net"], torch.cat([batch["state"], batch["action"]], 1), m[0], m[1])
        value_loss = (value - expected).pow(2).mean()
        self.vopt.zero_grad()
        value_loss.backward(retain_graph=True)
        self.vopt.step()
        gen = _mlp(N["policy_net"], batch["state"], m[2], m[3])
        policy_loss = -_mlp(N["value_net"], torch.cat([batch["state"], gen], 1), m[4], m[5]).mean()
        if step % P["policy_step"] == 0:
            self.popt.zero_grad()
            policy_loss.backward(retain_graph=True)
            pol = [N["policy_net"][k] for k in O.PARAM_ORDER]
            coef = min(-1.0 / (sum(float(p.grad.abs().sum()) for p in pol) + 1e-6), 1.0)     # clip_grad_norm_(.., -1, 1)
            with torch.no_grad():
                for p in pol:
                    p.grad.mul_(coef)
            self.popt.step()
            with torch.no_grad():
                for net, tgt in (("value_net", "target_value_net"), ("policy_net", "target_policy_net")):
                    for k in O.PARAM_ORDER:
                        N[tgt][k].copy_(N[tgt][k] * (1.0 - P["soft_tau"]) + N[net][k] * P["soft_tau"])
        return {"value": float(value_loss.detach()), "policy": float(policy_loss.detach())}

    def encoder_grads(self):
        return {n: (None if getattr(self.lstm, n).grad is None else getattr(self.lstm, n).grad.detach().double().clone()) for n in LSTM_PARAMS}


def fro(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def grad_bound(g32, g64, U, T):
    """max(4 ||G32cpu - G64|| / ||G64||, 2^-23 max(8, sqrt(U T))): relative Frobenius bound of one tensor."""
    return max(4.0 * fro(g32, g64), 2.0 ** -23 * max(8.0, float(np.sqrt(U * T))))
