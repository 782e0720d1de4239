"""Float64 restatement of the embeddings notebook's dueling DQN step, in two forms:

  * `autograd_step`: torch autograd on a notebook-shaped module (`RefDuelDQN`), the notebook's order of operations
    (zero grads, backward, clip_grad_norm_(dqn, -1, 1), embeddings step, DQN step);
  * `structured_grads`: the closed forms the kernels use (mean from column sums, gathered-row Q, scatter-sums, rank-1 terms).

Written from the algebra, not from the notebook's cells.  Everything runs on the CPU.
"""
import math

import torch
import torch.nn as nn


class RefDuelDQN(nn.Module):
    def __init__(self, input_dim, action_dim):
        super().__init__()
        self.feature = nn.Sequential(nn.Linear(input_dim, 128), nn.ReLU())
        self.advantage = nn.Sequential(nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, action_dim))
        self.value = nn.Sequential(nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 1))

    def forward(self, x):
        x = self.feature(x)
        a = self.advantage(x)
        return self.value(x) + a - a.mean()


def make_batch(B, F, n_items, gen, done_every=7):
    items_full = torch.randint(0, n_items, (B, F + 1), generator=gen)
    ratings_full = torch.randn(B, F + 1, generator=gen, dtype=torch.float64)
    done = torch.zeros(B, dtype=torch.float64)
    done[done_every - 1::done_every] = 1
    return {"items": items_full[:, :-1], "next_items": items_full[:, 1:], "ratings": ratings_full[:, :-1],
            "next_ratings": ratings_full[:, 1:], "action": items_full[:, -1], "reward": ratings_full[:, -1], "done": done}


def state_of(emb_w, items, ratings):
    B = items.shape[0]
    return torch.cat([emb_w[items].reshape(B, -1), ratings.to(emb_w.dtype)], 1)


def autograd_step(dqn, target, emb, batch, gamma, value_opt=None, emb_opt=None, learn=True):
    """One notebook step in place (float64 modules).  Returns (loss, Q(state) [B, N], clip L1 norm before the clip)."""
    B = batch["items"].shape[0]
    state = torch.cat([emb(batch["items"]).view(B, -1), batch["ratings"].to(emb.weight.dtype)], 1)
    next_state = torch.cat([emb(batch["next_items"]).view(B, -1), batch["next_ratings"].to(emb.weight.dtype)], 1)
    qv = dqn(state)
    with torch.no_grad():
        nq = target(next_state)
    q = qv.gather(1, batch["action"].unsqueeze(1)).squeeze(1)
    y = batch["reward"].to(qv.dtype) + gamma * nq.max(1)[0] * (1 - batch["done"].to(qv.dtype))
    loss = (q - y).pow(2).mean()
    norm = None
    if learn:
        emb_opt.zero_grad()
        value_opt.zero_grad()
        loss.backward()
        norm = float(torch.nn.utils.clip_grad_norm_(dqn.parameters(), -1, 1))
        emb_opt.step()
        value_opt.step()
    return float(loss), qv.detach(), norm


def structured_grads(dqn, target, emb_w, batch, gamma):
    """The kernels' closed forms in float64: returns dict with loss, mu, mu_t, next_max, and the UNCLIPPED gradients of every DQN
    parameter (state_dict names) and of the embedding table."""
    with torch.no_grad():
        B = batch["items"].shape[0]
        F = batch["items"].shape[1]
        P = {k: v.double() for k, v in dqn.state_dict().items()}
        T = {k: v.double() for k, v in target.state_dict().items()}
        ew = emb_w.double()
        a = batch["action"]

        def trunk(p, x):
            f = torch.relu(x @ p["feature.0.weight"].T + p["feature.0.bias"])
            ha = torch.relu(f @ p["advantage.0.weight"].T + p["advantage.0.bias"])
            hv = torch.relu(f @ p["value.0.weight"].T + p["value.0.bias"])
            return f, ha, hv

        x = state_of(ew, batch["items"], batch["ratings"])
        xn = state_of(ew, batch["next_items"], batch["next_ratings"])
        f, ha, hv = trunk(P, x)
        _, hat, hvt = trunk(T, xn)
        W, c = P["advantage.2.weight"], P["advantage.2.bias"]
        Wt, ct = T["advantage.2.weight"], T["advantage.2.bias"]
        N = W.shape[0]
        V = hv @ P["value.2.weight"][0] + P["value.2.bias"][0]
        Vt = hvt @ T["value.2.weight"][0] + T["value.2.bias"][0]
        mu = ha.sum(0) @ W.sum(0) / (B * N) + c.mean()
        mut = hat.sum(0) @ Wt.sum(0) / (B * N) + ct.mean()
        q = V + (ha * W[a]).sum(1) + c[a] - mu
        next_max = (hat @ Wt.T + ct).max(1)[0]
        nq = Vt + next_max - mut
        y = batch["reward"].double() + gamma * nq * (1 - batch["done"].double())
        g = 2 * (q - y) / B
        G = g.sum()
        kappa = G / (B * N)
        dW = torch.zeros_like(W).index_add_(0, a, g[:, None] * ha) - kappa * ha.sum(0)[None, :]
        dc = torch.zeros_like(c).index_add_(0, a, g) - G / N
        dha = (g[:, None] * W[a] - kappa * W.sum(0)[None, :]) * (ha > 0)
        dhv = g[:, None] * P["value.2.weight"][0][None, :] * (hv > 0)
        grads = {"advantage.2.weight": dW, "advantage.2.bias": dc, "value.2.weight": (g[:, None] * hv).sum(0, keepdim=True),
                 "value.2.bias": G.reshape(1), "advantage.0.weight": dha.T @ f, "advantage.0.bias": dha.sum(0),
                 "value.0.weight": dhv.T @ f, "value.0.bias": dhv.sum(0)}
        df = (dha @ P["advantage.0.weight"] + dhv @ P["value.0.weight"]) * (f > 0)
        grads["feature.0.weight"] = df.T @ x
        grads["feature.0.bias"] = df.sum(0)
        dstate = df @ P["feature.0.weight"]
        E = ew.shape[1]
        demb = torch.zeros_like(ew).index_add_(0, batch["items"].reshape(-1), dstate[:, :F * E].reshape(B * F, E))
        return {"loss": float(((q - y) ** 2).mean()), "mu": float(mu), "mu_t": float(mut), "next_max": next_max, "q": q,
                "grads": grads, "emb": demb}


def clip_l1(grads, max_norm=-1.0):
    """clip_grad_norm_(max_norm, norm_type=1) on a dict of gradients: (clipped dict, norm)."""
    norm = sum(float(v.abs().sum()) for v in grads.values())
    coef = min(max_norm / (norm + 1e-6), 1.0)
    return {k: v * coef for k, v in grads.items()}, norm


class RAdamRef:
    """torch.optim.RAdam (weight_decay 0) restated for one tensor, float64."""

    def __init__(self, lr, betas=(0.9, 0.999), eps=1e-8):
        self.lr, self.b1, self.b2, self.eps = lr, betas[0], betas[1], eps
        self.t, self.m, self.v = 0, None, None

    def step(self, p, g):
        if self.m is None:
            self.m, self.v = torch.zeros_like(p), torch.zeros_like(p)
        self.t += 1
        t, b1, b2 = self.t, self.b1, self.b2
        self.m = self.m + (1 - b1) * (g - self.m)
        self.v = b2 * self.v + (1 - b2) * g * g
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        rho_inf = 2 / (1 - b2) - 1
        rho_t = rho_inf - 2 * t * b2 ** t / bc2
        mh = self.m / bc1
        if rho_t > 5:
            r = math.sqrt((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t))
            return p - self.lr * mh * r * math.sqrt(bc2) / (self.v.sqrt() + self.eps)
        return p - self.lr * mh
