"""AnomalyDetector (reference: recnn/nn/models.py:7-38), Actor / Critic / DiscreteActor / bcqPerturbator / bcqGenerator
(reference: recnn/nn/models.py:41-73, :187-213, :76-184, :216-242, :245-295) and the Soft Actor-Critic networks of the
reference's `examples/1. Vanilla RL/4. SAC.ipynb` (StateCritic, SoftQ, StochasticActor: code cells 5-7).

Real nn.Modules with the reference's sub-module names (linear1/2/3, drop_layer), state_dict keys and
constructor RNG consumption (nn.Linear default init for linear1, linear2, linear3 in that order, then
linear3.weight/bias ~ U(-init_w, init_w)), so equal seeds give equal initial weights.  Called directly they
run the HIP GEMM kernels through `recnn_amd.nn.functional`; inside `ddpg_update` / `td3_update` their
parameters are adopted by the fused step engine (the parameter tensors become views into its flat arenas).
"""
import math

import torch
import torch.nn as nn

from . import functional as F_hip
from .attention import AttentionEncoder  # noqa: F401
from .transformer import TransformerStateEncoder  # noqa: F401

__all__ = ["DuelDQN", "AnomalyDetector", "Actor", "Critic", "DiscreteActor", "Beta", "bcqPerturbator", "bcqGenerator", "StateCritic", "SoftQ", "StochasticActor", "NextItemHead", "NegativeSampler", "AttentionEncoder", "TransformerStateEncoder"]


class DuelDQN(nn.Module):
    """The dueling DQN of the embeddings notebook (examples/0. Embeddings Generation/1. (proof of concept) DQN.ipynb): feature =
    Linear(input_dim, 128) ReLU, advantage = Linear(128, 128) ReLU Linear(128, action_dim), value = Linear(128, 128) ReLU Linear(128, 1),
    forward(x) = value + advantage - advantage.mean(), the mean ONE scalar over the whole [B, action_dim] matrix.  Same sub-modules,
    state_dict keys and default initialisation as the notebook's class; `forward` runs on the HIP kernels (csrc/dqn.hip and the GEMM
    kernels) and is differentiable.  Input: float32 [B, input_dim] on the GPU."""

    def __init__(self, input_dim, action_dim):
        super().__init__()
        self.feature = nn.Sequential(nn.Linear(input_dim, 128), nn.ReLU())
        self.advantage = nn.Sequential(nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, action_dim))
        self.value = nn.Sequential(nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 1))

    def forward(self, x):
        return F_hip.duel_dqn_forward(x, self)


class AnomalyDetector(nn.Module):
    """The reference's debugging autoencoder (models.py:7-38): 128 -> 64 -> 32 -> 64 -> 128, each hidden Linear followed by ReLU
    then BatchNorm1d, the output by ReLU.  `self.ae` is the same plain nn.Sequential (state_dict keys `ae.0.weight` ... `ae.9.bias`,
    constructor RNG consumption, `load_state_dict(torch.load('anomaly.pt'))`); `forward` and `rec_error` run on the HIP kernels
    (`functional.anomaly_forward` / `anomaly_rec_error`, csrc/anomaly.hip), in train mode with batch statistics and running-statistic
    updates as BatchNorm1d has them.  Input: float32 [rows, 128] on the GPU."""

    def __init__(self):
        super().__init__()
        self.ae = nn.Sequential(
            nn.Linear(128, 64), nn.ReLU(), nn.BatchNorm1d(64),
            nn.Linear(64, 32), nn.ReLU(), nn.BatchNorm1d(32),
            nn.Linear(32, 64), nn.ReLU(), nn.BatchNorm1d(64),
            nn.Linear(64, 128), nn.ReLU(),
        )

    def forward(self, x):
        return F_hip.anomaly_forward(x, self.ae, self.training)

    def rec_error(self, x):
        error = F_hip.anomaly_rec_error(x, self.ae, self.training)
        if x.size(1) != 1:
            return error.detach()
        return error.item()


class Actor(nn.Module):
    """state -> action: relu(L1) -> dropout(0.5) -> relu(L2) -> dropout(0.5) -> L3 [-> tanh]."""

    def __init__(self, input_dim, action_dim, hidden_size, init_w=2e-1):
        super().__init__()
        self.drop_layer = nn.Dropout(p=0.5)
        self.linear1 = nn.Linear(input_dim, hidden_size)
        self.linear2 = nn.Linear(hidden_size, hidden_size)
        self.linear3 = nn.Linear(hidden_size, action_dim)
        self.linear3.weight.data.uniform_(-init_w, init_w)
        self.linear3.bias.data.uniform_(-init_w, init_w)

    def forward(self, state, tanh=False):
        action = F_hip.mlp(state, self, self.training)
        return torch.tanh(action) if tanh else action


class Critic(nn.Module):
    """(state, action) -> value: the same MLP over cat([state, action], 1) with a single output."""

    def __init__(self, input_dim, action_dim, hidden_size, init_w=3e-5):
        super().__init__()
        self.drop_layer = nn.Dropout(p=0.5)
        self.linear1 = nn.Linear(input_dim + action_dim, hidden_size)
        self.linear2 = nn.Linear(hidden_size, hidden_size)
        self.linear3 = nn.Linear(hidden_size, 1)
        self.linear3.weight.data.uniform_(-init_w, init_w)
        self.linear3.bias.data.uniform_(-init_w, init_w)

    def forward(self, state, action):
        idx = F_hip.onehot_index_of(action)
        if idx is not None and state.is_cuda:
            # one-hot action rows (REINFORCE's discrete-action batches, data.batch_contstate_discaction): gather the B
            # weight columns instead of contracting over the whole catalogue
            return F_hip.mlp_onehot(state, idx, state.shape[1], self, self.training)
        return F_hip.mlp(torch.cat([state, action], 1), self, self.training)

    def candidates(self, state, actions, n):
        """self(repeat_interleave(state, n, 0), actions) for n consecutive candidate actions per state row, without
        dropout or gradient (`functional.mlp_candidates`: the state part of layer 1 once per state)."""
        return F_hip.mlp_candidates(state, actions, n, self.linear1.weight, self.linear1.bias, self.linear2.weight,
                                    self.linear2.bias, self.linear3.weight, self.linear3.bias)


class Beta(nn.Module):
    """The learned behaviour policy of the Top-K off-policy correction -- the `Beta` class the reference DEFINES IN ITS NOTEBOOK
    (`examples/2. REINFORCE TopK Off Policy Correction/3. TopK Reinforce Off Policy Correction.ipynb`, cell 3) and hands to
    `DiscreteActor._select_action_with_TopK_correction` as `beta_net.forward` (recnn/nn/models.py:113-141,143-184):

        self.net = Sequential(Linear(1290, num_items), Softmax());  optim = RAdam(lr=1e-5, weight_decay=1e-5);  CrossEntropyLoss
        forward(state, action):  p = net(state);  loss = criterion(p, action.argmax(1));  zero_grad / backward / optim.step();
                                 return p.detach()

    i.e. it TRAINS on every call (one optimizer step on the cross entropy of its own probabilities taken as logits -- the
    notebook's quirk, kept) and returns the probabilities it had BEFORE that step.  Same sub-module names (`net.0.weight`,
    `net.0.bias` in the state dict), same attributes `optim` / `criterion`.  Forward, loss, backward and optimizer run on the
    HIP kernels (`functional.beta_train_forward`, `recnn_amd.optim`).  Optimizer: the notebook's `torch_optimizer.RAdam` is an
    absent, un-pinned package; the default here follows `recnn_amd.nn.algo.set_default_optimizer` (this package's fused Ranger
    or Adam, lr = 1e-5, weight_decay = 1e-5), `optimizer=lambda params: ...` injects any other (the parity fixture injects
    torch.optim.Adam).  `last_loss` keeps the loss of the latest call as a device scalar."""

    def __init__(self, input_dim=1290, num_items=5000, lr=1e-5, weight_decay=1e-5, optimizer=None):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(input_dim, num_items), nn.Softmax(dim=1))
        self.criterion = nn.CrossEntropyLoss()
        self._opt_args = (lr, weight_decay, optimizer)
        self.optim = None
        self.last_loss = None

    def _optimizer(self):
        if self.optim is None:
            from .. import optim as O
            from . import algo
            lr, wd, make = self._opt_args
            if make is not None:
                self.optim = make(self.net.parameters())
            else:
                cls = O.Ranger if algo._DEFAULT_OPTIMIZER == "ranger" else O.Adam
                self.optim = cls(self.net.parameters(), lr=lr, weight_decay=wd)
        return self.optim

    def forward(self, state, action=None):
        lin = self.net[0]
        if action is None:                      # plain evaluation (no label, nothing to learn from)
            with torch.no_grad():
                tgt = torch.zeros(state.shape[0], dtype=torch.int64, device=state.device)
                p, _, _, _ = F_hip.beta_train_forward(state, tgt, lin.weight, lin.bias)
            return p
        idx = F_hip.onehot_index_of(action)
        tgt = idx if idx is not None else action.argmax(1)
        p, loss, gw, gb = F_hip.beta_train_forward(state, tgt, lin.weight, lin.bias)
        opt = self._optimizer()
        lin.weight.grad, lin.bias.grad = gw, gb          # (zero_grad + backward of the notebook)
        opt.step()
        self.last_loss = loss
        return p

    def log_prob(self, state, actions):
        """(log beta(a | s), logsumexp of the logits), float32 [B] each, for logged actions (int64 ids, `onehot_rows` rows or dense
        one-hot rows) -- `functional.catalogue_log_prob`: no [B, num_items] matrix, no clamp, and unlike `forward` nothing is
        trained: no optimizer is made or stepped."""
        lin = self.net[0]
        return F_hip.catalogue_log_prob(state, lin.weight, lin.bias, F_hip.action_ids(actions))


class DiscreteActor(nn.Module):
    """state -> probabilities over the catalogue: softmax(L2(relu(L1(state))))  (models.py:76-184), the REINFORCE policy.

    Same attributes as the reference: `saved_log_probs`, `rewards`, `correction`, `lambda_k` (the episode the update
    functions append to and `ChooseREINFORCE` consumes), `action_source` ({"pi": "pi", "beta": "beta"}; set pi to "beta"
    to score the behaviour policy's action, issue #7 of the reference) and the re-bindable `select_action`.
    Forward, sampling and log-prob are one autograd node on the HIP kernels (`functional.DiscretePolicyFunction`); the
    sampler is an inverse-CDF walk with a counter-based uniform per row (torch's multinomial stream is not reproduced --
    equal in distribution, tests/test_gpu_reinforce.py).  `forced_actions` (a list of int64 tensors, consumed first-in
    first-out) replaces the next draws of the policy: replaying logged actions, and the parity tests.
    """

    def __init__(self, input_dim, action_dim, hidden_size, init_w=0):
        super().__init__()
        self.linear1 = nn.Linear(input_dim, hidden_size)
        self.linear2 = nn.Linear(hidden_size, action_dim)
        self.saved_log_probs = []
        self.rewards = []
        self.correction = []
        self.lambda_k = []
        self.action_source = {"pi": "pi", "beta": "beta"}
        self.select_action = self._select_action
        self.forced_actions = []

    def forward(self, inputs):
        probs, _, _ = F_hip.discrete_policy(inputs, self)
        return probs

    def gc(self):
        del self.rewards[:]
        del self.saved_log_probs[:]
        del self.correction[:]
        del self.lambda_k[:]

    def _act(self, state, actions=None):
        """(probs, action, log_prob); draws the action unless one is given or queued in `forced_actions`."""
        if actions is None and self.forced_actions:
            actions = self.forced_actions.pop(0)
        return F_hip.discrete_policy(state, self, actions=actions, sample=actions is None)

    def log_prob(self, state, actions):
        """(log pi(a | s), logsumexp of the logits), float32 [B] each, for logged actions (int64 ids, `onehot_rows` rows or dense
        one-hot rows), for offline evaluation (`recnn_amd.ope`): `functional.catalogue_log_prob` over the hidden layer -- no
        [B, action_dim] matrix, no clamp, no gradient, and the episode lists and `forced_actions` are left alone."""
        return F_hip.discrete_log_prob(state, self, actions)

    def _select_action(self, state, **kwargs):
        # plain REINFORCE: there is no behaviour policy, `action_source` is not consulted (models.py:103-111)
        pi_probs, _, log_prob = self._act(state)
        self.saved_log_probs.append(log_prob)
        return pi_probs

    def pi_beta_sample(self, state, beta, action, **kwargs):
        """log-probs of the target (pi) and behaviour (beta) policies for one action each (models.py:113-141).
        `beta(state, action=...)` returns the behaviour policy's probabilities.  The HIP sampler (`F_hip.categorical`) is
        not differentiable: for a beta that detaches its output (the reference notebook's `Beta` does) nothing is lost; a
        beta that returns probabilities still on the autograd graph gets its log-prob recomputed with torch ops below so
        that the gradient through `corr = exp(pi_lp) / exp(beta_lp)` reaches it, as in the reference."""
        beta_probs = beta(state.detach(), action=action)
        beta_action, beta_log_prob_own = F_hip.categorical(beta_probs)
        if beta_probs.requires_grad:
            def _lp(act):   # Categorical(probs).log_prob(act): probs normalised, clamped to [eps, 1 - eps], log, gather
                pr = beta_probs / beta_probs.sum(-1, keepdim=True)
                eps = torch.finfo(pr.dtype).eps
                return torch.log(pr.clamp(eps, 1 - eps)).gather(-1, act.reshape(-1, 1).to(torch.int64)).reshape(act.shape)
            beta_log_prob_own = _lp(beta_action)
        if self.action_source["pi"] == "beta":
            pi_probs, pi_action, pi_log_prob = self._act(state, actions=beta_action)
        else:
            pi_probs, pi_action, pi_log_prob = self._act(state)
        if self.action_source["beta"] == "beta":
            beta_log_prob = beta_log_prob_own
        elif beta_probs.requires_grad:
            beta_log_prob = _lp(pi_action)
        else:
            _, beta_log_prob = F_hip.categorical(beta_probs, actions=pi_action)
        return pi_log_prob, beta_log_prob, pi_probs

    def _select_action_with_correction(self, state, beta, action, writer, step, **kwargs):
        pi_log_prob, beta_log_prob, pi_probs = self.pi_beta_sample(state, beta, action)
        corr = torch.exp(pi_log_prob) / torch.exp(beta_log_prob)      # off-policy importance weight
        writer.add_histogram("correction", corr, step)
        writer.add_histogram("pi_log_prob", pi_log_prob, step)
        writer.add_histogram("beta_log_prob", beta_log_prob, step)
        self.correction.append(corr)
        self.saved_log_probs.append(pi_log_prob)
        return pi_probs

    def _select_action_with_TopK_correction(self, state, beta, action, K, writer, step, **kwargs):
        pi_log_prob, beta_log_prob, pi_probs = self.pi_beta_sample(state, beta, action)
        corr = torch.exp(pi_log_prob) / torch.exp(beta_log_prob)
        l_k = K * (1 - torch.exp(pi_log_prob)) ** (K - 1)             # lambda_K = K (1 - pi)^(K-1)  (models.py:173)
        writer.add_histogram("correction", corr, step)
        writer.add_histogram("l_k", l_k, step)
        writer.add_histogram("pi_log_prob", pi_log_prob, step)
        writer.add_histogram("beta_log_prob", beta_log_prob, step)
        self.correction.append(corr)
        self.lambda_k.append(l_k)
        self.saved_log_probs.append(pi_log_prob)
        return pi_probs


class bcqPerturbator(nn.Module):
    """(state, action) -> action + MLP([state | action]): BCQ's perturbation network (models.py:216-242).  Same sub-module
    names, state_dict keys and constructor RNG consumption as the reference; forward / backward on the HIP GEMM kernels."""

    def __init__(self, num_inputs, num_actions, hidden_size, init_w=3e-1):
        super().__init__()
        self.drop_layer = nn.Dropout(p=0.5)
        self.linear1 = nn.Linear(num_inputs + num_actions, hidden_size)
        self.linear2 = nn.Linear(hidden_size, hidden_size)
        self.linear3 = nn.Linear(hidden_size, num_actions)
        self.linear3.weight.data.uniform_(-init_w, init_w)
        self.linear3.bias.data.uniform_(-init_w, init_w)

    def forward(self, state, action):
        return F_hip.mlp(torch.cat([state, action], 1), self, self.training) + action

    def candidates(self, state, actions, n):
        """self(repeat_interleave(state, n, 0), actions) without dropout or gradient (see Critic.candidates)."""
        return F_hip.mlp_candidates(state, actions, n, self.linear1.weight, self.linear1.bias, self.linear2.weight,
                                    self.linear2.bias, self.linear3.weight, self.linear3.bias) + actions


class bcqGenerator(nn.Module):
    """BCQ's conditional VAE (models.py:245-295): encoder e1, e2 -> (mean, log_std), z = mean + std * eps, decoder d1, d2, d3
    over [state | z].  `forward` returns (reconstructed action, mean, std); `decode(state)` draws z ~ clamp(N(0, 1), +-0.5).

    The encoder and the decoder each run as one 3-layer stack on the HIP GEMM kernels (the `mean` and `log_std` heads share
    one [2 latent, 750] GEMM); clamp / exp / reparametrisation are one kernel (csrc/vae.hip).  The reference draws its
    normals on the CPU from the global generator and copies them over; here they are drawn on the device
    (`torch.randn(device=...)`) -- equal in distribution.  `forced_noise` (a list of tensors, consumed first-in first-out)
    replaces the next draws: replaying logged noise, and the parity tests."""

    def __init__(self, state_dim, action_dim, latent_dim):
        super().__init__()
        self.e1 = nn.Linear(state_dim + action_dim, 750)
        self.e2 = nn.Linear(750, 750)
        self.mean = nn.Linear(750, latent_dim)
        self.log_std = nn.Linear(750, latent_dim)
        self.d1 = nn.Linear(state_dim + latent_dim, 750)
        self.d2 = nn.Linear(750, 750)
        self.d3 = nn.Linear(750, action_dim)
        self.latent_dim = latent_dim
        self.normal = torch.distributions.Normal(0, 1)
        self.forced_noise = []

    def _noise(self, rows, device):
        if self.forced_noise:
            z = self.forced_noise.pop(0)
            if tuple(z.shape) != (rows, self.latent_dim):
                raise ValueError(f"forced_noise entry has shape {tuple(z.shape)}, the call needs {(rows, self.latent_dim)}")
            return z.to(device=device, dtype=torch.float32)
        return torch.randn(rows, self.latent_dim, device=device)

    def forward(self, state, action):
        ml = F_hip.mlp3(torch.cat([state, action], 1), self.e1, self.e2,
                        torch.cat([self.mean.weight, self.log_std.weight], 0), torch.cat([self.mean.bias, self.log_std.bias], 0))
        z, std = F_hip.vae_latent(ml, self._noise(state.shape[0], state.device))
        return self.decode(state, z), ml[:, :self.latent_dim], std

    def decode(self, state, z=None):
        if z is None:
            z = self._noise(state.shape[0], state.device).clamp(-0.5, 0.5)
        return F_hip.mlp3(torch.cat([state, z], 1), self.d1, self.d2, self.d3.weight, self.d3.bias)

    def decode_candidates(self, state, n):
        """decode(repeat_interleave(state, n, 0)): n sampled actions per state row, [B n, action_dim], no gradient."""
        z = self._noise(state.shape[0] * n, state.device).clamp(-0.5, 0.5)
        return F_hip.mlp_candidates(state, z, n, self.d1.weight, self.d1.bias, self.d2.weight, self.d2.bias,
                                    self.d3.weight, self.d3.bias)


# ---- Soft Actor-Critic (examples/1. Vanilla RL/4. SAC.ipynb, code cells 5-7) ------------------------
class StateCritic(nn.Module):
    """state -> V(state): relu(L1) -> relu(L2) -> L3, no dropout (SAC.ipynb cell 5)."""

    def __init__(self, state_dim, hidden_dim, init_w=3e-3):
        super().__init__()
        self.linear1 = nn.Linear(state_dim, hidden_dim)
        self.linear2 = nn.Linear(hidden_dim, hidden_dim)
        self.linear3 = nn.Linear(hidden_dim, 1)
        self.linear3.weight.data.uniform_(-init_w, init_w)
        self.linear3.bias.data.uniform_(-init_w, init_w)

    def forward(self, state):
        return F_hip.mlp(state, self, False)


class SoftQ(nn.Module):
    """(state, action) -> Q: the same stack over cat([state, action], 1), no dropout (SAC.ipynb cell 6)."""

    def __init__(self, input_dim, action_dim, hidden_dim, init_w=3e-3):
        super().__init__()
        self.linear1 = nn.Linear(input_dim + action_dim, hidden_dim)
        self.linear2 = nn.Linear(hidden_dim, hidden_dim)
        self.linear3 = nn.Linear(hidden_dim, 1)
        self.linear3.weight.data.uniform_(-init_w, init_w)
        self.linear3.bias.data.uniform_(-init_w, init_w)

    def forward(self, state, action):
        return F_hip.mlp(torch.cat([state, action], 1), self, False)


class StochasticActor(nn.Module):
    """state -> (mean, log_std) of a tanh-squashed Gaussian policy (SAC.ipynb cell 7): relu(L1) -> dropout -> relu(L2) ->
    dropout -> {mean_linear, clamp(log_std_linear)}.  The trunk and BOTH heads run as one three-layer HIP MLP (the heads'
    weights concatenated to a [2 * action_dim, hidden] last layer; autograd splits the gradient back).

    Kept from the notebook: `evaluate` draws ONE standard-normal scalar `z` per call (`Normal(0, 1).sample()` has no batch
    shape) shared by every row and action dimension, evaluates `Normal(mean, std).log_prob` at the SQUASHED action, and does
    not sum the log-prob over the action dimension ([B, action_dim]).  `forced_z` (a list, consumed first-in first-out)
    replaces the next draws: replays and parity tests."""

    def __init__(self, input_dim, action_dim, hidden_size, params):
        super().__init__()
        self.log_std_min = params["log_std_min"]
        self.log_std_max = params["log_std_max"]
        self.drop_layer = nn.Dropout(p=0.5)
        self.linear1 = nn.Linear(input_dim, hidden_size)
        self.linear2 = nn.Linear(hidden_size, hidden_size)
        self.mean_linear = nn.Linear(hidden_size, action_dim)
        self.mean_linear.weight.data.uniform_(-params["mean_initw"], params["mean_initw"])
        self.mean_linear.bias.data.uniform_(-params["mean_initw"], params["mean_initw"])
        self.log_std_linear = nn.Linear(hidden_size, action_dim)
        self.log_std_linear.weight.data.uniform_(-params["std_initw"], params["std_initw"])
        self.log_std_linear.bias.data.uniform_(-params["std_initw"], params["std_initw"])
        self.forced_z = []

    def forward(self, state):
        w3 = torch.cat([self.mean_linear.weight, self.log_std_linear.weight], 0)
        b3 = torch.cat([self.mean_linear.bias, self.log_std_linear.bias], 0)
        out = F_hip.MLPFunction.apply(state.float(), self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias,
                                      w3, b3, self.training, torch.initial_seed(), F_hip._take_forced_masks(self, self.training), None)
        a = self.mean_linear.out_features
        return out[:, :a], torch.clamp(out[:, a:], self.log_std_min, self.log_std_max)

    def evaluate(self, state, epsilon=1e-6):
        mean, log_std = self.forward(state)
        std = log_std.exp()
        # (drawn on the device: no host value enters the step, so it can be captured -- recnn_amd.nn.GraphedUpdate)
        z = self.forced_z.pop(0) if self.forced_z else torch.randn((), device=mean.device)
        z = torch.as_tensor(z, dtype=torch.float32).to(mean.device)
        action = torch.tanh(mean + z * std)
        # torch.distributions.Normal(mean, std).log_prob(action), its formula written out (the class validates its arguments with
        # a host sync, which a captured step cannot have)
        log_prob = -((action - mean) ** 2) / (2 * std ** 2) - std.log() - math.log(math.sqrt(2 * math.pi))
        log_prob = log_prob - torch.log(1 - action.pow(2) + epsilon)
        return action, log_prob, z, mean, log_std


class NextItemHead:
    """Full-softmax next-item head over the catalogue: logits = x weight^T + bias, trained with the fused cross-entropy
    (`functional.catalogue_cross_entropy`, csrc/logprob_bwd.hip) -- the [rows, n_items] logits are never stored,
    forward or backward.

    `weight` is a contiguous float32 GPU tensor or Parameter [n_items, K] and is used as it is, never copied: it may be the very
    tensor passed as `SeqEnv.user_batch(table=)`, which ties the output weights to the input embeddings.  `bias` float32
    [n_items] or None.  The padded K may not exceed 256 (`functional.catalogue_log_prob_train`); the 2048- and 1290-wide heads of
    `DiscreteActor` and `Beta` keep their own training paths."""

    def __init__(self, weight, bias=None):
        if not isinstance(weight, torch.Tensor) or weight.dim() != 2 or weight.dtype != torch.float32 or not weight.is_contiguous():
            raise ValueError("NextItemHead: weight must be a contiguous float32 tensor [n_items, K]")
        if not weight.is_cuda:
            raise F_hip.L.RecnnHipError("NextItemHead: the weight must live on the GPU (no CPU fallback)")
        if bias is not None and not (isinstance(bias, torch.Tensor) and bias.dtype == torch.float32 and bias.is_cuda
                                     and tuple(bias.shape) == (weight.shape[0],)):
            raise ValueError(f"NextItemHead: bias must be a float32 GPU tensor [{weight.shape[0]}] or None")
        self.weight, self.bias = weight, bias

    @classmethod
    def new(cls, n_items, dim, bias=True, device="cuda"):
        """A head of its own: weight ~ N(0, 1 / dim), zero bias, both Parameters."""
        w = nn.Parameter(torch.randn(int(n_items), int(dim), device=device) / math.sqrt(dim))
        return cls(w, nn.Parameter(torch.zeros(int(n_items), device=device)) if bias else None)

    n_items = property(lambda self: self.weight.shape[0])

    def parameters(self):
        """The tensors of the head that require grad (for an optimizer)."""
        return [t for t in (self.weight, self.bias) if t is not None and t.requires_grad]

    def loss(self, x, targets, reduction="mean", ignore_index=-100, dtype=None):
        """`catalogue_cross_entropy` of x [rows, K] against the item ids `targets`."""
        return F_hip.catalogue_cross_entropy(x, self.weight, self.bias, targets, reduction=reduction, ignore_index=ignore_index,
                                             dtype=dtype)

    def sampled_loss(self, x, targets, *, sampler=None, n_negatives=None, negatives=None, in_batch=False, reduction="mean",
                     ignore_index=-100, dtype=None, sparse_grad=False):
        """`sampled_cross_entropy` of x [rows, K] against `targets` (csrc/sampled.hip).  The negatives, shared by every
        row, are either `negatives` (int64 [S], no corrections), or `n_negatives` draws from `sampler` (a `NegativeSampler`) with its
        log-Q corrections for negatives and targets.  `in_batch=True`: the batch's own targets are the negatives (ignored rows
        leave as -1), joined with the sampler's draws if a sampler is given; corrections come from the sampler when there is one.
        Accidental hits are removed."""
        if negatives is not None and (sampler is not None or in_batch):
            raise ValueError("NextItemHead.sampled_loss: pass explicit negatives, or a sampler with n_negatives and / or in_batch")
        if (sampler is None) != (n_negatives is None):
            raise ValueError("NextItemHead.sampled_loss: sampler and n_negatives go together")
        if negatives is None and sampler is None and not in_batch:
            raise ValueError("NextItemHead.sampled_loss: needs negatives, a sampler with n_negatives, or in_batch=True")
        t = F_hip.action_ids(targets).to(x.device)
        tq = nq = None
        if negatives is None:
            parts, qs = [], []
            if in_batch:
                own = torch.where(t == int(ignore_index), torch.full_like(t, -1), t)
                parts.append(own)
                if sampler is not None:
                    qs.append(sampler.log_q(own))
            if sampler is not None:
                ids, lq = sampler.sample(int(n_negatives))
                parts.append(ids.to(x.device))
                qs.append(lq.to(x.device))
                tq = sampler.log_q(t).to(x.device)
                nq = torch.cat(qs)
            negatives = torch.cat(parts)
        return F_hip.sampled_cross_entropy(x, self.weight, self.bias, t, negatives, target_log_q=tq, negative_log_q=nq,
                                           reduction=reduction, ignore_index=ignore_index, dtype=dtype, sparse_grad=sparse_grad)

    def log_prob(self, x, targets):
        """(log_prob, lse) of `catalogue_log_prob`: detached, for the off-policy meters."""
        return F_hip.catalogue_log_prob(x, self.weight, self.bias, F_hip.action_ids(targets))

    def index(self):
        """`FlatIndex(weight, "IP")` for `rank_of` / `RankingMeter`: a snapshot of the weight as it is now.  Refused when the head
        has a bias: the order of the logits is then not the inner-product order."""
        if self.bias is not None:
            raise ValueError("NextItemHead.index: the head has a bias, so its logits do not rank the items as the inner product "
                             "does; evaluate a bias-free head, or rank by the logits yourself")
        from ..retrieval import FlatIndex
        return FlatIndex(self.weight, "IP")


class NegativeSampler:
    """Draws item ids with replacement from a fixed distribution q over the catalogue and reports log q, the correction of the
    sampled softmax (`NextItemHead.sampled_loss`, `functional.sampled_log_prob_train`).  q is uniform when `counts` is None, else
    q proportional to (counts + smoothing)^power (word2vec's 0.75 by default).  Torch plumbing, not a kernel: a float64 inverse CDF,
    `torch.searchsorted`, and a `torch.Generator` on `device` seeded with `seed` -- equal seeds give equal draws.  An item with
    q = 0 could never be corrected for and is refused at construction."""

    def __init__(self, n_items, counts=None, power=0.75, smoothing=1.0, seed=0, device="cuda"):
        n_items = int(n_items)
        if n_items < 1:
            raise ValueError(f"NegativeSampler: n_items = {n_items}")
        self.device = torch.device(device)
        if counts is None:
            w = torch.ones(n_items, dtype=torch.float64, device=self.device)
        else:
            counts = torch.as_tensor(counts).to(device=self.device, dtype=torch.float64)
            if tuple(counts.shape) != (n_items,) or bool((counts < 0).any()):
                raise ValueError(f"NegativeSampler: counts must be {n_items} non-negative numbers, got shape {tuple(counts.shape)}")
            w = (counts + float(smoothing)) ** float(power)
        if not bool(torch.isfinite(w).all()) or bool((w <= 0).any()):
            raise ValueError("NegativeSampler: an item has q = 0 (a zero count with smoothing = 0): its log q is -inf and no "
                             "correction exists; use smoothing > 0")
        q = w / w.sum()
        self.n_items = n_items
        self._log_q = torch.log(q).to(torch.float32)
        cdf = torch.cumsum(q, 0)
        cdf[-1] = 1.0
        self._cdf = cdf
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(seed))

    @classmethod
    def from_store(cls, store, n_items, **kw):
        """counts = how often each item occurs in `store.items` (a `recnn_amd.data.store.ReplayStore`-like object)."""
        items = torch.as_tensor(store.items).reshape(-1).to(torch.int64)
        items = items[(items >= 0) & (items < int(n_items))]
        return cls(n_items, counts=torch.bincount(items, minlength=int(n_items)), **kw)

    def sample(self, n):
        """(ids int64 [n], log_q float32 [n]): n independent draws."""
        u = torch.rand(int(n), dtype=torch.float64, device=self.device, generator=self._gen)
        ids = torch.searchsorted(self._cdf, u, right=True).clamp_(max=self.n_items - 1)
        return ids, self._log_q[ids]

    def log_q(self, ids):
        """log q of any ids, float32; 0 for an id outside [0, n_items) (padding, ignored targets: such entries take no part)."""
        ids = torch.as_tensor(ids).to(device=self.device, dtype=torch.int64)
        ok = (ids >= 0) & (ids < self.n_items)
        return torch.where(ok, self._log_q[ids.clamp(0, self.n_items - 1)], torch.zeros((), device=self.device))
