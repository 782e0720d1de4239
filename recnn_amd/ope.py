"""Off-policy evaluation of the discrete policies (csrc/logprob.hip, csrc/ope.hip): what reward would the
policy pi have collected on data logged under the behaviour policy beta?

Each estimator needs only log pi(a_i | s_i) and log beta(a_i | s_i) at the logged action of every row -- `DiscreteActor.log_prob` /
`Beta.log_prob`, the fused catalogue kernel that never stores the [B, n_items] logits -- and the logged reward r_i.  With the
importance weight w_i = pi / beta (times the top-K factor lambda_K of Chen et al. 2019 when `top_k` >= 1) and n rows:

    ips        = sum w r / n                        (Horvitz-Thompson)
    capped_ips = sum min(w, cap) r / n
    snips      = sum w r / sum w                    (self-normalised: Swaminathan & Joachims 2015)
    dr         = sum (v_dm + w (r - q_logged)) / n  (doubly robust: Dudik et al. 2011; q_logged = q(s, a_logged) and
                                                     v_dm = E_{a ~ pi} q(s, a) of a direct-method model are inputs)
    ess        = (sum w)^2 / sum w^2                (effective sample size)

The sums are float64, accumulated on the GPU over the batches of a loader in a fixed order (`recnn_ope_accumulate`).
"""
import math

import torch

from . import _lib as L

__all__ = ["OffPolicyMeter", "evaluate_policy"]

_SUMS = ("w", "w2", "wr", "wc", "wcr", "r", "dr", "max_w")


def _row(t, n, what, name):
    if not t.is_cuda:
        raise L.RecnnHipError(f"{what}: {name} must be on the GPU (no CPU fallback)")
    t = t.detach()
    if t.dim() == 2 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 1 or (n is not None and t.shape[0] != n):
        raise ValueError(f"{what}: {name} must have shape [{'n' if n is None else n}], got {tuple(t.shape)}")
    return t


class OffPolicyMeter:
    """Accumulates the off-policy estimators over `update(lp_pi, lp_beta, reward)` calls (one per logged batch).

    `cap` bounds the weights of `capped_ips` (inf: none); `top_k` >= 1 multiplies every weight by
    lambda_K = K (1 - pi)^(K - 1), 0 leaves it out (K = 1 gives the plain weights too).  `mask` (optional, [n]) keeps the rows
    where it is non-zero.  A row whose lp_pi or lp_beta is NaN (an action outside the catalogue) counts in `invalid` and in
    nothing else.  `q_logged` / `v_dm` (both or neither, in every update or in none) feed `dr`.  Reading synchronises once; it
    raises ValueError when no row was counted, and `dr` does without its two inputs."""

    def __init__(self, cap=math.inf, top_k=0, device="cuda"):
        cap = float(cap)
        if not cap > 0:
            raise ValueError(f"OffPolicyMeter: cap must be positive (inf for none), got {cap}")
        if int(top_k) != top_k or top_k < 0:
            raise ValueError(f"OffPolicyMeter: top_k must be an integer >= 0, got {top_k}")
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise L.RecnnHipError("OffPolicyMeter: the accumulators live on the GPU (no CPU fallback)")
        self.cap, self.top_k = cap, int(top_k)
        self.sums = torch.zeros(len(_SUMS), dtype=torch.float64, device=device)
        self.counts = torch.zeros(3, dtype=torch.int64, device=device)       # rows, invalid, capped
        self._has_dm = None
        self._cache = None

    def update(self, lp_pi, lp_beta, reward, mask=None, q_logged=None, v_dm=None):
        """Adds one logged batch: lp_pi, lp_beta, reward float [n] on the GPU."""
        what = "OffPolicyMeter.update"
        lp_pi = _row(lp_pi, None, what, "lp_pi")
        n = lp_pi.shape[0]
        rows = [lp_pi, _row(lp_beta, n, what, "lp_beta"), _row(reward, n, what, "reward")]
        if (q_logged is None) != (v_dm is None):
            raise ValueError(f"{what}: q_logged and v_dm come together")
        has_dm = q_logged is not None
        if self._has_dm is not None and has_dm != self._has_dm:
            raise ValueError(f"{what}: earlier updates {'had' if self._has_dm else 'did not have'} q_logged / v_dm, this one "
                             f"{'has' if has_dm else 'does not'}")
        if has_dm:
            rows += [_row(q_logged, n, what, "q_logged"), _row(v_dm, n, what, "v_dm")]
        rows = [t.float().contiguous() for t in rows] + [None] * (5 - len(rows))
        if mask is not None:
            mask = (_row(mask, n, what, "mask") != 0).to(torch.uint8).contiguous()
        if n == 0:
            return
        self._has_dm = has_dm
        self._cache = None
        ws = L.workspace("recnn_ope_accumulate_workspace_bytes", n, device=lp_pi.device)
        L.call("recnn_ope_accumulate", L.ptr(rows[0]), L.ptr(rows[1]), L.ptr(rows[2]), L.ptr(mask), L.ptr(rows[3]), L.ptr(rows[4]), n,
               self.cap, self.top_k, L.ptr(self.sums), L.ptr(self.counts), L.ptr(ws), L.current_stream())

    def reset(self):
        self.sums.zero_()
        self.counts.zero_()
        self._has_dm = None
        self._cache = None

    def _read(self, need_rows=True):
        if self._cache is None:
            c = self.counts.tolist()                      # the one synchronisation; sums follow on the same stream
            self._cache = (c, dict(zip(_SUMS, self.sums.tolist())))
        c, f = self._cache
        if need_rows and c[0] == 0:
            raise ValueError("OffPolicyMeter: no rows counted yet")
        return c, f

    @property
    def rows(self):
        return self._read(need_rows=False)[0][0]

    @property
    def invalid(self):
        return self._read(need_rows=False)[0][1]

    @property
    def capped_share(self):
        c, _ = self._read()
        return c[2] / c[0]

    @property
    def ips(self):
        c, f = self._read()
        return f["wr"] / c[0]

    @property
    def capped_ips(self):
        c, f = self._read()
        return f["wcr"] / c[0]

    @property
    def snips(self):
        _, f = self._read()
        return f["wr"] / f["w"]

    @property
    def ess(self):
        _, f = self._read()
        return f["w"] * f["w"] / f["w2"]

    @property
    def mean_weight(self):
        c, f = self._read()
        return f["w"] / c[0]

    @property
    def max_weight(self):
        return self._read()[1]["max_w"]

    @property
    def logged_mean(self):
        c, f = self._read()
        return f["r"] / c[0]

    @property
    def dr(self):
        c, f = self._read()
        if not self._has_dm:
            raise ValueError("OffPolicyMeter: dr needs q_logged and v_dm in every update")
        return f["dr"] / c[0]


def evaluate_policy(policy, beta, batches, cap=math.inf, top_k=0, meter=None):
    """Runs `policy` (a DiscreteActor) and `beta` (a Beta, or anything with `log_prob(state, actions)`) over logged batches shaped
    like a discrete-action `FrameEnv` batch -- dicts with `state` [B, state_dim], `action` (one-hot rows or int64 ids) and `reward`
    [B] -- and returns the `OffPolicyMeter` (a new one with `cap` / `top_k`, or `meter`).  Nothing is trained or stored."""
    for net in (policy, beta):
        if type(net).__name__ == "VocabParallelDiscreteActor":
            raise TypeError("evaluate_policy: VocabParallelDiscreteActor (the catalogue-sharded actor) is not supported")
        if not callable(getattr(net, "log_prob", None)):
            raise TypeError(f"evaluate_policy: {type(net).__name__} has no log_prob(state, actions)")
    from .nn.functional import action_ids
    for batch in batches:
        state, action, reward = batch["state"], batch["action"], batch["reward"]
        if meter is None:
            meter = OffPolicyMeter(cap=cap, top_k=top_k, device=state.device)
        ids = action_ids(action)
        lp_pi, _ = policy.log_prob(state, ids)
        lp_beta, _ = beta.log_prob(state, ids)
        meter.update(lp_pi, lp_beta, reward.to(state.device))
    if meter is None:
        raise ValueError("evaluate_policy: no batches")
    return meter
