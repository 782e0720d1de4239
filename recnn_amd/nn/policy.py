"""The Wolpertinger policy (Dulac-Arnold et al., 2015, "Deep Reinforcement Learning in Large Discrete Action Spaces"): the actor
proposes a proto-action, its nearest items are retrieved, the critic picks among them.  DESIGN.md section 23."""
import torch

from . import functional as F_hip
from ..data.utils import gather_padded_rows
from ..retrieval import MAX_K, CriticIndex, FlatIndex, IVFFlatIndex, TwoStageIndex


class WolpertingerPolicy:
    """`actor` (state -> action of the table's width), `critic` (a three-layer `Critic`), `table` float32 [N, 128] on the GPU.

    Owns a `FlatIndex(table, metric)`, a `CriticIndex(critic, table)` and the `TwoStageIndex` over them.  `index="ivf"` makes the
    first stage an `IVFFlatIndex(table, nlist, metric)` searched with `nprobe` probes (`rank_of` is then refused).  The actor runs in eval
    semantics (no dropout, whatever `actor.training` says) without gradient; the critic's weights are a snapshot: call `refresh()`
    after training steps."""

    def __init__(self, actor, critic, table, n_candidates=MAX_K, metric="L2", index="flat", nlist=None, nprobe=None):
        if index not in ("flat", "ivf"):
            raise ValueError(f"WolpertingerPolicy: index must be \"flat\" or \"ivf\", got {index!r}")
        if index == "flat" and (nlist is not None or nprobe is not None):
            raise ValueError("WolpertingerPolicy: nlist and nprobe apply to index=\"ivf\"")
        if index == "ivf" and nlist is None:
            raise ValueError("WolpertingerPolicy: index=\"ivf\" needs nlist")
        self.actor = actor
        self.nprobe = nprobe
        self.flat = FlatIndex(table, metric) if index == "flat" else IVFFlatIndex(table, nlist, metric)
        self.critic_index = CriticIndex(critic, table)
        self.index = TwoStageIndex(self.flat, self.critic_index, n_candidates)
        self.table = self.critic_index.table

    def refresh(self):
        """Re-reads the critic's weights."""
        self.index.refresh()

    def proto_action(self, state):
        """float32 [B, 128]: the actor's action, eval semantics, no gradient."""
        with torch.no_grad():
            return F_hip.mlp(state, self.actor, False)

    def recommend(self, state, k=10, exclude=None, diversify=None):
        """(q float32 [B, k] descending, ids int64 [B, k]): the k candidates the critic values most among the `n_candidates` items
        nearest to the actor's action.  `exclude` as in `FlatIndex.search`.  `diversify=lam`: `TwoStageIndex.search`'s greedy MMR
        stage over the candidates (cosine similarity); q is then in the order of the choice, not descending."""
        return self.index.search(self.proto_action(state), state, k, exclude, self.nprobe, diversify)

    def act(self, state, exclude=None):
        """(ids int64 [B], actions float32 [B, 128], q float32 [B]): the best candidate, its table row and its value.  A row with
        nothing left gives id -1, a zero action and q = -inf."""
        q, ids = self.recommend(state, 1, exclude)
        ids, q = ids[:, 0], q[:, 0]
        actions = gather_padded_rows(ids.clamp_min(0), self.table)
        actions.masked_fill_((ids < 0)[:, None], 0.0)
        return ids, actions, q

    def rank_of(self, state, targets, exclude=None):
        """int32 [B]: `TwoStageIndex.rank_of` under the actor's action."""
        return self.index.rank_of(self.proto_action(state), state, targets, exclude)


__all__ = ["WolpertingerPolicy"]
