"""next_item_update -- one supervised step on the signal every sequential recommender starts from: which item did the user take
next.  The loss is the full-softmax cross-entropy over the catalogue (GRU4Rec, SASRec; the warm start of the Top-K off-policy
correction), computed by `NextItemHead.loss` on the fused kernels of csrc/logprob.hip / csrc/logprob_bwd.hip: no [rows, n_items]
matrix is stored in either pass.  New functionality: the reference has no supervised update.

`batch["state"]` may carry the state encoder's graph (`SeqEnv.user_batch`): the loss then back-propagates through time into the
encoder, and into the embedding table when the batch was made with `table=P`; with `NextItemHead(P)` the output weights are tied
to that table and `P.grad` receives both gradients.
"""
import torch

from ... import _lib as L
from ... import utils
from ..graphed import _Lazy
from ..models import NextItemHead

__all__ = ["next_item_update"]


def next_item_update(batch, params, nets, optimizer, device=torch.device("cuda"), debug=None, writer=utils.DummyWriter(), learn=True,
                     step=-1):
    """
    :param batch: dict with state [rows, K] (may require grad) and target int64 [rows] (`SeqEnv.target_items(batch)`)
    :param params: dict, optional entries ignore_index (default -100) and dtype ('fp32' / 'bf16'; default: set_catalogue_dtype's);
        sampler (a NegativeSampler) with n_negatives, and / or in_batch=True, switch the loss to the sampled softmax
        (`NextItemHead.sampled_loss`); without them the loss is the full softmax
    :param nets: dict(head: NextItemHead, proj: optional module applied to state before the head)
    :param optimizer: dict(optimizer): one torch optimizer over whatever is trained (head, proj, encoder, table)
    :param device: accepted for signature compatibility; the step runs where the head lives (the GPU)
    :param debug: dictionary that receives the per-row losses under 'row_loss' when given
    :param writer: torch.SummaryWriter
    :param learn: True: zero_grad, backward, step.  False: the loss only, nothing changes
    :param step: integer step for the loss dictionary / writer
    :return: {"loss": lazy device scalar (float(), .item() and format() read it), "step": step}
    """
    if not isinstance(nets, dict) or not isinstance(nets.get("head"), NextItemHead):
        raise TypeError("next_item_update: nets['head'] must be a recnn_amd.nn.NextItemHead")
    for k in ("state", "target"):
        if k not in batch:
            raise KeyError(f"next_item_update: batch lacks {k!r} (state rows and SeqEnv.target_items(batch))")
    if learn and (not isinstance(optimizer, dict) or "optimizer" not in optimizer):
        raise KeyError("next_item_update: optimizer must be dict(optimizer=...)")
    head, proj = nets["head"], nets.get("proj")
    params = params or {}
    state, target = batch["state"], batch["target"]
    if not state.is_cuda:
        raise L.RecnnHipError("next_item_update: the batch must live on the GPU (no CPU fallback)")
    if target.dim() != 1 or target.shape[0] != state.shape[0]:
        raise ValueError(f"next_item_update: {state.shape[0]} state rows but target of shape {tuple(target.shape)}")
    with torch.set_grad_enabled(bool(learn)):
        x = state if proj is None else proj(state)
        if params.get("sampler") is not None or params.get("in_batch"):
            rows = head.sampled_loss(x, target, sampler=params.get("sampler"), n_negatives=params.get("n_negatives"),
                                     in_batch=bool(params.get("in_batch")), reduction="none",
                                     ignore_index=params.get("ignore_index", -100), dtype=params.get("dtype"))
        else:
            rows = head.loss(x, target, reduction="none", ignore_index=params.get("ignore_index", -100), dtype=params.get("dtype"))
        kept = (target.to(rows.device) != params.get("ignore_index", -100)).sum()
        loss = rows.sum() / kept
    if debug is not None:
        debug["row_loss"] = rows.detach()
    if learn:
        opt = optimizer["optimizer"]
        opt.zero_grad()
        loss.backward()
        opt.step()
    losses = {"loss": _Lazy(loss.detach()), "step": step}
    if not isinstance(writer, utils.DummyWriter):
        utils.write_losses(writer, {"loss": float(losses["loss"]), "step": step}, kind="train" if learn else "test")
    return losses
