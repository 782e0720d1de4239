"""dqn_update -- one step of the embeddings notebook's dueling DQN (reference: `examples/0. Embeddings Generation/1. (proof of concept)
DQN.ipynb`, `dqn_update`).  The notebook keeps its networks and optimizers in globals and takes `(step, batch, params, learn)`; here they
travel the way the library's update functions take them: `nets` = {dqn, target_dqn, embeddings}, `optimizer` = {value_optimizer,
embeddings_optimizer}, `params` = {gamma}.

What the step computes, quirks included:
  * state = [embeddings(items).view(B, -1) | ratings], next_state the same from next_items / next_ratings and the SAME table;
  * q = DuelDQN(state)[b, action_b], next_q = max_n target(next_state)[b, n] (no gradient), y = reward + gamma next_q (1 - done),
    loss = mean (q - y)^2; the dueling mean is one scalar over the whole [B, N] matrix;
  * learn: both gradients zeroed, backward, clip_grad_norm_(dqn.parameters(), -1, 1) -- max_norm -1 NEGATES every DQN gradient and
    scales it to L1 norm 1 --, the embeddings optimizer steps, then the DQN optimizer; the embedding gradient is not clipped;
  * learn=False changes nothing and writes the full Q(state) matrix as the 'q_values' histogram.
The target network's soft update stays in the caller's loop (the notebook: soft_update(dqn, target_dqn) when step % 30 != 0).

How: the frame gather builds state and next_state on the GPU (recnn_frame_gather), the trunks run on the GEMM kernels, and the
catalogue-wide parts on csrc/dqn.hip: the online Q at the action is one gathered-row dot, the mean comes from column sums, the target's
max_n is the only catalogue GEMM (row-max epilogue, [B, N] never stored), and the head / embedding gradients are deterministic
scatter-sums.  The loss is the only value read back to the host.
"""

import torch

from ... import _lib as L
from ... import utils
from ...data.utils import gather_frames
from .. import functional as Fh

__all__ = ["dqn_update"]

_KEYS = ("items", "next_items", "ratings", "next_ratings", "action", "reward", "done")


def _unpack(batch):
    if isinstance(batch, dict):
        missing = [k for k in _KEYS if k not in batch]
        if missing:
            raise KeyError(f"dqn_update: batch lacks {missing} (expected the dict of recnn_amd.data.batch_no_embeddings)")
        return [batch[k] for k in _KEYS]
    if len(batch) != 7:
        raise ValueError("dqn_update: batch must be the dict of batch_no_embeddings or the notebook's 7-element list "
                         "[items, next_items, ratings, next_ratings, action, reward, done]")
    return list(batch)


def _check_embedding(emb):
    if not isinstance(emb, torch.nn.Embedding):
        raise TypeError("dqn_update: nets['embeddings'] must be an nn.Embedding")
    if emb.padding_idx is not None:
        raise ValueError("dqn_update: nn.Embedding with padding_idx is not supported")
    if emb.max_norm is not None:
        raise ValueError("dqn_update: nn.Embedding with max_norm is not supported")
    if emb.sparse:
        raise ValueError("dqn_update: nn.Embedding(sparse=True) is not supported (the gradient is dense)")
    if emb.embedding_dim != Fh.DQN_HIDDEN:
        raise ValueError(f"dqn_update: embedding_dim must be {Fh.DQN_HIDDEN}")
    w = emb.weight
    if not w.is_cuda:
        raise L.RecnnHipError("dqn_update: the embeddings and networks must live on the GPU (no CPU fallback)")
    if w.dtype != torch.float32 or not w.is_contiguous():
        raise L.RecnnHipError("dqn_update: the embedding table must be contiguous float32")


def _states(items, next_items, ratings, next_ratings, table):
    """[2B, ld] packed rows: state in rows 0..B-1, next_state in B..2B-1, columns 128 .. 128 + F*129 (zero beyond).  Each row is one
    history of F + 1 entries for recnn_frame_gather (its last entry only feeds outputs that are not used)."""
    B, F = items.shape
    hist_i = torch.cat([torch.cat([items, items[:, -1:]], 1), torch.cat([next_items, next_items[:, -1:]], 1)], 0)
    hist_r = torch.cat([torch.cat([ratings, ratings[:, -1:]], 1), torch.cat([next_ratings, next_ratings[:, -1:]], 1)], 0)
    dev = table.device
    off = torch.arange(2 * B + 1, dtype=torch.int64, device=dev) * (F + 1)
    users = torch.arange(2 * B, dtype=torch.int32, device=dev)
    fb = gather_frames(hist_i.reshape(-1).to(torch.int32).contiguous(), hist_r.reshape(-1).float().contiguous(), off, users, 2 * B, 2 * B,
                       F, table)
    xs, ld = fb.packed[0], fb.packed[5]
    return xs, ld


def dqn_update(batch, params, nets, optimizer, device=torch.device("cuda"), debug=None, writer=utils.DummyWriter(), learn=True,
               step=-1):
    """
    :param batch: dict from recnn_amd.data.batch_no_embeddings, or [items, next_items, ratings, next_ratings, action, reward, done]
    :param params: dict(gamma)
    :param nets: dict(dqn, target_dqn, embeddings)
    :param optimizer: dict(value_optimizer, embeddings_optimizer); any torch optimizers (recnn_amd.optim.RAdam runs fused with the clip)
    :param device: accepted for signature compatibility; the step runs where the networks live (the GPU)
    :param debug: dictionary where debug data is saved (q, next_q rows)
    :param writer: torch.SummaryWriter
    :param learn: whether to learn on this step (False: evaluation, nothing changes)
    :param step: integer step for the loss dictionary / writer
    :return: loss dictionary {"value", "step"}
    """
    dqn, target, emb = nets["dqn"], nets["target_dqn"], nets["embeddings"]
    raw = _unpack(batch)
    _check_embedding(emb)
    l0, la0, la2, lv0, lv2 = Fh.dqn_check_net(dqn)
    _, _, la2t, _, lv2t = Fh.dqn_check_net(target)
    dev = emb.weight.device
    items, next_items, ratings, next_ratings, action, reward, done = [torch.as_tensor(t).to(dev) for t in raw]
    if items.dim() != 2 or next_items.shape != items.shape or ratings.shape != items.shape or next_ratings.shape != items.shape:
        raise ValueError("dqn_update: items / next_items / ratings / next_ratings must all be [B, frame_size]")
    B, F = items.shape
    H = Fh.DQN_HIDDEN
    K = F * H + F
    if l0.in_features != K or target.feature[0].in_features != K:
        raise ValueError(f"dqn_update: DuelDQN input_dim must be (embedding_dim + 1) * frame_size = {K}")
    N = la2.out_features
    if la2t.out_features != N:
        raise ValueError("dqn_update: dqn and target_dqn have different action_dim")
    if B == 0:
        raise ValueError("dqn_update: empty batch")
    action = action.reshape(B).to(torch.int64).contiguous()
    items64 = items.to(torch.int64).contiguous()
    reward = reward.reshape(B).float().contiguous()
    done = done.reshape(B).float().contiguous()
    gamma = float(params["gamma"])
    s = L.current_stream()
    Kp = Fh._r64(K)

    table = emb.weight.detach()
    xs, ld = _states(items, next_items, ratings.float(), next_ratings.float(), table)
    x_on, x_tg = xs[:B, H:], xs[B:2 * B, H:]

    # forward: online trunk, target trunk, value rows, the gathered advantage, column sums, target row max, TD
    f, h2, w0p, w12 = Fh.dqn_trunk(dqn, x_on, K, Kp)
    _, h2t, _, _ = Fh.dqn_trunk(target, x_tg, K, Kp)
    W, c, wv, bv = la2.weight.detach(), la2.bias.detach(), lv2.weight.detach(), lv2.bias.detach()
    Wt, ct = la2t.weight.detach(), la2t.bias.detach()
    V = Fh.dqn_row_dot(h2[:, H:], wv, None, bv)
    adv = Fh.dqn_row_dot(h2, W, action, c)
    Vt = Fh.dqn_row_dot(h2t[:, H:], lv2t.weight.detach(), None, lv2t.bias.detach())
    sh, sw, sc = Fh.dqn_head_stats(h2, B, W, c)
    sht, swt, sct = Fh.dqn_head_stats(h2t, B, Wt, ct)
    rowmax = Fh.dqn_head(h2t, Wt, ct, rowmax=True)
    q = torch.empty(B, device=dev)
    g = torch.empty(B, device=dev)
    stats = torch.zeros(8, device=dev)
    L.call("recnn_dqn_td", L.ptr(V), L.ptr(adv), L.ptr(Vt), L.ptr(rowmax), L.ptr(reward), L.ptr(done), gamma, B, N, L.ptr(sh), L.ptr(sw),
           L.ptr(sc), L.ptr(sht), L.ptr(swt), L.ptr(sct), L.ptr(q), L.ptr(g), L.ptr(stats), s)
    if debug is not None:
        debug["q"] = q
        debug["next_q"] = Fh.ord_to_float(rowmax) + Vt - stats[5]

    if not learn:
        loss = float(stats[0].item())
        writer.add_histogram("q_values", Fh.dqn_head(h2, W, c, V, stats[4:5]), step)
        writer.add_scalar("value/test", loss, step)
        return {"value": loss, "step": step}

    # ---- backward into one flat gradient buffer for the DQN (the clip's L1 norm is one pass over it) and a dense embedding gradient
    dqn_params = list(dqn.parameters())
    n_flat = sum(p.numel() for p in dqn_params)
    flat = torch.empty(n_flat, device=dev)
    order = [l0.weight, l0.bias, la0.weight, lv0.weight, la0.bias, lv0.bias, la2.weight, la2.bias, lv2.weight, lv2.bias]
    if {id(p) for p in order} != {id(p) for p in dqn_params} or len(order) != len(dqn_params):
        raise ValueError("dqn_update: the DQN must have exactly the DuelDQN parameters")
    views, offs, at = {}, {}, 0
    for p in order:
        views[id(p)], offs[id(p)] = flat[at:at + p.numel()].view_as(p), at
        at += p.numel()
    # advantage.0 and value.0 are adjacent in the buffer: the stacked trunk layer's gradients land in place
    gw12 = flat[offs[id(la0.weight)]:offs[id(la0.weight)] + 2 * H * H].view(2 * H, H)
    gb12 = flat[offs[id(la0.bias)]:offs[id(la0.bias)] + 2 * H]

    ws = L.workspace("recnn_dqn_scatter_workspace_bytes", B * F, max(N, emb.num_embeddings), device=dev)
    # head: dW = sum_{a_b = n} g_b ha_b - kappa sum_b ha_b, dc = sum_{a_b = n} g_b - G / N; value head: sum_b g_b hv_b, G
    L.call("recnn_dqn_scatter_sum", L.ptr(h2), h2.stride(0), B, 1, L.ptr(action), 1, L.ptr(g), N, L.ptr(views[id(la2.weight)]),
           L.ptr(views[id(la2.bias)]), L.ptr(sh), L.ptr(stats[2:4]), L.ptr(ws), s)
    zeros = torch.zeros(B, dtype=torch.int64, device=dev)
    L.call("recnn_dqn_scatter_sum", L.ptr(h2[:, H:]), h2.stride(0), B, 1, L.ptr(zeros), 1, L.ptr(g), 1, L.ptr(views[id(lv2.weight)]),
           L.ptr(views[id(lv2.bias)]), None, None, L.ptr(ws), s)
    dh = torch.empty(B, 2 * H, device=dev)
    L.call("recnn_dqn_dh", L.ptr(h2), h2.stride(0), B, L.ptr(W), W.stride(0), N, L.ptr(action), L.ptr(sw), L.ptr(wv), L.ptr(g),
           L.ptr(stats), L.ptr(dh), s)
    dstate = Fh.dqn_trunk_backward(dh, f, x_on, K, Kp, w0p, w12, views[id(l0.weight)], views[id(l0.bias)], gw12, gb12, True)
    # embedding gradient: d emb[i] = sum over (b, f) with items[b, f] = i of dstate[b, f*128 : (f+1)*128], in (b, f) order
    gemb = torch.empty_like(emb.weight)
    L.call("recnn_dqn_scatter_sum", L.ptr(dstate), dstate.stride(0), B, F, L.ptr(items64), F, None, emb.num_embeddings, L.ptr(gemb), None,
           None, None, L.ptr(ws), s)

    for p in dqn_params:
        p.grad = views[id(p)]
    emb.weight.grad = gemb
    # clip_grad_norm_(dqn.parameters(), -1, 1): coefficient -1 / (|g|_1 + 1e-6) from a device scalar
    norm = torch.empty(1, device=dev)
    part = torch.empty(1024, device=dev)
    L.call("recnn_l1_norm_flat", L.ptr(flat), n_flat, L.ptr(part), L.ptr(norm), s)
    value_opt, emb_opt = optimizer["value_optimizer"], optimizer["embeddings_optimizer"]
    from ...optim import RAdam
    fused = type(value_opt) is RAdam and {id(p) for grp in value_opt.param_groups for p in grp["params"]} == {id(p) for p in dqn_params}
    if not fused:
        L.call("recnn_dqn_clip", L.ptr(flat), n_flat, L.ptr(norm), -1.0, s)
    emb_opt.step()
    if fused:
        value_opt.step_clipped(norm, -1.0)
    else:
        value_opt.step()
    loss = float(stats[0].item())
    writer.add_scalar("value/train", loss, step)
    return {"value": loss, "step": step}
