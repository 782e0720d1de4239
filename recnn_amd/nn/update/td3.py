"""td3_update (reference: recnn/nn/update/td3.py:8-150) on the fused HIP step engine.

Quirks kept: target action = target_policy(next_state) + clamp(N(0, noise_std), +-noise_clip); twin target
critics, min, NO clamp of the TD target; both critics updated every step (MSELoss); policy loss through
value_net1 every step; on `step % policy_update == 0` the actor update (with the L1 clip quirk) and soft updates
of BOTH target critics -- the target policy net is never soft-updated (td3.py:136-141).
"""
import torch

from ... import _lib as L
from ... import utils
from .. import fused

__all__ = ["td3_update"]


def _check_value_optimizers(nets, optimizer):
    """The attached route sends both value losses' d/d state through the encoder in ONE backward, which equals the reference's two only
    when nothing reachable from `state` is zeroed or stepped between them: each value optimizer must hold exactly its critic."""
    for key, net in (("value_optimizer1", "value_net1"), ("value_optimizer2", "value_net2")):
        held = [p for g in optimizer[key].param_groups for p in g["params"]]
        own = fused._module_params(nets[net])
        if len(held) != len(own) or any(all(p is not q for q in own) for p in held):
            raise L.RecnnHipError(
                f"td3_update: batch['state'] requires grad, and optimizer['{key}'] holds parameters other than its critic's (or not all "
                "of them).  Both value losses' gradients go through the state encoder in one backward pass, so no value optimizer may "
                "zero or step anything behind `state` -- put the encoder's parameters into policy_optimizer or into an optimizer of "
                "their own, or pass state.detach()")


def _update_attached(ctx, state, rows, params, optimizer, cfgs, policy_step, s):
    """The split phases with the input gradients handed to autograd (see td3_update's docstring)."""
    eng = ctx.engine
    popt, vopt1, vopt2 = optimizer["policy_optimizer"], optimizer["value_optimizer1"], optimizer["value_optimizer2"]
    if cfgs:        # optimizers the engine can run: their state IS the engine's arenas, on this route stepped by their own step()
        ctx.mirror_optimizer_state(popt, L.NET_POLICY)
        ctx.mirror_optimizer_state(vopt1, L.NET_VALUE1)
        ctx.mirror_optimizer_state(vopt2, L.NET_VALUE2)

    def send(which):
        g = eng.state_grads(rows, which)
        torch.autograd.backward([state], [g if g.dtype == state.dtype else g.to(state.dtype)], retain_graph=True)

    vopt1.zero_grad()
    vopt2.zero_grad()
    L.call("recnn_engine_value_grads", eng.handle, rows, 1, s)
    send(3)                     # both value losses', each through its critic as it is before any step: one launch, one backward
    ctx.attach_grads(L.NET_VALUE1)
    ctx.attach_grads(L.NET_VALUE2)
    vopt1.step()
    vopt2.step()
    ctx.refresh_stepped(L.NET_VALUE1)
    ctx.refresh_stepped(L.NET_VALUE2)
    if policy_step:
        popt.zero_grad()        # (before the launch that fills the actor's arena: zero_grad(set_to_none=False) writes into it)
    L.call("recnn_engine_policy_grads", eng.handle, rows, int(policy_step), s)
    if policy_step:
        send(1)
        L.call("recnn_engine_clip_policy_grads", eng.handle, 1.0, s)
        ctx.attach_grads(L.NET_POLICY)
        popt.step()
        ctx.refresh_stepped(L.NET_POLICY)
        tau = float(params["soft_tau"])
        L.call("recnn_engine_soft_update", eng.handle, L.NET_VALUE1, L.NET_TARGET_VALUE1, tau, s)
        L.call("recnn_engine_soft_update", eng.handle, L.NET_VALUE2, L.NET_TARGET_VALUE2, tau, s)
    # the engine's device counters follow the optimizers it mirrors (bias corrections of later fused steps)
    L.call("recnn_engine_finish", eng.handle, rows, int(bool(cfgs)), int(bool(cfgs) and policy_step), s)
    if cfgs:
        ctx.bump(vopt1, L.NET_VALUE1)
        ctx.bump(vopt2, L.NET_VALUE2)
        if policy_step:
            ctx.bump(popt, L.NET_POLICY)
    ctx.mark_stepped((L.NET_VALUE1, L.NET_VALUE2) + ((L.NET_POLICY, L.NET_TARGET_VALUE1, L.NET_TARGET_VALUE2) if policy_step else ()))
    ctx._sync_versions()


def td3_update(batch, params, nets, optimizer, device=torch.device("cpu"), debug=None, writer=utils.DummyWriter(),
               learn=False, step=-1):
    """
    :param params: dict(gamma, noise_std, noise_clip, soft_tau, policy_update)
    :param nets: dict(value_net1, target_value_net1, value_net2, target_value_net2, policy_net, target_policy_net)
    :param optimizer: dict(policy_optimizer, value_optimizer1, value_optimizer2)
    :return: {"value1": float, "value2": float, "policy": float, "step": step}

    A state with a graph behind it (an LSTM state encoder: `SeqEnv.user_batch`).  When `learn` is true, autograd is enabled and
    `batch["state"].requires_grad`, the update also sends the losses' gradients back into `state` (td3.py:95-141, misc.py:25-44):
    both value optimizers' `zero_grad()`, the two value losses' d/d state -- each through its critic as it is before any step,
    summed inside one HIP launch (`recnn_engine_state_grads`, which = 3) -- through ONE `torch.autograd.backward`, both critics'
    steps; on a policy step `policy_optimizer.zero_grad()`, the policy loss's d/d state -- through the UPDATED critic 1 and through the
    actor, the raw gradient: the clip quirk touches the actor's parameters only -- the clipped actor gradient, the actor's step, the soft
    updates of the two target critics (the target policy net is never soft-updated).  One backward for both value losses is a
    deliberate deviation from the reference's two: the encoder's backward is linear in the gradient it is handed, and it is the
    expensive part.  It gives the reference's result only when no value optimizer zeroes or steps anything behind `state`, so each
    value optimizer must hold exactly its critic's parameters (checked by identity; otherwise `RecnnHipError` names the optimizer):
    put the encoder into `policy_optimizer` or into an optimizer of its own.  All three optimizers are stepped by their own `step()`
    between the engine's phases, whatever their kind, so every parameter they hold (the encoder's) is stepped with them; the optimizer
    state the engine mirrors stays the same memory on either route.  `batch["next_state"]` is only read (the reference uses it under
    no_grad).  The value losses' gradient costs one backward pass through the encoder (one BPTT) on EVERY step; a caller whose encoder
    sits only in the policy optimizer can pass `state.detach()` on the steps that are no policy steps and gets the same parameters:
    the reference zeroes that gradient (`policy_optimizer.zero_grad()`) before anything uses it.  Every other call -- learn=False,
    torch.no_grad(), a detached state -- runs exactly as before.  The split-bf16 compute type (bf16x3) has no such launch: an attached
    state raises there instead of dropping its gradient.
    """
    if debug is None:
        debug = dict()
    attached = bool(learn) and torch.is_grad_enabled() and bool(getattr(batch["state"], "requires_grad", False))
    ctx = fused.context_for("td3", nets)
    if attached and ctx.dtype == "bf16x3":
        raise L.RecnnHipError("td3_update: batch['state'] requires grad, but this context computes in bf16x3 (split bf16), which has "
                              "no input-gradient launch -- use dtype 'fp32' or 'bf16', or pass state.detach()")
    if attached:
        _check_value_optimizers(nets, optimizer)
    ctx.ensure(nets, batch["state"].shape[0])
    rows = ctx.load_batch(batch)
    eng = ctx.engine
    keys = ("policy_optimizer", "value_optimizer1", "value_optimizer2")
    cfgs = fused.fused_adam_configs(optimizer, keys) if learn else None
    if cfgs and cfgs[1] != cfgs[2]:
        cfgs = None                          # the engine shares one Adam configuration between the twin critics
    ctx.set_hyper(params, cfgs[0] if cfgs else None, cfgs[1] if cfgs else None)
    ctx.apply_external(rows)
    policy_step = bool(learn) and (step % params["policy_update"] == 0)
    s = L.current_stream()
    if attached:
        _update_attached(ctx, batch["state"], rows, params, optimizer, cfgs, policy_step, s)
    elif not learn or cfgs:
        if learn:
            ctx.mirror_optimizer_state(optimizer["policy_optimizer"], L.NET_POLICY)
            ctx.mirror_optimizer_state(optimizer["value_optimizer1"], L.NET_VALUE1)
            ctx.mirror_optimizer_state(optimizer["value_optimizer2"], L.NET_VALUE2)
        L.call("recnn_engine_step", eng.handle, rows, int(bool(learn)), int(step), s)
        if learn:
            ctx.bump(optimizer["value_optimizer1"], L.NET_VALUE1)
            ctx.bump(optimizer["value_optimizer2"], L.NET_VALUE2)
            if policy_step:
                ctx.bump(optimizer["policy_optimizer"], L.NET_POLICY)
            ctx.mark_stepped((L.NET_VALUE1, L.NET_VALUE2)
                             + ((L.NET_POLICY, L.NET_TARGET_VALUE1, L.NET_TARGET_VALUE2) if policy_step else ()))
    else:
        L.call("recnn_engine_value_grads", eng.handle, rows, 1, s)
        ctx.attach_grads(L.NET_VALUE1)
        ctx.attach_grads(L.NET_VALUE2)
        optimizer["value_optimizer1"].step()
        optimizer["value_optimizer2"].step()
        eng.refresh(L.NET_VALUE1)
        eng.refresh(L.NET_VALUE2)
        L.call("recnn_engine_policy_grads", eng.handle, rows, int(policy_step), s)
        if policy_step:
            L.call("recnn_engine_clip_policy_grads", eng.handle, 1.0, s)
            ctx.attach_grads(L.NET_POLICY)
            optimizer["policy_optimizer"].step()
            eng.refresh(L.NET_POLICY)
            tau = float(params["soft_tau"])
            L.call("recnn_engine_soft_update", eng.handle, L.NET_VALUE1, L.NET_TARGET_VALUE1, tau, s)
            L.call("recnn_engine_soft_update", eng.handle, L.NET_VALUE2, L.NET_TARGET_VALUE2, tau, s)
        L.call("recnn_engine_finish", eng.handle, rows, 0, 0, s)
        ctx._sync_versions()
    if not learn:
        debug["next_action"] = eng.buffer("next_action", rows)
        debug["gen_action"] = eng.buffer("gen_action", rows)
        if not isinstance(writer, utils.DummyWriter):
            writer.add_figure("next_action", utils.pairwise_distances_fig(debug["next_action"][:50]), step)
            writer.add_histogram("value1", eng.buffer("q1", rows), step)
            writer.add_histogram("value2", eng.buffer("q2", rows), step)
            writer.add_histogram("target_value", eng.buffer("target_q", rows), step)
            writer.add_histogram("expected_value", eng.buffer("expected", rows), step)
            writer.add_figure("gen_action", utils.pairwise_distances_fig(debug["gen_action"][:50]), step)
            writer.add_histogram("policy_loss", -eng.buffer("q_pi", rows), step)
    lo = eng.losses()
    losses = {"value1": lo["value1"], "value2": lo["value2"], "policy": lo["policy"], "step": step}
    utils.write_losses(writer, losses, kind="train" if learn else "test")
    return losses
