"""The DDPG step's input gradient without a GPU: the restatement the GPU tests compare against (tests/state_grad_reference.py) against
autograd, and the new export's presence and argument checks."""
import ctypes as C

import torch

import state_grad_reference as SG
from oracle import recnn_oracle as O


def test_restatement_equals_autograd_through_the_modules():
    """gV / gP from the equations against autograd through the layers of recnn.nn.Critic / Actor in float64 (1e-12), with keep-masks.
    The modules' own forward is the GPU's (fp32, HIP); their nn.Linear layers are what autograd runs through here, with the masks
    applied as Dropout(0.5) applies them."""
    import recnn
    S, A, H, B = 27, 8, 16, 5
    torch.manual_seed(5)
    actor = recnn.nn.Actor(S, A, H, 6e-1).double()
    critic_v = recnn.nn.Critic(S, A, H, 54e-2).double()
    critic_p = recnn.nn.Critic(S, A, H, 54e-2).double()          # "after the value step": just another critic
    g = torch.Generator().manual_seed(6)
    state = torch.randn(B, S, generator=g, dtype=torch.float64)
    action = torch.randn(B, A, generator=g, dtype=torch.float64)
    expected = torch.randn(B, 1, generator=g, dtype=torch.float64)
    masks = [(torch.rand(B, H, generator=g) < 0.5).to(torch.uint8) for _ in range(6)]

    def run(mod, x, m1, m2):
        h1 = torch.relu(mod.linear1(x)) * (m1.double() * 2.0)
        h2 = torch.relu(mod.linear2(h1)) * (m2.double() * 2.0)
        return mod.linear3(h2)

    s = state.clone().requires_grad_(True)
    value_loss = (run(critic_v, torch.cat([s, action], 1), masks[0], masks[1]) - expected).pow(2).mean()
    (gV_auto,) = torch.autograd.grad(value_loss, s)
    s = state.clone().requires_grad_(True)
    policy_loss = -run(critic_p, torch.cat([s, run(actor, s, masks[2], masks[3])], 1), masks[4], masks[5]).mean()
    (gP_auto,) = torch.autograd.grad(policy_loss, s)

    as_p = lambda m: {k: v.double() for k, v in zip(O.PARAM_ORDER, (p.detach() for p in m.parameters()))}
    gV, gP, _ = SG.input_grads(as_p(actor), as_p(critic_v), as_p(critic_p), state, action, expected, masks)
    assert gV.abs().max() > 0 and gP.abs().max() > 0
    ev, ep = float((gV - gV_auto).abs().max()), float((gP - gP_auto).abs().max())
    print(f"restatement vs autograd: gV {ev:.3e} gP {ep:.3e}")
    assert ev <= 1e-12 and ep <= 1e-12


def test_export_and_null_engine():
    """recnn_engine_state_grads is exported, bound with its signature, and refuses a null engine with an error code and a message."""
    from recnn_amd import _lib as L
    assert "recnn_engine_state_grads" in L.SIGNATURES
    lib = L.load()
    assert lib.recnn_abi_version() == 2
    out = (C.c_float * 4)()
    rc = lib.recnn_engine_state_grads(None, 1, 0, C.cast(out, C.c_void_p), 4, None)
    assert rc == -1 and b"state_grads" in lib.recnn_last_error()
