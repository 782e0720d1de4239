"""Host restatements for training the LSTM state encoder (test infrastructure, not an oracle file): torch.nn.LSTM under autograd
in float64 and float32 on the CPU over the materialised [U, T, E + 1] inputs of seq_reference.lstm_inputs, the bound the GPU
gradients are held to, a hand-written BPTT of the equations the kernel is written from, and the small regression problem of the
"training works" test."""
import math

import numpy as np
import torch

from seq_reference import lstm_inputs, seq_env_data

PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
NAMES = PARAMS + ("h0", "c0")


def loss_weights(U, T, H, seed):
    """R1 [U, T, H], R2 [U, H], R3 [U, H] of the loss L = sum h * R1 + sum h_T * R2 + sum c_T * R3 (float32 values)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(U, T, H, generator=g), torch.randn(U, H, generator=g), torch.randn(U, H, generator=g)


def loss_of(h, hT, cT, R, use="all"):
    """use = "all": the whole loss; "final": only h_T and c_T (no gradient arrives through h); "head": only h[:, :20]."""
    R1, R2, R3 = (r.to(h.device, h.dtype) for r in R)
    if use == "final":
        return (hT * R2).sum() + (cT * R3).sum()
    if use == "head":
        return (h[:, :20] * R1[:, :20]).sum()
    return (h * R1).sum() + (hT * R2).sum() + (cT * R3).sum()


def cpu_copy(lstm, dtype):
    ref = torch.nn.LSTM(lstm.input_size, lstm.hidden_size, batch_first=True)
    ref.load_state_dict({k: v.detach().cpu() for k, v in lstm.state_dict().items()})
    return ref.to(dtype)


def cpu_grads(lstm, x, h0c0, R, dtype, use="all"):
    """{name: gradient} of loss_of over a CPU copy of `lstm` in `dtype`; "h0" / "c0" only when h0c0 is given."""
    ref = cpu_copy(lstm, dtype)
    hc = None
    if h0c0 is not None:
        hc = tuple(t.detach().cpu().to(dtype).reshape(1, x.shape[0], -1).requires_grad_(True) for t in h0c0)
    out, (h, c) = ref(x.to(dtype), hc)
    loss_of(out, h[0], c[0], R, use).backward()
    g = {n: getattr(ref, n).grad for n in PARAMS}
    if hc is not None:
        g["h0"], g["c0"] = hc[0].grad[0], hc[1].grad[0]
    return g


def grad_bounds(lstm, x, h0c0, R, use="all"):
    """(bounds, float64 gradients): per tensor G, max(4 max |G32cpu - G64cpu|, 2^-23 max(8, sqrt(U T)) max |G64|).
    The first term is the forward tests' rule (a different summation order, different exp / tanh); the second is the rounding
    error a float32 sum of U T terms is expected to carry, a floor for when the CPU's float32 run happens to land close."""
    U, T = x.shape[:2]
    g64 = cpu_grads(lstm, x, h0c0, R, torch.float64, use)
    g32 = cpu_grads(lstm, x, h0c0, R, torch.float32, use)
    floor = 2.0 ** -23 * max(8.0, math.sqrt(U * T))
    bounds = {n: max(4.0 * float((g32[n].double() - g64[n]).abs().max()), floor * float(g64[n].abs().max())) for n in g64}
    return bounds, g64


def bptt_by_hand(w_ih, w_hh, b_ih, b_hh, x, h0, c0, R):
    """The equations of the reverse chain, in float64 numpy: forward with the gates kept, then t = T - 1 .. 0
         dh = g_h[:, t] + dh_rec (+ g_hT at the last step);  dc = dc_next + dh o (1 - tanh^2 c_t) (+ g_cT at the last step)
         da_o = dh tanh(c_t) o (1 - o);  da_i = dc g i (1 - i);  da_f = dc c_{t-1} f (1 - f);  da_g = dc i (1 - g^2)
         dc_next = dc f;  dh_rec = da W_hh;  dW_hh += da^T h_{t-1};  dW_ih += da^T x_t;  db += sum da."""
    w_ih, w_hh, b_ih, b_hh, x, h0, c0 = (np.asarray(t.detach().double()) for t in (w_ih, w_hh, b_ih, b_hh, x, h0, c0))
    R1, R2, R3 = (np.asarray(r.double()) for r in R)
    U, T, _ = x.shape
    H = w_hh.shape[1]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    hs, cs, gates = [h0], [c0], []
    for t in range(T):
        a = x[:, t] @ w_ih.T + hs[-1] @ w_hh.T + b_ih + b_hh
        i, f, g, o = sig(a[:, :H]), sig(a[:, H:2 * H]), np.tanh(a[:, 2 * H:3 * H]), sig(a[:, 3 * H:])
        c = f * cs[-1] + i * g
        hs.append(o * np.tanh(c))
        cs.append(c)
        gates.append((i, f, g, o))
    d = {"weight_ih_l0": np.zeros_like(w_ih), "weight_hh_l0": np.zeros_like(w_hh), "bias_ih_l0": np.zeros_like(b_ih)}
    dh_rec, dc_next = np.zeros((U, H)), np.zeros((U, H))
    for t in range(T - 1, -1, -1):
        i, f, g, o = gates[t]
        tc = np.tanh(cs[t + 1])
        dh = R1[:, t] + dh_rec + (R2 if t == T - 1 else 0.0)
        dc = dc_next + dh * o * (1 - tc * tc) + (R3 if t == T - 1 else 0.0)
        da = np.concatenate([dc * g * i * (1 - i), dc * cs[t] * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
        dc_next = dc * f
        dh_rec = da @ w_hh
        d["weight_hh_l0"] += da.T @ hs[t]
        d["weight_ih_l0"] += da.T @ x[:, t]
        d["bias_ih_l0"] += da.sum(0)
    d["bias_hh_l0"] = d["bias_ih_l0"].copy()
    d["h0"], d["c0"] = dh_rec, dc_next
    return {k: torch.from_numpy(v) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------- "training works"
TRAIN_USERS = 5
TRAIN_SGD_STEPS = 20


def training_case():
    """E, H = 8, 16; the first 5 users of seq_env_data (37 steps); a fixed linear read-out of next_state regressed onto reward over
    the kept steps 1 .. 35; plain SGD on the encoder.  The learning rate is chosen HERE, on the float64 CPU restatement: the
    largest of a short list for which the float64 loss falls monotonically over TRAIN_SGD_STEPS steps and by at least 10 %.
    Returns (table, user_dict, users, lstm, steps, (w_read, b_read), lr, float64 losses [TRAIN_SGD_STEPS + 1])."""
    table, user_dict, users, lstm = seq_env_data()
    users = users[:TRAIN_USERS]
    steps = list(range(1, 36))
    g = torch.Generator().manual_seed(5)
    w_read, b_read = torch.randn(lstm.hidden_size, 1, generator=g) * 0.5, torch.zeros(1)
    items = [user_dict[u]["items"] for u in users]
    ratings = [user_dict[u]["ratings"] for u in users]
    x = lstm_inputs(table, items, ratings, steps[-1] + 1).double()
    reward = x[:, steps, -1]                                          # [U, K]

    def run(lr):
        ref = cpu_copy(lstm, torch.float64)
        opt = torch.optim.SGD(ref.parameters(), lr=lr)
        losses = []
        for _ in range(TRAIN_SGD_STEPS + 1):
            out, _ = ref(x)
            loss = ((out[:, steps] @ w_read.double() + b_read.double())[..., 0] - reward).pow(2).mean()
            losses.append(float(loss.detach()))
            opt.zero_grad()
            loss.backward()
            opt.step()
        return losses

    for lr in (0.1, 0.03, 0.01, 0.003):
        losses = run(lr)
        if all(b < a for a, b in zip(losses, losses[1:])) and losses[-1] <= 0.9 * losses[0]:
            return table, user_dict, users, lstm, steps, (w_read, b_read), lr, losses
    raise AssertionError("no learning rate of the list makes the float64 loss fall by 10 %")
