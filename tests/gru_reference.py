"""Host restatements for the GRU state encoder (test infrastructure, not an oracle file), in the style of seq_reference.py,
seq_grad_reference.py and seq_table_grad_reference.py: torch.nn.GRU in float64 / float32 on the CPU over the materialised
[U, T, E + 1] inputs of seq_reference.lstm_inputs, the forward and gradient bounds (the project's rules, from the references alone),
the table-gradient reference, a hand-written BPTT of the equations the reverse-chain kernel is written from, the SeqEnv loop of
seq_reference.seq_env_batches run over a GRU, and the small regression problem of the "training works" test."""
import math

import numpy as np
import torch

import seq_reference
from seq_reference import lstm_inputs, seq_env_data

PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
NAMES = PARAMS + ("h0",)


def cpu_copy(gru, dtype):
    ref = torch.nn.GRU(gru.input_size, gru.hidden_size, batch_first=True)
    ref.load_state_dict({k: v.detach().cpu() for k, v in gru.state_dict().items()})
    return ref.to(dtype)


def gru_cpu(gru, x, h0=None, dtype=torch.float64):
    """(h [U, T, H], h_T [U, H]) of a copy of `gru` in `dtype` on the CPU, users as the batch."""
    ref = cpu_copy(gru, dtype)
    hc = None if h0 is None else h0.detach().cpu().to(dtype).reshape(1, x.shape[0], -1)
    with torch.no_grad():
        out, h = ref(x.to(dtype), hc)
    return out, h[0]


def fp32_bound(gru, x, h0=None):
    """4 x max |GRU_fp32_cpu - GRU_fp64_cpu| on the same inputs, floored at 1e-6, for (h, h_T); and the float64 results."""
    r64 = gru_cpu(gru, x, h0, torch.float64)
    r32 = gru_cpu(gru, x, h0, torch.float32)
    return [max(4.0 * float((a.double() - b).abs().max()), 1e-6) for a, b in zip(r32, r64)], r64


def loss_weights(U, T, H, seed):
    """R1 [U, T, H], R2 [U, H] of the loss L = sum h * R1 + sum h_T * R2 (float32 values)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(U, T, H, generator=g), torch.randn(U, H, generator=g)


def loss_of(h, hT, R, use="all"):
    """use = "all": the whole loss; "final": only h_T (no gradient arrives through h); "head": only h[:, :20]."""
    R1, R2 = (r.to(h.device, h.dtype) for r in R)
    if use == "final":
        return (hT * R2).sum()
    if use == "head":
        return (h[:, :20] * R1[:, :20]).sum()
    return (h * R1).sum() + (hT * R2).sum()


def cpu_grads(gru, x, h0, R, dtype, use="all"):
    """{name: gradient} of loss_of over a CPU copy of `gru` in `dtype`; "h0" only when h0 is given."""
    ref = cpu_copy(gru, dtype)
    hc = None if h0 is None else h0.detach().cpu().to(dtype).reshape(1, x.shape[0], -1).requires_grad_(True)
    out, h = ref(x.to(dtype), hc)
    loss_of(out, h[0], R, use).backward()
    g = {n: getattr(ref, n).grad for n in PARAMS}
    if hc is not None:
        g["h0"] = hc.grad[0]
    return g


def _bounds(g32, g64, U, T):
    floor = 2.0 ** -23 * max(8.0, math.sqrt(U * T))
    return {n: max(4.0 * float((g32[n].double() - g64[n]).abs().max()), floor * float(g64[n].abs().max())) for n in g64}


def grad_bounds(gru, x, h0, R, use="all"):
    """(bounds, float64 gradients): per tensor G, max(4 max |G32cpu - G64cpu|, 2^-23 max(8, sqrt(U T)) max |G64|) -- the rule of
    seq_grad_reference.grad_bounds."""
    U, T = x.shape[:2]
    g64 = cpu_grads(gru, x, h0, R, torch.float64, use)
    g32 = cpu_grads(gru, x, h0, R, torch.float32, use)
    return _bounds(g32, g64, U, T), g64


# ---------------------------------------------------------------------------------------------------- table gradient
def positions(items, ratings, T, t0=0):
    """(idx int64 [U, T], ratings float32 [U, T]) of steps t0 .. t0 + T - 1 of every user."""
    idx = torch.from_numpy(np.stack([np.asarray(i[t0:t0 + T], dtype=np.int64) for i in items]))
    rts = torch.from_numpy(np.stack([np.asarray(r[t0:t0 + T], dtype=np.float32) for r in ratings]))
    return idx, rts


def cpu_table_grads(gru, table, idx, rts, h0, R, dtype, use="all"):
    """{name: gradient} of loss_of over a CPU copy of `gru` in `dtype` over cat([table[idx], rating]) with the TABLE requiring
    grad: "table" [n_items, E], the four weights, "h0" when given."""
    ref = cpu_copy(gru, dtype)
    tb = table.detach().to(dtype).clone().requires_grad_(True)
    x = torch.cat([tb[idx], rts.to(dtype)[..., None]], 2)
    hc = None if h0 is None else h0.detach().cpu().to(dtype).reshape(1, x.shape[0], -1).requires_grad_(True)
    out, h = ref(x, hc)
    loss_of(out, h[0], R, use).backward()
    g = {n: getattr(ref, n).grad for n in PARAMS}
    g["table"] = tb.grad
    if hc is not None:
        g["h0"] = hc.grad[0]
    return g


def table_grad_bounds(gru, table, idx, rts, h0, R, use="all"):
    """(bounds, float64 gradients) under the rule of seq_table_grad_reference.table_grad_bounds."""
    U, T = idx.shape
    g64 = cpu_table_grads(gru, table, idx, rts, h0, R, torch.float64, use)
    g32 = cpu_table_grads(gru, table, idx, rts, h0, R, torch.float32, use)
    return _bounds(g32, g64, U, T), g64


# ---------------------------------------------------------------------------------------------------- BPTT by hand
def bptt_by_hand(w_ih, w_hh, b_ih, b_hh, x, h0, R):
    """The equations of the reverse chain, in float64 numpy: forward with r, z, n, hn kept, then t = T - 1 .. 0
         dh = g_h[:, t] + dh_rec (+ g_hT at the last step)
         da_n = dh (1 - z)(1 - n^2);  da_z = dh (h_{t-1} - n) z (1 - z);  da_r = da_n hn r (1 - r);  da_hn = da_n r
         da_x = [da_r | da_z | da_n];  da_h = [da_r | da_z | da_hn];  dh_rec = dh z + da_h W_hh
         dW_ih += da_x^T x_t;  dW_hh += da_h^T h_{t-1};  db_ih += sum da_x;  db_hh += sum da_h."""
    w_ih, w_hh, b_ih, b_hh, x, h0 = (np.asarray(t.detach().double()) for t in (w_ih, w_hh, b_ih, b_hh, x, h0))
    R1, R2 = (np.asarray(r.double()) for r in R)
    U, T, _ = x.shape
    H = w_hh.shape[1]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    hs, kept = [h0], []
    for t in range(T):
        ax = x[:, t] @ w_ih.T + b_ih
        ah = hs[-1] @ w_hh.T + b_hh
        r, z = sig(ax[:, :H] + ah[:, :H]), sig(ax[:, H:2 * H] + ah[:, H:2 * H])
        hn = ah[:, 2 * H:]
        n = np.tanh(ax[:, 2 * H:] + r * hn)
        hs.append((1 - z) * n + z * hs[-1])
        kept.append((r, z, n, hn))
    d = {"weight_ih_l0": np.zeros_like(w_ih), "weight_hh_l0": np.zeros_like(w_hh), "bias_ih_l0": np.zeros_like(b_ih),
         "bias_hh_l0": np.zeros_like(b_hh)}
    dh_rec = np.zeros((U, H))
    for t in range(T - 1, -1, -1):
        r, z, n, hn = kept[t]
        dh = R1[:, t] + dh_rec + (R2 if t == T - 1 else 0.0)
        da_n = dh * (1 - z) * (1 - n * n)
        da_z = dh * (hs[t] - n) * z * (1 - z)
        da_r = da_n * hn * r * (1 - r)
        da_x = np.concatenate([da_r, da_z, da_n], 1)
        da_h = np.concatenate([da_r, da_z, da_n * r], 1)
        dh_rec = dh * z + da_h @ w_hh
        d["weight_ih_l0"] += da_x.T @ x[:, t]
        d["weight_hh_l0"] += da_h.T @ hs[t]
        d["bias_ih_l0"] += da_x.sum(0)
        d["bias_hh_l0"] += da_h.sum(0)
    d["h0"] = dh_rec
    return {k: torch.from_numpy(v) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------- SeqEnv
def gru_env_data():
    """seq_env_data's users and table with `torch.manual_seed(0); torch.nn.GRU(9, 16)` as the encoder."""
    table, user_dict, users, _ = seq_env_data()
    torch.manual_seed(0)
    return table, user_dict, users, torch.nn.GRU(table.shape[1] + 1, 16)


def gru_env_batches(table, user_dict, users, gru, batch_size, max_buf_size, n_batches, max_epochs=2):
    """seq_reference.seq_env_batches -- that loop, not a copy of it -- with the GRU as the encoder: the loop reaches its encoder only
    through the module-level `fp32_bound`, which is swapped for the GRU's for the duration of the call (the third result, the
    LSTM's c_T, has no GRU counterpart and is not looked at by the loop)."""
    def bound_of(enc, x, h0c0=None):
        b, (h, hT) = fp32_bound(enc, x)
        return b + [b[1]], (h, hT, None)

    keep = seq_reference.fp32_bound
    seq_reference.fp32_bound = bound_of
    try:
        return seq_reference.seq_env_batches(table, user_dict, users, gru, batch_size, max_buf_size, n_batches, max_epochs)
    finally:
        seq_reference.fp32_bound = keep


# ---------------------------------------------------------------------------------------------------- "training works"
TRAIN_USERS = 5
TRAIN_SGD_STEPS = 20


def training_case():
    """The GRU form of seq_grad_reference.training_case: the same users (the first 5 of seq_env_data), kept steps 1 .. 35, the same
    fixed linear read-out of next_state regressed onto reward, plain SGD on the encoder, the same learning-rate list.  The learning
    rate is chosen HERE, on the float64 CPU restatement: the largest of the list for which the float64 loss falls monotonically over
    TRAIN_SGD_STEPS steps and by at least 10 %.
    Returns (table, user_dict, users, gru, steps, (w_read, b_read), lr, float64 losses [TRAIN_SGD_STEPS + 1])."""
    table, user_dict, users, gru = gru_env_data()
    users = users[:TRAIN_USERS]
    steps = list(range(1, 36))
    g = torch.Generator().manual_seed(5)
    w_read, b_read = torch.randn(gru.hidden_size, 1, generator=g) * 0.5, torch.zeros(1)
    items = [user_dict[u]["items"] for u in users]
    ratings = [user_dict[u]["ratings"] for u in users]
    x = lstm_inputs(table, items, ratings, steps[-1] + 1).double()
    reward = x[:, steps, -1]                                          # [U, K]

    def run(lr):
        ref = cpu_copy(gru, torch.float64)
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
            return table, user_dict, users, gru, steps, (w_read, b_read), lr, losses
    raise AssertionError("no learning rate of the list makes the float64 loss fall by 10 %")
