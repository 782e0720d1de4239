"""Host restatements for training the item embeddings through the LSTM state encoder (test infrastructure, not an oracle file):
torch.nn.LSTM under autograd in float64 and float32 on the CPU over cat([table[idx], rating]) with the TABLE requiring grad, the
bound the GPU table gradient is held to (the rule of seq_grad_reference.grad_bounds), the hand-written form of the table gradient
from the equations of seq_grad_reference.bptt_by_hand, the preconditions every GPU case asserts first, and the "training works"
problem with the table trained alongside the encoder."""
import math

import numpy as np
import torch

from seq_grad_reference import PARAMS, TRAIN_SGD_STEPS, cpu_copy, loss_of, training_case

EXTRA_ROWS = 12            # table rows appended past the ids a store can hold: no position reaches them


def extended_table(table, seed):
    """`table` [n, E] with EXTRA_ROWS more rows (float32 numpy in, float32 torch out)."""
    extra = np.random.default_rng(1000 + seed).standard_normal((EXTRA_ROWS, table.shape[1])).astype(np.float32)
    return torch.from_numpy(np.concatenate([table, extra], 0))


def positions(items, ratings, T, t0=0):
    """(idx int64 [U, T], ratings float32 [U, T]) of steps t0 .. t0 + T - 1 of every user."""
    idx = torch.from_numpy(np.stack([np.asarray(i[t0:t0 + T], dtype=np.int64) for i in items]))
    rts = torch.from_numpy(np.stack([np.asarray(r[t0:t0 + T], dtype=np.float32) for r in ratings]))
    return idx, rts


def cpu_table_grads(lstm, table, idx, rts, h0c0, R, dtype, use="all"):
    """{name: gradient} of loss_of over a CPU copy of `lstm` in `dtype`: "table" [n_items, E], the four weights, "h0" / "c0" when
    h0c0 is given."""
    ref = cpu_copy(lstm, dtype)
    tb = table.detach().to(dtype).clone().requires_grad_(True)
    x = torch.cat([tb[idx], rts.to(dtype)[..., None]], 2)
    hc = None
    if h0c0 is not None:
        hc = tuple(t.detach().cpu().to(dtype).reshape(1, x.shape[0], -1).requires_grad_(True) for t in h0c0)
    out, (h, c) = ref(x, hc)
    loss_of(out, h[0], c[0], R, use).backward()
    g = {n: getattr(ref, n).grad for n in PARAMS}
    g["table"] = tb.grad
    if hc is not None:
        g["h0"], g["c0"] = hc[0].grad[0], hc[1].grad[0]
    return g


def table_grad_bounds(lstm, table, idx, rts, h0c0, R, use="all"):
    """(bounds, float64 gradients, max |G32 - G64| per tensor): per tensor G the project's rule
    max(4 max |G32cpu - G64cpu|, 2^-23 max(8, sqrt(U T)) max |G64|)."""
    U, T = idx.shape
    g64 = cpu_table_grads(lstm, table, idx, rts, h0c0, R, torch.float64, use)
    g32 = cpu_table_grads(lstm, table, idx, rts, h0c0, R, torch.float32, use)
    floor = 2.0 ** -23 * max(8.0, math.sqrt(U * T))
    d32 = {n: float((g32[n].double() - g64[n]).abs().max()) for n in g64}
    bounds = {n: max(4.0 * d32[n], floor * float(g64[n].abs().max())) for n in g64}
    return bounds, g64, d32


def table_grad_by_hand(w_ih, w_hh, b_ih, b_hh, table, idx, rts, h0, c0, R):
    """The table gradient from the equations of bptt_by_hand, in float64 numpy: forward with the gates kept, the reverse chain's
    da of every step, dX[u, t] = da[u, t] W_ih[:, 0:E], and d_table = index_add over the item ids."""
    w_ih, w_hh, b_ih, b_hh, table, h0, c0 = (np.asarray(t.detach().double()) for t in (w_ih, w_hh, b_ih, b_hh, table, h0, c0))
    R1, R2, R3 = (np.asarray(r.double()) for r in R)
    idx = np.asarray(idx)
    U, T = idx.shape
    H, E = w_hh.shape[1], table.shape[1]
    x = np.concatenate([table[idx], np.asarray(rts.double())[..., None]], 2)
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    hs, cs, gates = [h0], [c0], []
    for t in range(T):
        a = x[:, t] @ w_ih.T + hs[-1] @ w_hh.T + b_ih + b_hh
        i, f, g, o = sig(a[:, :H]), sig(a[:, H:2 * H]), np.tanh(a[:, 2 * H:3 * H]), sig(a[:, 3 * H:])
        c = f * cs[-1] + i * g
        hs.append(o * np.tanh(c))
        cs.append(c)
        gates.append((i, f, g, o))
    d_table = torch.zeros(table.shape, dtype=torch.float64)
    dh_rec, dc_next = np.zeros((U, H)), np.zeros((U, H))
    for t in range(T - 1, -1, -1):
        i, f, g, o = gates[t]
        tc = np.tanh(cs[t + 1])
        dh = R1[:, t] + dh_rec + (R2 if t == T - 1 else 0.0)
        dc = dc_next + dh * o * (1 - tc * tc) + (R3 if t == T - 1 else 0.0)
        da = np.concatenate([dc * g * i * (1 - i), dc * cs[t] * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
        dc_next = dc * f
        dh_rec = da @ w_hh
        d_table.index_add_(0, torch.from_numpy(idx[:, t]), torch.from_numpy(da @ w_ih[:, :E]))
    return d_table


def check_preconditions(tag, g64_table, idx, bound, hot=None):
    """What every GPU case needs from its data to mean something, from the float64 reference alone: rows no position reaches
    (at least EXTRA_ROWS, exactly zero), rows that are real sums (at least 30 with two or more contributions; a `hot` case: one
    row with `hot` contributions), and touched rows that stand far above the bound (max |G| of every touched row >= 100 bounds).
    Returns (touched mask, the figures)."""
    counts = torch.bincount(idx.reshape(-1), minlength=g64_table.shape[0])
    touched = counts > 0
    untouched = int((~touched).sum())
    multi = int((counts >= 2).sum())
    row_max = g64_table.abs().amax(1)
    smallest = float(row_max[touched].min() / bound)
    print(f"{tag} preconditions: untouched rows {untouched}, rows with >= 2 hits {multi}, most hits {int(counts.max())}, "
          f"smallest touched-row max / bound {smallest:.3e}")
    assert untouched >= EXTRA_ROWS and bool((g64_table[~touched] == 0).all())
    if hot is None:
        assert multi >= 30
    else:
        assert int((counts == hot).sum()) == 1 and int(touched.sum()) == 1
    assert smallest >= 100.0
    return touched, dict(untouched=untouched, multi=multi, smallest=smallest)


# ---------------------------------------------------------------------------------------------------- "training works"
def training_case_with_table():
    """seq_grad_reference.training_case with the table trained alongside the encoder (one plain SGD over both).  The learning
    rate is chosen HERE on the float64 CPU restatement by the same rule: the largest of the list for which the float64 loss falls
    monotonically over TRAIN_SGD_STEPS steps and by at least 10 %.
    Returns (table, user_dict, users, lstm, steps, (w_read, b_read), lr, float64 losses [TRAIN_SGD_STEPS + 1])."""
    table, user_dict, users, lstm, steps, (w_read, b_read), _, _ = training_case()
    T = steps[-1] + 1
    idx, rts = positions([user_dict[u]["items"] for u in users], [user_dict[u]["ratings"] for u in users], T)
    reward = rts.double()[:, steps]                                     # [U, K]

    def run(lr):
        ref = cpu_copy(lstm, torch.float64)
        tb = table.double().clone().requires_grad_(True)
        opt = torch.optim.SGD(list(ref.parameters()) + [tb], lr=lr)
        losses = []
        for _ in range(TRAIN_SGD_STEPS + 1):
            out, _ = ref(torch.cat([tb[idx], rts.double()[..., None]], 2))
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
