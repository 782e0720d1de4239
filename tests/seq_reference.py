"""Host restatements for the dynamic-length path (test infrastructure, not an oracle file): padder and the dynamic collate in plain
torch, torch.nn.LSTM in float64 on the CPU over materialised [U, T, E + 1] inputs, and the SeqEnv loop over it."""
import numpy as np
import torch


# The shape sweep between the two ends (8, 16) and (128, 256) (tests/test_gpu_seq_shapes.py has what each one reaches; the host-side
# tests check the workspace sizes at the same shapes): (E, H), and (U, T, h0 / c0 set).
SWEEP_SHAPES = ((24, 48), (16, 128), (40, 96), (72, 144), (120, 240))
SWEEP_CASES = ((33, 70, True), (16, 32, False), (17, 65, False))


def padder_ref(x):
    items = torch.nn.utils.rnn.pad_sequence([torch.as_tensor(np.asarray(b["items"])) for b in x], batch_first=True).long()
    ratings = torch.nn.utils.rnn.pad_sequence([torch.as_tensor(np.asarray(b["rates"])) for b in x], batch_first=True).float()
    return {"items": items, "ratings": ratings, "sizes": torch.tensor([b["sizes"] for b in x]).float(), "users": [b["users"] for b in x]}


def dynamic_ref(batch, table):
    return {"items": table[batch["items"]], "users": batch["users"], "ratings": batch["ratings"], "sizes": batch["sizes"]}


def lstm_inputs(table, items, ratings, T, t0=0):
    """float32 [U, T, E + 1]: [embedding(item_t) | rating_t] for steps t0 .. t0 + T - 1 of every user (lists of arrays)."""
    table = torch.as_tensor(table)
    rows = [torch.cat([table[torch.as_tensor(np.asarray(i[t0:t0 + T]), dtype=torch.long)],
                       torch.as_tensor(np.asarray(r[t0:t0 + T]), dtype=torch.float32)[:, None]], 1) for i, r in zip(items, ratings)]
    return torch.stack(rows)


def lstm_cpu(lstm, x, h0c0=None, dtype=torch.float64):
    """(h [U, T, H], h_T [U, H], c_T [U, H]) of a copy of `lstm` in `dtype` on the CPU, users as the batch."""
    ref = torch.nn.LSTM(lstm.input_size, lstm.hidden_size, batch_first=True)
    ref.load_state_dict({k: v.detach().cpu() for k, v in lstm.state_dict().items()})
    ref = ref.to(dtype)
    hc = None if h0c0 is None else tuple(t.detach().cpu().to(dtype).reshape(1, x.shape[0], -1) for t in h0c0)
    with torch.no_grad():
        out, (h, c) = ref(x.to(dtype), hc)
    return out, h[0], c[0]


def fp32_bound(lstm, x, h0c0=None):
    """4 x max |LSTM_fp32_cpu - LSTM_fp64_cpu| on the same inputs, floored at 1e-6, for (h, h_T, c_T); and the float64 results.
    The factor 4 allows for a different summation order and different exp / tanh implementations."""
    r64 = lstm_cpu(lstm, x, h0c0, torch.float64)
    r32 = lstm_cpu(lstm, x, h0c0, torch.float32)
    return [max(4.0 * float((a.double() - b).abs().max()), 1e-6) for a, b in zip(r32, r64)], r64


def seq_env_batches(table, user_dict, users, lstm, batch_size, max_buf_size, n_batches, max_epochs=2):
    """The first `n_batches` buffers the SeqEnv loop hands out (at most `max_epochs` passes over `users`), the encoder in float64.
    Also returns the largest fp32 bound over the user batches that were encoded."""
    table = torch.as_tensor(table)
    E, H = table.shape[1], lstm.hidden_size
    new = lambda: [np.zeros((max_buf_size, H)), np.zeros((max_buf_size, E), np.float32), np.zeros((max_buf_size, 1), np.float32),
                   np.zeros((max_buf_size, H))]
    buf, idx, steps, out, bound = new(), 0, [], [], 1e-6
    meta = {}

    def hand_out():
        nonlocal buf, idx, steps
        out.append({"state": buf[0], "action": buf[1], "reward": buf[2], "next_state": buf[3],
                    "meta": dict(meta, step=list(steps), rows=idx)})
        buf, idx, steps = new(), 0, []

    for _ in range(max_epochs):
        for i in range(0, len(users), batch_size):
            ids = list(users[i:i + batch_size])
            items = [user_dict[u]["items"] for u in ids]
            ratings = [user_dict[u]["ratings"] for u in ids]
            sizes = [len(a) for a in items]
            U, T = len(ids), min(sizes) - 1
            meta = {"users": ids, "sizes": sizes}
            if T > 0:
                x = lstm_inputs(table, items, ratings, T)
                b, (h, _, _) = fp32_bound(lstm, x)
                bound = max(bound, b[0])
                h = h.numpy()
            for t in range(T):
                if np.random.random() > 0.95 and t >= 1:
                    if idx + U > max_buf_size:
                        hand_out()
                    buf[0][idx:idx + U] = h[:, t - 1]
                    buf[1][idx:idx + U] = x[:, t, :E].numpy()
                    buf[2][idx:idx + U, 0] = x[:, t, E].numpy()
                    buf[3][idx:idx + U] = h[:, t]
                    idx += U
                    steps.append(t)
                    if idx >= max_buf_size:
                        hand_out()
                if len(out) >= n_batches:
                    return out[:n_batches], bound
    return out[:n_batches], bound


SEQ_ENV_SEED = 33


def seq_env_data(seed=0, n_users=12, n_items=50, E=8):
    """12 users of lengths 12 .. 40 (sorted longest first, as the env's datasets are), a table, an LSTM(E + 1, 16).  In batches of
    5 users the loop runs 37 + 35 + 11 steps per epoch, of which 5 % are kept: SEQ_ENV_SEED is a numpy seed for which it hands out
    three buffers of 20 rows within two epochs -- seed 0 hands out none, every comparison would be empty -- and for which one of them
    is handed out at 17 rows because the next 5 do not fit."""
    rng = np.random.default_rng(seed)
    lens = [40, 40, 39, 39, 38, 38, 37, 37, 36, 36, 30, 12][:n_users]
    user_dict = {u: {"items": rng.integers(0, n_items, size=L).astype(np.int64),
                     "ratings": (2.0 * (rng.integers(1, 11, size=L) * 0.5 - 2.5)).astype(np.float32)} for u, L in enumerate(lens)}
    table = torch.from_numpy(rng.standard_normal((n_items, E)).astype(np.float32))
    torch.manual_seed(seed)
    lstm = torch.nn.LSTM(E + 1, 16)
    return table, user_dict, list(range(n_users)), lstm
