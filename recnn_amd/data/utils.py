"""Batch construction helpers (reference: recnn/data/utils.py).

The collate of the reference (rolling_window + concatenate + emb[items] + cat + done scatter,
utils.py:7-10, :51-81, :161-187) is ONE HIP kernel here (`recnn_frame_gather`), fed by the
device-resident CSR store of `recnn_amd.data.store`.  These functions keep the reference's call
shapes so that user code (custom `embed_batch` callables, direct `get_base_batch` calls) still works.
"""
import numpy as np
import torch

from .. import _lib as L
from .pandas_backend import pd

__all__ = ["rolling_window", "get_irsu", "batch_tensor_embeddings", "batch_contstate_discaction", "batch_no_embeddings", "prepare_batch_static_size", "make_items_tensor",
           "sort_users_itemwise", "get_base_batch", "packed_ld", "FrameBatch", "padder", "prepare_batch_dynamic_size", "ReplayBuffer"]


def rolling_window(a, window):
    """Sliding windows of a 1-D array as a strided view (utils.py:7-10).  Host helper for user code;
    the engine never materialises windows."""
    return np.lib.stride_tricks.sliding_window_view(a, window)


def get_irsu(batch):
    return batch["items"], batch["ratings"], batch["sizes"], batch["users"]


def packed_ld(frame_size: int, emb_dim: int) -> int:
    """Row stride (floats) of the packed batch rows [action | state | 0-pad] the MFMA GEMMs read:
    the 16-byte aligned, zero-padded layout shared with the C engine (engine.hip setup_dims)."""
    state = frame_size * emb_dim + frame_size
    r128 = lambda x: (x + 127) // 128 * 128
    return max(r128(emb_dim + r128(state)), r128(emb_dim + state))


class FrameBatch(dict):
    """The SARS' dict the reference's collate returns (keys state, action, reward, next_state, done, meta),
    whose tensors are views into packed device rows.  `update()` binds those rows directly (no copy)."""
    packed = None   # (xs, xn, reward, done, rows, ld)


def _require_cuda(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise L.RecnnHipError(f"{what}: needs a GPU tensor (recnn_amd has no CPU fallback); got "
                              f"{getattr(t, 'device', type(t))}")


def gather_frames(items, ratings, user_off, batch_users, row_total, rows, frame_size, table, contiguous=False,
                  row_off=None, xs=None, xn=None, reward=None, done=None):
    """plan + gather on the current stream.  Returns a FrameBatch (without `meta`)."""
    dev = table.device
    E = table.shape[1]
    S = frame_size * E + frame_size
    n_users = batch_users.numel()
    stream = L.current_stream()
    if n_users > 1024:      # big user lists: explicit plan launch; otherwise the gather kernel plans inline
        if row_off is None:
            row_off = torch.empty(n_users + 1, dtype=torch.int32, device=dev)
        L.call("recnn_frame_plan", L.ptr(user_off), L.ptr(batch_users), n_users, frame_size, L.ptr(row_off), None, 0, stream)
    else:
        row_off = None
    out = FrameBatch()
    reward = torch.empty(rows, dtype=torch.float32, device=dev) if reward is None else reward
    done = torch.empty(rows, dtype=torch.float32, device=dev) if done is None else done
    if contiguous:
        state = torch.empty(rows, S, dtype=torch.float32, device=dev)
        nstate = torch.empty(rows, S, dtype=torch.float32, device=dev)
        action = torch.empty(rows, E, dtype=torch.float32, device=dev)
        lds, ldn, lda = S, S, E
    else:
        ld = packed_ld(frame_size, E)
        alloc_rows = (rows + 63) // 64 * 64
        if xs is None:
            xs = torch.empty(alloc_rows, ld, dtype=torch.float32, device=dev)
            xn = torch.empty(alloc_rows, ld, dtype=torch.float32, device=dev)
            xs[:, E + S:].zero_()
            xn[:, E + S:].zero_()
            xn[:, :E].zero_()          # next-action slot, written by the target actor during update()
        state, nstate, action = xs[:rows, E:E + S], xn[:rows, E:E + S], xs[:rows, :E]
        lds = ldn = lda = ld
        out.packed = (xs, xn, reward, done, rows, ld)
    if rows > 0:
        L.call("recnn_frame_gather", L.ptr(items), L.ptr(ratings), L.ptr(user_off), L.ptr(batch_users), L.ptr(row_off),
               n_users, rows, frame_size, E, L.ptr(table), L.ptr(state), lds, L.ptr(nstate), ldn, L.ptr(action), lda,
               L.ptr(reward), L.ptr(done), None, 0, stream)
    out.update(state=state, action=action, reward=reward[:rows], next_state=nstate, done=done[:rows])
    return out


def batch_tensor_embeddings(batch, item_embeddings_tensor, frame_size, *args, **kwargs):
    """Embed Batch: continuous state, continuous action (utils.py:51-81) for an already windowed batch
    {"items": int[B, F+1], "ratings": float[B, F+1], "sizes": int[U], "users": ...}.

    Runs the HIP gather with every window treated as a one-row history; `done` follows utils.py:70-71.
    (FrameEnv does not go through here by default: it gathers straight from the CSR store.)
    """
    items_t, ratings_t, sizes_t, users_t = get_irsu(batch)
    table = item_embeddings_tensor
    _require_cuda(table, "batch_tensor_embeddings(item_embeddings_tensor)")
    dev = table.device
    b = ratings_t.shape[0]
    f1 = frame_size + 1
    items = items_t.to(dev).reshape(-1).to(torch.int32).contiguous()
    ratings = ratings_t.to(dev).reshape(-1).float().contiguous()
    off = torch.arange(b + 1, dtype=torch.int64, device=dev) * f1
    users = torch.arange(b, dtype=torch.int32, device=dev)
    out = gather_frames(items, ratings, off, users, b, b, frame_size, table.float().contiguous(), contiguous=True)
    done = torch.zeros(b, device=dev)
    if b:
        idx = torch.cumsum(torch.as_tensor(sizes_t).to(dev) - frame_size, dim=0) - 1
        idx = idx[(idx >= 0) & (idx < b)]        # (a batch cut to rows_per_batch rows ends inside a user: the later users' last windows are not in it)
        done[idx.long()] = 1
    res = dict(out)
    res["done"] = done
    res["meta"] = {"users": users_t, "sizes": sizes_t}
    return res


def batch_contstate_discaction(batch, item_embeddings_tensor, frame_size, num_items, *args, **kwargs):
    """Embed Batch: continuous state, discrete action (utils.py:84-120): as `batch_tensor_embeddings`, but the action is
    the one-hot row of the item id at the end of the window (float[B, num_items]) -- what REINFORCE's critic and the
    behaviour policy consume.  State / next_state / reward come from the HIP gather, the one-hot rows from
    `recnn_onehot_rows`.  Use with a dataset truncated to `num_items` (`truncate_dataset`): ids must be < num_items."""
    res = batch_tensor_embeddings(batch, item_embeddings_tensor, frame_size)
    from ..nn.functional import onehot_rows
    dev = item_embeddings_tensor.device
    last = torch.as_tensor(batch["items"])[:, -1].to(dev)
    res["action"] = onehot_rows(last, int(num_items))
    return res


def batch_no_embeddings(batch, frame_size, *args, **kwargs):
    """Embed Batch: discrete state, discrete action (utils.py:23-48), the index batch the embeddings notebook's DQN learns from:
    items / next_items int[B, F] (the window without its last / first item), ratings / next_ratings float[B, F], action = the item id
    at the end of the window, reward = its rating, done = 1 on each user's last window (cumsum(sizes - F) - 1).  Host-side slicing
    like the reference; `dqn_update` moves the tensors to the GPU and gathers the embeddings there.

    Deliberate difference: the reference keys the ratings with the TENSOR (`ratings: "ratings"`, a typo); here the key is the string
    "ratings"."""
    items_t, ratings_t, sizes_t, users_t = get_irsu(batch)
    items_t, ratings_t, sizes_t = torch.as_tensor(items_t), torch.as_tensor(ratings_t), torch.as_tensor(sizes_t)
    b_size = ratings_t.size(0)
    done = torch.zeros(b_size)
    done[torch.cumsum(sizes_t - frame_size, dim=0) - 1] = 1
    return {
        "items": items_t[:, :-1],
        "next_items": items_t[:, 1:],
        "ratings": ratings_t[:, :-1],
        "next_ratings": ratings_t[:, 1:],
        "action": items_t[:, -1],
        "reward": ratings_t[:, -1],
        "done": done,
        "meta": {"users": users_t, "sizes": sizes_t},
    }


def prepare_batch_static_size(batch, item_embeddings_tensor, frame_size=10, embed_batch=batch_tensor_embeddings):
    """The reference's DataLoader collate_fn (utils.py:161-187): list of per-user dicts
    {"items", "rates", "sizes", "users"} -> SARS' batch."""
    sizes = [int(b["sizes"]) for b in batch]
    users_t = torch.tensor([b["users"] for b in batch])
    sizes_t = torch.tensor(sizes)
    if embed_batch is batch_tensor_embeddings:
        table = item_embeddings_tensor
        _require_cuda(table, "prepare_batch_static_size(item_embeddings_tensor)")
        dev = table.device
        items = torch.from_numpy(np.concatenate([np.asarray(b["items"]) for b in batch]).astype(np.int32)).to(dev)
        ratings = torch.from_numpy(np.concatenate([np.asarray(b["rates"]) for b in batch]).astype(np.float32)).to(dev)
        off = np.zeros(len(batch) + 1, dtype=np.int64)
        off[1:] = np.cumsum(sizes)
        rows = int(sum(max(s - frame_size, 0) for s in sizes))
        out = gather_frames(items, ratings, torch.from_numpy(off).to(dev), torch.arange(len(batch), dtype=torch.int32, device=dev),
                            rows, rows, frame_size, table.float().contiguous(), contiguous=True)
        res = dict(out)
        res["meta"] = {"users": users_t, "sizes": sizes_t}
        return res
    # user-supplied embed function: hand it the windowed index batch, as the reference does
    item_t = np.concatenate([rolling_window(np.asarray(b["items"]), frame_size + 1) for b in batch], 0)
    ratings_t = np.concatenate([rolling_window(np.asarray(b["rates"]), frame_size + 1) for b in batch], 0)
    win = {"items": torch.tensor(item_t), "users": users_t, "ratings": torch.tensor(ratings_t).float(), "sizes": sizes_t}
    return embed_batch(batch=win, item_embeddings_tensor=item_embeddings_tensor, frame_size=frame_size)


def padder(x):
    """Pad a list of `UserDataset` items to one length (utils.py:124-137): {"items": int64[U, Lmax], "ratings": float32[U, Lmax],
    "sizes": float32[U], "users": list}, zero-padded at the end as `pad_sequence(batch_first=True)` does.  Host index work, CPU
    tensors -- as in the reference; the embedding rows are gathered on the GPU by `prepare_batch_dynamic_size`."""
    sizes = [len(b["items"]) for b in x]
    lmax = max(sizes) if sizes else 0
    items = np.zeros((len(x), lmax), dtype=np.int64)
    ratings = np.zeros((len(x), lmax), dtype=np.float32)
    for i, b in enumerate(x):
        items[i, :sizes[i]] = np.asarray(b["items"])
        ratings[i, :sizes[i]] = np.asarray(b["rates"])
    return {"items": torch.from_numpy(items), "ratings": torch.from_numpy(ratings),
            "sizes": torch.tensor([b["sizes"] for b in x]).float(), "users": [b["users"] for b in x]}


def gather_padded_rows(item_idx, table):
    """float32[..., E] = table[item_idx] for an int64 id tensor of any shape, one HIP launch (`recnn_seq_gather_idx`)."""
    _require_cuda(table, "prepare_batch_dynamic_size(item_embeddings_tensor)")
    table = table.float().contiguous()
    idx = torch.as_tensor(item_idx).to(table.device, torch.int64).contiguous()
    out = torch.empty(*idx.shape, table.shape[1], dtype=torch.float32, device=table.device)
    L.call("recnn_seq_gather_idx", L.ptr(idx), idx.numel(), L.ptr(table), table.shape[0], table.shape[1], L.ptr(out), L.current_stream())
    return out


def gather_padded(store, table, slots, l_max=None, embeddings=True):
    """The padded batch of the users in `slots` straight from the CSR replay store, one HIP launch (`recnn_seq_gather`):
    (items int64[U, Lmax], ratings float32[U, Lmax], rows float32[U, Lmax, E] or None).  Lmax defaults to the longest history."""
    _require_cuda(table, "gather_padded(table)")
    slots = store.checked_slots(slots, "gather_padded", table.device)
    u = len(slots)
    if l_max is None:
        l_max = int(store.lengths[slots].max()) if u else 0
    dev = table.device
    items = torch.empty(u, l_max, dtype=torch.int64, device=dev)
    ratings = torch.empty(u, l_max, dtype=torch.float32, device=dev)
    rows = torch.empty(u, l_max, table.shape[1], dtype=torch.float32, device=dev) if embeddings else None
    slots_d = torch.from_numpy(slots).to(dev)
    L.call("recnn_seq_gather", L.ptr(store.items), L.ptr(store.ratings), L.ptr(store.user_off), L.ptr(slots_d), u, l_max,
           L.ptr(table), table.shape[0], table.shape[1], L.ptr(items), L.ptr(ratings), L.ptr(rows), L.current_stream())
    return items, ratings, rows


def prepare_batch_dynamic_size(batch, item_embeddings_tensor, embed_batch=None):
    """The dynamic-length collate (utils.py:149-153): the `padder` dict with "items" replaced by the embedding rows
    table[item_idx], float32[U, Lmax, E] on the table's device.  The reference's quirk is kept: a padded position holds index 0,
    so it receives item 0's row, not zeros.  `embed_batch` is accepted and unused, as in the reference."""
    item_idx, ratings_t, sizes_t, users_t = get_irsu(batch)
    return {"items": gather_padded_rows(item_idx, item_embeddings_tensor), "users": users_t, "ratings": ratings_t, "sizes": sizes_t}


class ReplayBuffer:
    """Fixed-size SARS' storage that SeqEnv fills (utils.py:217-262): `layout` is the four shapes of state, action, reward,
    next_state; `append` writes a batch's rows behind the ones already held and records batch["step"] in meta["step"]; `get`
    returns the FULL buffers (zeros beyond `len()`) with the meta dict; `flush` starts over with fresh zero tensors, so a batch
    handed out by `get` stays valid.

    Extension: `device` -- where the buffers live (default: the device of the first appended batch; "cpu" is allowed, the buffer
    is plain storage).  An append that does not fit raises ValueError (the reference dies inside a slice assignment)."""

    def __init__(self, buffer_size, layout, device=None):
        self.buffer = None
        self.idx = 0
        self.size = buffer_size
        self.layout = layout
        self.device = None if device is None else torch.device(device)
        self.meta = {"step": []}
        self.flush()

    def flush(self):
        self.buffer = None          # fresh zero tensors, made when they are first needed
        self.idx = 0
        self.meta["step"] = []

    def _ensure(self, like=None):
        if self.buffer is None:
            if self.device is None:
                self.device = torch.device("cpu") if like is None else like.device
            self.buffer = [torch.zeros(tuple(i), device=self.device) for i in self.layout]

    @property
    def capacity(self):
        """Rows the buffer can hold: `buffer_size`, or the shortest of the four tensors of `layout` if that is less."""
        return min(self.size, *(int(i[0]) for i in self.layout))

    def room(self, rows):
        """Whether `rows` more rows fit."""
        return self.idx + rows <= self.capacity

    def reserve(self, rows):
        """Views of the next `rows` rows of the four buffers, for a writer that fills them in place (SeqEnv's collect launch)."""
        if not self.room(rows):
            raise ValueError(f"ReplayBuffer: {rows} rows do not fit, {self.idx} of {self.capacity} are taken")
        self._ensure()
        lower, self.idx = self.idx, self.idx + rows
        return [b[lower:self.idx] for b in self.buffer]

    def append(self, batch):
        state = batch["state"]
        self._ensure(state)
        views = self.reserve(state.size(0))
        self.meta["step"].append(batch["step"])
        for v, k in zip(views, ("state", "action", "reward", "next_state")):
            v.copy_(batch[k])

    def get(self):
        self._ensure()
        state, action, reward, next_state = self.buffer
        return {"state": state, "action": action, "reward": reward, "next_state": next_state, "meta": self.meta}

    def len(self):
        return self.idx


def make_items_tensor(items_embeddings_key_dict):
    """{item key: tensor[E]} -> (float[N, E] table in sorted-key order, key_to_id, id_to_key)  (utils.py:203-214)."""
    keys = sorted(items_embeddings_key_dict.keys())
    key_to_id = {k: i for i, k in enumerate(keys)}
    id_to_key = {i: k for i, k in enumerate(keys)}
    table = torch.stack([torch.as_tensor(items_embeddings_key_dict[k]) for k in keys])
    return table, key_to_id, id_to_key


def sort_users_itemwise(user_dict, users):
    """User ids ordered by history length, longest first (utils.py:150-156)."""
    return (pd.get().Series({u: user_dict[u]["items"].shape[0] for u in users}).sort_values(ascending=False).index)


def get_base_batch(batch, device=torch.device("cuda"), done=True):
    """[state, action, reward[B,1], next_state, done[B,1]] on `device` (utils.py:265-276).
    Batches made by FrameEnv already live on the GPU, so `.to(device)` moves nothing."""
    b = [batch["state"], batch["action"], batch["reward"].unsqueeze(1), batch["next_state"]]
    if done:
        b.append(batch["done"].unsqueeze(1))
    return [i.to(device) for i in b]
