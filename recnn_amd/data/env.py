"""FrameEnv: static-length user environment producing SARS' batches (reference: recnn/data/env.py:23-256).

Same constructor, attributes and batch dict as the reference; the data path underneath is MI355X-first:
the user histories live in HBM as a CSR replay store, a batch is described by a list of user slots, and one
HIP kernel builds state / next_state / action / reward / done directly in the packed rows the MFMA GEMMs read.
No DataLoader worker processes, no pickling of batches, no host-to-device copy of 22 MB per step.
"""
import os
import pickle

import numpy as np
import torch

from . import dataset_functions as dset_F
from . import utils
from .pandas_backend import pd
from .store import ReplayStore

__all__ = ["UserDataset", "EnvBase", "DataPath", "Env", "FrameEnv", "FrameLoader", "SeqEnv", "SeqLoader"]


class UserDataset:
    """user index -> {'items', 'rates', 'sizes', 'users'} (env.py:23-64).  Pickle-compatible field names."""

    def __init__(self, users, user_dict):
        self.users = users
        self.user_dict = user_dict

    def __len__(self):
        return len(self.users)

    def __getitem__(self, idx):
        uid = self.users[idx]
        group = self.user_dict[uid]
        items = group["items"][:]
        return {"items": items, "rates": group["ratings"][:], "sizes": items.shape[0], "users": uid}


class EnvBase:
    """What gets pickled as the env cache (env.py:67-78)."""

    def __init__(self):
        self.train_user_dataset = None
        self.test_user_dataset = None
        self.embeddings = None
        self.key_to_id = None
        self.id_to_key = None


class DataPath:
    """Paths of ratings csv / embeddings pickle / optional cache (env.py:81-98)."""

    def __init__(self, base: str, ratings: str, embeddings: str, cache: str = "", use_cache: bool = True):
        self.ratings = base + ratings
        self.embeddings = base + embeddings
        self.cache = base + cache
        self.use_cache = use_cache


class Env:
    """Builds or loads the EnvBase (env.py:101-187)."""

    def __init__(self, path: DataPath, prepare_dataset=dset_F.prepare_dataset, embed_batch=utils.batch_tensor_embeddings,
                 **kwargs):
        self.base = EnvBase()
        self.embed_batch = embed_batch
        self.prepare_dataset = prepare_dataset
        if path is None:
            return
        if path.use_cache and os.path.isfile(path.cache):
            self.load_env(path.cache)
        else:
            self.process_env(path)
            if path.use_cache:
                self.save_env(path.cache)

    def process_env(self, path: DataPath, **kwargs):
        # NB (reference quirk, env.py:137-150): called without kwargs, so the user filter always uses
        # frame_size=10 / test_size=0.05 whatever the constructor was given.
        frame_size = kwargs.get("frame_size", 10)
        test_size = kwargs.get("test_size", 0.05)
        with open(path.embeddings, "rb") as f:
            key_dict = pickle.load(f)
        self.base.embeddings, self.base.key_to_id, self.base.id_to_key = utils.make_items_tensor(key_dict)
        ratings = pd.get().read_csv(path.ratings)
        args_mut = dset_F.DataFuncArgsMut(df=ratings, base=self.base, users=None, user_dict=None)
        self.prepare_dataset(args_mut, dset_F.DataFuncKwargs(frame_size=frame_size))
        self.base = args_mut.base
        self.df = args_mut.df
        self._split(args_mut.users, args_mut.user_dict, test_size)

    def _split(self, users, user_dict, test_size):
        from sklearn.model_selection import train_test_split
        train_users, test_users = train_test_split(users, test_size=test_size)
        train_users = utils.sort_users_itemwise(user_dict, train_users)[2:]   # env.py:178 drops the 2 longest
        test_users = utils.sort_users_itemwise(user_dict, test_users)
        self.base.train_user_dataset = UserDataset(train_users, user_dict)
        self.base.test_user_dataset = UserDataset(test_users, user_dict)

    def load_env(self, where: str):
        with open(where, "rb") as f:
            self.base = pickle.load(f)

    def save_env(self, where: str):
        with open(where, "wb") as f:
            pickle.dump(self.base, f)


class FrameLoader:
    """What `env.train_dataloader` is: a re-iterable, len()-able, shuffled stream of batches of
    `batch_size` USERS (reference: torch DataLoader(shuffle=True, collate_fn=...), env.py:225-239).
    A new random user order is drawn per iteration from torch's global CPU generator, as RandomSampler does."""

    def __init__(self, env, dataset: UserDataset, batch_size: int, shuffle: bool = True):
        self.env = env
        self.dataset = dataset
        self.batch_size = batch_size
        self.shuffle = shuffle

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        planner = getattr(self, "planner", None)
        if planner is not None:
            # an Algo drives this loader (Algo.attach_env(..., drive_loader=True)): one epoch of handles of the fixed-size
            # batches its engine draws -- `algo.update(batch)` queues them, `batch["state"]` materialises one on demand
            yield from planner.batches(planner.batches_left_in_epoch())
            return
        n = len(self.dataset)
        order = torch.randperm(n).numpy() if self.shuffle else np.arange(n)
        users = self.dataset.users
        for i in range(0, n, self.batch_size):
            yield self.env.collate_users([users[j] for j in order[i:i + self.batch_size]])


class StoreEnv(Env):
    """An Env whose user histories live on the GPU as one CSR replay store (`recnn_amd.data.store`), next to the embedding
    table: what FrameEnv and SeqEnv build their batches from.  Subclasses set `device` and implement `_make_loaders`."""
    _store = None
    _table = None
    _csr = None

    def _fill_from_user_dict(self, embeddings, user_dict, train_users, test_users):
        self.base.embeddings = embeddings
        n = embeddings.shape[0]
        self.base.key_to_id = {i: i for i in range(n)}
        self.base.id_to_key = {i: i for i in range(n)}
        self.base.train_user_dataset = UserDataset(list(train_users), user_dict)
        self.base.test_user_dataset = UserDataset(list(test_users), user_dict)
        self._make_loaders()

    def _fill_from_csr(self, embeddings, items, ratings, user_off, test_fraction):
        self.base.embeddings = embeddings
        n_users = len(user_off) - 1
        n_test = int(n_users * test_fraction)
        ids = list(range(n_users))
        self._csr = (np.asarray(items), np.asarray(ratings), np.asarray(user_off, dtype=np.int64))
        self.base.train_user_dataset = UserDataset(ids[: n_users - n_test], None)
        self.base.test_user_dataset = UserDataset(ids[n_users - n_test:], None)
        self._make_loaders()

    @property
    def store(self) -> ReplayStore:
        if self._store is None:
            if self.device.type != "cuda" or not torch.cuda.is_available():
                from .. import _lib as L
                raise L.RecnnHipError(f"{type(self).__name__} batches are built on the GPU; device {self.device} is not usable "
                                      "(no CPU fallback)")
            if getattr(self, "_csr", None) is not None:
                self._store = ReplayStore.from_arrays(*self._csr, self.device)
            else:
                user_dict = self.base.train_user_dataset.user_dict
                ids = list(self.base.train_user_dataset.users) + list(self.base.test_user_dataset.users)
                self._store = ReplayStore(ids, user_dict, self.device)
            self._table = self.base.embeddings.to(self.device, torch.float32).contiguous()
        return self._store

    @property
    def table(self) -> torch.Tensor:
        self.store
        return self._table


class FrameEnv(StoreEnv):
    """Static length user environment (env.py:190-256).

    Extra keyword arguments (extensions, all optional):
      device          torch device of the replay store and the batches (default: cuda)
      rows_per_batch  cut every batch to exactly this many transition rows (benchmark configuration
                      "batch 2048"); the reference's batch_size counts USERS, so its row count varies
      contiguous      return reference-layout contiguous tensors instead of views into packed rows
    """

    def __init__(self, path, frame_size=10, batch_size=25, num_workers=1, *args, device=None, rows_per_batch=None,
                 contiguous=False, **kwargs):
        kwargs["frame_size"] = frame_size
        super().__init__(path, min_seq_size=frame_size + 1, *args, **kwargs)
        self.frame_size = frame_size
        self.batch_size = batch_size
        self.num_workers = num_workers          # kept for API compatibility; there are no worker processes
        self.rows_per_batch = rows_per_batch
        self.contiguous = contiguous
        self.device = torch.device("cuda" if device is None else device)
        self._store = None
        self._table = None
        self._host_off = None                   # host copy of the store's user offsets (target_items)
        if path is not None:
            self._make_loaders()

    @classmethod
    def from_user_dict(cls, embeddings: torch.Tensor, user_dict, train_users, test_users=(), frame_size=10, batch_size=25,
                       **kwargs):
        """Build an env from in-memory data (the output contract of `prepare_dataset`) without csv / pickle files."""
        self = cls(None, frame_size, batch_size, **kwargs)
        self._fill_from_user_dict(embeddings, user_dict, train_users, test_users)
        return self

    @classmethod
    def from_store(cls, embeddings: torch.Tensor, items, ratings, user_off, frame_size=10, batch_size=25, test_fraction=0.05,
                   **kwargs):
        """Build an env straight from CSR arrays (items int[sum L], ratings float[sum L], user_off int64[U+1]): the
        replay-store form of the reference's `user_dict`, for data that never existed as per-user python objects."""
        self = cls(None, frame_size, batch_size, **kwargs)
        self._fill_from_csr(embeddings, items, ratings, user_off, test_fraction)
        return self

    def _make_loaders(self):
        self.train_dataloader = FrameLoader(self, self.base.train_user_dataset, self.batch_size, shuffle=True)
        self.test_dataloader = FrameLoader(self, self.base.test_user_dataset, self.batch_size, shuffle=True)

    # ------------------------------------------------------------------ batches
    def collate_users(self, user_ids):
        """Batch of the given users, windows concatenated in the given order (prepare_batch_static_size)."""
        return self.collate_slots(self.store.slots(user_ids), user_ids)

    def collate_slots(self, slots, user_ids=None, rows_per_batch="env"):
        """The same for users given by their slots in the replay store (what the engine's sampler permutes)."""
        st = self.store
        slots = np.asarray(slots, dtype=np.int32)          # (the gather kernels read 32-bit slots)
        if user_ids is None:
            user_ids = slots
        sizes = st.lengths[slots]
        total = int(np.maximum(sizes - self.frame_size, 0).sum())
        cut = self.rows_per_batch if rows_per_batch == "env" else rows_per_batch
        rows = total if cut is None else min(cut, total)
        meta = {"users": torch.as_tensor(np.asarray(list(user_ids))), "sizes": torch.from_numpy(sizes.copy())}
        if self.embed_batch is utils.batch_tensor_embeddings:
            users_d = torch.from_numpy(slots).to(self.device)
            batch = utils.gather_frames(st.items, st.ratings, st.user_off, users_d, total, rows, self.frame_size, self._table,
                                        contiguous=self.contiguous)
            batch["meta"] = meta
            return batch
        # custom embed function: give it the windowed index batch on the device (generic torch path)
        f1 = self.frame_size + 1
        starts = np.concatenate([st_off + np.arange(max(L - self.frame_size, 0)) for st_off, L in
                                 zip(st.user_off.cpu().numpy()[slots], sizes)]) if len(slots) else np.zeros(0, np.int64)
        idx = torch.from_numpy(starts[:rows, None] + np.arange(f1)[None, :]).to(self.device)
        win = {"items": st.items[idx].long(), "ratings": st.ratings[idx], "sizes": meta["sizes"].to(self.device),
               "users": meta["users"]}
        return self.embed_batch(batch=win, item_embeddings_tensor=self._table, frame_size=self.frame_size)

    def collate_rows(self, seq_slots, skip0: int, row_start: int, rows: int):
        """`rows` consecutive rows, starting at global row `row_start`, of the concatenated windows of the users `seq_slots` (store
        slots; the first one with its first `skip0` windows left out): what a DENSE epoch's batch holds (fused.attach_sampler).  The
        users that overlap the range are collated whole -- `prepare_batch_static_size` semantics, `done` at each user's last
        window -- and the range is cut out of that."""
        st = self.store
        seq = np.asarray(seq_slots, dtype=np.int64)
        wins = np.maximum(st.lengths[seq].astype(np.int64) - self.frame_size, 0)
        wins[0] = max(int(wins[0]) - int(skip0), 0)
        cum = np.cumsum(wins)
        if row_start + rows > int(cum[-1]):
            raise IndexError("collate_rows: the sequence holds fewer rows")
        i0 = int(np.searchsorted(cum, row_start, side="right"))
        i1 = int(np.searchsorted(cum, row_start + rows - 1, side="right"))
        before = int(cum[i0 - 1]) if i0 > 0 else 0
        a = row_start - before + (int(skip0) if i0 == 0 else 0)       # offset inside the whole-user collate of seq[i0 .. i1]
        whole = self.collate_slots(seq[i0:i1 + 1].astype(np.int32), rows_per_batch=None)
        out = {k: (v[a:a + rows] if isinstance(v, torch.Tensor) else v) for k, v in whole.items()}
        return out

    def _target_positions(self, batch, slots, what):
        """(pos, start): per row of the batch, the store position of its action (the item at the end of its window) and the store
        position where its user's history begins; host int64 arrays.  Shared by `target_items` and `seen_items`."""
        st = self.store
        meta = batch["meta"]
        if slots is None:
            try:
                slots = st.slots(meta["users"].tolist())
            except KeyError as e:
                raise ValueError(f"{what}: user {e} of the batch is not in the replay store (a collate_slots batch made "
                                 "without user_ids names slots: pass them as `slots`)") from None
        slots = np.asarray(slots, dtype=np.int32)
        sizes = meta["sizes"].numpy().astype(np.int64)
        if len(slots) != len(sizes) or not np.array_equal(st.lengths[slots], sizes):
            raise ValueError(f"{what}: the batch's users and sizes do not match the replay store")
        rows = batch["action"].shape[0]
        wins = np.maximum(sizes - self.frame_size, 0)
        if rows > int(wins.sum()):
            raise ValueError(f"{what}: the batch has {rows} rows but its users have {int(wins.sum())} windows")
        if self._host_off is None:
            self._host_off = np.concatenate([[0], np.cumsum(st.lengths)]).astype(np.int64)
        first = self._host_off[slots] + self.frame_size           # position of each user's first action in the store
        before = np.cumsum(wins) - wins                            # rows of the users before it
        pos = (np.repeat(first - before, wins) + np.arange(int(wins.sum())))[:rows]
        return pos, np.repeat(self._host_off[slots], wins)[:rows]

    def target_items(self, batch, slots=None):
        """int64 [rows] on the env's device: the table row id of each row's action, the item at the end of its window -- what
        `FlatIndex.rank_of(policy(batch["state"]), env.target_items(batch))` ranks.  Built from `batch["meta"]` and the batch's
        row count through the replay store: for each user of `meta["users"]` in order, the items at positions `frame_size ..` of
        its history, concatenated and cut to the batch's rows.  Covers the batches of `collate_users`, `collate_slots` and the
        two loaders, with or without `rows_per_batch`.  A `collate_slots` batch made without `user_ids` records the slots as its
        users; where those differ from the user ids (`from_user_dict`), give the slots here.  `collate_rows` batches start
        inside a user and are not covered."""
        pos, _ = self._target_positions(batch, slots, "target_items")
        return self.store.items[torch.from_numpy(pos).to(self.device)].long()

    def seen_items(self, batch, slots=None, keep_targets=True):
        """`retrieval.SeenItems` of the batch's rows: for each row, everything its user did before the row's target -- the window
        that forms the state included -- as a slice of the replay store's `items` (no ids are copied): `starts` is the user's
        offset in the store, `lengths` the target's store position minus that offset.  With `keep_targets` the row's own target
        (`target_items(batch)`) is taken out of its list again, so a user who consumed the target earlier can still be recommended
        it and `search` and `rank_of` stay consistent with each other.  Pass it as `exclude` to `FlatIndex.search` / `rank_of`.
        Covers the batches `target_items` covers, takes `slots` as it does and raises its errors."""
        from ..retrieval import SeenItems
        pos, start = self._target_positions(batch, slots, "seen_items")
        items = self.store.items
        keep = items[torch.from_numpy(pos).to(self.device)].long() if keep_targets else None
        return SeenItems(items, torch.from_numpy(start), torch.from_numpy(pos - start), keep)

    def prepare_batch_wrapper(self, x):
        """collate_fn-compatible entry (env.py:241-248): x = list of UserDataset items."""
        return self.collate_users([b["users"] for b in x])

    def train_batch(self):
        """A fresh shuffled iterator per call, first batch of it (env.py:250-252)."""
        return next(iter(self.train_dataloader))

    def test_batch(self):
        return next(iter(self.test_dataloader))


class SeqLoader:
    """What `SeqEnv.train_dataloader` is: a re-iterable, len()-able stream of batches of `batch_size` USERS in dataset order
    (the reference's DataLoader(shuffle=False, collate_fn=padder + prepare_batch_dynamic_size)).  Each batch is the
    `prepare_batch_dynamic_size` dict, built on the GPU from the replay store in one launch."""

    def __init__(self, env, dataset: UserDataset, batch_size: int):
        self.env = env
        self.dataset = dataset
        self.batch_size = batch_size

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def user_batches(self):
        users = self.dataset.users
        for i in range(0, len(users), self.batch_size):
            yield list(users[i:i + self.batch_size])

    def __iter__(self):
        for ids in self.user_batches():
            yield self.env.collate_users(ids)


class SeqEnv(StoreEnv):
    """Dynamic-length user environment: whole user histories run through a recurrent state encoder, and a replay buffer of
    (state, action, reward, next_state) rows is filled from a random 5 % of the steps (the design sketched, and left disabled, in
    the reference's env.py).  `train_batch()` / `test_batch()` are infinite generators of full buffers.

    Per batch of U users (dataset order; the datasets are sorted by length, so a batch holds users of similar length):
    T = min(sizes) - 1 steps; the input of step t is [embedding(item_t) | rating_t]; next_state = h_t, state = h_{t-1},
    action = embedding(item_t), reward = rating_t.  One `np.random.random()` draw per step, in step order; step t is kept when its
    draw is > 0.95 and t >= 1.  Each kept step appends U rows, meta["step"] receives t, meta["sizes"] / meta["users"] describe the
    current user batch.  When the buffer holds `max_buf_size` rows, or the next U rows would not fit, the buffers are yielded as
    {"state", "action", "reward", "next_state", "done", "meta"} (full tensors, zeros beyond meta["rows"]; `done` is all zeros, added
    so that `recnn.nn.ddpg_update` runs on the batch unchanged) and the buffer starts over.

    All T steps of a user batch are ONE HIP launch chain (`recnn_amd.nn.functional.lstm_encode` or `gru_encode`), the kept rows one
    more (`seq_collect`); the padded [U, Lmax, E] tensor is not built on this path.  `state_encoder` must be a single-layer
    unidirectional `torch.nn.LSTM(E + 1, H)` or `torch.nn.GRU(E + 1, H)`, or a `recnn_amd.nn.AttentionEncoder(E + 1, H, heads)`
    (`attn_encode`: causal self-attention over the steps of the batch) or a `recnn_amd.nn.TransformerStateEncoder(E + 1, H, heads)`
    (`transformer_encode`: pre-LN transformer blocks over the steps of the batch), on the GPU; `batch_first` is ignored (users are always
    the batch).  A module of any other type (a `torch.nn.RNN`, say) is refused at construction, naming the type.

    The encoder is a FROZEN feature extractor for the replay buffer: the states in the buffer carry no autograd graph, and the
    encoder's weights are read live, so a caller may change them between batches.  `user_batch(user_ids, steps)` is the way to
    TRAIN it: the same rows for one user batch, on policy, with `state` / `next_state` attached to the encoder's graph
    (`recnn_amd.nn.functional.lstm_encode_train` / `gru_encode_train`, backward through time in HIP).

    Default layout: [max_buf_size, H], [max_buf_size, E], [max_buf_size, 1], [max_buf_size, H] with H and E taken from the
    encoder and the embedding table (the reference hard-codes 256 and 128)."""

    def __init__(self, path, state_encoder, batch_size=25, device=torch.device("cuda"), layout=None, max_buf_size=1000,
                 num_workers=1, embed_batch=utils.batch_tensor_embeddings, *args, **kwargs):
        from ..nn.attention import AttentionEncoder
        from ..nn.transformer import TransformerStateEncoder
        if state_encoder is not None and not isinstance(state_encoder, (torch.nn.LSTM, torch.nn.GRU, AttentionEncoder,
                                                                        TransformerStateEncoder)):
            t = type(state_encoder)
            raise TypeError(f"SeqEnv: state_encoder is a {t.__module__}.{t.__qualname__}; the HIP encoders are a single-layer "
                            "torch.nn.LSTM(E + 1, H), a single-layer torch.nn.GRU(E + 1, H), a "
                            "recnn_amd.nn.AttentionEncoder(E + 1, H, heads) and a "
                            "recnn_amd.nn.TransformerStateEncoder(E + 1, H, heads)")
        super().__init__(path, min_seq_size=10, embed_batch=embed_batch, *args, **kwargs)
        self.state_encoder = state_encoder
        self.batch_size = batch_size
        self.num_workers = num_workers          # kept for API compatibility; there are no worker processes
        self.device = torch.device(device)
        self.max_buf_size = max_buf_size
        self.buffer_layout = layout
        if path is not None:
            self._make_loaders()

    @classmethod
    def from_user_dict(cls, embeddings: torch.Tensor, user_dict, train_users, test_users=(), state_encoder=None, **kwargs):
        """Build an env from in-memory data (the output contract of `prepare_dataset`) without csv / pickle files."""
        self = cls(None, state_encoder, **kwargs)
        self._fill_from_user_dict(embeddings, user_dict, train_users, test_users)
        return self

    @classmethod
    def from_store(cls, embeddings: torch.Tensor, items, ratings, user_off, state_encoder=None, test_fraction=0.05, **kwargs):
        """Build an env straight from CSR arrays (see FrameEnv.from_store)."""
        self = cls(None, state_encoder, **kwargs)
        self._fill_from_csr(embeddings, items, ratings, user_off, test_fraction)
        return self

    def _make_loaders(self):
        if self.buffer_layout is None:
            h, e = self.state_encoder.hidden_size, self.base.embeddings.shape[1]
            n = self.max_buf_size
            self.buffer_layout = [torch.Size([n, h]), torch.Size([n, e]), torch.Size([n, 1]), torch.Size([n, h])]
        self._check_layout()
        self.train_dataloader = SeqLoader(self, self.base.train_user_dataset, self.batch_size)
        self.test_dataloader = SeqLoader(self, self.base.test_user_dataset, self.batch_size)
        self.train_buffer = utils.ReplayBuffer(self.max_buf_size, layout=self.buffer_layout, device=self.device)
        self.test_buffer = utils.ReplayBuffer(self.max_buf_size, layout=self.buffer_layout, device=self.device)

    def _check_layout(self):
        """The collect launch writes rows of H, E, 1 and H floats: a layout of other widths (the reference's hard-coded 256 / 128
        over another encoder, say) or of unequal row counts is refused here, not discovered by the kernel."""
        h, e = self.state_encoder.hidden_size, self.base.embeddings.shape[1]
        lay = [tuple(int(v) for v in i) for i in self.buffer_layout]
        ok = len(lay) == 4 and all(len(i) >= 1 for i in lay) and len({i[0] for i in lay}) == 1 and lay[0][1:] == (h,) \
            and lay[1][1:] == (e,) and lay[2][1:] in ((), (1,)) and lay[3][1:] == (h,)
        if not ok:
            raise ValueError(f"SeqEnv: layout {lay} does not fit the encoder and the table: needs [n, {h}], [n, {e}], [n, 1] (or [n]), "
                             f"[n, {h}] with one n (hidden_size = {h}, embedding width = {e})")

    def collate_users(self, user_ids):
        """The `prepare_batch_dynamic_size` dict of the given users: items float32[U, Lmax, E] (padded positions hold item 0's
        row), ratings float32[U, Lmax], sizes float32[U], users list."""
        st = self.store
        slots = st.slots(user_ids)
        _, ratings, rows = utils.gather_padded(st, self._table, slots)
        return {"items": rows, "users": list(user_ids), "ratings": ratings, "sizes": torch.from_numpy(st.lengths[slots].copy()).float()}

    def prepare_batch_wrapper(self, x):
        """collate_fn-compatible entry: x = list of UserDataset items."""
        return utils.prepare_batch_dynamic_size(utils.padder(x), self.table)

    def _hand_out(self, buffer):
        out = buffer.get()
        out["meta"] = dict(buffer.meta, step=list(buffer.meta["step"]), rows=buffer.len())
        out["done"] = torch.zeros(out["state"].shape[0], device=out["state"].device)
        buffer.flush()
        return out

    def _generate(self, loader, buffer):
        from ..nn import functional as F_hip
        if len(loader.dataset) == 0:
            raise ValueError("SeqEnv: the dataset is empty, there is nothing to generate batches from")
        st = self.store
        # a step is kept only at t >= 1 of T = min(sizes) - 1 steps: some user batch must have histories of at least 3 elements
        if not any(int(st.lengths[st.slots(ids)].min()) >= 3 for ids in loader.user_batches()):
            raise ValueError("SeqEnv: no user batch has histories of at least 3 elements, no step can ever be kept")
        while True:
            for ids in loader.user_batches():
                slots = st.slots(ids)
                sizes = st.lengths[slots]
                n_users = len(ids)
                if n_users > buffer.capacity:
                    raise ValueError(f"SeqEnv: a batch of {n_users} users does not fit a buffer of {self.max_buf_size} rows")
                buffer.meta.update({"sizes": torch.from_numpy(sizes.copy()).float().to(self.device), "users": ids})
                n_steps = int(sizes.min()) - 1
                draws = np.random.random(n_steps) if n_steps > 0 else np.zeros(0)     # the stream of one draw per step
                kept = [t for t in range(1, n_steps) if draws[t] > 0.95]
                if not kept:
                    continue
                # one encode for every step up to the last kept one (the later steps would not be looked at)
                h = F_hip.state_encode(self.state_encoder, st, self._table, slots, kept[-1] + 1)
                while kept:
                    if not buffer.room(n_users):
                        yield self._hand_out(buffer)
                    fit = (buffer.capacity - buffer.len()) // n_users
                    now, kept = kept[:fit], kept[fit:]
                    F_hip.seq_collect(h, now, st, self._table, slots, buffer.reserve(n_users * len(now)))
                    buffer.meta["step"].extend(now)
                    if buffer.len() >= self.max_buf_size:
                        yield self._hand_out(buffer)

    def user_batch(self, user_ids, steps, table=None):
        """{"state", "action", "reward", "next_state", "done", "meta"} for the users `user_ids` and the kept `steps` (strictly
        increasing, 1 <= step < min(sizes) - 1): exactly the rows the generator would put into the buffer for them, U per step in
        the order k * U + u, without going through the buffer.  When grad mode is on and a parameter of the encoder requires
        grad, `state` and `next_state` are attached to the encoder's graph (`lstm_encode_train` or `gru_encode_train`, whichever
        the encoder is, + `seq_collect_rows`): a loss on them back-propagates through time into the encoder's weights.  Otherwise
        they are the detached rows of `lstm_encode` / `gru_encode`.

        `table` (default: the env's own embedding table, frozen) is a contiguous float32 GPU tensor of the env table's shape that
        is read INSTEAD of it -- a trainable copy of the embeddings, say.  When it requires grad, `state` / `next_state` are
        attached to it as well (`lstm_encode_train` / `gru_encode_train(..., train_table=True)`): their gradients reach `table.grad` through the
        encoder, also with every encoder parameter frozen.  The `action` rows are gathered from it and stay non-differentiable:
        a value loss's gradient with respect to `action` is not sent back (the update steps return state gradients only)."""
        from ..nn import functional as F_hip
        st = self.store
        ids = list(user_ids)
        slots = st.slots(ids)
        sizes = st.lengths[slots]
        steps = [int(t) for t in np.asarray(steps).reshape(-1)]
        if not ids or not steps:
            raise ValueError("SeqEnv.user_batch: needs at least one user and one step")
        n_steps = int(sizes.min()) - 1
        if any(b <= a for a, b in zip(steps, steps[1:])):
            raise ValueError(f"SeqEnv.user_batch: steps must be strictly increasing (got {steps})")
        if steps[0] < 1 or steps[-1] >= n_steps:
            raise ValueError(f"SeqEnv.user_batch: steps must lie in 1 .. {n_steps - 1} (the shortest history has "
                             f"{int(sizes.min())} elements)")
        tbl = self._table
        if table is not None:
            if not (isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.float32 and table.is_contiguous()
                    and table.shape == tbl.shape and table.device == tbl.device):
                raise ValueError(f"SeqEnv.user_batch: table must be a contiguous float32 tensor of shape {tuple(tbl.shape)} on "
                                 f"{tbl.device}")
            tbl = table
        h = F_hip.state_encode(self.state_encoder, st, tbl, slots, steps[-1] + 1, train=True, train_table=tbl.requires_grad)
        state, action, reward, next_state = F_hip.seq_collect_rows(h, steps, st, tbl.detach(), slots)
        meta = {"sizes": torch.from_numpy(sizes.copy()).float().to(self.device), "users": ids, "step": steps, "rows": state.shape[0]}
        return {"state": state, "action": action, "reward": reward, "next_state": next_state,
                "done": torch.zeros(state.shape[0], device=state.device), "meta": meta}

    def target_items(self, batch):
        """int64 [rows] on the env's device: the table row id of each row's action -- for row k * U + u of a `user_batch`, the item
        at position `steps[k]` of user u's history.  What a next-item loss over `batch["state"]` is trained on
        (`recnn_amd.nn.next_item_update`) and what `FlatIndex.rank_of` ranks.  Built from `batch["meta"]` (users, step) through
        the replay store, like `FrameEnv.target_items`; a generator batch whose rows stem from more than one user batch (its meta
        names the last one only) is refused."""
        st = self.store
        meta = batch["meta"]
        try:
            slots = np.asarray(st.slots(list(meta["users"])), dtype=np.int64)
        except KeyError as e:
            raise ValueError(f"target_items: user {e} of the batch is not in the replay store") from None
        steps = np.asarray([int(t) for t in meta["step"]], dtype=np.int64)
        rows = int(meta.get("rows", batch["state"].shape[0]))
        if rows != len(steps) * len(slots):
            raise ValueError(f"target_items: the batch has {rows} rows, its meta describes {len(steps)} steps of {len(slots)} users")
        if len(steps) and (steps.min() < 0 or steps.max() >= int(st.lengths[slots].min())):
            raise ValueError("target_items: the batch's steps do not lie inside its users' histories")
        off = np.concatenate([[0], np.cumsum(st.lengths)]).astype(np.int64)
        pos = (steps[:, None] + off[slots][None, :]).reshape(-1)
        return st.items[torch.from_numpy(pos).to(self.device)].long()

    def train_batch(self):
        return self._generate(self.train_dataloader, self.train_buffer)

    def test_batch(self):
        return self._generate(self.test_dataloader, self.test_buffer)
