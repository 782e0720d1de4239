"""The per-session key/value cache of the attention encoders and the session wrapper around it (csrc/attn_dev.h):
what `recnn_amd.nn.functional.attn_append` / `transformer_append` extend step by step."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from .attention import AttentionEncoder
from .transformer import TransformerStateEncoder


def _refuse_encoder(name, enc):
    t = type(enc)
    raise L.RecnnHipError(f"{name}: the encoder is a {t.__module__}.{t.__qualname__}; a key/value cache serves a "
                          "recnn_amd.nn.AttentionEncoder or a recnn_amd.nn.TransformerStateEncoder (a torch.nn.LSTM or torch.nn.GRU "
                          "already carries its state: lstm_encode / gru_encode take h0c0 / h0 and return the final state)")


def encoder_config(name, enc):
    """(E, H, heads, layers, window) of an attention encoder -- what a cache is built for; another module is refused by name."""
    if isinstance(enc, AttentionEncoder):
        layers = 1
    elif isinstance(enc, TransformerStateEncoder):
        layers = len(enc.layers)
    else:
        _refuse_encoder(name, enc)
    return (enc.input_size - 1, enc.hidden_size, enc.num_heads, layers, None if enc.window is None else int(enc.window))


class KVCache:
    """Keys and values of `n_sessions` sessions of one attention encoder, `capacity` positions each:

        kv       float32 [layers, n_sessions, capacity, 2 H] on the GPU: position p of a session holds [k_p | v_p] in slot p % capacity
                 (an AttentionEncoder has one layer)
        lengths  int64 numpy [n_sessions] on the host: the positions appended so far.  It is authoritative -- every append call uploads
                 the positions of its rows, nothing on the device counts -- and public, like `kv`

    `capacity` is a multiple of 64.  Without a window a session holds at most `capacity` positions.  With `encoder.window = w` the
    cache is a ring and a session may run for ever; the ring must keep apart the positions an append of up to `max_append` steps
    stages and the slots it writes: `capacity >= KVCache.min_capacity(w, max_append)`.  `reset(rows)` forgets sessions (their
    lengths become 0; the memory is not cleared: an append never reads a slot it has not written since).

    Refused: another encoder type and a CPU module (RecnnHipError), a capacity that is no multiple of 64 or below `min_capacity`,
    max_append < 1, n_sessions outside 1 .. 65535 (ValueError)."""

    def __init__(self, encoder, n_sessions, capacity, max_append=64, device=None):
        self.config = encoder_config("KVCache", encoder)
        E, H, heads, layers, window = self.config
        p = next(encoder.parameters())
        dev = torch.device(device) if device is not None else p.device
        if not p.is_cuda or dev.type != "cuda":
            raise L.RecnnHipError(f"KVCache: the encoder lives on {p.device} and the cache would live on {dev}; both need a GPU "
                                  "(recnn_amd has no CPU fallback)")
        n_sessions, capacity, max_append = int(n_sessions), int(capacity), int(max_append)
        if not 1 <= n_sessions <= 65535:
            raise ValueError(f"KVCache: n_sessions={n_sessions} must be in 1 .. 65535")
        if max_append < 1:
            raise ValueError(f"KVCache: max_append={max_append} must be at least 1")
        if capacity < 64 or capacity % 64:
            raise ValueError(f"KVCache: capacity={capacity} must be a positive multiple of 64")
        if window is None and max_append > capacity:
            raise ValueError(f"KVCache: max_append={max_append} does not fit capacity={capacity}")
        if window is not None and capacity < self.min_capacity(window, max_append):
            raise ValueError(f"KVCache: capacity={capacity} is below min_capacity(window={window}, max_append={max_append}) = "
                             f"{self.min_capacity(window, max_append)}")
        self.n_sessions, self.capacity, self.max_append, self.device = n_sessions, capacity, max_append, dev
        self.kv = torch.empty(layers, n_sessions, capacity, 2 * H, dtype=torch.float32, device=dev)
        self.lengths = np.zeros(n_sessions, dtype=np.int64)
        self._dense = {}

    @staticmethod
    def min_capacity(window, max_append):
        """The smallest ring for `window` and appends of up to `max_append` steps: 64 ceil((window - 1) / 64) + 64 ceil((max_append
        + 63) / 64), from the tile walk of the append's attention kernel.  Host arithmetic of the library."""
        out = C.c_int()
        L.call("recnn_kv_min_capacity", int(window), int(max_append), C.byref(out))
        return out.value

    def reset(self, rows=None):
        """Forget the sessions `rows` (default: all)."""
        if rows is None:
            self.lengths[:] = 0
        else:
            self.lengths[self.checked_rows(rows, "KVCache.reset")] = 0

    def checked_rows(self, rows, name, count=None):
        """`rows` as an int64 numpy array of distinct cache rows (default: all, in order); ValueError by the argument's name."""
        if rows is None:
            rows = np.arange(self.n_sessions, dtype=np.int64)
        else:
            if isinstance(rows, torch.Tensor):
                rows = rows.detach().cpu().numpy()
            rows = np.asarray(rows)
            if rows.ndim != 1 or (rows.size and not np.issubdtype(rows.dtype, np.integer)):
                raise ValueError(f"{name}: rows must be a one-dimensional sequence of integers")
            rows = rows.astype(np.int64)
            if rows.size and (rows.min() < 0 or rows.max() >= self.n_sessions):
                raise ValueError(f"{name}: rows must lie in 0 .. {self.n_sessions - 1} (the cache's sessions)")
            if np.unique(rows).size != rows.size:
                raise ValueError(f"{name}: rows must be distinct (a call extends a session once)")
        if count is not None and rows.size != count:
            raise ValueError(f"{name}: {rows.size} rows for {count} rows of items")
        return rows

    def dense_store(self, n):
        """(user_off int64 [n_sessions + 1], slots int32 [n_sessions]) on the device: [R, n] inputs given directly, read as a store
        whose histories are the rows -- the gathered linear kernel then runs its own chain on them."""
        if n not in self._dense:
            self._dense[n] = (torch.arange(self.n_sessions + 1, dtype=torch.int64, device=self.device) * n,
                              torch.arange(self.n_sessions, dtype=torch.int32, device=self.device))
        return self._dense[n]


class EncoderSession:
    """Serving sessions of an attention encoder: owns a `KVCache` of `n_sessions` sessions, `append(items, ratings, rows)` runs
    `attn_append` or `transformer_append` by the encoder's type and returns h [R, n, H]; `state(rows)` is the last returned row per
    session, [R, H] -- what `Actor` and `WolpertingerPolicy.recommend` take; `reset(rows)` starts sessions afresh.  Another encoder
    type is refused by name (a torch.nn.LSTM or torch.nn.GRU carries its state through `lstm_encode` / `gru_encode`)."""

    def __init__(self, enc, table, n_sessions, capacity, max_append=64):
        self.cache = KVCache(enc, n_sessions, capacity, max_append)
        self.enc, self.table = enc, table
        self._last = torch.zeros(n_sessions, enc.hidden_size, dtype=torch.float32, device=self.cache.device)

    def append(self, items, ratings, rows=None):
        from . import functional as F
        fn = F.attn_append if isinstance(self.enc, AttentionEncoder) else F.transformer_append
        h = fn(self.enc, self.cache, self.table, items, ratings, rows)
        self._last[self._index(rows, "EncoderSession.append")] = h[:, -1]
        return h

    def state(self, rows=None):
        idx = self.cache.checked_rows(rows, "EncoderSession.state")
        if idx.size and int(self.cache.lengths[idx].min()) == 0:
            raise ValueError("EncoderSession.state: rows holds a session nothing has been appended to")
        return self._last[torch.from_numpy(idx).to(self.cache.device)]

    def reset(self, rows=None):
        self.cache.reset(rows)

    def _index(self, rows, name):
        return torch.from_numpy(self.cache.checked_rows(rows, name)).to(self.cache.device)
