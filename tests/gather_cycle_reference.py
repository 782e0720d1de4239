"""numpy reference of the cycle gather (csrc/gather.hip frame_gather_multi_launch), shared by tests/test_gather_cycle_cpu.py (which pins
it to the oracle's collate) and tests/test_gpu_gather_cycle.py.

A plan row is (CSR offset of the window start << 1) | (1 on the user's last window), -1 where the batch has no row.  For a row with
window w = offset .. offset + F:
  state  = [emb(items[w0..wF-1]) | ratings[w0..wF-1]]   action = emb(items[wF])   reward = ratings[wF]   done = the flag
  next   = [emb(items[w1..wF])   | ratings[w1..wF]]     tail   = ratings[w1..wF]  (the form without next rows)
everything that is a row rounded to bf16 (nearest even), reward and done fp32.  Rows of plan entry -1 are not written."""
import numpy as np


def bf16_bits(x):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even; finite inputs."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def make_store(lengths, n_items, emb, seed):
    """A small replay store: users of the given history lengths, ratings on the half-star grid, a random fp32 table."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lengths)
    total = int(off[-1])
    items = rng.integers(0, n_items, size=total, dtype=np.int32)
    ratings = (2.0 * (rng.integers(1, 11, size=total) * 0.5 - 2.5)).astype(np.float32)
    table = rng.standard_normal((n_items, emb)).astype(np.float32)
    return items, ratings, off, table


def dense_plan(off, frame, rows, n_batches, cut=None):
    """The windows of all users in order, cut into n_batches batches of `rows` rows (a user's run crosses batch boundaries); plan
    rows from global row `cut` on are -1.  int64 [n_batches, rows]."""
    ent = []
    for u in range(len(off) - 1):
        n = int(off[u + 1] - off[u]) - frame
        for t in range(max(n, 0)):
            ent.append(((int(off[u]) + t) << 1) | (1 if t == n - 1 else 0))
    assert len(ent) >= n_batches * rows, "store too small for the plan"
    plan = np.asarray(ent[:n_batches * rows], dtype=np.int64)
    if cut is not None:
        plan[cut:] = -1
    return plan.reshape(n_batches, rows)


def cycle_gather_reference(items, ratings, table, plan, frame):
    """plan int64 [n_sets, rows] -> dict over the n_sets * rows output rows: valid bool[n], state / next_state uint16 [n, F * E + F],
    action uint16 [n, E], tail uint16 [n, F] (bf16 bit patterns), reward / done float32 [n]."""
    p = np.asarray(plan, dtype=np.int64).reshape(-1)
    n, F, E = p.size, frame, table.shape[1]
    valid = p >= 0
    src = np.where(valid, p >> 1, 0)
    win = src[:, None] + np.arange(F + 1)[None, :]
    emb = bf16_bits(table[items[win]])                       # [n, F + 1, E]
    rat = ratings[win]                                       # [n, F + 1]
    out = {"valid": valid,
           "state": np.concatenate([emb[:, :F].reshape(n, F * E), bf16_bits(rat[:, :F])], 1),
           "next_state": np.concatenate([emb[:, 1:].reshape(n, F * E), bf16_bits(rat[:, 1:])], 1),
           "action": emb[:, F].copy(),
           "tail": bf16_bits(rat[:, 1:]),
           "reward": rat[:, F].astype(np.float32),
           "done": (p & 1).astype(np.float32)}
    return out
