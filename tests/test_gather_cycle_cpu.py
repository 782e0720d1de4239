"""CPU: the numpy reference of the cycle gather (tests/gather_cycle_reference.py) pinned to the oracle's collate (oracle/recnn_oracle.py
frame_batch: rolling windows -> embeddings -> SARS', the reference project's prepare_batch_static_size + batch_tensor_embeddings), and
its own pieces -- the bf16 rounding, the dense plan -- to brute force.  tests/test_gpu_gather_cycle.py holds the kernels to this
reference and the reference once more to FrameEnv.collate_users, which needs the GPU."""
import numpy as np
import pytest
import torch

import gather_cycle_reference as G
from oracle import recnn_oracle as O


def test_bf16_bits_is_torch_round_to_nearest_even():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 7.0,
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, -2.5, 3.3895314e38, 1e-40], dtype=np.float32)])   # ties both ways
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(G.bf16_bits(x), want)


@pytest.mark.parametrize("frame,emb", [(3, 8), (10, 128)])
def test_reference_equals_the_oracle_collate(frame, emb):
    rng = np.random.default_rng(17)
    lengths = np.concatenate([np.full(5, frame + 1), rng.integers(frame + 2, frame + 6, size=9), [frame + 40]])
    rng.shuffle(lengths)
    items, ratings, off, table = G.make_store(lengths, 97, emb, seed=5)
    rows = int((lengths - frame).sum())
    plan = G.dense_plan(off, frame, rows, 1)
    ref = G.cycle_gather_reference(items, ratings, table, plan, frame)
    users = range(len(lengths))
    want = O.frame_batch([items[off[u]:off[u + 1]] for u in users], [ratings[off[u]:off[u + 1]] for u in users], table, frame)
    assert ref["valid"].all() and want["state"].shape[0] == rows
    for k in ("state", "next_state", "action"):
        assert np.array_equal(ref[k], G.bf16_bits(want[k])), k
    assert np.array_equal(ref["tail"], G.bf16_bits(want["next_state"][:, frame * emb:]))
    assert np.array_equal(ref["reward"], want["reward"]) and np.array_equal(ref["done"], want["done"])
    assert ref["done"].sum() == len(lengths)


def test_dense_plan_cuts_runs_at_batch_boundaries_and_ends_early():
    frame, rows = 3, 7
    lengths = [4, 10, 4, 4, 30]
    _, _, off, _ = G.make_store(lengths, 11, 8, seed=1)
    plan = G.dense_plan(off, frame, rows, 3, cut=18)
    assert plan.shape == (3, rows) and (plan.reshape(-1)[18:] == -1).all() and (plan.reshape(-1)[:18] >= 0).all()
    flat = plan.reshape(-1)[:18]
    # brute force: row g is window t of user u
    g = 0
    for u, n in enumerate(lengths):
        for t in range(n - frame):
            if g < 18:
                assert flat[g] >> 1 == off[u] + t and (flat[g] & 1) == (t == n - frame - 1), (u, t)
            g += 1
    # user 1's seven windows start at global row 1 and cross the first batch boundary (row 7) as one run
    assert (plan[0, 6] >> 1) + 1 == plan[1, 0] >> 1 and not plan[0, 6] & 1


def test_rows_without_a_plan_entry_are_marked_invalid():
    items, ratings, off, table = G.make_store([5, 6, 14], 13, 8, seed=2)
    plan = G.dense_plan(off, 3, 6, 2, cut=9)
    ref = G.cycle_gather_reference(items, ratings, table, plan, 3)
    assert ref["valid"].tolist() == [True] * 9 + [False] * 3
