"""tuning.frozen_window: in the bf16 cycle schedule the frozen networks read s' as shifted windows of the cycle's state / action rows
(+ the ten next ratings) instead of a materialised next_state row per transition (csrc/mlpf.hip: up to four layer-1 segments,
csrc/gather_dev.h: no next rows).  Same contraction order per output element, so everything is equal BIT FOR BIT with the knob on and off,
and equal to the eager step loop.

Shapes: 128 rows per batch (the 128-row and the 64-row workgroup forms are both eligible), users of 11-14 items = 1-4 windows each, so
user ends (done = 1, breaks of the sliding-window runs) fall inside 64- and 128-row panels and across batch boundaries.  policy period 3
and the request run(7) from step 5 = cycle segments of 2 + 3 + 2 steps: batch boundaries inside a panel-aligned cycle array, segments of
different lengths in both copies of the cycle arrays; with cycle_min_seg 3 the two 2-step segments take the fused forward on whole next
rows (the short-segment array of window mode) around a batched 3-step segment."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS, UPB, PE = 128, 128, 3
SEED = 977
FIRST, N = 5, 7
SEGS = (2, 3, 2)              # run(7) from step 5, policy steps 6 and 9; segment k lives in copy k & 1 of the cycle arrays


def _env(recnn_amd, cuda, n_users, seed=11, n_items=500):
    rng = np.random.default_rng(seed)
    lens = rng.integers(11, 15, size=n_users).astype(np.int64)          # 1..4 windows per user
    off = np.zeros(n_users + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    items = rng.integers(0, n_items, size=total, dtype=np.int32)
    ratings = (2.0 * (rng.integers(1, 11, size=total) * 0.5 - 2.5)).astype(np.float32)
    table = torch.randn(n_items, 128, generator=torch.Generator().manual_seed(seed))
    return recnn_amd.data.env.FrameEnv.from_store(table, items, ratings, off, frame_size=10, batch_size=25, device=cuda,
                                                  test_fraction=0.0, rows_per_batch=ROWS)


def _make(recnn_amd, cuda, env, algo):
    from recnn_amd.nn import fused
    fused.set_defaults(dtype="bf16", mask_mode="hash", seed=SEED)
    torch.manual_seed(31)
    nn = recnn_amd.nn
    if algo == "ddpg":
        a = nn.DDPG(nn.Actor(1290, 128, 256, 6e-1), nn.Critic(1290, 128, 256, 54e-2)).to(cuda)
        a.params["policy_step"] = PE
    else:
        a = nn.TD3(nn.Actor(1290, 128, 256, 6e-1), nn.Critic(1290, 128, 256, 54e-2), nn.Critic(1290, 128, 256, 54e-2)).to(cuda)
        a.params["policy_update"] = PE
    torch.manual_seed(57)                                  # the epoch permutation comes from the CPU generator
    a.attach_env(env, rows_per_batch=ROWS, users_per_batch=UPB)
    return a


def _masters(a):
    return {n: {k: v.detach().clone() for k, v in m.state_dict().items()} for n, m in a.nets.items()}


def _cycle_array(eng, name):
    """A cycle-mode array by its debug name (recnn_engine_buffer), wherever it lives -- the packed next rows of the cycle are the
    engine's own allocation, outside the workspace; None if the engine does not have the array."""
    r, c, ld, f = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
    p = eng.lib.recnn_engine_buffer(eng.handle, name.encode(), C.byref(r), C.byref(c), C.byref(ld), C.byref(f))
    if not p:
        return None
    esz = 4 if f.value else 2

    class Span:
        __cuda_array_interface__ = {"shape": (r.value * ld.value * esz,), "typestr": "|u1", "data": (int(p), False), "version": 2}
    raw = torch.as_tensor(Span(), device=eng.device)
    return raw.view(torch.float32 if f.value else torch.bfloat16).view(r.value, ld.value)[:, :c.value].clone()


def _run(recnn_amd, cuda, env, algo, window, min_seg):
    from recnn_amd._tune import set_default_tuning
    set_default_tuning(frozen_window=window, cycle_min_len=2, cycle_min_seg=min_seg)
    try:
        a = _make(recnn_amd, cuda, env, algo)
        eng = a._fused_ctx.engine
        assert eng.tuning.frozen_window == window and eng.tuning.cycle_min_seg == min_seg
        _, hist = a.run(FIRST, history=True)
        a.prepare_run(N, first_step=FIRST)                 # ONE made-to-order run graph: segments of 2 + 3 + 2 steps
        _, h = a.run(N, history=True)
        torch.cuda.synchronize()
        xn = [_cycle_array(eng, f"cycle_xn{b}") for b in range(2)]
        if window:
            assert xn[0] is None and xn[1] is None, "window mode must not allocate the cycle's packed next rows"
            na = [_cycle_array(eng, f"cycle_next_action{b}") for b in range(2)]
        else:
            assert xn[0] is not None and xn[1] is not None
            na = [x[:, :128] for x in xn]                  # the target actor's output: the action slot of the packed next rows
        out = {"hist": hist + h, "masters": _masters(a), "next_action": na,
               "gen_action": _cycle_array(eng, "cycle_gen_action"),
               "tq": [_cycle_array(eng, f"cycle_target_q{c + 1}") for c in range(2 if algo == "td3" else 1)]}
        assert all(t is not None for t in out["tq"]) and out["gen_action"] is not None
        return out
    finally:
        set_default_tuning(frozen_window=None, cycle_min_len=None, cycle_min_seg=None)


def _loop(recnn_amd, cuda, env, algo):
    a = _make(recnn_amd, cuda, env, algo)
    perm = a._fused_ctx.perm.cpu().numpy()
    hist = []
    for i in range(FIRST + N):
        batch = env.collate_users([int(u) for u in perm[i * UPB:(i + 1) * UPB]])
        assert batch["state"].shape[0] == ROWS
        done = batch["done"].float()
        assert 0 < int(done.sum()) < ROWS                  # user ends inside the batch
        hist.append(dict(a.update(batch, learn=True)))
        a.step()
    torch.cuda.synchronize()
    return hist, _masters(a)


_SHARED = {}


def _shared(recnn_amd, cuda, algo):
    """The env and the eager-loop reference of one algorithm, computed once for both segment thresholds."""
    if algo not in _SHARED:
        env = _env(recnn_amd, cuda, n_users=16 * UPB)
        _SHARED[algo] = (env, _loop(recnn_amd, cuda, env, algo))
    return _SHARED[algo]


@pytest.mark.parametrize("min_seg", [2, 3])
@pytest.mark.parametrize("algo", ["ddpg", "td3"])
def test_window_mode_equals_materialised_next_rows_and_the_eager_loop(cuda, algo, min_seg):
    import recnn_amd
    env, (lhist, lmasters) = _shared(recnn_amd, cuda, algo)
    on, off = _run(recnn_amd, cuda, env, algo, 1, min_seg), _run(recnn_amd, cuda, env, algo, 0, min_seg)
    # ---- knob on == knob off, bit for bit
    assert on["hist"] == off["hist"]
    for net, sd in off["masters"].items():
        for k, v in sd.items():
            assert torch.equal(v, on["masters"][net][k]), (net, k)
    assert torch.equal(on["gen_action"], off["gen_action"])
    for a, b in zip(on["tq"], off["tq"]):
        assert torch.equal(a, b)
    # the target actor's output of the batched segments: segment k of n steps left n * ROWS rows in copy k & 1 (the last one to use a
    # copy counts); segments below cycle_min_seg step through the fused forward, whose next_action lives elsewhere in window mode
    checked = 0
    for b in range(2):
        n_last = [n for k, n in enumerate(SEGS) if k & 1 == b][-1]
        if n_last < min_seg:
            continue
        rows = n_last * ROWS
        assert torch.equal(on["next_action"][b][:rows], off["next_action"][b][:rows]), b
        assert float(on["next_action"][b][:rows].float().abs().max()) > 0
        checked += 1
    assert checked >= 1
    # ---- == the eager step loop: parameters bit for bit, losses to summation order (as tests/test_gpu_bench_shape.py)
    for net, sd in lmasters.items():
        for k, v in sd.items():
            assert torch.equal(v, on["masters"][net][k]), (net, k)
    keys = ("value1", "value2", "policy") if algo == "td3" else ("value", "policy")
    assert len(on["hist"]) == len(lhist) == FIRST + N
    for x, y in zip(on["hist"], lhist):
        assert x["step"] == y["step"]
        for k in keys:
            assert np.isfinite(x[k]) and abs(x[k] - y[k]) <= 1e-5 * max(abs(y[k]), 1.0), (k, x, y)
