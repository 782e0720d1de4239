"""The cycle gather (csrc/gather.hip frame_gather_multi_launch) with tuning.gather_cycle 1 -- long row runs per workgroup, every line of a
run loaded once, 16-byte stores -- and 0 -- the generic body --, both against the numpy reference (tests/gather_cycle_reference.py) byte for
byte, through recnn_debug_gather_cycle (csrc/recnn_hip_debug.h) on shapes the engine never produces; the reference itself once more against
FrameEnv.collate_users; and a whole engine run with the knob on and off.

Shapes: R = 32 rows per workgroup, so R - 1 / R + 1 / 2R + 3 / 128 rows per batch give one ragged workgroup, a one-row second workgroup,
three workgroups with a three-row tail, and four full ones.  Users of exactly frame + 1 items (every row a run of its own, F + 1 lines
each: the LDS line list at its worst) are mixed with users of frame + 2 .. frame + 5 items and one user of more than 2R windows (a run
that fills a whole workgroup and crosses batch boundaries), so runs end on a workgroup's first row, on its last, in the middle.  The plan
has four batches and the device cursor starts at the last one -- its last three rows are -1 --, so a three-batch launch wraps around."""
import ctypes as C

import numpy as np
import pytest
import torch

import gather_cycle_reference as G

pytestmark = pytest.mark.gpu

R_WG = 32
N_BATCHES = 4
SENT16, SENTF = 0x7B7B, -77.0


def _lengths(frame, need, seed):
    """History lengths whose windows cover `need` rows: single-window users, 2..5-window users, one long user early on."""
    rng = np.random.default_rng(seed)
    out, total = [], 0
    while total < need:
        n = 2 * R_WG + 5 if len(out) == 3 else (1 if rng.random() < 0.4 else int(rng.integers(2, 6)))
        out.append(frame + n)
        total += n
    return out


_CASES = {}


def _case(emb, frame, rows):
    """Store, plan and reference of one shape (shared by the launches of both knob values and both forms)."""
    key = (emb, frame, rows)
    if key not in _CASES:
        items, ratings, off, table = G.make_store(_lengths(frame, N_BATCHES * rows, seed=rows), 211, emb, seed=emb + frame)
        plan = G.dense_plan(off, frame, rows, N_BATCHES, cut=N_BATCHES * rows - 3)
        _CASES[key] = (items, ratings, table, plan)
    return _CASES[key]


def _launch(cuda, case, frame, rows, n_sets, knob, with_next, ld_pad=8):
    from recnn_amd import _lib as L
    items, ratings, table, plan = case
    E, F = table.shape[1], frame
    S = F * E + F
    ld = (E + S + 7) // 8 * 8 + ld_pad                       # columns past the row and one guard row stay sentinel
    ld_tail = (F + 3) // 4 * 4 + 4
    n = n_sets * rows
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    t_items, t_ratings, t_table, t_plan = d(items), d(ratings), d(table), d(plan)
    cursor = torch.tensor([N_BATCHES - 2], dtype=torch.int32, device=cuda)     # + cursor_add 1: the last batch first, then 0, 1
    xs = torch.full((n + 1, ld), SENT16, dtype=torch.int16, device=cuda)
    xn = torch.full((n + 1, ld), SENT16, dtype=torch.int16, device=cuda)
    tail = torch.full((n + 1, ld_tail), SENT16, dtype=torch.int16, device=cuda)
    reward = torch.full((n + 1,), SENTF, dtype=torch.float32, device=cuda)
    done = torch.full((n + 1,), SENTF, dtype=torch.float32, device=cuda)
    a = L.GatherCycleDebugArgs()
    a.items, a.ratings, a.table = t_items.data_ptr(), t_ratings.data_ptr(), t_table.data_ptr()
    a.plan, a.plan_stride = t_plan.data_ptr(), rows
    a.cursor, a.cursor_add, a.cursor_mod = cursor.data_ptr(), 1, N_BATCHES
    a.rows, a.frame, a.emb, a.n_sets = rows, F, E, n_sets
    a.action_h, a.state_h, a.ld_h = xs.data_ptr(), xs.data_ptr() + 2 * E, ld
    if with_next:
        a.next_h = xn.data_ptr() + 2 * E
    else:
        a.tail_n, a.ld_tail = tail.data_ptr(), ld_tail
    a.reward, a.done = reward.data_ptr(), done.data_ptr()
    a.gather_cycle = knob
    L.check(L.load().recnn_debug_gather_cycle(C.byref(a), C.sizeof(a), None), "recnn_debug_gather_cycle")
    torch.cuda.synchronize()
    return {"xs": xs.cpu().numpy().view(np.uint16), "xn": xn.cpu().numpy().view(np.uint16), "tail": tail.cpu().numpy().view(np.uint16),
            "reward": reward.cpu().numpy(), "done": done.cpu().numpy()}


def _expected(case, frame, rows, n_sets, with_next, like):
    items, ratings, table, plan = case
    E, F = table.shape[1], frame
    S = F * E + F
    order = [(N_BATCHES - 1 + j) % N_BATCHES for j in range(n_sets)]
    ref = G.cycle_gather_reference(items, ratings, table, plan[order], F)
    v = np.flatnonzero(ref["valid"])
    exp = {k: np.full_like(a, SENTF if a.dtype == np.float32 else SENT16) for k, a in like.items()}
    exp["xs"][v, :E] = ref["action"][v]
    exp["xs"][v, E:E + S] = ref["state"][v]
    if with_next:
        exp["xn"][v, E:E + S] = ref["next_state"][v]
    else:
        exp["tail"][v, :F] = ref["tail"][v]
    exp["reward"][v] = ref["reward"][v]
    exp["done"][v] = ref["done"][v]
    return exp, ref


def _assert_equal(got, exp, what):
    for k in exp:
        assert np.array_equal(got[k].view(np.uint32 if got[k].dtype == np.float32 else np.uint16),
                              exp[k].view(np.uint32 if exp[k].dtype == np.float32 else np.uint16)), (what, k)


@pytest.mark.parametrize("rows", [R_WG - 1, R_WG + 1, 2 * R_WG + 3, 128])
@pytest.mark.parametrize("n_sets", [1, 3])
@pytest.mark.parametrize("frame", [3, 10])
@pytest.mark.parametrize("emb", [8, 128])
def test_cycle_gather_equals_the_reference_byte_for_byte(cuda, emb, frame, n_sets, rows):
    case = _case(emb, frame, rows)
    plan = case[3]
    if rows == 128:
        # the case holds what the shapes are chosen for: user ends on a workgroup's first row, on its last and in between; a run that
        # fills a workgroup; a run cut by a batch boundary; rows without a plan entry
        last = np.flatnonzero(plan.reshape(-1) & 1 & (plan.reshape(-1) >= 0)) % rows % R_WG
        assert {0, R_WG - 1} <= set(last.tolist()) and len(set(last.tolist())) > 4
        assert any(not (plan[b, g * R_WG:(g + 1) * R_WG] & 1).any() for b in range(N_BATCHES) for g in range(rows // R_WG))
        assert any(plan[b, -1] >= 0 and not plan[b, -1] & 1 for b in range(N_BATCHES - 1))
    assert (plan[-1, -3:] == -1).all()
    for with_next in (False, True):
        for knob in (1, 0):
            got = _launch(cuda, case, frame, rows, n_sets, knob, with_next)
            exp, ref = _expected(case, frame, rows, n_sets, with_next, got)
            assert ref["valid"].sum() == n_sets * rows - 3
            _assert_equal(got, exp, (knob, with_next))


@pytest.mark.parametrize("emb,frame", [(8, 3), (128, 10)])
def test_rows_that_fail_the_16_byte_check_take_the_generic_body(cuda, emb, frame):
    """A row stride of 8 (mod 16) bytes: the launch must fall back to 8-byte stores and still write the same bytes."""
    case = _case(emb, frame, 2 * R_WG + 3)
    for knob in (1, 0):
        got = _launch(cuda, case, frame, 2 * R_WG + 3, 3, knob, False, ld_pad=4)
        assert got["xs"].shape[1] % 8 == 4
        exp, _ = _expected(case, frame, 2 * R_WG + 3, 3, False, got)
        _assert_equal(got, exp, knob)


def test_reference_equals_collate_users(cuda):
    """The numpy reference against the package's own collate on a small store (fp32 rows, rounded here)."""
    import recnn_amd
    frame, emb = 10, 128
    lengths = _lengths(frame, 200, seed=9)
    items, ratings, off, table = G.make_store(lengths, 211, emb, seed=4)
    env = recnn_amd.data.env.FrameEnv.from_store(torch.from_numpy(table), items, ratings, off, frame_size=frame, batch_size=25, device=cuda,
                                                 test_fraction=0.0)
    users = list(range(len(lengths)))
    batch = env.collate_users(users)
    rows = int((np.asarray(lengths) - frame).sum())
    ref = G.cycle_gather_reference(items, ratings, table, G.dense_plan(off, frame, rows, 1), frame)
    bits = lambda t: G.bf16_bits(t.float().cpu().numpy())
    assert batch["state"].shape[0] == rows
    for k in ("state", "next_state", "action"):
        assert np.array_equal(bits(batch[k]), ref[k]), k
    assert np.array_equal(batch["reward"].cpu().numpy(), ref["reward"]) and np.array_equal(batch["done"].float().cpu().numpy(), ref["done"])


# ------------------------------------------------------------------------------------------------ engine level
ROWS, UPB, PE, FIRST, N = 128, 128, 3, 5, 7        # as tests/test_gpu_frozen_window.py: run(7) from step 5 = cycle segments of 2 + 3 + 2 steps
CYCLE_INPUTS = ("cycle_xs", "cycle_tail_n", "cycle_reward", "cycle_done")


def _run(recnn_amd, cuda, env, knob, min_seg):
    import test_gpu_frozen_window as W
    from recnn_amd._tune import set_default_tuning
    set_default_tuning(gather_cycle=knob, cycle_min_len=2, cycle_min_seg=min_seg)
    try:
        a = W._make(recnn_amd, cuda, env, "ddpg")
        eng = a._fused_ctx.engine
        assert eng.tuning.gather_cycle == knob and eng.tuning.frozen_window == 1
        _, hist = a.run(FIRST, history=True)
        a.prepare_run(N, first_step=FIRST)
        _, h = a.run(N, history=True)
        torch.cuda.synchronize()
        arrays = {f"{n}{b}": W._cycle_array(eng, f"{n}{b}") for n in CYCLE_INPUTS for b in range(2)}
        assert all(v is not None for v in arrays.values())
        return {"hist": hist + h, "masters": W._masters(a), "arrays": arrays}
    finally:
        set_default_tuning(gather_cycle=None, cycle_min_len=None, cycle_min_seg=None)


@pytest.mark.parametrize("min_seg", [2, 3])
def test_engine_run_is_bit_equal_with_the_knob_on_and_off(cuda, min_seg):
    """min_seg 2: all three segments are batched (the form without next rows, both copies of the cycle arrays); 3: the two 2-step segments
    step through the fused forward on whole next rows (the generic body under either knob value) around a batched 3-step segment."""
    import recnn_amd
    import test_gpu_frozen_window as W
    env = W._env(recnn_amd, cuda, n_users=16 * UPB)
    on, off = _run(recnn_amd, cuda, env, 1, min_seg), _run(recnn_amd, cuda, env, 0, min_seg)
    assert on["hist"] == off["hist"] and len(on["hist"]) == FIRST + N
    for net, sd in off["masters"].items():
        for k, v in sd.items():
            assert torch.equal(v, on["masters"][net][k]), (net, k)
    for k, v in off["arrays"].items():
        assert torch.equal(v.view(torch.int32 if v.dtype == torch.float32 else torch.int16),
                           on["arrays"][k].view(torch.int32 if v.dtype == torch.float32 else torch.int16)), k
    assert float(on["arrays"]["cycle_xs1"].float().abs().max()) > 0 and float(on["arrays"]["cycle_tail_n1"].float().abs().max()) > 0
