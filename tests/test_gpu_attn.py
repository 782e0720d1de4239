"""The causal self-attention state encoder on the GPU (csrc/attn.hip): `attn_encode` / `attn_encode_train` against the float64 layer of
tests/attn_reference.py, the bitwise properties the kernels promise, every gradient against float64 autograd, and the encoder through
`SeqEnv`, `user_batch`, `next_item_update` and `ddpg_update`.

Bounds come from the references alone (attn_reference.fp32_bound / grad_bounds); every test prints its measured error next to the
bound before it asserts.  Before a forward comparison the float64 reference is probed: with the mask removed, with the window removed
and with ALiBi flipped it must move by at least 100 bounds, so a kernel that ignores the option cannot pass.

The kernels' tiles are 64 query rows x 64 keys (and 64 rows per linear workgroup), so T runs over 1, 2, 63, 64, 65, 130: both sides of
one tile, and three tiles with a part-filled last one.  window = 5 at T = 130 has key tiles that are fully masked for some rows of a
block but not for the block (window < tile <= T - tile); window = 64 and 70 reach one and two tiles back.  Shapes (E, H, heads):
(8, 16, 1); (24, 48, 3) -- three ALiBi slopes, E's last k block half empty; (72, 64, 2); (128, 256, 4); (128, 256, 16)."""
import copy

import numpy as np
import pytest
import torch

import attn_reference as A
import seq_reference as R
from helpers import csr, make_store

pytestmark = pytest.mark.gpu

SHAPES = ((8, 16, 1), (24, 48, 3), (72, 64, 2), (128, 256, 4), (128, 256, 16))
N_USERS, N_ITEMS, LEN_MIN = 33, 300, 138          # t0 = 7 and T = 130 fit every history
EXTRA_ROWS = 12                                   # table rows past the ids the store can hold: no position reaches them
# (U, T, window, alibi, t0): every U of {1, 16, 17, 33}, every T around the tile edges, every window, ALiBi on and off, t0 0 and 7
FORWARD_CASES = ((17, 1, None, True, 0), (16, 2, None, True, 0), (1, 63, None, True, 0), (33, 64, None, True, 0),
                 (17, 65, None, True, 0), (33, 130, None, True, 0), (16, 130, 1, True, 0), (17, 130, 5, True, 0),
                 (33, 130, 64, True, 0), (1, 130, 70, True, 0), (16, 130, None, False, 0), (17, 65, 5, False, 0),
                 (17, 130, 70, True, 7), (16, 65, None, False, 7))
# (U, T, window, alibi, t0, sparse g_h)
BACKWARD_CASES = ((17, 65, None, True, 0, False), (33, 130, 5, True, 0, True), (16, 64, 64, False, 0, False),
                  (1, 63, None, True, 7, True), (17, 130, 70, False, 7, False))


@pytest.fixture(scope="module")
def seq_data():
    """Per E: 33 users with at least 138 elements and their table, extended by EXTRA_ROWS rows no position holds (CPU)."""
    out = {}
    for E in sorted({s[0] for s in SHAPES}):
        items, ratings, table = make_store(N_USERS, N_ITEMS, E, LEN_MIN, LEN_MIN + 8, seed=E)
        extra = np.random.default_rng(E + 1).standard_normal((EXTRA_ROWS, E)).astype(np.float32)
        out[E] = (items, ratings, torch.from_numpy(np.concatenate([table, extra])))
    return out


@pytest.fixture(scope="module")
def gpu_data(cuda, seq_data):
    from recnn_amd.data.store import ReplayStore
    return {E: (ReplayStore.from_arrays(*csr(items, ratings), cuda), table.to(cuda)) for E, (items, ratings, table) in seq_data.items()}


@pytest.fixture(scope="module")
def references():
    """Float64 / float32 CPU results and bounds, computed once per case and shared (never modified)."""
    return {}


def _enc(shape, window, alibi):
    E, H, heads = shape
    return A.make_encoder(E, H, heads, window, alibi, seed=E + H + heads)


def _inputs(seq_data, E, slots, T, t0=0):
    items, ratings, table = seq_data[E]
    return R.lstm_inputs(table, [items[s] for s in slots], [ratings[s] for s in slots], T, t0)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _forward_reference(references, seq_data, shape, case):
    key = ("fwd", shape, case)
    if key not in references:
        U, T, window, alibi, t0 = case
        enc = _enc(shape, window, alibi)
        x = _inputs(seq_data, shape[0], range(U), T, t0)
        references[key] = (enc, x) + A.fp32_bound(enc, x)
    return references[key]


# ---------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("case", FORWARD_CASES, ids=lambda c: "U%d-T%d-w%s-alibi%d-t0_%d" % c)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "E%d-H%d-heads%d" % s)
def test_forward_against_float64(cuda, seq_data, gpu_data, references, shape, case):
    from recnn_amd.nn import functional as F
    U, T, window, alibi, t0 = case
    enc, x, bound, h64 = _forward_reference(references, seq_data, shape, case)
    # the reference is sensitive to what this case tests
    if T >= 2:
        moved = float((A.attn_cpu(enc, x, causal=False) - h64).abs().max())
        print(f"mask removed: reference moves by {moved:.3e} = {moved / bound:.0f} bounds")
        assert moved >= 100 * bound
    if window is not None and window < T:
        moved = float((A.attn_cpu(enc, x, window=None) - h64).abs().max())
        print(f"window removed: reference moves by {moved:.3e} = {moved / bound:.0f} bounds")
        assert moved >= 100 * bound
    if T >= 2 and window != 1:
        moved = float((A.attn_cpu(enc, x, alibi=not alibi) - h64).abs().max())
        print(f"ALiBi flipped: reference moves by {moved:.3e} = {moved / bound:.0f} bounds")
        assert moved >= 100 * bound
    st, tbl = gpu_data[shape[0]]
    ge = copy.deepcopy(enc).to(cuda)
    h = F.attn_encode(ge, st, tbl, list(range(U)), T, t0=t0)
    assert h.shape == (U, T, shape[1]) and h.dtype == torch.float32 and not h.requires_grad
    err = float((h.cpu().double() - h64).abs().max())
    print(f"attn_encode {shape} {case}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.2f} max|h| {float(h64.abs().max()):.3e}")
    assert err <= bound
    # the training forward: the same bits, with and without the table in the graph; state_encode dispatches here
    ht = F.attn_encode_train(ge, st, tbl, list(range(U)), T, t0=t0)
    assert ht.requires_grad and _same_bits(ht, h)
    assert _same_bits(F.state_encode(ge, st, tbl, list(range(U)), T), h) or t0 != 0
    assert _same_bits(F.attn_encode(ge, st, tbl, list(range(U)), T, t0=t0), h)              # equal calls, equal bits


# ---------------------------------------------------------------------------------------------------- bitwise properties
PROPERTY_SHAPE = (24, 48, 3)


@pytest.mark.parametrize("window", (None, 5, 70))
def test_batch_independence_and_prefix(cuda, seq_data, gpu_data, window):
    from recnn_amd.nn import functional as F
    st, tbl = gpu_data[PROPERTY_SHAPE[0]]
    ge = _enc(PROPERTY_SHAPE, window, True).to(cuda)
    T = 130
    slots = list(range(25))
    h = F.attn_encode(ge, st, tbl, slots, T)
    perm = np.random.default_rng(5).permutation(25)
    assert _same_bits(F.attn_encode(ge, st, tbl, [slots[i] for i in perm], T), h[torch.from_numpy(perm).to(cuda)])
    for u in (0, 16, 24):                                  # alone: the bits it has among 24 others
        assert _same_bits(F.attn_encode(ge, st, tbl, [u], T), h[u:u + 1])
    for a in (1, 63, 64, 65):                              # a prefix of the steps: the first a steps of the longer call
        assert _same_bits(F.attn_encode(ge, st, tbl, slots, a), h[:, :a])
    assert bool(torch.isfinite(h).all()) and float(h.abs().max()) > 0


@pytest.mark.parametrize("window", (None, 5, 64))
def test_causality_and_window_are_bitwise(cuda, seq_data, gpu_data, window):
    """Another item and rating at position j of one user: h_t keeps its bits for t < j and, under a window w, for t >= j + w."""
    from recnn_amd.data.store import ReplayStore
    from recnn_amd.nn import functional as F
    E = PROPERTY_SHAPE[0]
    items, ratings, _ = seq_data[E]
    st, tbl = gpu_data[E]
    ge = _enc(PROPERTY_SHAPE, window, True).to(cuda)
    U, T, u, j = 17, 130, 3, 65                            # j sits inside the second key tile, and j + 64 inside the third
    items2, ratings2 = [i.copy() for i in items], [r.copy() for r in ratings]
    items2[u][j] = (items2[u][j] + 17) % N_ITEMS
    ratings2[u][j] = -ratings2[u][j] if ratings2[u][j] != 0 else 3.0
    st2 = ReplayStore.from_arrays(*csr(items2, ratings2), cuda)
    h = F.attn_encode(ge, st, tbl, list(range(U)), T)
    h2 = F.attn_encode(ge, st2, tbl, list(range(U)), T)
    others = [v for v in range(U) if v != u]
    assert _same_bits(h[others], h2[others])
    assert _same_bits(h[u, :j], h2[u, :j])
    reach = T if window is None else min(T, j + window)
    for t in range(j, reach):                              # every step that attends to j moved
        assert not _same_bits(h[u, t], h2[u, t]), t
    if window is not None:
        assert reach < T and _same_bits(h[u, reach:], h2[u, reach:])


def test_window_one_ignores_queries_and_keys(cuda, seq_data, gpu_data):
    """window = 1: the single unmasked probability is exactly 1, so h does not depend on the q and k rows of W_in and b_in."""
    from recnn_amd.nn import functional as F
    E, H, _ = PROPERTY_SHAPE
    st, tbl = gpu_data[E]
    ge = _enc(PROPERTY_SHAPE, 1, True).to(cuda)
    h = F.attn_encode(ge, st, tbl, list(range(17)), 65)
    with torch.no_grad():
        ge.in_proj_weight[: 2 * H].normal_(0.0, 2.0)
        ge.in_proj_bias[: 2 * H].normal_(0.0, 2.0)
    assert _same_bits(F.attn_encode(ge, st, tbl, list(range(17)), 65), h)
    with torch.no_grad():
        ge.in_proj_weight[2 * H:].mul_(1.5)
    assert not _same_bits(F.attn_encode(ge, st, tbl, list(range(17)), 65), h)


@pytest.mark.parametrize("window", (None, 5))
def test_out_of_table_ids(cuda, seq_data, gpu_data, window):
    """An item id outside the table at position j of one user: the other users keep their bits, that user's h_t is NaN for every
    t >= j that has j in its window, steps whose key tiles do not hold j keep their bits, and in the backward the id reaches no
    table row."""
    from recnn_amd.data.store import ReplayStore
    from recnn_amd.nn import functional as F
    E = PROPERTY_SHAPE[0]
    items, ratings, _ = seq_data[E]
    st, tbl = gpu_data[E]
    U, T, u, j = 17, 130, 5, 70
    for bad in (N_ITEMS + EXTRA_ROWS, -1, 2 ** 31 - 1):
        items2 = [i.copy() for i in items]
        items2[u][j] = bad
        st2 = ReplayStore.from_arrays(*csr(items2, ratings), cuda)
        ge = _enc(PROPERTY_SHAPE, window, True).to(cuda)
        h = F.attn_encode(ge, st, tbl, list(range(U)), T)
        h2 = F.attn_encode(ge, st2, tbl, list(range(U)), T)
        others = [v for v in range(U) if v != u]
        assert _same_bits(h[others], h2[others])
        reach = T if window is None else min(T, j + window)
        assert bool(torch.isnan(h2[u, j:reach]).all())
        assert _same_bits(h[u, :64], h2[u, :64])           # the first block of steps visits the first key tile only: j is not in it
    # backward: the id is in no list of the scatter; rows of items the bad user does not hold stay finite, untouched rows exact zeros
    tb = tbl.detach().clone().requires_grad_(True)
    ht = F.attn_encode_train(ge, st2, tb, list(range(U)), T, train_table=True)
    g = torch.zeros_like(ht)
    g[others] = 1.0
    ht.backward(g)
    assert tb.grad.shape == tb.shape and not tb.grad[N_ITEMS:].any()
    held_by_bad = set(int(i) for i in items2[u][:T])
    clean = [i for i in range(N_ITEMS) if i not in held_by_bad]
    assert len(clean) > 50 and bool(torch.isfinite(tb.grad[clean]).all()) and float(tb.grad[clean].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- backward
def _backward_reference(references, seq_data, shape, case):
    key = ("bwd", shape, case)
    if key not in references:
        U, T, window, alibi, t0, sparse = case
        enc = _enc(shape, window, alibi)
        items, ratings, table = seq_data[shape[0]]
        idx, rts = A.positions(items[:U], ratings[:U], T, t0)
        rows = [(u, t) for u in range(0, U, 3) for t in sorted({0, T // 2, T - 1})] if sparse else None
        g_h = A.loss_weights(U, T, shape[1], seed=U + T, rows=rows)
        references[key] = (enc, g_h, idx) + A.grad_bounds(enc, table, idx, rts, g_h)
    return references[key]


def _gpu_grads(cuda, ge, st, tb, U, T, t0, g_h, train_table):
    from recnn_amd.nn import functional as F
    ge.zero_grad(set_to_none=True)
    tb.grad = None
    h = F.attn_encode_train(ge, st, tb, list(range(U)), T, t0=t0, train_table=train_table)
    h.backward(g_h.to(cuda, torch.float32))
    out = {n: p.grad for n, p in ge.named_parameters() if p.grad is not None}
    if tb.grad is not None:
        out["table"] = tb.grad
    return out


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=lambda c: "U%d-T%d-w%s-alibi%d-t0_%d-sparse%d" % c)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "E%d-H%d-heads%d" % s)
def test_gradients_against_float64(cuda, seq_data, gpu_data, references, shape, case):
    U, T, window, alibi, t0, sparse = case
    enc, g_h, idx, bounds, g64 = _backward_reference(references, seq_data, shape, case)
    st, tbl = gpu_data[shape[0]]
    ge = copy.deepcopy(enc).to(cuda)
    tb = tbl.detach().clone().requires_grad_(True)
    got = _gpu_grads(cuda, ge, st, tb, U, T, t0, g_h, True)
    assert set(got) == set(g64)
    worst = []
    for n in g64:
        top = float(g64[n].abs().max())
        err = float((got[n].cpu().double() - g64[n]).abs().max())
        print(f"attn backward {shape} {case} {n}: err {err:.3e} bound {bounds[n]:.3e} ratio {err / bounds[n]:.2f} max|G| {top:.3e}")
        assert top >= 100 * bounds[n], (n, top, bounds[n])            # the comparison means something
        if not err <= bounds[n]:
            worst.append((n, err, bounds[n]))
    assert not worst, worst
    # the table gradient: exact zeros where no position holds the item; an item held at several positions of several users
    held = torch.zeros(tb.shape[0], dtype=torch.bool)
    held[idx.reshape(-1)] = True
    assert not held[N_ITEMS:].any() and not got["table"].cpu()[~held].any()
    if U > 1:
        counts = [(int((idx == i).sum()), int((idx == i).any(1).sum()), i) for i in idx.reshape(-1).unique().tolist()]
        shared = [c for c in counts if c[0] >= 2 and c[1] >= 2]
        assert shared
        n_pos, n_users, hot = max(shared, key=lambda c: float(g64["table"][c[2]].abs().max()))    # the one the loss reaches most
        err = float((got["table"][hot].cpu().double() - g64["table"][hot]).abs().max())
        print(f"item {hot} held at {n_pos} positions of {n_users} users: err {err:.3e} bound {bounds['table']:.3e}")
        assert err <= bounds["table"] and float(g64["table"][hot].abs().max()) > 0
    # without the table: recnn_attn_backward gives the bits recnn_attn_backward_table gives in the outputs they share; equal calls too
    tb2 = tbl.detach().clone()
    plain = _gpu_grads(cuda, ge, st, tb2, U, T, t0, g_h, False)
    assert set(plain) == set(A.PARAMS) and all(_same_bits(plain[n], got[n]) for n in A.PARAMS)
    again = _gpu_grads(cuda, ge, st, tb, U, T, t0, g_h, True)
    assert all(_same_bits(again[n], got[n]) for n in got)


def test_null_outputs_are_skipped(cuda, seq_data, gpu_data, references):
    """A frozen parameter's gradient is passed as NULL: it stays None, and the others keep their bits."""
    shape, case = (24, 48, 3), BACKWARD_CASES[0]
    U, T, window, alibi, t0, _ = case
    enc, g_h, _, _, _ = _backward_reference(references, seq_data, shape, case)
    st, tbl = gpu_data[shape[0]]
    ge = copy.deepcopy(enc).to(cuda)
    tb = tbl.detach().clone().requires_grad_(True)
    full = _gpu_grads(cuda, ge, st, tb, U, T, t0, g_h, True)
    params = dict(ge.named_parameters())
    for frozen in (("in_proj_weight",), ("in_proj_bias",), ("out_proj.weight",), ("out_proj.bias",),
                   ("in_proj_weight", "in_proj_bias"), A.PARAMS):
        for n, p in params.items():
            p.requires_grad_(n not in frozen)
        got = _gpu_grads(cuda, ge, st, tb, U, T, t0, g_h, True)
        assert set(got) == set(full) - set(frozen), frozen
        assert all(_same_bits(got[n], full[n]) for n in got), frozen
    for n, p in params.items():
        p.requires_grad_(n == "out_proj.bias")
    got = _gpu_grads(cuda, ge, st, tbl.detach().clone(), U, T, t0, g_h, False)                 # no attention backward at all
    assert set(got) == {"out_proj.bias"} and _same_bits(got["out_proj.bias"], full["out_proj.bias"])


# ---------------------------------------------------------------------------------------------------- through the stack
def _env_data(E=8):
    """seq_env_data's 12 users and table with an AttentionEncoder(E + 1, 16, 1) as the encoder."""
    table, user_dict, users, _ = R.seq_env_data(E=E)
    return table, user_dict, users, A.make_encoder(E, 16, 1, None, True, seed=0)


def _env(cuda, table, user_dict, users, enc, batch_size=5):
    from recnn_amd.data.env import SeqEnv
    return SeqEnv.from_user_dict(table, user_dict, users, state_encoder=copy.deepcopy(enc).to(cuda), batch_size=batch_size,
                                 max_buf_size=4 * batch_size, device=cuda)


def _env_batches(table, user_dict, users, enc, batch_size, max_buf_size, n_batches):
    """seq_reference.seq_env_batches -- that loop, not a copy of it -- with the attention layer as the encoder: the loop reaches its
    encoder only through the module-level `fp32_bound`, swapped for the duration of the call."""
    def bound_of(e, x, h0c0=None):
        b, h = A.fp32_bound(e, x)
        return [b, b, b], (h, None, None)

    keep = R.fp32_bound
    R.fp32_bound = bound_of
    try:
        return R.seq_env_batches(table, user_dict, users, enc, batch_size, max_buf_size, n_batches)
    finally:
        R.fp32_bound = keep


def test_seq_env_generator_matches_the_reference_loop(cuda):
    table, user_dict, users, enc = _env_data()
    np.random.seed(R.SEQ_ENV_SEED)
    ref, bound = _env_batches(table, user_dict, users, enc, 5, 20, 3)
    env = _env(cuda, table, user_dict, users, enc)
    assert [tuple(s) for s in env.buffer_layout] == [(20, 16), (20, 8), (20, 1), (20, 16)]
    np.random.seed(R.SEQ_ENV_SEED)
    gen = env.train_batch()
    compared = []
    for k, want in enumerate(ref):
        got = next(gen)
        m = got["meta"]
        assert m["step"] == want["meta"]["step"] and m["rows"] == want["meta"]["rows"] and list(m["users"]) == want["meta"]["users"]
        assert torch.equal(got["action"].cpu(), torch.from_numpy(want["action"]))
        assert torch.equal(got["reward"].cpu(), torch.from_numpy(want["reward"]))
        for key in ("state", "next_state"):
            err = float((got[key].cpu().double() - torch.from_numpy(want[key])).abs().max())
            print(f"SeqEnv (attention) batch {k} {key}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound
            assert got[key][:m["rows"]].abs().max() > 0 and not got[key][m["rows"]:].any()
        compared.append(m["rows"])
    assert compared == [20, 17, 20]                                   # an empty comparison must not pass


IDS, STEPS = [0, 1, 2, 3, 4], [3, 4, 9, 30]


def test_user_batch_gradients_reach_the_encoder_and_the_table(cuda):
    table, user_dict, users, enc = _env_data()
    env = _env(cuda, table, user_dict, users, enc)
    U, T, H = len(IDS), STEPS[-1] + 1, 16
    P = env.table.detach().clone().requires_grad_(True)
    batch = env.user_batch(IDS, STEPS, table=P)
    assert batch["state"].requires_grad and batch["next_state"].requires_grad and batch["state"].shape == (20, H)
    gen = torch.Generator().manual_seed(4)
    c_state, c_next = torch.randn(20, H, generator=gen, dtype=torch.float64), torch.randn(20, H, generator=gen, dtype=torch.float64)
    ((batch["state"] * c_state.to(cuda, torch.float32)).sum() + (batch["next_state"] * c_next.to(cuda, torch.float32)).sum()).backward()
    # rows k U + u: next_state is h[u, steps[k]], state h[u, steps[k] - 1]
    g_h = torch.zeros(U, T, H, dtype=torch.float64)
    for k, t in enumerate(STEPS):
        g_h[:, t] += c_next[k * U:(k + 1) * U]
        g_h[:, t - 1] += c_state[k * U:(k + 1) * U]
    idx, rts = A.positions([user_dict[u]["items"] for u in IDS], [user_dict[u]["ratings"] for u in IDS], T)
    bounds, g64 = A.grad_bounds(enc, table, idx, rts, g_h)
    got = {n: p.grad.cpu() for n, p in env.state_encoder.named_parameters()}
    got["table"] = P.grad.cpu()
    for n in g64:
        err = float((got[n].double() - g64[n]).abs().max())
        print(f"user_batch {n}: err {err:.3e} bound {bounds[n]:.3e} max|G| {float(g64[n].abs().max()):.3e}")
        assert err <= bounds[n] and float(g64[n].abs().max()) >= 100 * bounds[n]


def test_next_item_update_and_ddpg_update_train_the_encoder(cuda):
    import recnn_amd
    table, user_dict, users, enc = _env_data(E=16)
    env = _env(cuda, table, user_dict, users, enc)
    U, T = len(IDS), STEPS[-1] + 1
    P = env.table.detach().clone().requires_grad_(True)
    head = recnn_amd.nn.NextItemHead(P)
    batch = env.user_batch(IDS, STEPS, table=P)
    batch["target"] = env.target_items(batch)
    loss = float(recnn_amd.nn.next_item_update(batch, {}, {"head": head}, None, learn=False)["loss"])
    # the reference: float64 states, the full softmax over the table's rows, the mean over the 20 rows
    x = R.lstm_inputs(table, [user_dict[u]["items"] for u in IDS], [user_dict[u]["ratings"] for u in IDS], T)
    bound_h, h64 = A.fp32_bound(enc, x)
    state = torch.cat([h64[:, t - 1] for t in STEPS])
    target = torch.cat([torch.as_tensor([int(user_dict[u]["items"][t]) for u in IDS]) for t in STEPS])
    assert torch.equal(batch["target"].cpu(), target)
    want = float(torch.nn.functional.cross_entropy(state @ table.double().T, target))
    # a logit moves by at most max_i |P_i|_1 bound_h, the cross-entropy of a row by at most twice that; the fp32 head adds a few ulp
    bound = 2.0 * float(table.double().abs().sum(1).max()) * bound_h + 16 * 2.0 ** -24 * max(1.0, abs(want))
    print(f"next_item_update(learn=False): loss {loss:.8f} reference {want:.8f} err {abs(loss - want):.3e} bound {bound:.3e}")
    assert abs(loss - want) <= bound
    # one learning step moves the in-projection
    ge = env.state_encoder
    opt = torch.optim.SGD([P] + list(ge.parameters()), lr=0.1)
    before = ge.in_proj_weight.detach().clone()
    out = recnn_amd.nn.next_item_update(batch, {}, {"head": head}, {"optimizer": opt}, learn=True, step=0)
    assert np.isfinite(float(out["loss"])) and not torch.equal(ge.in_proj_weight.detach(), before)

    # ddpg_update on an attached batch leaves a finite, non-zero gradient in the in-projection
    from recnn_amd.nn import fused
    keep = dict(fused.DEFAULTS)
    fused.set_defaults(dtype="fp32", mask_mode="none", seed=11)
    try:
        torch.manual_seed(3)
        pol = recnn_amd.nn.Actor(16, 16, 32, 6e-1)
        val = recnn_amd.nn.Critic(16, 16, 32, 54e-2)
        nets = {"policy_net": pol, "target_policy_net": copy.deepcopy(pol), "value_net": val, "target_value_net": copy.deepcopy(val)}
        nets = {k: v.to(cuda).eval() for k, v in nets.items()}
        optimizer = {"policy_optimizer": torch.optim.SGD(list(nets["policy_net"].parameters()) + list(ge.parameters()), lr=1e-3),
                     "value_optimizer": torch.optim.SGD(nets["value_net"].parameters(), lr=1e-2)}
        ge.zero_grad(set_to_none=True)
        batch = env.user_batch(IDS, STEPS)
        params = {"gamma": 0.99, "min_value": -10, "max_value": 10, "policy_step": 2, "soft_tau": 0.01}
        losses = recnn_amd.nn.update.ddpg_update(batch, params, nets, optimizer, learn=True, step=1)
        g = ge.in_proj_weight.grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        assert all(np.isfinite(float(v)) for v in losses.values())
    finally:
        fused.set_defaults(**keep)
