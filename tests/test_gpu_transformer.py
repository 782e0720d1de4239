"""The transformer state encoder on the GPU (csrc/block.hip): `transformer_encode` / `transformer_encode_train` against the float64
model of tests/transformer_reference.py, the bitwise properties the kernels promise, every gradient against float64 autograd, and the
encoder through `SeqEnv`, `user_batch`, `next_item_update` and `ddpg_update`.

Bounds come from the references alone (transformer_reference.fp32_bound / grad_bounds); every test prints its measured error next to
the bound before it asserts.  Before a forward comparison the float64 reference is probed: with the LayerNorms replaced by identity,
the feed-forward removed, the residuals removed, the activation swapped and the mask removed it must move by at least 100 bounds, so
a kernel that ignores a piece cannot pass.

The kernels work on 64 rows per workgroup and 64 keys per tile, so T runs over 1, 2, 63, 64, 65, 130 and U over 1, 16, 17, 33.  The
feed-forward walks F in chunks of 32: F = 16 is less than a chunk, 80 two chunks and a half, 256 and 1024 whole chunks.  The linear
kernel stages at most 256 contraction columns at a time: the backward's products over F = 1024 and 3 H = 768 take the K-blocked walk,
those at H <= 64 the single stage.  Shapes (E, H, heads, F, L)."""
import copy

import numpy as np
import pytest
import torch

import attn_reference as A
import seq_reference as R
import transformer_reference as TR
from helpers import csr, make_store

pytestmark = pytest.mark.gpu

SHAPES = ((8, 16, 1, 16, 1), (24, 48, 3, 80, 2), (72, 64, 2, 256, 2), (128, 256, 4, 256, 2), (128, 256, 16, 1024, 3))
N_USERS, N_ITEMS, LEN_MIN = 33, 300, 138          # t0 = 7 and T = 130 fit every history
EXTRA_ROWS = 12                                   # table rows past the ids the store can hold: no position reaches them
# (U, T, window, alibi, t0): every U of {1, 16, 17, 33}, every T around the tile edges, every window, ALiBi on and off, t0 0 and 7
FORWARD_CASES = ((17, 1, None, True, 0), (16, 2, None, True, 0), (1, 63, None, True, 0), (33, 64, None, True, 0),
                 (17, 65, None, True, 0), (33, 130, None, True, 0), (16, 130, 1, True, 0), (17, 130, 5, True, 0),
                 (1, 130, 70, True, 0), (16, 130, None, False, 0), (17, 65, 5, False, 0), (17, 130, 70, True, 7),
                 (16, 65, None, False, 7))
# the two H = 256 shapes run the cases that differ in a tile edge, a window or t0, not the whole list (their references are the slow part)
LARGE_CASES = ((17, 1, None, True, 0), (1, 63, None, True, 0), (33, 64, None, True, 0), (17, 65, 5, False, 0), (33, 130, None, True, 0),
               (16, 130, 1, True, 0), (17, 130, 70, True, 7))
FORWARD = [(s, c, ("relu", "gelu")[(i + j) % 2]) for i, s in enumerate(SHAPES)
           for j, c in enumerate(FORWARD_CASES if s[1] < 256 else LARGE_CASES)]
# (U, T, window, alibi, t0, sparse g_h)
BACKWARD_CASES = ((17, 65, None, True, 0, False), (33, 130, 5, True, 0, True), (16, 64, 70, False, 0, False),
                  (1, 63, None, True, 7, True))
BACKWARD = [(s, c) for s in SHAPES for c in (BACKWARD_CASES if s[1] < 256 else BACKWARD_CASES[:2])]


def _fwd_id(p):
    s, c, act = p
    return "E%d-H%d-heads%d-F%d-L%d-" % s + "U%d-T%d-w%s-alibi%d-t0_%d-" % c + act


def _bwd_id(p):
    s, c = p
    return "E%d-H%d-heads%d-F%d-L%d-" % s + "U%d-T%d-w%s-alibi%d-t0_%d-sparse%d" % c


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


def _enc(shape, act, window, alibi, seed=None):
    E, H, heads, F, L = shape
    return TR.make_encoder(E, H, heads, F, L, act, window, alibi, seed=E + H + heads + F if seed is None else seed)


def _inputs(seq_data, E, slots, T, t0=0):
    items, ratings, table = seq_data[E]
    return R.lstm_inputs(table, [items[s] for s in slots], [ratings[s] for s in slots], T, t0)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------- forward
def forward_reference(seq_data, shape, case, act):
    """(enc, bound, h64, {probe: how far the float64 reference moves}) -- everything of a forward case that needs no GPU."""
    U, T, window, alibi, t0 = case
    enc = _enc(shape, act, window, alibi)
    x = _inputs(seq_data, shape[0], range(U), T, t0)
    bound, h64 = TR.fp32_bound(enc, x)
    probes = {"LayerNorms replaced by identity": dict(norms=False), "feed-forward removed": dict(ffn=False),
              "residuals removed": dict(residual=False), "activation swapped": dict(act="gelu" if act == "relu" else "relu")}
    if T >= 2:
        probes["mask removed"] = dict(causal=False)
    moved = {n: float((TR.model_cpu(enc, x, **kw) - h64).abs().max()) for n, kw in probes.items()}
    return enc, bound, h64, moved


@pytest.mark.parametrize("param", FORWARD, ids=_fwd_id)
def test_forward_against_float64(cuda, seq_data, gpu_data, param):
    from recnn_amd.nn import functional as F
    shape, case, act = param
    U, T, window, alibi, t0 = case
    enc, bound, h64, moved = forward_reference(seq_data, shape, case, act)
    for n, m in moved.items():
        print(f"{n}: reference moves by {m:.3e} = {m / bound:.0f} bounds")
        assert m >= 100 * bound, n
    st, tbl = gpu_data[shape[0]]
    ge = copy.deepcopy(enc).to(cuda)
    h = F.transformer_encode(ge, st, tbl, list(range(U)), T, t0=t0)
    assert h.shape == (U, T, shape[1]) and h.dtype == torch.float32 and not h.requires_grad
    err = float((h.cpu().double() - h64).abs().max())
    print(f"transformer_encode {shape} {case} {act}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.2f} "
          f"max|h| {float(h64.abs().max()):.3e}")
    assert err <= bound
    # the training forward: the same bits; state_encode dispatches here; equal calls, equal bits
    ht = F.transformer_encode_train(ge, st, tbl, list(range(U)), T, t0=t0)
    assert ht.requires_grad and _same_bits(ht, h)
    assert _same_bits(F.state_encode(ge, st, tbl, list(range(U)), T), h) or t0 != 0
    assert _same_bits(F.transformer_encode(ge, st, tbl, list(range(U)), T, t0=t0), h)
    with torch.no_grad():
        assert not F.transformer_encode_train(ge, st, tbl, list(range(U)), T, t0=t0).requires_grad


# ---------------------------------------------------------------------------------------------------- bitwise properties
PROPERTY_SHAPE = (24, 48, 3, 80, 2)


@pytest.mark.parametrize("window", (None, 5, 70))
def test_batch_independence_and_prefix(cuda, seq_data, gpu_data, window):
    from recnn_amd.nn import functional as F
    st, tbl = gpu_data[PROPERTY_SHAPE[0]]
    ge = _enc(PROPERTY_SHAPE, "gelu", window, True).to(cuda)
    T = 130
    slots = list(range(25))
    h = F.transformer_encode(ge, st, tbl, slots, T)
    perm = np.random.default_rng(5).permutation(25)
    assert _same_bits(F.transformer_encode(ge, st, tbl, [slots[i] for i in perm], T), h[torch.from_numpy(perm).to(cuda)])
    for u in (0, 16, 24):                                  # alone: the bits it has among 24 others
        assert _same_bits(F.transformer_encode(ge, st, tbl, [u], T), h[u:u + 1])
    for a in (1, 63, 64, 65):                              # a prefix of the steps: the first a steps of the longer call
        assert _same_bits(F.transformer_encode(ge, st, tbl, slots, a), h[:, :a])
    assert bool(torch.isfinite(h).all()) and float(h.abs().max()) > 0


@pytest.mark.parametrize("window", (None, 5, 70))
def test_causality_through_the_stack_is_bitwise(cuda, seq_data, gpu_data, window):
    """Another item and rating at position j of one user: h_t keeps its bits for t < j and, under a window w, for
    t >= j + L (w - 1) + 1 -- the receptive field of L layers is L (w - 1) + 1 steps."""
    from recnn_amd.data.store import ReplayStore
    from recnn_amd.nn import functional as F
    E, L = PROPERTY_SHAPE[0], PROPERTY_SHAPE[4]
    items, ratings, _ = seq_data[E]
    st, tbl = gpu_data[E]
    ge = _enc(PROPERTY_SHAPE, "relu", window, True).to(cuda)
    U, T, u, j = 17, 130, 3, 65 if window != 70 else 2     # window 70: j + 2 * 69 + 1 = 141 is past the call, every later step is reached
    items2, ratings2 = [i.copy() for i in items], [r.copy() for r in ratings]
    items2[u][j] = (items2[u][j] + 17) % N_ITEMS
    ratings2[u][j] = -ratings2[u][j] if ratings2[u][j] != 0 else 3.0
    st2 = ReplayStore.from_arrays(*csr(items2, ratings2), cuda)
    h = F.transformer_encode(ge, st, tbl, list(range(U)), T)
    h2 = F.transformer_encode(ge, st2, tbl, list(range(U)), T)
    others = [v for v in range(U) if v != u]
    assert _same_bits(h[others], h2[others])
    assert _same_bits(h[u, :j], h2[u, :j])
    reach = T if window is None else min(T, j + L * (window - 1) + 1)
    for t in range(j, reach):                              # every step inside the receptive field moved
        assert not _same_bits(h[u, t], h2[u, t]), t
    if window == 5:
        assert reach == j + 9 < T and _same_bits(h[u, reach:], h2[u, reach:])


@pytest.mark.parametrize("window", (None, 5, 70))
def test_out_of_table_ids(cuda, seq_data, gpu_data, window):
    """An item id outside the table at position j of one user: the other users keep their bits, that user's rows are NaN from j on
    (under a window w: as far as L layers reach, L (w - 1) + 1 steps), the steps of the first block (whose key tile does not hold j)
    keep their bits, and in the backward the id reaches no table row."""
    from recnn_amd.data.store import ReplayStore
    from recnn_amd.nn import functional as F
    E, L = PROPERTY_SHAPE[0], PROPERTY_SHAPE[4]
    items, ratings, _ = seq_data[E]
    st, tbl = gpu_data[E]
    U, T, u, j = 17, 130, 5, 70
    others = [v for v in range(U) if v != u]
    ge = _enc(PROPERTY_SHAPE, "gelu", window, True).to(cuda)
    h = F.transformer_encode(ge, st, tbl, list(range(U)), T)
    reach = T if window is None else min(T, j + L * (window - 1) + 1)
    for bad in (N_ITEMS + EXTRA_ROWS, -1, 2 ** 31 - 1):
        items2 = [i.copy() for i in items]
        items2[u][j] = bad
        st2 = ReplayStore.from_arrays(*csr(items2, ratings), cuda)
        h2 = F.transformer_encode(ge, st2, tbl, list(range(U)), T)
        assert _same_bits(h[others], h2[others])
        assert bool(torch.isnan(h2[u, j:reach]).all())
        assert _same_bits(h[u, :64], h2[u, :64])
    tb = tbl.detach().clone().requires_grad_(True)
    ht = F.transformer_encode_train(ge, st2, tb, list(range(U)), T, train_table=True)
    g = torch.zeros_like(ht)
    g[others] = 1.0
    ht.backward(g)
    assert tb.grad.shape == tb.shape and not tb.grad[N_ITEMS:].any()
    held_by_bad = set(int(i) for i in items2[u][:T])
    clean = [i for i in range(N_ITEMS) if i not in held_by_bad]
    assert len(clean) > 50 and bool(torch.isfinite(tb.grad[clean]).all()) and float(tb.grad[clean].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- backward
def backward_reference(seq_data, shape, case, act, seed=None):
    """(enc, g_h, idx, bounds, g64) -- everything of a gradient case that needs no GPU."""
    U, T, window, alibi, t0, sparse = case
    enc = _enc(shape, act, window, alibi, seed)
    items, ratings, table = seq_data[shape[0]]
    idx, rts = A.positions(items[:U], ratings[:U], T, t0)
    rows = [(u, t) for u in range(0, U, 3) for t in sorted({0, T // 2, T - 1})] if sparse else None
    g_h = A.loss_weights(U, T, shape[1], seed=U + T, rows=rows)
    return (enc, g_h, idx) + TR.grad_bounds(enc, table, idx, rts, g_h)


def _gpu_grads(cuda, ge, st, tb, U, T, t0, g_h, train_table):
    from recnn_amd.nn import functional as F
    ge.zero_grad(set_to_none=True)
    tb.grad = None
    h = F.transformer_encode_train(ge, st, tb, list(range(U)), T, t0=t0, train_table=train_table)
    h.backward(g_h.to(cuda, torch.float32))
    out = {n: p.grad for n, p in ge.named_parameters() if p.grad is not None}
    if tb.grad is not None:
        out["table"] = tb.grad
    return out


def _check_gradients(cuda, gpu_data, shape, case, ref, label):
    U, T, window, alibi, t0, sparse = case
    enc, g_h, idx, bounds, g64 = ref
    st, tbl = gpu_data[shape[0]]
    ge = copy.deepcopy(enc).to(cuda)
    tb = tbl.detach().clone().requires_grad_(True)
    got = _gpu_grads(cuda, ge, st, tb, U, T, t0, g_h, True)
    assert set(got) == set(g64)
    worst = []
    for n in g64:
        top = float(g64[n].abs().max())
        err = float((got[n].cpu().double() - g64[n]).abs().max())
        print(f"{label} {shape} {case} {n}: err {err:.3e} bound {bounds[n]:.3e} ratio {err / bounds[n]:.2f} max|G| {top:.3e}")
        assert top >= 100 * bounds[n], (n, top, bounds[n])            # the comparison means something
        if not err <= bounds[n]:
            worst.append((n, err, bounds[n]))
    assert not worst, worst
    # the table gradient: exact zeros where no position holds the item
    held = torch.zeros(tb.shape[0], dtype=torch.bool)
    held[idx.reshape(-1)] = True
    assert not held[N_ITEMS:].any() and not got["table"].cpu()[~held].any()
    # without the table: the same bits in the outputs the two calls share; equal calls too
    plain = _gpu_grads(cuda, ge, st, tbl.detach().clone(), U, T, t0, g_h, False)
    assert set(plain) == set(g64) - {"table"} and all(_same_bits(plain[n], got[n]) for n in plain)
    again = _gpu_grads(cuda, ge, st, tb, U, T, t0, g_h, True)
    assert all(_same_bits(again[n], got[n]) for n in got)


@pytest.mark.parametrize("param", BACKWARD, ids=_bwd_id)
def test_gelu_gradients_against_float64(cuda, seq_data, gpu_data, param):
    shape, case = param
    _check_gradients(cuda, gpu_data, shape, case, backward_reference(seq_data, shape, case, "gelu"), "gelu backward")


RELU_SHAPE, RELU_CASES = (8, 16, 1, 16, 2), ((3, 65, None, True, 0, False), (3, 65, 5, False, 0, True))
RELU_MARGIN = 1e-4


def relu_seed(seq_data, case):
    """The first seed >= 0 whose float64 reference keeps every pre-activation of both blocks at least RELU_MARGIN from relu's kink:
    nearer than rounding, the mask of fp32 and of float64 differ and a weight gradient moves by O(1), which says nothing about a kernel."""
    U, T, window, alibi, t0, _ = case
    x = _inputs(seq_data, RELU_SHAPE[0], range(U), T, t0)
    for seed in range(64):
        margin = TR.smallest_preactivation(_enc(RELU_SHAPE, "relu", window, alibi, seed), x)
        if margin >= RELU_MARGIN:
            return seed, margin
    raise AssertionError("no seed below 64 keeps relu's kink clear")


@pytest.mark.parametrize("case", RELU_CASES, ids=lambda c: "U%d-T%d-w%s-alibi%d-t0_%d-sparse%d" % c)
def test_relu_gradients_against_float64(cuda, seq_data, gpu_data, case):
    seed, margin = relu_seed(seq_data, case)
    print(f"relu gradients: seed {seed}, smallest |a_1| of the float64 reference {margin:.3e}")
    assert margin >= RELU_MARGIN
    _check_gradients(cuda, gpu_data, RELU_SHAPE, case, backward_reference(seq_data, RELU_SHAPE, case, "relu", seed), "relu backward")


def test_null_outputs_are_skipped(cuda, seq_data, gpu_data):
    """A frozen parameter's gradient is passed as NULL: it stays None, and the others keep their bits."""
    shape, case = PROPERTY_SHAPE, BACKWARD_CASES[0]
    U, T, window, alibi, t0, _ = case
    enc = _enc(shape, "gelu", window, alibi)
    g_h = A.loss_weights(U, T, shape[1], seed=3)
    st, tbl = gpu_data[shape[0]]
    ge = copy.deepcopy(enc).to(cuda)
    tb = tbl.detach().clone().requires_grad_(True)
    full = _gpu_grads(cuda, ge, st, tb, U, T, t0, g_h, True)
    params = dict(ge.named_parameters())
    assert set(full) == set(params) | {"table"}
    names = list(params)
    block0 = [n for n in names if n.startswith("layers.0.")]
    for frozen in ([n] for n in names if n.startswith("layers.1.") or n.startswith("norm.") or n.startswith("embed.")):
        for n, p in params.items():
            p.requires_grad_(n not in frozen)
        got = _gpu_grads(cuda, ge, st, tb, U, T, t0, g_h, True)
        assert set(got) == set(full) - set(frozen), frozen
        assert all(_same_bits(got[n], full[n]) for n in got), frozen
    for frozen in (block0, ["embed.weight", "embed.bias"] + block0, [n for n in names if "linear" in n], [n for n in names if "norm" in n],
                   names):
        for n, p in params.items():
            p.requires_grad_(n not in frozen)
        got = _gpu_grads(cuda, ge, st, tb, U, T, t0, g_h, True)
        assert set(got) == set(full) - set(frozen), frozen
        assert all(_same_bits(got[n], full[n]) for n in got), frozen
    # without the table and with everything below frozen nothing below the one live tensor is launched
    for live in ("norm.bias", "layers.1.linear2.bias", "layers.1.self_attn.out_proj.weight", "layers.0.norm1.weight"):
        for n, p in params.items():
            p.requires_grad_(n == live)
        got = _gpu_grads(cuda, ge, st, tbl.detach().clone(), U, T, t0, g_h, False)
        assert set(got) == {live} and _same_bits(got[live], full[live]), live


# ---------------------------------------------------------------------------------------------------- through the stack
def _env_data(E=8, act="gelu"):
    """seq_env_data's 12 users and table with a TransformerStateEncoder(E + 1, 16, 1, num_layers=2) as the encoder."""
    table, user_dict, users, _ = R.seq_env_data(E=E)
    return table, user_dict, users, TR.make_encoder(E, 16, 1, 16, 2, act, None, True, seed=0)


def _env(cuda, table, user_dict, users, enc, batch_size=5):
    from recnn_amd.data.env import SeqEnv
    return SeqEnv.from_user_dict(table, user_dict, users, state_encoder=copy.deepcopy(enc).to(cuda), batch_size=batch_size,
                                 max_buf_size=4 * batch_size, device=cuda)


def _env_batches(table, user_dict, users, enc, batch_size, max_buf_size, n_batches):
    """seq_reference.seq_env_batches -- that loop, not a copy of it -- with the transformer as the encoder: the loop reaches its
    encoder only through the module-level `fp32_bound`, swapped for the duration of the call."""
    def bound_of(e, x, h0c0=None):
        b, h = TR.fp32_bound(e, x)
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
            print(f"SeqEnv (transformer) batch {k} {key}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound
            assert got[key][:m["rows"]].abs().max() > 0 and not got[key][m["rows"]:].any()
        compared.append(m["rows"])
    assert compared == [20, 17, 20]                                   # an empty comparison must not pass


IDS, STEPS = [0, 1, 2, 3, 4], [3, 4, 9, 30]


def test_user_batch_gradients_reach_every_parameter_and_the_table(cuda):
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
    bounds, g64 = TR.grad_bounds(enc, table, idx, rts, g_h)
    got = {n: p.grad.cpu() for n, p in env.state_encoder.named_parameters()}
    got["table"] = P.grad.cpu()
    assert set(got) == set(g64)
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
    bound_h, h64 = TR.fp32_bound(enc, x)
    state = torch.cat([h64[:, t - 1] for t in STEPS])
    target = torch.cat([torch.as_tensor([int(user_dict[u]["items"][t]) for u in IDS]) for t in STEPS])
    assert torch.equal(batch["target"].cpu(), target)
    want = float(torch.nn.functional.cross_entropy(state @ table.double().T, target))
    # a logit moves by at most max_i |P_i|_1 bound_h, the cross-entropy of a row by at most twice that; the fp32 head adds a few ulp
    bound = 2.0 * float(table.double().abs().sum(1).max()) * bound_h + 16 * 2.0 ** -24 * max(1.0, abs(want))
    print(f"next_item_update(learn=False): loss {loss:.8f} reference {want:.8f} err {abs(loss - want):.3e} bound {bound:.3e}")
    assert abs(loss - want) <= bound
    # one learning step moves every parameter of the encoder
    ge = env.state_encoder
    opt = torch.optim.SGD([P] + list(ge.parameters()), lr=0.1)
    before = {n: p.detach().clone() for n, p in ge.named_parameters()}
    out = recnn_amd.nn.next_item_update(batch, {}, {"head": head}, {"optimizer": opt}, learn=True, step=0)
    assert np.isfinite(float(out["loss"]))
    still = [n for n, p in ge.named_parameters() if torch.equal(p.detach(), before[n])]
    assert not still, still

    # one ddpg_update policy step on an attached batch moves every parameter of the encoder too
    from recnn_amd.nn import fused
    keep = dict(fused.DEFAULTS)
    fused.set_defaults(dtype="fp32", mask_mode="none", seed=11)
    try:
        torch.manual_seed(3)
        pol = recnn_amd.nn.Actor(16, 16, 32, 6e-1)
        val = recnn_amd.nn.Critic(16, 16, 32, 54e-2)
        nets = {"policy_net": pol, "target_policy_net": copy.deepcopy(pol), "value_net": val, "target_value_net": copy.deepcopy(val)}
        nets = {k: v.to(cuda).eval() for k, v in nets.items()}
        optimizer = {"policy_optimizer": torch.optim.SGD(list(nets["policy_net"].parameters()) + list(ge.parameters()), lr=1e-1),
                     "value_optimizer": torch.optim.SGD(nets["value_net"].parameters(), lr=1e-2)}
        ge.zero_grad(set_to_none=True)
        before = {n: p.detach().clone() for n, p in ge.named_parameters()}
        batch = env.user_batch(IDS, STEPS)
        params = {"gamma": 0.99, "min_value": -10, "max_value": 10, "policy_step": 2, "soft_tau": 0.01}
        losses = recnn_amd.nn.update.ddpg_update(batch, params, nets, optimizer, learn=True, step=0)
        assert all(np.isfinite(float(v)) for v in losses.values())
        for n, p in ge.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
        still = [n for n, p in ge.named_parameters() if torch.equal(p.detach(), before[n])]
        assert not still, still
    finally:
        fused.set_defaults(**keep)
