"""The lattice of tests/mlp_exact_reference.py does what tests/test_gpu_frozen_exact.py relies on, checked without a GPU:

  * every case is ADMISSIBLE: each element of h1, h2 and out equals its bf16 rounding and every span stays below SPAN_LIMIT -- the share
    of inadmissible elements allowed is zero.  Hash masks exist only on the GPU, so a masked case is checked under the all-kept mask
    and under a random 0/1 mask (the GPU test repeats the check with the masks the kernel really draws);
  * every 64-wide slab of every contraction is populated, and zeroing any ONE of them changes the reference: a kernel that drops,
    repeats or misplaces a slab cannot equal it;
  * the three one-line defects the lattice is for -- a segment's w1_col applied late, the last layer-2 k quarter skipped, a bias group
    shifted by four columns -- each change a compared output of a named case.

Magnitudes measured over CASES (printed by test_magnitudes_stay_where_bf16_is_exact with -s): see its assertion."""
import pytest
import torch

from tests import mlp_exact_reference as R

IDS = [c.id for c in R.CASES]


def _masks(case, how):
    if not case.masked:
        return None, None
    if how == "kept":
        return torch.ones(case.rows, R.HP), torch.ones(case.rows, R.HP)
    g = torch.Generator().manual_seed(R._seed("cpu-mask", case.id))
    return torch.randint(0, 2, (case.rows, R.HP), generator=g), torch.randint(0, 2, (case.rows, R.HP), generator=g)


def _refs(case):
    n = R.net(case)
    for how in (("kept", "random") if case.masked else ("none",)):
        yield how, n, R.reference(n, case, *_masks(case, how))


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_every_stored_stage_is_exact_in_bf16(case):
    for how, _, (res, spans) in _refs(case):
        assert R.inadmissible(res, spans) == {}, (case.id, how)
        for k, v in res.items():
            assert not torch.signbit(v[v == 0]).any(), (k, "the reference holds no negative zero")
            assert float(v.abs().max()) > 0, (case.id, how, k)


def test_magnitudes_stay_where_bf16_is_exact():
    """max |h1|, |h2|, |out|, |q| and the largest span over all cases: bf16 holds every integer up to 256 and every even one up to 512;
    an unmasked output with a half-integer addend must stay below 128."""
    top = {}
    for case in R.CASES:
        for how, _, (res, spans) in _refs(case):
            for k, v in res.items():
                key = (k, how != "none", case.add)
                top[key] = max(top.get(key, 0.0), float(v.abs().max()))
            top["span"] = max(top.get("span", 0.0), max(spans.values()))
    print({str(k): v for k, v in sorted(top.items(), key=str)})
    assert top["span"] < R.SPAN_LIMIT / 64
    assert top["out", False, True] < 128
    for key, v in top.items():
        if key != "span" and key[0] != "q":
            assert v <= 512, key


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_every_slab_is_populated_and_seen(case):
    n = R.net(case)
    pop = R.slab_population(n, case)
    full = case.H == 256 and case.out_dim == 128
    for name, counts in pop.items():
        if name == "W3" and case.critic:
            continue
        assert min(counts) > 0, (case.id, name, counts)
        if full:       # the recipe's figures: 256 x 32 non-zeros over at most 23 slabs of W1, 256 x 8 over W2's four, 128 x 2 over W3's four
            assert min(counts) >= {"W1": 300, "W2": 400, "W3": 40}[name], (case.id, name, counts)
    masks = _masks(case, "random")
    res, _ = R.reference(n, case, *masks)
    final = "q" if case.critic else "out"
    k1 = sum(case.segs) // 64
    for name, slabs, seen_in in (("W1", k1, "h1"), ("W2", (case.H + 63) // 64, "h2"), ("W3", (case.H + 63) // 64, "out")):
        if name == "W3" and case.critic:
            continue
        for t in range(slabs):
            got, _ = R.reference(R.zero_slab(n, name, t), case, *masks)
            assert not torch.equal(got[seen_in], res[seen_in]), (case.id, name, t)
            assert not torch.equal(got[final], res[final]), (case.id, name, t, "the defect must reach the output too")


def _case(cid):
    return next(c for c in R.CASES if c.id == cid)


@pytest.mark.parametrize("cid", ["64x64-r64-actor_plain", "64x64x64-r130-critic", "1152x128x64x128-r256-actor_add", "64x64x64-r130-actor_hash-H200"])
def test_the_named_defects_change_the_reference(cid):
    """(a) w1_col of a segment applied one segment late, (b) layer 2's last k quarter skipped, (c) a bias group four columns off.  Each
    count below is the number of compared elements that the defect moves: a kernel with the defect fails the bit comparison on that case.

    The matching one-line edits of csrc/mlpf.hip (each compiles for gfx950; none was run): (a) in issue_l1,
    `col = g1 ? P.w1_col[0] : (g2 ? P.w1_col[1] : P.w1_col[2])`; (b) `if (q == 3) continue;` behind layer 2's `next_post()`; (c) b1v
    loaded from `cst + n + 4`.  Why each must show: (a) contracts segment g against the W1 columns of segment g - 1, i.e. against other
    rows' +-1 entries -- in case 64x64-r64-actor_plain 9377 of h1's 16384 elements, 9363 of h2's and 6435 of out's 8192 move; (b) is W2's
    columns 192 .. 255 zeroed, where every row of the lattice holds about two of its eight entries -- 5519 elements of h2 and 4566 of out
    move there, and in 64x64x64-r130-critic 11801 of h2's 33280 and all 130 q; (c) gives unit n the bias of unit n + 4, integers in
    [-2, 2] that differ four times in five -- 7141 elements of h1, 5645 of out, all 130 q of the critic case."""
    case = _case(cid)
    n = R.net(case)
    masks = _masks(case, "random")
    res, _ = R.reference(n, case, *masks)
    final = "q" if case.critic else "out"
    moved = lambda m, k: int((R.reference(m, case, *masks)[0][k] != res[k]).sum())
    for g in range(1, len(case.segs)):
        assert moved(R.late_w1_col(n, g), "h1") > case.rows and moved(R.late_w1_col(n, g), final) > 0, (cid, "w1_col", g)
    last = (case.H + 63) // 64 - 1
    assert moved(R.zero_slab(n, "W2", last), "h2") > case.rows // 2 and moved(R.zero_slab(n, "W2", last), final) > 0, (cid, "W2 quarter")
    for b, k in (("b1", "h1"), ("b2", "h2")):
        assert moved(R.shifted_bias(n, b), k) > case.rows and moved(R.shifted_bias(n, b), final) > 0, (cid, b)
    if not case.critic:
        assert moved(R.shifted_bias(n, "b3"), "out") > case.rows, (cid, "b3")


def test_the_padding_is_visible():
    """H < 256: whatever lies at or beyond H in the weights, the biases and w3row is non-zero, so a kernel that used it would differ"""
    case = _case("64x64x64-r130-critic-H200")
    n = R.net(case)
    assert (n["W1"][case.H:] != 0).all() and (n["W2"][case.H:] != 0).all() and (n["W2"][:, case.H:] != 0).all() and (n["W3"][:, case.H:] != 0).all()
    assert (n["b1"][case.H:] != 0).all() and (n["b2"][case.H:] != 0).all() and (n["w3row"][case.H:] != 0).all()
    assert all((a[:, k:] != 0).all() for a, k in zip(n["A"], case.segs)) and (n["W1"][:, sum(case.segs):] != 0).all()


# ------------------------------------------------------------------------------------------------ the engine's step (StepEngine)
ENGINE = sorted({(algo, B) for algo, B, *_ in R.ENGINE_CASES})


@pytest.mark.parametrize("algo,B", ENGINE, ids=lambda v: str(v))
def test_engine_step_is_exact_at_every_stage(algo, B):
    """every stage the bf16 engine holds in bf16 equals its bf16 rounding, every fp32 result its fp32 rounding, every span stays below
    SPAN_LIMIT; the backward stages where 2 / B is a power of two (elsewhere tests/test_gpu_engine_exact.py compares the forward only)"""
    batch, masks, noise, ref = R.engine_case(B, algo)
    backward = B & (B - 1) == 0
    assert R.engine_inadmissible(ref, B, backward) == {}
    assert batch["reward"].frac().abs().max() == 0 and set(batch["done"].tolist()) <= {0.0, 1.0}
    delta = ref["q1"] - ref["expected"]
    # the reward keeps the critic's loss seed at two significant bits (TD3: three -- half a target_q that carries the noise's halves)
    assert 0 < float(delta.abs().max()) <= (1.75 if algo == "td3" else 1.5) and (delta * 4).frac().abs().max() == 0
    for k, v in ref.items():
        if torch.is_tensor(v):
            assert float(v.abs().max()) > 0, k
    if noise is not None:
        assert float(noise.abs().max()) < 3.0 and (noise * 2).frac().abs().max() == 0 and (noise.frac() != 0).any()
    print(algo, B, {k: float(v.abs().max()) for k, v in ref.items() if torch.is_tensor(v)}, ref["spans"])


def test_engine_networks_populate_every_slab_and_show_a_dropped_one():
    """every 64-wide slab of every contraction of the engine's networks holds non-zeros -- the action columns of a critic's layer 1
    included, one entry per hidden unit -- and zeroing one changes the compared stage behind it"""
    nets = R.engine_nets()
    batch, masks, noise, ref = R.engine_case(64, "ddpg")
    for name, p in nets.items():
        for k in ("w1", "w2", "w3"):
            counts = [int((p[k][:, c:c + 64] != 0).sum()) for c in range(0, p[k].shape[1], 64)]
            assert min(counts) >= 8, (name, k, counts)       # (the thinnest: the 10 columns behind 22 whole slabs of [state | action])
    assert int((nets["critic1"]["w1"][:, R.ES:] != 0).sum()) == R.EH
    x = torch.cat([batch["state"], batch["action"]], 1)
    base = R._mlp(nets["critic1"], x, masks[0], masks[1])
    for k, width in (("w1", R.ES + R.EA), ("w2", R.EH), ("w3", R.EH)):
        for c in range(0, width, 64):
            p = dict(nets["critic1"])
            p[k] = p[k].clone()
            p[k][:, c:c + 64] = 0
            assert not torch.equal(R._mlp(p, x, masks[0], masks[1])[0], base[0]), (k, c)
