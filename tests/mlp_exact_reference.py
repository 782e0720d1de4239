"""Exact references for the fused three-layer networks of the bf16 engine (mlp_frozen_kernel, csrc/mlpf.hip), CPU only.

tests/gemm_exact_reference.py makes ONE product exact; here a whole network is: operands from lattices on which every partial sum
of every layer is an integer (or a half) far below 2^24, AND every activation that the kernel stores as bf16 between two layers is
representable in bf16.  A correct kernel then equals the float64 network bit for bit at every stored stage, in any summation order.

  inputs A         integers in [-1, 1]; the padding columns of a pitch wider than K hold +-1
  W1 [H, K]        NNZ1 = 32 entries of +-1 per row, positions drawn over the whole contraction
  W2 [H, H]        NNZ2 = 8 entries of +-1 per row
  W3 [out, H]      NNZ3 = 2 entries of +-1 per row, in the 64-column slabs 2 r and 2 r + 1 (mod their number) for row r
  critic w3row     integers in [-3, 3] (fp32)
  biases           integers in [-2, 2]
  addend           multiples of 0.5 in [-3, 3] with add_clip 1.5; next to dropout masks whole numbers with add_clip 1.0 (a masked
                   output is even and can pass 128, where bf16 has no halves)
  dropout          a kept element counts twice

The weights are always [256, >= 256] (W3: [128, >= 256]) as the kernel streams them, whatever H and out_dim: everything at or
beyond H (rows and columns) or out_dim (rows of W3, entries of b3) holds +-1, entries of the biases and of w3row there +-2, so a
result that used the padding differs from the reference.

Admissibility (`inadmissible`) is a condition on the operands, not a tolerance on the kernel: every element of h1, h2 and out must
equal its bf16 rounding and every contraction's span -- max over outputs of sum_k |a||b| plus the epilogue's terms, in units of the
least significant bit (1; 0.5 for an output with an addend) -- must stay below gemm_exact_reference.SPAN_LIMIT.  tests/test_mlp_exact_cpu.py asserts it
for every case of CASES; tests/test_gpu_frozen_exact.py repeats it with the masks the GPU drew before it compares.

The second half of the file (engine_nets, engine_case, engine_inadmissible, ENGINE_CASES) does the same for one whole DDPG / TD3 step
of the bf16 StepEngine, forward and backward: tests/test_gpu_engine_exact.py.
"""
import functools
import zlib
from dataclasses import dataclass

import torch

from tests.gemm_exact_reference import SPAN_LIMIT

HP, OUTP = 256, 128             # rows of W1 / W2 and of W3 that the kernel streams whatever H and out_dim
NNZ1, NNZ2, NNZ3 = 32, 8, 2
ADD_CLIP, ADD_CLIP_MASKED = 1.5, 1.0
SEGMENTS = [(128,), (64, 64), (64, 64, 64), (64, 64, 64, 64), (1152, 128, 64, 128)]
ROWS = (64, 130, 256)
KINDS = ("actor_plain", "actor_add", "critic", "actor_hash")


@dataclass(frozen=True)
class Case:
    id: str
    segs: tuple
    rows: int
    kind: str                   # actor_plain | actor_add | critic | actor_hash | actor_hash_add
    H: int = 256
    out_dim: int = 128
    rows_per_set: int = 0       # hash masks: batches of this many rows, batch j draws its masks at step + j (0: one batch)
    store_row0: int = 0

    @property
    def masked(self):
        return self.kind.startswith("actor_hash")

    @property
    def add(self):
        return self.kind in ("actor_add", "actor_hash_add")

    @property
    def critic(self):
        return self.kind == "critic"

    @property
    def add_clip(self):
        return ADD_CLIP_MASKED if self.masked else ADD_CLIP


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _pm1(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()


def _sparse(rows, cols, nnz, g):
    """[rows, cols] with min(nnz, cols) entries of +-1 per row"""
    keep = torch.rand(rows, cols, generator=g).argsort(dim=1) < min(nnz, cols)
    return torch.where(keep, _pm1((rows, cols), g), torch.zeros(rows, cols, dtype=torch.float64))


def w1_cols(segs):
    """the segments' W1 columns in reverse order: every w1_col differs from the running k"""
    cols, c = [], sum(segs)
    for k in segs:
        c -= k
        cols.append(c)
    return cols


@functools.lru_cache(maxsize=4)
def _net(segs, rows, H):
    g = torch.Generator().manual_seed(_seed("mlp", segs, rows, H))
    k1 = sum(segs)
    n = dict(segs=segs, rows=rows, H=H, w1_col=w1_cols(segs))
    n["A"] = []
    for i, k in enumerate(segs):                                   # pitches wider than K, the padding +-1
        a = _pm1((rows, k + 8 * (i + 1)), g)
        a[:, :k] = torch.randint(-1, 2, (rows, k), generator=g).double()
        n["A"].append(a)
    for name, r, ld, valid_c, nnz in (("W1", HP, k1 + 8, k1, NNZ1), ("W2", HP, HP + 8, H, NNZ2), ("W3", OUTP, HP + 8, H, NNZ3)):
        w = _pm1((r, ld), g)
        valid_r = H if name != "W3" else OUTP                      # (W3's rows at and beyond out_dim are lattice rows too: computed, never stored)
        w[:valid_r, :valid_c] = _sparse(valid_r, valid_c, nnz, g)
        slabs = (valid_c + 63) // 64
        if name == "W3" and slabs > 1:
            # two entries per row cannot be left to chance with four output rows: row r takes slabs 2 r and 2 r + 1 (mod their number),
            # so any two neighbouring rows populate all four
            w[:valid_r, :valid_c] = 0
            for j in range(NNZ3):
                s = (NNZ3 * torch.arange(valid_r) + j) % slabs
                width = torch.clamp(valid_c - 64 * s, max=64)
                col = 64 * s + (torch.rand(valid_r, generator=g) * width).long()
                w[torch.arange(valid_r), col] = _pm1((valid_r,), g)
        n[name] = w
    for name, size in (("b1", HP), ("b2", HP), ("b3", OUTP)):
        n[name] = torch.randint(-2, 3, (size,), generator=g).double()
    n["w3row"] = torch.randint(-3, 4, (HP,), generator=g).double()
    for name in ("b1", "b2", "w3row"):
        n[name][H:] = 2.0
    half = torch.randint(-6, 7, (rows, OUTP + 4), generator=g).double() * 0.5
    n["addend"] = {False: half, True: torch.randint(-3, 4, (rows, OUTP + 4), generator=g).double()}
    return n


def net(case):
    """The operands of a case as float64 tensors (a fresh shallow copy: cases that share segments, rows and H share one draw).
    b3 beyond out_dim holds 2, `addend` is the case's own lattice."""
    n = dict(_net(case.segs, case.rows, case.H))
    n["b3"] = n["b3"].clone()
    n["b3"][case.out_dim:] = 2.0
    n["addend"] = n["addend"][case.masked]
    return n


def layer1_operands(n):
    """(x [rows, K], w [HP, K]) of layer 1 in contraction order: the segments against their W1 columns"""
    x = torch.cat([a[:, :k] for a, k in zip(n["A"], n["segs"])], dim=1)
    w = torch.cat([n["W1"][:, c:c + k] for c, k in zip(n["w1_col"], n["segs"])], dim=1)
    return x, w


def set_masks(case):
    """[(first row, rows)] of the batches that draw dropout masks of their own"""
    rps = case.rows_per_set or case.rows
    return [(r0, min(rps, case.rows - r0)) for r0 in range(0, case.rows, rps)]


def reference(n, case, keep1=None, keep2=None):
    """float64 {h1, h2 [rows, 256], out [rows, out_dim] | q [rows]} and {stage: span}.  keep1 / keep2: [rows, >= H] keep masks of
    a masked case.  relu(x W^T + b), times the keep mask times 2; padded columns are +0; no negative zeros."""
    H, res, spans = case.H, {}, {}

    def hidden(x, w, b, keep, name):
        v = torch.relu(x @ w.t() + b)
        spans[name] = float((x.abs() @ w.abs().t() + b.abs()).max())
        if case.masked:
            v = torch.where(keep[:, :H].bool(), v * 2.0, torch.zeros_like(v))
        full = torch.zeros(case.rows, HP, dtype=torch.float64)
        full[:, :H] = v
        res[name] = full + 0.0
        return v

    x, w = layer1_operands(n)
    h1 = hidden(x, w[:H], n["b1"][:H], keep1, "h1")
    h2 = hidden(h1, n["W2"][:H, :H], n["b2"][:H], keep2, "h2")
    if case.critic:
        res["q"] = h2 @ n["w3row"][:H] + n["b3"][0]
        spans["q"] = float((h2.abs() @ n["w3row"][:H].abs() + n["b3"][0].abs()).max())
    else:
        od = case.out_dim
        out = h2 @ n["W3"][:od, :H].t() + n["b3"][:od]
        spans["out"] = float((h2.abs() @ n["W3"][:od, :H].abs().t() + n["b3"][:od].abs()).max())
        if case.add:
            out = out + n["addend"][:, :od].clamp(-case.add_clip, case.add_clip)
            spans["out"] = 2.0 * (spans["out"] + case.add_clip)     # (in halves)
        res["out"] = out + 0.0
    return res, spans


def inadmissible(res, spans):
    """{stage: share of elements that bf16 does not hold | 1.0 for a span at or beyond SPAN_LIMIT}, empty for an admissible case"""
    bad = {}
    for k, v in res.items():
        if k != "q":
            share = float((v.float().to(torch.bfloat16).double() != v).double().mean())
            if share:
                bad[k] = share
    for k, s in spans.items():
        if not s < SPAN_LIMIT:
            bad["span_" + k] = 1.0
    return bad


# ------------------------------------------------------------------------------------------- the defects the lattice is for
def zero_slab(n, name, t):
    """`n` with 64-wide contraction slab t of W1 (in contraction order), W2 or W3 zeroed"""
    m = dict(n)
    w = n[name].clone()
    if name == "W1":
        for c, k in zip(n["w1_col"], n["segs"]):
            if t < k // 64:
                w[:, c + 64 * t:c + 64 * t + 64] = 0
                break
            t -= k // 64
    else:
        w[:, 64 * t:64 * t + 64] = 0
    m[name] = w
    return m


def late_w1_col(n, g):
    """`n` with segment g (>= 1) contracted against the W1 columns of segment g - 1: a re-basing applied one segment late"""
    m = dict(n)
    m["w1_col"] = list(n["w1_col"])
    m["w1_col"][g] = n["w1_col"][g - 1]
    return m


def shifted_bias(n, name, by=4):
    m = dict(n)
    m[name] = torch.roll(n[name], by)
    return m


def slab_population(n, case):
    """non-zeros per 64-wide contraction slab of the rows and columns a case uses: {W1: [...], W2: [...], W3: [...]}"""
    H = case.H
    _, w1 = layer1_operands(n)
    rows3 = n["W3"][:case.out_dim, :H]
    count = lambda w: [int((w[:, c:c + 64] != 0).sum()) for c in range(0, w.shape[1], 64)]
    return dict(W1=count(w1[:H]), W2=count(n["W2"][:H, :H]), W3=count(rows3))


# ---------------------------------------------------------------------------------------------------------------- the case table
def _build():
    cs = []
    # segments x rows x kinds; the masked actor in batches of 64 rows: the mask step changes inside a 128-row panel
    for segs in SEGMENTS:
        sid = "x".join(map(str, segs))
        for rows in ROWS:
            for kind in KINDS:
                cs.append(Case(f"{sid}-r{rows}-{kind}", segs, rows, kind, rows_per_set=64 if kind == "actor_hash" else 0))
    # batches of 32 rows (the step changes inside a 64-row panel too), one batch for the whole problem, masks next to an addend
    for rows in ROWS:
        cs.append(Case(f"64x64x64-r{rows}-hash-rps32", (64, 64, 64), rows, "actor_hash", rows_per_set=32))
    cs.append(Case("64x64-r130-hash-rps0", (64, 64), 130, "actor_hash"))
    cs.append(Case("64x64x64-r130-hash-add-rps64", (64, 64, 64), 130, "actor_hash_add", rows_per_set=64))
    # the first stored row: inside a 128-row panel and behind a whole 64-row one (72), on a panel edge (128), nothing stored (rows)
    for r0 in (72, 128, 130):
        for kind in ("actor_hash", "critic"):
            cs.append(Case(f"64x64x64-r130-{kind}-row0_{r0}", (64, 64, 64), 130, kind, rows_per_set=64 if kind == "actor_hash" else 0, store_row0=r0))
    # narrow outputs: the four forms of the output stage
    for od in (4, 120, 124, 128):
        for kind in ("actor_plain", "actor_add"):
            cs.append(Case(f"64x64x64-r130-{kind}-out{od}", (64, 64, 64), 130, kind, out_dim=od))
    # hidden widths below 256
    for H in (8, 64, 200, 256):
        for kind in ("actor_add", "critic", "actor_hash"):
            cs.append(Case(f"64x64x64-r130-{kind}-H{H}", (64, 64, 64), 130, kind, H=H, out_dim=120 if kind == "actor_add" else 128,
                           rows_per_set=32 if kind == "actor_hash" else 0))
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _build()


# ============================================================================================ the bf16 engine's step (StepEngine)
# One DDPG / TD3 step (oracle/recnn_oracle.py ddpg_step / td3_step) at S, A, H = 1290, 128, 256 on lattice networks and a lattice
# batch, external dropout masks, gamma = 0.5, no clamp of the TD target, and a critic learning rate of ZERO: the critic's optimizer
# launch runs (and its gradient is compared) but leaves the parameters on the lattice, so the policy half of the step -- the critic
# on [state | gen_action], dact, the actor's gradient -- is exact too and meets the float64 chain itself, not a conditioned one.
#
#   state, action, next_state   integers in [-1, 1]
#   actor                       W1 16, W2 4, W3 1 entries of +-1 per row, biases in [-1, 1]: |gen_action| stays near 100, because ...
#   critics                     W1 31 entries of +-1 per row over the state columns and ONE over the action columns (every slab of
#                               [state | action] populated; an action of 100 enters a hidden unit once), W2 8 per row, w3 in [-1, 1],
#                               biases in [-2, 2]
#   TD3 noise                   multiples of 0.5 in [-1, 1], inside the clip
#   done                        0 or 1
#   reward                      the integer that brings expected within [-1, 1.5] of q1: q1 - ceil((1 - done) gamma target_q) + u,
#                               u in {-1, 0, 1}.  d = (q1 - expected) 2 / B then has two significant bits and dz2, dz1 (stored as
#                               bf16, with or without the per-row factor d) stay representable; B is a power of two for the backward.
ES, EA, EH = 1290, 128, 256
GAMMA = 0.5
ENGINE_ROWS = (64, 96, 333, 1024)
# (algo, rows, split_fwd, dw_fuse, policy_fused): every batch size under the fused and the split forward; the backward (64 and 1024 rows)
# under both critic dW forms and both actor dW forms; TD3 with lattice noise at 1024 rows
ENGINE_CASES = [("ddpg", 64, 0, 1, 0), ("ddpg", 64, 2, 1, 3), ("ddpg", 96, 0, 1, 3), ("ddpg", 96, 2, 1, 3), ("ddpg", 333, 0, 1, 3),
                ("ddpg", 333, 2, 1, 3), ("ddpg", 1024, 0, 0, 0), ("ddpg", 1024, 0, 1, 3), ("ddpg", 1024, 2, 0, 3), ("ddpg", 1024, 2, 1, 0),
                ("td3", 1024, 0, 1, 3), ("td3", 1024, 2, 1, 3)]


def _engine_net(inp, out, g, nnz, brange, action_cols=0):
    state_cols = inp - action_cols
    w1 = torch.zeros(EH, inp, dtype=torch.float64)
    w1[:, :state_cols] = _sparse(EH, state_cols, nnz[0], g)
    if action_cols:
        w1[torch.arange(EH), state_cols + torch.randint(0, action_cols, (EH,), generator=g)] = _pm1((EH,), g)
    w3 = _sparse(out, EH, nnz[2], g) if out > 1 else torch.randint(-1, 2, (1, EH), generator=g).double()
    b = lambda n: torch.randint(-brange, brange + 1, (n,), generator=g).double()
    return dict(w1=w1, b1=b(EH), w2=_sparse(EH, EH, nnz[1], g), b2=b(EH), w3=w3, b3=b(out))


@functools.lru_cache(maxsize=1)
def engine_nets():
    g = torch.Generator().manual_seed(_seed("engine-nets"))
    return dict(actor=_engine_net(ES, EA, g, (16, 4, 1), 1), critic1=_engine_net(ES + EA, 1, g, (31, 8, 0), 2, EA),
                critic2=_engine_net(ES + EA, 1, g, (31, 8, 0), 2, EA))


def _span(spans, tag, a, b, unit):
    """records max sum_k |a||b| of the product a @ b in units of its least significant bit"""
    if spans is not None:
        spans[tag] = max(spans.get(tag, 0.0), float((a.abs() @ b.abs()).max()) / unit)


def _mlp(p, x, m1=None, m2=None, spans=None, unit=1.0):
    drop = lambda h, m: h if m is None else torch.where(m.bool(), h * 2.0, torch.zeros_like(h))
    h1 = drop(torch.relu(x @ p["w1"].t() + p["b1"]), m1)
    h2 = drop(torch.relu(h1 @ p["w2"].t() + p["b2"]), m2)
    for tag, a, w in (("fwd1", x, p["w1"]), ("fwd2", h1, p["w2"]), ("fwd3", h2, p["w3"])):
        _span(spans, tag, a, w.t(), unit)
    return h2 @ p["w3"].t() + p["b3"], h1 + 0.0, h2 + 0.0


def _mlp_backward(p, x, h1, h2, dout, spans=None, unit=1.0):
    """oracle/recnn_oracle.py mlp_backward with dropout (the gates are the stored activations' signs), in float64"""
    g = dict(w3=dout.t() @ h2, b3=dout.sum(0))
    dz2 = (dout @ p["w3"]) * ((h2 > 0).double() * 2.0)
    g.update(w2=dz2.t() @ h1, b2=dz2.sum(0))
    dz1 = (dz2 @ p["w2"]) * ((h1 > 0).double() * 2.0)
    g.update(w1=dz1.t() @ x, b1=dz1.sum(0))
    for tag, a, b in (("dw3", dout.t(), h2), ("dx3", dout, p["w3"]), ("dw2", dz2.t(), h1), ("dx2", dz2, p["w2"]), ("dw1", dz1.t(), x),
                      ("dx1", dz1, p["w1"])):
        _span(spans, tag, a, b, unit)
    return g, dz2 + 0.0, dz1 + 0.0, dz1 @ p["w1"]


@functools.lru_cache(maxsize=2)
def engine_case(B, algo):
    """(batch, masks, noise | None, float64 reference of every compared stage) of one step on B rows"""
    td3 = algo == "td3"
    nets = engine_nets()
    g = torch.Generator().manual_seed(_seed("engine-batch", B, algo))
    ints = lambda *shape: torch.randint(-1, 2, shape, generator=g).double()
    s, a, s2 = ints(B, ES), ints(B, EA), ints(B, ES)
    done = torch.randint(0, 2, (B,), generator=g).double()
    masks = [torch.randint(0, 2, (B, EH), generator=g).to(torch.uint8) for _ in range(8 if td3 else 6)]
    noise = torch.randint(-2, 3, (B, EA), generator=g).double() * 0.5 if td3 else None
    r, sp = {}, {}
    fw, bw = dict(spans=sp, unit=0.5), dict(spans=sp, unit=1.0 / (4 * B))   # (halves: the TD3 noise; 1 / (4 B): a half times 2 / B, times a half)
    na, r["ta_h1"], r["ta_h2"] = _mlp(nets["actor"], s2, **fw)
    r["next_action"] = na + noise if td3 else na
    xn = torch.cat([s2, r["next_action"]], 1)
    tq, r["tc1_h1"], r["tc1_h2"] = _mlp(nets["critic1"], xn, **fw)
    if td3:
        tq2, r["tc2_h1"], r["tc2_h2"] = _mlp(nets["critic2"], xn, **fw)
        tq = torch.minimum(tq, tq2)
    r["target_q"] = tq[:, 0]
    x = torch.cat([s, a], 1)
    q1, r["critic1_h1"], r["critic1_h2"] = _mlp(nets["critic1"], x, masks[0], masks[1], **fw)
    r["q1"] = q1[:, 0]
    if td3:
        q2, r["critic2_h1"], r["critic2_h2"] = _mlp(nets["critic2"], x, masks[2], masks[3], **fw)
        r["q2"] = q2[:, 0]
    future = (1.0 - done) * GAMMA * r["target_q"]
    reward = r["q1"] - torch.ceil(future) + torch.randint(-1, 2, (B,), generator=g).double()
    r["expected"] = reward + future
    dq = ((r["q1"] - r["expected"]) * (2.0 / B)).reshape(B, 1)
    r["value_grads"], r["critic1_dz2"], r["critic1_dz1"], _ = _mlp_backward(nets["critic1"], x, r["critic1_h1"], r["critic1_h2"], dq, **bw)
    k = 4 if td3 else 2
    r["gen_action"], r["actor_h1"], r["actor_h2"] = _mlp(nets["actor"], s, masks[k], masks[k + 1], **fw)
    xp = torch.cat([s, r["gen_action"]], 1)
    qpi, r["pc_h1"], r["pc_h2"] = _mlp(nets["critic1"], xp, masks[k + 2], masks[k + 3], **fw)
    r["q_pi"] = qpi[:, 0]
    _, r["dze2"], r["dze1"], dx = _mlp_backward(nets["critic1"], xp, r["pc_h1"], r["pc_h2"], torch.full((B, 1), -1.0 / B, dtype=torch.float64), **bw)
    r["dact"] = dx[:, ES:] + 0.0
    r["policy_grads"], r["dzp2"], r["dzp1"], _ = _mlp_backward(nets["actor"], s, r["actor_h1"], r["actor_h2"], r["dact"], **bw)
    r["spans"] = sp
    batch = dict(state=s, action=a, reward=reward, next_state=s2, done=done)
    return batch, masks, noise, r


# what the engine holds in bf16 (in memory or in a workgroup's panel between two layers); the rest is fp32
ENGINE_BF16 = ("next_action", "gen_action", "ta_h1", "ta_h2", "tc1_h1", "tc1_h2", "tc2_h1", "tc2_h2", "critic1_h1", "critic1_h2", "critic2_h1",
               "critic2_h2", "actor_h1", "actor_h2", "pc_h1", "pc_h2", "critic1_dz2", "critic1_dz1", "dze2", "dze1", "dact", "dzp2", "dzp1")


ENGINE_BACKWARD = ("critic1_dz2", "critic1_dz1", "dze2", "dze1", "dact", "dzp2", "dzp1", "value_grads", "policy_grads")


def engine_inadmissible(r, B, backward=True):
    """{stage: share of elements that bf16 (ENGINE_BF16) or fp32 (the rest) does not hold | 1.0 for a contraction whose span reaches
    SPAN_LIMIT}, empty for an admissible case.  backward = False: the forward stages only (2 / B is no power of two)."""
    bad = {}
    flat = {k: v for k, v in r.items() if torch.is_tensor(v)}
    for tag in ("value_grads", "policy_grads"):
        flat.update({f"{tag}.{k}": v for k, v in r[tag].items()})
    for k, v in flat.items():
        if not backward and k.split(".")[0] in ENGINE_BACKWARD:
            continue
        narrow = v.float().to(torch.bfloat16).double() if k in ENGINE_BF16 else v.float().double()
        share = float((narrow != v).double().mean())
        if share:
            bad[k] = share
    for k, v in r["spans"].items():
        if not v < SPAN_LIMIT and (backward or k.startswith("fwd")):
            bad["span_" + k] = 1.0
    return bad
