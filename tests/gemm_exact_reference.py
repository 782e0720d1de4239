"""Exact references for the GEMM entry points (recnn_gemm_fwd / recnn_gemm_dx / recnn_gemm_dw), CPU only.

The operands are drawn from lattices on which every partial sum of a product is exactly representable in fp32, so a correct
kernel equals the float64 product bit for bit in ANY summation order and at any tile shape -- no tolerance:

  ints : integers in [-3, 3] (exact in bf16 and fp32);
  wide : m / 256 with |m| <= 4095 (12 significant bits: beyond bf16 and tf32).  A wide operand only ever meets an ints one: in
         fp32 it shows any narrowing of the inputs, in split-bf16 its lo half is non-zero while the other operand has none, so
         hi*hi + lo*hi is the exact product and the dropped lo*lo term is zero.  Never used for plain bf16.

Epilogue operands are exact too: bias integers in [-4, 4], addend multiples of 0.5 in [-3, 3] (clamped at 1.5 or unclamped), gate
operand in {-1, 0, 1} with scale 0.5, dropout masks (x 2).

`span(case)` is max over outputs of sum_k |a||b| in units of the lattice's least significant bit; a case is admissible below 2^22
(fp32 holds 2^24; the factor 4 is margin for a matrix unit that aligns its addends to the largest exponent before adding).

The case table (CASES) is shared by tests/test_gemm_exact_cpu.py and tests/test_gpu_gemm_exact.py.  The dispatch notes next to
each group restate gemm.hip launch_t / launch_dma / x3_fwd_launch under the default GemmTune (KB = k per 256-byte stage).
"""
import functools
import zlib
from dataclasses import dataclass, replace

import torch

from tests.helpers import x3_pack_ref

SPAN_LIMIT = 2 ** 22
LSB = {"ints": 1.0, "wide": 2.0 ** -8}
ADD_CLIP = 1.5
GATE_SCALE = 0.5
HASH_KEY = (123, 7, 2)          # (seed, step, stream id) of the hash-mask cases


@dataclass(frozen=True)
class Case:
    id: str
    family: str                 # the kernel family the case is for
    op: str                     # fwd | dx | dw
    dtype: str                  # fp32 | bf16 | x3
    M: int
    N: int
    K: tuple                    # logical contraction length per segment (dw: the number of rows)
    a_lat: str = "ints"
    b_lat: str = "ints"
    out: str = "f32"            # f32 | tc (the compute type in memory: fp32, bf16 or split rows)
    ldc: int = 0                # 0: a padded default
    a_f32: bool = False         # bf16 compute, A stored as fp32
    b_f32: bool = False
    # forward epilogue
    bias: bool = False
    relu: bool = False
    mask: str = "none"          # none | ext | hash
    add: str = "none"           # none | clamp | inf | div3
    gate: bool = False          # yref gate (fwd: scale 0.5 after relu; dx: scale 0.5)
    ws: str = "none"            # none | fit | small   (split-K scratch)
    hook: tuple = ()            # (debug hook, value, value to restore)
    # dx
    ldb: int = 0                # pitch of the k-strided B (logical columns; split-bf16 doubles it)
    colsum: bool = False
    # dw
    splits: int = 1
    valid: int = 0              # dw_valid_cols (0: N)
    rot: int = 0
    pad: int = 0                # extra operand pitch beyond roundup(., 64)

    @property
    def scale(self):
        return GATE_SCALE if self.gate else (2.0 if self.op == "dx" else 1.0)


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def lattice(kind, shape, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "ints":
        return torch.randint(-3, 4, shape, generator=g).double()
    assert kind == "wide"
    return torch.randint(-4095, 4096, shape, generator=g).double() / 256.0


@functools.lru_cache(maxsize=3)
def _operands(op, M, N, K, a_lat, b_lat):
    a, b = [], []
    for s, k in enumerate(K):
        if op == "fwd":
            sa, sb = (M, k), (N, k)
        elif op == "dx":
            sa, sb = (M, k), (k, N)
        else:
            sa, sb = (k, M), (k, N)
        a.append(lattice(a_lat, sa, _seed("a", op, M, N, K, s, a_lat)))
        b.append(lattice(b_lat, sb, _seed("b", op, M, N, K, s, b_lat)))
    mul = {"fwd": lambda x, y: x @ y.t(), "dx": lambda x, y: x @ y, "dw": lambda x, y: x.t() @ y}[op]
    prod = sum(mul(x, y) for x, y in zip(a, b))
    absum = sum(mul(x.abs(), y.abs()) for x, y in zip(a, b))
    return a, b, prod, float(absum.max()) / (LSB[a_lat] * LSB[b_lat])


def operands(case):
    """(A segments, B segments, float64 product) of a case; equal shapes and lattices share one draw."""
    return _operands(case.op, case.M, case.N, case.K, case.a_lat, case.b_lat)[:3]


def span(case):
    return _operands(case.op, case.M, case.N, case.K, case.a_lat, case.b_lat)[3]


@functools.lru_cache(maxsize=4)
def epilogue_operands(M, N):
    g = torch.Generator().manual_seed(_seed("epi", M, N))
    return dict(bias=torch.randint(-4, 5, (N,), generator=g).float(),
                addend=torch.randint(-6, 7, (M, N), generator=g).float() * 0.5,
                yref=torch.randint(-1, 2, (M, N), generator=g).float(),
                mask=torch.randint(0, 2, (M, N), generator=g).to(torch.uint8))


def reference(case, hash_mask=None):
    """float64 result of a case before the output type.  fwd: the order of gemm.hip epilogue_fwd -- bias, clamped addend, relu,
    gate, mask.  dx: scale and gate.  dw: the stored columns, rotated.  `hash_mask`: the [M, N] keep mask of a hash case."""
    prod = operands(case)[2]
    e = epilogue_operands(case.M, case.N)
    if case.op == "dw":
        valid = case.valid or case.N
        return torch.roll(prod[:, :valid], case.rot, dims=1)
    if case.op == "dx":
        ref = prod * case.scale
        return torch.where(e["yref"].double() > 0, ref, torch.zeros_like(ref)) if case.gate else ref
    ref = prod.clone()
    if case.bias:
        ref = ref + e["bias"].double()
    if case.add != "none":
        add = e["addend"].double()
        if case.add == "div3":
            add = add[torch.arange(case.M) // 3]
        ref = ref + (add if case.add == "inf" else add.clamp(-ADD_CLIP, ADD_CLIP))
    if case.relu:
        ref = torch.relu(ref)
    if case.gate:
        ref = torch.where(e["yref"].double() > 0, ref * case.scale, torch.zeros_like(ref))
    if case.mask != "none":
        keep = e["mask"] if case.mask == "ext" else hash_mask
        ref = torch.where(keep.bool(), ref * 2.0, torch.zeros_like(ref))
    return ref + 0.0            # (no negative zeros: the kernels never produce one)


def colsum_reference(ref):
    """dX column sums per 32-row slab, the ragged last slab included: float64 [ceil(M / 32), N]."""
    M = ref.shape[0]
    return torch.stack([ref[s:s + 32].sum(0) for s in range(0, M, 32)])


def to_output(ref, case):
    """The float64 reference in the case's output type: fp32, bf16 (round to nearest even) or split-bf16 rows."""
    if case.out == "f32" or case.dtype == "fp32":
        return ref.float()
    if case.dtype == "bf16":
        return ref.float().to(torch.bfloat16)
    return x3_pack_ref(ref.float())


def memory_type(t, case, which):
    """An operand as it is stored: fp32, bf16 or (split-bf16) the fp32 values its split rows hold."""
    f32 = case.dtype == "fp32" or (which == "a" and case.a_f32) or (which == "b" and case.b_f32)
    return t.float() if f32 or case.dtype == "x3" else t.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------- the case table
# epilogue options, thinned to a covering set: every value of every option, every pair of options at least once in most pairings
#        bias relu  mask    add      gate
_EPI = [(0, 0, "none", "none", 0), (1, 1, "ext", "clamp", 1), (1, 0, "hash", "div3", 0), (0, 1, "hash", "clamp", 1),
        (1, 1, "none", "div3", 1), (0, 0, "ext", "div3", 0), (1, 0, "ext", "none", 1), (0, 1, "none", "clamp", 0),
        (1, 1, "hash", "none", 0), (0, 0, "hash", "div3", 1), (0, 1, "ext", "inf", 0), (1, 0, "none", "inf", 1),
        (1, 1, "hash", "inf", 1)]


def _epi(c, e):
    return replace(c, id=f"{c.id}-epi{_EPI.index(e)}", bias=bool(e[0]), relu=bool(e[1]), mask=e[2], add=e[3], gate=bool(e[4]))


def _build():
    cs = []
    kb = {"fp32": 64, "bf16": 128}

    def lat(dtype, i):          # fp32 / split-bf16: wide against ints, the orientation alternating
        if dtype == "bf16":
            return "ints", "ints"
        return ("wide", "ints") if i % 2 == 0 else ("ints", "wide")

    # ---- forward, generic register-staged kernel: K not a multiple of KB (k-tail zero fill; fp32 wide A)
    for dtype, ks in (("fp32", (4, 36, 68, 100)), ("bf16", (8, 72, 136, 200))):
        for i, k in enumerate(ks):
            for M, N in ((33, 16), (70, 130), (1, 1)):
                cs.append(Case(f"gen-{dtype}-{M}x{N}-k{k}", "gemm_fwd", "fwd", dtype, M, N, (k,), "wide" if dtype == "fp32" else "ints",
                               "ints", out="tc" if i % 2 else "f32", ldc=4 if N == 1 else 0))
        # >= 512 tiles of 64 x 64: the 64 x 64 variant instead of 32 x 64
        cs.append(Case(f"gen-{dtype}-grid-k{ks[0]}", "gemm_fwd_64", "fwd", dtype, 1990, 1050, (ks[0],), "wide" if dtype == "fp32" else "ints"))
    cs.append(Case("gen-fp32-70x130-k68-wideB", "gemm_fwd", "fwd", "fp32", 70, 130, (68,), "ints", "wide"))
    # fp32 A with bf16 compute
    cs.append(Case("gen-a32-2seg", "gemm_fwd_a32", "fwd", "bf16", 70, 130, (8, 72), a_f32=True, out="tc"))
    cs.append(Case("gen-a32-k200", "gemm_fwd_a32", "fwd", "bf16", 70, 130, (200,), a_f32=True))
    # ---- LDS-DMA ring, 5 stages (<= 320 tiles of 32 x 64): fewer stages than the prefetch distance, the ring, one wrap
    for dtype in ("fp32", "bf16"):
        for i, n in enumerate((1, 2, 4, 5, 6)):
            for j, (M, N) in enumerate(((70, 130), (33, 62))):
                a, b = lat(dtype, i + j)
                cs.append(Case(f"dma5-{dtype}-{M}x{N}-s{n}", "dma5", "fwd", dtype, M, N, (n * kb[dtype],), a, b, out="tc" if (i + j) % 2 else "f32"))
        cs.append(Case(f"dma5-{dtype}-2seg", "dma5", "fwd", dtype, 70, 130, (kb[dtype], 2 * kb[dtype]), *lat(dtype, 0)))
    # ---- LDS-DMA ring, 3 stages (> 320 tiles); N % 4 = 2 and ldc = N + 2
    for dtype in ("fp32", "bf16"):
        for n in (1, 2, 3, 4):
            for out in ("f32", "tc"):
                cs.append(Case(f"dma3-{dtype}-s{n}-{out}", "dma3", "fwd", dtype, 650, 1030, (n * kb[dtype],), *lat(dtype, n), out=out, ldc=1032))
    # ---- catalogue-wide (N >= 8192, M >= 128): 128 x 128 kernel; bf16 above 128 rows: the wave-specialised 256 x 128 kernel
    cs.append(Case("wide-fp32", "wide", "fwd", "fp32", 130, 8200, (192,), "wide", "ints"))
    cs.append(Case("wide-bf16-m128", "wide", "fwd", "bf16", 128, 8200, (256,)))
    for out in ("tc", "f32"):
        cs.append(Case(f"tall-{out}", "tall", "fwd", "bf16", 257, 8200, (384,), out=out))
        cs.append(Case(f"tall-{out}-square", "wide", "fwd", "bf16", 257, 8200, (384,), out=out, hook=("recnn_debug_wide_ws", 0, 1)))
    # ---- split-K (K >= 32768 and scratch): uneven last slice, the whole epilogue in splitk_finish_kernel; too little scratch: one walk
    for dtype, k in (("fp32", 32960), ("bf16", 33152)):
        for out in ("f32", "tc"):
            for ws in ("fit", "small"):
                cs.append(Case(f"splitk-{dtype}-{out}-{ws}", "splitk" if ws == "fit" else "wide", "fwd", dtype, 128, 130, (k,), out=out, ws=ws,
                               bias=True, relu=True, mask="ext", add="clamp", gate=True))
    # ---- the epilogue sweep at one ragged shape per family (M % 3, M % 4 and N % 4 all non-zero)
    for e in _EPI:
        for dtype in ("fp32", "bf16"):
            a, b = lat(dtype, _EPI.index(e))
            out = "tc" if _EPI.index(e) % 2 else "f32"
            cs.append(_epi(Case(f"gen-{dtype}", "gemm_fwd", "fwd", dtype, 70, 130, ({"fp32": 36, "bf16": 72}[dtype],), a, b, out=out), e))
            cs.append(_epi(Case(f"dma5-{dtype}", "dma5", "fwd", dtype, 70, 130, (2 * kb[dtype],), a, b, out=out), e))
            cs.append(_epi(Case(f"splitk-{dtype}", "splitk", "fwd", dtype, 130, 130, ({"fp32": 32960, "bf16": 33152}[dtype],), out=out, ws="fit"), e))
        cs.append(_epi(Case("tall", "tall", "fwd", "bf16", 257, 8202, (128,), out="tc" if _EPI.index(e) % 2 else "f32"), e))
    # ---- forward, split-bf16: 5-stage ring, 3-stage ring, 64 x 128 tiles (>= 192 of them)
    for M, N, fam, ks in ((70, 130, "x3_fwd_5", (64, 128, 320, 384)), (650, 1030, "x3_fwd_3", (64, 128, 320, 384)), (2050, 770, "x3_fwd_big", (64,))):
        for k in ks:
            for i in (0, 1):
                for out in ("tc", "f32"):
                    cs.append(Case(f"x3-{M}x{N}-k{k}-{lat('x3', i)[0]}A-{out}", fam, "fwd", "x3", M, N, (k,), *lat("x3", i), out=out))
        if 384 in ks:
            for out in ("tc", "f32"):
                cs.append(Case(f"x3-{M}x{N}-k384-intsAB-{out}", fam, "fwd", "x3", M, N, (384,), out=out))
        cs.append(Case(f"x3-{M}x{N}-hash", fam, "fwd", "x3", M, N, (64,), "wide", "ints", out="tc", bias=True, relu=True, mask="hash"))
        cs.append(Case(f"x3-{M}x{N}-clamp", fam, "fwd", "x3", M, N, (64,), "ints", "wide", out="tc", bias=True, add="clamp", gate=True))
    cs.append(Case("x3-70x130-k128-allwaves", "x3_fwd_allwaves", "fwd", "x3", 70, 130, (128,), "wide", "ints", out="tc", bias=True, relu=True,
                   mask="ext", hook=("recnn_debug_x3_fwd", 0, -1)))
    # ---- dX: gemm_kernel<DX> and x3_dx_kernel; colsum per 32-row slab
    i = 0
    for dtype, ks in (("fp32", (8, 72, 256)), ("bf16", (8, 72, 256)), ("x3", (32, 96, 256))):
        for M in (1, 33, 70):
            for N, ldb in ((40, 64), (200, 256), (64, 64)):
                for k in ks:
                    i += 1
                    a, b = lat(dtype, i)
                    cs.append(Case(f"dx-{dtype}-{M}x{N}-k{k}", "x3_dx" if dtype == "x3" else "gemm_dx", "dx", dtype, M, N, (k,), a, b,
                                   out="tc" if i % 2 else "f32", gate=i % 5 != 0, ldb=ldb, colsum=True))
    for dtype in ("fp32", "bf16"):   # 64-row tiles (>= 512 of 64 x 64) and their conditional second slab
        cs.append(Case(f"dx-{dtype}-2081x1024-k64", "gemm_dx_64", "dx", dtype, 2081, 1024, (64,), *lat(dtype, 0), out="tc", gate=True, ldb=1024,
                       colsum=True))
    # ---- dW: fp32 generic, bf16 with fp32 B (generic), bf16 both operands (gemm_dw_dma_kernel), split-bf16
    i = 0
    for form, dtype, fam in (("fp32", "fp32", "gemm_dw"), ("b32", "bf16", "gemm_dw"), ("bf16", "bf16", "dw_dma"), ("x3", "x3", "x3_dw")):
        for rows in (1, 31, 65, 333):
            for M, N in ((16, 27), (130, 200)):
                for splits in (1, 2, 16):
                    i += 1
                    a, b = lat(dtype, i)
                    cs.append(Case(f"dw-{form}-r{rows}-{M}x{N}-s{splits}", fam, "dw", dtype, M, N, (rows,), a, b, b_f32=form == "b32",
                                   splits=splits, valid=N if i % 3 else N - 3, rot=5 if i % 2 else 0, pad=64 if i % 4 == 0 else 0))
    for form, dtype in (("fp32", "fp32"), ("b32", "bf16")):   # >= 512 tiles x splits: the 64 x 64 variant of the generic kernel
        cs.append(Case(f"dw-{form}-r333-450x500-s8", "gemm_dw_64", "dw", dtype, 450, 500, (333,), *lat(dtype, 0), b_f32=form == "b32", splits=8,
                       valid=497, rot=5))
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _build()
