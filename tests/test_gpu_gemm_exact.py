"""recnn_gemm_fwd / recnn_gemm_dx / recnn_gemm_dw against EXACT products at every tile edge, with zero tolerance.

The operands come from the lattices of tests/gemm_exact_reference.py: every partial sum is exactly representable in fp32, so each
kernel family behind the three entry points must equal the float64 product bit for bit whatever its summation order, tile shape,
ring depth or k split.  A lost 16-byte k chunk, a k tail that is not zero filled, a ring stage skipped or read twice, a short
split-K slice, a narrowed operand or accumulator, a dropout word indexed by the wrong row: each moves some output by at least
one unit of the lattice, and the comparison is `torch.equal`.

Every output (C, column sums, dW slabs) is allocated with a pitch wider than N and one row more than M and prefilled with a NaN
sentinel; after the call the sentinel must still stand everywhere outside [M, N].  Operand padding (columns past K of the
k-contiguous operands, columns past N / M of the k-strided ones) holds NaN: nothing read there may reach a stored output.
"""
import ctypes as C
import functools

import pytest
import torch

from tests import gemm_exact_reference as R
from tests.helpers import x3_cols, x3_pack_ref

pytestmark = pytest.mark.gpu

SENT32 = 0x7FC05A5A         # a NaN fp32 pattern
SENT16 = 0x7FC1             # a NaN bf16 pattern
NAN = float("nan")


def _lib():
    from recnn_amd import _lib as L
    L.load()
    return L


def _r(x, m):
    return (x + m - 1) // m * m


def _x3_ld(n):
    return 2 * _r(n, 32)


def _plain(t, f32, ld, fill=NAN):
    """float64 [R, C] -> fp32 / bf16 [R, ld] on the host, the padding columns holding `fill`"""
    out = torch.full((t.shape[0], ld), fill, dtype=torch.float32)
    out[:, :t.shape[1]] = t.float()
    return out if f32 else out.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ operands on the device
@functools.lru_cache(maxsize=2)
def _dev_operands(key):
    case = key
    dev = torch.device("cuda")
    a, b, _ = R.operands(case)
    x3 = case.dtype == "x3"
    fa = case.dtype == "fp32" or case.a_f32
    fb = case.dtype == "fp32" or case.b_f32
    A, B, lda, ldb = [], [], [], []
    for ta, tb in zip(a, b):
        if case.op == "dw":
            wa, wb = _r(case.M, 64) + case.pad, _r(case.N, 64) + case.pad
        else:
            wa = ta.shape[1] + (32 if x3 else 8)                     # k contiguous: any pitch >= K
            wb = tb.shape[1] + (32 if x3 else 8) if case.op == "fwd" else case.ldb
        A.append((x3_pack_ref(ta.float(), 2 * wa) if x3 else _plain(ta, fa, wa)).to(dev))
        B.append((x3_pack_ref(tb.float(), 2 * wb) if x3 else _plain(tb, fb, wb)).to(dev))
        lda.append(2 * wa if x3 else wa)
        ldb.append(2 * wb if x3 else wb)
    return A, B, lda, ldb


def _operand_key(case):
    """the fields the device operands depend on (cases that differ only in their epilogue share them)"""
    return R.Case("", "", case.op, case.dtype, case.M, case.N, case.K, case.a_lat, case.b_lat, a_f32=case.a_f32, b_f32=case.b_f32,
                  ldb=case.ldb, pad=case.pad)


@functools.lru_cache(maxsize=2)
def _dev_epilogue(M, N, dtype):
    dev = torch.device("cuda")
    e = R.epilogue_operands(M, N)
    ld4, ld1 = _r(N, 4) + 4, N + 1
    d = dict(bias=e["bias"].to(dev))
    # two pitches each: 16-byte friendly rows (the vector loads of the wave-specialised epilogues) and odd ones (their scalar paths)
    for name, t in (("addend", e["addend"]), ("mask", e["mask"])):
        for ld in (ld4, ld1):
            buf = torch.zeros((M, ld), dtype=t.dtype)
            buf[:, :N] = t
            d[name, ld % 4 == 0] = (buf.to(dev), ld)
    if dtype == "x3":
        y = x3_pack_ref(e["yref"])
        d["yref"] = (y.to(dev), y.shape[1])
    else:
        d["yref"] = (_plain(e["yref"].double(), dtype == "fp32", ld1, fill=1.0).to(dev), ld1)
    d["step"] = torch.tensor([R.HASH_KEY[1]], dtype=torch.int32, device=dev)
    return d


@functools.lru_cache(maxsize=2)
def _hash_mask(M, N):
    L = _lib()
    out = torch.zeros(M, N, dtype=torch.uint8, device="cuda")
    seed, step, stream = R.HASH_KEY
    L.call("recnn_hash_mask_dump", seed, step, stream, M, N, L.ptr(out), L.current_stream())
    torch.cuda.synchronize()
    return out.cpu()


# ------------------------------------------------------------------------------------------------ outputs with sentinels
def _sentinel(rows, ld, kind):
    """[rows, ld] of the NaN sentinel on the device: fp32 ('f32') or bf16 ('bf16' / 'x3')"""
    if kind == "f32":
        return torch.full((rows, ld), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full((rows, ld), SENT16, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _check(buf, want, kind, what):
    """`want` ([M, N] in the output type; split rows: [M, x3_ld(N)] with the logical width in `kind`) inside, the sentinel outside"""
    got = buf.cpu()
    M = want.shape[0]
    if isinstance(kind, tuple):        # ("x3", N): the hi / lo columns of the N logical ones
        cols = x3_cols(kind[1])
        cols = torch.cat([cols, cols + 32])
        bits, wbits, sent = got.view(torch.int16).clone(), want.view(torch.int16), SENT16
        inside = bits[:M][:, cols]
        assert torch.equal(inside, wbits[:, cols]), (what, int((inside != wbits[:, cols]).sum()))
        bits[:M, cols] = sent
    else:
        N = want.shape[1]
        inside = got[:M, :N]
        if kind == "f32":
            assert torch.equal(inside, want), (what, _first_bad(inside, want))
            bits, sent = got.view(torch.int32).clone(), SENT32
        else:
            bits, sent = got.view(torch.int16).clone(), SENT16
            assert torch.equal(bits[:M, :N], want.view(torch.int16)), (what, _first_bad(inside.float(), want.float()))
        bits[:M, :N] = sent
    bad = (bits != sent).nonzero()
    assert bad.numel() == 0, (what, "written outside [M, N] at", bad[:4].tolist())


def _first_bad(got, want):
    bad = (got != want).nonzero()
    r, c = bad[0].tolist()
    return dict(mismatches=int(bad.shape[0]), first=(r, c), got=float(got[r, c]), want=float(want[r, c]))


def _out_kind(case):
    if case.out == "f32" or case.dtype == "fp32":
        return "f32"
    return "bf16" if case.dtype == "bf16" else "x3"


def _args(L, case):
    a = L.GemmArgs()
    C.memset(C.byref(a), 0, C.sizeof(a))
    a.dtype = {"fp32": L.F32, "bf16": L.BF16, "x3": L.BF16X3}[case.dtype]
    a.M, a.N = case.M, case.N
    a.dx_scale = 1.0
    a.dw_splits = 1
    return a


def _set_operands(a, case, ops):
    A, B, lda, ldb = ops
    phys = 2 if case.dtype == "x3" and case.op != "dw" else 1      # split rows: K counts physical columns
    for s in range(len(A)):
        a.A[s], a.B[s], a.lda[s], a.ldb[s], a.K[s] = A[s].data_ptr(), B[s].data_ptr(), lda[s], ldb[s], phys * case.K[s]
        a.a_f32[s], a.b_f32[s] = int(case.a_f32), int(case.b_f32)


def _run(L, entry, a, case):
    lib = L.load()
    try:
        if case.hook:
            getattr(lib, case.hook[0])(case.hook[1])
        L.call(entry, C.byref(a), L.current_stream())
        torch.cuda.synchronize()
    finally:
        if case.hook:
            getattr(lib, case.hook[0])(case.hook[2])


def _ids(op):
    return dict(argvalues=[c for c in R.CASES if c.op == op], ids=lambda c: c.id)


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("case", **_ids("fwd"))
def test_fwd_equals_the_float64_product(cuda, case):
    L = _lib()
    M, N = case.M, case.N
    ops = _dev_operands(_operand_key(case))
    kind = _out_kind(case)
    ldc = case.ldc or (_x3_ld(N) + 64 if kind == "x3" else _r(N, 8) + 8)
    out = _sentinel(M + 1, ldc, kind)
    a = _args(L, case)
    _set_operands(a, case, ops)
    a.C, a.ldc, a.c_f32 = out.data_ptr(), ldc, int(case.out == "f32")
    e = _dev_epilogue(M, N, case.dtype)
    vec = case.bias                       # (an arbitrary but fixed choice of which cases take the 16-byte friendly pitches)
    if case.bias:
        a.bias = e["bias"].data_ptr()
    a.relu = int(case.relu)
    if case.add != "none":
        t, ld = e["addend", vec]
        a.addend, a.ld_add = t.data_ptr(), ld
        a.add_clip = float("inf") if case.add == "inf" else R.ADD_CLIP
        a.add_row_div = 3 if case.add == "div3" else 0
    if case.gate:
        t, ld = e["yref"]
        a.yref, a.ldy, a.dx_scale = t.data_ptr(), ld, case.scale
    hash_mask = None
    if case.mask == "ext":
        t, ld = e["mask", not vec]
        a.mask_mode, a.mask, a.ld_mask = L.MASK_EXTERNAL, t.data_ptr(), ld
    elif case.mask == "hash":
        assert M % 4 and N % 4
        hash_mask = _hash_mask(M, N)
        a.mask_mode, a.seed, a.stream_id, a.step_ptr = L.MASK_HASH, R.HASH_KEY[0], R.HASH_KEY[2], e["step"].data_ptr()
    ws = None
    if case.ws != "none":
        ws = torch.empty((8 if case.ws == "fit" else 2) * M * N, device=cuda)
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    _run(L, "recnn_gemm_fwd", a, case)
    want = R.to_output(R.reference(case, hash_mask), case)
    _check(out, want, ("x3", N) if kind == "x3" else kind, case.id)


# ------------------------------------------------------------------------------------------------ dX
@pytest.mark.parametrize("case", **_ids("dx"))
def test_dx_equals_the_float64_product(cuda, case):
    L = _lib()
    M, N = case.M, case.N
    ops = _dev_operands(_operand_key(case))
    kind = _out_kind(case)
    ldc = _x3_ld(N) + 64 if kind == "x3" else _r(N, 8) + 8
    out = _sentinel(M + 1, ldc, kind)
    slabs = (M + 31) // 32
    colsum = _sentinel(slabs + 1, N, "f32")
    a = _args(L, case)
    _set_operands(a, case, ops)
    a.C, a.ldc, a.c_f32 = out.data_ptr(), ldc, int(case.out == "f32")
    a.dx_scale, a.colsum = case.scale, colsum.data_ptr()
    if case.gate:
        t, ld = _dev_epilogue(M, N, case.dtype)["yref"]
        a.yref, a.ldy = t.data_ptr(), ld
    _run(L, "recnn_gemm_dx", a, case)
    ref = R.reference(case)
    _check(out, R.to_output(ref, case), ("x3", N) if kind == "x3" else kind, case.id)
    # the column sums are taken over the fp32 values before the output type, per 32-row slab, the ragged last slab included
    _check(colsum, R.colsum_reference(ref).float(), "f32", (case.id, "colsum"))


# ------------------------------------------------------------------------------------------------ dW
@pytest.mark.parametrize("case", **_ids("dw"))
def test_dw_slabs_sum_to_the_float64_product(cuda, case):
    L = _lib()
    M, N = case.M, case.N
    valid = case.valid or N
    ops = _dev_operands(_operand_key(case))
    ldc = valid + 1
    stride = (M + 1) * ldc
    slabs = _sentinel(case.splits * (M + 1), ldc, "f32")
    a = _args(L, case)
    _set_operands(a, case, ops)
    a.C, a.ldc = slabs.data_ptr(), ldc
    a.dw_splits, a.dw_slab_stride, a.dw_valid_cols, a.dw_col_rot = case.splits, stride, valid, case.rot
    _run(L, "recnn_gemm_dw", a, case)
    got = slabs.cpu().view(case.splits, M + 1, ldc)
    inside = got[:, :M, :valid]
    assert not torch.isnan(inside).any(), (case.id, "a slab (one with an empty k range?) was not written")
    ref = R.reference(case)
    assert torch.equal(inside.double().sum(0), ref), (case.id, _first_bad(inside.double().sum(0), ref))
    bits = got.view(torch.int32).clone()
    bits[:, :M, :valid] = SENT32
    assert bool((bits == SENT32).all()), (case.id, "written outside [M, valid columns]")


# ------------------------------------------------------------------------------------------------ the pitch contract
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("op,M,N,lda,ldb", [("dx", 8, 40, 8, 40), ("dx", 8, 200, 8, 200), ("dw", 16, 64, 16, 64), ("dw", 64, 40, 64, 40),
                                            ("dw", 130, 200, 192, 200)])
def test_short_pitch_of_a_k_strided_operand_is_refused(cuda, dtype, op, M, N, lda, ldb):
    """B of dX and both operands of dW are read in whole 64-column tiles on every k row (include/recnn_hip.h recnn_gemm_args): a
    pitch below roundup(., 64) is RECNN_E_INVALID with a message, and nothing is launched (the output keeps its sentinel)."""
    L = _lib()
    lib = L.load()
    rows = 8
    tdt = torch.float32 if dtype == "fp32" else torch.bfloat16
    A = torch.zeros(rows * 256, dtype=tdt, device=cuda)          # (room for any of the pitches: nothing reads them anyway)
    B = torch.zeros(rows * 256, dtype=tdt, device=cuda)
    out = _sentinel(M, N, "f32")
    a = L.GemmArgs()
    C.memset(C.byref(a), 0, C.sizeof(a))
    a.dtype, a.M, a.N, a.dx_scale, a.dw_splits = (L.F32 if dtype == "fp32" else L.BF16), M, N, 1.0, 1
    a.A[0], a.B[0], a.lda[0], a.ldb[0], a.K[0] = A.data_ptr(), B.data_ptr(), lda, ldb, rows
    a.C, a.ldc, a.c_f32 = out.data_ptr(), N, 1
    a.dw_slab_stride, a.dw_valid_cols = M * N, N
    rc = getattr(lib, "recnn_gemm_" + op)(C.byref(a), L.current_stream())
    torch.cuda.synchronize()
    assert rc == -1, rc                                         # RECNN_E_INVALID
    msg = lib.recnn_last_error().decode()
    assert "pitch below the tile width" in msg and f"gemm {op}" in msg, msg
    assert bool((out.cpu().view(torch.int32) == SENT32).all())
    # the smallest pitches the contract allows are accepted
    a.lda[0] = _r(M, 64) if op == "dw" else lda
    a.ldb[0] = _r(N, 64)
    L.call("recnn_gemm_" + op, C.byref(a), L.current_stream())
    torch.cuda.synchronize()
    assert bool((out.cpu() == 0).all())
