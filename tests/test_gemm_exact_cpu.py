"""The exact-product GEMM cases (tests/gemm_exact_reference.py) checked on the CPU: the premises the GPU tests rest on.

For every case of the table: the operands survive their memory type unchanged, the span sum_k |a||b| / lsb stays below 2^22, the
fp32 product on the CPU already equals the float64 one (so any summation order does), and a wide operand never meets another.
Per kernel family at least one case has outputs above 256 in magnitude that bf16 cannot hold, in an output type that keeps
them: an accumulator narrower than fp32 would fail there.
"""
import pytest
import torch

from tests import gemm_exact_reference as R
from tests.helpers import x3_value

# the nine kernel families behind the three entry points (tile / ring variants of one kernel share a family)
FAMILY = {"gemm_fwd": "gemm_kernel FWD", "gemm_fwd_64": "gemm_kernel FWD", "gemm_fwd_a32": "gemm_kernel FWD",
          "gemm_dx": "gemm_kernel DX", "gemm_dx_64": "gemm_kernel DX", "gemm_dw": "gemm_kernel DW", "gemm_dw_64": "gemm_kernel DW",
          "dma5": "LDS-DMA ring", "dma3": "LDS-DMA ring", "wide": "wide 128 x 128", "tall": "tall 256 x 128", "splitk": "split-K",
          "dw_dma": "gemm_dw_dma_kernel", "x3_fwd_5": "split-bf16 forward", "x3_fwd_3": "split-bf16 forward",
          "x3_fwd_big": "split-bf16 forward", "x3_fwd_allwaves": "split-bf16 forward", "x3_dx": "x3_dx_kernel", "x3_dw": "x3_dw_kernel"}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_case_is_exact(case):
    a, b, prod = R.operands(case)
    assert not (case.a_lat == "wide" and case.b_lat == "wide")
    assert case.dtype != "bf16" or (case.a_lat, case.b_lat) == ("ints", "ints")
    for which, segs in (("a", a), ("b", b)):
        for t in segs:
            m = R.memory_type(t, case, which)
            assert torch.equal(m.double(), t)                   # the memory type holds the lattice
            if case.dtype == "x3":
                assert torch.equal(x3_value(m).double(), t)       # ... and so do hi + lo of a split row
    s = R.span(case)
    assert s < R.SPAN_LIMIT, s
    mul = {"fwd": lambda x, y: x @ y.t(), "dx": lambda x, y: x @ y, "dw": lambda x, y: x.t() @ y}[case.op]
    acc = torch.zeros(prod.shape)
    for x, y in zip(a, b):
        acc = acc + mul(x.float(), y.float())
    assert torch.equal(acc.double(), prod)
    # the epilogue keeps every value a multiple of lsb / 2 below 2^24 of them, and the reference in the output type is finite
    mask = R.epilogue_operands(case.M, case.N)["mask"] if case.mask == "hash" else None
    ref = R.reference(case, mask)
    assert torch.equal(ref.float().double(), ref)
    if case.colsum:     # 32 values of one column are added in plain fp32 (no matrix unit): 2^24 is the bound
        cs = R.colsum_reference(ref)
        lsb = R.LSB[case.a_lat] * R.LSB[case.b_lat] * min(case.scale, 1.0)
        assert float(R.colsum_reference(ref.abs()).max()) / lsb < 2 ** 24
        assert torch.equal(cs.float().double(), cs)


def test_every_case_belongs_to_a_family_and_every_family_has_cases():
    assert {c.family for c in R.CASES} == set(FAMILY)


@pytest.mark.parametrize("family", sorted(set(FAMILY.values())))
def test_family_has_outputs_a_narrow_accumulator_would_lose(family):
    for case in R.CASES:
        if FAMILY[case.family] != family or (case.dtype == "bf16" and case.out == "tc"):
            continue
        if max(case.K) < 16:
            continue
        ref = R.reference(case, R.epilogue_operands(case.M, case.N)["mask"] if case.mask == "hash" else None)
        big = ref[ref.abs() > 256]
        if big.numel() and bool((big.float().bfloat16().double() != big).any()):
            return
    pytest.fail(f"no case of {family} has |C| > 256 outside bf16 in an fp32 or split output")
