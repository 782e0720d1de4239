"""mlp_frozen_kernel (csrc/mlpf.hip) against the float64 network, BIT FOR BIT, through recnn_debug_frozen_forward.

The operands come from the lattice of tests/mlp_exact_reference.py: every partial sum of every layer is exact in fp32 and every
activation stored as bf16 between two layers is representable, so both workgroup forms must equal the float64 reference at h1, h2
and out (bf16) and at q (fp32) whatever their summation order.  tests/test_gpu_frozen_direct.py compares the two forms with each
other; a defect they share -- a slab dropped when a third one exists, a w1_col applied a segment late, a bias group four columns
off, a mask word indexed by the wrong row -- moves some element here by at least one unit of the lattice
(tests/test_mlp_exact_cpu.py shows that for every slab of every case), and the comparison is equality of the bits.

Cases (mlp_exact_reference.CASES): 2, 2, 3, 4 and 23 layer-1 slabs with w1_col in reverse order and segments in allocations of their
own with pitches wider than K x 64, 130 and 256 rows x {plain actor, actor with a clipped addend, critic, actor with hash masks in
batches of 64 rows}; hash masks in batches of 32 rows, as one batch and next to an addend; a first stored row inside a 128-row
panel / behind a whole 64-row one / on a panel edge / at the end; outputs of 4, 120, 124 and 128 columns with and without an addend;
hidden widths 8, 64, 200 and 256 with weights of 256 rows whose padding holds non-zero lattice values.  Every case runs in the 128-row
and in the 64-row form.

Outputs are prefilled with a sentinel: h1 / h2 [rows, 264] keep it in rows below store_row0 and in columns 256 .. 263 (the kernel
stores all 256 columns of a row, +0 at and beyond H), out [rows, 132] keeps it from out_dim on.

The keep masks of a hash case come from recnn_hash_mask_dump, once per batch j with step + j and stream1 | stream2, indexed by the
row WITHIN the batch: hidden_epilogue (mlp_panel.h) is called with m0 = the sub-panel's first row minus its batch's first row and
takes mask_word(key, m >> 2, n0 >> 2), mask_keep(word, m & 3, r) -- hash_mask_dump_kernel's expression with its own row index.  The
admissibility of the case is asserted again under these masks before anything is compared."""
import functools

import pytest
import torch

import test_gpu_frozen_direct as D
from tests import mlp_exact_reference as R

pytestmark = pytest.mark.gpu

LDH = R.HP + 8
SEED, STREAM1, STREAM2, STEP = 4711, 2, 3, 5     # what test_gpu_frozen_direct._forward passes


class _DevNet:
    """The float64 operands of a case on the device in the kernel's types (the attributes test_gpu_frozen_direct._forward reads)"""

    def __init__(self, n, dev):
        bf = lambda t: t.to(torch.bfloat16).contiguous().to(dev)
        f32 = lambda t: t.float().contiguous().to(dev)
        self.segs, self.rows, self.w1_col = n["segs"], n["rows"], n["w1_col"]
        self.A = [bf(a) for a in n["A"]]
        self.W1, self.W2, self.W3 = bf(n["W1"]), bf(n["W2"]), bf(n["W3"])
        self.b1, self.b2, self.w3row = f32(n["b1"]), f32(n["b2"]), f32(n["w3row"])


@functools.lru_cache(maxsize=2)
def _dev_net(segs, rows, H):
    return _DevNet(R._net(segs, rows, H), torch.device("cuda"))


def _keep_masks(case):
    """([rows, 256] keep masks of layer 1 and layer 2) as the kernel draws them"""
    from recnn_amd import _lib as L
    L.load()
    keep = [torch.zeros(case.rows, R.HP, dtype=torch.uint8) for _ in range(2)]
    per_set = case.rows_per_set or case.rows
    for j, (r0, nr) in enumerate(R.set_masks(case)):
        for k, stream in zip(keep, (STREAM1, STREAM2)):
            out = torch.zeros(per_set, R.HP, dtype=torch.uint8, device="cuda")
            L.call("recnn_hash_mask_dump", SEED, STEP + j, stream, per_set, R.HP, L.ptr(out), L.current_stream())
            torch.cuda.synchronize()
            k[r0:r0 + nr] = out.cpu()[:nr]
    return keep


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_frozen_network_equals_float64(cuda, case):
    n = R.net(case)
    net = _dev_net(case.segs, case.rows, case.H)
    net.b3 = n["b3"].float().to(cuda)
    net.addend = n["addend"].float().contiguous().to(cuda)
    keep = _keep_masks(case) if case.masked else (None, None)
    if case.masked:
        assert 0.3 < float(keep[0].float().mean()) < 0.7 and not torch.equal(keep[0], keep[1])
        if case.rows_per_set:
            rps = case.rows_per_set
            assert not torch.equal(keep[0][:32], keep[0][rps:rps + 32]), "batches draw masks of their own"
    ref, spans = R.reference(n, case, *keep)
    assert R.inadmissible(ref, spans) == {}, "the case is not exact under the masks the kernel draws"

    want = {}
    for k in ("h1", "h2"):
        w = torch.full((case.rows, LDH), D.SENTINEL, dtype=torch.bfloat16)
        w[case.store_row0:, :R.HP] = ref[k][case.store_row0:].float().to(torch.bfloat16)
        want[k] = w
    if case.critic:
        want["q"] = ref["q"].float()
    else:
        w = torch.full((case.rows, D.OUT + 4), D.SENTINEL, dtype=torch.bfloat16)
        w[:, :case.out_dim] = ref["out"].float().to(torch.bfloat16)
        want["out"] = w

    for panel_rows in (128, 64):
        got = D._forward(net, case.kind, panel_rows, out_dim=case.out_dim, store_row0=case.store_row0, rows_per_set=case.rows_per_set,
                         hidden=case.H, add_clip=case.add_clip, masks=case.masked, add=case.add, ldh=LDH)
        assert got.keys() == want.keys()
        for k, w in want.items():
            g = got[k]
            assert g.dtype == w.dtype and g.shape == w.shape
            if not torch.equal(_bits(g), _bits(w)):
                bad = (_bits(g) != _bits(w)).nonzero()
                i = tuple(int(x) for x in bad[0])
                raise AssertionError(f"{case.id} panel_rows={panel_rows} {k}: {len(bad)} of {w.numel()} elements differ, first at {i}: "
                                     f"got {float(g[i])}, want {float(w[i])}")


def test_short_pitches_are_refused(cuda):
    """the kernel stores 256 columns of every activation row and streams 256 columns of W2 / W3 whatever H: pitches below that are refused"""
    from recnn_amd import _lib as L
    case = next(c for c in R.CASES if c.id == "64x64x64-r130-critic-H64")
    n = R.net(case)
    net = _dev_net(case.segs, case.rows, case.H)
    net.b3 = n["b3"].float().to(cuda)
    with pytest.raises(L.RecnnHipError):
        D._forward(net, "critic", 128, hidden=64, ldh=64)
    narrow = _DevNet(R._net(case.segs, case.rows, case.H), cuda)
    narrow.b3 = net.b3
    narrow.W2 = narrow.W2[:, :128].contiguous()           # (never launched: refused by the check)
    with pytest.raises(L.RecnnHipError):
        D._forward(narrow, "critic", 128, hidden=64, ldh=LDH)
