"""mlp_frozen_kernel (csrc/mlpf.hip) on its own, through recnn_debug_frozen_forward (csrc/recnn_hip_debug.h), and once more through the
engine.  The kernel's epilogues and output stage take the mask mode, the presence of an addend and a full 128-column output as uniform
branches; the engine reaches only some of their combinations and always gives layer 1 21 or 23 slabs.

(a) directly: segment lists that give 2, 2, 3, 4 and 23 layer-1 slabs -- a third slab exists or not, a boundary between contraction
    segments at every slab -- on a single panel, a ragged last panel and two panels, for an actor with hash masks, an actor with a
    clipped addend, a plain actor and a critic.  The 64-row and the 128-row workgroup forms compute every output element by the same
    arithmetic, so their outputs are equal BIT FOR BIT.  The float64 reference of the kernel is tests/test_gpu_frozen_exact.py (lattice
    operands, every stored stage equal bit for bit); this file remains the test of form against form on ordinary random operands,
    where the cases also check that an option changes what it must change (masks, the addend, the first stored row), that a narrow output equals the
    matching columns of a full one, and that what lies beyond out_dim or below the first stored row is never written.
(b) through the engine on the shapes of tests/test_gpu_frozen_window.py (128 rows per batch, users of 11-14 items, policy period 3,
    run(7) from step 5 = segments of 2 + 3 + 2, all batched: cycle_min_seg 2), 128-row and 64-row workgroups (frozen_half 0 | 1):
    equal to each other bit for bit, and to the eager step loop -- which runs on other kernels -- in the parameters bit for bit and in
    the losses to that test's 1e-5 summation-order bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_frozen_window as FW

pytestmark = pytest.mark.gpu

H, OUT = 256, 128
SEGMENTS = [(128,), (64, 64), (64, 64, 64), (64, 64, 64, 64), (1152, 128, 64, 128)]
ROWS = (64, 130, 256)          # a single panel (half a 128-row one), a ragged last panel, two 128-row panels
SENTINEL = 7.25                # exactly representable in bf16


def _bf(t):
    return t.to(torch.bfloat16).contiguous()


class _Net:
    """Weights and inputs of one case, made once; the segments of layer 1 live in arrays of their own, with pitches wider than K."""

    def __init__(self, cuda, segs, rows, seed):
        g = torch.Generator().manual_seed(seed)
        k1 = sum(segs)
        self.segs, self.rows = segs, rows
        self.A = [_bf(torch.randn(rows, k + 8 * (i + 1), generator=g)).to(cuda) for i, k in enumerate(segs)]
        # the segments' W1 columns in reverse order: every w1_col differs from the running k
        cols, c = [], k1
        for k in segs:
            c -= k
            cols.append(c)
        self.w1_col = cols
        self.W1 = _bf(torch.randn(H, k1 + 8, generator=g) * (1.0 / k1 ** 0.5)).to(cuda)
        self.W2 = _bf(torch.randn(H, H, generator=g) * 0.08).to(cuda)
        self.W3 = _bf(torch.randn(OUT, H, generator=g) * 0.1).to(cuda)
        self.b1 = (torch.randn(H, generator=g) * 0.1).to(cuda)
        self.b2 = (torch.randn(H, generator=g) * 0.1).to(cuda)
        self.b3 = (torch.randn(OUT, generator=g) * 0.3).to(cuda)
        self.w3row = (torch.randn(H, generator=g) * 0.1).to(cuda)
        self.addend = (torch.randn(rows, OUT + 4, generator=g) * 0.5).to(cuda)


def _forward(net, kind, panel_rows, *, out_dim=OUT, store_row0=0, acts=True, rows_per_set=0, hidden=H, add_clip=0.3, masks=None, add=None, ldh=H):
    """One launch; returns {"out" | "q", "h1", "h2"} as CPU tensors.  kind: "actor_hash", "actor_add", "actor_plain", "critic".
    (tests/test_gpu_frozen_exact.py drives the same plumbing with `hidden`, `add_clip`, a pitch `ldh` of the stored activations and
    `masks` / `add` that override what the kind implies.)"""
    masks = kind == "actor_hash" if masks is None else masks
    add = kind == "actor_add" if add is None else add
    from recnn_amd import _lib as L
    lib = L.load()
    dev = net.W1.device
    a = L.FrozenDebugArgs()
    for i, k in enumerate(net.segs):
        a.A[i], a.lda[i], a.K[i], a.w1_col[i] = net.A[i].data_ptr(), net.A[i].stride(0), k, net.w1_col[i]
    a.nseg = len(net.segs)
    a.W1, a.ldw1, a.W2, a.ldw2 = net.W1.data_ptr(), net.W1.stride(0), net.W2.data_ptr(), net.W2.stride(0)
    a.b1, a.b2, a.b3 = net.b1.data_ptr(), net.b2.data_ptr(), net.b3.data_ptr()
    a.rows, a.H, a.out_dim = net.rows, hidden, out_dim
    a.mask_mode = L.MASK_HASH if masks else L.MASK_NONE
    a.seed, a.stream1, a.stream2, a.step, a.rows_per_set = 4711, 2, 3, 5, rows_per_set
    res = {}
    if acts:
        res["h1"] = torch.full((net.rows, ldh), SENTINEL, dtype=torch.bfloat16, device=dev)
        res["h2"] = torch.full((net.rows, ldh), SENTINEL, dtype=torch.bfloat16, device=dev)
        a.h1, a.h2, a.ldh, a.store_row0 = res["h1"].data_ptr(), res["h2"].data_ptr(), ldh, store_row0
    if kind == "critic":
        a.w3row = net.w3row.data_ptr()
        res["q"] = torch.full((net.rows,), SENTINEL, dtype=torch.float32, device=dev)
        a.q = res["q"].data_ptr()
    else:
        a.W3, a.ldw3 = net.W3.data_ptr(), net.W3.stride(0)
        res["out"] = torch.full((net.rows, OUT + 4), SENTINEL, dtype=torch.bfloat16, device=dev)
        a.out, a.ldo = res["out"].data_ptr(), res["out"].stride(0)
        if add:
            a.addend, a.ld_add, a.add_clip = net.addend.data_ptr(), net.addend.stride(0), add_clip
    a.panel_rows = panel_rows
    L.check(lib.recnn_debug_frozen_forward(C.byref(a), C.sizeof(a), None), "recnn_debug_frozen_forward")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def _same(x, y, what):
    assert x.keys() == y.keys()
    for k in x:
        assert torch.equal(x[k], y[k]), (what, k)


@pytest.mark.parametrize("segs", SEGMENTS, ids=lambda s: "x".join(map(str, s)))
def test_panel_forms_agree_bit_for_bit_and_options_do_what_they_must(cuda, segs):
    for rows in ROWS:
        net = _Net(cuda, segs, rows, seed=rows + len(segs))
        got = {}
        for kind in ("actor_hash", "actor_add", "actor_plain", "critic"):
            # batches of 64 rows for the masked actor: the mask step changes inside the problem, for 128-row workgroups inside the panel
            kw = dict(rows_per_set=64) if kind == "actor_hash" else {}
            ref = got[kind] = _forward(net, kind, 128, **kw)
            for k, v in ref.items():
                assert torch.isfinite(v.float()).all() and float(v.float().abs().max()) > 0, (kind, k)
            if "out" in ref:
                assert (ref["out"][:, OUT:] == SENTINEL).all(), "columns beyond out_dim must stay untouched"
            _same(ref, _forward(net, kind, 64, **kw), (segs, rows, kind))
        plain, add, masked = got["actor_plain"], got["actor_add"], got["actor_hash"]
        # the addend changes the output only, by at most the clip; the masks change everything behind layer 1
        _same({k: plain[k] for k in ("h1", "h2")}, {k: add[k] for k in ("h1", "h2")}, "addend")
        diff = (add["out"][:, :OUT].float() - plain["out"][:, :OUT].float()).abs().max()
        top = float(add["out"][:, :OUT].float().abs().max())
        assert 0 < float(diff) <= 0.3 + 2.0 ** -7 * top       # |clip| <= 0.3, and two bf16 roundings of at most half an ulp (2^-8) each
        assert not torch.equal(plain["h1"], masked["h1"]) and float((masked["h1"] == 0).float().mean()) > float((plain["h1"] == 0).float().mean())


def test_first_stored_row_and_narrow_outputs(cuda):
    """store_row0 inside a 128-row panel (and behind a whole 64-row one): rows below it keep the sentinel, rows from it on equal a full
    store; an output of 120 or 124 columns equals those columns of the 128-column output and nothing behind them is stored, with and
    without an addend (the four forms of the output stage); a width that is no multiple of four is refused."""
    from recnn_amd import _lib as L
    net = _Net(cuda, (64, 64, 64), 130, seed=5)
    for panel_rows in (64, 128):
        full = _forward(net, "actor_hash", panel_rows, rows_per_set=64)
        part = _forward(net, "actor_hash", panel_rows, rows_per_set=64, store_row0=72)
        assert torch.equal(full["out"], part["out"])
        for k in ("h1", "h2"):
            assert (part[k][:72] == SENTINEL).all() and torch.equal(part[k][72:], full[k][72:]), (k, panel_rows)
        none = _forward(net, "actor_hash", panel_rows, rows_per_set=64, acts=False)
        assert torch.equal(full["out"], none["out"])
        for kind in ("actor_plain", "actor_add"):
            wide = _forward(net, kind, panel_rows)["out"]
            for od in (120, 124):
                nar = _forward(net, kind, panel_rows, out_dim=od)["out"]
                assert torch.equal(nar[:, :od], wide[:, :od]), (kind, od, panel_rows)
                assert (nar[:, od:] == SENTINEL).all(), "nothing is stored beyond out_dim"
    with pytest.raises(L.RecnnHipError):
        _forward(net, "actor_plain", 128, out_dim=126)


def _run(recnn_amd, cuda, env, algo, half):
    from recnn_amd._tune import set_default_tuning
    set_default_tuning(frozen_half=half, frozen_window=1, cycle_min_len=2, cycle_min_seg=2)
    try:
        a = FW._make(recnn_amd, cuda, env, algo)
        eng = a._fused_ctx.engine
        assert eng.tuning.frozen_half == half and eng.tuning.cycle_min_seg == 2
        _, hist = a.run(FW.FIRST, history=True)
        a.prepare_run(FW.N, first_step=FW.FIRST)           # ONE made-to-order run graph: segments of 2 + 3 + 2 steps, all batched
        _, h = a.run(FW.N, history=True)
        torch.cuda.synchronize()
        out = {"hist": hist + h, "masters": FW._masters(a), "gen_action": FW._cycle_array(eng, "cycle_gen_action"),
               "next_action": [FW._cycle_array(eng, f"cycle_next_action{b}") for b in range(2)],
               "tq": [FW._cycle_array(eng, f"cycle_target_q{c + 1}") for c in range(2 if algo == "td3" else 1)]}
        assert out["gen_action"] is not None and all(t is not None for t in out["tq"] + out["next_action"])
        return out
    finally:
        set_default_tuning(frozen_half=None, frozen_window=None, cycle_min_len=None, cycle_min_seg=None)


@pytest.mark.parametrize("algo", ["ddpg", "td3"])
def test_panel_forms_agree_through_the_engine_and_with_the_eager_loop(cuda, algo):
    import recnn_amd
    env, (lhist, lmasters) = FW._shared(recnn_amd, cuda, algo)
    off = _run(recnn_amd, cuda, env, algo, 0)
    runs = [_run(recnn_amd, cuda, env, algo, 1)]
    for on in runs:
        # ---- 64-row workgroups where they are eligible == 128-row workgroups everywhere, bit for bit
        assert on["hist"] == off["hist"]
        for net, sd in off["masters"].items():
            for k, v in sd.items():
                assert torch.equal(v, on["masters"][net][k]), (net, k)
        assert torch.equal(on["gen_action"], off["gen_action"]) and float(on["gen_action"].float().abs().max()) > 0
        for a, b in zip(on["tq"] + on["next_action"], off["tq"] + off["next_action"]):
            assert torch.equal(a, b)
        assert float(on["next_action"][0].float().abs().max()) > 0
    # ---- == the eager step loop: parameters bit for bit, losses to summation order (the bound of tests/test_gpu_frozen_window.py)
    for on in runs + [off]:
        for net, sd in lmasters.items():
            for k, v in sd.items():
                assert torch.equal(v, on["masters"][net][k]), (net, k)
        keys = ("value1", "value2", "policy") if algo == "td3" else ("value", "policy")
        assert len(on["hist"]) == len(lhist) == FW.FIRST + FW.N
        for x, y in zip(on["hist"], lhist):
            assert x["step"] == y["step"]
            for k in keys:
                assert np.isfinite(x[k]) and abs(x[k] - y[k]) <= 1e-5 * max(abs(y[k]), 1.0), (k, x, y)
