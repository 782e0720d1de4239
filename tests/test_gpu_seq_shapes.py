"""The LSTM encode, its backward through time and the weight-gradient launches (csrc/lstm.hip, csrc/seq_chain.h, csrc/seq_bwd.h, csrc/seq_grad.h) at the
shapes BETWEEN the two ends tests/test_gpu_seq.py and tests/test_gpu_seq_grad.py run at: every instantiation and masking path the
kernels take as (E, H), U and T move through their tiles.

  (E, H)       what it reaches
  (24, 48)     two k blocks of E with the last half empty; 3 hidden tiles, five idle waves
  (16, 128)    no empty half; 8 tiles, all waves on in the one-tile-per-wave kernels; 66,048 B of backward LDS; dW_hh of two full tiles
  (40, 96)     the first H whose backward LDS passes 48 KiB (49,664 B) on the one-tile kernel; dW_hh's second tile 32 wide
  (72, 144)    two tiles per wave with only wave 0 owning a second; dW_hh's third tile 16 wide, dW_ih's second 8 wide; 9 row tiles
  (120, 240)   two tiles per wave with wave 7's second off; E's last k block half empty at the top of the stager; dW_ih's second 56 wide

  (U, T, state)       what it reaches
  (33, 70, h0 set)    three user tiles, the last with one live row; chunks of 32 + 32 + 6 (a middle chunk reads dh_in and accumulates)
  (16, 32, zero)      exactly one tile, exactly one chunk
  (17, 65, zero)      a last chunk of one step

References and bounds are those of the two neighbouring files, unchanged (seq_reference.fp32_bound: 4 max |fp32 CPU - fp64 CPU| floored
at 1e-6; seq_grad_reference.grad_bounds: max(4 max |G32cpu - G64cpu|, 2^-23 max(8, sqrt(U T)) max |G64|)).  Before anything is compared
every case asserts from the float64 reference alone that the regions an indexing slip would hit carry signal: the last 16 columns of
dW_hh, the last 8 columns of dW_ih before the rating column, the rating column and the last 16 hidden units of h each hold a value of at
least 100 times the bound of their tensor.  Every test prints its measured error next to the bound before it asserts."""
import numpy as np
import pytest
import torch

import seq_grad_reference as G
import seq_reference as R
from helpers import make_store
from test_gpu_seq_grad import _check, _gpu_grads, _h0c0, _on_gpu

pytestmark = pytest.mark.gpu

N_USERS = 35
SHAPES, CASES = R.SWEEP_SHAPES, R.SWEEP_CASES                        # (E, H); (U, T, h0 / c0 set)
SIGNAL = 100.0


@pytest.fixture(scope="module")
def seq_data():
    """Per (E, H): 35 users with at least 71 elements, their table and an LSTM(E + 1, H) (CPU master copies)."""
    out = {}
    for E, H in SHAPES:
        items, ratings, table = make_store(N_USERS, 300, E, 71, 79, seed=E)
        torch.manual_seed(E)
        out[(E, H)] = (items, ratings, torch.from_numpy(table), torch.nn.LSTM(E + 1, H))
    return out


@pytest.fixture(scope="module")
def references():
    """Float64 / float32 CPU results, gradients and bounds, computed once per case and shared (never modified)."""
    return {}


def _slots(U):
    return np.arange(N_USERS - U, N_USERS, dtype=np.int32)          # from the end of the store: slots are looked up, not assumed


def edge_signal(E, fwd_bounds, ref, bounds, g64):
    """{region: max |float64| / bound of its tensor} for the regions only the in-between shapes' last tiles reach."""
    return {"dW_hh last 16 columns": float(g64["weight_hh_l0"][:, -16:].abs().max()) / bounds["weight_hh_l0"],
            "dW_ih last 8 columns before the rating": float(g64["weight_ih_l0"][:, E - 8:E].abs().max()) / bounds["weight_ih_l0"],
            "dW_ih rating column": float(g64["weight_ih_l0"][:, E].abs().max()) / bounds["weight_ih_l0"],
            "h last 16 hidden units": float(ref[0][..., -16:].abs().max()) / fwd_bounds[0]}


def reference_case(data, EH, case):
    """(h0c0, loss weights, forward bounds, float64 forward, gradient bounds, float64 gradients) of one case, from the CPU alone."""
    items, ratings, table, lstm = data
    U, T, with_h0 = case
    slots = _slots(U)
    x = R.lstm_inputs(table, [items[s] for s in slots], [ratings[s] for s in slots], T)
    hc = _h0c0(U, EH[1], U) if with_h0 else None
    Rw = G.loss_weights(U, T, EH[1], seed=T + U)
    fwd_bounds, ref = R.fp32_bound(lstm, x, hc)
    bounds, g64 = G.grad_bounds(lstm, x, hc, Rw, "all")
    return hc, Rw, fwd_bounds, ref, bounds, g64


def _reference(references, seq_data, EH, case):
    key = (EH, case)
    if key not in references:
        references[key] = reference_case(seq_data[EH], EH, case)
    hc, Rw, fwd_bounds, ref, bounds, g64 = references[key]
    signal = edge_signal(EH[0], fwd_bounds, ref, bounds, g64)
    print(f"signal E,H={EH} U,T,h0={case}: " + ", ".join(f"{k} {v:.3g} x bound" for k, v in signal.items()))
    assert all(v >= SIGNAL for v in signal.values()), (EH, case, signal)
    return references[key]


def _tag(EH, case):
    return f"E,H={EH} U={case[0]} T={case[1]} h0={'set' if case[2] else 'zero'}"


# ---------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"U{c[0]}-T{c[1]}")
@pytest.mark.parametrize("EH", SHAPES, ids=lambda s: f"E{s[0]}-H{s[1]}")
def test_encode_against_float64(cuda, seq_data, references, EH, case):
    from recnn_amd.nn import functional as F
    U, T, _ = case
    hc, _, bounds, ref, _, _ = _reference(references, seq_data, EH, case)
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    slots = _slots(U)
    hcg = None if hc is None else tuple(t.to(cuda) for t in hc)
    res, bad = {}, []
    for variant in ("fused", "chunked"):
        F.set_lstm_variant(variant)
        try:
            h, (hT, cT) = F.lstm_encode(gl, st, tbl, slots, T, hcg)
            ht, (hTt, cTt) = F.lstm_encode_train(gl, st, tbl, slots, T, hcg)
        finally:
            F.set_lstm_variant("chunked")
        assert h.shape == (U, T, EH[1]) and hT.shape == (U, EH[1]) and torch.equal(h[:, -1], hT)
        assert ht.requires_grad and not h.requires_grad
        assert torch.equal(ht, h) and torch.equal(hTt, hT) and torch.equal(cTt, cT), (variant, "training forward")
        res[variant] = (h.cpu(), hT.cpu(), cT.cpu())
        errs = [float((a.double() - b).abs().max()) for a, b in zip(res[variant], ref)]
        print(f"encode {_tag(EH, case)} {variant}: err h/hT/cT " + " ".join(f"{e:.3e}" for e in errs)
              + " bounds " + " ".join(f"{b:.3e}" for b in bounds) + f" worst err/bound {max(e / b for e, b in zip(errs, bounds)):.3f}")
        bad += [(variant, n, e, b) for n, e, b in zip(("h", "h_T", "c_T"), errs, bounds) if not e <= b]
    assert not bad, bad
    for a, b in zip(res["fused"], res["chunked"]):
        assert torch.equal(a, b)                                     # the two schedules sum in the same fixed order


# ---------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"U{c[0]}-T{c[1]}")
@pytest.mark.parametrize("EH", SHAPES, ids=lambda s: f"E{s[0]}-H{s[1]}")
def test_gradients_against_float64(cuda, seq_data, references, EH, case):
    U, T, with_h0 = case
    hc, Rw, _, _, bounds, g64 = _reference(references, seq_data, EH, case)
    assert set(g64) == set(G.NAMES if with_h0 else G.PARAMS)
    st, tbl, gl = _on_gpu(cuda, seq_data[EH])
    got = _gpu_grads(cuda, gl, st, tbl, _slots(U), T, hc, Rw)
    assert torch.equal(got["bias_ih_l0"], got["bias_hh_l0"])
    _check(f"grad {_tag(EH, case)}", got, g64, bounds)


# ---------------------------------------------------------------------------------------------------- carry
CARRY_EH, CARRY_CASE, CARRY_CUTS = (72, 144), (33, 70, True), (32, 33)


def test_carry_forward_bit_for_bit(cuda, seq_data, references):
    """70 steps in one call against 32 + 38 (the cut on a chunk boundary) and 33 + 37 (one step past it), the state carried."""
    from recnn_amd.nn import functional as F
    U, T, _ = CARRY_CASE
    hc = _reference(references, seq_data, CARRY_EH, CARRY_CASE)[0]
    st, tbl, gl = _on_gpu(cuda, seq_data[CARRY_EH])
    slots = _slots(U)
    hcg = tuple(t.to(cuda) for t in hc)
    h, (hT, cT) = F.lstm_encode(gl, st, tbl, slots, T, hcg)
    for cut in CARRY_CUTS:
        ha, hca = F.lstm_encode(gl, st, tbl, slots, cut, hcg)
        hb, (hTb, cTb) = F.lstm_encode(gl, st, tbl, slots, T - cut, hca, t0=cut)
        assert torch.equal(torch.cat([ha, hb], 1), h) and torch.equal(hTb, hT) and torch.equal(cTb, cT), cut


def test_carry_training_form(cuda, seq_data, references):
    """The same two cuts with (h_T, c_T) carried and requiring grad: h0 / c0 gradients bit for bit those of the one-call run, the
    parameter gradients within the bound of float64."""
    from recnn_amd.nn import functional as F
    U, T, _ = CARRY_CASE
    hc, Rw, _, _, bounds, g64 = _reference(references, seq_data, CARRY_EH, CARRY_CASE)
    st, tbl, gl = _on_gpu(cuda, seq_data[CARRY_EH])
    slots = _slots(U)
    one = _gpu_grads(cuda, gl, st, tbl, slots, T, hc, Rw)
    for cut in CARRY_CUTS:
        gl.zero_grad(set_to_none=True)
        hcg = tuple(t.to(cuda).requires_grad_(True) for t in hc)
        ha, hca = F.lstm_encode_train(gl, st, tbl, slots, cut, hcg)
        assert hca[0].requires_grad and hca[1].requires_grad
        hb, (hT, cT) = F.lstm_encode_train(gl, st, tbl, slots, T - cut, hca, t0=cut)
        G.loss_of(torch.cat([ha, hb], 1), hT, cT, Rw).backward()
        two = {n: getattr(gl, n).grad.cpu() for n in G.PARAMS}
        two["h0"], two["c0"] = hcg[0].grad.cpu(), hcg[1].grad.cpu()
        assert torch.equal(two["h0"], one["h0"]) and torch.equal(two["c0"], one["c0"]), cut
        _check(f"carry {cut} + {T - cut} vs float64", two, g64, bounds)
