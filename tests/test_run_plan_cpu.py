"""recnn_run_plan / recnn_run_family_init (csrc/engine_graph.hip): how recnn_engine_graph_run cuts a request into run graphs.  Host
arithmetic only, so it is checked here without a GPU: the pieces cover the request exactly once and in order, no piece is longer than a
run graph may be, every piece's kind fits the phase it starts at and names a graph that exists, without alignment the list is the
composition the engine has always used, and with alignment a request that has reached the step after a policy step stays on whole
aligned cycles for as long as one fits."""
import ctypes as C

import pytest

PES = (2, 3, 10, 17, 40)


def _family(L, pe, align, graph_run=-1):
    fam = L.RunFamily()
    assert L.load().recnn_run_family_init(pe, graph_run, align, C.byref(fam)) == 0
    return fam


def _plan(L, pe, fam, first, n, align, cap=4096):
    kinds, lens = (C.c_int * cap)(), (C.c_int * cap)()
    k = L.load().recnn_run_plan(pe, C.byref(fam), first, n, align, kinds, lens, cap)
    assert 0 <= k <= cap
    return [(kinds[i], lens[i]) for i in range(k)]


def _parent_loop(L, pe, fam, first, n):
    """The composition without alignment, restated: at a policy step the multi-cycle graph while it fits, else the policy step with as
    many of its cycle's ordinary steps as the request has left and a graph exists for; elsewhere the longest existing ordinary stretch
    up to the next policy step / the end of the request."""
    out, i = [], 0
    while i < n:
        step, rem = first + i, n - i
        if step % pe == 0:
            if fam.multi_len and rem >= fam.multi_len:
                kind, ln = L.RUN_MULTI, fam.multi_len
            else:
                k = min(min(rem, pe) - 1, L.RUN_MAX)
                while k >= 1 and not fam.has_p[k]:
                    k -= 1
                kind, ln = (L.RUN_POLICY_HEAD, k + 1) if k >= 1 else (L.RUN_POLICY_STEP, 1)
        else:
            k = min(pe - step % pe, rem, L.RUN_MAX)
            while k >= 2 and not fam.has_o[k]:
                k -= 1
            kind, ln = (L.RUN_ORDINARY, k) if k >= 2 else (L.RUN_STEP, 1)
        out.append((kind, ln))
        i += ln
    return out


def _n_steps(pe):
    return sorted({1, 2, pe - 1, pe, pe + 1, 63, 64, 65, 200, 2000} - {0})


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("pe", PES)
def test_pieces_cover_the_request_with_graphs_that_exist(pe, align):
    from recnn_amd import _lib as L
    fam = _family(L, pe, align)
    assert bool(fam.aligned_cycle_len) == bool(align) and fam.aligned_cycle_len in (0, pe)
    assert fam.aligned_multi_len == (fam.multi_len if align else 0)
    for first in range(0, 2 * pe + 1):
        for n in _n_steps(pe):
            pieces = _plan(L, pe, fam, first, n, align)
            pos, reached = first, False
            for kind, ln in pieces:
                phase, rem = pos % pe, first + n - pos
                assert 1 <= ln <= min(L.RUN_MAX, rem), (pe, first, n, pieces)
                pol = [(pos + j) % pe == 0 for j in range(ln)]
                if kind == L.RUN_STEP:
                    assert ln == 1 and not pol[0]
                elif kind == L.RUN_POLICY_STEP:
                    assert ln == 1 and pol[0]
                elif kind == L.RUN_ORDINARY:
                    assert ln >= 2 and fam.has_o[ln] and not any(pol)
                elif kind == L.RUN_POLICY_HEAD:
                    assert ln >= 2 and fam.has_p[ln - 1] and pol[0] and not any(pol[1:])
                elif kind == L.RUN_MULTI:
                    assert ln == fam.multi_len > 0 and phase == 0
                elif kind == L.RUN_ALIGNED_MULTI:
                    assert align and ln == fam.aligned_multi_len > 0 and phase == 1 % pe and pol[-1]
                elif kind == L.RUN_ALIGNED_CYCLE:
                    assert align and ln == fam.aligned_cycle_len == pe and phase == 1 % pe and pol[-1]
                else:
                    raise AssertionError(kind)
                # aligned: from the step after a policy step on, no piece begins ON a policy step while a whole cycle is left
                if align and reached and rem >= pe:
                    assert phase != 0, (pe, first, n, pieces)
                reached = reached or phase == 1 % pe
                pos += ln
            assert pos == first + n, (pe, first, n, pieces)


@pytest.mark.parametrize("pe", PES)
def test_without_alignment_the_composition_is_the_old_loop(pe):
    from recnn_amd import _lib as L
    for fam in (_family(L, pe, 0), _family(L, pe, 1)):        # (aligned members in the family change nothing while align is off)
        for first in range(0, 2 * pe + 1):
            for n in _n_steps(pe):
                assert _plan(L, pe, fam, first, n, 0) == _parent_loop(L, pe, fam, first, n), (pe, first, n)


def test_long_aligned_request_is_stretch_policy_step_then_whole_cycles():
    from recnn_amd import _lib as L
    fam = _family(L, 10, 1)
    assert (fam.multi_len, fam.aligned_multi_len, fam.aligned_cycle_len) == (60, 60, 10)
    # 200 steps from step 205: 5 ordinary steps, the policy step, 3 x 60, one cycle of 10, the last 4
    assert _plan(L, 10, fam, 205, 200, 1) == [(L.RUN_ORDINARY, 5), (L.RUN_POLICY_STEP, 1)] + [(L.RUN_ALIGNED_MULTI, 60)] * 3 + \
        [(L.RUN_ALIGNED_CYCLE, 10), (L.RUN_ORDINARY, 4)]
    # a request the multi-cycle graph serves whole stays ONE launch: nothing aligned fits behind its first policy step
    assert _plan(L, 10, fam, 200, 60, 1) == [(L.RUN_MULTI, 60)]
    # a short buffer: the count is still the whole plan's, and planning again from where the written pieces end continues it
    whole = _plan(L, 10, fam, 205, 2000, 1)
    kinds, lens = (C.c_int * 3)(), (C.c_int * 3)()
    assert L.load().recnn_run_plan(10, C.byref(fam), 205, 2000, 1, kinds, lens, 3) == len(whole)
    head = [(kinds[i], lens[i]) for i in range(3)]
    done = sum(ln for _, ln in head)
    assert head + _plan(L, 10, fam, 205 + done, 2000 - done, 1) == whole
    # graph_run 0 / 1: single-step graphs only
    fam1 = _family(L, 10, 1, graph_run=1)
    assert fam1.multi_len == fam1.aligned_multi_len == fam1.aligned_cycle_len == 0
    assert _plan(L, 10, fam1, 9, 3, 1) == [(L.RUN_STEP, 1), (L.RUN_POLICY_STEP, 1), (L.RUN_STEP, 1)]


def test_bad_arguments_are_refused():
    from recnn_amd import _lib as L
    fam = _family(L, 10, 1)
    assert L.load().recnn_run_plan(0, C.byref(fam), 0, 5, 1, None, None, 0) < 0
    assert L.load().recnn_run_plan(10, None, 0, 5, 1, None, None, 0) < 0
    assert L.load().recnn_run_family_init(0, -1, 1, C.byref(fam)) < 0
