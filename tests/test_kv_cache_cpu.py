"""The step-by-step path of the attention encoders without a GPU: the incremental float64 model of tests/kv_cache_reference.py is
held to the whole-history model of tests/transformer_reference.py, `KVCache.min_capacity` to a brute-force enumeration of the append
kernel's tile walk, the workspace query is host arithmetic, and a CPU module is refused."""
import ctypes as C

import numpy as np
import pytest
import torch

import kv_cache_reference as KR
import seq_reference as R
import transformer_reference as TR
from helpers import make_store

SHAPES = ((8, 16, 1, 16, 1), (24, 48, 3, 80, 2))
SPLITS = ((130,), (64, 66), (63, 1, 1, 65), (1, 129), (1,) * 130)


def _x(E, U, T):
    items, ratings, table = make_store(U, 60, E, T, T + 5, seed=E)
    return R.lstm_inputs(table, items, ratings, T)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "E%d-H%d-heads%d-F%d-L%d" % s)
@pytest.mark.parametrize("alibi", (True, False))
def test_incremental_model_is_the_whole_history_model_under_every_split(shape, alibi):
    E, H, heads, F, L = shape
    enc = TR.make_encoder(E, H, heads, F, L, "gelu", None, alibi, seed=3)
    x = _x(E, 3, 130)
    want = TR.model_cpu(enc, x)
    for sizes in SPLITS:
        err = float((KR.run_split(enc, x, sizes) - want).abs().max())
        print(f"{shape} alibi {alibi} split {sizes[:4]}{'..' if len(sizes) > 4 else ''}: max |incremental - whole| {err:.3e}")
        assert err <= 1e-12
    assert float(want.abs().max()) > 0.1


@pytest.mark.parametrize("window,n", ((1, 1), (1, 7), (5, 1), (5, 7), (70, 1), (70, 7)))
def test_incremental_model_under_a_window_keeps_only_what_the_window_reaches(window, n):
    E, H, heads, F, L = SHAPES[1]
    enc = TR.make_encoder(E, H, heads, F, L, "relu", window, True, seed=4)
    T = 200
    x = _x(E, 2, T)
    want = TR.model_cpu(enc, x)
    sizes = (n,) * (T // n) + ((T % n,) if T % n else ())
    m, out, at = KR.IncrementalModel(enc), [], 0
    for s in sizes:
        out.append(m.append(x[:, at:at + s]))
        at += s
        assert m.k[0].shape[1] <= window - 1 + s
    err = float((torch.cat(out, 1) - want).abs().max())
    print(f"window {window} appends of {n}: max |incremental - whole| {err:.3e}")
    assert err <= 1e-12


CAPACITY_CASES = ((1, 1), (5, 7), (70, 64), (200, 1))


def test_min_capacity_is_a_multiple_of_64_monotone_and_enough_for_the_tile_walk():
    from recnn_amd.nn import KVCache
    for w, n in CAPACITY_CASES:
        cap = KVCache.min_capacity(w, n)
        print(f"min_capacity(window={w}, max_append={n}) = {cap}")
        assert cap % 64 == 0 and cap >= 64
        assert cap == 64 * -(-(w - 1) // 64) + 64 * -(-(n + 63) // 64)
        assert KVCache.min_capacity(w + 1, n) >= cap and KVCache.min_capacity(w, n + 1) >= cap
        assert KVCache.min_capacity(w + 64, n) > cap and KVCache.min_capacity(w, n + 64) > cap
        for pos in range(0, 401):
            for m in sorted({1, n}):                      # every append size up to max_append is covered by the largest
                assert KR.ring_is_safe(pos, m, w, cap), (w, n, pos, m)
    # and the enumeration can fail: a ring one tile smaller is unsafe somewhere, for every case
    for w, n in CAPACITY_CASES:
        cap = KVCache.min_capacity(w, n) - 64
        assert cap == 0 or not all(KR.ring_is_safe(pos, n, w, cap) for pos in range(0, 401)), (w, n)
    assert [KVCache.min_capacity(w, n) for w, n in CAPACITY_CASES] == [64, 192, 256, 320]


def test_staged_positions_without_a_window_are_every_position_so_far():
    for pos, n in ((0, 1), (63, 2), (64, 64), (100, 7)):
        assert KR.staged_positions(pos, n, None) == set(range(pos + n))


def test_workspace_query_is_host_only_and_validates():
    from recnn_amd import _lib as L
    lib = L.load()
    a, b = C.c_int64(), C.c_int64()
    assert lib.recnn_kv_append_workspace_bytes(25, 1, 256, C.byref(a)) == 0
    assert lib.recnn_kv_append_workspace_bytes(25, 64, 256, C.byref(b)) == 0
    assert a.value == 25 * 256 * 4 * 5 and b.value == 64 * a.value and a.value % 256 == 0
    assert lib.recnn_kv_append_workspace_bytes(0, 1, 16, C.byref(a)) == 0 and a.value == 0
    assert lib.recnn_kv_append_workspace_bytes(25, 1, 250, C.byref(a)) != 0 and b"hidden" in lib.recnn_last_error()
    assert lib.recnn_kv_append_workspace_bytes(25, 0, 256, C.byref(a)) != 0 and b"n >= 1" in lib.recnn_last_error()
    assert lib.recnn_kv_append_workspace_bytes(70000, 1, 256, C.byref(a)) != 0 and b"n_rows" in lib.recnn_last_error()
    assert lib.recnn_kv_append_workspace_bytes(25, 1, 256, None) != 0 and b"null" in lib.recnn_last_error()
    c = C.c_int()
    assert lib.recnn_kv_min_capacity(0, 1, C.byref(c)) != 0 and b"window" in lib.recnn_last_error()
    # the append entry points refuse on the host, before any launch: null pointers, a ring below min_capacity, a ragged capacity
    p = C.c_void_p(256)
    head = (p, p, p, p, 3, 7, p, 10, 8, 32, 2)
    tail = (p, p, p, p, p)
    assert lib.recnn_attn_append(*([None] * 4), 3, 7, None, 10, 8, 32, 2, 0, 1, *([None] * 5), 4, 64, *([None] * 5)) != 0
    assert b"null" in lib.recnn_last_error()
    assert lib.recnn_attn_append(*head, 5, 1, p, p, p, p, p, 4, 128, *tail) != 0 and b"capacity" in lib.recnn_last_error()
    assert lib.recnn_attn_append(*head, 0, 1, p, p, p, p, p, 4, 100, *tail) != 0 and b"capacity" in lib.recnn_last_error()
    assert lib.recnn_attn_append(*head, 0, 1, p, p, p, p, p, 2, 64, *tail) != 0 and b"n_sessions" in lib.recnn_last_error()
    blk = (p, 3, 7, 32, 2, 16, 0, 5, 1, C.c_float(1e-5)) + (p,) * 12
    assert lib.recnn_block_append(*blk, p, 4, 128, *tail) != 0 and b"capacity" in lib.recnn_last_error()
    assert lib.recnn_block_append(*blk[:5], 24, *blk[6:], p, 4, 192, *tail) != 0 and b"dim_feedforward" in lib.recnn_last_error()


def test_a_cpu_module_is_refused_everywhere():
    from recnn_amd import _lib as L
    from recnn_amd.nn import AttentionEncoder, EncoderSession, KVCache, TransformerStateEncoder, functional as F
    table = torch.zeros(40, 8)
    items, ratings = torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3)
    for enc, fn in ((AttentionEncoder(9, 16, 1), F.attn_append), (TransformerStateEncoder(9, 16, 1), F.transformer_append)):
        with pytest.raises(L.RecnnHipError, match="GPU"):
            KVCache(enc, 2, 64)
        with pytest.raises(L.RecnnHipError, match="GPU"):
            EncoderSession(enc, table, 2, 64)
        with pytest.raises(L.RecnnHipError, match="GPU module"):
            fn(enc, None, table, items, ratings)
    with pytest.raises(L.RecnnHipError, match="AttentionEncoder"):
        F.attn_append(TransformerStateEncoder(9, 16, 1), None, table, items, ratings)
    with pytest.raises(L.RecnnHipError, match="TransformerStateEncoder"):
        F.transformer_append(AttentionEncoder(9, 16, 1), None, table, items, ratings)
    for other in (torch.nn.LSTM(9, 16), torch.nn.GRU(9, 16)):
        with pytest.raises(L.RecnnHipError, match="lstm_encode / gru_encode"):
            KVCache(other, 2, 64)
