"""Module-level MLP forward/backward on the HIP GEMM kernels (autograd.Function).

This is the generic path behind `Actor.__call__` / `Critic.__call__` (inference in notebooks, user-defined
losses).  The training step proper does not come through here: `ddpg_update` / `td3_update` run the fused
engine (recnn_amd/nn/fused.py).  fp32 (exact-fp32 MFMA) only; operands are zero-padded to the kernels'
16-byte / 64-element contraction granularity with torch copies (plumbing), bias-gradient column sums come
from the dX kernel's epilogue.
Replaces recnn/nn/models.py:66-73 and :207-213 (addmm, relu, dropout) and their autograd backward.
"""
import ctypes as C
import itertools

import numpy as np

import torch

from .. import _lib as L
from .attention import AttentionEncoder
from .transformer import ACTIVATIONS as TRANSFORMER_ACTIVATIONS, TransformerStateEncoder

_call_counter = itertools.count(1)

# Dropout-mask keys on the device (captured updates, recnn_amd/nn/graphed.py): while a key scope is open, every train-mode MLP call
# keys its two hash masks with `*dev + add` (add = calls so far in the scope) instead of the host-side call counter, so that a
# captured graph draws fresh masks on every replay; the scope's owner advances *dev by the calls consumed.
_key_scope = {"dev": None, "add": 0}


def open_key_scope(dev_counter):
    _key_scope["dev"], _key_scope["add"] = dev_counter, 0


def close_key_scope() -> int:
    used = _key_scope["add"]
    _key_scope["dev"], _key_scope["add"] = None, 0
    return used


def _dump_masks(seed, B, H, m1, m2, s):
    if _key_scope["dev"] is not None:
        add = _key_scope["add"]
        _key_scope["add"] = add + 1
        for stream_id, m in ((0, m1), (1, m2)):
            L.call("recnn_hash_mask_dump_at", seed & 0xFFFFFFFF, L.ptr(_key_scope["dev"]), add, stream_id, B, H, L.ptr(m), s)
        return
    key = next(_call_counter)
    L.call("recnn_hash_mask_dump", seed & 0xFFFFFFFF, key & 0x7FFFFFFF, 0, B, H, L.ptr(m1), s)
    L.call("recnn_hash_mask_dump", seed & 0xFFFFFFFF, key & 0x7FFFFFFF, 1, B, H, L.ptr(m2), s)


def _r64(x):
    return (x + 63) // 64 * 64


def _pad(t, rows, cols):
    t = t.detach()
    if t.shape == (rows, cols) and t.is_contiguous() and t.dtype == torch.float32:
        return t
    out = torch.zeros(rows, cols, dtype=torch.float32, device=t.device)
    out[: t.shape[0], : t.shape[1]] = t
    return out


_derived = {}
_written = {}     # id(parameter) -> number of writes the HIP engine made behind autograd's back (mark_written)


_capture_cache = {"d": None}


def open_capture_cache():
    _capture_cache["d"] = {}


def close_capture_cache():
    _capture_cache["d"] = None


def mark_written(params):
    """The fused engine (ddpg_update / td3_update / value_update / Algo.run) writes adopted parameters in place from its
    kernels: no torch op runs, so their autograd version counters do not move.  Every caller that lets the engine step a
    network reports its parameters here; `_derived_of` folds the count into its staleness tag, so a cached bf16 shadow /
    padded / transposed copy made before the step is rebuilt at the next module-level forward.  (A user's own
    `p.data.copy_()` is invisible to both counters -- `.data` carries its own version; call
    `fused.notify_params_changed(module)` after such a write.)"""
    for p in params:
        k = id(p)
        _written[k] = _written.get(k, 0) + 1


def _derived_of(w, kind, build):
    """A layout derived from parameter `w` (transposed / padded copy), kept until `w` is written again.  Staleness is
    detected through the autograd version counter -- torch's in-place ops bump it, and so do recnn_amd's own torch-side
    writers (optim.Adam / Ranger, utils.soft_update call torch.autograd.graph.increment_version) -- plus the engine's
    write count (`mark_written`) for the kernels that update adopted parameters without any torch op."""
    import weakref
    if w.is_cuda and torch.cuda.is_current_stream_capturing():
        # a captured update (recnn_amd/nn/graphed.py) must rebuild the layout on every replay: a hit in the long-lived cache would
        # leave the build out of the graph, and the graph would keep reading the copy made before the capture after `w` moved on.
        # Inside ONE capture the same version of `w` is built once (a cache that lives as long as the capture: every replay
        # rebuilds at the same points of the step).
        tag = (w._version, w.data_ptr(), tuple(w.shape), _written.get(id(w), 0))
        scoped = _capture_cache.get("d")
        if scoped is None:
            return build(w.detach())
        hit = scoped.get((id(w), kind))
        if hit is not None and hit[0] == tag:
            return hit[1]
        out = build(w.detach())
        scoped[(id(w), kind)] = (tag, out, w)      # (w kept alive: its id must not be reused while the capture runs)
        return out
    key = (id(w), kind)
    tag = (w._version, w.data_ptr(), tuple(w.shape), _written.get(id(w), 0))
    hit = _derived.get(key)
    if hit is not None and hit[0]() is w and hit[1] == tag:
        return hit[2]
    out = build(w.detach())
    _derived[key] = (weakref.ref(w, lambda _r, k=key: (_derived.pop(k, None), _written.pop(k[0], None))), tag, out)
    return out


def shadow_target(p):
    """(kind, tensor) of a cached row-padded copy of the 2-D parameter `p` (same rows and columns, wider leading dimension, fp32 or
    bf16: the "padded" / "bf16..." layouts above; transposed copies do not qualify) that is CURRENT -- an optimizer kernel that
    writes `p` can rewrite it in the same pass (`recnn_*_flat_shadow`) instead of leaving a full conversion pass to the next
    forward -- or None.  The caller reports the write with `shadow_written`."""
    if p.dim() != 2 or not p.is_cuda or torch.cuda.is_current_stream_capturing():
        return None
    tag = (p._version, p.data_ptr(), tuple(p.shape), _written.get(id(p), 0))
    best = None
    for (pid, kind), (ref, have, out) in _derived.items():
        if pid != id(p) or ref() is not p or have != tag or kind.startswith("transposed"):
            continue
        if out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < p.shape[0] or out.shape[1] < p.shape[1]:
            continue
        if out.dtype not in (torch.float32, torch.bfloat16) or out.data_ptr() == p.data_ptr():
            continue
        if best is None or (out.dtype == torch.bfloat16 and best[1].dtype != torch.bfloat16):
            best = (kind, out)
    return best


def shadow_written(p, kind):
    """`p` was stepped (its version already bumped) and the kernel rewrote the cached layout `kind`: it is current again."""
    key = (id(p), kind)
    hit = _derived.get(key)
    if hit is not None and hit[0]() is p:
        _derived[key] = (hit[0], (p._version, p.data_ptr(), tuple(p.shape), _written.get(id(p), 0)), hit[2])


_catalogue_dtype = "fp32"


def set_catalogue_dtype(dtype: str):
    """Compute type of the catalogue-sized GEMMs of the REINFORCE path ([rows, hidden] x [hidden, n_items] of the policy
    head and its backward, [rows, state + n_items] x [., hidden] of the critic over action distributions, the logits GEMM of the
    learned behaviour policy `Beta`):
    'fp32' (default; exact-fp32 MFMA, the parity mode) or 'bf16' (bf16 MFMA with fp32 accumulation over bf16 copies of the
    weights kept per weight version; softmax, log-prob, optimizer and all small layers stay fp32)."""
    global _catalogue_dtype
    if dtype not in ("fp32", "bf16"):
        raise ValueError(dtype)
    _catalogue_dtype = dtype


def _r128(x):
    return (x + 127) // 128 * 128


_mlp_dtype = "fp32"


def set_mlp_dtype(dtype: str):
    """Compute type of the module-level MLP stacks (`Actor` / `Critic` / `bcqPerturbator` / `bcqGenerator` called directly, and
    therefore of `bcq_update`): 'fp32' (default; exact-fp32 MFMA, the parity mode) or 'bf16' (bf16 MFMA with fp32 accumulation:
    bf16 copies of the weights kept per weight version, activations and backward tensors in bf16, weight / bias gradients,
    outputs and every optimizer in fp32).  The fused DDPG / TD3 engine has its own switch (`fused.set_defaults(dtype=...)`)."""
    global _mlp_dtype
    if dtype not in ("fp32", "bf16"):
        raise ValueError(dtype)
    _mlp_dtype = dtype


def _args(M, N, dtype=None):
    a = L.GemmArgs()
    a.dtype = L.F32 if dtype is None else dtype
    a.M, a.N = M, N
    a.dx_scale = 1.0
    a.dw_splits = 1
    return a


def _fwd(x, K, w, bias, out, ldc, N, relu, mask, addend=None, yref=None, scale=1.0, dtype=None, add_row_div=0, c_f32=1):
    a = _args(x.shape[0], N, dtype)
    a.A[0], a.B[0], a.lda[0], a.ldb[0], a.K[0] = x.data_ptr(), w.data_ptr(), x.stride(0), w.stride(0), K
    a.C, a.ldc, a.c_f32 = out.data_ptr(), ldc, c_f32
    a.bias, a.relu = (bias.data_ptr() if bias is not None else None), int(relu)
    if addend is not None:      # added before the relu (gemm.hip epilogue_fwd)
        a.addend, a.ld_add, a.add_clip = addend.data_ptr(), addend.stride(0), float("inf")
        a.add_row_div = add_row_div
    if yref is not None:
        a.yref, a.ldy, a.dx_scale = yref.data_ptr(), yref.stride(0), scale
    if mask is not None:
        a.mask_mode, a.mask, a.ld_mask = L.MASK_EXTERNAL, mask.data_ptr(), mask.stride(0)
    if K >= 32768 and x.shape[0] * N <= (1 << 20):
        # a catalogue-long contraction with a small output: scratch for the library's split-K (recnn_gemm_args::ws)
        ws = _splitk_scratch(x.device, 8 * x.shape[0] * N)
        a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    L.call("recnn_gemm_fwd", C.byref(a), L.current_stream())


_splitk_ws = {}          # (device type, index, stream) -> [tensor, handed out during a stream capture?]
_splitk_retired = []     # outgrown buffers a captured graph may still replay into: alive for the process, nothing else is kept
_SPLITK_MAX_STREAMS = 8  # eager scratch buffers kept (least recently used first out); captured ones are never dropped


def _splitk_scratch(device, floats):
    """fp32 scratch of at least `floats` elements on `device` for the library's split-K, one per (device, STREAM): products issued on
    different streams never share a buffer.  A buffer that was handed out DURING A STREAM CAPTURE has its pointer baked into a
    graph (GraphedUpdate) that may replay into it for the life of the process: when it has to grow it is retired, not freed, and its
    stream's entry is never evicted.  Buffers only ever used eagerly are plain cache entries: replaced when they grow, and at most
    _SPLITK_MAX_STREAMS of them are kept (every stream used to pin its buffer, and the outgrown ones, forever)."""
    key = (device.type, device.index, int(torch.cuda.current_stream(device).cuda_stream))
    capturing = torch.cuda.is_current_stream_capturing()
    ent = _splitk_ws.pop(key, None)               # (re-inserted below: dict order = recency)
    if ent is None or ent[0].numel() < floats:
        if ent is not None and ent[1]:
            _splitk_retired.append(ent[0])
        ent = [torch.empty(floats, dtype=torch.float32, device=device), False]
    ent[1] = ent[1] or capturing
    _splitk_ws[key] = ent
    eager = [k for k, e in _splitk_ws.items() if not e[1]]
    for k in eager[:max(0, len(eager) - _SPLITK_MAX_STREAMS)]:
        del _splitk_ws[k]
    return ent[0]


def _dx(dz, Kc, w, N, out, yref, scale, colsum, dtype=None, c_f32=1):
    a = _args(dz.shape[0], N, dtype)
    a.A[0], a.B[0], a.lda[0], a.ldb[0], a.K[0] = dz.data_ptr(), w.data_ptr(), dz.stride(0), w.stride(0), Kc
    a.C, a.ldc, a.c_f32 = out.data_ptr(), out.stride(0), c_f32
    if yref is not None:
        a.yref, a.ldy, a.dx_scale = yref.data_ptr(), yref.stride(0), scale
    if colsum is not None:
        a.colsum = colsum.data_ptr()
    L.call("recnn_gemm_dx", C.byref(a), L.current_stream())


def _dw(dz, M, x, N, out, dtype=None):
    a = _args(M, N, dtype)
    a.A[0], a.B[0], a.lda[0], a.ldb[0], a.K[0] = dz.data_ptr(), x.data_ptr(), dz.stride(0), x.stride(0), dz.shape[0]
    a.C, a.ldc = out.data_ptr(), N
    a.dw_splits, a.dw_slab_stride, a.dw_valid_cols, a.dw_col_rot = 1, M * N, N, 0
    L.call("recnn_gemm_dw", C.byref(a), L.current_stream())


class MLPFunction(torch.autograd.Function):
    @classmethod
    def apply(cls, *args):
        # autograd runs Function.forward with grad mode OFF whatever the caller's mode is, so the caller's mode (does a backward
        # pass through this call exist at all?) is captured here and handed in as the last argument
        args = tuple(args) + (None,) * (11 - len(args))
        return super().apply(*args, torch.is_grad_enabled())

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, train, seed, masks=None, addend1=None, grad_mode=True):
        if not x.is_cuda:
            raise L.RecnnHipError("recnn_amd networks run on the GPU only (no CPU fallback): move the module and its "
                                  "inputs to 'cuda'")
        B, K = x.shape
        H, O = w1.shape[0], w3.shape[0]
        dev = x.device
        if _mlp_dtype == "bf16" and K < 4096:
            return MLPFunction._forward_bf16(ctx, x, w1, b1, w2, b2, w3, b3, train, seed, masks, addend1)
        Kp, Hp, Op = _r64(K), _r64(H), _r64(O)
        # catalogue-wide layer 1 (the critic over action distributions) in bf16 mode: the fp32 operands are only
        # materialised when a backward pass will need them
        big16 = _catalogue_dtype == "bf16" and K >= 4096
        # (needs_input_grad reflects requires_grad of the inputs even under torch.no_grad(): the reward / target forwards of
        #  reinforce_update run there and must not pay an 830 MB fp32 copy of W1 they never read)
        lean = big16 and not (grad_mode and any(ctx.needs_input_grad))
        xp = None if lean else _pad(x, B, Kp)
        if lean:
            w1p = None
        elif w1.numel() >= (1 << 22) and w1.is_leaf:
            w1p = _derived_of(w1, "padded", lambda w: _pad(w, Hp, Kp))      # 100k-wide rows are not 16-byte aligned as stored
        else:
            w1p = _pad(w1, Hp, Kp)
        w2p, w3p = _pad(w2, Hp, Hp), _pad(w3, Op, Hp)
        h1 = torch.zeros(B, Hp, device=dev)
        h2 = torch.zeros(B, Hp, device=dev)
        out = torch.empty(B, O, device=dev)
        m1 = m2 = None
        if train and masks is not None:
            m1, m2 = (m.to(device=dev, dtype=torch.uint8).contiguous() for m in masks)
        elif train:
            m1 = torch.empty(B, H, dtype=torch.uint8, device=dev)
            m2 = torch.empty(B, H, dtype=torch.uint8, device=dev)
            _dump_masks(seed, B, H, m1, m2, L.current_stream())
        b1c, b2c, b3c = b1.detach().float().contiguous(), b2.detach().float().contiguous(), b3.detach().float().contiguous()
        add1 = None if addend1 is None else addend1.detach().float().contiguous()
        if big16:
            # the critic over [state | action distribution]: layer 1 contracts over the catalogue
            K16 = _r128(K)
            x16 = torch.zeros(B, K16, dtype=torch.bfloat16, device=dev)
            x16[:, :K] = x
            def shadow(w):
                t = torch.zeros(Hp, K16, dtype=torch.bfloat16, device=dev)
                t[:H, :K] = w
                return t
            w16 = _derived_of(w1, "bf16_padded", shadow)
            _fwd(x16, K16, w16, b1c, h1, Hp, H, True, m1, addend=add1, dtype=L.BF16)
        else:
            _fwd(xp, Kp, w1p, b1c, h1, Hp, H, True, m1, addend=add1)
        _fwd(h1, Hp, w2p, b2c, h2, Hp, H, True, m2)
        _fwd(h2, Hp, w3p, b3c, out, O, O, False, None)
        ctx.save_for_backward(xp, h1, h2, w1p, w2p, w3p)
        ctx.dims = (B, K, H, O, Kp, Hp, Op)
        ctx.train = bool(train)
        ctx.bf16 = False
        return out

    # ---- bf16 compute mode (set_mlp_dtype): the same three GEMM + epilogue launches on bf16 operands
    @staticmethod
    def _shadow16(w, rows, cols):
        def build(t):
            out = torch.zeros(rows, cols, dtype=torch.bfloat16, device=t.device)
            out[: t.shape[0], : t.shape[1]] = t
            return out
        return _derived_of(w, f"bf16_{rows}x{cols}", build) if w.is_leaf else build(w.detach())

    @staticmethod
    def _buf16(rows, cols, valid, dev):
        """bf16 [rows, cols] whose columns >= valid are zero and whose first `valid` columns the caller's kernel writes: only the
        padding is filled (whole-buffer torch.zeros calls were 17 % of the BCQ step's kernel time, profiles/r03_bcq_*)."""
        t = torch.empty(rows, cols, dtype=torch.bfloat16, device=dev)
        if cols != valid:
            t[:, valid:].zero_()
        return t

    @staticmethod
    def _forward_bf16(ctx, x, w1, b1, w2, b2, w3, b3, train, seed, masks, addend1):
        B, K = x.shape
        H, O = w1.shape[0], w3.shape[0]
        Kp, Hp, Op = _r128(K), _r128(H), _r64(O)
        dev = x.device
        x16 = MLPFunction._buf16(B, Kp, K, dev)
        x16[:, :K] = x.detach()
        w1s, w2s, w3s = MLPFunction._shadow16(w1, Hp, Kp), MLPFunction._shadow16(w2, Hp, Hp), MLPFunction._shadow16(w3, Op, Hp)
        m1 = m2 = None
        if train and masks is not None:
            m1, m2 = (m.to(device=dev, dtype=torch.uint8).contiguous() for m in masks)
        elif train:
            m1 = torch.empty(B, H, dtype=torch.uint8, device=dev)
            m2 = torch.empty(B, H, dtype=torch.uint8, device=dev)
            _dump_masks(seed, B, H, m1, m2, L.current_stream())
        f = lambda t: t.detach().float().contiguous()
        add1 = None if addend1 is None else f(addend1)
        h1 = MLPFunction._buf16(B, Hp, H, dev)
        h2 = MLPFunction._buf16(B, Hp, H, dev)
        out = torch.empty(B, O, device=dev)
        _fwd(x16, Kp, w1s, f(b1), h1, Hp, H, True, m1, addend=add1, dtype=L.BF16, c_f32=0)
        _fwd(h1, Hp, w2s, f(b2), h2, Hp, H, True, m2, dtype=L.BF16, c_f32=0)
        _fwd(h2, Hp, w3s, f(b3), out, O, O, False, None, dtype=L.BF16)
        ctx.save_for_backward(x16, h1, h2, w1s, w2s, w3s)
        ctx.dims = (B, K, H, O, Kp, Hp, Op)
        ctx.train = bool(train)
        ctx.bf16 = True
        return out

    @staticmethod
    def _backward_bf16(ctx, dout):
        x16, h1, h2, w1s, w2s, w3s = ctx.saved_tensors
        B, K, H, O, Kp, Hp, Op = ctx.dims
        dev = dout.device
        scale = 2.0 if ctx.train else 1.0
        tiles = (B + 31) // 32
        need = ctx.needs_input_grad
        d16 = MLPFunction._buf16(B, Op, O, dev)
        d16[:, :O] = dout
        gw3 = gb3 = gw2 = gw1 = None
        if need[5]:
            gw3 = torch.empty(O, H, device=dev)
            _dw(d16, O, h2, H, gw3, dtype=L.BF16)
        if need[6]:
            gb3 = dout.float().sum(0)
        dz2 = MLPFunction._buf16(B, Hp, H, dev)
        cs2 = torch.empty(tiles, H, device=dev)
        _dx(d16, Op, w3s, H, dz2, h2, scale, cs2, dtype=L.BF16, c_f32=0)
        if need[3]:
            gw2 = torch.empty(H, H, device=dev)
            _dw(dz2, H, h1, H, gw2, dtype=L.BF16)
        dz1 = MLPFunction._buf16(B, Hp, H, dev)
        cs1 = torch.empty(tiles, H, device=dev)
        _dx(dz2, Hp, w2s, H, dz1, h1, scale, cs1, dtype=L.BF16, c_f32=0)
        if need[1]:
            gw1 = torch.empty(H, K, device=dev)
            _dw(dz1, H, x16, K, gw1, dtype=L.BF16)
        gx = None
        if need[0]:
            gx = torch.empty(B, K, device=dev)
            _dx(dz1, Hp, w1s, K, gx, None, 1.0, None, dtype=L.BF16)
        gadd = dz1[:, :H].float() if need[10] else None
        return (gx, gw1, cs1.sum(0) if need[2] else None, gw2, cs2.sum(0) if need[4] else None, gw3, gb3, None, None, None,
                gadd, None)

    @staticmethod
    def backward(ctx, dout):
        if ctx.bf16:
            return MLPFunction._backward_bf16(ctx, dout)
        xp, h1, h2, w1p, w2p, w3p = ctx.saved_tensors
        B, K, H, O, Kp, Hp, Op = ctx.dims
        dev = dout.device
        scale = 2.0 if ctx.train else 1.0
        tiles = (B + 31) // 32
        need = ctx.needs_input_grad      # frozen weights (a critic scoring a policy's action) skip their dW GEMMs
        doutp = _pad(dout, B, Op)
        gw3 = gb3 = gw2 = gw1 = None
        if need[5]:
            gw3 = torch.empty(O, H, device=dev)
            _dw(doutp, O, h2, H, gw3)
        if need[6]:
            gb3 = dout.sum(0)
        dz2 = torch.zeros(B, Hp, device=dev)
        cs2 = torch.empty(tiles, H, device=dev)
        _dx(doutp, Op, w3p, H, dz2, h2, scale, cs2)
        if need[3]:
            gw2 = torch.empty(H, H, device=dev)
            _dw(dz2, H, h1, H, gw2)
        dz1 = torch.zeros(B, Hp, device=dev)
        cs1 = torch.empty(tiles, H, device=dev)
        _dx(dz2, Hp, w2p, H, dz1, h1, scale, cs1)
        if need[1]:
            gw1 = torch.empty(H, K, device=dev)
            _dw(dz1, H, xp, K, gw1)
        gx = None
        if need[0]:
            gx = torch.empty(B, K, device=dev)
            _dx(dz1, Hp, w1p, K, gx, None, 1.0, None)
        gadd = dz1[:, :H] if need[10] else None     # d/d addend1 = dZ1
        return (gx, gw1, cs1.sum(0) if need[2] else None, gw2, cs2.sum(0) if need[4] else None, gw3, gb3, None, None, None,
                gadd, None)


def mlp(x, module, train: bool):
    """`module.forced_masks` (a list of (m1, m2) uint8 keep-mask pairs, consumed first-in first-out) replaces the hash masks
    of the next train-mode calls: replaying logged masks, and the parity tests."""
    return MLPFunction.apply(x.float(), module.linear1.weight, module.linear1.bias, module.linear2.weight,
                             module.linear2.bias, module.linear3.weight, module.linear3.bias, train, torch.initial_seed(),
                             _take_forced_masks(module, train), None)


def mlp_frozen(x, module, train: bool):
    """`mlp` with the module's weights taken as constants: the gradient reaches `x` only (a critic scoring the action of the
    policy being trained -- its own dW / db GEMMs would be thrown away by the next zero_grad)."""
    d = lambda t: t.detach()
    return MLPFunction.apply(x.float(), d(module.linear1.weight), d(module.linear1.bias), d(module.linear2.weight),
                             d(module.linear2.bias), d(module.linear3.weight), d(module.linear3.bias), train,
                             torch.initial_seed(), _take_forced_masks(module, train), None)


def mlp3(x, l1, l2, w3, b3):
    """relu(l1) -> relu(l2) -> x W3^T + b3 without dropout (the VAE encoder / decoder stacks of bcqGenerator)."""
    return MLPFunction.apply(x.float(), l1.weight, l1.bias, l2.weight, l2.bias, w3, b3, False, 0, None, None)


def mlp_candidates(state, x, n, w1, b1, w2, b2, w3, b3):
    """MLP([repeat_interleave(state, n, 0) | x]) for `x` holding n consecutive candidate rows per state row -- relu, relu,
    linear, no dropout, no gradient (the target side of BCQ's critic step, recnn/nn/update/bcq.py:98-106, where the
    reference materialises the repeated states and multiplies them n times over).  Layer 1 is split along its input:
    the state part  S1 = state W1[:, :S]^T + b1  is computed ONCE per state row, the candidate part adds it back per row
    through the GEMM epilogue (`add_row_div`: output row m reads S1 row m / n) before the relu.  10 candidates per state at
    state 1290 / candidate 128..512 wide: 4..8 x fewer layer-1 FLOPs and no [B n, 1290] operand in memory."""
    if not state.is_cuda:
        raise L.RecnnHipError("recnn_amd networks run on the GPU only (no CPU fallback)")
    with torch.no_grad():
        B, S = state.shape
        R, Kx = x.shape
        if R != B * n or w1.shape[1] != S + Kx:
            raise ValueError(f"mlp_candidates: {R} candidate rows for {B} states x {n}, layer 1 takes {w1.shape[1]} inputs")
        H, O = w1.shape[0], w3.shape[0]
        Sp, Kp, Hp, Op = _r64(S), _r64(Kx), _r64(H), _r64(O)
        dev = state.device
        f = lambda t: t.detach().float().contiguous()
        if _mlp_dtype == "bf16":
            Sp, Kp, Hp = _r128(S), _r128(Kx), _r128(H)
            buf16 = MLPFunction._buf16

            def to16(t, rows, cols):       # only the padding is filled (whole-buffer zeros + copies were 11 % of the graphed BCQ step)
                o = buf16(rows, cols, t.shape[1], dev)
                if rows != t.shape[0]:
                    o[t.shape[0]:].zero_()
                o[: t.shape[0], : t.shape[1]] = t.detach()
                return o

            def w16(part, lo, hi, cols):   # bf16 copy of W1's columns [lo, hi), kept per weight version when W1 is a leaf
                build = lambda w: to16(w[:, lo:hi], Hp, cols)
                return _derived_of(w1, f"bf16_cols_{lo}_{hi}_{Hp}x{cols}", build) if w1.is_leaf else build(w1)
            s1 = torch.empty(B, Hp, device=dev)                 # the shared state part stays fp32 (it is an epilogue addend)
            if Hp != H:
                s1[:, H:].zero_()
            _fwd(to16(state, B, Sp), Sp, w16("state", 0, S, Sp), f(b1), s1, Hp, H, False, None, dtype=L.BF16)
            h1 = buf16(R, Hp, H, dev)
            _fwd(to16(x, R, Kp), Kp, w16("cand", S, S + Kx, Kp), None, h1, Hp, H, True, None, addend=s1, add_row_div=n, dtype=L.BF16, c_f32=0)
            h2 = buf16(R, Hp, H, dev)
            _fwd(h1, Hp, MLPFunction._shadow16(w2, Hp, Hp), f(b2), h2, Hp, H, True, None, dtype=L.BF16, c_f32=0)
            out = torch.empty(R, O, device=dev)
            _fwd(h2, Hp, MLPFunction._shadow16(w3, Op, Hp), f(b3), out, O, O, False, None, dtype=L.BF16)
            return out
        s1 = torch.zeros(B, Hp, device=dev)
        _fwd(_pad(state, B, Sp), Sp, _pad(w1[:, :S], Hp, Sp), f(b1), s1, Hp, H, False, None)
        h1 = torch.zeros(R, Hp, device=dev)
        _fwd(_pad(x, R, Kp), Kp, _pad(w1[:, S:], Hp, Kp), None, h1, Hp, H, True, None, addend=s1, add_row_div=n)
        h2 = torch.zeros(R, Hp, device=dev)
        _fwd(h1, Hp, _pad(w2, Hp, Hp), f(b2), h2, Hp, H, True, None)
        out = torch.empty(R, O, device=dev)
        _fwd(h2, Hp, _pad(w3, Op, Hp), f(b3), out, O, O, False, None)
        return out


# ------------------------------------------------------------------------------------------------------------------------
# Conditional VAE of BCQ: latent layer and loss as autograd nodes over csrc/vae.hip.
# Replaces recnn/nn/models.py:271-277 and recnn/nn/update/bcq.py:78-81 (and the graph torch would record for them).

class VaeLatentFunction(torch.autograd.Function):
    """(z, std) = latent(ml, eps): ml = [mean | raw log_std]; std = exp(clamp(raw, -4, 15)); z = mean + std * eps."""

    @staticmethod
    def forward(ctx, ml, eps):
        if not ml.is_cuda:
            raise L.RecnnHipError("recnn_amd VAE latent layer: needs GPU tensors (no CPU fallback)")
        ml = ml.float().contiguous()
        eps = eps.to(device=ml.device, dtype=torch.float32).contiguous()
        B, L2 = ml.shape
        Ld = L2 // 2
        z = torch.empty(B, Ld, device=ml.device)
        std = torch.empty(B, Ld, device=ml.device)
        L.call("recnn_vae_latent_fwd", L.ptr(ml), ml.stride(0), L.ptr(eps), eps.stride(0), B, Ld, L.ptr(z), z.stride(0),
               L.ptr(std), std.stride(0), L.current_stream())
        ctx.save_for_backward(ml, eps, std)
        return z, std

    @staticmethod
    def backward(ctx, dz, dstd):
        ml, eps, std = ctx.saved_tensors
        B, L2 = ml.shape
        Ld = L2 // 2
        rows = lambda t: None if t is None else (t.float() if t.stride(1) == 1 else t.float().contiguous())
        dz, dstd = rows(dz), rows(dstd)        # dz is usually the latent columns of the decoder's dX: strided rows
        dml = torch.empty_like(ml)
        L.call("recnn_vae_latent_bwd", L.ptr(ml), ml.stride(0), L.ptr(eps), eps.stride(0), L.ptr(std), std.stride(0),
               L.ptr(dz), 0 if dz is None else dz.stride(0), None, 0, L.ptr(dstd), 0 if dstd is None else dstd.stride(0),
               B, Ld, L.ptr(dml), dml.stride(0), L.current_stream())
        return dml, None


def vae_latent(ml, eps):
    return VaeLatentFunction.apply(ml, eps)


class VaeLossFunction(torch.autograd.Function):
    """out3 = (mse(recon, action), KL, mse + kl_weight * KL), KL = -0.5 mean(1 + log(std^2) - mean^2 - std^2)."""

    @staticmethod
    def forward(ctx, recon, action, mean, std, kl_weight):
        if not recon.is_cuda:
            raise L.RecnnHipError("recnn_amd VAE loss: needs GPU tensors (no CPU fallback)")
        recon, action = recon.float(), action.detach().float()
        mean, std = mean.float(), std.float()
        for t in (recon, action, mean, std):
            if t.stride(1) != 1:
                raise L.RecnnHipError("recnn_amd VAE loss: rows must be contiguous")
        B, A = recon.shape
        Ld = mean.shape[1]
        out = torch.empty(3, device=recon.device)
        scratch = torch.empty(512, device=recon.device)
        L.call("recnn_vae_loss_fwd", L.ptr(recon), recon.stride(0), L.ptr(action), action.stride(0), L.ptr(mean), mean.stride(0),
               L.ptr(std), std.stride(0), B, A, Ld, float(kl_weight), L.ptr(out), L.ptr(scratch), L.current_stream())
        ctx.save_for_backward(recon, action, mean, std)
        ctx.kl_weight = float(kl_weight)
        return out

    @staticmethod
    def backward(ctx, g):
        recon, action, mean, std = ctx.saved_tensors
        B, A = recon.shape
        Ld = mean.shape[1]
        g = g.float().contiguous()
        d_recon = torch.empty(B, A, device=recon.device)
        d_mean = torch.empty(B, Ld, device=recon.device)
        d_std = torch.empty(B, Ld, device=recon.device)
        L.call("recnn_vae_loss_bwd", L.ptr(recon), recon.stride(0), L.ptr(action), action.stride(0), L.ptr(mean), mean.stride(0),
               L.ptr(std), std.stride(0), B, A, Ld, L.ptr(g), ctx.kl_weight, L.ptr(d_recon), A, L.ptr(d_mean), Ld,
               L.ptr(d_std), Ld, L.current_stream())
        return d_recon, None, d_mean, d_std, None


def vae_loss(recon, action, mean, std, kl_weight=0.5):
    """float[3] = (reconstruction loss, KL loss, reconstruction + kl_weight * KL)  (bcq.py:78-81)."""
    return VaeLossFunction.apply(recon, action, mean, std, kl_weight)


def _take_forced_masks(module, train):
    forced = getattr(module, "forced_masks", None)
    return forced.pop(0) if (train and forced) else None


# ------------------------------------------------------------------------------------------------------------------------
# Categorical policy head of REINFORCE: DiscreteActor = linear1 -> relu -> linear2 -> softmax, plus
# Categorical sampling / log-prob, as ONE autograd node over the HIP kernels (csrc/gemm.hip, csrc/policy.hip).
# Replaces recnn/nn/models.py:95-111 and the autograd graph torch would record for it.

def _r4(x):
    return (x + 3) // 4 * 4


def categorical(probs, actions=None, seed=None):
    """Categorical(probs).sample() and .log_prob(action) of torch.distributions (probs / probs.sum, clamp to [eps, 1-eps], log)
    over rows of an (unnormalised) probability matrix, no gradient.  actions=None draws them.  Returns (actions, log_prob)."""
    if not probs.is_cuda:
        raise L.RecnnHipError("recnn_amd categorical: needs a GPU tensor (no CPU fallback)")
    p = probs.detach()
    B, N = p.shape
    if p.dtype != torch.float32 or p.stride(1) != 1 or p.stride(0) % 4 or p.data_ptr() % 16:
        q = torch.zeros(B, _r4(N), dtype=torch.float32, device=p.device)
        q[:, :N] = p
        p = q
    act = torch.empty(B, dtype=torch.int64, device=p.device) if actions is None else actions.to(torch.int64).contiguous()
    lp = torch.empty(B, dtype=torch.float32, device=p.device)
    flags = L.CAT_SAMPLE if actions is None else 0
    seed = torch.initial_seed() if seed is None else seed
    L.call("recnn_categorical_rows", L.ptr(p), p.stride(0), B, N, flags, seed & 0xFFFFFFFF, next(_call_counter) & 0x7FFFFFFF,
           L.ptr(act), L.ptr(lp), None, L.current_stream())
    return act, lp


class DiscretePolicyFunction(torch.autograd.Function):
    """(probs, action, log_prob) = head(x): h = relu(x W1^T + b1), p = softmax(h W2^T + b2), action ~ p (or given),
    log_prob = log(clamp(p[action] / sum p)).  Backward takes d log_prob (REINFORCE) and / or d probs."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, actions, sample, seed):
        if not x.is_cuda:
            raise L.RecnnHipError("recnn_amd networks run on the GPU only (no CPU fallback): move the module and its "
                                  "inputs to 'cuda'")
        ctx.set_materialize_grads(False)
        B, K = x.shape
        H, N = w1.shape[0], w2.shape[0]
        bf16 = _catalogue_dtype == "bf16"
        Kp, Hp, ldn = _r64(K), (_r128(H) if bf16 else _r64(H)), (_r128(N) if bf16 else _r64(N))
        dev = x.device
        xp = _pad(x, B, Kp)
        w1p = _pad(w1, Hp, Kp)
        h = torch.zeros(B, Hp, device=dev)
        buf = torch.empty(B, ldn, device=dev)
        if ldn != N:
            buf[:, N:].zero_()
        _fwd(xp, Kp, w1p, b1.detach().float().contiguous(), h, Hp, H, True, None)
        if bf16:
            def shadow(w):
                t = torch.zeros(N, Hp, dtype=torch.bfloat16, device=dev)
                t[:, :H] = w
                return t
            w2p = _derived_of(w2, "bf16", shadow)
            h16 = h.to(torch.bfloat16)
            _fwd(h16, Hp, w2p, b2.detach().float().contiguous(), buf, ldn, N, False, None, dtype=L.BF16)
        else:
            w2p = _pad(w2, _r4(N), Hp)     # no copy for the usual shapes (N % 4 == 0, H % 64 == 0)
            _fwd(h, Hp, w2p, b2.detach().float().contiguous(), buf, ldn, N, False, None)
        stat = torch.empty(B, 4, device=dev)
        lp = torch.zeros(B, device=dev)
        flags = L.CAT_SOFTMAX
        if sample:
            act = torch.empty(B, dtype=torch.int64, device=dev)
            flags |= L.CAT_SAMPLE
        elif actions is not None:
            act = actions.to(device=dev, dtype=torch.int64).contiguous()
        else:
            act = None
        L.call("recnn_categorical_rows", L.ptr(buf), ldn, B, N, flags, seed & 0xFFFFFFFF, next(_call_counter) & 0x7FFFFFFF,
               L.ptr(act), L.ptr(lp), L.ptr(stat), L.current_stream())
        probs = buf[:, :N]
        act_out = act if act is not None else torch.full((B,), -1, dtype=torch.int64, device=dev)
        ctx.save_for_backward(xp, h, w1p, w2p, probs, act_out, stat)
        ctx.w2_param = w2
        ctx.bf16 = bf16
        ctx.dims = (B, K, H, N, Kp, Hp, ldn)
        ctx.has_action = act is not None
        ctx.mark_non_differentiable(act_out)
        return probs, act_out, lp

    @staticmethod
    def backward(ctx, dprobs, _dact, dlp):
        xp, h, w1p, w2p, probs, act, stat = ctx.saved_tensors
        B, K, H, N, Kp, Hp, ldn = ctx.dims
        dev = probs.device
        s = L.current_stream()
        if dprobs is None and (dlp is None or not ctx.has_action):
            return (None,) * 8
        bf16 = ctx.bf16 and dprobs is None      # (a gradient through the probabilities themselves stays on the fp32 path)
        dlog = torch.empty(B, ldn, device=dev, dtype=torch.bfloat16 if bf16 else torch.float32)
        if ldn != _r4(N):
            dlog[:, _r4(N):].zero_()
        acc = 0
        if dprobs is not None:
            dpr = dprobs.float().contiguous()
            L.call("recnn_softmax_bwd", L.ptr(probs), probs.stride(0), B, N, L.ptr(dpr), dpr.stride(0), L.ptr(dlog), ldn, s)
            acc = L.LPB_ACCUMULATE
        if bf16:
            acc |= L.LPB_BF16
        g = None
        if dlp is not None and ctx.has_action:
            g = dlp.float().contiguous()
        if not ctx.has_action:
            act = torch.zeros(B, dtype=torch.int64, device=dev)
        gb2 = torch.empty(N, device=dev)
        scratch = torch.empty((B + 31) // 32, _r4(N), device=dev)
        L.call("recnn_logprob_bwd", L.ptr(probs), probs.stride(0), B, N, L.ptr(act), L.ptr(g), L.ptr(stat), L.ptr(dlog), ldn, acc,
               L.ptr(gb2), L.ptr(scratch), s)
        del scratch
        gdt = L.BF16 if bf16 else None
        h_op = h.to(torch.bfloat16) if bf16 else h       # [rows, hidden]: small next to the catalogue operands
        need_w2 = bool(ctx.needs_input_grad[3])          # (a frozen head -- requires_grad False -- gets no gradient, deferred or not)
        defer = need_w2 and _episode["on"] and dprobs is None and ctx.w2_param.is_leaf
        gw2 = None                                       # deferred: ONE dW over the whole episode's rows at the end of the pass (episode_backward)
        if need_w2 and not defer:
            gw2 = torch.empty(N, H, device=dev)
            _dw(dlog, N, h_op, H, gw2, dtype=gdt)
        dz1 = torch.zeros(B, Hp, device=dev)
        # dZ1 = (dlogits W2) * [h > 0]: contraction over the catalogue.  W2 is [n_items, hidden], k-strided for this product;
        # its transpose (made once per weight version, shared by the backward passes of a whole episode) puts the
        # contraction on the contiguous axis, so the LDS-DMA forward kernel runs it (measured 4.2 -> 1.3 ms at 256 x 100k x 2048)
        def transposed(w):
            return transposed_rows(w, ldn, bf16)
        w2t = _derived_of(ctx.w2_param, "transposed_bf16" if bf16 else "transposed", transposed)
        _fwd(dlog, ldn, w2t, None, dz1, Hp, H, False, None, yref=h_op, scale=1.0, dtype=gdt)
        if defer:     # grouped by (parameter, operand type): set_catalogue_dtype may change between the steps of an episode
            _episode["pending"].setdefault((id(ctx.w2_param), gdt), (ctx.w2_param, gdt, []))[2].append((dlog, h_op))
        del dlog
        gb1 = dz1[:, :H].sum(0)
        gw1 = torch.empty(H, K, device=dev)
        _dw(dz1, H, xp, K, gw1)
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty(B, K, device=dev)
            _dx(dz1, Hp, w1p, K, gx, None, 1.0, None)
        return gx, gw1, gb1, gw2, gb2, None, None, None


def transposed_rows(w, ldt, bf16=False):
    """[cols, ldt] (fp32 or bf16, padding columns zero) with out[c, r] = w[r, c], by the tiled HIP transpose (recnn_transpose_rows)."""
    w = w.detach().float().contiguous()
    R, Cc = w.shape
    t = torch.zeros(Cc, ldt, device=w.device, dtype=torch.bfloat16 if bf16 else torch.float32)
    L.call("recnn_transpose_rows", L.ptr(w), w.stride(0), R, Cc, L.ptr(t), ldt, int(bool(bf16)), L.current_stream())
    return t


# ---- the policy head's weight gradient over an EPISODE.  ChooseREINFORCE's loss is a sum over the `policy_step` steps of the
# episode, each term a separate autograd node of DiscretePolicyFunction: left to autograd, every node computes its own
# [n_items, hidden] gradient (a dW launch that writes 819 MB at 100k x 2048) and AccumulateGrad adds them one by one (nine 819 MB
# add_ passes).  Inside `episode_backward()` the nodes keep their d logits instead and ONE dW GEMM over all the episode's rows
# (k = steps x batch) writes the gradient once; it is added to `.grad` like autograd would.
_episode = {"on": False, "pending": {}}


class episode_backward:
    """`with episode_backward(): loss.backward()` -- see above.  Only nodes whose log-prob (not the probabilities) carries the
    gradient take part; everything else in the graph is untouched."""

    def __enter__(self):
        if _episode["on"]:
            raise RuntimeError("episode_backward is not re-entrant")
        _episode["on"], _episode["pending"] = True, {}
        return self

    def __exit__(self, exc_type, exc, tb):
        pending, _episode["pending"], _episode["on"] = _episode["pending"], {}, False
        if exc_type is not None:
            return False
        def gather(terms, i):
            # the terms' tensors into one [rows, ld] operand, each released as soon as it is copied (torch.cat would hold the
            # episode twice: ~2 x 1 GB of d logits at 10 x 256 x 100k)
            if len(terms) == 1:
                return terms[0][i]
            first = terms[0][i]
            out = torch.empty((sum(t[i].shape[0] for t in terms),) + tuple(first.shape[1:]), dtype=first.dtype, device=first.device)
            off = 0
            for k in range(len(terms)):
                t = terms[k][i]
                out[off:off + t.shape[0]].copy_(t)
                off += t.shape[0]
                terms[k] = tuple(None if j == i else terms[k][j] for j in range(2))
            return out
        for w2, gdt, terms in pending.values():
            N, H = w2.shape
            dlog = gather(terms, 0)
            h_op = gather(terms, 1)
            gw2 = torch.empty(N, H, device=w2.device)
            _dw(dlog, N, h_op, H, gw2, dtype=gdt)
            del dlog, h_op
            with torch.no_grad():
                if w2.grad is None:
                    w2.grad = gw2
                else:
                    w2.grad.add_(gw2)
        return False


def discrete_policy(x, module, actions=None, sample=False):
    """probs, action, log_prob of `module` (a DiscreteActor) for a batch of states."""
    return DiscretePolicyFunction.apply(x.float(), module.linear1.weight, module.linear1.bias, module.linear2.weight,
                                        module.linear2.bias, actions, bool(sample), torch.initial_seed())


def beta_train_forward(state, target, weight, bias):
    """The learned behaviour policy of the Top-K off-policy correction (`Beta` of the reference's notebook
    `examples/2. REINFORCE TopK Off Policy Correction/3. TopK Reinforce Off Policy Correction.ipynb`, cell 3):

        p    = Softmax()(Linear(state))                      # the probabilities it returns (detached)
        loss = CrossEntropyLoss()(p, action.argmax(1))       # NB: the cross entropy of the PROBABILITIES taken as logits

    Returns (p float32 [B, n_items] -- a view into a 16-byte aligned buffer --, loss (device scalar), dW [n_items, K], db [n_items]): every
    catalogue-wide pass runs in HIP kernels -- the logits GEMM, the two softmaxes (of the logits, and of p inside the loss:
    recnn_categorical_rows), d loss / d p = (softmax(p) - onehot) / B (recnn_logprob_bwd with g = -1 / B), the softmax backward
    (recnn_softmax_bwd) and the weight-gradient GEMM; the bias gradient is the column sum of d logits (recnn_colsum_rows).  No autograd graph is recorded (the notebook's forward steps its optimizer itself)."""
    if not state.is_cuda:
        raise L.RecnnHipError("recnn_amd Beta: needs GPU tensors (no CPU fallback)")
    x = state.detach().float()
    B, K = x.shape
    N = weight.shape[0]
    dev = x.device
    Kp, ldn = _r64(K), _r64(N)
    s = L.current_stream()
    xp = _pad(x, B, Kp)
    p = torch.empty(B, ldn, device=dev)
    if ldn != N:
        p[:, N:].zero_()
    if _catalogue_dtype == "bf16" and N >= 4096:
        # the logits GEMM is catalogue-sized ([B, 1290] x [n_items, 1290]^T): bf16 operands in the bf16 catalogue mode, like the policy
        # head's; the bf16 copy of the weight is kept current by the optimizer pass (shadow_target)
        K16 = _r128(K)
        x16 = torch.zeros(B, K16, dtype=torch.bfloat16, device=dev)
        x16[:, :K] = x

        def shadow(w):
            t = torch.zeros(_r4(N), K16, dtype=torch.bfloat16, device=dev)
            t[:N, :K] = w
            return t
        w16 = _derived_of(weight, "bf16_padded", shadow)
        _fwd(x16, K16, w16, bias.detach().float().contiguous(), p, ldn, N, False, None, dtype=L.BF16)
    else:
        wp = _derived_of(weight, "padded", lambda w: _pad(w.detach(), _r4(N), Kp)) if (K != Kp or N != _r4(N)) else weight.detach()
        _fwd(xp, Kp, wp, bias.detach().float().contiguous(), p, ldn, N, False, None)
    tgt = target.to(device=dev, dtype=torch.int64).contiguous()
    L.call("recnn_categorical_rows", L.ptr(p), ldn, B, N, L.CAT_SOFTMAX, 0, 0, None, None, None, s)          # p = softmax(logits)
    q = p.clone()
    stat = torch.empty(B, 4, device=dev)
    lp = torch.empty(B, device=dev)
    L.call("recnn_categorical_rows", L.ptr(q), ldn, B, N, L.CAT_SOFTMAX, 0, 0, L.ptr(tgt), L.ptr(lp), L.ptr(stat), s)   # q = softmax(p), lp = log q[target]
    loss = -lp.mean()
    g = torch.full((B,), -1.0 / B, device=dev)
    dprobs = torch.empty(B, ldn, device=dev)
    if ldn != _r4(N):
        dprobs[:, _r4(N):].zero_()
    L.call("recnn_logprob_bwd", L.ptr(q), ldn, B, N, L.ptr(tgt), L.ptr(g), L.ptr(stat), L.ptr(dprobs), ldn, 0, None, None, s)
    del q
    dlog = torch.empty(B, ldn, device=dev)
    if ldn != _r4(N):
        dlog[:, _r4(N):].zero_()
    L.call("recnn_softmax_bwd", L.ptr(p), ldn, B, N, L.ptr(dprobs), ldn, L.ptr(dlog), ldn, s)
    del dprobs
    gw = torch.empty(N, K, device=dev)
    if _catalogue_dtype == "bf16" and N >= 4096:
        # the weight gradient d logits^T x state ([n_items, 256] x [256, 1290]: 66 GFLOP at 100k items) on the bf16 LDS-DMA dW kernel like the
        # policy head's; the fp32 register-staged kernel it replaces was 17.5 % of the 100k bf16 step (profiles/r04_reinforce_100k_bf16_*)
        _dw(dlog.to(torch.bfloat16), N, x16, K, gw, dtype=L.BF16)
    else:
        _dw(dlog, N, xp, K, gw)
    gb = torch.empty(N, device=dev)
    L.call("recnn_colsum_rows", L.ptr(dlog), ldn, B, N, L.ptr(gb), s)      # sum over the batch rows of d logits
    return p[:, :N], loss, gw, gb


# ------------------------------------------------------------------------------------------------------------------------
# Off-policy evaluation (csrc/logprob.hip): log pi(a | s) of ONE action per row under a softmax over the whole
# catalogue, the [B, n_items] logits never in memory.

def default_items_per_slice(B, N):
    """Catalogue slice length of `catalogue_log_prob`: a multiple of the 128-item tile, chosen from (B, N) alone so that the
    row tiles (128 rows) x slices come to about two workgroups on each of the 256 compute units."""
    row_tiles = max(1, (B + 127) // 128)
    tiles = (N + 127) // 128
    slices = max(1, min(tiles, 512 // row_tiles))
    return (tiles + slices - 1) // slices * 128


def _current_derived(w, kind):
    """The cached layout `kind` of `w` if one exists and is current (see `_derived_of`), else None."""
    hit = _derived.get((id(w), kind))
    if hit is None or hit[0]() is not w or hit[1] != (w._version, w.data_ptr(), tuple(w.shape), _written.get(id(w), 0)):
        return None
    return hit[2]


def catalogue_log_prob(x, weight, bias, actions, *, dtype=None, items_per_slice=None, _x_padded=False):
    """(log_prob, lse), float32 [B] each, of the logits z = x weight^T + bias over the catalogue:
    lse = logsumexp(z, 1), log_prob = min(z[b, actions[b]] - lse[b], 0), not clamped below.  x float32 [B, K], weight [N, K],
    bias [N] or None, all finite; actions
    int64 [B]; an action outside [0, N) gives NaN in its row only.  One fused launch plus a per-row merge
    (recnn_catalogue_logprob): two floats per row and catalogue slice reach memory, never a [B, N] matrix.  `dtype` 'fp32' (exact
    fp32 MFMA) or 'bf16' (bf16 MFMA over the bf16 shadow of the weight, x rounded on load); None follows `set_catalogue_dtype`.
    Operands are zero-padded as `DiscretePolicyFunction` / `beta_train_forward` pad theirs, and the padded / bf16 copies of the
    weight are the ones those keep per weight version.  `items_per_slice` (a multiple of 128) defaults to
    `default_items_per_slice(B, N)`; with it fixed a row's bits do not depend on the batch around it.  No gradient is recorded."""
    return _catalogue_forward(_catalogue_operands(x, weight, bias, actions, dtype, items_per_slice, _x_padded))[:2]


def _catalogue_operands(x, weight, bias, actions, dtype, items_per_slice, _x_padded=False, _null_bias=False):
    """The checked, padded operands of one `recnn_catalogue_logprob` call: (xp, wp, c, act, B, N, K, Kp, bf16, ips).  `_null_bias`
    (the sampled kernels, which take NULL for it): no bias gives c = None instead of [N] zeros."""
    if not (x.is_cuda and weight.is_cuda):
        raise L.RecnnHipError("recnn_amd catalogue_log_prob: needs GPU tensors (no CPU fallback)")
    dtype = _catalogue_dtype if dtype is None else dtype
    if dtype not in ("fp32", "bf16"):
        raise ValueError(dtype)
    if x.dim() != 2 or weight.dim() != 2:
        raise ValueError(f"catalogue_log_prob: x {tuple(x.shape)} and weight {tuple(weight.shape)} must be matrices")
    B = x.shape[0]
    N, K = weight.shape
    dev = x.device
    bf16 = dtype == "bf16"
    Kp = _r128(K) if bf16 else _r64(K)
    # (_x_padded, discrete_log_prob's hidden layer: x comes [B, Kp] with zero columns past K and is used as it is)
    if x.shape[1] != (Kp if _x_padded else K):
        raise ValueError(f"catalogue_log_prob: x {tuple(x.shape)} does not match weight {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (N,):
        raise ValueError(f"catalogue_log_prob: bias {tuple(bias.shape)} does not match weight {tuple(weight.shape)}")
    xp = x.detach()
    if xp.dtype != torch.float32 or xp.shape[1] != Kp or xp.stride(1) != 1 or xp.stride(0) % 4 or xp.data_ptr() % 16:
        xp = _pad(xp.float(), B, Kp)
    if bf16:
        def shadow(w):
            t = torch.zeros(_r4(N), Kp, dtype=torch.bfloat16, device=dev)
            t[:N, :K] = w
            return t
        wp = _current_derived(weight, "bf16")       # the policy head's shadow [N, Kp], if DiscretePolicyFunction has made it
        if wp is None or wp.shape[1] != Kp:
            wp = _derived_of(weight, "bf16_padded", shadow)
    elif K != Kp or N != _r4(N) or weight.dtype != torch.float32 or not weight.is_contiguous() or weight.data_ptr() % 16:
        def padded(w):
            p = _pad(w.detach(), _r4(N), Kp)
            return p.clone() if p.data_ptr() % 16 else p      # (an aligned shape at an unaligned offset: a view into a larger tensor)
        wp = _derived_of(weight, "padded", padded)
    else:
        wp = weight.detach()
    c = (None if _null_bias else torch.zeros(N, device=dev)) if bias is None else bias.detach().float().contiguous()
    act = actions.detach().to(device=dev, dtype=torch.int64).contiguous()
    if act.shape != (B,):
        raise ValueError(f"catalogue_log_prob: {B} rows but actions of shape {tuple(act.shape)}")
    ips = default_items_per_slice(B, N) if items_per_slice is None else int(items_per_slice)
    return xp, wp, c, act, B, N, K, Kp, bf16, ips


def _catalogue_forward(ops):
    """(log_prob, lse, operands): the one `recnn_catalogue_logprob` call of `catalogue_log_prob` and `catalogue_log_prob_train`."""
    xp, wp, c, act, B, N, K, Kp, bf16, ips = ops
    dev = xp.device
    lp = torch.empty(B, device=dev)
    lse = torch.empty(B, device=dev)
    ws = L.workspace("recnn_catalogue_logprob_workspace_bytes", B, N, ips, device=dev)
    L.call("recnn_catalogue_logprob", L.ptr(xp), xp.stride(0), B, Kp, L.ptr(wp), wp.stride(0), int(bf16), L.ptr(c), N, L.ptr(act),
           ips, L.ptr(lp), L.ptr(lse), L.ptr(ws), L.current_stream())
    return lp, lse, ops


def action_ids(actions):
    """int64 ids of a batch of logged actions given as integer ids [B] or [B, 1], as a tensor made by `onehot_rows`, or as dense
    one-hot rows [B, n_items]."""
    integer = not (actions.dtype.is_floating_point or actions.dtype == torch.bool)
    if actions.dim() == 2 and actions.shape[1] == 1 and integer:
        actions = actions[:, 0]
    if actions.dim() == 1:
        if not integer:
            raise ValueError(f"action ids must be integers, got {actions.dtype}")
        return actions.to(torch.int64)
    if actions.dim() != 2:
        raise ValueError(f"actions must be ids [B] or one-hot rows [B, n_items], got shape {tuple(actions.shape)}")
    idx = onehot_index_of(actions)
    return idx if idx is not None else actions.argmax(1)


def discrete_log_prob(state, module, actions):
    """`catalogue_log_prob` of a DiscreteActor's head for given actions: the hidden layer by the GEMM kernel, nothing stored."""
    if not state.is_cuda:
        raise L.RecnnHipError("recnn_amd networks run on the GPU only (no CPU fallback): move the module and its inputs to 'cuda'")
    x = state.detach().float()
    B, K = x.shape
    w1 = module.linear1.weight
    H = w1.shape[0]
    Kp, Hp = _r64(K), (_r128(H) if _catalogue_dtype == "bf16" else _r64(H))
    h = torch.zeros(B, Hp, device=x.device)
    _fwd(_pad(x, B, Kp), Kp, _pad(w1, Hp, Kp), module.linear1.bias.detach().float().contiguous(), h, Hp, H, True, None)
    # h goes in at its padded width (its columns past H are zero): no second padded copy inside
    return catalogue_log_prob(h, module.linear2.weight, module.linear2.bias, action_ids(actions), _x_padded=True)


# ------------------------------------------------------------------------------------------------------------------------
# Next-item training (csrc/logprob_bwd.hip): the catalogue log-prob with its backward, and the full-softmax
# cross-entropy over it.  Neither pass stores a [B, n_items] matrix.

CATALOGUE_BWD_KMAX = 256       # padded width the backward's register-resident output tile is built for


def catalogue_bwd_items_per_slice(B, N, K):
    """Catalogue slice length of the dx kernel of `catalogue_log_prob_train`'s backward when none was given: a function of
    (B, N, K) alone.  Row tiles x slices come to about one workgroup per place on the 256 compute units: one place each, two where
    K <= 128 lets the fp32 kernel keep its output tile in half the register file."""
    row_tiles = max(1, (B + 127) // 128)
    tiles = (N + 127) // 128
    slices = max(1, min(tiles, (512 if K <= 128 else 256) // row_tiles))
    return (tiles + slices - 1) // slices * 128


def _padded_width(K, dtype):
    return _r128(K) if (_catalogue_dtype if dtype is None else dtype) == "bf16" else _r64(K)


class CatalogueLogProbFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, actions, dtype, items_per_slice):
        lp, lse, ops = _catalogue_forward(_catalogue_operands(x, weight, bias, actions, dtype, items_per_slice))
        ctx.ops, ctx.lse, ctx.user_ips = ops, lse.detach(), items_per_slice      # (detach: the output itself would tie ctx into a cycle)
        ctx.dtypes = (x.dtype, weight.dtype, None if bias is None else bias.dtype)
        ctx.save_for_backward(x, weight)       # (for autograd's check that neither was written in between)
        ctx.set_materialize_grads(False)
        return lp, lse

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_lp, g_lse):
        ctx.saved_tensors
        xp, wp, c, act, B, N, K, Kp, bf16, _ = ctx.ops
        need_x, need_w, need_c = ctx.needs_input_grad[:3]
        need_c = need_c and ctx.dtypes[2] is not None
        if (g_lp is None and g_lse is None) or not (need_x or need_w or need_c):
            return None, None, None, None, None, None
        dev = xp.device
        g_lp = None if g_lp is None else g_lp.float().contiguous()
        g_lse = None if g_lse is None else g_lse.float().contiguous()
        ips = catalogue_bwd_items_per_slice(B, N, K) if ctx.user_ips is None else int(ctx.user_ips)
        dx = torch.empty(B, Kp, device=dev) if need_x else None
        dw = torch.empty(N, Kp, device=dev) if need_w else None
        dc = torch.empty(N, device=dev) if need_c else None
        ws = L.workspace("recnn_catalogue_logprob_bwd_workspace_bytes", B, N, Kp, ips, device=dev) if need_x else None
        L.call("recnn_catalogue_logprob_bwd", L.ptr(xp), xp.stride(0), B, Kp, L.ptr(wp), wp.stride(0), int(bf16), L.ptr(c), N, L.ptr(act),
               L.ptr(ctx.lse), L.ptr(g_lp), L.ptr(g_lse), ips, L.ptr(dx), Kp, L.ptr(dw), Kp, L.ptr(dc), L.ptr(ws), L.current_stream())

        def strip(t, dt):
            if t is None:
                return None
            t = t if K == Kp else t[:, :K].contiguous()
            return t if t.dtype == dt else t.to(dt)
        return strip(dx, ctx.dtypes[0]), strip(dw, ctx.dtypes[1]), (None if dc is None else dc.to(ctx.dtypes[2])), None, None, None


def catalogue_log_prob_train(x, weight, bias, actions, *, dtype=None, items_per_slice=None):
    """`catalogue_log_prob` with a gradient: (log_prob, lse) with the bits `catalogue_log_prob` gives on the same inputs (the very
    same call, padding, cached weight copies and default slice length), attached to x, weight and bias.  The backward is one
    `recnn_catalogue_logprob_bwd` call (csrc/logprob_bwd.hip): with p = exp(z - lse) and D = (g_lse - g_lp) p + g_lp [n == a] it
    returns dx = D W, dW = D^T x and dbias = sum_b D, D recomputed tile by tile and never stored; only the gradients that are
    needed are computed.  The derivative is that of z_a - lse (the forward's clamp at 0 is a rounding guard).  A row whose action
    lies outside [0, n_items) gives NaN in its log_prob, as in `catalogue_log_prob`, and its log_prob gradient counts as 0: no
    NaN reaches any gradient, and its lse gradient still flows.  The padded width of K (a multiple of 64, of 128 in bf16 mode)
    may not exceed 256; a wider product is refused before anything is launched (the policy head of `DiscreteActor` and `Beta`,
    2048 and 1290 wide, stay on their own training paths).  The dx kernel's slice length is `items_per_slice` when given, else
    `catalogue_bwd_items_per_slice(B, N, K)`; with it fixed a row's dx bits do not depend on the batch around it.  No float
    atomics: equal calls give equal bits.  Not twice differentiable."""
    if weight.dim() == 2 and _padded_width(weight.shape[1], dtype) > CATALOGUE_BWD_KMAX:
        raise ValueError(f"catalogue_log_prob_train: K = {weight.shape[1]} pads to {_padded_width(weight.shape[1], dtype)}, above the "
                         f"backward's limit of {CATALOGUE_BWD_KMAX} (its output tile is register-resident; there is no K-chunked path)")
    return CatalogueLogProbFunction.apply(x, weight, bias, actions, dtype, items_per_slice)


def catalogue_cross_entropy(x, weight, bias, targets, *, reduction="mean", ignore_index=-100, dtype=None):
    """Full-softmax cross-entropy of the logits x weight^T + bias against `targets` (int64 [B]) without the logits:
    -`catalogue_log_prob_train(...)[0]`, reduced by `reduction` ('mean', 'sum' or 'none').  Rows whose target equals `ignore_index`
    contribute 0 and are left out of the mean (torch.nn.functional.cross_entropy's semantics, for padded sequences); any other
    target outside [0, n_items) raises ValueError."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"catalogue_cross_entropy: reduction {reduction!r} is not 'mean', 'sum' or 'none'")
    if not (x.is_cuda and weight.is_cuda):
        raise L.RecnnHipError("recnn_amd catalogue_cross_entropy: needs GPU tensors (no CPU fallback)")
    t = action_ids(targets).to(x.device)
    keep = t != int(ignore_index)
    N = weight.shape[0]
    if bool((keep & ((t < 0) | (t >= N))).any()):
        raise ValueError(f"catalogue_cross_entropy: a target lies outside [0, {N}) and is not ignore_index = {ignore_index}")
    lp, _ = catalogue_log_prob_train(x, weight, bias, torch.where(keep, t, torch.full_like(t, -1)), dtype=dtype)
    loss = torch.where(keep, -lp, torch.zeros_like(lp))
    if reduction == "none":
        return loss
    return loss.sum() if reduction == "sum" else loss.sum() / keep.sum()


# ------------------------------------------------------------------------------------------------------------------------
# Sampled softmax with negatives shared by the batch (csrc/sampled.hip): the target against S sampled items, with
# the log-Q correction and accidental-hit removal.  Neither pass stores a [B, S] matrix or a gathered [S, K] copy of the table.

def _sampled_operands(x, weight, bias, targets, negatives, target_log_q, negative_log_q, dtype, items_per_slice):
    """The checked operands of the sampled kernels: `_catalogue_operands`' padding and weight shadows, then the negatives and
    corrections.  (xp, wp, c or None, act, neg, tq, nq, B, S, N, K, Kp, bf16)."""
    if not (isinstance(negatives, torch.Tensor) and negatives.is_cuda):
        raise L.RecnnHipError("recnn_amd sampled_log_prob_train: needs GPU tensors (no CPU fallback)")
    xp, wp, c, act, B, N, K, Kp, bf16, _ = _catalogue_operands(x, weight, bias, targets, dtype, 128, _null_bias=True)
    dev = xp.device
    if negatives.dim() != 1 or negatives.dtype.is_floating_point or negatives.dtype == torch.bool:
        raise ValueError(f"sampled_log_prob_train: negatives must be integer ids [S], got {negatives.dtype} {tuple(negatives.shape)}")
    neg = negatives.detach().to(device=dev, dtype=torch.int64).contiguous()
    S = neg.shape[0]
    if S == 0:
        raise ValueError("sampled_log_prob_train: S = 0: the list of negatives is empty (at least one is needed)")

    def corr(t, n, name):
        if t is None:
            return None
        if tuple(t.shape) != (n,):
            raise ValueError(f"sampled_log_prob_train: {name} of shape {tuple(t.shape)} does not match its {n} ids")
        return t.detach().to(device=dev, dtype=torch.float32).contiguous()
    tq, nq = corr(target_log_q, B, "target_log_q"), corr(negative_log_q, S, "negative_log_q")
    if items_per_slice is not None and (int(items_per_slice) < 128 or int(items_per_slice) % 128):
        raise ValueError(f"sampled_log_prob_train: items_per_slice must be a positive multiple of 128, got {items_per_slice}")
    return xp, wp, c, act, neg, tq, nq, B, S, N, K, Kp, bf16


class SampledLogProbFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, targets, negatives, target_log_q, negative_log_q, remove_hits, dtype, items_per_slice, sparse_grad):
        ops = _sampled_operands(x, weight, bias, targets, negatives, target_log_q, negative_log_q, dtype, items_per_slice)
        xp, wp, c, act, neg, tq, nq, B, S, N, K, Kp, bf16 = ops
        dev = xp.device
        lp, lse, zt = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)
        if B:
            ips = default_items_per_slice(B, S) if items_per_slice is None else int(items_per_slice)
            ws = L.workspace("recnn_sampled_logprob_workspace_bytes", B, S, ips, device=dev)
            L.call("recnn_sampled_logprob", L.ptr(xp), xp.stride(0), B, Kp, L.ptr(wp), wp.stride(0), int(bf16), L.ptr(c), N, L.ptr(act),
                   L.ptr(neg), S, L.ptr(tq), L.ptr(nq), int(bool(remove_hits)), ips, L.ptr(lp), L.ptr(lse), L.ptr(zt), L.ptr(ws),
                   L.current_stream())
        ctx.ops, ctx.lse, ctx.zt, ctx.user_ips = ops, lse.detach(), zt, items_per_slice
        ctx.remove_hits, ctx.sparse = bool(remove_hits), bool(sparse_grad)
        ctx.dtypes = (x.dtype, weight.dtype, None if bias is None else bias.dtype)
        ctx.save_for_backward(x, weight)       # (for autograd's check that neither was written in between)
        ctx.set_materialize_grads(False)
        return lp, lse

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_lp, g_lse):
        ctx.saved_tensors
        xp, wp, c, act, neg, tq, nq, B, S, N, K, Kp, bf16 = ctx.ops
        need_x, need_w, need_c = ctx.needs_input_grad[:3]
        need_c = need_c and ctx.dtypes[2] is not None
        none = (None,) * 11
        if (g_lp is None and g_lse is None) or not (need_x or need_w or need_c):
            return none
        dev = xp.device

        def strip(t, dt):
            t = t if K == Kp else t[:, :K].contiguous()
            return t if t.dtype == dt else t.to(dt)
        if B == 0:      # nothing to launch: exact zeros
            gw = None
            if need_w:
                gw = (torch.sparse_coo_tensor(torch.empty(1, 0, dtype=torch.int64, device=dev), torch.empty(0, K, device=dev), (N, K))
                      if ctx.sparse else torch.zeros(N, K, device=dev)).to(ctx.dtypes[1])
            return (torch.zeros(0, K, device=dev, dtype=ctx.dtypes[0]) if need_x else None, gw,
                    torch.zeros(N, device=dev, dtype=ctx.dtypes[2]) if need_c else None) + none[3:]
        g_lp = None if g_lp is None else g_lp.float().contiguous()
        g_lse = None if g_lse is None else g_lse.float().contiguous()
        ips = catalogue_bwd_items_per_slice(B, S, K) if ctx.user_ips is None else int(ctx.user_ips)
        sparse_w = need_w and ctx.sparse
        dx = torch.empty(B, Kp, device=dev) if need_x else None
        dws = torch.empty(S, Kp, device=dev) if need_w else None
        dcs = torch.empty(S, device=dev) if need_c else None
        dt = torch.empty(B, device=dev)
        dwt = torch.empty(B, Kp, device=dev) if sparse_w else None
        ws = L.workspace("recnn_sampled_logprob_bwd_workspace_bytes", B, S, Kp, ips, device=dev)
        L.call("recnn_sampled_logprob_bwd", L.ptr(xp), xp.stride(0), B, Kp, L.ptr(wp), wp.stride(0), int(bf16), L.ptr(c), N, L.ptr(act),
               L.ptr(neg), S, L.ptr(nq), int(ctx.remove_hits), L.ptr(ctx.lse), L.ptr(ctx.zt), L.ptr(g_lp), L.ptr(g_lse), ips,
               L.ptr(dx), Kp, L.ptr(dws), Kp, L.ptr(dcs), L.ptr(dt), L.ptr(dwt), Kp, L.ptr(ws), L.current_stream())
        gw = gc = None
        dense_w = need_w and not ctx.sparse
        if dense_w or need_c:
            dw = torch.empty(N, Kp, device=dev) if dense_w else None
            gc = torch.empty(N, device=dev) if need_c else None
            ws2 = L.workspace("recnn_sampled_scatter_workspace_bytes", B, S, N, Kp, device=dev)
            L.call("recnn_sampled_scatter", L.ptr(neg), S, L.ptr(act), B, L.ptr(dws), Kp, L.ptr(dcs), L.ptr(xp), xp.stride(0), int(bf16),
                   L.ptr(dt), Kp, N, L.ptr(dw), Kp, L.ptr(gc), L.ptr(ws2), L.current_stream())
            if dense_w:
                gw = strip(dw, ctx.dtypes[1])
            if need_c:
                gc = gc.to(ctx.dtypes[2])
        if sparse_w:
            # uncoalesced: one entry per valid negative, then one per valid target; nothing of size n_items is written
            keep_n, keep_t = (neg >= 0) & (neg < N), (act >= 0) & (act < N)
            idx = torch.cat([neg[keep_n], act[keep_t]])
            val = torch.cat([dws[keep_n], dwt[keep_t]])
            gw = torch.sparse_coo_tensor(idx[None], strip(val, ctx.dtypes[1]), (N, K))
        return (strip(dx, ctx.dtypes[0]) if need_x else None, gw, gc) + none[3:]


def sampled_log_prob_train(x, weight, bias, targets, negatives, *, target_log_q=None, negative_log_q=None, remove_accidental_hits=True,
                           dtype=None, items_per_slice=None, sparse_grad=False):
    """(log_prob, lse), float32 [B] each, of the sampled softmax of x [B, K] over `targets` [B] and the negatives [S] that every row
    shares (repeats allowed), with gradients to x, weight [N, K] and bias ([N] or None):

        z_t[b] = x_b . W[a_b] + c[a_b] - target_log_q[b]        z[b, s] = x_b . W[n_s] + c[n_s] - negative_log_q[s]
        lse[b] = log(exp z_t[b] + sum_s exp z[b, s])            log_prob[b] = min(z_t[b] - lse[b], 0)

    `remove_accidental_hits`: a negative equal to a row's target is left out of that row (no probability, no gradient).  A negative
    outside [0, N) is left out of every row (-1 padding).  A target outside [0, N) gives NaN in its log_prob only, its lse is taken
    over the negatives, its log_prob gradient counts as 0 and its lse gradient still flows.  S = 0 and a K that pads above 256
    are refused by name before any launch.  In-batch negatives are `negatives=targets`.
    Forward: `recnn_sampled_logprob`; backward: `recnn_sampled_logprob_bwd` (dx and one compact gradient row per negative) and
    `recnn_sampled_scatter`, which sums the S + B contributions by item id into the dense [N, K] / [N] gradients (csrc/sampled.hip);
    the rows of the table are read through the ids, so neither a [B, S] matrix nor a gathered [S, K] copy exists.  Operands are
    padded and shadowed as `catalogue_log_prob` pads them; `dtype` 'fp32' or 'bf16' as there, gradients fp32 either way.
    `sparse_grad=True`: the weight gradient is an uncoalesced `torch.sparse_coo_tensor` [N, K] with indices cat(valid negatives,
    valid targets) and the compact rows as values -- for `torch.optim.SparseAdam`; no [N, K] tensor is made, and no scatter launch
    unless the bias needs its (dense) gradient.  `items_per_slice` (a multiple of 128) cuts the negatives; it defaults to
    `default_items_per_slice(B, S)` forward and `catalogue_bwd_items_per_slice(B, S, K)` backward, and with it fixed a row's
    log_prob, lse and dx bits do not depend on the batch around it.  No float atomics: equal calls give equal bits.  Not twice
    differentiable."""
    if weight.dim() == 2 and _padded_width(weight.shape[1], dtype) > CATALOGUE_BWD_KMAX:
        raise ValueError(f"sampled_log_prob_train: K = {weight.shape[1]} pads to {_padded_width(weight.shape[1], dtype)}, above the "
                         f"kernels' limit of {CATALOGUE_BWD_KMAX} (their output tile is register-resident; there is no K-chunked path)")
    return SampledLogProbFunction.apply(x, weight, bias, targets, negatives, target_log_q, negative_log_q, remove_accidental_hits, dtype,
                                        items_per_slice, sparse_grad)


def sampled_cross_entropy(x, weight, bias, targets, negatives, *, target_log_q=None, negative_log_q=None, reduction="mean",
                          ignore_index=-100, remove_accidental_hits=True, dtype=None, items_per_slice=None, sparse_grad=False):
    """Sampled-softmax cross-entropy: -`sampled_log_prob_train(...)[0]`, reduced by `reduction` ('mean', 'sum' or 'none') with
    `catalogue_cross_entropy`'s semantics: rows whose target equals `ignore_index` contribute 0 and are left out of the mean; any
    other target outside [0, n_items) raises ValueError."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"sampled_cross_entropy: reduction {reduction!r} is not 'mean', 'sum' or 'none'")
    if not (x.is_cuda and weight.is_cuda):
        raise L.RecnnHipError("recnn_amd sampled_cross_entropy: needs GPU tensors (no CPU fallback)")
    t = action_ids(targets).to(x.device)
    keep = t != int(ignore_index)
    N = weight.shape[0]
    if bool((keep & ((t < 0) | (t >= N))).any()):
        raise ValueError(f"sampled_cross_entropy: a target lies outside [0, {N}) and is not ignore_index = {ignore_index}")
    lp, _ = sampled_log_prob_train(x, weight, bias, torch.where(keep, t, torch.full_like(t, -1)), negatives, target_log_q=target_log_q,
                                   negative_log_q=negative_log_q, remove_accidental_hits=remove_accidental_hits, dtype=dtype,
                                   items_per_slice=items_per_slice, sparse_grad=sparse_grad)
    loss = torch.where(keep, -lp, torch.zeros_like(lp))
    if reduction == "none":
        return loss
    return loss.sum() if reduction == "sum" else loss.sum() / keep.sum()


def onehot_rows(idx, n):
    """float[B, n] one-hot rows of int64 indices (recnn/data/utils.py:108-109: zeros + scatter_).  The result remembers
    its indices (`onehot_index`): a Critic reading it gathers the B weight columns instead of multiplying a [B, n] matrix
    of zeros (`mlp_onehot`)."""
    B = idx.numel()
    ld = _r4(n)
    idx = idx.to(torch.int64).contiguous()
    if B:
        lo, hi = torch.aminmax(idx)
        if int(lo) < 0 or int(hi) >= n:      # the reference's scatter_ raises for such ids (utils.py:108-109)
            raise IndexError(f"onehot_rows: index range [{int(lo)}, {int(hi)}] outside the catalogue [0, {n})")
    out = torch.empty(B, ld, dtype=torch.float32, device=idx.device)
    L.call("recnn_onehot_rows", L.ptr(idx), B, n, L.ptr(out), ld, L.current_stream())
    out = out if ld == n else out[:, :n]
    out.onehot_index = (idx, out._version)
    return out


def onehot_index_of(t):
    """The indices of a tensor made by `onehot_rows`, or None (also when it was written to since)."""
    tag = getattr(t, "onehot_index", None)
    if tag is None or tag[1] != t._version or tag[0].numel() != t.shape[0]:
        return None
    return tag[0]


class OneHotLayer1Function(torch.autograd.Function):
    """(W1[:, :S], W1[:, S + idx]^T) of a critic's first layer over [state | one-hot action].  Written as plain slicing +
    index_select, autograd answers with TWO catalogue-wide gradients for W1 -- zeros(W1) with the state block copied in, zeros(W1)
    with the columns scattered -- a clone and an add_ over them (at [2048, 101290]: two 830 MB fills, a copy and an add per step,
    1.2 ms); this node builds the ONE dense gradient the optimizer reads: a fill and two small writes."""

    @staticmethod
    def forward(ctx, w1, idx, n_state):
        ctx.save_for_backward(idx)
        ctx.meta = (tuple(w1.shape), int(n_state))
        return w1[:, :n_state].contiguous(), w1.index_select(1, idx + n_state).t().contiguous()

    @staticmethod
    def backward(ctx, g_state, g_cols):
        (idx,) = ctx.saved_tensors
        shape, n_state = ctx.meta
        ref = g_state if g_state is not None else g_cols
        g = torch.zeros(shape, dtype=torch.float32, device=ref.device)
        if g_state is not None:
            g[:, :n_state] = g_state
        if g_cols is not None:
            g.index_add_(1, idx + n_state, g_cols.t().float())
        return g, None, None


def mlp_onehot(state, idx, n_state, module, train: bool):
    """`mlp(cat([state, onehot(idx)], 1))` without the one-hot operand: layer 1 is state W1[:, :S]^T + W1[:, S + idx]^T + b1
    (the column gather enters the GEMM epilogue before the relu); autograd scatters the gathered columns' gradient back."""
    w1 = module.linear1.weight
    w_state, cols = OneHotLayer1Function.apply(w1, idx, n_state)           # [H, S], [B, H]
    return MLPFunction.apply(state.float(), w_state, module.linear1.bias, module.linear2.weight, module.linear2.bias,
                             module.linear3.weight, module.linear3.bias, train, torch.initial_seed(),
                             _take_forced_masks(module, train), cols)


# ------------------------------------------------------------------------------------------------------------------------
# The reference's debugging autoencoder (recnn/nn/models.py:7-38, `AnomalyDetector`) over csrc/anomaly.hip.
# Replaces the Sequential's addmm / relu / batch_norm chain, `sum((x - ae(x)) ** 2, 1)` and their autograd backward.

_AE_WIDTHS = ((128, 64), (64, 32), (32, 64), (64, 128))


def _ae_layers(ae):
    """(the four Linear modules, the three BatchNorm1d modules) of the reference's Sequential, checked."""
    lins, bns = [ae[0], ae[3], ae[6], ae[9]], [ae[2], ae[5], ae[8]]
    for lin, (i, o) in zip(lins, _AE_WIDTHS):
        if lin.in_features != i or lin.out_features != o or lin.bias is None:
            raise ValueError(f"AnomalyDetector: expected Linear({i}, {o}) with bias, got {lin}")
    for bn in bns:
        if bn.momentum is None:
            raise NotImplementedError("AnomalyDetector: BatchNorm1d(momentum=None) (cumulative average) is not supported")
        if not bn.affine:
            raise NotImplementedError("AnomalyDetector: BatchNorm1d(affine=False) is not supported")
        if not bn.track_running_stats:
            raise NotImplementedError("AnomalyDetector: BatchNorm1d(track_running_stats=False) is not supported")
    return lins, bns


def _ae_params(lins, bns, tensors=None):
    """recnn_ae_params for the modules; `tensors` (w0, b0, ..., w3, b3, g0, be0, ..., g2, be2) overrides the parameters."""
    if tensors is None:
        tensors = [t for lin in lins for t in (lin.weight, lin.bias)] + [t for bn in bns for t in (bn.weight, bn.bias)]
    for t in tensors:
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16:
            raise L.RecnnHipError("recnn_amd AnomalyDetector: parameters must be contiguous float32 GPU tensors")
    p = L.AeParams()
    for i in range(4):
        p.w[i], p.b[i] = tensors[2 * i].data_ptr(), tensors[2 * i + 1].data_ptr()
    for i, bn in enumerate(bns):
        p.gamma[i], p.beta[i] = tensors[8 + 2 * i].data_ptr(), tensors[9 + 2 * i].data_ptr()
        for name in ("running_mean", "running_var"):
            buf = getattr(bn, name)
            if not buf.is_cuda or buf.dtype != torch.float32 or not buf.is_contiguous():
                raise L.RecnnHipError(f"recnn_amd AnomalyDetector: BatchNorm {name} must be a contiguous float32 GPU tensor")
            getattr(p, name)[i] = buf.data_ptr()
        p.num_batches_tracked[i] = bn.num_batches_tracked.data_ptr()
        p.eps[i], p.momentum[i] = float(bn.eps), float(bn.momentum)
    return p


def _ae_input(x):
    if not x.is_cuda:
        raise L.RecnnHipError("recnn_amd AnomalyDetector: needs GPU tensors (no CPU fallback)")
    if x.dim() != 2 or x.shape[1] != 128 or x.dtype != torch.float32:
        raise ValueError(f"AnomalyDetector: input must be float32 [rows, 128], got {tuple(x.shape)} {x.dtype}")
    if x.stride(1) != 1 or x.stride(0) < 128 or x.data_ptr() % 16 or x.stride(0) % 4:
        x = x.contiguous()
    return x


def _ae_run(x, lins, bns, train, want_err, keep, tensors=None):
    """(out or err, act, workspace): one eval launch, or the four-launch forward when training or keeping activations."""
    rows = x.shape[0]
    if train and rows < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    p = _ae_params(lins, bns, tensors)
    res = torch.empty(rows, device=x.device) if want_err else torch.empty(rows, 128, device=x.device)
    err, out = (res, None) if want_err else (None, res)
    if rows == 0:
        return res, None, None
    if not train and not keep:
        L.call("recnn_ae_eval", C.byref(p), L.ptr(x), x.stride(0), rows, L.ptr(out), 128, L.ptr(err), L.current_stream())
        return res, None, None
    act = L.workspace("recnn_ae_act_floats", rows, device=x.device)
    ws = L.workspace("recnn_ae_workspace_bytes", rows, device=x.device)
    L.call("recnn_ae_forward", C.byref(p), int(train), L.ptr(x), x.stride(0), rows, L.ptr(out), 128, L.ptr(err), L.ptr(act),
           int(keep), L.ptr(ws), L.current_stream())
    return res, act, ws


class AnomalyDetectorFunction(torch.autograd.Function):
    """out = ae(x) for the reference's autoencoder Sequential `ae`; train mode normalises with batch statistics and updates the
    running ones (as BatchNorm1d does, with or without grad), eval mode uses the running statistics."""

    @classmethod
    def apply(cls, x, ae, train, *tensors):
        # (Function.forward runs with grad mode off: whether a backward can exist is decided here)
        return super().apply(x, ae, train, torch.is_grad_enabled(), *tensors)

    @staticmethod
    def forward(ctx, x, ae, train, grad_mode, *tensors):
        lins, bns = _ae_layers(ae)
        xin = _ae_input(x)
        keep = bool(grad_mode and (x.requires_grad or any(t.requires_grad for t in tensors)))
        out, act, ws = _ae_run(xin, lins, bns, train, False, keep and xin.shape[0] > 0, tensors)
        ctx.train, ctx.bns = bool(train), bns
        if keep:
            ctx.save_for_backward(xin, out, act, ws, *tensors)
        return out

    @staticmethod
    def backward(ctx, dout):
        xin, out, act, ws, *tensors = ctx.saved_tensors
        rows = xin.shape[0]
        grads = [torch.empty_like(t) for t in tensors]
        dx = torch.empty(rows, 128, device=xin.device) if ctx.needs_input_grad[0] else None
        if rows == 0:
            return (None if dx is None else dx, None, None, None, *[g.zero_() for g in grads])
        dout = dout.float()
        if dout.stride(1) != 1 or dout.stride(0) < 128:
            dout = dout.contiguous()
        p = _ae_params(None, ctx.bns, tensors)
        g = L.AeGrads()
        for i in range(4):
            g.w[i], g.b[i] = grads[2 * i].data_ptr(), grads[2 * i + 1].data_ptr()
        for i in range(3):
            g.gamma[i], g.beta[i] = grads[8 + 2 * i].data_ptr(), grads[9 + 2 * i].data_ptr()
        L.call("recnn_ae_backward", C.byref(p), C.byref(g), int(ctx.train), L.ptr(xin), xin.stride(0), rows, L.ptr(out), 128,
               L.ptr(dout), dout.stride(0), L.ptr(act), L.ptr(dx), 128, L.ptr(ws), L.current_stream())
        need = ctx.needs_input_grad[4:]
        return (dx, None, None, None, *[gr if nd else None for gr, nd in zip(grads, need)])


def _ae_tensors(lins, bns):
    return [t for lin in lins for t in (lin.weight, lin.bias)] + [t for bn in bns for t in (bn.weight, bn.bias)]


def anomaly_forward(x, ae, train: bool):
    """ae(x) for the reference's AnomalyDetector Sequential on the HIP kernels (differentiable)."""
    lins, bns = _ae_layers(ae)
    return AnomalyDetectorFunction.apply(x, ae, bool(train), *_ae_tensors(lins, bns))


def anomaly_rec_error(x, ae, train: bool):
    """sum((x - ae(x)) ** 2, 1), fused: the 128-wide output is never stored.  Not differentiable (the reference detaches it);
    in train mode the running statistics are updated, as the reference's train-mode call does."""
    lins, bns = _ae_layers(ae)
    xin = _ae_input(x)
    err, _, _ = _ae_run(xin, lins, bns, bool(train), True, False)
    return err


# ------------------------------------------------------------------------------------------------------------------------
# Dueling DQN of the embeddings notebook (csrc/dqn.hip): Q = V + A - mean(A) with A = h W^T + c over the catalogue.
# The trunk (feature, advantage.0 and value.0 as ONE stacked [256, 128] layer) runs on the GEMM kernels; the catalogue head, the mean
# and the head's gradients on csrc/dqn.hip.  The learn step itself (recnn_amd/nn/update/dqn.py) reuses these pieces.
DQN_HIDDEN = 128


def dqn_colsum(x, rows, cols, scale=1.0, out=None):
    """float[cols]: scale * column sums of x[:rows, :cols] (row stride x.stride(0)) in a fixed order."""
    ws = L.workspace("recnn_dqn_colsum_workspace_floats", rows, cols, device=x.device)
    out = torch.empty(cols, dtype=torch.float32, device=x.device) if out is None else out
    L.call("recnn_dqn_colsum", L.ptr(x), x.stride(0) if x.dim() == 2 else 1, rows, cols, float(scale), L.ptr(out), L.ptr(ws),
           L.current_stream())
    return out


def dqn_row_dot(x, w, idx=None, bias=None, out=None):
    """float[rows]: x_b . w[idx_b] + bias[idx_b] over 128 columns (idx None: row 0 of w)."""
    rows = x.shape[0]
    out = torch.empty(rows, dtype=torch.float32, device=x.device) if out is None else out
    L.call("recnn_dqn_row_dot", L.ptr(x), x.stride(0), rows, L.ptr(w), w.stride(0), L.ptr(idx), w.shape[0], L.ptr(bias), L.ptr(out),
           L.current_stream())
    return out


def dqn_head_weight(w):
    """(operand, is_bf16) of the catalogue weight [N, 128] in the current catalogue compute type (bf16: a copy per weight version)."""
    if _catalogue_dtype == "bf16":
        return _derived_of(w, "bf16_dqn", lambda t: t.to(torch.bfloat16).contiguous()), 1
    return w.detach(), 0


def dqn_head(h, w, c, V=None, mu=None, rowmax=False):
    """The catalogue GEMM: Q [B, N] = h W^T + c + V - mu (store), or the int32 order-preserving image of max_n (h W^T + c)_n."""
    B, N = h.shape[0], w.shape[0]
    wop, bf = dqn_head_weight(w)
    s = L.current_stream()
    if rowmax:
        out = torch.empty(B, dtype=torch.int32, device=h.device)
        L.call("recnn_dqn_head", L.ptr(h), h.stride(0), B, L.ptr(wop), wop.stride(0), bf, L.ptr(c), N, None, None, None, 0, L.ptr(out), s)
    else:
        out = torch.empty(B, N, dtype=torch.float32, device=h.device)
        L.call("recnn_dqn_head", L.ptr(h), h.stride(0), B, L.ptr(wop), wop.stride(0), bf, L.ptr(c), N, L.ptr(V), L.ptr(mu), L.ptr(out), N,
               None, s)
    return out


def ord_to_float(t):
    """Decode recnn_dqn_head's row-max image (int32) to float32."""
    i = t.to(torch.int32)
    return torch.where(i >= 0, i, i ^ 0x7FFFFFFF).view(torch.float32)


def dqn_check_net(net):
    """(feature Linear, stacked (advantage.0, value.0), advantage.2, value.2) of a DuelDQN-shaped module, checked."""
    try:
        l0, la0, la2, lv0, lv2 = net.feature[0], net.advantage[0], net.advantage[2], net.value[0], net.value[2]
    except (AttributeError, IndexError, TypeError):
        raise ValueError("expected a DuelDQN-shaped module (feature / advantage / value Sequentials)") from None
    if l0.out_features != DQN_HIDDEN or la0.in_features != DQN_HIDDEN or la0.out_features != DQN_HIDDEN or \
            lv0.out_features != DQN_HIDDEN or lv2.out_features != 1 or la2.in_features != DQN_HIDDEN:
        raise ValueError(f"DuelDQN kernels need hidden width {DQN_HIDDEN}")
    for p in net.parameters():
        if not p.is_cuda:
            raise L.RecnnHipError("recnn_amd DuelDQN runs on the GPU only (no CPU fallback): move the module and its inputs to 'cuda'")
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise L.RecnnHipError("recnn_amd DuelDQN: parameters must be contiguous float32")
    return l0, la0, la2, lv0, lv2


def dqn_trunk(net, x, K, Kp):
    """(f [B, 128], h2 = [ha | hv] [B, 256], padded feature weight [128, Kp], stacked weight [256, 128]) for x [B, >= Kp] whose
    columns K .. Kp are zero."""
    l0, la0, _, lv0, _ = dqn_check_net(net)
    B = x.shape[0]
    dev = x.device
    w0p = _derived_of(l0.weight, f"dqn_pad{Kp}", lambda w: _pad(w, DQN_HIDDEN, Kp))
    w12 = torch.cat([la0.weight.detach(), lv0.weight.detach()], 0)
    b12 = torch.cat([la0.bias.detach(), lv0.bias.detach()], 0)
    f = torch.empty(B, DQN_HIDDEN, device=dev)
    h2 = torch.empty(B, 2 * DQN_HIDDEN, device=dev)
    if B:
        _fwd(x, Kp, w0p, l0.bias.detach(), f, DQN_HIDDEN, DQN_HIDDEN, True, None)
        _fwd(f, DQN_HIDDEN, w12, b12, h2, 2 * DQN_HIDDEN, 2 * DQN_HIDDEN, True, None)
    return f, h2, w0p, w12


def dqn_head_stats(h2, B, w, c):
    """(sum_b ha_b, sum_n W_n, sum_n c_n): the three column sums mean(A) is made of."""
    N = w.shape[0]
    return dqn_colsum(h2, B, DQN_HIDDEN), dqn_colsum(w.detach(), N, DQN_HIDDEN), dqn_colsum(c.detach().view(N, 1), N, 1)


def dqn_trunk_backward(dh, f, x, K, Kp, w0p, w12, gw0, gb0, gw12, gb12, want_dx):
    """Gradients of the trunk from dh = d[ha | hv] (pre-activation, [B, 256]): written into gw0 [128, K], gb0, gw12 [256, 128], gb12;
    returns d x [B, Kp] (or None)."""
    B = dh.shape[0]
    dev = dh.device
    _dw(dh, 2 * DQN_HIDDEN, f, DQN_HIDDEN, gw12)
    dqn_colsum(dh, B, 2 * DQN_HIDDEN, out=gb12)
    df = torch.empty(B, DQN_HIDDEN, device=dev)
    _dx(dh, 2 * DQN_HIDDEN, w12, DQN_HIDDEN, df, f, 1.0, None)
    dw0 = torch.empty(DQN_HIDDEN, Kp, device=dev)
    _dw(df, DQN_HIDDEN, x, Kp, dw0)
    gw0.copy_(dw0[:, :K])
    dqn_colsum(df, B, DQN_HIDDEN, out=gb0)
    if not want_dx:
        return None
    dx = torch.empty(B, Kp, device=dev)
    _dx(df, DQN_HIDDEN, w0p, Kp, dx, None, 1.0, None)
    return dx


class DuelDQNFunction(torch.autograd.Function):
    """Q = DuelDQN(x) [B, N] and its backward for any upstream dQ: dV = rowsum(dQ), dA = dQ - sum(dQ) / (B N)."""

    @staticmethod
    def forward(ctx, x, net, *params):
        if not x.is_cuda:
            raise L.RecnnHipError("recnn_amd DuelDQN runs on the GPU only (no CPU fallback): move the module and its inputs to 'cuda'")
        _, _, la2, _, lv2 = dqn_check_net(net)
        B, K = x.shape
        Kp = _r64(K)
        xp = _pad(x, B, Kp)
        f, h2, w0p, w12 = dqn_trunk(net, xp, K, Kp)
        W, c = la2.weight.detach(), la2.bias.detach()
        N = W.shape[0]
        V = dqn_row_dot(h2[:, DQN_HIDDEN:], lv2.weight.detach(), None, lv2.bias.detach())
        sh, sw, sc = dqn_head_stats(h2, B, W, c)
        mu = torch.empty(1, device=x.device)
        if B:
            L.call("recnn_dqn_mean", L.ptr(sh), L.ptr(sw), L.ptr(sc), B, N, L.ptr(mu), L.current_stream())
        Q = dqn_head(h2, W, c, V, mu)
        ctx.net = net
        ctx.params = params
        ctx.dims = (B, K, Kp, N)
        ctx.save_for_backward(xp, f, h2, w0p, w12, sh, sw)
        return Q

    @staticmethod
    def backward(ctx, dQ):
        xp, f, h2, w0p, w12, sh, sw = ctx.saved_tensors
        B, K, Kp, N = ctx.dims
        net = ctx.net
        l0, la0, la2, lv0, lv2 = dqn_check_net(net)
        dev = dQ.device
        H = DQN_HIDDEN
        N4 = _r4(N)
        dQp = torch.zeros(B, N4, device=dev)
        dQp[:, :N] = dQ
        s = dQp.sum() / (B * N)                      # d mean(A) seed, on the device
        dV = dQp.sum(1)
        ha, hv = h2[:, :H], h2[:, H:]
        W = la2.weight.detach()
        gW = torch.empty(N, H, device=dev)
        # dQ^T ha: contraction over the batch; the product reads dQ in whole 64-column tiles along N (recnn_gemm_args: pitch rule)
        _dw(_pad(dQp, B, _r64(N)), N, ha, H, gW)
        gW -= s * sh[None, :]
        gc = dQp[:, :N].sum(0) - s * B
        Wp = _pad(W, N4, H)
        dha = torch.empty(B, H, device=dev)
        _dx(dQp, N4, Wp, H, dha, None, 1.0, None)    # dQ W: contraction over the catalogue
        dh = torch.empty(B, 2 * H, device=dev)
        dh[:, :H] = (dha - s * sw[None, :]) * (ha > 0)
        wv = lv2.weight.detach()
        dh[:, H:] = dV[:, None] * wv * (hv > 0)
        gwv = (dV[:, None] * hv).sum(0, keepdim=True)
        gbv = dV.sum().reshape(1)
        gw0, gb0 = torch.empty(H, K, device=dev), torch.empty(H, device=dev)
        gw12, gb12 = torch.empty(2 * H, H, device=dev), torch.empty(2 * H, device=dev)
        dx = dqn_trunk_backward(dh, f, xp, K, Kp, w0p, w12, gw0, gb0, gw12, gb12, ctx.needs_input_grad[0])
        grads = {id(l0.weight): gw0, id(l0.bias): gb0, id(la0.weight): gw12[:H], id(la0.bias): gb12[:H], id(lv0.weight): gw12[H:],
                 id(lv0.bias): gb12[H:], id(la2.weight): gW, id(la2.bias): gc, id(lv2.weight): gwv, id(lv2.bias): gbv}
        pg = tuple(grads.get(id(p)) for p in ctx.params)
        return (dx[:, :K] if dx is not None else None, None) + pg


def duel_dqn_forward(x, net):
    """DuelDQN(x) on the kernels, differentiable in x and in every parameter of `net`."""
    return DuelDQNFunction.apply(x, net, *net.parameters())


# ------------------------------------------------------------------------------------------------------------------------
# LSTM state encoder over whole user histories (csrc/lstm.hip over csrc/seq_chain.h): what SeqEnv turns a user batch into states with.
LSTM_VARIANTS = {"fused": 0, "chunked": 1}
_lstm_variant = "chunked"


def set_lstm_variant(name: str):
    """How `lstm_encode` schedules the input projection: "fused" into every step, or "chunked" (projected per chunk of steps by a
    grid-wide launch, the chain launch starts from it).  Both compute the same bits; DESIGN.md 14 has the timings.  `gru_encode` and
    `gru_encode_train` follow the same setting."""
    global _lstm_variant
    if name not in LSTM_VARIANTS:
        raise ValueError(f"unknown LSTM variant {name!r}; choose from {sorted(LSTM_VARIANTS)}")
    _lstm_variant = name


_CELLS = {"lstm": (torch.nn.LSTM, (("num_layers", 1), ("bidirectional", False), ("proj_size", 0), ("dropout", 0), ("bias", True)),
                   "without projection or dropout", "a torch.nn.GRU goes to gru_encode / gru_encode_train"),
          "gru": (torch.nn.GRU, (("num_layers", 1), ("bidirectional", False), ("dropout", 0), ("bias", True)),
                  "without dropout", "a torch.nn.LSTM goes to lstm_encode / lstm_encode_train")}


def _check_cell(module, cell):
    """The one recurrent layer an encode kernel implements; anything else is refused by name, never approximated.  The type comes
    first: the kernels read 4H (LSTM) or 3H (GRU) weight rows, and a module of the other kind has the same attribute names."""
    cls, attrs, tail, other = _CELLS[cell]
    if not isinstance(module, cls):
        t = type(module)
        raise L.RecnnHipError(f"{cell}_encode: the state encoder is a {t.__module__}.{t.__qualname__}, not a torch.nn.{cls.__name__} "
                              f"({other})")
    for attr, want in attrs:
        got = getattr(module, attr, want)
        if got != want:
            raise L.RecnnHipError(f"{cell}_encode: {attr}={got!r} is not supported (needs {attr}={want!r}): the HIP encoder is a "
                                  f"single-layer, unidirectional torch.nn.{cls.__name__} with biases, {tail}")
    w = module.weight_ih_l0
    if not w.is_cuda:
        raise L.RecnnHipError(f"{cell}_encode: the module lives on {w.device} (weight_ih_l0.device); it needs a GPU module "
                              "(recnn_amd has no CPU fallback)")
    for name in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
        p = getattr(module, name)
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise L.RecnnHipError(f"{cell}_encode: {name} must be a contiguous float32 tensor (got {p.dtype})")


def _encode_call_args(name, cell, module, store, table, slots, T, states, t0):
    """The checks of `lstm_encode` / `gru_encode`, for the encode entry points: (dev, E, H, U, T, t0, slots, states), `states` the
    carried tensors as [U, H] each, or None."""
    _check_cell(module, cell)
    dev = module.weight_ih_l0.device
    if not (isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.float32 and table.is_contiguous()):
        raise L.RecnnHipError(f"{name}: table must be a contiguous float32 GPU tensor")
    E, H = table.shape[1], module.hidden_size
    if module.input_size != E + 1:
        raise L.RecnnHipError(f"{name}: input_size={module.input_size} but the table has {E} columns (needs E + 1: the rating)")
    slots = store.checked_slots(slots, name, dev)
    U, T, t0 = len(slots), int(T), int(t0)
    if table.device != dev:
        raise ValueError(f"{name}: the table lives on {table.device}, the module on {dev}")
    if T < 1 or t0 < 0:
        raise ValueError(f"{name}: need T >= 1 and t0 >= 0 (got T={T}, t0={t0})")
    if U and int(store.lengths[slots].min()) < t0 + T:
        raise ValueError(f"{name}: steps {t0} .. {t0 + T - 1} asked of a history of {int(store.lengths[slots].min())} elements")
    if states is not None:
        states = tuple(t.to(dev, torch.float32).reshape(U, H).contiguous() for t in states)
    return dev, E, H, U, T, t0, slots, states


def _refuse_table_grad(name, table, train_table):
    """What every `*_encode_train` opens with: the refusal of a table gradient nobody asked for."""
    if isinstance(table, torch.Tensor) and table.requires_grad and not train_table:
        raise L.RecnnHipError(f"{name}: table.requires_grad is set, but gradients with respect to the embedding table are "
                              "computed only on request; pass train_table=True to train it, or table.detach()")


def _wants_graph(table, tensors):
    """Whether a `*_encode_train` call records anything: grad mode, and the table (only with train_table) or one of `tensors`."""
    return torch.is_grad_enabled() and (table.requires_grad or any(t.requires_grad for t in tensors))


def _f32_on(dev):
    """`new(*shape)`: an uninitialised float32 tensor on `dev`."""
    return lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)


def _train_buffers(query, dev, *dims):
    """(`saved`, bytes of the backward's workspace) of a training forward, sized by the entry point `query`."""
    nsaved, nbwd = C.c_int64(), C.c_int64()
    L.call(query, *dims, C.byref(nsaved), C.byref(nbwd))
    return torch.empty(max(nsaved.value, 16), dtype=torch.uint8, device=dev), nbwd.value


def _call_backward(kind, head, w_table, mid, d_table, ws, table_dims, dev):
    """recnn_<kind>_backward, or -- `d_table` wanted -- recnn_<kind>_backward_table, which also takes the weight next to the table
    (`w_table`) and the table workspace of recnn_<kind>_table_grad_workspace_bytes(*table_dims)."""
    if d_table is None:
        L.call(f"recnn_{kind}_backward", *head, *mid, L.ptr(ws), L.current_stream())
    else:
        tws = L.workspace(f"recnn_{kind}_table_grad_workspace_bytes", *table_dims, device=dev)
        L.call(f"recnn_{kind}_backward_table", *head, L.ptr(w_table), *mid, L.ptr(d_table), L.ptr(ws), L.ptr(tws), L.current_stream())


def _train_call_args(name, cell, module, store, table, slots, T, states, t0, train_table):
    """The prologue of `lstm_encode_train` / `gru_encode_train`: `_refuse_table_grad`, then `_encode_call_args`' tuple with
    (params, live) appended -- the four weights, and whether anything wants a graph."""
    _refuse_table_grad(name, table, train_table)
    *head, states = _encode_call_args(name, cell, module, store, table, slots, T, states, t0)
    params = (module.weight_ih_l0, module.weight_hh_l0, module.bias_ih_l0, module.bias_hh_l0)
    return (*head, states, params, _wants_graph(table, (*params, *(states or ()))))


def _store_args(store, slots_d, U, t0, T, table, E, H):
    """The leading arguments of every encode and backward entry point: the replay store, the step range, the table, the sizes."""
    return (L.ptr(store.items), L.ptr(store.ratings), L.ptr(store.user_off), L.ptr(slots_d), U, t0, T, L.ptr(table), table.shape[0],
            E, H)


def _encode_buffers(cell, nstate, dev, U, T, E, H, train=False):
    """What one encode call allocates: (variant, projection workspace, `saved` record, bytes of the backward's workspace, h [U, T, H],
    a tuple of the `nstate` final states [U, H] each); `saved` is None and the bytes 0 unless `train`."""
    variant = LSTM_VARIANTS[_lstm_variant]
    saved, nbwd = _train_buffers(f"recnn_{cell}_train_workspace_bytes", dev, U, T, H, E, variant) if train else (None, 0)
    ws = L.workspace(f"recnn_{cell}_workspace_bytes", U, T, H, variant, device=dev)
    new = _f32_on(dev)
    return variant, ws, saved, nbwd, new(U, T, H), tuple(new(U, H) for _ in range(nstate))


@torch.no_grad()
def lstm_encode(lstm, store, table, slots, T, h0c0=None, *, t0=0):
    """States of the users `slots` (store slots) after each of the steps t0 .. t0 + T - 1 of their histories, one HIP launch
    chain: the input of step t is [table[item_t] | rating_t] (width E + 1 == lstm.input_size), read through the replay `store`.
    Returns (h float32[U, T, H], (h_T, c_T) float32[U, H] each).  `h0c0` = (h0, c0), each [U, H] or [1, U, H]; default zeros.
    Carrying (h_T, c_T) into a call with t0 moved on gives bit for bit what one longer call gives.

    Runs under no_grad (`lstm_encode_train` is the same call with a graph); the weights are read live from the module on every call (weight_ih_l0, weight_hh_l0, bias_ih_l0,
    bias_hh_l0, gate order i, f, g, o), state and accumulation are fp32.  Refused with RecnnHipError naming the attribute:
    num_layers != 1, bidirectional, proj_size != 0, dropout != 0, bias=False, a CPU module -- and, naming the type, a module that is
    not a torch.nn.LSTM (a torch.nn.GRU has the same attribute names and 3H weight rows: it goes to `gru_encode`).

    `batch_first` is ignored: the users are always the batch and time always runs along a user's own history.  (The
    reference's commented-out SeqEnv feeds [1, U, E + 1] to its encoder, which a batch_first=True LSTM reads as ONE sequence
    running across the users -- the bug that makes its notebook "not work yet".  It is not reproduced.)"""
    dev, E, H, U, T, t0, slots, hc = _encode_call_args("lstm_encode", "lstm", lstm, store, table, slots, T, h0c0, t0)
    h0, c0 = hc if hc is not None else (None, None)
    variant, ws, _, _, h, (hT, cT) = _encode_buffers("lstm", 2, dev, U, T, E, H)
    slots_d = torch.from_numpy(slots).to(dev)
    L.call("recnn_lstm_encode", *_store_args(store, slots_d, U, t0, T, table, E, H), L.ptr(lstm.weight_ih_l0), L.ptr(lstm.weight_hh_l0),
           L.ptr(lstm.bias_ih_l0), L.ptr(lstm.bias_hh_l0), L.ptr(h0), L.ptr(c0), L.ptr(h), L.ptr(hT), L.ptr(cT), variant, L.ptr(ws),
           L.current_stream())
    return h, (hT, cT)


def seq_collect(h, steps, store, table, slots, views):
    """Fill `views` = (state, action, reward, next_state) rows [len(steps) * U, ...] for the kept `steps` of one user batch from
    the encode output h [U, T, H]: one launch (`recnn_seq_collect`).

    The kernel writes rows of H, E, 1 and H floats and cannot see the destinations' sizes, so they are checked here, before
    anything else: each view float32, contiguous, on h's device and shaped [rows, H], [rows, E], [rows] or [rows, 1], [rows, H]
    with rows == len(steps) * U.  ValueError naming the sizes otherwise."""
    if not (isinstance(h, torch.Tensor) and h.dim() == 3 and h.dtype == torch.float32 and h.is_contiguous()):
        raise ValueError("seq_collect: h must be a contiguous float32 [U, T, H] tensor")
    U, T, H = h.shape
    E = table.shape[1]
    steps = np.asarray(steps, dtype=np.int32).reshape(-1)
    if len(steps) and (steps.min() < 1 or steps.max() >= T):
        raise ValueError(f"seq_collect: steps must lie in 1 .. {T - 1}")
    if len(slots) != U:
        raise ValueError(f"seq_collect: {len(slots)} slots for the {U} users of h")
    rows = len(steps) * U
    if len(views) != 4:
        raise ValueError(f"seq_collect: views must be (state, action, reward, next_state), got {len(views)} tensors")
    want = {"state": [(rows, H)], "action": [(rows, E)], "reward": [(rows,), (rows, 1)], "next_state": [(rows, H)]}
    for (name, shapes), v in zip(want.items(), views):
        if not isinstance(v, torch.Tensor) or tuple(v.shape) not in shapes or v.dtype != torch.float32 or not v.is_contiguous() \
                or v.device != h.device:
            got = (tuple(v.shape), v.dtype, str(v.device), "contiguous" if v.is_contiguous() else "strided") \
                if isinstance(v, torch.Tensor) else type(v)
            raise ValueError(f"seq_collect: {name} must be a contiguous float32 tensor of shape {' or '.join(map(str, shapes))} on "
                             f"{h.device} ({len(steps)} steps x {U} users, H = {H}, E = {E}); got {got}")
    if not h.is_cuda:
        raise L.RecnnHipError(f"seq_collect: needs GPU tensors (recnn_amd has no CPU fallback); got {h.device}")
    if not (table.is_cuda and table.dtype == torch.float32 and table.is_contiguous() and table.device == h.device):
        raise L.RecnnHipError("seq_collect: table must be a contiguous float32 tensor on h's device")
    slots = store.checked_slots(slots, "seq_collect", h.device)
    if len(steps) and int(store.lengths[slots].min()) <= int(steps.max()):
        raise ValueError(f"seq_collect: step {int(steps.max())} asked of a history of {int(store.lengths[slots].min())} elements")
    state, action, reward, next_state = views
    # (both index tensors stay referenced until the launch is queued: a temporary freed inside the argument list hands its block
    # to the next one)
    steps_d = torch.from_numpy(steps).to(h.device)
    slots_d = torch.from_numpy(slots).to(h.device)
    L.call("recnn_seq_collect", L.ptr(h), U, T, H, L.ptr(steps_d), len(steps), L.ptr(store.items),
           L.ptr(store.ratings), L.ptr(store.user_off), L.ptr(slots_d), L.ptr(table), table.shape[0],
           E, L.ptr(state), L.ptr(action), L.ptr(reward), L.ptr(next_state), L.current_stream())


# ------------------------------------------------------------------------------------------------------------------------
# Training the encoder (csrc/seq_bwd.h): backward through time for the encode chain, a differentiable collect.
class LSTMEncodeFunction(torch.autograd.Function):
    """(h, h_T, c_T) of the encode chain with the gates and cell states recorded, and backward through time for them
    (`recnn_lstm_encode_train` / `recnn_lstm_backward`).  Differentiable in the four weights, in h0 / c0 and in the embedding
    `table` (`recnn_lstm_backward_table`: the dense [n_items, E] gradient, allocated only when `needs_input_grad` asks for it); once."""

    @staticmethod
    def forward(ctx, w_ih, w_hh, b_ih, b_hh, h0, c0, store, table, slots_d, T, t0):
        U, E, H = slots_d.shape[0], table.shape[1], w_hh.shape[1]
        variant, ws, saved, nbwd, h, (hT, cT) = _encode_buffers("lstm", 2, w_ih.device, U, T, E, H, train=True)
        L.call("recnn_lstm_encode_train", *_store_args(store, slots_d, U, t0, T, table, E, H), L.ptr(w_ih), L.ptr(w_hh), L.ptr(b_ih),
               L.ptr(b_hh), L.ptr(h0), L.ptr(c0), L.ptr(h), L.ptr(hT), L.ptr(cT), variant, L.ptr(ws), L.ptr(saved), L.current_stream())
        ctx.store, ctx.dims, ctx.bwd_bytes = store, (U, T, t0, E, H), nbwd
        ctx.set_materialize_grads(False)                  # an unused output's gradient arrives as None and is passed as NULL
        ctx.has_h0 = h0 is not None
        ctx.save_for_backward(w_hh, table, slots_d, saved, h, w_ih, *((h0, c0) if h0 is not None else ()))
        return h, hT, cT

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_h, g_hT, g_cT):
        w_hh, table, slots_d, saved, h, w_ih = ctx.saved_tensors[:6]
        h0, c0 = ctx.saved_tensors[6:] if ctx.has_h0 else (None, None)
        U, T, t0, E, H = ctx.dims
        store, dev = ctx.store, h.device
        need = ctx.needs_input_grad
        if g_h is None and g_hT is None and g_cT is None:
            return (None,) * 11
        g_h, g_hT, g_cT = (None if g is None else g.to(torch.float32).contiguous() for g in (g_h, g_hT, g_cT))
        new = _f32_on(dev)
        d_w_ih = new(4 * H, E + 1) if need[0] else None
        d_w_hh = new(4 * H, H) if need[1] else None
        d_b = new(4 * H) if need[2] or need[3] else None
        d_h0 = new(U, H) if need[4] else None
        d_c0 = new(U, H) if need[5] else None
        d_table = new(table.shape[0], E) if need[7] else None
        ws = torch.empty(max(ctx.bwd_bytes, 16), dtype=torch.uint8, device=dev)
        head = _store_args(store, slots_d, U, t0, T, table, E, H)
        mid = (L.ptr(w_hh), L.ptr(saved), L.ptr(h), L.ptr(h0), L.ptr(c0), L.ptr(g_h), L.ptr(g_hT), L.ptr(g_cT), L.ptr(d_w_ih),
               L.ptr(d_w_hh), L.ptr(d_b), L.ptr(d_h0), L.ptr(d_c0))
        _call_backward("lstm", head, w_ih, mid, d_table, ws, (U, T, H, E, table.shape[0]), dev)
        return (d_w_ih, d_w_hh, d_b if need[2] else None, (d_b.clone() if need[2] else d_b) if need[3] else None, d_h0, d_c0,
                None, d_table, None, None, None)


def lstm_encode_train(lstm, store, table, slots, T, h0c0=None, *, t0=0, train_table=False):
    """`lstm_encode` with a graph: the same arguments, checks and return value (h, (h_T, c_T)) -- bit for bit the same numbers
    under either variant -- differentiable with respect to weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, and to h0 / c0 when
    they require grad, so truncated BPTT over calls with `t0` moved on works: carry (h_T, c_T) into the next call.

    The forward also records the gate activations and cell states (5 U T H floats, U rounded up to 16); the backward is one HIP
    launch chain backward through time plus the weight-gradient launches per chunk of steps (csrc/seq_bwd.h), in fixed
    summation orders: equal calls give equal gradients bit for bit.  It is once differentiable.

    The embedding table: by default a `table` that requires grad is refused with RecnnHipError (pass `table.detach()` to keep the
    embeddings frozen).  With `train_table=True` the call is differentiable in `table` as well when it requires grad -- even with
    every encoder parameter frozen --: the backward adds one contraction launch per chunk of steps and one deterministic
    scatter-sum over the item ids, and `table.grad` receives the dense [n_items, E] gradient, exact zeros in the
    rows of items the batch's steps do not hold.  The weight gradients, dh0 and dc0 keep their bits.

    Under `torch.no_grad()`, or when nothing requires grad, this IS `lstm_encode`: nothing is recorded."""
    dev, E, H, U, T, t0, slots, hc, params, live = _train_call_args("lstm_encode_train", "lstm", lstm, store, table, slots, T, h0c0, t0,
                                                                    train_table)
    if not live:
        return lstm_encode(lstm, store, table.detach(), slots, T, hc, t0=t0)
    h0, c0 = hc if hc is not None else (None, None)
    h, hT, cT = LSTMEncodeFunction.apply(*params, h0, c0, store, table, torch.from_numpy(slots).to(dev), T, t0)
    return h, (hT, cT)


# ------------------------------------------------------------------------------------------------------------------------
# A GRU as the state encoder (csrc/gru.hip): the same path with one carried tensor and three gates.
@torch.no_grad()
def gru_encode(gru, store, table, slots, T, h0=None, *, t0=0):
    """`lstm_encode` for a single-layer unidirectional `torch.nn.GRU(E + 1, H)` on the GPU: the states of the users `slots` after
    each of the steps t0 .. t0 + T - 1 of their histories, one HIP launch chain, the input of step t being
    [table[item_t] | rating_t].  Returns (h float32[U, T, H], h_T float32[U, H]).  `h0`: [U, H] or [1, U, H]; default zeros.
    Carrying h_T into a call with t0 moved on gives bit for bit what one longer call gives; both schedules of `set_lstm_variant`
    apply and give the same bits.

    Runs under no_grad (`gru_encode_train` is the same call with a graph); the weights are read live from the module (gate order
    r, z, n; b_hn inside the reset product, as torch.nn.GRU has it), state and accumulation are fp32.  Refused with RecnnHipError
    naming what is wrong: a module that is not a torch.nn.GRU (an LSTM goes to `lstm_encode`), num_layers != 1, bidirectional,
    dropout != 0, bias=False, a CPU module, a non-contiguous or non-float32 weight, input_size != E + 1.  `batch_first` is ignored."""
    dev, E, H, U, T, t0, slots, h0 = _encode_call_args("gru_encode", "gru", gru, store, table, slots, T, None if h0 is None else (h0,), t0)
    h0 = None if h0 is None else h0[0]
    variant, ws, _, _, h, (hT,) = _encode_buffers("gru", 1, dev, U, T, E, H)
    slots_d = torch.from_numpy(slots).to(dev)
    L.call("recnn_gru_encode", *_store_args(store, slots_d, U, t0, T, table, E, H), L.ptr(gru.weight_ih_l0), L.ptr(gru.weight_hh_l0),
           L.ptr(gru.bias_ih_l0), L.ptr(gru.bias_hh_l0), L.ptr(h0), L.ptr(h), L.ptr(hT), variant, L.ptr(ws), L.current_stream())
    return h, hT


class GRUEncodeFunction(torch.autograd.Function):
    """(h, h_T) of the GRU encode chain with r, z, n and hn recorded, and backward through time for them (`recnn_gru_encode_train` /
    `recnn_gru_backward`).  Differentiable in the four weights, in h0 and in the embedding `table` (`recnn_gru_backward_table`: the
    dense [n_items, E] gradient, allocated only when `needs_input_grad` asks for it); once."""

    @staticmethod
    def forward(ctx, w_ih, w_hh, b_ih, b_hh, h0, store, table, slots_d, T, t0):
        U, E, H = slots_d.shape[0], table.shape[1], w_hh.shape[1]
        variant, ws, saved, nbwd, h, (hT,) = _encode_buffers("gru", 1, w_ih.device, U, T, E, H, train=True)
        L.call("recnn_gru_encode_train", *_store_args(store, slots_d, U, t0, T, table, E, H), L.ptr(w_ih), L.ptr(w_hh), L.ptr(b_ih),
               L.ptr(b_hh), L.ptr(h0), L.ptr(h), L.ptr(hT), variant, L.ptr(ws), L.ptr(saved), L.current_stream())
        ctx.store, ctx.dims, ctx.bwd_bytes = store, (U, T, t0, E, H), nbwd
        ctx.set_materialize_grads(False)                  # an unused output's gradient arrives as None and is passed as NULL
        ctx.has_h0 = h0 is not None
        ctx.save_for_backward(w_hh, table, slots_d, saved, h, w_ih, *((h0,) if h0 is not None else ()))
        return h, hT

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_h, g_hT):
        w_hh, table, slots_d, saved, h, w_ih = ctx.saved_tensors[:6]
        h0 = ctx.saved_tensors[6] if ctx.has_h0 else None
        U, T, t0, E, H = ctx.dims
        store, dev = ctx.store, h.device
        need = ctx.needs_input_grad
        if g_h is None and g_hT is None:
            return (None,) * 10
        g_h, g_hT = (None if g is None else g.to(torch.float32).contiguous() for g in (g_h, g_hT))
        new = _f32_on(dev)
        d_w_ih = new(3 * H, E + 1) if need[0] else None
        d_w_hh = new(3 * H, H) if need[1] else None
        d_b_ih = new(3 * H) if need[2] else None
        d_b_hh = new(3 * H) if need[3] else None
        d_h0 = new(U, H) if need[4] else None
        d_table = new(table.shape[0], E) if need[6] else None
        ws = torch.empty(max(ctx.bwd_bytes, 16), dtype=torch.uint8, device=dev)
        head = _store_args(store, slots_d, U, t0, T, table, E, H)
        mid = (L.ptr(w_hh), L.ptr(saved), L.ptr(h), L.ptr(h0), L.ptr(g_h), L.ptr(g_hT), L.ptr(d_w_ih), L.ptr(d_w_hh), L.ptr(d_b_ih),
               L.ptr(d_b_hh), L.ptr(d_h0))
        _call_backward("gru", head, w_ih, mid, d_table, ws, (U, T, H, E, table.shape[0]), dev)
        return d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_h0, None, d_table, None, None, None


def gru_encode_train(gru, store, table, slots, T, h0=None, *, t0=0, train_table=False):
    """`gru_encode` with a graph: the same arguments, checks and return value (h, h_T) -- bit for bit the same numbers under either
    variant -- differentiable with respect to weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0 (the two bias gradients differ in
    their last H entries: b_hn sits inside the reset product), and to h0 when it requires grad, so truncated BPTT over calls with
    `t0` moved on works: carry h_T into the next call.

    The forward also records r, z, n and W_hn h + b_hn (4 U T H floats, U rounded up to 16); the backward is one HIP launch chain
    backward through time plus the weight-gradient launches per chunk of steps (csrc/gru.hip), in fixed summation orders: equal
    calls give equal gradients bit for bit.  It is once differentiable.

    The embedding table is handled as in `lstm_encode_train`: a `table` that requires grad is refused with RecnnHipError unless
    `train_table=True`, and then `table.grad` receives the dense [n_items, E] gradient, exact zeros in the rows of items the batch's
    steps do not hold -- also with every encoder parameter frozen.  The weight gradients and dh0 keep their bits.

    Under `torch.no_grad()`, or when nothing requires grad, this IS `gru_encode`: nothing is recorded."""
    dev, E, H, U, T, t0, slots, h0, params, live = _train_call_args("gru_encode_train", "gru", gru, store, table, slots, T,
                                                                    None if h0 is None else (h0,), t0, train_table)
    h0 = None if h0 is None else h0[0]
    if not live:
        return gru_encode(gru, store, table.detach(), slots, T, h0, t0=t0)
    return GRUEncodeFunction.apply(*params, h0, store, table, torch.from_numpy(slots).to(dev), T, t0)


# ------------------------------------------------------------------------------------------------------------------------
# Causal self-attention as the state encoder (csrc/attn.hip): the one encoder whose work is parallel over the steps.
_ATTN_PARAMS = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")


def _attn_call_args(name, enc, store, table, slots, T, t0):
    """The checks of `attn_encode` / `attn_encode_train`, on the host and by argument name, before any launch:
    (dev, E, H, U, T, t0, slots, params)."""
    params, shapes_of = _attn_spec(name, enc)
    return _attn_checked(name, enc, _ATTN_PARAMS, params, shapes_of, "in_proj_weight", store, table, slots, T, t0)


def _attn_spec(name, enc):
    """(params, shapes_of) of an `AttentionEncoder`; another module is refused by name."""
    if not isinstance(enc, AttentionEncoder):
        t = type(enc)
        raise L.RecnnHipError(f"{name}: the state encoder is a {t.__module__}.{t.__qualname__}, not a recnn_amd.nn.AttentionEncoder "
                              "(a torch.nn.LSTM goes to lstm_encode, a torch.nn.GRU to gru_encode)")
    params = (enc.in_proj_weight, enc.in_proj_bias, enc.out_proj.weight, enc.out_proj.bias)
    return params, lambda E, H: ((3 * H, E + 1), (3 * H,), (H, H), (H,))


def _attn_checked(name, enc, pnames, params, shapes_of, first, store, table, slots, T, t0):
    """The checks that `AttentionEncoder` and `TransformerStateEncoder` share: (dev, E, H, U, T, t0, slots, params)."""
    dev, E, H = _attn_module_checked(name, enc, pnames, params, shapes_of, table)
    slots = store.checked_slots(slots, name, dev)
    U, T, t0 = len(slots), int(T), int(t0)
    if T < 1 or t0 < 0:
        raise ValueError(f"{name}: need T >= 1 and t0 >= 0 (got T={T}, t0={t0})")
    if U * T >= 1 << 31 or U > 65535:
        raise ValueError(f"{name}: U * T = {U * T} must stay below 2^31 and U = {U} below 65536")
    if U and int(store.lengths[slots].min()) < t0 + T:
        raise ValueError(f"{name}: steps {t0} .. {t0 + T - 1} asked of a history of {int(store.lengths[slots].min())} elements")
    _module_on_gpu(name, params, first, dev)
    if table.device != dev:
        raise ValueError(f"{name}: the table lives on {table.device}, the module on {dev}")
    return dev, E, H, U, T, t0, slots, params


def _module_on_gpu(name, params, first, dev):
    if not params[0].is_cuda:
        raise L.RecnnHipError(f"{name}: the module lives on {dev} ({first}.device); it needs a GPU module "
                              "(recnn_amd has no CPU fallback)")


def _attn_module_checked(name, enc, pnames, params, shapes_of, table):
    """What `_attn_checked` asks of the module and the table alone (the append calls ask the same): (dev, E, H)."""
    dev = params[0].device
    for pname, p in zip(pnames, params):
        if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
            raise L.RecnnHipError(f"{name}: {pname} must be a contiguous float32 tensor on {dev} (got {p.dtype} on {p.device}, "
                                  f"{'contiguous' if p.is_contiguous() else 'strided'})")
    if not (isinstance(table, torch.Tensor) and table.dim() == 2 and table.dtype == torch.float32 and table.is_contiguous()):
        raise L.RecnnHipError(f"{name}: table must be a contiguous float32 [n_items, E] tensor")
    E, H, heads = table.shape[1], enc.hidden_size, enc.num_heads
    if enc.input_size != E + 1:
        raise L.RecnnHipError(f"{name}: input_size={enc.input_size} but the table has {E} columns (needs E + 1: the rating)")
    if heads < 1 or H % heads:
        raise L.RecnnHipError(f"{name}: hidden_size={H} is not a multiple of num_heads={heads}")
    if H // heads not in (16, 32, 64):
        raise L.RecnnHipError(f"{name}: head_dim={H // heads} is not supported (hidden_size / num_heads must be 16, 32 or 64)")
    if H % 16 or H > 256:
        raise L.RecnnHipError(f"{name}: hidden_size={H} must be a multiple of 16 up to 256")
    if E % 8 or E > 128 or E < 8:
        raise L.RecnnHipError(f"{name}: the table's width E={E} must be a multiple of 8 up to 128")
    if enc.window is not None and int(enc.window) < 1:
        raise L.RecnnHipError(f"{name}: window={enc.window} must be at least 1 (or None)")
    if any(tuple(p.shape) != shape for p, shape in zip(params, shapes_of(E, H))):
        raise L.RecnnHipError(f"{name}: the parameters do not have the shapes of hidden_size={H}, input_size={E + 1}")
    return dev, E, H


def _attn_head(enc, store, slots_d, U, t0, T, table, E, H):
    """The leading arguments of every recnn_attn_* launch: `_store_args`, then heads, window (0: none) and alibi."""
    return (*_store_args(store, slots_d, U, t0, T, table, E, H), enc.num_heads, enc.window or 0, int(enc.alibi))


@torch.no_grad()
def attn_encode(enc, store, table, slots, T, *, t0=0):
    """h float32[U, T, H] of a `recnn_amd.nn.AttentionEncoder` for the users `slots` (store slots) over the steps t0 .. t0 + T - 1 of
    their histories: step t attends to steps max(0, t - window + 1) .. t of THIS call (positions before t0 are not seen; this call
    carries no state -- `attn_append` serves a session step by step from a `KVCache`, with this call's bits), its input being
    [table[item_t] | rating_t] read through the replay `store`.  Three launches: the in-projection
    (rows gathered through the store), the flash-style attention, the out-projection; fp32 on the exact-f32 MFMA.

    Equal calls give equal bits; a user's rows do not depend on the other users or on its place in the batch; the first `a` steps
    of a longer call are bit for bit the call with T = a; h_t does not depend on the bits of any position it does not attend to.
    Runs under no_grad (`attn_encode_train` is the same call with a graph); the parameters are read live from the module.  Refused
    with RecnnHipError naming what is wrong: another module type, a CPU module, a non-contiguous or non-float32 parameter,
    input_size != E + 1, hidden_size % num_heads, head_dim outside {16, 32, 64}, hidden_size not a multiple of 16 up to 256, E not a
    multiple of 8 up to 128, window < 1; with ValueError: a history shorter than t0 + T, U * T >= 2^31."""
    dev, E, H, U, T, t0, slots, params = _attn_call_args("attn_encode", enc, store, table, slots, T, t0)
    ws = L.workspace("recnn_attn_workspace_bytes", U, T, H, enc.num_heads, device=dev)
    h = _f32_on(dev)(U, T, H)
    slots_d = torch.from_numpy(slots).to(dev)
    L.call("recnn_attn_encode", *_attn_head(enc, store, slots_d, U, t0, T, table, E, H), *(L.ptr(p) for p in params), L.ptr(h),
           L.ptr(ws), L.current_stream())
    return h


class AttnEncodeFunction(torch.autograd.Function):
    """h of the attention encoder with qkv, o and the log-sum-exp kept, and its backward (`recnn_attn_encode_train` /
    `recnn_attn_backward`).  Differentiable in the four parameters and in the embedding `table` (`recnn_attn_backward_table`: the
    dense [n_items, E] gradient, allocated only when `needs_input_grad` asks for it); once."""

    @staticmethod
    def forward(ctx, w_in, b_in, w_o, b_o, enc, store, table, slots_d, T, t0):
        U, E, H = slots_d.shape[0], table.shape[1], w_o.shape[0]
        dev = w_in.device
        saved, ctx.bwd_bytes = _train_buffers("recnn_attn_train_workspace_bytes", dev, U, T, H, E, enc.num_heads)
        h = _f32_on(dev)(U, T, H)
        head = _attn_head(enc, store, slots_d, U, t0, T, table, E, H)
        L.call("recnn_attn_encode_train", *head, L.ptr(w_in), L.ptr(b_in), L.ptr(w_o), L.ptr(b_o), L.ptr(h), L.ptr(saved),
               L.current_stream())
        ctx.enc, ctx.store, ctx.dims = enc, store, (U, T, t0, E, H)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(w_in, w_o, table, slots_d, saved)
        return h

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_h):
        w_in, w_o, table, slots_d, saved = ctx.saved_tensors
        U, T, t0, E, H = ctx.dims
        need = ctx.needs_input_grad
        if g_h is None:
            return (None,) * 10
        dev = saved.device
        g_h = g_h.to(torch.float32).contiguous()
        new = _f32_on(dev)
        d_w_in = new(3 * H, E + 1) if need[0] else None
        d_b_in = new(3 * H) if need[1] else None
        d_w_o = new(H, H) if need[2] else None
        d_b_o = new(H) if need[3] else None
        d_table = new(table.shape[0], E) if need[6] else None
        ws = torch.empty(max(ctx.bwd_bytes, 16), dtype=torch.uint8, device=dev)
        head = _attn_head(ctx.enc, ctx.store, slots_d, U, t0, T, table, E, H)
        mid = (L.ptr(w_o), L.ptr(saved), L.ptr(g_h), L.ptr(d_w_in), L.ptr(d_b_in), L.ptr(d_w_o), L.ptr(d_b_o))
        _call_backward("attn", head, w_in, mid, d_table, ws, (U, T, H, E, table.shape[0]), dev)
        return d_w_in, d_b_in, d_w_o, d_b_o, None, None, d_table, None, None, None


def attn_encode_train(enc, store, table, slots, T, *, t0=0, train_table=False):
    """`attn_encode` with a graph: the same arguments, checks and h -- bit for bit -- differentiable with respect to
    in_proj_weight, in_proj_bias, out_proj.weight and out_proj.bias.  The forward keeps qkv [U, T, 3H], o [U, T, H] and the
    log-sum-exp per (user, head, step); the backward recomputes the probabilities from them in three launches (a sweep that sums
    delta = sum_j p dP, one that owns keys and gives dK and dV, one that owns queries and gives dQ), then the weight-gradient tile
    of the recurrent encoders over segments of the samples: fixed summation orders and no float atomics, so equal calls give equal
    gradients bit for bit.  Once differentiable.

    The embedding table is handled as in `lstm_encode_train`: a `table` that requires grad is refused with RecnnHipError unless
    `train_table=True`, and then `table.grad` receives the dense [n_items, E] gradient, exact zeros in the rows of items the batch's
    steps do not hold -- also with every encoder parameter frozen.  The parameter gradients keep their bits.

    Under `torch.no_grad()`, or when nothing requires grad, this IS `attn_encode`: nothing is kept."""
    _refuse_table_grad("attn_encode_train", table, train_table)
    dev, E, H, U, T, t0, slots, params = _attn_call_args("attn_encode_train", enc, store, table, slots, T, t0)
    if not _wants_graph(table, params):
        return attn_encode(enc, store, table.detach(), slots, T, t0=t0)
    return AttnEncodeFunction.apply(*params, enc, store, table, torch.from_numpy(slots).to(dev), T, t0)


# ------------------------------------------------------------------------------------------------------------------------
# The transformer state encoder (csrc/block.hip): embedding, pre-LN blocks on a dense [U, T, H] stream, final LayerNorm.
_BLOCK_PARAMS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                 "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
                 "norm2.bias")


def _block_params(blk):
    sa = blk.self_attn
    return (sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight, sa.out_proj.bias, blk.linear1.weight, blk.linear1.bias,
            blk.linear2.weight, blk.linear2.bias, blk.norm1.weight, blk.norm1.bias, blk.norm2.weight, blk.norm2.bias)


def _transformer_call_args(name, enc, store, table, slots, T, t0):
    """The checks of `transformer_encode` / `transformer_encode_train`, on the host and by argument name, before any launch: those of
    `_attn_call_args`, then num_layers, dim_feedforward, activation and eps.  (dev, E, H, U, T, t0, slots, params, cfg) with params
    = embed's two, twelve per block, norm's two, and cfg = (heads, F, act, window or 0, alibi, eps)."""
    pnames, params, shapes_of, cfg = _transformer_spec(name, enc)
    dev, E, H, U, T, t0, slots, params = _attn_checked(name, enc, pnames, params, shapes_of, "embed.weight", store, table, slots, T, t0)
    return dev, E, H, U, T, t0, slots, params, cfg


def _transformer_spec(name, enc):
    """(pnames, params, shapes_of, cfg) of a `TransformerStateEncoder`, its own settings checked; another module is refused by name."""
    if not isinstance(enc, TransformerStateEncoder):
        t = type(enc)
        raise L.RecnnHipError(f"{name}: the state encoder is a {t.__module__}.{t.__qualname__}, not a "
                              "recnn_amd.nn.TransformerStateEncoder (an AttentionEncoder goes to attn_encode, a torch.nn.LSTM to "
                              "lstm_encode, a torch.nn.GRU to gru_encode)")
    if int(enc.num_layers) < 1 or len(enc.layers) != int(enc.num_layers):
        raise L.RecnnHipError(f"{name}: num_layers={enc.num_layers} must be at least 1 and the length of `layers` ({len(enc.layers)})")
    F = int(enc.dim_feedforward)
    if F % 16 or not 16 <= F <= 1024:
        raise L.RecnnHipError(f"{name}: dim_feedforward={F} must be a multiple of 16 in 16 .. 1024")
    if enc.activation not in TRANSFORMER_ACTIVATIONS:
        raise L.RecnnHipError(f"{name}: activation={enc.activation!r} is not one of {sorted(TRANSFORMER_ACTIVATIONS)}")
    if not float(enc.eps) > 0:
        raise L.RecnnHipError(f"{name}: eps={enc.eps} must be positive")
    pnames = ["embed.weight", "embed.bias"] + [f"layers.{i}.{n}" for i in range(len(enc.layers)) for n in _BLOCK_PARAMS] \
        + ["norm.weight", "norm.bias"]
    params = (enc.embed.weight, enc.embed.bias) + tuple(p for blk in enc.layers for p in _block_params(blk)) \
        + (enc.norm.weight, enc.norm.bias)

    def shapes_of(E, H):
        block = ((3 * H, H), (3 * H,), (H, H), (H,), (F, H), (F,), (H, F), (H,), (H,), (H,), (H,), (H,))
        return ((H, E + 1), (H,)) + block * len(enc.layers) + ((H,), (H,))
    cfg = (enc.num_heads, F, TRANSFORMER_ACTIVATIONS[enc.activation], enc.window or 0, int(enc.alibi), float(enc.eps))
    return pnames, params, shapes_of, cfg


def _block_head(x, cfg):
    """The leading arguments of every recnn_block_* launch on x [U, T, H]."""
    U, T, H = x.shape
    heads, F, act, window, alibi, eps = cfg
    return (L.ptr(x), U, T, H, heads, F, act, window, alibi, C.c_float(eps))


@torch.no_grad()
def transformer_encode(enc, store, table, slots, T, *, t0=0):
    """h float32[U, T, H] of a `recnn_amd.nn.TransformerStateEncoder` for the users `slots` (store slots) over the steps
    t0 .. t0 + T - 1 of their histories (nothing is carried between calls: step t sees steps of THIS call only; `transformer_append`
    serves a session step by step from a `KVCache`, with this call's bits).  One gathered
    embedding launch, four launches per block -- LN1 fused into the in-projection, the flash-style attention, the out-projection
    with the residual in its epilogue, and the fused feed-forward (LN2, linear1, activation, linear2, residual), whose [U T, F]
    activation never reaches memory -- and the final LayerNorm; fp32 on the exact-f32 MFMA.

    Equal calls give equal bits; a user's rows do not depend on the other users or on its place in the batch; the first `a` steps
    of a longer call are bit for bit the call with T = a; h_t does not depend on any position after t, nor, under a window w, on
    positions more than num_layers (w - 1) steps back.  Runs under no_grad (`transformer_encode_train` is the same call with a
    graph).  Refused with RecnnHipError naming what is wrong: everything `attn_encode` refuses, and num_layers < 1, dim_feedforward
    not a multiple of 16 in 16 .. 1024, an unknown activation, eps <= 0."""
    dev, E, H, U, T, t0, slots, params, cfg = _transformer_call_args("transformer_encode", enc, store, table, slots, T, t0)
    slots_d = torch.from_numpy(slots).to(dev)
    x = _f32_on(dev)(U, T, H)
    y = torch.empty_like(x)
    L.call("recnn_seq_embed", *_store_args(store, slots_d, U, t0, T, table, E, H), L.ptr(params[0]), L.ptr(params[1]), L.ptr(x),
           L.current_stream())
    ws = L.workspace("recnn_block_workspace_bytes", U, T, H, cfg[0], device=dev)
    for i in range(len(enc.layers)):
        L.call("recnn_block_forward", *_block_head(x, cfg), *(L.ptr(p) for p in params[2 + 12 * i:14 + 12 * i]), L.ptr(y), L.ptr(ws),
               L.current_stream())
        x, y = y, x
    L.call("recnn_layernorm_rows", L.ptr(x), U * T, H, L.ptr(params[-2]), L.ptr(params[-1]), C.c_float(cfg[5]), L.ptr(y),
           L.current_stream())
    return y


class SeqEmbedFunction(torch.autograd.Function):
    """x^0 = embed([table[item] | rating]) through the store, and its backward (`recnn_seq_embed*`): differentiable in the two
    parameters and, when asked, in the table."""

    @staticmethod
    def forward(ctx, w_e, b_e, store, table, slots_d, T, t0):
        U, E, H = slots_d.shape[0], table.shape[1], w_e.shape[0]
        x = _f32_on(w_e.device)(U, T, H)
        L.call("recnn_seq_embed", *_store_args(store, slots_d, U, t0, T, table, E, H), L.ptr(w_e), L.ptr(b_e), L.ptr(x),
               L.current_stream())
        ctx.store, ctx.dims = store, (U, T, t0, E, H)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(w_e, table, slots_d)
        return x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_x):
        w_e, table, slots_d = ctx.saved_tensors
        U, T, t0, E, H = ctx.dims
        need = ctx.needs_input_grad
        if g_x is None:
            return (None,) * 7
        dev = w_e.device
        g_x = g_x.to(torch.float32).contiguous()
        new = _f32_on(dev)
        d_w = new(H, E + 1) if need[0] else None
        d_b = new(H) if need[1] else None
        d_table = new(table.shape[0], E) if need[3] else None
        head = _store_args(ctx.store, slots_d, U, t0, T, table, E, H)
        ws = L.workspace("recnn_seq_embed_backward_workspace_bytes", U, T, H, E, device=dev)
        _call_backward("seq_embed", head, w_e, (L.ptr(g_x), L.ptr(d_w), L.ptr(d_b)), d_table, ws, (U, T, H, E, table.shape[0]), dev)
        return d_w, d_b, None, d_table, None, None, None


class TransformerBlockFunction(torch.autograd.Function):
    """y of one block with qkv, o, the log-sum-exp, u and the pre-activation kept, and its backward (`recnn_block_forward_train` /
    `recnn_block_backward`): differentiable in x and the twelve parameters; a gradient nobody needs is not computed."""

    @staticmethod
    def forward(ctx, x, cfg, *params):
        U, T, H = x.shape
        dev = x.device
        y = torch.empty_like(x)
        ctx.set_materialize_grads(False)
        if not any(ctx.needs_input_grad):
            ws = L.workspace("recnn_block_workspace_bytes", U, T, H, cfg[0], device=dev)
            L.call("recnn_block_forward", *_block_head(x, cfg), *(L.ptr(p) for p in params), L.ptr(y), L.ptr(ws), L.current_stream())
            return y
        saved, ctx.bwd_bytes = _train_buffers("recnn_block_train_workspace_bytes", dev, U, T, H, cfg[0], cfg[1])
        L.call("recnn_block_forward_train", *_block_head(x, cfg), *(L.ptr(p) for p in params), L.ptr(y), L.ptr(saved), L.current_stream())
        ctx.cfg = cfg
        ctx.save_for_backward(x, saved, *params)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_y):
        if g_y is None:
            return (None,) * 14
        x, saved, *params = ctx.saved_tensors
        need = ctx.needs_input_grad
        g_y = g_y.to(torch.float32).contiguous()
        d_x = torch.empty_like(x) if need[0] else None
        grads = [torch.empty_like(p) if need[2 + i] else None for i, p in enumerate(params)]
        ws = torch.empty(max(ctx.bwd_bytes, 16), dtype=torch.uint8, device=x.device)
        L.call("recnn_block_backward", *_block_head(x, ctx.cfg), *(L.ptr(p) for p in params), L.ptr(saved), L.ptr(g_y), L.ptr(d_x),
               *(L.ptr(g) for g in grads), L.ptr(ws), L.current_stream())
        return (d_x, None, *grads)


class LayerNormRowsFunction(torch.autograd.Function):
    """LN(x) over the last axis of x [U, T, H] and its backward (`recnn_layernorm_rows*`)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        out = torch.empty_like(x)
        H = x.shape[-1]
        L.call("recnn_layernorm_rows", L.ptr(x), x.numel() // H, H, L.ptr(gamma), L.ptr(beta), C.c_float(eps), L.ptr(out),
               L.current_stream())
        ctx.eps = eps
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, gamma)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        x, gamma = ctx.saved_tensors
        need = ctx.needs_input_grad
        H = x.shape[-1]
        rows = x.numel() // H
        g = g.to(torch.float32).contiguous()
        d_x = torch.empty_like(x) if need[0] else None
        d_g = torch.empty_like(gamma) if need[1] else None
        d_b = torch.empty_like(gamma) if need[2] else None
        ws = L.workspace("recnn_layernorm_rows_backward_workspace_bytes", rows, H, device=x.device)
        L.call("recnn_layernorm_rows_backward", L.ptr(x), rows, H, L.ptr(gamma), C.c_float(ctx.eps), L.ptr(g), L.ptr(d_x), L.ptr(d_g),
               L.ptr(d_b), L.ptr(ws), L.current_stream())
        return d_x, d_g, d_b, None


def transformer_encode_train(enc, store, table, slots, T, *, t0=0, train_table=False):
    """`transformer_encode` with a graph: the same arguments, checks and h -- bit for bit -- differentiable with respect to every
    parameter of the module.  Three kinds of autograd node are chained (the embedding, one per block, the final LayerNorm); between
    them only [U, T, H] tensors cross.  A block keeps qkv, o, the log-sum-exp, u and the feed-forward's pre-activation [U T, F]; its
    backward recomputes the normalised rows, the activation and the attention probabilities.  Fixed summation orders and no float
    atomics: equal calls give equal gradients bit for bit.  A frozen parameter's gradient is not computed.  Once differentiable.

    The embedding table is handled as in `attn_encode_train`: a `table` that requires grad is refused with RecnnHipError unless
    `train_table=True`, and then `table.grad` receives the dense [n_items, E] gradient, exact zeros in the rows of items the batch's
    steps do not hold -- also with every encoder parameter frozen.

    Under `torch.no_grad()`, or when nothing requires grad, this IS `transformer_encode`: nothing is kept."""
    _refuse_table_grad("transformer_encode_train", table, train_table)
    dev, E, H, U, T, t0, slots, params, cfg = _transformer_call_args("transformer_encode_train", enc, store, table, slots, T, t0)
    if not _wants_graph(table, params):
        return transformer_encode(enc, store, table.detach(), slots, T, t0=t0)
    x = SeqEmbedFunction.apply(params[0], params[1], store, table, torch.from_numpy(slots).to(dev), T, t0)
    for i in range(len(enc.layers)):
        x = TransformerBlockFunction.apply(x, cfg, *params[2 + 12 * i:14 + 12 * i])
    return LayerNormRowsFunction.apply(x, params[-2], params[-1], cfg[5])


# ------------------------------------------------------------------------------------------------------------------------
# Serving the two attention encoders step by step (nn/kv_cache.py, csrc/attn_dev.h): append n steps to sessions
# whose keys and values live in a KVCache; the returned rows are the whole-history call's, bit for bit.
def _append_call_args(name, enc, pnames, params, shapes_of, first, cache, table, items, ratings, rows):
    """The checks of `attn_append` / `transformer_append`, on the host and by argument name, before any launch (a refused call
    leaves the cache as it was): (dev, E, H, R, n, rows int64 numpy, items int32, ratings)."""
    from .kv_cache import KVCache, encoder_config
    dev, E, H = _attn_module_checked(name, enc, pnames, params, shapes_of, table)
    _module_on_gpu(name, params, first, dev)
    if not isinstance(cache, KVCache):
        raise L.RecnnHipError(f"{name}: cache must be a recnn_amd.nn.KVCache (got a {type(cache).__qualname__})")
    config = encoder_config(name, enc)
    if cache.config != config:
        raise L.RecnnHipError(f"{name}: the cache was built for (E, H, heads, layers, window) = {cache.config}, the encoder has {config}")
    kv = cache.kv
    if not (isinstance(kv, torch.Tensor) and kv.is_cuda):
        raise L.RecnnHipError(f"{name}: cache.kv must live on the GPU (recnn_amd has no CPU fallback)")
    if kv.dtype != torch.float32 or not kv.is_contiguous() or tuple(kv.shape) != (config[3], cache.n_sessions, cache.capacity, 2 * H) \
            or kv.device != dev:
        raise L.RecnnHipError(f"{name}: cache.kv must be a contiguous float32 [{config[3]}, {cache.n_sessions}, {cache.capacity}, "
                              f"{2 * H}] tensor on {dev} (got {kv.dtype} {tuple(kv.shape)} on {kv.device})")
    for arg, t, dtypes in (("table", table, (torch.float32,)), ("items", items, (torch.int64, torch.int32)),
                           ("ratings", ratings, (torch.float32,))):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise L.RecnnHipError(f"{name}: {arg} must be a GPU tensor (recnn_amd has no CPU fallback)")
        if t.dtype not in dtypes:
            raise L.RecnnHipError(f"{name}: {arg} must be {' or '.join(str(d) for d in dtypes)} (got {t.dtype})")
        if t.device != dev:
            raise ValueError(f"{name}: {arg} lives on {t.device}, the module on {dev}")
    if items.dim() != 2 or ratings.shape != items.shape:
        raise ValueError(f"{name}: items and ratings must both be [R, n] (got items {tuple(items.shape)}, ratings {tuple(ratings.shape)})")
    R, n = items.shape
    if not 1 <= n <= cache.max_append:
        raise ValueError(f"{name}: n = items.shape[1] = {n} must be in 1 .. max_append = {cache.max_append}")
    rows = cache.checked_rows(rows, name, count=R)
    lengths = cache.lengths
    if not (isinstance(lengths, np.ndarray) and lengths.shape == (cache.n_sessions,) and lengths.dtype == np.int64
            and (lengths >= 0).all()):
        raise ValueError(f"{name}: cache.lengths must be a non-negative int64 numpy array [{cache.n_sessions}]")
    if R and config[4] is None and int(lengths[rows].max()) + n > cache.capacity:
        raise ValueError(f"{name}: an append of n = {n} at position {int(lengths[rows].max())} runs past capacity = {cache.capacity} "
                         "(the encoder has no window: the cache is no ring)")
    if R and int(lengths[rows].max()) + n >= 1 << 30:
        raise ValueError(f"{name}: a session of {int(lengths[rows].max()) + n} positions; positions stay below 2^30")
    if items.dtype == torch.int64:      # an id outside the table stays outside it in 32 bits
        items = torch.where((items < 0) | (items >= table.shape[0]), -1, items).to(torch.int32)
    return dev, E, H, R, n, rows, items.contiguous(), ratings.contiguous()


def _cache_tail(cache, layer, pos_rows):
    """The trailing cache arguments of recnn_attn_append / recnn_block_append: this layer's kv, n_sessions, capacity, pos, rows."""
    return (L.ptr(cache.kv[layer]), cache.n_sessions, cache.capacity, L.ptr(pos_rows[0]), L.ptr(pos_rows[1]))


def _pos_rows(cache, rows, dev):
    """int32 [2, R] on the device: each row's position, then the row."""
    return torch.from_numpy(np.stack([cache.lengths[rows], rows]).astype(np.int32)).to(dev)


@torch.no_grad()
def attn_append(enc, cache, table, items, ratings, rows=None):
    """Extend the sessions `rows` of a `recnn_amd.nn.KVCache` by n steps each and return their h float32[R, n, H]: for a session whose
    appended inputs so far are x_0 .. x_{P + n - 1}, rows P .. P + n - 1 of `attn_encode` over those P + n steps, BIT FOR BIT -- however
    the history was split into appends, whatever R, the row's place in `rows`, the other sessions, the capacity, or the bits of slots
    the session has not written.  `items` int64 or int32 [R, n] and `ratings` float32 [R, n] are the new steps' inputs, given
    directly (no ReplayStore); `rows` the R distinct cache rows (default: all, in order); a row is extended from its own position
    `cache.lengths[row]`, and the call writes the new k and v into the cache and advances `lengths` by n.

    Four launches: the in-projection of the new rows (the gathered linear kernel reading [R, n] as a store), k and v into their
    slots, the attention of the new rows over the cache (query blocks aligned to absolute positions, key tiles staged from the ring),
    the out-projection.  An item id outside the table gives NaN rows for that session from that step on, as the whole-history call
    does for the steps it has not yet returned; other sessions keep their bits.

    Refused before any launch, the cache untouched -- RecnnHipError: everything `attn_encode` refuses of the module, a cache that is
    no KVCache or was built for another (E, H, heads, layers, window), a CPU cache, table, items or ratings, a wrong dtype;
    ValueError: items and ratings not both [R, n], n outside 1 .. cache.max_append, rows duplicate, out of range or not R of them,
    an append past capacity without a window."""
    params, shapes_of = _attn_spec("attn_append", enc)
    dev, E, H, R, n, rows, items, ratings = _append_call_args("attn_append", enc, _ATTN_PARAMS, params, shapes_of, "in_proj_weight",
                                                              cache, table, items, ratings, rows)
    h = _f32_on(dev)(R, n, H)
    if R == 0:
        return h
    user_off, slots = cache.dense_store(n)
    ws = L.workspace("recnn_kv_append_workspace_bytes", R, n, H, device=dev)
    L.call("recnn_attn_append", L.ptr(items), L.ptr(ratings), L.ptr(user_off), L.ptr(slots), R, n, L.ptr(table), table.shape[0], E, H,
           enc.num_heads, enc.window or 0, int(enc.alibi), L.ptr(enc.in_proj_weight), L.ptr(enc.in_proj_bias), L.ptr(enc.out_proj.weight),
           L.ptr(enc.out_proj.bias), *_cache_tail(cache, 0, _pos_rows(cache, rows, dev)), L.ptr(h), L.ptr(ws), L.current_stream())
    cache.lengths[rows] += n
    return h


@torch.no_grad()
def transformer_append(enc, cache, table, items, ratings, rows=None):
    """`attn_append` for a `recnn_amd.nn.TransformerStateEncoder`: h float32[R, n, H], rows P .. P + n - 1 of `transformer_encode`
    over the session's P + n steps, bit for bit; the cache holds k and v of every block.  The embedding of the new steps (the
    gathered linear kernel on [R, n] read as a store), per block the LN1 + in-projection, k and v into the block's slots, the
    attention over the cache, the out-projection with its residual and the fused feed-forward, then the final LayerNorm: the
    row-wise launches are `transformer_encode`'s kernels on R n dense rows.  Arguments, refusals and the NaN rule as `attn_append`,
    with everything `transformer_encode` refuses of the module."""
    name = "transformer_append"
    pnames, params, shapes_of, cfg = _transformer_spec(name, enc)
    dev, E, H, R, n, rows, items, ratings = _append_call_args(name, enc, pnames, params, shapes_of, "embed.weight", cache, table, items,
                                                              ratings, rows)
    x = _f32_on(dev)(R, n, H)
    y = torch.empty_like(x)
    if R == 0:
        return y
    user_off, slots = cache.dense_store(n)
    L.call("recnn_seq_embed", L.ptr(items), L.ptr(ratings), L.ptr(user_off), L.ptr(slots), R, 0, n, L.ptr(table), table.shape[0], E, H,
           L.ptr(params[0]), L.ptr(params[1]), L.ptr(x), L.current_stream())
    ws = L.workspace("recnn_kv_append_workspace_bytes", R, n, H, device=dev)
    pos_rows = _pos_rows(cache, rows, dev)
    for i in range(len(enc.layers)):
        L.call("recnn_block_append", *_block_head(x, cfg), *(L.ptr(p) for p in params[2 + 12 * i:14 + 12 * i]),
               *_cache_tail(cache, i, pos_rows), L.ptr(y), L.ptr(ws), L.current_stream())
        x, y = y, x
    L.call("recnn_layernorm_rows", L.ptr(x), R * n, H, L.ptr(params[-2]), L.ptr(params[-1]), C.c_float(cfg[5]), L.ptr(y),
           L.current_stream())
    cache.lengths[rows] += n
    return y


def state_encode(encoder, store, table, slots, T, *, train=False, train_table=False):
    """h float32[U, T, H] of whichever state encoder `encoder` is -- the one place that dispatches on the module's type (SeqEnv goes
    through it): a torch.nn.LSTM runs `lstm_encode` / `lstm_encode_train`, a torch.nn.GRU `gru_encode` / `gru_encode_train`, from a
    zero state at step 0, a recnn_amd.nn.AttentionEncoder `attn_encode` / `attn_encode_train`, a
    recnn_amd.nn.TransformerStateEncoder `transformer_encode` / `transformer_encode_train`.  Any other module is refused by name."""
    kw = dict(train_table=train_table) if train else {}
    if isinstance(encoder, AttentionEncoder):
        return (attn_encode_train if train else attn_encode)(encoder, store, table, slots, T, **kw)
    if isinstance(encoder, TransformerStateEncoder):
        return (transformer_encode_train if train else transformer_encode)(encoder, store, table, slots, T, **kw)
    if isinstance(encoder, torch.nn.LSTM):
        fn = lstm_encode_train if train else lstm_encode
    elif isinstance(encoder, torch.nn.GRU):
        fn = gru_encode_train if train else gru_encode
    else:
        t = type(encoder)
        raise L.RecnnHipError(f"state encoder: a {t.__module__}.{t.__qualname__} is not supported; the HIP encoders are a single-layer "
                              "torch.nn.LSTM(E + 1, H), a single-layer torch.nn.GRU(E + 1, H), a recnn_amd.nn.AttentionEncoder(E + 1, H, "
                              "heads) and a recnn_amd.nn.TransformerStateEncoder(E + 1, H, heads)")
    return fn(encoder, store, table, slots, T, **kw)[0]


class SeqCollectFunction(torch.autograd.Function):
    """The rows of `seq_collect`, and the gather that returns the gradients of the state / next_state rows to h."""

    @staticmethod
    def forward(ctx, h, steps, store, table, slots):
        U, T, H = h.shape
        rows, E = len(steps) * U, table.shape[1]
        views = (h.new_empty(rows, H), h.new_empty(rows, E), h.new_empty(rows, 1), h.new_empty(rows, H))
        seq_collect(h, steps, store, table, slots, views)
        ctx.steps, ctx.shape = np.asarray(steps, dtype=np.int32).reshape(-1), (U, T, H)
        ctx.mark_non_differentiable(views[1], views[2])
        ctx.set_materialize_grads(False)
        return views

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_state, _ga, _gr, g_next):
        U, T, H = ctx.shape
        if g_state is None and g_next is None:
            return None, None, None, None, None
        g_state, g_next = (None if g is None else g.to(torch.float32).contiguous() for g in (g_state, g_next))
        dev = (g_state if g_state is not None else g_next).device
        g_h = _f32_on(dev)(U, T, H)
        steps_d = torch.from_numpy(ctx.steps).to(dev)
        L.call("recnn_seq_collect_bwd", L.ptr(g_state), L.ptr(g_next), U, T, H, L.ptr(steps_d), len(ctx.steps), L.ptr(g_h),
               L.current_stream())
        return g_h, None, None, None, None


def seq_collect_rows(h, steps, store, table, slots):
    """`seq_collect` with a graph: allocates and returns (state, action, reward, next_state) for the kept `steps` (strictly
    increasing) of one user batch, rows in the order k * U + u, bit for bit what `seq_collect` writes.  The gradients of the
    state and next_state rows reach `h` (one gather launch, `recnn_seq_collect_bwd`); action and reward carry none."""
    if not (isinstance(h, torch.Tensor) and h.is_cuda):
        raise L.RecnnHipError(f"seq_collect_rows: needs GPU tensors (recnn_amd has no CPU fallback); got "
                              f"{h.device if isinstance(h, torch.Tensor) else type(h)}")
    st = np.asarray(steps, dtype=np.int64).reshape(-1)
    if len(st) > 1 and (np.diff(st) <= 0).any():
        raise ValueError(f"seq_collect_rows: steps must be strictly increasing (got {st.tolist()})")
    if h.dim() == 3 and h.dtype == torch.float32 and not h.is_contiguous():
        h = h.contiguous()
    return SeqCollectFunction.apply(h, [int(t) for t in st], store, table, slots)

