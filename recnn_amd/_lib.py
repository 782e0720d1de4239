"""ctypes binding of librecnn_hip.so (the C ABI declared in include/recnn_hip.h).

The library is the product: there is NO fallback.  If it has not been built
(`python -c "import __graft_entry__ as g; g.build()"` or `make -C recnn_amd/csrc`) every
entry point raises `RecnnHipMissing`.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RECNN_HIP_LIB") or os.path.join(_HERE, "csrc", "librecnn_hip.so")   # override: A/B of builds

F32, BF16, BF16X3 = 0, 1, 2      # BF16X3: split bf16 (hi + lo, three MFMAs per product), include/recnn_hip.h
DTYPES = {"fp32": F32, "bf16": BF16, "bf16x3": BF16X3}
MASK_NONE, MASK_HASH, MASK_EXTERNAL = 0, 1, 2
ALGO_DDPG, ALGO_TD3 = 0, 1
OPT_ADAM, OPT_RANGER = 0, 1
CAT_SOFTMAX, CAT_SAMPLE = 1, 2
LPB_ACCUMULATE, LPB_BF16 = 1, 2
NET_POLICY, NET_TARGET_POLICY, NET_VALUE1, NET_TARGET_VALUE1, NET_VALUE2, NET_TARGET_VALUE2 = range(6)


class RecnnHipMissing(RuntimeError):
    pass


class RecnnHipError(RuntimeError):
    pass


class GemmArgs(C.Structure):
    _fields_ = [
        ("dtype", C.c_int), ("M", C.c_int), ("N", C.c_int),
        ("A", C.c_void_p * 2), ("B", C.c_void_p * 2),
        ("lda", C.c_int64 * 2), ("ldb", C.c_int64 * 2),
        ("K", C.c_int * 2), ("a_f32", C.c_int * 2), ("b_f32", C.c_int * 2),
        ("C", C.c_void_p), ("ldc", C.c_int64), ("c_f32", C.c_int),
        ("bias", C.c_void_p), ("relu", C.c_int), ("mask_mode", C.c_int),
        ("mask", C.c_void_p), ("ld_mask", C.c_int64),
        ("seed", C.c_uint32), ("stream_id", C.c_uint32), ("step_ptr", C.c_void_p),
        ("addend", C.c_void_p), ("ld_add", C.c_int64), ("add_clip", C.c_float), ("add_row_div", C.c_int),
        ("yref", C.c_void_p), ("ldy", C.c_int64), ("dx_scale", C.c_float),
        ("colsum", C.c_void_p),
        ("dw_splits", C.c_int), ("dw_slab_stride", C.c_int64),
        ("dw_valid_cols", C.c_int), ("dw_col_rot", C.c_int),
        ("ws", C.c_void_p), ("ws_bytes", C.c_int64),
    ]


class ShadowOut(C.Structure):
    """include/recnn_hip.h recnn_shadow_out"""
    _fields_ = [("dst", C.c_void_p), ("cols", C.c_int), ("ld", C.c_int64), ("bf16", C.c_int)]


class AeParams(C.Structure):
    """include/recnn_hip.h recnn_ae_params (the anomaly detector's parameters and BatchNorm state)"""
    _fields_ = [("w", C.c_void_p * 4), ("b", C.c_void_p * 4), ("gamma", C.c_void_p * 3), ("beta", C.c_void_p * 3),
                ("running_mean", C.c_void_p * 3), ("running_var", C.c_void_p * 3), ("num_batches_tracked", C.c_void_p * 3),
                ("eps", C.c_float * 3), ("momentum", C.c_float * 3)]


class AeGrads(C.Structure):
    """include/recnn_hip.h recnn_ae_grads"""
    _fields_ = [("w", C.c_void_p * 4), ("b", C.c_void_p * 4), ("gamma", C.c_void_p * 3), ("beta", C.c_void_p * 3)]


class EngineConfig(C.Structure):
    _fields_ = [
        ("algo", C.c_int), ("dtype", C.c_int), ("state_dim", C.c_int), ("action_dim", C.c_int),
        ("hidden", C.c_int), ("max_rows", C.c_int), ("mask_mode", C.c_int), ("seed", C.c_uint32),
        ("device", C.c_int),
    ]


class Hyper(C.Structure):
    _fields_ = [
        ("gamma", C.c_float), ("min_value", C.c_float), ("max_value", C.c_float),
        ("soft_tau", C.c_float), ("policy_every", C.c_int),
        ("noise_std", C.c_float), ("noise_clip", C.c_float),
        ("lr", C.c_float * 2), ("beta1", C.c_float * 2), ("beta2", C.c_float * 2),
        ("eps", C.c_float * 2), ("weight_decay", C.c_float * 2),
        ("opt_kind", C.c_int * 2), ("la_alpha", C.c_float * 2), ("la_k", C.c_int * 2), ("nsma_threshold", C.c_float * 2),
    ]


class EngineSizes(C.Structure):
    _fields_ = [
        ("master_floats_actor", C.c_int64), ("master_floats_critic", C.c_int64),
        ("workspace_bytes", C.c_int64), ("ld_x", C.c_int64), ("x_rows", C.c_int64),
    ]


class Sampler(C.Structure):
    _fields_ = [
        ("items", C.c_void_p), ("ratings", C.c_void_p), ("user_off", C.c_void_p), ("perm", C.c_void_p),
        ("users_per_batch", C.c_int), ("n_batches", C.c_int), ("frame", C.c_int), ("emb_dim", C.c_int),
        ("table", C.c_void_p), ("row_off", C.c_void_p), ("cursor", C.c_void_p),
        ("plan", C.c_void_p), ("plan_rows", C.c_int),
    ]


TUNING_FIELDS = ("fused_mlp", "chain_target_critic", "bwd_panel", "policy_chain", "split_fwd", "cycle_min_len", "cycle_min_seg",
                 "frozen_fused", "frozen_gemm", "graph_run", "pregather", "defer_policy_fwd", "sampler_f32_rows", "dw_splits", "comm_fused",
                 "l1_big", "gemm_variant", "gemm_v0_threshold", "gemm_dma", "gemm_dma_depth", "gemm_dma_waves", "gemm_waves", "dw_dma", "x3_tail", "x3_fwd", "dw_fuse", "tail_half", "l1_ws", "frozen_half",
                 "frozen_window", "run_align", "frozen_acts_policy_only", "gather_cycle", "policy_fused")


RUN_MAX = 64
RUN_STEP, RUN_POLICY_STEP, RUN_ORDINARY, RUN_POLICY_HEAD, RUN_MULTI, RUN_ALIGNED_MULTI, RUN_ALIGNED_CYCLE = range(7)


class RunFamily(C.Structure):
    """include/recnn_hip.h recnn_run_family: which run graphs recnn_engine_graph_build captures."""
    _fields_ = [("has_o", C.c_ubyte * (RUN_MAX + 1)), ("has_p", C.c_ubyte * (RUN_MAX + 1)), ("multi_len", C.c_int),
                ("aligned_multi_len", C.c_int), ("aligned_cycle_len", C.c_int)]


class EngineTuning(C.Structure):
    """include/recnn_hip.h recnn_engine_tuning: schedule / tile choices of ONE engine (all compute the same numbers)."""
    _fields_ = [(f, C.c_int) for f in TUNING_FIELDS]


_P = C.c_void_p
_I = C.c_int
_L = C.c_int64
_F = C.c_float
_U = C.c_uint32

# name -> (restype, argtypes).  Mirrors include/recnn_hip.h one to one.
SIGNATURES = {
    "recnn_abi_version": (_I, []),
    "recnn_last_error": (C.c_char_p, []),
    "recnn_abi_sizeof": (_L, [_I]),
    "recnn_engine_tuning_init": (None, [C.POINTER(EngineTuning)]),
    "recnn_engine_set_tuning": (_I, [_P, C.POINTER(EngineTuning)]),
    "recnn_engine_get_tuning": (_I, [_P, C.POINTER(EngineTuning)]),
    "recnn_engine_sampler_eager": (_I, [_P, _I]),
    "recnn_engine_unit_backward": (_I, [_P]),
    "recnn_engine_dp_sets": (_I, [_P]),
    "recnn_engine_read_counters": (_I, [_P, _P, _P]),
    "recnn_frame_plan_rows": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "recnn_frame_plan_dense": (_I, [_P, _P, _I, _I, _I, _I, _P, _L, _P, _P]),
    "recnn_frame_plan": (_I, [_P, _P, _I, _I, _P, _P, _I, _P]),
    "recnn_frame_gather": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _L, _P, _L, _P, _L, _P, _P, _P, _I, _P]),
    "recnn_pack_batch": (_I, [_P, _L, _P, _L, _P, _L, _I, _I, _I, _P, _P, _L, _P]),
    "recnn_gemm_fwd": (_I, [C.POINTER(GemmArgs), _P]),
    "recnn_gemm_dx": (_I, [C.POINTER(GemmArgs), _P]),
    "recnn_gemm_dw": (_I, [C.POINTER(GemmArgs), _P]),
    "recnn_x3_pack": (_I, [_P, _L, _I, _I, _P, _L, _P]),
    "recnn_x3_unpack": (_I, [_P, _L, _I, _I, _P, _L, _P]),
    "recnn_hash_mask_dump": (_I, [_U, C.c_int32, _U, _I, _I, _P, _P]),
    "recnn_hash_mask_dump_at": (_I, [_U, _P, _I, _U, _I, _I, _P, _P]),
    "recnn_soft_update_flat": (_I, [_P, _P, _L, _F, _P]),
    "recnn_adam_flat": (_I, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _I, _F, _P]),
    "recnn_adam_flat_shadow": (_I, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _I, _F, _P, _P]),
    "recnn_adam_flat_at": (_I, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _P, _I, _F, _P]),
    "recnn_l1_norm_flat": (_I, [_P, _L, _P, _P, _P]),
    "recnn_engine_query": (_I, [C.POINTER(EngineConfig), C.POINTER(EngineSizes)]),
    "recnn_engine_create": (_I, [C.POINTER(EngineConfig), _P, C.POINTER(_P)]),
    "recnn_engine_destroy": (None, [_P]),
    "recnn_engine_bind_net": (_I, [_P, _I, _P, _P, _P, _P]),
    "recnn_engine_bind_batch": (_I, [_P, _P, _P, _P, _P]),
    "recnn_engine_bind_slow": (_I, [_P, _I, _P]),
    "recnn_categorical_rows": (_I, [_P, _L, _I, _I, _I, C.c_uint32, C.c_int32, _P, _P, _P, _P]),
    "recnn_logprob_bwd": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _L, _I, _P, _P, _P]),
    "recnn_softmax_bwd": (_I, [_P, _L, _I, _I, _P, _L, _P, _L, _P]),
    "recnn_onehot_rows": (_I, [_P, _I, _I, _P, _L, _P]),
    "recnn_colsum_rows": (_I, [_P, _L, _I, _I, _P, _P]),
    "recnn_shard_softmax_pass": (_I, [_P, _L, _I, _I, _I, _P, _P, _P, _P]),
    "recnn_shard_logprob_bwd": (_I, [_P, _L, _I, _I, _P, _P, _P, _L, _P]),
    "recnn_transpose_rows": (_I, [_P, _L, _I, _I, _P, _L, _I, _P]),
    "recnn_vae_latent_fwd": (_I, [_P, _L, _P, _L, _I, _I, _P, _L, _P, _L, _P]),
    "recnn_vae_latent_bwd": (_I, [_P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _P, _L, _P]),
    "recnn_vae_loss_fwd": (_I, [_P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _F, _P, _P, _P]),
    "recnn_vae_loss_bwd": (_I, [_P, _L, _P, _L, _P, _L, _P, _L, _I, _I, _I, _P, _F, _P, _L, _P, _L, _P, _L, _P]),
    "recnn_csr_workspace_bytes": (_I, [_L, C.POINTER(_L)]),
    "recnn_csr_build": (_I, [_P, _P, _P, _P, _L, _P, _P, _I, _P, _P, _P, _P, _P, _P, C.POINTER(_L), _P, _L, _P]),
    "recnn_ranger_flat": (_I, [_P, _P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _F, _I, _F, _I, _F, _P]),
    "recnn_ranger_flat_shadow": (_I, [_P, _P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _F, _I, _F, _I, _F, _P, _P]),
    "recnn_engine_bind_external": (_I, [_P, _P, _P]),
    "recnn_engine_bind_sampler": (_I, [_P, C.POINTER(Sampler)]),
    "recnn_engine_profile": (_I, [_P, _I, _I, _I, _P, C.POINTER(_F), C.POINTER(C.c_double), C.POINTER(C.c_char_p), C.POINTER(_I)]),
    "recnn_engine_set_hyper": (_I, [_P, C.POINTER(Hyper)]),
    "recnn_engine_set_mask_mode": (_I, [_P, _I]),
    "recnn_engine_refresh": (_I, [_P, _I, _P]),
    "recnn_engine_set_counters": (_I, [_P, _I, _I, _I, _I]),
    "recnn_engine_step": (_I, [_P, _I, _I, _I, _P]),
    "recnn_engine_value_grads": (_I, [_P, _I, _I, _P]),
    "recnn_engine_value_apply": (_I, [_P, _I, _F, _P]),
    "recnn_engine_policy_grads": (_I, [_P, _I, _I, _P]),
    "recnn_engine_state_grads": (_I, [_P, _I, _I, _P, _L, _P]),
    "recnn_engine_policy_apply": (_I, [_P, _I, _F, _P]),
    "recnn_engine_clip_policy_grads": (_I, [_P, _F, _P]),
    "recnn_engine_soft_update": (_I, [_P, _I, _I, _F, _P]),
    "recnn_engine_finish": (_I, [_P, _I, _I, _I, _P]),
    "recnn_engine_graph_build": (_I, [_P, _I, _P]),
    "recnn_engine_graph_run": (_I, [_P, _I, _I, _P]),
    "recnn_engine_graph_prepare": (_I, [_P, _I, _I, _P]),
    "recnn_run_family_init": (_I, [_I, _I, _I, _P]),
    "recnn_run_plan": (_I, [_I, _P, _I, _I, _I, _P, _P, _I]),
    "recnn_engine_dp_graph_build": (_I, [_P, _I, _F, _I, _P]),
    "recnn_engine_dp_graph_launch": (_I, [_P, _I, _P]),
    "recnn_comm_create": (_I, [_I, _I, _L, C.POINTER(_P)]),
    "recnn_comm_handle_bytes": (_L, []),
    "recnn_comm_export": (_I, [_P, _P, _L]),
    "recnn_comm_connect": (_I, [_P, _P, _L]),
    "recnn_dp_allreduce_flat": (_I, [_P, _P, _L, _P]),
    "recnn_comm_status": (_I, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "recnn_comm_set_timeout_ms": (_I, [_P, _I]),
    "recnn_comm_clear_status": (_I, [_P]),
    "recnn_comm_destroy": (None, [_P]),
    "recnn_engine_set_comm": (_I, [_P, _P, _F]),
    "recnn_comm_create_ex": (_I, [_I, _I, _L, _I, C.POINTER(_P)]),
    "recnn_comm_set_workgroups": (_I, [_P, _I]),
    "recnn_engine_read_losses": (_I, [_P, _P, _P]),
    "recnn_topk_item_aux": (_I, [_P, _I, _I, _I, _P, _P]),
    "recnn_topk_workspace_bytes": (_I, [_I, _I, C.POINTER(_L)]),
    "recnn_topk_search": (_I, [_P, _L, _I, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P]),
    "recnn_dist_item_aux_floats": (_I, [_I, _I, _I, C.POINTER(_L)]),
    "recnn_dist_item_aux": (_I, [_P, _I, _I, _I, _P, _P]),
    "recnn_dist_workspace_bytes": (_I, [_I, _I, _I, _I, C.POINTER(_L)]),
    "recnn_dist_matrix": (_I, [_P, _L, _I, _P, _I, _I, _I, C.c_double, _P, _P, _L, _P, _P]),
    "recnn_dist_topk": (_I, [_P, _L, _I, _P, _I, _I, _I, C.c_double, _P, _I, _P, _P, _P, _P]),
    "recnn_ae_act_floats": (_I, [_I, C.POINTER(_L)]),
    "recnn_ae_workspace_bytes": (_I, [_I, C.POINTER(_L)]),
    "recnn_ae_eval": (_I, [C.POINTER(AeParams), _P, _L, _I, _P, _L, _P, _P]),
    "recnn_ae_forward": (_I, [C.POINTER(AeParams), _I, _P, _L, _I, _P, _L, _P, _P, _I, _P, _P]),
    "recnn_ae_backward": (_I, [C.POINTER(AeParams), C.POINTER(AeGrads), _I, _P, _L, _I, _P, _L, _P, _L, _P, _P, _L, _P, _P]),
    "recnn_dqn_head": (_I, [_P, _L, _I, _P, _L, _I, _P, _I, _P, _P, _P, _L, _P, _P]),
    "recnn_dqn_row_dot": (_I, [_P, _L, _I, _P, _L, _P, _I, _P, _P, _P]),
    "recnn_dqn_colsum_workspace_floats": (_I, [_I, _I, C.POINTER(_L)]),
    "recnn_dqn_colsum": (_I, [_P, _L, _I, _I, _F, _P, _P, _P]),
    "recnn_dqn_mean": (_I, [_P, _P, _P, _I, _I, _P, _P]),
    "recnn_dqn_td": (_I, [_P, _P, _P, _P, _P, _P, _F, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "recnn_dqn_dh": (_I, [_P, _L, _I, _P, _L, _I, _P, _P, _P, _P, _P, _P, _P]),
    "recnn_dqn_scatter_workspace_bytes": (_I, [_L, _I, C.POINTER(_L)]),
    "recnn_dqn_scatter_sum": (_I, [_P, _L, _I, _I, _P, _L, _P, _I, _P, _P, _P, _P, _P, _P]),
    "recnn_dqn_clip": (_I, [_P, _L, _P, _F, _P]),
    "recnn_radam_flat": (_I, [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _I, _P, _F, _P]),
    "recnn_engine_buffer": (_P, [_P, C.c_char_p, C.POINTER(_L), C.POINTER(_L), C.POINTER(_L), C.POINTER(_I)]),
    "recnn_topk_stats_workspace_bytes": (_I, [_I, _I, C.POINTER(_L)]),
    "recnn_topk_stats": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "recnn_seq_gather": (_I, [_P, _P, _P, _P, _I, _I, _P, _I, _I, _P, _P, _P, _P]),
    "recnn_seq_gather_idx": (_I, [_P, _L, _P, _I, _I, _P, _P]),
    "recnn_lstm_workspace_bytes": (_I, [_I, _I, _I, _I, C.POINTER(_L)]),
    "recnn_lstm_encode": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P]),
    "recnn_seq_collect": (_I, [_P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "recnn_lstm_train_workspace_bytes": (_I, [_I, _I, _I, _I, _I, C.POINTER(_L), C.POINTER(_L)]),
    "recnn_lstm_encode_train": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P]),
    "recnn_lstm_backward": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "recnn_lstm_table_grad_workspace_bytes": (_I, [_I, _I, _I, _I, _I, C.POINTER(_L)]),
    "recnn_lstm_backward_table": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _I] + [_P] * 18),
    "recnn_seq_collect_bwd": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _P]),
    "recnn_gru_workspace_bytes": (_I, [_I, _I, _I, _I, C.POINTER(_L)]),
    "recnn_gru_encode": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _I] + [_P] * 7 + [_I, _P, _P]),
    "recnn_gru_train_workspace_bytes": (_I, [_I, _I, _I, _I, _I, C.POINTER(_L), C.POINTER(_L)]),
    "recnn_gru_encode_train": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _I] + [_P] * 7 + [_I, _P, _P, _P]),
    "recnn_gru_backward": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _I] + [_P] * 13),
    "recnn_gru_table_grad_workspace_bytes": (_I, [_I, _I, _I, _I, _I, C.POINTER(_L)]),
    "recnn_gru_backward_table": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _I] + [_P] * 16),
    "recnn_attn_workspace_bytes": (_I, [_I, _I, _I, _I, C.POINTER(_L)]),
    "recnn_attn_encode": (_I, [_P, _P, _P, _P, _I, _I, _I, _P] + [_I] * 6 + [_P] * 7),
    "recnn_attn_train_workspace_bytes": (_I, [_I, _I, _I, _I, _I, C.POINTER(_L), C.POINTER(_L)]),
    "recnn_attn_encode_train": (_I, [_P, _P, _P, _P, _I, _I, _I, _P] + [_I] * 6 + [_P] * 7),
    "recnn_attn_backward": (_I, [_P, _P, _P, _P, _I, _I, _I, _P] + [_I] * 6 + [_P] * 9),
    "recnn_attn_table_grad_workspace_bytes": (_I, [_I, _I, _I, _I, _I, C.POINTER(_L)]),
    "recnn_attn_backward_table": (_I, [_P, _P, _P, _P, _I, _I, _I, _P] + [_I] * 6 + [_P] * 12),
    "recnn_seq_embed": (_I, [_P, _P, _P, _P, _I, _I, _I, _P] + [_I] * 3 + [_P] * 4),
    "recnn_seq_embed_backward_workspace_bytes": (_I, [_I, _I, _I, _I, C.POINTER(_L)]),
    "recnn_seq_embed_backward": (_I, [_P, _P, _P, _P, _I, _I, _I, _P] + [_I] * 3 + [_P] * 5),
    "recnn_seq_embed_table_grad_workspace_bytes": (_I, [_I, _I, _I, _I, _I, C.POINTER(_L)]),
    "recnn_seq_embed_backward_table": (_I, [_P, _P, _P, _P, _I, _I, _I, _P] + [_I] * 3 + [_P] * 8),
    "recnn_block_workspace_bytes": (_I, [_I, _I, _I, _I, C.POINTER(_L)]),
    "recnn_block_forward": (_I, [_P] + [_I] * 8 + [_F] + [_P] * 15),
    "recnn_block_train_workspace_bytes": (_I, [_I, _I, _I, _I, _I, C.POINTER(_L), C.POINTER(_L)]),
    "recnn_block_forward_train": (_I, [_P] + [_I] * 8 + [_F] + [_P] * 15),
    "recnn_block_backward": (_I, [_P] + [_I] * 8 + [_F] + [_P] * 29),
    "recnn_layernorm_rows": (_I, [_P, _I, _I, _P, _P, _F, _P, _P]),
    "recnn_layernorm_rows_backward_workspace_bytes": (_I, [_I, _I, C.POINTER(_L)]),
    "recnn_layernorm_rows_backward": (_I, [_P, _I, _I, _P, _F, _P, _P, _P, _P, _P, _P]),
    "recnn_kv_min_capacity": (_I, [_I, _I, C.POINTER(_I)]),
    "recnn_kv_append_workspace_bytes": (_I, [_I, _I, _I, C.POINTER(_L)]),
    "recnn_attn_append": (_I, [_P, _P, _P, _P, _I, _I, _P] + [_I] * 6 + [_P] * 5 + [_I, _I] + [_P] * 5),
    "recnn_block_append": (_I, [_P] + [_I] * 8 + [_F] + [_P] * 13 + [_I, _I] + [_P] * 5),
    "recnn_dist_target_rank_workspace_bytes": (_I, [_I, _I, _I, C.POINTER(_L)]),
    "recnn_dist_target_rank": (_I, [_P, _L, _I, _P, _I, _I, _I, C.c_double, _P, _P, _P, _P, _P]),
    "recnn_topk_target_rank_workspace_bytes": (_I, [_I, _I, C.POINTER(_L)]),
    "recnn_topk_target_rank": (_I, [_P, _L, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "recnn_rank_metrics_workspace_bytes": (_I, [_I, C.POINTER(_L)]),
    "recnn_rank_metrics": (_I, [_P, _P, _I, _P, _I, _P, _P, _P, _P]),
    "recnn_seen_mask_words": (_I, [_I, C.POINTER(_L)]),
    "recnn_seen_mask_build": (_I, [_P, _L, _P, _P, _P, _I, _I, _P, _P]),
    "recnn_topk_search_excluding": (_I, [_P, _L, _I, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, _L]),
    "recnn_dist_topk_excluding": (_I, [_P, _L, _I, _P, _I, _I, _I, C.c_double, _P, _I, _P, _P, _P, _P, _P, _L]),
    "recnn_topk_target_rank_excluding": (_I, [_P, _L, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _L]),
    "recnn_dist_target_rank_excluding": (_I, [_P, _L, _I, _P, _I, _I, _I, C.c_double, _P, _P, _P, _P, _P, _P, _L]),
    "recnn_qrank_hidden_padded": (_I, [_I, C.POINTER(_I)]),
    "recnn_qrank_block_rows": (_I, [_I, _L, C.POINTER(_L)]),
    "recnn_qrank_layer1": (_I, [_P, _L, _I, _I, _P, _L, _P, _I, _P, _L, _P]),
    "recnn_qrank_scores": (_I, [_P, _L, _I, _P, _L, _I, _I, _P, _P, _P, _F, _P, _L, _P]),
    "recnn_scores_topk_workspace_bytes": (_I, [_I, _I, C.POINTER(_L)]),
    "recnn_scores_topk": (_I, [_P, _L, _I, _I, _I, _P, _P, _P, _P, _P, _L]),
    "recnn_scores_rank_workspace_bytes": (_I, [_I, _I, C.POINTER(_L)]),
    "recnn_scores_rank": (_I, [_P, _L, _I, _I, _P, _P, _P, _P, _P, _L]),
    "recnn_qcand_scores": (_I, [_P, _L, _I, _P, _L, _I, _I, _P, _P, _P, _F, _P, _L, _I, _I, _P, _L, _P]),
    "recnn_qcand_rerank": (_I, [_P, _L, _I, _P, _L, _I, _I, _P, _P, _P, _F, _P, _L, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "recnn_ivf_lists_workspace_bytes": (_I, [_I, _I, C.POINTER(_L)]),
    "recnn_ivf_build_lists": (_I, [_P, _I, _I, _P, _P, _P, _P, _P]),
    "recnn_ivf_update_centroids": (_I, [_P, _I, _P, _P, _I, _P, _P]),
    "recnn_ivf_gather_rows": (_I, [_P, _I, _P, _P, _P]),
    "recnn_ivf_search_workspace_bytes": (_I, [_I, _I, _I, _I, C.POINTER(_L)]),
    "recnn_ivf_scan": (_I, [_P, _L, _I, _P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _P, _P, _L]),
    "recnn_slate_similarity": (_I, [_P, _I, _P, _L, _I, _I, _I, _I, _P, _P]),
    "recnn_slate_rerank": (_I, [_P, _I, _P, _L, _I, _I, _I, _I, _P, _L, _F, _I, _I, _P, _P, _P, _P]),
    "recnn_slate_ild": (_I, [_P, _I, _P, _L, _I, _I, _I, _I, _P, _P]),
    "recnn_catalogue_logprob_workspace_bytes": (_I, [_I, _I, _I, C.POINTER(_L)]),
    "recnn_catalogue_logprob": (_I, [_P, _L, _I, _I, _P, _L, _I, _P, _I, _P, _I, _P, _P, _P, _P]),
    "recnn_catalogue_logprob_bwd_workspace_bytes": (_I, [_I, _I, _I, _I, C.POINTER(_L)]),
    "recnn_catalogue_logprob_bwd": (_I, [_P, _L, _I, _I, _P, _L, _I, _P, _I, _P, _P, _P, _P, _I, _P, _L, _P, _L, _P, _P, _P]),
    "recnn_ope_accumulate_workspace_bytes": (_I, [_I, C.POINTER(_L)]),
    "recnn_ope_accumulate": (_I, [_P, _P, _P, _P, _P, _P, _I, C.c_double, _I, _P, _P, _P, _P]),
    "recnn_sampled_logprob_workspace_bytes": (_I, [_I, _I, _I, C.POINTER(_L)]),
    "recnn_sampled_logprob": (_I, [_P, _L, _I, _I, _P, _L, _I, _P, _I, _P, _P, _I, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "recnn_sampled_logprob_bwd_workspace_bytes": (_I, [_I, _I, _I, _I, C.POINTER(_L)]),
    "recnn_sampled_logprob_bwd": (_I, [_P, _L, _I, _I, _P, _L, _I, _P, _I, _P, _P, _I, _P, _I, _P, _P, _P, _P, _I,
                                       _P, _L, _P, _L, _P, _P, _P, _L, _P, _P]),
    "recnn_sampled_scatter_workspace_bytes": (_I, [_I, _I, _I, _I, C.POINTER(_L)]),
    "recnn_sampled_scatter": (_I, [_P, _I, _P, _I, _P, _L, _P, _P, _L, _I, _P, _I, _I, _P, _L, _P, _P, _P]),
}

class FrozenDebugArgs(C.Structure):
    """recnn_amd/csrc/recnn_hip_debug.h recnn_debug_frozen_args: one frozen network on caller-supplied device buffers."""
    _fields_ = [("A", C.c_void_p * 4), ("lda", C.c_int64 * 4), ("K", C.c_int * 4), ("w1_col", C.c_int * 4), ("nseg", C.c_int),
                ("W1", C.c_void_p), ("ldw1", C.c_int64), ("W2", C.c_void_p), ("ldw2", C.c_int64), ("W3", C.c_void_p), ("ldw3", C.c_int64),
                ("b1", C.c_void_p), ("b2", C.c_void_p), ("b3", C.c_void_p), ("w3row", C.c_void_p),
                ("rows", C.c_int), ("H", C.c_int), ("out_dim", C.c_int), ("mask_mode", C.c_int),
                ("seed", C.c_uint32), ("stream1", C.c_uint32), ("stream2", C.c_uint32),
                ("step", C.c_int), ("rows_per_set", C.c_int),
                ("h1", C.c_void_p), ("h2", C.c_void_p), ("ldh", C.c_int64), ("store_row0", C.c_int),
                ("out", C.c_void_p), ("ldo", C.c_int64), ("addend", C.c_void_p), ("ld_add", C.c_int64), ("add_clip", C.c_float),
                ("q", C.c_void_p), ("panel_rows", C.c_int)]


class GatherCycleDebugArgs(C.Structure):
    """recnn_amd/csrc/recnn_hip_debug.h recnn_debug_gather_cycle_args: the cycle gather on caller-supplied device buffers."""
    _fields_ = [("items", C.c_void_p), ("ratings", C.c_void_p), ("table", C.c_void_p),
                ("plan", C.c_void_p), ("plan_stride", C.c_int64),
                ("cursor", C.c_void_p), ("cursor_add", C.c_int), ("cursor_mod", C.c_int),
                ("rows", C.c_int), ("frame", C.c_int), ("emb", C.c_int), ("n_sets", C.c_int),
                ("state_h", C.c_void_p), ("action_h", C.c_void_p), ("next_h", C.c_void_p), ("ld_h", C.c_int64),
                ("tail_n", C.c_void_p), ("ld_tail", C.c_int64),
                ("reward", C.c_void_p), ("done", C.c_void_p),
                ("gather_cycle", C.c_int)]


# private debug / test hooks (recnn_amd/csrc/recnn_hip_debug.h): exported, but not part of the public header
DEBUG_SIGNATURES = {
    "recnn_debug_gather_cycle": (_I, [C.POINTER(GatherCycleDebugArgs), _L, _P]),
    "recnn_debug_frozen_forward": (_I, [C.POINTER(FrozenDebugArgs), _L, _P]),
    "recnn_debug_mlp_fault": (None, [_I]),
    "recnn_debug_mlp_probe": (None, [_I]),
    "recnn_debug_mlp_trace": (None, [_P]),
    "recnn_debug_tail_trace": (None, [_P]),
    "recnn_debug_frozen_trace": (None, [_P]),
    "recnn_debug_l1_trace": (None, [_P]),
    "recnn_debug_x3_fwd": (None, [_I]),
    "recnn_debug_x3_ws_probe": (None, [_I]),
    "recnn_debug_wide_ws": (None, [_I]),
    "recnn_debug_ws_trace": (None, [_P]),
    "recnn_debug_dwadam_trace": (None, [_P]),
}

_lib = None


def load():
    """Load librecnn_hip.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RecnnHipMissing(
            f"{LIB_PATH} not found: build it with `make -C recnn_amd/csrc` "
            "(or __graft_entry__.build()).  recnn_amd has no CPU or PyTorch fallback.")
    import torch  # noqa: F401  -- loads libamdhip64.so.7 first; ours must bind to the same runtime
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in list(SIGNATURES.items()) + list(DEBUG_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for which, st in enumerate((GemmArgs, EngineConfig, Hyper, EngineSizes, Sampler, EngineTuning, ShadowOut,
                                     AeParams, AeGrads)):
        if lib.recnn_abi_sizeof(which) != C.sizeof(st):
            raise RecnnHipError(f"ABI mismatch for {st.__name__}: C={lib.recnn_abi_sizeof(which)} py={C.sizeof(st)}")
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().recnn_last_error()
        raise RecnnHipError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def call(name: str, *args):
    """Call an int-returning entry point and raise on a non-zero code."""
    check(getattr(load(), name)(*args), name)


def ptr(t):
    """Device (or host) address of a torch tensor, None -> NULL."""
    return None if t is None else C.c_void_p(t.data_ptr())


def workspace(query: str, *args, device):
    """Scratch tensor (uint8) of the size the entry point `query` (a `recnn_*_workspace_bytes` or `*_floats`) reports for `args`,
    never empty: a zero-size request still gets storage to point at."""
    import torch
    n = C.c_int64()
    call(query, *args, C.byref(n))
    nbytes = n.value * (4 if query.endswith("_floats") else 1)
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
