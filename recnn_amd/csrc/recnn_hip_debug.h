/* recnn_hip_debug.h -- PRIVATE debug / test hooks of librecnn_hip.so: in-kernel shader-clock traces, timing probes and fault
 * injection.  Not part of the public C ABI (include/recnn_hip.h): process-wide, not thread-safe, results of probe runs are
 * garbage by design.  Used by tests/test_gpu_engine.py::test_broken_handoff_is_reported and tools/{mlp,split}_trace.py. */
#ifndef RECNN_HIP_DEBUG_H
#define RECNN_HIP_DEBUG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* break an in-launch hand-off of the fused forward on purpose: 1 = producers do not raise their flag, 2 = critics do not fill the
 * Q slot; the bounded waits then report through recnn_engine_read_losses / read_counters (RECNN_E_STATE).  0 = off. */
void recnn_debug_mlp_fault(int mode);
/* timing experiments on the fused forward (csrc/mlps.hip): bit 0 = no MFMA work / fragment reads, bit 1 = no DMA */
void recnn_debug_mlp_probe(int bits);
/* shader-clock stamps of a kernel's phases: device uint64 [workgroup][32] (mlps_fwd_kernel) / [workgroup][16]; NULL = off */
void recnn_debug_mlp_trace(void* device_u64_wg32);
void recnn_debug_tail_trace(void* device_u64_wg16);
void recnn_debug_frozen_trace(void* device_u64_wg16);   /* mlp_frozen_kernel: read at launch (= capture) time */
void recnn_debug_l1_trace(void* device_u64_wg16);
/* ONE frozen network (csrc/mlpf.hip mlp_frozen_kernel) on caller-supplied device buffers: the direct way to the kernel's edge cases (two
 * and three layer-1 slabs, every segment boundary, ragged panels, a first stored row), which the engine's networks -- 21 or 23 slabs --
 * never reach.  Layer 1 contracts nseg (1..4) k-contiguous bf16 segments A[g] [rows, lda[g]] (K[g] a multiple of 64) against columns
 * w1_col[g] .. of W1 [H, ldw1]; W3 != NULL: an actor (out [rows, ldo] bf16 = h2 W3^T + b3 + clip(addend), out_dim <= 128), else a critic
 * (q [rows] fp32 = h2 . w3row + b3[0]).  mask_mode RECNN_MASK_NONE | RECNN_MASK_HASH with (seed, step + batch index, stream1 | stream2),
 * batches of rows_per_set rows (0: one batch); h1 / h2 optional bf16 [rows, ldh], rows store_row0 .. stored.  panel_rows 128 | 64 (the
 * same numbers).  Whatever H and out_dim, the kernel streams 256 rows of W1 and W2, 128 rows of W3 and 256 columns of W2 / W3, and stores
 * 256 columns of h1 / h2 (+0 at and beyond H): the arrays must be that large (ldw2, ldw3, ldh >= 256 are checked; the row counts cannot
 * be); what lies at or beyond H never reaches a result.  sizeof_args = sizeof(recnn_debug_frozen_args) as the caller sees it (refused if it differs). */
typedef struct recnn_debug_frozen_args {
  const void* A[4]; int64_t lda[4]; int K[4]; int w1_col[4]; int nseg;
  const void* W1; int64_t ldw1; const void* W2; int64_t ldw2; const void* W3; int64_t ldw3;
  const float* b1; const float* b2; const float* b3; const float* w3row;
  int rows, H, out_dim, mask_mode;
  uint32_t seed, stream1, stream2;
  int step, rows_per_set;
  void* h1; void* h2; int64_t ldh; int store_row0;
  void* out; int64_t ldo; const float* addend; int64_t ld_add; float add_clip;
  float* q;
  int panel_rows;
} recnn_debug_frozen_args;
int recnn_debug_frozen_forward(const recnn_debug_frozen_args* a, int64_t sizeof_args, void* stream);
/* The cycle gather (csrc/gather.hip frame_gather_multi_launch) on caller-supplied device buffers: shapes the engine never produces (small
 * embeddings and frames, ragged row counts, plans that end early, rows whose alignment sends the launch to the generic body).  Batch j
 * (0 .. n_sets - 1) reads plan row (*cursor + cursor_add + j) mod cursor_mod (cursor NULL: row 0 for every j) of plan [.., plan_stride]
 * and lands j * rows rows below the given outputs: bf16 state_h / action_h (row stride ld_h elements; state = frame * emb embeddings +
 * frame ratings), fp32 reward / done, and either next_h (bf16, ld_h) or, with next_h NULL, the next ratings into bf16 tail_n [.., ld_tail].
 * gather_cycle as recnn_engine_tuning::gather_cycle.  sizeof_args = sizeof(recnn_debug_gather_cycle_args) as the caller sees it. */
typedef struct recnn_debug_gather_cycle_args {
  const int32_t* items; const float* ratings; const float* table;
  const int64_t* plan; int64_t plan_stride;
  const int32_t* cursor; int cursor_add, cursor_mod;
  int rows, frame, emb, n_sets;
  void* state_h; void* action_h; void* next_h; int64_t ld_h;
  void* tail_n; int64_t ld_tail;
  float* reward; float* done;
  int gather_cycle;
} recnn_debug_gather_cycle_args;
int recnn_debug_gather_cycle(const recnn_debug_gather_cycle_args* a, int64_t sizeof_args, void* stream);
/* kernel variant of the split-bf16 forward GEMM for the single-problem entry point recnn_gemm_fwd (engines carry their own:
 * recnn_engine_tuning::x3_fwd); -1 = off */
void recnn_debug_x3_fwd(int variant);
/* timing experiments on the wave-specialised split-bf16 forward GEMM (results garbage): bit 0 consumers idle, bit 1 no DMA, bit 2 fragment
 * reads without MFMAs, bit 3 MFMAs without fragment reads, bit 4 no epilogue, bit 5 exit at entry, bit 6 direct epilogue stores, bit 7 plain
 * tile stores, bit 8 no kernel-argument prefetch, bit 9 the unpipelined consumer loop, bit 10 the general epilogue on full tiles (bits 9 and 10
 * leave the results intact: A/B runs of the step, RECNN_X3_WS_PROBE) */
void recnn_debug_x3_ws_probe(int bits);
/* catalogue-wide bf16 forward products of more than 128 rows: 1 (default) = 256 x 128 tiles on the wave-specialised kernel, 0 = round 3's
 * 128 x 128 kernel (A/B runs; the results are bit-identical); 2..5 = other tile / ring shapes (tools/wide_fwd_probe.py) */
void recnn_debug_wide_ws(int on);
/* shader-clock stamps of the plain-bf16 wave-specialised kernel's epilogue: device uint64 [workgroup][8] (loop end, barrier, image written,
 * barrier, stores issued, stores acknowledged); NULL = off */
void recnn_debug_ws_trace(void* device_u64_wg8);
/* shader-clock stamps of dw_adam_kernel's tile workgroups (csrc/dwadam.hip): device uint64 [workgroup][8] (entry, state requested, first stage
 * landed, contraction done, partial tiles in LDS, optimizer arithmetic done, stores issued, stores acknowledged); NULL = off */
void recnn_debug_dwadam_trace(void* device_u64_wg8);
#ifdef __cplusplus
}
#endif
#endif
