/*
 * recnn_hip.h -- C ABI of librecnn_hip.so: the MI355X (gfx950) implementation of the RecNN
 * DDPG/TD3 inner training step.
 *
 * The reference (awarebayes/RecNN) is pure Python and has no FFI; the "drop-in boundary" is
 * its Python API, mirrored by the `recnn_amd` package.  This header is the native boundary
 * underneath: every entry point below replaces one group of reference Python/ATen calls and
 * is what a maintainer of the reference would bind with ctypes.
 *
 * Conventions
 *   - every function returns 0 on success, a negative RECNN_E_* code or a positive hipError_t;
 *     `recnn_last_error()` returns a human-readable message for the calling thread.
 *   - all pointers are DEVICE pointers unless the parameter name starts with `h_`.
 *   - `stream` is a `hipStream_t` passed as void* (NULL = the null stream).  All work is
 *     stream-ordered; nothing synchronises the host unless stated.
 *   - no ownership is transferred: callers allocate every buffer (the Python host uses torch
 *     for device memory); the engine object only records pointers.
 *   - "tc" buffers hold the compute type of the engine: float (RECNN_F32) or bfloat16
 *     (RECNN_BF16, fp32 accumulate, fp32 master weights).
 *
 * Reference lines each group replaces are cited as `recnn/...py:lines` (relative to the
 * upstream repository root).
 */
#ifndef RECNN_HIP_H
#define RECNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): recnn_engine_tuning replaced the recnn_tune_* setters, recnn_gemm_args grew ws / ws_bytes, recnn_shadow_out and the
 * split-bf16 type were added (round 4), recnn_engine_tuning::x3_fwd took a reserved slot. */
#define RECNN_ABI_VERSION 2

enum {
  RECNN_OK = 0,
  RECNN_E_INVALID = -1,   /* bad argument (null pointer, unsupported size, misalignment) */
  RECNN_E_STATE = -2,     /* call order violated (e.g. step before bind) */
  RECNN_E_UNSUPPORTED = -3
};

/* Compute types.  RECNN_BF16X3 ("split bf16"): every value is held as hi = bf16(x), lo = bf16(x - hi) and every product is
 * evaluated as hi*hi + hi*lo + lo*hi on the bf16 matrix cores into an fp32 accumulator: fp32-grade results (the 1e-4 loss-curve
 * parity of the fp32 path) at bf16 MFMA rates.  Tensors of this type are bfloat16 arrays with TWICE the logical columns: logical
 * column c lives at physical column x = 2 (c & ~31) + (c & 31) (hi) and x + 32 (lo); leading dimensions and contraction lengths
 * passed for such tensors are PHYSICAL, output extents / bias / mask indices logical (csrc/x3.h). */
enum { RECNN_F32 = 0, RECNN_BF16 = 1, RECNN_BF16X3 = 2 };

/* dropout mask source for the train-mode networks */
enum {
  RECNN_MASK_NONE = 0,     /* no dropout (eval) */
  RECNN_MASK_HASH = 1,     /* in-kernel counter-based generator keyed by (seed, step, stream, row, col) */
  RECNN_MASK_EXTERNAL = 2  /* uint8 keep-masks supplied by the caller (parity tests) */
};

int recnn_abi_version(void);
const char* recnn_last_error(void);
/* sizeof() of an ABI struct: 0 recnn_gemm_args, 1 recnn_engine_config, 2 recnn_hyper,
 * 3 recnn_engine_sizes, 4 recnn_sampler, 5 recnn_engine_tuning, 6 recnn_shadow_out, 7 recnn_ae_params, 8 recnn_ae_grads (lets a
 * binding verify its declarations);
 * -1 if unknown. */
int64_t recnn_abi_sizeof(int which);
/* =====================================================================================
 * 1. Replay sampler + embedding gather
 *    replaces recnn/data/utils.py:161-187 (prepare_batch_static_size: rolling_window +
 *    concatenate) and recnn/data/utils.py:51-81 (batch_tensor_embeddings: emb[items], view,
 *    cat, done scatter).  Integer/copy work: bit-exact.
 *
 *    Replay store (device resident CSR): items int32[sum L] (dense item ids, time-sorted per
 *    user), ratings float[sum L], user_off int64[n_store_users+1].
 * ===================================================================================== */

/* row_off[0..n_users] = exclusive prefix sum of max(L_u - frame, 0) over the batch's users.
 * row_off[n_users] is the total row count of the batch.
 * `cursor` (device int32, may be NULL): the user list actually read is
 * batch_users + (*cursor) * cursor_stride -- lets a replayed hipGraph walk an epoch permutation. */
int recnn_frame_plan(const int64_t* user_off, const int32_t* batch_users, int n_users, int frame,
                     int32_t* row_off, const int32_t* cursor, int cursor_stride, void* stream);

/* Builds rows [0, rows) of the batch.  Output row r of user u at window t:
 *   state[r]      = [emb(i_t .. i_{t+F-1}) | r_t .. r_{t+F-1}]          (F*E + F floats)
 *   next_state[r] = [emb(i_{t+1} .. i_{t+F}) | r_{t+1} .. r_{t+F}]
 *   action[r]     = emb(i_{t+F}),  reward[r] = r_{t+F},  done[r] = (t == L_u - F - 1)
 * ld_* are row strides in floats (>= row width); rows must be 8-byte aligned, 16-byte
 * aligned rows take the vector path.  `rows` may be smaller than row_off[n_users]
 * (fixed-row batches); rows >= row_off[n_users] are left untouched.
 * row_off may be NULL when n_users <= 1024: the kernel then computes the plan itself (per workgroup, in
 * LDS) and no recnn_frame_plan launch is needed. */
int recnn_frame_gather(const int32_t* items, const float* ratings, const int64_t* user_off,
                       const int32_t* batch_users, const int32_t* row_off, int n_users, int rows,
                       int frame, int emb_dim, const float* table,
                       float* state, int64_t ld_state, float* next_state, int64_t ld_next,
                       float* action, int64_t ld_action, float* reward, float* done,
                       const int32_t* cursor, int cursor_stride, void* stream);

/* Packs a caller-made canonical batch (reference layout, utils.py:265-276 get_base_batch)
 * into the engine's packed rows: xs[r] = [action | state | 0-pad], xn[r] = [<next action
 * slot> | next_state | 0-pad].  Used when the batch did not come from recnn_frame_gather. */
int recnn_pack_batch(const float* state, int64_t ld_state, const float* action, int64_t ld_action,
                     const float* next_state, int64_t ld_next, int rows, int state_dim, int action_dim,
                     float* xs, float* xn, int64_t ld_x, void* stream);

/* =====================================================================================
 * 2. Dense layers (MFMA GEMMs) -- single-problem launchers used by the module-level
 *    forward/backward and by the kernel unit tests.  The fused step (section 4) launches
 *    the same kernels through grouped descriptors.
 *    replaces recnn/nn/models.py:66-73 and :207-213 (addmm/relu/dropout) and their autograd
 *    backward (mm, threshold_backward, dropout mul, bias sum).
 * ===================================================================================== */

typedef struct recnn_gemm_args {
  int dtype;              /* RECNN_F32 | RECNN_BF16: compute type tc */
  int M, N;               /* output rows / cols */
  /* contraction segment 0 and optional segment 1 (accumulated into the same tile) */
  const void* A[2];       /* fwd/dx: [M, lda] (k contiguous).  dw: [Kc, lda] (m = row index) */
  const void* B[2];       /* fwd: [N, ldb] (k contiguous).  dx/dw: [Kc, ldb]                 */
  int64_t lda[2], ldb[2]; /* row pitches in elements of the operand's memory type, 16-byte multiples.  The k-strided operands (B of
                             dx, A and B of dw) are read in whole 64-column tiles on every one of their Kc rows: dx needs
                             ldb >= roundup(N, 64), dw lda >= roundup(M, 64) and ldb >= roundup(N, 64) (RECNN_BF16X3: twice that,
                             the split width of the tiles); the padding columns may hold anything, they only reach outputs that
                             are never stored.  A smaller pitch is refused with RECNN_E_INVALID before any launch. */
  int K[2];               /* contraction length per segment; K[1] = 0 if unused.  fwd/dx: a multiple of
                             one 16-byte chunk of the compute type (4 fp32 / 8 bf16); multiples of 64 (128 for
                             bf16) take the LDS-DMA kernels.  dw: the number of valid rows (any value). */
  int a_f32[2];           /* segment's A operand is float in memory although tc is bf16 */
  int b_f32[2];           /* same for B (dw of layer 1: B = packed fp32 batch rows) */
  /* epilogue */
  void* C; int64_t ldc; int c_f32;
  const float* bias;      /* fwd: [N] or NULL */
  int relu;               /* fwd */
  int mask_mode;          /* fwd: RECNN_MASK_* */
  const uint8_t* mask; int64_t ld_mask;      /* external keep mask [M, ld_mask] */
  uint32_t seed, stream_id; const int32_t* step_ptr;   /* hash mask key (step read from device) */
  const float* addend; int64_t ld_add; float add_clip; /* fwd: C += clamp(addend, +-add_clip) (TD3 noise) */
  int add_row_div;        /* fwd: output row m reads addend row m / add_row_div (0 or 1: row m).  One addend row serves a
                             run of consecutive output rows: the state part of layer 1 shared by the n candidate actions
                             scored per state (BCQ, recnn/nn/update/bcq.py:98-104).  Sits in what used to be padding. */
  const void* yref; int64_t ldy; float dx_scale;       /* dx: C = acc * dx_scale * [yref > 0]; yref NULL = plain.
                                                          fwd: same gate applied after bias/relu (a dX computed with
                                                          pre-transposed weights through the k-contiguous kernels) */
  float* colsum;          /* dx: column sums per 32-row slab, float[ceil(M/32)][N] (bias gradients) */
  int dw_splits;          /* dw: number of K splits; slab s written at C + s*dw_slab_stride */
  int64_t dw_slab_stride;
  int dw_valid_cols;      /* dw: columns >= this are not stored */
  int dw_col_rot;         /* dw: stored column = (col + rot) mod valid_cols */
  void* ws; int64_t ws_bytes;   /* fwd, optional: caller-owned scratch.  A one-segment product with a LONG contraction and few output
                             tiles (K >= 32768, at most 64 tiles of 128 x 128: [256, 2048] x K = 100k, the catalogue-wide
                             contractions of REINFORCE) is then split into up to 8 K slices, one workgroup column each; their fp32
                             partial products (slices * M * N floats must fit) are summed in slice order by a second launch that
                             applies the epilogue.  NULL: one workgroup per tile walks the whole K. */
} recnn_gemm_args;

/* C[M,N] = epi( sum_seg A_seg[M,K] * B_seg[N,K]^T ) */
int recnn_gemm_fwd(const recnn_gemm_args* h_args, void* stream);
/* C[M,N] = epi( A[M,Kc] * B[Kc,N] )            (dX = dZ * W) */
int recnn_gemm_dx(const recnn_gemm_args* h_args, void* stream);
/* C[M,N] = A[Kc,M]^T * B[Kc,N], split over Kc  (dW = dZ^T * X) */
int recnn_gemm_dw(const recnn_gemm_args* h_args, void* stream);

/* fp32 [rows, cols] (row stride ld) <-> split-bf16 rows (RECNN_BF16X3; row stride ldx >= 2 * roundup(cols, 32) bfloat16, padding
 * columns of the split rows are left untouched by pack). */
int recnn_x3_pack(const float* src, int64_t ld, int rows, int cols, void* dst, int64_t ldx, void* stream);
int recnn_x3_unpack(const void* src, int64_t ldx, int rows, int cols, float* dst, int64_t ld, void* stream);

/* Writes the keep-mask the RECNN_MASK_HASH generator produces for (seed, step, stream_id)
 * into out[M, N] (uint8).  Lets tests feed the in-kernel masks to the CPU oracle. */
int recnn_hash_mask_dump(uint32_t seed, int32_t step, uint32_t stream_id, int M, int N,
                         uint8_t* out, void* stream);
/* ... with the step in device memory (step = *step_dev + step_add): a captured graph draws fresh masks on every replay */
int recnn_hash_mask_dump_at(uint32_t seed, const int32_t* step_dev, int step_add, uint32_t stream_id, int M, int N, uint8_t* out,
                            void* stream);

/* =====================================================================================
 * 3. Flat-arena optimizer / soft-update kernels
 *    replaces torch.optim.Adam.step (the optimizer the reference's users inject,
 *    recnn/nn/update/misc.py:44, ddpg.py:93, td3.py:97,101,134), the clip quirk
 *    torch.nn.utils.clip_grad_norm_(params, -1, 1) (ddpg.py:92, td3.py:133) and
 *    recnn/utils/misc.py:1-5 (soft_update).
 * ===================================================================================== */

/* target = target*(1-tau) + net*tau over n floats (operand order as the reference). */
int recnn_soft_update_flat(float* target, const float* net, int64_t n, float tau, void* stream);

/* One Adam step over a flat fp32 arena: p, m, v updated in place from g * grad_scale.
 * step_t is the 1-based step count (bias correction). */
int recnn_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int step_t, float grad_scale, void* stream);

/* ... and, in the same pass, a row-padded copy of the updated [n / cols, cols] parameter in another leading dimension and
 * optionally in bfloat16 (the layout the GEMM kernels read in place of a weight whose rows are not 16-byte aligned, or the bf16
 * operand of the catalogue-wide products): the optimizer has the new value in a register, a separate conversion pass would
 * read 4 bytes per element again.  Padding columns [cols, ld) are not touched.  h_shadow NULL or dst NULL: plain step. */
typedef struct recnn_shadow_out {
  void* dst;       /* float or bfloat16 [n / cols, ld] */
  int cols;        /* n % cols == 0 */
  int64_t ld;      /* >= cols */
  int bf16;        /* 1: dst is bfloat16 (round to nearest even), 0: float */
} recnn_shadow_out;
int recnn_adam_flat_shadow(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                           float weight_decay, int step_t, float grad_scale, const recnn_shadow_out* h_shadow, void* stream);

/* The same step with the 1-based step count taken from device memory: t = *step_dev + step_add.  For captured graphs
 * (recnn_amd.optim.Adam(capturable=True)): the graph advances *step_dev itself, every replay steps with the right count. */
int recnn_adam_flat_at(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                       float weight_decay, const int32_t* step_dev, int step_add, float grad_scale, void* stream);

/* out[0] = sum |g| over n floats (deterministic two-pass reduction; scratch >= 1024 floats). */
int recnn_l1_norm_flat(const float* g, int64_t n, float* scratch, float* out, void* stream);

/* =====================================================================================
 * 4. The fused DDPG / TD3 step engine
 *    replaces recnn/nn/update/ddpg.py:8-104, recnn/nn/update/misc.py:10-55,
 *    recnn/nn/update/td3.py:8-150 for nets = Actor/Critic (recnn/nn/models.py) and the
 *    Adam optimizer, including the soft target update.
 * ===================================================================================== */

typedef struct recnn_engine recnn_engine;

enum { RECNN_ALGO_DDPG = 0, RECNN_ALGO_TD3 = 1 };

/* network slots inside an engine */
enum {
  RECNN_NET_POLICY = 0, RECNN_NET_TARGET_POLICY = 1,
  RECNN_NET_VALUE1 = 2, RECNN_NET_TARGET_VALUE1 = 3,
  RECNN_NET_VALUE2 = 4, RECNN_NET_TARGET_VALUE2 = 5,
  RECNN_NET_COUNT = 6
};

typedef struct recnn_engine_config {
  int algo;            /* RECNN_ALGO_* */
  int dtype;           /* RECNN_F32 | RECNN_BF16 */
  int state_dim;       /* S = F*E + F (1290) */
  int action_dim;      /* A (128) */
  int hidden;          /* H (256) */
  int max_rows;        /* batch capacity */
  int mask_mode;       /* RECNN_MASK_* for the learning nets */
  uint32_t seed;
  int device;          /* hip device ordinal */
} recnn_engine_config;

typedef struct recnn_hyper {
  float gamma, min_value, max_value;   /* DDPG clamps the TD target; TD3 passes -inf/+inf */
  float soft_tau;
  int policy_every;                    /* policy_step / policy_update */
  float noise_std, noise_clip;         /* TD3 */
  /* optimizer slots: [0] = policy optimizer, [1] = value optimizer(s) */
  float lr[2], beta1[2], beta2[2], eps[2], weight_decay[2];
  /* opt_kind: RECNN_OPT_ADAM = torch.optim.Adam arithmetic (L2 weight decay folded into the gradient);
   *           RECNN_OPT_RANGER = RAdam (variance-rectified Adam, decoupled lr*wd*p decay) + Lookahead(la_k, la_alpha):
   *           the shape of the reference's default torch_optimizer.Ranger (recnn/nn/algo.py:84-89, 139-147); needs the
   *           slow-weight arena bound with recnn_engine_bind_slow. */
  int opt_kind[2];
  float la_alpha[2];          /* Lookahead interpolation (Ranger default 0.5) */
  int la_k[2];                /* Lookahead period in optimizer steps (Ranger default 6) */
  float nsma_threshold[2];    /* rectification switch: adaptive step iff N_sma > threshold (Ranger default 5) */
} recnn_hyper;
enum { RECNN_OPT_ADAM = 0, RECNN_OPT_RANGER = 1 };

/* Sizes (in bytes) of the buffers the caller must allocate for an engine. */
typedef struct recnn_engine_sizes {
  int64_t master_floats_actor, master_floats_critic;  /* canonical flat parameter arenas */
  int64_t workspace_bytes;                            /* everything else, one allocation */
  int64_t ld_x;                                       /* packed batch row stride (floats) */
  int64_t x_rows;                                     /* rows to allocate for xs / xn */
} recnn_engine_sizes;

int recnn_engine_query(const recnn_engine_config* h_cfg, recnn_engine_sizes* h_out);

/* `workspace` must be zero-initialised, 256-byte aligned, workspace_bytes long. */
int recnn_engine_create(const recnn_engine_config* h_cfg, void* workspace, recnn_engine** h_out);
void recnn_engine_destroy(recnn_engine* e);

/* Bind the canonical fp32 arenas of one network: params / grads / Adam moments, each a flat
 * array laid out [w1 | b1 | w2 | b2 | w3 | b3] in torch's [out,in] row-major layout.
 * grads/m/v may be NULL for target networks. */
int recnn_engine_bind_net(recnn_engine* e, int net, float* params, float* grads, float* adam_m, float* adam_v);
/* Lookahead slow weights of a learning network (flat fp32 arena, canonical layout, initialised by the caller with the
 * parameters as they were when the optimizer state was created); required for RECNN_OPT_RANGER. */
int recnn_engine_bind_slow(recnn_engine* e, int net, float* slow);
/* One optimizer step over a flat fp32 array, RAdam + Lookahead (RECNN_OPT_RANGER arithmetic; step_t = 1-based step). */
int recnn_ranger_flat(float* p, const float* g, float* m, float* v, float* slow, int64_t n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, float la_alpha, int la_k, float nsma_threshold, int step_t,
                      float grad_scale, void* stream);
int recnn_ranger_flat_shadow(float* p, const float* g, float* m, float* v, float* slow, int64_t n, float lr, float beta1, float beta2,
                             float eps, float weight_decay, float la_alpha, int la_k, float nsma_threshold, int step_t,
                             float grad_scale, const recnn_shadow_out* h_shadow, void* stream);

/* =====================================================================================
 * 3b. Categorical policy head (REINFORCE)
 *    replaces F.softmax + torch.distributions.Categorical(probs).sample() / .log_prob() of
 *    DiscreteActor (recnn/nn/models.py:95-99, :107-111, :116-141), their autograd backward, and the
 *    one-hot action rows of batch_contstate_discaction (recnn/data/utils.py:108-109).
 *    Rows are float[rows, ld] with ld % 4 == 0, 16-byte aligned; columns [n, ld) are padding.
 * ===================================================================================== */
#define RECNN_CAT_SOFTMAX 1 /* x holds logits; overwritten with p = softmax(x) (padding columns become 0) */
#define RECNN_CAT_SAMPLE 2  /* draw actions[row] ~ p / sum p (else actions[row] is read; NULL = no action) */
/* logprob[row] = log(clamp(p[a] / sum p, eps, 1 - eps)) (torch.distributions.Categorical arithmetic);
 * rowstat[row] = {max logit, sum exp, sum p, 1.0 if the clamp was active}.  logprob / rowstat may be NULL.
 * The uniform of row r is a pure function of (seed, step, r); the inverse-CDF walks items in a fixed order. */
int recnn_categorical_rows(float* x, int64_t ld, int rows, int n, int flags, uint32_t seed, int32_t step,
                           int64_t* actions, float* logprob, float* rowstat, void* stream);
#define RECNN_LPB_ACCUMULATE 1 /* dlogits += ... (else =) */
#define RECNN_LPB_BF16 2       /* dlogits is bfloat16[rows, ldd] (operand of the bf16 catalogue GEMMs); else float */
/* dlogits (+)= g[row] * (onehot(a) - p / sum p), zero for rows whose clamp was active (g NULL = zeros);
 * colsum[n] (optional) = column sums of the resulting dlogits (bias gradient), scratch = float[ceil(rows/32) * round4(n)]. */
int recnn_logprob_bwd(const float* p, int64_t ldp, int rows, int n, const int64_t* actions, const float* g,
                      const float* rowstat, void* dlogits, int64_t ldd, int flags, float* colsum, float* scratch,
                      void* stream);
/* dlogits = p * (dprobs - sum_j dprobs_j p_j): backward of p = softmax(logits). */
int recnn_softmax_bwd(const float* p, int64_t ldp, int rows, int n, const float* dprobs, int64_t lddp, float* dlogits,
                      int64_t ldd, void* stream);
/* out[r, :] = onehot(idx[r]) over n columns (columns [n, ld) zeroed). */
int recnn_onehot_rows(const int64_t* idx, int rows, int n, float* out, int64_t ld, void* stream);
/* out[c] = sum over rows of x[r, c], c < n (rows added in order; x rows 16-byte aligned, ld % 4 == 0, padded to 4 floats): the bias
 * gradient of a catalogue-wide Linear from d logits. */
int recnn_colsum_rows(const float* x, int64_t ld, int rows, int n, float* out, void* stream);
/* The softmax of rows whose columns are SHARDED over ranks (the vocabulary-parallel policy head, recnn_amd/parallel.py; replaces the
 * F.softmax of recnn/nn/models.py:95-99 on a shard): three passes over this rank's float[rows, ld] logits x, the all-reduces between
 * them are the caller's.  pass 0: rowval[r] = max_j x[r, j].  pass 1: x = exp(x - rowval[r]) in place (rowval = the max over ALL shards),
 * pa[r] = the row's sum.  pass 2: x /= rowval[r] in place (rowval = the sum over all shards) -> this shard's probabilities, pa[r] =
 * x[r, local[r]] if 0 <= local[r] < n else 0 (local = the row's action minus the shard's first item). */
int recnn_shard_softmax_pass(float* x, int64_t ld, int rows, int n, int pass, float* rowval, const int64_t* local, float* pa, void* stream);
/* dlogits[r, j] = -g[r] p[r, j] (+ g[r] at j = local[r] when the shard owns it): backward of log(clamp(p_a)) through the sharded softmax */
int recnn_shard_logprob_bwd(const float* p, int64_t ldp, int rows, int n, const int64_t* local, const float* g, float* dlogits, int64_t ldd,
                            void* stream);
/* dst[c, r] = src[r, c]: float [rows, cols] (row stride ld) -> float or bfloat16 [cols, ldt] (ldt >= rows; columns [rows, ldt) are
 * not touched).  The transposed copy of the policy head's W2 [n_items, hidden] that puts the catalogue on the contiguous axis
 * for the backward product d logits x W2 (made once per weight version). */
int recnn_transpose_rows(const float* src, int64_t ld, int rows, int cols, void* dst, int64_t ldt, int dst_bf16, void* stream);

/* =====================================================================================
 * 3c. Conditional-VAE latent layer and loss (BCQ)
 *    replaces the ATen chain of bcqGenerator.forward between the encoder and decoder GEMMs
 *    (recnn/nn/models.py:271-277: clamp(log_std, -4, 15), exp, z = mean + std * eps) and the generator loss of
 *    bcq_update (recnn/nn/update/bcq.py:78-81: mse(recon, action) + 0.5 * KL), with their autograd backward.
 *    All operands float[rows, ld]; `ml` holds [mean | raw log_std] side by side (2 * latent columns).
 * ===================================================================================== */
#define RECNN_VAE_LOG_STD_MIN (-4.0f)
#define RECNN_VAE_LOG_STD_MAX (15.0f)
/* std = exp(clamp(ml[:, L:2L])), z = ml[:, :L] + std * eps */
int recnn_vae_latent_fwd(const float* ml, int64_t ld_ml, const float* eps, int64_t ld_eps, int rows, int latent, float* z,
                         int64_t ldz, float* std_out, int64_t ld_std, void* stream);
/* dml[:, :L] = dz + dmean;  dml[:, L:] = (dz * eps + dstd) * std * [min <= raw <= max];  dz / dmean / dstd may be NULL */
int recnn_vae_latent_bwd(const float* ml, int64_t ld_ml, const float* eps, int64_t ld_eps, const float* std_in, int64_t ld_std,
                         const float* dz, int64_t ld_dz, const float* dmean, int64_t ld_dmean, const float* dstd,
                         int64_t ld_dstd, int rows, int latent, float* dml, int64_t ld_dml, void* stream);
/* out3 = { mean((recon - action)^2), -0.5 * mean(1 + log(std^2) - mean^2 - std^2), out3[0] + kl_weight * out3[1] };
 * scratch: 512 floats.  Fixed summation order (bit-reproducible). */
int recnn_vae_loss_fwd(const float* recon, int64_t ld_recon, const float* action, int64_t ld_action, const float* mean,
                       int64_t ld_mean, const float* std_in, int64_t ld_std, int rows, int action_dim, int latent,
                       float kl_weight, float* out3, float* scratch, void* stream);
/* gradients of sum_i gout[i] * out3[i] w.r.t. recon, mean and std (gout: float[3] on the device) */
int recnn_vae_loss_bwd(const float* recon, int64_t ld_recon, const float* action, int64_t ld_action, const float* mean,
                       int64_t ld_mean, const float* std_in, int64_t ld_std, int rows, int action_dim, int latent,
                       const float* gout, float kl_weight, float* d_recon, int64_t ld_drecon, float* d_mean, int64_t ld_dmean,
                       float* d_std, int64_t ld_dstd, void* stream);

/* =====================================================================================
 * 3d. Replay-store builder: ratings rows -> CSR ordered by (user, time)   
 *    replaces recnn/data/dataset_functions.py:84-126 (prepare_dataset: rating transform and movieId -> dense id map as
 *    per-row Python lambdas, sort_values(by="timestamp"), a Python callback per user group).  All pointers are device
 *    memory except host_counts.  Rows with equal (user, timestamp) keep their input order (pandas' unstable sort leaves
 *    that order host-dependent; everything else is bit-identical to the reference).
 * ===================================================================================== */
int recnn_csr_workspace_bytes(int64_t n_rows, int64_t* bytes);
/* in : user_ids / item_keys / timestamps int64[n_rows], ratings double[n_rows] (raw, e.g. 0.5..5);
 *      map_keys (ascending) / map_vals int64[n_map]: item key -> dense id, NULL = keep the keys;
 * out: items_out int64[n_rows] (-1 where the key is not in the map), ratings_out double[n_rows] = 2 (r - 2.5),
 *      users_out int64[<= n_rows] ascending user ids, user_off_out int64[users + 1], order_out int64[n_rows] or NULL
 *      (output row i is input row order_out[i]), mapped_rows_out int64[n_rows] or NULL (dense id of INPUT row i);
 *      host_counts[3] (HOST memory) = { users, rows with an unmapped item key, key bits sorted }.
 * Synchronises the stream twice (key ranges decide the number of radix passes; the user count is returned). */
int recnn_csr_build(const int64_t* user_ids, const int64_t* item_keys, const double* ratings, const int64_t* timestamps,
                    int64_t n_rows, const int64_t* map_keys, const int64_t* map_vals, int n_map, int64_t* items_out,
                    double* ratings_out, int64_t* users_out, int64_t* user_off_out, int64_t* order_out, int64_t* mapped_rows_out,
                    int64_t* host_counts, void* workspace, int64_t workspace_bytes, void* stream);

/* Packed batch buffers (float[x_rows, ld_x]) + reward/done (float[max_rows]). */
int recnn_engine_bind_batch(recnn_engine* e, float* xs, float* xn, float* reward, float* done);

/* Device-resident replay sampler: when bound, every step first builds its batch on the GPU
 * (recnn_frame_plan + recnn_frame_gather straight into the packed rows) from
 * perm[cursor*users_per_batch .. +users_per_batch), cut to the step's `rows`, and then advances
 * the cursor (mod n_batches).  This makes the whole hot path -- sampler, gather, networks,
 * optimizer, soft update -- one launch sequence / one hipGraph.
 *   replaces the DataLoader + collate of recnn/data/env.py:225-252. */
/* Plan table of a whole epoch permutation: plan[b * rows + r] = (CSR offset of the window start of row r of batch b) << 1 |
 * (1 if that window is its user's last: done), -1 where batch b has fewer than r + 1 rows.  One workgroup per batch.
 *   replaces, ahead of time, the per-step users -> offsets -> prefix scan -> row search of recnn_frame_gather. */
int recnn_frame_plan_rows(const int64_t* user_off, const int32_t* perm, int users_per_batch, int n_batches, int frame,
                          int rows, int64_t* plan, void* stream);
/* Plan table of a DENSE epoch: the windows of the users seq[0 .. n_seq) (store slots) concatenated in that order -- every L - F
 * windows of every user, as the reference's collate builds them (recnn/data/utils.py:161-187) -- and cut into batches of `rows`
 * rows: plan[g] for global row g, same encoding as recnn_frame_plan_rows, done = 1 at each user's last window wherever it falls.
 * skip0: windows of seq[0] already consumed (the previous epoch's leftover is carried into this one).  Slots past the epoch's last
 * whole batch repeat its first batches.  row_off: scratch int32[n_seq + 1] (prefix sums of the window counts; the total must fit
 * 31 bits).  Bind the table with recnn_sampler.plan / plan_rows = rows; the sampler's perm / users_per_batch are then unused. */
int recnn_frame_plan_dense(const int64_t* user_off, const int32_t* seq, int n_seq, int skip0, int frame, int rows, int32_t* row_off,
                           int64_t n_rows, int64_t* plan, void* stream);
typedef struct recnn_sampler {
  const int32_t* items; const float* ratings; const int64_t* user_off;  /* CSR replay store */
  const int32_t* perm;        /* epoch permutation of store user slots, int32[n_batches*users_per_batch] */
  int users_per_batch;
  int n_batches;
  int frame, emb_dim;
  const float* table;         /* float[n_items, emb_dim] */
  int32_t* row_off;           /* scratch int32[users_per_batch + 1] */
  int32_t* cursor;            /* device int32: next batch index */
  const int64_t* plan;        /* optional: int64[n_batches * plan_rows] made by recnn_frame_plan_rows for THIS perm (NULL = the
                                 gather plans its rows itself); must be re-made whenever perm changes */
  int plan_rows;              /* rows per batch the plan covers (steps of at most this many rows use it) */
} recnn_sampler;
int recnn_engine_bind_sampler(recnn_engine* e, const recnn_sampler* h_sampler);  /* NULL unbinds */
/* Who draws from a bound sampler: graph replays (recnn_engine_graph_run), the data-parallel phase graphs and
 * recnn_engine_profile always do.  Eager calls (recnn_engine_step / value_grads / finish) run on the BOUND batch --
 * `algo.update(env.test_batch(), learn=False)` between two replays evaluates the batch it was given and leaves the
 * sampler cursor alone -- unless on = 1 is set here (eager data-parallel phases). */
int recnn_engine_sampler_eager(recnn_engine* e, int on);

/* External inputs for parity runs: masks uint8[n_masks][max_rows][hidden] (6 DDPG, 8 TD3, in the
 * reference's consumption order), noise float[max_rows][action_dim] (TD3, unclipped). */
int recnn_engine_bind_external(recnn_engine* e, const uint8_t* masks, const float* noise);

int recnn_engine_set_hyper(recnn_engine* e, const recnn_hyper* h_hyper);
/* switch the dropout-mask source of the learning nets (RECNN_MASK_*); invalidates built graphs. */
int recnn_engine_set_mask_mode(recnn_engine* e, int mask_mode);

/* Re-derive the compute-layout shadow of a network from its canonical arena (call after the
 * canonical parameters were changed by anything other than the engine). */
int recnn_engine_refresh(recnn_engine* e, int net, void* stream);

/* Set optimizer step counters (1-based count of steps already taken). */
int recnn_engine_set_counters(recnn_engine* e, int policy_t, int value1_t, int value2_t, int step);

/* One full update on the bound batch (rows valid rows).
 *   learn      : 0 = losses only (reference learn=False), 1 = update
 *   step       : the caller's step counter (policy step iff step % policy_every == 0)
 *   fused_optim: 1 = run Adam + soft update inside; 0 = stop after gradients (phases below)
 * Losses are written to the device loss buffer; fetch with recnn_engine_read_losses. */
int recnn_engine_step(recnn_engine* e, int rows, int learn, int step, void* stream);

/* Phase API (external optimizers, data-parallel all-reduce between phases):
 *   value_grads  : [sampler gather if bound,] TD target, critic forward/backward -> value grads in the bound
 *                  grad arenas
 *   value_apply  : Adam on the critic(s) (+ fused soft update when `soft`), shadows refreshed
 *   policy_grads : actor forward, critic forward, policy loss; with `backward` also the actor
 *                  gradient (reduced into the bound grad arena, NOT yet clipped)
 *   policy_apply : L1 clip quirk + Adam on the actor (+ soft update when `soft`)
 * grad_scale multiplies gradients inside the apply phases (1/world_size after an all-reduce). */
int recnn_engine_value_grads(recnn_engine* e, int rows, int learn, void* stream);
int recnn_engine_value_apply(recnn_engine* e, int soft, float grad_scale, void* stream);
int recnn_engine_policy_grads(recnn_engine* e, int rows, int backward, void* stream);
int recnn_engine_policy_apply(recnn_engine* e, int soft, float grad_scale, void* stream);
/* The input gradient of a DDPG / TD3 step: d loss / d state, what the value losses' and the policy loss's backward() send into `state`
 * when it is attached to a graph (an LSTM state encoder in front: recnn/nn/update/ddpg.py:58-104, td3.py:95-132, misc.py:25-44).  One
 * launch (csrc/state_grad.hip) writes out[rows, state_dim] (fp32, row stride ld_out >= state_dim; columns past state_dim are not touched):
 *   which 0 (value loss [1]): gV1 = dz_c1[0] * W1c1[:, state columns]
 *                          valid after recnn_engine_value_grads(.., learn = 1) and BEFORE a value optimizer is applied or a critic
 *                          refreshed: W1c1 is the critic the value backward used.
 *   which 1 (policy loss): gP = dz_e1 * W1c1[:, state columns] + dz_p1 * W1a   (the raw gradient: neither clipped nor sign-flipped)
 *                          valid after recnn_engine_policy_grads(.., backward = 1) and before either network is applied or refreshed:
 *                          W1c1 is the UPDATED critic (TD3: critic 1) the policy loss went through.
 *   which 2 (TD3, value loss 2): gV2 = dz_c1[1] * W1c2[:, state columns]        valid as which 0, critic 2 as the value backward used it
 *   which 3 (TD3, value losses 1 + 2): gV1 + gV2 in ONE launch, two contraction segments, critic 1 first -- what a single backward
 *                          through the encoder needs (the encoder's backward is linear in the gradient it is handed).  Valid as which 0.
 * The dz are the layer-1 pre-activation gradients of the phase (dropout's mask and scale folded in), the weights the compute-type
 * values the phase multiplied with (bf16 engines: the master rounded to nearest even); fp32 engines multiply on the exact-fp32 MFMA,
 * bf16 engines on the bf16 MFMA with fp32 accumulation; where the fused bf16 forward left unit backward tensors, each critic's per-row
 * seed multiplies its segment's fp32 accumulator.  The contraction runs in a fixed order inside one workgroup per output tile
 * (no atomics, no split-K): two calls give the same bits.  Anything else in between (a step, a graph replay, another phase, an apply
 * or refresh of EITHER critic for which 0 / 2 / 3) makes the call return RECNN_E_STATE.  RECNN_F32 / RECNN_BF16 engines only: a
 * RECNN_BF16X3 engine, and which 2 / 3 on a DDPG engine, get RECNN_E_UNSUPPORTED.  Not part of recnn_engine_step or of any graph.
 * recnn_engine_buffer names "critic2_dz2" / "critic2_dz1" are critic 2's backward tensors (TD3 engines). */
int recnn_engine_state_grads(recnn_engine* e, int rows, int which /* 0 value loss, 1 policy loss; TD3: 2 value loss 2, 3 both */,
                             float* out, int64_t ld_out, void* stream);
/* the same pieces for callers that run their own optimizer: */
int recnn_engine_clip_policy_grads(recnn_engine* e, float grad_scale, void* stream);  /* g *= coef */
int recnn_engine_soft_update(recnn_engine* e, int net, int target_net, float tau, void* stream);
/* closes a step driven through the phase API: reduces the loss partials into the loss buffer
 * and advances the device step / optimizer counters. */
int recnn_engine_finish(recnn_engine* e, int rows, int value_stepped, int policy_stepped, void* stream);

/* Capture `recnn_engine_step` for a fixed row count into hipGraphs -- one ordinary step, one policy step, and a family
 * of RUN graphs (k ordinary steps; a policy step + k ordinary steps, k < policy_every; whole policy cycles up to 64
 * steps, see tuning.graph_run; with tuning.run_align also whole cycles that start right AFTER a policy step) -- and replay `n_steps` consecutive steps starting at `first_step`: ANY
 * (first_step, n_steps) is covered with at most n_steps / policy_every + 2 graph launches (policy_every <= 17; longer
 * cycles compose power-of-two stretches).  Inside a run graph the device counters are ticked once at its end, the sampler + gather of step t+1 and the policy-loss forward of step t ride on
 * other launches (tuning.pregather, tuning.defer_policy_fwd), and every step's losses land in the history ring
 * (recnn_engine_read_counters). */
int recnn_engine_graph_build(recnn_engine* e, int rows, void* stream);
int recnn_engine_graph_run(recnn_engine* e, int first_step, int n_steps, void* stream);
/* Optional: a run graph made to order for requests of exactly n_steps (2..64) steps whose first step number is congruent
 * to first_step modulo policy_every; recnn_engine_graph_run then serves such requests with ONE graph launch instead of
 * composing them from the family.  Up to 4 are kept (oldest replaced); dropped with the other graphs. */
int recnn_engine_graph_prepare(recnn_engine* e, int first_step, int n_steps, void* stream);

/* How recnn_engine_graph_run composes a request from the run-graph family (host arithmetic only: no GPU, no engine).
 * recnn_run_family_init describes the family recnn_engine_graph_build captures for (policy_every, tuning.graph_run, tuning.run_align);
 * recnn_run_plan cuts [first_step, first_step + n_steps) into pieces (kind, length) of that family, in order:
 *   align = 0  [ordinary stretch up to the next policy step] [multi-cycle graphs] [policy step + the rest of its cycle] ... [policy step + tail]
 *   align = 1  when the largest aligned graph fits behind the next policy step: [ordinary stretch] [that policy step alone]
 *              [aligned multi-cycle graphs] [aligned single cycles], then the pieces of align = 0 for what is left
 * Returns the number of pieces; at most `cap` of them are written (a caller with a short buffer plans again from where they end: the
 * composition of a remainder depends on nothing before it).  < 0: bad arguments. */
#define RECNN_RUN_MAX 64
enum {
  RECNN_RUN_STEP = 0,           /* one ordinary step */
  RECNN_RUN_POLICY_STEP = 1,    /* one policy step */
  RECNN_RUN_ORDINARY = 2,       /* len ordinary steps (len >= 2) */
  RECNN_RUN_POLICY_HEAD = 3,    /* a policy step + len - 1 ordinary steps */
  RECNN_RUN_MULTI = 4,          /* whole cycles, starts ON a policy step */
  RECNN_RUN_ALIGNED_MULTI = 5,  /* whole cycles, starts right AFTER a policy step and ends on one */
  RECNN_RUN_ALIGNED_CYCLE = 6   /* one such cycle */
};
typedef struct recnn_run_family {
  unsigned char has_o[RECNN_RUN_MAX + 1];   /* has_o[k]: the graph of k ordinary steps exists (k >= 2) */
  unsigned char has_p[RECNN_RUN_MAX + 1];   /* has_p[k]: the graph of a policy step + k ordinary steps exists (k >= 1) */
  int multi_len;                            /* steps of the multi-cycle graph (0: none) */
  int aligned_multi_len;                    /* steps of the aligned multi-cycle graph (0: none) */
  int aligned_cycle_len;                    /* policy_every when the aligned single cycle exists, else 0 */
} recnn_run_family;
int recnn_run_family_init(int policy_every, int graph_run, int align, recnn_run_family* h_out);
int recnn_run_plan(int policy_every, const recnn_run_family* h_family, int first_step, int n_steps, int align, int* h_kinds, int* h_lens,
                   int cap);

/* Runs n_steps eager steps with a hipEvent pair around every kernel launch and returns, per
 * launch slot, the average device time in milliseconds (h_ms[i]), its name (h_names[i], static
 * strings) and, for GEMM slots, the algorithmic FLOPs of one launch (h_flops[i], 0 otherwise).
 * Kernels whose relaunch does not change state (everything but Adam and the loss/counter kernel) are issued
 * 8 times back to back inside their event pair and the time divided by 8, which amortises the event overhead.
 * *h_n is in: capacity, out: slots used.  Policy and non-policy steps have different slot
 * lists; only steps with (step % policy_every == 0) == policy_steps are run and averaged.  policy_steps = 2 profiles CYCLE
 * MODE (what run graphs of >= tuning.cycle_min_len steps replay): the gather of one policy cycle's batches, the frozen
 * networks on all of them, then one ordinary step of the cycle on the split forward. */
int recnn_engine_profile(recnn_engine* e, int rows, int policy_steps, int n_steps, void* stream,
                         float* h_ms, double* h_flops, const char** h_names, int* h_n);

/* Data-parallel replay: the step cut into four hipGraphs around the two gradient all-reduces the caller issues
 * (torch.distributed / RCCL) on the same stream:
 *   0: batch, all forwards, critic backward, slab reduction   -> caller all-reduces the critic gradient arena(s)
 *   1: non-policy step: critic Adam, policy loss, finish
 *   2: policy step: critic Adam (+soft update), policy loss, actor backward -> caller all-reduces the actor arena
 *   3: policy step: L1 clip + actor Adam (+soft update), finish
 *   4: (overlap_actor = 1 only) the actor forward alone; graph 0 then omits it, and the caller launches graph 4
 *      right after starting the critic all-reduce so that the collective's latency hides behind it
 *   5: graph 1 of step t followed by graph 0 of step t+1 in ONE graph (one graph launch per step instead of two)
 *   6: graph 3 of step t followed by graph 0 of step t+1
 * `which` = kind + 8 * set, set = batch buffer set holding step t's batch: recnn_engine_dp_sets() returns 2 when
 * consecutive steps alternate between two sets (then the sampler + gather of step t+1 rides on step t's critic
 * optimizer launch inside graph 5), else 1 (always pass set 0).  A run of n steps:
 *   launch 0;  per step: all-reduce critic arena(s); ordinary step: launch 5 (1 on the last step);
 *   policy step: launch 2, all-reduce actor arena, launch 6 (3 on the last step);  set ^= 1 after 5 / 6 if 2 sets.
 * grad_scale (1/world_size) is baked into the graphs. */
int recnn_engine_dp_graph_build(recnn_engine* e, int rows, float grad_scale, int overlap_actor, void* stream);
int recnn_engine_dp_graph_launch(recnn_engine* e, int which, void* stream);
int recnn_engine_dp_sets(recnn_engine* e);

/* ---- device-side gradient exchange (csrc/comm.hip; SURVEY.md 8(b) `dp_allreduce_flat`, 5 "two-shot P2P all-reduce").
 * New functionality (the reference is single-process); what it preserves is the gradient of the GLOBAL batch mean that
 * recnn/nn/update/ddpg.py:74-87 / td3.py:95-123 compute on one concatenated batch: sum over ranks x 1 / world.
 *
 * Every rank (one process per GPU, up to 8 = one node) creates a communicator able to carry `max_floats` floats, exports its
 * peer buffer as an opaque handle of recnn_comm_handle_bytes() bytes (a hipIpcMemHandle_t), exchanges the handles out of band
 * (torch.distributed all_gather_object, MPI, a file: anything) and connects with the `world` handles in rank order.  After
 * that recnn_dp_allreduce_flat sums data[0 .. n) over the ranks IN PLACE with ONE kernel launch on `stream`: reduce-scatter by
 * direct peer reads, all-gather by direct peer writes over xGMI, ranks added in the order 0 .. world-1 (every rank gets the
 * same bits; world 2 == any other order).  The launch can be captured: epochs are advanced on the device.  Every rank must
 * issue the same sequence of collectives.  A peer that does not arrive within 4 s sets an error word instead of hanging the
 * GPU: recnn_comm_status then returns RECNN_E_STATE and names the rank(s).
 *
 * recnn_engine_set_comm attaches a connected communicator to an engine: from then on every step -- eager or inside the run
 * graphs (rebuild them) -- all-reduces the critics' flat gradient arenas each step and the actor's on policy steps in-stream
 * and the optimizers step on grad * grad_scale (1 / world); the L1 clip quirk acts on the reduced actor gradient.  A
 * data-parallel run is then recnn_engine_graph_run on every rank: no host code between the phases of a step.  NULL detaches. */
typedef struct recnn_comm recnn_comm;
int recnn_comm_create(int world, int rank, int64_t max_floats, recnn_comm** out);
int64_t recnn_comm_handle_bytes(void);
int recnn_comm_export(recnn_comm* c, void* handle_out, int64_t bytes);
int recnn_comm_connect(recnn_comm* c, const void* handles, int64_t bytes_each);
int recnn_dp_allreduce_flat(recnn_comm* c, float* data, int64_t n, void* stream);
int recnn_comm_status(recnn_comm* c, int32_t* timed_out_ranks, int32_t* epoch);
/* bound (ms, default 4000) of every peer wait of the collectives launched or captured afterwards; clear a reported time-out */
int recnn_comm_set_timeout_ms(recnn_comm* c, int ms);
int recnn_comm_clear_status(recnn_comm* c);
void recnn_comm_destroy(recnn_comm* c);
int recnn_engine_set_comm(recnn_engine* e, recnn_comm* comm, float grad_scale);
/* Settings of ONE communicator (round 6: no process-wide communicator state is left): recnn_comm_create_ex takes the memory kind of the
 * peer buffers -- 0 fine-grained (default, = recnn_comm_create), 1 uncached, 2 ordinary device memory; recnn_comm_set_workgroups the
 * workgroups per collective launch made or captured afterwards (default 128; ranks that share ONE GPU in tests need every rank's
 * collective resident at once: 32). */
int recnn_comm_create_ex(int world, int rank, int64_t max_floats, int memory_kind, recnn_comm** out);
int recnn_comm_set_workgroups(recnn_comm* c, int n);

/* ---- per-engine tuning.  Every field selects among schedules / kernel tilings that produce the SAME numbers (the GPU suite runs
 * under several of them); nothing here is process-wide: two engines of one process can run different schedules.
 * recnn_engine_tuning_init fills the defaults, recnn_engine_set_tuning copies a (clamped) tuning into an engine and drops its
 * graphs.  In-launch hand-offs of the fused forward wait with a bound: a wait that runs out sets a device error word and
 * recnn_engine_read_losses / read_counters then return RECNN_E_STATE (debug hooks that provoke this: csrc/recnn_hip_debug.h). */
typedef struct recnn_engine_tuning {
  int fused_mlp;            /* 1: bf16 engines with hidden <= 256 run the networks of a step as ONE fused row-panel launch (csrc/mlps.hip)
                               when a launch has >= 3 of them, 2: always, 0: layer-by-layer GEMM launches */
  int chain_target_critic;  /* 1: the target critics run inside the fused launch (producer workgroups + flag hand-off), 0: after it */
  int bwd_panel;            /* where the critic head + first backward GEMM run: 2 inside the fused forward launch (unit backward
                               tensors, per-row seed applied by the dW launch), 1 one row-panel launch (bwd.hip), 0 head + dX launches */
  int policy_chain;         /* 1: policy steps run the gradient chain from the policy loss into the actor as ONE row-panel launch */
  int split_fwd;            /* 0: fused forward everywhere; 1: run graphs of >= cycle_min_len steps run in cycle mode (a policy cycle's
                               batches gathered at once, frozen networks applied to all of them: mlpf.hip; per-step launches = split
                               forward of the learning critics: l1gemm.hip + mlpt.hip); 2: split forward and cycle mode everywhere */
  int cycle_min_len;        /* default 20 (round 5; 30 before) */
  int cycle_min_seg;        /* cycle mode: segments shorter than this step through the fused forward (default 4 since round 6: the per-step launches of cycle mode got cheaper; 5 in round 5, 3 before) */
  int frozen_fused;         /* cycle mode: 1 each frozen network as one launch of 128-row panels, 0 tiled layer 1 + later layers */
  int frozen_gemm;          /* ... whose later layers run as tiled GEMMs (1) or row-panel tails (0) */
  int graph_run;            /* steps per run graph: -1 as many whole policy cycles as fit 64 steps, 0 single-step graphs only */
  int pregather;            /* 1: inside a run graph the sampler + gather of step t+1 ride on step t's critic optimizer launch */
  int defer_policy_fwd;     /* 1: ... and the policy-loss forward of step t on step t+1's forward launch(es) */
  int sampler_f32_rows;     /* 1: an engine that samples its own batches also fills the bound fp32 packed rows (inspection) */
  int dw_splits;            /* batch splits (gradient slabs) of the layer-1 dW GEMM, 1..8 */
  int comm_fused;           /* data parallel: 1 the critics' gradient exchange runs inside their optimizer launch, 0 as its own launches */
  int l1_big;               /* tile of the cycle-batched layer-1 GEMMs: 1 = 128 x 128 (default), 2 = 128 x 64 */
  int gemm_variant;         /* register-staged GEMM tile: -1 per launch, 0 = 64 x 64, 1 = 32 x 64 with a 2x longer k stage */
  int gemm_v0_threshold;    /* ... the per-launch choice takes 64 x 64 from this many tiles on (512) */
  int gemm_dma;             /* 1: forward GEMMs on compute-type operands use the LDS-DMA ring kernel */
  int gemm_dma_depth;       /* 1: 5-stage ring for launches of <= 320 tiles */
  int gemm_dma_waves;       /* 8 | 4 waves per workgroup of the LDS-DMA forward kernel */
  int gemm_waves;           /* 8 | 4 waves per workgroup of the register-staged dX kernel */
  int dw_dma;               /* bf16 dW: 0 register-staged loader, 1..7 LDS-DMA + transpose reads with (rows per stage, ring slots) =
                               (128,2) (64,2) (64,3) (64,4) (32,2) (32,4) (32,3); default 2 */
  int x3_tail;              /* split-bf16 engines (hidden 256, action 128): 1 layers 2 + 3 of a step's networks as row-panel launches
                               that keep h2 on chip (csrc/x3tail.hip), 0 grouped GEMM launches per layer */
  int x3_fwd;               /* split-bf16 forward GEMM kernel: 2 (default) wave-specialised -- loader waves + consumer waves (csrc/gemm.hip
                               x3_fwd_ws_kernel), 11 only its 64 x 128-tile launches, 0 every wave loads and multiplies (round 4) */
  int dw_fuse;              /* 1 (default): on the single-GPU bf16 step whose backward tensors come from the split forward (cycle mode), the critics'
                               weight-gradient GEMMs carry the optimizer in their epilogue -- ONE launch, no gradient slabs (csrc/dwadam.hip);
                               0: dW launch + optimizer launch.  Bit-identical results */
  int tail_half;            /* 1 (default): the learning critic's tail launch (csrc/mlpt.hip) runs 16-row panels -- twice the workgroups, half the
                               per-workgroup epilogue work (its phases are bound by the CU's vector issue); 0: 32-row panels.  Bit-identical */
  int l1_ws;                /* 1: the per-step layer-1 GEMM (csrc/l1gemm.hip, 64 x 64 tiles) runs with 4 loader + 8 consumer waves; 0: all 16 waves
                               load and multiply.  Bit-identical */
  int frozen_half;          /* 1: a cycle segment's frozen-network launch (csrc/mlpf.hip) runs 64-row workgroups instead of 128-row ones while
                               it then still fits one round of workgroups (short segments: a request that starts or ends inside a policy
                               cycle); 0: always 128 rows.  Bit-identical */
  int frozen_window;        /* 1 (default): bf16 cycle mode with frozen_fused does not materialise next_state rows for the frozen networks -- the
                               cycle gather writes state rows, action rows and the ten next ratings only, and the target networks' layer 1 reads s'
                               as shifted windows of those (csrc/mlpf.hip: up to four contraction segments); the packed next rows of the cycle are
                               then not allocated.  0: the gather also writes a next_state row per transition.  Bit-identical */
  int run_align;            /* 1 (default): recnn_engine_graph_build also captures run graphs that START right after a policy step and END on
                               one (whole cycles: every cycle segment ends on its policy step, none is a lone step), and
                               recnn_engine_graph_run composes long requests from them (recnn_run_plan); 0: the family that starts on a
                               policy step only.  Bit-identical */
  int frozen_acts_policy_only;  /* 1 (default): the cycle-batched actor launch (csrc/mlpf.hip) stores its hidden activations only for the
                               batch that reads them -- the policy step's, a segment's last -- and for none in a segment without a policy
                               step; 0: for every batch of the segment.  Bit-identical */
  int gather_cycle;         /* 1 (default): the cycle gather without next rows (frozen_window) runs 32 consecutive plan rows per workgroup,
                               loads every embedding line of a user's run once and writes 16 bytes per store (csrc/gather.hip) where the
                               rows' alignment allows; 0: the generic gather body, four rows per workgroup.  Took the last reserved slot:
                               the struct's size is unchanged.  Bit-identical */
  int policy_fused;         /* the policy step's own launches on the single-GPU plain-bf16 engine (policy_chain, no communicator), a bit set:
                               bit 0: layer 1 of the policy-loss critic runs on the per-step tiled kernel (csrc/l1gemm.hip) wherever the
                               step's learning critics do; bit 1: the actor's three weight gradients are summed over their batch slices on
                               chip and written to the flat gradient arena by ONE launch without slabs (csrc/dwadam.hip dw_grad_kernel),
                               the clip quirk's |g| sums then come from that arena -- where the tile plan fits (batches of 1024, 2048, ...
                               rows), else the dW launch + slab reduction stay.  0: the generic launches.  Default 3.  Bit-identical.
                               (Grows the struct by one int: recnn_abi_sizeof(5).) */
} recnn_engine_tuning;
void recnn_engine_tuning_init(recnn_engine_tuning* h_t);
int recnn_engine_set_tuning(recnn_engine* e, const recnn_engine_tuning* h_t);
int recnn_engine_get_tuning(recnn_engine* e, recnn_engine_tuning* h_t);

/* Device counters {steps finalized, actor optimizer steps, critic 1 steps, critic 2 steps} (synchronises the stream).
 * The debug view "loss_ring" ([1024][4] fp32: value1, value2 / policy, policy per recnn_engine_read_losses' layout)
 * holds the losses of the last 1024 steps at index (step counter value of that step) mod 1024 -- including every
 * step replayed inside a run graph, whose per-step partial sums are kept and reduced at the end of the run. */
int recnn_engine_read_counters(recnn_engine* e, int32_t* h_out4, void* stream);
/* Host copy of the last step's losses (synchronises `stream`):
 * DDPG: {value, policy}; TD3: {value1, value2, policy}.  h_out has room for 4 floats. */
int recnn_engine_read_losses(recnn_engine* e, float* h_out, void* stream);

/* 1 if the last step left UNIT backward tensors in the debug views "critic1_dz2" / "critic1_dz1" (dz / d: the per-row
 * loss seed "delta1" is applied by the consumers inside the dW launch), 0 if they hold dz itself. */
int recnn_engine_unit_backward(recnn_engine* e);
/* Debug / test access to intermediate device buffers by name
 * ("next_action", "expected", "q1", "gen_action", ...).  Returns NULL if unknown.  Cycle mode's arrays (MSET_MAX x max_rows rows each):
 * "cycle_gen_action", "cycle_actor_h1" / "cycle_actor_h2" (the actor's hidden activations: with tuning.frozen_acts_policy_only only the
 * policy step's batch of a batched segment is written), "cycle_target_q1" / "2", "cycle_next_action0" / "1" (the target actor's output of window mode, per copy) and
 * "cycle_xn0" / "1" (the packed next rows whose action slot holds it otherwise: the engine's own allocation, NULL while it has none);
 * what the cycle gather writes, per copy: "cycle_xs0" / "1" (packed [action | state] rows), "cycle_tail_n0" / "1" (window mode's next
 * ratings; NULL where the dims do not allow that mode), "cycle_reward0" / "1", "cycle_done0" / "1".  "actor_l1part": the clip quirk's
 * |g| sum per optimizer workgroup of the actor as the last policy step left them (fp32, one row per workgroup).
 * "<net>_w1_shadow" / "<net>_w2_shadow" / (actors) "<net>_w3_shadow" with <net> one of policy, target_policy, value1, target_value1,
 * value2, target_value2: the compute-type copy of that weight which the optimizer pass rewrites -- [out, ld] rows in the engine's compute
 * type, zero padded; a critic's W1 columns rotated to [action | state]; split-bf16 rows in their physical layout (h_cols is the logical
 * column count, h_ld the physical pitch). */
const void* recnn_engine_buffer(recnn_engine* e, const char* name, int64_t* h_rows, int64_t* h_cols,
                                int64_t* h_ld, int* h_is_f32);

/* =====================================================================================
 * 5. Batched exact top-K action scoring ("next" row)
 *    replaces the retrieval step after the actor: faiss IndexFlatL2 / IndexFlatIP / IP on normalised rows
 *    (examples/streamlit_demo.py:190-204) and MilvusConnection.search (recnn/data/db_con.py:45-56).  The per-item
 *    scipy loop `rank` (streamlit_demo.py:207-231) and its metrics are section 7.
 *    metric: 0 = IP (q.t, descending), 1 = L2 (|q-t|^2, ascending), 2 = COS (q.t/|t|, descending).
 *    Ties are broken towards the smaller item id.  emb_dim must be 128, k <= 64.
 * ===================================================================================== */
enum { RECNN_METRIC_IP = 0, RECNN_METRIC_L2 = 1, RECNN_METRIC_COS = 2 };
/* per-item auxiliary array float[n_items] needed by L2 (|t|^2) and COS (1/|t|); build once per table */
int recnn_topk_item_aux(const float* table, int n_items, int emb_dim, int metric, float* aux, void* stream);
int recnn_topk_workspace_bytes(int n_queries, int k, int64_t* h_bytes);
/* out_dist float[n_queries, k], out_ids int64[n_queries, k] (faiss / Milvus result layout) */
int recnn_topk_search(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                      int metric, const float* item_aux, int k, float* out_dist, int64_t* out_ids, void* workspace,
                      void* stream);

/* =====================================================================================
 * 6. Anomaly detector: the reference's debugging autoencoder (recnn/nn/models.py:7-38)
 *    x[128] -> Linear(128,64) ReLU BN(64) -> Linear(64,32) ReLU BN(32) -> Linear(32,64) ReLU BN(64)
 *           -> Linear(64,128) ReLU;  rec_error(x) = sum((x - ae(x))^2, 1).
 *    Widths are fixed.  fp32 throughout (exact-f32 MFMA), every reduction in a fixed order: two identical calls give
 *    bit-identical outputs, gradients and running statistics.
 *
 *    Layouts: x is [rows, 128] with row stride ldx (unit column stride; any ldx >= 128); out is [rows, 128] (ldo), err is
 *    float[rows].  Weights are nn.Linear's [out, in] row-major arrays, contiguous and 16-byte aligned.  BatchNorm i (i = 0, 1, 2)
 *    normalises the output of Linear i.  act (train-style forward / backward) holds the activations backward needs,
 *    recnn_ae_act_floats(rows) floats, 16-byte aligned.  workspace: recnn_ae_workspace_bytes(rows) bytes, 16-byte aligned.
 *    Errors: RECNN_E_INVALID for a null pointer, a misaligned operand, rows < 0, or rows < 2 in train mode.
 * ===================================================================================== */
typedef struct recnn_ae_params {
  const float* w[4];              /* [64,128] [32,64] [64,32] [128,64] */
  const float* b[4];              /* [64] [32] [64] [128] */
  const float* gamma[3];          /* BatchNorm weight [64] [32] [64] */
  const float* beta[3];           /* BatchNorm bias */
  float* running_mean[3];         /* read in eval mode; updated in train mode (momentum, unbiased variance) */
  float* running_var[3];
  int64_t* num_batches_tracked[3];  /* incremented once per train-mode forward */
  float eps[3];
  float momentum[3];
} recnn_ae_params;

typedef struct recnn_ae_grads {  /* outputs of recnn_ae_backward, shaped like the parameters */
  float* w[4];
  float* b[4];
  float* gamma[3];
  float* beta[3];
} recnn_ae_grads;

int recnn_ae_act_floats(int rows, int64_t* h_floats);
int recnn_ae_workspace_bytes(int rows, int64_t* h_bytes);
/* Eval mode (running statistics), ONE launch: exactly one of out (forward) and err (rec_error; the 128-wide output is never
 * stored) is non-NULL.  rows == 0 launches nothing. */
int recnn_ae_eval(const recnn_ae_params* h_p, const float* x, int64_t ldx, int rows, float* out, int64_t ldo, float* err,
                  void* stream);
/* Segmented forward, four launches (one per BatchNorm seam).  train = 1: batch statistics (biased variance), running statistics
 * and num_batches_tracked updated; train = 0: running statistics.  Writes a0..a2 (post-ReLU) into act always and the normalised
 * h0..h2 plus the statistics used only when keep != 0 (what recnn_ae_backward reads).  Exactly one of out / err non-NULL. */
int recnn_ae_forward(const recnn_ae_params* h_p, int train, const float* x, int64_t ldx, int rows, float* out, int64_t ldo,
                     float* err, float* act, int keep, void* workspace, void* stream);
/* Gradients of sum(dout * out) for the forward that filled act (keep = 1) with the same train flag: every field of h_g is
 * written; dx (may be NULL) gets d/dx.  dout: [rows, 128] (ld_dout), out: that forward's output (ldo). */
int recnn_ae_backward(const recnn_ae_params* h_p, const recnn_ae_grads* h_g, int train, const float* x, int64_t ldx, int rows,
                      const float* out, int64_t ldo, const float* dout, int64_t ld_dout, const float* act, float* dx,
                      int64_t lddx, void* workspace, void* stream);

/* =====================================================================================
 * 7. Ranking under scipy's distance metrics: the reference's per-item scipy loop `rank`
 *    (examples/streamlit_demo.py:207-231; examples/[Results]/1. Ranking.ipynb).  Each metric is
 *    scipy.spatial.distance.cdist's (scipy 1.15), computed in fp32 with a fixed summation order over the 128 elements
 *    (DESIGN.md 11): a pair's distance does not depend on the batch, the tile or the call, and recnn_dist_topk reports
 *    bit for bit what recnn_dist_matrix stores.  minkowski needs p >= 1 (p = inf allowed); p = 1, 2, inf give the bits of
 *    cityblock, euclidean, chebyshev.  NaN distances (cosine against a zero row, correlation against a constant row,
 *    braycurtis(0, 0)) are reported as NaN and rank after every number; ties go to the smaller item id.
 *    Limits: emb_dim == 128, k <= 64 and k <= n_items, ld_q % 4 == 0, queries / table / aux / workspace 16-byte aligned.
 *    Errors: RECNN_E_INVALID, before any HIP call, for an unknown metric, p < 1 or NaN for minkowski, a null pointer, a
 *    misaligned operand, a missing aux (cosine / correlation) and the limits above.
 * ===================================================================================== */
enum {
  RECNN_DIST_SQEUCLIDEAN = 0, RECNN_DIST_EUCLIDEAN = 1, RECNN_DIST_CITYBLOCK = 2, RECNN_DIST_CHEBYSHEV = 3,
  RECNN_DIST_MINKOWSKI = 4, RECNN_DIST_CANBERRA = 5, RECNN_DIST_BRAYCURTIS = 6, RECNN_DIST_COSINE = 7,
  RECNN_DIST_CORRELATION = 8
};
/* floats of the per-table aux array: n_items * 128 for cosine / correlation (normalised, centred rows), else 0 */
int recnn_dist_item_aux_floats(int n_items, int emb_dim, int metric, int64_t* h_floats);
/* builds the aux rows of `table` (cosine / correlation only); once per table */
int recnn_dist_item_aux(const float* table, int n_items, int emb_dim, int metric, float* aux, void* stream);
/* workspace of one call: k = 0 for recnn_dist_matrix, else the k of recnn_dist_topk */
int recnn_dist_workspace_bytes(int n_queries, int n_items, int metric, int k, int64_t* h_bytes);
/* out float[n_queries, n_items] with row stride ld_out >= n_items */
int recnn_dist_matrix(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                      int metric, double p, const float* item_aux, float* out, int64_t ld_out, void* workspace, void* stream);
/* out_dist float[n_queries, k] ascending, out_ids int64[n_queries, k] (table row ids) */
int recnn_dist_topk(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                    int metric, double p, const float* item_aux, int k, float* out_dist, int64_t* out_ids, void* workspace,
                    void* stream);

/* =====================================================================================
 * 8. Dueling DQN of the embeddings notebook (examples/0. Embeddings Generation/1. (proof of concept) DQN.ipynb): the catalogue-wide
 *    head Q[b, n] = V_b + A[b, n] - mean(A), A = h W^T + c (W [n_items, 128]), its learn step without the [B, N] matrix, the
 *    deterministic scatter-sums of the embedding / head gradients (csrc/dqn.hip), the clip_grad_norm_ coefficient on the device and
 *    torch's RAdam (csrc/optim.hip).
 *    Algebra, layouts and error bounds: DESIGN.md 12.  Every float sum has a fixed order (no float atomics): repeated calls are
 *    bit-identical.  Hidden width 128.  h rows and W rows 16-byte aligned.  Ids outside their range are dropped (scatter) or give NaN
 *    (row dot); nothing is read or written out of bounds.
 * ===================================================================================== */
/* the catalogue GEMM.  Exactly one of out / rowmax is non-NULL:
 *   out    float[B, ldo]: out[b, n] = h_b . W_n + c_n + V_b - *mu                (DuelDQN.forward)
 *   rowmax int32[B]    : the order-preserving integer image of max_n (h_b . W_n + c_n); [B, N] is never stored (target network).
 * W is fp32 (w_bf16 = 0, exact-f32 MFMA) or bfloat16 (w_bf16 = 1: h rounded to bf16 on load, fp32 accumulation). */
int recnn_dqn_head(const float* h, int64_t ldh, int B, const void* W, int64_t ldw, int w_bf16, const float* c, int N, const float* V,
                   const float* mu, float* out, int64_t ldo, int32_t* rowmax, void* stream);
/* out[b] = x_b . w[idx_b] + bias[idx_b] over 128 columns (idx NULL: row 0 of w, bias[0]; bias may be NULL) */
int recnn_dqn_row_dot(const float* x, int64_t ldx, int rows, const float* w, int64_t ldw, const int64_t* idx, int n_w, const float* bias,
                      float* out, void* stream);
/* out[col] = scale * sum over rows of x[row, col] (cols <= 256), rows in fixed chunks added in chunk order */
int recnn_dqn_colsum_workspace_floats(int rows, int cols, int64_t* h_floats);
int recnn_dqn_colsum(const float* x, int64_t ldx, int rows, int cols, float scale, float* out, float* workspace, void* stream);
/* *mu = (sh . sw) / (B N) + *sc / N: mean(A) from the column sums sh = sum_b h_b, sw = sum_n W_n and sc = sum_n c_n */
int recnn_dqn_mean(const float* sh, const float* sw, const float* sc, int B, int N, float* mu, void* stream);
/* TD step of the notebook's loss: q = V + adv - mu, y = reward + gamma (Vt + max' - mu') (1 - done), g = 2 (q - y) / B.
 * adv = h_b . W[a_b] + c[a_b] (recnn_dqn_row_dot), rowmax from recnn_dqn_head.  q / g may be NULL.
 * stats float[8]: loss = mean (q - y)^2, G = sum g, G / (B N), G / N, mu, mu'. */
int recnn_dqn_td(const float* V, const float* adv, const float* Vt, const int32_t* rowmax, const float* reward, const float* done,
                 float gamma, int B, int N, const float* sh, const float* sw, const float* sc, const float* sht, const float* swt,
                 const float* sct, float* q, float* g, float* stats, void* stream);
/* dh [B, 256] = [ [ha > 0] (g_b W[a_b] - stats[2] sw) | [hv > 0] g_b wv ] for h2 = [ha | hv] (ldh >= 256) */
int recnn_dqn_dh(const float* h2, int64_t ldh, int B, const float* W, int64_t ldw, int N, const int64_t* act, const float* sw,
                 const float* wv, const float* g, const float* stats, float* dh, void* stream);
/* out[d, 0:128] = sum over contributions j with id d, in j order, of scale[j / per_row] * src[(j / per_row) ld_src + (j % per_row) 128 ...]
 * (scale NULL: 1), minus coef[0] * rank1 when rank1 is given; out_s[d] (may be NULL) = the sum of the weights minus coef[1] (coef NULL: 0).
 * Contribution j reads its id at ids[(j / per_row) ld_ids + j % per_row].  Every one of the n_dest rows is written (dense gradient). */
int recnn_dqn_scatter_workspace_bytes(int64_t contributions, int n_dest, int64_t* h_bytes);
int recnn_dqn_scatter_sum(const float* src, int64_t ld_src, int rows, int per_row, const int64_t* ids, int64_t ld_ids, const float* scale,
                          int n_dest, float* out, float* out_s, const float* rank1, const float* coef, void* workspace, void* stream);
/* clip_grad_norm_(max_norm, norm_type = 1) on a flat gradient whose L1 norm is *norm (device): g *= min(max_norm / (*norm + 1e-6), 1) */
int recnn_dqn_clip(float* g, int64_t n, const float* norm, float max_norm, void* stream);
/* One torch.optim.RAdam step over a flat fp32 array (foreach arithmetic; L2 weight decay; step_t 1-based).  clip_norm (device, may be
 * NULL): the gradient is first scaled by the recnn_dqn_clip coefficient and the scaled gradient written back to g. */
int recnn_radam_flat(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                     int step_t, const float* clip_norm, float max_norm, void* stream);

/* =====================================================================================
 * 9. Statistics of a top-K result (csrc/divstats.hip): what the reference's diversity / distances notebooks compute on the host
 *    from the ids and distances of a search (np.unique(ids, return_counts=True), D.mean(axis=1).mean(), D.std(axis=1).mean()).
 *    dist float[n_queries, k] and ids int64[n_queries, k], both contiguous and 16-byte aligned, are what recnn_topk_search /
 *    recnn_dist_topk write.  x = (double)dist, or sqrt((double)dist) when take_sqrt.  Per row, in float64, two passes, both sums in
 *    index order: mean = (sum x) / k, std = sqrt(sum (x - mean)^2 / k) (ddof = 0); NaN entries propagate as in numpy.  Integer atomics
 *    for the counts, no float atomics: totals are summed in a fixed order that depends on n_queries alone, equal calls give equal bits.
 *    Limits: 0 < k <= 64.  Errors: RECNN_E_INVALID, before any HIP call, for a null pointer, k out of range, n_items <= 0,
 *    n_queries < 0 or a misaligned operand.  n_queries == 0 launches nothing.  DESIGN.md 13.
 * ===================================================================================== */
int recnn_topk_stats_workspace_bytes(int n_queries, int k, int64_t* h_bytes);
/* counts int32[n_items]: ACCUMULATED into (the caller zeroes it once); ids outside [0, n_items) are not counted.
 * row_mean, row_std double[n_queries]: written.
 * totals double[4]: ACCUMULATED into: sum of row_mean, sum of row_std, rows seen, ids outside [0, n_items). */
int recnn_topk_stats(const float* dist, const int64_t* ids, int n_queries, int k, int n_items, int take_sqrt, int32_t* counts,
                     double* row_mean, double* row_std, double* totals, void* workspace, void* stream);

/* =====================================================================================
 * 10. Dynamic-length user batches (csrc/seq.hip; the LSTM state encoder: csrc/lstm.hip over csrc/seq_chain.h): the padded gathers behind recnn.data.utils.padder /
 *    prepare_batch_dynamic_size, an LSTM state encoder over whole user histories, and the replay-buffer collect of SeqEnv.
 *    The replay store is the CSR triple of section 2 (items int32, ratings float, user_off int64) and `slots` int32[n_users] names
 *    the batch's users.  table float[n_items, emb_dim], 16-byte aligned rows.  An item id outside [0, n_items) gives NaN in whatever
 *    is derived from it; nothing is read or written out of bounds.  No atomics: equal calls give equal bits.
 *    Errors: RECNN_E_INVALID with a message, before any launch, for a null pointer, an unsupported shape or a misaligned operand.
 *    DESIGN.md 14.
 * ===================================================================================== */
/* out_items int64[n_users, l_max], out_ratings float[n_users, l_max], out_emb float[n_users, l_max, emb_dim] (may be NULL).
 * Positions past a user's history hold id 0, rating 0 and therefore table row 0 (the reference's quirk).  emb_dim % 4 == 0. */
int recnn_seq_gather(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                     int l_max, const float* table, int n_items, int emb_dim, int64_t* out_items, float* out_ratings,
                     float* out_emb, void* stream);
/* the same rows from an already padded id tensor: out_emb float[n, emb_dim] = table[idx[i]] */
int recnn_seq_gather_idx(const int64_t* idx, int64_t n, const float* table, int n_items, int emb_dim, float* out_emb,
                         void* stream);
/* torch.nn.LSTM(emb_dim + 1, hidden), one layer, one direction, gate order i, f, g, o, weights read in place:
 * w_ih float[4 hidden, emb_dim + 1], w_hh float[4 hidden, hidden], b_ih / b_hh float[4 hidden].  The input of step t of user u is
 * [table[items_u[t]] | ratings_u[t]]; steps t0 .. t0 + T - 1 run from the state (h0, c0) float[n_users, hidden] (both NULL: zeros).
 * h_out float[n_users, T, hidden]; h_T, c_T float[n_users, hidden] (may alias h0, c0).  Every history must hold t0 + T elements
 * (positions past an end are clamped to the last element).  fp32 state and accumulation (exact-f32 MFMA); a user's result does not
 * depend on the other users of the batch or on how its steps are cut into calls.  emb_dim: multiple of 8 up to 128; hidden:
 * multiple of 16 up to 256.  variant 0: input projection fused into the step; variant 1: projected per chunk of steps into
 * `workspace` (recnn_lstm_workspace_bytes; 16-byte aligned) by a grid-wide launch -- the same bits. */
int recnn_lstm_workspace_bytes(int n_users, int T, int hidden, int variant, int64_t* h_bytes);
int recnn_lstm_encode(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                      int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_ih,
                      const float* w_hh, const float* b_ih, const float* b_hh, const float* h0, const float* c0, float* h_out,
                      float* h_T, float* c_T, int variant, void* workspace, void* stream);
/* Rows k n_users + u (k < n_steps) of the four replay-buffer tensors, each pointer already offset to the first row to write, from
 * h float[n_users, T, hidden] of an encode call with t0 = 0 and the kept steps steps int32[n_steps] (device; 1 <= step < T):
 * state = h[u, step - 1], next_state = h[u, step], action = table[items_u[step]], reward = ratings_u[step].
 * state / next_state rows hidden floats, action rows emb_dim floats, reward one float; all contiguous.  hidden, emb_dim % 4 == 0. */
int recnn_seq_collect(const float* h, int n_users, int T, int hidden, const int32_t* steps, int n_steps, const int32_t* items,
                      const float* ratings, const int64_t* user_off, const int32_t* slots, const float* table, int n_items,
                      int emb_dim, float* state, float* action, float* reward, float* next_state, void* stream);

/* Training the encoder (csrc/lstm.hip over csrc/seq_chain.h and csrc/seq_bwd.h; the collect backward: csrc/seq.hip).  recnn_lstm_encode_train is recnn_lstm_encode -- the same h_out, h_T, c_T bit for bit,
 * either variant -- that also records, per (user, step, hidden unit), the gate activations i, f, g, o and the cell state c_t into
 * `saved` (saved_bytes of recnn_lstm_train_workspace_bytes: 5 * 16 ceil(n_users / 16) * T * hidden floats; 16-byte aligned; its
 * layout is private to the library).  `workspace` is that of recnn_lstm_workspace_bytes, as for recnn_lstm_encode.
 *
 * recnn_lstm_backward is backward through time over the steps of ONE such call (same store, slots, t0, T, table, w_hh, h0 / c0;
 * `saved` and `h_out` as that call wrote them).  Upstream gradients, each may be NULL (zeros): g_h float[n_users, T, hidden],
 * g_hT / g_cT float[n_users, hidden].  Outputs, each may be NULL (not wanted): d_w_ih float[4 hidden, emb_dim + 1], d_w_hh
 * float[4 hidden, hidden], d_b float[4 hidden] (the gradient of b_ih and of b_hh), d_h0 / d_c0 float[n_users, hidden]; they are
 * written, not added to.  With d_w_ih, d_w_hh and d_b all NULL the weight-gradient launches are skipped.  `workspace`: bwd_bytes of
 * recnn_lstm_train_workspace_bytes, 16-byte aligned.  Fixed summation orders, no atomics: equal calls give equal bits.  T >= 1. */
int recnn_lstm_train_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int variant, int64_t* saved_bytes,
                                     int64_t* bwd_bytes);
int recnn_lstm_encode_train(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                            int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_ih,
                            const float* w_hh, const float* b_ih, const float* b_hh, const float* h0, const float* c0, float* h_out,
                            float* h_T, float* c_T, int variant, void* workspace, void* saved, void* stream);
int recnn_lstm_backward(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                        int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_hh,
                        const void* saved, const float* h_out, const float* h0, const float* c0, const float* g_h,
                        const float* g_hT, const float* g_cT, float* d_w_ih, float* d_w_hh, float* d_b, float* d_h0, float* d_c0,
                        void* workspace, void* stream);
/* The gradient of the embedding table through the encoder (csrc/seq_bwd.h, csrc/seq_grad.h).  recnn_lstm_backward_table is
 * recnn_lstm_backward -- the same arguments, and the same bits in d_w_ih, d_w_hh, d_b, d_h0, d_c0 -- that also writes
 * d_table float[n_items, emb_dim] (required, 16-byte aligned; EVERY row is written, items the call's positions do not hold get exact
 * zeros): d_table[item] = sum of dX[u, t, 0:emb_dim] over the positions (u, t) with items_u[t0 + t] == item, where
 * dX[u, t, n] = sum_m da[u, t, m] w_ih[m, n] and da is the gradient of the gate pre-activations.  w_ih float[4 hidden, emb_dim + 1] is
 * read in place (its rating column is not used).  The weight-gradient outputs may all be NULL: d_table alone is computed then.
 * `table_workspace`: recnn_lstm_table_grad_workspace_bytes (host-only; a packed transpose of w_ih[:, 0:emb_dim], dX of the whole call
 * -- n_users * T * emb_dim floats, the one place where [n_users, T, emb_dim] is materialised --, the inverted index of the call's
 * n_users * T positions by item id and the partial sums of its pieces), 16-byte aligned; n_users * T < 2^31.  dX runs on the exact-f32
 * MFMA in a fixed contraction order; the sum per item runs over its positions in ascending u * T + t, cut into fixed pieces added in
 * order: no float atomics (integer atomics build the index), equal calls give equal bits.  Item ids outside [0, n_items) contribute to
 * no row. */
int recnn_lstm_table_grad_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int n_items, int64_t* bytes);
int recnn_lstm_backward_table(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                              int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_ih,
                              const float* w_hh, const void* saved, const float* h_out, const float* h0, const float* c0,
                              const float* g_h, const float* g_hT, const float* g_cT, float* d_w_ih, float* d_w_hh, float* d_b,
                              float* d_h0, float* d_c0, float* d_table, void* workspace, void* table_workspace, void* stream);
/* Backward of recnn_seq_collect with respect to h: g_h float[n_users, T, hidden] (every element written) from the gradients of the
 * state and next_state rows (each float[n_steps * n_users, hidden] or NULL: zeros): g_h[u, t] = g_next_state[k n_users + u] where
 * steps[k] == t, plus g_state[k' n_users + u] where steps[k'] == t + 1.  steps int32[n_steps] (device) must be strictly increasing
 * (the caller checks). */
int recnn_seq_collect_bwd(const float* g_state, const float* g_next_state, int n_users, int T, int hidden, const int32_t* steps,
                          int n_steps, float* g_h, void* stream);

/* A GRU as the state encoder (csrc/gru.hip over the same csrc/seq_chain.h and csrc/seq_bwd.h): the recnn_lstm_* family for torch.nn.GRU(emb_dim + 1, hidden), one layer,
 * one direction, gate order r, z, n, weights read in place: w_ih float[3 hidden, emb_dim + 1], w_hh float[3 hidden, hidden],
 * b_ih / b_hh float[3 hidden];
 *   r = sigmoid(W_ir x + b_ir + W_hr h + b_hr), z = sigmoid(W_iz x + b_iz + W_hz h + b_hz), n = tanh(W_in x + b_in + r (W_hn h + b_hn)),
 *   h' = (1 - z) n + z h.
 * The store, the input of a step, t0 / T, the shape limits (emb_dim a multiple of 8 up to 128, hidden a multiple of 16 up to 256), the
 * two variants (bit-identical), the alignment rules and the independence of a user's result from the batch and from how its steps are
 * cut into calls are those of recnn_lstm_encode.  There is no cell state: steps run from h0 float[n_users, hidden] (NULL: zeros);
 * h_out float[n_users, T, hidden]; h_T float[n_users, hidden] (may alias h0).  With tiles = ceil(n_users / 16) and
 * Tc = min(T, 32):
 *   recnn_gru_workspace_bytes        variant 1: tiles * Tc * (hidden / 16) * 3 * 64 * 16 (r, z and the input half of n per step of a
 *                                    chunk, accumulator layout); variant 0: 0.
 *   recnn_gru_train_workspace_bytes  saved_bytes = tiles * T * (hidden / 16) * 4 * 64 * 16 (r, z, n and hn = W_hn h + b_hn per user,
 *                                    step and hidden unit; layout private to the library);
 *                                    bwd_bytes = 12 hidden^2 (W_hh^T) + round16(4 n_users hidden) (the dh hand-over)
 *                                                + tiles * 16 * Tc * 4 hidden * 4 (one chunk of [da_r | da_z | da_n | da_hn]).
 *   recnn_gru_table_grad_workspace_bytes  round256(12 emb_dim hidden) (packed W_ih^T) + 2 round256(4 n_users T emb_dim) (dX and the
 *                                    piece partials) + the inverted index: round256(4 n_items) + round256(4 (n_items + 1))
 *                                    + 3 round256(4 n_users T).  n_users * T < 2^31.
 * All three are host-only.
 *
 * recnn_gru_encode_train is recnn_gru_encode -- the same h_out and h_T bit for bit, either variant -- that also writes `saved`.
 * recnn_gru_backward is backward through time over the steps of ONE such call (same store, slots, t0, T, table, w_hh, h0; `saved` and
 * `h_out` as that call wrote them).  Upstream gradients, each may be NULL (zeros): g_h float[n_users, T, hidden], g_hT
 * float[n_users, hidden].  Outputs, each may be NULL (not wanted), written, not added to: d_w_ih float[3 hidden, emb_dim + 1], d_w_hh
 * float[3 hidden, hidden], d_b_ih and d_b_hh float[3 hidden] -- two tensors: they agree in their first 2 hidden entries and differ in
 * the last hidden, because b_hn sits inside the reset product --, d_h0 float[n_users, hidden].  With all four weight outputs NULL the
 * weight-gradient launches are skipped.  `workspace`: bwd_bytes, 16-byte aligned.  T >= 1.
 * recnn_gru_backward_table is recnn_gru_backward -- the same bits in the outputs they share -- that also writes d_table
 * float[n_items, emb_dim] (required; EVERY row, exact zeros for items the call's positions do not hold) as
 * recnn_lstm_backward_table does, with da = [da_r | da_z | da_n]; w_ih is read in place (its rating column is not used).
 * Fixed summation orders, no float atomics: equal calls give equal bits.  Errors: RECNN_E_INVALID with a message, before any launch. */
int recnn_gru_workspace_bytes(int n_users, int T, int hidden, int variant, int64_t* bytes);
int recnn_gru_encode(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users, int t0,
                     int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_ih, const float* w_hh,
                     const float* b_ih, const float* b_hh, const float* h0, float* h_out, float* h_T, int variant, void* workspace,
                     void* stream);
int recnn_gru_train_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int variant, int64_t* saved_bytes,
                                    int64_t* bwd_bytes);
int recnn_gru_encode_train(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                           int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_ih,
                           const float* w_hh, const float* b_ih, const float* b_hh, const float* h0, float* h_out, float* h_T,
                           int variant, void* workspace, void* saved, void* stream);
int recnn_gru_backward(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users, int t0,
                       int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_hh, const void* saved,
                       const float* h_out, const float* h0, const float* g_h, const float* g_hT, float* d_w_ih, float* d_w_hh,
                       float* d_b_ih, float* d_b_hh, float* d_h0, void* workspace, void* stream);
int recnn_gru_table_grad_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int n_items, int64_t* bytes);
int recnn_gru_backward_table(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                             int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_ih,
                             const float* w_hh, const void* saved, const float* h_out, const float* h0, const float* g_h,
                             const float* g_hT, float* d_w_ih, float* d_w_hh, float* d_b_ih, float* d_b_hh, float* d_h0,
                             float* d_table, void* workspace, void* table_workspace, void* stream);

/* Causal self-attention as the state encoder (csrc/attn.hip): one multi-head attention layer over the steps of a call.
 * Per user, for the call's steps t = 0 .. T - 1 (history positions t0 .. t0 + T - 1; positions before t0 are not seen):
 *   x_t = [table[item_t] | rating_t],   [q_t | k_t | v_t] = w_in x_t + b_in      w_in float[3 hidden, emb_dim + 1], b_in float[3 hidden]
 *   s_a(t, j) = (q_t^a . k_j^a) / sqrt(d) - m_a (t - j)   for j in [max(0, t - window + 1), t], head a of n_heads, d = hidden / n_heads
 *   p_a(t, .) = softmax_j s_a(t, .),   o_t^a = sum_j p_a(t, j) v_j^a,   h_t = w_o o_t + b_o      w_o float[hidden, hidden], b_o float[hidden]
 * with m_a = 2^(-8 (a + 1) / n_heads) when `alibi` is non-zero, else 0; `window` = 0 means no window (j in [0, t]).  The store, slots,
 * t0, T, table and the limits on emb_dim and hidden are those of recnn_lstm_encode; besides, hidden % n_heads == 0, d in {16, 32, 64},
 * n_users <= 65535, n_users * T < 2^31, T >= 1.  Everything is fp32 on v_mfma_f32_16x16x4_f32 in fixed summation orders and without float
 * atomics: equal calls give equal bits; a user's h does not depend on the other users of the batch or on its place among them; h[:, 0:a]
 * of a call with T = a + b equals the call with T = a bit for bit.  Key tiles of 64 lie on multiples of 64 from the call's step 0; tiles
 * above the diagonal or left of the window are not visited, masked keys inside a visited tile are a select on the score (probability
 * exactly 0), so h_t does not depend on the bits of a masked position -- as long as they are finite:
 * an item id outside [0, n_items) at position j of a user makes that user's q_j, k_j, v_j NaN (nothing is read out of bounds); h_t is NaN
 * for every t >= j that has j in its window, and ALSO for the user's other steps t that visit the key tile holding j (t in the same block
 * of 64 steps, or j left of t's window inside a visited tile): 0 * NaN in P V is NaN.  Other users are bitwise unaffected.
 * With round256(x) = x rounded up to 256:
 *   recnn_attn_workspace_bytes        round256(12 n_users T hidden) (qkv [n_users, T, 3 hidden]) + round256(4 n_users T hidden) (o)
 *                                     + round256(8 n_users n_heads T) (the log-sum-exp per user, head and step, held as its two
 *                                     parts: the row maximum m and l = sum exp(s - m))
 *   recnn_attn_train_workspace_bytes  saved_bytes = the same three tensors, kept for the backward;
 *                                     bwd_bytes = round256(4 hidden^2) (w_o^T) + round256(4 n_users T hidden) (dO)
 *                                                 + round256(4 n_users n_heads T) (delta) + round256(12 n_users T hidden) (dqkv)
 *                                                 + round256(4 nsplit max(3 hidden (emb_dim + 2), hidden (hidden + 1))) (the parts of the
 *                                                 weight gradients: the call's n_users T samples are summed in
 *                                                 nsplit = clamp(ceil(n_users T / 1024), 1, 64) segments, the parts added in order)
 *   recnn_attn_table_grad_workspace_bytes  as recnn_gru_table_grad_workspace_bytes (3 hidden rows of w_in).
 * All three are host-only.
 *
 * recnn_attn_encode writes h_out float[n_users, T, hidden]; `workspace` as above, 16-byte aligned like table, w_o and h_out.
 * recnn_attn_encode_train is the same call -- the same h_out bit for bit -- that keeps qkv, o and the log-sum-exp in `saved`.
 * recnn_attn_backward is the backward of ONE such call (same store, slots, t0, T, table, n_heads, window, alibi, w_o; `saved` as that
 * call wrote it) for the upstream gradient g_h float[n_users, T, hidden] (required, 16-byte aligned).  Outputs, each may be NULL (not
 * wanted: its launch is skipped), written, not added to: d_w_in float[3 hidden, emb_dim + 1], d_b_in float[3 hidden], d_w_o
 * float[hidden, hidden], d_b_o float[hidden].  P is recomputed from q, k and the log-sum-exp; delta = sum_j p dP comes from a first
 * sweep over the queries, dK and dV from a launch that owns keys, dQ from one that owns queries: no float atomics.
 * recnn_attn_backward_table is recnn_attn_backward -- the same bits in the outputs they share -- that also writes d_table
 * float[n_items, emb_dim] (required; EVERY row, exact zeros for items the call's positions do not hold) as recnn_lstm_backward_table
 * does, with da = [dq | dk | dv]; w_in is read in place (its rating column is not used).  Item ids outside the table contribute to no row.
 * Errors: RECNN_E_INVALID with a message, before any launch. */
int recnn_attn_workspace_bytes(int n_users, int T, int hidden, int n_heads, int64_t* bytes);
int recnn_attn_encode(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users, int t0,
                      int T, const float* table, int n_items, int emb_dim, int hidden, int n_heads, int window, int alibi,
                      const float* w_in, const float* b_in, const float* w_o, const float* b_o, float* h_out, void* workspace,
                      void* stream);
int recnn_attn_train_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int n_heads, int64_t* saved_bytes,
                                     int64_t* bwd_bytes);
int recnn_attn_encode_train(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                            int t0, int T, const float* table, int n_items, int emb_dim, int hidden, int n_heads, int window, int alibi,
                            const float* w_in, const float* b_in, const float* w_o, const float* b_o, float* h_out, void* saved,
                            void* stream);
int recnn_attn_backward(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users, int t0,
                        int T, const float* table, int n_items, int emb_dim, int hidden, int n_heads, int window, int alibi,
                        const float* w_o, const void* saved, const float* g_h, float* d_w_in, float* d_b_in, float* d_w_o,
                        float* d_b_o, void* workspace, void* stream);
int recnn_attn_table_grad_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int n_items, int64_t* bytes);
int recnn_attn_backward_table(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                              int t0, int T, const float* table, int n_items, int emb_dim, int hidden, int n_heads, int window,
                              int alibi, const float* w_in, const float* w_o, const void* saved, const float* g_h, float* d_w_in,
                              float* d_b_in, float* d_w_o, float* d_b_o, float* d_table, void* workspace, void* table_workspace,
                              void* stream);

/* The transformer state encoder (csrc/block.hip): a gathered embedding, pre-LN transformer blocks on a dense residual
 * stream x float[n_users, T, hidden], and a final LayerNorm.  The calls are cut along the autograd nodes; between them only
 * [n_users, T, hidden] tensors cross.  Per user, for the call's steps t = 0 .. T - 1 (nothing is carried between calls):
 *   embedding   x_t = w_e [table[item_t] | rating_t] + b_e                       w_e float[hidden, emb_dim + 1], b_e float[hidden]
 *   block       u = x + w_o Attn(LN1(x)) + b_o                                   Attn: the layer above on a dense input, w_in
 *                                                                                float[3 hidden, hidden] (q | k | v), b_in float[3 hidden]
 *               y = u + w2 act(w1 LN2(u) + b1) + b2                              w1 float[ffn, hidden], w2 float[hidden, ffn]
 *   LayerNorm   LN(z) = (z - mean(z)) / sqrt(var_biased(z) + eps) gamma + beta   (g1, be1), (g2, be2): float[hidden] each
 * act: 0 = relu, 1 = gelu in its exact erf form.  n_heads, window, alibi, the limits on hidden, head width, emb_dim, n_users and T are
 * those of recnn_attn_encode; besides, ffn is a multiple of 16 in 16 .. 1024 and eps > 0.  Everything is fp32 on
 * v_mfma_f32_16x16x4_f32 in fixed summation orders, no float atomics.  A row's mean and variance are summed by four lanes (lane q:
 * columns q, q + 4, .. upwards; then (s0 + s1) + (s2 + s3)), the mean first, then the centred squares.  Every product chain starts
 * from its bias and walks the contraction index upwards; a residual is added after the chain is finished: u = x + (b_o + ..),
 * y = u + (b2 + ..).  So equal calls give equal bits, a user's rows do not depend on the batch, and the first `a` steps of a longer call
 * are the shorter call's.  An item id outside the table makes x_t NaN for that row (nothing is read out of bounds); the NaN then follows
 * the attention's rule above through every block, and other users are bitwise unaffected.
 *
 * recnn_seq_embed writes x_out float[n_users, T, hidden] (16-byte aligned, like table); store, slots, t0, T, table as recnn_lstm_encode.
 * recnn_seq_embed_backward: g_x float[n_users, T, hidden] (required) -> d_w_e float[hidden, emb_dim + 1], d_b_e float[hidden]; each may be
 * NULL (not wanted: its launch is skipped), written, not added to.  workspace: recnn_seq_embed_backward_workspace_bytes =
 * round256(4 nsplit hidden (emb_dim + 2)), nsplit as for recnn_attn_backward.  recnn_seq_embed_backward_table also writes d_table
 * float[n_items, emb_dim] (required; every row) as recnn_attn_backward_table does, with da = g_x and w_e read in place;
 * recnn_seq_embed_table_grad_workspace_bytes as recnn_gru_table_grad_workspace_bytes (hidden rows of w_e).
 *
 * recnn_block_forward: x -> y (y must not be x; both 16-byte aligned, like the four weight matrices and the workspace).
 *   recnn_block_workspace_bytes = recnn_attn_workspace_bytes (qkv, o, log-sum-exp) + round256(4 n_users T hidden) (u).  It does not
 *   depend on ffn: the [n_users T, ffn] activation lives in LDS, 64 rows by 32 columns at a time.  Host-only.
 * recnn_block_forward_train is the same call -- the same y bit for bit -- that keeps in `saved` what the backward needs: qkv, o, the
 *   log-sum-exp, u and the pre-activation a = w1 LN2(u) + b1 float[n_users T, ffn].  The LayerNorm statistics, the normalised rows and
 *   act(a) are NOT kept: the backward recomputes them (the same functions, the same bits).
 *   recnn_block_train_workspace_bytes: saved_bytes = recnn_block_workspace_bytes + round256(4 n_users T ffn); with W = max(ffn, 3 hidden),
 *   bwd_bytes = round256(4 W hidden) (a transposed weight) + 2 round256(4 n_users T hidden) + round256(4 n_users T W)
 *               + round256(4 n_users n_heads T) (delta) + round256(4 nsplit W (hidden + 1)) (the parts of the weight gradients)
 *               + round256(8 hidden (ceil(n_users T / 64) + ceil(ceil(n_users T / 64) / 64))) (the parts of d_gamma / d_beta).
 * recnn_block_backward is the backward of ONE recnn_block_forward_train call (the same x, sizes, parameters; `saved` as that call wrote
 *   it) for g_y float[n_users, T, hidden] (required).  Outputs, each may be NULL (not wanted: its launch is skipped -- and everything
 *   upstream of it that nothing else needs), written, not added to: d_x float[n_users, T, hidden] and the twelve parameter gradients in
 *   the shapes of their parameters.  d_gamma / d_beta: each workgroup of 64 rows sums its columns in row order, the parts are added in
 *   groups of 64 consecutive workgroups and then group after group.  The weight gradients are recnn_attn_backward's segmented tile.
 *
 * recnn_layernorm_rows: out = LN(x) for x float[rows, hidden] (the final LayerNorm); recnn_layernorm_rows_backward: g_out float[rows,
 * hidden] -> d_x, d_gamma, d_beta (each may be NULL), workspace of recnn_layernorm_rows_backward_workspace_bytes (the d_gamma / d_beta
 * parts above).  Errors: RECNN_E_INVALID with a message, before any launch. */
int recnn_seq_embed(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users, int t0, int T,
                    const float* table, int n_items, int emb_dim, int hidden, const float* w_e, const float* b_e, float* x_out,
                    void* stream);
int recnn_seq_embed_backward_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int64_t* bytes);
int recnn_seq_embed_backward(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                             int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* g_x, float* d_w_e,
                             float* d_b_e, void* workspace, void* stream);
int recnn_seq_embed_table_grad_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int n_items, int64_t* bytes);
int recnn_seq_embed_backward_table(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                                   int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden,
                                   const float* w_e, const float* g_x, float* d_w_e, float* d_b_e, float* d_table, void* workspace,
                                   void* table_workspace, void* stream);
int recnn_block_workspace_bytes(int n_users, int T, int hidden, int n_heads, int64_t* bytes);
int recnn_block_forward(const float* x, int n_users, int T, int hidden, int n_heads, int ffn, int act, int window, int alibi, float eps,
                        const float* w_in, const float* b_in, const float* w_o, const float* b_o, const float* w1, const float* b1,
                        const float* w2, const float* b2, const float* g1, const float* be1, const float* g2, const float* be2, float* y,
                        void* workspace, void* stream);
int recnn_block_train_workspace_bytes(int n_users, int T, int hidden, int n_heads, int ffn, int64_t* saved_bytes, int64_t* bwd_bytes);
int recnn_block_forward_train(const float* x, int n_users, int T, int hidden, int n_heads, int ffn, int act, int window, int alibi,
                              float eps, const float* w_in, const float* b_in, const float* w_o, const float* b_o, const float* w1,
                              const float* b1, const float* w2, const float* b2, const float* g1, const float* be1, const float* g2,
                              const float* be2, float* y, void* saved, void* stream);
int recnn_block_backward(const float* x, int n_users, int T, int hidden, int n_heads, int ffn, int act, int window, int alibi, float eps,
                         const float* w_in, const float* b_in, const float* w_o, const float* b_o, const float* w1, const float* b1,
                         const float* w2, const float* b2, const float* g1, const float* be1, const float* g2, const float* be2,
                         const void* saved, const float* g_y, float* d_x, float* d_w_in, float* d_b_in, float* d_w_o, float* d_b_o,
                         float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* d_g1, float* d_be1, float* d_g2, float* d_be2,
                         void* workspace, void* stream);
int recnn_layernorm_rows(const float* x, int rows, int hidden, const float* gamma, const float* beta, float eps, float* out,
                         void* stream);
int recnn_layernorm_rows_backward_workspace_bytes(int rows, int hidden, int64_t* bytes);
int recnn_layernorm_rows_backward(const float* x, int rows, int hidden, const float* gamma, float eps, const float* g_out, float* d_x,
                                  float* d_gamma, float* d_beta, void* workspace, void* stream);

/* Serving the two encoders above step by step (csrc/attn_dev.h): a per-session key/value cache and "append n steps".
 * The cache of one attention layer is kv float[n_sessions, capacity, 2 hidden]: position p of a session holds [k_p | v_p] in slot
 * p % capacity.  capacity is a multiple of 64; without a window a session holds at most capacity positions, with window = w the cache
 * is a ring and capacity >= recnn_kv_min_capacity(w, n) = 64 ceil((w - 1) / 64) + 64 ceil((n + 63) / 64): the key tiles an append
 * stages and the slots it writes then never share a slot (host-only; window, n >= 1).
 * An append call extends n_rows DISTINCT sessions rows[i] (int32, in [0, n_sessions)) by n steps each, session i from its own position
 * pos[i] (int32 >= 0: the number of positions it holds; without a window pos[i] + n <= capacity).  The caller owns pos: nothing on the
 * device counts.  The call writes k and v of positions pos[i] .. pos[i] + n - 1 into the cache and returns rows pos[i] .. pos[i] + n - 1
 * of the whole-history call over the session's pos[i] + n steps, BIT FOR BIT: the query blocks stay aligned to absolute multiples of 64,
 * a key tile is staged from the cache with pos[i] + n in T's place, and every row-wise product is the whole-history kernel on n_rows n
 * dense rows.  A staged row is a written, not yet overwritten position or zero: what other slots hold (stale rows, NaN) is never read.
 * A session the checks above would refuse (row or pos out of range) is skipped on the device: nothing is written out of bounds.
 * The new steps' inputs are given directly: items int32[n_rows, n] and ratings float[n_rows, n] are read as a store whose histories
 * are the rows -- user_off int64[n_rows + 1] = {0, n, 2 n, ..}, slots int32[n_rows] = {0, 1, ..} -- so the input rows go down the
 * gathered linear kernel's own chain (recnn_seq_embed with t0 = 0, T = n is the transformer's embedding of the new steps).
 *   recnn_kv_append_workspace_bytes  round256(12 n_rows n hidden) (qkv) + 2 round256(4 n_rows n hidden) (o, u).  Host-only.
 * recnn_attn_append: the layer of recnn_attn_encode; h_out float[n_rows, n, hidden].
 * recnn_block_append: the block of recnn_block_forward on x float[n_rows, n, hidden] -> y (y must not be x); kv is this block's cache.
 * Limits on hidden, n_heads, emb_dim, ffn, act, eps as in the whole-history calls; n_rows <= 65535, n_rows * n < 2^31; kv, table, the
 * weight matrices, x, y, h_out and the workspace 16-byte aligned.  Errors: RECNN_E_INVALID with a message, before any launch. */
int recnn_kv_min_capacity(int window, int n, int* capacity);
int recnn_kv_append_workspace_bytes(int n_rows, int n, int hidden, int64_t* bytes);
int recnn_attn_append(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_rows, int n,
                      const float* table, int n_items, int emb_dim, int hidden, int n_heads, int window, int alibi, const float* w_in,
                      const float* b_in, const float* w_o, const float* b_o, float* kv, int n_sessions, int capacity, const int32_t* pos,
                      const int32_t* rows, float* h_out, void* workspace, void* stream);
int recnn_block_append(const float* x, int n_rows, int n, int hidden, int n_heads, int ffn, int act, int window, int alibi, float eps,
                       const float* w_in, const float* b_in, const float* w_o, const float* b_o, const float* w1, const float* b1,
                       const float* w2, const float* b2, const float* g1, const float* be1, const float* g2, const float* be2, float* kv,
                       int n_sessions, int capacity, const int32_t* pos, const int32_t* rows, float* y, void* workspace, void* stream);

/* =====================================================================================
 * 11. Offline ranking evaluation (csrc/rank.hip, csrc/topk.hip, csrc/evalrank.hip): where the item the user took
 *    next lands in the ranking a generated action induces over the catalogue, and the hit rate / NDCG / MRR of a batch of such ranks.
 *    rank[b] = the number of items i != targets[b] that come before item targets[b] in the order of the search of section 7
 *    (recnn_dist_target_rank: distance ascending, -0 as +0, every NaN as one value after +inf, ties to the smaller id) or of
 *    section 5 (recnn_topk_target_rank: the internal key q.t, 2 q.t - |t|^2 or q.t / |t| descending, ties to the smaller id; an
 *    item whose key is NaN comes after every number, NaN keys order by id), in [0, n_items - 1].  The target's own key has the
 *    bits the scoring loop produces for that pair, so the result agrees with recnn_dist_matrix / recnn_dist_topk /
 *    recnn_topk_search entry for entry, and does not depend on the batch, the tile or the split.  A target id outside
 *    [0, n_items) gives rank -1; nothing is read out of bounds.  No limit on the rank: the whole table is counted.
 *    Per-split integer counts are summed afterwards (no atomics on global memory): equal calls give equal results.
 *    Limits: emb_dim == 128, ld_q % 4 == 0, queries / table / aux / workspace 16-byte aligned; item_aux as in sections 5 and 7.
 *    Errors: RECNN_E_INVALID, before any HIP call, for an unknown metric, p < 1 or NaN for minkowski, a null pointer, a misaligned
 *    operand, a missing aux and the limits above.  n_queries == 0 launches nothing.
 * ===================================================================================== */
int recnn_dist_target_rank_workspace_bytes(int n_queries, int n_items, int metric, int64_t* h_bytes);
/* targets int64[n_queries] (table row ids), out_rank int32[n_queries]; the metrics and p of section 7 */
int recnn_dist_target_rank(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                           int metric, double p, const float* item_aux, const int64_t* targets, int32_t* out_rank, void* workspace,
                           void* stream);
int recnn_topk_target_rank_workspace_bytes(int n_queries, int n_items, int64_t* h_bytes);
/* the same for RECNN_METRIC_IP / L2 / COS of section 5 */
int recnn_topk_target_rank(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                           int metric, const float* item_aux, const int64_t* targets, int32_t* out_rank, void* workspace,
                           void* stream);
/* Metrics of ranks int32[n], one relevant item per row.  mask uint8[n] (may be NULL): a zero byte skips the row.  h_ks: n_ks
 * cutoffs on the HOST, 1 <= n_ks <= 8, each >= 1, strictly ascending, of any size.  Both accumulators are device arrays that are
 * ACCUMULATED into (the caller zeroes them once):
 *   acc_f double[n_ks + 1]: per cutoff K the sum of 1 / log2(rank + 2) over the rows with 0 <= rank < K (NDCG@K, IDCG = 1), then the
 *                           sum of 1 / (rank + 1) (MRR);
 *   acc_i int64[n_ks + 3]:  per cutoff K the rows with 0 <= rank < K (hits), then the sum of ranks, the rows counted, and the rows with
 *                           rank < 0 that were not masked out (invalid: they count in nothing else).
 * Integers are exact; the float64 sums run in a fixed order that depends on n alone (per-workgroup trees, then one workgroup in
 * workgroup order): equal call sequences give equal bits.  workspace: recnn_rank_metrics_workspace_bytes(n) bytes, 8-byte aligned.
 * Errors: RECNN_E_INVALID, before any HIP call, for a null pointer, n < 0, n_ks outside 1..8 and cutoffs that are < 1 or not
 * strictly ascending.  n == 0 launches nothing. */
int recnn_rank_metrics_workspace_bytes(int n, int64_t* h_bytes);
int recnn_rank_metrics(const int32_t* ranks, const uint8_t* mask, int n, const int32_t* h_ks, int n_ks, double* acc_f,
                       int64_t* acc_i, void* workspace, void* stream);

/* =====================================================================================
 * 12. Per-row exclusion for the searches of sections 5 and 7 and the ranks of section 11 (csrc/seen.hip): leave the
 *    items a user has already consumed out of the candidate set, as the usual offline protocol does before hit@K / NDCG / MRR.
 *    mask: uint64[n_rows][W], W = ceil(n_items / 64); bit (i & 63) of word (i >> 6) of row b set = item i does not exist for query
 *    row b; the bits above n_items are zero.  recnn_seen_mask_build fills it from slices of one device id array: row b's list is
 *    ids[starts[b] : starts[b] + lengths[b]], unordered, duplicates allowed.  An id outside [0, n_items) and a position outside
 *    [0, n_ids) (a negative start or length, a list running past the end) are ignored: nothing is read out of bounds.  keep (may be
 *    NULL): bit keep[b] of row b is cleared after the row is built; a keep[b] outside [0, n_items) is a no-op.  A row is built in
 *    one workgroup's LDS with integer atomics and stored once (no global atomics, no memset): equal calls give equal words.
 *    Limit: n_items <= 1,048,576 (one row's words in LDS).  recnn_seen_mask_words is host-only.
 *    The *_excluding entry points take (mask, words_per_row = W) after the arguments of the call they extend, use that call's
 *    workspace query, and report its results over the items whose bit is clear:
 *      search  an excluded item is never reported, whatever its key.  A row with fewer than k items left ends in id -1 with distance
 *              +inf where distances ascend (L2, section 7) and -inf where scores descend (IP, COS).  k <= min(64, n_items) as before.
 *      rank    the number of items i != targets[b] that are not excluded in row b and come before the target.  The target's own bit is
 *              not consulted; its key has the bits of the plain call.  A target outside [0, n_items) gives -1.
 *    Errors: those of the extended call, and RECNN_E_INVALID for a null or misaligned mask, words_per_row != W, n_items above the limit.
 * ===================================================================================== */
int recnn_seen_mask_words(int n_items, int64_t* h_words);
int recnn_seen_mask_build(const int32_t* ids, int64_t n_ids, const int64_t* starts, const int64_t* lengths, const int64_t* keep,
                          int n_rows, int n_items, uint64_t* out_words, void* stream);
int recnn_topk_search_excluding(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                                int metric, const float* item_aux, int k, float* out_dist, int64_t* out_ids, void* workspace,
                                void* stream, const uint64_t* mask, int64_t words_per_row);
int recnn_dist_topk_excluding(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                              int metric, double p, const float* item_aux, int k, float* out_dist, int64_t* out_ids, void* workspace,
                              void* stream, const uint64_t* mask, int64_t words_per_row);
int recnn_topk_target_rank_excluding(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                                     int metric, const float* item_aux, const int64_t* targets, int32_t* out_rank, void* workspace,
                                     void* stream, const uint64_t* mask, int64_t words_per_row);
int recnn_dist_target_rank_excluding(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                                     int metric, double p, const float* item_aux, const int64_t* targets, int32_t* out_rank,
                                     void* workspace, void* stream, const uint64_t* mask, int64_t words_per_row);

/* =====================================================================================
 * 13. The catalogue ranked by the critic's Q-value (csrc/qrank.hip, csrc/scoresel.hip).
 *    For a critic  Q(s, a) = w3 . relu(W2 . relu(W1 [s | a] + b1) + b2) + b3  and an item table [n_items][128], layer 1 splits along
 *    its input:  S1 = state . W1[:, :S]^T + b1  per state row,  E1 = table . W1[:, S:]^T  per item (both recnn_qrank_layer1), and
 *    recnn_qrank_scores writes  Q[b][n] = w3 . relu(W2 . relu(S1[b] + E1[n]) + b2) + b3  for every pair, float32, exact-fp32 MFMA;
 *    no per-pair activation reaches memory.  The bits of Q[b][n] depend on the operands of that pair alone: not on n_states, n_items,
 *    the pair's place in a tile or how the caller blocks the state rows.
 *    hidden_padded: the hidden width zero-padded to a multiple of 64 (recnn_qrank_hidden_padded; hidden <= 256).  All operands are
 *    padded to it with zeros by the caller: w [hidden_padded][ld_w], bias / b2 / w3 [hidden_padded], w2 [hidden_padded][hidden_padded]
 *    (row j = output unit j), S1 / E1 rows of hidden_padded floats.  recnn_qrank_layer1: k % 16 == 0 (zero-pad the input columns),
 *    bias may be NULL.  16-byte aligned x, w, s1, e1, w2; strides multiples of 4 floats.
 *    recnn_qrank_block_rows (host-only): how many state rows of Q fit max_bytes, in whole 16-row tiles, at least one tile.
 *
 *    recnn_scores_topk / recnn_scores_rank select from float32 scores [n_rows][n_items] with row stride ld (floats) that already exist:
 *    larger score first, ties to the smaller id (-0 == +0), NaN after every number in id order.  mask (may be NULL, then
 *    words_per_row = 0): the exclusion words of section 12; an excluded item does not exist for its row.
 *      topk  0 < k <= 64, k may exceed n_items; a row with fewer than k items left ends in id -1 with score -inf.
 *      rank  int32: the items i != targets[b], not excluded, that come before the target; the target's own bit is not consulted; a target
 *            outside [0, n_items) gives -1 and reads nothing.
 *    Per-(row, split) results go through the workspace to a finishing kernel (no atomics): results do not depend on the split.
 *    Errors: RECNN_E_INVALID before any HIP call for null pointers, k outside 1..64, ld < n_items, misalignment, hidden above 256, and
 *    the mask errors of section 12.  Zero rows launch nothing.
 * ===================================================================================== */
int recnn_qrank_hidden_padded(int hidden, int* h_padded);
int recnn_qrank_block_rows(int n_items, int64_t max_bytes, int64_t* h_rows);
int recnn_qrank_layer1(const float* x, int64_t ld_x, int n_rows, int k, const float* w, int64_t ld_w, const float* bias,
                       int hidden_padded, float* out, int64_t ld_out, void* stream);
int recnn_qrank_scores(const float* s1, int64_t ld_s1, int n_states, const float* e1, int64_t ld_e1, int n_items, int hidden_padded,
                       const float* w2, const float* b2, const float* w3, float b3, float* out, int64_t ld_out, void* stream);
int recnn_scores_topk_workspace_bytes(int n_rows, int k, int64_t* h_bytes);
int recnn_scores_topk(const float* scores, int64_t ld, int n_rows, int n_items, int k, float* out_scores, int64_t* out_ids,
                      void* workspace, void* stream, const uint64_t* mask, int64_t words_per_row);
int recnn_scores_rank_workspace_bytes(int n_rows, int n_items, int64_t* h_bytes);
int recnn_scores_rank(const float* scores, int64_t ld, int n_rows, int n_items, const int64_t* targets, int32_t* out_rank,
                      void* workspace, void* stream, const uint64_t* mask, int64_t words_per_row);

/* =====================================================================================
 * 14. The critic's Q-value over per-row candidate lists, and the list sorted by it (csrc/qcand.hip): the second stage
 *    of a retrieve-then-rerank recommender.  s1, e1, hidden_padded, w2, b2, w3, b3 are the operands of recnn_qrank_scores (section 13).
 *    ids: [n_states][n_candidates] table row ids with row stride ld_ids (elements), int32 (ids_are_int64 = 0) or int64 (1).
 *      Q[b][j] = w3 . relu(W2 . relu(S1[b] + E1[ids[b][j]]) + b2) + b3,  with the bits of recnn_qrank_scores' Q[b][ids[b][j]]
 *    whatever n_states, n_candidates or the slot j.  A slot whose id is outside [0, n_items) is empty: it reads nothing, Q = -inf.
 *    recnn_qcand_scores: any n_candidates >= 1, out float32 [n_states][n_candidates] with row stride ld_out.
 *    recnn_qcand_rerank: n_candidates <= 64, 1 <= k <= n_candidates; writes the first k slots of every row in the order
 *      larger Q first, ties to the smaller id, equal ids to the smaller slot, -0 == +0, NaN after every number in id order, empty
 *      slots last (id -1 at -inf)  into out_q float32 / out_ids int64 [n_states][k], in the launch that computes Q.
 *      targets (int64 [n_states], may be NULL together with out_pos): out_pos[b] int32 = the non-empty slots that come before the
 *      first slot holding targets[b], -1 if no slot holds it or it is outside [0, n_items).  fallback_rank (int32 [n_states], may
 *      be NULL): where the target is in range but in no slot, out_pos[b] = fallback_rank[b] < 0 ? -1 : max(fallback_rank[b], the
 *      row's non-empty slots) instead: the target's rank when every other item follows the candidates in the first stage's order.
 *    One launch each, no workspace, no atomics.  Errors: RECNN_E_INVALID before any HIP call for null pointers, misalignment,
 *    strides below the row length, hidden above 256, n_candidates above 64 (rerank) and k outside 1..n_candidates.  Zero rows
 *    launch nothing.
 * ===================================================================================== */
int recnn_qcand_scores(const float* s1, int64_t ld_s1, int n_states, const float* e1, int64_t ld_e1, int n_items, int hidden_padded,
                       const float* w2, const float* b2, const float* w3, float b3, const void* ids, int64_t ld_ids, int n_candidates,
                       int ids_are_int64, float* out, int64_t ld_out, void* stream);
int recnn_qcand_rerank(const float* s1, int64_t ld_s1, int n_states, const float* e1, int64_t ld_e1, int n_items, int hidden_padded,
                       const float* w2, const float* b2, const float* w3, float b3, const void* ids, int64_t ld_ids, int n_candidates,
                       int ids_are_int64, int k, float* out_q, int64_t* out_ids, const int64_t* targets, int32_t* out_pos,
                       const int32_t* fallback_rank, void* stream);

/* =====================================================================================
 * 15. IVF-Flat (csrc/ivf.hip): a k-means coarse quantiser over the item table, the items stored per nearest centroid,
 *    a search that scores only the lists a query probes.  emb_dim is 128 throughout.  Distances to centroids -- an item's nearest
 *    centroid while training, a query's nprobe nearest while searching -- are recnn_topk_search over the centroid table (section 5);
 *    the entry points here take its int64 ids.
 *    recnn_ivf_build_lists: assign int64 [n_items] (list of every item) -> out_assignment int32 [n_items] (-1 for an id outside
 *      [0, nlist), which is then in no list), list_start int32 [nlist + 1] (CSR), list_ids int32 [n_items]: the item ids list by list,
 *      ascending id inside a list.  A stable counting sort, integers only: a function of the ids alone.
 *    recnn_ivf_update_centroids: centroids[c] = sum(table rows of list c) / count[c] in place, fp32.  The sum's order is fixed by the
 *      list (rows dealt round-robin to four partial sums, added as (0 + 1) + (2 + 3)), the division is the correctly rounded one; no
 *      float atomics.  An empty list keeps its centroid.
 *    recnn_ivf_gather_rows: out_rows[r] = table[list_ids[r]], the table in list order.
 *    recnn_ivf_scan: queries float32 [n_queries][128] (row stride ld_q), list_rows / list_aux the table and its |t|^2 (section 5's
 *      item aux, L2 only) in list order, probe int64 [n_queries][nprobe] the lists of every query (distinct within a row; an id outside
 *      [0, nlist) is an empty slot).  Reports, over the items of the probed lists, what recnn_topk_search reports over the table:
 *      out_dist float32 / out_ids int64 [n_queries][k], L2 squared distances ascending or IP scores descending, ties to the smaller
 *      item id, each value with the bits recnn_topk_search gives that (query, item) pair; a row with fewer than k items in reach ends
 *      in id -1 at +inf (L2) / -inf (IP).  k may exceed the items in reach.  mask (may be NULL) / words_per_row: section 12's
 *      exclusion bits over item ids.  metric: RECNN_TOPK IP (0) or L2 (1).
 *    The *_workspace_bytes queries are host-only.  Limits: 1 <= nlist <= n_items, nprobe <= min(64, nlist), k <= 64,
 *    n_queries * nprobe < 2^25.  Errors: RECNN_E_INVALID before any HIP call, with a message that names the argument.
 * ===================================================================================== */
int recnn_ivf_lists_workspace_bytes(int n_items, int nlist, int64_t* h_bytes);
int recnn_ivf_build_lists(const int64_t* assign, int n_items, int nlist, int32_t* out_assignment, int32_t* list_start,
                          int32_t* list_ids, void* workspace, void* stream);
int recnn_ivf_update_centroids(const float* table, int n_items, const int32_t* list_start, const int32_t* list_ids, int nlist,
                               float* centroids, void* stream);
int recnn_ivf_gather_rows(const float* table, int n_items, const int32_t* list_ids, float* out_rows, void* stream);
int recnn_ivf_search_workspace_bytes(int n_queries, int nprobe, int nlist, int k, int64_t* h_bytes);
int recnn_ivf_scan(const float* queries, int64_t ld_q, int n_queries, const float* list_rows, const float* list_aux,
                   const int32_t* list_start, const int32_t* list_ids, int nlist, int n_items, int metric, const int64_t* probe,
                   int nprobe, int k, float* out_dist, int64_t* out_ids, void* workspace, void* stream, const uint64_t* mask,
                   int64_t words_per_row);

/* =====================================================================================
 * 16. A candidate slate diversified (csrc/slate.hip): the similarity matrix of a row's candidates, the greedy
 *    maximal-marginal-relevance pick over it, and the slate's intra-list distance.  table float32 [n_items][128], 16-byte aligned;
 *    ids [n_rows][n_candidates] table row ids with row stride ld_ids (elements), int32 (ids_are_int64 = 0) or int64 (1),
 *    1 <= n_candidates <= 64; a slot whose id is outside [0, n_items) is empty and reads nothing.  kind: 0 IP, 1 L2, 2 COS.
 *      G = X X^T over the gathered rows X (exact fp32 MFMA), n_i = G_ii
 *      IP  S_ij = G_ij     COS  S_ij = G_ij / (sqrt(n_i) sqrt(n_j)), 0 where a norm is 0     L2  S_ij = -max((n_i + n_j) - 2 G_ij, 0)
 *    Entries of an empty slot are 0.  S is bitwise symmetric, and the bits of S_ij depend on the two table rows alone.
 *    recnn_slate_similarity: out float32 [n_rows][n_candidates][n_candidates].
 *    recnn_slate_rerank: rel float32 [n_rows][n_candidates] (row stride ld_rel), larger is better; 0 <= lam <= 1; 1 <= k <= n_candidates.
 *      With mu = 1 - lam (fp32) step 1 scores slot j as lam * r_j, step t > 1 as (lam * r_j) - (mu * m_j), m_j the largest S_js over
 *      the slots s chosen so far, every operation one correctly rounded fp32 operation; the slot chosen is the first one not yet
 *      chosen in the order of section 14 (larger score first, -0 == +0, ties to the smaller id, equal ids to the smaller slot, NaN
 *      after every number, empty slots last).  r_j = rel_j, or with normalize = 1 (rel_j - mn) / (mx - mn), mn and mx over the row's
 *      non-empty slots of finite relevance (0 when mx == mn; a non-finite relevance passes through).  Writes out_score float32 (the
 *      score at the moment of the choice), out_ids int64 and out_slot int32 (the slot's index in the list), [n_rows][k]; once the
 *      non-empty slots run out: -inf, -1, -1.
 *    recnn_slate_ild: out float64 [n_rows]: the mean over unordered pairs of non-empty slots of D_ij, formed in fp32 from S_ij (COS
 *      1 - S_ij, L2 sqrt(-S_ij), IP -S_ij) and summed in float64; NaN with fewer than two non-empty slots.
 *    One launch each up to 2^20 rows (more are looped inside the call), no workspace, no atomics.  Errors: RECNN_E_INVALID before any
 *    HIP call, with a message that names the argument.  Zero rows launch nothing.
 * ===================================================================================== */
int recnn_slate_similarity(const float* table, int n_items, const void* ids, int64_t ld_ids, int n_rows, int n_candidates,
                           int ids_are_int64, int kind, float* out, void* stream);
int recnn_slate_rerank(const float* table, int n_items, const void* ids, int64_t ld_ids, int n_rows, int n_candidates,
                       int ids_are_int64, int kind, const float* rel, int64_t ld_rel, float lam, int normalize, int k,
                       float* out_score, int64_t* out_ids, int32_t* out_slot, void* stream);
int recnn_slate_ild(const float* table, int n_items, const void* ids, int64_t ld_ids, int n_rows, int n_candidates, int ids_are_int64,
                    int kind, double* out, void* stream);

/* =====================================================================================
 * 17. Off-policy evaluation of the discrete policies (csrc/logprob.hip, csrc/ope.hip).
 *    recnn_catalogue_logprob: x float32 [B][K] (row stride ld_x), W [N][K] (row stride ld_w; float32, or bf16 with w_bf16 = 1, x then
 *      rounded to bf16 on load), c float32 [N], actions int64 [B].  With z[b, n] = x[b] . W[n] + c[n] (exact-fp32 or bf16 MFMA, fp32
 *      accumulation) it writes lse[b] = log sum_n exp(z[b, n]) and logprob[b] = min(z[b, a_b] - lse[b], 0), float32 [B] each; the
 *      [B, N] matrix is never stored.  An action outside [0, N) gives NaN in logprob[b]; lse[b] is valid and no other row changes.
 *      The catalogue is cut into slices of items_per_slice items (a positive multiple of 128), one workgroup column each, merged per
 *      row in slice order: no atomics, equal calls give equal bits, and a row's bits depend on that row, W, c and items_per_slice
 *      alone, not on B or the row's position.  K a multiple of 32 (float32) / 64 (bf16), rows 16-byte aligned, ld_x, ld_w >= K.
 *      x, W and c must be finite: a row whose logits are all -inf, or hold +inf or NaN, gets NaN (no other row is affected).
 *      workspace: recnn_catalogue_logprob_workspace_bytes(B, N, items_per_slice) bytes, 4-byte aligned (host arithmetic only).
 *    recnn_ope_accumulate: lp_pi, lp_beta, reward float32 [n]; mask uint8 [n] or NULL (a zero byte skips the row); q_logged, v_dm
 *      float32 [n], both or both NULL; cap > 0, +inf for none; top_k >= 0, 0 for off.  A masked-out row counts nowhere; an unmasked
 *      row with a NaN in lp_pi or lp_beta counts in acc_i[1] and nowhere else.  For every other row, in float64,
 *        w = exp(lp_pi - lp_beta);  top_k >= 1: w *= top_k (1 - exp(lp_pi))^(top_k - 1);  wc = min(w, cap)
 *      and the call adds to acc_f float64 [8]: sum w, sum w^2, sum w r, sum wc, sum wc r, sum r, sum v_dm + w (r - q_logged), and
 *      takes the maximum of acc_f[7] and max w; to acc_i int64 [3]: rows counted, invalid rows, rows with w > cap.  The sums have one
 *      order that depends on n alone (recnn_rank_metrics', section 11); no atomics: equal call sequences give equal bits.
 *      workspace: recnn_ope_accumulate_workspace_bytes(n) bytes, 8-byte aligned.
 *    Errors: RECNN_E_INVALID before any HIP call, with a message.  Zero rows launch nothing.
 * ===================================================================================== */
int recnn_catalogue_logprob_workspace_bytes(int B, int N, int items_per_slice, int64_t* h_bytes);
int recnn_catalogue_logprob(const float* x, int64_t ld_x, int B, int K, const void* W, int64_t ld_w, int w_bf16, const float* c, int N,
                            const int64_t* actions, int items_per_slice, float* logprob, float* lse, void* workspace, void* stream);
int recnn_ope_accumulate_workspace_bytes(int n, int64_t* h_bytes);
int recnn_ope_accumulate(const float* lp_pi, const float* lp_beta, const float* reward, const uint8_t* mask, const float* q_logged,
                         const float* v_dm, int n, double cap, int top_k, double* acc_f, int64_t* acc_i, void* workspace,
                         void* stream);

/* =====================================================================================
 * 18. Backward of the catalogue log-prob: full-softmax cross-entropy training (csrc/logprob_bwd.hip).
 *    recnn_catalogue_logprob_bwd: x, W, c, actions, K, N, w_bf16, the strides and items_per_slice as recnn_catalogue_logprob takes
 *      them (section 17); lse float32 [B] as that call wrote it; g_lp, g_lse float32 [B], the gradients arriving at logprob and lse,
 *      either may be NULL for zeros.  With p[b, n] = exp(z[b, n] - lse[b]) and
 *        D[b, n] = (g_lse[b] - g_lp[b]) p[b, n] + g_lp[b] [n == a_b]
 *      (the derivative of z_a - lse: the forward's min(., 0) is a rounding guard) it writes dx = D W float32 [B][K] (row stride
 *      ld_dx), dW = D^T x float32 [N][K] (row stride ld_dw) and dc[n] = sum_b D[b, n] float32 [N].  D is recomputed tile by tile
 *      and never stored.  A row whose action lies outside [0, N) takes g_lp[b] as 0: no one-hot term, no NaN; g_lse[b] still flows.
 *      dx NULL skips the dx kernels; dW and dc both NULL skip the other kernel; dW or dc alone may be NULL.  B == 0 launches nothing
 *      and zero-fills dW / dc where given.  w_bf16 = 1: W is the bf16 copy, x is rounded to bf16 on load and D before the second
 *      product; dW is float32 either way.
 *      K (as passed, i.e. padded) is at most 256: the output tile stays in registers, and a larger K is refused before any launch.
 *      No atomics: equal calls give equal bits, and with items_per_slice fixed a row's dx bits depend on that row, W, c, its lse and
 *      gradients and items_per_slice alone.  dx, dW rows and the workspace 16-byte aligned, ld_dx, ld_dw >= K and multiples of 4.
 *      workspace: recnn_catalogue_logprob_bwd_workspace_bytes(B, N, K, items_per_slice) bytes (host arithmetic only): one [B][K]
 *      partial of dx per catalogue slice.  Needed for dx only.
 *    Errors: RECNN_E_INVALID before any HIP call, with a message.
 * ===================================================================================== */
int recnn_catalogue_logprob_bwd_workspace_bytes(int B, int N, int K, int items_per_slice, int64_t* h_bytes);
int recnn_catalogue_logprob_bwd(const float* x, int64_t ld_x, int B, int K, const void* W, int64_t ld_w, int w_bf16, const float* c, int N,
                                const int64_t* actions, const float* lse, const float* g_lp, const float* g_lse, int items_per_slice,
                                float* dx, int64_t ld_dx, float* dW, int64_t ld_dw, float* dc, void* workspace, void* stream);

/* =====================================================================================
 * 19. Sampled softmax with negatives shared by the batch (csrc/sampled.hip).
 *    x, W, K, N, w_bf16 and the strides as in section 17; c float32 [N] or NULL (zeros); targets int64 [B]; negatives int64 [S],
 *    S >= 1, one list for every row, repeats allowed; target_log_q float32 [B] and negative_log_q float32 [S], either may be NULL.
 *        z_t[b]  = x[b] . W[a_b] + c[a_b] - target_log_q[b]          z[b, s] = x[b] . W[n_s] + c[n_s] - negative_log_q[s]
 *        lse[b]  = log(exp z_t[b] + sum_s exp z[b, s])               logprob[b] = min(z_t[b] - lse[b], 0)
 *    A negative outside [0, N) is an absent column for every row; with remove_hits != 0 a negative equal to a row's target is absent in
 *    that row.  A target outside [0, N): logprob[b] = NaN, lse[b] over the negatives alone, g_lp[b] counts as 0, g_lse[b] flows.
 *    Neither pass stores a [B][S] matrix or a gathered [S][K] copy of W: the rows are read through the ids.
 *    recnn_sampled_logprob writes logprob, lse and z_target (z_t; NaN for an invalid target), float32 [B] each.  The negatives are cut
 *      into slices of items_per_slice (a positive multiple of 128), merged per row in slice order, the target's term last.
 *      workspace: recnn_sampled_logprob_workspace_bytes(B, S, items_per_slice) bytes, 4-byte aligned.
 *    recnn_sampled_logprob_bwd: lse and z_target as the forward wrote them; g_lp, g_lse float32 [B] or NULL for zeros.  With
 *      p = exp(z - lse), gd = g_lse - g_lp:   D[b, s] = gd_b p[b, s]   D_t[b] = gd_b p_t[b] + g_lp[b]
 *      it writes d_target = D_t float32 [B] (always), dx = D W[n] + D_t W[a] float32 [B][K], the compact dWs[s] = sum_b D[b, s] x[b]
 *      float32 [S][K] and dcs[s] = sum_b D[b, s] float32 [S], and dWt[b] = D_t[b] x[b] float32 [B][K]; each of dx, dWs, dcs, dWt may
 *      be NULL.  dWs / dcs are summed over chunks of the rows, merged in chunk order; the chunk count depends on (B, S) alone.
 *      w_bf16 = 1: x is rounded to bf16 where it meets W or D, D before the second product; D_t is not rounded.  B == 0 launches
 *      nothing and zero-fills dWs / dcs.  workspace: recnn_sampled_logprob_bwd_workspace_bytes(B, S, K, items_per_slice) bytes,
 *      16-byte aligned.
 *    recnn_sampled_scatter sums the S + B contributions by item id: dW[n] = sum_{s: n_s = n} dWs[s] + sum_{b: a_b = n} D_t[b] x[b]
 *      float32 [N][K] (x rounded to bf16 first when x_bf16 != 0), dc[n] likewise from dcs and D_t; dW or dc may be NULL.  Ids outside
 *      [0, N) contribute nothing.  Every row of dW and dc is written once, exact +0 where nothing landed; a row's contributions are
 *      added in the order negatives (by s), then targets (by b).  workspace: recnn_sampled_scatter_workspace_bytes(B, S, N, K).
 *    K (as passed, i.e. padded) is at most 256; a wider K and S = 0 are refused by name before any launch.  No float atomics: equal
 *    calls give equal bits, and with items_per_slice fixed a row's logprob, lse and dx bits depend on that row, W, c, the negatives
 *    and the corrections alone.  The *_workspace_bytes queries are host arithmetic only.
 *    Errors: RECNN_E_INVALID before any HIP call, with a message.
 * ===================================================================================== */
int recnn_sampled_logprob_workspace_bytes(int B, int S, int items_per_slice, int64_t* h_bytes);
int recnn_sampled_logprob(const float* x, int64_t ld_x, int B, int K, const void* W, int64_t ld_w, int w_bf16, const float* c, int N,
                          const int64_t* targets, const int64_t* negatives, int S, const float* target_log_q,
                          const float* negative_log_q, int remove_hits, int items_per_slice, float* logprob, float* lse,
                          float* z_target, void* workspace, void* stream);
int recnn_sampled_logprob_bwd_workspace_bytes(int B, int S, int K, int items_per_slice, int64_t* h_bytes);
int recnn_sampled_logprob_bwd(const float* x, int64_t ld_x, int B, int K, const void* W, int64_t ld_w, int w_bf16, const float* c, int N,
                              const int64_t* targets, const int64_t* negatives, int S, const float* negative_log_q, int remove_hits,
                              const float* lse, const float* z_target, const float* g_lp, const float* g_lse, int items_per_slice,
                              float* dx, int64_t ld_dx, float* dWs, int64_t ld_dws, float* dcs, float* d_target, float* dWt,
                              int64_t ld_dwt, void* workspace, void* stream);
int recnn_sampled_scatter_workspace_bytes(int B, int S, int N, int K, int64_t* h_bytes);
int recnn_sampled_scatter(const int64_t* negatives, int S, const int64_t* targets, int B, const float* dWs, int64_t ld_dws,
                          const float* dcs, const float* x, int64_t ld_x, int x_bf16, const float* d_target, int K, int N, float* dW,
                          int64_t ld_dw, float* dc, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RECNN_HIP_H */
