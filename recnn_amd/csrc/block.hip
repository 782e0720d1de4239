// block.hip -- the transformer state encoder of the dynamic-length path: the gathered embedding, pre-LN transformer
// blocks on a dense [U, T, H] residual stream, and the final LayerNorm; forward and backward, and the recnn_seq_embed*, recnn_block_*
// and recnn_layernorm_rows* entry points.  The attention inside a block is attn.hip's layer on a dense qkv (attn_dev.h).
//
//   the block        u = x + W_o Attn(LN1(x)) + b_o,  y = u + W_2 act(W_1 LN2(u) + b_1) + b_2         (act: relu, or gelu in its erf form)
//   LayerNorm        per row of H values, by the four lanes that share the row: lane q sums columns q, q + 4, .. upwards, the four sums
//                    are folded (s0 + s1) + (s2 + s3); the mean first, then the centred squares the same way (two passes: no
//                    E[x^2] - E[x]^2), rstd = 1 / sqrt(var + eps), n = fma((x - mean) rstd, gamma, beta).  One function (ln_rows) on
//                    rows held in LDS serves every kernel that normalises, so a row's normalised bits are the same wherever it is met.
//   linear kernels   attn_dev.h describes them: the embedding is its gathered linear, every other product its dense linear -- with LN
//                    for the in-projection, the residual epilogue for the out-projection, the act' epilogue for d_a.
//   feed-forward     one workgroup per 64 rows: LN2 in place in LDS, then F is walked in chunks of 32: wave w computes 32 rows by 16
//                    columns of the chunk's a = W_1 n + b_1 (bias first, k upwards), act(a) goes to a [64][32] tile in LDS, and that
//                    tile feeds y's accumulators (wave w owns column tiles w, w + 4, .. of H: 64 accumulator registers at H = 256),
//                    k upwards inside the chunk and chunk after chunk: y = u + (b_2 + sum_f act(a)[f] W_2[., f]), f = 0, 1, ..; the
//                    residual is added last.  The [rows, F] activation reaches memory only when the training forward asks for the
//                    pre-activation a (the backward needs its sign / its value).
//   backward         what the training forward keeps per block: qkv, o, the log-sum-exp parts, u and a.  The normalised rows and
//                    act(a) are recomputed.  Weight gradients are attn_dev.h's launch_weight_grad over segments of the
//                    samples; products with a transposed weight run the linear kernel over a transposed copy; the LayerNorm backward
//                    is row-wise with the forward's lane layout and also sums, per 64 rows, the columns of dn xhat and dn -- those
//                    parts are added in groups of 64 consecutive workgroups and then group after group (no atomics, one order).
//   append           recnn_block_append: the block on the n new steps of sessions whose keys and values live in a KV cache
//                    -- the forward's launches on R n dense rows, attn_dev.h's attention over the cache, and for few rows the
//                    feed-forward in 16-row workgroups (blk_ffn_rows16_kernel: the same element chains).
// Every sum has a fixed order that depends on nothing but the row's own data and (t, j): equal calls give equal bits, a user's bits
// do not depend on the batch, and h[:, :a] of a longer call equals the shorter call's.
#include "attn_dev.h"

namespace {

constexpr int FF_C = 32;            // feed-forward: columns of F per chunk (two workgroups per CU fit at H = 256: 75.8 KB of LDS each)
constexpr int FF_LD = FF_C + AT_PAD;
constexpr int BLK_GROUP = 64;       // LayerNorm backward: workgroup parts per first-level sum

// ------------------------------------------------------------------------------------------------ feed-forward
struct FfnArgs {
  int rows, H, F, act;
  const float* u;                   // [rows][H]
  const float *w1, *b1, *w2, *b2;   // [F][H], [F], [H][F], [H]
  const float *gamma, *beta;        // LN2
  float eps;
  float* a1;                        // [rows][F] or NULL: the pre-activation, kept for the backward
  float* y;                         // [rows][H]
};
inline size_t ffn_lds(int H) { return (size_t)LIN_ROWS * (H + AT_PAD + FF_LD) * sizeof(float); }

// grid ceil(rows / 64), 256 threads
__global__ __launch_bounds__(256) void blk_ffn_kernel(const FfnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = a.H, F = a.F, ldx = H + AT_PAD;
  float* xs = smem;                 // [64][ldx]: LN2(u)
  float* hs = xs + LIN_ROWS * ldx;  // [64][FF_LD]: act(a) of the chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int s0 = blockIdx.x * LIN_ROWS;
  const int ntiles = H >> 4;
  stage_rows(xs, ldx, a.u, H, s0, a.rows, H, tid);
  __syncthreads();
  ln_rows(xs, ldx, H, a.gamma, a.beta, a.eps, tid);
  __syncthreads();
  f32x4 acc[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float bias = wave + 4 * j < ntiles ? a.b2[(wave + 4 * j) * 16 + r] : 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[j][mt] = f32x4{bias, bias, bias, bias};
  }
  for (int f0 = 0; f0 < F; f0 += FF_C) {
    // the chunk's pre-activation [64][32]: wave w owns column tile w & 1 and row tiles 2 (w >> 1), 2 (w >> 1) + 1
    const int ct = wave & 1, mh = 2 * (wave >> 1);
    const bool on = f0 + 16 * ct < F;                           // F is a multiple of 16: a tile is whole or absent (wave-uniform)
    const int col = f0 + 16 * ct + r;
    f32x4 t[2];
    if (on) {
      const float bias = a.b1[col];
#pragma unroll
      for (int m = 0; m < 2; ++m) t[m] = f32x4{bias, bias, bias, bias};
      const float* wrow = a.w1 + (int64_t)col * H;
      for (int k0 = 0; k0 < H; k0 += 16) {
        const f32x4 bv = *(const f32x4*)(wrow + k0 + 4 * g);
        f32x4 av[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) av[m] = *(const f32x4*)(xs + (16 * (mh + m) + r) * ldx + k0 + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int m = 0; m < 2; ++m) t[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][e], bv[e], t[m], 0, 0, 0);
      }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 16 * (mh + m) + 4 * g + i;
        float v = 0.f;
        if (on) {
          v = act_fwd(t[m][i], a.act);
          if (a.a1 && s0 + row < a.rows) a.a1[(int64_t)(s0 + row) * F + col] = t[m][i];
        }
        hs[row * FF_LD + 16 * ct + r] = v;
      }
    __syncthreads();
    const int kw = min(FF_C, F - f0);
    for (int k0 = 0; k0 < kw; k0 += 16) {
      f32x4 av[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) av[mt] = *(const f32x4*)(hs + (16 * mt + r) * FF_LD + k0 + 4 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (wave + 4 * j >= ntiles) continue;                   // (wave-uniform)
        const f32x4 bv = *(const f32x4*)(a.w2 + (int64_t)((wave + 4 * j) * 16 + r) * F + f0 + k0 + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) acc[j][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][e], bv[e], acc[j][mt], 0, 0, 0);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (wave + 4 * j >= ntiles) continue;
    const int col = (wave + 4 * j) * 16 + r;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int s = s0 + 16 * mt + 4 * g + i;
        if (s < a.rows) a.y[(int64_t)s * H + col] = a.u[(int64_t)s * H + col] + acc[j][mt][i];
      }
  }
}

// The feed-forward for FEW rows (the append path, DESIGN.md 31: R n rows, often 25): blk_ffn_kernel's element chains in another
// distribution of the work.  With one workgroup per 64 rows, 25 rows are ONE workgroup that walks F in 32 chunks, each a serial run of
// dependent weight loads.  Here a workgroup owns 16 rows (one MFMA row tile) and walks F in chunks of 128: wave w computes column tiles
// 2 w and 2 w + 1 of the chunk's a = W_1 n + b_1 (bias first, k upwards), act(a) goes to a [16][128] tile in LDS, and that tile feeds y's
// accumulators (wave w owns column tiles w, w + 4, .. of H), k upwards inside the chunk and chunk after chunk.  Every element of a and
// of y is the same chain of the same MFMAs as in blk_ffn_kernel -- the bias, then f = 0, 1, .. in blocks of 16, e = 0 .. 3 inside a
// block, the residual last -- so the bits are that kernel's (tests/test_gpu_kv_cache.py compares them on both sides of FFN_FEW_ROWS).
constexpr int FFR = 16;             // rows per workgroup
constexpr int FFR_C = 128;          // columns of F per chunk
constexpr int FFR_LD = FFR_C + AT_PAD;
constexpr int FFN_FEW_ROWS = 4096;  // up to here the append path runs this kernel: 256 workgroups
inline size_t ffn_rows16_lds(int H) { return (size_t)FFR * (H + AT_PAD + FFR_LD) * sizeof(float); }

// grid ceil(rows / 16), 256 threads; a.a1 is not written (no backward follows an append)
__global__ __launch_bounds__(256) void blk_ffn_rows16_kernel(const FfnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = a.H, F = a.F, ldx = H + AT_PAD, C4 = H >> 2;
  float* xs = smem;                 // [16][ldx]: LN2(u)
  float* hs = xs + FFR * ldx;       // [16][FFR_LD]: act(a) of the chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int s0 = blockIdx.x * FFR;
  const int ntiles = H >> 4;
  for (int idx = tid; idx < FFR * C4; idx += 256) {
    const int row = idx / C4, c = idx - row * C4, s = s0 + row;
    *(float4*)(xs + row * ldx + 4 * c) = s < a.rows ? *(const float4*)(a.u + (int64_t)s * H + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  if (tid < 4 * FFR) ln_rows(xs, ldx, H, a.gamma, a.beta, a.eps, tid);      // (all of wave 0: row tid >> 2, lane tid & 3 of its four)
  __syncthreads();
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float bias = wave + 4 * j < ntiles ? a.b2[(wave + 4 * j) * 16 + r] : 0.f;
    acc[j] = f32x4{bias, bias, bias, bias};
  }
  for (int f0 = 0; f0 < F; f0 += FFR_C) {
    f32x4 t[2];
    bool on[2];
    const float* wrow[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int col = f0 + 16 * (2 * wave + c) + r;
      on[c] = f0 + 16 * (2 * wave + c) < F;                       // F is a multiple of 16: a tile is whole or absent (wave-uniform)
      const float bias = on[c] ? a.b1[col] : 0.f;
      t[c] = f32x4{bias, bias, bias, bias};
      wrow[c] = a.w1 + (int64_t)(on[c] ? col : 0) * H;
    }
    if (on[0]) {                                                  // (an absent tile reads row 0 of W_1 and is dropped below)
      f32x4 b0 = *(const f32x4*)(wrow[0] + 4 * g), b1 = *(const f32x4*)(wrow[1] + 4 * g);
      for (int k0 = 0; k0 < H; k0 += 16) {
        const int kn = k0 + 16 < H ? k0 + 16 : k0;                // the next block's weights are in flight under this block's products
        const f32x4 n0 = *(const f32x4*)(wrow[0] + kn + 4 * g), n1 = *(const f32x4*)(wrow[1] + kn + 4 * g);
        const f32x4 av = *(const f32x4*)(xs + r * ldx + k0 + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          t[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], b0[e], t[0], 0, 0, 0);
          t[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], b1[e], t[1], 0, 0, 0);
        }
        b0 = n0;
        b1 = n1;
      }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) hs[(4 * g + i) * FFR_LD + 16 * (2 * wave + c) + r] = on[c] ? act_fwd(t[c][i], a.act) : 0.f;
    __syncthreads();
    const int kw = min(FFR_C, F - f0);
    const float* w2row[4];
    f32x4 bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int tile = wave + 4 * j < ntiles ? wave + 4 * j : 0;        // (an absent tile reads tile 0 of W_2 and is not stored)
      w2row[j] = a.w2 + (int64_t)(tile * 16 + r) * F + f0 + 4 * g;
      bv[j] = *(const f32x4*)w2row[j];
    }
    for (int k0 = 0; k0 < kw; k0 += 16) {
      const int kn = k0 + 16 < kw ? k0 + 16 : k0;
      f32x4 nv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) nv[j] = *(const f32x4*)(w2row[j] + kn);
      const f32x4 av = *(const f32x4*)(hs + r * FFR_LD + k0 + 4 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[j][e], acc[j], 0, 0, 0);
        bv[j] = nv[j];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (wave + 4 * j >= ntiles) continue;
    const int col = (wave + 4 * j) * 16 + r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int s = s0 + 4 * g + i;
      if (s < a.rows) a.y[(int64_t)s * H + col] = a.u[(int64_t)s * H + col] + acc[j][i];
    }
  }
}

// ------------------------------------------------------------------------------------------------ row-wise kernels
// out = LN(x), rows of H; grid ceil(rows / 64), 256 threads, LDS [64][H + 4]
__global__ __launch_bounds__(256) void blk_ln_rows_kernel(const float* x, int rows, int H, const float* gamma, const float* beta, float eps,
                                                          float* out) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ldx = H + AT_PAD, tid = threadIdx.x, s0 = blockIdx.x * LIN_ROWS, C4 = H >> 2;
  stage_rows(smem, ldx, x, H, s0, rows, H, tid);
  __syncthreads();
  ln_rows(smem, ldx, H, gamma, beta, eps, tid);
  __syncthreads();
  for (int idx = tid; idx < LIN_ROWS * C4; idx += 256) {
    const int row = idx / C4, c = idx - row * C4, s = s0 + row;
    if (s < rows) *(float4*)(out + (int64_t)s * H + 4 * c) = *(const float4*)(smem + row * ldx + 4 * c);
  }
}

struct LnBwdArgs {
  int rows, H;
  const float *x, *dn, *gamma;      // [rows][H], [rows][H], [H]
  float eps;
  const float* res;                 // [rows][H] or NULL: dx = res + (the LayerNorm's dx)
  float* dx;                        // [rows][H] or NULL
  float* part;                      // [workgroups][2][H] or NULL: the column sums of dn xhat and of dn over the workgroup's rows
};
inline size_t ln_bwd_lds(int H) { return (size_t)2 * LIN_ROWS * (H + AT_PAD) * sizeof(float); }

// grid ceil(rows / 64), 256 threads.  With g = dn gamma: dx = rstd (g - mean(g) - xhat mean(g xhat)), the two means summed as ln_stats
// sums; then column c of the tile is summed over rows 0 .. 63 in that order.
__global__ __launch_bounds__(256) void blk_ln_bwd_kernel(const LnBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = a.H, ldx = H + AT_PAD, tid = threadIdx.x, s0 = blockIdx.x * LIN_ROWS;
  float* xs = smem;                 // x, then dn xhat
  float* ds = xs + LIN_ROWS * ldx;  // dn
  stage_rows(xs, ldx, a.x, H, s0, a.rows, H, tid);
  stage_rows(ds, ldx, a.dn, H, s0, a.rows, H, tid);
  __syncthreads();
  const int row = tid >> 2, q = tid & 3, s = s0 + row;
  float* xrow = xs + row * ldx;
  const float* drow = ds + row * ldx;
  float mean, rstd;
  ln_stats(xrow, H, a.eps, q, mean, rstd);
  float s1 = 0.f, s2 = 0.f;
  for (int c = q; c < H; c += 4) {
    const float xh = (xrow[c] - mean) * rstd, gg = drow[c] * a.gamma[c];
    s1 += gg;
    s2 = fmaf(gg, xh, s2);
  }
  const float m1 = row4_sum(s1) / (float)H, m2 = row4_sum(s2) / (float)H;
  for (int c = q; c < H; c += 4) {
    const float xh = (xrow[c] - mean) * rstd, gg = drow[c] * a.gamma[c];
    const float d = fmaf(-xh, m2, gg - m1) * rstd;
    if (a.dx && s < a.rows) a.dx[(int64_t)s * H + c] = a.res ? a.res[(int64_t)s * H + c] + d : d;
    xrow[c] = drow[c] * xh;
  }
  __syncthreads();
  if (a.part && tid < H) {
    float sg = 0.f, sb = 0.f;
    for (int rr = 0; rr < LIN_ROWS; ++rr) {
      sg += xs[rr * ldx + tid];
      sb += ds[rr * ldx + tid];
    }
    float* p = a.part + (int64_t)blockIdx.x * 2 * H;
    p[tid] = sg;
    p[H + tid] = sb;
  }
}

// out[gi][i] = part[gi group][i] + part[gi group + 1][i] + .. (up to `group` parts, in that order), i < n; part rows have `stride`
// floats and the sum starts at float `off` of a row.  grid (ceil(n / 256), groups)
__global__ __launch_bounds__(256) void blk_sum_groups_kernel(const float* __restrict__ part, int nparts, int64_t stride, int off, int n,
                                                             int group, float* __restrict__ out, int64_t out_stride) {
  const int i = blockIdx.x * 256 + threadIdx.x, z0 = blockIdx.y * group, z1 = min(nparts, z0 + group);
  if (i >= n) return;
  float acc = part[(int64_t)z0 * stride + off + i];
  for (int z = z0 + 1; z < z1; ++z) acc += part[(int64_t)z * stride + off + i];
  out[(int64_t)blockIdx.y * out_stride + i] = acc;
}

// out = act(a), element by element
__global__ __launch_bounds__(256) void blk_act_kernel(const float* __restrict__ a, int64_t n, int act, float* __restrict__ out) {
  flat_walk<1>(n, [&](int64_t i, Width<1>) { out[i] = act_fwd(a[i], act); });
}

// ------------------------------------------------------------------------------------------------ host
int launch_ln_rows(const float* x, int rows, int H, const float* gamma, const float* beta, float eps, float* out, hipStream_t s) {
  const size_t lds = lin_lds(H);
  if (int rc = raise_lds(blk_ln_rows_kernel, lds)) return rc;
  hipLaunchKernelGGL(blk_ln_rows_kernel, dim3((rows + LIN_ROWS - 1) / LIN_ROWS), dim3(256), lds, s, x, rows, H, gamma, beta, eps, out);
  return 0;
}
inline int ln_wgs(int64_t rows) { return (int)((rows + LIN_ROWS - 1) / LIN_ROWS); }
inline int ln_groups(int64_t rows) { return (ln_wgs(rows) + BLK_GROUP - 1) / BLK_GROUP; }
// floats of the LayerNorm backward's parts: one [2][H] per workgroup, then one per group
inline int64_t ln_part_floats(int64_t rows, int H) { return (int64_t)(ln_wgs(rows) + ln_groups(rows)) * 2 * H; }
// dx (with the residual), and the ordered column sums into d_gamma / d_beta (each may be NULL)
int launch_ln_bwd(const float* x, const float* dn, const float* gamma, float eps, const float* res, int rows, int H, float* dx,
                  float* d_gamma, float* d_beta, float* part, hipStream_t s) {
  if (!dx && !d_gamma && !d_beta) return 0;
  LnBwdArgs b{};
  b.rows = rows; b.H = H; b.x = x; b.dn = dn; b.gamma = gamma; b.eps = eps; b.res = res; b.dx = dx;
  b.part = d_gamma || d_beta ? part : nullptr;
  const size_t lds = ln_bwd_lds(H);
  if (int rc = raise_lds(blk_ln_bwd_kernel, lds)) return rc;
  const int nwg = ln_wgs(rows), ngr = ln_groups(rows);
  hipLaunchKernelGGL(blk_ln_bwd_kernel, dim3(nwg), dim3(256), lds, s, b);
  if (b.part) {
    float* part2 = part + (int64_t)nwg * 2 * H;
    hipLaunchKernelGGL(blk_sum_groups_kernel, dim3((2 * H + 255) / 256, ngr), dim3(256), 0, s, part, nwg, (int64_t)2 * H, 0, 2 * H, BLK_GROUP,
                       part2, (int64_t)2 * H);
    if (d_gamma)
      hipLaunchKernelGGL(blk_sum_groups_kernel, dim3((H + 255) / 256, 1), dim3(256), 0, s, part2, ngr, (int64_t)2 * H, 0, H, ngr, d_gamma,
                         (int64_t)0);
    if (d_beta)
      hipLaunchKernelGGL(blk_sum_groups_kernel, dim3((H + 255) / 256, 1), dim3(256), 0, s, part2, ngr, (int64_t)2 * H, H, H, ngr, d_beta,
                         (int64_t)0);
  }
  return 0;
}

// dW[m, n] = sum_s da[s, m] x[s, n] and db[m] = sum_s da[s, m] over S samples, dense operands x [S][N]
void dense_weight_grad(const float* da, int lda, const float* x, int Gr, int N, int S, float* part, float* d_w, float* d_b, hipStream_t s) {
  launch_weight_grad(nullptr, 0, 1, S, da, lda, x, N, Gr, N, part, d_w, d_b, s);
}

// what a block's forward keeps: attn.hip's three tensors, u, and (training only) the pre-activation a [rows][F]
struct BlockWs {
  AttnWs at;
  int64_t u, a1, total;
};
inline BlockWs block_ws(int U, int T, int H, int heads, int F, bool train) {
  const int64_t M = (int64_t)U * T;
  BlockWs w;
  w.at = attn_ws(U, T, H, heads);
  w.u = w.at.total;
  w.a1 = w.u + scatter_index_round(M * H * 4);
  w.total = w.a1 + (train ? scatter_index_round(M * F * 4) : 0);
  return w;
}
// workspace of a block's backward: a transposed weight, two [rows][H] buffers, one [rows][max(F, 3H)], delta, the parts of the weight
// gradients (the largest tensor with its bias) and of the LayerNorm column sums
struct BlockBwdWs {
  int64_t wt, n, du, big, delta, parts, lnparts, total;
};
inline BlockBwdWs block_bwd_ws(int U, int T, int H, int heads, int F) {
  const int64_t M = (int64_t)U * T, W = std::max(F, 3 * H);
  BlockBwdWs w;
  w.wt = 0;
  w.n = scatter_index_round(W * H * 4);
  w.du = w.n + scatter_index_round(M * H * 4);
  w.big = w.du + scatter_index_round(M * H * 4);
  w.delta = w.big + scatter_index_round(M * W * 4);
  w.parts = w.delta + scatter_index_round((int64_t)U * heads * T * 4);
  w.lnparts = w.parts + scatter_index_round((int64_t)adw_nsplit(M) * W * (H + 1) * 4);
  w.total = w.lnparts + scatter_index_round(ln_part_floats(M, H) * 4);
  return w;
}

#define RECNN_BLOCK_DIMS_OK(what, hidden, n_heads, ffn, act, eps)                                                                   \
  RECNN_ATTN_DIMS_OK(what, 8, hidden, n_heads);                                                                                     \
  RECNN_REQUIRE(ffn >= 16 && ffn % 16 == 0 && ffn <= 1024, "%s: dim_feedforward must be a multiple of 16 in 16 .. 1024 (got %d)", \
                what, ffn);                                                                                                         \
  RECNN_REQUIRE(act == ACT_RELU || act == ACT_GELU, "%s: act must be 0 (relu) or 1 (gelu), got %d", what, act);                     \
  RECNN_REQUIRE(eps > 0.f, "%s: eps must be positive (got %g)", what, (double)eps)

struct BlockParams {
  const float *w_in, *b_in, *w_o, *b_o, *w1, *b1, *w2, *b2, *g1, *be1, *g2, *be2;
  bool all() const { return w_in && b_in && w_o && b_o && w1 && b1 && w2 && b2 && g1 && be1 && g2 && be2; }
};

int block_forward_impl(const char* what, const float* x, int n_users, int T, int hidden, int n_heads, int ffn, int act, int window,
                       int alibi, float eps, const BlockParams& p, float* y, void* keep, bool train, void* stream) {
  RECNN_REQUIRE(x && y && keep && p.all(), "%s: null pointer", what);
  RECNN_BLOCK_DIMS_OK(what, hidden, n_heads, ffn, act, eps);
  RECNN_ATTN_SIZE_OK(what, n_users, T);
  RECNN_REQUIRE(T >= 1 && window >= 0, "%s: need T >= 1 and window >= 0 (0: none)", what);
  RECNN_REQUIRE(x != y, "%s: y must not be x", what);
  RECNN_REQUIRE(aligned16(x, y, keep, p.w_in, p.w_o, p.w1, p.w2), "%s: x, y, the weights and the workspace / saved must be 16-byte aligned", what);
  if (n_users == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  const int H = hidden, M = n_users * T;
  const BlockWs w = block_ws(n_users, T, H, n_heads, ffn, train);
  char* kp = (char*)keep;
  float* u = (float*)(kp + w.u);
  DenseLinArgs l{};
  l.rows = M; l.K = H; l.N = 3 * H; l.x = x; l.w = p.w_in; l.ldw = H; l.b = p.b_in;
  l.gamma = p.g1; l.beta = p.be1; l.eps = eps; l.out = (float*)(kp + w.at.qkv);
  if (int rc = launch_dense_linear(l, true, s)) return rc;
  AttnArgs a = attn_args(n_users, T, H, n_heads, window, alibi);
  a.qkv = (const float*)(kp + w.at.qkv);
  a.o = (float*)(kp + w.at.o);
  a.lse = (float*)(kp + w.at.lse);
  launch_query<0>(a, s);
  DenseLinArgs o{};
  o.rows = M; o.K = H; o.N = H; o.x = a.o; o.w = p.w_o; o.ldw = H; o.b = p.b_o; o.res = x; o.out = u;
  if (int rc = launch_dense_linear(o, false, s)) return rc;
  FfnArgs f{};
  f.rows = M; f.H = H; f.F = ffn; f.act = act; f.u = u;
  f.w1 = p.w1; f.b1 = p.b1; f.w2 = p.w2; f.b2 = p.b2; f.gamma = p.g2; f.beta = p.be2; f.eps = eps;
  f.a1 = train ? (float*)(kp + w.a1) : nullptr;
  f.y = y;
  const size_t lds = ffn_lds(H);
  if (int rc = raise_lds(blk_ffn_kernel, lds)) return rc;
  hipLaunchKernelGGL(blk_ffn_kernel, dim3((M + LIN_ROWS - 1) / LIN_ROWS), dim3(256), lds, s, f);
  return recnn_check_hip(hipGetLastError(), what);
}

struct BlockGrads {
  float *w_in, *b_in, *w_o, *b_o, *w1, *b1, *w2, *b2, *g1, *be1, *g2, *be2;
};

int block_backward_impl(const float* x, int n_users, int T, int hidden, int n_heads, int ffn, int act, int window, int alibi, float eps,
                        const BlockParams& p, const void* saved, const float* g_y, float* d_x, const BlockGrads& d, void* workspace,
                        void* stream) {
  const char* what = "block_backward";
  RECNN_REQUIRE(x && saved && g_y && workspace && p.all(), "%s: null pointer", what);
  RECNN_BLOCK_DIMS_OK(what, hidden, n_heads, ffn, act, eps);
  RECNN_ATTN_SIZE_OK(what, n_users, T);
  RECNN_REQUIRE(T >= 1 && window >= 0, "%s: need T >= 1 and window >= 0 (0: none)", what);
  RECNN_REQUIRE(aligned16(x, saved, g_y, d_x, workspace, p.w_in, p.w_o, p.w1, p.w2),
                "%s: x, saved, g_y, d_x, the weights and workspace must be 16-byte aligned", what);
  if (n_users == 0) return 0;       // (the caller's gradients of an empty batch are its own zeros)
  const hipStream_t s = (hipStream_t)stream;
  const int H = hidden, F = ffn, M = n_users * T;
  const BlockWs sv = block_ws(n_users, T, H, n_heads, F, true);
  const BlockBwdWs w = block_bwd_ws(n_users, T, H, n_heads, F);
  const char* sp = (const char*)saved;
  char* ws = (char*)workspace;
  const float* u = (const float*)(sp + sv.u);
  const float* a1 = (const float*)(sp + sv.a1);
  const float* o = (const float*)(sp + sv.at.o);
  float* wt = (float*)(ws + w.wt);
  float* nb = (float*)(ws + w.n);
  float* du = (float*)(ws + w.du);
  float* big = (float*)(ws + w.big);
  float* part = (float*)(ws + w.parts);
  float* lnpart = (float*)(ws + w.lnparts);
  const bool need_ln1 = d_x || d.g1 || d.be1;
  const bool need_attn = need_ln1 || d.w_in || d.b_in;
  const bool need_du = need_attn || d.w_o || d.b_o || d.g2 || d.be2;
  const bool need_da1 = need_du || d.w1 || d.b1;
  auto transpose = [&](const float* wsrc, int rows_out, int cols_out) {      // wsrc [cols_out][rows_out] -> wt [rows_out][cols_out]
    hipLaunchKernelGGL(whh_transpose_kernel, dim3(grid_for((int64_t)rows_out * cols_out, 256, 2048)), dim3(256), 0, s, wsrc, rows_out,
                       cols_out, wt);
  };
  // the feed-forward: d_w2[h, f] = sum_s g_y[s, h] act(a)[s, f], d_b2
  if (d.w2 || d.b2) {
    if (d.w2) hipLaunchKernelGGL(blk_act_kernel, dim3(grid_for((int64_t)M * F, 256, 4096)), dim3(256), 0, s, a1, (int64_t)M * F, act, big);
    dense_weight_grad(g_y, H, big, H, F, M, part, d.w2, d.b2, s);
  }
  if (!need_da1) return recnn_check_hip(hipGetLastError(), what);
  // d_a = (g_y W_2) act'(a)   [rows][F]
  transpose(p.w2, F, H);
  DenseLinArgs l{};
  l.rows = M; l.K = H; l.N = F; l.x = g_y; l.w = wt; l.ldw = H; l.aux = a1; l.act = act; l.out = big;
  if (int rc = launch_dense_linear(l, false, s)) return rc;
  if (d.w1 || d.b1) {
    if (d.w1)
      if (int rc = launch_ln_rows(u, M, H, p.g2, p.be2, eps, nb, s)) return rc;
    dense_weight_grad(big, F, nb, F, H, M, part, d.w1, d.b1, s);
  }
  if (!need_du) return recnn_check_hip(hipGetLastError(), what);
  // d(LN2 u) = d_a W_1, then d_u = g_y + LN2's backward
  transpose(p.w1, H, F);
  l = DenseLinArgs{};
  l.rows = M; l.K = F; l.N = H; l.x = big; l.w = wt; l.ldw = F; l.out = nb;
  if (int rc = launch_dense_linear(l, false, s)) return rc;
  if (int rc = launch_ln_bwd(u, nb, p.g2, eps, g_y, M, H, du, d.g2, d.be2, lnpart, s)) return rc;
  // the out-projection
  dense_weight_grad(du, H, o, H, H, M, part, d.w_o, d.b_o, s);
  if (!need_attn) return recnn_check_hip(hipGetLastError(), what);
  transpose(p.w_o, H, H);
  l = DenseLinArgs{};
  l.rows = M; l.K = H; l.N = H; l.x = du; l.w = wt; l.ldw = H; l.out = nb;          // dO
  if (int rc = launch_dense_linear(l, false, s)) return rc;
  AttnArgs a = attn_args(n_users, T, H, n_heads, window, alibi);
  a.qkv = (const float*)(sp + sv.at.qkv);
  a.lse = (float*)(sp + sv.at.lse);                  // (read only)
  a.d_o = nb;
  a.delta = (const float*)(ws + w.delta);
  a.delta_out = (float*)(ws + w.delta);
  a.dqkv = big;
  launch_query<1>(a, s);
  launch_key(a, s);
  launch_query<2>(a, s);
  // the in-projection: LN1(x) recomputed for d_w_in
  if (d.w_in || d.b_in) {
    if (d.w_in)
      if (int rc = launch_ln_rows(x, M, H, p.g1, p.be1, eps, nb, s)) return rc;
    dense_weight_grad(big, 3 * H, nb, 3 * H, H, M, part, d.w_in, d.b_in, s);
  }
  if (!need_ln1) return recnn_check_hip(hipGetLastError(), what);
  transpose(p.w_in, H, 3 * H);
  l = DenseLinArgs{};
  l.rows = M; l.K = 3 * H; l.N = H; l.x = big; l.w = wt; l.ldw = 3 * H; l.out = nb;
  if (int rc = launch_dense_linear(l, false, s)) return rc;
  if (int rc = launch_ln_bwd(x, nb, p.g1, eps, du, M, H, d_x, d.g1, d.be1, lnpart, s)) return rc;
  return recnn_check_hip(hipGetLastError(), what);
}

// ------------------------------------------------------------------------------------------------ embedding
int seq_embed_backward_impl(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users, int t0,
                            int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_e, const float* g_x,
                            float* d_w_e, float* d_b_e, float* d_table, bool with_table, void* workspace, void* table_workspace,
                            void* stream) {
  const char* what = with_table ? "seq_embed_backward_table" : "seq_embed_backward";
  if (with_table) RECNN_REQUIRE(d_table && w_e && table_workspace, "%s: null pointer (d_table, w_e, table_workspace)", what);
  RECNN_REQUIRE(store_ok(items, ratings, user_off, slots, table) && g_x && workspace, "%s: null pointer", what);
  RECNN_LSTM_DIMS_OK(what, emb_dim, hidden);
  RECNN_ATTN_SIZE_OK(what, n_users, T);
  RECNN_REQUIRE(t0 >= 0 && T >= 1 && n_items > 0, "%s: need t0 >= 0, T >= 1 and n_items > 0", what);
  RECNN_REQUIRE(aligned16(table, g_x, workspace), "%s: table, g_x and workspace must be 16-byte aligned", what);
  if (with_table) RECNN_REQUIRE(aligned16(d_table, table_workspace), "%s: d_table and table_workspace must be 16-byte aligned", what);
  const hipStream_t s = (hipStream_t)stream;
  if (n_users == 0) {
    if (with_table) RECNN_HIP(hipMemsetAsync(d_table, 0, (size_t)n_items * emb_dim * sizeof(float), s));
    return 0;
  }
  const int H = hidden, S = n_users * T;
  const SeqStore st{items, ratings, user_off, slots, n_users, table, n_items, emb_dim};
  if (with_table) {
    TableGrad tg{};
    RECNN_HIP(table_grad_prepare(tg, st, t0, T, H, H, T, g_x, w_e, table_workspace, s));
    table_grad_chunk(tg, 0, T, s);
    table_grad_finish(tg, d_table, s);
  }
  launch_weight_grad(&st, t0, T, S, g_x, H, nullptr, emb_dim, H, emb_dim, (float*)workspace, d_w_e, d_b_e, s);
  return recnn_check_hip(hipGetLastError(), what);
}

}  // namespace

extern "C" int recnn_seq_embed(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users, int t0,
                               int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_e, const float* b_e,
                               float* x_out, void* stream) {
  const char* what = "seq_embed";
  RECNN_REQUIRE(store_ok(items, ratings, user_off, slots, table) && w_e && b_e && x_out, "%s: null pointer", what);
  RECNN_LSTM_DIMS_OK(what, emb_dim, hidden);
  RECNN_ATTN_SIZE_OK(what, n_users, T);
  RECNN_REQUIRE(t0 >= 0 && T >= 1 && n_items > 0, "%s: need t0 >= 0, T >= 1 and n_items > 0", what);
  RECNN_REQUIRE(aligned16(table, x_out), "%s: table and x_out must be 16-byte aligned", what);
  if (n_users == 0) return 0;
  LinArgs l{};
  l.s = SeqStore{items, ratings, user_off, slots, n_users, table, n_items, emb_dim};
  l.t0 = t0; l.T = T; l.rows = n_users * T;
  l.K = emb_dim; l.w = w_e; l.ldw = emb_dim + 1; l.b = b_e;
  l.out = x_out; l.N = hidden;
  if (int rc = launch_linear(l, (hipStream_t)stream)) return rc;
  return recnn_check_hip(hipGetLastError(), what);
}

extern "C" int recnn_seq_embed_backward_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int64_t* bytes) {
  const char* what = "seq_embed_backward_workspace_bytes";
  RECNN_REQUIRE(bytes, "%s: null pointer", what);
  RECNN_LSTM_DIMS_OK(what, emb_dim, hidden);
  RECNN_ATTN_SIZE_OK(what, n_users, T);
  *bytes = scatter_index_round((int64_t)adw_nsplit((int64_t)n_users * T) * hidden * (emb_dim + 2) * 4);
  return 0;
}

extern "C" int recnn_seq_embed_backward(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                                        int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden,
                                        const float* g_x, float* d_w_e, float* d_b_e, void* workspace, void* stream) {
  return seq_embed_backward_impl(items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, nullptr, g_x, d_w_e,
                                 d_b_e, nullptr, false, workspace, nullptr, stream);
}

extern "C" int recnn_seq_embed_table_grad_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int n_items, int64_t* bytes) {
  const char* what = "seq_embed_table_grad_workspace_bytes";
  RECNN_REQUIRE(bytes, "%s: null pointer", what);
  RECNN_LSTM_DIMS_OK(what, emb_dim, hidden);
  RECNN_REQUIRE(n_users >= 0 && T >= 0 && n_items >= 1 && (int64_t)n_users * T < (1LL << 31),
                "%s: need n_users >= 0, T >= 0, n_items >= 1 and n_users * T < 2^31", what);
  *bytes = table_ws(n_users, T, hidden, emb_dim, n_items).total;
  return 0;
}

extern "C" int recnn_seq_embed_backward_table(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                                              int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden,
                                              const float* w_e, const float* g_x, float* d_w_e, float* d_b_e, float* d_table,
                                              void* workspace, void* table_workspace, void* stream) {
  return seq_embed_backward_impl(items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, w_e, g_x, d_w_e, d_b_e,
                                 d_table, true, workspace, table_workspace, stream);
}

extern "C" int recnn_block_workspace_bytes(int n_users, int T, int hidden, int n_heads, int64_t* bytes) {
  const char* what = "block_workspace_bytes";
  RECNN_REQUIRE(bytes, "%s: null pointer", what);
  RECNN_ATTN_DIMS_OK(what, 8, hidden, n_heads);
  RECNN_ATTN_SIZE_OK(what, n_users, T);
  *bytes = block_ws(n_users, T, hidden, n_heads, 0, false).total;
  return 0;
}

extern "C" int recnn_block_forward(const float* x, int n_users, int T, int hidden, int n_heads, int ffn, int act, int window, int alibi,
                                   float eps, const float* w_in, const float* b_in, const float* w_o, const float* b_o, const float* w1,
                                   const float* b1, const float* w2, const float* b2, const float* g1, const float* be1, const float* g2,
                                   const float* be2, float* y, void* workspace, void* stream) {
  return block_forward_impl("block_forward", x, n_users, T, hidden, n_heads, ffn, act, window, alibi, eps,
                            BlockParams{w_in, b_in, w_o, b_o, w1, b1, w2, b2, g1, be1, g2, be2}, y, workspace, false, stream);
}

// One block on the n new steps of n_rows sessions: recnn_block_forward's launches on x [n_rows, n, hidden], with the
// attention reading its keys and values from this layer's cache `kv`, which first receives the new rows' k and v.
extern "C" int recnn_block_append(const float* x, int n_rows, int n, int hidden, int n_heads, int ffn, int act, int window, int alibi,
                                  float eps, const float* w_in, const float* b_in, const float* w_o, const float* b_o, const float* w1,
                                  const float* b1, const float* w2, const float* b2, const float* g1, const float* be1, const float* g2,
                                  const float* be2, float* kv, int n_sessions, int capacity, const int32_t* pos, const int32_t* rows,
                                  float* y, void* workspace, void* stream) {
  const char* what = "block_append";
  const BlockParams p{w_in, b_in, w_o, b_o, w1, b1, w2, b2, g1, be1, g2, be2};
  RECNN_REQUIRE(x && y && workspace && p.all(), "%s: null pointer", what);
  RECNN_BLOCK_DIMS_OK(what, hidden, n_heads, ffn, act, eps);
  RECNN_KV_CACHE_OK(what, n_rows, n, n_sessions, capacity, window, kv, pos, rows);
  RECNN_REQUIRE(x != y, "%s: y must not be x", what);
  RECNN_REQUIRE(aligned16(x, y, workspace, p.w_in, p.w_o, p.w1, p.w2), "%s: x, y, the weights and the workspace must be 16-byte aligned", what);
  if (n_rows == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  const int H = hidden, M = n_rows * n;
  const AppendWs w = append_ws(n_rows, n, H);
  char* ws = (char*)workspace;
  float* qkv = (float*)(ws + w.qkv);
  float* o = (float*)(ws + w.o);
  float* u = (float*)(ws + w.u);
  DenseLinArgs l{};
  l.rows = M; l.K = H; l.N = 3 * H; l.x = x; l.w = p.w_in; l.ldw = H; l.b = p.b_in;
  l.gamma = p.g1; l.beta = p.be1; l.eps = eps; l.out = qkv;
  if (int rc = launch_dense_linear(l, true, s)) return rc;
  launch_cache_attention(qkv, o, n_rows, n, H, n_heads, window, alibi, kv, n_sessions, capacity, pos, rows, s);
  DenseLinArgs ol{};
  ol.rows = M; ol.K = H; ol.N = H; ol.x = o; ol.w = p.w_o; ol.ldw = H; ol.b = p.b_o; ol.res = x; ol.out = u;
  if (int rc = launch_dense_linear(ol, false, s)) return rc;
  FfnArgs f{};
  f.rows = M; f.H = H; f.F = ffn; f.act = act; f.u = u;
  f.w1 = p.w1; f.b1 = p.b1; f.w2 = p.w2; f.b2 = p.b2; f.gamma = p.g2; f.beta = p.be2; f.eps = eps;
  f.y = y;
  if (M <= FFN_FEW_ROWS) {
    hipLaunchKernelGGL(blk_ffn_rows16_kernel, dim3((M + FFR - 1) / FFR), dim3(256), ffn_rows16_lds(H), s, f);
  } else {
    const size_t lds = ffn_lds(H);
    if (int rc = raise_lds(blk_ffn_kernel, lds)) return rc;
    hipLaunchKernelGGL(blk_ffn_kernel, dim3((M + LIN_ROWS - 1) / LIN_ROWS), dim3(256), lds, s, f);
  }
  return recnn_check_hip(hipGetLastError(), what);
}

extern "C" int recnn_block_train_workspace_bytes(int n_users, int T, int hidden, int n_heads, int ffn, int64_t* saved_bytes,
                                                 int64_t* bwd_bytes) {
  const char* what = "block_train_workspace_bytes";
  RECNN_REQUIRE(saved_bytes && bwd_bytes, "%s: null pointer", what);
  RECNN_BLOCK_DIMS_OK(what, hidden, n_heads, ffn, 0, 1.f);
  RECNN_ATTN_SIZE_OK(what, n_users, T);
  *saved_bytes = block_ws(n_users, T, hidden, n_heads, ffn, true).total;
  *bwd_bytes = block_bwd_ws(n_users, T, hidden, n_heads, ffn).total;
  return 0;
}

extern "C" int recnn_block_forward_train(const float* x, int n_users, int T, int hidden, int n_heads, int ffn, int act, int window,
                                         int alibi, float eps, const float* w_in, const float* b_in, const float* w_o, const float* b_o,
                                         const float* w1, const float* b1, const float* w2, const float* b2, const float* g1,
                                         const float* be1, const float* g2, const float* be2, float* y, void* saved, void* stream) {
  return block_forward_impl("block_forward_train", x, n_users, T, hidden, n_heads, ffn, act, window, alibi, eps,
                            BlockParams{w_in, b_in, w_o, b_o, w1, b1, w2, b2, g1, be1, g2, be2}, y, saved, true, stream);
}

extern "C" int recnn_block_backward(const float* x, int n_users, int T, int hidden, int n_heads, int ffn, int act, int window, int alibi,
                                    float eps, const float* w_in, const float* b_in, const float* w_o, const float* b_o, const float* w1,
                                    const float* b1, const float* w2, const float* b2, const float* g1, const float* be1, const float* g2,
                                    const float* be2, const void* saved, const float* g_y, float* d_x, float* d_w_in, float* d_b_in,
                                    float* d_w_o, float* d_b_o, float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* d_g1,
                                    float* d_be1, float* d_g2, float* d_be2, void* workspace, void* stream) {
  return block_backward_impl(x, n_users, T, hidden, n_heads, ffn, act, window, alibi, eps,
                             BlockParams{w_in, b_in, w_o, b_o, w1, b1, w2, b2, g1, be1, g2, be2}, saved, g_y, d_x,
                             BlockGrads{d_w_in, d_b_in, d_w_o, d_b_o, d_w1, d_b1, d_w2, d_b2, d_g1, d_be1, d_g2, d_be2}, workspace, stream);
}

#define RECNN_LN_ROWS_OK(what, rows, hidden)                                                                                       \
  RECNN_REQUIRE(hidden >= 16 && hidden % 16 == 0 && hidden <= 256, "%s: hidden must be a multiple of 16 up to 256 (got %d)", what, \
                hidden);                                                                                                           \
  RECNN_REQUIRE(rows >= 0, "%s: rows must not be negative", what)

extern "C" int recnn_layernorm_rows(const float* x, int rows, int hidden, const float* gamma, const float* beta, float eps, float* out,
                                    void* stream) {
  const char* what = "layernorm_rows";
  RECNN_REQUIRE(x && gamma && beta && out, "%s: null pointer", what);
  RECNN_LN_ROWS_OK(what, rows, hidden);
  RECNN_REQUIRE(eps > 0.f, "%s: eps must be positive (got %g)", what, (double)eps);
  RECNN_REQUIRE(aligned16(x, out), "%s: x and out must be 16-byte aligned", what);
  if (rows == 0) return 0;
  if (int rc = launch_ln_rows(x, rows, hidden, gamma, beta, eps, out, (hipStream_t)stream)) return rc;
  return recnn_check_hip(hipGetLastError(), what);
}

extern "C" int recnn_layernorm_rows_backward_workspace_bytes(int rows, int hidden, int64_t* bytes) {
  const char* what = "layernorm_rows_backward_workspace_bytes";
  RECNN_REQUIRE(bytes, "%s: null pointer", what);
  RECNN_LN_ROWS_OK(what, rows, hidden);
  *bytes = scatter_index_round(ln_part_floats(rows, hidden) * 4);
  return 0;
}

extern "C" int recnn_layernorm_rows_backward(const float* x, int rows, int hidden, const float* gamma, float eps, const float* g_out,
                                             float* d_x, float* d_gamma, float* d_beta, void* workspace, void* stream) {
  const char* what = "layernorm_rows_backward";
  RECNN_REQUIRE(x && gamma && g_out && workspace, "%s: null pointer", what);
  RECNN_LN_ROWS_OK(what, rows, hidden);
  RECNN_REQUIRE(eps > 0.f, "%s: eps must be positive (got %g)", what, (double)eps);
  RECNN_REQUIRE(aligned16(x, g_out, d_x, workspace), "%s: x, g_out, d_x and workspace must be 16-byte aligned", what);
  if (rows == 0) return 0;
  if (int rc = launch_ln_bwd(x, g_out, gamma, eps, nullptr, rows, hidden, d_x, d_gamma, d_beta, (float*)workspace, (hipStream_t)stream))
    return rc;
  return recnn_check_hip(hipGetLastError(), what);
}
