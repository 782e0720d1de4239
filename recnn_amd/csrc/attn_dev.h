// attn_dev.h -- the device half of the causal self-attention encoder, shared by attn.hip (the layer over the store)
// and block.hip (the same layer on a dense [U, T, H] input inside a transformer block): the two 64-row linear kernels, the
// attention kernels with their arguments, the attention of appended steps over a per-session KV cache, the segmented
// weight-gradient tile, the workspace layouts and the launchers.  attn.hip describes the layer and the attention kernels.
//
//   linear kernels   out[s, n] = b[n] + sum_k x[s, k] w[n, k] for 64 rows s per workgroup, one fixed-order chain per element on the
//                    exact-f32 MFMA: the bias first, then k upwards in blocks of 16, MFMA e = 0 .. 3 inside a block.  Two kernels:
//     gathered       (attn_linear_kernel) the rows are [table[item] | rating] read through the store -- [U, T, E] is never
//                    materialised -- and the chain starts with fma(rating, w[n, E], b[n]), the rank-1 link of seq_chain.h (K = E + 1
//                    is never padded).  The in-projection of attn.hip and the embedding of block.hip.
//     dense          (dense_linear_kernel<LN>) the rows are x [rows][K]; every other product of both encoders, those with a
//                    transposed weight (over a transposed copy) included.  A workgroup owns 64 rows and 256 columns, wave w column
//                    tiles w, w + 4, w + 8, w + 12 of them, so a staged row block is read once for four column tiles.  K > 256 is
//                    staged in blocks of 256, upwards, into the same accumulators (still one chain per element).  LN: the staged
//                    rows are normalised in place before the products (ln_rows), so the no-grad encode writes no normalised copy.
//                    Two epilogues: out = res + acc (the residual link; the chain is finished before the residual is added) and
//                    out = acc act'(aux) (the activation's derivative at the saved pre-activation).
#pragma once
#include <algorithm>

#include "seq_bwd.h"

namespace {

constexpr int AT_Q = 64;            // query rows per workgroup, keys per tile
constexpr int AT_PAD = 4;
constexpr int AT_MAXHEADS = 16;
constexpr int LIN_ROWS = 64;

__device__ __forceinline__ float neg_inf() { return -__builtin_inff(); }

// ------------------------------------------------------------------------------------------------ gathered linear
struct LinArgs {
  SeqStore s;                       // x rows are [table[item] | rating] through the store
  int t0, T;
  int rows;                         // samples s = u T + t
  int K;                            // contraction width without the rating column (a multiple of 8)
  const float* w;                   // [N][ldw]
  int ldw;
  const float* b;                   // [N] or NULL
  float* out;                       // [rows][N]
  int N;                            // a multiple of 16
};

inline size_t lin_lds(int K) { return (size_t)(LIN_ROWS * (((K + 15) & ~15) + AT_PAD) + LIN_ROWS) * sizeof(float); }

// grid ceil(rows / 64), 256 threads; wave w owns column tiles w, w + 4, ..
__global__ __launch_bounds__(256) void attn_linear_kernel(const LinArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int K = a.K, KX = (K + 15) & ~15, ldx = KX + AT_PAD, C4 = KX >> 2;
  float* xs = smem;                 // [64][ldx]
  float* rs = xs + LIN_ROWS * ldx;  // [64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int s0 = blockIdx.x * LIN_ROWS;
  for (int idx = tid; idx < LIN_ROWS * C4; idx += 256) {
    const int row = idx / C4, c = idx - row * C4, s = s0 + row;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s < a.rows && 4 * c < K) {
      const int u = s / a.T, t = s - u * a.T;
      const StorePos p = store_pos(a.s, u, a.t0 + t);
      v = p.live() ? table_chunk(a.s, a.s.items[p.pos], c) : nan4();
      if (c == 0) rs[row] = p.live() ? a.s.ratings[p.pos] : __builtin_nanf("");
    } else if (c == 0) {
      rs[row] = 0.f;
    }
    *(float4*)(xs + row * ldx + 4 * c) = v;
  }
  __syncthreads();
  const int ntiles = a.N >> 4;
  for (int jt = wave; jt < ntiles; jt += 4) {
    const int col = jt * 16 + r;
    const float* wrow = a.w + (int64_t)col * a.ldw;
    const float bias = a.b ? a.b[col] : 0.f;
    f32x4 acc[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[mt][i] = fmaf(rs[16 * mt + 4 * g + i], wrow[K], bias);
    for (int k0 = 0; k0 < K; k0 += 16) {
      const bool kin = k0 + 4 * g < K;        // K a multiple of 8: the last k block may be half empty (x there is zero)
      const f32x4 bv = kin ? (f32x4)(*(const f32x4u*)(wrow + k0 + 4 * g)) : f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 av[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) av[mt] = *(const f32x4*)(xs + (16 * mt + r) * ldx + k0 + 4 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][e], bv[e], acc[mt], 0, 0, 0);
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int s = s0 + 16 * mt + 4 * g + i;
        if (s < a.rows) a.out[(int64_t)s * a.N + col] = acc[mt][i];
      }
  }
}

// ------------------------------------------------------------------------------------------------ rows in LDS
constexpr int LIN_KB = 256;         // contraction columns per LDS stage of the dense linear kernel
constexpr int LIN_COLS = 256;       // output columns per workgroup of the dense linear kernel

enum { ACT_RELU = 0, ACT_GELU = 1 };

__device__ __forceinline__ float act_fwd(float a, int act) {
  if (act == ACT_RELU) return a < 0.f ? 0.f : a;                   // (a NaN stays a NaN)
  return 0.5f * a * (1.f + erff(a * 0.70710678118654752440f));
}
__device__ __forceinline__ float act_grad(float a, int act) {
  if (act == ACT_RELU) return a > 0.f ? 1.f : (a != a ? a : 0.f);
  const float cdf = 0.5f * (1.f + erff(a * 0.70710678118654752440f));
  return fmaf(a * 0.39894228040143267794f, expf(-0.5f * a * a), cdf);      // Phi(a) + a phi(a)
}

// rows s0 .. s0 + 63 of x [rows][ld], columns 0 .. kw - 1 (a multiple of 4), into xs [64][ldx]; rows at or past `rows` are zeros
__device__ __forceinline__ void stage_rows(float* xs, int ldx, const float* x, int64_t ld, int s0, int rows, int kw, int tid) {
  const int C4 = kw >> 2;
  for (int idx = tid; idx < LIN_ROWS * C4; idx += 256) {
    const int row = idx / C4, c = idx - row * C4, s = s0 + row;
    *(float4*)(xs + row * ldx + 4 * c) = s < rows ? *(const float4*)(x + (int64_t)s * ld + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
__device__ __forceinline__ float row4_sum(float v) {      // the sum over the four lanes of a row, in every one of them
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v;
}
// mean and 1 / sqrt(var + eps) of a row of K values in LDS; lane q of the row's four (tid & 3)
__device__ __forceinline__ void ln_stats(const float* xrow, int K, float eps, int q, float& mean, float& rstd) {
  float s = 0.f;
  for (int c = q; c < K; c += 4) s += xrow[c];
  mean = row4_sum(s) / (float)K;
  float v = 0.f;
  for (int c = q; c < K; c += 4) {
    const float d = xrow[c] - mean;
    v = fmaf(d, d, v);
  }
  rstd = 1.f / sqrtf(row4_sum(v) / (float)K + eps);
}
// xs [64][ldx] -> LN(xs) in place; thread tid owns columns (tid & 3) + 4 i of row tid >> 2.  The caller puts a barrier on both sides.
__device__ __forceinline__ void ln_rows(float* xs, int ldx, int K, const float* gamma, const float* beta, float eps, int tid) {
  float* xrow = xs + (tid >> 2) * ldx;
  const int q = tid & 3;
  float mean, rstd;
  ln_stats(xrow, K, eps, q, mean, rstd);
  for (int c = q; c < K; c += 4) xrow[c] = fmaf((xrow[c] - mean) * rstd, gamma[c], beta[c]);
}

// ------------------------------------------------------------------------------------------------ dense linear
struct DenseLinArgs {
  int rows, K, N;                   // K and N multiples of 16
  const float* x;                   // [rows][K]
  const float* w;                   // [N][ldw]
  int ldw;
  const float* b;                   // [N] or NULL
  const float *gamma, *beta;        // LN: [K], K <= LIN_KB
  float eps;
  const float* res;                 // [rows][N] or NULL: out = res + acc
  const float* aux;                 // [rows][N] or NULL: out = acc act'(aux)
  int act;
  float* out;                       // [rows][N]
};
inline size_t dense_lin_lds(int K) { return (size_t)LIN_ROWS * (std::min(K, LIN_KB) + AT_PAD) * sizeof(float); }

// grid (ceil(rows / 64), ceil(N / 256)), 256 threads
template <bool LN>
__global__ __launch_bounds__(256) void dense_linear_kernel(const DenseLinArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int K = a.K, KB = K < LIN_KB ? K : LIN_KB, ldx = KB + AT_PAD;
  float* xs = smem;                 // [64][ldx]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int s0 = blockIdx.x * LIN_ROWS;
  const int ntiles = a.N >> 4, jt0 = blockIdx.y * (LIN_COLS / 16) + wave;
  f32x4 acc[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool on = jt0 + 4 * j < ntiles;
    const float bias = on && a.b ? a.b[(jt0 + 4 * j) * 16 + r] : 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[j][mt] = f32x4{bias, bias, bias, bias};
  }
  for (int kb = 0; kb < K; kb += KB) {
    const int kw = min(KB, K - kb);
    if (kb) __syncthreads();
    stage_rows(xs, ldx, a.x + kb, K, s0, a.rows, kw, tid);
    __syncthreads();
    if constexpr (LN) {
      ln_rows(xs, ldx, K, a.gamma, a.beta, a.eps, tid);
      __syncthreads();
    }
    for (int k0 = 0; k0 < kw; k0 += 16) {
      f32x4 av[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) av[mt] = *(const f32x4*)(xs + (16 * mt + r) * ldx + k0 + 4 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (jt0 + 4 * j >= ntiles) continue;                    // (wave-uniform)
        const f32x4 bv = *(const f32x4*)(a.w + (int64_t)((jt0 + 4 * j) * 16 + r) * a.ldw + kb + k0 + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) acc[j][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][e], bv[e], acc[j][mt], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (jt0 + 4 * j >= ntiles) continue;
    const int col = (jt0 + 4 * j) * 16 + r;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int s = s0 + 16 * mt + 4 * g + i;
        if (s >= a.rows) continue;
        const int64_t at = (int64_t)s * a.N + col;
        float v = acc[j][mt][i];
        if (a.res) v = a.res[at] + v;
        if (a.aux) v = v * act_grad(a.aux[at], a.act);
        a.out[at] = v;
      }
  }
}

// ------------------------------------------------------------------------------------------------ attention
struct AttnArgs {
  int U, T, H, heads, window;       // window: 1 .. T (T: no window)
  float scale;                      // 1 / sqrt(d)
  float slope[AT_MAXHEADS];
  const float* qkv;                 // [U][T][3H]
  float* o;                         // [U][T][H]
  float* lse;                       // [2][U][heads][T]: the log-sum-exp of a row in two parts, its maximum m and the sum l of exp(s - m)
  const float* d_o;                 // backward: [U][T][H]
  const float* delta;               // backward: [U][heads][T]
  float* delta_out;                 // MODE 1 writes it
  float* dqkv;                      // backward: [U][T][3H]
};

// a 64 x D tile of rows t0 .. t0 + 63 of one head's columns (src points at row 0 of the user, the head's first column; row stride ld)
// into LDS [64][D + 4]; rows at or past T are zeros
template <int D>
__device__ __forceinline__ void stage_tile(float* dst, const float* src, int64_t ld, int t0, int T, int tid) {
  constexpr int C4 = D / 4, LD = D + AT_PAD;
  for (int idx = tid; idx < AT_Q * C4; idx += 256) {
    const int row = idx / C4, c = idx - row * C4, t = t0 + row;
    *(float4*)(dst + row * LD + 4 * c) = t < T ? *(const float4*)(src + (int64_t)t * ld + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__device__ __forceinline__ float fold4(float v) {   // the sum over the four lane groups of a query, in every lane
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// grid (query blocks, heads, users), 256 threads.  MODE 0: the forward, o and the log-sum-exp.  MODE 1 and 2: the query owner of the
// backward -- 1: delta[t] = sum_j p(t, j) dP(t, j), 2: dQ.
template <int D, int MODE>
__global__ __launch_bounds__(256) void attn_query_kernel(const AttnArgs a) {
  constexpr int LD = D + AT_PAD, DT = D / 16;
  constexpr bool BWD = MODE != 0;
  __shared__ __attribute__((aligned(16))) float Ks[AT_Q * LD];
  __shared__ __attribute__((aligned(16))) float Vs[AT_Q * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int qb = gridDim.x - 1 - blockIdx.x, head = blockIdx.y, u = blockIdx.z;      // the heaviest blocks first
  const int T = a.T, H = a.H, H3 = 3 * H, w = a.window;
  const int q0 = qb * AT_Q, tq = q0 + 16 * wave + r;   // the lane's query
  const bool qlive = tq < T;
  const float* base = a.qkv + (int64_t)u * T * H3 + head * D;
  const float slope = a.slope[head], scale = a.scale;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 qf[DT];
  [[maybe_unused]] f32x4 dof[DT];
#pragma unroll
  for (int kb = 0; kb < DT; ++kb) {
    qf[kb] = qlive ? *(const f32x4*)(base + (int64_t)tq * H3 + 16 * kb + 4 * g) : zero4;
    if constexpr (BWD) dof[kb] = qlive ? *(const f32x4*)(a.d_o + ((int64_t)u * T + tq) * H + head * D + 16 * kb + 4 * g) : zero4;
  }
  const int64_t lplane = (int64_t)a.U * a.heads * T;          // l sits one plane behind m
  [[maybe_unused]] float m_q = 0.f, il_q = 0.f, delta_q = 0.f;
  if constexpr (BWD) {
    if (qlive) {
      m_q = a.lse[((int64_t)u * a.heads + head) * T + tq];
      il_q = 1.f / a.lse[lplane + ((int64_t)u * a.heads + head) * T + tq];
      if constexpr (MODE == 2) delta_q = a.delta[((int64_t)u * a.heads + head) * T + tq];
    }
  }
  f32x4 oacc[DT];                    // O^T (BWD: dQ^T): columns 16 dt + 4 g + i of query tq
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) oacc[dt] = zero4;
  float m = neg_inf(), l = 0.f;
  [[maybe_unused]] float dsum = 0.f;
  const int tq_lo = q0 + 16 * wave, tq_hi = tq_lo + 15;      // the wave's rows
  const int tile_lo = max(0, q0 - w + 1) / AT_Q;

  for (int kt = tile_lo; kt <= qb; ++kt) {
    const int k0 = kt * AT_Q;
    __syncthreads();
    stage_tile<D>(Ks, base + H, H3, k0, T, tid);
    stage_tile<D>(Vs, base + 2 * H, H3, k0, T, tid);
    __syncthreads();
    if (k0 > tq_hi || k0 + AT_Q - 1 < tq_lo - w + 1) continue;      // nothing of the tile is in the wave's reach (wave-uniform)
    f32x4 s[4] = {zero4, zero4, zero4, zero4};
    [[maybe_unused]] f32x4 dp[4] = {zero4, zero4, zero4, zero4};
#pragma unroll
    for (int kb = 0; kb < DT; ++kb) {
      f32x4 kf[4];
      [[maybe_unused]] f32x4 vf[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        kf[c] = *(const f32x4*)(Ks + (16 * c + r) * LD + 16 * kb + 4 * g);
        if constexpr (BWD) vf[c] = *(const f32x4*)(Vs + (16 * c + r) * LD + 16 * kb + 4 * g);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          s[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[c][e], qf[kb][e], s[c], 0, 0, 0);
          if constexpr (BWD) dp[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[c][e], dof[kb][e], dp[c], 0, 0, 0);
        }
    }
    // s[c][i]: key k0 + 16 c + 4 g + i against query tq
    if constexpr (!BWD) {
      float tmax = neg_inf();
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int dist = tq - (k0 + 16 * c + 4 * g + i);
          const bool valid = dist >= 0 && dist < w;
          const float sc = valid ? fmaf(-slope, (float)dist, s[c][i] * scale) : neg_inf();
          s[c][i] = sc;
          tmax = fmaxf(tmax, sc);
        }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float m_new = fmaxf(m, tmax);
      const float m_use = m_new == neg_inf() ? 0.f : m_new;       // a row nothing has reached yet: exp(-inf - 0) = 0, never inf - inf
      const float alpha = expf(m - m_use);
      float psum = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = expf(s[c][i] - m_use);
          s[c][i] = p;
          psum += p;
        }
      psum = fold4(psum);
      l = fmaf(l, alpha, psum);
      m = m_new;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) oacc[dt] *= alpha;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int dist = tq - (k0 + 16 * c + 4 * g + i);
          const bool valid = qlive && dist >= 0 && dist < w;
          const float sc = fmaf(-slope, (float)dist, s[c][i] * scale);
          const float p = valid ? expf(sc - m_q) * il_q : 0.f;
          if constexpr (MODE == 1) dsum = fmaf(p, dp[c][i], dsum);
          else s[c][i] = p * (dp[c][i] - delta_q) * scale;         // dS, with the 1 / sqrt(d) of dQ = dS K / sqrt(d)
        }
    }
    if constexpr (MODE == 1) continue;
    const float* Bs = BWD ? Ks : Vs;                               // O^T += V^T P^T;  dQ^T += K^T dS^T
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Bs[(16 * c + 4 * g + e) * LD + 16 * dt + r], s[c][e], oacc[dt], 0, 0, 0);
  }
  if (!qlive) return;
  if constexpr (!BWD) {
    const float inv = 1.f / l;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
      *(f32x4*)(a.o + ((int64_t)u * T + tq) * H + head * D + 16 * dt + 4 * g) = oacc[dt] * inv;
    if (g == 0) {
      a.lse[((int64_t)u * a.heads + head) * T + tq] = m;
      a.lse[lplane + ((int64_t)u * a.heads + head) * T + tq] = l;
    }
  } else if constexpr (MODE == 1) {
    dsum = fold4(dsum);
    if (g == 0) a.delta_out[((int64_t)u * a.heads + head) * T + tq] = dsum;
  } else {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) *(f32x4*)(a.dqkv + ((int64_t)u * T + tq) * H3 + head * D + 16 * dt + 4 * g) = oacc[dt];
  }
}

// the key owner of the backward: grid (key blocks, heads, users), 256 threads; wave w owns keys 16 w .. 16 w + 15 of the block
template <int D>
__global__ __launch_bounds__(256) void attn_key_kernel(const AttnArgs a) {
  constexpr int LD = D + AT_PAD, DT = D / 16;
  __shared__ __attribute__((aligned(16))) float Qs[AT_Q * LD];
  __shared__ __attribute__((aligned(16))) float Os[AT_Q * LD];      // dO
  __shared__ __attribute__((aligned(16))) float Ls[AT_Q];      // m
  __shared__ __attribute__((aligned(16))) float Is[AT_Q];      // 1 / l
  __shared__ __attribute__((aligned(16))) float Ds[AT_Q];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int kb_ = blockIdx.x, head = blockIdx.y, u = blockIdx.z;    // (key block 0 is the heaviest)
  const int T = a.T, H = a.H, H3 = 3 * H, w = a.window;
  const int k0 = kb_ * AT_Q, jk = k0 + 16 * wave + r;               // the lane's key
  const bool klive = jk < T;
  const float* base = a.qkv + (int64_t)u * T * H3 + head * D;
  const float* dobase = a.d_o + (int64_t)u * T * H + head * D;
  const float* lrow = a.lse + ((int64_t)u * a.heads + head) * T;
  const float* srow = lrow + (int64_t)a.U * a.heads * T;
  const float* drow = a.delta + ((int64_t)u * a.heads + head) * T;
  const float slope = a.slope[head], scale = a.scale;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 kf[DT], vf[DT], dk[DT], dv[DT];
#pragma unroll
  for (int kb = 0; kb < DT; ++kb) {
    kf[kb] = klive ? *(const f32x4*)(base + (int64_t)jk * H3 + H + 16 * kb + 4 * g) : zero4;
    vf[kb] = klive ? *(const f32x4*)(base + (int64_t)jk * H3 + 2 * H + 16 * kb + 4 * g) : zero4;
    dk[kb] = zero4;
    dv[kb] = zero4;
  }
  const int jk_lo = k0 + 16 * wave, jk_hi = jk_lo + 15;             // the wave's keys
  const int nqb = (T + AT_Q - 1) / AT_Q;
  const int qt_hi = min(nqb - 1, (k0 + AT_Q - 1 + w - 1) / AT_Q);

  for (int qt = kb_; qt <= qt_hi; ++qt) {
    const int t0 = qt * AT_Q;
    __syncthreads();
    stage_tile<D>(Qs, base, H3, t0, T, tid);
    stage_tile<D>(Os, dobase, H, t0, T, tid);
    if (tid < AT_Q) {
      const bool in = t0 + tid < T;
      Ls[tid] = in ? lrow[t0 + tid] : 0.f;
      Is[tid] = in ? 1.f / srow[t0 + tid] : 0.f;
      Ds[tid] = in ? drow[t0 + tid] : 0.f;
    }
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
      const int tc = t0 + 16 * c;                                   // queries tc .. tc + 15
      if (tc + 15 < jk_lo || tc - jk_hi >= w || tc >= T) continue;  // out of the wave's reach (wave-uniform)
      f32x4 s = zero4, dp = zero4;
#pragma unroll
      for (int kb = 0; kb < DT; ++kb) {
        const f32x4 qa = *(const f32x4*)(Qs + (16 * c + r) * LD + 16 * kb + 4 * g);
        const f32x4 oa = *(const f32x4*)(Os + (16 * c + r) * LD + 16 * kb + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[e], kf[kb][e], s, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_16x16x4f32(oa[e], vf[kb][e], dp, 0, 0, 0);
        }
      }
      // s[i]: query tc + 4 g + i against key jk
      const f32x4 l4 = *(const f32x4*)(Ls + 16 * c + 4 * g), i4 = *(const f32x4*)(Is + 16 * c + 4 * g);
      const f32x4 d4 = *(const f32x4*)(Ds + 16 * c + 4 * g);
      f32x4 pv, dsv;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = tc + 4 * g + i, dist = t - jk;
        const bool valid = klive && t < T && dist >= 0 && dist < w;
        const float sc = fmaf(-slope, (float)dist, s[i] * scale);
        const float p = valid ? expf(sc - l4[i]) * i4[i] : 0.f;
        pv[i] = p;
        dsv[i] = p * (dp[i] - d4[i]) * scale;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          dv[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Os[(16 * c + 4 * g + e) * LD + 16 * dt + r], pv[e], dv[dt], 0, 0, 0);
          dk[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Qs[(16 * c + 4 * g + e) * LD + 16 * dt + r], dsv[e], dk[dt], 0, 0, 0);
        }
    }
  }
  if (!klive) return;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    float* dst = a.dqkv + ((int64_t)u * T + jk) * H3 + head * D + 16 * dt + 4 * g;
    *(f32x4*)(dst + H) = dk[dt];
    *(f32x4*)(dst + 2 * H) = dv[dt];
  }
}

// ------------------------------------------------------------------------------------------------ attention over the KV cache
// The step-by-step path: a call appends n steps to each of R sessions; session u of the call extends cache row rows[u]
// from its own position pos[u].  The cache row holds [k | v] (2H floats) per position, position p in slot p % cap; cap is a multiple
// of 64, so a 64-aligned tile of positions is 64 consecutive slots.
struct AttnCacheArgs {
  int R, n, H, heads, window;       // window: 1 .. AT_NO_WINDOW
  float scale;
  float slope[AT_MAXHEADS];
  const float* qkv;                 // [R][n][3H]: the new rows' in-projection (q is read here; k and v from the cache)
  float* kv;                        // [n_sessions][cap][2H]
  int n_sessions, cap, ring;        // ring: a position past cap wraps (the encoder has a window); else pos + n <= cap
  const int32_t* pos;               // [R]
  const int32_t* rows;              // [R]
  float* o;                         // [R][n][H]
};
constexpr int AT_NO_WINDOW = 1 << 30;

// a session the host's checks would have refused writes and reads nothing
__device__ __forceinline__ bool cache_row_ok(const AttnCacheArgs& a, int row, int pos) {
  return (unsigned)row < (unsigned)a.n_sessions && pos >= 0 && pos <= AT_NO_WINDOW && (a.ring || pos + a.n <= a.cap);
}

// the k and v columns of the new rows go to their slots: 16-byte vector stores, one thread per chunk
__global__ __launch_bounds__(256) void kv_scatter_kernel(const AttnCacheArgs a) {
  const int C4 = a.H >> 1;          // 2H / 4
  const int64_t total = (int64_t)a.R * a.n * C4;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t s = idx / C4;
    const int c = (int)(idx - s * C4), u = (int)(s / a.n), j = (int)(s - (int64_t)u * a.n);
    const int row = a.rows[u], pos = a.pos[u];
    if (!cache_row_ok(a, row, pos)) continue;
    const int slot = (pos + j) % a.cap;
    *(float4*)(a.kv + ((int64_t)row * a.cap + slot) * 2 * a.H + 4 * c) = *(const float4*)(a.qkv + s * 3 * a.H + a.H + 4 * c);
  }
}

// The forward of attn_query_kernel<D, 0> for the new rows of a session: query blocks stay aligned to ABSOLUTE positions (grid x runs
// over the 64-aligned blocks [pos, pos + n) touches, the heaviest first; a lane is live iff pos <= tq < pos + n), the key tiles
// tile_lo .. qb are staged from the cache with pos + n in T's place, and the score / softmax / P V code below is that kernel's, line
// for line: a live lane computes the chain it computes in a whole-history call of pos + n steps.  A staged row is a live position or
// zero -- a slot nothing has written, or one that holds an overwritten position, is never read (DESIGN.md 31 derives the ring size that
// guarantees it), so stale or NaN bits never reach an MFMA.  The next tile's loads are in flight while the current one is computed
// (at n = 1 the kernel is a stream over the session's keys and values: one workgroup per (session, head), 64 positions per stage).
template <int D>
__global__ __launch_bounds__(256) void attn_cache_kernel(const AttnCacheArgs a) {
  constexpr int LD = D + AT_PAD, DT = D / 16, C4 = D / 4;
  __shared__ __attribute__((aligned(16))) float Ks[AT_Q * LD];
  __shared__ __attribute__((aligned(16))) float Vs[AT_Q * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int head = blockIdx.y, u = blockIdx.z;
  const int row = a.rows[u], pos = a.pos[u];
  if (!cache_row_ok(a, row, pos)) return;
  const int T = pos + a.n, H = a.H, H3 = 3 * H, w = a.window;
  const int qb = (T - 1) / AT_Q - (int)blockIdx.x;
  if (qb < pos / AT_Q) return;                         // (uniform over the workgroup: before any barrier)
  const int q0 = qb * AT_Q, tq = q0 + 16 * wave + r;   // the lane's query, an absolute position
  const bool qlive = tq >= pos && tq < T;
  const float* qrow = a.qkv + ((int64_t)u * a.n + (tq - pos)) * H3 + head * D;
  const float* kbase = a.kv + (int64_t)row * a.cap * 2 * H + head * D;
  const float slope = a.slope[head], scale = a.scale;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 qf[DT];
#pragma unroll
  for (int kb = 0; kb < DT; ++kb) qf[kb] = qlive ? *(const f32x4*)(qrow + 16 * kb + 4 * g) : zero4;
  f32x4 oacc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) oacc[dt] = zero4;
  float m = neg_inf(), l = 0.f;
  const int tq_lo = q0 + 16 * wave, tq_hi = tq_lo + 15;
  const int tile_lo = max(0, q0 - w + 1) / AT_Q;

  float4 kr[DT], vr[DT];            // the tile in flight: chunk tid + 256 i of its [64][D / 4] chunks
  auto fetch = [&](int kt) {
    const int k0 = kt * AT_Q;
    const float* src = kbase + (int64_t)(k0 % a.cap) * 2 * H;
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      const int idx = tid + 256 * i, rw = idx / C4, c = idx - rw * C4;
      const bool in = k0 + rw < T;
      kr[i] = in ? *(const float4*)(src + (int64_t)rw * 2 * H + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
      vr[i] = in ? *(const float4*)(src + (int64_t)rw * 2 * H + H + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  fetch(tile_lo);
  for (int kt = tile_lo; kt <= qb; ++kt) {
    const int k0 = kt * AT_Q;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < DT; ++i) {
      const int idx = tid + 256 * i, rw = idx / C4, c = idx - rw * C4;
      *(float4*)(Ks + rw * LD + 4 * c) = kr[i];
      *(float4*)(Vs + rw * LD + 4 * c) = vr[i];
    }
    __syncthreads();
    if (kt < qb) fetch(kt + 1);
    if (k0 > tq_hi || k0 + AT_Q - 1 < tq_lo - w + 1) continue;      // nothing of the tile is in the wave's reach (wave-uniform)
    f32x4 s[4] = {zero4, zero4, zero4, zero4};
#pragma unroll
    for (int kb = 0; kb < DT; ++kb) {
      f32x4 kf[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) kf[c] = *(const f32x4*)(Ks + (16 * c + r) * LD + 16 * kb + 4 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[c][e], qf[kb][e], s[c], 0, 0, 0);
    }
    // s[c][i]: key k0 + 16 c + 4 g + i against query tq
    float tmax = neg_inf();
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int dist = tq - (k0 + 16 * c + 4 * g + i);
        const bool valid = dist >= 0 && dist < w;
        const float sc = valid ? fmaf(-slope, (float)dist, s[c][i] * scale) : neg_inf();
        s[c][i] = sc;
        tmax = fmaxf(tmax, sc);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m, tmax);
    const float m_use = m_new == neg_inf() ? 0.f : m_new;
    const float alpha = expf(m - m_use);
    float psum = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = expf(s[c][i] - m_use);
        s[c][i] = p;
        psum += p;
      }
    psum = fold4(psum);
    l = fmaf(l, alpha, psum);
    m = m_new;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) oacc[dt] *= alpha;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(Vs[(16 * c + 4 * g + e) * LD + 16 * dt + r], s[c][e], oacc[dt], 0, 0, 0);
  }
  if (!qlive) return;
  const float inv = 1.f / l;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
    *(f32x4*)(a.o + ((int64_t)u * a.n + (tq - pos)) * H + head * D + 16 * dt + 4 * g) = oacc[dt] * inv;
}

// ------------------------------------------------------------------------------------------------ weight gradients
// dW[m, n] = sum_s da[s, m] X[s, n] over the call's samples s = u T + t: the tile of seq_dw_kernel (seq_grad.h: 64 x 64 of dW per
// workgroup, 16 samples per LDS stage, exact-f32 MFMA, the rating column and db as plain sums of the same stage) with one more grid
// dimension.  There a workgroup walks ALL samples of a chunk of 32 steps; here the whole call is one "chunk" of U T samples, and
// 12 x 2 workgroups walking 25 000 samples one after the other took 7 of the backward's 9 ms.  So the samples are cut
// into `nsplit` segments of `seg` samples (a function of U T alone), workgroup z sums its segment in sample order into part[z], and
// attn_sum_parts_kernel adds the parts in the order z = 0, 1, ..: still no atomics, still one fixed order for equal calls.
struct AdwArgs {
  SeqStore s;                       // GATHER: X rows are table rows through the store, and the rating is one more column
  int t0, T;
  int S, seg;                       // samples of the call; samples per segment (a multiple of 16)
  const float* da;                  // [S][lda], columns 0 .. G - 1
  int lda;
  const float* x;                   // dense X rows [S][ldx]
  int ldx;
  int G, N;                         // rows of dW (a multiple of 16), columns without the rating column (a multiple of 4)
  float* part;                      // [nsplit][G][ldp], ldp = N (+ 1: the rating column, GATHER); NULL: dW is not wanted
  int ldp;
  float* part_b;                    // [nsplit][G]; NULL: db is not wanted
};

// grid (ceil(G / 64), ceil(N / 64) or 1, nsplit), 256 threads
template <bool GATHER>
__global__ __launch_bounds__(256) void attn_dw_kernel(const AdwArgs a) {
  __shared__ __attribute__((aligned(16))) float As[2][DW_S][DW_LD];
  __shared__ __attribute__((aligned(16))) float Xs[2][DW_S][DW_LD];
  __shared__ float Rs[2][DW_S];
  const int G = a.G, N = a.N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * DW_T, n0 = blockIdx.y * DW_T;
  const int s_lo = blockIdx.z * a.seg, s_hi = min(a.S, s_lo + a.seg), nb = (s_hi - s_lo + DW_S - 1) / DW_S;
  const int sr = tid >> 4, sc = tid & 15;     // the stager: sample row sr of a stage, 16-byte chunk sc of both operands
  const bool xcol = n0 + 4 * sc < N, arow = m0 + 4 * sc < G;
  const bool extras = blockIdx.y == 0 && (a.part_b || (GATHER && a.part));

  auto fetch = [&](int b, float4& av, float4& xv, float& rv) {
    const int s = s_lo + b * DW_S + sr;
    av = make_float4(0.f, 0.f, 0.f, 0.f);
    xv = av;
    rv = 0.f;
    if (s >= s_hi) return;
    if (arow) av = *(const float4*)(a.da + (int64_t)s * a.lda + m0 + 4 * sc);
    if constexpr (GATHER) {
      const int u = s / a.T, t = s - u * a.T;
      const StorePos p = store_pos(a.s, u, a.t0 + t);
      if (xcol) xv = p.live() ? table_chunk(a.s, a.s.items[p.pos], (n0 >> 2) + sc) : nan4();
      if (sc == 0) rv = p.live() ? a.s.ratings[p.pos] : __builtin_nanf("");
    } else {
      if (xcol) xv = *(const float4*)(a.x + (int64_t)s * a.ldx + n0 + 4 * sc);
    }
  };
  auto put = [&](int buf, const float4& av, const float4& xv, float rv) {
    *(float4*)&As[buf][sr][4 * sc] = av;
    *(float4*)&Xs[buf][sr][4 * sc] = xv;
    if (GATHER && sc == 0) Rs[buf][sr] = rv;
  };

  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4] = {zero4, zero4, zero4, zero4};
  float bsum = 0.f, rsum = 0.f;
  float4 av, xv;
  float rv;
  if (nb > 0) {
    fetch(0, av, xv, rv);
    put(0, av, xv, rv);
  }
  __syncthreads();
  for (int b = 0; b < nb; ++b) {
    const int buf = b & 1;
    if (b + 1 < nb) fetch(b + 1, av, xv, rv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float am = As[buf][4 * g + e][16 * wave + r];
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) {
        if (n0 + 16 * tn >= N) continue;
        acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(am, Xs[buf][4 * g + e][16 * tn + r], acc[tn], 0, 0, 0);
      }
    }
    if (extras && tid < DW_T) {       // db and the rating column of this tile's rows: plain sums in sample order
#pragma unroll
      for (int s = 0; s < DW_S; ++s) {
        const float d = As[buf][s][tid];
        bsum += d;
        if constexpr (GATHER) rsum = fmaf(d, Rs[buf][s], rsum);
      }
    }
    if (b + 1 < nb) put(buf ^ 1, av, xv, rv);
    __syncthreads();
  }
  if (a.part) {
    float* out = a.part + (int64_t)blockIdx.z * G * a.ldp;
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      const int n = n0 + 16 * tn + r;
      if (n >= N) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + 16 * wave + 4 * g + i;
        if (m < G) out[(int64_t)m * a.ldp + n] = acc[tn][i];
      }
    }
    if (GATHER && extras && tid < DW_T && m0 + tid < G) out[(int64_t)(m0 + tid) * a.ldp + N] = rsum;
  }
  if (a.part_b && extras && tid < DW_T && m0 + tid < G) a.part_b[(int64_t)blockIdx.z * G + m0 + tid] = bsum;
}

// out[i] = part[0][i] + part[1][i] + .., in that order
__global__ __launch_bounds__(256) void attn_sum_parts_kernel(const float* __restrict__ part, int nsplit, int64_t n, float* __restrict__ out) {
  flat_walk<1>(n, [&](int64_t i, Width<1>) {
    float acc = part[i];
    for (int z = 1; z < nsplit; ++z) acc += part[(int64_t)z * n + i];
    out[i] = acc;
  });
}

constexpr int ADW_MAX_SPLIT = 64, ADW_MIN_SEG = 1024;
inline int adw_nsplit(int64_t S) { return (int)std::max<int64_t>(1, std::min<int64_t>(ADW_MAX_SPLIT, (S + ADW_MIN_SEG - 1) / ADW_MIN_SEG)); }
inline int adw_seg(int64_t S) {
  const int n = adw_nsplit(S);
  return (int)(((S + n - 1) / n + DW_S - 1) / DW_S * DW_S);
}

// ------------------------------------------------------------------------------------------------ host
// what the forward keeps (the workspace of recnn_attn_encode, `saved` of recnn_attn_encode_train): qkv, o, and the log-sum-exp as (m, l)
struct AttnWs {
  int64_t qkv, o, lse, total;
};
inline AttnWs attn_ws(int U, int T, int H, int heads) {
  const int64_t M = (int64_t)U * T;
  AttnWs w;
  w.qkv = 0;
  w.o = scatter_index_round(M * 3 * H * 4);
  w.lse = w.o + scatter_index_round(M * H * 4);
  w.total = w.lse + scatter_index_round((int64_t)U * heads * T * 8);
  return w;
}
// workspace of a backward call: W_o^T, dO, delta, dqkv, the parts of the weight gradients (W_in's [3H][E + 1] + [3H], reused by W_o's)
struct AttnBwdWs {
  int64_t wt, d_o, delta, dqkv, parts, total;
};
inline AttnBwdWs attn_bwd_ws(int U, int T, int H, int E, int heads) {
  const int64_t M = (int64_t)U * T;
  AttnBwdWs w;
  w.wt = 0;
  w.d_o = scatter_index_round((int64_t)H * H * 4);
  w.delta = w.d_o + scatter_index_round(M * H * 4);
  w.dqkv = w.delta + scatter_index_round((int64_t)U * heads * T * 4);
  w.parts = w.dqkv + scatter_index_round(M * 3 * H * 4);
  const int64_t per_part = std::max<int64_t>((int64_t)3 * H * (E + 2), (int64_t)H * (H + 1));      // [3H][E + 1] + [3H], or [H][H] + [H]
  w.total = w.parts + scatter_index_round((int64_t)adw_nsplit(M) * per_part * 4);
  return w;
}

#define RECNN_ATTN_DIMS_OK(what, emb_dim, hidden, n_heads)                                                                      \
  RECNN_LSTM_DIMS_OK(what, emb_dim, hidden);                                                                                    \
  RECNN_REQUIRE(n_heads >= 1 && hidden % n_heads == 0, "%s: hidden must be a multiple of n_heads (got hidden=%d, n_heads=%d)", \
                what, hidden, n_heads);                                                                                         \
  RECNN_REQUIRE(hidden / n_heads == 16 || hidden / n_heads == 32 || hidden / n_heads == 64,                                     \
                "%s: head_dim = hidden / n_heads must be 16, 32 or 64 (got %d)", what, hidden / n_heads)
#define RECNN_ATTN_SIZE_OK(what, n_users, T)                                                                     \
  RECNN_REQUIRE(n_users >= 0 && T >= 0 && (int64_t)n_users * T < (1LL << 31) && n_users <= 65535,                \
                "%s: need n_users in 0 .. 65535, T >= 0 and n_users * T < 2^31", what)

AttnArgs attn_args(int U, int T, int H, int heads, int window, int alibi) {
  AttnArgs a{};
  a.U = U; a.T = T; a.H = H; a.heads = heads;
  a.window = window <= 0 || window > T ? T : window;
  a.scale = (float)(1.0 / sqrt((double)(H / heads)));
  for (int h = 0; h < heads; ++h) a.slope[h] = alibi ? (float)exp2(-8.0 * (h + 1) / heads) : 0.f;
  return a;
}

template <int MODE>
void launch_query(const AttnArgs& a, hipStream_t s) {
  const dim3 grid((a.T + AT_Q - 1) / AT_Q, a.heads, a.U);
  switch (a.H / a.heads) {
    case 16: hipLaunchKernelGGL((attn_query_kernel<16, MODE>), grid, dim3(256), 0, s, a); break;
    case 32: hipLaunchKernelGGL((attn_query_kernel<32, MODE>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((attn_query_kernel<64, MODE>), grid, dim3(256), 0, s, a); break;
  }
}
void launch_key(const AttnArgs& a, hipStream_t s) {
  const dim3 grid((a.T + AT_Q - 1) / AT_Q, a.heads, a.U);
  switch (a.H / a.heads) {
    case 16: hipLaunchKernelGGL((attn_key_kernel<16>), grid, dim3(256), 0, s, a); break;
    case 32: hipLaunchKernelGGL((attn_key_kernel<32>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((attn_key_kernel<64>), grid, dim3(256), 0, s, a); break;
  }
}
// The append path.  What one append call keeps in its workspace: the new rows' qkv, o and (inside a block) u.
struct AppendWs {
  int64_t qkv, o, u, total;
};
inline AppendWs append_ws(int R, int n, int H) {
  const int64_t M = (int64_t)R * n;
  AppendWs w;
  w.qkv = 0;
  w.o = scatter_index_round(M * 3 * H * 4);
  w.u = w.o + scatter_index_round(M * H * 4);
  w.total = w.u + scatter_index_round(M * H * 4);
  return w;
}
// the smallest ring that keeps every staged position apart from every slot the append writes: the key tiles of the first query block
// q0 = 64 floor(pos / 64) start at q0 - 64 ceil((w - 1) / 64), and the last written position is at most q0 + 63 + n - 1
inline int kv_min_capacity(int window, int n) { return 64 * ((window - 1 + 63) / 64) + 64 * ((n + 63 + 63) / 64); }

#define RECNN_KV_CACHE_OK(what, n_rows, n, n_sessions, capacity, window, kv, pos, rows)                                              \
  RECNN_REQUIRE(kv && pos && rows, "%s: null pointer (kv, pos, rows)", what);                                                        \
  RECNN_REQUIRE(n >= 1 && n_rows >= 0 && n_rows <= 65535 && (int64_t)n_rows * n < (1LL << 31),                                       \
                "%s: need n >= 1, n_rows in 0 .. 65535 and n_rows * n < 2^31 (got n_rows=%d, n=%d)", what, n_rows, n);               \
  RECNN_REQUIRE(n_sessions >= n_rows, "%s: n_rows=%d distinct rows do not fit n_sessions=%d", what, n_rows, n_sessions);             \
  RECNN_REQUIRE(capacity >= 64 && capacity % 64 == 0, "%s: capacity must be a positive multiple of 64 (got %d)", what, capacity);   \
  RECNN_REQUIRE(window >= 0 && window < AT_NO_WINDOW, "%s: window must be in 0 .. 2^30 - 1 (0: none), got %d", what, window);        \
  RECNN_REQUIRE(n <= capacity && (window == 0 || capacity >= kv_min_capacity(window, n)),                                            \
                "%s: capacity=%d is too small for window=%d and n=%d (a ring needs %d; without a window n <= capacity)", what,       \
                capacity, window, n, window ? kv_min_capacity(window, n) : n);                                                       \
  RECNN_REQUIRE(aligned16(kv), "%s: kv must be 16-byte aligned", what)

// k and v of the new rows into the cache, then the attention of the new rows over it: qkv [R][n][3H] -> o [R][n][H]
void launch_cache_attention(const float* qkv, float* o, int R, int n, int H, int heads, int window, int alibi, float* kv, int n_sessions,
                            int cap, const int32_t* pos, const int32_t* rows, hipStream_t s) {
  const AttnArgs base = attn_args(R, n, H, heads, 0, alibi);      // scale and slopes as in the whole-history call
  AttnCacheArgs a{};
  a.R = R; a.n = n; a.H = H; a.heads = heads;
  a.window = window > 0 ? window : AT_NO_WINDOW;
  a.scale = base.scale;
  for (int h = 0; h < AT_MAXHEADS; ++h) a.slope[h] = base.slope[h];
  a.qkv = qkv; a.kv = kv; a.n_sessions = n_sessions; a.cap = cap; a.ring = window > 0;
  a.pos = pos; a.rows = rows; a.o = o;
  hipLaunchKernelGGL(kv_scatter_kernel, dim3(grid_for((int64_t)R * n * (H >> 1), 256, 2048)), dim3(256), 0, s, a);
  const dim3 grid((n + AT_Q - 2) / AT_Q + 1, heads, R);            // the 64-aligned blocks n consecutive positions can touch
  switch (H / heads) {
    case 16: hipLaunchKernelGGL((attn_cache_kernel<16>), grid, dim3(256), 0, s, a); break;
    case 32: hipLaunchKernelGGL((attn_cache_kernel<32>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((attn_cache_kernel<64>), grid, dim3(256), 0, s, a); break;
  }
}

int launch_linear(const LinArgs& l, hipStream_t s) {
  const size_t lds = lin_lds(l.K);
  if (int rc = raise_lds(attn_linear_kernel, lds)) return rc;
  hipLaunchKernelGGL(attn_linear_kernel, dim3((l.rows + LIN_ROWS - 1) / LIN_ROWS), dim3(256), lds, s, l);
  return 0;
}
int launch_dense_linear(const DenseLinArgs& l, bool ln, hipStream_t s) {
  const size_t lds = dense_lin_lds(l.K);
  const dim3 grid((l.rows + LIN_ROWS - 1) / LIN_ROWS, (l.N + LIN_COLS - 1) / LIN_COLS);
  if (ln) {
    if (int rc = raise_lds(dense_linear_kernel<true>, lds)) return rc;
    hipLaunchKernelGGL((dense_linear_kernel<true>), grid, dim3(256), lds, s, l);
  } else {
    if (int rc = raise_lds(dense_linear_kernel<false>, lds)) return rc;
    hipLaunchKernelGGL((dense_linear_kernel<false>), grid, dim3(256), lds, s, l);
  }
  return 0;
}

// dW[m, n] = sum_s da[s, m] X[s, n] (G rows, N columns) and db[m] = sum_s da[s, m] over the S = U T samples of a call, either may be
// NULL: the tile launch over the segments of the samples into `part`, then the parts summed into d_w and d_b.  `st`: X rows are
// gathered through the store at steps t0 .. t0 + T - 1 and d_w [G][N + 1] has the rating column; NULL: X is x [S][ldx].  `part` holds
// nsplit ([G][ldp] + [G]) floats, free again when the launches have run (stream order).
void launch_weight_grad(const SeqStore* st, int t0, int T, int S, const float* da, int lda, const float* x, int ldx, int G, int N,
                        float* part, float* d_w, float* d_b, hipStream_t s) {
  if (!d_w && !d_b) return;
  const int nsplit = adw_nsplit(S);
  AdwArgs a{};
  if (st) a.s = *st;
  a.t0 = t0; a.T = T; a.S = S; a.seg = adw_seg(S);
  a.da = da; a.lda = lda; a.x = x; a.ldx = ldx;
  a.G = G; a.N = N; a.ldp = N + (st ? 1 : 0);
  a.part = d_w ? part : nullptr;
  a.part_b = d_b ? part + (int64_t)nsplit * G * a.ldp : nullptr;
  const dim3 grid((G + DW_T - 1) / DW_T, d_w ? (N + DW_T - 1) / DW_T : 1, nsplit);
  if (st) hipLaunchKernelGGL((attn_dw_kernel<true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((attn_dw_kernel<false>), grid, dim3(256), 0, s, a);
  if (d_w) {
    const int64_t n = (int64_t)G * a.ldp;
    hipLaunchKernelGGL(attn_sum_parts_kernel, dim3(grid_for(n, 256, 2048)), dim3(256), 0, s, a.part, nsplit, n, d_w);
  }
  if (d_b) hipLaunchKernelGGL(attn_sum_parts_kernel, dim3(grid_for(G, 256, 2048)), dim3(256), 0, s, a.part_b, nsplit, (int64_t)G, d_b);
}

}  // namespace
