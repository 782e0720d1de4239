// logprob_bwd.hip -- backward of the catalogue log-prob (section 18 of include/recnn_hip.h): the gradients of
// logprob[b] = z[b, a_b] - lse[b] and lse[b] with respect to x, W and c, the [B, N] gradient matrix never in memory.
//
//   p[b, n] = exp(z[b, n] - lse[b])      D[b, n] = (g_lse[b] - g_lp[b]) p[b, n] + g_lp[b] [n == a_b]
//   dx = D W   [B, K]        dW = D^T x   [N, K]        dc[n] = sum_b D[b, n]
//
// One kernel body serves both products.  A workgroup (4 waves) recomputes a 128 x 128 tile of z with the forward's stage / k-loop
// (logprob_tile.h), but cut the other way: a wave holds all 128 rows of the tile's A side and 32 columns of its B side, as 8 x 2 MFMA
// blocks.  D is formed in those accumulators.  Lane (q, r16) then holds A-side rows 4 q + r of B-side column r16, which is the
// A-operand layout of the TRANSPOSED tile: the second product contracts over the tile's A side and its output rows are the wave's
// 32 B-side columns, without D ever leaving the registers.
//   dW / dc kernel: A side = 128 batch rows, B side = 128 items.  One workgroup per item tile walks the row tiles in row order; the
//     [128 items, Kp] accumulator (32 items per wave, 128 registers per lane at Kp = 256) stays in registers and every element of dW
//     and dc is written once.
//   dx kernel: A side = 128 items, B side = 128 batch rows (the stage is stored swapped).  Grid: row tiles x catalogue slices; a
//     workgroup walks its slice's item tiles in order and writes one [128 rows, Kp] partial per (row tile, slice); the merge kernel
//     adds the partials in slice order.
// The second product's other operand (x rows for dW, W rows for dx) is read from global memory as the tile's A-side rows, 16 bytes a
// lane: column block j of lane r16 stands for column (Kp / 16) r16 + j, so a lane's columns are contiguous in memory.
//   fp32: mfma_f32_16x16x4f32, contraction rows {4 q + r} per step.   bf16: mfma_f32_16x16x32_bf16, D rounded to bf16 (nearest even),
//     x rounded as the forward rounds it; a lane's 8 contraction rows are 4 q + r of two neighbouring 16-row blocks.
// No atomics.  Every sum has one order, fixed by (B, N, K, items_per_slice): equal calls give equal bits, and a row's dx bits depend
// on that row, W, c, its lse and gradients and the slice length alone (an output row of the second product reads one column of D,
// which reads one x row; the items are contracted in tile order whatever the row's position).
// Longest chains of additions: dx  items of a slice (4 or 32 per MFMA step, one step after the other) + slices;
//                              dW  rows, padded to whole tiles with exact zeros;   dc  rows / 4 in a lane + 2 across the four q.
#include <math.h>

#include "logprob_tile.h"

namespace {
using namespace logprob_tile;

constexpr int KMAX = 256;     // padded K the register-resident accumulator is built for

struct RowInfo {
  float lse, gd, glp;   // gd = g_lse - g_lp
  int act;              // the action if it lies in [0, N), else -1
};

// KT: K rounded up to a multiple of 64 (64 .. 256).  DX: the dx kernel (A side = items) else the dW / dc kernel (A side = rows).
// The fp32 dx kernel at KT <= 128 fits 256 registers (7 spilled) and with them two workgroups on a compute unit; every other variant
// needs more than half the register file for its output tile and runs one.
template <typename T, int KT, bool DX>
__global__ __launch_bounds__(256, (DX && KT <= 128 && sizeof(T) == 4) ? 2 : 1) void logprob_bwd_kernel(
                                                          const float* __restrict__ x, int64_t ldx, int B, int K,
                                                          const T* __restrict__ W, int64_t ldw, const float* __restrict__ c, int N,
                                                          const int64_t* __restrict__ actions, const float* __restrict__ lse,
                                                          const float* __restrict__ g_lp, const float* __restrict__ g_lse,
                                                          int tiles_per_slice, float* __restrict__ out, int64_t ld_out,
                                                          float* __restrict__ dc) {
  constexpr int NJ = KT / 16;       // 16-column blocks of the output; lane r16 owns columns NJ r16 .. NJ r16 + NJ - 1
  constexpr bool BF = sizeof(T) == 2;
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE_BYTES];
  __shared__ RowInfo ri[BM];
  __shared__ float cv[BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, r16 = lane & 15;
  const int nk = K / Stage<T>::BK;
  // DX: fixed row tile, item tiles [t0, t1) of the slice.  Else: fixed item tile, every row tile.
  const int t0 = DX ? blockIdx.y * tiles_per_slice : 0;
  const int t1 = DX ? min((N + BN - 1) / BN, t0 + tiles_per_slice) : (B + BM - 1) / BM;

  f32x4 o[2][NJ];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn)
#pragma unroll
    for (int j = 0; j < NJ; ++j) o[tn][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dcs[2] = {0.f, 0.f};

  Stage<T> st;
  for (int t = t0; t < t1; ++t) {
    const int b0 = (DX ? blockIdx.x : t) * BM, n0 = (DX ? t : blockIdx.x) * BN;
    f32x4 acc[8][2];
#pragma unroll
    for (int tm = 0; tm < 8; ++tm)
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};

    // per-row and per-item scalars of the tile (read after the k-loop's barriers; the barrier that ends the tile frees them again).
    // A row at or past B gets lse = +inf and an item at or past N gets c = -inf: p = exp(-inf) = 0 and D = 0 there.
    if (tid < BM) {
      const int b = b0 + tid;
      RowInfo r = {INFINITY, 0.f, 0.f, -1};
      if (b < B) {
        const int64_t a = actions[b];
        const bool ok = a >= 0 && a < N;
        const float gl = g_lse ? g_lse[b] : 0.f;
        const float gp = (g_lp && ok) ? g_lp[b] : 0.f;
        r = RowInfo{lse[b], gl - gp, gp, ok ? (int)a : -1};
      }
      ri[tid] = r;
    } else {
      const int n = n0 + tid - BM;
      cv[tid - BM] = n < N ? c[n] : -INFINITY;
    }

    st.fetch(x, ldx, B, b0, W, ldw, N, n0, 0, tid);
    stage_store<T, DX>(st, lds, tid);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const bool more = kt + 1 < nk;
      if (more) st.fetch(x, ldx, B, b0, W, ldw, N, n0, (kt + 1) * Stage<T>::BK, tid);
      stage_mma<T, 8, 2>(lds + (kt & 1) * STAGE_BYTES, 0, BM + 32 * wave, q, r16, acc);
      if (more) stage_store<T, DX>(st, lds + ((kt + 1) & 1) * STAGE_BYTES, tid);
      __syncthreads();
    }

    // D in place of z: acc[tm][tn][r] is A-side row ia = 16 tm + 4 q + r, B-side column ib = 32 wave + 16 tn + r16
    RowInfo rb[2];    // DX: the lane's two batch rows
    float cb[2];      // else: the lane's two items
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int ib = 32 * wave + 16 * tn + r16;
      if constexpr (DX) rb[tn] = ri[ib]; else cb[tn] = cv[ib];
    }
#pragma unroll
    for (int tm = 0; tm < 8; ++tm)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ia = 16 * tm + 4 * q + r;
        RowInfo ra;
        float ca;
        if constexpr (DX) ca = cv[ia]; else ra = ri[ia];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          const RowInfo R = DX ? rb[tn] : ra;
          const float cn = DX ? ca : cb[tn];
          const int n = n0 + (DX ? ia : 32 * wave + 16 * tn + r16);
          const float p = expf(acc[tm][tn][r] + cn - R.lse);
          const float d = R.gd * p + (R.act == n ? R.glp : 0.f);
          acc[tm][tn][r] = d;
          if constexpr (!DX) dcs[tn] += d;
        }
      }

    // second product: o[tn] += D[:, tn block]^T V, V the A side's rows at full K (x rows for dW, W rows for dx)
    const int a0 = DX ? n0 : b0, alim = DX ? N : B;
    if constexpr (!BF) {
      const float* V = DX ? (const float*)W : x;
      const int64_t ldv = DX ? ldw : ldx;
#pragma unroll
      for (int tm = 0; tm < 8; ++tm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = a0 + 16 * tm + 4 * q + r;
          f32x4 v[NJ / 4];
#pragma unroll
          for (int jc = 0; jc < NJ / 4; ++jc) {
            const int k = NJ * r16 + 4 * jc;
            v[jc] = (row < alim && k < K) ? *(const f32x4*)(V + (int64_t)row * ldv + k) : f32x4{0.f, 0.f, 0.f, 0.f};
          }
#pragma unroll
          for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
              o[tn][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[tm][tn][r], v[j / 4][j % 4], o[tn][j], 0, 0, 0);
        }
    } else {
      // contraction slot jj (0..7) of k-step ks: A-side row 16 (2 ks + jj / 4) + 4 q + jj % 4
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        uint4 dfrag[2];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          const f32x4 lo = acc[2 * ks][tn], hi = acc[2 * ks + 1][tn];
          dfrag[tn] = make_uint4(cvt_pk_bf16(lo[0], lo[1]), cvt_pk_bf16(lo[2], lo[3]), cvt_pk_bf16(hi[0], hi[1]), cvt_pk_bf16(hi[2], hi[3]));
        }
#pragma unroll
        for (int jc = 0; jc < NJ / 4; ++jc) {
          const int k = NJ * r16 + 4 * jc;
          uint4 vfrag[4];     // vfrag[e]: the 8 contraction rows of column k + e, as packed bf16 pairs
          if constexpr (DX) {
            uint2 v[8];       // 4 bf16 of W per row
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
              const int row = a0 + 16 * (2 * ks + jj / 4) + 4 * q + jj % 4;
              v[jj] = (row < alim && k < K) ? *(const uint2*)((const bf16_t*)W + (int64_t)row * ldw + k) : make_uint2(0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              uint32_t d[4];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const uint32_t s_lo = e < 2 ? v[2 * i].x : v[2 * i].y, s_hi = e < 2 ? v[2 * i + 1].x : v[2 * i + 1].y;
                d[i] = (e & 1) ? ((s_lo >> 16) | (s_hi & 0xFFFF0000u)) : ((s_lo & 0xFFFFu) | (s_hi << 16));
              }
              vfrag[e] = make_uint4(d[0], d[1], d[2], d[3]);
            }
          } else {
            f32x4 v[8];       // 4 floats of x per row, rounded in pairs of rows
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
              const int row = a0 + 16 * (2 * ks + jj / 4) + 4 * q + jj % 4;
              v[jj] = (row < alim && k < K) ? *(const f32x4*)(x + (int64_t)row * ldx + k) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
              vfrag[e] = make_uint4(cvt_pk_bf16(v[0][e], v[1][e]), cvt_pk_bf16(v[2][e], v[3][e]), cvt_pk_bf16(v[4][e], v[5][e]),
                                    cvt_pk_bf16(v[6][e], v[7][e]));
          }
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
              o[tn][4 * jc + e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, dfrag[tn]),
                                                                          __builtin_bit_cast(bf16x8, vfrag[e]), o[tn][4 * jc + e], 0, 0, 0);
        }
      }
    }
    __syncthreads();      // ri / cv and the first stage are rewritten at the top of the next tile
  }

  // o[tn][j][i]: output row 32 wave + 16 tn + 4 q + i, column NJ r16 + j
  const int r0 = (DX ? blockIdx.x * BM : blockIdx.x * BN), rlim = DX ? B : N;
  float* dst = DX ? out + (int64_t)blockIdx.y * B * ld_out : out;
  if (dst) {
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = r0 + 32 * wave + 16 * tn + 4 * q + i;
        if (row >= rlim) continue;
#pragma unroll
        for (int jc = 0; jc < NJ / 4; ++jc) {
          const int k = NJ * r16 + 4 * jc;
          if (k < K)
            *(f32x4*)(dst + (int64_t)row * ld_out + k) =
                f32x4{o[tn][4 * jc][i], o[tn][4 * jc + 1][i], o[tn][4 * jc + 2][i], o[tn][4 * jc + 3][i]};
        }
      }
  }
  if constexpr (!DX) {
    if (dc) {
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        float s = dcs[tn];
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const int n = r0 + 32 * wave + 16 * tn + r16;
        if (q == 0 && n < N) dc[n] = s;
      }
    }
  }
}

// dx[b, k] = sum over slices, in slice order, of the partials [n_slices][B][K]
__global__ __launch_bounds__(256) void logprob_bwd_merge_kernel(const float* __restrict__ ws, int B, int K, int n_slices,
                                                                float* __restrict__ dx, int64_t ld_dx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // one thread per 4 columns
  const int kq = K / 4;
  if (i >= (int64_t)B * kq) return;
  const int b = (int)(i / kq), k = (int)(i % kq) * 4;
  f32x4 s = *(const f32x4*)(ws + (int64_t)b * K + k);
  for (int sl = 1; sl < n_slices; ++sl) s += *(const f32x4*)(ws + ((int64_t)sl * B + b) * K + k);
  *(f32x4*)(dx + (int64_t)b * ld_dx + k) = s;
}

template <typename T, bool DX, typename... A>
void launch_bwd(int K, dim3 grid, hipStream_t s, A... a) {
  switch ((K + 63) / 64) {
    case 1: hipLaunchKernelGGL((logprob_bwd_kernel<T, 64, DX>), grid, dim3(256), 0, s, a...); break;
    case 2: hipLaunchKernelGGL((logprob_bwd_kernel<T, 128, DX>), grid, dim3(256), 0, s, a...); break;
    case 3: hipLaunchKernelGGL((logprob_bwd_kernel<T, 192, DX>), grid, dim3(256), 0, s, a...); break;
    default: hipLaunchKernelGGL((logprob_bwd_kernel<T, 256, DX>), grid, dim3(256), 0, s, a...); break;
  }
}
}  // namespace

extern "C" int recnn_catalogue_logprob_bwd_workspace_bytes(int B, int N, int K, int items_per_slice, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes, "catalogue_logprob_bwd_workspace_bytes: null pointer");
  int n_slices = 0;
  RECNN_REQUIRE(B >= 0 && slices_of(N, items_per_slice, &n_slices),
                "catalogue_logprob_bwd_workspace_bytes: need B >= 0, N >= 1 and items_per_slice a positive multiple of 128 (got %d, %d, %d)",
                B, N, items_per_slice);
  RECNN_REQUIRE(K >= 32 && K % 32 == 0, "catalogue_logprob_bwd_workspace_bytes: K must be a positive multiple of 32 (got %d)", K);
  RECNN_REQUIRE(K <= KMAX, "catalogue_logprob_bwd_workspace_bytes: K = %d is above the limit of %d (padded) the backward is built for", K,
                KMAX);
  *h_bytes = (int64_t)n_slices * B * K * 4;
  return 0;
}

extern "C" int recnn_catalogue_logprob_bwd(const float* x, int64_t ld_x, int B, int K, const void* W, int64_t ld_w, int w_bf16,
                                           const float* c, int N, const int64_t* actions, const float* lse, const float* g_lp,
                                           const float* g_lse, int items_per_slice, float* dx, int64_t ld_dx, float* dW, int64_t ld_dw,
                                           float* dc, void* workspace, void* stream) {
  RECNN_REQUIRE(W && c && ((x && actions && lse) || B == 0), "catalogue_logprob_bwd: null pointer");
  RECNN_REQUIRE(!dx || workspace || B == 0, "catalogue_logprob_bwd: dx needs the workspace");
  int n_slices = 0;
  RECNN_REQUIRE(B >= 0 && slices_of(N, items_per_slice, &n_slices),
                "catalogue_logprob_bwd: need B >= 0, N >= 1 and items_per_slice a positive multiple of 128 (got %d, %d, %d)", B, N,
                items_per_slice);
  const int bk = w_bf16 ? 64 : 32;
  RECNN_REQUIRE(K >= bk && K % bk == 0, "catalogue_logprob_bwd: K must be a positive multiple of %d (got %d)", bk, K);
  RECNN_REQUIRE(K <= KMAX, "catalogue_logprob_bwd: K = %d is above the limit of %d (padded) the backward is built for", K, KMAX);
  RECNN_REQUIRE(ld_x >= K && ld_x % 4 == 0 && ld_w >= K && ld_w % (w_bf16 ? 8 : 4) == 0 && aligned16(x, W),
                "catalogue_logprob_bwd: x / W rows must be 16-byte aligned and at least K long");
  RECNN_REQUIRE((!dx || (ld_dx >= K && ld_dx % 4 == 0)) && (!dW || (ld_dw >= K && ld_dw % 4 == 0)) && aligned16(dx, dW) &&
                    ((uintptr_t)workspace & 15) == 0,
                "catalogue_logprob_bwd: dx / dW rows and the workspace must be 16-byte aligned, rows at least K long");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {
    if (dW) RECNN_HIP(hipMemset2DAsync(dW, (size_t)ld_dw * 4, 0, (size_t)K * 4, (size_t)N, s));
    if (dc) RECNN_HIP(hipMemsetAsync(dc, 0, (size_t)N * 4, s));
    return 0;
  }
  const int row_tiles = (B + BM - 1) / BM, item_tiles = (N + BN - 1) / BN;
  RECNN_REQUIRE(n_slices <= 65535, "catalogue_logprob_bwd: more than 65535 slices (items_per_slice %d too small for N %d)", items_per_slice,
                N);
  const int tiles = items_per_slice / BN;
  if (dx) {
    float* ws = (float*)workspace;
    const dim3 grid(row_tiles, n_slices);
    if (w_bf16)
      launch_bwd<bf16_t, true>(K, grid, s, x, ld_x, B, K, (const bf16_t*)W, ld_w, c, N, actions, lse, g_lp, g_lse, tiles, ws, (int64_t)K,
                               (float*)nullptr);
    else
      launch_bwd<float, true>(K, grid, s, x, ld_x, B, K, (const float*)W, ld_w, c, N, actions, lse, g_lp, g_lse, tiles, ws, (int64_t)K,
                              (float*)nullptr);
    const int64_t quads = (int64_t)B * (K / 4);
    hipLaunchKernelGGL(logprob_bwd_merge_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, (const float*)ws, B, K, n_slices, dx,
                       ld_dx);
  }
  if (dW || dc) {
    const dim3 grid(item_tiles);
    if (w_bf16)
      launch_bwd<bf16_t, false>(K, grid, s, x, ld_x, B, K, (const bf16_t*)W, ld_w, c, N, actions, lse, g_lp, g_lse, tiles, dW, ld_dw, dc);
    else
      launch_bwd<float, false>(K, grid, s, x, ld_x, B, K, (const float*)W, ld_w, c, N, actions, lse, g_lp, g_lse, tiles, dW, ld_dw, dc);
  }
  return recnn_check_hip(hipGetLastError(), "catalogue_logprob_bwd");
}
