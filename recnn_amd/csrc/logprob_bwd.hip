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
#include "logprob_kernels.h"      // logprob_bwd_kernel<T, KT, DX, DenseCols>, its merge and launch_bwd: shared with sampled.hip

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
  const DenseCols cols{c, N};
  if (dx) {
    float* ws = (float*)workspace;
    const dim3 grid(row_tiles, n_slices);
    if (w_bf16)
      launch_bwd<bf16_t, true, DenseCols>(K, grid, s, x, ld_x, B, K, (const bf16_t*)W, ld_w, cols, actions, lse, g_lp, g_lse, tiles, ws,
                                          (int64_t)K, (float*)nullptr);
    else
      launch_bwd<float, true, DenseCols>(K, grid, s, x, ld_x, B, K, (const float*)W, ld_w, cols, actions, lse, g_lp, g_lse, tiles, ws,
                                         (int64_t)K, (float*)nullptr);
    const int64_t quads = (int64_t)B * (K / 4);
    hipLaunchKernelGGL(logprob_bwd_merge_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, (const float*)ws, B, K, n_slices, dx,
                       ld_dx);
  }
  if (dW || dc) {
    const dim3 grid(item_tiles);      // one part: every row tile in row order
    if (w_bf16)
      launch_bwd<bf16_t, false, DenseCols>(K, grid, s, x, ld_x, B, K, (const bf16_t*)W, ld_w, cols, actions, lse, g_lp, g_lse, row_tiles, dW,
                                           ld_dw, dc);
    else
      launch_bwd<float, false, DenseCols>(K, grid, s, x, ld_x, B, K, (const float*)W, ld_w, cols, actions, lse, g_lp, g_lse, row_tiles, dW,
                                          ld_dw, dc);
  }
  return recnn_check_hip(hipGetLastError(), "catalogue_logprob_bwd");
}
