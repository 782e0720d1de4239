// logprob.hip -- log-probability of one action per row under a softmax over the whole catalogue, the [B, N] logits never in memory
// (section 17 of include/recnn_hip.h).
//
//   z[b, n] = x[b] . W[n] + c[n]      lse[b] = log sum_n exp(z[b, n])      logprob[b] = min(z[b, a[b]] - lse[b], 0)
//
// Grid: row tiles of BM = 128 rows x catalogue slices of items_per_slice items.  A workgroup (4 waves, each 32 rows x 128 items as
// 2 x 8 MFMA blocks) walks the 128-item tiles of its slice; per tile an ordinary k-loop streams 128-byte row pieces of x and W through
// a double-buffered LDS stage (global -> registers while the previous stage multiplies, registers -> LDS, one barrier per stage; the
// 16-byte chunks of a row are xor-swizzled by the row, so the fragment reads of 16 rows spread over the banks without padding).
// After each tile the accumulators (+ c) fold into a running pair per row, m = max z and s = sum exp(z - m): the tile's 128 columns
// of a row sit in one 16-lane group, 8 per lane; the 8 are added left to right, the 16 lanes by an xor butterfly (every lane gets the
// same bits), then s = s exp(m - m') + tile sum.  A column at or past N counts as -inf.  The lane that holds column a[b] writes that
// very accumulator value as the picked logit.  Per (row, slice) the pair goes to the workspace; logprob_merge_kernel (one thread per
// row) takes the slices in slice order: M = max m, S = sum s exp(m - M), lse = M + log S.
// No atomics at all.  A row's bits depend on that row, W, c and the slice length alone: an MFMA output row reads one row of the A
// operand, and the reduction pattern is the same for every row position.
// The longest chain of additions a term of s passes through: 7 (in lane) + 4 (butterfly) + tiles per slice + slices.
#include "logprob_kernels.h"      // logprob_slice_kernel<T, DenseCols>: shared with sampled.hip

namespace {

__global__ __launch_bounds__(256) void logprob_merge_kernel(const float* __restrict__ ws_m, const float* __restrict__ ws_s,
                                                            const float* __restrict__ ws_za, const int64_t* __restrict__ actions, int B,
                                                            int N, int n_slices, float* __restrict__ logprob, float* __restrict__ lse) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float M = -INFINITY;
  for (int i = 0; i < n_slices; ++i) M = fmaxf(M, ws_m[(int64_t)i * B + b]);
  float S = 0.f;
  for (int i = 0; i < n_slices; ++i) S += ws_s[(int64_t)i * B + b] * expf(ws_m[(int64_t)i * B + b] - M);
  const float l = M + logf(S);
  lse[b] = l;
  const int64_t a = actions[b];
  logprob[b] = (a >= 0 && a < N) ? fminf(ws_za[b] - l, 0.f) : __int_as_float(0x7FC00000);
}

}  // namespace

extern "C" int recnn_catalogue_logprob_workspace_bytes(int B, int N, int items_per_slice, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes, "catalogue_logprob_workspace_bytes: null pointer");
  int n_slices = 0;
  RECNN_REQUIRE(B >= 0 && slices_of(N, items_per_slice, &n_slices),
                "catalogue_logprob_workspace_bytes: need B >= 0, N >= 1 and items_per_slice a positive multiple of 128 (got %d, %d, %d)", B, N,
                items_per_slice);
  *h_bytes = ((int64_t)2 * n_slices + 1) * B * 4;
  return 0;
}

extern "C" int recnn_catalogue_logprob(const float* x, int64_t ld_x, int B, int K, const void* W, int64_t ld_w, int w_bf16, const float* c,
                                       int N, const int64_t* actions, int items_per_slice, float* logprob, float* lse, void* workspace,
                                       void* stream) {
  RECNN_REQUIRE(W && c && ((x && actions && logprob && lse && workspace) || B == 0), "catalogue_logprob: null pointer");
  int n_slices = 0;
  RECNN_REQUIRE(B >= 0 && slices_of(N, items_per_slice, &n_slices),
                "catalogue_logprob: need B >= 0, N >= 1 and items_per_slice a positive multiple of 128 (got %d, %d, %d)", B, N,
                items_per_slice);
  const int bk = w_bf16 ? 64 : 32;
  RECNN_REQUIRE(K >= bk && K % bk == 0, "catalogue_logprob: K must be a positive multiple of %d (got %d)", bk, K);
  RECNN_REQUIRE(ld_x >= K && ld_x % 4 == 0 && ld_w >= K && ld_w % (w_bf16 ? 8 : 4) == 0 && aligned16(x, W),
                "catalogue_logprob: x / W rows must be 16-byte aligned and at least K long");
  RECNN_REQUIRE(((uintptr_t)workspace & 3) == 0, "catalogue_logprob: workspace must be 4-byte aligned");
  if (B == 0) return 0;
  RECNN_REQUIRE(n_slices <= 65535, "catalogue_logprob: more than 65535 slices (items_per_slice %d too small for N %d)", items_per_slice, N);
  hipStream_t s = (hipStream_t)stream;
  float* ws_m = (float*)workspace;
  float* ws_s = ws_m + (int64_t)n_slices * B;
  float* ws_za = ws_s + (int64_t)n_slices * B;
  const dim3 grid((B + BM - 1) / BM, n_slices);
  const int tiles = items_per_slice / BN;
  const DenseCols cols{c, N};
  if (w_bf16)
    hipLaunchKernelGGL((logprob_slice_kernel<bf16_t, DenseCols>), grid, dim3(256), 0, s, x, ld_x, B, K, (const bf16_t*)W, ld_w, cols, actions,
                       tiles, ws_m, ws_s, ws_za);
  else
    hipLaunchKernelGGL((logprob_slice_kernel<float, DenseCols>), grid, dim3(256), 0, s, x, ld_x, B, K, (const float*)W, ld_w, cols, actions,
                       tiles, ws_m, ws_s, ws_za);
  hipLaunchKernelGGL(logprob_merge_kernel, dim3((B + 255) / 256), dim3(256), 0, s, (const float*)ws_m, (const float*)ws_s,
                     (const float*)ws_za, actions, B, N, n_slices, logprob, lse);
  return recnn_check_hip(hipGetLastError(), "catalogue_logprob");
}
