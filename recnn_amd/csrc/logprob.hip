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
#include <math.h>

#include "logprob_tile.h"

namespace {
using namespace logprob_tile;      // Stage, stage_store, stage_mma, lds_at: shared with logprob_bwd.hip

// ws_m, ws_s: [n_slices][B]; ws_za: [B] (written by the one lane of the one slice that holds a valid a[b])
template <typename T>
__global__ __launch_bounds__(256) void logprob_slice_kernel(const float* __restrict__ x, int64_t ldx, int B, int K, const T* __restrict__ W,
                                                            int64_t ldw, const float* __restrict__ c, int N,
                                                            const int64_t* __restrict__ actions, int tiles_per_slice,
                                                            float* __restrict__ ws_m, float* __restrict__ ws_s, float* __restrict__ ws_za) {
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, r16 = lane & 15;
  const int b0 = blockIdx.x * BM;
  const int ntiles = (N + BN - 1) / BN;
  const int t0 = blockIdx.y * tiles_per_slice;
  const int t1 = min(ntiles, t0 + tiles_per_slice);
  const int nk = K / Stage<T>::BK;

  // rows of this lane's accumulator elements: b0 + 32 wave + 16 tm + 4 q + r
  float m[2][4], s[2][4];
  int64_t act[2][4];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m[tm][r] = -INFINITY;
      s[tm][r] = 0.f;
      const int b = b0 + 32 * wave + 16 * tm + 4 * q + r;
      act[tm][r] = b < B ? actions[b] : -1;
    }

  Stage<T> st;
  for (int t = t0; t < t1; ++t) {
    const int n0 = t * BN;
    f32x4 acc[2][NTN];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int tn = 0; tn < NTN; ++tn) acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};

    st.fetch(x, ldx, B, b0, W, ldw, N, n0, 0, tid);
    stage_store(st, lds, tid);      // (the previous tile's k-loop ended at a barrier: nobody still reads the stage)
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const bool more = kt + 1 < nk;
      if (more) st.fetch(x, ldx, B, b0, W, ldw, N, n0, (kt + 1) * Stage<T>::BK, tid);
      stage_mma<T, 2, NTN>(lds + (kt & 1) * STAGE_BYTES, 32 * wave, BM, q, r16, acc);
      if (more) stage_store(st, lds + ((kt + 1) & 1) * STAGE_BYTES, tid);
      __syncthreads();
    }

    // fold the tile: lane holds rows 4 q + r of each 16-row block, column n0 + 16 tn + r16
    float cn[NTN];
    bool live[NTN];
#pragma unroll
    for (int tn = 0; tn < NTN; ++tn) {
      const int n = n0 + 16 * tn + r16;
      live[tn] = n < N;
      cn[tn] = live[tn] ? c[n] : 0.f;
    }
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float z[NTN];
        float tmax = -INFINITY;
#pragma unroll
        for (int tn = 0; tn < NTN; ++tn) {
          z[tn] = live[tn] ? acc[tm][tn][r] + cn[tn] : -INFINITY;
          tmax = fmaxf(tmax, z[tn]);
          if (live[tn] && act[tm][r] == (int64_t)(n0 + 16 * tn + r16)) ws_za[b0 + 32 * wave + 16 * tm + 4 * q + r] = z[tn];
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 8));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 4));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 2));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 1));
        const float mn = fmaxf(m[tm][r], tmax);      // column n0 of the tile is below N, so finite for finite operands (the header asks for them)
        float e = expf(z[0] - mn);
#pragma unroll
        for (int tn = 1; tn < NTN; ++tn) e += expf(z[tn] - mn);
        e += __shfl_xor(e, 8);
        e += __shfl_xor(e, 4);
        e += __shfl_xor(e, 2);
        e += __shfl_xor(e, 1);
        s[tm][r] = s[tm][r] * expf(m[tm][r] - mn) + e;
        m[tm][r] = mn;
      }
  }

  if (r16 == 0) {
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int b = b0 + 32 * wave + 16 * tm + 4 * q + r;
        if (b < B) {
          ws_m[(int64_t)blockIdx.y * B + b] = m[tm][r];
          ws_s[(int64_t)blockIdx.y * B + b] = s[tm][r];
        }
      }
  }
}

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
  if (w_bf16)
    hipLaunchKernelGGL(logprob_slice_kernel<bf16_t>, grid, dim3(256), 0, s, x, ld_x, B, K, (const bf16_t*)W, ld_w, c, N, actions, tiles, ws_m,
                       ws_s, ws_za);
  else
    hipLaunchKernelGGL(logprob_slice_kernel<float>, grid, dim3(256), 0, s, x, ld_x, B, K, (const float*)W, ld_w, c, N, actions, tiles, ws_m,
                       ws_s, ws_za);
  hipLaunchKernelGGL(logprob_merge_kernel, dim3((B + 255) / 256), dim3(256), 0, s, (const float*)ws_m, (const float*)ws_s,
                     (const float*)ws_za, actions, B, N, n_slices, logprob, lse);
  return recnn_check_hip(hipGetLastError(), "catalogue_logprob");
}
