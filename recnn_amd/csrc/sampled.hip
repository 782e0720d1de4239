// sampled.hip -- sampled-softmax next-item training with negatives shared by the batch (section 19 of include/recnn_hip.h).
//
//   z_t[b]   = x_b . W[a_b] + c[a_b] - tq[b]                     the target's logit
//   z[b, s]  = x_b . W[n_s] + c[n_s] - nq[s]                     the S negatives, one list for every row (repeats allowed)
//   lse[b]   = log(exp z_t[b] + sum_s exp z[b, s])              logprob[b] = min(z_t[b] - lse[b], 0)
//
// A negative outside [0, N) is an absent column; with remove_hits a negative equal to the row's target is absent in that row.  A target
// outside [0, N) gives NaN in its logprob, its lse is taken over the negatives, its g_lp counts as 0.
//
// Forward, three launches: sampled_target_kernel (one wave per row: the target's dot product, its 4 products per lane added in order,
// the 64 lanes by an xor butterfly), logprob_slice_kernel<T, GatheredCols> (logprob_kernels.h: row tiles x slices of the negatives; the
// B side of the stage is filled from W + ids[s] ld_w, so no [S, K] copy of the table exists), sampled_merge_kernel (per row: the slices in
// slice order, then the target's term).
// Backward: p = exp(z - lse), gd = g_lse - g_lp.
//   D[b, s] = gd_b p[b, s]         D_t[b] = gd_b p_t[b] + g_lp[b]
//   dx = D W[n] + D_t W[a]         dWs[s] = sum_b D[b, s] x_b     dcs[s] = sum_b D[b, s]       (compact: one row per negative)
// sampled_dt_kernel writes D_t (and, when asked, the compact target rows D_t[b] x_b); logprob_bwd_kernel<.., DX, GatheredCols> runs its dx
// role over row tiles x slices and sampled_dx_merge_kernel adds the partials in slice order and then D_t W[a]; its dW / dc role runs
// over item tiles x ROW CHUNKS (S = 4096 is 32 item tiles on 256 compute units), partials merged in chunk order.  The chunk count is a
// function of (B, S) alone.
// recnn_sampled_scatter sums the S + B contributions by item id into the dense dW [N, K] / dc [N] over the inverted index of
// scatter_index.h: contribution j < S is dWs[j] / dcs[j], contribution S + b is D_t[b] x_b / D_t[b], formed on the fly.  A wave sums
// PIECE sorted entries (the run of each destination in list order), a second pass adds a destination's pieces in order and writes every
// row of dW and dc once -- exact +0 where nothing landed.
// bf16 mode: W is the bf16 shadow; x is rounded where it meets W or D (nearest even), D is rounded before the second product, D_t is
// not.  Gradients stay fp32.
// No float atomics.  Every sum has one order fixed by the shapes: equal calls give equal bits, and with items_per_slice fixed a row's
// logprob, lse and dx depend on that row, W, c, the negatives and the corrections alone.
// Longest chains of additions: lse  7 + 4 + tiles per slice + slices + 1;   dx  negatives of a slice + slices + 1;
//   dWs  rows of a chunk + chunks;   dcs  rows of a chunk / 4 + 2 + chunks;   a dense row  its contributions.
#include <algorithm>

#include "logprob_kernels.h"
#include "scatter_index.h"

namespace {

constexpr int PIECE = 16;        // scatter-sum: sorted entries per wave in the first pass

__device__ inline float bf16_round(float f) { return __uint_as_float(cvt_pk_bf16(f, 0.f) << 16); }
__device__ inline f32x4 load_w4(const float* W) { return *(const f32x4*)W; }
__device__ inline f32x4 load_w4(const bf16_t* W) {
  const uint2 v = *(const uint2*)W;
  return f32x4{__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xFFFF0000u), __uint_as_float(v.y << 16),
               __uint_as_float(v.y & 0xFFFF0000u)};
}
__device__ inline f32x4 load_x4(const float* x, bool round) {
  const f32x4 v = *(const f32x4*)x;
  return round ? f32x4{bf16_round(v[0]), bf16_round(v[1]), bf16_round(v[2]), bf16_round(v[3])} : v;
}

// one wave per row; lane owns columns 4 lane .. 4 lane + 3 (K <= 256)
template <typename T>
__global__ __launch_bounds__(256) void sampled_target_kernel(const float* __restrict__ x, int64_t ldx, int B, int K, const T* __restrict__ W,
                                                             int64_t ldw, const float* __restrict__ c, int N,
                                                             const int64_t* __restrict__ targets, const float* __restrict__ tq,
                                                             float* __restrict__ zt) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;
  const int64_t a = targets[b];
  if (a < 0 || a >= N) {
    if (lane == 0) zt[b] = __int_as_float(0x7FC00000);
    return;
  }
  float s = 0.f;
  const int k = 4 * lane;
  if (k < K) {
    const f32x4 xv = load_x4(x + (int64_t)b * ldx + k, sizeof(T) == 2), wv = load_w4(W + a * ldw + k);
    s = xv[0] * wv[0];
    s = fmaf(xv[1], wv[1], s);
    s = fmaf(xv[2], wv[2], s);
    s = fmaf(xv[3], wv[3], s);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) zt[b] = s + (c ? c[a] : 0.f) - (tq ? tq[b] : 0.f);
}

// per row: the slices' (m, s) pairs in slice order, then the target's term (a NaN z_t: the target is invalid and has no term)
__global__ __launch_bounds__(256) void sampled_merge_kernel(const float* __restrict__ ws_m, const float* __restrict__ ws_s,
                                                            const float* __restrict__ zt, int B, int n_slices, float* __restrict__ logprob,
                                                            float* __restrict__ lse) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float z = zt[b];
  const bool ok = z == z;
  float M = ok ? z : -INFINITY;
  for (int i = 0; i < n_slices; ++i) M = fmaxf(M, ws_m[(int64_t)i * B + b]);
  const float Ms = M == -INFINITY ? 0.f : M;      // nothing live in the row at all: lse = log 0 = -inf
  float S = 0.f;
  for (int i = 0; i < n_slices; ++i) S += ws_s[(int64_t)i * B + b] * expf(ws_m[(int64_t)i * B + b] - Ms);
  if (ok) S += expf(z - Ms);
  const float l = Ms + logf(S);
  lse[b] = l;
  logprob[b] = ok ? fminf(z - l, 0.f) : z;
}

// one wave per row: D_t[b] = (g_lse - g_lp) exp(z_t - lse) + g_lp, 0 for an invalid target; rows: D_t[b] x_b (x rounded in bf16 mode)
__global__ __launch_bounds__(256) void sampled_dt_kernel(const float* __restrict__ zt, const float* __restrict__ lse,
                                                         const float* __restrict__ g_lp, const float* __restrict__ g_lse, int B,
                                                         float* __restrict__ dt, const float* __restrict__ x, int64_t ldx, int K, int x_bf16,
                                                         float* __restrict__ rows, int64_t ld_rows) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;
  const float z = zt[b];
  float d = 0.f;
  if (z == z) {
    const float gp = g_lp ? g_lp[b] : 0.f, gl = g_lse ? g_lse[b] : 0.f;
    d = (gl - gp) * expf(z - lse[b]) + gp;
  }
  if (lane == 0) dt[b] = d;
  const int k = 4 * lane;
  if (rows && k < K) *(f32x4*)(rows + (int64_t)b * ld_rows + k) = d * load_x4(x + (int64_t)b * ldx + k, x_bf16 != 0);
}

// dx[b, k] = sum over slices, in slice order, of the partials [n_slices][B][K], then + D_t[b] W[a_b, k]
template <typename T>
__global__ __launch_bounds__(256) void sampled_dx_merge_kernel(const float* __restrict__ ws, int B, int K, int n_slices,
                                                               const float* __restrict__ dt, const int64_t* __restrict__ targets,
                                                               const T* __restrict__ W, int64_t ldw, int N, float* __restrict__ dx,
                                                               int64_t ld_dx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // one thread per 4 columns
  const int kq = K / 4;
  if (i >= (int64_t)B * kq) return;
  const int b = (int)(i / kq), k = (int)(i % kq) * 4;
  f32x4 s = *(const f32x4*)(ws + (int64_t)b * K + k);
  for (int sl = 1; sl < n_slices; ++sl) s += *(const f32x4*)(ws + ((int64_t)sl * B + b) * K + k);
  const int64_t a = targets[b];
  if (a >= 0 && a < N) {
    const f32x4 wv = load_w4(W + a * ldw + k);
    const float d = dt[b];
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = fmaf(d, wv[e], s[e]);
  }
  *(f32x4*)(dx + (int64_t)b * ld_dx + k) = s;
}

// dcs[s] = sum over chunks, in chunk order, of the partials [chunks][S]
__global__ __launch_bounds__(256) void sampled_dc_merge_kernel(const float* __restrict__ ws, int S, int chunks, float* __restrict__ dcs) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  float v = ws[s];
  for (int ch = 1; ch < chunks; ++ch) v += ws[(int64_t)ch * S + s];
  dcs[s] = v;
}

// ---------------------------------------------------------------- scatter-sum of the S + B contributions by item id
struct SampledId {
  const int64_t* neg;
  const int64_t* tgt;
  int S;
  __device__ int64_t operator()(int j) const { return j < S ? neg[j] : tgt[j - S]; }
};
// pass 1: one wave per PIECE sorted entries; the run of each destination inside the piece is summed in list order and written at the
// run's first sorted position.  Lane owns columns 4 lane .. 4 lane + 3.
__global__ __launch_bounds__(256) void sampled_piece_kernel(const SampledId id_of, int want_w, const float* __restrict__ dWs, int64_t ld_dws,
                                                            const float* __restrict__ dcs, const float* __restrict__ x, int64_t ldx,
                                                            int x_bf16, const float* __restrict__ dt, int K,
                                                            const int* __restrict__ sorted, const int* __restrict__ total_ptr,
                                                            float* __restrict__ part, float* __restrict__ part_s) {
  const int total = *total_ptr;
  const int piece = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int p0 = piece * PIECE;
  if (p0 >= total) return;
  const int p1 = min(total, p0 + PIECE);
  const int k = 4 * lane;
  const bool mine = want_w && k < K;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  float as = 0.f;
  int first = p0;
  int64_t cur = id_of(sorted[p0]);
  for (int p = p0; p < p1; ++p) {
    const int j = sorted[p];
    if (j < id_of.S) {
      if (mine) a += *(const f32x4*)(dWs + (int64_t)j * ld_dws + k);
      if (dcs) as += dcs[j];
    } else {
      const int b = j - id_of.S;
      const float d = dt[b];
      if (mine) a += d * load_x4(x + (int64_t)b * ldx + k, x_bf16 != 0);
      as += d;
    }
    const int64_t nxt = p + 1 < p1 ? id_of(sorted[p + 1]) : -1;
    if (nxt != cur) {
      if (mine) *(f32x4*)(part + (int64_t)first * K + k) = a;
      if (lane == 0) part_s[first] = as;
      a = f32x4{0.f, 0.f, 0.f, 0.f};
      as = 0.f;
      first = p + 1;
      cur = nxt;
    }
  }
}
// pass 2: one wave per destination, the pieces of its list in order
__global__ __launch_bounds__(256) void sampled_scatter_merge_kernel(const int* __restrict__ start, int n_dest, int K,
                                                                    const float* __restrict__ part, const float* __restrict__ part_s,
                                                                    float* __restrict__ dW, int64_t ld_dw, float* __restrict__ dc) {
  const int d = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (d >= n_dest) return;
  const int s = start[d], e = start[d + 1];
  const int k = 4 * lane;
  const bool mine = dW && k < K;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  float as = 0.f;
  if (e > s) {
    for (int pc = s / PIECE; pc <= (e - 1) / PIECE; ++pc) {
      const int at = max(s, pc * PIECE);
      if (mine) a += *(const f32x4*)(part + (int64_t)at * K + k);
      as += part_s[at];
    }
  }
  if (mine) *(f32x4*)(dW + (int64_t)d * ld_dw + k) = a;
  if (dc && lane == 0) dc[d] = as;
}

// row chunks of the dW / dc role: item tiles x chunks come to about one workgroup per compute unit; a function of (B, S) alone
void chunks_of(int B, int S, int* chunks, int* tiles_per_chunk) {
  const int row_tiles = (B + BM - 1) / BM, item_tiles = (S + BN - 1) / BN;
  const int want = std::max(1, std::min(row_tiles, 256 / std::max(1, item_tiles)));
  *tiles_per_chunk = std::max(1, (row_tiles + want - 1) / want);
  *chunks = std::max(1, (row_tiles + *tiles_per_chunk - 1) / *tiles_per_chunk);
}
inline int64_t r256(int64_t b) { return (b + 255) / 256 * 256; }

bool shape_ok(const char* who, int B, int S, int N, int items_per_slice, int* n_slices) {
  if (S == 0) {
    recnn_set_error("%s: S = 0: the list of negatives is empty (at least one is needed)", who);
    return false;
  }
  if (!(B >= 0 && N >= 1 && S >= 1 && slices_of(S, items_per_slice, n_slices))) {
    recnn_set_error("%s: need B >= 0, N >= 1, S >= 1 and items_per_slice a positive multiple of 128 (got %d, %d, %d, %d)", who, B, N, S,
                    items_per_slice);
    return false;
  }
  return true;
}
bool width_ok(const char* who, int K, int w_bf16) {
  const int bk = w_bf16 ? 64 : 32;
  if (!(K >= bk && K % bk == 0)) {
    recnn_set_error("%s: K must be a positive multiple of %d (got %d)", who, bk, K);
    return false;
  }
  if (K > KMAX) {
    recnn_set_error("%s: K = %d is above the limit of %d (padded) the kernels are built for", who, K, KMAX);
    return false;
  }
  return true;
}
}  // namespace

extern "C" int recnn_sampled_logprob_workspace_bytes(int B, int S, int items_per_slice, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes, "sampled_logprob_workspace_bytes: null pointer");
  int n_slices = 0;
  if (!shape_ok("sampled_logprob_workspace_bytes", B, S, 1, items_per_slice, &n_slices)) return RECNN_E_INVALID;
  *h_bytes = (int64_t)2 * n_slices * B * 4;
  return 0;
}

extern "C" int recnn_sampled_logprob(const float* x, int64_t ld_x, int B, int K, const void* W, int64_t ld_w, int w_bf16, const float* c, int N,
                                     const int64_t* targets, const int64_t* negatives, int S, const float* target_log_q,
                                     const float* negative_log_q, int remove_hits, int items_per_slice, float* logprob, float* lse,
                                     float* z_target, void* workspace, void* stream) {
  int n_slices = 0;
  if (!shape_ok("sampled_logprob", B, S, N, items_per_slice, &n_slices) || !width_ok("sampled_logprob", K, w_bf16)) return RECNN_E_INVALID;
  RECNN_REQUIRE(W && negatives && ((x && targets && logprob && lse && z_target && workspace) || B == 0), "sampled_logprob: null pointer");
  RECNN_REQUIRE(ld_x >= K && ld_x % 4 == 0 && ld_w >= K && ld_w % (w_bf16 ? 8 : 4) == 0 && aligned16(x, W),
                "sampled_logprob: x / W rows must be 16-byte aligned and at least K long");
  RECNN_REQUIRE(((uintptr_t)workspace & 3) == 0, "sampled_logprob: workspace must be 4-byte aligned");
  if (B == 0) return 0;
  RECNN_REQUIRE(n_slices <= 65535, "sampled_logprob: more than 65535 slices (items_per_slice %d too small for S %d)", items_per_slice, S);
  hipStream_t s = (hipStream_t)stream;
  float* ws_m = (float*)workspace;
  float* ws_s = ws_m + (int64_t)n_slices * B;
  const dim3 grid((B + BM - 1) / BM, n_slices);
  const int tiles = items_per_slice / BN;
  const GatheredCols cols{negatives, c, negative_log_q, S, N, remove_hits != 0};
  if (w_bf16) {
    hipLaunchKernelGGL(sampled_target_kernel<bf16_t>, dim3((B + 3) / 4), dim3(256), 0, s, x, ld_x, B, K, (const bf16_t*)W, ld_w, c, N, targets,
                       target_log_q, z_target);
    hipLaunchKernelGGL((logprob_slice_kernel<bf16_t, GatheredCols>), grid, dim3(256), 0, s, x, ld_x, B, K, (const bf16_t*)W, ld_w, cols,
                       targets, tiles, ws_m, ws_s, (float*)nullptr);
  } else {
    hipLaunchKernelGGL(sampled_target_kernel<float>, dim3((B + 3) / 4), dim3(256), 0, s, x, ld_x, B, K, (const float*)W, ld_w, c, N, targets,
                       target_log_q, z_target);
    hipLaunchKernelGGL((logprob_slice_kernel<float, GatheredCols>), grid, dim3(256), 0, s, x, ld_x, B, K, (const float*)W, ld_w, cols, targets,
                       tiles, ws_m, ws_s, (float*)nullptr);
  }
  hipLaunchKernelGGL(sampled_merge_kernel, dim3((B + 255) / 256), dim3(256), 0, s, (const float*)ws_m, (const float*)ws_s,
                     (const float*)z_target, B, n_slices, logprob, lse);
  return recnn_check_hip(hipGetLastError(), "sampled_logprob");
}

extern "C" int recnn_sampled_logprob_bwd_workspace_bytes(int B, int S, int K, int items_per_slice, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes, "sampled_logprob_bwd_workspace_bytes: null pointer");
  int n_slices = 0;
  if (!shape_ok("sampled_logprob_bwd_workspace_bytes", B, S, 1, items_per_slice, &n_slices) ||
      !width_ok("sampled_logprob_bwd_workspace_bytes", K, 0))
    return RECNN_E_INVALID;
  int chunks, tpc;
  chunks_of(B, S, &chunks, &tpc);
  *h_bytes = r256((int64_t)n_slices * B * K * 4) + (chunks > 1 ? r256((int64_t)chunks * S * K * 4) + r256((int64_t)chunks * S * 4) : 0);
  return 0;
}

extern "C" int recnn_sampled_logprob_bwd(const float* x, int64_t ld_x, int B, int K, const void* W, int64_t ld_w, int w_bf16, const float* c,
                                         int N, const int64_t* targets, const int64_t* negatives, int S, const float* negative_log_q,
                                         int remove_hits, const float* lse, const float* z_target, const float* g_lp, const float* g_lse,
                                         int items_per_slice, float* dx, int64_t ld_dx, float* dWs, int64_t ld_dws, float* dcs,
                                         float* d_target, float* dWt, int64_t ld_dwt, void* workspace, void* stream) {
  int n_slices = 0;
  if (!shape_ok("sampled_logprob_bwd", B, S, N, items_per_slice, &n_slices) || !width_ok("sampled_logprob_bwd", K, w_bf16)) return RECNN_E_INVALID;
  RECNN_REQUIRE(W && negatives && ((x && targets && lse && z_target && d_target && workspace) || B == 0), "sampled_logprob_bwd: null pointer");
  RECNN_REQUIRE(ld_x >= K && ld_x % 4 == 0 && ld_w >= K && ld_w % (w_bf16 ? 8 : 4) == 0 && aligned16(x, W),
                "sampled_logprob_bwd: x / W rows must be 16-byte aligned and at least K long");
  RECNN_REQUIRE((!dx || (ld_dx >= K && ld_dx % 4 == 0)) && (!dWs || (ld_dws >= K && ld_dws % 4 == 0)) &&
                    (!dWt || (ld_dwt >= K && ld_dwt % 4 == 0)) && aligned16(dx, dWs, dWt) && ((uintptr_t)workspace & 15) == 0,
                "sampled_logprob_bwd: dx / dWs / dWt rows and the workspace must be 16-byte aligned, rows at least K long");
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {
    if (dWs) RECNN_HIP(hipMemset2DAsync(dWs, (size_t)ld_dws * 4, 0, (size_t)K * 4, (size_t)S, s));
    if (dcs) RECNN_HIP(hipMemsetAsync(dcs, 0, (size_t)S * 4, s));
    return 0;
  }
  RECNN_REQUIRE(n_slices <= 65535, "sampled_logprob_bwd: more than 65535 slices (items_per_slice %d too small for S %d)", items_per_slice, S);
  const int row_tiles = (B + BM - 1) / BM, item_tiles = (S + BN - 1) / BN;
  const int tiles = items_per_slice / BN;
  int chunks, tpc;
  chunks_of(B, S, &chunks, &tpc);
  char* wsb = (char*)workspace;
  float* ws_dx = (float*)wsb;
  float* ws_dw = (float*)(wsb + r256((int64_t)n_slices * B * K * 4));
  float* ws_dc = (float*)((char*)ws_dw + r256((int64_t)chunks * S * K * 4));
  const GatheredCols cols{negatives, c, negative_log_q, S, N, remove_hits != 0};

  hipLaunchKernelGGL(sampled_dt_kernel, dim3((B + 3) / 4), dim3(256), 0, s, z_target, lse, g_lp, g_lse, B, d_target, x, ld_x, K, w_bf16, dWt,
                     ld_dwt);
  if (dx) {
    const dim3 grid(row_tiles, n_slices);
    const int64_t quads = (int64_t)B * (K / 4);
    const dim3 mgrid((unsigned)((quads + 255) / 256));
    if (w_bf16) {
      launch_bwd<bf16_t, true, GatheredCols>(K, grid, s, x, ld_x, B, K, (const bf16_t*)W, ld_w, cols, targets, lse, g_lp, g_lse, tiles, ws_dx,
                                             (int64_t)K, (float*)nullptr);
      hipLaunchKernelGGL(sampled_dx_merge_kernel<bf16_t>, mgrid, dim3(256), 0, s, (const float*)ws_dx, B, K, n_slices,
                         (const float*)d_target, targets, (const bf16_t*)W, ld_w, N, dx, ld_dx);
    } else {
      launch_bwd<float, true, GatheredCols>(K, grid, s, x, ld_x, B, K, (const float*)W, ld_w, cols, targets, lse, g_lp, g_lse, tiles, ws_dx,
                                            (int64_t)K, (float*)nullptr);
      hipLaunchKernelGGL(sampled_dx_merge_kernel<float>, mgrid, dim3(256), 0, s, (const float*)ws_dx, B, K, n_slices, (const float*)d_target,
                         targets, (const float*)W, ld_w, N, dx, ld_dx);
    }
  }
  if (dWs || dcs) {
    const dim3 grid(item_tiles, chunks);
    const bool direct = chunks == 1;
    float* out = dWs ? (direct ? dWs : ws_dw) : nullptr;
    const int64_t ld_out = direct ? ld_dws : K;
    float* dc = dcs ? (direct ? dcs : ws_dc) : nullptr;
    if (w_bf16)
      launch_bwd<bf16_t, false, GatheredCols>(K, grid, s, x, ld_x, B, K, (const bf16_t*)W, ld_w, cols, targets, lse, g_lp, g_lse, tpc, out,
                                              ld_out, dc);
    else
      launch_bwd<float, false, GatheredCols>(K, grid, s, x, ld_x, B, K, (const float*)W, ld_w, cols, targets, lse, g_lp, g_lse, tpc, out,
                                             ld_out, dc);
    if (!direct) {
      const int64_t quads = (int64_t)S * (K / 4);
      if (dWs)
        hipLaunchKernelGGL(logprob_bwd_merge_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, (const float*)ws_dw, S, K, chunks,
                           dWs, ld_dws);
      if (dcs) hipLaunchKernelGGL(sampled_dc_merge_kernel, dim3((S + 255) / 256), dim3(256), 0, s, (const float*)ws_dc, S, chunks, dcs);
    }
  }
  return recnn_check_hip(hipGetLastError(), "sampled_logprob_bwd");
}

extern "C" int recnn_sampled_scatter_workspace_bytes(int B, int S, int N, int K, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes && B >= 0 && S >= 0 && N >= 1 && K >= 4 && K % 4 == 0 && K <= KMAX && (int64_t)B + S < (1LL << 31),
                "sampled_scatter_workspace_bytes: need B, S >= 0, N >= 1 and K a multiple of 4 up to %d (got %d, %d, %d, %d)", KMAX, B, S, N, K);
  const int64_t M = (int64_t)B + S;
  *h_bytes = scatter_index_bytes(M, N) + r256(4LL * M * K) + r256(4LL * M) + scatter_scan_scratch_bytes(N);
  return 0;
}

extern "C" int recnn_sampled_scatter(const int64_t* negatives, int S, const int64_t* targets, int B, const float* dWs, int64_t ld_dws,
                                     const float* dcs, const float* x, int64_t ld_x, int x_bf16, const float* d_target, int K, int N,
                                     float* dW, int64_t ld_dw, float* dc, void* workspace, void* stream) {
  RECNN_REQUIRE(B >= 0 && S >= 0 && N >= 1 && K >= 4 && K % 4 == 0 && K <= KMAX && (int64_t)B + S < (1LL << 31),
                "sampled_scatter: need B, S >= 0, N >= 1 and K a multiple of 4 up to %d (got %d, %d, %d, %d)", KMAX, B, S, N, K);
  RECNN_REQUIRE(workspace && (dW || dc) && (negatives || S == 0) && ((targets && d_target) || B == 0), "sampled_scatter: null pointer");
  RECNN_REQUIRE(!dW || ((dWs || S == 0) && (x || B == 0) && ld_dw >= K && ld_dw % 4 == 0 && (!dWs || (ld_dws >= K && ld_dws % 4 == 0)) &&
                        (!x || (ld_x >= K && ld_x % 4 == 0)) && aligned16(dW, dWs, x)),
                "sampled_scatter: dW needs dWs and x, rows 16-byte aligned and at least K long");
  RECNN_REQUIRE(!dc || dcs || S == 0, "sampled_scatter: dc needs dcs");
  RECNN_REQUIRE(((uintptr_t)workspace & 15) == 0, "sampled_scatter: the workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int M = B + S;
  char* p = (char*)workspace;
  const ScatterIndex ix = scatter_index_carve(p, M, N);
  float* part = (float*)p;
  float* part_s = (float*)(p + r256(4LL * M * K));
  int* scan_scratch = (int*)(p + r256(4LL * M * K) + r256(4LL * M));
  const SampledId id_of{negatives, targets, S};
  // few ids into a large catalogue: rank by contribution, scan the counts in chunks
  RECNN_HIP(scatter_index_build(ix, id_of, M, N, s, M < N, scan_scratch));
  if (M) {
    // (dropped ids are not in the lists: the pieces cover the first start[N] sorted entries)
    const int pieces = (M + PIECE - 1) / PIECE;
    hipLaunchKernelGGL(sampled_piece_kernel, dim3((pieces + 3) / 4), dim3(256), 0, s, id_of, dW != nullptr, dWs, ld_dws, dc ? dcs : nullptr, x,
                       ld_x, x_bf16, d_target, K, (const int*)ix.sorted, (const int*)(ix.start + N), part, part_s);
  }
  hipLaunchKernelGGL(sampled_scatter_merge_kernel, dim3((N + 3) / 4), dim3(256), 0, s, (const int*)ix.start, N, K, (const float*)part,
                     (const float*)part_s, dW, ld_dw, dc);
  return recnn_check_hip(hipGetLastError(), "sampled_scatter");
}
