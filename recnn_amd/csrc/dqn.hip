// dqn.hip -- the dueling DQN of the embeddings notebook (section 8 of include/recnn_hip.h; its norm clip and RAdam:
// optim.hip).
//
// Q[b, n] = V_b + A[b, n] - mean(A), A = h W^T + c over the whole catalogue.  The algebra of DESIGN.md 12 keeps the [B, N] matrix out of
// the learn step: the mean is (sum_b h_b) . (sum_n W_n) / (B N) + mean(c), the online Q at the action is one gathered-row dot, and the
// target's max_n runs as the only catalogue GEMM, with a row-max epilogue (dqn_head_kernel, MODE_MAX) that never stores A.
// Every float sum has a fixed order: column sums in fixed row chunks added in chunk order, the TD reduction as a fixed tree, and the
// scatter-sums through an inverted index built by a stable counting sort (histogram, scan, placement, per-destination rank by
// contribution index: scatter_index.h), long lists cut into pieces of PIECE entries whose partial sums are added in piece order.
// Integer atomics only (counts, and the row max on the order-preserving integer image of a float, which is exact in any order).
#include <type_traits>

#include "common.h"
#include "scatter_index.h"

namespace {

constexpr int HK = 128;          // hidden width = contraction length of the catalogue head
constexpr int PIECE = 16;        // scatter-sum: sorted entries per wave in the first pass
constexpr int CS_ROWS = 64;      // colsum: rows per workgroup chunk
constexpr int MODE_STORE = 0, MODE_MAX = 1;

__device__ inline int f2ord(float f) {
  const int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7FFFFFFF;
}
__device__ inline float ord2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7FFFFFFF); }

// ---------------------------------------------------------------- catalogue head GEMM
// One wave: 32 rows of h (two 16-row MFMA blocks) x 64 catalogue columns (four blocks) per step; the workgroup's 4 waves take 128 rows
// and walk the same column tiles (their W loads meet in the cache).  K = 128 is split across the four 16-lane groups of the wave: group
// q = lane >> 4 owns k in [32q, 32q + 32), so every lane loads contiguous 128-byte (fp32) / 64-byte (bf16) runs of its row.
template <typename T>
struct HeadFrag;
template <>
struct HeadFrag<float> {
  float v[32];
  __device__ void load(const float* row, int q) {
    const f32x4* p = (const f32x4*)(row + 32 * q);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const f32x4 x = p[i];
      v[4 * i] = x[0]; v[4 * i + 1] = x[1]; v[4 * i + 2] = x[2]; v[4 * i + 3] = x[3];
    }
  }
  __device__ void zero() {
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = 0.f;
  }
};
struct Bf16Frag {
  uint4 v[4];
  __device__ void zero() {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = make_uint4(0, 0, 0, 0);
  }
};
template <>
struct HeadFrag<bf16_t> : Bf16Frag {
  __device__ void load(const bf16_t* row, int q) {
    const uint4* p = (const uint4*)(row + 32 * q);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = p[i];
  }
};
// h is fp32 in memory in both modes; the bf16 mode rounds it to bf16 on load (round to nearest even)
__device__ inline void load_h_bf16(Bf16Frag& f, const float* row, int q) {
  const f32x4* p = (const f32x4*)(row + 32 * q);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4 a = p[2 * i], b = p[2 * i + 1];
    f.v[i] = make_uint4(cvt_pk_bf16(a[0], a[1]), cvt_pk_bf16(a[2], a[3]), cvt_pk_bf16(b[0], b[1]), cvt_pk_bf16(b[2], b[3]));
  }
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void dqn_head_kernel(const float* __restrict__ h, int64_t ldh, int B, const T* __restrict__ W, int64_t ldw,
                                                       const float* __restrict__ c, int N, int tiles_per_wg, const float* __restrict__ V,
                                                       const float* __restrict__ mu, float* __restrict__ out, int64_t ldo,
                                                       int* __restrict__ rowmax) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = lane >> 4, r16 = lane & 15;
  const int b0 = blockIdx.x * 128 + wave * 32;
  if (b0 >= B) return;
  const int ntiles = (N + 63) / 64;
  const int t0 = blockIdx.y * tiles_per_wg;
  const int t1 = min(ntiles, t0 + tiles_per_wg);
  if (t0 >= t1) return;

  // this lane's A fragments: rows b0 + 16 tm + r16
  constexpr bool F32 = sizeof(T) == 4;
  typedef typename std::conditional<F32, HeadFrag<float>, Bf16Frag>::type AFrag;
  AFrag a[2];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm) {
    const int b = b0 + 16 * tm + r16;
    if (b < B) {
      if constexpr (F32) ((HeadFrag<float>&)a[tm]).load(h + (int64_t)b * ldh, q);
      else load_h_bf16((Bf16Frag&)a[tm], h + (int64_t)b * ldh, q);
    } else {
      a[tm].zero();
    }
  }
  float vrow[2][4], runmax[2][4];
  const float m0 = MODE == MODE_STORE ? mu[0] : 0.f;
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int b = b0 + 16 * tm + 4 * q + r;
      vrow[tm][r] = (MODE == MODE_STORE && b < B) ? V[b] - m0 : 0.f;
      runmax[tm][r] = -INFINITY;
    }

  for (int t = t0; t < t1; ++t) {
    const int n0 = t * 64;
    HeadFrag<T> w[4];
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      const int n = n0 + 16 * tn + r16;
      if (n < N) w[tn].load(W + (int64_t)n * ldw, q);
      else w[tn].zero();
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (F32) {
#pragma unroll
      for (int s = 0; s < 32; ++s)
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
          for (int tn = 0; tn < 4; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(((HeadFrag<float>&)a[tm]).v[s], w[tn].v[s], acc[tm][tn], 0, 0, 0);
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
          for (int tn = 0; tn < 4; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ((Bf16Frag&)a[tm]).v[s]),
                                                                  __builtin_bit_cast(bf16x8, w[tn].v[s]), acc[tm][tn], 0, 0, 0);
    }
    // C/D: lane holds rows 4q + r of the 16-row block, column r16
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      const int n = n0 + 16 * tn + r16;
      if (n >= N) continue;
      const float cn = c[n];
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float adv = acc[tm][tn][r] + cn;
          if (MODE == MODE_STORE) {
            const int b = b0 + 16 * tm + 4 * q + r;
            if (b < B) out[(int64_t)b * ldo + n] = adv + vrow[tm][r];
          } else {
            runmax[tm][r] = fmaxf(runmax[tm][r], adv);
          }
        }
    }
  }
  if (MODE == MODE_MAX) {
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float m = runmax[tm][r];
        m = fmaxf(m, __shfl_xor(m, 8));
        m = fmaxf(m, __shfl_xor(m, 4));
        m = fmaxf(m, __shfl_xor(m, 2));
        m = fmaxf(m, __shfl_xor(m, 1));
        const int b = b0 + 16 * tm + 4 * q + r;
        if (r16 == 0 && b < B) atomicMax(rowmax + b, f2ord(m));
      }
  }
}

__global__ void fill_i32_kernel(int* p, int n, int v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// ---------------------------------------------------------------- row dots, column sums, mean
// out[b] = x_b . w[idx_b] + bias[idx_b] (idx NULL: row 0 of w and bias[0]); one wave per row, lanes own k and k + 64, fixed tree.
__global__ __launch_bounds__(256) void dqn_row_dot_kernel(const float* __restrict__ x, int64_t ldx, int rows, const float* __restrict__ w,
                                                          int64_t ldw, const int64_t* __restrict__ idx, int n_w,
                                                          const float* __restrict__ bias, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= rows) return;
  int64_t j = idx ? idx[b] : 0;
  const bool ok = j >= 0 && j < n_w;
  if (!ok) j = 0;
  const float* xr = x + (int64_t)b * ldx;
  const float* wr = w + j * ldw;
  float s = xr[lane] * wr[lane] + xr[lane + 64] * wr[lane + 64];
  s = wave_sum(s);
  if (lane == 0) out[b] = ok ? s + (bias ? bias[j] : 0.f) : __int_as_float(0x7FC00000);
}

// part[chunk][col] = sum of rows [chunk * CS_ROWS, ...) in row order; one thread per column (cols <= 256)
__global__ __launch_bounds__(256) void dqn_colsum_part_kernel(const float* __restrict__ x, int64_t ldx, int rows, int cols,
                                                              float* __restrict__ part) {
  const int col = threadIdx.x;
  if (col >= cols) return;
  const int r0 = blockIdx.x * CS_ROWS, r1 = min(rows, r0 + CS_ROWS);
  float s = 0.f;
#pragma unroll 8
  for (int r = r0; r < r1; ++r) s += x[(int64_t)r * ldx + col];
  part[(int64_t)blockIdx.x * cols + col] = s;
}
// out[col] = scale * sum of the chunk partials: thread t adds chunks t, t + 256, ... in order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void dqn_colsum_final_kernel(const float* __restrict__ part, int chunks, int cols, float* __restrict__ out,
                                                               float scale) {
  __shared__ float red[4];
  const int col = blockIdx.x;
  float s = 0.f;
  for (int k = threadIdx.x; k < chunks; k += 256) s += part[(int64_t)k * cols + col];
  s = block_sum256(s, red);
  if (threadIdx.x == 0) out[col] = s * scale;
}

// mu = (sh . sw) / (B N) + sc / N: the mean of A = h W^T + c over [B, N]
__device__ inline float head_mean(const float* sh, const float* sw, float sc, int B, int N) {
  float d = 0.f;
  for (int k = 0; k < HK; ++k) d += sh[k] * sw[k];
  return d / ((float)B * (float)N) + sc / (float)N;
}
__global__ void dqn_mean_kernel(const float* sh, const float* sw, const float* sc, int B, int N, float* mu) {
  if (threadIdx.x == 0) mu[0] = head_mean(sh, sw, sc[0], B, N);
}

// ---------------------------------------------------------------- TD step
// One workgroup.  stats: [0] loss, [1] G = sum g, [2] kappa = G / (B N), [3] G / N, [4] mu, [5] mu', [6] clip coefficient slot (unused here)
__global__ __launch_bounds__(256) void dqn_td_kernel(const float* __restrict__ V, const float* __restrict__ adv, const float* __restrict__ Vt,
                                                     const int* __restrict__ rowmax, const float* __restrict__ reward,
                                                     const float* __restrict__ done, float gamma, int B, int N, const float* __restrict__ sh,
                                                     const float* __restrict__ sw, const float* __restrict__ sc, const float* __restrict__ sht,
                                                     const float* __restrict__ swt, const float* __restrict__ sct, float* __restrict__ q_out,
                                                     float* __restrict__ g_out, float* __restrict__ stats) {
  __shared__ float mus[2];
  __shared__ float red[4];
  if (threadIdx.x == 0) mus[0] = head_mean(sh, sw, sc[0], B, N);
  if (threadIdx.x == 64) mus[1] = head_mean(sht, swt, sct[0], B, N);
  __syncthreads();
  const float mu = mus[0], mut = mus[1];
  float l = 0.f, gs = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float q = V[b] + adv[b] - mu;
    const float nq = Vt[b] + ord2f(rowmax[b]) - mut;
    const float y = reward[b] + gamma * nq * (1.f - done[b]);
    const float d = q - y;
    const float g = 2.f * d / (float)B;
    if (q_out) q_out[b] = q;
    if (g_out) g_out[b] = g;
    l += d * d;
    gs += g;
  }
  const float lt = block_sum256(l, red);
  const float gt = block_sum256(gs, red);
  if (threadIdx.x == 0) {
    stats[0] = lt / (float)B;
    stats[1] = gt;
    stats[2] = gt / ((float)B * (float)N);
    stats[3] = gt / (float)N;
    stats[4] = mu;
    stats[5] = mut;
  }
}

// dh = [dha | dhv] ([rows, 256]): dha = [ha > 0] (g_b W[a_b] - kappa sum_n W_n), dhv = [hv > 0] g_b wv
__global__ __launch_bounds__(256) void dqn_dh_kernel(const float* __restrict__ h2, int64_t ldh, int B, const float* __restrict__ W,
                                                     int64_t ldw, int N, const int64_t* __restrict__ act, const float* __restrict__ sw,
                                                     const float* __restrict__ wv, const float* __restrict__ g,
                                                     const float* __restrict__ stats, float* __restrict__ dh) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (b >= B) return;
  const float gb = g[b];
  const float hv = h2[(int64_t)b * ldh + k];
  float d;
  if (k < HK) {
    int64_t a = act[b];
    const float wa = (a >= 0 && a < N) ? W[a * ldw + k] : 0.f;
    d = gb * wa - stats[2] * sw[k];
  } else {
    d = gb * wv[k - HK];
  }
  dh[(int64_t)b * 2 * HK + k] = hv > 0.f ? d : 0.f;
}

// ---------------------------------------------------------------- deterministic scatter-sum
// contribution j (j < rows * per_row): source row src + (j / per_row) ld + (j % per_row) 128, weight scale[j / per_row] (1 if NULL),
// destination ids[(j / per_row) ld_ids + j % per_row].  Ids outside [0, n_dest) are dropped.
struct ScatterWs {
  ScatterIndex ix;  // count, start, slot, placed, sorted (scatter_index.h)
  float* part;      // [M][128] piece partial rows
  float* part_s;    // [M] piece partial weights
};
// the destination of contribution j: for the index build (scatter_index.h) and, through contrib_id, for the float passes
struct MatrixId {
  const int64_t* ids;
  int64_t ld_ids;
  int per_row;
  __device__ int64_t operator()(int j) const { return ids[(int64_t)(j / per_row) * ld_ids + j % per_row]; }
};
__device__ inline int contrib_id(const int64_t* ids, int64_t ld_ids, int per_row, int j) {
  return (int)MatrixId{ids, ld_ids, per_row}(j);
}
// pass 1: one wave per PIECE sorted entries; the run of each destination inside the piece is summed in list order and written at the
// run's first sorted position.  Lanes own columns lane and lane + 64.
__global__ __launch_bounds__(256) void scatter_piece_kernel(const float* __restrict__ src, int64_t ld_src, int per_row,
                                                            const int64_t* __restrict__ ids, int64_t ld_ids, const float* __restrict__ scale,
                                                            const int* __restrict__ sorted, const int* __restrict__ total_ptr,
                                                            float* __restrict__ part, float* __restrict__ part_s) {
  const int total = *total_ptr;
  const int piece = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int p0 = piece * PIECE;
  if (p0 >= total) return;
  const int p1 = min(total, p0 + PIECE);
  float a0 = 0.f, a1 = 0.f, as = 0.f;
  int first = p0;
  int cur = contrib_id(ids, ld_ids, per_row, sorted[p0]);
  for (int p = p0; p < p1; ++p) {
    const int j = sorted[p];
    const int row = j / per_row;
    const float w = scale ? scale[row] : 1.f;
    const float* s = src + (int64_t)row * ld_src + (int64_t)(j % per_row) * HK;
    a0 += w * s[lane];
    a1 += w * s[lane + 64];
    as += w;
    const int nxt = p + 1 < p1 ? contrib_id(ids, ld_ids, per_row, sorted[p + 1]) : -1;
    if (nxt != cur) {
      part[(int64_t)first * HK + lane] = a0;
      part[(int64_t)first * HK + lane + 64] = a1;
      if (lane == 0) part_s[first] = as;
      a0 = a1 = as = 0.f;
      first = p + 1;
      cur = nxt;
    }
  }
}
// pass 2: one wave per destination, the pieces of its list in order; out = S - coef[0] rank1, out_s = s - coef[1] (rank1 / coef NULL: 0).
__global__ __launch_bounds__(256) void scatter_merge_kernel(const int* __restrict__ start, int n_dest, const float* __restrict__ part,
                                                            const float* __restrict__ part_s, float* __restrict__ out,
                                                            float* __restrict__ out_s, const float* __restrict__ rank1,
                                                            const float* __restrict__ coef) {
  const int d = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (d >= n_dest) return;
  const int s = start[d], e = start[d + 1];
  float a0 = 0.f, a1 = 0.f, as = 0.f;
  if (e > s) {
    for (int k = s / PIECE; k <= (e - 1) / PIECE; ++k) {
      const int at = max(s, k * PIECE);
      a0 += part[(int64_t)at * HK + lane];
      a1 += part[(int64_t)at * HK + lane + 64];
      as += part_s[at];
    }
  }
  if (rank1) {
    const float k0 = coef[0];
    a0 -= k0 * rank1[lane];
    a1 -= k0 * rank1[lane + 64];
  }
  out[(int64_t)d * HK + lane] = a0;
  out[(int64_t)d * HK + lane + 64] = a1;
  if (out_s && lane == 0) out_s[d] = coef ? as - coef[1] : as;
}

}  // namespace

extern "C" int recnn_dqn_head(const float* h, int64_t ldh, int B, const void* W, int64_t ldw, int w_bf16, const float* c, int N,
                              const float* V, const float* mu, float* out, int64_t ldo, int32_t* rowmax, void* stream) {
  RECNN_REQUIRE(h && W && c && B >= 0 && N >= 1 && (out != nullptr) != (rowmax != nullptr), "dqn_head: bad arguments");
  RECNN_REQUIRE(!out || (V && mu && ldo >= N), "dqn_head: store mode needs V, mu and ldo >= N");
  RECNN_REQUIRE(aligned16(h, W) && ldh % 4 == 0 && ldh >= HK && ldw >= HK && ldw % (w_bf16 ? 8 : 4) == 0,
                "dqn_head: h / W rows must be 16-byte aligned, 128 wide");
  if (B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int ntiles = (N + 63) / 64, gx = (B + 127) / 128;
  int gy = (2048 + gx - 1) / gx;
  if (gy > ntiles) gy = ntiles;
  const int per = (ntiles + gy - 1) / gy;
  gy = (ntiles + per - 1) / per;
  if (rowmax) hipLaunchKernelGGL(fill_i32_kernel, dim3((B + 255) / 256), dim3(256), 0, s, (int*)rowmax, B, (int)0x807FFFFF);
#define HEAD_GO(T, MODE)                                                                                                            \
  hipLaunchKernelGGL((dqn_head_kernel<T, MODE>), dim3(gx, gy), dim3(256), 0, s, h, ldh, B, (const T*)W, ldw, c, N, per, V, mu, out, \
                     ldo, (int*)rowmax)
  if (w_bf16) { if (out) HEAD_GO(bf16_t, MODE_STORE); else HEAD_GO(bf16_t, MODE_MAX); }
  else { if (out) HEAD_GO(float, MODE_STORE); else HEAD_GO(float, MODE_MAX); }
#undef HEAD_GO
  return recnn_check_hip(hipGetLastError(), "dqn_head");
}

extern "C" int recnn_dqn_row_dot(const float* x, int64_t ldx, int rows, const float* w, int64_t ldw, const int64_t* idx, int n_w,
                                 const float* bias, float* out, void* stream) {
  RECNN_REQUIRE(x && w && out && rows >= 0 && n_w >= 1 && ldx >= HK && ldw >= HK, "dqn_row_dot: bad arguments");
  if (rows == 0) return 0;
  hipLaunchKernelGGL(dqn_row_dot_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, ldx, rows, w, ldw, idx, n_w, bias, out);
  return recnn_check_hip(hipGetLastError(), "dqn_row_dot");
}

extern "C" int recnn_dqn_colsum_workspace_floats(int rows, int cols, int64_t* h_floats) {
  RECNN_REQUIRE(h_floats && rows >= 0 && cols >= 1 && cols <= 256, "dqn_colsum_workspace_floats: bad arguments");
  *h_floats = (int64_t)((rows + CS_ROWS - 1) / CS_ROWS + 1) * cols;
  return 0;
}
extern "C" int recnn_dqn_colsum(const float* x, int64_t ldx, int rows, int cols, float scale, float* out, float* workspace, void* stream) {
  RECNN_REQUIRE(x && out && workspace && rows >= 0 && cols >= 1 && cols <= 256 && ldx >= cols, "dqn_colsum: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const int chunks = (rows + CS_ROWS - 1) / CS_ROWS;
  if (chunks) hipLaunchKernelGGL(dqn_colsum_part_kernel, dim3(chunks), dim3(256), 0, s, x, ldx, rows, cols, workspace);
  hipLaunchKernelGGL(dqn_colsum_final_kernel, dim3(cols), dim3(256), 0, s, workspace, chunks, cols, out, scale);
  return recnn_check_hip(hipGetLastError(), "dqn_colsum");
}

extern "C" int recnn_dqn_mean(const float* sh, const float* sw, const float* sc, int B, int N, float* mu, void* stream) {
  RECNN_REQUIRE(sh && sw && sc && mu && B >= 1 && N >= 1, "dqn_mean: bad arguments");
  hipLaunchKernelGGL(dqn_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sh, sw, sc, B, N, mu);
  return recnn_check_hip(hipGetLastError(), "dqn_mean");
}

extern "C" int recnn_dqn_td(const float* V, const float* adv, const float* Vt, const int32_t* rowmax, const float* reward, const float* done,
                            float gamma, int B, int N, const float* sh, const float* sw, const float* sc, const float* sht, const float* swt,
                            const float* sct, float* q, float* g, float* stats, void* stream) {
  RECNN_REQUIRE(V && adv && Vt && rowmax && reward && done && sh && sw && sc && sht && swt && sct && stats && B >= 1 && N >= 1,
                "dqn_td: bad arguments");
  hipLaunchKernelGGL(dqn_td_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, V, adv, Vt, (const int*)rowmax, reward, done, gamma, B, N,
                     sh, sw, sc, sht, swt, sct, q, g, stats);
  return recnn_check_hip(hipGetLastError(), "dqn_td");
}

extern "C" int recnn_dqn_dh(const float* h2, int64_t ldh, int B, const float* W, int64_t ldw, int N, const int64_t* act, const float* sw,
                            const float* wv, const float* g, const float* stats, float* dh, void* stream) {
  RECNN_REQUIRE(h2 && W && act && sw && wv && g && stats && dh && B >= 0 && N >= 1 && ldh >= 2 * HK, "dqn_dh: bad arguments");
  if (B == 0) return 0;
  hipLaunchKernelGGL(dqn_dh_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, h2, ldh, B, W, ldw, N, act, sw, wv, g, stats, dh);
  return recnn_check_hip(hipGetLastError(), "dqn_dh");
}

namespace {
ScatterWs scatter_ws(void* ws, int M, int n_dest) {
  char* p = (char*)ws;
  auto take = [&](int64_t bytes) { char* r = p; p += (bytes + 255) / 256 * 256; return r; };
  ScatterWs w;
  w.ix = scatter_index_carve(p, M, n_dest);
  w.part = (float*)take(4LL * M * HK);
  w.part_s = (float*)take(4LL * M);
  return w;
}
}  // namespace

extern "C" int recnn_dqn_scatter_workspace_bytes(int64_t contributions, int n_dest, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes && contributions >= 0 && contributions < (1LL << 31) && n_dest >= 1, "dqn_scatter_workspace_bytes: bad arguments");
  const int64_t M = contributions;
  auto r = [](int64_t b) { return (b + 255) / 256 * 256; };
  *h_bytes = r(4LL * n_dest) + r(4LL * (n_dest + 1)) + 3 * r(4LL * M) + r(4LL * M * HK) + r(4LL * M);
  return 0;
}

extern "C" int recnn_dqn_scatter_sum(const float* src, int64_t ld_src, int rows, int per_row, const int64_t* ids, int64_t ld_ids,
                                     const float* scale, int n_dest, float* out, float* out_s, const float* rank1, const float* coef,
                                     void* workspace, void* stream) {
  RECNN_REQUIRE(src && ids && out && workspace && rows >= 0 && per_row >= 1 && n_dest >= 1 && ld_ids >= per_row &&
                    ld_src >= (int64_t)per_row * HK && (int64_t)rows * per_row < (1LL << 31),
                "dqn_scatter_sum: bad arguments");
  RECNN_REQUIRE(!rank1 || coef, "dqn_scatter_sum: rank1 needs coef");
  hipStream_t s = (hipStream_t)stream;
  const int M = rows * per_row;
  ScatterWs w = scatter_ws(workspace, M, n_dest);
  RECNN_HIP(scatter_index_build(w.ix, MatrixId{ids, ld_ids, per_row}, M, n_dest, s));
  if (M) {
    // (dropped ids are not in the lists: the pieces cover the first start[n_dest] sorted entries)
    const int pieces = (M + PIECE - 1) / PIECE;
    hipLaunchKernelGGL(scatter_piece_kernel, dim3((pieces + 3) / 4), dim3(256), 0, s, src, ld_src, per_row, ids, ld_ids, scale, w.ix.sorted,
                       w.ix.start + n_dest, w.part, w.part_s);
  }
  hipLaunchKernelGGL(scatter_merge_kernel, dim3((n_dest + 3) / 4), dim3(256), 0, s, w.ix.start, n_dest, w.part, w.part_s, out, out_s, rank1,
                     coef);
  return recnn_check_hip(hipGetLastError(), "dqn_scatter_sum");
}
