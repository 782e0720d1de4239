// qrank.hip -- the critic's Q-value of every (state row, catalogue item) pair, for ranking a catalogue by value (gfx950).
//
//   S1[b, :] = state[b] . W1[:, :S]^T + b1        qrank_layer1_kernel, once per state row
//   E1[n, :] = table[n] . W1[:, S:]^T             qrank_layer1_kernel, once per index
//   Q[b, n]  = w3 . relu(W2 . relu(S1[b] + E1[n]) + b2) + b3        qrank_pair_kernel: 2 H^2 flops per pair, nothing per pair in memory
//
// DESIGN.md section 22.  Pair kernel: a workgroup owns 16 state rows x 16 items = 256 pair rows.  Wave w owns state rows 4w .. 4w+3;
// one of its four MFMA row tiles is (one state row) x (the 16 items).  The pair activation relu(S1[b, k] + E1[n, k]) is formed in
// registers as the A operand of v_mfma_f32_16x16x4_f32 (exact fp32) from the two LDS tiles; W2 streams through LDS in slabs of 16 k
// values (HP x 16 floats, register-staged: the next slab's loads are in flight while this one is multiplied), each slab shared by the
// 256 pair rows.  The wave keeps all HP output columns of its 64 pair rows in accumulators (HP / 16 column tiles x 4 row tiles), so the
// epilogue -- + b2, relu, . w3 over the columns -- needs no other wave: per lane over its column tiles in ascending order, then a fixed
// butterfly over the 16 lanes of a row.
//
// Bit-invariance: the k order of a pair's contraction (slab, then the four MFMAs of a slab, each contracting its four k values in the
// instruction's own order) and the column order of its epilogue are the same for every pair, whatever its place in a tile and whatever
// B, N or the row blocking.  The layer-1 kernel likewise contracts each output element over k in one fixed chain.  No atomics.
#include "common.h"

namespace {
constexpr int QR_TB = 16;      // state rows per workgroup
constexpr int QR_TN = 16;      // items per workgroup
constexpr int QR_KS = 16;      // k values per W2 slab
constexpr int QR_WP = QR_KS + 4;   // floats per LDS row of a slab (+4 pad: conflict-light b128 reads)
constexpr int QR_HMAX = 256;
constexpr int QR_GRANULE = 64; // H is zero-padded to a multiple of this (the column-tile counts the kernel is compiled for)

struct PairArgs {
  const float* s1; int64_t ld_s1; int B;
  const float* e1; int64_t ld_e1; int N;
  const float* w2;     // [HP][HP] row j = output column j, contiguous over k
  const float* b2;     // [HP]
  const float* w3;     // [HP]
  float b3;
  float* out; int64_t ld_out;
};

template <int HP>
__global__ __launch_bounds__(256) void qrank_pair_kernel(const PairArgs a) {
  constexpr int NCT = HP / 16;          // column tiles
  constexpr int PS = HP + 4;            // floats per LDS row of the S1 / E1 tiles
  constexpr int STAGE = HP * (QR_KS / 4) / 256;   // float4 per thread per slab
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Ss = (float*)smem;             // [QR_TB][PS]
  float* Es = Ss + QR_TB * PS;          // [QR_TN][PS]
  float* Ws = Es + QR_TN * PS;          // [HP][QR_WP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int n0 = blockIdx.x * QR_TN, b0 = blockIdx.y * QR_TB;

  f32x4 stage[STAGE];
  const float* wsrc = a.w2 + (int64_t)(tid >> 2) * HP + (tid & 3) * 4;     // this thread's float4 of a slab; the next ones are 64 rows on
#pragma unroll
  for (int s = 0; s < STAGE; ++s) stage[s] = *(const f32x4*)(wsrc + (int64_t)s * 64 * HP);
  // S1 and E1 tiles -> LDS (rows past B / N are zero; their results are not stored)
  for (int c = tid; c < QR_TB * (HP / 4); c += 256) {
    const int r = c / (HP / 4), k4 = c % (HP / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b0 + r < a.B) v = *(const float4*)(a.s1 + (int64_t)(b0 + r) * a.ld_s1 + k4 * 4);
    *(float4*)&Ss[r * PS + k4 * 4] = v;
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n0 + r < a.N) u = *(const float4*)(a.e1 + (int64_t)(n0 + r) * a.ld_e1 + k4 * 4);
    *(float4*)&Es[r * PS + k4 * 4] = u;
  }

  f32x4 acc[4][NCT];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[mt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int k0 = 0; k0 < HP; k0 += QR_KS) {
    __syncthreads();                      // the previous slab's readers are done (first pass: nothing to wait for)
#pragma unroll
    for (int s = 0; s < STAGE; ++s) {
      const int c = tid + s * 256;
      *(f32x4*)&Ws[(c >> 2) * QR_WP + (c & 3) * 4] = stage[s];
    }
    __syncthreads();                      // (first pass: the S1 / E1 tiles are complete too)
    if (k0 + QR_KS < HP) {
#pragma unroll
      for (int s = 0; s < STAGE; ++s) stage[s] = *(const f32x4*)(wsrc + (int64_t)s * 64 * HP + k0 + QR_KS);
    }
    // A fragments: lane (fr, fg) holds pair row fr (= item fr) at k = k0 + fg * 4 + e
    const f32x4 ef = *(const f32x4*)&Es[fr * PS + k0 + fg * 4];
    float av[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const f32x4 sf = *(const f32x4*)&Ss[(wave * 4 + mt) * PS + k0 + fg * 4];
#pragma unroll
      for (int e = 0; e < 4; ++e) av[mt][e] = fmaxf(sf[e] + ef[e], 0.f);
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const f32x4 wb = *(const f32x4*)&Ws[(ct * 16 + fr) * QR_WP + fg * 4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          acc[mt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][e], wb[e], acc[mt][ct], 0, 0, 0);
    }
  }
  // ---- epilogue: acc[mt][ct][r] = Z[state row wave*4+mt, item fg*4+r][column ct*16+fr]
  float b2v[NCT], w3v[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) { b2v[ct] = a.b2[ct * 16 + fr]; w3v[ct] = a.w3[ct * 16 + fr]; }
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int b = b0 + wave * 4 + mt;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = 0.f;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) v += fmaxf(acc[mt][ct][r] + b2v[ct], 0.f) * w3v[ct];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);      // over the 16 lanes of the row: one fixed tree
      const int n = n0 + fg * 4 + r;
      if (fr == 0 && b < a.B && n < a.N) a.out[(int64_t)b * a.ld_out + n] = v + a.b3;
      __builtin_amdgcn_sched_barrier(0);    // one pair row's accumulators at a time: the scheduler would otherwise read all 256 up front
    }
  }
}

// out[m, j] = x[m, :K] . w[j, :K] + bias[j] for j < HPc (a multiple of 64), 64 x 64 per workgroup, k in chunks of 16 through LDS.
// One MFMA chain over k per output element: its bits do not depend on M or on the element's place in a tile.
constexpr int L1_P = 16 + 4;
__global__ __launch_bounds__(256) void qrank_layer1_kernel(const float* __restrict__ x, int64_t ldx, int M, int K, const float* __restrict__ w,
                                                           int64_t ldw, const float* __restrict__ bias, float* __restrict__ out,
                                                           int64_t ldo) {
  __shared__ __attribute__((aligned(16))) float Xs[64 * L1_P];
  __shared__ __attribute__((aligned(16))) float Wt[64 * L1_P];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int m0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
  const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
  const int lr = tid >> 2, lk = (tid & 3) * 4;          // this thread's row and k offset of a 64 x 16 chunk
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 16) {
    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m0 + lr < M) xv = *(const float4*)(x + (int64_t)(m0 + lr) * ldx + k0 + lk);
    const float4 wv = *(const float4*)(w + (int64_t)(j0 + lr) * ldw + k0 + lk);
    __syncthreads();
    *(float4*)&Xs[lr * L1_P + lk] = xv;
    *(float4*)&Wt[lr * L1_P + lk] = wv;
    __syncthreads();
    float4 xa[2], wb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) xa[i] = *(const float4*)&Xs[(wm0 + i * 16 + fr) * L1_P + fg * 4];
#pragma unroll
    for (int j = 0; j < 2; ++j) wb[j] = *(const float4*)&Wt[(wn0 + j * 16 + fr) * L1_P + fg * 4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(((const float*)&xa[i])[e], ((const float*)&wb[j])[e], acc[i][j], 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = j0 + wn0 + j * 16 + fr;
      const float bv = bias ? bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm0 + i * 16 + fg * 4 + r;
        if (m < M) out[(int64_t)m * ldo + col] = acc[i][j][r] + bv;
      }
    }
}

template <int HP> int launch_pair(const PairArgs& a, hipStream_t st) {
  const size_t lds = (size_t)((QR_TB + QR_TN) * (HP + 4) + HP * QR_WP) * 4;
  hipLaunchKernelGGL(qrank_pair_kernel<HP>, dim3((a.N + QR_TN - 1) / QR_TN, (a.B + QR_TB - 1) / QR_TB), dim3(256), lds, st, a);
  return recnn_check_hip(hipGetLastError(), "qrank_pair_kernel");
}
}  // namespace

extern "C" int recnn_qrank_hidden_padded(int hidden, int* h_padded) {
  RECNN_REQUIRE(h_padded, "qrank_hidden_padded: null pointer");
  RECNN_REQUIRE(hidden > 0 && hidden <= QR_HMAX, "qrank_hidden_padded: the pair kernel takes 0 < hidden <= %d (got %d)", QR_HMAX, hidden);
  *h_padded = (hidden + QR_GRANULE - 1) / QR_GRANULE * QR_GRANULE;
  return 0;
}

extern "C" int recnn_qrank_block_rows(int n_items, int64_t max_bytes, int64_t* h_rows) {
  RECNN_REQUIRE(h_rows && n_items > 0 && max_bytes > 0, "qrank_block_rows: need n_items > 0, max_bytes > 0 and a result pointer");
  int64_t rows = max_bytes / ((int64_t)n_items * 4) / QR_TB * QR_TB;    // whole row tiles of the pair kernel
  if (rows < QR_TB) rows = QR_TB;                                       // never less than one tile, whatever the limit
  if (rows > (int64_t)65535 * QR_TB) rows = (int64_t)65535 * QR_TB;     // one launch's grid
  *h_rows = rows;
  return 0;
}

extern "C" int recnn_qrank_layer1(const float* x, int64_t ld_x, int n_rows, int k, const float* w, int64_t ld_w, const float* bias,
                                  int hidden_padded, float* out, int64_t ld_out, void* stream) {
  RECNN_REQUIRE(w && ((x && out) || n_rows == 0), "qrank_layer1: null pointer");
  RECNN_REQUIRE(n_rows >= 0 && k > 0 && k % 16 == 0, "qrank_layer1: need n_rows >= 0 and k a positive multiple of 16 (got %d)", k);
  RECNN_REQUIRE(hidden_padded > 0 && hidden_padded <= QR_HMAX && hidden_padded % QR_GRANULE == 0,
                "qrank_layer1: hidden_padded must be a multiple of %d up to %d (got %d)", QR_GRANULE, QR_HMAX, hidden_padded);
  RECNN_REQUIRE(aligned16(x, w) && ld_x % 4 == 0 && ld_w % 4 == 0 && ld_x >= k && ld_w >= k && ld_out >= hidden_padded,
                "qrank_layer1: 16-byte alignment (rows and strides), strides at least the row length");
  if (n_rows == 0) return 0;
  RECNN_REQUIRE((n_rows + 63) / 64 <= 0x7FFFFFFF / 64, "qrank_layer1: too many rows");
  hipLaunchKernelGGL(qrank_layer1_kernel, dim3((n_rows + 63) / 64, hidden_padded / 64), dim3(256), 0, (hipStream_t)stream, x, ld_x, n_rows,
                     k, w, ld_w, bias, out, ld_out);
  return recnn_check_hip(hipGetLastError(), "qrank_layer1_kernel");
}

extern "C" int recnn_qrank_scores(const float* s1, int64_t ld_s1, int n_states, const float* e1, int64_t ld_e1, int n_items,
                                  int hidden_padded, const float* w2, const float* b2, const float* w3, float b3, float* out,
                                  int64_t ld_out, void* stream) {
  RECNN_REQUIRE(e1 && w2 && b2 && w3 && ((s1 && out) || n_states == 0), "qrank_scores: null pointer");
  RECNN_REQUIRE(n_states >= 0 && n_items > 0, "qrank_scores: need n_states >= 0 and n_items > 0");
  RECNN_REQUIRE(hidden_padded > 0 && hidden_padded <= QR_HMAX && hidden_padded % QR_GRANULE == 0,
                "qrank_scores: hidden_padded must be a multiple of %d up to %d (got %d)", QR_GRANULE, QR_HMAX, hidden_padded);
  RECNN_REQUIRE(aligned16(s1, e1, w2) && ld_s1 % 4 == 0 && ld_e1 % 4 == 0 && ld_s1 >= hidden_padded && ld_e1 >= hidden_padded,
                "qrank_scores: 16-byte alignment (rows and strides), strides at least hidden_padded");
  RECNN_REQUIRE(ld_out >= n_items, "qrank_scores: ld_out is smaller than n_items");
  RECNN_REQUIRE((n_states + QR_TB - 1) / QR_TB <= 65535, "qrank_scores: at most %d state rows per call", 65535 * QR_TB);
  if (n_states == 0) return 0;
  PairArgs a;
  a.s1 = s1; a.ld_s1 = ld_s1; a.B = n_states; a.e1 = e1; a.ld_e1 = ld_e1; a.N = n_items;
  a.w2 = w2; a.b2 = b2; a.w3 = w3; a.b3 = b3; a.out = out; a.ld_out = ld_out;
  hipStream_t st = (hipStream_t)stream;
  switch (hidden_padded) {
    case 64: return launch_pair<64>(a, st);
    case 128: return launch_pair<128>(a, st);
    case 192: return launch_pair<192>(a, st);
    default: return launch_pair<256>(a, st);
  }
}
