// topk_dev.h -- what the exact-fp32 searches share (topk.hip: the flat search and the target rank; ivf.hip: the inverted-list scan):
// the tile shape, the staging of a 64-row tile into LDS, the 64 x 64 scoring tile, the ranking key, the scan kernels' LDS layout and
// the query's squared norm.  A (query, item) pair scored through these has the same bits in every kernel: an element's k order does
// not depend on its place in a tile.  The orders and the list insert are select_dev.h's.
#pragma once
#include "common.h"
#include "select_dev.h"

namespace {
constexpr int QT = 64;     // query rows per workgroup
constexpr int IT = 64;     // items per chunk
constexpr int DIM = 128;   // embedding width (the reference's)
constexpr int SPITCH = IT + 4;   // floats per LDS row of the score tile
enum { M_IP = 0, M_L2 = 1, M_COS = 2 };

// LDS of a scan kernel (topk_scores_kernel, ivf_scan_kernel), as byte offsets; a kernel's own arrays follow from `shared`
struct ScanLds {
  static constexpr size_t Qs = 0;                             // float [QT][PITCH] query tile
  static constexpr size_t Ts = Qs + QT * PITCH * 4;           // float [IT][PITCH] chunk
  static constexpr size_t Ss = Ts + IT * PITCH * 4;           // float [QT][SPITCH] score tile
  static constexpr size_t Ls = Ss + QT * SPITCH * 4;          // float [QT][KMAX] list keys
  static constexpr size_t Li = Ls + QT * KMAX * 4;            // int [QT][KMAX] list ids
  static constexpr size_t shared = Li + QT * KMAX * 4;
};

// 64 rows of 128 floats -> the LDS tile `dst` (all 256 threads).  row_of(r, row) tells whether tile row r exists and, if so, which row
// of `src` (row stride ld) it is; a row that does not exist is zero
template <class RowOf>
__device__ __forceinline__ void stage_rows(float* dst, const float* src, int64_t ld, int tid, RowOf row_of) {
  for (int c = tid; c < 64 * (DIM / 4); c += 256) {
    const int r = c / (DIM / 4), k4 = c % (DIM / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    int64_t row;
    if (row_of(r, row)) v = *(const float4*)(src + row * ld + k4 * 4);
    *(float4*)&dst[r * PITCH + k4 * 4] = v;
  }
}

// rows n0 .. n0 + 63 of a [.][128] table -> Ts; rows from n_end on are zero
__device__ __forceinline__ void stage_chunk(float* Ts, const float* table, int n0, int n_end, int tid) {
  stage_rows(Ts, table, DIM, tid, [&](int r, int64_t& row) { row = n0 + r; return n0 + r < n_end; });
}

// 64 x 64 scores of the query tile against the 64 rows in Ts: one k order for every element of the tile
__device__ __forceinline__ void score_tile(const float* Qs, const float* Ts, int wm0, int wn0, int fr, int fg, f32x4 (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int ks = 0; ks < DIM / 16; ++ks) {
    float4 qa[2], tb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) qa[i] = *(const float4*)&Qs[(wm0 + i * 16 + fr) * PITCH + ks * 16 + fg * 4];
#pragma unroll
    for (int j = 0; j < 2; ++j) tb[j] = *(const float4*)&Ts[(wn0 + j * 16 + fr) * PITCH + ks * 16 + fg * 4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(((const float*)&qa[i])[e], ((const float*)&tb[j])[e], acc[i][j], 0, 0, 0);
  }
}

// the ranking key (larger = better) of a score q.t; ax: the item's |t|^2 (L2) or 1/|t| (COS).  L2 leaves |q|^2 out: it is constant
// per row and does not change the order
__device__ __forceinline__ float rank_score(float s, float ax, int metric) {
  if (metric == M_L2) s = 2.f * s - ax;
  else if (metric == M_COS) s = s * ax;
  return s;
}

// the keys of a scored chunk (items n0 .. n0 + 63, `aux` indexed like them) into the score tile; columns from n_end on get -inf
__device__ __forceinline__ void keys_to_tile(const f32x4 (&acc)[2][2], float* Ss, const float* aux, int metric, int n0,
                                             int n_end, int wm0, int wn0, int fr, int fg) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = wn0 + j * 16 + fr;
      const int n = n0 + col;
      float ax = 0.f;
      if (metric != M_IP && n < n_end) ax = aux[n];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm0 + i * 16 + fg * 4 + r;
        float s = rank_score(acc[i][j][r], ax, metric);
        if (n >= n_end) s = -INFINITY;
        Ss[row * SPITCH + col] = s;
      }
    }
}

// |q|^2 of query row `row`, in every lane of the wave: the sum the L2 searches subtract their key from
__device__ __forceinline__ float query_sqnorm(const float* __restrict__ q, int64_t ldq, int row, int E, int lane) {
  float qn = 0.f;
  for (int k = lane; k < E; k += 64) { const float v = q[(int64_t)row * ldq + k]; qn += v * v; }
  return wave_sum(qn);
}
}  // namespace
