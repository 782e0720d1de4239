// topk_dev.h -- what the exact-fp32 searches share (topk.hip: the flat search and the target rank; ivf.hip: the inverted-list scan):
// the tile shape, the order of two candidates, the 64 x 64 scoring tile and the query's squared norm.  A (query, item) pair scored
// through these has the same bits in every kernel: an element's k order does not depend on its place in a tile.
#pragma once
#include "common.h"

namespace {
constexpr int QT = 64;     // query rows per workgroup
constexpr int IT = 64;     // items per chunk
constexpr int KMAX = 64;   // largest supported K
constexpr int PITCH = 132; // floats per LDS row of a [rows][128] tile (+4 pad: conflict-light b128 reads)
enum { M_IP = 0, M_L2 = 1, M_COS = 2 };

__device__ inline bool better(float s, int id, float s2, int id2) { return s > s2 || (s == s2 && id < id2); }

// 64 x 64 scores of the query tile against the 64 rows in Ts: the k order of topk_scores_kernel, which is the same for every element
// of the tile
__device__ __forceinline__ void score_tile(const float* Qs, const float* Ts, int wm0, int wn0, int fr, int fg, f32x4 (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int ks = 0; ks < 128 / 16; ++ks) {
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

// |q|^2 of query row `row`, in every lane of the wave: the sum the L2 searches subtract their key from
__device__ __forceinline__ float query_sqnorm(const float* __restrict__ q, int64_t ldq, int row, int E, int lane) {
  float qn = 0.f;
  for (int k = lane; k < E; k += 64) { const float v = q[(int64_t)row * ldq + k]; qn += v * v; }
  return wave_sum(qn);
}
}  // namespace
