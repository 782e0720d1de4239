// target_rank.h -- the last step of the target-rank epilogues of rank.hip and topk.hip: a row's rank is the sum of its per-split counts
// (integers: exact in any order), or -1 when its target id is outside [0, n_items).
#pragma once
#include "common.h"

namespace {
// part: [B][splits] items of the split that come before the row's target
__global__ __launch_bounds__(256) void target_rank_finish_kernel(const int32_t* __restrict__ part, int splits,
                                                                 const int64_t* __restrict__ targets, int B, int N,
                                                                 int32_t* __restrict__ out_rank) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  int r = -1;
  if ((uint64_t)targets[b] < (uint64_t)N) {
    r = 0;
    for (int s = 0; s < splits; ++s) r += part[(int64_t)b * splits + s];
  }
  out_rank[b] = r;
}
}  // namespace
