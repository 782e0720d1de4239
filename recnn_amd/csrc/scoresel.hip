// scoresel.hip -- selection from a score matrix that already exists: per row of float32 scores [B][N] (row stride ld), the k best
// items, or the number of items that come before one target item (gfx950).  DESIGN.md section 22.
//
// The other top-K and counting epilogues of the library are fused into their scoring kernels (topk.hip, rank.hip); these two take the
// scores from memory: the Q block of CriticIndex (qrank.hip), or any [B, N] matrix such as DiscreteActor's probabilities.
//
// Order: larger score first, ties to the smaller id (-0 == +0), NaN after every number in id order -- `comes_before` of select_dev.h,
// whose list insert and merge the top-K kernels use under that order.  An empty list slot is (NaN, NONE_ID): every item comes before
// it.  An item whose bit is set in its row's mask (seen.h; the mask may be NULL) does not exist for that row.
//
// One wave owns one (row, split of the items): it streams its split in blocks of 64 consecutive items that start at a multiple of 64
// (one item per lane, coalesced; one mask word per block).  Ids are int32, nothing is sized by N: N is limited by int32 alone (by
// seen.h's limit when a mask is given).  Per-(row, split) results go through a workspace to a finishing kernel: no atomics.
#include <algorithm>

#include "common.h"
#include "seen.h"
#include "select_dev.h"
#include "target_rank.h"

namespace {
constexpr int SS_MAX_SPLITS = 8;    // the merge holds 8 x 64 candidates, 8 per lane
constexpr int SS_TARGET_WAVES = 2048;
constexpr int SS_MIN_PER = 256;     // items per split, at least

struct SelPlan { int splits, per; };
SelPlan make_sel_plan(int B, int N) {
  int s = std::min(SS_MAX_SPLITS, std::max(1, SS_TARGET_WAVES / std::max(B, 1)));
  s = std::max(1, std::min(s, N / SS_MIN_PER));
  SelPlan pl;
  pl.per = (int)((((int64_t)N + s - 1) / s + 63) / 64 * 64);     // whole 64-item blocks: a block's exclusion bits are one word
  pl.splits = (int)(((int64_t)N + pl.per - 1) / pl.per);         // no empty split
  return pl;
}

// part_s / part_i: [B][splits][K], each list sorted, empty slots (NaN, NONE_ID)
__global__ __launch_bounds__(256) void scores_topk_kernel(const float* __restrict__ scores, int64_t ld, int B, int N, int K, int splits, int per,
                                                          const uint64_t* __restrict__ mask, int64_t W, float* __restrict__ part_s,
                                                          int32_t* __restrict__ part_i) {
  __shared__ float Ls[4][KMAX];
  __shared__ int Li[4][KMAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= B) return;                                  // whole waves leave; no workgroup barrier below
  float* ls = Ls[wave];
  int* li = Li[wave];
  ls[lane] = __builtin_nanf("");
  li[lane] = NONE_ID;
  const int n_begin = blockIdx.y * per, n_end = (int)min((int64_t)N, (int64_t)n_begin + per);
  const float* srow = scores + (int64_t)row * ld;
  float s_next = n_begin + lane < n_end ? srow[n_begin + lane] : 0.f;
  for (int n0 = n_begin; n0 < n_end; n0 += 64) {
    const float s = s_next;
    const int id = n0 + lane;
    if (n0 + 64 < n_end) s_next = n0 + 64 + lane < n_end ? srow[n0 + 64 + lane] : 0.f;
    unsigned long long m = __ballot(id < n_end && comes_before(s, id, ls[K - 1], li[K - 1]));
    if (mask) m &= ~seen_word(mask, W, row, n0);
    insert_survivors<comes_before>(m, s, [&](int src) { return n0 + src; }, ls, li, K, lane);
  }
  if (lane < K) {
    const int64_t o = ((int64_t)row * splits + blockIdx.y) * K + lane;
    part_s[o] = ls[lane];
    part_i[o] = li[lane];
  }
}

// merges a row's sorted partial lists; one wave per row.  An empty slot is reported as id -1 with score -inf.
__global__ __launch_bounds__(256) void scores_topk_merge_kernel(const float* __restrict__ ps, const int32_t* __restrict__ pi, int B, int splits,
                                                                int K, float* __restrict__ out_s, int64_t* __restrict__ out_i) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= B) return;
  const int64_t total = splits * K;
  merge_candidates<comes_before>(ps + row * total, pi + row * total, (int)total, K, __builtin_nanf(""), lane, [&](int k, float bs, int bi) {
    out_s[(int64_t)row * K + k] = bi == NONE_ID ? -INFINITY : bs;
    out_i[(int64_t)row * K + k] = bi == NONE_ID ? -1 : bi;
  });
}

// part[row][split] = items of the split, other than the target and not excluded, that come before the row's target
__global__ __launch_bounds__(256) void scores_rank_kernel(const float* __restrict__ scores, int64_t ld, int B, int N, int splits, int per,
                                                          const int64_t* __restrict__ targets, const uint64_t* __restrict__ mask, int64_t W,
                                                          int32_t* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= B) return;
  const int64_t g = targets[row];
  const bool valid = (uint64_t)g < (uint64_t)N;
  const int tg = valid ? (int)g : -1;
  const float* srow = scores + (int64_t)row * ld;
  const float ts = valid ? srow[tg] : 0.f;               // a target outside the table reads nothing; the finish reports -1
  const int n_begin = blockIdx.y * per, n_end = (int)min((int64_t)N, (int64_t)n_begin + per);
  int cnt = 0;
  for (int n0 = n_begin; n0 < n_end; n0 += 256) {         // four blocks' loads in flight together
    float s[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t id = (int64_t)n0 + c * 64 + lane;
      s[c] = id < n_end ? srow[id] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t nb = (int64_t)n0 + c * 64;
      if (nb >= n_end) break;
      const int64_t id = nb + lane;
      unsigned long long m = __ballot(id < n_end && id != tg && comes_before(s[c], (int)id, ts, tg));
      if (mask) m &= ~seen_word(mask, W, row, (int)nb);
      cnt += __popcll(m);
    }
  }
  if (lane == 0) part[(int64_t)row * splits + blockIdx.y] = cnt;
}

int scores_check(const char* fn, const float* scores, int64_t ld, int B, int N, const uint64_t* mask, int64_t W) {
  RECNN_REQUIRE(B >= 0 && N > 0, "%s: need n_rows >= 0 and n_items > 0", fn);
  RECNN_REQUIRE(scores || B == 0, "%s: null pointer", fn);
  RECNN_REQUIRE(((uintptr_t)scores & 3) == 0 && ld >= N, "%s: scores must be 4-byte aligned with a row stride of at least n_items", fn);
  RECNN_REQUIRE((B + 3) / 4 <= 0x7FFFFFFF / 4, "%s: too many rows", fn);
  if (mask || W) return seen_check(fn, mask, W, B, N);
  return 0;
}
}  // namespace

extern "C" int recnn_scores_topk_workspace_bytes(int n_rows, int k, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes && n_rows >= 0 && k > 0 && k <= KMAX, "scores_topk_workspace_bytes: bad arguments (0 < k <= 64)");
  *h_bytes = (int64_t)n_rows * SS_MAX_SPLITS * k * 8;     // per split: k scores and k ids
  return 0;
}

extern "C" int recnn_scores_topk(const float* scores, int64_t ld, int n_rows, int n_items, int k, float* out_scores, int64_t* out_ids,
                                 void* workspace, void* stream, const uint64_t* mask, int64_t words_per_row) {
  if (int rc = scores_check("scores_topk", scores, ld, n_rows, n_items, mask, words_per_row)) return rc;
  RECNN_REQUIRE(k > 0 && k <= KMAX, "scores_topk: need 0 < k <= 64 (got %d)", k);
  RECNN_REQUIRE((out_scores && out_ids && workspace) || n_rows == 0, "scores_topk: null pointer");
  if (n_rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const SelPlan pl = make_sel_plan(n_rows, n_items);
  float* part_s = (float*)workspace;
  int32_t* part_i = (int32_t*)((char*)workspace + (int64_t)n_rows * SS_MAX_SPLITS * k * 4);
  const int wgs = (n_rows + 3) / 4;
  hipLaunchKernelGGL(scores_topk_kernel, dim3(wgs, pl.splits), dim3(256), 0, st, scores, ld, n_rows, n_items, k, pl.splits, pl.per, mask,
                     words_per_row, part_s, part_i);
  hipLaunchKernelGGL(scores_topk_merge_kernel, dim3(wgs), dim3(256), 0, st, part_s, part_i, n_rows, pl.splits, k, out_scores, out_ids);
  return recnn_check_hip(hipGetLastError(), "scores_topk");
}

extern "C" int recnn_scores_rank_workspace_bytes(int n_rows, int n_items, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes && n_rows >= 0 && n_items > 0, "scores_rank_workspace_bytes: bad arguments");
  *h_bytes = n_rows > 0 ? (int64_t)n_rows * make_sel_plan(n_rows, n_items).splits * 4 : 0;
  return 0;
}

extern "C" int recnn_scores_rank(const float* scores, int64_t ld, int n_rows, int n_items, const int64_t* targets, int32_t* out_rank,
                                 void* workspace, void* stream, const uint64_t* mask, int64_t words_per_row) {
  if (int rc = scores_check("scores_rank", scores, ld, n_rows, n_items, mask, words_per_row)) return rc;
  RECNN_REQUIRE((targets && out_rank && workspace) || n_rows == 0, "scores_rank: null pointer");
  if (n_rows == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const SelPlan pl = make_sel_plan(n_rows, n_items);
  int32_t* part = (int32_t*)workspace;
  hipLaunchKernelGGL(scores_rank_kernel, dim3((n_rows + 3) / 4, pl.splits), dim3(256), 0, st, scores, ld, n_rows, n_items, pl.splits, pl.per,
                     targets, mask, words_per_row, part);
  hipLaunchKernelGGL(target_rank_finish_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, st, part, pl.splits, targets, n_rows, n_items,
                     out_rank);
  return recnn_check_hip(hipGetLastError(), "scores_rank");
}
