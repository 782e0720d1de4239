// select_dev.h -- what the top-K selections share (topk.hip, ivf.hip, scoresel.hip; rank.hip takes the limits and the empty slot; qcand.hip
// and slate.hip take the order of a candidate list's slots): the order of two candidates, the insert of a chunk's survivors into a row's sorted list, and the merge of a row's partial lists.
// Comparisons, shuffles and moves only, no floating-point arithmetic: the header means the same under any contraction setting.
#pragma once
#include "common.h"

namespace {
constexpr int KMAX = 64;             // largest supported K
constexpr int PITCH = 132;           // floats per LDS row of a [rows][128] tile (+4 pad: conflict-light b128 reads)
constexpr int NONE_ID = 0x7FFFFFFF;  // id of an empty list slot: after every item's id

// (key, id) pairs, larger key first, ties to the smaller id.  better() is for numbers only: a NaN key never wins, nor is it ever beaten
__device__ inline bool better(float s, int id, float s2, int id2) { return s > s2 || (s == s2 && id < id2); }

// the total order: better() wherever both keys are numbers; a NaN key comes after every number, and NaN keys order by id
__device__ inline bool comes_before(float s, int id, float s2, int id2) {
  if (s != s) return s2 != s2 && id < id2;
  return s2 != s2 || better(s, id, s2, id2);
}
using Order = bool (*)(float, int, float, int);

// The order of the slots of a per-row candidate list (qcand.hip's sorted form, slate.hip's greedy pick): slot a (score qa, id ia >= 0
// or < 0 = empty, index sa) comes before slot b.  Larger score first, -0 == +0, ties to the smaller id, equal ids to the smaller slot,
// NaN scores after every number in (id, slot) order, empty slots last in slot order.
__device__ inline bool slot_before(float qa, int ia, int sa, float qb, int ib, int sb) {
  const int ca = ia < 0 ? 2 : (qa != qa ? 1 : 0), cb = ib < 0 ? 2 : (qb != qb ? 1 : 0);
  if (ca != cb) return ca < cb;
  if (ca == 2) return sa < sb;
  if (ca == 0 && qa != qb) return qa > qb;
  return ia < ib || (ia == ib && sa < sb);
}

// The same order as one unsigned key, for a wave-wide maximum: a comes before b  <=>  slot_key(a) > slot_key(b), or the keys are equal
// (one score or both NaN, one id) and sa < sb.  An empty slot's key is 0, below every other; empty slots are not ordered among themselves.
__device__ inline uint64_t slot_key(float q, int id) {
  if (id < 0) return 0;
  uint32_t hi = 1u;                                                     // NaN: after every number (-inf maps to 0x007FFFFF)
  if (q == q) {
    const uint32_t u = q == 0.f ? 0u : __builtin_bit_cast(uint32_t, q);  // -0 == +0
    hi = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                    // ascending with q
  }
  return ((uint64_t)hi << 32) | (uint32_t)(0x7FFFFFFF - id);
}

// A wave inserts a chunk's survivors into the sorted list (ls, li) of K <= 64 entries, entry e handled by lane e.  m: the ballot of
// the lanes whose candidate beats the list's K-th; lane src offers (its s, id_of(src)).  Survivors enter in lane order, each checked
// again against the K-th of the moment; an empty ballot costs the loop test alone.
template <Order BEFORE, class IdOf>
__device__ __forceinline__ void insert_survivors(unsigned long long m, float s, IdOf id_of, float* ls, int* li, int K, int lane) {
  while (m) {                                         // rare after the first chunks
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    const float cs = __shfl(s, src, 64);
    const int cid = id_of(src);
    if (!BEFORE(cs, cid, ls[K - 1], li[K - 1])) continue;
    // lanes shift the tail in parallel
    const float mine = lane < K ? ls[lane] : 0.f;
    const int mine_id = lane < K ? li[lane] : 0;
    const bool before = lane < K && BEFORE(mine, mine_id, cs, cid);        // entries that stay in front
    const int pos = __popcll(__ballot(before));                            // insertion position
    const float up = __shfl_up(mine, 1, 64);                               // (all lanes: no divergent shuffles)
    const int up_id = __shfl_up(mine_id, 1, 64);
    if (lane < K) {
      if (lane == pos) { ls[lane] = cs; li[lane] = cid; }
      else if (lane > pos) { ls[lane] = up; li[lane] = up_id; }
    }
  }
}

// A wave takes the K best of one row's `total` <= 512 candidates (ps, pi): S sorted partial lists whose ids are unique, up to 8
// candidates per lane.  An empty slot is (none, NONE_ID), which must come after every item under BEFORE.  out(k, key, id) is called by
// lane 0, best first; a row with fewer than K items ends in (none, NONE_ID).
template <Order BEFORE, class Out>
__device__ __forceinline__ void merge_candidates(const float* __restrict__ ps, const int32_t* __restrict__ pi, int total, int K, float none,
                                                 int lane, Out out) {
  float cs[8]; int ci[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = lane + j * 64;
    cs[j] = c < total ? ps[c] : none;
    ci[j] = c < total ? pi[c] : NONE_ID;
  }
  for (int k = 0; k < K; ++k) {
    float bs = none; int bi = NONE_ID;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (BEFORE(cs[j], ci[j], bs, bi)) { bs = cs[j]; bi = ci[j]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float os = __shfl_xor(bs, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (BEFORE(os, oi, bs, bi)) { bs = os; bi = oi; }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (ci[j] == bi) { cs[j] = none; ci[j] = NONE_ID; }
    if (lane == 0) out(k, bs, bi);
  }
}
}  // namespace
