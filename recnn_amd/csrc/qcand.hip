// qcand.hip -- the critic's Q-value over per-row candidate lists, and the list sorted by it in the same launch (gfx950): the second
// stage of a retrieve-then-rerank recommender.  DESIGN.md section 23.
//
//   Q[b, j] = w3 . relu(W2 . relu(S1[b] + E1[ids[b, j]]) + b2) + b3        S1, E1, W2, b2, w3, b3 exactly as qrank.hip takes them
//
// A slot whose id is outside [0, N) is empty: it reads nothing and its Q is -inf.  A workgroup of four waves owns MT state rows and
// up to 64 candidates of each; a wave owns one state row and MT blocks of 16 of its candidates (MT = 4: one wave per row).  W2 streams
// through LDS in slabs of 16 k values, register-staged, shared by the workgroup's pair rows, as in qrank_pair_kernel.  The E1 operand
// is per (row, slot), so it is not an LDS tile: lane (fr, fg) loads its 16 bytes of E1[ids[b, 16 mt + fr], k0 + 4 fg ..] from global
// memory, the next slab's before this slab's MFMAs.
//
// Bits: the contraction of a pair is qrank_pair_kernel's -- slabs of 16 k ascending, within a slab the four v_mfma_f32_16x16x4_f32
// steps e = 0..3, then per lane the ascending sum over the column tiles, the xor butterfly 8, 4, 2, 1, + b3 -- so Q[b, j] has the bits
// of recnn_qrank_scores' Q[b, ids[b, j]], whatever B, K, the slot or MT.  No atomics.
//
// Sorted form (K <= 64): the Q of a row meet in LDS and one wave ranks them: each lane counts the slots that come before its own.
// Order: larger Q first, ties to the smaller id, equal ids to the smaller slot, -0 == +0, NaN after every number in id order, empty
// slots last (written as id -1 at -inf).
#include <climits>

#include "common.h"
#include "select_dev.h"   // slot_before: the order of a list's slots

namespace {
constexpr int QC_KS = 16;          // k values per W2 slab
constexpr int QC_WP = QC_KS + 4;   // floats per LDS row of a slab
constexpr int QC_HMAX = 256;
constexpr int QC_GRANULE = 64;
constexpr int QC_SLOTS = 64;       // candidates of one row per workgroup; the sorted form's largest K

struct CandArgs {
  const float* s1; int64_t ld_s1; int B;
  const float* e1; int64_t ld_e1; int N;
  const float* w2;     // [HP][HP] row j = output column j, contiguous over k
  const float* b2;     // [HP]
  const float* w3;     // [HP]
  float b3;
  const void* ids; int64_t ld_ids; int K; int ids64;
  float* out; int64_t ld_out;                       // plain form
  int k_out; float* sq; int64_t* sid;               // sorted form: [B][k_out]
  const int64_t* targets; int32_t* pos; const int32_t* fallback;
};

template <int HP, int MT, bool SORT>
__global__ __launch_bounds__(256) void qcand_kernel(const CandArgs a) {
  constexpr int NCT = HP / 16;          // column tiles
  constexpr int PS = HP + 4;            // floats per LDS row of the S1 tile
  constexpr int STAGE = HP * (QC_KS / 4) / 256;   // float4 per thread per slab
  constexpr int ROWS = MT;              // state rows per workgroup
  constexpr int WPR = 4 / MT;           // waves per state row
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Ss = (float*)smem;             // [ROWS][PS]
  float* Ws = Ss + ROWS * PS;           // [HP][QC_WP]
  float* Qs = Ws + HP * QC_WP;          // [ROWS][QC_SLOTS]
  int* Is = (int*)(Qs + ROWS * QC_SLOTS);   // [ROWS][QC_SLOTS]: the id of a slot, -1 for an empty one
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int row_l = wave / WPR, sub = wave % WPR;
  const int b0 = blockIdx.x * ROWS, b = b0 + row_l;
  const int c0 = sub * MT * 16;         // this wave's first slot within the workgroup's 64
  const int j0 = blockIdx.y * QC_SLOTS; // the workgroup's first slot of the list

  f32x4 stage[STAGE];
  const float* wsrc = a.w2 + (int64_t)(tid >> 2) * HP + (tid & 3) * 4;     // this thread's float4 of a slab; the next ones are 64 rows on
#pragma unroll
  for (int s = 0; s < STAGE; ++s) stage[s] = *(const f32x4*)(wsrc + (int64_t)s * 64 * HP);
  // this lane's candidates: slot c0 + 16 mt + fr of row b
  const float* esrc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int c = c0 + mt * 16 + fr;
    int64_t v = -1;
    if (b < a.B && j0 + c < a.K) {
      const int64_t o = (int64_t)b * a.ld_ids + j0 + c;
      v = a.ids64 ? ((const int64_t*)a.ids)[o] : (int64_t)((const int32_t*)a.ids)[o];
    }
    const bool ok = (uint64_t)v < (uint64_t)a.N;
    esrc[mt] = ok ? a.e1 + v * a.ld_e1 + fg * 4 : nullptr;
    if (fg == 0) Is[row_l * QC_SLOTS + c] = ok ? (int)v : -1;
  }
  f32x4 ef[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) ef[mt] = esrc[mt] ? *(const f32x4*)esrc[mt] : f32x4{0.f, 0.f, 0.f, 0.f};
  // S1 tile -> LDS (rows past B are zero; their results are not stored)
  for (int c = tid; c < ROWS * (HP / 4); c += 256) {
    const int r = c / (HP / 4), k4 = c % (HP / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b0 + r < a.B) v = *(const float4*)(a.s1 + (int64_t)(b0 + r) * a.ld_s1 + k4 * 4);
    *(float4*)&Ss[r * PS + k4 * 4] = v;
  }

  f32x4 acc[MT][NCT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[mt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int k0 = 0; k0 < HP; k0 += QC_KS) {
    __syncthreads();                      // the previous slab's readers are done (first pass: nothing to wait for)
#pragma unroll
    for (int s = 0; s < STAGE; ++s) {
      const int c = tid + s * 256;
      *(f32x4*)&Ws[(c >> 2) * QC_WP + (c & 3) * 4] = stage[s];
    }
    __syncthreads();                      // (first pass: the S1 tile and the slot ids are complete too)
    if (k0 + QC_KS < HP) {
#pragma unroll
      for (int s = 0; s < STAGE; ++s) stage[s] = *(const f32x4*)(wsrc + (int64_t)s * 64 * HP + k0 + QC_KS);
    }
    // A fragments: lane (fr, fg) holds pair row fr of row tile mt (= slot c0 + 16 mt + fr) at k = k0 + fg * 4 + e
    const f32x4 sf = *(const f32x4*)&Ss[row_l * PS + k0 + fg * 4];
    float av[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int e = 0; e < 4; ++e) av[mt][e] = fmaxf(sf[e] + ef[mt][e], 0.f);
    if (k0 + QC_KS < HP) {                // the next slab's E1 fragments are in flight during this slab's MFMAs
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        if (esrc[mt]) ef[mt] = *(const f32x4*)(esrc[mt] + k0 + QC_KS);
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const f32x4 wb = *(const f32x4*)&Ws[(ct * 16 + fr) * QC_WP + fg * 4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[mt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][e], wb[e], acc[mt][ct], 0, 0, 0);
    }
  }
  // ---- epilogue: acc[mt][ct][r] = Z[slot c0 + 16 mt + fg*4 + r of row b][column ct*16+fr]
  float b2v[NCT], w3v[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) { b2v[ct] = a.b2[ct * 16 + fr]; w3v[ct] = a.w3[ct * 16 + fr]; }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = 0.f;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) v += fmaxf(acc[mt][ct][r] + b2v[ct], 0.f) * w3v[ct];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);      // over the 16 lanes of the row: one fixed tree
      const int c = c0 + mt * 16 + fg * 4 + r;
      if (fr == 0) {
        const float q = Is[row_l * QC_SLOTS + c] >= 0 ? v + a.b3 : -INFINITY;
        if (SORT) Qs[row_l * QC_SLOTS + c] = q;
        else if (b < a.B && j0 + c < a.K) a.out[(int64_t)b * a.ld_out + j0 + c] = q;
      }
      __builtin_amdgcn_sched_barrier(0);    // one pair row's accumulators at a time
    }
  }
  if (!SORT) return;
  // ---- the row sorted: lane = slot; its place is the number of slots that come before it
  __syncthreads();
  if (sub != 0 || b >= a.B) return;
  const float* qs = Qs + row_l * QC_SLOTS;
  const int* is = Is + row_l * QC_SLOTS;
  const float q = qs[lane];
  const int id = is[lane];
  int place = 0;
  for (int j = 0; j < QC_SLOTS; ++j) place += slot_before(qs[j], is[j], j, q, id, lane) ? 1 : 0;
  if (place < a.k_out) {
    a.sq[(int64_t)b * a.k_out + place] = id < 0 ? -INFINITY : q;
    a.sid[(int64_t)b * a.k_out + place] = id;
  }
  if (a.pos) {
    const int64_t g = a.targets[b];
    const bool valid = (uint64_t)g < (uint64_t)a.N;
    int first = valid && id == (int)g ? place : INT_MAX;     // non-empty slots come before every empty one: place = non-empty before
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
    const int filled = __popcll(__ballot(id >= 0));
    if (lane == 0) {
      int p = first == INT_MAX ? -1 : first;
      if (p < 0 && valid && a.fallback) {                     // not a candidate: its rank in the first stage's order, after the candidates
        const int f = a.fallback[b];
        p = f < 0 ? -1 : max(f, filled);
      }
      a.pos[b] = p;
    }
  }
}

// row tiles per wave: four (one wave owns a state row's 64 candidates) while the accumulators leave room for the operands; at
// HP = 256 two, so that a row's candidates are shared by two waves and nothing spills.
template <int HP> constexpr int qc_mt() { return HP <= 192 ? 4 : 2; }

template <int HP, bool SORT> int launch_cand(const CandArgs& a, hipStream_t st) {
  constexpr int MT = qc_mt<HP>();
  const size_t lds = (size_t)(MT * (HP + 4) + HP * QC_WP + 2 * MT * QC_SLOTS) * 4;
  const dim3 grid((a.B + MT - 1) / MT, SORT ? 1 : (a.K + QC_SLOTS - 1) / QC_SLOTS);
  hipLaunchKernelGGL((qcand_kernel<HP, MT, SORT>), grid, dim3(256), lds, st, a);
  return recnn_check_hip(hipGetLastError(), "qcand_kernel");
}

template <bool SORT> int dispatch_cand(const CandArgs& a, int hidden_padded, hipStream_t st) {
  switch (hidden_padded) {
    case 64: return launch_cand<64, SORT>(a, st);
    case 128: return launch_cand<128, SORT>(a, st);
    case 192: return launch_cand<192, SORT>(a, st);
    default: return launch_cand<256, SORT>(a, st);
  }
}

int cand_check(const char* fn, const float* s1, int64_t ld_s1, int n_states, const float* e1, int64_t ld_e1, int n_items,
               int hidden_padded, const float* w2, const float* b2, const float* w3, const void* ids, int64_t ld_ids, int n_cand,
               int ids_are_int64) {
  RECNN_REQUIRE(e1 && w2 && b2 && w3 && ((s1 && ids) || n_states == 0), "%s: null pointer", fn);
  RECNN_REQUIRE(n_states >= 0 && n_items > 0 && n_cand > 0, "%s: need n_states >= 0, n_items > 0 and n_candidates > 0", fn);
  RECNN_REQUIRE(hidden_padded > 0 && hidden_padded <= QC_HMAX && hidden_padded % QC_GRANULE == 0,
                "%s: hidden_padded must be a multiple of %d up to %d (got %d)", fn, QC_GRANULE, QC_HMAX, hidden_padded);
  RECNN_REQUIRE(aligned16(s1, e1, w2) && ld_s1 % 4 == 0 && ld_e1 % 4 == 0 && ld_s1 >= hidden_padded && ld_e1 >= hidden_padded,
                "%s: 16-byte alignment (rows and strides), strides at least hidden_padded", fn);
  RECNN_REQUIRE(ids_are_int64 == 0 || ids_are_int64 == 1, "%s: ids_are_int64 must be 0 (int32) or 1 (int64)", fn);
  RECNN_REQUIRE(((uintptr_t)ids & (ids_are_int64 ? 7 : 3)) == 0 && (ld_ids >= n_cand || n_states <= 1),
                "%s: ids must be aligned to their element with a row stride of at least n_candidates", fn);
  return 0;
}
}  // namespace

extern "C" int recnn_qcand_scores(const float* s1, int64_t ld_s1, int n_states, const float* e1, int64_t ld_e1, int n_items,
                                  int hidden_padded, const float* w2, const float* b2, const float* w3, float b3, const void* ids,
                                  int64_t ld_ids, int n_candidates, int ids_are_int64, float* out, int64_t ld_out, void* stream) {
  if (int rc = cand_check("qcand_scores", s1, ld_s1, n_states, e1, ld_e1, n_items, hidden_padded, w2, b2, w3, ids, ld_ids, n_candidates,
                          ids_are_int64))
    return rc;
  RECNN_REQUIRE(out || n_states == 0, "qcand_scores: null pointer");
  RECNN_REQUIRE(ld_out >= n_candidates || n_states <= 1, "qcand_scores: ld_out is smaller than n_candidates");
  RECNN_REQUIRE((n_candidates + QC_SLOTS - 1) / QC_SLOTS <= 65535, "qcand_scores: at most %d candidates per row", 65535 * QC_SLOTS);
  if (n_states == 0) return 0;
  CandArgs a = {};
  a.s1 = s1; a.ld_s1 = ld_s1; a.B = n_states; a.e1 = e1; a.ld_e1 = ld_e1; a.N = n_items;
  a.w2 = w2; a.b2 = b2; a.w3 = w3; a.b3 = b3; a.ids = ids; a.ld_ids = ld_ids; a.K = n_candidates; a.ids64 = ids_are_int64;
  a.out = out; a.ld_out = ld_out;
  return dispatch_cand<false>(a, hidden_padded, (hipStream_t)stream);
}

extern "C" int recnn_qcand_rerank(const float* s1, int64_t ld_s1, int n_states, const float* e1, int64_t ld_e1, int n_items,
                                  int hidden_padded, const float* w2, const float* b2, const float* w3, float b3, const void* ids,
                                  int64_t ld_ids, int n_candidates, int ids_are_int64, int k, float* out_q, int64_t* out_ids,
                                  const int64_t* targets, int32_t* out_pos, const int32_t* fallback_rank, void* stream) {
  if (int rc = cand_check("qcand_rerank", s1, ld_s1, n_states, e1, ld_e1, n_items, hidden_padded, w2, b2, w3, ids, ld_ids, n_candidates,
                          ids_are_int64))
    return rc;
  RECNN_REQUIRE(n_candidates <= QC_SLOTS, "qcand_rerank: the sorted form takes at most %d candidates per row (got %d)", QC_SLOTS,
                n_candidates);
  RECNN_REQUIRE(k >= 1 && k <= n_candidates, "qcand_rerank: need 1 <= k <= n_candidates (got k = %d, n_candidates = %d)", k, n_candidates);
  RECNN_REQUIRE((out_q && out_ids) || n_states == 0, "qcand_rerank: null pointer");
  RECNN_REQUIRE((targets != nullptr) == (out_pos != nullptr) || n_states == 0, "qcand_rerank: targets and out_pos go together");
  RECNN_REQUIRE(!fallback_rank || out_pos, "qcand_rerank: fallback_rank needs targets and out_pos");
  if (n_states == 0) return 0;
  CandArgs a = {};
  a.s1 = s1; a.ld_s1 = ld_s1; a.B = n_states; a.e1 = e1; a.ld_e1 = ld_e1; a.N = n_items;
  a.w2 = w2; a.b2 = b2; a.w3 = w3; a.b3 = b3; a.ids = ids; a.ld_ids = ld_ids; a.K = n_candidates; a.ids64 = ids_are_int64;
  a.k_out = k; a.sq = out_q; a.sid = out_ids; a.targets = targets; a.pos = out_pos; a.fallback = fallback_rank;
  return dispatch_cand<true>(a, hidden_padded, (hipStream_t)stream);
}
