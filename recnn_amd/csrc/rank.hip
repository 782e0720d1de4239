// rank.hip -- exact scipy-metric distances between action vectors and the item table (gfx950): the full [B, N] matrix, or
// fused with a per-query top-K selection.
//
// The reference ranks the catalogue for a generated action with a per-item scipy loop (examples/streamlit_demo.py:207-231,
// `rank`; examples/[Results]/1. Ranking.ipynb): `metric(emb[i], action)` for every item, sorted ascending, first k.  The
// metrics are those of scipy.spatial.distance.cdist (scipy 1.15):
//
//   sqeuclidean  sum (q-t)^2            euclidean  sqrt(sqeuclidean)     cityblock  sum |q-t|      chebyshev  max |q-t|
//   minkowski p  (sum |q-t|^p)^(1/p)    canberra   sum |q-t| / (|q|+|t|), a 0/0 term counts 0
//   braycurtis   sum |q-t| / sum |q+t|  cosine     1 - clip(q.t / (|q| |t|), -1, 1)     correlation  cosine of centred rows
//
// None of them is an inner product of the raw rows, so the MFMA scoring GEMM of topk.hip does not apply: the inner loop is f32
// VALU, an elementwise combine plus a running reduction per (query, item) pair.  cosine / correlation run the same loop as a
// dot product over rows normalised (and centred) once by a prep kernel: the table's in an aux array owned by the caller, the
// queries' in the workspace.  A zero row (cosine) or a constant row (correlation) becomes a NaN row, which makes every distance
// against it NaN, as scipy reports.
//
// Grid = (query tiles) x (item splits).  A workgroup takes QT = 4*TQ query rows and streams its split of the table through LDS
// in chunks of IT = 64*TI items (the next chunk is register-staged while the current one is scored).  Wave w owns query rows
// TQ*w .. TQ*w+TQ-1 (read from memory at wave-uniform addresses) and lane l owns items l, l+64, ... of the chunk, so each lane keeps a TQ x TI
// register tile of pairs.  Every pair's reduction runs over k = 0..127 in that order, with explicitly rounded operations and
// contraction off, and ends in the same finishing step in both epilogues: a pair's value does not depend on the tile, the split,
// the batch or the epilogue, and `recnn_dist_topk` reports bit for bit what `recnn_dist_matrix` stores.
//
// Epilogues: MATRIX stores the tile; TOPK lets each wave keep the sorted K-best list of each of its rows in registers (entry e in
// lane e; one ballot per row and 64 items against the row's current K-th, survivors inserted) and writes it as one partial list per (row, split); a
// merge kernel then takes the K best of a row's sorted partial lists.  Order: distance ascending, NaN after every number, ties
// to the smaller item id.  A third kernel, dist_rank_kernel, streams the table the same way and only counts, per row, the items that
// come before one target item in that order.  Both kernels walk the table through the same device functions
// (load_chunk, store_chunk, accumulate), and the host picks a kernel's <LOOP, TQ, TI> in one place (dispatch).
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "seen.h"
#include "select_dev.h"   // KMAX, PITCH, NONE_ID: no floating-point arithmetic in it, so nothing there depends on the pragma below
#include "target_rank.h"

#pragma clang fp contract(off)

namespace {
constexpr int E = 128;          // embedding width (the reference's)
constexpr int MERGE_CAND = 4096;  // largest splits * K the merge keeps in LDS
constexpr int MAX_SPLITS = 256;   // the merge's wave holds 4 list heads per lane
constexpr int TARGET_WG = 1024;   // workgroups to aim for: 4 per CU

enum { SQEUCLIDEAN = RECNN_DIST_SQEUCLIDEAN, EUCLIDEAN = RECNN_DIST_EUCLIDEAN, CITYBLOCK = RECNN_DIST_CITYBLOCK,
       CHEBYSHEV = RECNN_DIST_CHEBYSHEV, MINKOWSKI = RECNN_DIST_MINKOWSKI, CANBERRA = RECNN_DIST_CANBERRA,
       BRAYCURTIS = RECNN_DIST_BRAYCURTIS, COSINE = RECNN_DIST_COSINE, CORRELATION = RECNN_DIST_CORRELATION };
// inner-loop kinds: the per-element combine of a (query, item) pair
enum Loop { L_SQ, L_ABS, L_MAX, L_POW, L_CANB, L_BRAY, L_DOT };

struct DistArgs {
  const float* q; int64_t ldq; int B;   // query rows (cosine / correlation: the prepared rows)
  const float* t; int N;                // item rows [N][128] (cosine / correlation: the aux rows)
  int metric; float p, invp;            // minkowski exponent and 1/p
  int per;                              // items per split (a multiple of IT)
  float* out; int64_t ldo;              // MATRIX epilogue
  int K, splits; float* part_d; int32_t* part_i;  // TOPK epilogue: [B][splits][K]
};
// the excluding kernels take the mask of seen.h behind the same arguments; the plain ones keep their argument block
struct DistArgsX : DistArgs { const uint64_t* mask; int64_t W; };
template <bool EXCL> using DistArgsOf = std::conditional_t<EXCL, DistArgsX, DistArgs>;

// the same order as one 64-bit key: distance bits (distances are >= +0: -0 counts as +0, every NaN as one value above +inf),
// then the id
__device__ inline uint64_t rank_key(float d, int id) {
  const uint32_t b = __builtin_isnan(d) ? 0x7FC00000u : (__builtin_bit_cast(uint32_t, d) & 0x7FFFFFFFu);
  return ((uint64_t)b << 32) | (uint32_t)id;
}

// lane l <- lane l-1 (DPP wave_shr:1; lane 0 gets 0)
__device__ inline int shr1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xF, 0xF, false); }
__device__ inline float shr1(float v) { return __builtin_bit_cast(float, shr1(__builtin_bit_cast(int, v))); }

__device__ inline float readlane_f(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

template <int LOOP> __device__ __forceinline__ void combine(float& a0, float& a1, float q, float t, float p) {
  if constexpr (LOOP == L_SQ) {
    const float d = __fsub_rn(q, t);
    a0 = __fmaf_rn(d, d, a0);
  } else if constexpr (LOOP == L_ABS) {
    a0 = __fadd_rn(a0, fabsf(__fsub_rn(q, t)));
  } else if constexpr (LOOP == L_MAX) {
    a0 = fmaxf(a0, fabsf(__fsub_rn(q, t)));
  } else if constexpr (LOOP == L_POW) {       // |d|^p = exp2(p log2|d|); |d| = 0 -> log2 = -inf -> 0
    a0 = __fadd_rn(a0, __builtin_amdgcn_exp2f(__fmul_rn(p, __builtin_amdgcn_logf(fabsf(__fsub_rn(q, t))))));
  } else if constexpr (LOOP == L_CANB) {      // |q-t| <= |q|+|t|, so the only 0 denominator has a 0 numerator
    const float den = __fadd_rn(fabsf(q), fabsf(t));
    const float term = __fmul_rn(fabsf(__fsub_rn(q, t)), __builtin_amdgcn_rcpf(den));
    a0 = __fadd_rn(a0, den > 0.f ? term : 0.f);
  } else if constexpr (LOOP == L_BRAY) {
    a0 = __fadd_rn(a0, fabsf(__fsub_rn(q, t)));
    a1 = __fadd_rn(a1, fabsf(__fadd_rn(q, t)));
  } else {
    a0 = __fmaf_rn(q, t, a0);
  }
}

// the pair's distance from its accumulators: one code path for both epilogues
template <int LOOP> __device__ __forceinline__ float finish(float a0, float a1, int metric, float invp) {
  // square root and quotient by the hardware instructions (v_sqrt_f32, v_rcp_f32; 1 ulp): the same instruction in every
  // kernel, where the compiler's correctly rounded expansions may differ between two of them
  if constexpr (LOOP == L_SQ) return metric == EUCLIDEAN ? __builtin_amdgcn_sqrtf(a0) : a0;
  else if constexpr (LOOP == L_POW) return __builtin_amdgcn_exp2f(__fmul_rn(invp, __builtin_amdgcn_logf(a0)));
  else if constexpr (LOOP == L_BRAY) return __fmul_rn(a0, __builtin_amdgcn_rcpf(a1));   // 0/0 -> NaN, x/0 -> inf, as scipy
  else if constexpr (LOOP == L_DOT) {
    float c = a0;
    if (fabsf(c) > 1.f) c = copysignf(1.f, c);                                   // scipy's clip; NaN stays NaN
    return __fsub_rn(1.f, c);
  } else return a0;
}

template <int LOOP> __device__ __forceinline__ void combine4(float& a0, float& a1, const float4& q, const float4& t, float p) {
  combine<LOOP>(a0, a1, q.x, t.x, p);
  combine<LOOP>(a0, a1, q.y, t.y, p);
  combine<LOOP>(a0, a1, q.z, t.z, p);
  combine<LOOP>(a0, a1, q.w, t.w, p);
}

// ---- a workgroup's walk over its split of the table, shared by dist_kernel and dist_rank_kernel

// the wave's query rows, read with wave-uniform addresses (rows past B repeat row B-1; their results are not kept)
template <int TQ> __device__ __forceinline__ void query_rows(const DistArgs& a, int q0, int wave, const float* (&qrow)[TQ]) {
#pragma unroll
  for (int i = 0; i < TQ; ++i) qrow[i] = a.q + (int64_t)min(q0 + wave * TQ + i, a.B - 1) * a.ldq;
}

// items n0 .. n0 + 64 TI - 1 -> registers, TI * 8 float4 per thread (rows from n_end on are zero) ...
template <int TI> __device__ __forceinline__ void load_chunk(float4 (&stage)[TI * 8], const float* t, int n0, int n_end, int tid) {
#pragma unroll
  for (int s = 0; s < TI * 8; ++s) {
    const int c = tid + s * 256, r = c >> 5, k4 = c & 31;
    stage[s] = n0 + r < n_end ? *(const float4*)(t + (int64_t)(n0 + r) * E + k4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// ... and from there into the LDS tile Ts [64 TI][PITCH], once the previous chunk's readers are done
template <int TI> __device__ __forceinline__ void store_chunk(const float4 (&stage)[TI * 8], float* Ts, int tid) {
  __syncthreads();
#pragma unroll
  for (int s = 0; s < TI * 8; ++s) {
    const int c = tid + s * 256;
    *(float4*)&Ts[(c >> 5) * PITCH + (c & 31) * 4] = stage[s];
  }
  __syncthreads();
}

// the accumulators of the lane's TQ x TI pairs against the chunk in Ts: every pair runs over k = 0..127 in that order
template <int LOOP, int TQ, int TI>
__device__ __forceinline__ void accumulate(const float* Ts, const float* (&qrow)[TQ], int lane, float p, float (&a0)[TQ][TI],
                                           float (&a1)[TQ][TI]) {
#pragma unroll
  for (int i = 0; i < TQ; ++i)
#pragma unroll
    for (int j = 0; j < TI; ++j) { a0[i][j] = 0.f; a1[i][j] = 0.f; }
#pragma unroll 2
  for (int k = 0; k < E; k += 4) {
    float4 tv[TI];
#pragma unroll
    for (int j = 0; j < TI; ++j) tv[j] = *(const float4*)&Ts[(j * 64 + lane) * PITCH + k];
#pragma unroll
    for (int i = 0; i < TQ; ++i) {
      const float4 qv = *(const float4*)(qrow[i] + k);
#pragma unroll
      for (int j = 0; j < TI; ++j) combine4<LOOP>(a0[i][j], a1[i][j], qv, tv[j], p);
    }
  }
}

template <int LOOP, int TQ, int TI, bool TOPK, bool EXCL = false>
__global__ __launch_bounds__(256) void dist_kernel(const DistArgsOf<EXCL> a) {
  static_assert(TOPK || !EXCL, "a matrix has no notion of absence");
  constexpr int QT = 4 * TQ, IT = 64 * TI;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Ts = (float*)smem;                     // [IT][PITCH]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = blockIdx.x * QT;
  const int n_begin = blockIdx.y * a.per, n_end = min(a.N, n_begin + a.per);
  const int K = a.K;

  // TOPK: the sorted K-best list of each of the wave's rows, entry e in lane e; (NaN, INT_MAX) ranks after every item
  float ld[TQ];
  int li[TQ];
#pragma unroll
  for (int i = 0; i < TQ; ++i) { ld[i] = __builtin_nanf(""); li[i] = NONE_ID; }
  const float* qrow[TQ];
  query_rows<TQ>(a, q0, wave, qrow);
  float4 stage[TI * 8];
  if (n_begin < n_end) load_chunk<TI>(stage, a.t, n_begin, n_end, tid);
  const bool wave_live = q0 + wave * TQ < a.B;    // wave-uniform: rows of this wave exist

  for (int n0 = n_begin; n0 < n_end; n0 += IT) {
    store_chunk<TI>(stage, Ts, tid);
    if (n0 + IT < n_end) load_chunk<TI>(stage, a.t, n0 + IT, n_end, tid);     // in flight while this chunk is scored
    if (!wave_live) continue;
    float a0[TQ][TI], a1[TQ][TI];
    accumulate<LOOP>(Ts, qrow, lane, a.p, a0, a1);

#pragma unroll
    for (int i = 0; i < TQ; ++i) {
      const int row = wave * TQ + i;
      if (q0 + row >= a.B) break;                 // wave-uniform
#pragma unroll
      for (int j = 0; j < TI; ++j) {
        const int id = n0 + j * 64 + lane;
        const float d = finish<LOOP>(a0[i][j], a1[i][j], a.metric, a.invp);
        if constexpr (!TOPK) {
          if (id < n_end) a.out[(int64_t)(q0 + row) * a.ldo + id] = d;
        } else {
          // candidates better than the row's K-th, in lane order; the threshold lives in scalar registers, and every
          // insertion re-ballots the rest against the new K-th, so a chunk costs one ballot plus its insertions
          const uint64_t key = id < n_end ? rank_key(d, id) : ~0ull;
          uint64_t thr = rank_key(readlane_f(ld[i], K - 1), __builtin_amdgcn_readlane(li[i], K - 1));
          unsigned long long m = __ballot(key < thr);
          if constexpr (EXCL) {
            // per and n0 are multiples of 64: the block's 64 exclusion bits are one aligned word at a wave-uniform address; an
            // excluded item is never a candidate, and the re-ballots below only clear bits of m
            if (n0 + j * 64 < n_end) m &= ~seen_word(a.mask, a.W, q0 + row, n0 + j * 64);
          }
          while (m) {
            const int src = __ffsll((long long)m) - 1;
            const float cd = readlane_f(d, src);
            const int cid = n0 + j * 64 + src;
            // insert (cd, cid): the lanes of the list shift its tail by one in parallel
            const int pos = __popcll(__ballot(lane < K && rank_key(ld[i], li[i]) < rank_key(cd, cid)));
            const float up = shr1(ld[i]);
            const int up_id = shr1(li[i]);
            if (lane == pos) { ld[i] = cd; li[i] = cid; }
            else if (lane > pos && lane < K) { ld[i] = up; li[i] = up_id; }
            thr = rank_key(readlane_f(ld[i], K - 1), __builtin_amdgcn_readlane(li[i], K - 1));
            m &= (m - 1) & __ballot(key < thr);
          }
        }
      }
    }
  }
  if constexpr (TOPK) {
#pragma unroll
    for (int i = 0; i < TQ; ++i) {
      const int row = q0 + wave * TQ + i;
      if (row < a.B && lane < K) {
        const int64_t o = ((int64_t)row * a.splits + blockIdx.y) * K + lane;
        a.part_d[o] = ld[i];
        a.part_i[o] = li[i];
      }
    }
  }
}

// The rank of a target item: row b counts the items of its split whose rank_key is below that of (d(b, g_b), g_b), g_b = targets[b].
// The target's distance is computed first, by the chain every streamed pair goes through (combine over k = 0..127 in order, then
// finish), so it has the bits the stream produces for item g_b: the target itself compares equal and is not counted, and a twin
// row ties and is decided by its id.  Rows and items are tiled as in dist_kernel.  A wave's count of a row is a ballot's popcount:
// it lives in scalar registers and goes out as one partial per (row, split).  A target outside [0, N) reads row 0; its count is
// ignored by the finishing kernel, which reports -1.
template <int LOOP, int TQ, int TI, bool EXCL = false>
__global__ __launch_bounds__(256) void dist_rank_kernel(const DistArgsOf<EXCL> a, const int64_t* __restrict__ targets,
                                                        int32_t* __restrict__ part) {   // part: [B][splits]
  constexpr int QT = 4 * TQ, IT = 64 * TI;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Ts = (float*)smem;                     // [IT][PITCH]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = blockIdx.x * QT;
  const int n_begin = blockIdx.y * a.per, n_end = min(a.N, n_begin + a.per);

  const float* qrow[TQ];
  query_rows<TQ>(a, q0, wave, qrow);
  float4 stage[TI * 8];
  if (n_begin < n_end) load_chunk<TI>(stage, a.t, n_begin, n_end, tid);
  const bool wave_live = q0 + wave * TQ < a.B;

  // the rows' target keys (wave-uniform)
  uint64_t tkey[TQ];
  int cnt[TQ];
#pragma unroll
  for (int i = 0; i < TQ; ++i) {
    const int64_t g64 = targets[min(q0 + wave * TQ + i, a.B - 1)];
    const int g = (uint64_t)g64 < (uint64_t)a.N ? (int)g64 : 0;
    const float* trow = a.t + (int64_t)g * E;
    float t0 = 0.f, t1 = 0.f;
    for (int k = 0; k < E; k += 4) {
      combine4<LOOP>(t0, t1, *(const float4*)(qrow[i] + k), *(const float4*)(trow + k), a.p);
    }
    const uint64_t key = rank_key(finish<LOOP>(t0, t1, a.metric, a.invp), g);
    tkey[i] = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(key >> 32)) << 32) |
              (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
    cnt[i] = 0;
  }

  for (int n0 = n_begin; n0 < n_end; n0 += IT) {
    store_chunk<TI>(stage, Ts, tid);
    if (n0 + IT < n_end) load_chunk<TI>(stage, a.t, n0 + IT, n_end, tid);     // in flight while this chunk is scored
    if (!wave_live) continue;
    float a0[TQ][TI], a1[TQ][TI];
    accumulate<LOOP>(Ts, qrow, lane, a.p, a0, a1);
#pragma unroll
    for (int i = 0; i < TQ; ++i)
#pragma unroll
      for (int j = 0; j < TI; ++j) {
        const int id = n0 + j * 64 + lane;
        const float d = finish<LOOP>(a0[i][j], a1[i][j], a.metric, a.invp);
        unsigned long long m = __ballot(id < n_end && rank_key(d, id) < tkey[i]);
        if constexpr (EXCL) {
          // one aligned word at a wave-uniform address (rows past B repeat row B-1, as their queries do); the target's own bit is
          // never consulted: its key is not below itself
          if (n0 + j * 64 < n_end) m &= ~seen_word(a.mask, a.W, min(q0 + wave * TQ + i, a.B - 1), n0 + j * 64);
        }
        cnt[i] += __popcll(m);
      }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < TQ; ++i) {
      const int row = q0 + wave * TQ + i;
      if (row < a.B) part[(int64_t)row * a.splits + blockIdx.y] = cnt[i];
    }
  }
}

// K best of a row's S sorted partial lists (S <= 256, S*K <= MERGE_CAND): one 64-lane workgroup per row, the lists in LDS,
// lane l holding the heads of lists l, l+64, l+128, l+192
template <bool EXCL = false>
__global__ __launch_bounds__(64) void dist_merge_kernel(const float* __restrict__ pd, const int32_t* __restrict__ pi, int S, int K,
                                                        float* __restrict__ out_d, int64_t* __restrict__ out_i) {
  __shared__ float cd[MERGE_CAND];
  __shared__ int ci[MERGE_CAND];
  const int lane = threadIdx.x, row = blockIdx.x;
  const int total = S * K;
  for (int c = lane; c < total; c += 64) { cd[c] = pd[(int64_t)row * total + c]; ci[c] = pi[(int64_t)row * total + c]; }
  __syncthreads();
  int head[4];
  float hd[4];
  int hi[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int s = lane + 64 * j;
    head[j] = 0;
    hd[j] = s < S ? cd[s * K] : __builtin_nanf("");
    hi[j] = s < S ? ci[s * K] : NONE_ID;
  }
  for (int r = 0; r < K; ++r) {
    float bd = hd[0];
    int bi = hi[0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (rank_key(hd[j], hi[j]) < rank_key(bd, bi)) { bd = hd[j]; bi = hi[j]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float od = __shfl_xor(bd, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (rank_key(od, oi) < rank_key(bd, bi)) { bd = od; bi = oi; }
    }
    // k <= n_items, so the best head is a real item; its id is unique across the lists.  EXCL: a row may have fewer than K items
    // left; then every head is the sentinel, nothing advances, and the slot reads (+inf, -1)
    if constexpr (EXCL) {
      if (bi == NONE_ID) { bd = INFINITY; bi = -1; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (hi[j] == bi) {
        const int s = lane + 64 * j;
        ++head[j];
        hd[j] = head[j] < K ? cd[s * K + head[j]] : __builtin_nanf("");
        hi[j] = head[j] < K ? ci[s * K + head[j]] : NONE_ID;
      }
    if (lane == 0) {
      out_d[(int64_t)row * K + r] = bd;
      out_i[(int64_t)row * K + r] = bi;
    }
  }
}

// cosine: x / |x|;  correlation: (x - mean) / |x - mean|.  A zero row (cosine) or a constant row (correlation: its centred row is
// exactly zero in exact arithmetic) becomes a NaN row.  One wave per row, two elements per lane, fixed-order sums.
__global__ __launch_bounds__(256) void dist_prep_kernel(const float* __restrict__ x, int64_t ldx, int rows, int centre,
                                                        float* __restrict__ y) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  if (r >= rows) return;
  float v0 = x[(int64_t)r * ldx + lane], v1 = x[(int64_t)r * ldx + lane + 64];
  bool degenerate;
  if (centre) {
    const float mean = __fdiv_rn(wave_sum(__fadd_rn(v0, v1)), (float)E);
    degenerate = wave_max(fmaxf(v0, v1)) == -wave_max(-fminf(v0, v1));
    v0 = __fsub_rn(v0, mean);
    v1 = __fsub_rn(v1, mean);
  }
  const float ss = wave_sum(__fmaf_rn(v1, v1, __fmul_rn(v0, v0)));
  if (!centre) degenerate = ss == 0.f;
  const float inv = __fdiv_rn(1.f, __fsqrt_rn(ss));
  y[(int64_t)r * E + lane] = degenerate ? __builtin_nanf("") : __fmul_rn(v0, inv);
  y[(int64_t)r * E + lane + 64] = degenerate ? __builtin_nanf("") : __fmul_rn(v1, inv);
}

bool needs_aux(int metric) { return metric == COSINE || metric == CORRELATION; }

// minkowski with p = 1, 2, inf is cityblock, euclidean, chebyshev (same kernel, same bits)
int effective_metric(int metric, double p) {
  if (metric != MINKOWSKI) return metric;
  if (p == 1.0) return CITYBLOCK;
  if (p == 2.0) return EUCLIDEAN;
  if (__builtin_isinf(p)) return CHEBYSHEV;
  return MINKOWSKI;
}

struct Plan {
  bool big;            // TQ = 8, TI = 2 (QT = 32, IT = 128); else TQ = 1, TI = 1 (QT = 4, IT = 64)
  int tiles, splits, per;
};

Plan make_plan(int B, int N, int K) {
  Plan pl;
  pl.big = B > 4;
  const int qt = pl.big ? 32 : 4, it = pl.big ? 128 : 64;
  pl.tiles = (B + qt - 1) / qt;
  const int chunks = (N + it - 1) / it;
  int s = (TARGET_WG + pl.tiles - 1) / pl.tiles;     // small batches fill the GPU through the item split
  s = std::min(s, chunks);
  s = std::min(s, MAX_SPLITS);
  if (K > 0) s = std::min(s, MERGE_CAND / K);
  s = std::max(s, 1);
  pl.per = (chunks + s - 1) / s * it;
  pl.splits = (N + pl.per - 1) / pl.per;             // no empty split
  return pl;
}

size_t lds_bytes(bool big) { return (size_t)(big ? 128 : 64) * PITCH * 4; }

// launches KERNEL over the plan's grid; each kernel raises its dynamic-LDS limit once
template <auto KERNEL, class... Args> int launch_tiled(const Plan& pl, hipStream_t st, const Args&... args) {
  const size_t lds = lds_bytes(pl.big);
  static bool attr = false;
  if (!attr) {
    RECNN_HIP(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3(pl.tiles, pl.splits), dim3(256), lds, st, args...);
  return 0;
}

template <int V> using Int = std::integral_constant<int, V>;

// f(loop kind, TQ, TI), as compile-time constants, for the metric's inner loop and the plan's tile
template <class F> int dispatch(int metric, const Plan& pl, F f) {
  auto tile = [&](auto loop) {
    return pl.big ? f(loop, Int<8>{}, Int<2>{}) : f(loop, Int<1>{}, Int<1>{});
  };
  switch (metric) {
    case SQEUCLIDEAN: case EUCLIDEAN: return tile(Int<L_SQ>{});
    case CITYBLOCK: return tile(Int<L_ABS>{});
    case CHEBYSHEV: return tile(Int<L_MAX>{});
    case MINKOWSKI: return tile(Int<L_POW>{});
    case CANBERRA: return tile(Int<L_CANB>{});
    case BRAYCURTIS: return tile(Int<L_BRAY>{});
    default: return tile(Int<L_DOT>{});
  }
}

template <bool TOPK, bool EXCL = false> int launch(const DistArgsOf<EXCL>& a, const Plan& pl, hipStream_t st) {
  return dispatch(a.metric, pl, [&](auto loop, auto tq, auto ti) { return launch_tiled<dist_kernel<decltype(loop)::value, decltype(tq)::value, decltype(ti)::value, TOPK, EXCL>>(pl, st, a); });
}

template <bool EXCL = false> int launch_rank(const DistArgsOf<EXCL>& a, const Plan& pl, const int64_t* targets, int32_t* part, hipStream_t st) {
  return dispatch(a.metric, pl, [&](auto loop, auto tq, auto ti) {
    return launch_tiled<dist_rank_kernel<decltype(loop)::value, decltype(tq)::value, decltype(ti)::value, EXCL>>(pl, st, a, targets, part);
  });
}

int64_t query_prep_bytes(int B, int metric) { return needs_aux(metric) ? ((int64_t)B * E * 4 + 255) / 256 * 256 : 0; }

// argument checks shared by matrix and top-K (before any HIP call)
int check_common(const char* fn, const float* q, int64_t ld_q, int B, const float* table, int N, int emb_dim, int metric, double p,
                 const float* aux) {
  RECNN_REQUIRE(metric >= SQEUCLIDEAN && metric <= CORRELATION, "%s: unknown metric %d", fn, metric);
  RECNN_REQUIRE(metric != MINKOWSKI || p >= 1.0, "%s: minkowski needs p >= 1 (got %g)", fn, p);   // NaN fails too
  RECNN_REQUIRE((q || B == 0) && table, "%s: null pointer", fn);   // an empty batch may come without rows
  RECNN_REQUIRE(!needs_aux(metric) || aux, "%s: cosine / correlation need the item aux rows (recnn_dist_item_aux)", fn);
  RECNN_REQUIRE(B >= 0 && N > 0, "%s: need n_queries >= 0 and n_items > 0", fn);
  RECNN_REQUIRE(emb_dim == E, "%s: emb_dim must be 128 (the reference's embedding width)", fn);
  RECNN_REQUIRE(aligned16(q, table, aux) && ld_q % 4 == 0 && ld_q >= E,
                "%s: 16-byte alignment (rows and ld_q)", fn);
  return 0;
}

// fills the args common to both epilogues; cosine / correlation queries are prepared into the workspace first
int prepare(DistArgs& a, const float* q, int64_t ld_q, int B, const float* table, int N, int metric, double p, const float* aux,
            void* ws, hipStream_t st) {
  a = DistArgs{};
  a.metric = effective_metric(metric, p);
  a.p = (float)p;
  a.invp = (float)(1.0 / p);
  a.q = q; a.ldq = ld_q; a.B = B; a.t = table; a.N = N;
  if (needs_aux(metric)) {
    hipLaunchKernelGGL(dist_prep_kernel, dim3((B + 3) / 4), dim3(256), 0, st, q, ld_q, B, (int)(metric == CORRELATION), (float*)ws);
    a.q = (const float*)ws; a.ldq = E; a.t = aux;
  }
  return 0;
}
}  // namespace

extern "C" int recnn_dist_item_aux_floats(int n_items, int emb_dim, int metric, int64_t* h_floats) {
  RECNN_REQUIRE(h_floats && n_items >= 0 && emb_dim == E && metric >= SQEUCLIDEAN && metric <= CORRELATION,
                "dist_item_aux_floats: bad arguments (emb_dim 128, metric id 0..8)");
  *h_floats = needs_aux(metric) ? (int64_t)n_items * E : 0;
  return 0;
}

extern "C" int recnn_dist_item_aux(const float* table, int n_items, int emb_dim, int metric, float* aux, void* stream) {
  RECNN_REQUIRE(needs_aux(metric), "dist_item_aux: only cosine / correlation have an item aux");
  RECNN_REQUIRE(table && aux && n_items > 0 && emb_dim == E, "dist_item_aux: bad arguments");
  RECNN_REQUIRE(aligned16(table, aux), "dist_item_aux: 16-byte alignment");
  hipLaunchKernelGGL(dist_prep_kernel, dim3((n_items + 3) / 4), dim3(256), 0, (hipStream_t)stream, table, (int64_t)E, n_items,
                     (int)(metric == CORRELATION), aux);
  return recnn_check_hip(hipGetLastError(), "dist_prep_kernel");
}

extern "C" int recnn_dist_workspace_bytes(int n_queries, int n_items, int metric, int k, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes && n_queries >= 0 && n_items > 0 && metric >= SQEUCLIDEAN && metric <= CORRELATION && k >= 0 && k <= KMAX,
                "dist_workspace_bytes: bad arguments (k = 0 for the matrix, else k <= 64)");
  int64_t b = query_prep_bytes(n_queries, metric);
  if (k > 0 && n_queries > 0) b += (int64_t)n_queries * make_plan(n_queries, n_items, k).splits * k * 8;
  *h_bytes = b;
  return 0;
}

extern "C" int recnn_dist_matrix(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                                 int metric, double p, const float* item_aux, float* out, int64_t ld_out, void* workspace,
                                 void* stream) {
  if (int rc = check_common("dist_matrix", queries, ld_q, n_queries, table, n_items, emb_dim, metric, p, item_aux)) return rc;
  RECNN_REQUIRE((out || n_queries == 0) && ld_out >= n_items, "dist_matrix: null output or ld_out < n_items");
  RECNN_REQUIRE(workspace || !needs_aux(metric) || n_queries == 0, "dist_matrix: cosine / correlation need the workspace");
  RECNN_REQUIRE(aligned16(workspace), "dist_matrix: 16-byte alignment (workspace)");
  if (n_queries == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  DistArgs a;
  prepare(a, queries, ld_q, n_queries, table, n_items, metric, p, item_aux, workspace, st);
  const Plan pl = make_plan(n_queries, n_items, 0);
  a.per = pl.per; a.out = out; a.ldo = ld_out;
  if (int rc = launch<false>(a, pl, st)) return rc;
  return recnn_check_hip(hipGetLastError(), "dist_matrix");
}

namespace {
template <bool EXCL>
int dist_topk_impl(const char* fn, const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                   int metric, double p, const float* item_aux, int k, float* out_dist, int64_t* out_ids, void* workspace,
                   void* stream, const uint64_t* mask, int64_t words_per_row) {
  if (int rc = check_common(fn, queries, ld_q, n_queries, table, n_items, emb_dim, metric, p, item_aux)) return rc;
  RECNN_REQUIRE((out_dist && out_ids && workspace) || n_queries == 0, "%s: null pointer", fn);
  RECNN_REQUIRE(k > 0 && k <= KMAX && k <= n_items, "%s: need 0 < k <= min(64, n_items)", fn);
  RECNN_REQUIRE(aligned16(workspace), "%s: 16-byte alignment (workspace)", fn);
  if constexpr (EXCL) {
    if (int rc = seen_check(fn, mask, words_per_row, n_queries, n_items)) return rc;
  }
  if (n_queries == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  DistArgsOf<EXCL> a;
  prepare(a, queries, ld_q, n_queries, table, n_items, metric, p, item_aux, workspace, st);
  const Plan pl = make_plan(n_queries, n_items, k);
  a.per = pl.per; a.K = k; a.splits = pl.splits;
  a.part_d = (float*)((char*)workspace + query_prep_bytes(n_queries, metric));
  a.part_i = (int32_t*)(a.part_d + (int64_t)n_queries * pl.splits * k);
  if constexpr (EXCL) { a.mask = mask; a.W = words_per_row; }
  if (int rc = launch<true, EXCL>(a, pl, st)) return rc;
  hipLaunchKernelGGL(dist_merge_kernel<EXCL>, dim3(n_queries), dim3(64), 0, st, a.part_d, a.part_i, pl.splits, k, out_dist, out_ids);
  return recnn_check_hip(hipGetLastError(), fn);
}

template <bool EXCL>
int dist_target_rank_impl(const char* fn, const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items,
                          int emb_dim, int metric, double p, const float* item_aux, const int64_t* targets, int32_t* out_rank,
                          void* workspace, void* stream, const uint64_t* mask, int64_t words_per_row) {
  if (int rc = check_common(fn, queries, ld_q, n_queries, table, n_items, emb_dim, metric, p, item_aux)) return rc;
  RECNN_REQUIRE((targets && out_rank && workspace) || n_queries == 0, "%s: null pointer", fn);
  RECNN_REQUIRE(aligned16(workspace), "%s: 16-byte alignment (workspace)", fn);
  if constexpr (EXCL) {
    if (int rc = seen_check(fn, mask, words_per_row, n_queries, n_items)) return rc;
  }
  if (n_queries == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  DistArgsOf<EXCL> a;
  prepare(a, queries, ld_q, n_queries, table, n_items, metric, p, item_aux, workspace, st);
  const Plan pl = make_plan(n_queries, n_items, 0);
  a.per = pl.per; a.splits = pl.splits;
  if constexpr (EXCL) { a.mask = mask; a.W = words_per_row; }
  int32_t* part = (int32_t*)((char*)workspace + query_prep_bytes(n_queries, metric));
  if (int rc = launch_rank<EXCL>(a, pl, targets, part, st)) return rc;
  hipLaunchKernelGGL(target_rank_finish_kernel, dim3((n_queries + 255) / 256), dim3(256), 0, st, part, pl.splits, targets, n_queries,
                     n_items, out_rank);
  return recnn_check_hip(hipGetLastError(), fn);
}
}  // namespace

extern "C" int recnn_dist_topk(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                               int metric, double p, const float* item_aux, int k, float* out_dist, int64_t* out_ids,
                               void* workspace, void* stream) {
  return dist_topk_impl<false>("dist_topk", queries, ld_q, n_queries, table, n_items, emb_dim, metric, p, item_aux, k, out_dist,
                               out_ids, workspace, stream, nullptr, 0);
}

// the same search over the items whose bit in `mask` (seen.h) is clear; short rows end in (+inf, -1)
extern "C" int recnn_dist_topk_excluding(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items,
                                         int emb_dim, int metric, double p, const float* item_aux, int k, float* out_dist,
                                         int64_t* out_ids, void* workspace, void* stream, const uint64_t* mask,
                                         int64_t words_per_row) {
  return dist_topk_impl<true>("dist_topk_excluding", queries, ld_q, n_queries, table, n_items, emb_dim, metric, p, item_aux, k,
                              out_dist, out_ids, workspace, stream, mask, words_per_row);
}

extern "C" int recnn_dist_target_rank_workspace_bytes(int n_queries, int n_items, int metric, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes && n_queries >= 0 && n_items > 0 && metric >= SQEUCLIDEAN && metric <= CORRELATION,
                "dist_target_rank_workspace_bytes: bad arguments");
  int64_t b = query_prep_bytes(n_queries, metric);
  if (n_queries > 0) b += (int64_t)n_queries * make_plan(n_queries, n_items, 0).splits * 4;
  *h_bytes = b;
  return 0;
}

extern "C" int recnn_dist_target_rank(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                                      int metric, double p, const float* item_aux, const int64_t* targets, int32_t* out_rank,
                                      void* workspace, void* stream) {
  return dist_target_rank_impl<false>("dist_target_rank", queries, ld_q, n_queries, table, n_items, emb_dim, metric, p, item_aux,
                                      targets, out_rank, workspace, stream, nullptr, 0);
}

// the same count over the items whose bit in `mask` (seen.h) is clear
extern "C" int recnn_dist_target_rank_excluding(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items,
                                                int emb_dim, int metric, double p, const float* item_aux, const int64_t* targets,
                                                int32_t* out_rank, void* workspace, void* stream, const uint64_t* mask,
                                                int64_t words_per_row) {
  return dist_target_rank_impl<true>("dist_target_rank_excluding", queries, ld_q, n_queries, table, n_items, emb_dim, metric, p,
                                     item_aux, targets, out_rank, workspace, stream, mask, words_per_row);
}
