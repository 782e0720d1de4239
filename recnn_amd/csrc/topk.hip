// topk.hip -- batched exact top-K scoring of action vectors against the item-embedding table (gfx950).
//
// SURVEY.md 8(f2) "next": replaces faiss IndexFlatL2 / IndexFlatIP / IP-on-normalised rows (examples/streamlit_demo.py:190-204)
// and the Milvus service (recnn/data/db_con.py:45-56, `MilvusConnection.search`), two of the external retrieval paths the
// reference uses to turn a generated action into recommended items, by one exact-fp32 MFMA scoring GEMM fused with a
// per-query top-K selection.  It gives the order of scipy's euclidean (and of cosine up to the query's norm) but not the
// scipy metrics of the per-item loop (examples/streamlit_demo.py:207-231, `rank`): those are rank.hip.
//
//   score(q, t):  IP  = q.t          (larger is better)
//                 L2  = |q - t|^2    (smaller is better; squared distance, as faiss IndexFlatL2 reports)
//                 COS = q.t / |t|    (larger is better; the demo normalises the table rows, not the query)
//
// Grid = (ceil(B/64) query tiles) x (S item splits).  A workgroup keeps its 64 query rows in LDS, streams its share
// of the table in 64-item chunks (register-staged, fp32), multiplies with v_mfma_f32_16x16x4_f32 (exact fp32: ranking
// by bf16 scores would reorder near ties), parks the 64x64 score tile in LDS and lets each wave maintain the sorted
// top-K lists of 16 query rows: a chunk's scores are compared against the row's current K-th best with one ballot per
// 64 items, and only the (rare) survivors are inserted.  Ties are broken towards the smaller item id.  Partial lists
// [B][S][K] are merged by a second tiny kernel.
//
// topk_rank_kernel scores the same way and, instead of selecting, counts per query row the items that come before one target
// item: no lists, no limit on K.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "seen.h"
#include "target_rank.h"
#include "topk_dev.h"   // tile shape, staging, score_tile(), rank_score(), the scan's LDS layout; select_dev.h: orders, insert, merge

namespace {
struct TopkArgs {
  const float* q; int64_t ldq; int B;
  const float* table; int N;
  const float* aux;        // L2: |t|^2 per item;  COS: 1/|t| per item;  IP: unused
  int metric, K, splits;
  float* part_score;       // [B][S][K]  internal key (larger = better)
  int32_t* part_id;        // [B][S][K]
};
// the excluding kernel takes the mask of seen.h behind the same arguments, and a split that is a multiple of IT so that a chunk's 64
// exclusion bits are one word (results do not depend on the split); the plain kernel keeps its argument block and its split
struct TopkArgsX : TopkArgs { const uint64_t* mask; int64_t W; int per; };

template <bool EXCL> struct TopkLds : ScanLds {
  static constexpr size_t Xw = shared;                        // EXCL: uint64 [QT] the chunk's exclusion word of each query row
  static constexpr size_t bytes = Xw + (EXCL ? QT * 8 : 0);
};

// The chunk stage, the key block and the list insert below are written out, although topk_dev.h (stage_chunk, keys_to_tile) and
// select_dev.h (insert_survivors<better>) hold the same code for ivf_scan_kernel: through those functions this kernel measured
// 1.0 to 1.9 % slower at B = 2048 (N = 26,744 and 100,000), so it keeps the instruction stream it had.
template <bool EXCL = false>
__global__ __launch_bounds__(256) void topk_scores_kernel(const std::conditional_t<EXCL, TopkArgsX, TopkArgs> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using Lds = TopkLds<EXCL>;
  float* Qs = (float*)(smem + Lds::Qs);
  float* Ts = (float*)(smem + Lds::Ts);
  float* Ss = (float*)(smem + Lds::Ss);
  float* Ls = (float*)(smem + Lds::Ls);
  int* Li = (int*)(smem + Lds::Li);
  uint64_t* Xw = (uint64_t*)(smem + Lds::Xw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * QT;
  int per;
  if constexpr (EXCL) per = a.per;
  else per = (a.N + a.splits - 1) / a.splits;
  const int n_begin = blockIdx.y * per, n_end = min(a.N, n_begin + per);
  const int K = a.K;

  for (int i = tid; i < QT * KMAX; i += 256) { Ls[i] = -INFINITY; Li[i] = NONE_ID; }
  stage_rows(Qs, a.q, a.ldq, tid, [&](int r, int64_t& row) { row = q0 + r; return q0 + r < a.B; });   // rows past B are zero
  const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;   // wave tile: 32 queries x 32 items
  const int fr = lane & 15, fg = lane >> 4;
  __syncthreads();

  for (int n0 = n_begin; n0 < n_end; n0 += IT) {
    // ---- table chunk -> LDS
    for (int c = tid; c < IT * (DIM / 4); c += 256) {
      const int r = c / (DIM / 4), k4 = c % (DIM / 4);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n0 + r < n_end) v = *(const float4*)(a.table + (int64_t)(n0 + r) * DIM + k4 * 4);
      *(float4*)&Ts[r * PITCH + k4 * 4] = v;
    }
    if constexpr (EXCL) {
      if (tid < QT) Xw[tid] = q0 + tid < a.B ? seen_word(a.mask, a.W, q0 + tid, n0) : 0ull;   // n0 is a multiple of 64
    }
    __syncthreads();
    f32x4 acc[2][2];
    score_tile(Qs, Ts, wm0, wn0, fr, fg, acc);                // scores = Q T^T (exact fp32 MFMA)
    // ---- ranking key (larger = better) into the score tile
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = wn0 + j * 16 + fr;
        const int n = n0 + col;
        float ax = 0.f;
        if (a.metric != M_IP && n < n_end) ax = a.aux[n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = wm0 + i * 16 + fg * 4 + r;
          float s = rank_score(acc[i][j][r], ax, a.metric);
          if (n >= n_end) s = -INFINITY;
          Ss[row * (IT + 4) + col] = s;
        }
      }
    __syncthreads();
    // ---- selection: wave w owns query rows 16w .. 16w+15; lane = item of the chunk
    for (int rr = 0; rr < 16; ++rr) {
      const int row = wave * 16 + rr;
      if (q0 + row >= a.B) break;
      float* ls = Ls + row * KMAX;
      int* li = Li + row * KMAX;
      const float s = Ss[row * (IT + 4) + lane];
      const int id = n0 + lane;
      float thr = ls[K - 1];
      int thr_id = li[K - 1];
      unsigned long long m = __ballot(id < n_end && better(s, id, thr, thr_id));
      if constexpr (EXCL) m &= ~Xw[row];                // an excluded item is never a candidate
      while (m) {                                       // rare after the first chunks
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float cs = __shfl(s, src, 64);
        const int cid = n0 + src;
        if (!better(cs, cid, ls[K - 1], li[K - 1])) continue;
        // insert (cs, cid) into the sorted list: lanes shift the tail in parallel
        const float mine = lane < K ? ls[lane] : 0.f;
        const int mine_id = lane < K ? li[lane] : 0;
        const bool before = lane < K && better(mine, mine_id, cs, cid);       // entries that stay in front
        const int pos = __popcll(__ballot(before));                            // insertion position
        const float up = __shfl_up(mine, 1, 64);                               // (all lanes: no divergent shuffles)
        const int up_id = __shfl_up(mine_id, 1, 64);
        if (lane < K) {
          if (lane == pos) { ls[lane] = cs; li[lane] = cid; }
          else if (lane > pos) { ls[lane] = up; li[lane] = up_id; }
        }
      }
    }
    __syncthreads();
  }
  // ---- partial lists out
  for (int i = tid; i < QT * K; i += 256) {
    const int row = i / K, j = i % K;
    if (q0 + row < a.B) {
      const int64_t o = ((int64_t)(q0 + row) * a.splits + blockIdx.y) * K + j;
      a.part_score[o] = Ls[row * KMAX + j];
      a.part_id[o] = Li[row * KMAX + j];
    }
  }
}

// merge S sorted partial lists per query (S*K <= 512); one wave per query row
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ ps, const int32_t* __restrict__ pi, int B, int S, int K,
                                                         int metric, const float* __restrict__ q, int64_t ldq, int E,
                                                         float* __restrict__ out_d, int64_t* __restrict__ out_i) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= B) return;
  const int64_t total = S * K;
  float qn = 0.f;
  if (metric == M_L2) qn = query_sqnorm(q, ldq, row, E, lane);
  merge_candidates<better>(ps + row * total, pi + row * total, (int)total, K, -INFINITY, lane, [&](int k, float bs, int bi) {
    out_d[(int64_t)row * K + k] = metric == M_L2 ? fmaxf(qn - bs, 0.f) : bs;  // L2: |q|^2 - (2 q.t - |t|^2)
    out_i[(int64_t)row * K + k] = bi == NONE_ID ? -1 : bi;
  });
}

// per-item auxiliary term of the metric: L2 -> |t|^2, COS -> 1/|t|
__global__ __launch_bounds__(256) void topk_aux_kernel(const float* __restrict__ table, int N, int E, int metric, float* __restrict__ aux) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * 4 + wave;
  if (n >= N) return;
  float s = 0.f;
  for (int k = lane; k < E; k += 64) { const float v = table[(int64_t)n * E + k]; s += v * v; }
  s = wave_sum(s);
  if (lane == 0) aux[n] = metric == M_L2 ? s : (s > 0.f ? 1.0f / sqrtf(s) : 0.f);
}

// ---------------------------------------------------------------- the rank of a target item
struct TopkRankArgs {
  const float* q; int64_t ldq; int B;
  const float* table; int N;
  const float* aux;
  int metric, splits, per;   // per: items per split, a multiple of IT
  const int64_t* targets;    // [B]
  int32_t* part;             // [B][splits]
};
struct TopkRankArgsX : TopkRankArgs { const uint64_t* mask; int64_t W; };

// Row b counts the items of its split that come before item g_b = targets[b].  The workgroup first gathers the target rows of its
// 64 queries into the chunk buffer and runs the scoring tile on them: the diagonal holds each row's target key, with the bits the
// stream produces for that pair (an element's k order does not depend on its place in the tile).  Then it streams its split
// (register-staged) and compares every score, still in the MFMA accumulators, against its row's target key; the target itself is
// skipped by id.  Counts: per lane, summed over each 16-lane row, then over the two waves of a row with LDS integer atomics.  A
// target outside [0, N) scores a zero row; the finishing kernel reports -1 for it.
// EXCL: an item whose bit is set in its row's mask (seen.h) is not counted.  The chunk's 64 words, one per query row, travel with the
// register-staged table chunk into LDS; the target's own bit is never consulted (the target is skipped by id).
template <bool EXCL = false>
__global__ __launch_bounds__(256) void topk_rank_kernel(const std::conditional_t<EXCL, TopkRankArgsX, TopkRankArgs> a) {
  constexpr int STAGE = IT * (DIM / 4) / 256;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Qs = (float*)smem;                  // [QT][PITCH]
  float* Ts = Qs + QT * PITCH;               // [IT][PITCH]
  float* Tk = Ts + IT * PITCH;               // [QT] target keys
  int* Tg = (int*)(Tk + QT);                 // [QT] target ids, -1: none
  int* Cn = Tg + QT;                         // [QT] counts
  uint64_t* Xw = (uint64_t*)(Cn + QT);       // EXCL: [QT] the chunk's exclusion word of each query row (8-byte aligned: 3 QT ints)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * QT;
  const int n_begin = blockIdx.y * a.per, n_end = min(a.N, n_begin + a.per);

  if (tid < QT) {
    const int64_t g = q0 + tid < a.B ? a.targets[q0 + tid] : -1;
    Tg[tid] = (uint64_t)g < (uint64_t)a.N ? (int)g : -1;
    Cn[tid] = 0;
  }
  stage_rows(Qs, a.q, a.ldq, tid, [&](int r, int64_t& row) { row = q0 + r; return q0 + r < a.B; });
  float4 stage[STAGE];
  uint64_t xstage = 0ull;
  auto load_chunk = [&](int n0) {
#pragma unroll
    for (int s = 0; s < STAGE; ++s) {
      const int c = tid + s * 256, r = c >> 5, k4 = c & 31;
      stage[s] = n0 + r < n_end ? *(const float4*)(a.table + (int64_t)(n0 + r) * DIM + k4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if constexpr (EXCL) {
      if (tid < QT && q0 + tid < a.B) xstage = seen_word(a.mask, a.W, q0 + tid, n0);   // per and n0 are multiples of 64
    }
  };
  if (n_begin < n_end) load_chunk(n_begin);
  const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;   // wave tile: 32 queries x 32 items
  const int fr = lane & 15, fg = lane >> 4;
  __syncthreads();
  // ---- target rows -> Ts, scored like a chunk; the diagonal is each row's target key
  stage_rows(Ts, a.table, DIM, tid, [&](int r, int64_t& row) { row = Tg[r]; return row >= 0; });
  __syncthreads();
  f32x4 acc[2][2];
  score_tile(Qs, Ts, wm0, wn0, fr, fg, acc);
  if (wm0 == wn0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int col = wn0 + i * 16 + fr;
      const int g = Tg[col];
      const float ax = a.metric != M_IP && g >= 0 ? a.aux[g] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (wm0 + i * 16 + fg * 4 + r == col) Tk[col] = rank_score(acc[i][i][r], ax, a.metric);
    }
  }
  __syncthreads();
  float tk[2][4];
  int tg[2][4], cnt[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wm0 + i * 16 + fg * 4 + r;
      tk[i][r] = Tk[row];
      tg[i][r] = Tg[row];
      cnt[i][r] = 0;
    }

  for (int n0 = n_begin; n0 < n_end; n0 += IT) {
    __syncthreads();                              // the previous tile's readers are done
#pragma unroll
    for (int s = 0; s < STAGE; ++s) {
      const int c = tid + s * 256;
      *(float4*)&Ts[(c >> 5) * PITCH + (c & 31) * 4] = stage[s];
    }
    if constexpr (EXCL) {
      if (tid < QT) Xw[tid] = xstage;
    }
    __syncthreads();
    if (n0 + IT < n_end) load_chunk(n0 + IT);     // in flight while this chunk is scored
    score_tile(Qs, Ts, wm0, wn0, fr, fg, acc);
    uint64_t xw[2][4];
    if constexpr (EXCL) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) xw[i][r] = Xw[wm0 + i * 16 + fg * 4 + r];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn0 + j * 16 + fr;
      const bool live = n < n_end;
      const float ax = a.metric != M_IP && live ? a.aux[n] : 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = rank_score(acc[i][j][r], ax, a.metric);
          bool counts = live && n != tg[i][r];
          if constexpr (EXCL) counts = counts && !((xw[i][r] >> (n & 63)) & 1);
          cnt[i][r] += counts && comes_before(s, n, tk[i][r], tg[i][r]);
        }
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int c = cnt[i][r];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);      // over the 16 lanes that share fg
      if (fr == 0) atomicAdd(&Cn[wm0 + i * 16 + fg * 4 + r], c);
    }
  __syncthreads();
  if (tid < QT && q0 + tid < a.B) a.part[(int64_t)(q0 + tid) * a.splits + blockIdx.y] = Cn[tid];
}

constexpr int RANK_TARGET_WG = 512;   // workgroups to aim for: two per CU, which is what the LDS tile lets a CU hold
constexpr int RANK_MIN_CHUNKS = 4;    // per split: the target tile costs one chunk's work

struct RankPlan { int tiles, splits, per; };

RankPlan make_rank_plan(int B, int N) {
  RankPlan pl;
  pl.tiles = (B + QT - 1) / QT;
  const int chunks = (N + IT - 1) / IT;
  int s = std::min(RANK_TARGET_WG / pl.tiles, (chunks + RANK_MIN_CHUNKS - 1) / RANK_MIN_CHUNKS);
  s = std::max(s, 1);
  pl.per = (chunks + s - 1) / s * IT;
  pl.splits = (N + pl.per - 1) / pl.per;     // no empty split
  return pl;
}
}  // namespace

extern "C" int recnn_topk_workspace_bytes(int n_queries, int k, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes && n_queries >= 0 && k > 0 && k <= KMAX, "topk_workspace_bytes: bad arguments (k <= 64)");
  *h_bytes = (int64_t)n_queries * 8 * k * 8;   // 8 splits x (score + id)
  return 0;
}

extern "C" int recnn_topk_item_aux(const float* table, int n_items, int emb_dim, int metric, float* aux, void* stream) {
  RECNN_REQUIRE(table && aux && n_items > 0 && emb_dim > 0 && (metric == M_L2 || metric == M_COS), "topk_item_aux: bad arguments");
  hipLaunchKernelGGL(topk_aux_kernel, dim3((n_items + 3) / 4), dim3(256), 0, (hipStream_t)stream, table, n_items, emb_dim, metric, aux);
  return recnn_check_hip(hipGetLastError(), "topk_aux_kernel");
}

namespace {
template <bool EXCL>
int topk_search_impl(const char* fn, const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                     int metric, const float* item_aux, int k, float* out_dist, int64_t* out_ids, void* workspace, void* stream,
                     const uint64_t* mask, int64_t words_per_row) {
  RECNN_REQUIRE(queries && table && out_dist && out_ids && workspace, "%s: null pointer", fn);
  RECNN_REQUIRE(n_queries >= 0 && n_items > 0 && k > 0 && k <= KMAX && k <= n_items, "%s: need 0 < k <= min(64, n_items)", fn);
  RECNN_REQUIRE(emb_dim == 128, "%s: emb_dim must be 128 (the reference's embedding width)", fn);
  RECNN_REQUIRE(metric == M_IP || ((metric == M_L2 || metric == M_COS) && item_aux), "%s: L2 / COS need the item aux array", fn);
  RECNN_REQUIRE((((uintptr_t)queries | (uintptr_t)table) & 15) == 0 && (ld_q % 4) == 0, "%s: 16-byte alignment", fn);
  if constexpr (EXCL) {
    if (int rc = seen_check(fn, mask, words_per_row, n_queries, n_items)) return rc;
  }
  if (n_queries == 0) return 0;
  std::conditional_t<EXCL, TopkArgsX, TopkArgs> a;
  a.q = queries; a.ldq = ld_q; a.B = n_queries; a.table = table; a.N = n_items; a.aux = item_aux;
  a.metric = metric; a.K = k;
  const int tiles = (n_queries + QT - 1) / QT;
  int splits = 512 / tiles;               // enough workgroups to fill 256 CUs twice
  if (splits < 1) splits = 1;
  if (splits > 8) splits = 8;
  while (splits > 1 && (n_items + splits - 1) / splits < 4 * IT) --splits;
  if constexpr (EXCL) {                   // whole chunks per split, no empty split (never more splits than the plain launch)
    a.per = ((n_items + splits - 1) / splits + IT - 1) / IT * IT;
    splits = (n_items + a.per - 1) / a.per;
    a.mask = mask; a.W = words_per_row;
  }
  a.splits = splits;
  a.part_score = (float*)workspace;
  a.part_id = (int32_t*)((char*)workspace + (int64_t)n_queries * 8 * k * 4);
  const size_t lds = TopkLds<EXCL>::bytes;
  static bool attr = false;
  if (!attr) {
    RECNN_HIP(hipFuncSetAttribute((const void*)topk_scores_kernel<EXCL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr = true;
  }
  hipLaunchKernelGGL((topk_scores_kernel<EXCL>), dim3(tiles, splits), dim3(256), lds, (hipStream_t)stream, a);
  // a short row's trailing slots hold the lists' sentinel, which the merge reports as id -1 at -inf (L2: +inf)
  hipLaunchKernelGGL(topk_merge_kernel, dim3((n_queries + 3) / 4), dim3(256), 0, (hipStream_t)stream, a.part_score, a.part_id, n_queries,
                     splits, k, metric, queries, ld_q, emb_dim, out_dist, out_ids);
  return recnn_check_hip(hipGetLastError(), fn);
}

template <bool EXCL>
int topk_target_rank_impl(const char* fn, const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items,
                          int emb_dim, int metric, const float* item_aux, const int64_t* targets, int32_t* out_rank, void* workspace,
                          void* stream, const uint64_t* mask, int64_t words_per_row) {
  RECNN_REQUIRE(table && ((queries && targets && out_rank && workspace) || n_queries == 0), "%s: null pointer", fn);
  RECNN_REQUIRE(n_queries >= 0 && n_items > 0, "%s: need n_queries >= 0 and n_items > 0", fn);
  RECNN_REQUIRE(emb_dim == 128, "%s: emb_dim must be 128 (the reference's embedding width)", fn);
  RECNN_REQUIRE(metric == M_IP || ((metric == M_L2 || metric == M_COS) && item_aux), "%s: metric must be IP, or L2 / COS with the item aux array", fn);
  RECNN_REQUIRE(aligned16(queries, table) && ld_q % 4 == 0 && ld_q >= 128, "%s: 16-byte alignment (rows and ld_q)", fn);
  if constexpr (EXCL) {
    if (int rc = seen_check(fn, mask, words_per_row, n_queries, n_items)) return rc;
  }
  if (n_queries == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const RankPlan pl = make_rank_plan(n_queries, n_items);
  std::conditional_t<EXCL, TopkRankArgsX, TopkRankArgs> a;
  a.q = queries; a.ldq = ld_q; a.B = n_queries; a.table = table; a.N = n_items; a.aux = item_aux;
  a.metric = metric; a.splits = pl.splits; a.per = pl.per; a.targets = targets; a.part = (int32_t*)workspace;
  if constexpr (EXCL) { a.mask = mask; a.W = words_per_row; }
  const size_t lds = (size_t)(QT * PITCH + IT * PITCH + 3 * QT) * 4 + (EXCL ? QT * 8 : 0);
  static bool attr = false;
  if (!attr) {
    RECNN_HIP(hipFuncSetAttribute((const void*)topk_rank_kernel<EXCL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr = true;
  }
  hipLaunchKernelGGL(topk_rank_kernel<EXCL>, dim3(pl.tiles, pl.splits), dim3(256), lds, st, a);
  hipLaunchKernelGGL(target_rank_finish_kernel, dim3((n_queries + 255) / 256), dim3(256), 0, st, a.part, pl.splits, targets, n_queries,
                     n_items, out_rank);
  return recnn_check_hip(hipGetLastError(), fn);
}
}  // namespace

extern "C" int recnn_topk_search(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                                 int metric, const float* item_aux, int k, float* out_dist, int64_t* out_ids, void* workspace,
                                 void* stream) {
  return topk_search_impl<false>("topk_search", queries, ld_q, n_queries, table, n_items, emb_dim, metric, item_aux, k, out_dist,
                                 out_ids, workspace, stream, nullptr, 0);
}

// the same search over the items whose bit in `mask` (seen.h) is clear; short rows end in id -1 at -inf (L2: +inf)
extern "C" int recnn_topk_search_excluding(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items,
                                           int emb_dim, int metric, const float* item_aux, int k, float* out_dist, int64_t* out_ids,
                                           void* workspace, void* stream, const uint64_t* mask, int64_t words_per_row) {
  return topk_search_impl<true>("topk_search_excluding", queries, ld_q, n_queries, table, n_items, emb_dim, metric, item_aux, k,
                                out_dist, out_ids, workspace, stream, mask, words_per_row);
}

extern "C" int recnn_topk_target_rank_workspace_bytes(int n_queries, int n_items, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes && n_queries >= 0 && n_items > 0, "topk_target_rank_workspace_bytes: bad arguments");
  *h_bytes = n_queries > 0 ? (int64_t)n_queries * make_rank_plan(n_queries, n_items).splits * 4 : 0;
  return 0;
}

extern "C" int recnn_topk_target_rank(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items, int emb_dim,
                                      int metric, const float* item_aux, const int64_t* targets, int32_t* out_rank, void* workspace,
                                      void* stream) {
  return topk_target_rank_impl<false>("topk_target_rank", queries, ld_q, n_queries, table, n_items, emb_dim, metric, item_aux, targets,
                                      out_rank, workspace, stream, nullptr, 0);
}

// the same count over the items whose bit in `mask` (seen.h) is clear
extern "C" int recnn_topk_target_rank_excluding(const float* queries, int64_t ld_q, int n_queries, const float* table, int n_items,
                                                int emb_dim, int metric, const float* item_aux, const int64_t* targets,
                                                int32_t* out_rank, void* workspace, void* stream, const uint64_t* mask,
                                                int64_t words_per_row) {
  return topk_target_rank_impl<true>("topk_target_rank_excluding", queries, ld_q, n_queries, table, n_items, emb_dim, metric, item_aux,
                                     targets, out_rank, workspace, stream, mask, words_per_row);
}
