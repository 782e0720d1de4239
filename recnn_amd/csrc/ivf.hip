// ivf.hip -- IVF-Flat: a k-means coarse quantiser over the item table, the items stored per nearest centroid, and a search that
// scores only the lists a query probes (gfx950).  What faiss's IndexIVFFlat and Milvus's IVF_FLAT do, and what
// gives `nprobe` of the reference's `MilvusConnection.search` (recnn/data/db_con.py:45-56) a meaning.
//
// The scorer of both steps that rank by distance -- an item's nearest centroid while training, a query's nearest centroids while
// searching -- is topk.hip's flat search, called by the host on the centroid table.  This file holds the rest:
//
//   lists     the inverted index of an assignment (scatter_index.h: a stable counting sort, integers only): list_start is a CSR over
//             the lists, list_ids the item ids list by list, ascending id inside a list.
//   update    centroid[c] = sum(rows of list c) / count[c], one workgroup per list.  The rows of a list are dealt round-robin, in
//             list order, to four waves; each wave sums its share in order, the four partial sums are added as (0 + 1) + (2 + 3), and
//             the division is the correctly rounded fp32 one.  No float atomics: the order is a function of the ids alone.  A list
//             with no items keeps its centroid.
//   gather    the table rows in list order, so that a list is one contiguous stream.
//   scan      list-major.  The B * p (query, probe slot) pairs are inverted by list with scatter_index.h; a workgroup takes one list
//             and up to 64 of the pairs that probe it, keeps their query rows in LDS, streams the list's rows in chunks of 64 through
//             topk_dev.h's staging, scoring tile and key (exact fp32 MFMA, the bits of topk.hip for every pair) and maintains each
//             pair's sorted K best with select_dev.h's ballot insert, under better() like topk_scores_kernel.  Exclusion (seen.h): list order is a permutation of the ids, so a chunk's
//             bits are not one word; a lane looks up the bit of (row, item id) only when its item would enter the row's list.
//   merge     one workgroup per query row folds the p sorted partial lists (up to 64 x 64 candidates) from LDS: a p-way merge, one lane
//             per list, and reports topk.hip's conventions (L2: fmaxf(|q|^2 - key, 0) ascending; IP descending; ties to the smaller
//             id; a short row ends in id -1 at +inf / -inf).
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "scatter_index.h"
#include "seen.h"
#include "topk_dev.h"

namespace {
constexpr int IVF_MAX_PROBE = 64;

struct IdOfI64 {
  const int64_t* ids;
  __device__ int64_t operator()(int j) const { return ids[j]; }
};

// ---------------------------------------------------------------- lists
__global__ void ivf_narrow_kernel(const int64_t* __restrict__ src, int n, int n_dest, int32_t* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t v = src[i];
  dst[i] = (v >= 0 && v < n_dest) ? (int32_t)v : -1;
}

inline int64_t ivf_lists_bytes(int64_t n_items, int nlist) {
  return scatter_index_round(4LL * nlist) + 2 * scatter_index_round(4LL * n_items);
}

// ---------------------------------------------------------------- centroid update
__global__ __launch_bounds__(256) void ivf_update_kernel(const float* __restrict__ table, int n_items, const int* __restrict__ list_start,
                                                         const int* __restrict__ list_ids, float* __restrict__ centroids) {
  __shared__ float part[4][DIM];
  const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s0 = list_start[c], s1 = list_start[c + 1];
  if (s1 <= s0) return;                                  // an empty list keeps its centroid (uniform: no barrier is skipped by some)
  float2 sum = make_float2(0.f, 0.f);
  auto row = [&](int i) {
    const int id = list_ids[i];
    return (unsigned)id < (unsigned)n_items ? *(const float2*)(table + (int64_t)id * DIM + 2 * lane) : make_float2(0.f, 0.f);
  };
  int i = s0 + wave;
  for (; i + 12 < s1; i += 16) {                         // four rows in flight, added in list order
    const float2 v0 = row(i), v1 = row(i + 4), v2 = row(i + 8), v3 = row(i + 12);
    sum.x += v0.x; sum.y += v0.y;
    sum.x += v1.x; sum.y += v1.y;
    sum.x += v2.x; sum.y += v2.y;
    sum.x += v3.x; sum.y += v3.y;
  }
  for (; i < s1; i += 4) {
    const float2 v = row(i);
    sum.x += v.x; sum.y += v.y;
  }
  part[wave][2 * lane] = sum.x;
  part[wave][2 * lane + 1] = sum.y;
  __syncthreads();
  if (threadIdx.x < DIM) {
    const int d = threadIdx.x;
    const float total = (part[0][d] + part[1][d]) + (part[2][d] + part[3][d]);
    centroids[(int64_t)c * DIM + d] = total / (float)(s1 - s0);      // IEEE division (hipcc's default), not a reciprocal multiply
  }
}

// ---------------------------------------------------------------- rows in list order
__global__ __launch_bounds__(256) void ivf_gather_kernel(const float* __restrict__ table, int n_items, const int* __restrict__ list_ids,
                                                         int n_rows, float* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r = c >> 5;
  const int k4 = (int)(c & 31);
  if (r >= n_rows) return;
  const int id = list_ids[r];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if ((unsigned)id < (unsigned)n_items) v = *(const float4*)(table + (int64_t)id * DIM + k4 * 4);
  *(float4*)(out + r * DIM + k4 * 4) = v;
}

// ---------------------------------------------------------------- the scan's work list: (list, group of 64 pairs)
__global__ void ivf_group_count_kernel(const int* __restrict__ pair_start, int nlist, int* __restrict__ gcount) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l < nlist) gcount[l] = (pair_start[l + 1] - pair_start[l] + QT - 1) / QT;
}
__global__ void ivf_group_fill_kernel(const int* __restrict__ gstart, int nlist, int max_groups, int2* __restrict__ work) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nlist) return;
  const int g0 = gstart[l], n = gstart[l + 1] - g0;
  for (int g = 0; g < n; ++g)
    if (g0 + g < max_groups) work[g0 + g] = make_int2(l, g);
}

struct IvfScanArgs {
  const float* q; int64_t ldq;
  const float* rows;         // [N][128] table rows in list order
  const float* aux;          // [N] |t|^2 in list order (L2)
  const int* list_start;     // [nlist + 1]
  const int* list_ids;       // [N]
  const int* pair_start;     // [nlist + 1] CSR of the (query, slot) pairs by list
  const int* pair_sorted;    // [B p] pair index j = b p + slot, ascending inside a list
  const int* gstart;         // [nlist + 1] CSR of the work list by list
  const int2* work;          // [groups] (list, group)
  int nlist, p, metric, K;
  float* part_score;         // [B p][K] internal key (larger = better)
  int32_t* part_id;          // [B p][K]
};
struct IvfScanArgsX : IvfScanArgs { const uint64_t* mask; int64_t W; };

struct IvfLds : ScanLds {
  static constexpr size_t Pj = shared;                        // int [QT] pair index of each row, -1: none
  static constexpr size_t Pb = Pj + QT * 4;                   // int [QT] its query row
  static constexpr size_t Ci = Pb + QT * 4;                   // int [IT] item ids of the chunk
  static constexpr size_t bytes = Ci + IT * 4;
};

template <bool EXCL>
__global__ __launch_bounds__(256) void ivf_scan_kernel(const std::conditional_t<EXCL, IvfScanArgsX, IvfScanArgs> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Qs = (float*)(smem + IvfLds::Qs);
  float* Ts = (float*)(smem + IvfLds::Ts);
  float* Ss = (float*)(smem + IvfLds::Ss);
  float* Ls = (float*)(smem + IvfLds::Ls);
  int* Li = (int*)(smem + IvfLds::Li);
  int* Pj = (int*)(smem + IvfLds::Pj);
  int* Pb = (int*)(smem + IvfLds::Pb);
  int* Ci = (int*)(smem + IvfLds::Ci);
  if ((int)blockIdx.x >= a.gstart[a.nlist]) return;      // the grid is the host's upper bound of the work list
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int2 wk = a.work[blockIdx.x];
  const int ps = a.pair_start[wk.x] + wk.y * QT;
  const int pn = min(QT, a.pair_start[wk.x + 1] - ps);
  const int n_begin = a.list_start[wk.x], n_end = a.list_start[wk.x + 1];
  const int K = a.K;

  for (int i = tid; i < QT * KMAX; i += 256) { Ls[i] = -INFINITY; Li[i] = NONE_ID; }
  if (tid < QT) {
    const int j = tid < pn ? a.pair_sorted[ps + tid] : -1;
    Pj[tid] = j;
    Pb[tid] = j >= 0 ? j / a.p : 0;
  }
  __syncthreads();
  // query rows of the group's pairs -> LDS (rows past the group are zero)
  stage_rows(Qs, a.q, a.ldq, tid, [&](int r, int64_t& row) {
    if (r < pn) row = Pb[r];
    return r < pn;
  });
  const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;   // wave tile: 32 queries x 32 items
  const int fr = lane & 15, fg = lane >> 4;
  __syncthreads();

  for (int n0 = n_begin; n0 < n_end; n0 += IT) {
    stage_chunk(Ts, a.rows, n0, n_end, tid);
    if (tid < IT) Ci[tid] = n0 + tid < n_end ? a.list_ids[n0 + tid] : NONE_ID;
    __syncthreads();
    f32x4 acc[2][2];
    score_tile(Qs, Ts, wm0, wn0, fr, fg, acc);
    keys_to_tile(acc, Ss, a.aux, a.metric == M_L2 ? M_L2 : M_IP, n0, n_end, wm0, wn0, fr, fg);   // the lists know IP and L2 only
    __syncthreads();
    // ---- selection: wave w owns rows 16w .. 16w+15; lane = item of the chunk
    for (int rr = 0; rr < 16; ++rr) {
      const int row = wave * 16 + rr;
      if (row >= pn) break;
      float* ls = Ls + row * KMAX;
      int* li = Li + row * KMAX;
      const float s = Ss[row * SPITCH + lane];
      const int id = Ci[lane];
      bool cand = n0 + lane < n_end && better(s, id, ls[K - 1], li[K - 1]);
      if constexpr (EXCL) {                             // the bit of (row, item id), for would-be survivors only
        if (cand) cand = !((a.mask[(int64_t)Pb[row] * a.W + (id >> 6)] >> (id & 63)) & 1ull);
      }
      insert_survivors<better>(__ballot(cand), s, [&](int src) { return __shfl(id, src, 64); }, ls, li, K, lane);
    }
    __syncthreads();
  }
  // ---- partial lists out (an empty list leaves its pairs the sentinels)
  for (int i = tid; i < pn * K; i += 256) {
    const int row = i / K, j = i % K;
    const int64_t o = (int64_t)Pj[row] * K + j;
    a.part_score[o] = Ls[row * KMAX + j];
    a.part_id[o] = Li[row * KMAX + j];
  }
}

// p sorted partial lists per query row -> the K best.  One workgroup per row stages the lists in LDS; wave 0 merges, lane s at the
// head of list s.  A slot whose probe id is outside [0, nlist) (a NaN query's) was scanned by nobody and counts as empty.
__global__ __launch_bounds__(256) void ivf_merge_kernel(const float* __restrict__ ps, const int32_t* __restrict__ pi,
                                                        const int64_t* __restrict__ probe, int nlist, int p, int K, int metric,
                                                        const float* __restrict__ q, int64_t ldq, float* __restrict__ out_d,
                                                        int64_t* __restrict__ out_i) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Cs = (float*)smem;              // [p][K]
  int* Cid = (int*)(Cs + p * K);         // [p][K]
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x;
  const int total = p * K;
  for (int i = threadIdx.x; i < total; i += 256) {
    const int64_t l = probe[(int64_t)row * p + i / K];
    const bool live = l >= 0 && l < nlist;
    Cs[i] = live ? ps[(int64_t)row * total + i] : -INFINITY;
    Cid[i] = live ? pi[(int64_t)row * total + i] : NONE_ID;
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  float qn = 0.f;
  if (metric == M_L2) qn = query_sqnorm(q, ldq, row, DIM, lane);
  int head = 0;
  for (int k = 0; k < K; ++k) {
    float hs = -INFINITY; int hi = NONE_ID;
    if (lane < p && head < K) { hs = Cs[lane * K + head]; hi = Cid[lane * K + head]; }
    float bs = hs; int bi = hi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float os = __shfl_xor(bs, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (better(os, oi, bs, bi)) { bs = os; bi = oi; }
    }
    if (hi == bi && bi != NONE_ID) ++head;              // ids are unique across the lists
    if (lane == 0) {
      out_d[(int64_t)row * K + k] = metric == M_L2 ? fmaxf(qn - bs, 0.f) : bs;  // L2: |q|^2 - (2 q.t - |t|^2)
      out_i[(int64_t)row * K + k] = bi == NONE_ID ? -1 : bi;
    }
  }
}

// the scan's work list is at most this long: a group per non-empty list and one more per 64 further pairs
inline int64_t ivf_max_groups(int64_t pairs, int nlist) { return std::min<int64_t>(nlist, pairs) + pairs / QT; }

struct IvfSearchWs {
  ScatterIndex idx;
  int* gcount; int* gstart; int2* work;
  float* part_score; int32_t* part_id;
};
inline int64_t ivf_search_bytes(int64_t B, int p, int nlist, int k) {
  const int64_t pairs = B * p;
  return scatter_index_bytes(pairs, nlist) + scatter_index_round(4LL * nlist) + scatter_index_round(4LL * (nlist + 1)) +
         scatter_index_round(8LL * ivf_max_groups(pairs, nlist)) + 2 * scatter_index_round(4LL * pairs * k);
}
inline IvfSearchWs ivf_search_carve(void* workspace, int64_t B, int p, int nlist, int k) {
  char* ptr = (char*)workspace;
  const int64_t pairs = B * p;
  auto take = [&](int64_t bytes) { char* r = ptr; ptr += scatter_index_round(bytes); return r; };
  IvfSearchWs w;
  w.idx = scatter_index_carve(ptr, pairs, nlist);
  w.gcount = (int*)take(4LL * nlist);
  w.gstart = (int*)take(4LL * (nlist + 1));
  w.work = (int2*)take(8LL * ivf_max_groups(pairs, nlist));
  w.part_score = (float*)take(4LL * pairs * k);
  w.part_id = (int32_t*)take(4LL * pairs * k);
  return w;
}

template <bool EXCL>
int ivf_scan_launch(std::conditional_t<EXCL, IvfScanArgsX, IvfScanArgs>& a, int groups, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    RECNN_HIP(hipFuncSetAttribute((const void*)ivf_scan_kernel<EXCL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)IvfLds::bytes));
    attr = true;
  }
  hipLaunchKernelGGL(ivf_scan_kernel<EXCL>, dim3(groups), dim3(256), IvfLds::bytes, st, a);
  return 0;
}
}  // namespace

extern "C" int recnn_ivf_lists_workspace_bytes(int n_items, int nlist, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes, "ivf_lists_workspace_bytes: null pointer");
  RECNN_REQUIRE(n_items > 0 && nlist >= 1 && nlist <= n_items, "ivf_lists_workspace_bytes: need 1 <= nlist <= n_items (got nlist %d, n_items %d)",
                nlist, n_items);
  *h_bytes = ivf_lists_bytes(n_items, nlist);
  return 0;
}

extern "C" int recnn_ivf_build_lists(const int64_t* assign, int n_items, int nlist, int32_t* out_assignment, int32_t* list_start,
                                     int32_t* list_ids, void* workspace, void* stream) {
  RECNN_REQUIRE(assign && out_assignment && list_start && list_ids && workspace, "ivf_build_lists: null pointer");
  RECNN_REQUIRE(n_items > 0 && nlist >= 1 && nlist <= n_items, "ivf_build_lists: need 1 <= nlist <= n_items (got nlist %d, n_items %d)", nlist,
                n_items);
  hipStream_t st = (hipStream_t)stream;
  char* ptr = (char*)workspace;
  auto take = [&](int64_t bytes) { char* r = ptr; ptr += scatter_index_round(bytes); return r; };
  ScatterIndex w;
  w.count = (int*)take(4LL * nlist);
  w.slot = (int*)take(4LL * n_items);
  w.placed = (int*)take(4LL * n_items);
  w.start = list_start;
  w.sorted = list_ids;
  hipLaunchKernelGGL(ivf_narrow_kernel, dim3((n_items + 255) / 256), dim3(256), 0, st, assign, n_items, nlist, out_assignment);
  RECNN_HIP(scatter_index_build(w, IdOfI64{assign}, n_items, nlist, st));
  return recnn_check_hip(hipGetLastError(), "ivf_build_lists");
}

extern "C" int recnn_ivf_update_centroids(const float* table, int n_items, const int32_t* list_start, const int32_t* list_ids, int nlist,
                                          float* centroids, void* stream) {
  RECNN_REQUIRE(table && list_start && list_ids && centroids, "ivf_update_centroids: null pointer");
  RECNN_REQUIRE(n_items > 0 && nlist >= 1 && nlist <= n_items, "ivf_update_centroids: need 1 <= nlist <= n_items (got nlist %d, n_items %d)",
                nlist, n_items);
  RECNN_REQUIRE(aligned16(table, centroids), "ivf_update_centroids: 16-byte alignment");
  hipLaunchKernelGGL(ivf_update_kernel, dim3(nlist), dim3(256), 0, (hipStream_t)stream, table, n_items, list_start, list_ids, centroids);
  return recnn_check_hip(hipGetLastError(), "ivf_update_centroids");
}

extern "C" int recnn_ivf_gather_rows(const float* table, int n_items, const int32_t* list_ids, float* out_rows, void* stream) {
  RECNN_REQUIRE(table && list_ids && out_rows, "ivf_gather_rows: null pointer");
  RECNN_REQUIRE(n_items > 0, "ivf_gather_rows: need n_items > 0");
  RECNN_REQUIRE(aligned16(table, out_rows), "ivf_gather_rows: 16-byte alignment");
  const int64_t chunks = (int64_t)n_items * (DIM / 4);
  hipLaunchKernelGGL(ivf_gather_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, table, n_items, list_ids,
                     n_items, out_rows);
  return recnn_check_hip(hipGetLastError(), "ivf_gather_rows");
}

extern "C" int recnn_ivf_search_workspace_bytes(int n_queries, int nprobe, int nlist, int k, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes, "ivf_search_workspace_bytes: null pointer");
  RECNN_REQUIRE(n_queries >= 0, "ivf_search_workspace_bytes: n_queries must not be negative (got %d)", n_queries);
  RECNN_REQUIRE(nlist >= 1 && nprobe >= 1 && nprobe <= IVF_MAX_PROBE && nprobe <= nlist,
                "ivf_search_workspace_bytes: need 1 <= nprobe <= min(64, nlist) (got nprobe %d, nlist %d)", nprobe, nlist);
  RECNN_REQUIRE(k >= 1 && k <= KMAX, "ivf_search_workspace_bytes: need 1 <= k <= 64 (got %d)", k);
  RECNN_REQUIRE((int64_t)n_queries * nprobe < (1LL << 31) / KMAX, "ivf_search_workspace_bytes: n_queries * nprobe must stay below 2^25 (got %lld)",
                (long long)n_queries * nprobe);
  *h_bytes = ivf_search_bytes(n_queries, nprobe, nlist, k);
  return 0;
}

// The items of the probed lists scored against their queries, the k best per query.  probe: int64 [n_queries][nprobe], the list ids
// a flat search over the centroids reported (distinct within a row; an id outside [0, nlist) is an empty slot).  mask (may be NULL):
// the exclusion bits of seen.h over item ids, words_per_row words per query row.
extern "C" int recnn_ivf_scan(const float* queries, int64_t ld_q, int n_queries, const float* list_rows, const float* list_aux,
                              const int32_t* list_start, const int32_t* list_ids, int nlist, int n_items, int metric,
                              const int64_t* probe, int nprobe, int k, float* out_dist, int64_t* out_ids, void* workspace,
                              void* stream, const uint64_t* mask, int64_t words_per_row) {
  const char* fn = "ivf_scan";
  RECNN_REQUIRE(list_rows && list_start && list_ids, "%s: null pointer", fn);
  RECNN_REQUIRE((queries && probe && out_dist && out_ids && workspace) || n_queries == 0, "%s: null pointer", fn);
  RECNN_REQUIRE(n_queries >= 0 && n_items > 0 && nlist >= 1 && nlist <= n_items, "%s: need n_queries >= 0 and 1 <= nlist <= n_items", fn);
  RECNN_REQUIRE(nprobe >= 1 && nprobe <= IVF_MAX_PROBE && nprobe <= nlist, "%s: need 1 <= nprobe <= min(64, nlist) (got %d)", fn, nprobe);
  RECNN_REQUIRE(k >= 1 && k <= KMAX, "%s: need 1 <= k <= 64 (got %d)", fn, k);
  RECNN_REQUIRE(metric == M_IP || (metric == M_L2 && list_aux), "%s: metric must be IP, or L2 with the |t|^2 array", fn);
  RECNN_REQUIRE(aligned16(queries, list_rows) && ld_q % 4 == 0 && ld_q >= DIM, "%s: 16-byte alignment (rows and ld_q)", fn);
  RECNN_REQUIRE((int64_t)n_queries * nprobe < (1LL << 31) / KMAX, "%s: n_queries * nprobe must stay below 2^25", fn);
  if (mask) {
    if (int rc = seen_check(fn, mask, words_per_row, n_queries, n_items)) return rc;
  }
  if (n_queries == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int pairs = n_queries * nprobe;
  const IvfSearchWs w = ivf_search_carve(workspace, n_queries, nprobe, nlist, k);
  const int groups = (int)ivf_max_groups(pairs, nlist);
  // the pairs by list, then the work list: (list, group of 64 pairs)
  RECNN_HIP(scatter_index_build(w.idx, IdOfI64{probe}, pairs, nlist, st));
  hipLaunchKernelGGL(ivf_group_count_kernel, dim3((nlist + 255) / 256), dim3(256), 0, st, w.idx.start, nlist, w.gcount);
  hipLaunchKernelGGL(scatter_scan_kernel, dim3(1), dim3(1024), 0, st, w.gcount, nlist, w.gstart);
  hipLaunchKernelGGL(ivf_group_fill_kernel, dim3((nlist + 255) / 256), dim3(256), 0, st, w.gstart, nlist, groups, w.work);
  IvfScanArgsX a;
  a.q = queries; a.ldq = ld_q; a.rows = list_rows; a.aux = list_aux; a.list_start = list_start; a.list_ids = list_ids;
  a.pair_start = w.idx.start; a.pair_sorted = w.idx.sorted; a.gstart = w.gstart; a.work = w.work;
  a.nlist = nlist; a.p = nprobe; a.metric = metric; a.K = k; a.part_score = w.part_score; a.part_id = w.part_id;
  a.mask = mask; a.W = words_per_row;
  if (mask) {
    if (int rc = ivf_scan_launch<true>(a, groups, st)) return rc;
  } else {
    IvfScanArgs& plain = a;
    if (int rc = ivf_scan_launch<false>(plain, groups, st)) return rc;
  }
  hipLaunchKernelGGL(ivf_merge_kernel, dim3(n_queries), dim3(256), (size_t)nprobe * k * 8, st, w.part_score, w.part_id, probe, nlist, nprobe,
                     k, metric, queries, ld_q, out_dist, out_ids);
  return recnn_check_hip(hipGetLastError(), fn);
}
