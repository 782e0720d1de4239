// evalrank.hip -- ranking metrics of a batch of target ranks, accumulated on the GPU (gfx950).
//
// A rank is what recnn_dist_target_rank / recnn_topk_target_rank report: how many items come before the item the user took next, in the
// order the generated action induces over the catalogue.  With one relevant item per row the usual offline metrics are functions of
// that rank alone; one pass over ranks int32[n] (and an optional byte mask: a zero byte skips the row) adds, per cutoff K,
//   hits[K] += #{0 <= rank < K}                  (hit rate @K = hits / rows)
//   ndcg[K] += sum over those rows of 1 / log2(rank + 2)       (NDCG@K: IDCG = 1)
// and overall  mrr += sum 1 / (rank + 1),  rank_sum += sum rank,  rows += rows counted,  invalid += unmasked rows with rank < 0
// (a target id outside the table; they count in nothing else).  Up to 8 cutoffs, ascending, of any size.  DESIGN.md section 20.
//
// Integer quantities are exact.  The float64 sums have one order that depends on n alone: thread t of a workgroup adds rows t, t + 256,
// ... of the workgroup's PER rows, a fixed LDS tree adds the threads, and a second one-workgroup launch adds the workgroups' partials
// in workgroup order (thread t takes t, t + 256, ...; then the tree) into the caller's accumulators.  No floating-point atomics: equal
// call sequences give equal bits.
#include "common.h"

namespace {
constexpr int TPB = 256;
constexpr int PER = 4 * TPB;   // rows per workgroup
constexpr int MAXK = 8;
constexpr int NF = MAXK + 1;   // float64 slots: ndcg[0..8), mrr
constexpr int NI = MAXK + 3;   // int64 slots: hits[0..8), rank_sum, rows, invalid

struct Cutoffs { int n; int32_t k[MAXK]; };

template <class T> __device__ inline T block_tree(T v, T* s, int tid) {   // fixed tree over TPB values; every thread gets the total
  s[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = TPB / 2; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  const T r = s[0];
  __syncthreads();
  return r;
}

// part_f: [NF][nwg], part_i: [NI][nwg]
__global__ __launch_bounds__(TPB) void rank_metrics_kernel(const int32_t* __restrict__ ranks, const uint8_t* __restrict__ mask, int n,
                                                           const Cutoffs ks, double* __restrict__ part_f, int64_t* __restrict__ part_i) {
  __shared__ double red_f[TPB];
  __shared__ int64_t red_i[TPB];
  const int tid = threadIdx.x;
  double f[NF];
  int64_t c[NI];
#pragma unroll
  for (int j = 0; j < NF; ++j) f[j] = 0.0;
#pragma unroll
  for (int j = 0; j < NI; ++j) c[j] = 0;
  const int64_t base = (int64_t)blockIdx.x * PER;
  for (int j = 0; j < PER / TPB; ++j) {
    const int64_t i = base + tid + j * TPB;
    if (i >= n || (mask && !mask[i])) continue;
    const int r = ranks[i];
    if (r < 0) { ++c[MAXK + 2]; continue; }
    const double gain = 1.0 / log2((double)r + 2.0);
#pragma unroll
    for (int q = 0; q < MAXK; ++q)
      if (q < ks.n && r < ks.k[q]) { ++c[q]; f[q] += gain; }
    f[MAXK] += 1.0 / ((double)r + 1.0);
    c[MAXK] += r;
    ++c[MAXK + 1];
  }
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const double t = block_tree(f[j], red_f, tid);
    if (tid == 0) part_f[(int64_t)j * gridDim.x + blockIdx.x] = t;
  }
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int64_t t = block_tree(c[j], red_i, tid);
    if (tid == 0) part_i[(int64_t)j * gridDim.x + blockIdx.x] = t;
  }
}

// one workgroup: the partials in workgroup order, added into the accumulators acc_f [n_ks + 1], acc_i [n_ks + 3]
__global__ __launch_bounds__(TPB) void rank_metrics_finish_kernel(const double* __restrict__ part_f, const int64_t* __restrict__ part_i,
                                                                  int nwg, int n_ks, double* __restrict__ acc_f,
                                                                  int64_t* __restrict__ acc_i) {
  __shared__ double red_f[TPB];
  __shared__ int64_t red_i[TPB];
  const int tid = threadIdx.x;
  for (int j = 0; j < NF; ++j) {
    double s = 0.0;
    for (int i = tid; i < nwg; i += TPB) s += part_f[(int64_t)j * nwg + i];
    s = block_tree(s, red_f, tid);
    if (tid == 0) {
      if (j < n_ks) acc_f[j] += s;
      else if (j == MAXK) acc_f[n_ks] += s;
    }
  }
  for (int j = 0; j < NI; ++j) {
    int64_t s = 0;
    for (int i = tid; i < nwg; i += TPB) s += part_i[(int64_t)j * nwg + i];
    s = block_tree(s, red_i, tid);
    if (tid == 0) {
      if (j < n_ks) acc_i[j] += s;
      else if (j >= MAXK) acc_i[n_ks + (j - MAXK)] += s;
    }
  }
}

inline int metrics_workgroups(int n) { return (n + PER - 1) / PER; }
}  // namespace

extern "C" int recnn_rank_metrics_workspace_bytes(int n, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes && n >= 0, "rank_metrics_workspace_bytes: bad arguments");
  *h_bytes = (int64_t)metrics_workgroups(n) * (NF + NI) * 8;
  return 0;
}

extern "C" int recnn_rank_metrics(const int32_t* ranks, const uint8_t* mask, int n, const int32_t* h_ks, int n_ks, double* acc_f,
                                  int64_t* acc_i, void* workspace, void* stream) {
  RECNN_REQUIRE(h_ks && acc_f && acc_i && ((ranks && workspace) || n == 0), "rank_metrics: null pointer");
  RECNN_REQUIRE(n >= 0, "rank_metrics: need n >= 0");
  RECNN_REQUIRE(n_ks >= 1 && n_ks <= MAXK, "rank_metrics: need 1 to 8 cutoffs (got %d)", n_ks);
  Cutoffs ks{};
  ks.n = n_ks;
  for (int i = 0; i < n_ks; ++i) {
    RECNN_REQUIRE(h_ks[i] >= 1 && (i == 0 || h_ks[i] > h_ks[i - 1]), "rank_metrics: cutoffs must be >= 1 and strictly ascending");
    ks.k[i] = h_ks[i];
  }
  RECNN_REQUIRE(((uintptr_t)workspace & 7) == 0 && (((uintptr_t)acc_f | (uintptr_t)acc_i) & 7) == 0, "rank_metrics: 8-byte alignment");
  if (n == 0) return 0;
  const int nwg = metrics_workgroups(n);
  double* part_f = (double*)workspace;
  int64_t* part_i = (int64_t*)(part_f + (int64_t)NF * nwg);
  hipLaunchKernelGGL(rank_metrics_kernel, dim3(nwg), dim3(TPB), 0, (hipStream_t)stream, ranks, mask, n, ks, part_f, part_i);
  hipLaunchKernelGGL(rank_metrics_finish_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, (const double*)part_f,
                     (const int64_t*)part_i, nwg, n_ks, acc_f, acc_i);
  return recnn_check_hip(hipGetLastError(), "rank_metrics");
}
