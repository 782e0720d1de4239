// divstats.hip -- what the reference's diversity / distances notebooks compute from a top-K result, on the GPU (gfx950).
//
// examples/[Results]/2. Diversity Test (Indexes).ipynb and 3. Distances Test.ipynb copy the [B, k] ids and distances of a search
// to the host and run np.unique(ids, return_counts=True), D.mean(axis=1).mean() and D.std(axis=1).mean() there.  Here one
// launch streams the result once (12 B k bytes in, 16 B out) and leaves, on the device,
//   counts[id]  += 1 for every id in [0, n_items)            (integer atomics: exact in any order)
//   row_mean[r]  = (sum_i x_ri) / k,   row_std[r] = sqrt(sum_i (x_ri - row_mean[r])^2 / k)     (float64, two passes, index order)
//   totals      += { sum_r row_mean, sum_r row_std, rows, ids out of range }
// with x = (double)dist, or sqrt((double)dist) when take_sqrt (the demo's "l2 -> euclidean").  DESIGN.md section 13.
//
// A workgroup owns ROWS consecutive rows, i.e. one contiguous run of ROWS * k floats and ROWS * k int64: it reads both runs flat,
// 16 bytes per lane, whatever k is (one lane per row would read with stride k).  Distances are parked in LDS at an odd row pitch and
// lane r then walks row r in index order (conflict-free: consecutive rows start in consecutive banks), so a row's two sums have
// one order that depends on k alone.  The ids never touch LDS: each is range-checked and counted as it is read.  The workgroup's
// sums of row_mean / row_std (a fixed LDS tree) go to the workspace; a second one-workgroup launch adds them in workgroup order
// and accumulates into totals.  No floating-point atomics: equal calls give equal bits.
#include "common.h"

namespace {
constexpr int ROWS = 128;   // rows per workgroup == threads per workgroup
constexpr int KMAX = 64;    // topk.hip's limit

__device__ inline double block_sum(double v, double* s, int tid) {   // fixed tree over ROWS values; every thread gets the total
  s[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = ROWS / 2; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();                                                     // s may be reused at once
  return r;
}

__global__ __launch_bounds__(ROWS) void topk_stats_kernel(const float* __restrict__ dist, const int64_t* __restrict__ ids, int B, int k,
                                                          int n_items, int take_sqrt, int32_t* __restrict__ counts,
                                                          double* __restrict__ row_mean, double* __restrict__ row_std,
                                                          double* __restrict__ part) {   // part: [3][gridDim.x]
  extern __shared__ __attribute__((aligned(16))) float xs[];   // [ROWS][pitch]
  __shared__ double red[ROWS];
  __shared__ int bad_s;
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * ROWS;
  const int nrows = min(ROWS, B - row0);
  const int pitch = k | 1;
  const int total = nrows * k;                       // <= 8192
  const int64_t base = (int64_t)row0 * k;            // multiple of 128: the runs below start 16-byte aligned
  if (tid == 0) bad_s = 0;

  // ---- distances -> LDS
  const float* d = dist + base;
  for (int v = tid; v < total / 4; v += ROWS) {
    const float4 f = *(const float4*)(d + 4 * v);
    const float e[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = 4 * v + j, r = idx / k;
      xs[r * pitch + (idx - r * k)] = e[j];
    }
  }
  for (int idx = (total & ~3) + tid; idx < total; idx += ROWS) {
    const int r = idx / k;
    xs[r * pitch + (idx - r * k)] = d[idx];
  }
  // ---- ids -> counts
  const int64_t* p = ids + base;
  int bad = 0;
  for (int v = tid; v < total / 2; v += ROWS) {
    const longlong2 q = *(const longlong2*)(p + 2 * v);
    if ((uint64_t)q.x < (uint64_t)n_items) atomicAdd(&counts[q.x], 1); else ++bad;
    if ((uint64_t)q.y < (uint64_t)n_items) atomicAdd(&counts[q.y], 1); else ++bad;
  }
  if ((total & 1) && tid == 0) {
    const int64_t q = p[total - 1];
    if ((uint64_t)q < (uint64_t)n_items) atomicAdd(&counts[q], 1); else ++bad;
  }
  __syncthreads();
  if (bad) atomicAdd(&bad_s, bad);

  // ---- lane r: row r, two passes in index order
  double mean = 0.0, sd = 0.0;
  if (tid < nrows) {
    const float* x = xs + tid * pitch;
    double s = 0.0;
    for (int i = 0; i < k; ++i) {
      const double v = (double)x[i];
      s += take_sqrt ? sqrt(v) : v;
    }
    mean = s / (double)k;
    double ss = 0.0;
    for (int i = 0; i < k; ++i) {
      const double v = (double)x[i];
      const double c = (take_sqrt ? sqrt(v) : v) - mean;
      ss += c * c;
    }
    sd = sqrt(ss / (double)k);
    row_mean[row0 + tid] = mean;
    row_std[row0 + tid] = sd;
  }
  const double sm = block_sum(mean, red, tid);
  const double ssd = block_sum(sd, red, tid);
  if (tid == 0) {
    part[blockIdx.x] = sm;
    part[gridDim.x + blockIdx.x] = ssd;
    part[2 * gridDim.x + blockIdx.x] = (double)bad_s;
  }
}

// one workgroup: partials in workgroup order (thread t takes t, t + ROWS, ...; then the fixed tree), accumulated into totals
__global__ __launch_bounds__(ROWS) void topk_stats_finish_kernel(const double* __restrict__ part, int nwg, int B, double* __restrict__ totals) {
  __shared__ double red[ROWS];
  const int tid = threadIdx.x;
  double t[3];
  for (int w = 0; w < 3; ++w) {
    double s = 0.0;
    for (int i = tid; i < nwg; i += ROWS) s += part[(int64_t)w * nwg + i];
    t[w] = block_sum(s, red, tid);
  }
  if (tid == 0) {
    totals[0] += t[0];
    totals[1] += t[1];
    totals[2] += (double)B;
    totals[3] += t[2];
  }
}

inline int stats_workgroups(int n_queries) { return (n_queries + ROWS - 1) / ROWS; }
}  // namespace

extern "C" int recnn_topk_stats_workspace_bytes(int n_queries, int k, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes && n_queries >= 0 && k > 0 && k <= KMAX, "topk_stats_workspace_bytes: bad arguments (0 < k <= 64)");
  *h_bytes = (int64_t)stats_workgroups(n_queries) * 3 * (int64_t)sizeof(double);
  return 0;
}

extern "C" int recnn_topk_stats(const float* dist, const int64_t* ids, int n_queries, int k, int n_items, int take_sqrt, int32_t* counts,
                                double* row_mean, double* row_std, double* totals, void* workspace, void* stream) {
  RECNN_REQUIRE(dist && ids && counts && row_mean && row_std && totals && workspace, "topk_stats: null pointer");
  RECNN_REQUIRE(k > 0 && k <= KMAX, "topk_stats: need 0 < k <= 64 (got %d)", k);
  RECNN_REQUIRE(n_items > 0 && n_queries >= 0, "topk_stats: need n_items > 0 and n_queries >= 0");
  RECNN_REQUIRE((((uintptr_t)dist | (uintptr_t)ids) & 15) == 0 && ((uintptr_t)workspace & 7) == 0, "topk_stats: 16-byte alignment");
  if (n_queries == 0) return 0;
  const int nwg = stats_workgroups(n_queries);
  const size_t lds = (size_t)ROWS * (k | 1) * sizeof(float);
  hipLaunchKernelGGL(topk_stats_kernel, dim3(nwg), dim3(ROWS), lds, (hipStream_t)stream, dist, ids, n_queries, k, n_items, take_sqrt,
                     counts, row_mean, row_std, (double*)workspace);
  hipLaunchKernelGGL(topk_stats_finish_kernel, dim3(1), dim3(ROWS), 0, (hipStream_t)stream, (const double*)workspace, nwg, n_queries,
                     totals);
  return recnn_check_hip(hipGetLastError(), "topk_stats");
}
