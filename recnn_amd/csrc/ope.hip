// ope.hip -- off-policy estimators of a logged batch, accumulated on the GPU (section 17 of include/recnn_hip.h).
//
// Per row: lp_pi, lp_beta (the two policies' log-probabilities of the logged action) and the logged reward r, all fp32; an optional
// byte mask (a zero byte skips the row), optional q_logged / v_dm (both or neither) for the doubly robust estimate.  A masked-out row
// counts nowhere; an unmasked row with a NaN log-probability counts in `invalid` and nowhere else.  For every other row, in float64,
//   w = exp(lp_pi - lp_beta);   top_k >= 1:  w *= top_k (1 - exp(lp_pi))^(top_k - 1)  (1 - exp as -expm1; the power by squaring)
//   wc = min(w, cap)
// and the call adds   acc_f: [0] sum w  [1] sum w^2  [2] sum w r  [3] sum wc  [4] sum wc r  [5] sum r  [6] sum v_dm + w (r - q_logged)
//                            [7] max w (a maximum, not a sum)
//                     acc_i: [0] rows  [1] invalid  [2] capped = #{w > cap}
// The float64 sums have one order that depends on n alone, the one of evalrank.hip: thread t of a workgroup adds rows t, t + 256, ...
// of the workgroup's PER rows, a fixed LDS tree adds the threads, a second one-workgroup launch adds the workgroups' partials in
// workgroup order (thread t takes t, t + 256, ...; then the tree) into the caller's accumulators.  A maximum has no order.  No atomics.
#include <math.h>

#include "common.h"

namespace {
constexpr int TPB = 256;
constexpr int PER = 4 * TPB;   // rows per workgroup
constexpr int NS = 7;          // float64 sums
constexpr int NF = NS + 1;     // + max w
constexpr int NI = 3;

template <class T, class Op> __device__ inline T block_tree(T v, T* s, int tid, Op op) {   // fixed tree over TPB values
  s[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = TPB / 2; o > 0; o >>= 1) {
    if (tid < o) s[tid] = op(s[tid], s[tid + o]);
    __syncthreads();
  }
  const T r = s[0];
  __syncthreads();
  return r;
}
struct Add { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };
struct Max { __device__ double operator()(double a, double b) const { return fmax(a, b); } };

__device__ inline double pow_int(double b, int e) {   // b^e, e >= 0, by squaring: a fixed sequence of correctly rounded products
  double r = 1.0;
  while (e) {
    if (e & 1) r *= b;
    b *= b;
    e >>= 1;
  }
  return r;
}

// part_f: [NF][nwg], part_i: [NI][nwg]
__global__ __launch_bounds__(TPB) void ope_kernel(const float* __restrict__ lp_pi, const float* __restrict__ lp_beta,
                                                  const float* __restrict__ reward, const uint8_t* __restrict__ mask,
                                                  const float* __restrict__ q_logged, const float* __restrict__ v_dm, int n, double cap,
                                                  int top_k, double* __restrict__ part_f, int64_t* __restrict__ part_i) {
  __shared__ double red_f[TPB];
  __shared__ int64_t red_i[TPB];
  const int tid = threadIdx.x;
  double f[NS], mx = 0.0;
  int64_t c[NI];
#pragma unroll
  for (int j = 0; j < NS; ++j) f[j] = 0.0;
#pragma unroll
  for (int j = 0; j < NI; ++j) c[j] = 0;
  const int64_t base = (int64_t)blockIdx.x * PER;
  for (int j = 0; j < PER / TPB; ++j) {
    const int64_t i = base + tid + j * TPB;
    if (i >= n || (mask && !mask[i])) continue;
    const double lp = (double)lp_pi[i], lb = (double)lp_beta[i];
    if (lp != lp || lb != lb) { ++c[1]; continue; }
    double w = exp(lp - lb);
    if (top_k >= 1) w *= (double)top_k * pow_int(-expm1(lp), top_k - 1);
    const double wc = fmin(w, cap);
    const double r = (double)reward[i];
    f[0] += w;
    f[1] += w * w;
    f[2] += w * r;
    f[3] += wc;
    f[4] += wc * r;
    f[5] += r;
    if (q_logged) f[6] += (double)v_dm[i] + w * (r - (double)q_logged[i]);
    mx = fmax(mx, w);
    ++c[0];
    if (w > cap) ++c[2];
  }
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const double t = block_tree(f[j], red_f, tid, Add());
    if (tid == 0) part_f[(int64_t)j * gridDim.x + blockIdx.x] = t;
  }
  {
    const double t = block_tree(mx, red_f, tid, Max());
    if (tid == 0) part_f[(int64_t)NS * gridDim.x + blockIdx.x] = t;
  }
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int64_t t = block_tree(c[j], red_i, tid, Add());
    if (tid == 0) part_i[(int64_t)j * gridDim.x + blockIdx.x] = t;
  }
}

// one workgroup: the partials in workgroup order, added into the accumulators acc_f [8], acc_i [3]
__global__ __launch_bounds__(TPB) void ope_finish_kernel(const double* __restrict__ part_f, const int64_t* __restrict__ part_i, int nwg,
                                                         double* __restrict__ acc_f, int64_t* __restrict__ acc_i) {
  __shared__ double red_f[TPB];
  __shared__ int64_t red_i[TPB];
  const int tid = threadIdx.x;
  for (int j = 0; j < NS; ++j) {
    double s = 0.0;
    for (int i = tid; i < nwg; i += TPB) s += part_f[(int64_t)j * nwg + i];
    s = block_tree(s, red_f, tid, Add());
    if (tid == 0) acc_f[j] += s;
  }
  {
    double s = 0.0;
    for (int i = tid; i < nwg; i += TPB) s = fmax(s, part_f[(int64_t)NS * nwg + i]);
    s = block_tree(s, red_f, tid, Max());
    if (tid == 0) acc_f[NS] = fmax(acc_f[NS], s);
  }
  for (int j = 0; j < NI; ++j) {
    int64_t s = 0;
    for (int i = tid; i < nwg; i += TPB) s += part_i[(int64_t)j * nwg + i];
    s = block_tree(s, red_i, tid, Add());
    if (tid == 0) acc_i[j] += s;
  }
}

inline int ope_workgroups(int n) { return (n + PER - 1) / PER; }
}  // namespace

extern "C" int recnn_ope_accumulate_workspace_bytes(int n, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes && n >= 0, "ope_accumulate_workspace_bytes: bad arguments");
  *h_bytes = (int64_t)ope_workgroups(n) * (NF + NI) * 8;
  return 0;
}

extern "C" int recnn_ope_accumulate(const float* lp_pi, const float* lp_beta, const float* reward, const uint8_t* mask,
                                    const float* q_logged, const float* v_dm, int n, double cap, int top_k, double* acc_f,
                                    int64_t* acc_i, void* workspace, void* stream) {
  RECNN_REQUIRE(acc_f && acc_i && ((lp_pi && lp_beta && reward && workspace) || n == 0), "ope_accumulate: null pointer");
  RECNN_REQUIRE(n >= 0, "ope_accumulate: need n >= 0");
  RECNN_REQUIRE((q_logged != nullptr) == (v_dm != nullptr), "ope_accumulate: q_logged and v_dm come together");
  RECNN_REQUIRE(cap == cap && cap > 0.0, "ope_accumulate: cap must be positive (+inf for none)");
  RECNN_REQUIRE(top_k >= 0, "ope_accumulate: top_k must be >= 0 (0 for off)");
  RECNN_REQUIRE(((uintptr_t)workspace & 7) == 0 && (((uintptr_t)acc_f | (uintptr_t)acc_i) & 7) == 0, "ope_accumulate: 8-byte alignment");
  if (n == 0) return 0;
  const int nwg = ope_workgroups(n);
  double* part_f = (double*)workspace;
  int64_t* part_i = (int64_t*)(part_f + (int64_t)NF * nwg);
  hipLaunchKernelGGL(ope_kernel, dim3(nwg), dim3(TPB), 0, (hipStream_t)stream, lp_pi, lp_beta, reward, mask, q_logged, v_dm, n, cap, top_k,
                     part_f, part_i);
  hipLaunchKernelGGL(ope_finish_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, (const double*)part_f, (const int64_t*)part_i, nwg,
                     acc_f, acc_i);
  return recnn_check_hip(hipGetLastError(), "ope_accumulate");
}
