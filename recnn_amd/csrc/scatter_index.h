// scatter_index.h -- the inverted index of the deterministic scatter-sums (dqn.hip: gradients of gathered embedding rows; seq_grad.h:
// the table gradient of the LSTM encoder).  M contributions j = 0 .. M - 1, each with a destination id id_of(j); the index lists, per
// destination, its contributions in ascending j: a stable counting sort (histogram, scan, placement, per-destination rank by j).
// Integers only -- integer atomics for the counts, whose arrival order the rank pass removes again -- so the index, and with it the
// order of every float sum taken over it, is a function of the ids alone.  The float passes over the index stay with their callers
// (their row widths and weights differ).  Ids outside [0, n_dest) are dropped: they are in no list.
//
// id_of is a functor `int64_t operator()(int j) const` (device), passed by value: dqn reads an int64 matrix, seq_grad.h an int32 history
// through the replay store.
#pragma once
#include "common.h"

namespace {

struct ScatterIndex {
  int* count;     // [n_dest]
  int* start;     // [n_dest + 1]: list of destination d = sorted[start[d] .. start[d + 1])
  int* slot;      // [M] arrival slot of contribution j in its list (unordered)
  int* placed;    // [M] contributions by destination, arrival order
  int* sorted;    // [M] ... in contribution order (the inverted index)
};

template <class IdOf>
__global__ void scatter_hist_kernel(const IdOf id_of, int M, int n_dest, int* count, int* slot) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= M) return;
  const int64_t id = id_of(j);
  slot[j] = (id >= 0 && id < n_dest) ? atomicAdd(count + id, 1) : -1;
}
// exclusive scan of count into start[0 .. n + 1): one workgroup of 1024, each thread a contiguous run
__global__ __launch_bounds__(1024) void scatter_scan_kernel(const int* __restrict__ count, int n, int* __restrict__ start) {
  __shared__ int sums[1024];
  const int per = (n + 1023) / 1024;
  const int i0 = threadIdx.x * per, i1 = min(n, i0 + per);
  int s = 0;
  for (int i = i0; i < i1; ++i) s += count[i];
  sums[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = threadIdx.x >= off ? sums[threadIdx.x - off] : 0;
    __syncthreads();
    sums[threadIdx.x] += v;
    __syncthreads();
  }
  int run = sums[threadIdx.x] - s;
  for (int i = i0; i < i1; ++i) {
    start[i] = run;
    run += count[i];
  }
  if (threadIdx.x == 1023) start[n] = sums[1023];
}
// The same scan for a large n, where one workgroup's bandwidth is the whole cost: chunks of SCAN_CHUNK counts, their sums, the scan above
// over those sums, then every chunk scanned from its offset.  Integer sums: the result is the single-workgroup scan's, bit for bit.
constexpr int SCAN_CHUNK = 4096;
inline int scatter_scan_chunks(int n) { return (n + SCAN_CHUNK - 1) / SCAN_CHUNK; }
__global__ __launch_bounds__(256) void scatter_chunk_sum_kernel(const int* __restrict__ count, int n, int* __restrict__ csum) {
  __shared__ int part[256];
  const int t = threadIdx.x, i0 = blockIdx.x * SCAN_CHUNK, i1 = min(n, i0 + SCAN_CHUNK);
  int s = 0;
  for (int i = i0 + t; i < i1; i += 256) s += count[i];
  part[t] = s;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (t < off) part[t] += part[t + off];
    __syncthreads();
  }
  if (t == 0) csum[blockIdx.x] = part[0];
}
// thread t of chunk b owns counts b SCAN_CHUNK + 16 t .. + 15; coff[b] is the chunk's offset, coff[n_chunks] the total
__global__ __launch_bounds__(256) void scatter_chunk_scan_kernel(const int* __restrict__ count, int n, const int* __restrict__ coff,
                                                                 int n_chunks, int* __restrict__ start) {
  __shared__ int sums[256];
  constexpr int PER = SCAN_CHUNK / 256;
  const int t = threadIdx.x, i0 = min(n, blockIdx.x * SCAN_CHUNK + t * PER), i1 = min(n, i0 + PER);
  int s = 0;
  for (int i = i0; i < i1; ++i) s += count[i];
  sums[t] = s;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int v = t >= off ? sums[t - off] : 0;
    __syncthreads();
    sums[t] += v;
    __syncthreads();
  }
  int run = coff[blockIdx.x] + sums[t] - s;
  for (int i = i0; i < i1; ++i) {
    start[i] = run;
    run += count[i];
  }
  if (blockIdx.x == n_chunks - 1 && t == 255) start[n] = coff[n_chunks];
}
template <class IdOf>
__global__ void scatter_place_kernel(const IdOf id_of, int M, const int* __restrict__ start, const int* __restrict__ slot,
                                     int* __restrict__ placed) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= M || slot[j] < 0) return;
  placed[start[(int)id_of(j)] + slot[j]] = j;
}
// stable order: each destination's list sorted by contribution index j (all distinct, < M).  One workgroup per destination with two
// or more entries.  Lists of up to 256 entries: in LDS, rank = number of smaller j in the list.  Longer lists (the popular items): a
// bitmap of the list's j over [0, M) in LDS, rank = popcount below j -- linear in M / 32 + L instead of quadratic in L.  (M beyond the
// bitmap: the quadratic count over LDS chunks.)
//
// Which destination a workgroup takes is a functor `int operator()(int block) const` (-1: none).  BlockIsDest: workgroup d takes
// destination d, a grid of n_dest.  FirstOfList: workgroup j takes the destination of contribution j if j arrived first in its list, a
// grid of M -- for few contributions into many destinations (sampled.hip: a few thousand ids into a catalogue of a million), where a
// workgroup per destination would be nearly all empty launches.  The sorted lists are the same either way.
constexpr int RANK_SMALL = 256, RANK_WORDS = 16384;
struct BlockIsDest {
  __device__ int operator()(int block) const { return block; }
};
template <class IdOf>
struct FirstOfList {
  IdOf id_of;
  const int* slot;
  __device__ int operator()(int block) const { return slot[block] == 0 ? (int)id_of(block) : -1; }
};
template <class DestOf>
__global__ __launch_bounds__(256) void scatter_rank_kernel(const DestOf dest_of, const int* __restrict__ start, int n_dest,
                                                           const int* __restrict__ placed, int M, int* __restrict__ sorted) {
  __shared__ uint32_t bits[RANK_WORDS];
  __shared__ int tsum[256];
  const int d = dest_of(blockIdx.x), t = threadIdx.x;
  if (d < 0 || d >= n_dest) return;
  const int s = start[d], L = start[d + 1] - s;
  if (L <= 1) {
    if (L == 1 && t == 0) sorted[s] = placed[s];
    return;
  }
  int* lst = (int*)bits;
  const int words = (M + 31) / 32;
  if (L > RANK_SMALL && words <= RANK_WORDS) {
    for (int w = t; w < words; w += 256) bits[w] = 0u;
    __syncthreads();
    for (int i = t; i < L; i += 256) {
      const int j = placed[s + i];
      atomicOr(&bits[j >> 5], 1u << (j & 31));
    }
    __syncthreads();
    const int per = (words + 255) / 256, w0 = t * per, w1 = min(words, w0 + per);
    int c = 0;
    for (int w = w0; w < w1; ++w) c += __popc(bits[w]);
    tsum[t] = c;
    __syncthreads();
    if (t == 0) {
      int run = 0;
      for (int k = 0; k < 256; ++k) { const int v = tsum[k]; tsum[k] = run; run += v; }
    }
    __syncthreads();
    for (int i = t; i < L; i += 256) {
      const int j = placed[s + i], w = j >> 5, owner = w / per;
      int r = tsum[owner];
      for (int k = owner * per; k < w; ++k) r += __popc(bits[k]);
      r += __popc(bits[w] & ((1u << (j & 31)) - 1u));
      sorted[s + r] = j;
    }
    return;
  }
  for (int g0 = 0; g0 < L; g0 += 256) {
    const int i = g0 + t;
    const int mine = i < L ? placed[s + i] : 0x7FFFFFFF;
    int rank = 0;
    for (int c0 = 0; c0 < L; c0 += RANK_WORDS) {
      const int n = min(RANK_WORDS, L - c0);
      __syncthreads();
      for (int k = t; k < n; k += 256) lst[k] = placed[s + c0 + k];
      __syncthreads();
      for (int k = 0; k < n; ++k) rank += lst[k] < mine;
    }
    if (i < L) sorted[s + rank] = mine;
  }
}

// the index's share of a workspace: five int arrays, each rounded up to 256 bytes
inline int64_t scatter_index_round(int64_t bytes) { return (bytes + 255) / 256 * 256; }
inline int64_t scatter_index_bytes(int64_t M, int n_dest) {
  return scatter_index_round(4LL * n_dest) + scatter_index_round(4LL * (n_dest + 1)) + 3 * scatter_index_round(4LL * M);
}
// carves the index out of `p` and moves `p` past it
inline ScatterIndex scatter_index_carve(char*& p, int64_t M, int n_dest) {
  auto take = [&](int64_t bytes) { char* r = p; p += scatter_index_round(bytes); return r; };
  ScatterIndex w;
  w.count = (int*)take(4LL * n_dest);
  w.start = (int*)take(4LL * (n_dest + 1));
  w.slot = (int*)take(4LL * M);
  w.placed = (int*)take(4LL * M);
  w.sorted = (int*)take(4LL * M);
  return w;
}
// the launches of one index build, in stream order: clear the counts, histogram, scan, placement, rank.  M == 0: every list is empty
// (start is all zeros).  The pieces of the callers' float passes cover the first start[n_dest] sorted entries.
// rank_by_contribution: the rank pass runs a workgroup per contribution (FirstOfList) instead of one per destination.
// scan_scratch: 2 scatter_scan_chunks(n_dest) + 1 ints (scatter_scan_scratch_bytes); when given, n_dest > SCAN_CHUNK is scanned in chunks.
inline int64_t scatter_scan_scratch_bytes(int n_dest) { return (4LL * (2 * scatter_scan_chunks(n_dest) + 1) + 255) / 256 * 256; }
template <class IdOf>
inline hipError_t scatter_index_build(const ScatterIndex& w, const IdOf& id_of, int M, int n_dest, hipStream_t s,
                                      bool rank_by_contribution = false, int* scan_scratch = nullptr) {
  const hipError_t e = hipMemsetAsync(w.count, 0, 4LL * n_dest, s);
  if (e != hipSuccess) return e;
  if (M) hipLaunchKernelGGL((scatter_hist_kernel<IdOf>), dim3((M + 255) / 256), dim3(256), 0, s, id_of, M, n_dest, w.count, w.slot);
  if (scan_scratch && n_dest > SCAN_CHUNK) {
    const int nc = scatter_scan_chunks(n_dest);
    int* csum = scan_scratch;
    int* coff = scan_scratch + nc;
    hipLaunchKernelGGL(scatter_chunk_sum_kernel, dim3(nc), dim3(256), 0, s, (const int*)w.count, n_dest, csum);
    hipLaunchKernelGGL(scatter_scan_kernel, dim3(1), dim3(1024), 0, s, (const int*)csum, nc, coff);
    hipLaunchKernelGGL(scatter_chunk_scan_kernel, dim3(nc), dim3(256), 0, s, (const int*)w.count, n_dest, (const int*)coff, nc, w.start);
  } else {
    hipLaunchKernelGGL(scatter_scan_kernel, dim3(1), dim3(1024), 0, s, w.count, n_dest, w.start);
  }
  if (M) {
    hipLaunchKernelGGL((scatter_place_kernel<IdOf>), dim3((M + 255) / 256), dim3(256), 0, s, id_of, M, w.start, w.slot, w.placed);
    if (rank_by_contribution)
      hipLaunchKernelGGL((scatter_rank_kernel<FirstOfList<IdOf>>), dim3(M), dim3(256), 0, s, FirstOfList<IdOf>{id_of, w.slot}, w.start,
                         n_dest, w.placed, M, w.sorted);
    else
      hipLaunchKernelGGL((scatter_rank_kernel<BlockIsDest>), dim3(n_dest), dim3(256), 0, s, BlockIsDest{}, w.start, n_dest, w.placed, M,
                         w.sorted);
  }
  return hipSuccess;
}

}  // namespace
