// seen.hip -- builds the per-row exclusion mask of seen.h from per-row slices of one id array (gfx950).
//
// The usual offline protocol ranks the held-out item against the catalogue WITHOUT what the user has already consumed, and a served
// top-K should not repeat the window it was computed from.  "What row b has consumed" is a slice ids[starts[b] : starts[b] +
// lengths[b]] of an array that is already on the GPU (the replay store's `items`), so the mask is built from (start, length) pairs
// and no id is copied.  DESIGN.md section 21.
//
// One workgroup per row.  The row's words live in LDS: zeroed, filled with LDS integer atomicOr (a set of bits: the result does not
// depend on the order or on duplicates), the optional `keep` bit cleared after a barrier, and written out once with plain vector
// stores -- no global atomics, no memset.  Ids outside [0, n_items) and positions outside [0, n_ids) are ignored; nothing is read
// out of bounds whatever starts / lengths hold.
#include "seen.h"

namespace {
__global__ __launch_bounds__(256) void seen_mask_kernel(const int32_t* __restrict__ ids, int64_t n_ids,
                                                        const int64_t* __restrict__ starts, const int64_t* __restrict__ lengths,
                                                        const int64_t* __restrict__ keep, int n_items, int64_t W,
                                                        uint64_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* w32 = (uint32_t*)smem;              // [2 W]: little-endian halves of the row's 64-bit words
  const int tid = threadIdx.x, b = blockIdx.x;
  const int n32 = (int)(2 * W);
  for (int i = tid; i < n32; i += 256) w32[i] = 0u;
  // the row's positions, clipped to [0, n_ids) without overflow
  const int64_t s = starts[b], len = lengths[b];
  int64_t lo = 0, hi = 0;
  if (len > 0 && s < n_ids) {
    lo = s > 0 ? s : 0;
    if (s < 0) hi = s + len;                    // s < 0 < len: no overflow
    else hi = len > n_ids - s ? n_ids : s + len;
    if (hi > n_ids) hi = n_ids;
  }
  __syncthreads();
  for (int64_t p = lo + tid; p < hi; p += 256) {
    const int32_t id = ids[p];
    if ((uint32_t)id < (uint32_t)n_items) atomicOr(&w32[id >> 5], 1u << (id & 31));
  }
  __syncthreads();
  if (tid == 0 && keep) {
    const int64_t k = keep[b];
    if ((uint64_t)k < (uint64_t)n_items) w32[k >> 5] &= ~(1u << (k & 31));
  }
  __syncthreads();
  const uint2* w64 = (const uint2*)smem;
  uint2* o = (uint2*)(out + (int64_t)b * W);
  for (int i = tid; i < (int)W; i += 256) o[i] = w64[i];
}
}  // namespace

extern "C" int recnn_seen_mask_words(int n_items, int64_t* h_words) {
  RECNN_REQUIRE(h_words && n_items > 0, "seen_mask_words: bad arguments (n_items > 0)");
  RECNN_REQUIRE(n_items <= SEEN_MAX_ITEMS, "seen_mask_words: an exclusion mask covers at most %d items (got %d)", SEEN_MAX_ITEMS,
                n_items);
  *h_words = seen_words(n_items);
  return 0;
}

extern "C" int recnn_seen_mask_build(const int32_t* ids, int64_t n_ids, const int64_t* starts, const int64_t* lengths,
                                     const int64_t* keep, int n_rows, int n_items, uint64_t* out_words, void* stream) {
  RECNN_REQUIRE(n_rows >= 0 && n_items > 0 && n_ids >= 0, "seen_mask_build: need n_rows >= 0, n_items > 0 and n_ids >= 0");
  RECNN_REQUIRE(n_items <= SEEN_MAX_ITEMS, "seen_mask_build: an exclusion mask covers at most %d items (got %d)", SEEN_MAX_ITEMS,
                n_items);
  RECNN_REQUIRE((ids || n_ids == 0) && ((starts && lengths && out_words) || n_rows == 0), "seen_mask_build: null pointer");
  RECNN_REQUIRE((((uintptr_t)out_words | (uintptr_t)starts | (uintptr_t)lengths | (uintptr_t)keep) & 7) == 0 &&
                    ((uintptr_t)ids & 3) == 0, "seen_mask_build: misaligned operand");
  if (n_rows == 0) return 0;
  const int64_t W = seen_words(n_items);
  const size_t lds = (size_t)W * 8;
  static size_t attr = 0;                       // the largest dynamic LDS size asked for so far
  if (lds > attr) {
    RECNN_HIP(hipFuncSetAttribute((const void*)seen_mask_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr = lds;
  }
  hipLaunchKernelGGL(seen_mask_kernel, dim3(n_rows), dim3(256), lds, (hipStream_t)stream, ids, n_ids, starts, lengths, keep, n_items,
                     W, out_words);
  return recnn_check_hip(hipGetLastError(), "seen_mask_kernel");
}
