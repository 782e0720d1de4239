// seen.h -- the per-row exclusion mask of the streaming search / rank kernels (seen.hip builds it).
//
// mask: uint64 [rows][W], W = ceil(n_items / 64).  Bit (i & 63) of word (i >> 6) of row b is set when item i does not exist for
// query row b; the bits of the last word above n_items are zero.  Every kernel that takes a mask walks the table in blocks of 64
// consecutive items that start at a multiple of 64, so the 64 bits of a (row, block) are one aligned word.
#pragma once
#include "common.h"

namespace {
constexpr int SEEN_MAX_ITEMS = 1 << 20;   // one row's words are built in one workgroup's LDS: 2^20 bits = 128 KiB of the CU's 160

inline int64_t seen_words(int n_items) { return ((int64_t)n_items + 63) / 64; }

// the word of row `row` that holds item n0's bit (n0 < n_items)
__device__ __forceinline__ uint64_t seen_word(const uint64_t* __restrict__ mask, int64_t W, int row, int n0) {
  return mask[(int64_t)row * W + (n0 >> 6)];
}

// argument checks of the excluding entry points (before any HIP call)
inline int seen_check(const char* fn, const void* mask, int64_t words_per_row, int n_queries, int n_items) {
  RECNN_REQUIRE(n_items <= SEEN_MAX_ITEMS, "%s: an exclusion mask covers at most %d items (got %d)", fn, SEEN_MAX_ITEMS, n_items);
  RECNN_REQUIRE(words_per_row == seen_words(n_items), "%s: the mask has %lld words per row, %d items need %lld", fn,
                (long long)words_per_row, n_items, (long long)seen_words(n_items));
  RECNN_REQUIRE((mask || n_queries == 0) && ((uintptr_t)mask & 7) == 0, "%s: null or misaligned exclusion mask", fn);
  return 0;
}
}  // namespace
