// flat_walk.h -- the element walk of the flat passes (optimizers, soft update, clip: optim.hip; padded gathers, collect and its backward: seq.hip; the W_hh transpose: seq_bwd.h).
#pragma once
#include <type_traits>

#include "common.h"

// The element walk of every flat pass: body(i, width) once per run of `width` consecutive elements starting at i, each element in exactly
// one run.  VEC = 4: 16 bytes per lane and load over the n >> 2 whole quads (catalogue-sized tensors -- REINFORCE at 100k items -- are
// bound by bytes in flight, not by HBM, with 4-byte lanes), then the n % 4 tail one by one; VEC = 1 (unaligned callers): one by one
// throughout.  The body is written once for both widths (flat_ld / flat_st take the width from their array): element by element the same
// arithmetic.  Floating-point contraction follows the body's own pragma, not this function's.
template <int W> using Width = std::integral_constant<int, W>;
template <int VEC, class Body> __device__ __forceinline__ void flat_walk(int64_t n, Body body) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  int64_t done = 0;
  if constexpr (VEC == 4) {
    const int64_t n4 = n >> 2;
    for (int64_t q = gid; q < n4; q += stride) body(q << 2, Width<4>());
    done = n4 << 2;
  }
  for (int64_t i = done + gid; i < n; i += stride) body(i, Width<1>());
}
template <int W> __device__ __forceinline__ void flat_ld(const float* a, int64_t i, float (&x)[W]) {
  if constexpr (W == 4) {
    const float4 t = *(const float4*)(a + i);
    x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
  } else {
    x[0] = a[i];
  }
}
template <int W> __device__ __forceinline__ void flat_st(float* a, int64_t i, const float (&x)[W]) {
  if constexpr (W == 4) *(float4*)(a + i) = make_float4(x[0], x[1], x[2], x[3]);
  else a[i] = x[0];
}
