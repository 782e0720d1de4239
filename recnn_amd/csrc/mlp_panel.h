// mlp_panel.h -- pieces shared by the fused row-panel kernels (mlps.hip, mlpt.hip, mlpf.hip): the 32 x 256 bf16 activation panel (the
// next layer's A operand), the hidden-layer epilogue that fills it and the panel x weight-slab product (mlps.hip, mlpt.hip).
#pragma once
#include <type_traits>
#include "mlp.h"
#include "lds_stream.h"

namespace {
constexpr int BM = 32;            // rows per workgroup
constexpr int HP = 256;           // hidden width handled
constexpr int PANEL_HALF = BM * 256;          // one k half (128 columns) of the 32 x 256 activation panel
constexpr int KB1 = 64;           // k elements per weight-slab row
constexpr int SLAB_PITCH = 2 * KB1;           // ... = 128 bytes
constexpr int OW = 8;             // waves of the actor's 128-column output layer

// acc += panel(k quarter q: columns 64 q .. 64 q + 63 of the 32 x 256 activation panel; rows of 256 bytes per 128-column half, chunk c
// of row r at c ^ (r & 15)) * W(rows wrow0 + fr, 64 k of a ring slab: rows of SLAB_PITCH bytes, chunk c of row r at c ^ ((r >> 1) & 7))^T.
// Operands swapped: acc[tm][0][r] = C[row 16 tm + fr][column wrow0 + 4 fg + r].  two = false: 16-row panel, only the first row block exists.
__device__ __forceinline__ void mma_panel(const unsigned char* panel, int q, const unsigned char* sb, f32x4 (&acc)[2][1], int wrow0, int fr, int fg,
                                          const bool two) {
  const int sw = (fr >> 1) & 7;
  const unsigned char* sa = panel + (q >> 1) * PANEL_HALF;
#pragma unroll
  for (int ks = 0; ks < KB1 / 32; ++ks) {
    const int posa = ((((q & 1) * 8) + ks * 4 + fg) ^ fr) * 16;
    const int posb = ((ks * 4 + fg) ^ sw) * 16;
    uint4 a[2], b;
    a[0] = *(const uint4*)(sa + fr * 256 + posa);
    if (two) a[1] = *(const uint4*)(sa + (16 + fr) * 256 + posa);
    b = *(const uint4*)(sb + (wrow0 + fr) * SLAB_PITCH + posb);
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, b), __builtin_bit_cast(bf16x8, a[0]), acc[0][0], 0, 0, 0);
    if (two) acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, b), __builtin_bit_cast(bf16x8, a[1]), acc[1][0], 0, 0, 0);
  }
}

// hidden-layer epilogue: bias + relu + dropout -> bf16 into the LDS panel (the next layer's A operand).  Kept lean on purpose
// (in-kernel trace + ISA count: the first version spent 630 instructions per wave here, 80 per element, mostly on per-element
// exec-masked 2-byte global stores and address arithmetic -- 7k ticks per epilogue, a third of the workgroup's time): the
// activations now reach global memory from the finished panel as whole rows (panel_to_global), and the four rows of an
// accumulator register group differ only by r in the swizzled chunk position ((c ^ (rb | r)) = (c ^ rb) ^ r).
template <int TNH>
__device__ __forceinline__ void hidden_epilogue(f32x4 (&acc)[2][TNH], const f32x4 (&bias_v)[TNH], int H, int rows, int m0, int wave, int fr,
                                                int fg, int mask_mode, const uint8_t* mask, int64_t ld_mask, uint32_t key,
                                                unsigned char* panel, uint32_t* gbits = nullptr, const bool two = true) {   // two = false: 16-row panel
  uint32_t bits = 0;
#pragma unroll
  for (int tn = 0; tn < TNH; ++tn) {
    const int n0 = wave * (16 * TNH) + tn * 16 + fg * 4;      // this lane's four columns n0 .. n0 + 3
    // panel image: k half (n / 128), row, chunk ((n % 128) / 8) ^ (row & 15), element n % 8
    unsigned char* col = panel + (n0 >> 7) * PANEL_HALF + (n0 & 7) * 2;
    const int c = (n0 & 127) >> 3;
    // (row blocks as compile-time constants; the second one under a uniform branch: a loop that breaks on the run-time flag would not
    //  be unrolled and its accumulator indexing would turn into select chains)
    auto row_block = [&](auto TMc) {
      constexpr int tm = decltype(TMc)::value;
      const int row = tm * 16 + fr, m = m0 + row;
      uint32_t word = 0;
      if (mask_mode == RECNN_MASK_HASH) word = mask_word(key, (uint32_t)(m >> 2), (uint32_t)(n0 >> 2));
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = fmaxf(acc[tm][tn][r] + bias_v[tn][r], 0.f);
        if (mask_mode == RECNN_MASK_EXTERNAL) v[r] = (m < rows && n0 + r < H && mask[(int64_t)m * ld_mask + n0 + r]) ? v[r] * 2.f : 0.f;
        else if (mask_mode == RECNN_MASK_HASH) v[r] = mask_keep(word, m & 3, r) ? v[r] * 2.f : 0.f;
        if (n0 + r >= H) v[r] = 0.f;
      }
      const uint32_t lo = pack_bf2(v[0], v[1]), hi = pack_bf2(v[2], v[3]);
      // gate bit = the ROUNDED activation is positive (what the backward kernels test on the stored bf16 value)
      if (lo & 0x7FFFu) bits |= 1u << (tn * 8 + tm * 4 + 0);
      if (lo & 0x7FFF0000u) bits |= 1u << (tn * 8 + tm * 4 + 1);
      if (hi & 0x7FFFu) bits |= 1u << (tn * 8 + tm * 4 + 2);
      if (hi & 0x7FFF0000u) bits |= 1u << (tn * 8 + tm * 4 + 3);
      *(uint2*)(col + row * 256 + ((c ^ fr) << 4)) = make_uint2(lo, hi);   // row & 15 == fr
    };
    row_block(std::integral_constant<int, 0>{});
    if (two) row_block(std::integral_constant<int, 1>{});
  }
  if (gbits) *gbits = bits;
}

// the finished 32 x 256 panel -> global [rows, ldg] bf16: whole 512-byte rows, one 16-byte chunk per thread and pass; of the panel's
// rows m0 .. m0 + 31 those in [row_lo, rows) are stored
template <int NW>
__device__ __forceinline__ void panel_to_global(const unsigned char* panel, bf16_t* gout, int64_t ldg, int m0, int rows, int tid, int row_lo = 0) {
#pragma unroll
  for (int j = 0; j < (BM * 32) / (NW * 64); ++j) {
    const int idx = tid + j * NW * 64, row = idx >> 5, cc = idx & 31;
    const uint4 v = *(const uint4*)(panel + (cc >> 4) * PANEL_HALF + row * 256 + (((cc & 15) ^ (row & 15)) << 4));
    if (m0 + row < rows && m0 + row >= row_lo) *(uint4*)(gout + (int64_t)(m0 + row) * ldg + cc * 8) = v;
  }
}
}  // namespace
