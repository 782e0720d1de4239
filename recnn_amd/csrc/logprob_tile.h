// logprob_tile.h -- the 128 x 128 logits tile of the catalogue log-prob kernels (logprob.hip forward, logprob_bwd.hip backward): the
// double-buffered LDS stage that streams 128-byte row pieces of x and W, and the MFMA k-step over it.
//
// A stage holds 256 rows of ROWB = 128 bytes: rows [0, 128) are the A side of the product, rows [128, 256) the B side.  The 16-byte
// chunks of a row are xor-swizzled by the row, so the fragment reads of 16 rows spread over the banks without padding.  The forward
// and the dW / dc kernel put x on the A side and W on the B side; the dx kernel stores them swapped (stage_store<T, true>) and gets
// the transposed tile from the same k-step.
//
// Which table row stands behind a B-side column, and which bias it carries, is a policy (`Cols`): DenseCols is the whole catalogue in
// its own order (logprob.hip, logprob_bwd.hip), GatheredCols a list of item ids (sampled.hip), whose rows are read through the ids
// straight into the stage -- a gathered copy of the table never exists.
#pragma once
#include "common.h"

namespace logprob_tile {

constexpr int BM = 128;         // rows per workgroup
constexpr int BN = 128;         // items per tile
constexpr int NTN = BN / 16;    // 16-column MFMA blocks per tile
constexpr int WCH = BN * 8 / 256;   // 16-byte chunks of a W stage per thread
constexpr int ROWB = 128;       // bytes of one operand row per k-stage: 32 fp32 / 64 bf16
constexpr int STAGE_BYTES = (BM + BN) * ROWB;
// byte offset of 16-byte chunk j (of 8) of stage row `row`: the chunk index xor the row's low bits
__device__ inline int lds_at(int row, int j) { return row * ROWB + ((j ^ (row & 7)) << 4); }

// Column n of the logits is table row n; columns at or past N are absent.  The column that equals a row's action is its picked logit.
struct DenseCols {
  const float* c;
  int N;
  static constexpr bool PICK = true;
  __host__ __device__ int count() const { return N; }
  __device__ int64_t row(int n) const { return n < N ? n : -1; }      // table row of column n, -1: absent
  __device__ float bias(int n, int64_t) const { return c[n]; }
};
// Column n is table row ids[n], its bias c[ids[n]] - log_q[n] (c, log_q may be NULL: 0).  An id outside [0, N) is an absent column.
// No column is picked; with drop_hits a column whose id equals a row's action is absent in that row.
struct GatheredCols {
  const int64_t* ids;
  const float* c;
  const float* log_q;
  int S, N, drop_hits;
  static constexpr bool PICK = false;
  __host__ __device__ int count() const { return S; }
  __device__ int64_t row(int n) const {
    if (n >= S) return -1;
    const int64_t id = ids[n];
    return (id >= 0 && id < N) ? id : -1;
  }
  __device__ float bias(int n, int64_t r) const { return (c ? c[r] : 0.f) - (log_q ? log_q[n] : 0.f); }
};

template <typename T>
struct Stage;
// fp32: 32 k per stage; the 16-byte chunk j (of 8) of a row holds k 4j .. 4j + 3
template <>
struct Stage<float> {
  static constexpr int BK = ROWB / 4;
  uint4 xr[4], wr[WCH];
  template <class Cols>
  __device__ void fetch(const float* __restrict__ x, int64_t ldx, int B, int b0, const float* __restrict__ W, int64_t ldw, const Cols& cols,
                        int n0, int k0, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = tid + 256 * i, row = ch >> 3, j = ch & 7;
      const int b = b0 + row;
      xr[i] = b < B ? *(const uint4*)(x + (int64_t)b * ldx + k0 + 4 * j) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
      const int ch = tid + 256 * i, row = ch >> 3, j = ch & 7;
      const int64_t n = cols.row(n0 + row);
      wr[i] = n >= 0 ? *(const uint4*)(W + n * ldw + k0 + 4 * j) : make_uint4(0, 0, 0, 0);
    }
  }
};
// bf16: 64 k per stage; x is fp32 in memory and rounded here (nearest even), W is bf16 in memory
template <>
struct Stage<bf16_t> {
  static constexpr int BK = ROWB / 2;
  uint4 xr[4], wr[WCH];
  template <class Cols>
  __device__ void fetch(const float* __restrict__ x, int64_t ldx, int B, int b0, const bf16_t* __restrict__ W, int64_t ldw, const Cols& cols,
                        int n0, int k0, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = tid + 256 * i, row = ch >> 3, j = ch & 7;
      const int b = b0 + row;
      if (b < B) {
        const f32x4* p = (const f32x4*)(x + (int64_t)b * ldx + k0 + 8 * j);
        const f32x4 lo = p[0], hi = p[1];
        xr[i] = make_uint4(cvt_pk_bf16(lo[0], lo[1]), cvt_pk_bf16(lo[2], lo[3]), cvt_pk_bf16(hi[0], hi[1]), cvt_pk_bf16(hi[2], hi[3]));
      } else {
        xr[i] = make_uint4(0, 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
      const int ch = tid + 256 * i, row = ch >> 3, j = ch & 7;
      const int64_t n = cols.row(n0 + row);
      wr[i] = n >= 0 ? *(const uint4*)(W + n * ldw + k0 + 8 * j) : make_uint4(0, 0, 0, 0);
    }
  }
};

// x rows to the A side and W rows to the B side; SWAP: the other way round
template <typename T, bool SWAP = false>
__device__ inline void stage_store(const Stage<T>& st, char* buf, int tid) {
  static_assert(WCH == 4, "both sides of a stage are 128 rows");
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ch = tid + 256 * i, row = ch >> 3, j = ch & 7;
    *(uint4*)(buf + lds_at((SWAP ? BM : 0) + row, j)) = st.xr[i];
  }
#pragma unroll
  for (int i = 0; i < WCH; ++i) {
    const int ch = tid + 256 * i, row = ch >> 3, j = ch & 7;
    *(uint4*)(buf + lds_at((SWAP ? 0 : BM) + row, j)) = st.wr[i];
  }
}

// One stage of a wave's 16 TM x 16 TN block, in two halves of the stage's k: A rows from stage row a_row0, B rows from stage row
// b_row0 (>= BM).  Lane (q, r16) reads chunks 2 q + h of rows r16 (+ 16 per block) of both operands: the same k for A and B, which is
// all the MFMA needs.  acc[tm][tn][r] is row 16 tm + 4 q + r of the A block, column 16 tn + r16 of the B block.
template <typename T, int TM, int TN>
__device__ inline void stage_mma(const char* buf, int a_row0, int b_row0, int q, int r16, f32x4 (&acc)[TM][TN]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    uint4 a[TM], w[TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) a[tm] = *(const uint4*)(buf + lds_at(a_row0 + 16 * tm + r16, 2 * q + h));
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) w[tn] = *(const uint4*)(buf + lds_at(b_row0 + 16 * tn + r16, 2 * q + h));
    if constexpr (sizeof(T) == 4) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn) {
            const uint32_t av = e == 0 ? a[tm].x : e == 1 ? a[tm].y : e == 2 ? a[tm].z : a[tm].w;
            const uint32_t wv = e == 0 ? w[tn].x : e == 1 ? w[tn].y : e == 2 ? w[tn].z : w[tn].w;
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(av), __uint_as_float(wv), acc[tm][tn], 0, 0, 0);
          }
    } else {
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[tm]), __builtin_bit_cast(bf16x8, w[tn]),
                                                                acc[tm][tn], 0, 0, 0);
    }
  }
}

inline bool slices_of(int N, int items_per_slice, int* n_slices) {
  if (N < 1 || items_per_slice < BN || items_per_slice % BN) return false;
  *n_slices = (int)(((int64_t)N + items_per_slice - 1) / items_per_slice);
  return true;
}

}  // namespace logprob_tile
