// gemm.hip -- grouped MFMA GEMM kernels for the actor/critic MLPs (gfx950).
//
// Replaces the ATen op groups K4/K5 of SURVEY.md 2.3:
//   forward   addmm + relu + dropout                recnn/nn/models.py:66-73, :207-213
//   backward  mm (dX, dW), threshold_backward, dropout mul, bias sum   (autograd of the above)
//
// One kernel template, three operand-layout modes (all accumulate in fp32 MFMA):
//   FWD  C[m,n] = epi( sum_k A[m,k] * W[n,k] )          A, W k-contiguous           (X * W^T)
//   DX   C[m,j] = epi( sum_n dZ[m,n] * W[n,j] )         dZ k-contiguous, W k-strided (dZ * W)
//   DW   C[i,j] =      sum_m dZ[m,i] * X[m,j]           both k-strided, split over m (dZ^T * X)
// k-strided operands are transposed in registers while they are staged into LDS, so the LDS
// image is always [tile_row][k] with k contiguous and the MFMA inner loop is identical for the
// three modes.  fp32 mode uses v_mfma_f32_16x16x4_f32 (exact fp32), bf16 mode
// v_mfma_f32_16x16x32_bf16; an fp32-in-memory operand can be converted to bf16 on the fly
// (the packed fp32 batch rows feed layer 1 directly).
//
// Tile: 256 threads = 4 waves as 2x2, wave tile (16*TM) x (16*TN), block tile (32*TM) x (32*TN).
// LDS: double buffered, row pitch 144 B (128 B of k + 16 B pad).  One barrier per k-tile; the
// global loads of tile t+1 are in flight while tile t is multiplied.
#include <type_traits>
#include "gemm.h"
#include "dw_tile.h"
#include "x3.h"

template <class TC, int KB> struct LdsCfg {
  static constexpr int VEC = TcTraits<TC>::VEC;
  static constexpr int BK = KB;          // k elements per LDS stage
  static constexpr int BKP = BK + VEC;   // padded pitch in elements (+16 bytes)
};

// ------------------------------------------------------------------ staging: k-contiguous
template <class TC, bool MEM32, int R, int KB, int NT> struct KCLoader {
  static constexpr int VEC = LdsCfg<TC, KB>::VEC, BK = LdsCfg<TC, KB>::BK, BKP = LdsCfg<TC, KB>::BKP;
  static constexpr int CPR = BK / VEC;          // 16-byte LDS chunks per row (8)
  static constexpr int NCH = R * CPR / NT;      // chunks per thread
  static constexpr bool CVT = MEM32 && (sizeof(TC) == 2);
  uint4 raw[NCH][CVT ? 2 : 1];

  __device__ inline void load(const void* base, int64_t ld, int row0, int row_max, int k0, int k_end, int tid) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      int c = tid + i * NT;
      int row = c / CPR, kc = c % CPR;
      int gr = min(row0 + row, row_max);  // clamp: rows past the end re-read the last valid row
      if (k0 + kc * VEC >= k_end) {       // k tail of the last stage: zeros
        raw[i][0] = make_uint4(0, 0, 0, 0);
        if constexpr (CVT) raw[i][1] = make_uint4(0, 0, 0, 0);
        continue;
      }
      if constexpr (CVT) {
        const float* p = (const float*)base + (int64_t)gr * ld + k0 + kc * 8;
        raw[i][0] = *(const uint4*)p;
        raw[i][1] = *(const uint4*)(p + 4);
      } else if constexpr (sizeof(TC) == 4) {
        const float* p = (const float*)base + (int64_t)gr * ld + k0 + kc * 4;
        raw[i][0] = *(const uint4*)p;
      } else {
        const bf16_t* p = (const bf16_t*)base + (int64_t)gr * ld + k0 + kc * 8;
        raw[i][0] = *(const uint4*)p;
      }
    }
  }
  __device__ inline void store(TC* lds, int tid) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      int c = tid + i * NT;
      int row = c / CPR, kc = c % CPR;
      uint4 v;
      if constexpr (CVT) {
        const float* f0 = (const float*)&raw[i][0];
        const float* f1 = (const float*)&raw[i][1];
        v.x = pack_bf2(f0[0], f0[1]); v.y = pack_bf2(f0[2], f0[3]);
        v.z = pack_bf2(f1[0], f1[1]); v.w = pack_bf2(f1[2], f1[3]);
      } else {
        v = raw[i][0];
      }
      *(uint4*)&lds[row * BKP + kc * VEC] = v;
    }
  }
};

// ------------------------------------------------------------------ staging: k-strided (transpose)
// Source is [Kc, ld] with the tile dimension contiguous.  A unit = 4 consecutive k rows x one
// 16-byte load along the tile dimension (NE elements); it is transposed in registers and written
// as NE small vectors of 4 k values.
template <class TC, bool MEM32, int R, int KB, bool TGF, int NT> struct KSLoader {
  static constexpr int VEC = LdsCfg<TC, KB>::VEC, BK = LdsCfg<TC, KB>::BK, BKP = LdsCfg<TC, KB>::BKP;
  static constexpr bool SRC32 = MEM32 || (sizeof(TC) == 4);
  static constexpr int NE = SRC32 ? 4 : 8;      // tile elements per 16-byte load
  static constexpr int KG = BK / 4;             // k groups per stage
  static constexpr int UNITS = (R / NE) * KG;
  static constexpr int UPT = (UNITS + NT - 1) / NT;
  uint4 raw[UPT][4];

  __device__ inline void load(const void* base, int64_t ld, int tile0, int k0, int k_end, int tid) {
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      int u = tid + i * NT;
      if (UNITS % NT == 0 || u < UNITS) {
        // TGF: consecutive lanes walk the (contiguous) tile dimension -> 256-byte runs per k row in global memory
        // (LDS writes then collide 4-way); otherwise consecutive lanes walk k (conflict-free LDS writes).
        int kg = TGF ? u / (R / NE) : u % KG, tg = TGF ? u % (R / NE) : u / KG;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          int kr = k0 + kg * 4 + j;
          uint4 v = make_uint4(0, 0, 0, 0);
          if (kr < k_end) {
            if constexpr (SRC32) v = *(const uint4*)((const float*)base + (int64_t)kr * ld + tile0 + tg * NE);
            else v = *(const uint4*)((const bf16_t*)base + (int64_t)kr * ld + tile0 + tg * NE);
          }
          raw[i][j] = v;
        }
      }
    }
  }
  __device__ inline void store(TC* lds, int tid) {
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      int u = tid + i * NT;
      if (UNITS % NT == 0 || u < UNITS) {
        int kg = TGF ? u / (R / NE) : u % KG, tg = TGF ? u % (R / NE) : u / KG;
        if constexpr (sizeof(TC) == 4) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float4 v;
            v.x = ((const float*)&raw[i][0])[e]; v.y = ((const float*)&raw[i][1])[e];
            v.z = ((const float*)&raw[i][2])[e]; v.w = ((const float*)&raw[i][3])[e];
            *(float4*)&lds[(tg * 4 + e) * BKP + kg * 4] = v;
          }
        } else if constexpr (SRC32) {  // fp32 in memory -> bf16 in LDS
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            uint2 v;
            v.x = pack_bf2(((const float*)&raw[i][0])[e], ((const float*)&raw[i][1])[e]);
            v.y = pack_bf2(((const float*)&raw[i][2])[e], ((const float*)&raw[i][3])[e]);
            *(uint2*)&lds[(tg * 4 + e) * BKP + kg * 4] = v;
          }
        } else {  // bf16 in memory
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            uint2 v;
            uint32_t h0 = ((const uint16_t*)&raw[i][0])[e], h1 = ((const uint16_t*)&raw[i][1])[e];
            uint32_t h2 = ((const uint16_t*)&raw[i][2])[e], h3 = ((const uint16_t*)&raw[i][3])[e];
            v.x = h0 | (h1 << 16);
            v.y = h2 | (h3 << 16);
            *(uint2*)&lds[(tg * 8 + e) * BKP + kg * 4] = v;
          }
        }
      }
    }
  }
};

// ------------------------------------------------------------------ MFMA on one LDS stage
template <class TC, int TM, int TN, int KB>
__device__ inline void mma_stage(const TC* As, const TC* Bs, f32x4 (&acc)[TM][TN], int wm0, int wn0, int lane) {
  constexpr int VEC = LdsCfg<TC, KB>::VEC, BK = LdsCfg<TC, KB>::BK, BKP = LdsCfg<TC, KB>::BKP, KSTEP = TcTraits<TC>::KSTEP;
  const int fr = lane & 15, fg = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < BK / KSTEP; ++ks) {
    uint4 a[TM], b[TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) a[tm] = *(const uint4*)&As[(wm0 + tm * 16 + fr) * BKP + ks * KSTEP + fg * VEC];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) b[tn] = *(const uint4*)&Bs[(wn0 + tn * 16 + fr) * BKP + ks * KSTEP + fg * VEC];
    if constexpr (sizeof(TC) == 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(((const float*)&a[tm])[j], ((const float*)&b[tn])[j],
                                                               acc[tm][tn], 0, 0, 0);
    } else {
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[tm]),
                                                                __builtin_bit_cast(bf16x8, b[tn]), acc[tm][tn], 0, 0, 0);
    }
  }
}

// ------------------------------------------------------------------ forward epilogue (shared by both fwd kernels)
template <class TC, int TM, int TN>
__device__ inline void epilogue_fwd(const GemmProb& P, f32x4 (&acc)[TM][TN], int m0, int n0, int wm0, int wn0, int lane,
                                    int part_idx) {
  const int fr = lane & 15, fg = lane >> 4;
  float sdot = 0.f;
  {
    uint32_t key = 0;
    if (P.mask_mode == RECNN_MASK_HASH) key = mask_key(P.seed, (P.step_ptr ? *P.step_ptr : 0) + P.step_add, P.stream_id);
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        const int n = n0 + wn0 + tn * 16 + fr;
        const int mb = m0 + wm0 + tm * 16 + fg * 4;
        if (n < P.N) {
          const float bv = P.bias ? P.bias[n] : 0.f;
          const float dw = P.dot_w ? P.dot_w[n] : 0.f;
          uint32_t word = 0;
          if (P.mask_mode == RECNN_MASK_HASH) word = mask_word(key, (uint32_t)(mb >> 2), (uint32_t)(n >> 2));
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = mb + r;
            if (m < P.M) {
              float v = acc[tm][tn][r] + bv;
              if (P.addend) {
                const int ma = P.add_row_div > 1 ? m / P.add_row_div : m;
                float z = P.addend[(int64_t)ma * P.ld_add + n];
                v += fminf(fmaxf(z, -P.add_clip), P.add_clip);
              }
              if (P.relu) v = fmaxf(v, 0.f);
              if (P.yref) {  // gate of a backward pass run as a forward-layout GEMM (transposed weights): [yref > 0] * scale
                const float y = tc_load((const TC*)P.yref + (int64_t)m * P.ldy + n);
                v = y > 0.f ? v * P.dx_scale : 0.f;
              }
              if (P.mask_mode == RECNN_MASK_EXTERNAL) v = P.mask[(int64_t)m * P.ld_mask + n] ? v * 2.f : 0.f;
              else if (P.mask_mode == RECNN_MASK_HASH) v = mask_keep(word, r, n & 3) ? v * 2.f : 0.f;
              if (P.c_f32) {
                ((float*)P.C)[(int64_t)m * P.ldc + n] = v;
              } else {
                TC* dst = (TC*)P.C + (int64_t)m * P.ldc + n;
                tc_store(dst, v);
                if constexpr (sizeof(TC) == 2) v = bf2f(f2bf(v));  // the value a consumer of C would read
              }
              sdot += v * dw;
              if (n == 0 && P.dot_bias) sdot += P.dot_bias[0];
            }
          }
        }
      }
  }
  if (P.dot_part) {  // uniform
    sdot = wave_sum(sdot);
    if (lane == 0) P.dot_part[part_idx] = sdot;
  }
}

// ------------------------------------------------------------------ forward epilogue, split-bf16 output (x3.h)
// The x3 kernels multiply with the operands swapped (weights first): acc[tm][tn][r] = C[row 16 tm + fr][column 16 tn + 4 fg + r],
// i.e. a lane owns FOUR NEIGHBOURING COLUMNS of one row -- one 8-byte store for their hi halves and one for the lo halves (the
// generic layout, four rows of one column, would take eight 2-byte stores), one 16-byte load of the bias / addend, one dropout
// word per 4 x 4 block.  Same arithmetic, element by element, as epilogue_fwd.
// lds_tile != nullptr (wave-specialised kernel, full tiles of split output): the hi / lo halves go into an LDS image of the tile -- row
// r = m - m0 at r * X3_TILE_PITCH, physical column x3_col(n - n0) -- instead of global memory; the caller then writes the tile out as whole
// 16-byte x 64-lane rows (a lane's two 8-byte stores per block hit 16 rows x 32 bytes per wave instruction: the store tail was 5 of the
// layer-1 launch's 24 us, profiles/r05_x3_ws_probe_fixed.txt).
constexpr int X3_TILE_PITCH_PAD = 16;
// SPLIT = false (round 5, the wave-specialised kernel on PLAIN bf16 operands: catalogue-wide products): the same lane layout and arithmetic,
// plain fp32 / bf16 output (16- / 8-byte stores of four neighbouring columns), yref a plain bf16 matrix; the LDS tile image is then
// [row][BN outputs] in the output type.
template <int TM, int TN, bool SPLIT = true>
__device__ inline void epilogue_fwd_x3(const GemmProb& P, f32x4 (&acc)[TM][TN], int m0, int n0, int wm0, int wn0, int lane, int part_idx,
                                       unsigned char* lds_tile = nullptr, int tile_pitch = 0) {
  const int fr = lane & 15, fg = lane >> 4;
  float sdot = 0.f;
  uint32_t key = 0;
  if (P.mask_mode == RECNN_MASK_HASH) key = mask_key(P.seed, (P.step_ptr ? *P.step_ptr : 0) + P.step_add, P.stream_id);
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    const int m = m0 + wm0 + tm * 16 + fr;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int nb = n0 + wn0 + tn * 16 + fg * 4;
      if (m >= P.M || nb >= P.N) continue;
      const bool full = nb + 3 < P.N;
      float bv[4] = {0.f, 0.f, 0.f, 0.f}, dw[4] = {0.f, 0.f, 0.f, 0.f}, ad[4] = {0.f, 0.f, 0.f, 0.f};
      uint32_t mk = 0x01010101u;
      uint2 yh = make_uint2(0x3F803F80u, 0x3F803F80u);   // (bf16 1.0: gate open)
      // every load of the block before the first use
      if (P.bias) {
        if (full) { const float4 t = *(const float4*)(P.bias + nb); bv[0] = t.x; bv[1] = t.y; bv[2] = t.z; bv[3] = t.w; }
        else for (int r = 0; r < 4; ++r) if (nb + r < P.N) bv[r] = P.bias[nb + r];
      }
      if (P.dot_w) {
        if (full) { const float4 t = *(const float4*)(P.dot_w + nb); dw[0] = t.x; dw[1] = t.y; dw[2] = t.z; dw[3] = t.w; }
        else for (int r = 0; r < 4; ++r) if (nb + r < P.N) dw[r] = P.dot_w[nb + r];
      }
      if (P.addend) {
        const int ma = P.add_row_div > 1 ? m / P.add_row_div : m;
        const float* ap = P.addend + (int64_t)ma * P.ld_add + nb;
        if (full && !(P.ld_add & 3) && !((uintptr_t)P.addend & 15)) { const float4 t = *(const float4*)ap; ad[0] = t.x; ad[1] = t.y; ad[2] = t.z; ad[3] = t.w; }
        else for (int r = 0; r < 4; ++r) if (nb + r < P.N) ad[r] = ap[r];
      }
      if (P.yref) {
        if constexpr (SPLIT) yh = *(const uint2*)((const bf16_t*)P.yref + (int64_t)m * P.ldy + x3_col(nb));
        else {
          const bf16_t* yp = (const bf16_t*)P.yref + (int64_t)m * P.ldy + nb;
          if (full && !(P.ldy & 3) && !((uintptr_t)P.yref & 7)) yh = *(const uint2*)yp;
          else {
            uint32_t e[4] = {0x3F80u, 0x3F80u, 0x3F80u, 0x3F80u};
            for (int r = 0; r < 4; ++r) if (nb + r < P.N) e[r] = yp[r];
            yh = make_uint2(e[0] | (e[1] << 16), e[2] | (e[3] << 16));
          }
        }
      }
      if (P.mask_mode == RECNN_MASK_EXTERNAL) {
        const uint8_t* mp = P.mask + (int64_t)m * P.ld_mask + nb;
        if (full && !(P.ld_mask & 3) && !((uintptr_t)P.mask & 3)) mk = *(const uint32_t*)mp;
        else { mk = 0; for (int r = 0; r < 4; ++r) if (nb + r < P.N) mk |= (uint32_t)(mp[r] ? 1u : 0u) << (8 * r); }
      }
      uint32_t word = 0;
      if (P.mask_mode == RECNN_MASK_HASH) word = mask_word(key, (uint32_t)(m >> 2), (uint32_t)(nb >> 2));
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = acc[tm][tn][r] + bv[r];
        if (P.addend) x += fminf(fmaxf(ad[r], -P.add_clip), P.add_clip);
        if (P.relu) x = fmaxf(x, 0.f);
        if (P.yref) {
          const float y = bf2f((bf16_t)((r < 2 ? yh.x : yh.y) >> ((r & 1) * 16)));
          x = y > 0.f ? x * P.dx_scale : 0.f;
        }
        if (P.mask_mode == RECNN_MASK_EXTERNAL) x = ((mk >> (8 * r)) & 0xFFu) ? x * 2.f : 0.f;
        else if (P.mask_mode == RECNN_MASK_HASH) x = mask_keep(word, m & 3, r) ? x * 2.f : 0.f;
        v[r] = x;
      }
      if (P.c_f32) {
        float* dst = (float*)P.C + (int64_t)m * P.ldc + nb;
        if (!SPLIT && lds_tile) *(float4*)(lds_tile + (m - m0) * tile_pitch + (nb - n0) * 4) = make_float4(v[0], v[1], v[2], v[3]);
        else if (full && !(P.ldc & 3) && !((uintptr_t)P.C & 15)) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
        else for (int r = 0; r < 4; ++r) if (nb + r < P.N) dst[r] = v[r];
      } else if constexpr (!SPLIT) {
        const uint2 pk = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
        bf16_t* dst = (bf16_t*)P.C + (int64_t)m * P.ldc + nb;
        if (lds_tile) *(uint2*)(lds_tile + (m - m0) * tile_pitch + (nb - n0) * 2) = pk;
        else if (full && !(P.ldc & 3) && !((uintptr_t)P.C & 7)) *(uint2*)dst = pk;
        else for (int r = 0; r < 4; ++r) if (nb + r < P.N) dst[r] = (bf16_t)((r < 2 ? pk.x : pk.y) >> ((r & 1) * 16));
        // the values a consumer of C would read
        v[0] = bf2f((bf16_t)(pk.x & 0xFFFFu)); v[1] = bf2f((bf16_t)(pk.x >> 16)); v[2] = bf2f((bf16_t)(pk.y & 0xFFFFu)); v[3] = bf2f((bf16_t)(pk.y >> 16));
      } else {
        uint2 hi, lo;
        x3_split4(v, hi, lo);
        bf16_t* dst = (bf16_t*)P.C + (int64_t)m * P.ldc + x3_col(nb);
        if (lds_tile) {
          unsigned char* t = lds_tile + (m - m0) * tile_pitch + x3_col(nb - n0) * 2;
          *(uint2*)t = hi;
          *(uint2*)(t + 64) = lo;
        } else if (full) {
          *(uint2*)dst = hi;
          *(uint2*)(dst + 32) = lo;
        } else {
          for (int r = 0; r < 4; ++r)
            if (nb + r < P.N) {
              dst[r] = (bf16_t)((r < 2 ? hi.x : hi.y) >> ((r & 1) * 16));
              dst[32 + r] = (bf16_t)((r < 2 ? lo.x : lo.y) >> ((r & 1) * 16));
            }
        }
        // the values a consumer of C would read
        v[0] = bf2f((bf16_t)(hi.x & 0xFFFFu)) + bf2f((bf16_t)(lo.x & 0xFFFFu)); v[1] = bf2f((bf16_t)(hi.x >> 16)) + bf2f((bf16_t)(lo.x >> 16));
        v[2] = bf2f((bf16_t)(hi.y & 0xFFFFu)) + bf2f((bf16_t)(lo.y & 0xFFFFu)); v[3] = bf2f((bf16_t)(hi.y >> 16)) + bf2f((bf16_t)(lo.y >> 16));
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) if (nb + r < P.N) sdot += v[r] * dw[r];
      if (nb == 0 && P.dot_bias) sdot += P.dot_bias[0];
    }
  }
  if (P.dot_part) {  // uniform
    sdot = wave_sum(sdot);
    if (lane == 0) P.dot_part[part_idx] = sdot;
  }
}

// ------------------------------------------------------------------ the kernel
template <class TC, int MODE, bool A32, bool B32, int TM, int TN, int KB, bool TGF, int NW>
__global__ __launch_bounds__(NW * 64) void gemm_kernel(const GemmBatch batch) {
  // NW waves as 2 x (NW/2): wave tile (16 TM) x (16 TN), block tile (32 TM) x (16 TN NW/2)
  constexpr int WC = NW / 2, NT = NW * 64;
  constexpr int BM = 32 * TM, BN = 16 * TN * WC;
  constexpr int BK = LdsCfg<TC, KB>::BK, BKP = LdsCfg<TC, KB>::BKP;
  constexpr bool A_KS = (MODE == GEMM_DW);
  constexpr bool B_KS = (MODE != GEMM_FWD);
  const GemmProb& P = batch.p[blockIdx.y];

  const int splits = (MODE == GEMM_DW) ? P.dw_splits : 1;
  const int nwg = P.tiles_m * P.tiles_n * splits;
  if ((int)blockIdx.x >= nwg) return;
  const int lid = xcd_remap(blockIdx.x, nwg);
  const int tile_n = lid % P.tiles_n;
  const int tile_m = (lid / P.tiles_n) % P.tiles_m;
  const int split = lid / (P.tiles_n * P.tiles_m);
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  __shared__ __attribute__((aligned(16))) TC smem[2 * (BM + BN) * BKP];
  constexpr int STAGE = (BM + BN) * BKP;  // one LDS stage: A tile then B tile

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm0 = (wave / WC) * 16 * TM, wn0 = (wave % WC) * 16 * TN;

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // contraction schedule
  int nt0, nt1 = 0, kbeg = 0, kend = 0;
  if constexpr (MODE == GEMM_DW) {
    const int Kc = P.seg[0].K;
    int chunk = (((Kc + splits - 1) / splits) + BK - 1) / BK * BK;
    kbeg = split * chunk;
    kend = min(Kc, kbeg + chunk);
    nt0 = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;
  } else {
    nt0 = (P.seg[0].K + BK - 1) / BK;
    nt1 = P.nseg > 1 ? (P.seg[1].K + BK - 1) / BK : 0;
    kend = P.seg[0].K;
  }
  const int nt = nt0 + nt1;

  using ALoader = typename std::conditional<A_KS, KSLoader<TC, A32, BM, KB, TGF, NT>, KCLoader<TC, A32, BM, KB, NT>>::type;
  using BLoader = typename std::conditional<B_KS, KSLoader<TC, B32, BN, KB, TGF, NT>, KCLoader<TC, B32, BN, KB, NT>>::type;
  ALoader la;
  BLoader lb;

  auto issue = [&](int t) {
    const int s = (t < nt0) ? 0 : 1;
    const GemmSeg& G = P.seg[s];
    const int k0 = kbeg + (s == 0 ? t : t - nt0) * BK;
    const int ke = (MODE == GEMM_DW) ? kend : G.K;
    if constexpr (A_KS) la.load(G.A, G.lda, m0, k0, ke, tid);
    else la.load(G.A, G.lda, m0, P.M - 1, k0, ke, tid);
    if constexpr (B_KS) lb.load(G.B, G.ldb, n0, k0, ke, tid);
    else lb.load(G.B, G.ldb, n0, P.N - 1, k0, ke, tid);
  };

  if (nt > 0) {
    issue(0);
    la.store(smem, tid);
    lb.store(smem + BM * BKP, tid);
  }
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) issue(t + 1);
    TC* sa = smem + cur * STAGE;
    TC* sn = smem + (cur ^ 1) * STAGE;
    mma_stage<TC, TM, TN, KB>(sa, sa + BM * BKP, acc, wm0, wn0, lane);
    if (t + 1 < nt) {
      la.store(sn, tid);
      lb.store(sn + BM * BKP, tid);
    }
    __syncthreads();
  }

  // ------------------------------------------------------------------ epilogue
  const int fr = lane & 15, fg = lane >> 4;
  if constexpr (MODE == GEMM_FWD) {
    epilogue_fwd<TC, TM, TN>(P, acc, m0, n0, wm0, wn0, lane, lid * NW + wave);
  } else if constexpr (MODE == GEMM_DX) {
    float cs[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) cs[tn] = 0.f;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        const int n = n0 + wn0 + tn * 16 + fr;
        const int mb = m0 + wm0 + tm * 16 + fg * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = mb + r;
          if (m < P.M && n < P.N) {
            float v = acc[tm][tn][r] * P.dx_scale;
            if (P.yref) {
              float y = tc_load((const TC*)P.yref + (int64_t)m * P.ldy + n);
              v = y > 0.f ? v : 0.f;
            }
            cs[tn] += v;
            if (P.c_f32) ((float*)P.C)[(int64_t)m * P.ldc + n] = v;
            else tc_store((TC*)P.C + (int64_t)m * P.ldc + n, v);
          }
        }
      }
    if (P.colsum) {
      // column sums of this row tile -> colsum[tile_m][n]  (deterministic: fixed summation tree)
      float* red = (float*)smem;  // [2 (wave row)][BN]
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        float v = cs[tn];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (fg == 0) red[(wave / WC) * BN + wn0 + tn * 16 + fr] = v;
      }
      __syncthreads();
      // slab granularity is 32 rows whatever the block tile: a 64-row tile writes two slabs
      if (tid < BN && n0 + tid < P.N) {
        if constexpr (BM == 32) {
          P.colsum[(int64_t)tile_m * P.N + n0 + tid] = red[tid] + red[BN + tid];
        } else {
          P.colsum[(int64_t)(2 * tile_m) * P.N + n0 + tid] = red[tid];
          if (m0 + 32 < P.M) P.colsum[(int64_t)(2 * tile_m + 1) * P.N + n0 + tid] = red[BN + tid];
        }
      }
    }
  } else {  // GEMM_DW
    float* Cs = (float*)P.C + (int64_t)split * P.dw_slab_stride;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        const int n = n0 + wn0 + tn * 16 + fr;
        const int mb = m0 + wm0 + tm * 16 + fg * 4;
        if (n < P.dw_valid_cols) {
          int cc = n + P.dw_col_rot;
          if (cc >= P.dw_valid_cols) cc -= P.dw_valid_cols;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = mb + r;
            if (m < P.M) Cs[(int64_t)m * P.ldc + cc] = acc[tm][tn][r];
          }
        }
      }
  }
}

// ------------------------------------------------------------------ forward GEMM, LDS-DMA pipeline
// C = epi(A W^T) for k-contiguous operands stored in the compute type.  Tiles are copied global -> LDS by
// `global_load_lds_dwordx4` (no VGPR round trip) into a 3-stage ring: two k stages are in flight while the third
// is multiplied, one raw s_barrier per stage, counted vmcnt waits (the asm loads are invisible to hipcc's wait
// insertion, which would otherwise drain every DMA before each ds_read).  A k stage is 256 bytes per tile row;
// the 16-byte chunk c of row r sits at chunk position c ^ (r & 15) of its LDS row (the DMA writes lane-linear,
// so the XOR is applied to each lane's SOURCE address), which makes the 16 rows x one chunk of an MFMA fragment
// read hit 16 different bank quads.  (dma16, lds_stream.h)

// X3 (x3.h): the operands are split-bf16 rows; a 256-byte stage row is two logical 32-k groups [hi 32 | lo 32 | hi 32 | lo 32], each
// contracted with three MFMAs (hi hi + hi lo + lo hi); K / lda / ldb are physical, the epilogue writes split columns.
// MFAST: consecutive workgroup ids walk the ROW tiles of one column tile (catalogue-wide products: few rows, 100k columns) -- the
// two / four row tiles that share a weight panel run side by side on one XCD, so the panel leaves HBM once.
template <class TC, int TM, int TN, int NS, int NW, bool X3 = false, bool MFAST = false>
__global__ __launch_bounds__(NW * 64) void gemm_fwd_dma_kernel(const GemmBatch batch) {
  // NW waves arranged (NW/2) x 2 ... 4 waves: 2x2 wave tiles of (16 TM) x (16 TN); 8 waves: 2x4 wave tiles
  constexpr int WCOLS = NW / 2;
  constexpr int BM = 32 * TM, BN = 16 * TN * WCOLS;
  constexpr int ES = sizeof(TC), KB = 256 / ES;  // k elements per stage (256-byte rows)
  constexpr int D = NS - 1;                      // prefetch distance: D k stages are in flight ahead of the MFMAs
  constexpr int STAGE_BYTES = (BM + BN) * 256;
  constexpr int NA = BM / (4 * NW), NB = BN / (4 * NW);  // DMA instructions per wave and stage (4 rows each)
  constexpr int KSTEP = TcTraits<TC>::KSTEP;
  const GemmProb& P = batch.p[blockIdx.y];
  const int nwg = P.tiles_m * P.tiles_n;
  if ((int)blockIdx.x >= nwg) return;
  const int lid = xcd_remap(blockIdx.x, nwg);
  const int tile_n = MFAST ? lid / P.tiles_m : lid % P.tiles_n, tile_m = MFAST ? lid % P.tiles_m : lid / P.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  extern __shared__ __attribute__((aligned(16))) unsigned char dsmem[];
  const unsigned lds0 = (unsigned)(size_t)dsmem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wave / WCOLS) * 16 * TM, wn0 = (wave % WCOLS) * 16 * TN;
  const int fr = lane & 15, fg = lane >> 4;

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nt0 = P.seg[0].K / KB;
  const int nt1 = P.nseg > 1 ? P.seg[1].K / KB : 0;
  const int nt = nt0 + nt1;

  // per-lane source geometry (constant over the k loop): chunk q = (j*4 + wave)*64 + lane of a tile
  const int q_row = lane >> 4, q_pos = lane & 15;  // within the 4 rows one wave instruction covers

  // the i-th of the wave's NA + NB DMA instructions of tile t (A rows first)
  auto issue_one = [&](int t, int stage, int i) {
    const int sidx = (t < nt0) ? 0 : 1;
    const GemmSeg& G = P.seg[sidx];
    const int k0 = (sidx == 0 ? t : t - nt0) * KB;
    const unsigned sbase = lds0 + stage * STAGE_BYTES;
    const bool isa = i < NA;
    const int j = isa ? i : i - NA;
    const int row = (j * NW + wave) * 4 + q_row;
    const int c = q_pos ^ (row & 15);
    if (isa) {
      const int gr = min(m0 + row, P.M - 1);
      dma16((const char*)G.A + ((int64_t)gr * G.lda + k0) * ES + c * 16, sbase + (j * NW + wave) * 1024);
    } else {
      const int gr = min(n0 + row, P.N - 1);
      dma16((const char*)G.B + ((int64_t)gr * G.ldb + k0) * ES + c * 16, sbase + BM * 256 + (j * NW + wave) * 1024);
    }
  };
  auto issue = [&](int t, int stage) {
#pragma unroll
    for (int i = 0; i < NA + NB; ++i) issue_one(t, stage, i);
  };

#pragma unroll
  for (int i = 0; i < D; ++i)
    if (i < nt) issue(i, i);
  for (int t = 0; t < nt; ++t) {
    // tile t has landed once at most the loads of the (up to D-1) younger tiles are still outstanding
    const int younger = min(D - 1, nt - 1 - t);
    if (younger >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * (NA + NB)) : "memory");
    else if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (NA + NB)) : "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NA + NB) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave's part of tile t is in LDS; every wave is done reading tile t-1
    if (t + D < nt) issue(t + D, (t + D) % NS);
    const unsigned char* sa = dsmem + (t % NS) * STAGE_BYTES;
    const unsigned char* sb = sa + BM * 256;
    if constexpr (X3) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int ph = ((g * 8 + fg) ^ fr) * 16, pl = ((g * 8 + 4 + fg) ^ fr) * 16;
        uint4 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
          ah[tm] = *(const uint4*)(sa + (wm0 + tm * 16 + fr) * 256 + ph);
          al[tm] = *(const uint4*)(sa + (wm0 + tm * 16 + fr) * 256 + pl);
        }
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
          bh[tn] = *(const uint4*)(sb + (wn0 + tn * 16 + fr) * 256 + ph);
          bl[tn] = *(const uint4*)(sb + (wn0 + tn * 16 + fr) * 256 + pl);
        }
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = x3_mfma(__builtin_bit_cast(bf16x8, bh[tn]), __builtin_bit_cast(bf16x8, bl[tn]), __builtin_bit_cast(bf16x8, ah[tm]),
                                  __builtin_bit_cast(bf16x8, al[tm]), acc[tm][tn]);   // (weights first: a lane owns 4 columns of one row)
      }
    } else
#pragma unroll
    for (int ks = 0; ks < KB / KSTEP; ++ks) {
      const int pos = ((ks * 4 + fg) ^ fr) * 16;
      uint4 a[TM], b[TN];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) a[tm] = *(const uint4*)(sa + (wm0 + tm * 16 + fr) * 256 + pos);
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) b[tn] = *(const uint4*)(sb + (wn0 + tn * 16 + fr) * 256 + pos);
      if constexpr (ES == 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
              acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(((const float*)&a[tm])[j], ((const float*)&b[tn])[j],
                                                                 acc[tm][tn], 0, 0, 0);
      } else {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[tm]),
                                                                  __builtin_bit_cast(bf16x8, b[tn]), acc[tm][tn], 0, 0, 0);
      }
    }
  }
  if constexpr (X3) epilogue_fwd_x3<TM, TN>(P, acc, m0, n0, wm0, wn0, lane, lid * NW + wave);
  else epilogue_fwd<TC, TM, TN>(P, acc, m0, n0, wm0, wn0, lane, lid * NW + wave);
}

// The same epilogue for a FULL tile of split output that leaves through the LDS image (the wave-specialised kernel's common case), written
// lean: the problem's fields in registers once, the bias (and last-layer weights) of a lane's column groups loaded once, no ragged-edge /
// backward-gate code.  epilogue_fwd_x3's general body costs ~1900 clk per (tm, tn) block even with everything switched off (3.2 of the layer-1 launch's
// 23.3 us: recnn_debug_ws_trace) -- kernel-argument loads and branches, not arithmetic.  Element by element the same arithmetic.
template <int TM, int TN>
__device__ __forceinline__ void epilogue_x3_full_tile(const GemmProb& P, f32x4 (&acc)[TM][TN], int m0, int n0, int wm0, int wn0, int lane,
                                                      int part_idx, unsigned char* lds_tile, int tile_pitch) {
  const int fr = lane & 15, fg = lane >> 4;
  const float* const bias = P.bias;
  const float* const addend = P.addend;
  const uint8_t* const mask = P.mask;
  const int relu = P.relu, mask_mode = P.mask_mode, add_row_div = P.add_row_div;
  const int64_t ld_add = P.ld_add, ld_mask = P.ld_mask;
  const float add_clip = P.add_clip;
  uint32_t key = 0;
  if (mask_mode == RECNN_MASK_HASH) key = mask_key(P.seed, (P.step_ptr ? *P.step_ptr : 0) + P.step_add, P.stream_id);
  // the last layer's dot product riding on this GEMM (the policy loss: -Q(s, pi(s)) summed from these partials): per lane in the general
  // epilogue's block order, over the values a consumer of C would read (hi + lo), one partial per wave
  float* const dot_part = P.dot_part;
  const float* const dot_w = dot_part ? P.dot_w : nullptr;
  const float* const dot_bias = dot_part ? P.dot_bias : nullptr;
  float sdot = 0.f;
  f32x4 bv[TN], dwv[TN];
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    bv[tn] = bias ? *(const f32x4*)(bias + n0 + wn0 + tn * 16 + fg * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    dwv[tn] = dot_w ? *(const f32x4*)(dot_w + n0 + wn0 + tn * 16 + fg * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) {
    const int m = m0 + wm0 + tm * 16 + fr;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int nb = n0 + wn0 + tn * 16 + fg * 4;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[tm][tn][r] + bv[tn][r];
      if (addend) {
        const int ma = add_row_div > 1 ? m / add_row_div : m;
        const float* ap = addend + (int64_t)ma * ld_add + nb;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += fminf(fmaxf(ap[r], -add_clip), add_clip);
      }
      if (relu) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
      }
      if (mask_mode == RECNN_MASK_EXTERNAL) {
        const uint8_t* mp = mask + (int64_t)m * ld_mask + nb;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = mp[r] ? v[r] * 2.f : 0.f;
      } else if (mask_mode == RECNN_MASK_HASH) {
        const uint32_t word = mask_word(key, (uint32_t)(m >> 2), (uint32_t)(nb >> 2));
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = mask_keep(word, m & 3, r) ? v[r] * 2.f : 0.f;
      }
      uint2 hi, lo;
      x3_split4(v, hi, lo);
      unsigned char* t = lds_tile + (m - m0) * tile_pitch + x3_col(nb - n0) * 2;
      *(uint2*)t = hi;
      *(uint2*)(t + 64) = lo;
      if (dot_part) {
        const float c0 = bf2f((bf16_t)(hi.x & 0xFFFFu)) + bf2f((bf16_t)(lo.x & 0xFFFFu)), c1 = bf2f((bf16_t)(hi.x >> 16)) + bf2f((bf16_t)(lo.x >> 16));
        const float c2 = bf2f((bf16_t)(hi.y & 0xFFFFu)) + bf2f((bf16_t)(lo.y & 0xFFFFu)), c3 = bf2f((bf16_t)(hi.y >> 16)) + bf2f((bf16_t)(lo.y >> 16));
        sdot += c0 * dwv[tn][0];
        sdot += c1 * dwv[tn][1];
        sdot += c2 * dwv[tn][2];
        sdot += c3 * dwv[tn][3];
        if (nb == 0 && dot_bias) sdot += dot_bias[0];
      }
    }
  }
  if (dot_part) {  // uniform
    sdot = wave_sum(sdot);
    if (lane == 0) dot_part[part_idx] = sdot;
  }
}

// ------------------------------------------------------------------ split-bf16 forward GEMM, wave-specialised (round 5)
// Same tile image, arithmetic and epilogue as gemm_fwd_dma_kernel<.., X3>, different division of labour: NL LOADER waves do nothing
// but issue the LDS-DMA of the ring (tile t + D while tile t is multiplied), WR x WC CONSUMER waves do nothing but read fragments and
// issue MFMAs.  In the all-waves-do-everything kernel a wave's MFMAs of tile t sit behind its own DMA instructions of tile t + D in
// program order, and those stall at the CU's vector-memory issue (one 1 KB global_load_lds_dwordx4 ~ 25-60 clk, CU-serial), so the
// matrix pipe idles for the whole issue burst of every stage (profiles/r04_x3_pmc.txt: matrix cores 25 % busy, waves parked 40 %).
// One s_barrier per k stage, taken by all waves; loaders leave after the last one.
// SR = bytes per stage row: 256 (two logical 32-k groups per stage, chunk c of row r at position c ^ (r & 15)) or 128 (one group per
// stage -- tiles of 128 x 128 / 128 x 256 then fit a 3-4 deep ring; chunk c of row r at position c ^ ((r >> 1) & 7): rows r, r + 1 sit in
// the two halves of one 256-byte bank row, so the 16 rows x 16 bytes of a fragment read still cover all 64 banks exactly once).
template <int TM, int TN, int WR, int WC, int NL, int NS, int SR = 256, bool X3 = true>
__global__ __launch_bounds__((WR * WC + NL) * 64) void x3_fwd_ws_kernel(const GemmBatch batch, const int probe, unsigned long long* trace) {
  // probe (recnn_debug_x3_ws_probe, timing experiments only, results garbage): bit 0 consumers do nothing but the barriers, bit 1 loaders
  // issue nothing, bit 2 consumers read their fragments but issue no MFMA, bit 3 consumers issue the MFMAs on stale registers (no reads),
  // bit 4 no epilogue, bit 5 exit at entry, bit 6 epilogue stores straight to global memory (round 5's first form),
  // bit 7 plain (not write-through) tile stores, bit 8 no kernel-argument prefetch, bit 9 the unpipelined consumer loop (round 5's first form), bit 10 the general epilogue on full tiles
  constexpr int NC = WR * WC, BM = 16 * TM * WR, BN = 16 * TN * WC;
  constexpr int KB = SR / 2;                      // physical k elements per stage
  constexpr int NG = SR / 128;                    // logical 32-k groups per stage
  constexpr int RPI = 1024 / SR, CPR = SR / 16;   // tile rows per 1 KB DMA instruction, 16-byte chunks per stage row
  constexpr int D = NS - 1;
  constexpr int STAGE_BYTES = (BM + BN) * SR;
  constexpr int NINST = (BM + BN) / RPI;          // DMA instructions per stage
  static_assert(SR == 256 || SR == 128, "stage rows of 256 or 128 bytes");
  static_assert(NINST % NL == 0, "loader waves must divide the stage");
  constexpr int PER = NINST / NL;
  static_assert(PER * (D - 1 > 3 ? 3 : D - 1) <= 60, "vmcnt range");
  // pull the kernel-argument cache lines of this workgroup's problem into the scalar cache NOW, all in flight together: the epilogue reads
  // a dozen fields of it 20 us from here, and each first touch of a 64-byte line there is a dependent scalar-cache miss (l1gemm.hip's idiom)
  if (!(probe & 256)) kernarg_prefetch<(int)sizeof(GemmProb)>((int)(blockIdx.y * sizeof(GemmProb)));
  const GemmProb& P = batch.p[blockIdx.y];
  const int nwg = P.tiles_m * P.tiles_n;
  if ((int)blockIdx.x >= nwg) return;
  if (probe & 32) return;
  const int lid = xcd_remap(blockIdx.x, nwg);
  // (plain bf16 = the catalogue-wide products: few rows, 100k columns -- the row tiles of one weight panel side by side on one XCD)
  const int tile_n = X3 ? lid % P.tiles_n : lid / P.tiles_m, tile_m = X3 ? lid / P.tiles_n : lid % P.tiles_m;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  extern __shared__ __attribute__((aligned(16))) unsigned char dsmem[];
  const unsigned lds0 = (unsigned)(size_t)dsmem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nt0 = P.seg[0].K / KB;
  const int nt1 = P.nseg > 1 ? P.seg[1].K / KB : 0;
  const int nt = nt0 + nt1;

  if (wave >= NC) {
    // ------------------------------------------------------------ loader wave lw: instructions lw, lw + NL, ... of every stage
    const int lw = wave - NC;
    const int q_row = lane / CPR, q_pos = lane % CPR;
    const char* rp[PER];      // this lane's source address of instruction j at k = 0 of the current segment
    auto setup = [&](int sidx) {
      const GemmSeg& G = P.seg[sidx];
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int trow = (j * NL + lw) * RPI + q_row;        // row of the [A tile | B tile] stage image
        const bool isa = trow < BM;
        const int row = isa ? trow : trow - BM;
        const int c = SR == 256 ? (q_pos ^ (row & 15)) : (q_pos ^ ((row >> 1) & 7));
        const int gr = isa ? min(m0 + row, P.M - 1) : min(n0 + row, P.N - 1);
        rp[j] = (isa ? (const char*)G.A + (int64_t)gr * G.lda * 2 : (const char*)G.B + (int64_t)gr * G.ldb * 2) + c * 16;
      }
    };
    int cur = 0;
    setup(0);
    auto issue = [&](int t, int stage) {
      const int sidx = (t < nt0) ? 0 : 1;
      if (sidx != cur) { setup(sidx); cur = sidx; }
      const int koff = (sidx == 0 ? t : t - nt0) * (KB * 2);
      const unsigned sbase = lds0 + stage * STAGE_BYTES + lw * 1024;
#pragma unroll
      for (int j = 0; j < PER; ++j) dma16(rp[j] + koff, sbase + j * (NL * 1024));
    };
    const bool dma_on = !(probe & 2);
#pragma unroll
    for (int i = 0; i < D; ++i)
      if (i < nt && dma_on) issue(i, i);
    for (int t = 0; t < nt; ++t) {
      const int younger = min(D - 1, nt - 1 - t);
      if (younger >= 4 && 4 * PER <= 60) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * PER <= 60 ? 4 * PER : 0) : "memory");
      else if (younger >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * PER) : "memory");
      else if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PER) : "memory");
      else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();   // this wave's part of tile t has landed; the consumers are done with tile t - 1
      if (t + D < nt && dma_on) issue(t + D, (t + D) % NS);
    }
    return;
  }

  // -------------------------------------------------------------- consumer wave
  const int wm0 = (wave / WC) * 16 * TM, wn0 = (wave % WC) * 16 * TN;
  const int fr = lane & 15, fg = lane >> 4;
  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint4 sink = make_uint4(0, 0, 0, 0);
  // One fragment set: split bf16 -- one logical 32-k group = 64 physical k of every tile row of the wave (hi at chunk fg, lo at chunk
  // 4 + fg; three products); plain bf16 -- one 32-k group (chunk 4 g + fg; "l" unused; one product).
  static_assert(X3 || SR == 128, "the plain bf16 form is built for 128-byte stage rows");
  constexpr int SETS = X3 ? SR / 128 : SR / 64;   // fragment sets per k stage
  struct Frag { uint4 ah[TM], al[TM], bh[TN], bl[TN]; };
  auto load = [&](Frag& f, int t, int g) {
    const unsigned char* sa = dsmem + (t % NS) * STAGE_BYTES;
    const unsigned char* sb = sa + BM * SR;
    int ph, pl;
    if constexpr (SR == 256) { ph = ((g * 8 + fg) ^ fr) * 16; pl = ((g * 8 + 4 + fg) ^ fr) * 16; }
    else { const int sw = (fr >> 1) & 7; ph = (((X3 ? 0 : 4 * g) + fg) ^ sw) * 16; pl = ((4 + fg) ^ sw) * 16; }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      f.ah[tm] = *(const uint4*)(sa + (wm0 + tm * 16 + fr) * SR + ph);
      if constexpr (X3) f.al[tm] = *(const uint4*)(sa + (wm0 + tm * 16 + fr) * SR + pl);
    }
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      f.bh[tn] = *(const uint4*)(sb + (wn0 + tn * 16 + fr) * SR + ph);
      if constexpr (X3) f.bl[tn] = *(const uint4*)(sb + (wn0 + tn * 16 + fr) * SR + pl);
    }
  };
  auto mult = [&](const Frag& f) {
    // product-major, so that consecutive MFMAs never share an accumulator.  Split bf16: x3_mfma's three products (lo.hi, hi.lo, hi.hi: x3.h),
    // plain bf16: the one product; weights first in both (a lane owns 4 columns of one row: epilogue_fwd_x3).
#pragma unroll
    for (int p = 0; p < (X3 ? 3 : 1); ++p)
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
          if constexpr (X3) {
            const bf16x8 w = __builtin_bit_cast(bf16x8, p == 0 ? f.bl[tn] : f.bh[tn]);
            const bf16x8 x = __builtin_bit_cast(bf16x8, p == 1 ? f.al[tm] : f.ah[tm]);
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, x, acc[tm][tn], 0, 0, 0);
          } else {
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, f.bh[tn]), __builtin_bit_cast(bf16x8, f.ah[tm]),
                                                                  acc[tm][tn], 0, 0, 0);
          }
        }
  };
  // the stage barrier of the pipelined loops: this wave's reads of the tile before have all returned (they were issued a group of MFMAs
  // ago), so the loaders may overwrite its slot; behind the barrier the next tile is in LDS
  auto next_tile = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  // two fragment sets + the accumulators must fit the 170 registers a wave of a 768-thread workgroup may have (the 128 x 256 probe tile: no)
  constexpr bool PIPE = (TM + TN) * (X3 ? 16 : 8) + TM * TN * 4 <= 150;
  if (PIPE && !(probe & (512 | 4 | 8))) {   // (the read-only / MFMA-only probes time the unpipelined loop: a branch inside this one would
                                            // make the compiler wait for ALL outstanding reads in front of every MFMA group)
    // Software-pipelined over the fragment sets F[0] / F[1]: the reads of the NEXT set are in flight while the MFMAs of the current one
    // issue, across the stage barrier too.  (Round 5's first form read a group, waited, multiplied: the two consumer waves of a SIMD leave
    // every barrier in step, wait ~250 clk for their reads together and then queue 2 x 192 clk of MFMAs -- the matrix pipe ran at 60 %
    // inside the loop.)  Same MFMAs in the same order per accumulator: same bits.  sched_barrier: the compiler's scheduler otherwise
    // sinks every read to just in front of its first use to save registers.  The last tile(s) stand on their own: a conditional
    // barrier inside the loop joins two paths in front of a mult() and the compiler then waits for the reads just issued instead of the
    // ones it needs.
    Frag F[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int i = 0; i < TM; ++i) F[s].ah[i] = F[s].al[i] = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < TN; ++i) F[s].bh[i] = F[s].bl[i] = make_uint4(0, 0, 0, 0);
    }
    __builtin_amdgcn_s_barrier();       // every loader's part of tile 0 is in LDS
    if (probe & 1) {
      for (int t = 1; t < nt; ++t) __builtin_amdgcn_s_barrier();
    } else if constexpr (SETS == 2) {   // two sets per tile
      load(F[0], 0, 0);
      for (int t = 0; t + 1 < nt; ++t) {
        load(F[1], t, 1);
        __builtin_amdgcn_sched_barrier(0);
        mult(F[0]);
        __builtin_amdgcn_sched_barrier(0);
        next_tile();
        load(F[0], t + 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        mult(F[1]);
        __builtin_amdgcn_sched_barrier(0);
      }
      load(F[1], nt - 1, 1);
      __builtin_amdgcn_sched_barrier(0);
      mult(F[0]);
      mult(F[1]);
    } else {                            // one set per tile; nt is even (K is a multiple of 128 physical k)
      static_assert(SETS == 1, "one or two fragment sets per stage");
      load(F[0], 0, 0);
      for (int t = 0; t + 2 < nt; t += 2) {
        next_tile();
        load(F[1], t + 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        mult(F[0]);
        __builtin_amdgcn_sched_barrier(0);
        next_tile();
        load(F[0], t + 2, 0);
        __builtin_amdgcn_sched_barrier(0);
        mult(F[1]);
        __builtin_amdgcn_sched_barrier(0);
      }
      next_tile();
      load(F[1], nt - 1, 0);
      __builtin_amdgcn_sched_barrier(0);
      mult(F[0]);
      mult(F[1]);
    }
  } else {
  uint4 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) ah[i] = al[i] = make_uint4(0, 0, 0, 0);
#pragma unroll
  for (int i = 0; i < TN; ++i) bh[i] = bl[i] = make_uint4(0, 0, 0, 0);
  for (int t = 0; t < nt; ++t) {
    __builtin_amdgcn_s_barrier();     // every loader's part of tile t is in LDS
    if (probe & 1) continue;
    const unsigned char* sa = dsmem + (t % NS) * STAGE_BYTES;
    const unsigned char* sb = sa + BM * SR;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      int ph, pl;
      if constexpr (SR == 256) { ph = ((g * 8 + fg) ^ fr) * 16; pl = ((g * 8 + 4 + fg) ^ fr) * 16; }
      else { const int sw = (fr >> 1) & 7; ph = (fg ^ sw) * 16; pl = ((4 + fg) ^ sw) * 16; }
      if (!(probe & 8)) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
          ah[tm] = *(const uint4*)(sa + (wm0 + tm * 16 + fr) * SR + ph);
          al[tm] = *(const uint4*)(sa + (wm0 + tm * 16 + fr) * SR + pl);
        }
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
          bh[tn] = *(const uint4*)(sb + (wn0 + tn * 16 + fr) * SR + ph);
          bl[tn] = *(const uint4*)(sb + (wn0 + tn * 16 + fr) * SR + pl);
        }
      }
      if (probe & 4) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) { sink.x ^= ah[tm].x ^ al[tm].y; sink.y ^= ah[tm].z ^ al[tm].w; }
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) { sink.z ^= bh[tn].x ^ bl[tn].y; sink.w ^= bh[tn].z ^ bl[tn].w; }
        continue;
      }
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
          if constexpr (X3) {
            acc[tm][tn] = x3_mfma(__builtin_bit_cast(bf16x8, bh[tn]), __builtin_bit_cast(bf16x8, bl[tn]), __builtin_bit_cast(bf16x8, ah[tm]),
                                  __builtin_bit_cast(bf16x8, al[tm]), acc[tm][tn]);   // (weights first: a lane owns 4 columns of one row)
          } else {
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bh[tn]), __builtin_bit_cast(bf16x8, ah[tm]), acc[tm][tn], 0, 0, 0);
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, bl[tn]), __builtin_bit_cast(bf16x8, al[tm]), acc[tm][tn], 0, 0, 0);
          }
        }
    }
  }
  }
  if (probe && (sink.x ^ sink.y ^ sink.z ^ sink.w) == 0x9E3779B9u) acc[0][0][0] += 1.f;
  if (probe & 16) {   // no epilogue (a never-taken store keeps EVERY accumulator alive)
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) t += (acc[i][j][0] + acc[i][j][1]) + (acc[i][j][2] + acc[i][j][3]);
    if (t == 12345.678f) ((float*)P.C)[0] = t;
    return;
  }
  // full tiles of split output leave through an LDS image of the tile (the ring is idle: every loader waited for its last DMA before
  // the last barrier): whole 1 KB wave stores instead of 8-byte ones.  Uniform per workgroup; the loaders have left (or are leaving:
  // a terminated wave does not take part in s_barrier).
  if constexpr (!X3) {
    // Plain output.  Full tiles: the RAW accumulators go into an fp32 LDS image of the tile (16 tight 16-byte stores per lane), then
    // the waves walk the image row-wise -- a lane takes four neighbouring columns of one row per step (its column group never changes:
    // bias loaded once), applies the forward epilogue element by element (the arithmetic of epilogue_fwd) and stores 16 (fp32) / 8
    // (bf16) bytes: a wave instruction covers two whole 512- / 256-byte tile rows.  The first form ran epilogue_fwd_x3's fully
    // unrolled body per (tm, tn) block here: 16 blocks x ~800 instructions, 12.5 of the 14.7 us a workgroup spent behind its k loop
    // (recnn_debug_ws_trace; 72 of the catalogue-wide product's 206 us).  Ragged tiles keep the direct form.
    constexpr int TPF = BN * 4 + 16;       // image row pitch: + 16 bytes against bank conflicts
    const int es = P.c_f32 ? 4 : 2;
    const bool st = m0 + BM <= P.M && n0 + BN <= P.N && !(((int64_t)P.ldc * es) & 15) && !((uintptr_t)P.C & 15) && !((uintptr_t)P.bias & 15) &&
                    BM * TPF <= NS * STAGE_BYTES && !P.dot_part && !(probe & 64);
    // (row pointer without TRACE_ROW's pin: a consumer wave has no DMA in flight that a stamp could drain)
    unsigned long long* trow = (trace && tid == 0) ? trace + (int64_t)blockIdx.x * 8 : nullptr;
    TRACE_STAMP(trow, 0);
    if (!st) {
      epilogue_fwd_x3<TM, TN, false>(P, acc, m0, n0, wm0, wn0, lane, lid * NC + wave);
      return;
    }
    __builtin_amdgcn_s_barrier();          // every consumer is done reading the last k stage
    TRACE_STAMP(trow, 1);
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
        *(f32x4*)(dsmem + (wm0 + tm * 16 + fr) * TPF + (wn0 + tn * 16 + fg * 4) * 4) = acc[tm][tn];
    TRACE_STAMP(trow, 2);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's part of the image is IN LDS (s_barrier alone does not wait for LDS writes)
    __builtin_amdgcn_s_barrier();
    TRACE_STAMP(trow, 3);
    constexpr int CPR = BN / 4;            // 4-column groups per tile row
    static_assert((NC * 64) % CPR == 0, "a lane keeps its column group");
    const int ch = (wave * 64 + lane) % CPR;
    const int nb = n0 + ch * 4;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (P.bias) bv = *(const f32x4*)(P.bias + nb);
    uint32_t key = 0;
    if (P.mask_mode == RECNN_MASK_HASH) key = mask_key(P.seed, (P.step_ptr ? *P.step_ptr : 0) + P.step_add, P.stream_id);
    // the problem's fields in registers (the kernel-argument loads would otherwise repeat in every step of the walk), and no memory
    // clobber on the stores (nothing in this kernel reads the output): the steps overlap
    const float* const addend = P.addend;
    const bf16_t* const yref = (const bf16_t*)P.yref;
    const uint8_t* const mask = P.mask;
    const int mask_mode = P.mask_mode, relu = P.relu, add_row_div = P.add_row_div, c_f32 = P.c_f32;
    const int64_t ld_add = P.ld_add, ldy = P.ldy, ld_mask = P.ld_mask, ldc = P.ldc;
    const float add_clip = P.add_clip, dx_scale = P.dx_scale;
    char* const Cb = (char*)P.C;
#pragma unroll 2
    for (int row = (wave * 64 + lane) / CPR; row < BM; row += NC * 64 / CPR) {
      const int m = m0 + row;
      const f32x4 a4 = *(const f32x4*)(dsmem + row * TPF + ch * 16);
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = a4[r] + bv[r];
      if (addend) {
        const int ma = add_row_div > 1 ? m / add_row_div : m;
        const float* ap = addend + (int64_t)ma * ld_add + nb;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += fminf(fmaxf(ap[r], -add_clip), add_clip);
      }
      if (relu) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
      }
      if (yref) {
        const bf16_t* yp = yref + (int64_t)m * ldy + nb;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = bf2f(yp[r]) > 0.f ? v[r] * dx_scale : 0.f;
      }
      if (mask_mode == RECNN_MASK_EXTERNAL) {
        const uint8_t* mp = mask + (int64_t)m * ld_mask + nb;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = mp[r] ? v[r] * 2.f : 0.f;
      } else if (mask_mode == RECNN_MASK_HASH) {
        const uint32_t word = mask_word(key, (uint32_t)(m >> 2), (uint32_t)(nb >> 2));
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = mask_keep(word, m & 3, r) ? v[r] * 2.f : 0.f;
      }
      char* dst = Cb + ((int64_t)m * ldc + nb) * es;
      if (c_f32) {
        const f32x4 o = {v[0], v[1], v[2], v[3]};
        asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst), "v"(o));   // write-through: the tile drains while the launch runs,
                                                                                  // not at its end (guide: publish-large)
      } else {
        typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
        const u32x2_t o = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
        asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(dst), "v"(o));
      }
    }
    if (trow) { TRACE_STAMP(trow, 4); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TRACE_STAMP(trow, 5); }
    return;
  }
  constexpr int TP = BN * 4 + X3_TILE_PITCH_PAD;            // bytes per tile row: 2 BN bf16 + a 16-byte skew against bank conflicts
  const bool staged = !P.c_f32 && !P.yref && m0 + BM <= P.M && n0 + BN <= P.N && !(P.ldc & 7) && !((uintptr_t)P.C & 15) && BM * TP <= NS * STAGE_BYTES &&
                      !(probe & 64);
  unsigned long long* trow = (trace && tid == 0) ? trace + (int64_t)blockIdx.x * 8 : nullptr;
  TRACE_STAMP(trow, 0);
  if (staged) __builtin_amdgcn_s_barrier();                 // every consumer is done reading the last k stage: the tile image may overwrite it
  TRACE_STAMP(trow, 1);
  if (staged && !((uintptr_t)P.bias & 15) && !((uintptr_t)P.dot_w & 15) && !(probe & 1024)) epilogue_x3_full_tile<TM, TN>(P, acc, m0, n0, wm0, wn0, lane, lid * NC + wave, dsmem, TP);
  else epilogue_fwd_x3<TM, TN>(P, acc, m0, n0, wm0, wn0, lane, lid * NC + wave, staged ? dsmem : nullptr, TP);
  TRACE_STAMP(trow, 2);
  if (staged) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's part of the image is IN LDS (s_barrier alone does not wait for LDS writes)
    __builtin_amdgcn_s_barrier();
    TRACE_STAMP(trow, 3);
    constexpr int CPR2 = BN * 4 / 16;                          // 16-byte chunks per tile row
    bf16_t* C = (bf16_t*)P.C + (int64_t)m0 * P.ldc + x3_col(n0);
    for (int idx = wave * 64 + lane; idx < BM * CPR2; idx += NC * 64) {
      const int row = idx / CPR2, ch = idx - row * CPR2;
      const uint4 v = *(const uint4*)(dsmem + row * TP + ch * 16);
      uint4* dst = (uint4*)(C + (int64_t)row * P.ldc + ch * 8);
      if (probe & 128) *dst = v;
      else { typedef unsigned u32x4_t __attribute__((ext_vector_type(4))); const u32x4_t vv = {v.x, v.y, v.z, v.w};
             asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst), "v"(vv) : "memory"); }   // write-through: the tile drains while the
                                                                                                 // launch runs, not at its end (guide: publish-large)
    }
    if (trow) { TRACE_STAMP(trow, 4); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TRACE_STAMP(trow, 5); }
  }
}

// ------------------------------------------------------------------ dW GEMM, LDS-DMA + transpose reads (bf16)
// dW[m][n] = sum_b dZ[b][m] * X[b][n], batch split into slabs (deterministic): the 64 x 64 tile itself is dw_tile.h; here the
// split-batch driver that writes one fp32 slab per batch slice (summed later by grad_reduce / the Adam pass).  The single-GPU step
// whose backward tensors come from mlpt.hip takes dwadam.hip instead (whole batch per tile, optimizer in the epilogue: no slabs).
constexpr int DW_SCALE_ROWS = 512;    // per-row scales of a workgroup's k range are staged in LDS up to this many rows
// one 32-row panel of one critic: per-column sums over the rows of d_r * {h2, u2, U}; thread = column
__device__ __forceinline__ void dw_vec_role(const DwVecProb& V, int panel) {
  const int m0 = panel * 32;
  if (m0 >= V.rows) return;
  for (int k = threadIdx.x; k < V.H; k += 256) {
    // four row chunks of 8, each an fma chain upwards, combined (c0 + c1) + (c2 + c3): the order of mlpt.hip's panel sums
    // (the chunk loop is NOT unrolled: 24 loads in flight; more would raise the kernel's VGPR count and cost the GEMM tiles
    // their occupancy -- 96 in flight made the whole dW launch 18 us instead of 10)
    float c3[4], c2[4], c1[4];
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
      float s3 = 0.f, s2 = 0.f, s1 = 0.f;
#pragma unroll
      for (int r = c * 8; r < c * 8 + 8; ++r) {
        const int m = min(m0 + r, V.rows - 1);
        const float d = m0 + r < V.rows ? V.delta[m] : 0.f;
        const int64_t off = (int64_t)m * V.ldh + k;
        s3 = fmaf(d, bf2f(((const bf16_t*)V.h2)[off]), s3);
        s2 = fmaf(d, bf2f(((const bf16_t*)V.u2)[off]), s2);
        s1 = fmaf(d, bf2f(((const bf16_t*)V.U)[off]), s1);
      }
      c3[c] = s3; c2[c] = s2; c1[c] = s1;
    }
    const float s3 = (c3[0] + c3[1]) + (c3[2] + c3[3]), s2 = (c2[0] + c2[1]) + (c2[2] + c2[3]), s1 = (c1[0] + c1[1]) + (c1[2] + c1[3]);
    V.dw3_part[(int64_t)panel * V.H + k] = s3;
    V.db2_part[(int64_t)panel * V.H + k] = s2;
    V.colsum[(int64_t)panel * V.H + k] = s1;
  }
}

// SUB = batch rows per stage, NS = ring slots (all filled before the first MFMA).
template <int SUB, int NS> __global__ __launch_bounds__(256) void gemm_dw_dma_kernel(const GemmBatch batch, const DwVec vec, const int nprob) {
  // (no kernarg prefetch here: measured +0.4 us on this launch -- 736 short workgroups each paying the wait; round 5)
  // extra workgroups, first in the launch order (their chain of row loads is the longest single-workgroup path):
  // row-vector partial sums for the bias / last-layer gradients
  const int y0 = vec.n > 0 ? 1 : 0;
  if (y0 && blockIdx.y == 0) {
    const int vb = blockIdx.x;
    if (vb < vec.n * ((vec.p[0].rows + 31) / 32)) dw_vec_role(vec.p[vb % vec.n], vb / vec.n);
    return;
  }
  (void)nprob;
  const GemmProb& P = batch.p[(int)blockIdx.y - y0];
  const int nwg = P.tiles_m * P.tiles_n * P.dw_splits;
  if ((int)blockIdx.x >= nwg) return;
  const int lid = xcd_remap(blockIdx.x, nwg);
  const int tile_n = lid % P.tiles_n;
  const int tile_m = (lid / P.tiles_n) % P.tiles_m;
  const int split = lid / (P.tiles_n * P.tiles_m);
  const int m0 = tile_m * 64, n0 = tile_n * 64;

  extern __shared__ __attribute__((aligned(16))) unsigned char dsmem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
  const int fr = lane & 15, fg = lane >> 4;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int Kc = P.seg[0].K;
  const int chunk = (((Kc + P.dw_splits - 1) / P.dw_splits) + 63) / 64 * 64;
  const int kbeg = split * chunk;
  const int kend = min(Kc, kbeg + chunk);
  dw_tile_accumulate<SUB, NS, 1>(P, m0, n0, kbeg, kend, dsmem, DW_SCALE_ROWS, acc, [] {});

  float* Cs = (float*)P.C + (int64_t)split * P.dw_slab_stride;
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int n = n0 + wn0 + tn * 16 + fr;
      const int mb = m0 + wm0 + tm * 16 + fg * 4;
      if (n < P.dw_valid_cols) {
        int cc = n + P.dw_col_rot;
        if (cc >= P.dw_valid_cols) cc -= P.dw_valid_cols;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = mb + r;
          if (m < P.M) Cs[(int64_t)m * P.ldc + cc] = acc[tm][tn][r];
        }
      }
    }
}

static const GemmTune kDefaultTune;
static inline const GemmTune& tune_of(const GemmLaunch* L) { return L->tune ? *L->tune : kDefaultTune; }

// both operands bf16 in memory, 64-column tiles readable inside the row pitch (padding columns may hold anything:
// they only reach outputs that are never written)
static bool dw_dma_eligible(const GemmLaunch* L) {
  if (!tune_of(L).dw_dma || L->mode != GEMM_DW || L->dtype != RECNN_BF16 || L->a_f32 || L->b_f32) return false;
  for (int i = 0; i < L->nprob; ++i) {
    const GemmProb& p = L->batch.p[i];
    if (p.nseg != 1 || p.seg[0].K <= 0) return false;
    if (p.seg[0].lda < (p.M + 63) / 64 * 64 || p.seg[0].ldb < (p.N + 63) / 64 * 64) return false;
  }
  return true;
}

template <int SUB, int NS> static int launch_dw_dma_v(GemmLaunch* L, hipStream_t stream) {
  constexpr int LDS = NS * SUB * 256 + DW_SCALE_ROWS * 4;
  static bool attr_done = false;
  if (!attr_done) {
    int rc = recnn_check_hip(hipFuncSetAttribute((const void*)gemm_dw_dma_kernel<SUB, NS>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS),
                             "gemm dw dma attr");
    if (rc) return rc;
    attr_done = true;
  }
  int maxwg = 0;
  for (int i = 0; i < L->nprob; ++i) {
    GemmProb& p = L->batch.p[i];
    p.tiles_m = (p.M + 63) / 64;
    p.tiles_n = (p.N + 63) / 64;
    const int nwg = p.tiles_m * p.tiles_n * p.dw_splits;
    if (nwg > maxwg) maxwg = nwg;
  }
  if (maxwg == 0) return 0;
  DwVec vec;
  memset(&vec, 0, sizeof(vec));
  int extra = 0;
  if (L->vec && L->vec->n > 0) {
    vec = *L->vec;
    extra = 1;
    const int vb = vec.n * ((vec.p[0].rows + 31) / 32);
    if (vb > maxwg) maxwg = vb;
  }
  hipLaunchKernelGGL((gemm_dw_dma_kernel<SUB, NS>), dim3(maxwg, L->nprob + extra, 1), dim3(256, 1, 1), LDS, stream, L->batch, vec, L->nprob);
  return recnn_check_hip(hipGetLastError(), "gemm_dw_dma_kernel launch");
}
static int launch_dw_dma(GemmLaunch* L, hipStream_t stream, int variant = 0) {
  switch (variant ? variant : tune_of(L).dw_dma) {
    case 2: return launch_dw_dma_v<64, 2>(L, stream);
    case 3: return launch_dw_dma_v<64, 3>(L, stream);
    case 4: return launch_dw_dma_v<64, 4>(L, stream);
    case 5: return launch_dw_dma_v<32, 2>(L, stream);
    case 6: return launch_dw_dma_v<32, 4>(L, stream);
    case 7: return launch_dw_dma_v<32, 3>(L, stream);
    case 1: return launch_dw_dma_v<128, 2>(L, stream);
    default: return launch_dw_dma_v<64, 2>(L, stream);
  }
}

// ------------------------------------------------------------------ host side
void gemm_prob_init(GemmProb* p) {
  memset(p, 0, sizeof(*p));
  p->nseg = 1;
  p->dx_scale = 1.f;
  p->dw_splits = 1;
}

// Tile variants: 0 = 64x64 block tile, short k stage; 1 = 32x64 block tile, 2x longer k stage (more, smaller
// workgroups with more bytes in flight each: these GEMMs have M = batch rows only, so they are latency bound).



template <class TC, int MODE, bool A32, bool B32, int TM, int TN, int KB, int NW>
static int launch_v(GemmLaunch* L, hipStream_t stream) {
  constexpr int BM = 32 * TM, BN = 16 * TN * (NW / 2);
  int maxwg = 0;
  for (int i = 0; i < L->nprob; ++i) {
    GemmProb& p = L->batch.p[i];
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.N + BN - 1) / BN;
    int splits = (MODE == GEMM_DW) ? p.dw_splits : 1;
    int nwg = p.tiles_m * p.tiles_n * splits;
    p.dot_parts = nwg * NW;
    if (nwg > maxwg) maxwg = nwg;
  }
  if (maxwg == 0) return 0;
  dim3 grid(maxwg, L->nprob, 1), block(NW * 64, 1, 1);
  hipLaunchKernelGGL((gemm_kernel<TC, MODE, A32, B32, TM, TN, KB, false, NW>), grid, block, 0, stream, L->batch);
  return recnn_check_hip(hipGetLastError(), "gemm_kernel launch");
}




template <class TC, int NS, int NW> static int launch_dma_nw(GemmLaunch* L, hipStream_t stream) {
  constexpr int TM = 1, TN = (NW == 8 ? 1 : 2), BM = 32 * TM, BN = 16 * TN * (NW / 2);
  constexpr int LDS = NS * (BM + BN) * 256;
  static bool attr_done = false;
  if (!attr_done) {
    int rc = recnn_check_hip(hipFuncSetAttribute((const void*)gemm_fwd_dma_kernel<TC, TM, TN, NS, NW>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, LDS), "gemm dma attr");
    if (rc) return rc;
    attr_done = true;
  }
  int maxwg = 0;
  for (int i = 0; i < L->nprob; ++i) {
    GemmProb& p = L->batch.p[i];
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.N + BN - 1) / BN;
    const int nwg = p.tiles_m * p.tiles_n;
    p.dot_parts = nwg * NW;
    if (nwg > maxwg) maxwg = nwg;
  }
  if (maxwg == 0) return 0;
  hipLaunchKernelGGL((gemm_fwd_dma_kernel<TC, TM, TN, NS, NW>), dim3(maxwg, L->nprob, 1), dim3(NW * 64, 1, 1), LDS, stream, L->batch);
  return recnn_check_hip(hipGetLastError(), "gemm_fwd_dma_kernel launch");
}

// split-bf16 forward (x3.h), 8 waves.  Every tile streams (BM + BN) x 256 bytes per 64 logical k through one CU's L2 -> LDS path
// (~41 B / clk): the launch time is (tiles x bytes per tile) / (CUs x rate), so the tile should be as large as still gives
// every CU a workgroup -- 64 x 128 (wave tile 32 x 32: 8 fragment reads per 12 MFMAs) for the grouped layer-1 / layer-2
// launches (256 tiles at 2048 rows x 4 networks), 32 x 64 for the small ones.
template <int TM, int TN, int NS, int NW = 8> static int launch_dma_x3(GemmLaunch* L, hipStream_t stream) {
  constexpr int BM = 32 * TM, BN = 16 * TN * (NW / 2);
  constexpr int LDS = NS * (BM + BN) * 256;
  static bool attr_done = false;
  if (!attr_done) {
    int rc = recnn_check_hip(hipFuncSetAttribute((const void*)gemm_fwd_dma_kernel<bf16_t, TM, TN, NS, NW, true>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, LDS), "gemm x3 dma attr");
    if (rc) return rc;
    attr_done = true;
  }
  int maxwg = 0;
  for (int i = 0; i < L->nprob; ++i) {
    GemmProb& p = L->batch.p[i];
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.N + BN - 1) / BN;
    const int nwg = p.tiles_m * p.tiles_n;
    p.dot_parts = nwg * NW;
    if (nwg > maxwg) maxwg = nwg;
  }
  if (maxwg == 0) return 0;
  hipLaunchKernelGGL((gemm_fwd_dma_kernel<bf16_t, TM, TN, NS, NW, true>), dim3(maxwg, L->nprob, 1), dim3(NW * 64, 1, 1), LDS, stream, L->batch);
  return recnn_check_hip(hipGetLastError(), "gemm_fwd_dma_kernel (x3) launch");
}
static unsigned long long* g_ws_trace = nullptr;   // recnn_debug_ws_trace: [workgroup][8] shader-clock stamps of the plain-bf16 epilogue
extern "C" void recnn_debug_ws_trace(void* p) { g_ws_trace = (unsigned long long*)p; }
static int g_x3_ws_probe = 0;    // recnn_debug_x3_ws_probe (csrc/recnn_hip_debug.h)
extern "C" void recnn_debug_x3_ws_probe(int bits) { g_x3_ws_probe = bits; }
template <int TM, int TN, int WR, int WC, int NL, int NS, int SR = 256, bool X3 = true> static int launch_x3_ws(GemmLaunch* L, hipStream_t stream) {
  constexpr int NC = WR * WC, BM = 16 * TM * WR, BN = 16 * TN * WC;
  constexpr int LDS = NS * (BM + BN) * SR;
  static bool attr_done = false;
  if (!attr_done) {
    int rc = recnn_check_hip(hipFuncSetAttribute((const void*)x3_fwd_ws_kernel<TM, TN, WR, WC, NL, NS, SR, X3>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, LDS), "gemm x3 ws attr");
    if (rc) return rc;
    attr_done = true;
  }
  int maxwg = 0;
  for (int i = 0; i < L->nprob; ++i) {
    GemmProb& p = L->batch.p[i];
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.N + BN - 1) / BN;
    const int nwg = p.tiles_m * p.tiles_n;
    p.dot_parts = nwg * NC;
    if (nwg > maxwg) maxwg = nwg;
  }
  if (maxwg == 0) return 0;
  hipLaunchKernelGGL((x3_fwd_ws_kernel<TM, TN, WR, WC, NL, NS, SR, X3>), dim3(maxwg, L->nprob, 1), dim3((NC + NL) * 64, 1, 1), LDS, stream, L->batch, g_x3_ws_probe, g_ws_trace);
  return recnn_check_hip(hipGetLastError(), "x3_fwd_ws_kernel launch");
}
static int g_x3_fwd_debug = -1;   // recnn_debug_x3_fwd (csrc/recnn_hip_debug.h): overrides GemmTune::x3_fwd, probes only
extern "C" void recnn_debug_x3_fwd(int v) { g_x3_fwd_debug = v; }
static constexpr int g_x3_big_min_wg = 192;   // launches with at least this many 64 x 128 tiles take them
int x3_fwd_launch(GemmLaunch* L, hipStream_t stream) {
  for (int i = 0; i < L->nprob; ++i) {
    const GemmProb& p = L->batch.p[i];
    for (int s = 0; s < p.nseg; ++s)
      if (p.seg[s].K % 128) { recnn_set_error("gemm fwd (bf16x3): physical K=%d is not a multiple of 128", p.seg[s].K); return RECNN_E_UNSUPPORTED; }
    if (!p.c_f32 && p.ldc < x3_ld(p.N)) { recnn_set_error("gemm fwd (bf16x3): ldc=%lld below the split row width %lld", (long long)p.ldc, (long long)x3_ld(p.N)); return RECNN_E_INVALID; }
  }
  long wg = 0, wg_big = 0;
  for (int i = 0; i < L->nprob; ++i) {
    wg += (long)((L->batch.p[i].M + 31) / 32) * ((L->batch.p[i].N + 63) / 64);
    wg_big += (long)((L->batch.p[i].M + 63) / 64) * ((L->batch.p[i].N + 127) / 128);
  }
  // Measured (DDPG, 2048 rows, 4 networks' layer 1 = 256 tiles of 64 x 128): 27.9 us with 16 waves, 29.4 with 8 (wave tile 32 x 32),
  // 31.5 as 1024 tiles of 32 x 64, 42.5 as 128 tiles of 128 x 128 -- the launch moves 290 MB (590 MB in the small tiling) through
  // L2 -> LDS at 10-19 TB/s whatever the tile: what is left is the memory system, not the tile shape (profiles/NOTES_r01_r05.md 5d).
  // Counters (profiles/r04_x3_pmc.txt): matrix cores 25 % busy, LDS array 25 % busy, no bank conflicts -- the time goes into ISSUING
  // the LDS-DMA (one 1 KB global_load_lds_dwordx4 ~ 60 clk of CU-serial issue: 48 per 64-k stage of this tile = 1440 clk per 32
  // logical k, 1680 observed).  Tried instead: every wave loading its own MFMA fragments straight from L2 into registers (16-byte
  // loads, 16 rows x 64 B per instruction, 3 steps ahead, no LDS): bit-identical and 3.5x SLOWER (202 us / step against 117) -- a
  // wave instruction that touches 16 lines costs far more than one that touches 8 contiguous ones.  Removed again.
  // Kernel choice (GemmTune::x3_fwd; all compute the same bits).  2 (default): the wave-specialised kernel -- 64 x 128 tiles for launches
  // that fill the machine with them, else 32 x 64 tiles with a 3-stage ring (72 KB: two workgroups share a CU) above 320 tiles and a
  // 5-stage ring below.  Measured in the step's run graphs (profiles/r05_x3_fwd_ab.txt): 113.6 us/step with 0, 111.1 with 11 (only the
  // big launches), 108.6 with 2.  7 / 8: 128 x 128 and 128 x 256 tiles on 128-byte stage rows for cycle-sized M -- no faster per row
  // than 64 x 128 at M = 20480 (profiles/r05_x3_ws_big_tiles_m20480.txt: the consumer waves, not the bytes, bound those), kept for
  // tools/x3_fwd_probe.py.
  const int var = g_x3_fwd_debug >= 0 ? g_x3_fwd_debug : tune_of(L).x3_fwd;
  const bool big = L->nprob > 0 && wg_big >= g_x3_big_min_wg;
  switch (var) {
    case 2: if (big) return launch_x3_ws<2, 2, 2, 4, 4, 3>(L, stream);
            if (wg > 320) return launch_x3_ws<1, 2, 2, 2, 4, 3>(L, stream);
            return launch_x3_ws<1, 2, 2, 2, 4, 5>(L, stream);
    case 11: if (big) return launch_x3_ws<2, 2, 2, 4, 4, 3>(L, stream); break;   // small launches stay on the round-4 kernel
    case 7: return launch_x3_ws<4, 2, 2, 4, 4, 4, 128>(L, stream);    // 128 x 128, wave tile 64 x 32
    case 8: return launch_x3_ws<4, 4, 2, 4, 4, 3, 128>(L, stream);    // 128 x 256, wave tile 64 x 64
    default: break;
  }
  if (big) return launch_dma_x3<2, 1, 3, 16>(L, stream);
  if (L->nprob == 0 || wg <= 320) return launch_dma_x3<1, 1, 5>(L, stream);
  return launch_dma_x3<1, 1, 3>(L, stream);
}

// Catalogue-wide forward products ([256, 2048] x [2048, 100k], recnn/nn/models.py:93-95 at a 100k-item catalogue): 128 x 128
// tiles (wave tile 64 x 32: 6 fragment reads per 8 MFMAs), two 64 KB ring stages, row tiles fastest.  The 32 x 64 tile tuned
// for the 256-wide MLPs streams 4.5 GB through L2 -> LDS for this shape (0.093 of the bf16 peak, round 3); this one 1.6 GB.
// Round 5: in bf16 with more than 128 rows (REINFORCE's 256-row batches) the wave-specialised kernel takes them as 256 x 128 tiles -- the
// whole batch against one weight panel: the panel goes L2 -> LDS once instead of twice (1.2 GB per product instead of 1.6), 4 loader waves
// stream 48 KB stages of 128-byte rows through a 3-slot ring, 8 consumer waves (wave tile 64 x 64: 8 fragment reads per 16 MFMAs) multiply,
// software-pipelined.  Same products in the same k order: bit-identical to the 128 x 128 form (tests/test_gpu_reinforce.py).
static int g_wide_ws = 1;   // recnn_debug_wide_ws (csrc/recnn_hip_debug.h): 0 = the 128 x 128 kernel everywhere (A/B runs)
extern "C" void recnn_debug_wide_ws(int on) { g_wide_ws = on; }
template <class TC> static int launch_dma_wide(GemmLaunch* L, hipStream_t stream) {
  if constexpr (sizeof(TC) == 2) {
    bool tall = g_wide_ws != 0 && L->nprob > 0;
    for (int i = 0; i < L->nprob; ++i) tall = tall && L->batch.p[i].M > 128 && !L->batch.p[i].dot_part;
    if (tall) switch (g_wide_ws) {
      case 2: return launch_x3_ws<4, 2, 2, 4, 4, 4, 128, false>(L, stream);   // 128 x 128, 4 stages
      case 3: return launch_x3_ws<2, 4, 2, 4, 4, 4, 128, false>(L, stream);   //  64 x 256, 4 stages
      case 4: return launch_x3_ws<4, 4, 2, 4, 4, 3, 128, false>(L, stream);   // 128 x 256, 3 stages
      case 5: return launch_x3_ws<2, 2, 2, 4, 4, 6, 128, false>(L, stream);   //  64 x 128, 6 stages
      default: return launch_x3_ws<4, 4, 4, 2, 4, 3, 128, false>(L, stream);  // 256 x 128, 3 stages
    }
  }
  constexpr int TM = 4, TN = 2, NS = 2, NW = 8, BM = 128, BN = 128;
  constexpr int LDS = NS * (BM + BN) * 256;
  static bool attr_done = false;
  if (!attr_done) {
    int rc = recnn_check_hip(hipFuncSetAttribute((const void*)gemm_fwd_dma_kernel<TC, TM, TN, NS, NW, false, true>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, LDS), "gemm dma wide attr");
    if (rc) return rc;
    attr_done = true;
  }
  int maxwg = 0;
  for (int i = 0; i < L->nprob; ++i) {
    GemmProb& p = L->batch.p[i];
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.N + BN - 1) / BN;
    const int nwg = p.tiles_m * p.tiles_n;
    p.dot_parts = nwg * NW;
    if (nwg > maxwg) maxwg = nwg;
  }
  if (maxwg == 0) return 0;
  hipLaunchKernelGGL((gemm_fwd_dma_kernel<TC, TM, TN, NS, NW, false, true>), dim3(maxwg, L->nprob, 1), dim3(NW * 64, 1, 1), LDS, stream, L->batch);
  return recnn_check_hip(hipGetLastError(), "gemm_fwd_dma_kernel (wide) launch");
}

// ------------------------------------------------------------------ split-K forward (long contraction, few output tiles)
// [256, 2048] x K = 100k (REINFORCE: d loss / d hidden = dlogits x W2 over the catalogue, and the critic's first layer over action
// distributions, recnn/nn/models.py:93-95, 207-209) is 32 tiles of 128 x 128: one workgroup per tile leaves 7/8 of the machine
// idle and walks 100k k each (448 us with the 32 x 64 tiling).  Here K is cut into S <= 8 slices, slice s a grouped problem of the
// wide kernel that writes its raw fp32 partial product; splitk_finish_kernel sums the slices in slice order (deterministic) and
// applies the forward epilogue -- the arithmetic of epilogue_fwd, element by element.
template <class TC>
__global__ __launch_bounds__(256) void splitk_finish_kernel(const GemmProb P, const float* __restrict__ ws, int S, int64_t stride) {
  const int n4 = (P.N + 3) / 4;
  const int64_t total = (int64_t)P.M * n4;
  uint32_t key = 0;
  if (P.mask_mode == RECNN_MASK_HASH) key = mask_key(P.seed, (P.step_ptr ? *P.step_ptr : 0) + P.step_add, P.stream_id);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int m = (int)(i / n4), nb = (int)(i - (int64_t)m * n4) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const bool vec = nb + 3 < P.N && !(P.N & 3);
    for (int s = 0; s < S; ++s) {
      const float* src = ws + s * stride + (int64_t)m * P.N + nb;
      if (vec) { const float4 t = *(const float4*)src; v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w; }
      else for (int r = 0; r < 4; ++r) if (nb + r < P.N) v[r] += src[r];
    }
    uint32_t word = 0;
    if (P.mask_mode == RECNN_MASK_HASH) word = mask_word(key, (uint32_t)(m >> 2), (uint32_t)(nb >> 2));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = nb + r;
      if (n >= P.N) break;
      float x = v[r] + (P.bias ? P.bias[n] : 0.f);
      if (P.addend) {
        const int ma = P.add_row_div > 1 ? m / P.add_row_div : m;
        const float z = P.addend[(int64_t)ma * P.ld_add + n];
        x += fminf(fmaxf(z, -P.add_clip), P.add_clip);
      }
      if (P.relu) x = fmaxf(x, 0.f);
      if (P.yref) {
        const float y = tc_load((const TC*)P.yref + (int64_t)m * P.ldy + n);
        x = y > 0.f ? x * P.dx_scale : 0.f;
      }
      if (P.mask_mode == RECNN_MASK_EXTERNAL) x = P.mask[(int64_t)m * P.ld_mask + n] ? x * 2.f : 0.f;
      else if (P.mask_mode == RECNN_MASK_HASH) x = mask_keep(word, m & 3, r) ? x * 2.f : 0.f;
      if (P.c_f32) ((float*)P.C)[(int64_t)m * P.ldc + n] = x;
      else tc_store((TC*)P.C + (int64_t)m * P.ldc + n, x);
    }
  }
}

constexpr int SPLITK_MIN_K = 32768, SPLITK_MAX_TILES = 64;
template <class TC> static bool splitk_wanted(const GemmLaunch* L) {
  if (L->nprob != 1 || !L->ws) return false;
  const GemmProb& p = L->batch.p[0];
  if (p.nseg != 1 || p.seg[0].K < SPLITK_MIN_K || p.M < 128 || p.dot_part || p.dot_w) return false;
  const long tiles = (long)((p.M + 127) / 128) * ((p.N + 127) / 128);
  return tiles <= SPLITK_MAX_TILES;
}
template <class TC> static int launch_dma_splitk(GemmLaunch* L, hipStream_t stream) {
  const GemmProb P = L->batch.p[0];
  constexpr int ES = sizeof(TC), KB = 256 / ES;
  const int tiles = ((P.M + 127) / 128) * ((P.N + 127) / 128);
  const int nstage = P.seg[0].K / KB;
  int S = 256 / tiles;
  S = S > GEMM_MAX_GROUP ? GEMM_MAX_GROUP : S;
  const int per = (nstage + S - 1) / S;
  S = (nstage + per - 1) / per;
  const int64_t stride = (int64_t)P.M * P.N;
  if (S < 2 || S * stride * 4 > L->ws_bytes) return launch_dma_wide<TC>(L, stream);
  GemmLaunch L2 = *L;
  L2.nprob = S;
  L2.ws = nullptr;
  for (int s = 0; s < S; ++s) {
    GemmProb& q = L2.batch.p[s];
    q = P;
    const int st0 = s * per, cnt = (st0 + per <= nstage ? per : nstage - st0);
    q.seg[0].A = (const char*)P.seg[0].A + (int64_t)st0 * 256;
    q.seg[0].B = (const char*)P.seg[0].B + (int64_t)st0 * 256;
    q.seg[0].K = cnt * KB;
    q.C = L->ws + s * stride; q.ldc = P.N; q.c_f32 = 1;
    q.bias = nullptr; q.relu = 0; q.mask_mode = RECNN_MASK_NONE; q.addend = nullptr; q.yref = nullptr;
  }
  int rc = launch_dma_wide<TC>(&L2, stream);
  if (rc) return rc;
  const int64_t total = (int64_t)P.M * ((P.N + 3) / 4);
  const int grid = (int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
  hipLaunchKernelGGL(splitk_finish_kernel<TC>, dim3(grid), dim3(256), 0, stream, P, (const float*)L->ws, S, stride);
  return recnn_check_hip(hipGetLastError(), "splitk_finish_kernel launch");
}

template <class TC, int NS> static int launch_dma_ns(GemmLaunch* L, hipStream_t stream) {
  if (tune_of(L).dma_waves == 8 && L->nprob > 0) return launch_dma_nw<TC, NS, 8>(L, stream);
  return launch_dma_nw<TC, NS, 4>(L, stream);
}

// Ring depth by launch size: a launch with at most ~1 workgroup per CU keeps 4 k stages in flight per workgroup
// (5-stage ring, 120 KB of LDS); bigger grouped launches use the 3-stage ring so that 2 workgroups share a CU.
template <class TC> static int launch_dma(GemmLaunch* L, hipStream_t stream) {
  if (splitk_wanted<TC>(L)) return launch_dma_splitk<TC>(L, stream);
  if (L->nprob == 1 && L->batch.p[0].N >= 8192 && L->batch.p[0].M >= 128 && !L->batch.p[0].dot_part) return launch_dma_wide<TC>(L, stream);
  long wg = 0;
  for (int i = 0; i < L->nprob; ++i) wg += (long)((L->batch.p[i].M + 31) / 32) * ((L->batch.p[i].N + 63) / 64);
  if (L->nprob == 0 || (tune_of(L).dma_deep && wg <= 320)) return launch_dma_ns<TC, 5>(L, stream);
  return launch_dma_ns<TC, 3>(L, stream);
}

// the DMA pipeline needs both operands stored in the compute type and whole 256-byte k stages
template <class TC> static bool dma_eligible(const GemmLaunch* L) {
  if (!tune_of(L).dma || L->mode != GEMM_FWD) return false;
  if (sizeof(TC) == 2 && (L->a_f32 || L->b_f32)) return false;
  const int KB = 256 / (int)sizeof(TC);
  for (int i = 0; i < L->nprob; ++i)
    for (int s = 0; s < L->batch.p[i].nseg; ++s)
      if (L->batch.p[i].seg[s].K % KB) return false;
  return true;
}

// make the one-time function attribute calls outside of any stream capture
int gemm_init() {
  GemmLaunch L;
  memset(&L, 0, sizeof(L));
  int rc;
  L.mode = GEMM_DW;
  for (int v = 1; v <= 7; ++v)
    if ((rc = launch_dw_dma(&L, nullptr, v))) return rc;
  L.mode = GEMM_FWD;
  if ((rc = launch_dma_nw<float, 3, 4>(&L, nullptr))) return rc;
  if ((rc = launch_dma_nw<float, 5, 4>(&L, nullptr))) return rc;
  if ((rc = launch_dma_nw<bf16_t, 3, 4>(&L, nullptr))) return rc;
  if ((rc = launch_dma_nw<bf16_t, 5, 4>(&L, nullptr))) return rc;
  if ((rc = launch_dma_wide<float>(&L, nullptr))) return rc;
  if ((rc = launch_dma_wide<bf16_t>(&L, nullptr))) return rc;
  if ((rc = launch_dma_nw<float, 3, 8>(&L, nullptr))) return rc;
  if ((rc = launch_dma_nw<float, 5, 8>(&L, nullptr))) return rc;
  if ((rc = launch_dma_nw<bf16_t, 3, 8>(&L, nullptr))) return rc;
  if ((rc = launch_dma_x3<1, 1, 3>(&L, nullptr))) return rc;
  if ((rc = launch_dma_x3<1, 1, 5>(&L, nullptr))) return rc;
  if ((rc = launch_dma_x3<2, 1, 3, 16>(&L, nullptr))) return rc;
  if ((rc = x3_init())) return rc;
  return launch_dma_nw<bf16_t, 5, 8>(&L, nullptr);
}

template <class TC, int MODE, bool A32, bool B32>
static int launch_t(GemmLaunch* L, hipStream_t stream) {
  constexpr int KB0 = TcTraits<TC>::BK;
  if constexpr (MODE == GEMM_FWD && !A32 && !B32) {
    if (dma_eligible<TC>(L)) return launch_dma<TC>(L, stream);
  }
  if constexpr (MODE == GEMM_DW && sizeof(TC) == 2 && !A32 && !B32) {
    if (dw_dma_eligible(L)) return launch_dw_dma(L, stream);
  }
  if constexpr (MODE == GEMM_DW) {
    bool scaled = L->vec != nullptr;
    for (int i = 0; i < L->nprob; ++i) scaled = scaled || L->batch.p[i].a_row_scale != nullptr;
    if (scaled) { recnn_set_error("gemm dw: row scaling / vector partials need the bf16 DMA kernel"); return RECNN_E_UNSUPPORTED; }
  }
  int v = tune_of(L).variant;
  if (v < 0) {  // enough 64x64 tiles to give every CU a few workgroups?  else take the small-tile variant
    long wg = 0;
    for (int i = 0; i < L->nprob; ++i) {
      const GemmProb& p = L->batch.p[i];
      wg += (long)((p.M + 63) / 64) * ((p.N + 63) / 64) * (MODE == GEMM_DW ? p.dw_splits : 1);
    }
    v = wg >= tune_of(L).v0_min_wg ? 0 : 1;
  }
  // same block tiles with 4 waves (2x2) or 8 waves (2x4): more waves = more loads in flight per CU
  // (measured: dX 7.5 -> 6.5 us with 8 waves, the dW launch 14 -> 19.5 us: its k-strided loads are spread too thin)
  if (tune_of(L).waves == 8 && MODE != GEMM_DW) {
    if (v == 0) return launch_v<TC, MODE, A32, B32, 2, 1, KB0, 8>(L, stream);
    return launch_v<TC, MODE, A32, B32, 1, 1, 2 * KB0, 8>(L, stream);
  }
  if (v == 0) return launch_v<TC, MODE, A32, B32, 2, 2, KB0, 4>(L, stream);
  return launch_v<TC, MODE, A32, B32, 1, 2, 2 * KB0, 4>(L, stream);
}

template <class TC, int MODE> static int launch_m(GemmLaunch* L, hipStream_t s) {
  if (sizeof(TC) == 4) return launch_t<TC, MODE, false, false>(L, s);
  // bf16: operands may be fp32 in memory.  Only the combinations the engine uses are built.
  if (MODE == GEMM_FWD) {
    if (L->b_f32) { recnn_set_error("gemm fwd: B must be tc"); return RECNN_E_UNSUPPORTED; }
    return L->a_f32 ? launch_t<TC, MODE, true, false>(L, s) : launch_t<TC, MODE, false, false>(L, s);
  }
  if (MODE == GEMM_DX) {
    if (L->a_f32 || L->b_f32) { recnn_set_error("gemm dx: operands must be tc"); return RECNN_E_UNSUPPORTED; }
    return launch_t<TC, MODE, false, false>(L, s);
  }
  if (L->a_f32) { recnn_set_error("gemm dw: A must be tc"); return RECNN_E_UNSUPPORTED; }
  return L->b_f32 ? launch_t<TC, MODE, false, true>(L, s) : launch_t<TC, MODE, false, false>(L, s);
}

int gemm_launch(GemmLaunch* L, hipStream_t stream) {
  if (L->nprob <= 0) return 0;
  if (L->nprob > GEMM_MAX_GROUP) { recnn_set_error("gemm group too large"); return RECNN_E_INVALID; }
  // k-contiguous operands are read in 16-byte chunks of the compute type; a chunk never straddles the end of K (the tail of
  // the last LDS stage is zero filled by the loaders).  The LDS-DMA kernels want whole stages and are only chosen for such K.
  if (L->dtype == RECNN_BF16X3) return x3_gemm_launch(L, stream);
  const int BK = L->dtype == RECNN_F32 ? 4 : 8;
  for (int i = 0; i < L->nprob; ++i) {
    const GemmProb& p = L->batch.p[i];
    for (int s = 0; s < p.nseg; ++s) {
      const GemmSeg& g = p.seg[s];
      if (!g.A || !g.B) { recnn_set_error("gemm: null operand"); return RECNN_E_INVALID; }
      if (L->mode != GEMM_DW && (g.K % BK)) { recnn_set_error("gemm: K=%d not a multiple of %d", g.K, BK); return RECNN_E_INVALID; }
      if (((uintptr_t)g.A | (uintptr_t)g.B) & 15) { recnn_set_error("gemm: operand not 16-byte aligned"); return RECNN_E_INVALID; }
      const int64_t ea = (L->a_f32 || L->dtype == RECNN_F32) ? 4 : 2, eb = (L->b_f32 || L->dtype == RECNN_F32) ? 4 : 2;
      if ((g.lda * ea) % 16 || (g.ldb * eb) % 16) { recnn_set_error("gemm: leading dimension not 16-byte aligned"); return RECNN_E_INVALID; }
      // k-strided operands (KSLoader, gemm_dw_dma_kernel) are read in whole 16-byte units up to the end of the 64-wide tile,
      // on every k row: the pitch has to hold the last tile
      const int64_t wm = (int64_t)(p.M + 63) / 64 * 64, wn = (int64_t)(p.N + 63) / 64 * 64;
      if (L->mode == GEMM_DX && g.ldb < wn) {
        recnn_set_error("gemm dx: operand pitch below the tile width (ldb=%lld N=%d, need %lld)", (long long)g.ldb, p.N, (long long)wn);
        return RECNN_E_INVALID;
      }
      if (L->mode == GEMM_DW && (g.lda < wm || g.ldb < wn)) {
        recnn_set_error("gemm dw: operand pitch below the tile width (lda=%lld M=%d, ldb=%lld N=%d)", (long long)g.lda, p.M,
                        (long long)g.ldb, p.N);
        return RECNN_E_INVALID;
      }
    }
    if (!p.C) { recnn_set_error("gemm: null output"); return RECNN_E_INVALID; }
  }
  if (L->dtype == RECNN_F32) {
    switch (L->mode) {
      case GEMM_FWD: return launch_m<float, GEMM_FWD>(L, stream);
      case GEMM_DX: return launch_m<float, GEMM_DX>(L, stream);
      case GEMM_DW: return launch_m<float, GEMM_DW>(L, stream);
    }
  } else if (L->dtype == RECNN_BF16) {
    switch (L->mode) {
      case GEMM_FWD: return launch_m<bf16_t, GEMM_FWD>(L, stream);
      case GEMM_DX: return launch_m<bf16_t, GEMM_DX>(L, stream);
      case GEMM_DW: return launch_m<bf16_t, GEMM_DW>(L, stream);
    }
  }
  recnn_set_error("gemm: bad dtype/mode");
  return RECNN_E_INVALID;
}

int gemm_from_args(const recnn_gemm_args* a, int mode, GemmLaunch* L) {
  if (!a) { recnn_set_error("null args"); return RECNN_E_INVALID; }
  memset(L, 0, sizeof(*L));
  L->dtype = a->dtype;
  L->mode = mode;
  L->nprob = 1;
  L->a_f32 = a->a_f32[0];
  L->b_f32 = a->b_f32[0];
  GemmProb& p = L->batch.p[0];
  gemm_prob_init(&p);
  p.nseg = (mode == GEMM_FWD && a->K[1] > 0) ? 2 : 1;
  for (int s = 0; s < p.nseg; ++s) {
    p.seg[s].A = a->A[s]; p.seg[s].B = a->B[s];
    p.seg[s].lda = a->lda[s]; p.seg[s].ldb = a->ldb[s];
    p.seg[s].K = a->K[s];
    if (a->a_f32[s] != a->a_f32[0] || a->b_f32[s] != a->b_f32[0]) {
      recnn_set_error("gemm: segments must share operand memory types");
      return RECNN_E_UNSUPPORTED;
    }
  }
  p.M = a->M; p.N = a->N;
  p.C = a->C; p.ldc = a->ldc; p.c_f32 = a->c_f32;
  p.bias = a->bias; p.relu = a->relu; p.mask_mode = a->mask_mode;
  p.mask = a->mask; p.ld_mask = a->ld_mask;
  p.seed = a->seed; p.stream_id = a->stream_id; p.step_ptr = a->step_ptr;
  p.addend = a->addend; p.ld_add = a->ld_add; p.add_clip = a->add_clip; p.add_row_div = a->add_row_div;
  p.yref = a->yref; p.ldy = a->ldy; p.dx_scale = a->dx_scale; p.colsum = a->colsum;
  p.dw_splits = a->dw_splits > 0 ? a->dw_splits : 1;
  p.dw_slab_stride = a->dw_slab_stride;
  p.dw_valid_cols = a->dw_valid_cols > 0 ? a->dw_valid_cols : a->N;
  p.dw_col_rot = a->dw_col_rot;
  if (mode == GEMM_DW) p.c_f32 = 1;
  if (mode == GEMM_FWD) { L->ws = (float*)a->ws; L->ws_bytes = a->ws ? a->ws_bytes : 0; }
  return 0;
}

extern "C" int recnn_gemm_fwd(const recnn_gemm_args* a, void* stream) {
  GemmLaunch L;
  int rc = gemm_from_args(a, GEMM_FWD, &L);
  return rc ? rc : gemm_launch(&L, (hipStream_t)stream);
}
extern "C" int recnn_gemm_dx(const recnn_gemm_args* a, void* stream) {
  GemmLaunch L;
  int rc = gemm_from_args(a, GEMM_DX, &L);
  return rc ? rc : gemm_launch(&L, (hipStream_t)stream);
}
extern "C" int recnn_gemm_dw(const recnn_gemm_args* a, void* stream) {
  GemmLaunch L;
  int rc = gemm_from_args(a, GEMM_DW, &L);
  return rc ? rc : gemm_launch(&L, (hipStream_t)stream);
}

// ------------------------------------------------------------------ mask dump (tests)
__global__ void hash_mask_dump_kernel(uint32_t seed, int32_t step, uint32_t stream_id, int M, int N, uint8_t* out) {
  const uint32_t key = mask_key(seed, step, stream_id);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)M * N) return;
  int m = (int)(i / N), n = (int)(i % N);
  out[i] = mask_keep(mask_word(key, (uint32_t)(m >> 2), (uint32_t)(n >> 2)), m & 3, n & 3) ? 1 : 0;
}
// ... with the step on the device (step = *step_ptr + step_add): what a captured graph needs to draw fresh masks per replay
__global__ void hash_mask_dump_at_kernel(uint32_t seed, const int32_t* step_ptr, int step_add, uint32_t stream_id, int M, int N, uint8_t* out) {
  const uint32_t key = mask_key(seed, *step_ptr + step_add, stream_id);
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)M * N) return;
  int m = (int)(i / N), n = (int)(i % N);
  out[i] = mask_keep(mask_word(key, (uint32_t)(m >> 2), (uint32_t)(n >> 2)), m & 3, n & 3) ? 1 : 0;
}
extern "C" int recnn_hash_mask_dump_at(uint32_t seed, const int32_t* step_dev, int step_add, uint32_t stream_id, int M, int N, uint8_t* out,
                                       void* stream) {
  RECNN_REQUIRE(out && step_dev && M > 0 && N > 0, "hash_mask_dump_at: bad args");
  int64_t n = (int64_t)M * N;
  hipLaunchKernelGGL(hash_mask_dump_at_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, step_dev,
                     step_add, stream_id, M, N, out);
  return recnn_check_hip(hipGetLastError(), "hash_mask_dump_at");
}
extern "C" int recnn_hash_mask_dump(uint32_t seed, int32_t step, uint32_t stream_id, int M, int N, uint8_t* out, void* stream) {
  RECNN_REQUIRE(out && M > 0 && N > 0, "hash_mask_dump: bad args");
  int64_t n = (int64_t)M * N;
  hipLaunchKernelGGL(hash_mask_dump_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, step,
                     stream_id, M, N, out);
  return recnn_check_hip(hipGetLastError(), "hash_mask_dump");
}
