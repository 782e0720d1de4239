// state_grad.hip -- the input gradient of the DDPG / TD3 step: d loss / d state through layer 1 of the critic(s) and the actor
// (recnn/nn/update/ddpg.py:58-104, td3.py:95-132: the value losses' and the policy loss's backward reach `state`).
//
//   out[rows, S] (fp32) = sum_seg dz_seg[rows, K] * W_seg[K, S]
//
// one GEMM with M = rows, N = S, and the 1 or 2 segments as ONE concatenated contraction in a fixed order: segment 0 first, k
// ascending.  A workgroup owns a 64 x 64 output tile for the whole contraction -- no split-K, no atomics, no partial sums between
// workgroups: two launches give the same bits.  4 waves as 2 x 2, a wave owns 32 x 32 = 2 x 2 MFMA tiles.
//
// Operands.  dz rows are the engine's [Bc, Hp] backward buffers, W rows the engine's compute-type weight SHADOWS (rotated to
// [action | state], row stride a multiple of 128 elements, zero padded): every 16-byte chunk of either operand is aligned and lies
// inside its row's allocation, also the last chunk of an S that is no multiple of the chunk (S = 1290, S = 27); what such a chunk
// holds past column S only reaches output columns >= S, which are never stored.  Rows >= rows and k >= K are predicated off (zeros).
//
// Seeds.  A segment may carry an fp32 [rows] seed d (the fused bf16 path leaves UNIT backward tensors u = dz / d): its part of the
// sum is d[r] * (u[r, :] * W).  One segment: the seed multiplies the accumulator in the epilogue.  Two segments of which any carries a
// seed (FOLD; TD3's merged twin-critic gradient d1 (u1 W1c1) + d2 (u2 W1c2)): the accumulator tile is folded into a second tile at
// each segment's last stage -- total = acc * d for segment 0 (assigned), total = fma(acc, d, total) for segment 1 -- and cleared.
// Either way the seed meets the fp32 accumulator, never the bf16 operand (d u rounded to bf16 would cost 2^-9 per term).  The
// launches without a fold are a separate instantiation: their instruction sequence does not know about the second tile.
//
// The weights go in as the MFMA's first operand, so a lane ends up with four neighbouring columns of one output row:
//   fp32  v_mfma_f32_16x16x4_f32  : lane (fr, fg) supplies W[k = 4 fg + e][n = fr] and dz[m = fr][k = 4 fg + e], e = 0..3 per 16 k
//   bf16  v_mfma_f32_16x16x32_bf16: W fragment by transpose reads of the [k][n] LDS image (lds_stream.h tr_frag), dz fragment = the
//                                   lane's 8 contiguous k of row fr
//   acc[i] = out[m = fr][n = 4 fg + i]
// Stages of 32 k, register-staged and double buffered (the next stage's global loads are in flight under the MFMAs of this one).
// The real launches are small (rows 25..2048, S 256 | 1290, K 256..512): at rows = 50, S = 256 the grid is 4 workgroups and the launch
// is bound by its latency, not by anything in here.
#include "state_grad.h"
#include "lds_stream.h"

namespace {

constexpr int SG_BM = 64, SG_BN = 64, SG_KT = 32;

template <class T> struct SgTraits;
template <> struct SgTraits<float> {
  static constexpr int VEC = 4;
  static constexpr int PA = (SG_KT + 4) * 4;     // bytes per dz row of a stage (32 k + 16 bytes: the 16 rows of a fragment read spread over the banks)
  static constexpr int PB = (SG_BN + 4) * 4;     // bytes per W row (one k) of a stage
};
template <> struct SgTraits<bf16_t> {
  static constexpr int VEC = 8;
  static constexpr int PA = SG_KT * 2 + 16;
  static constexpr int PB = SG_BN * 2 + 16;      // (the pitch of x3.hip's transpose-read image)
};

template <class T, bool FOLD>
__global__ __launch_bounds__(256) void state_grad_kernel(const StateGradArgs a) {
  using TR = SgTraits<T>;
  constexpr int VEC = TR::VEC, PA = TR::PA, PB = TR::PB;
  constexpr int CA = SG_KT / VEC;                 // 16-byte chunks per dz row of a stage
  constexpr int CB = SG_BN / VEC;                 // ... per W row
  constexpr int NCH = SG_BM * CA / 256;           // chunks per thread and operand (2 fp32, 1 bf16); SG_KT * CB / 256 is the same number
  static_assert(SG_BM * CA == SG_KT * CB && SG_BM * CA % 256 == 0, "stage chunk counts");
  __shared__ __attribute__((aligned(16))) unsigned char sa[2][SG_BM * PA];
  __shared__ __attribute__((aligned(16))) unsigned char sb[2][SG_KT * PB];

  const int tiles_n = (a.S + SG_BN - 1) / SG_BN;
  const int tile_n = blockIdx.x % tiles_n, tile_m = blockIdx.x / tiles_n;
  const int m0 = tile_m * SG_BM, n0 = tile_n * SG_BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
  const int nk = (a.K + SG_KT - 1) / SG_KT;       // stages per segment
  const int nt = nk * a.nseg;

  uint4 ra[NCH], rb[NCH];
  auto fetch = [&](int t) {
    const int sg = t / nk, kb = (t - sg * nk) * SG_KT;
    const StateGradSeg& G = a.seg[sg];
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int c = u * 256 + tid;
      {
        const int row = c / CA, kc = c - row * CA;
        const int m = m0 + row, k = kb + kc * VEC;
        ra[u] = (m < a.rows && k < a.K) ? *(const uint4*)((const T*)G.dz + (int64_t)m * G.ld_dz + k) : make_uint4(0, 0, 0, 0);
      }
      {
        const int kr = c / CB, nc = c - kr * CB;
        const int k = kb + kr, n = n0 + nc * VEC;
        rb[u] = (k < a.K && n < a.S) ? *(const uint4*)((const T*)G.W + (int64_t)k * G.ld_w + n) : make_uint4(0, 0, 0, 0);
      }
    }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int c = u * 256 + tid;
      *(uint4*)(sa[buf] + (c / CA) * PA + (c % CA) * 16) = ra[u];
      *(uint4*)(sb[buf] + (c / CB) * PB + (c % CB) * 16) = rb[u];
    }
  };

  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[2][2] = {{zero4, zero4}, {zero4, zero4}};
  [[maybe_unused]] f32x4 total[2][2] = {{zero4, zero4}, {zero4, zero4}};   // FOLD only: the sum of the folded segments
  if (nt > 0) {
    fetch(0);
    put(0);
  }
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    if (t + 1 < nt) fetch(t + 1);
    const unsigned char* pa = sa[buf];
    const unsigned char* pb = sb[buf];
    if constexpr (sizeof(T) == 4) {
#pragma unroll
      for (int ks = 0; ks < SG_KT / 16; ++ks) {
        float4 av[2];
        float bv[2][4];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) av[tm] = *(const float4*)(pa + (wm0 + tm * 16 + fr) * PA + (ks * 16 + 4 * fg) * 4);
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
          for (int e = 0; e < 4; ++e) bv[tn][e] = *(const float*)(pb + (ks * 16 + 4 * fg + e) * PB + (wn0 + tn * 16 + fr) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
              acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[tn][e], ((const float*)&av[tm])[e], acc[tm][tn], 0, 0, 0);
      }
    } else {
      bf16x8 av[2], bv[2];
#pragma unroll
      for (int tm = 0; tm < 2; ++tm) av[tm] = __builtin_bit_cast(bf16x8, *(const uint4*)(pa + (wm0 + tm * 16 + fr) * PA + fg * 16));
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) bv[tn] = tr_frag(pb, PB, wn0 + tn * 16, fr, fg);
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bv[tn], av[tm], acc[tm][tn], 0, 0, 0);
    }
    if constexpr (FOLD) {
      const int sg = t / nk;
      if (t + 1 == (sg + 1) * nk) {   // the segment's last stage (uniform over the workgroup): fold its tile, seeded per row
        const float* d = a.seg[sg].scale;
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) {
          const int m = m0 + wm0 + tm * 16 + fr;
          const float sc = (d && m < a.rows) ? d[m] : 1.0f;
#pragma unroll
          for (int tn = 0; tn < 2; ++tn) {
#pragma unroll
            for (int i = 0; i < 4; ++i) total[tm][tn][i] = sg == 0 ? acc[tm][tn][i] * sc : __builtin_fmaf(acc[tm][tn][i], sc, total[tm][tn][i]);
            acc[tm][tn] = zero4;
          }
        }
      }
    }
    if (t + 1 < nt) put(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue: optional per-row seed (one segment; a fold has applied its seeds already), masked fp32 store (16 bytes per lane
  // where the row allows it)
  const float* row_scale = FOLD ? nullptr : a.seg[0].scale;
  const bool vec_ok = (a.ld_out & 3) == 0 && (((uintptr_t)a.out) & 15) == 0;
#pragma unroll
  for (int tm = 0; tm < 2; ++tm) {
    const int m = m0 + wm0 + tm * 16 + fr;
    if (m >= a.rows) continue;
    const float sc = row_scale ? row_scale[m] : 1.0f;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int n = n0 + wn0 + tn * 16 + 4 * fg;
      if (n >= a.S) continue;
      f32x4 v = FOLD ? total[tm][tn] : acc[tm][tn];
      if (row_scale) v *= sc;
      float* o = a.out + (int64_t)m * a.ld_out + n;
      if (vec_ok && n + 3 < a.S) {
        *(f32x4*)o = v;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (n + i < a.S) o[i] = v[i];
      }
    }
  }
}

}  // namespace

int state_grad_launch(const StateGradArgs& a, int dtype, hipStream_t s) {
  RECNN_REQUIRE(dtype == RECNN_F32 || dtype == RECNN_BF16, "state_grad: compute type %d is not supported (fp32 and bf16 are)", dtype);
  RECNN_REQUIRE(a.rows > 0 && a.S > 0 && a.K > 0 && a.K % 8 == 0, "state_grad: need rows > 0, S > 0, K a positive multiple of 8");
  RECNN_REQUIRE(a.nseg == 1 || a.nseg == 2, "state_grad: 1 or 2 segments");
  RECNN_REQUIRE(a.out && a.ld_out >= a.S, "state_grad: bad output");
  const int vec = dtype == RECNN_F32 ? 4 : 8;
  for (int i = 0; i < a.nseg; ++i) {
    const StateGradSeg& G = a.seg[i];
    RECNN_REQUIRE(G.dz && G.W, "state_grad: null operand");
    RECNN_REQUIRE(aligned16((const char*)G.dz, (const char*)G.W) && G.ld_dz % vec == 0 && G.ld_w % vec == 0,
                  "state_grad: operand rows must be 16-byte aligned");
    RECNN_REQUIRE(G.ld_dz >= a.K && G.ld_w >= (a.S + vec - 1) / vec * vec, "state_grad: operand rows shorter than the chunks read from them");
  }
  const int64_t tiles = (int64_t)((a.rows + SG_BM - 1) / SG_BM) * ((a.S + SG_BN - 1) / SG_BN);
  RECNN_REQUIRE(tiles < (1 << 30), "state_grad: too many tiles");
  // (a seed on a segment the launch does not have is ignored; one segment never folds: its seed is the epilogue's)
  const bool fold = a.nseg == 2 && (a.seg[0].scale || a.seg[1].scale);
  if (dtype == RECNN_F32) {
    if (fold) hipLaunchKernelGGL((state_grad_kernel<float, true>), dim3((unsigned)tiles), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((state_grad_kernel<float, false>), dim3((unsigned)tiles), dim3(256), 0, s, a);
  } else {
    if (fold) hipLaunchKernelGGL((state_grad_kernel<bf16_t, true>), dim3((unsigned)tiles), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((state_grad_kernel<bf16_t, false>), dim3((unsigned)tiles), dim3(256), 0, s, a);
  }
  return recnn_check_hip(hipGetLastError(), "state_grad launch");
}
