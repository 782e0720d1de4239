// anomaly.hip -- the reference's debugging autoencoder (recnn/nn/models.py:7-38) on the exact-f32 MFMA.
//
//   x[128] -> L0(128,64) ReLU BN0 -> L1(64,32) ReLU BN1 -> L2(32,64) ReLU BN2 -> L3(64,128) ReLU
//
// Every kernel works on 64-row panels with four waves; wave w owns panel rows 16w .. 16w+15 through a whole layer, so the
// products are 16 x N strips on v_mfma_f32_16x16x4_f32 (A = the wave's activation rows in LDS, B = weight rows in LDS, k in a
// fixed order).  Three launch plans:
//   eval (ae_eval_kernel): ONE persistent launch, all 21,408 parameters in LDS; every BatchNorm is the per-column affine
//     (scale = gamma rsqrt(var + eps), shift = beta - mean scale) applied in the epilogue of the layer before it; rec_error sums
//     (x - out)^2 per row in the last epilogue and never stores the 128-wide output.
//   train-style forward (ae_fwd_seg_kernel<L>): one launch per layer -- each BatchNorm is a grid-wide seam.  Launch L writes
//     a_L = relu(L_L(h_{L-1})) and per-panel column partials (count, mean, M2); launch L+1 merges them in panel order (Chan's
//     formula) before it normalises its input; its workgroup 0 updates the running statistics and num_batches_tracked.
//   backward (ae_bwd_seg_kernel<L>, L = 3 .. 0, then recnn_gemm_dw x 4 and ae_grad_final_kernel): launch L turns the incoming
//     gradient g_L into dz_L (ReLU gate, BatchNorm backward from the merged column sums of g_L and g_L x_hat_L), computes
//     g_{L-1} = dz_L W_L and the partial column sums the next launch merges.  dW_L = dz_L^T h_{L-1} is recnn_gemm_dw split over
//     rows into slabs; the slabs and the bias-gradient partials are summed in a fixed order by one final launch.
// No atomics anywhere: two identical calls give bit-identical results.
#include "common.h"

namespace {

constexpr int NT = 256;     // 4 waves
constexpr int BMR = 64;     // rows per panel
constexpr int PAD = 4;      // LDS row padding (floats): rows stay 16-byte aligned, fragment reads spread over banks
constexpr int MAXC = 128;   // widest layer
constexpr int GW_SLAB = 64 * 128 + 32 * 64 + 64 * 32 + 128 * 64;   // all four weight matrices: 20,480 floats

__host__ __device__ constexpr int lin_in(int l) { return l == 0 ? 128 : l == 1 ? 64 : l == 2 ? 32 : 64; }
__host__ __device__ constexpr int lin_out(int l) { return l == 0 ? 64 : l == 1 ? 32 : l == 2 ? 64 : 128; }
__host__ __device__ constexpr int w_off(int l) { return l == 0 ? 0 : l == 1 ? 64 * 128 : l == 2 ? 64 * 128 + 32 * 64 : 64 * 128 + 2 * 32 * 64; }

// Row pitch of the matrices recnn_gemm_dw reads (h_l, dz_l): its operands are read in whole 64-column tiles on every row, so a
// 32-column matrix sits in rows of 64 (include/recnn_hip.h recnn_gemm_args; the padding columns are never written and only
// reach outputs that are never stored).
__host__ __device__ constexpr int dw_pitch(int cols) { return cols < 64 ? 64 : cols; }

// act layout (floats, N = rows): a0 [N,64] | a1 [N,32] | a2 [N,64] | h0 [N,64] | h1 [N,32 of pitch 64] | h2 [N,64] | stats [3][2][64]
__host__ __device__ inline int64_t act_a_off(int l, int64_t n) { return l == 0 ? 0 : l == 1 ? 64 * n : 96 * n; }
__host__ __device__ inline int64_t act_h_off(int l, int64_t n) { return 160 * n + 64 * l * n; }
__host__ __device__ inline int64_t act_st_off(int64_t n) { return 352 * n; }
__host__ __device__ inline int64_t act_floats(int64_t n) { return 352 * n + 3 * 2 * 64; }

// workspace layout (floats), P panels, S dW slabs; every region starts on a 64-float boundary
struct WsLayout {
  int64_t fpart, bpart, dbpart, slabs, g[3], dz[4], total;
  int P, S;
};
__host__ __device__ inline int64_t r64(int64_t v) { return (v + 63) / 64 * 64; }
__host__ __device__ inline WsLayout ws_layout(int rows) {
  WsLayout w;
  const int64_t n = rows;
  w.P = (rows + BMR - 1) / BMR;
  w.S = rows / 512 < 1 ? 1 : (rows / 512 > 64 ? 64 : rows / 512);
  int64_t o = 0;
  w.fpart = o;  o += r64((int64_t)3 * w.P * 3 * 64);     // [seam][panel][count | mean | M2][64]
  w.bpart = o;  o += r64((int64_t)3 * w.P * 2 * 64);     // [seam][panel][sum g | sum g x_hat][64]
  w.dbpart = o; o += r64((int64_t)4 * w.P * MAXC);       // [layer][panel][128]
  w.slabs = o;  o += r64((int64_t)w.S * GW_SLAB);        // [slab][all four dW]
  for (int l = 0; l < 3; ++l) { w.g[l] = o; o += r64(n * lin_out(l)); }    // g_l: gradient w.r.t. h_l
  for (int l = 0; l < 4; ++l) { w.dz[l] = o; o += r64(n * dw_pitch(lin_out(l))); }   // dz_l: gradient w.r.t. Linear l's output
  w.total = o;
  return w;
}

// acc[t][i] = sum_k a[4g + i][k] * w[16 t + r][k] for this wave's 16 rows (r = lane & 15, g = lane >> 4).  a: LDS, row stride
// KC + PAD; w: LDS [NO][KC + PAD].  A lane's float4 holds k0 + 4g .. +3 of both operands; MFMA j contracts element j over the four
// lane groups, so the k order is fixed by the instruction sequence.
template <int KC, int NO>
__device__ __forceinline__ void mm16(const float* a, const float* w, f32x4 (&acc)[NO / 16], int lane) {
  const int r = lane & 15, g = lane >> 4;
#pragma unroll
  for (int t = 0; t < NO / 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int k0 = 0; k0 < KC; k0 += 16) {
    const f32x4 av = *(const f32x4*)(a + r * (KC + PAD) + k0 + 4 * g);
#pragma unroll
    for (int t = 0; t < NO / 16; ++t) {
      const f32x4 bv = *(const f32x4*)(w + (t * 16 + r) * (KC + PAD) + k0 + 4 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc[t], 0, 0, 0);
    }
  }
}

// global [NO][K] row-major -> LDS [NO][K + PAD]
template <int NO, int K>
__device__ __forceinline__ void stage_w(const float* __restrict__ w, float* s, int tid) {
  for (int i = tid; i < NO * K / 4; i += NT) {
    const int row = i / (K / 4), c4 = i - row * (K / 4);
    *(f32x4*)(s + row * (K + PAD) + 4 * c4) = *(const f32x4*)(w + (int64_t)row * K + 4 * c4);
  }
}

__device__ __forceinline__ f32x4 load_row4(const float* p, bool vec) {
  if (vec) return *(const f32x4*)p;
  return f32x4{p[0], p[1], p[2], p[3]};
}

// sum over the 16 lanes of a lane group (same g), fixed butterfly: every lane of the group ends with the same value
__device__ __forceinline__ float group16_sum(float v) {
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 1);
  return v;
}

// ------------------------------------------------------------------------------------------------ eval: one launch
constexpr int EV_W0 = 0, EV_W1 = EV_W0 + 64 * (128 + PAD), EV_W2 = EV_W1 + 32 * (64 + PAD), EV_W3 = EV_W2 + 64 * (32 + PAD);
constexpr int EV_B = EV_W3 + 128 * (64 + PAD);                 // biases 64 | 32 | 64 | 128
constexpr int EV_SC = EV_B + 288;                              // scale / shift: BN0 64 + 64, BN1 32 + 32, BN2 64 + 64
constexpr int EV_X = EV_SC + 320;                              // x panel [64][132]
constexpr int EV_HA = EV_X + BMR * (128 + PAD);                // [64][68]: h0, then h2
constexpr int EV_HB = EV_HA + BMR * (64 + PAD);                // [64][36]: h1
constexpr int EV_FLOATS = EV_HB + BMR * (32 + PAD);
constexpr int EV_LDS = EV_FLOATS * 4;                          // 149,632 bytes
static_assert(EV_LDS <= 160 * 1024, "eval kernel LDS");
__host__ __device__ constexpr int ev_b_off(int l) { return l == 0 ? 0 : l == 1 ? 64 : l == 2 ? 96 : 160; }
__host__ __device__ constexpr int ev_sc_off(int i) { return i == 0 ? 0 : i == 1 ? 128 : 192; }   // scale at +0, shift at +width

// hidden-layer epilogue: h = relu(acc + b) * scale + shift into the LDS panel (row stride NO + PAD)
template <int NO>
__device__ __forceinline__ void ev_hidden(const f32x4 (&acc)[NO / 16], const float* sb, const float* ssc, float* hout, int lane) {
  const int r = lane & 15, g = lane >> 4;
#pragma unroll
  for (int t = 0; t < NO / 16; ++t) {
    const int c = t * 16 + r;
    const float b = sb[c], sc = ssc[c], sh = ssc[NO + c];
#pragma unroll
    for (int i = 0; i < 4; ++i) hout[(4 * g + i) * (NO + PAD) + c] = fmaxf(acc[t][i] + b, 0.f) * sc + sh;
  }
}

template <bool ERR>
__global__ __launch_bounds__(NT) void ae_eval_kernel(const recnn_ae_params p, const float* __restrict__ x, int64_t ldx, int xvec, int rows,
                                                     float* __restrict__ out, int64_t ldo, float* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  stage_w<64, 128>(p.w[0], smem + EV_W0, tid);
  stage_w<32, 64>(p.w[1], smem + EV_W1, tid);
  stage_w<64, 32>(p.w[2], smem + EV_W2, tid);
  stage_w<128, 64>(p.w[3], smem + EV_W3, tid);
  for (int l = 0; l < 4; ++l)
    for (int c = tid; c < lin_out(l); c += NT) smem[EV_B + ev_b_off(l) + c] = p.b[l][c];
  for (int i = 0; i < 3; ++i) {
    const int C = lin_out(i);
    for (int c = tid; c < C; c += NT) {
      const float inv = 1.f / sqrtf(p.running_var[i][c] + p.eps[i]);
      const float sc = p.gamma[i][c] * inv;
      smem[EV_SC + ev_sc_off(i) + c] = sc;
      smem[EV_SC + ev_sc_off(i) + C + c] = p.beta[i][c] - p.running_mean[i][c] * sc;
    }
  }
  const int P = (rows + BMR - 1) / BMR;
  float* sx = smem + EV_X + wave * 16 * (128 + PAD);
  float* ha = smem + EV_HA + wave * 16 * (64 + PAD);
  float* hb = smem + EV_HB + wave * 16 * (32 + PAD);
  for (int panel = blockIdx.x; panel < P; panel += gridDim.x) {
    __syncthreads();                          // parameters staged / previous panel's LDS reads done
    const int mw = panel * BMR + wave * 16;   // this wave's first row
#pragma unroll
    for (int j = 0; j < 8; ++j) {             // 16 rows x 32 float4, wave-private
      const int idx = lane + 64 * j, row = idx >> 5, c4 = idx & 31;
      const int m = mw + row;
      const f32x4 v = m < rows ? load_row4(x + (int64_t)m * ldx + 4 * c4, xvec) : f32x4{0.f, 0.f, 0.f, 0.f};
      *(f32x4*)(sx + row * (128 + PAD) + 4 * c4) = v;
    }
    __syncthreads();
    {
      f32x4 acc[4];
      mm16<128, 64>(sx, smem + EV_W0, acc, lane);
      ev_hidden<64>(acc, smem + EV_B + ev_b_off(0), smem + EV_SC + ev_sc_off(0), ha, lane);
    }
    __syncthreads();
    {
      f32x4 acc[2];
      mm16<64, 32>(ha, smem + EV_W1, acc, lane);
      ev_hidden<32>(acc, smem + EV_B + ev_b_off(1), smem + EV_SC + ev_sc_off(1), hb, lane);
    }
    __syncthreads();
    {
      f32x4 acc[4];
      mm16<32, 64>(hb, smem + EV_W2, acc, lane);
      ev_hidden<64>(acc, smem + EV_B + ev_b_off(2), smem + EV_SC + ev_sc_off(2), ha, lane);
    }
    __syncthreads();
    f32x4 acc[8];
    mm16<64, 128>(ha, smem + EV_W3, acc, lane);
    const float* sb3 = smem + EV_B + ev_b_off(3);
    if constexpr (ERR) {
      float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int c = t * 16 + r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float d = sx[(4 * g + i) * (128 + PAD) + c] - fmaxf(acc[t][i] + sb3[c], 0.f);
          s[i] = fmaf(d, d, s[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = group16_sum(s[i]);
        const int m = mw + 4 * g + i;
        if (r == 0 && m < rows) err[m] = v;
      }
    } else {
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int c = t * 16 + r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = mw + 4 * g + i;
          if (m < rows) out[(int64_t)m * ldo + c] = fmaxf(acc[t][i] + sb3[c], 0.f);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ train-style forward
// LDS: W_L [NO][K+PAD] | b [NO] | scale [K] | shift [K] | input panel [64][K+PAD] | output panel [64][NO+PAD] (partials) | [3][NT]
template <int L>
__host__ __device__ constexpr int fs_floats() {
  return lin_out(L) * (lin_in(L) + PAD) + lin_out(L) + 2 * lin_in(L) + BMR * (lin_in(L) + PAD) + BMR * (lin_out(L) + PAD) + 3 * NT;
}

// count / mean / M2 of column c over panels [b0, b1), merged in panel order (Chan et al.); merge2 folds (nb, mb, qb) into (n, mean, m2)
__device__ __forceinline__ void merge2(float& n, float& mean, float& m2, float nb, float mb, float qb) {
  const float nab = n + nb;
  if (nab == 0.f) return;
  const float d = mb - mean;
  mean = mean + d * (nb / nab);
  m2 = m2 + qb + d * d * (n * nb / nab);
  n = nab;
}
__device__ inline void merge_range(const float* __restrict__ part, int b0, int b1, int c, float& n, float& mean, float& m2) {
  n = 0.f; mean = 0.f; m2 = 0.f;
#pragma unroll 8
  for (int b = b0; b < b1; ++b) merge2(n, mean, m2, part[(int64_t)b * 192 + c], part[(int64_t)b * 192 + 64 + c], part[(int64_t)b * 192 + 128 + c]);
}

template <int L, int MODE>   // MODE 0: hidden layer (writes a_L), 1: forward output, 2: rec_error
__global__ __launch_bounds__(NT) void ae_fwd_seg_kernel(const recnn_ae_params p, int train, const float* __restrict__ x, int64_t ldx,
                                                        int xvec, int rows, float* __restrict__ out, int64_t ldo, float* __restrict__ err,
                                                        float* __restrict__ act, int keep, float* __restrict__ ws, int64_t fpart) {
  constexpr int K = lin_in(L), NO = lin_out(L);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sw = smem;
  float* sb = sw + NO * (K + PAD);
  float* ssc = sb + NO;
  float* ssh = ssc + K;
  float* sin = ssh + K;
  float* sout = sin + BMR * (K + PAD);
  float* sred = sout + BMR * (NO + PAD);        // [3][NT] chunk merges
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int P = (rows + BMR - 1) / BMR;
  const int64_t n = rows;
  const int m0 = blockIdx.x * BMR;
  stage_w<NO, K>(p.w[L], sw, tid);
  for (int c = tid; c < NO; c += NT) sb[c] = p.b[L][c];
  if constexpr (L > 0) {
    constexpr int bn = L - 1;
    float* st = act + act_st_off(n) + bn * 128;
    if (train) {   // NT / K panel chunks merged in parallel (chunk ch of column c: thread ch K + c), then the chunks in order
      const int c = tid % K, ch = tid / K, nch = NT / K;
      float cn, cm, cq;
      merge_range(ws + fpart + (int64_t)bn * P * 192, (int)((int64_t)P * ch / nch), (int)((int64_t)P * (ch + 1) / nch), c, cn, cm, cq);
      sred[tid] = cn;
      sred[NT + tid] = cm;
      sred[2 * NT + tid] = cq;
      __syncthreads();
    }
    for (int c = tid; c < K; c += NT) {
      float mean, inv;
      if (train) {
        float cnt = 0.f, m2 = 0.f;
        mean = 0.f;
        for (int ch = 0; ch < NT / K; ++ch) merge2(cnt, mean, m2, sred[ch * K + c], sred[NT + ch * K + c], sred[2 * NT + ch * K + c]);
        inv = 1.f / sqrtf(m2 / cnt + p.eps[bn]);
        if (blockIdx.x == 0) {
          const float mo = p.momentum[bn];
          p.running_mean[bn][c] = (1.f - mo) * p.running_mean[bn][c] + mo * mean;
          p.running_var[bn][c] = (1.f - mo) * p.running_var[bn][c] + mo * (m2 / (cnt - 1.f));
        }
      } else {
        mean = p.running_mean[bn][c];
        inv = 1.f / sqrtf(p.running_var[bn][c] + p.eps[bn]);
      }
      if (keep && blockIdx.x == 0) {
        st[c] = mean;
        st[64 + c] = inv;
      }
      const float sc = p.gamma[bn][c] * inv;
      ssc[c] = sc;
      ssh[c] = p.beta[bn][c] - mean * sc;
    }
    if (train && blockIdx.x == 0 && tid == 0) *p.num_batches_tracked[bn] += 1;
  }
  __syncthreads();
  // input panel: x rows, or a_{L-1} normalised (and kept as h_{L-1} for backward)
  for (int i = tid; i < BMR * K / 4; i += NT) {
    const int row = i / (K / 4), c4 = i - row * (K / 4);
    const int m = m0 + row;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (m < rows) {
      if constexpr (L == 0) {
        v = load_row4(x + (int64_t)m * ldx + 4 * c4, xvec);
      } else {
        v = *(const f32x4*)(act + act_a_off(L - 1, n) + (int64_t)m * K + 4 * c4);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] * ssc[4 * c4 + j] + ssh[4 * c4 + j];
        if (keep) *(f32x4*)(act + act_h_off(L - 1, n) + (int64_t)m * dw_pitch(K) + 4 * c4) = v;
      }
    }
    *(f32x4*)(sin + row * (K + PAD) + 4 * c4) = v;
  }
  __syncthreads();
  f32x4 acc[NO / 16];
  mm16<K, NO>(sin + wave * 16 * (K + PAD), sw, acc, lane);
  const int mw = m0 + wave * 16;
  if constexpr (MODE == 0) {
    float* a = act + act_a_off(L, n);
#pragma unroll
    for (int t = 0; t < NO / 16; ++t) {
      const int c = t * 16 + r;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wave * 16 + 4 * g + i, m = m0 + row;
        const float v = fmaxf(acc[t][i] + sb[c], 0.f);
        if (m < rows) a[(int64_t)m * NO + c] = v;
        sout[row * (NO + PAD) + c] = v;
      }
    }
    if (train) {
      __syncthreads();
      const int nv = rows - m0 < BMR ? rows - m0 : BMR;
      float* part = ws + fpart + ((int64_t)L * P + blockIdx.x) * 192;
      for (int c = tid; c < NO; c += NT) {
        float s = 0.f;
        for (int row = 0; row < nv; ++row) s += sout[row * (NO + PAD) + c];
        const float mean = s / (float)nv;
        float q = 0.f;
        for (int row = 0; row < nv; ++row) {
          const float d = sout[row * (NO + PAD) + c] - mean;
          q = fmaf(d, d, q);
        }
        part[c] = (float)nv;
        part[64 + c] = mean;
        part[128 + c] = q;
      }
    }
  } else if constexpr (MODE == 1) {
#pragma unroll
    for (int t = 0; t < NO / 16; ++t) {
      const int c = t * 16 + r;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = mw + 4 * g + i;
        if (m < rows) out[(int64_t)m * ldo + c] = fmaxf(acc[t][i] + sb[c], 0.f);
      }
    }
  } else {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NO / 16; ++t) {
      const int c = t * 16 + r;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = mw + 4 * g + i;
        const float xv = m < rows ? x[(int64_t)m * ldx + c] : 0.f;
        const float d = xv - fmaxf(acc[t][i] + sb[c], 0.f);
        s[i] = fmaf(d, d, s[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = group16_sum(s[i]);
      const int m = mw + 4 * g + i;
      if (r == 0 && m < rows) err[m] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward
// LDS: W_L^T [K][NO+PAD] | coefficients 5 x [NO] | dz panel [64][NO+PAD] | g_{L-1} panel [64][K+PAD] (first: [2][NT] chunk sums)
template <int L>
__host__ __device__ constexpr int bs_floats() {
  return lin_in(L) * (lin_out(L) + PAD) + 5 * lin_out(L) + BMR * (lin_out(L) + PAD) + (BMR * (lin_in(L) + PAD) > 2 * NT ? BMR * (lin_in(L) + PAD) : 2 * NT);
}

template <int L, bool DX>
__global__ __launch_bounds__(NT) void ae_bwd_seg_kernel(const recnn_ae_params p, recnn_ae_grads gr, int train, int rows,
                                                        const float* __restrict__ out, int64_t ldo, const float* __restrict__ dout,
                                                        int64_t ld_dout, const float* __restrict__ act, float* __restrict__ dx,
                                                        int64_t lddx, float* __restrict__ ws, WsLayout wl) {
  constexpr int K = lin_in(L), NO = lin_out(L);
  constexpr bool PRODUCT = L > 0 || DX;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* swt = smem;
  float* sca = swt + K * (NO + PAD);
  float* scb = sca + NO;
  float* scc = scb + NO;
  float* smean = scc + NO;
  float* sinv = smean + NO;
  float* sdz = sinv + NO;
  float* sgp = sdz + BMR * (NO + PAD);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int P = wl.P;
  const int64_t n = rows;
  const int m0 = blockIdx.x * BMR;
  const int nv = rows - m0 < BMR ? rows - m0 : BMR;
  const float* st = act + act_st_off(n);
  if constexpr (PRODUCT) {
    for (int i = tid; i < NO * K; i += NT) {          // W_L^T: swt[k][j] = W_L[j][k]
      const int j = i / K, k = i - j * K;
      swt[k * (NO + PAD) + j] = p.w[L][i];
    }
  }
  if constexpr (L < 3) {
    // BatchNorm L backward coefficients from the merged column sums of g_L and g_L x_hat_L
    const float* part = ws + wl.bpart + (int64_t)L * P * 128;
    {  // NT / NO panel chunks summed in parallel, then the chunk sums in order
      const int c = tid % NO, ch = tid / NO, nch = NT / NO;
      const int b0 = (int)((int64_t)P * ch / nch), b1 = (int)((int64_t)P * (ch + 1) / nch);
      float sg = 0.f, sgx = 0.f;
#pragma unroll 8
      for (int b = b0; b < b1; ++b) {
        sg += part[(int64_t)b * 128 + c];
        sgx += part[(int64_t)b * 128 + 64 + c];
      }
      sgp[tid] = sg;
      sgp[NT + tid] = sgx;
      __syncthreads();
    }
    for (int c = tid; c < NO; c += NT) {
      float sg = 0.f, sgx = 0.f;
      for (int ch = 0; ch < NT / NO; ++ch) {
        sg += sgp[ch * NO + c];
        sgx += sgp[NT + ch * NO + c];
      }
      const float inv = st[L * 128 + 64 + c];
      sca[c] = p.gamma[L][c] * inv;
      scb[c] = train ? sg / (float)rows : 0.f;
      scc[c] = train ? sgx / (float)rows : 0.f;
      smean[c] = st[L * 128 + c];
      sinv[c] = inv;
      if (blockIdx.x == 0) {
        gr.gamma[L][c] = sgx;
        gr.beta[L][c] = sg;
      }
    }
  }
  __syncthreads();
  // dz_L for the panel
  float* dzg = ws + wl.dz[L];
  for (int i = tid; i < BMR * NO; i += NT) {
    const int row = i / NO, c = i - row * NO, m = m0 + row;
    float dz = 0.f;
    if (m < rows) {
      if constexpr (L == 3) {
        dz = out[(int64_t)m * ldo + c] > 0.f ? dout[(int64_t)m * ld_dout + c] : 0.f;
      } else {
        const float gv = ws[wl.g[L] + (int64_t)m * NO + c];
        const float a = act[act_a_off(L, n) + (int64_t)m * NO + c];
        const float xh = (a - smean[c]) * sinv[c];
        dz = a > 0.f ? sca[c] * (gv - scb[c] - xh * scc[c]) : 0.f;
      }
      dzg[(int64_t)m * dw_pitch(NO) + c] = dz;
    }
    sdz[row * (NO + PAD) + c] = dz;
  }
  __syncthreads();
  {
    float* dbp = ws + wl.dbpart + ((int64_t)L * P + blockIdx.x) * MAXC;
    for (int c = tid; c < NO; c += NT) {
      float s = 0.f;
      for (int row = 0; row < nv; ++row) s += sdz[row * (NO + PAD) + c];
      dbp[c] = s;
    }
  }
  if constexpr (PRODUCT) {
    f32x4 acc[K / 16];
    mm16<NO, K>(sdz + wave * 16 * (NO + PAD), swt, acc, lane);
    if constexpr (L == 0) {
#pragma unroll
      for (int t = 0; t < K / 16; ++t) {
        const int c = t * 16 + r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = m0 + wave * 16 + 4 * g + i;
          if (m < rows) dx[(int64_t)m * lddx + c] = acc[t][i];
        }
      }
    } else {
      float* gp = ws + wl.g[L - 1];
#pragma unroll
      for (int t = 0; t < K / 16; ++t) {
        const int c = t * 16 + r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = wave * 16 + 4 * g + i, m = m0 + row;
          if (m < rows) gp[(int64_t)m * K + c] = acc[t][i];
          sgp[row * (K + PAD) + c] = acc[t][i];
        }
      }
      __syncthreads();
      // partial column sums of g_{L-1} and g_{L-1} x_hat_{L-1} for BatchNorm L-1
      const float* a = act + act_a_off(L - 1, n);
      float* bp = ws + wl.bpart + ((int64_t)(L - 1) * P + blockIdx.x) * 128;
      for (int c = tid; c < K; c += NT) {
        const float mean = st[(L - 1) * 128 + c], inv = st[(L - 1) * 128 + 64 + c];
        float sg = 0.f, sgx = 0.f;
        for (int row = 0; row < nv; ++row) {
          const float gv = sgp[row * (K + PAD) + c];
          sg += gv;
          sgx = fmaf(gv, (a[(int64_t)(m0 + row) * K + c] - mean) * inv, sgx);
        }
        bp[c] = sg;
        bp[64 + c] = sgx;
      }
    }
  }
}

// dW_l = sum of the slabs in slab order (blocks 0 .. FIN_W-1); db_l = one wave per column: lane j sums panel chunk j in order, then the
// fixed DPP tree of wave_sum (blocks FIN_W ..)
constexpr int FIN_W = (GW_SLAB + NT - 1) / NT, FIN_B = (288 + NT / WAVE - 1) / (NT / WAVE);
__global__ __launch_bounds__(NT) void ae_grad_final_kernel(recnn_ae_grads gr, const float* __restrict__ ws, WsLayout wl) {
  if ((int)blockIdx.x < FIN_W) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= GW_SLAB) return;
    float s = 0.f;
#pragma unroll 8
    for (int sl = 0; sl < wl.S; ++sl) s += ws[wl.slabs + (int64_t)sl * GW_SLAB + i];
    const int l = i < w_off(1) ? 0 : i < w_off(2) ? 1 : i < w_off(3) ? 2 : 3;
    gr.w[l][i - w_off(l)] = s;
    return;
  }
  const int j = ((int)blockIdx.x - FIN_W) * (NT / WAVE) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= 288) return;   // (wave-uniform)
  const int l = j < 64 ? 0 : j < 96 ? 1 : j < 160 ? 2 : 3;
  const int c = j - (l == 0 ? 0 : l == 1 ? 64 : l == 2 ? 96 : 160);
  const int b0 = (int)((int64_t)wl.P * lane / WAVE), b1 = (int)((int64_t)wl.P * (lane + 1) / WAVE);
  float s = 0.f;
  for (int b = b0; b < b1; ++b) s += ws[wl.dbpart + ((int64_t)l * wl.P + b) * MAXC + c];
  s = wave_sum(s);
  if (lane == 0) gr.b[l][c] = s;
}

// ------------------------------------------------------------------------------------------------ host side
template <class F>
int set_lds(F* kern, int bytes) {
  return recnn_check_hip(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes), "anomaly lds attr");
}

int cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cached[dev]) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cached[dev] = v;
  }
  return cached[dev];
}

int check_params(const recnn_ae_params* p, bool writes_stats) {
  RECNN_REQUIRE(p, "anomaly: null params");
  for (int l = 0; l < 4; ++l) RECNN_REQUIRE(p->w[l] && p->b[l] && aligned16(p->w[l]), "anomaly: weight %d null or not 16-byte aligned", l);
  for (int i = 0; i < 3; ++i) {
    RECNN_REQUIRE(p->gamma[i] && p->beta[i] && p->running_mean[i] && p->running_var[i], "anomaly: BatchNorm %d: null pointer", i);
    RECNN_REQUIRE(!writes_stats || p->num_batches_tracked[i], "anomaly: BatchNorm %d: null num_batches_tracked", i);
  }
  return 0;
}

template <int L, int MODE>
int launch_fwd_seg(const recnn_ae_params& p, int train, const float* x, int64_t ldx, int xvec, int rows, float* out, int64_t ldo,
                   float* err, float* act, int keep, float* ws, int64_t fpart, int P, hipStream_t s) {
  constexpr int bytes = fs_floats<L>() * 4;
  static int attr = set_lds(ae_fwd_seg_kernel<L, MODE>, bytes);
  if (attr) return attr;
  hipLaunchKernelGGL((ae_fwd_seg_kernel<L, MODE>), dim3(P), dim3(NT), bytes, s, p, train, x, ldx, xvec, rows, out, ldo, err, act, keep,
                     ws, fpart);
  return recnn_check_hip(hipGetLastError(), "anomaly forward segment launch");
}

template <int L, bool DX>
int launch_bwd_seg(const recnn_ae_params& p, const recnn_ae_grads& g, int train, int rows, const float* out, int64_t ldo,
                   const float* dout, int64_t ld_dout, const float* act, float* dx, int64_t lddx, float* ws, const WsLayout& wl,
                   hipStream_t s) {
  constexpr int bytes = bs_floats<L>() * 4;
  static int attr = set_lds(ae_bwd_seg_kernel<L, DX>, bytes);
  if (attr) return attr;
  hipLaunchKernelGGL((ae_bwd_seg_kernel<L, DX>), dim3(wl.P), dim3(NT), bytes, s, p, g, train, rows, out, ldo, dout, ld_dout, act, dx,
                     lddx, ws, wl);
  return recnn_check_hip(hipGetLastError(), "anomaly backward segment launch");
}

}  // namespace

extern "C" {

int recnn_ae_act_floats(int rows, int64_t* h_floats) {
  RECNN_REQUIRE(h_floats && rows >= 0, "ae_act_floats: bad arguments");
  *h_floats = act_floats(rows);
  return 0;
}

int recnn_ae_workspace_bytes(int rows, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes && rows >= 0, "ae_workspace_bytes: bad arguments");
  *h_bytes = ws_layout(rows).total * 4;
  return 0;
}

int recnn_ae_eval(const recnn_ae_params* h_p, const float* x, int64_t ldx, int rows, float* out, int64_t ldo, float* err, void* stream) {
  if (int rc = check_params(h_p, false)) return rc;
  RECNN_REQUIRE(x && rows >= 0 && ldx >= 128 && ((out != nullptr) != (err != nullptr)), "ae_eval: bad arguments (x, rows, ldx, out xor err)");
  RECNN_REQUIRE(!out || ldo >= 128, "ae_eval: ldo < 128");
  if (rows == 0) return 0;
  const int xvec = aligned16(x) && (ldx % 4) == 0;
  const int P = (rows + BMR - 1) / BMR;
  const int grid = P < cu_count() ? P : cu_count();
  hipStream_t s = (hipStream_t)stream;
  if (err) {
    static int attr = set_lds(ae_eval_kernel<true>, EV_LDS);
    if (attr) return attr;
    hipLaunchKernelGGL(ae_eval_kernel<true>, dim3(grid), dim3(NT), EV_LDS, s, *h_p, x, ldx, xvec, rows, out, ldo, err);
  } else {
    static int attr = set_lds(ae_eval_kernel<false>, EV_LDS);
    if (attr) return attr;
    hipLaunchKernelGGL(ae_eval_kernel<false>, dim3(grid), dim3(NT), EV_LDS, s, *h_p, x, ldx, xvec, rows, out, ldo, err);
  }
  return recnn_check_hip(hipGetLastError(), "ae_eval launch");
}

int recnn_ae_forward(const recnn_ae_params* h_p, int train, const float* x, int64_t ldx, int rows, float* out, int64_t ldo, float* err,
                     float* act, int keep, void* workspace, void* stream) {
  if (int rc = check_params(h_p, train != 0)) return rc;
  RECNN_REQUIRE(x && act && workspace && rows >= 0 && ldx >= 128 && ((out != nullptr) != (err != nullptr)),
                "ae_forward: bad arguments (x, act, workspace, rows, ldx, out xor err)");
  RECNN_REQUIRE(!out || ldo >= 128, "ae_forward: ldo < 128");
  RECNN_REQUIRE(!train || rows >= 2, "ae_forward: train mode needs at least 2 rows (got %d)", rows);
  RECNN_REQUIRE(aligned16(act, workspace), "ae_forward: act / workspace not 16-byte aligned");
  if (rows == 0) return 0;
  const recnn_ae_params& p = *h_p;
  const WsLayout wl = ws_layout(rows);
  const int xvec = aligned16(x) && (ldx % 4) == 0;
  float* ws = (float*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int rc = launch_fwd_seg<0, 0>(p, train, x, ldx, xvec, rows, out, ldo, err, act, keep, ws, wl.fpart, wl.P, s);
  if (!rc) rc = launch_fwd_seg<1, 0>(p, train, x, ldx, xvec, rows, out, ldo, err, act, keep, ws, wl.fpart, wl.P, s);
  if (!rc) rc = launch_fwd_seg<2, 0>(p, train, x, ldx, xvec, rows, out, ldo, err, act, keep, ws, wl.fpart, wl.P, s);
  if (!rc) rc = err ? launch_fwd_seg<3, 2>(p, train, x, ldx, xvec, rows, out, ldo, err, act, keep, ws, wl.fpart, wl.P, s)
                    : launch_fwd_seg<3, 1>(p, train, x, ldx, xvec, rows, out, ldo, err, act, keep, ws, wl.fpart, wl.P, s);
  return rc;
}

int recnn_ae_backward(const recnn_ae_params* h_p, const recnn_ae_grads* h_g, int train, const float* x, int64_t ldx, int rows,
                      const float* out, int64_t ldo, const float* dout, int64_t ld_dout, const float* act, float* dx, int64_t lddx,
                      void* workspace, void* stream) {
  if (int rc = check_params(h_p, false)) return rc;
  RECNN_REQUIRE(h_g, "ae_backward: null grads");
  for (int l = 0; l < 4; ++l) RECNN_REQUIRE(h_g->w[l] && h_g->b[l], "ae_backward: null weight / bias gradient %d", l);
  for (int i = 0; i < 3; ++i) RECNN_REQUIRE(h_g->gamma[i] && h_g->beta[i], "ae_backward: null BatchNorm gradient %d", i);
  RECNN_REQUIRE(x && out && dout && act && workspace && rows > 0 && ldx >= 128 && ldo >= 128 && ld_dout >= 128,
                "ae_backward: bad arguments");
  RECNN_REQUIRE(!dx || lddx >= 128, "ae_backward: lddx < 128");
  RECNN_REQUIRE(!train || rows >= 2, "ae_backward: train mode needs at least 2 rows");
  RECNN_REQUIRE(aligned16(x, act, workspace) && ldx % 4 == 0, "ae_backward: x / act / workspace not 16-byte aligned");
  const recnn_ae_params& p = *h_p;
  const recnn_ae_grads& g = *h_g;
  const WsLayout wl = ws_layout(rows);
  float* ws = (float*)workspace;
  hipStream_t s = (hipStream_t)stream;
  int rc = launch_bwd_seg<3, false>(p, g, train, rows, out, ldo, dout, ld_dout, act, dx, lddx, ws, wl, s);
  if (!rc) rc = launch_bwd_seg<2, false>(p, g, train, rows, out, ldo, dout, ld_dout, act, dx, lddx, ws, wl, s);
  if (!rc) rc = launch_bwd_seg<1, false>(p, g, train, rows, out, ldo, dout, ld_dout, act, dx, lddx, ws, wl, s);
  if (!rc) rc = dx ? launch_bwd_seg<0, true>(p, g, train, rows, out, ldo, dout, ld_dout, act, dx, lddx, ws, wl, s)
                   : launch_bwd_seg<0, false>(p, g, train, rows, out, ldo, dout, ld_dout, act, dx, lddx, ws, wl, s);
  // dW_l = dz_l^T h_{l-1} (h_{-1} = x): recnn_gemm_dw split over rows into wl.S slabs
  for (int l = 0; l < 4 && !rc; ++l) {
    recnn_gemm_args a;
    memset(&a, 0, sizeof(a));
    a.dtype = RECNN_F32;
    a.M = lin_out(l);
    a.N = lin_in(l);
    a.A[0] = ws + wl.dz[l];
    a.lda[0] = dw_pitch(lin_out(l));
    a.B[0] = l == 0 ? (const void*)x : (const void*)(act + act_h_off(l - 1, rows));
    a.ldb[0] = l == 0 ? ldx : dw_pitch(lin_in(l));
    a.K[0] = rows;
    a.C = ws + wl.slabs + w_off(l);
    a.ldc = lin_in(l);
    a.c_f32 = 1;
    a.dx_scale = 1.f;
    a.dw_splits = wl.S;
    a.dw_slab_stride = GW_SLAB;
    a.dw_valid_cols = lin_in(l);
    rc = recnn_gemm_dw(&a, stream);
  }
  if (rc) return rc;
  hipLaunchKernelGGL(ae_grad_final_kernel, dim3(FIN_W + FIN_B), dim3(NT), 0, s, g, (const float*)ws, wl);
  return recnn_check_hip(hipGetLastError(), "ae_grad_final launch");
}

}  // extern "C"
