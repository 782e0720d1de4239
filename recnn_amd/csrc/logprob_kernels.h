// logprob_kernels.h -- the kernels over the 128 x 128 logits tile (logprob_tile.h), written once for every way of naming the columns:
// logprob.hip / logprob_bwd.hip run them over the whole catalogue (DenseCols), sampled.hip over a list of gathered item ids
// (GatheredCols).  The files that include this header describe the grids, workspaces and chains; here is what the two policies share
// and where they part:
//   DenseCols     the column equal to a row's action is its picked logit (forward: written to ws_za; backward: D gains g_lp there).
//   GatheredCols  nothing is picked (the target's logit is the caller's own per-row product); with drop_hits a column whose id equals
//                 the row's action is absent in that row (z = -inf, D = 0).  Absent columns can empty a whole tile of a row, so the
//                 running log-sum-exp guards its maximum against -inf.
// The MFMA sequence of a tile does not depend on the policy.
#pragma once
#include <math.h>

#include "logprob_tile.h"

namespace {
using namespace logprob_tile;      // Stage, stage_store, stage_mma, lds_at

// ---------------------------------------------------------------- forward: running (max, sum exp) per row and slice of the columns
// ws_m, ws_s: [n_slices][B]; ws_za: [B] (PICK only: written by the one lane of the one slice that holds a valid a[b])
template <typename T, class Cols>
__global__ __launch_bounds__(256) void logprob_slice_kernel(const float* __restrict__ x, int64_t ldx, int B, int K, const T* __restrict__ W,
                                                            int64_t ldw, const Cols cols, const int64_t* __restrict__ actions,
                                                            int tiles_per_slice, float* __restrict__ ws_m, float* __restrict__ ws_s,
                                                            float* __restrict__ ws_za) {
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, r16 = lane & 15;
  const int b0 = blockIdx.x * BM;
  const int ntiles = (cols.count() + BN - 1) / BN;
  const int t0 = blockIdx.y * tiles_per_slice;
  const int t1 = min(ntiles, t0 + tiles_per_slice);
  const int nk = K / Stage<T>::BK;

  // rows of this lane's accumulator elements: b0 + 32 wave + 16 tm + 4 q + r
  float m[2][4], s[2][4];
  int64_t act[2][4];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m[tm][r] = -INFINITY;
      s[tm][r] = 0.f;
      const int b = b0 + 32 * wave + 16 * tm + 4 * q + r;
      act[tm][r] = b < B ? actions[b] : -1;
    }

  Stage<T> st;
  for (int t = t0; t < t1; ++t) {
    const int n0 = t * BN;
    f32x4 acc[2][NTN];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int tn = 0; tn < NTN; ++tn) acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};

    st.fetch(x, ldx, B, b0, W, ldw, cols, n0, 0, tid);
    stage_store(st, lds, tid);      // (the previous tile's k-loop ended at a barrier: nobody still reads the stage)
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const bool more = kt + 1 < nk;
      if (more) st.fetch(x, ldx, B, b0, W, ldw, cols, n0, (kt + 1) * Stage<T>::BK, tid);
      stage_mma<T, 2, NTN>(lds + (kt & 1) * STAGE_BYTES, 32 * wave, BM, q, r16, acc);
      if (more) stage_store(st, lds + ((kt + 1) & 1) * STAGE_BYTES, tid);
      __syncthreads();
    }

    // fold the tile: lane holds rows 4 q + r of each 16-row block, column n0 + 16 tn + r16
    float cn[NTN];
    bool live[NTN];
    int64_t id[NTN];      // the column's table row, -1: absent
#pragma unroll
    for (int tn = 0; tn < NTN; ++tn) {
      const int n = n0 + 16 * tn + r16;
      id[tn] = cols.row(n);
      live[tn] = id[tn] >= 0;
      cn[tn] = live[tn] ? cols.bias(n, id[tn]) : 0.f;
    }
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float z[NTN];
        float tmax = -INFINITY;
#pragma unroll
        for (int tn = 0; tn < NTN; ++tn) {
          z[tn] = live[tn] ? acc[tm][tn][r] + cn[tn] : -INFINITY;
          if constexpr (Cols::PICK) {
            if (live[tn] && act[tm][r] == id[tn]) ws_za[b0 + 32 * wave + 16 * tm + 4 * q + r] = z[tn];
          } else {
            if (cols.drop_hits && act[tm][r] == id[tn]) z[tn] = -INFINITY;
          }
          tmax = fmaxf(tmax, z[tn]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 8));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 4));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 2));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 1));
        // PICK: column n0 of the tile is below N, so the maximum is finite for finite operands (the header asks for them).  Else a
        // row may have seen nothing yet: the exponents are then taken against 0 and every term is exp(-inf) = 0.
        const float mn = fmaxf(m[tm][r], tmax);
        const float ms = (!Cols::PICK && mn == -INFINITY) ? 0.f : mn;
        float e = expf(z[0] - ms);
#pragma unroll
        for (int tn = 1; tn < NTN; ++tn) e += expf(z[tn] - ms);
        e += __shfl_xor(e, 8);
        e += __shfl_xor(e, 4);
        e += __shfl_xor(e, 2);
        e += __shfl_xor(e, 1);
        s[tm][r] = s[tm][r] * expf(m[tm][r] - ms) + e;
        m[tm][r] = mn;
      }
  }

  if (r16 == 0) {
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int b = b0 + 32 * wave + 16 * tm + 4 * q + r;
        if (b < B) {
          ws_m[(int64_t)blockIdx.y * B + b] = m[tm][r];
          ws_s[(int64_t)blockIdx.y * B + b] = s[tm][r];
        }
      }
  }
}

// ---------------------------------------------------------------- backward: D recomputed per tile, second product from registers
constexpr int KMAX = 256;     // padded K the register-resident accumulator is built for

struct RowInfo {
  float lse, gd, glp;   // gd = g_lse - g_lp
  int act;              // the action if it lies in [0, N), else -1
};

// KT: K rounded up to a multiple of 64 (64 .. 256).  DX: the dx kernel (A side = columns) else the dW / dc kernel (A side = rows).
// The fp32 dx kernel at KT <= 128 fits 256 registers (7 spilled) and with them two workgroups on a compute unit; every other variant
// needs more than half the register file for its output tile and runs one.
// blockIdx.y cuts the walk: DX, slices of the columns (tiles_per_part column tiles each); else chunks of the rows (tiles_per_part row
// tiles each).  Part y writes its own [rows or columns][ld_out] block of `out`, and its own [columns] block of dc.
template <typename T, int KT, bool DX, class Cols>
__global__ __launch_bounds__(256, (DX && KT <= 128 && sizeof(T) == 4) ? 2 : 1) void logprob_bwd_kernel(
                                                          const float* __restrict__ x, int64_t ldx, int B, int K,
                                                          const T* __restrict__ W, int64_t ldw, const Cols cols,
                                                          const int64_t* __restrict__ actions, const float* __restrict__ lse,
                                                          const float* __restrict__ g_lp, const float* __restrict__ g_lse,
                                                          int tiles_per_part, float* __restrict__ out, int64_t ld_out,
                                                          float* __restrict__ dc) {
  constexpr int NJ = KT / 16;       // 16-column blocks of the output; lane r16 owns columns NJ r16 .. NJ r16 + NJ - 1
  constexpr bool BF = sizeof(T) == 2;
  constexpr bool PICK = Cols::PICK;
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE_BYTES];
  __shared__ RowInfo ri[BM];
  __shared__ float cv[BN];
  __shared__ int cid[PICK ? 1 : BN];      // gathered columns: the table row behind each column of the tile, -1: absent
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, r16 = lane & 15;
  const int nk = K / Stage<T>::BK;
  const int NC = cols.count();
  const int t0 = blockIdx.y * tiles_per_part;
  const int t1 = min(((DX ? NC : B) + BM - 1) / BM, t0 + tiles_per_part);

  f32x4 o[2][NJ];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn)
#pragma unroll
    for (int j = 0; j < NJ; ++j) o[tn][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dcs[2] = {0.f, 0.f};

  Stage<T> st;
  for (int t = t0; t < t1; ++t) {
    const int b0 = (DX ? blockIdx.x : t) * BM, n0 = (DX ? t : blockIdx.x) * BN;
    f32x4 acc[8][2];
#pragma unroll
    for (int tm = 0; tm < 8; ++tm)
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};

    // per-row and per-column scalars of the tile (read after the k-loop's barriers; the barrier that ends the tile frees them again).
    // A row at or past B gets lse = +inf and an absent column gets c = -inf: p = exp(-inf) = 0 and D = 0 there.
    if (tid < BM) {
      const int b = b0 + tid;
      RowInfo r = {INFINITY, 0.f, 0.f, -1};
      if (b < B) {
        const int64_t a = actions[b];
        const bool ok = a >= 0 && a < cols.N;
        const float gl = g_lse ? g_lse[b] : 0.f;
        const float gp = (g_lp && ok) ? g_lp[b] : 0.f;
        float l = lse[b];
        if (!PICK && l == -INFINITY) l = INFINITY;      // a row with no live column at all: p = 0 everywhere
        r = RowInfo{l, gl - gp, gp, ok ? (int)a : -1};
      }
      ri[tid] = r;
    } else {
      const int n = n0 + tid - BM;
      const int64_t id = cols.row(n);
      cv[tid - BM] = id >= 0 ? cols.bias(n, id) : -INFINITY;
      if constexpr (!PICK) cid[tid - BM] = (int)id;
    }

    st.fetch(x, ldx, B, b0, W, ldw, cols, n0, 0, tid);
    stage_store<T, DX>(st, lds, tid);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const bool more = kt + 1 < nk;
      if (more) st.fetch(x, ldx, B, b0, W, ldw, cols, n0, (kt + 1) * Stage<T>::BK, tid);
      stage_mma<T, 8, 2>(lds + (kt & 1) * STAGE_BYTES, 0, BM + 32 * wave, q, r16, acc);
      if (more) stage_store<T, DX>(st, lds + ((kt + 1) & 1) * STAGE_BYTES, tid);
      __syncthreads();
    }

    // D in place of z: acc[tm][tn][r] is A-side row ia = 16 tm + 4 q + r, B-side column ib = 32 wave + 16 tn + r16
    RowInfo rb[2];    // DX: the lane's two batch rows
    float cb[2];      // else: the lane's two columns
    int idb[2] = {-1, -1};
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int ib = 32 * wave + 16 * tn + r16;
      if constexpr (DX) rb[tn] = ri[ib]; else cb[tn] = cv[ib];
      if constexpr (!DX && !PICK) idb[tn] = cid[ib];
    }
#pragma unroll
    for (int tm = 0; tm < 8; ++tm)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ia = 16 * tm + 4 * q + r;
        RowInfo ra;
        float ca;
        int ida = -1;
        if constexpr (DX) ca = cv[ia]; else ra = ri[ia];
        if constexpr (DX && !PICK) ida = cid[ia];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          const RowInfo R = DX ? rb[tn] : ra;
          const float cn = DX ? ca : cb[tn];
          const float p = expf(acc[tm][tn][r] + cn - R.lse);
          float d;
          if constexpr (PICK) {
            const int n = n0 + (DX ? ia : 32 * wave + 16 * tn + r16);
            d = R.gd * p + (R.act == n ? R.glp : 0.f);
          } else {
            d = (cols.drop_hits && R.act == (DX ? ida : idb[tn])) ? 0.f : R.gd * p;
          }
          acc[tm][tn][r] = d;
          if constexpr (!DX) dcs[tn] += d;
        }
      }

    // second product: o[tn] += D[:, tn block]^T V, V the A side's rows at full K (x rows for dW, W rows for dx).  vrow: the row of V
    // behind A-side row i of the tile, -1: none
    auto vrow = [&](int i) -> int64_t {
      if constexpr (!DX) return b0 + i < B ? b0 + i : -1;
      else if constexpr (PICK) return cols.row(n0 + i);
      else return cid[i];
    };
    if constexpr (!BF) {
      const float* V = DX ? (const float*)W : x;
      const int64_t ldv = DX ? ldw : ldx;
#pragma unroll
      for (int tm = 0; tm < 8; ++tm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t row = vrow(16 * tm + 4 * q + r);
          f32x4 v[NJ / 4];
#pragma unroll
          for (int jc = 0; jc < NJ / 4; ++jc) {
            const int k = NJ * r16 + 4 * jc;
            v[jc] = (row >= 0 && k < K) ? *(const f32x4*)(V + row * ldv + k) : f32x4{0.f, 0.f, 0.f, 0.f};
          }
#pragma unroll
          for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
              o[tn][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[tm][tn][r], v[j / 4][j % 4], o[tn][j], 0, 0, 0);
        }
    } else {
      // contraction slot jj (0..7) of k-step ks: A-side row 16 (2 ks + jj / 4) + 4 q + jj % 4
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        uint4 dfrag[2];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          const f32x4 lo = acc[2 * ks][tn], hi = acc[2 * ks + 1][tn];
          dfrag[tn] = make_uint4(cvt_pk_bf16(lo[0], lo[1]), cvt_pk_bf16(lo[2], lo[3]), cvt_pk_bf16(hi[0], hi[1]), cvt_pk_bf16(hi[2], hi[3]));
        }
        int64_t rows[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) rows[jj] = vrow(16 * (2 * ks + jj / 4) + 4 * q + jj % 4);
#pragma unroll
        for (int jc = 0; jc < NJ / 4; ++jc) {
          const int k = NJ * r16 + 4 * jc;
          uint4 vfrag[4];     // vfrag[e]: the 8 contraction rows of column k + e, as packed bf16 pairs
          if constexpr (DX) {
            uint2 v[8];       // 4 bf16 of W per row
#pragma unroll
            for (int jj = 0; jj < 8; ++jj)
              v[jj] = (rows[jj] >= 0 && k < K) ? *(const uint2*)((const bf16_t*)W + rows[jj] * ldw + k) : make_uint2(0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              uint32_t d[4];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const uint32_t s_lo = e < 2 ? v[2 * i].x : v[2 * i].y, s_hi = e < 2 ? v[2 * i + 1].x : v[2 * i + 1].y;
                d[i] = (e & 1) ? ((s_lo >> 16) | (s_hi & 0xFFFF0000u)) : ((s_lo & 0xFFFFu) | (s_hi << 16));
              }
              vfrag[e] = make_uint4(d[0], d[1], d[2], d[3]);
            }
          } else {
            f32x4 v[8];       // 4 floats of x per row, rounded in pairs of rows
#pragma unroll
            for (int jj = 0; jj < 8; ++jj)
              v[jj] = (rows[jj] >= 0 && k < K) ? *(const f32x4*)(x + rows[jj] * ldx + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e)
              vfrag[e] = make_uint4(cvt_pk_bf16(v[0][e], v[1][e]), cvt_pk_bf16(v[2][e], v[3][e]), cvt_pk_bf16(v[4][e], v[5][e]),
                                    cvt_pk_bf16(v[6][e], v[7][e]));
          }
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
              o[tn][4 * jc + e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, dfrag[tn]),
                                                                          __builtin_bit_cast(bf16x8, vfrag[e]), o[tn][4 * jc + e], 0, 0, 0);
        }
      }
    }
    __syncthreads();      // ri / cv / cid and the first stage are rewritten at the top of the next tile
  }

  // o[tn][j][i]: output row 32 wave + 16 tn + 4 q + i, column NJ r16 + j
  const int r0 = blockIdx.x * BM, rlim = DX ? B : NC;
  if (out) {
    float* dst = out + (int64_t)blockIdx.y * rlim * ld_out;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = r0 + 32 * wave + 16 * tn + 4 * q + i;
        if (row >= rlim) continue;
#pragma unroll
        for (int jc = 0; jc < NJ / 4; ++jc) {
          const int k = NJ * r16 + 4 * jc;
          if (k < K)
            *(f32x4*)(dst + (int64_t)row * ld_out + k) =
                f32x4{o[tn][4 * jc][i], o[tn][4 * jc + 1][i], o[tn][4 * jc + 2][i], o[tn][4 * jc + 3][i]};
        }
      }
  }
  if constexpr (!DX) {
    if (dc) {
#pragma unroll
      for (int tn = 0; tn < 2; ++tn) {
        float s = dcs[tn];
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const int n = r0 + 32 * wave + 16 * tn + r16;
        if (q == 0 && n < NC) dc[(int64_t)blockIdx.y * NC + n] = s;
      }
    }
  }
}

// out[r, k] = sum over the parts, in part order, of the partials [n_parts][R][K]
__global__ __launch_bounds__(256) void logprob_bwd_merge_kernel(const float* __restrict__ ws, int R, int K, int n_parts,
                                                                float* __restrict__ out, int64_t ld_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // one thread per 4 columns
  const int kq = K / 4;
  if (i >= (int64_t)R * kq) return;
  const int b = (int)(i / kq), k = (int)(i % kq) * 4;
  f32x4 s = *(const f32x4*)(ws + (int64_t)b * K + k);
  for (int sl = 1; sl < n_parts; ++sl) s += *(const f32x4*)(ws + ((int64_t)sl * R + b) * K + k);
  *(f32x4*)(out + (int64_t)b * ld_out + k) = s;
}

template <typename T, bool DX, class Cols, typename... A>
void launch_bwd(int K, dim3 grid, hipStream_t s, A... a) {
  switch ((K + 63) / 64) {
    case 1: hipLaunchKernelGGL((logprob_bwd_kernel<T, 64, DX, Cols>), grid, dim3(256), 0, s, a...); break;
    case 2: hipLaunchKernelGGL((logprob_bwd_kernel<T, 128, DX, Cols>), grid, dim3(256), 0, s, a...); break;
    case 3: hipLaunchKernelGGL((logprob_bwd_kernel<T, 192, DX, Cols>), grid, dim3(256), 0, s, a...); break;
    default: hipLaunchKernelGGL((logprob_bwd_kernel<T, 256, DX, Cols>), grid, dim3(256), 0, s, a...); break;
  }
}

}  // namespace
