// seq_grad.h -- what the backward calls of the two state encoders (lstm.hip: LSTM, gru.hip: GRU) share once their reverse chain has
// written the gate pre-activation gradients da of a chunk: the weight-gradient tiles, the dX contraction, the packed W_ih^T and the
// deterministic scatter-sum of the table gradient.  Everything here is written over the number of gate rows G (4H for the LSTM, 3H for
// the GRU) and the row stride lda of da; backward_impl of seq_bwd.h launches them.  The method:
//
//   weight gradients  per chunk, grid-wide: dW[m, n] = sum over the chunk's (user, step) samples of da[s, m] X[s, n], X = h_{t-1}
//                     rows (dW_hh) or table rows gathered through the store (dW_ih; [U, T, E] is never materialised).  One
//                     workgroup owns a 64 x 64 tile of dW and walks ALL samples in order, 16 per LDS stage, on the exact-f32 MFMA:
//                     no partial sums between workgroups.  The rating column of dW_ih and db are rank-1 / plain sums on the VALU
//                     of the same stage.  Chunks are added into dW in launch order (last chunk first).  No atomics anywhere.
//                     Only the rows of real users are walked: the clamped rows of a partly filled tile give nothing.
//                     (Which panel columns are a dW's rows is the cell's business: its launch_dw.)
//                     (dw_tile.h / gemm.h are bf16 tiles; the gradients here are exact f32, so they are not reused.)
//   table gradient   (recnn_*_backward_table only) d_table[item] = sum of dX[u, t, 0:E] over the call's positions (u, t) that hold
//                     `item`, dX[u, t, n] = sum_m da[u, t, m] W_ih[m, n].  dX: one launch per chunk after its chain launch, a grid
//                     over tiles of 16 samples (real users only), wave w of a workgroup owning column tiles w and w + 4, on the
//                     exact-f32 MFMA.  One accumulator per element, from zero; the contraction walks m in blocks of 16 upwards,
//                     four MFMAs e = 0 .. 3 per block, MFMA e adding the products m = m0 + e, m0 + 4 + e, m0 + 8 + e, m0 + 12 + e.
//                     W_ih[:, 0:E] (row stride E + 1: 4-byte aligned only) is read from a packed transposed copy [E][NG H] made
//                     once per call, so the contraction index is contiguous and a lane loads 16 bytes of either operand.  dX is
//                     written to a [U, T, E] buffer for the WHOLE call -- the one place where [U, T, E] is materialised -- so that
//                     the scatter's order does not depend on the chunk cut.  The scatter-sum runs once per call over the inverted
//                     index of scatter_index.h (stable counting sort by item id, per item its contributions in ascending
//                     j = u T + t; built before the chain starts, it does not depend on da): the sorted entries are cut into
//                     pieces of 16, a wave sums the run of each item inside its piece in list order from zero, and one wave per
//                     item adds the piece partials of its list in piece order from zero.  Every row of d_table is written
//                     (untouched items: exact zeros).  No float atomics.  Ids outside the table are in no list.
#pragma once
#include "scatter_index.h"
#include "seq_chain.h"

namespace {

// ------------------------------------------------------------------------------------------------ weight gradients
constexpr int DW_T = 64;            // output tile, rows (of G) and columns (of H or E)
constexpr int DW_S = 16;            // samples per stage
constexpr int DW_LD = DW_T + PAD;

struct DwArgs {
  SeqStore s;
  int t0;                           // the call's step 0 is position t0 of a history
  int U, T, H, tb, Tc, da_T;
  int G, lda;                       // rows of dW; floats per sample of da (lda >= G)
  int msplit, mshift;               // row m of dW reads column m of da, rows m >= msplit column m + mshift (the GRU's dW_hh: its last
                                    // third is da_hn, which sits behind da_n); msplit is a multiple of 4.  LSTM: msplit = G, mshift = 0
  const float* da;
  const float *h_out, *h0;          // dW_hh: X rows are h_{t-1}: h_out[u, t - 1], h0[u] (NULL: zeros) at the call's step 0
  float* out;                       // [G][ldo], columns 0 .. N - 1
  int ldo, N;
  float *d_wr, *d_b;                // the rating column (stride ldo; dW_ih only) and db; NULL: not wanted
  int accumulate;                   // add to out / d_wr / d_b (a later launch of the same call) or write them
};

// grid (ceil(G / 64), ceil(N / 64)), 256 threads: wave w owns rows 16 w .. 16 w + 15 of the tile and its four 16-column tiles.
// ROWS = false (the LSTM): G = 4H is a multiple of 64, row m reads column m, and db comes with dW_ih only.  ROWS = true (the GRU): G = 3H
// need not be a multiple of 64 (48, 144, ..) -- rows past G are staged as zeros and never written --, rows are mapped through msplit /
// mshift, and the dW_hh launch sums a db of its own.  A template parameter, not a run-time test: the LSTM's launches keep the
// instructions they had before the GRU came (the guards cost 3.7 % of its forward + backward at U = 256 when they were run-time).
template <bool IH, bool ROWS>
__global__ __launch_bounds__(256) void seq_dw_kernel(const DwArgs a) {
  __shared__ __attribute__((aligned(16))) float As[2][DW_S][DW_LD];
  __shared__ __attribute__((aligned(16))) float Xs[2][DW_S][DW_LD];
  __shared__ float Rs[2][DW_S];
  const int H = a.H, G = a.G, N = a.N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * DW_T, n0 = blockIdx.y * DW_T;
  const int S = a.U * a.Tc, nb = (S + DW_S - 1) / DW_S;
  const int sr = tid >> 4, sc = tid & 15;     // the stager: sample row sr of a stage, 16-byte chunk sc of both operands
  const bool xcol = n0 + 4 * sc < N;          // (N is a multiple of 4)
  const int mrow = m0 + 4 * sc;               // (G and msplit are multiples of 4: a chunk lies on one side of either)
  const bool arow = !ROWS || mrow < G;
  const int acol = ROWS ? mrow + (mrow >= a.msplit ? a.mshift : 0) : mrow;
  const bool extras = (IH || ROWS) && blockIdx.y == 0 && (a.d_wr || a.d_b);

  auto fetch = [&](int b, float4& av, float4& xv, float& rv) {
    const int s = b * DW_S + sr;
    av = make_float4(0.f, 0.f, 0.f, 0.f);
    xv = av;
    rv = 0.f;
    if (s >= S) return;
    const int u = s / a.Tc, tl = s - u * a.Tc, t = a.tb + tl;
    if (arow) av = *(const float4*)(a.da + ((int64_t)u * a.da_T + tl) * a.lda + acol);
    if constexpr (IH) {
      const StorePos p = store_pos(a.s, u, a.t0 + t);
      if (xcol) xv = p.live() ? table_chunk(a.s, a.s.items[p.pos], (n0 >> 2) + sc) : nan4();
      if (sc == 0) rv = p.live() ? a.s.ratings[p.pos] : __builtin_nanf("");
    } else {
      if (xcol) {
        if (t >= 1) xv = *(const float4*)(a.h_out + ((int64_t)u * a.T + t - 1) * H + n0 + 4 * sc);
        else if (a.h0) xv = *(const float4*)(a.h0 + (int64_t)u * H + n0 + 4 * sc);
      }
    }
  };
  auto put = [&](int buf, const float4& av, const float4& xv, float rv) {
    *(float4*)&As[buf][sr][4 * sc] = av;
    *(float4*)&Xs[buf][sr][4 * sc] = xv;
    if (IH && sc == 0) Rs[buf][sr] = rv;
  };

  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4] = {zero4, zero4, zero4, zero4};
  float bsum = 0.f, rsum = 0.f;
  float4 av, xv;
  float rv;
  if (nb > 0) {
    fetch(0, av, xv, rv);
    put(0, av, xv, rv);
  }
  __syncthreads();
  for (int b = 0; b < nb; ++b) {
    const int buf = b & 1;
    if (b + 1 < nb) fetch(b + 1, av, xv, rv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float am = As[buf][4 * g + e][16 * wave + r];
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) {
        if (n0 + 16 * tn >= N) continue;
        acc[tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(am, Xs[buf][4 * g + e][16 * tn + r], acc[tn], 0, 0, 0);
      }
    }
    if (extras && tid < DW_T) {       // db and the rating column of this tile's rows: plain sums in sample order
#pragma unroll
      for (int s = 0; s < DW_S; ++s) {
        const float d = As[buf][s][tid];
        bsum += d;
        if constexpr (IH) rsum = fmaf(d, Rs[buf][s], rsum);
      }
    }
    if (b + 1 < nb) put(buf ^ 1, av, xv, rv);
    __syncthreads();
  }
  if (a.out) {
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      const int n = n0 + 16 * tn + r;
      if (n >= N) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + 16 * wave + 4 * g + i;
        if (ROWS && m >= G) continue;
        float* o = a.out + (int64_t)m * a.ldo + n;
        *o = a.accumulate ? *o + acc[tn][i] : acc[tn][i];
      }
    }
  }
  if (extras && tid < DW_T && (!ROWS || m0 + tid < G)) {
    const int m = m0 + tid;
    if (a.d_b) a.d_b[m] = a.accumulate ? a.d_b[m] + bsum : bsum;
    if (IH && a.d_wr) a.d_wr[(int64_t)m * a.ldo] = a.accumulate ? a.d_wr[(int64_t)m * a.ldo] + rsum : rsum;
  }
}

// ------------------------------------------------------------------------------------------------ table gradient
// wp[n][m] = w_ih[m][n], n < E: W_ih without its rating column, transposed and packed
__global__ __launch_bounds__(256) void seq_wih_pack_kernel(const float* __restrict__ w, int E, int G, float* __restrict__ wp) {
  flat_walk<1>((int64_t)E * G, [&](int64_t i, Width<1>) {
    const int n = (int)(i / G), m = (int)(i - (int64_t)n * G);
    wp[i] = w[(int64_t)m * (E + 1) + n];
  });
}

constexpr int DX_S = 16;            // samples per workgroup
constexpr int DX_WV = 4;            // waves per workgroup

struct DxArgs {
  int U, T, E, tb, Tc, da_T;
  int G, lda;                       // the contraction runs over columns 0 .. G - 1 of da (a multiple of 16); floats per sample of da
  const float* da;                  // the chunk's [..][da_T][lda]
  const float* wp;                  // [E][G]
  float* dx;                        // [U][T][E]
};

// grid ceil(U Tc / 16), min(4, ceil(E / 16)) waves: sample s = u Tc + tl of the chunk (u < U: real users only); wave w owns columns 16 w .. 16 w + 15
// and 16 (w + 4) .. of the 16 samples.  Both operands come straight from global memory, 16 bytes per lane, the next block's loads
// issued ahead of this block's products (the four waves read the same da rows: they meet in the cache).
__global__ __launch_bounds__(64 * DX_WV) void seq_dx_kernel(const DxArgs a) {
  const int G = a.G, E = a.E;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int S = a.U * a.Tc, s0 = blockIdx.x * DX_S;
  const int ntiles = (E + 15) >> 4;
  if (wave >= ntiles) return;                          // (wave-uniform; the kernel has no barrier)
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const bool alive = s0 + r < S;
  const int ua = alive ? (s0 + r) / a.Tc : 0, tla = alive ? s0 + r - ua * a.Tc : 0;
  const float* arow = a.da + ((int64_t)ua * a.da_T + tla) * a.lda + 4 * g;
  bool on[2], bl[2];
  const float* brow[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = (wave + DX_WV * j) * 16 + r;
    on[j] = wave + DX_WV * j < ntiles;
    bl[j] = on[j] && n < E;                            // E is a multiple of 8: the last column tile may be half empty
    brow[j] = a.wp + (int64_t)(bl[j] ? n : 0) * G + 4 * g;
  }
  f32x4 acc[2] = {zero4, zero4};
  f32x4 an = alive ? *(const f32x4*)arow : zero4, bn[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) bn[j] = bl[j] ? *(const f32x4*)brow[j] : zero4;
  for (int k0 = 0; k0 < G; k0 += 16) {
    const f32x4 av = an;
    f32x4 bv[2];
    const int kn = k0 + 16 < G ? k0 + 16 : k0;
    an = alive ? *(const f32x4*)(arow + kn) : zero4;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      bv[j] = bn[j];
      bn[j] = bl[j] ? *(const f32x4*)(brow[j] + kn) : zero4;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[0][e], acc[0], 0, 0, 0);
      if (on[1]) acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[1][e], acc[1], 0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!bl[j]) continue;
    const int n = (wave + DX_WV * j) * 16 + r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int s = s0 + 4 * g + i;
      if (s >= S) continue;
      const int u = s / a.Tc, tl = s - u * a.Tc;
      a.dx[((int64_t)u * a.T + a.tb + tl) * E + n] = acc[j][i];
    }
  }
}

// contribution j = u T + t of a call: the item at position t0 + t of user u's history (the encode's clamp; the host refuses steps
// past a history's end)
struct StoreId {
  const int32_t* items;
  const int64_t* user_off;
  const int32_t* slots;
  int T, t0;
  __device__ int64_t operator()(int j) const {
    const int u = j / T, t = j - u * T;
    const StorePos p = store_pos(slots, user_off, u, t0 + t);
    return p.live() ? (int64_t)items[p.pos] : -1;
  }
};

constexpr int TG_PIECE = 16;        // scatter-sum: sorted entries per wave in the first pass
// pass 1: one wave per TG_PIECE sorted entries; the run of each item inside the piece is summed in list order and written at the
// run's first sorted position.  Lanes own columns lane and lane + 64 (E <= 128).
__global__ __launch_bounds__(256) void table_piece_kernel(const float* __restrict__ dx, int E, const StoreId id_of,
                                                          const int* __restrict__ sorted, const int* __restrict__ total_ptr,
                                                          float* __restrict__ part) {
  const int total = *total_ptr;
  const int piece = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int p0 = piece * TG_PIECE;
  if (p0 >= total) return;
  const int p1 = min(total, p0 + TG_PIECE);
  const bool c0 = lane < E, c1 = lane + 64 < E;
  float a0 = 0.f, a1 = 0.f;
  int first = p0;
  int cur = (int)id_of(sorted[p0]);
  for (int p = p0; p < p1; ++p) {
    const float* s = dx + (int64_t)sorted[p] * E;
    if (c0) a0 += s[lane];
    if (c1) a1 += s[lane + 64];
    const int nxt = p + 1 < p1 ? (int)id_of(sorted[p + 1]) : -1;
    if (nxt != cur) {
      if (c0) part[(int64_t)first * E + lane] = a0;
      if (c1) part[(int64_t)first * E + lane + 64] = a1;
      a0 = a1 = 0.f;
      first = p + 1;
      cur = nxt;
    }
  }
}
// pass 2: one wave per item, the pieces of its list in order; an item nothing reached gets zeros
__global__ __launch_bounds__(256) void table_merge_kernel(const int* __restrict__ start, int n_items, int E, const float* __restrict__ part,
                                                          float* __restrict__ out) {
  const int d = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (d >= n_items) return;
  const int s = start[d], e = start[d + 1];
  const bool c0 = lane < E, c1 = lane + 64 < E;
  float a0 = 0.f, a1 = 0.f;
  if (e > s) {
    for (int k = s / TG_PIECE; k <= (e - 1) / TG_PIECE; ++k) {
      const int at = max(s, k * TG_PIECE);
      if (c0) a0 += part[(int64_t)at * E + lane];
      if (c1) a1 += part[(int64_t)at * E + lane + 64];
    }
  }
  if (c0) out[(int64_t)d * E + lane] = a0;
  if (c1) out[(int64_t)d * E + lane + 64] = a1;
}

// workspace of the table gradient: packed W_ih^T [E][G], dX of the whole call, the inverted index, the piece partials (each rounded
// up to 256 bytes)
struct TableWs {
  int64_t wp, dx, index, part, total;    // byte offsets
};
inline TableWs table_ws(int n_users, int T, int G, int E, int n_items) {
  const int64_t M = (int64_t)n_users * T;
  TableWs w;
  w.wp = 0;
  w.dx = scatter_index_round((int64_t)E * G * 4);
  w.index = w.dx + scatter_index_round(M * E * 4);
  w.part = w.index + scatter_index_bytes(M, n_items);
  w.total = w.part + scatter_index_round(M * E * 4);
  return w;
}

// The table gradient's launches around the chunk loop of a backward call: what does not depend on da (prepare, before the chain
// starts), dX of one chunk (after its chain launch), and the scatter-sum (after the last chunk).
struct TableGrad {
  DxArgs dx;
  ScatterIndex ix;
  StoreId id_of;
  float* part;
  int M, n_items;
};
inline hipError_t table_grad_prepare(TableGrad& tg, const SeqStore& st, int t0, int T, int G, int lda, int da_T, const float* da,
                                     const float* w_ih, void* table_workspace, hipStream_t s) {
  const int U = st.n_users, E = st.E;
  tg.id_of = StoreId{st.items, st.user_off, st.slots, T, t0};
  tg.M = U * T;                                        // (checked below 2^31 by the caller)
  tg.n_items = st.n_items;
  const TableWs tw = table_ws(U, T, G, E, st.n_items);
  char* tp = (char*)table_workspace;
  tg.dx = DxArgs{};
  tg.dx.U = U; tg.dx.T = T; tg.dx.E = E; tg.dx.da_T = da_T; tg.dx.G = G; tg.dx.lda = lda;
  tg.dx.da = da;
  tg.dx.wp = (const float*)(tp + tw.wp);
  tg.dx.dx = (float*)(tp + tw.dx);
  tg.part = (float*)(tp + tw.part);
  char* ip = tp + tw.index;
  tg.ix = scatter_index_carve(ip, tg.M, st.n_items);
  hipLaunchKernelGGL(seq_wih_pack_kernel, dim3(grid_for((int64_t)E * G, 256, 2048)), dim3(256), 0, s, w_ih, E, G, (float*)(tp + tw.wp));
  return scatter_index_build(tg.ix, tg.id_of, tg.M, st.n_items, s);
}
inline void table_grad_chunk(TableGrad& tg, int tb, int Tc, hipStream_t s) {
  tg.dx.tb = tb; tg.dx.Tc = Tc;
  const int E = tg.dx.E;
  const int dx_waves = (E + 15) / 16 < DX_WV ? (E + 15) / 16 : DX_WV;      // E <= 48: no wave without a column tile
  hipLaunchKernelGGL(seq_dx_kernel, dim3((tg.dx.U * Tc + DX_S - 1) / DX_S), dim3(64 * dx_waves), 0, s, tg.dx);
}
inline void table_grad_finish(const TableGrad& tg, float* d_table, hipStream_t s) {
  // (dropped ids are not in the lists: the pieces cover the first start[n_items] sorted entries)
  const int pieces = (tg.M + TG_PIECE - 1) / TG_PIECE;
  hipLaunchKernelGGL(table_piece_kernel, dim3((pieces + 3) / 4), dim3(256), 0, s, tg.dx.dx, tg.dx.E, tg.id_of, tg.ix.sorted,
                     tg.ix.start + tg.n_items, tg.part);
  hipLaunchKernelGGL(table_merge_kernel, dim3((tg.n_items + 3) / 4), dim3(256), 0, s, tg.ix.start, tg.n_items, tg.dx.E, tg.part, d_table);
}

}  // namespace
