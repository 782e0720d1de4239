// gru.hip -- a GRU state encoder over whole user histories: the second recurrent cell of the dynamic-length path (seq.hip has the
// first, an LSTM, and describes the chain layout this file follows).
//
//   cell             torch.nn.GRU(E + 1, H), one layer, one direction, gate order r, z, n, weights read in place:
//                      r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)     z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
//                      hn = W_hn h + b_hn                             n = tanh(W_in x + b_in + r hn)
//                      h' = (1 - z) n + z h                           (computed as n + z (h - n))
//   forward chain    the LSTM's layout (seq_lstm.h): 16 users per workgroup, 8 waves, wave w owns hidden tiles w and w + 8, exact-f32
//                    MFMA, x rows staged one step ahead through the store, W_hh streamed from L2 with the next k block's loads issued
//                    ahead.  FOUR accumulators per hidden tile: r, z, nx (the input links of n) and nh (the h products of n, started
//                    from b_hn) -- the two halves of n meet only after r is known, so they cannot share one.  r and z are one
//                    fixed-order chain each: fma(rating, w_ih[:, E], b_ih + b_hh), the x products, the h products.  nx:
//                    fma(rating, w_ih[:, E], b_ih), the x products.  nh: b_hh, the h products.  A step issues three h-product
//                    MFMAs per k where the LSTM issues four.  h_{t-1} of a lane's own (user, hidden unit) pairs stays in registers.
//     variant 0      the input links are computed inside the step.
//     variant 1      a grid-wide launch per chunk of LSTM_CHUNK steps writes r, z and nx after their input links into a workspace of
//                    three gates in accumulator layout; the chain launch starts from them.  The same chains: the same bits.
//   training forward the same arithmetic plus one 16-byte store per lane and saved quantity: r, z, n and hn in accumulator order.
//                    h_{t-1} is read back from h_out / h0.
//   reverse chain    one workgroup owns the same 16 users and walks the steps downwards; the gate derivatives are lane-local:
//                      dh = g_h[:, t] + dh_rec (+ g_hT at the call's last step)
//                      da_n = dh (1 - z)(1 - n^2)     da_z = dh (h_{t-1} - n) z (1 - z)
//                      da_r = da_n hn r (1 - r)       da_hn = da_n r
//                      dh_rec = dh z + [da_r | da_z | da_hn] . W_hh
//                    The panel [16][4H] = da_r, da_z, da_n, da_hn of a step is staged in LDS (double-buffered, the LSTM's budget) and
//                    copied to the chunk's workspace; dh_rec runs on the exact-f32 MFMA from W_hh^T [H][3H] (made once per call),
//                    one accumulator per gate, added ((r + z) + hn) + dh z.  dh passes between chunk launches through a [U, H]
//                    buffer in stream order.
//   weight gradients the kernels of seq_grad.h over G = 3H rows: dW_ih and db_ih from columns [da_r | da_z | da_n] of the panel, dW_hh
//                    and db_hh from [da_r | da_z | da_hn]: the two bias gradients differ in their last third.
//   table gradient   dX = [da_r | da_z | da_n] . W_ih[:, :E] per chunk into a [U, T, E] buffer of the whole call, then the one
//                    scatter-sum over the inverted index (seq_grad.h, scatter_index.h).  No float atomics.
#include "seq_grad.h"

namespace {

constexpr int GRU_PRE_Q = 3;      // r, z, nx
constexpr int GRU_SAVED_Q = 4;    // r, z, n, hn

// [user tile][T][H / 16][nq][64 lanes] f32x4, accumulator order: lane (r, g), element i = user 4 g + i of the tile, hidden unit 16 jt + r
__device__ __forceinline__ int64_t gru_index(int tile, int T, int t, int ntiles, int jt, int nq, int q, int lane) {
  return ((((int64_t)tile * T + t) * ntiles + jt) * nq + q) * 64 + lane;
}

// EncArgs as for the LSTM; c0 / c_T are not used.  pre: GRU_PRE_Q gates, saved: GRU_SAVED_Q quantities.
template <int TPW, bool PRE, bool SAVE>
__global__ __launch_bounds__(NT) void gru_encode_kernel(const EncArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int E = a.s.E, H = a.H, U = a.s.n_users, T = a.T;
  const int KX = (E + 15) & ~15, ldx = KX + PAD, ldh = H + PAD, ntiles = H >> 4;
  float* xb = smem;                    // [2][16][ldx]
  float* hb = xb + 2 * MT * ldx;       // [2][16][ldh]
  float* rb = hb + 2 * MT * ldh;       // [2][16]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int u0 = blockIdx.x * MT;
  const Stager st(a.s, u0, tid);
  const bool xlive = !PRE && 4 * st.sc < E;

  int jt[TPW];
  bool on[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    jt[j] = wave + NWV * j;
    on[j] = jt[j] < ntiles;
  }

  // ---- prologue: h_{t0 - 1} into LDS and, for the lane's own pairs, into registers; x and rating of the first step, the id of the second
  for (int i = tid; i < MT * H; i += NT) {
    const int uu = i / H, j = i - uu * H;
    hb[uu * ldh + j] = a.h0 ? a.h0[(int64_t)min(u0 + uu, U - 1) * H + j] : 0.f;
  }
  f32x4 hl[TPW];
  float bhn[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      hl[j][i] = (a.h0 && on[j]) ? a.h0[(int64_t)min(u0 + 4 * g + i, U - 1) * H + jt[j] * 16 + r] : 0.f;
    bhn[j] = on[j] ? a.b_hh[2 * H + jt[j] * 16 + r] : 0.f;
  }
  int idn = -1;
  if (!PRE) {
    if (4 * st.sc >= E && 4 * st.sc < KX) {     // zero columns E .. KX - 1 of both panels, once
      *(float4*)(xb + st.su * ldx + 4 * st.sc) = make_float4(0.f, 0.f, 0.f, 0.f);
      *(float4*)(xb + MT * ldx + st.su * ldx + 4 * st.sc) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (xlive) *(float4*)(xb + st.su * ldx + 4 * st.sc) = table_chunk(a.s, st.id(a.s, a.t0), st.sc);
    if (st.sc == 0) rb[st.su] = st.rating(a.s, a.t0);
    if (xlive && T > 1) idn = st.id(a.s, a.t0 + 1);
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const int cur = t & 1;
    const float* xs = xb + cur * MT * ldx;
    const float* hs = hb + cur * MT * ldh;
    float* hnew = hb + (cur ^ 1) * MT * ldh;
    // ---- the next step's x row and rating, and the id of the step after it, in flight under this step's products
    float4 xn = make_float4(0.f, 0.f, 0.f, 0.f);
    float rn = 0.f;
    int idn2 = -1;
    const bool more = !PRE && t + 1 < T;
    if (more && xlive) xn = table_chunk(a.s, idn, st.sc);
    if (more && st.sc == 0) rn = st.rating(a.s, a.t0 + t + 1);
    if (!PRE && xlive && t + 2 < T) idn2 = st.id(a.s, a.t0 + t + 2);

    f32x4 acc[TPW][4];                  // r, z, nx, nh
    if constexpr (PRE) {
#pragma unroll
      for (int j = 0; j < TPW; ++j)
        if (on[j])
#pragma unroll
          for (int q = 0; q < GRU_PRE_Q; ++q)
            acc[j][q] = ((const f32x4*)a.pre)[gru_index(blockIdx.x, T, t, ntiles, jt[j], GRU_PRE_Q, q, lane)];
    } else {
      input_links<TPW, GRU_PRE_Q>(a, xs, rb + cur * MT, ldx, jt, on, acc, lane);
    }
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[j][3][i] = bhn[j];
    // ---- the H products of h_{t-1}: W_hh row blocks r, z, n into acc 0, 1, 3
    const float* wrow[TPW][3];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
      for (int q = 0; q < 3; ++q) wrow[j][q] = a.w_hh + (int64_t)(q * H + (on[j] ? jt[j] : 0) * 16 + r) * H + 4 * g;
    f32x4 bn[TPW][3];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
      for (int q = 0; q < 3; ++q) bn[j][q] = *(const f32x4*)(wrow[j][q]);
    for (int k0 = 0; k0 < H; k0 += 16) {
      const f32x4 av = *(const f32x4*)(hs + r * ldh + k0 + 4 * g);
      f32x4 bv[TPW][3];
      const int kn = k0 + 16 < H ? k0 + 16 : k0;
#pragma unroll
      for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          bv[j][q] = bn[j][q];
          bn[j][q] = *(const f32x4*)(wrow[j][q] + kn);
        }
#pragma unroll
      for (int j = 0; j < TPW; ++j) {
        if (!on[j]) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[j][0][e], acc[j][0], 0, 0, 0);
          acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[j][1][e], acc[j][1], 0, 0, 0);
          acc[j][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[j][2][e], acc[j][3], 0, 0, 0);
        }
      }
    }
    // ---- cell update: lane (r, g) holds users 4g .. 4g + 3 of hidden unit 16 jt + r
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      if (!on[j]) continue;
      const int hid = jt[j] * 16 + r;
      [[maybe_unused]] f32x4 sv[3];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float rg = sigmoidf_(acc[j][0][i]), zg = sigmoidf_(acc[j][1][i]);
        const float ng = tanhf(fmaf(rg, acc[j][3][i], acc[j][2][i]));
        if constexpr (SAVE) { sv[0][i] = rg; sv[1][i] = zg; sv[2][i] = ng; }
        const float hv = fmaf(zg, hl[j][i] - ng, ng);
        hl[j][i] = hv;
        hnew[(4 * g + i) * ldh + hid] = hv;
        const int u = u0 + 4 * g + i;
        if (u < U) a.h_out[((int64_t)u * a.T_out + a.t_out0 + t) * H + hid] = hv;
      }
      if constexpr (SAVE) {
        f32x4* dst = (f32x4*)a.saved + gru_index(blockIdx.x, a.T_out, a.t_out0 + t, ntiles, jt[j], GRU_SAVED_Q, 0, lane);
#pragma unroll
        for (int q = 0; q < 3; ++q) dst[64 * q] = sv[q];
        dst[64 * 3] = acc[j][3];
      }
    }
    if (more) {
      if (xlive) *(float4*)(xb + (cur ^ 1) * MT * ldx + st.su * ldx + 4 * st.sc) = xn;
      if (st.sc == 0) rb[(cur ^ 1) * MT + st.su] = rn;
    }
    idn = idn2;
    __syncthreads();
  }

  if (T > 0) {
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      if (!on[j]) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int u = u0 + 4 * g + i;
        if (u < U) a.h_T[(int64_t)u * H + jt[j] * 16 + r] = hl[j][i];
      }
    }
  }
}

// variant 1, grid (user tiles, steps of the chunk): the input links of r, z and nx of step t0 + blockIdx.y for 16 users, into a.pre
template <int TPW>
__global__ __launch_bounds__(NT) void gru_project_kernel(const EncArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int E = a.s.E, KX = (E + 15) & ~15, ldx = KX + PAD, ntiles = a.H >> 4;
  float* xs = smem;              // [16][ldx]
  float* rs = xs + MT * ldx;     // [16]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, t = blockIdx.y;
  const Stager st(a.s, blockIdx.x * MT, tid);
  if (4 * st.sc < KX)
    *(float4*)(xs + st.su * ldx + 4 * st.sc) =
        4 * st.sc < E ? table_chunk(a.s, st.id(a.s, a.t0 + t), st.sc) : make_float4(0.f, 0.f, 0.f, 0.f);
  if (st.sc == 0) rs[st.su] = st.rating(a.s, a.t0 + t);
  int jt[TPW];
  bool on[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    jt[j] = wave + NWV * j;
    on[j] = jt[j] < ntiles;
  }
  __syncthreads();
  f32x4 acc[TPW][4];
  input_links<TPW, GRU_PRE_Q>(a, xs, rs, ldx, jt, on, acc, lane);
#pragma unroll
  for (int j = 0; j < TPW; ++j)
    if (on[j])
#pragma unroll
      for (int q = 0; q < GRU_PRE_Q; ++q)
        ((f32x4*)a.pre)[gru_index(blockIdx.x, a.T, t, ntiles, jt[j], GRU_PRE_Q, q, lane)] = acc[j][q];
}

inline int chunk_steps(int T) { return T < LSTM_CHUNK ? T : LSTM_CHUNK; }
inline int64_t gru_pre_bytes(int n_users, int T, int H) {
  return (int64_t)user_tiles(n_users) * chunk_steps(T) * (H / 16) * GRU_PRE_Q * 64 * (int64_t)sizeof(f32x4);
}
inline int64_t gru_saved_bytes(int n_users, int T, int H) {
  return (int64_t)user_tiles(n_users) * T * (H / 16) * GRU_SAVED_Q * 64 * (int64_t)sizeof(f32x4);
}

// The launches of one encode call.  variant 1: per chunk one projection launch and one chain launch; the state passes through h_T.
template <bool SAVE>
inline void launch_gru_encode(EncArgs a, int t0, int T, const float* h0, int variant, hipStream_t s) {
  const int emb_dim = a.s.E, hidden = a.H;
  a.T_out = T;
  const dim3 grid(user_tiles(a.s.n_users));
  const bool two = hidden > 16 * NWV;
  const size_t lds = encode_lds(emb_dim, hidden);
  if (variant == 0 || T == 0) {
    a.t0 = t0; a.T = T; a.t_out0 = 0; a.h0 = h0;
    if (two) hipLaunchKernelGGL((gru_encode_kernel<2, false, SAVE>), grid, dim3(NT), lds, s, a);
    else hipLaunchKernelGGL((gru_encode_kernel<1, false, SAVE>), grid, dim3(NT), lds, s, a);
    return;
  }
  for (int done = 0; done < T; done += LSTM_CHUNK) {
    a.t0 = t0 + done;
    a.T = T - done < LSTM_CHUNK ? T - done : LSTM_CHUNK;
    a.t_out0 = done;
    a.h0 = done ? a.h_T : h0;
    const dim3 pgrid(grid.x, a.T);
    if (two) {
      hipLaunchKernelGGL((gru_project_kernel<2>), pgrid, dim3(NT), project_lds(emb_dim), s, a);
      hipLaunchKernelGGL((gru_encode_kernel<2, true, SAVE>), grid, dim3(NT), lds, s, a);
    } else {
      hipLaunchKernelGGL((gru_project_kernel<1>), pgrid, dim3(NT), project_lds(emb_dim), s, a);
      hipLaunchKernelGGL((gru_encode_kernel<1, true, SAVE>), grid, dim3(NT), lds, s, a);
    }
  }
}

// ------------------------------------------------------------------------------------------------ W_hh^T
__global__ __launch_bounds__(256) void gru_whh_transpose_kernel(const float* __restrict__ w, int H, float* __restrict__ wt) {
  const int G = 3 * H;
  flat_walk<1>((int64_t)H * G, [&](int64_t i, Width<1>) {
    const int j = (int)(i / G), k = (int)(i - (int64_t)j * G);
    wt[i] = w[(int64_t)k * H + j];
  });
}

// ------------------------------------------------------------------------------------------------ reverse chain
struct GruBwdArgs {
  int U, T, H;                       // T: steps of the whole call (saved, h_out and g_h are [.., T, ..])
  int tb, Tc;                        // this launch walks the call's steps tb + Tc - 1 down to tb
  const float* saved;
  const float* w_hhT;                // [H][3H]
  const float *h_out, *h0, *g_h, *g_hT;
  const float* dh_in;                // [U][H] from the launch of the later chunk; NULL: zeros (the call's last chunk)
  float* dh_out;                     // [U][H]: d h_{tb - 1}
  float* da;                         // [user tiles * 16][da_T][4H]: this chunk's da_r, da_z, da_n, da_hn; NULL: not wanted
  int da_T;
};

inline size_t gru_bwd_lds(int H) { return (size_t)2 * MT * (4 * H + PAD) * sizeof(float); }

template <int TPW>
__global__ __launch_bounds__(NT) void gru_bwd_chain_kernel(const GruBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = a.H, U = a.U, P = 4 * H, G = 3 * H, ldd = P + PAD, ntiles = H >> 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int u0 = blockIdx.x * MT;

  int jt[TPW];
  bool on[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    jt[j] = wave + NWV * j;
    on[j] = jt[j] < ntiles;
  }
  bool live[4];                       // rows past the batch are the forward's clamped copies of user U - 1: they give nothing
  int uc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    live[i] = u0 + 4 * g + i < U;
    uc[i] = min(u0 + 4 * g + i, U - 1);
  }
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const f32x4* sv = (const f32x4*)a.saved;

  // what a step reads: r, z, n, hn and h_{t-1} of the lane's pairs, and g_h[u, t]
  auto load_gates = [&](int t, f32x4 (&gt)[TPW][4]) {
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        gt[j][q] = on[j] ? sv[gru_index(blockIdx.x, a.T, t, ntiles, jt[j], GRU_SAVED_Q, q, lane)] : zero4;
  };
  auto load_hprev = [&](int t, f32x4 (&hv)[TPW]) {      // h_{t-1}; t = 0: h0 (or zero)
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      hv[j] = zero4;
      if (!on[j]) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (t >= 1) hv[j][i] = a.h_out[((int64_t)uc[i] * a.T + t - 1) * H + jt[j] * 16 + r];
        else if (a.h0) hv[j][i] = a.h0[(int64_t)uc[i] * H + jt[j] * 16 + r];
      }
    }
  };
  auto load_gh = [&](int t, f32x4 (&gv)[TPW]) {
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      gv[j] = zero4;
      if (!on[j] || !a.g_h) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (live[i]) gv[j][i] = a.g_h[((int64_t)uc[i] * a.T + t) * H + jt[j] * 16 + r];
    }
  };

  // ---- prologue: the state handed over by the later chunk, and the first step's operands
  f32x4 dhr[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    dhr[j] = zero4;
    if (!on[j] || !a.dh_in) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (live[i]) dhr[j][i] = a.dh_in[(int64_t)uc[i] * H + jt[j] * 16 + r];
  }
  const int t_last = a.tb + a.Tc - 1;
  const bool call_end = t_last == a.T - 1;            // the call's last step takes g_hT
  f32x4 gt[TPW][4], hp[TPW], gh[TPW];
  load_gates(t_last, gt);
  load_hprev(t_last, hp);
  load_gh(t_last, gh);

  // W_hh^T row of the lane's hidden unit; gate blocks r, z, n of its 3H columns meet panel columns 0, H and 3H (da_hn)
  const float* wrow[TPW][3];
#pragma unroll
  for (int j = 0; j < TPW; ++j)
#pragma unroll
    for (int q = 0; q < 3; ++q) wrow[j][q] = a.w_hhT + (int64_t)((on[j] ? jt[j] : 0) * 16 + r) * G + q * H + 4 * g;
  const int pcol[3] = {0, H, 3 * H};

  for (int tl = a.Tc - 1; tl >= 0; --tl) {
    const int t = a.tb + tl;
    float* ds = smem + ((tl & 1) ? MT * ldd : 0);
    f32x4 dhz[TPW];
    // ---- gate derivatives of the lane's pairs -> the panel in LDS
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      dhz[j] = zero4;
      if (!on[j]) continue;
      const int hid = jt[j] * 16 + r;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float rg = gt[j][0][i], zg = gt[j][1][i], ng = gt[j][2][i], hn = gt[j][3][i];
        float dh = gh[j][i] + dhr[j][i];
        if (call_end && tl == a.Tc - 1 && a.g_hT && live[i]) dh += a.g_hT[(int64_t)uc[i] * H + hid];
        const float da_n = dh * (1.f - zg) * (1.f - ng * ng);
        const float da_z = dh * (hp[j][i] - ng) * zg * (1.f - zg);
        const float da_r = da_n * hn * rg * (1.f - rg);
        const float da_hn = da_n * rg;
        dhz[j][i] = live[i] ? dh * zg : 0.f;
        float* row = ds + (4 * g + i) * ldd + hid;
        row[0] = live[i] ? da_r : 0.f;
        row[H] = live[i] ? da_z : 0.f;
        row[2 * H] = live[i] ? da_n : 0.f;
        row[3 * H] = live[i] ? da_hn : 0.f;
      }
    }
    __syncthreads();
    // ---- the next (earlier) step's operands, in flight under this step's products
    if (tl > 0) {
      load_gates(t - 1, gt);
      load_hprev(t - 1, hp);
      load_gh(t - 1, gh);
    }
    // ---- the panel of this step -> the chunk's workspace, for the weight gradients and dX
    if (a.da) {
      const int P4 = P >> 2;
      for (int idx = tid; idx < MT * P4; idx += NT) {
        const int row = idx / P4, c4 = idx - row * P4;
        *(float4*)(a.da + ((int64_t)(u0 + row) * a.da_T + tl) * P + 4 * c4) = *(const float4*)(ds + row * ldd + 4 * c4);
      }
    }
    // ---- dh_rec[16, H] = dh z + [da_r | da_z | da_hn][16, 3H] . W_hh: one accumulator per gate block, one hidden tile at a time
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      if (!on[j]) continue;
      f32x4 acc[3], bn[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        acc[q] = zero4;
        bn[q] = *(const f32x4*)(wrow[j][q]);
      }
      for (int k0 = 0; k0 < H; k0 += 16) {
        f32x4 av[3], bv[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) av[q] = *(const f32x4*)(ds + r * ldd + pcol[q] + k0 + 4 * g);
        const int kn = k0 + 16 < H ? k0 + 16 : k0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          bv[q] = bn[q];
          bn[q] = *(const f32x4*)(wrow[j][q] + kn);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int q = 0; q < 3; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q][e], bv[q][e], acc[q], 0, 0, 0);
      }
      dhr[j] = ((acc[0] + acc[1]) + acc[2]) + dhz[j];
    }
    // (no barrier here: the next step writes the other LDS buffer, and its barrier orders this step's reads before the
    // step after it writes this buffer again)
  }

#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    if (!on[j]) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (live[i]) a.dh_out[(int64_t)uc[i] * H + jt[j] * 16 + r] = dhr[j][i];
  }
}

// workspace of a backward call: W_hh^T [H][3H], the dh hand-over buffer, one chunk of the [.., 4H] panel
struct GruBwdWs {
  int64_t wt, dh, da, total;    // byte offsets
};
inline GruBwdWs gru_bwd_ws(int n_users, int T, int H) {
  GruBwdWs w;
  const int64_t state = ((int64_t)n_users * H * 4 + 15) & ~(int64_t)15;
  w.wt = 0;
  w.dh = (int64_t)H * 3 * H * 4;
  w.da = w.dh + state;
  w.total = w.da + (int64_t)user_tiles(n_users) * MT * chunk_steps(T) * 4 * H * 4;
  return w;
}

int gru_encode_impl(const char* what, bool train, const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                    int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_ih,
                    const float* w_hh, const float* b_ih, const float* b_hh, const float* h0, float* h_out, float* h_T, int variant,
                    void* workspace, void* saved, void* stream) {
  RECNN_REQUIRE(store_ok(items, ratings, user_off, slots, table) && w_ih && w_hh && b_ih && b_hh && h_out && h_T && (saved || !train),
                "%s: null pointer", what);
  RECNN_REQUIRE(emb_dim >= 8 && emb_dim % 8 == 0 && emb_dim <= 128, "%s: emb_dim must be a multiple of 8 up to 128 (got %d)", what, emb_dim);
  RECNN_REQUIRE(hidden >= 16 && hidden % 16 == 0 && hidden <= 256, "%s: hidden must be a multiple of 16 up to 256 (got %d)", what, hidden);
  RECNN_REQUIRE(n_users >= 0 && t0 >= 0 && T >= 0 && n_items > 0, "%s: need n_users, t0, T >= 0 and n_items > 0", what);
  RECNN_REQUIRE(variant == 0 || variant == 1, "%s: variant must be 0 (fused input projection) or 1 (chunked), got %d", what, variant);
  RECNN_REQUIRE(variant == 0 || workspace, "%s: variant 1 needs the workspace of recnn_gru_workspace_bytes", what);
  RECNN_REQUIRE(aligned16(table, w_hh, workspace, saved), "%s: table, w_hh, workspace and saved must be 16-byte aligned", what);
  if (n_users == 0) return 0;
  EncArgs a{};
  a.s = SeqStore{items, ratings, user_off, slots, n_users, table, n_items, emb_dim};
  a.H = hidden;
  a.w_ih = w_ih; a.w_hh = w_hh; a.b_ih = b_ih; a.b_hh = b_hh;
  a.h_out = h_out; a.h_T = h_T;
  a.pre = (float*)workspace;
  a.saved = (float*)saved;
  if (train) launch_gru_encode<true>(a, t0, T, h0, variant, (hipStream_t)stream);
  else launch_gru_encode<false>(a, t0, T, h0, variant, (hipStream_t)stream);
  return recnn_check_hip(hipGetLastError(), what);
}

// recnn_gru_backward (d_table == NULL: w_ih and table_workspace are not looked at) and recnn_gru_backward_table
int gru_backward_impl(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users, int t0,
                      int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_ih, const float* w_hh,
                      const void* saved, const float* h_out, const float* h0, const float* g_h, const float* g_hT, float* d_w_ih,
                      float* d_w_hh, float* d_b_ih, float* d_b_hh, float* d_h0, float* d_table, void* workspace, void* table_workspace,
                      void* stream) {
  RECNN_REQUIRE(store_ok(items, ratings, user_off, slots, table) && w_hh && saved && h_out && workspace, "gru_backward: null pointer");
  RECNN_LSTM_DIMS_OK("gru_backward", emb_dim, hidden);
  RECNN_REQUIRE(n_users >= 0 && t0 >= 0 && T >= 1 && n_items > 0, "gru_backward: need n_users, t0 >= 0, T >= 1 and n_items > 0");
  RECNN_REQUIRE(aligned16(table, w_hh, saved, h_out, h0, workspace),
                "gru_backward: table, w_hh, saved, h_out, h0 and workspace must be 16-byte aligned");
  if (d_table) {
    RECNN_REQUIRE(w_ih && table_workspace, "gru_backward_table: null pointer (w_ih, table_workspace)");
    RECNN_REQUIRE(aligned16(d_table, table_workspace), "gru_backward_table: d_table and table_workspace must be 16-byte aligned");
    RECNN_REQUIRE((int64_t)n_users * T < (1LL << 31), "gru_backward_table: n_users * T must stay below 2^31");
  }
  const hipStream_t s = (hipStream_t)stream;
  if (n_users == 0) {
    if (d_table) RECNN_HIP(hipMemsetAsync(d_table, 0, (size_t)n_items * emb_dim * sizeof(float), s));
    return 0;
  }
  const int H = hidden, G = 3 * H, P = 4 * H;
  const GruBwdWs w = gru_bwd_ws(n_users, T, H);
  char* ws = (char*)workspace;
  float* wt = (float*)(ws + w.wt);
  float* dh = (float*)(ws + w.dh);
  const bool want_w = d_w_ih || d_w_hh || d_b_ih || d_b_hh;
  const size_t lds = gru_bwd_lds(H);
  const bool two = H > 16 * NWV;
  if (lds > 48 * 1024)
    RECNN_HIP(hipFuncSetAttribute(two ? (const void*)gru_bwd_chain_kernel<2> : (const void*)gru_bwd_chain_kernel<1>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(gru_whh_transpose_kernel, dim3(grid_for((int64_t)H * G, 256, 2048)), dim3(256), 0, s, w_hh, H, wt);

  GruBwdArgs a{};
  a.U = n_users; a.T = T; a.H = H;
  a.saved = (const float*)saved;
  a.w_hhT = wt;
  a.h_out = h_out; a.h0 = h0; a.g_h = g_h; a.g_hT = g_hT;
  a.da = want_w || d_table ? (float*)(ws + w.da) : nullptr;
  a.da_T = chunk_steps(T);
  DwArgs d{};
  d.s = SeqStore{items, ratings, user_off, slots, n_users, table, n_items, emb_dim};
  d.t0 = t0;
  d.U = n_users; d.T = T; d.H = H; d.da_T = a.da_T;
  d.G = G; d.lda = P;
  d.da = a.da;
  TableGrad tg{};
  if (d_table) RECNN_HIP(table_grad_prepare(tg, d.s, t0, T, G, P, a.da_T, a.da, w_ih, table_workspace, s));
  const int nchunks = (T + LSTM_CHUNK - 1) / LSTM_CHUNK;
  const int mtiles = (G + DW_T - 1) / DW_T;
  for (int ci = nchunks - 1; ci >= 0; --ci) {
    a.tb = ci * LSTM_CHUNK;
    a.Tc = T - a.tb < LSTM_CHUNK ? T - a.tb : LSTM_CHUNK;
    a.dh_in = ci == nchunks - 1 ? nullptr : dh;
    a.dh_out = ci == 0 && d_h0 ? d_h0 : dh;
    const dim3 grid(user_tiles(n_users));
    if (two) hipLaunchKernelGGL((gru_bwd_chain_kernel<2>), grid, dim3(NT), lds, s, a);
    else hipLaunchKernelGGL((gru_bwd_chain_kernel<1>), grid, dim3(NT), lds, s, a);
    if (d_table) table_grad_chunk(tg, a.tb, a.Tc, s);
    if (!want_w) continue;
    d.tb = a.tb; d.Tc = a.Tc;
    d.accumulate = ci != nchunks - 1;
    if (d_w_hh || d_b_hh) {             // rows [da_r | da_z | da_hn]: the last third sits one block further in the panel
      DwArgs x = d;
      x.msplit = 2 * H; x.mshift = H;
      x.h_out = h_out; x.h0 = h0;
      x.out = d_w_hh; x.ldo = H; x.N = H;
      x.d_b = d_b_hh;
      hipLaunchKernelGGL((seq_dw_kernel<false, true>), dim3(mtiles, d_w_hh ? (H + DW_T - 1) / DW_T : 1), dim3(256), 0, s, x);
    }
    if (d_w_ih || d_b_ih) {             // rows [da_r | da_z | da_n]
      DwArgs x = d;
      x.msplit = G; x.mshift = 0;
      x.out = d_w_ih; x.ldo = emb_dim + 1; x.N = emb_dim;
      x.d_wr = d_w_ih ? d_w_ih + emb_dim : nullptr;
      x.d_b = d_b_ih;
      hipLaunchKernelGGL((seq_dw_kernel<true, true>), dim3(mtiles, d_w_ih ? (emb_dim + DW_T - 1) / DW_T : 1), dim3(256), 0, s, x);
    }
  }
  if (d_table) table_grad_finish(tg, d_table, s);
  return recnn_check_hip(hipGetLastError(), d_table ? "gru_backward_table" : "gru_backward");
}

}  // namespace

extern "C" int recnn_gru_workspace_bytes(int n_users, int T, int hidden, int variant, int64_t* bytes) {
  RECNN_REQUIRE(bytes, "gru_workspace_bytes: null pointer");
  RECNN_REQUIRE(n_users >= 0 && T >= 0 && hidden > 0 && hidden % 16 == 0 && hidden <= 256 && (variant == 0 || variant == 1),
                "gru_workspace_bytes: need n_users >= 0, T >= 0, hidden a multiple of 16 up to 256, variant 0 or 1");
  *bytes = variant == 1 ? gru_pre_bytes(n_users, T, hidden) : 0;
  return 0;
}

extern "C" int recnn_gru_encode(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                                int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_ih,
                                const float* w_hh, const float* b_ih, const float* b_hh, const float* h0, float* h_out, float* h_T,
                                int variant, void* workspace, void* stream) {
  return gru_encode_impl("gru_encode", false, items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, w_ih, w_hh,
                         b_ih, b_hh, h0, h_out, h_T, variant, workspace, nullptr, stream);
}

extern "C" int recnn_gru_train_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int variant, int64_t* saved_bytes,
                                               int64_t* bwd_bytes) {
  RECNN_REQUIRE(saved_bytes && bwd_bytes, "gru_train_workspace_bytes: null pointer");
  RECNN_LSTM_DIMS_OK("gru_train_workspace_bytes", emb_dim, hidden);
  RECNN_REQUIRE(n_users >= 0 && T >= 0 && (variant == 0 || variant == 1),
                "gru_train_workspace_bytes: need n_users >= 0, T >= 0, variant 0 or 1");
  *saved_bytes = gru_saved_bytes(n_users, T, hidden);
  *bwd_bytes = gru_bwd_ws(n_users, T, hidden).total;
  return 0;
}

extern "C" int recnn_gru_encode_train(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                                      int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden,
                                      const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* h0,
                                      float* h_out, float* h_T, int variant, void* workspace, void* saved, void* stream) {
  return gru_encode_impl("gru_encode_train", true, items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, w_ih,
                         w_hh, b_ih, b_hh, h0, h_out, h_T, variant, workspace, saved, stream);
}

extern "C" int recnn_gru_table_grad_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int n_items, int64_t* bytes) {
  RECNN_REQUIRE(bytes, "gru_table_grad_workspace_bytes: null pointer");
  RECNN_LSTM_DIMS_OK("gru_table_grad_workspace_bytes", emb_dim, hidden);
  RECNN_REQUIRE(n_users >= 0 && T >= 0 && n_items >= 1 && (int64_t)n_users * T < (1LL << 31),
                "gru_table_grad_workspace_bytes: need n_users >= 0, T >= 0, n_items >= 1 and n_users * T < 2^31");
  *bytes = table_ws(n_users, T, 3 * hidden, emb_dim, n_items).total;
  return 0;
}

extern "C" int recnn_gru_backward(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                                  int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_hh,
                                  const void* saved, const float* h_out, const float* h0, const float* g_h, const float* g_hT,
                                  float* d_w_ih, float* d_w_hh, float* d_b_ih, float* d_b_hh, float* d_h0, void* workspace,
                                  void* stream) {
  return gru_backward_impl(items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, nullptr, w_hh, saved, h_out,
                           h0, g_h, g_hT, d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_h0, nullptr, workspace, nullptr, stream);
}

extern "C" int recnn_gru_backward_table(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                                        int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden,
                                        const float* w_ih, const float* w_hh, const void* saved, const float* h_out, const float* h0,
                                        const float* g_h, const float* g_hT, float* d_w_ih, float* d_w_hh, float* d_b_ih, float* d_b_hh,
                                        float* d_h0, float* d_table, void* workspace, void* table_workspace, void* stream) {
  RECNN_REQUIRE(d_table, "gru_backward_table: null pointer (d_table; recnn_gru_backward is the call without it)");
  return gru_backward_impl(items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, w_ih, w_hh, saved, h_out, h0,
                           g_h, g_hT, d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_h0, d_table, workspace, table_workspace, stream);
}
