// seq_lstm.h -- what the inference encode (seq.hip) and the training encode and its backward (seq_bwd.hip) share: the replay-store
// view, the LSTM chain kernel and its launch sequence.  seq.hip describes the chain; SAVE adds the stores the backward reads.
// The GRU encoder (gru.hip) takes the store view, the stager, the input links and the shape checks from here.
#pragma once
#include "flat_walk.h"

namespace {

constexpr int NT = 512;         // 8 waves
constexpr int NWV = 8;
constexpr int MT = 16;          // users per workgroup
constexpr int PAD = 4;          // LDS row padding (floats)
constexpr int LSTM_CHUNK = 32;  // steps per projection launch (variant 1)

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // w_ih rows have stride E + 1: 4-byte aligned only

struct SeqStore {
  const int32_t* items;
  const float* ratings;
  const int64_t* user_off;
  const int32_t* slots;
  int n_users;
  const float* table;
  int n_items, E;
};

__device__ __forceinline__ float4 nan4() {
  const float n = __builtin_nanf("");
  return make_float4(n, n, n, n);
}
// row `id` of the table, 16-byte chunk c; ids outside the table give NaN, never an out-of-bounds read
__device__ __forceinline__ float4 table_chunk(const SeqStore& s, int64_t id, int c) {
  return (uint64_t)id < (uint64_t)s.n_items ? *(const float4*)(s.table + id * s.E + 4 * c) : nan4();
}

// ------------------------------------------------------------------------------------------------ LSTM encode
struct EncArgs {
  SeqStore s;
  int t0, T, T_out, t_out0, H;     // this launch runs steps t0 .. t0 + T - 1 and writes h_out[:, t_out0 .. t_out0 + T - 1] of [U, T_out, H]
  const float *w_ih, *w_hh, *b_ih, *b_hh, *h0, *c0;
  float *h_out, *h_T, *c_T;
  float* pre;                      // variant 1: [user tile][T][H / 16][4 gates][64 lanes] f32x4
  float* saved;                    // SAVE: [user tile][T_out][H / 16][i, f, g, o, c][64 lanes] f32x4, what the backward reads
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// The stager: thread (su = tid >> 5, sc = tid & 31) owns 16-byte chunk sc of user row su of the x panel.  Positions past a history's
// end are clamped to its last element (the host refuses such a T; nothing is read out of bounds).
struct Stager {
  int su, sc;
  int64_t off;
  int len;
  __device__ __forceinline__ Stager(const SeqStore& s, int u0, int tid) {
    su = tid >> 5;
    sc = tid & 31;
    const int slot = s.slots[min(u0 + su, s.n_users - 1)];
    off = s.user_off[slot];
    len = (int)(s.user_off[slot + 1] - off);
  }
  __device__ __forceinline__ int64_t pos(int t) const { return off + max(min(t, len - 1), 0); }
  __device__ __forceinline__ int id(const SeqStore& s, int t) const { return len > 0 ? s.items[pos(t)] : -1; }
  __device__ __forceinline__ float rating(const SeqStore& s, int t) const { return len > 0 ? s.ratings[pos(t)] : __builtin_nanf(""); }
};

// first E + 1 links of the chains of hidden tile jt: acc[q] = fma(rating, w_ih[row, E], b_ih[row] + b_hh[row]) + sum_k x[k] w_ih[row, k]
// with row = q H + 16 jt + r.  xs: LDS [16][ldx] (columns E .. KX - 1 zero), rs: LDS [16].
// NG = 4: the LSTM's gates.  NG = 3: the GRU's r, z and the input half of n (gru.hip), whose chain starts from b_ih alone: b_hh of n
// belongs to the h products, inside the reset product.  acc[.][3] is not touched then.
template <int TPW, int NG = 4>
__device__ __forceinline__ void input_links(const EncArgs& a, const float* xs, const float* rs, int ldx, const int (&jt)[TPW],
                                            const bool (&on)[TPW], f32x4 (&acc)[TPW][4], int lane) {
  const int r = lane & 15, g = lane >> 4, E = a.s.E, H = a.H, K1 = E + 1;
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    if (!on[j]) continue;
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      const int row = q * H + jt[j] * 16 + r;
      const float b = (NG == 3 && q == 2) ? a.b_ih[row] : a.b_ih[row] + a.b_hh[row], wr = a.w_ih[(int64_t)row * K1 + E];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[j][q][i] = fmaf(rs[4 * g + i], wr, b);
    }
  }
  for (int k0 = 0; k0 < E; k0 += 16) {
    const f32x4 av = *(const f32x4*)(xs + r * ldx + k0 + 4 * g);
    const bool kin = k0 + 4 * g < E;        // E is a multiple of 8: the last k block may be half empty (x there is zero)
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      if (!on[j]) continue;
      f32x4 bv[NG];
#pragma unroll
      for (int q = 0; q < NG; ++q) {
        const int row = q * H + jt[j] * 16 + r;
        bv[q] = kin ? (f32x4)(*(const f32x4u*)(a.w_ih + (int64_t)row * K1 + k0 + 4 * g)) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int q = 0; q < NG; ++q) acc[j][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[q][e], acc[j][q], 0, 0, 0);
    }
  }
}

__device__ __forceinline__ int64_t pre_index(int tile, int T, int t, int ntiles, int jt, int q, int lane) {
  return ((((int64_t)tile * T + t) * ntiles + jt) * 4 + q) * 64 + lane;
}
// the training forward's record of step t (of the whole call): q = 0 .. 3 the gate activations i, f, g, o, q = 4 the cell state c_t,
// each in accumulator order (lane (r, g), element i = user 4 g + i of the tile, hidden unit 16 jt + r): the backward's lanes own the
// same (user, hidden unit) pairs and read 16 bytes per lane.
constexpr int SAVED_Q = 5;
__device__ __forceinline__ int64_t saved_index(int tile, int T, int t, int ntiles, int jt, int q, int lane) {
  return ((((int64_t)tile * T + t) * ntiles + jt) * SAVED_Q + q) * 64 + lane;
}

template <int TPW, bool PRE, bool SAVE>
__global__ __launch_bounds__(NT) void lstm_encode_kernel(const EncArgs a) {
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

  // ---- prologue: h_{t0 - 1} into LDS, c_{t0 - 1} into registers, x and rating of the first step, the id of the second
  for (int i = tid; i < MT * H; i += NT) {
    const int uu = i / H, j = i - uu * H;
    hb[uu * ldh + j] = a.h0 ? a.h0[(int64_t)min(u0 + uu, U - 1) * H + j] : 0.f;
  }
  f32x4 c[TPW], hl[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      c[j][i] = (a.c0 && on[j]) ? a.c0[(int64_t)min(u0 + 4 * g + i, U - 1) * H + jt[j] * 16 + r] : 0.f;
      hl[j][i] = 0.f;
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
    float* hn = hb + (cur ^ 1) * MT * ldh;
    // ---- the next step's x row and rating, and the id of the step after it, in flight under this step's products
    float4 xn = make_float4(0.f, 0.f, 0.f, 0.f);
    float rn = 0.f;
    int idn2 = -1;
    const bool more = !PRE && t + 1 < T;
    if (more && xlive) xn = table_chunk(a.s, idn, st.sc);
    if (more && st.sc == 0) rn = st.rating(a.s, a.t0 + t + 1);
    if (!PRE && xlive && t + 2 < T) idn2 = st.id(a.s, a.t0 + t + 2);

    f32x4 acc[TPW][4];
    if constexpr (PRE) {
#pragma unroll
      for (int j = 0; j < TPW; ++j)
        if (on[j])
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[j][q] = ((const f32x4*)a.pre)[pre_index(blockIdx.x, T, t, ntiles, jt[j], q, lane)];
    } else {
      input_links<TPW>(a, xs, rb + cur * MT, ldx, jt, on, acc, lane);
    }
    // ---- the H products of h_{t-1}
    // (W_hh comes from L2 every step: the loads of the next k block are issued ahead of this block's products)
    const float* wrow[TPW][4];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) wrow[j][q] = a.w_hh + (int64_t)(q * H + (on[j] ? jt[j] : 0) * 16 + r) * H + 4 * g;
    f32x4 bn[TPW][4];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) bn[j][q] = *(const f32x4*)(wrow[j][q]);
    for (int k0 = 0; k0 < H; k0 += 16) {
      const f32x4 av = *(const f32x4*)(hs + r * ldh + k0 + 4 * g);
      f32x4 bv[TPW][4];
      const int kn = k0 + 16 < H ? k0 + 16 : k0;
#pragma unroll
      for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          bv[j][q] = bn[j][q];
          bn[j][q] = *(const f32x4*)(wrow[j][q] + kn);
        }
#pragma unroll
      for (int j = 0; j < TPW; ++j) {
        if (!on[j]) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[j][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[j][q][e], acc[j][q], 0, 0, 0);
      }
    }
    // ---- cell update: lane (r, g) holds users 4g .. 4g + 3 of hidden unit 16 jt + r
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      if (!on[j]) continue;
      const int hid = jt[j] * 16 + r;
      [[maybe_unused]] f32x4 sv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float ig = sigmoidf_(acc[j][0][i]), fg = sigmoidf_(acc[j][1][i]), gg = tanhf(acc[j][2][i]), og = sigmoidf_(acc[j][3][i]);
        if constexpr (SAVE) { sv[0][i] = ig; sv[1][i] = fg; sv[2][i] = gg; sv[3][i] = og; }
        c[j][i] = fg * c[j][i] + ig * gg;
        const float hv = og * tanhf(c[j][i]);
        hl[j][i] = hv;
        hn[(4 * g + i) * ldh + hid] = hv;
        const int u = u0 + 4 * g + i;
        if (u < U) a.h_out[((int64_t)u * a.T_out + a.t_out0 + t) * H + hid] = hv;
      }
      if constexpr (SAVE) {
        f32x4* dst = (f32x4*)a.saved + saved_index(blockIdx.x, a.T_out, a.t_out0 + t, ntiles, jt[j], 0, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[64 * q] = sv[q];
        dst[64 * 4] = c[j];
      }
    }
    if (more) {
      if (xlive) *(float4*)(xb + (cur ^ 1) * MT * ldx + st.su * ldx + 4 * st.sc) = xn;
      if (st.sc == 0) rb[(cur ^ 1) * MT + st.su] = rn;
    }
    idn = idn2;
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    if (!on[j]) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = u0 + 4 * g + i;
      if (u >= U) continue;
      const int64_t o = (int64_t)u * H + jt[j] * 16 + r;
      if (T > 0) a.h_T[o] = hl[j][i];
      a.c_T[o] = c[j][i];
    }
  }
}

// variant 1, grid (user tiles, steps of the chunk): the first E + 1 links of step t0 + blockIdx.y for 16 users, into a.pre
template <int TPW>
__global__ __launch_bounds__(NT) void lstm_project_kernel(const EncArgs a) {
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
  input_links<TPW>(a, xs, rs, ldx, jt, on, acc, lane);
#pragma unroll
  for (int j = 0; j < TPW; ++j)
    if (on[j])
#pragma unroll
      for (int q = 0; q < 4; ++q) ((f32x4*)a.pre)[pre_index(blockIdx.x, a.T, t, ntiles, jt[j], q, lane)] = acc[j][q];
}

inline size_t encode_lds(int E, int H) { return (size_t)(2 * MT * (((E + 15) & ~15) + PAD) + 2 * MT * (H + PAD) + 2 * MT) * sizeof(float); }
inline size_t project_lds(int E) { return (size_t)(MT * (((E + 15) & ~15) + PAD) + MT) * sizeof(float); }
inline int user_tiles(int n_users) { return (n_users + MT - 1) / MT; }
inline int64_t pre_bytes(int n_users, int T, int H) {
  return (int64_t)user_tiles(n_users) * (T < LSTM_CHUNK ? T : LSTM_CHUNK) * (H / 16) * 4 * 64 * (int64_t)sizeof(f32x4);
}
inline int64_t saved_bytes_of(int n_users, int T, int H) {
  return (int64_t)user_tiles(n_users) * T * (H / 16) * SAVED_Q * 64 * (int64_t)sizeof(f32x4);
}

// The launches of one encode call (a.s, a.H, the weights, a.h_out / h_T / c_T, a.pre and a.saved set by the caller).
// variant 1: per chunk one grid-wide projection launch and one chain launch; the chain's state passes through h_T / c_T (stream order)
template <bool SAVE>
inline void launch_encode(EncArgs a, int t0, int T, const float* h0, const float* c0, int variant, hipStream_t s) {
  const int emb_dim = a.s.E, hidden = a.H;
  a.T_out = T;
  const dim3 grid(user_tiles(a.s.n_users));
  const bool two = hidden > 16 * NWV;
  const size_t lds = encode_lds(emb_dim, hidden);
  if (variant == 0 || T == 0) {
    a.t0 = t0; a.T = T; a.t_out0 = 0; a.h0 = h0; a.c0 = c0;
    if (two) hipLaunchKernelGGL((lstm_encode_kernel<2, false, SAVE>), grid, dim3(NT), lds, s, a);
    else hipLaunchKernelGGL((lstm_encode_kernel<1, false, SAVE>), grid, dim3(NT), lds, s, a);
    return;
  }
  for (int done = 0; done < T; done += LSTM_CHUNK) {
    a.t0 = t0 + done;
    a.T = T - done < LSTM_CHUNK ? T - done : LSTM_CHUNK;
    a.t_out0 = done;
    a.h0 = done ? a.h_T : h0;
    a.c0 = done ? a.c_T : c0;
    const dim3 pgrid(grid.x, a.T);
    if (two) {
      hipLaunchKernelGGL((lstm_project_kernel<2>), pgrid, dim3(NT), project_lds(emb_dim), s, a);
      hipLaunchKernelGGL((lstm_encode_kernel<2, true, SAVE>), grid, dim3(NT), lds, s, a);
    } else {
      hipLaunchKernelGGL((lstm_project_kernel<1>), pgrid, dim3(NT), project_lds(emb_dim), s, a);
      hipLaunchKernelGGL((lstm_encode_kernel<1, true, SAVE>), grid, dim3(NT), lds, s, a);
    }
  }
}

// argument checks that recnn_lstm_encode and its training form share
#define RECNN_LSTM_DIMS_OK(what, emb_dim, hidden)                                                                              \
  RECNN_REQUIRE(emb_dim >= 8 && emb_dim % 8 == 0 && emb_dim <= 128, what ": emb_dim must be a multiple of 8 up to 128 (got %d)", \
                emb_dim);                                                                                                      \
  RECNN_REQUIRE(hidden >= 16 && hidden % 16 == 0 && hidden <= 256, what ": hidden must be a multiple of 16 up to 256 (got %d)",  \
                hidden)

inline bool store_ok(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, const float* table) {
  return items && ratings && user_off && slots && table;
}

}  // namespace
