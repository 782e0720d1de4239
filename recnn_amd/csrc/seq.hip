// seq.hip -- dynamic-length user batches (reference: recnn/data/utils.py padder / prepare_batch_dynamic_size and the SeqEnv design
// of recnn/data/env.py) on gfx950: padded gathers, an LSTM state encoder over whole user histories, and the replay-buffer collect.
//
//   padded gather   [U, Lmax] ids / ratings and [U, Lmax, E] embedding rows from the CSR replay store (or from an already padded id
//                   tensor): a flat walk over 16-byte chunks, a pure copy.  A padded position holds id 0, so it gets table row 0.
//   LSTM encode     h_t, c_t = LSTM([emb(item_t) | rating_t], h_{t-1}, c_{t-1}) for t = t0 .. t0 + T - 1, torch.nn.LSTM(E + 1, H) weights
//                   read in place (gate order i, f, g, o).  One workgroup owns 16 users -- one M tile of v_mfma_f32_16x16x4_f32 --
//                   for all steps of a launch: the chain of a sequence never leaves its workgroup, no workgroup waits on another
//                   (variant 1 cuts T into a stream-ordered chain of launches, the state passing through h_T / c_T).  Eight waves;
//                   wave w owns the hidden units of tiles w and w + 8, and for each the four gate tiles, so a lane holds i, f, g, o
//                   of the same (user, hidden unit) and the cell update is lane-local; c lives in registers, h_{t-1} and x_t in LDS
//                   (double-buffered: one barrier per step).  A pre-activation is one FIXED-ORDER chain:
//                     fma(rating, w_ih[:, E], b_ih + b_hh), then the x products, then the h_{t-1} products, 16 columns per block,
//                     MFMA e of a block taking columns k0 + e, k0 + 4 + e, k0 + 8 + e, k0 + 12 + e (how the instruction sums its
//                     four products is the hardware's business, and the same every time)
//                   -- the same order for every row, user and launch, so a user's bits do not depend on its row in the tile, on
//                   the other users, or on how T is cut into calls.
//                   The rating column (K = E + 1 = 129) is the rank-1 first link of that chain, on the VALU: no padded GEMM.
//                   Item rows are gathered through the store one step ahead of their use; [U, T, E] is never materialised.
//     variant 0     the input projection is fused into the step.
//     variant 1     the first E + 1 links of every chain are computed by a grid-wide launch per chunk of LSTM_CHUNK steps into a
//                   workspace in accumulator layout (a few MB: L2 / Infinity Cache resident), and the chain launch of that chunk
//                   starts from them.  The same chains: bit-identical to variant 0.  W_hh is streamed from L2 every step in
//                   both (how W_hh is best held is still open).
//   collect         rows of the replay buffer for the kept steps of one user batch: state = h_{t-1}, action = emb(item_t),
//                   reward = rating_t, next_state = h_t, one launch.
// No atomics, fixed orders: equal calls give equal bits.
// gather_dev.h is not used here: its body is the sliding-window gather (rows of one user share F of F + 1 lines, packed / bf16 /
// split destinations, a row plan); a padded batch has no shared lines and one fp32 destination, which is a flat walk over chunks.
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

// ------------------------------------------------------------------------------------------------ padded gathers
__global__ __launch_bounds__(256) void seq_gather_kernel(const SeqStore s, int l_max, int64_t* __restrict__ out_items,
                                                         float* __restrict__ out_ratings, float* __restrict__ out_emb) {
  const int E4 = s.E >> 2;
  const int64_t cells = (int64_t)s.n_users * l_max;
  flat_walk<1>(cells * E4, [&](int64_t i, Width<1>) {
    const int64_t cell = i / E4;
    const int c = (int)(i - cell * E4);
    const int u = (int)(cell / l_max), p = (int)(cell - (int64_t)u * l_max);
    const int slot = s.slots[u];
    const int64_t o = s.user_off[slot];
    const bool in = p < (int)(s.user_off[slot + 1] - o);
    const int64_t id = in ? s.items[o + p] : 0;
    if (c == 0) {
      out_items[cell] = id;
      out_ratings[cell] = in ? s.ratings[o + p] : 0.f;
    }
    if (out_emb) *(float4*)(out_emb + cell * s.E + 4 * c) = table_chunk(s, id, c);
  });
}

__global__ __launch_bounds__(256) void seq_gather_idx_kernel(const int64_t* __restrict__ idx, int64_t n, const SeqStore s,
                                                             float* __restrict__ out_emb) {
  const int E4 = s.E >> 2;
  flat_walk<1>(n * E4, [&](int64_t i, Width<1>) {
    const int64_t cell = i / E4;
    const int c = (int)(i - cell * E4);
    *(float4*)(out_emb + cell * s.E + 4 * c) = table_chunk(s, idx[cell], c);
  });
}

// ------------------------------------------------------------------------------------------------ collect
__global__ __launch_bounds__(256) void seq_collect_kernel(const float* __restrict__ h, int T, int H, const int32_t* __restrict__ steps,
                                                          int n_steps, const SeqStore s, float* __restrict__ state,
                                                          float* __restrict__ action, float* __restrict__ reward,
                                                          float* __restrict__ next_state) {
  const int H4 = H >> 2, E4 = s.E >> 2, per = 2 * H4 + E4;
  flat_walk<1>((int64_t)n_steps * s.n_users * per, [&](int64_t i, Width<1>) {
    const int64_t row = i / per;                       // row = k * U + u: U rows per kept step, as ReplayBuffer.append lays them
    const int c = (int)(i - row * per);
    const int k = (int)(row / s.n_users), u = (int)(row - (int64_t)k * s.n_users);
    const int t = steps[k];
    if (t < 1 || t >= T) return;                       // (refused on the host; never read outside h)
    const float* hu = h + ((int64_t)u * T + t) * H;
    if (c < H4) {
      *(float4*)(state + row * H + 4 * c) = *(const float4*)(hu - H + 4 * c);
    } else if (c < 2 * H4) {
      *(float4*)(next_state + row * H + 4 * (c - H4)) = *(const float4*)(hu + 4 * (c - H4));
    } else {
      const int slot = s.slots[u];
      const int64_t o = s.user_off[slot];
      const int len = (int)(s.user_off[slot + 1] - o);
      const int ce = c - 2 * H4;
      const bool in = t < len;
      *(float4*)(action + row * s.E + 4 * ce) = in ? table_chunk(s, s.items[o + t], ce) : nan4();
      if (ce == 0) reward[row] = in ? s.ratings[o + t] : __builtin_nanf("");
    }
  });
}

// ------------------------------------------------------------------------------------------------ LSTM encode
struct EncArgs {
  SeqStore s;
  int t0, T, T_out, t_out0, H;     // this launch runs steps t0 .. t0 + T - 1 and writes h_out[:, t_out0 .. t_out0 + T - 1] of [U, T_out, H]
  const float *w_ih, *w_hh, *b_ih, *b_hh, *h0, *c0;
  float *h_out, *h_T, *c_T;
  float* pre;                      // variant 1: [user tile][T][H / 16][4 gates][64 lanes] f32x4
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
template <int TPW>
__device__ __forceinline__ void input_links(const EncArgs& a, const float* xs, const float* rs, int ldx, const int (&jt)[TPW],
                                            const bool (&on)[TPW], f32x4 (&acc)[TPW][4], int lane) {
  const int r = lane & 15, g = lane >> 4, E = a.s.E, H = a.H, K1 = E + 1;
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    if (!on[j]) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = q * H + jt[j] * 16 + r;
      const float b = a.b_ih[row] + a.b_hh[row], wr = a.w_ih[(int64_t)row * K1 + E];
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
      f32x4 bv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = q * H + jt[j] * 16 + r;
        bv[q] = kin ? (f32x4)(*(const f32x4u*)(a.w_ih + (int64_t)row * K1 + k0 + 4 * g)) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[j][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[q][e], acc[j][q], 0, 0, 0);
    }
  }
}

__device__ __forceinline__ int64_t pre_index(int tile, int T, int t, int ntiles, int jt, int q, int lane) {
  return ((((int64_t)tile * T + t) * ntiles + jt) * 4 + q) * 64 + lane;
}

template <int TPW, bool PRE>
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
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float ig = sigmoidf_(acc[j][0][i]), fg = sigmoidf_(acc[j][1][i]), gg = tanhf(acc[j][2][i]), og = sigmoidf_(acc[j][3][i]);
        c[j][i] = fg * c[j][i] + ig * gg;
        const float hv = og * tanhf(c[j][i]);
        hl[j][i] = hv;
        hn[(4 * g + i) * ldh + hid] = hv;
        const int u = u0 + 4 * g + i;
        if (u < U) a.h_out[((int64_t)u * a.T_out + a.t_out0 + t) * H + hid] = hv;
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

bool store_ok(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, const float* table) {
  return items && ratings && user_off && slots && table;
}

}  // namespace

extern "C" int recnn_seq_gather(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                                int l_max, const float* table, int n_items, int emb_dim, int64_t* out_items, float* out_ratings,
                                float* out_emb, void* stream) {
  RECNN_REQUIRE(store_ok(items, ratings, user_off, slots, table) && out_items && out_ratings, "seq_gather: null pointer");
  RECNN_REQUIRE(n_users >= 0 && l_max >= 0 && n_items > 0, "seq_gather: need n_users >= 0, l_max >= 0, n_items > 0");
  RECNN_REQUIRE(emb_dim > 0 && emb_dim % 4 == 0, "seq_gather: emb_dim must be a positive multiple of 4 (got %d)", emb_dim);
  RECNN_REQUIRE(aligned16(table, out_emb), "seq_gather: table and out_emb must be 16-byte aligned");
  const int64_t chunks = (int64_t)n_users * l_max * (emb_dim / 4);
  if (chunks == 0) return 0;
  const SeqStore s{items, ratings, user_off, slots, n_users, table, n_items, emb_dim};
  hipLaunchKernelGGL(seq_gather_kernel, dim3(grid_for(chunks, 256, 2048)), dim3(256), 0, (hipStream_t)stream, s, l_max, out_items,
                     out_ratings, out_emb);
  return recnn_check_hip(hipGetLastError(), "seq_gather");
}

extern "C" int recnn_seq_gather_idx(const int64_t* idx, int64_t n, const float* table, int n_items, int emb_dim, float* out_emb,
                                    void* stream) {
  RECNN_REQUIRE(idx && table && out_emb, "seq_gather_idx: null pointer");
  RECNN_REQUIRE(n >= 0 && n_items > 0, "seq_gather_idx: need n >= 0 and n_items > 0");
  RECNN_REQUIRE(emb_dim > 0 && emb_dim % 4 == 0, "seq_gather_idx: emb_dim must be a positive multiple of 4 (got %d)", emb_dim);
  RECNN_REQUIRE(aligned16(table, out_emb), "seq_gather_idx: table and out_emb must be 16-byte aligned");
  if (n == 0) return 0;
  const SeqStore s{nullptr, nullptr, nullptr, nullptr, 0, table, n_items, emb_dim};
  hipLaunchKernelGGL(seq_gather_idx_kernel, dim3(grid_for(n * (emb_dim / 4), 256, 2048)), dim3(256), 0, (hipStream_t)stream, idx, n, s,
                     out_emb);
  return recnn_check_hip(hipGetLastError(), "seq_gather_idx");
}

extern "C" int recnn_seq_collect(const float* h, int n_users, int T, int hidden, const int32_t* steps, int n_steps, const int32_t* items,
                                 const float* ratings, const int64_t* user_off, const int32_t* slots, const float* table, int n_items,
                                 int emb_dim, float* state, float* action, float* reward, float* next_state, void* stream) {
  RECNN_REQUIRE(h && steps && store_ok(items, ratings, user_off, slots, table) && state && action && reward && next_state,
                "seq_collect: null pointer");
  RECNN_REQUIRE(n_users >= 0 && T >= 0 && n_steps >= 0 && n_items > 0, "seq_collect: negative size");
  RECNN_REQUIRE(hidden > 0 && hidden % 4 == 0 && emb_dim > 0 && emb_dim % 4 == 0,
                "seq_collect: hidden and emb_dim must be positive multiples of 4 (got %d, %d)", hidden, emb_dim);
  RECNN_REQUIRE(aligned16(h, table, state, action, next_state), "seq_collect: 16-byte alignment");
  const int64_t chunks = (int64_t)n_steps * n_users * (2 * (hidden / 4) + emb_dim / 4);
  if (chunks == 0) return 0;
  const SeqStore s{items, ratings, user_off, slots, n_users, table, n_items, emb_dim};
  hipLaunchKernelGGL(seq_collect_kernel, dim3(grid_for(chunks, 256, 2048)), dim3(256), 0, (hipStream_t)stream, h, T, hidden, steps,
                     n_steps, s, state, action, reward, next_state);
  return recnn_check_hip(hipGetLastError(), "seq_collect");
}

extern "C" int recnn_lstm_workspace_bytes(int n_users, int T, int hidden, int variant, int64_t* h_bytes) {
  RECNN_REQUIRE(h_bytes, "lstm_workspace_bytes: null pointer");
  RECNN_REQUIRE(n_users >= 0 && T >= 0 && hidden > 0 && hidden % 16 == 0 && hidden <= 256 && (variant == 0 || variant == 1),
                "lstm_workspace_bytes: need n_users >= 0, T >= 0, hidden a multiple of 16 up to 256, variant 0 or 1");
  *h_bytes = variant == 1 ? pre_bytes(n_users, T, hidden) : 0;
  return 0;
}

extern "C" int recnn_lstm_encode(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                                 int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_ih,
                                 const float* w_hh, const float* b_ih, const float* b_hh, const float* h0, const float* c0, float* h_out,
                                 float* h_T, float* c_T, int variant, void* workspace, void* stream) {
  RECNN_REQUIRE(store_ok(items, ratings, user_off, slots, table) && w_ih && w_hh && b_ih && b_hh && h_out && h_T && c_T,
                "lstm_encode: null pointer");
  RECNN_REQUIRE((h0 == nullptr) == (c0 == nullptr), "lstm_encode: h0 and c0 come together");
  RECNN_REQUIRE(emb_dim >= 8 && emb_dim % 8 == 0 && emb_dim <= 128, "lstm_encode: emb_dim must be a multiple of 8 up to 128 (got %d)",
                emb_dim);
  RECNN_REQUIRE(hidden >= 16 && hidden % 16 == 0 && hidden <= 256, "lstm_encode: hidden must be a multiple of 16 up to 256 (got %d)",
                hidden);
  RECNN_REQUIRE(n_users >= 0 && t0 >= 0 && T >= 0 && n_items > 0, "lstm_encode: need n_users, t0, T >= 0 and n_items > 0");
  RECNN_REQUIRE(variant == 0 || variant == 1, "lstm_encode: variant must be 0 (fused input projection) or 1 (chunked), got %d", variant);
  RECNN_REQUIRE(variant == 0 || workspace, "lstm_encode: variant 1 needs the workspace of recnn_lstm_workspace_bytes");
  RECNN_REQUIRE(aligned16(table, w_hh, workspace), "lstm_encode: table, w_hh and workspace must be 16-byte aligned");
  if (n_users == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  EncArgs a{};
  a.s = SeqStore{items, ratings, user_off, slots, n_users, table, n_items, emb_dim};
  a.H = hidden;
  a.w_ih = w_ih; a.w_hh = w_hh; a.b_ih = b_ih; a.b_hh = b_hh;
  a.h_out = h_out; a.h_T = h_T; a.c_T = c_T;
  a.T_out = T;
  a.pre = (float*)workspace;
  const dim3 grid(user_tiles(n_users));
  const bool two = hidden > 16 * NWV;
  const size_t lds = encode_lds(emb_dim, hidden);
  if (variant == 0 || T == 0) {
    a.t0 = t0; a.T = T; a.t_out0 = 0; a.h0 = h0; a.c0 = c0;
    if (two) hipLaunchKernelGGL((lstm_encode_kernel<2, false>), grid, dim3(NT), lds, s, a);
    else hipLaunchKernelGGL((lstm_encode_kernel<1, false>), grid, dim3(NT), lds, s, a);
    return recnn_check_hip(hipGetLastError(), "lstm_encode");
  }
  // variant 1: per chunk one grid-wide projection launch and one chain launch; the chain's state passes through h_T / c_T (stream order)
  for (int done = 0; done < T; done += LSTM_CHUNK) {
    a.t0 = t0 + done;
    a.T = T - done < LSTM_CHUNK ? T - done : LSTM_CHUNK;
    a.t_out0 = done;
    a.h0 = done ? h_T : h0;
    a.c0 = done ? c_T : c0;
    const dim3 pgrid(grid.x, a.T);
    if (two) {
      hipLaunchKernelGGL((lstm_project_kernel<2>), pgrid, dim3(NT), project_lds(emb_dim), s, a);
      hipLaunchKernelGGL((lstm_encode_kernel<2, true>), grid, dim3(NT), lds, s, a);
    } else {
      hipLaunchKernelGGL((lstm_project_kernel<1>), pgrid, dim3(NT), project_lds(emb_dim), s, a);
      hipLaunchKernelGGL((lstm_encode_kernel<1, true>), grid, dim3(NT), lds, s, a);
    }
  }
  return recnn_check_hip(hipGetLastError(), "lstm_encode");
}
