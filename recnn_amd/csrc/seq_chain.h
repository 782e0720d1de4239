// seq_chain.h -- the forward half of the two state encoders of the dynamic-length path (lstm.hip: torch.nn.LSTM, gru.hip:
// torch.nn.GRU): the replay-store view, the stager, the input links, and ONE chain kernel, projection kernel,
// launch sequence and checked host call, each a template over a `Cell`.  seq_bwd.h is the reverse half.
//
//   the chain       h_t = cell([emb(item_t) | rating_t], h_{t-1}, ..) for t = t0 .. t0 + T - 1, torch.nn weights read in place.  One
//                   workgroup owns 16 users -- one M tile of v_mfma_f32_16x16x4_f32 -- for all steps of a launch: the chain of a
//                   sequence never leaves its workgroup, no workgroup waits on another (variant 1 cuts T into a stream-ordered
//                   chain of launches, the state passing through h_T / c_T).  Eight waves; wave w owns the hidden units of tiles w
//                   and w + 8, and for each the cell's gate tiles, so a lane holds every gate of the same (user, hidden unit) and
//                   the cell update is lane-local; the cell's carried state lives in registers, h_{t-1} and x_t in LDS
//                   (double-buffered: one barrier per step).  A pre-activation is one FIXED-ORDER chain:
//                     fma(rating, w_ih[:, E], bias), then the x products, then the h_{t-1} products, 16 columns per block,
//                     MFMA e of a block taking columns k0 + e, k0 + 4 + e, k0 + 8 + e, k0 + 12 + e (how the instruction sums its
//                     four products is the hardware's business, and the same every time), the gates interleaved inside e
//                   -- the same order for every row, user and launch, so a user's bits do not depend on its row in the tile, on
//                   the other users, or on how T is cut into calls.
//                   The rating column (K = E + 1 = 129) is the rank-1 first link of that chain, on the VALU: no padded GEMM.
//                   Item rows are gathered through the store one step ahead of their use; [U, T, E] is never materialised.
//     variant 0     the input projection is fused into the step.
//     variant 1     the first E + 1 links of every chain are computed by a grid-wide launch per chunk of LSTM_CHUNK steps into a
//                   workspace in accumulator layout (a few MB: L2 / Infinity Cache resident), and the chain launch of that chunk
//                   starts from them.  The same chains: bit-identical to variant 0.  W_hh is streamed from L2 every step in
//                   both, the loads of the next k block issued ahead (how W_hh is best held is still open).
//     SAVE          the training forward: the same arithmetic in the same order plus one 16-byte store per lane, saved quantity
//                   and step, in accumulator order (acc_index), which the reverse chain's lanes read back as they wrote them.
//
// What a Cell supplies (plain structs with static inline members; the cell is a compile-time parameter everywhere -- a run-time
// test inside a step loop costs what seq_grad.h records for seq_dw_kernel):
//   NAME, NG (row blocks of W), PRE_Q (accumulators the input links write), SAVED_Q (quantities the training forward records),
//   NSTATE (carried tensors), acc_slot(q) (the accumulator that takes the h products of W_hh's row block q), links_take_bhh(q);
//   State: the registers a lane holds per hidden tile besides h (a plain type), with carried / init (its load from h0 / c0),
//   prepare (what else it needs once), seed (accumulators the input links do not write), update (the new h, and the values to
//   save) and finish (the epilogue store) -- each for ONE element: the loops stay in the kernels, where the compiler schedules them
//   as it did when every cell had kernels of its own;
//   and what seq_bwd.h lists for the backward call.
// No atomics, fixed orders: equal calls give equal bits.
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

// ------------------------------------------------------------------------------------------------ encode
struct EncArgs {
  SeqStore s;
  int t0, T, T_out, t_out0, H;     // this launch runs steps t0 .. t0 + T - 1 and writes h_out[:, t_out0 .. t_out0 + T - 1] of [U, T_out, H]
  const float *w_ih, *w_hh, *b_ih, *b_hh, *h0, *c0;
  float *h_out, *h_T, *c_T;        // (c0 / c_T: cells with NSTATE = 2)
  float* pre;                      // variant 1: [user tile][T][H / 16][PRE_Q][64 lanes] f32x4
  float* saved;                    // SAVE: [user tile][T_out][H / 16][SAVED_Q][64 lanes] f32x4, what the backward reads
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// Position t of user u's history through the store, for the kernels that meet a (user, step) sample at a time: where it lies in
// items / ratings -- past the history's end it is clamped to the last element (the host refuses such a step; nothing is read out of
// bounds) -- and whether the history holds anything at all (an empty one gives NaN rows and is in no list).
struct StorePos {
  int64_t pos;
  int len;
  __device__ __forceinline__ bool live() const { return len > 0; }
};
__device__ __forceinline__ StorePos store_pos(const int32_t* slots, const int64_t* user_off, int u, int t) {
  const int slot = slots[u];
  const int64_t off = user_off[slot];
  const int len = (int)(user_off[slot + 1] - off);
  return StorePos{off + max(min(t, len - 1), 0), len};
}
__device__ __forceinline__ StorePos store_pos(const SeqStore& s, int u, int t) { return store_pos(s.slots, s.user_off, u, t); }

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
// with row = q H + 16 jt + r, for q < Cell::PRE_Q.  xs: LDS [16][ldx] (columns E .. KX - 1 zero), rs: LDS [16].
// A chain the cell says does not take b_hh starts from b_ih alone (the GRU's input half of n: b_hh of n belongs to the h products,
// inside the reset product).  Accumulators PRE_Q .. 3 are not touched.
template <class Cell, int TPW>
__device__ __forceinline__ void input_links(const EncArgs& a, const float* xs, const float* rs, int ldx, const int (&jt)[TPW],
                                            const bool (&on)[TPW], f32x4 (&acc)[TPW][4], int lane) {
  constexpr int NQ = Cell::PRE_Q;
  const int r = lane & 15, g = lane >> 4, E = a.s.E, H = a.H, K1 = E + 1;
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    if (!on[j]) continue;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int row = q * H + jt[j] * 16 + r;
      const float b = Cell::links_take_bhh(q) ? a.b_ih[row] + a.b_hh[row] : a.b_ih[row], wr = a.w_ih[(int64_t)row * K1 + E];
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
      f32x4 bv[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int row = q * H + jt[j] * 16 + r;
        bv[q] = kin ? (f32x4)(*(const f32x4u*)(a.w_ih + (int64_t)row * K1 + k0 + 4 * g)) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[j][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[q][e], acc[j][q], 0, 0, 0);
    }
  }
}

// `pre` and `saved`: [user tile][T][H / 16][nq][64 lanes] f32x4 in accumulator order -- lane (r, g), element i = user 4 g + i of the
// tile, hidden unit 16 jt + r: the backward's lanes own the same (user, hidden unit) pairs and read 16 bytes per lane
__device__ __forceinline__ int64_t acc_index(int tile, int T, int t, int ntiles, int jt, int nq, int q, int lane) {
  return ((((int64_t)tile * T + t) * ntiles + jt) * nq + q) * 64 + lane;
}

template <class Cell, int TPW, bool PRE, bool SAVE>
__global__ __launch_bounds__(NT) void seq_encode_kernel(const EncArgs a) {
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

  // ---- prologue: h_{t0 - 1} into LDS, the cell's carried tensor of the lane's own pairs into registers, x and rating of the first
  // step, the id of the second
  for (int i = tid; i < MT * H; i += NT) {
    const int uu = i / H, j = i - uu * H;
    hb[uu * ldh + j] = a.h0 ? a.h0[(int64_t)min(u0 + uu, U - 1) * H + j] : 0.f;
  }
  typename Cell::State cs[TPW];
  f32x4 hl[TPW];                       // the lane's own h_{t-1}
  const float* s0 = Cell::carried(a);
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      Cell::init(cs[j], hl[j], i, (s0 && on[j]) ? s0[(int64_t)min(u0 + 4 * g + i, U - 1) * H + jt[j] * 16 + r] : 0.f);
    Cell::prepare(cs[j], a, on[j], jt[j] * 16 + r);
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
          for (int q = 0; q < Cell::PRE_Q; ++q)
            acc[j][q] = ((const f32x4*)a.pre)[acc_index(blockIdx.x, T, t, ntiles, jt[j], Cell::PRE_Q, q, lane)];
    } else {
      input_links<Cell, TPW>(a, xs, rb + cur * MT, ldx, jt, on, acc, lane);
    }
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) Cell::seed(cs[j], acc[j], i);
    // ---- the H products of h_{t-1}: W_hh row block q into accumulator acc_slot(q)
    // (W_hh comes from L2 every step: the loads of the next k block are issued ahead of this block's products)
    const float* wrow[TPW][Cell::NG];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
      for (int q = 0; q < Cell::NG; ++q) wrow[j][q] = a.w_hh + (int64_t)(q * H + (on[j] ? jt[j] : 0) * 16 + r) * H + 4 * g;
    f32x4 bn[TPW][Cell::NG];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
      for (int q = 0; q < Cell::NG; ++q) bn[j][q] = *(const f32x4*)(wrow[j][q]);
    for (int k0 = 0; k0 < H; k0 += 16) {
      const f32x4 av = *(const f32x4*)(hs + r * ldh + k0 + 4 * g);
      f32x4 bv[TPW][Cell::NG];
      const int kn = k0 + 16 < H ? k0 + 16 : k0;
#pragma unroll
      for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int q = 0; q < Cell::NG; ++q) {
          bv[j][q] = bn[j][q];
          bn[j][q] = *(const f32x4*)(wrow[j][q] + kn);
        }
#pragma unroll
      for (int j = 0; j < TPW; ++j) {
        if (!on[j]) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int q = 0; q < Cell::NG; ++q)
            acc[j][Cell::acc_slot(q)] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[j][q][e], acc[j][Cell::acc_slot(q)], 0, 0, 0);
      }
    }
    // ---- cell update: lane (r, g) holds users 4g .. 4g + 3 of hidden unit 16 jt + r
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      if (!on[j]) continue;
      const int hid = jt[j] * 16 + r;
      [[maybe_unused]] f32x4 sv[Cell::SAVED_Q];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float hv = Cell::template update<SAVE>(cs[j], acc[j], i, hl[j][i], sv);
        hl[j][i] = hv;
        hn[(4 * g + i) * ldh + hid] = hv;
        const int u = u0 + 4 * g + i;
        if (u < U) a.h_out[((int64_t)u * a.T_out + a.t_out0 + t) * H + hid] = hv;
      }
      if constexpr (SAVE) {
        f32x4* dst = (f32x4*)a.saved + acc_index(blockIdx.x, a.T_out, a.t_out0 + t, ntiles, jt[j], Cell::SAVED_Q, 0, lane);
#pragma unroll
        for (int q = 0; q < Cell::SAVED_Q; ++q) dst[64 * q] = sv[q];
      }
    }
    if (more) {
      if (xlive) *(float4*)(xb + (cur ^ 1) * MT * ldx + st.su * ldx + 4 * st.sc) = xn;
      if (st.sc == 0) rb[(cur ^ 1) * MT + st.su] = rn;
    }
    idn = idn2;
    __syncthreads();
  }

  // ---- epilogue: h_T only when a step ran; what else the cell carries, always
  if (T > 0 || Cell::NSTATE > 1) {
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      if (!on[j]) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int u = u0 + 4 * g + i;
        if (u >= U) continue;
        const int64_t o = (int64_t)u * H + jt[j] * 16 + r;
        if (T > 0) a.h_T[o] = hl[j][i];
        Cell::finish(cs[j], a, o, i);
      }
    }
  }
}

// variant 1, grid (user tiles, steps of the chunk): the first E + 1 links of step t0 + blockIdx.y for 16 users, into a.pre
template <class Cell, int TPW>
__global__ __launch_bounds__(NT) void seq_project_kernel(const EncArgs a) {
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
  input_links<Cell, TPW>(a, xs, rs, ldx, jt, on, acc, lane);
#pragma unroll
  for (int j = 0; j < TPW; ++j)
    if (on[j])
#pragma unroll
      for (int q = 0; q < Cell::PRE_Q; ++q)
        ((f32x4*)a.pre)[acc_index(blockIdx.x, a.T, t, ntiles, jt[j], Cell::PRE_Q, q, lane)] = acc[j][q];
}

// a launch with more than 48 KB of dynamic LDS has to be opted in, kernel by kernel
template <class Kern>
int raise_lds(Kern kern, size_t lds) {
  if (lds > 48 * 1024) RECNN_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}

inline size_t encode_lds(int E, int H) { return (size_t)(2 * MT * (((E + 15) & ~15) + PAD) + 2 * MT * (H + PAD) + 2 * MT) * sizeof(float); }
inline size_t project_lds(int E) { return (size_t)(MT * (((E + 15) & ~15) + PAD) + MT) * sizeof(float); }
inline int user_tiles(int n_users) { return (n_users + MT - 1) / MT; }
inline int chunk_steps(int T) { return T < LSTM_CHUNK ? T : LSTM_CHUNK; }
// bytes of `pre` (steps = chunk_steps(T), nq = PRE_Q) and of `saved` (steps = T, nq = SAVED_Q)
inline int64_t acc_bytes(int n_users, int steps, int H, int nq) {
  return (int64_t)user_tiles(n_users) * steps * (H / 16) * nq * 64 * (int64_t)sizeof(f32x4);
}

// The launches of one encode call (a.s, a.H, the weights, a.h_out / h_T / c_T, a.pre and a.saved set by the caller).
// variant 1: per chunk one grid-wide projection launch and one chain launch; the chain's state passes through h_T / c_T (stream order)
template <class Cell, bool SAVE>
inline void launch_encode(EncArgs a, int t0, int T, const float* h0, const float* c0, int variant, hipStream_t s) {
  const int emb_dim = a.s.E, hidden = a.H;
  a.T_out = T;
  const dim3 grid(user_tiles(a.s.n_users));
  const bool two = hidden > 16 * NWV;
  const size_t lds = encode_lds(emb_dim, hidden);
  if (variant == 0 || T == 0) {
    a.t0 = t0; a.T = T; a.t_out0 = 0; a.h0 = h0; a.c0 = c0;
    if (two) hipLaunchKernelGGL((seq_encode_kernel<Cell, 2, false, SAVE>), grid, dim3(NT), lds, s, a);
    else hipLaunchKernelGGL((seq_encode_kernel<Cell, 1, false, SAVE>), grid, dim3(NT), lds, s, a);
    return;
  }
  for (int done = 0; done < T; done += LSTM_CHUNK) {
    a.t0 = t0 + done;
    a.T = chunk_steps(T - done);
    a.t_out0 = done;
    a.h0 = done ? a.h_T : h0;
    a.c0 = done ? a.c_T : c0;
    const dim3 pgrid(grid.x, a.T);
    if (two) {
      hipLaunchKernelGGL((seq_project_kernel<Cell, 2>), pgrid, dim3(NT), project_lds(emb_dim), s, a);
      hipLaunchKernelGGL((seq_encode_kernel<Cell, 2, true, SAVE>), grid, dim3(NT), lds, s, a);
    } else {
      hipLaunchKernelGGL((seq_project_kernel<Cell, 1>), pgrid, dim3(NT), project_lds(emb_dim), s, a);
      hipLaunchKernelGGL((seq_encode_kernel<Cell, 1, true, SAVE>), grid, dim3(NT), lds, s, a);
    }
  }
}

// argument checks that every entry point of the two encoders shares (the name is from when the LSTM was the only cell); `what`
// is a C string
#define RECNN_LSTM_DIMS_OK(what, emb_dim, hidden)                                                                                   \
  RECNN_REQUIRE(emb_dim >= 8 && emb_dim % 8 == 0 && emb_dim <= 128, "%s: emb_dim must be a multiple of 8 up to 128 (got %d)", what, \
                emb_dim);                                                                                                           \
  RECNN_REQUIRE(hidden >= 16 && hidden % 16 == 0 && hidden <= 256, "%s: hidden must be a multiple of 16 up to 256 (got %d)", what,  \
                hidden)

inline bool store_ok(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, const float* table) {
  return items && ratings && user_off && slots && table;
}

// recnn_<cell>_workspace_bytes
template <class Cell>
int workspace_bytes_impl(const char* what, int n_users, int T, int hidden, int variant, int64_t* bytes) {
  RECNN_REQUIRE(bytes, "%s: null pointer", what);
  RECNN_REQUIRE(n_users >= 0 && T >= 0 && hidden > 0 && hidden % 16 == 0 && hidden <= 256 && (variant == 0 || variant == 1),
                "%s: need n_users >= 0, T >= 0, hidden a multiple of 16 up to 256, variant 0 or 1", what);
  *bytes = variant == 1 ? acc_bytes(n_users, chunk_steps(T), hidden, Cell::PRE_Q) : 0;
  return 0;
}

// recnn_<cell>_encode (train = false: `saved` is not looked at) and recnn_<cell>_encode_train.  c0 / c_T: cells with NSTATE = 2.
template <class Cell>
int encode_impl(const char* what, bool train, const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_ih,
                const float* w_hh, const float* b_ih, const float* b_hh, const float* h0, const float* c0, float* h_out, float* h_T,
                float* c_T, int variant, void* workspace, void* saved, void* stream) {
  constexpr bool two_states = Cell::NSTATE == 2;
  RECNN_REQUIRE(store_ok(items, ratings, user_off, slots, table) && w_ih && w_hh && b_ih && b_hh && h_out && h_T &&
                    (c_T || !two_states) && (saved || !train),
                "%s: null pointer", what);
  RECNN_REQUIRE(!two_states || (h0 == nullptr) == (c0 == nullptr), "%s: h0 and c0 come together", what);
  RECNN_LSTM_DIMS_OK(what, emb_dim, hidden);
  RECNN_REQUIRE(n_users >= 0 && t0 >= 0 && T >= 0 && n_items > 0, "%s: need n_users, t0, T >= 0 and n_items > 0", what);
  RECNN_REQUIRE(variant == 0 || variant == 1, "%s: variant must be 0 (fused input projection) or 1 (chunked), got %d", what, variant);
  RECNN_REQUIRE(variant == 0 || workspace, "%s: variant 1 needs the workspace of recnn_%s_workspace_bytes", what, Cell::NAME);
  // (the LSTM's inference call has always named three pointers here, the other three calls four)
  RECNN_REQUIRE(aligned16(table, w_hh, workspace, saved),
                two_states && !train ? "%s: table, w_hh and workspace must be 16-byte aligned"
                                     : "%s: table, w_hh, workspace and saved must be 16-byte aligned", what);
  if (n_users == 0) return 0;
  EncArgs a{};
  a.s = SeqStore{items, ratings, user_off, slots, n_users, table, n_items, emb_dim};
  a.H = hidden;
  a.w_ih = w_ih; a.w_hh = w_hh; a.b_ih = b_ih; a.b_hh = b_hh;
  a.h_out = h_out; a.h_T = h_T; a.c_T = c_T;
  a.pre = (float*)workspace;
  a.saved = (float*)saved;
  if (train) launch_encode<Cell, true>(a, t0, T, h0, c0, variant, (hipStream_t)stream);
  else launch_encode<Cell, false>(a, t0, T, h0, c0, variant, (hipStream_t)stream);
  return recnn_check_hip(hipGetLastError(), what);
}

}  // namespace
