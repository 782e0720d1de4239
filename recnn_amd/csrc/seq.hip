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
#include "seq_lstm.h"

namespace {

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
  RECNN_LSTM_DIMS_OK("lstm_encode", emb_dim, hidden);
  RECNN_REQUIRE(n_users >= 0 && t0 >= 0 && T >= 0 && n_items > 0, "lstm_encode: need n_users, t0, T >= 0 and n_items > 0");
  RECNN_REQUIRE(variant == 0 || variant == 1, "lstm_encode: variant must be 0 (fused input projection) or 1 (chunked), got %d", variant);
  RECNN_REQUIRE(variant == 0 || workspace, "lstm_encode: variant 1 needs the workspace of recnn_lstm_workspace_bytes");
  RECNN_REQUIRE(aligned16(table, w_hh, workspace), "lstm_encode: table, w_hh and workspace must be 16-byte aligned");
  if (n_users == 0) return 0;
  EncArgs a{};
  a.s = SeqStore{items, ratings, user_off, slots, n_users, table, n_items, emb_dim};
  a.H = hidden;
  a.w_ih = w_ih; a.w_hh = w_hh; a.b_ih = b_ih; a.b_hh = b_hh;
  a.h_out = h_out; a.h_T = h_T; a.c_T = c_T;
  a.pre = (float*)workspace;
  launch_encode<false>(a, t0, T, h0, c0, variant, (hipStream_t)stream);
  return recnn_check_hip(hipGetLastError(), "lstm_encode");
}
