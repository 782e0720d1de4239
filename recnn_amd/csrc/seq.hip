// seq.hip -- dynamic-length user batches (reference: recnn/data/utils.py padder / prepare_batch_dynamic_size and the SeqEnv design
// of recnn/data/env.py) on gfx950: padded gathers, and the replay-buffer collect with its backward.
//
//   padded gather   [U, Lmax] ids / ratings and [U, Lmax, E] embedding rows from the CSR replay store (or from an already padded id
//                   tensor): a flat walk over 16-byte chunks, a pure copy.  A padded position holds id 0, so it gets table row 0.
//   state encoders  an LSTM (lstm.hip) or a GRU (gru.hip) over whole user histories: the chains of seq_chain.h / seq_bwd.h.
//   collect         rows of the replay buffer for the kept steps of one user batch: state = h_{t-1}, action = emb(item_t),
//                   reward = rating_t, next_state = h_t, one launch.
//   collect backward g_h[u, t] = g_next_state[k U + u] where steps[k] == t, plus g_state[k' U + u] where steps[k'] == t + 1: a
//                   gather over 16-byte chunks of g_h (flat_walk.h), each chunk summing its two or fewer sources.
// No atomics, fixed orders: equal calls give equal bits.
// gather_dev.h is not used here: its body is the sliding-window gather (rows of one user share F of F + 1 lines, packed / bf16 /
// split destinations, a row plan); a padded batch has no shared lines and one fp32 destination, which is a flat walk over chunks.
#include "seq_chain.h"

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

// ------------------------------------------------------------------------------------------------ collect backward
__global__ __launch_bounds__(256) void seq_collect_bwd_kernel(const float* __restrict__ g_state, const float* __restrict__ g_next,
                                                              int U, int T, int H, const int32_t* __restrict__ steps, int n_steps,
                                                              float* __restrict__ g_h) {
  const int H4 = H >> 2;
  flat_walk<1>((int64_t)U * T * H4, [&](int64_t i, Width<1>) {
    const int64_t cell = i / H4;
    const int c = (int)(i - cell * H4);
    const int u = (int)(cell / T), t = (int)(cell - (int64_t)u * T);
    int lo = 0, hi = n_steps;                            // first k with steps[k] >= t (steps is strictly increasing)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (steps[mid] < t) lo = mid + 1;
      else hi = mid;
    }
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    int k = lo;
    if (k < n_steps && steps[k] == t) {
      if (g_next) v = *(const float4*)(g_next + ((int64_t)k * U + u) * H + 4 * c);
      ++k;
    }
    if (k < n_steps && steps[k] == t + 1 && g_state) {
      const float4 w = *(const float4*)(g_state + ((int64_t)k * U + u) * H + 4 * c);
      v = make_float4(v.x + w.x, v.y + w.y, v.z + w.z, v.w + w.w);
    }
    *(float4*)(g_h + cell * H + 4 * c) = v;
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

extern "C" int recnn_seq_collect_bwd(const float* g_state, const float* g_next_state, int n_users, int T, int hidden,
                                     const int32_t* steps, int n_steps, float* g_h, void* stream) {
  RECNN_REQUIRE(g_h && (steps || n_steps == 0), "seq_collect_bwd: null pointer");
  RECNN_REQUIRE(n_users >= 0 && T >= 0 && n_steps >= 0, "seq_collect_bwd: negative size");
  RECNN_REQUIRE(hidden > 0 && hidden % 4 == 0, "seq_collect_bwd: hidden must be a positive multiple of 4 (got %d)", hidden);
  RECNN_REQUIRE(aligned16(g_state, g_next_state, g_h), "seq_collect_bwd: 16-byte alignment");
  const int64_t chunks = (int64_t)n_users * T * (hidden / 4);
  if (chunks == 0) return 0;
  hipLaunchKernelGGL(seq_collect_bwd_kernel, dim3(grid_for(chunks, 256, 2048)), dim3(256), 0, (hipStream_t)stream, g_state,
                     g_next_state, n_users, T, hidden, steps, n_steps, g_h);
  return recnn_check_hip(hipGetLastError(), "seq_collect_bwd");
}
