// seq_bwd.hip -- training the LSTM state encoder of seq.hip: the encode that records what its backward needs, backward through
// time, the weight gradients, and the backward of the replay-buffer collect.
//
//   training forward  lstm_encode_kernel<.., SAVE = true> (seq_lstm.h): the chain of seq.hip, the same arithmetic in the same order,
//                     plus one 16-byte store per lane, gate and step: i, f, g, o and c_t in accumulator order (saved_index).
//   reverse chain     one workgroup owns the same 16 users for all steps of a launch and walks them downwards.  Wave w owns hidden
//                     tiles w and w + 8 as in the forward, so a lane meets the (user, hidden unit) pairs whose gates it saved: the
//                     gate derivatives are lane-local.  da[16, 4H] of a step is staged in LDS (double-buffered: one barrier per
//                     step) and dh_rec[16, H] = da . W_hh runs on v_mfma_f32_16x16x4_f32 with the contraction cut by gate into four
//                     accumulators per hidden tile, added ((i + f) + g) + o: four independent MFMA chains per wave and hidden tile,
//                     and an accumulator tile is again the lane's own (user, hidden unit) set, so dh_rec and dc never leave
//                     registers inside a launch.  W_hh is read from a transposed copy [H, 4H] made once per backward call:
//                     the contraction index is contiguous and a lane loads 16 bytes, the forward's access pattern.
//                     T is cut into launches of LSTM_CHUNK steps (the da workspace is per chunk); dh / dc pass through two [U, H]
//                     buffers in stream order.  A launch adds nothing and reorders nothing, so the cut changes no bit.
//   weight gradients  per chunk, grid-wide: dW[m, n] = sum over the chunk's (user, step) samples of da[s, m] X[s, n], X = h_{t-1}
//                     rows (dW_hh) or table rows gathered through the store (dW_ih; [U, T, E] is never materialised).  One
//                     workgroup owns a 64 x 64 tile of dW and walks ALL samples in order, 16 per LDS stage, on the exact-f32 MFMA:
//                     no partial sums between workgroups.  The rating column of dW_ih and db are rank-1 / plain sums on the VALU
//                     of the same stage.  Chunks are added into dW in launch order (last chunk first).  No atomics anywhere.
//                     Only the rows of real users are walked: the clamped rows of a partly filled tile give nothing.
//                     (The kernels of this and of the table gradient live in seq_grad.h, shared with the GRU encoder of gru.hip.)
//                     (dw_tile.h / gemm.h are bf16 tiles; the gradients here are exact f32, so they are not reused.)
//   table gradient   (recnn_lstm_backward_table only) d_table[item] = sum of dX[u, t, 0:E] over the call's positions (u, t) that hold
//                     `item`, dX[u, t, n] = sum_m da[u, t, m] W_ih[m, n].  dX: one launch per chunk after its chain launch, a grid
//                     over tiles of 16 samples (real users only), wave w of a workgroup owning column tiles w and w + 4, on the
//                     exact-f32 MFMA.  One accumulator per element, from zero; the contraction walks m in blocks of 16 upwards,
//                     four MFMAs e = 0 .. 3 per block, MFMA e adding the products m = m0 + e, m0 + 4 + e, m0 + 8 + e, m0 + 12 + e.
//                     W_ih[:, 0:E] (row stride E + 1: 4-byte aligned only) is read from a packed transposed copy [E][4H] made
//                     once per call, so the contraction index is contiguous and a lane loads 16 bytes of either operand.  dX is
//                     written to a [U, T, E] buffer for the WHOLE call -- the one place where [U, T, E] is materialised -- so that
//                     the scatter's order does not depend on the chunk cut.  The scatter-sum runs once per call over the inverted
//                     index of scatter_index.h (stable counting sort by item id, per item its contributions in ascending
//                     j = u T + t; built before the chain starts, it does not depend on da): the sorted entries are cut into
//                     pieces of 16, a wave sums the run of each item inside its piece in list order from zero, and one wave per
//                     item adds the piece partials of its list in piece order from zero.  Every row of d_table is written
//                     (untouched items: exact zeros).  No float atomics.  Ids outside the table are in no list.
//   collect backward  g_h[u, t] = g_next_state[k U + u] where steps[k] == t, plus g_state[k' U + u] where steps[k'] == t + 1: a
//                     gather over 16-byte chunks of g_h (flat_walk.h), each chunk summing its two or fewer sources.
#include "seq_grad.h"

namespace {

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

// ------------------------------------------------------------------------------------------------ W_hh^T
__global__ __launch_bounds__(256) void lstm_whh_transpose_kernel(const float* __restrict__ w, int H, float* __restrict__ wt) {
  const int G = 4 * H;
  flat_walk<1>((int64_t)H * G, [&](int64_t i, Width<1>) {
    const int j = (int)(i / G), k = (int)(i - (int64_t)j * G);
    wt[i] = w[(int64_t)k * H + j];
  });
}

// ------------------------------------------------------------------------------------------------ reverse chain
struct BwdArgs {
  int U, T, H;                       // T: steps of the whole call (saved and g_h are [.., T, ..])
  int tb, Tc;                        // this launch walks the call's steps tb + Tc - 1 down to tb
  const float* saved;
  const float* w_hhT;                // [H][4H]
  const float *c0, *g_h, *g_hT, *g_cT;
  const float *dh_in, *dc_in;        // [U][H] from the launch of the later chunk; NULL: zeros (the call's last chunk)
  float *dh_out, *dc_out;            // [U][H]: d h_{tb - 1}, d c_{tb - 1}
  float* da;                         // [user tiles * 16][da_T][4H]: this chunk's gate pre-activation gradients; NULL: not wanted
  int da_T;
};

inline size_t bwd_lds(int H) { return (size_t)2 * MT * (4 * H + PAD) * sizeof(float); }

template <int TPW>
__global__ __launch_bounds__(NT) void lstm_bwd_chain_kernel(const BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = a.H, U = a.U, G = 4 * H, ldd = G + PAD, ntiles = H >> 4;
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

  // what a step reads: the gates and c_{t-1} of the lane's pairs, and g_h[u, t]
  auto load_gates = [&](int t, f32x4 (&gt)[TPW][4]) {
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        gt[j][q] = on[j] ? sv[saved_index(blockIdx.x, a.T, t, ntiles, jt[j], q, lane)] : zero4;
  };
  auto load_c = [&](int t, f32x4 (&cv)[TPW]) {      // c_t; t = -1: c0 (or zero)
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      cv[j] = zero4;
      if (!on[j]) continue;
      if (t >= 0) {
        cv[j] = sv[saved_index(blockIdx.x, a.T, t, ntiles, jt[j], 4, lane)];
      } else if (a.c0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) cv[j][i] = a.c0[(int64_t)uc[i] * H + jt[j] * 16 + r];
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
  f32x4 dhr[TPW], dcn[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    dhr[j] = zero4;
    dcn[j] = zero4;
    if (!on[j]) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t o = (int64_t)uc[i] * H + jt[j] * 16 + r;
      if (a.dh_in && live[i]) dhr[j][i] = a.dh_in[o];
      if (a.dc_in && live[i]) dcn[j][i] = a.dc_in[o];
    }
  }
  const int t_last = a.tb + a.Tc - 1;
  const bool call_end = t_last == a.T - 1;            // the call's last step takes g_hT / g_cT
  f32x4 gt[TPW][4], cc[TPW], cp[TPW], gh[TPW];
  load_gates(t_last, gt);
  load_c(t_last, cc);
  load_c(t_last - 1, cp);
  load_gh(t_last, gh);

  const float* wrow[TPW][4];
#pragma unroll
  for (int j = 0; j < TPW; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) wrow[j][q] = a.w_hhT + (int64_t)((on[j] ? jt[j] : 0) * 16 + r) * G + q * H + 4 * g;

  for (int tl = a.Tc - 1; tl >= 0; --tl) {
    const int t = a.tb + tl;
    float* ds = smem + ((tl & 1) ? MT * ldd : 0);
    // ---- gate derivatives of the lane's pairs -> da in LDS
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      if (!on[j]) continue;
      const int hid = jt[j] * 16 + r;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float ig = gt[j][0][i], fg = gt[j][1][i], gg = gt[j][2][i], og = gt[j][3][i];
        const float tc = tanhf(cc[j][i]);
        float dh = gh[j][i] + dhr[j][i];
        float dcin = dcn[j][i];
        if (call_end && tl == a.Tc - 1) {
          if (a.g_hT && live[i]) dh += a.g_hT[(int64_t)uc[i] * H + hid];
          if (a.g_cT && live[i]) dcin += a.g_cT[(int64_t)uc[i] * H + hid];
        }
        const float dc = dcin + dh * og * (1.f - tc * tc);
        const float da_o = dh * tc * og * (1.f - og);
        const float da_i = dc * gg * ig * (1.f - ig);
        const float da_f = dc * cp[j][i] * fg * (1.f - fg);
        const float da_g = dc * ig * (1.f - gg * gg);
        dcn[j][i] = live[i] ? dc * fg : 0.f;
        float* row = ds + (4 * g + i) * ldd + hid;
        row[0] = live[i] ? da_i : 0.f;
        row[H] = live[i] ? da_f : 0.f;
        row[2 * H] = live[i] ? da_g : 0.f;
        row[3 * H] = live[i] ? da_o : 0.f;
      }
    }
    __syncthreads();
    // ---- the next (earlier) step's operands, in flight under this step's products
#pragma unroll
    for (int j = 0; j < TPW; ++j) cc[j] = cp[j];
    if (tl > 0) {
      load_gates(t - 1, gt);
      load_c(t - 2, cp);
      load_gh(t - 1, gh);
    }
    // ---- da of this step -> the chunk's workspace, for the weight gradients
    if (a.da) {
      const int G4 = G >> 2;
      for (int idx = tid; idx < MT * G4; idx += NT) {
        const int row = idx / G4, c4 = idx - row * G4;
        *(float4*)(a.da + ((int64_t)(u0 + row) * a.da_T + tl) * G + 4 * c4) = *(const float4*)(ds + row * ldd + 4 * c4);
      }
    }
    // ---- dh_rec[16, H] = da[16, 4H] . W_hh: per hidden tile one accumulator per gate block of the contraction (one hidden tile
    // at a time: four chains per wave in flight keep the MFMA issuing, and the operands of eight would not fit the registers)
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      if (!on[j]) continue;
      f32x4 acc[4], bn[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[q] = zero4;
        bn[q] = *(const f32x4*)(wrow[j][q]);
      }
      for (int k0 = 0; k0 < H; k0 += 16) {
        f32x4 av[4], bv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) av[q] = *(const f32x4*)(ds + r * ldd + q * H + k0 + 4 * g);
        const int kn = k0 + 16 < H ? k0 + 16 : k0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          bv[q] = bn[q];
          bn[q] = *(const f32x4*)(wrow[j][q] + kn);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q][e], bv[q][e], acc[q], 0, 0, 0);
      }
      dhr[j] = ((acc[0] + acc[1]) + acc[2]) + acc[3];
    }
    // (no barrier here: the next step writes the other LDS buffer, and its barrier orders this step's reads before the
    // step after it writes this buffer again)
  }

#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    if (!on[j]) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!live[i]) continue;
      const int64_t o = (int64_t)uc[i] * H + jt[j] * 16 + r;
      a.dh_out[o] = dhr[j][i];
      a.dc_out[o] = dcn[j][i];
    }
  }
}

// workspace of a backward call: W_hh^T, the dh / dc hand-over buffers, one chunk of da
struct BwdWs {
  int64_t wt, dh, dc, da, total;    // byte offsets
};
inline BwdWs bwd_ws(int n_users, int T, int H) {
  BwdWs w;
  const int64_t state = ((int64_t)n_users * H * 4 + 15) & ~(int64_t)15;
  w.wt = 0;
  w.dh = (int64_t)H * 4 * H * 4;
  w.dc = w.dh + state;
  w.da = w.dc + state;
  w.total = w.da + (int64_t)user_tiles(n_users) * MT * (T < LSTM_CHUNK ? T : LSTM_CHUNK) * 4 * H * 4;
  return w;
}

}  // namespace

extern "C" int recnn_lstm_train_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int variant, int64_t* saved_bytes,
                                                int64_t* bwd_bytes) {
  RECNN_REQUIRE(saved_bytes && bwd_bytes, "lstm_train_workspace_bytes: null pointer");
  RECNN_LSTM_DIMS_OK("lstm_train_workspace_bytes", emb_dim, hidden);
  RECNN_REQUIRE(n_users >= 0 && T >= 0 && (variant == 0 || variant == 1),
                "lstm_train_workspace_bytes: need n_users >= 0, T >= 0, variant 0 or 1");
  *saved_bytes = saved_bytes_of(n_users, T, hidden);
  *bwd_bytes = bwd_ws(n_users, T, hidden).total;
  return 0;
}

extern "C" int recnn_lstm_encode_train(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                                       int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden,
                                       const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* h0,
                                       const float* c0, float* h_out, float* h_T, float* c_T, int variant, void* workspace, void* saved,
                                       void* stream) {
  RECNN_REQUIRE(store_ok(items, ratings, user_off, slots, table) && w_ih && w_hh && b_ih && b_hh && h_out && h_T && c_T && saved,
                "lstm_encode_train: null pointer");
  RECNN_REQUIRE((h0 == nullptr) == (c0 == nullptr), "lstm_encode_train: h0 and c0 come together");
  RECNN_LSTM_DIMS_OK("lstm_encode_train", emb_dim, hidden);
  RECNN_REQUIRE(n_users >= 0 && t0 >= 0 && T >= 0 && n_items > 0, "lstm_encode_train: need n_users, t0, T >= 0 and n_items > 0");
  RECNN_REQUIRE(variant == 0 || variant == 1, "lstm_encode_train: variant must be 0 (fused input projection) or 1 (chunked), got %d",
                variant);
  RECNN_REQUIRE(variant == 0 || workspace, "lstm_encode_train: variant 1 needs the workspace of recnn_lstm_workspace_bytes");
  RECNN_REQUIRE(aligned16(table, w_hh, workspace, saved), "lstm_encode_train: table, w_hh, workspace and saved must be 16-byte aligned");
  if (n_users == 0) return 0;
  EncArgs a{};
  a.s = SeqStore{items, ratings, user_off, slots, n_users, table, n_items, emb_dim};
  a.H = hidden;
  a.w_ih = w_ih; a.w_hh = w_hh; a.b_ih = b_ih; a.b_hh = b_hh;
  a.h_out = h_out; a.h_T = h_T; a.c_T = c_T;
  a.pre = (float*)workspace;
  a.saved = (float*)saved;
  launch_encode<true>(a, t0, T, h0, c0, variant, (hipStream_t)stream);
  return recnn_check_hip(hipGetLastError(), "lstm_encode_train");
}

extern "C" int recnn_lstm_table_grad_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int n_items, int64_t* bytes) {
  RECNN_REQUIRE(bytes, "lstm_table_grad_workspace_bytes: null pointer");
  RECNN_LSTM_DIMS_OK("lstm_table_grad_workspace_bytes", emb_dim, hidden);
  RECNN_REQUIRE(n_users >= 0 && T >= 0 && n_items >= 1 && (int64_t)n_users * T < (1LL << 31),
                "lstm_table_grad_workspace_bytes: need n_users >= 0, T >= 0, n_items >= 1 and n_users * T < 2^31");
  *bytes = table_ws(n_users, T, 4 * hidden, emb_dim, n_items).total;
  return 0;
}

// recnn_lstm_backward (d_table == NULL: w_ih and table_workspace are not looked at) and recnn_lstm_backward_table
static int lstm_backward_impl(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                              int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_ih,
                              const float* w_hh, const void* saved, const float* h_out, const float* h0, const float* c0,
                              const float* g_h, const float* g_hT, const float* g_cT, float* d_w_ih, float* d_w_hh, float* d_b,
                              float* d_h0, float* d_c0, float* d_table, void* workspace, void* table_workspace, void* stream) {
  RECNN_REQUIRE(store_ok(items, ratings, user_off, slots, table) && w_hh && saved && h_out && workspace, "lstm_backward: null pointer");
  RECNN_REQUIRE((h0 == nullptr) == (c0 == nullptr), "lstm_backward: h0 and c0 come together");
  RECNN_LSTM_DIMS_OK("lstm_backward", emb_dim, hidden);
  RECNN_REQUIRE(n_users >= 0 && t0 >= 0 && T >= 1 && n_items > 0, "lstm_backward: need n_users, t0 >= 0, T >= 1 and n_items > 0");
  RECNN_REQUIRE(aligned16(table, w_hh, saved, h_out, h0, workspace),
                "lstm_backward: table, w_hh, saved, h_out, h0 and workspace must be 16-byte aligned");
  if (d_table) {
    RECNN_REQUIRE(w_ih && table_workspace, "lstm_backward_table: null pointer (w_ih, table_workspace)");
    RECNN_REQUIRE(aligned16(d_table, table_workspace), "lstm_backward_table: d_table and table_workspace must be 16-byte aligned");
    RECNN_REQUIRE((int64_t)n_users * T < (1LL << 31), "lstm_backward_table: n_users * T must stay below 2^31");
  }
  const hipStream_t s = (hipStream_t)stream;
  if (n_users == 0) {
    if (d_table) RECNN_HIP(hipMemsetAsync(d_table, 0, (size_t)n_items * emb_dim * sizeof(float), s));
    return 0;
  }
  const int H = hidden, G = 4 * H;
  const BwdWs w = bwd_ws(n_users, T, H);
  char* ws = (char*)workspace;
  float* wt = (float*)(ws + w.wt);
  float* dh = (float*)(ws + w.dh);
  float* dc = (float*)(ws + w.dc);
  const bool want_w = d_w_ih || d_w_hh || d_b;
  const size_t lds = bwd_lds(H);
  const bool two = H > 16 * NWV;
  if (lds > 48 * 1024)
    RECNN_HIP(hipFuncSetAttribute(two ? (const void*)lstm_bwd_chain_kernel<2> : (const void*)lstm_bwd_chain_kernel<1>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(lstm_whh_transpose_kernel, dim3(grid_for((int64_t)H * G, 256, 2048)), dim3(256), 0, s, w_hh, H, wt);

  BwdArgs a{};
  a.U = n_users; a.T = T; a.H = H;
  a.saved = (const float*)saved;
  a.w_hhT = wt;
  a.c0 = c0; a.g_h = g_h; a.g_hT = g_hT; a.g_cT = g_cT;
  a.da = want_w || d_table ? (float*)(ws + w.da) : nullptr;
  a.da_T = T < LSTM_CHUNK ? T : LSTM_CHUNK;
  DwArgs d{};
  d.s = SeqStore{items, ratings, user_off, slots, n_users, table, n_items, emb_dim};
  d.t0 = t0;
  d.U = n_users; d.T = T; d.H = H; d.da_T = a.da_T;
  d.G = G; d.lda = G; d.msplit = G; d.mshift = 0;
  d.da = a.da;
  // the table gradient's operands that do not depend on da: the packed W_ih^T and the inverted index of the call's positions
  TableGrad tg{};
  if (d_table) RECNN_HIP(table_grad_prepare(tg, d.s, t0, T, G, G, a.da_T, a.da, w_ih, table_workspace, s));
  const int nchunks = (T + LSTM_CHUNK - 1) / LSTM_CHUNK;
  for (int ci = nchunks - 1; ci >= 0; --ci) {
    a.tb = ci * LSTM_CHUNK;
    a.Tc = T - a.tb < LSTM_CHUNK ? T - a.tb : LSTM_CHUNK;
    a.dh_in = ci == nchunks - 1 ? nullptr : dh;
    a.dc_in = ci == nchunks - 1 ? nullptr : dc;
    a.dh_out = ci == 0 && d_h0 ? d_h0 : dh;
    a.dc_out = ci == 0 && d_c0 ? d_c0 : dc;
    const dim3 grid(user_tiles(n_users));
    if (two) hipLaunchKernelGGL((lstm_bwd_chain_kernel<2>), grid, dim3(NT), lds, s, a);
    else hipLaunchKernelGGL((lstm_bwd_chain_kernel<1>), grid, dim3(NT), lds, s, a);
    if (d_table) table_grad_chunk(tg, a.tb, a.Tc, s);
    if (!want_w) continue;
    d.tb = a.tb; d.Tc = a.Tc;
    d.accumulate = ci != nchunks - 1;
    if (d_w_hh) {
      DwArgs x = d;
      x.h_out = h_out; x.h0 = h0;
      x.out = d_w_hh; x.ldo = H; x.N = H;
      hipLaunchKernelGGL((seq_dw_kernel<false, false>), dim3(G / DW_T, (H + DW_T - 1) / DW_T), dim3(256), 0, s, x);
    }
    if (d_w_ih || d_b) {
      DwArgs x = d;
      x.out = d_w_ih; x.ldo = emb_dim + 1; x.N = emb_dim;
      x.d_wr = d_w_ih ? d_w_ih + emb_dim : nullptr;
      x.d_b = d_b;
      hipLaunchKernelGGL((seq_dw_kernel<true, false>), dim3(G / DW_T, d_w_ih ? (emb_dim + DW_T - 1) / DW_T : 1), dim3(256), 0, s, x);
    }
  }
  if (d_table) table_grad_finish(tg, d_table, s);
  return recnn_check_hip(hipGetLastError(), d_table ? "lstm_backward_table" : "lstm_backward");
}

extern "C" int recnn_lstm_backward(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                                   int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_hh,
                                   const void* saved, const float* h_out, const float* h0, const float* c0, const float* g_h,
                                   const float* g_hT, const float* g_cT, float* d_w_ih, float* d_w_hh, float* d_b, float* d_h0,
                                   float* d_c0, void* workspace, void* stream) {
  return lstm_backward_impl(items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, nullptr, w_hh, saved,
                            h_out, h0, c0, g_h, g_hT, g_cT, d_w_ih, d_w_hh, d_b, d_h0, d_c0, nullptr, workspace, nullptr, stream);
}

extern "C" int recnn_lstm_backward_table(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                                         int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden,
                                         const float* w_ih, const float* w_hh, const void* saved, const float* h_out, const float* h0,
                                         const float* c0, const float* g_h, const float* g_hT, const float* g_cT, float* d_w_ih,
                                         float* d_w_hh, float* d_b, float* d_h0, float* d_c0, float* d_table, void* workspace,
                                         void* table_workspace, void* stream) {
  RECNN_REQUIRE(d_table, "lstm_backward_table: null pointer (d_table; recnn_lstm_backward is the call without it)");
  return lstm_backward_impl(items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, w_ih, w_hh, saved, h_out,
                            h0, c0, g_h, g_hT, g_cT, d_w_ih, d_w_hh, d_b, d_h0, d_c0, d_table, workspace, table_workspace, stream);
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
