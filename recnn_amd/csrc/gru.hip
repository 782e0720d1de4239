// gru.hip -- the GRU state encoder of the dynamic-length path: what is the GRU's own in the forward chain of
// seq_chain.h, its reverse chain kernel (seq_bwd.h has what surrounds it, and why it is per cell), and the recnn_gru_* entry points.
//
//   cell             torch.nn.GRU(E + 1, H), one layer, one direction, gate order r, z, n, weights read in place:
//                      r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)     z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
//                      hn = W_hn h + b_hn                             n = tanh(W_in x + b_in + r hn)
//                      h' = (1 - z) n + z h                           (computed as n + z (h - n))
//   forward chain    FOUR accumulators per hidden tile: r, z, nx (the input links of n) and nh (the h products of n, started
//                    from b_hn) -- the two halves of n meet only after r is known, so they cannot share one.  r and z are one
//                    fixed-order chain each: fma(rating, w_ih[:, E], b_ih + b_hh), the x products, the h products.  nx:
//                    fma(rating, w_ih[:, E], b_ih), the x products.  nh: b_hh, the h products.  A step issues three h-product
//                    MFMAs per k where the LSTM issues four.  h_{t-1} of a lane's own (user, hidden unit) pairs stays in registers,
//                    seeded from h0.  The projection workspace of variant 1 holds r, z and nx.
//   training forward records r, z, n and hn.  h_{t-1} is read back from h_out / h0.
//   reverse chain      dh = g_h[:, t] + dh_rec (+ g_hT at the call's last step)
//                      da_n = dh (1 - z)(1 - n^2)     da_z = dh (h_{t-1} - n) z (1 - z)
//                      da_r = da_n hn r (1 - r)       da_hn = da_n r
//                      dh_rec = dh z + [da_r | da_z | da_hn] . W_hh, added ((r + z) + hn) + dh z
//                    The panel is [da_r | da_z | da_n | da_hn]: W_hh^T's column blocks r, z, n meet panel blocks 0, 1 and 3.
//   weight gradients the kernels of seq_grad.h over G = 3H rows: dW_ih and db_ih from columns [da_r | da_z | da_n] of the panel, dW_hh
//                    and db_hh from [da_r | da_z | da_hn]: the two bias gradients differ in their last third.
//   table gradient   dX = [da_r | da_z | da_n] . W_ih[:, :E].
#include "seq_bwd.h"

namespace {

struct GruCell {
  static constexpr const char* NAME = "gru";
  static constexpr const char* BWD[2] = {"gru_backward", "gru_backward_table"};
  static constexpr int NG = 3, PRE_Q = 3, SAVED_Q = 4, NSTATE = 1;
  static __device__ __forceinline__ constexpr int acc_slot(int q) { return q < 2 ? q : 3; }
  static __device__ __forceinline__ constexpr bool links_take_bhh(int q) { return q != 2; }

  // ---- forward
  using State = float;               // b_hh of n, the seed of nh
  static __device__ __forceinline__ const float* carried(const EncArgs& a) { return a.h0; }
  static __device__ __forceinline__ void init(State&, f32x4& hl, int i, float h0) { hl[i] = h0; }
  static __device__ __forceinline__ void prepare(State& bhn, const EncArgs& a, bool on, int hid) { bhn = on ? a.b_hh[2 * a.H + hid] : 0.f; }
  static __device__ __forceinline__ void seed(const State& bhn, f32x4 (&acc)[4], int i) { acc[3][i] = bhn; }
  template <bool SAVE>
  static __device__ __forceinline__ float update(State&, const f32x4 (&acc)[4], int i, float hprev, f32x4 (&sv)[SAVED_Q]) {
    const float rg = sigmoidf_(acc[0][i]), zg = sigmoidf_(acc[1][i]);
    const float ng = tanhf(fmaf(rg, acc[3][i], acc[2][i]));
    if constexpr (SAVE) { sv[0][i] = rg; sv[1][i] = zg; sv[2][i] = ng; sv[3][i] = acc[3][i]; }
    return fmaf(zg, hprev - ng, ng);
  }
  static __device__ __forceinline__ void finish(const State&, const EncArgs&, int64_t, int) {}

  // ---- reverse
  struct BwdState {
    const float *h_out, *h0;
  };
  static void chunk_state(BwdState& st, const float* h_out, const float* h0, const float*, const float*, const float*, float*) {
    st = BwdState{h_out, h0};
  }
  // G = 3H need not be a multiple of 64, and the rows of dW_hh are [da_r | da_z | da_hn]: the last third sits one block further in the
  // panel; each launch sums a bias gradient of its own
  static void launch_dw(const DwArgs& d, const float* h_out, const float* h0, float* d_w_ih, float* d_w_hh, float* d_b_ih, float* d_b_hh,
                        hipStream_t s) {
    const int H = d.H, E = d.s.E, mtiles = (d.G + DW_T - 1) / DW_T;
    if (d_w_hh || d_b_hh) {
      DwArgs x = d;
      x.msplit = 2 * H; x.mshift = H;
      x.h_out = h_out; x.h0 = h0;
      x.out = d_w_hh; x.ldo = H; x.N = H;
      x.d_b = d_b_hh;
      hipLaunchKernelGGL((seq_dw_kernel<false, true>), dim3(mtiles, d_w_hh ? (H + DW_T - 1) / DW_T : 1), dim3(256), 0, s, x);
    }
    if (d_w_ih || d_b_ih) {             // rows [da_r | da_z | da_n]
      DwArgs x = d;
      x.msplit = d.G; x.mshift = 0;
      x.out = d_w_ih; x.ldo = E + 1; x.N = E;
      x.d_wr = d_w_ih ? d_w_ih + E : nullptr;
      x.d_b = d_b_ih;
      hipLaunchKernelGGL((seq_dw_kernel<true, true>), dim3(mtiles, d_w_ih ? (E + DW_T - 1) / DW_T : 1), dim3(256), 0, s, x);
    }
  }
};

// ------------------------------------------------------------------------------------------------ reverse chain
template <int TPW>
__global__ __launch_bounds__(NT) void gru_bwd_chain_kernel(const BwdArgs<GruCell> a) {
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
        gt[j][q] = on[j] ? sv[acc_index(blockIdx.x, a.T, t, ntiles, jt[j], GruCell::SAVED_Q, q, lane)] : zero4;
  };
  auto load_hprev = [&](int t, f32x4 (&hv)[TPW]) {      // h_{t-1}; t = 0: h0 (or zero)
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      hv[j] = zero4;
      if (!on[j]) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (t >= 1) hv[j][i] = a.st.h_out[((int64_t)uc[i] * a.T + t - 1) * H + jt[j] * 16 + r];
        else if (a.st.h0) hv[j][i] = a.st.h0[(int64_t)uc[i] * H + jt[j] * 16 + r];
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

}  // namespace

extern "C" int recnn_gru_workspace_bytes(int n_users, int T, int hidden, int variant, int64_t* bytes) {
  return workspace_bytes_impl<GruCell>("gru_workspace_bytes", n_users, T, hidden, variant, bytes);
}

extern "C" int recnn_gru_encode(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                                int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_ih,
                                const float* w_hh, const float* b_ih, const float* b_hh, const float* h0, float* h_out, float* h_T,
                                int variant, void* workspace, void* stream) {
  return encode_impl<GruCell>("gru_encode", false, items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, w_ih,
                              w_hh, b_ih, b_hh, h0, nullptr, h_out, h_T, nullptr, variant, workspace, nullptr, stream);
}

extern "C" int recnn_gru_train_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int variant, int64_t* saved_bytes,
                                               int64_t* bwd_bytes) {
  return train_workspace_bytes_impl<GruCell>("gru_train_workspace_bytes", n_users, T, hidden, emb_dim, variant, saved_bytes, bwd_bytes);
}

extern "C" int recnn_gru_encode_train(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                                      int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden,
                                      const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* h0,
                                      float* h_out, float* h_T, int variant, void* workspace, void* saved, void* stream) {
  return encode_impl<GruCell>("gru_encode_train", true, items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden,
                              w_ih, w_hh, b_ih, b_hh, h0, nullptr, h_out, h_T, nullptr, variant, workspace, saved, stream);
}

extern "C" int recnn_gru_table_grad_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int n_items, int64_t* bytes) {
  return table_grad_workspace_bytes_impl<GruCell>("gru_table_grad_workspace_bytes", n_users, T, hidden, emb_dim, n_items, bytes);
}

extern "C" int recnn_gru_backward(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                                  int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_hh,
                                  const void* saved, const float* h_out, const float* h0, const float* g_h, const float* g_hT,
                                  float* d_w_ih, float* d_w_hh, float* d_b_ih, float* d_b_hh, float* d_h0, void* workspace,
                                  void* stream) {
  return backward_impl<GruCell>(gru_bwd_chain_kernel<1>, gru_bwd_chain_kernel<2>, items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, nullptr, w_hh, saved,
                                h_out, h0, nullptr, g_h, g_hT, nullptr, d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_h0, nullptr, nullptr, workspace,
                                nullptr, stream);
}

extern "C" int recnn_gru_backward_table(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                                        int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden,
                                        const float* w_ih, const float* w_hh, const void* saved, const float* h_out, const float* h0,
                                        const float* g_h, const float* g_hT, float* d_w_ih, float* d_w_hh, float* d_b_ih, float* d_b_hh,
                                        float* d_h0, float* d_table, void* workspace, void* table_workspace, void* stream) {
  RECNN_REQUIRE(d_table, "gru_backward_table: null pointer (d_table; recnn_gru_backward is the call without it)");
  return backward_impl<GruCell>(gru_bwd_chain_kernel<1>, gru_bwd_chain_kernel<2>, items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, w_ih, w_hh, saved,
                                h_out, h0, nullptr, g_h, g_hT, nullptr, d_w_ih, d_w_hh, d_b_ih, d_b_hh, d_h0, nullptr, d_table, workspace,
                                table_workspace, stream);
}
