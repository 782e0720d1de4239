// lstm.hip -- the LSTM state encoder of the dynamic-length path: what is the LSTM's own in the forward chain
// of seq_chain.h, its reverse chain kernel (seq_bwd.h has what surrounds it, and why it is per cell), and the recnn_lstm_* entry points.
//
//   cell             torch.nn.LSTM(E + 1, H), one layer, one direction, gate order i, f, g, o, weights read in place:
//                      c' = f c + i g          h' = o tanh(c')
//   forward chain    four accumulators per hidden tile, one per gate, each the whole fixed-order chain from
//                    fma(rating, w_ih[:, E], b_ih + b_hh); c lives in registers and passes between chunk launches through c_T,
//                    which is written even by a call of no steps (h_T is not).
//   training forward records i, f, g, o and c_t.
//   reverse chain      dh = g_h[:, t] + dh_rec (+ g_hT at the call's last step)     dc = dc_next f_{t+1} (+ g_cT) + dh o (1 - tanh(c)^2)
//                      da_o = dh tanh(c) o (1 - o)      da_i = dc g i (1 - i)
//                      da_f = dc c_{t-1} f (1 - f)      da_g = dc i (1 - g^2)
//                      dh_rec = [da_i | da_f | da_g | da_o] . W_hh, added ((i + f) + g) + o
//                    c_{t-1} is read back from the record (c0 at the call's step 0); dc passes between chunk launches like dh.
//   weight gradients the kernels of seq_grad.h over G = 4H rows, the panel's columns as they stand; one db (b_ih and b_hh share it).
#include "seq_bwd.h"

namespace {

struct LstmCell {
  static constexpr const char* NAME = "lstm";
  static constexpr const char* BWD[2] = {"lstm_backward", "lstm_backward_table"};
  static constexpr int NG = 4, PRE_Q = 4, SAVED_Q = 5, NSTATE = 2;
  static __device__ __forceinline__ constexpr int acc_slot(int q) { return q; }
  static __device__ __forceinline__ constexpr bool links_take_bhh(int) { return true; }

  // ---- forward
  using State = f32x4;               // c of the lane's four users
  static __device__ __forceinline__ const float* carried(const EncArgs& a) { return a.c0; }
  static __device__ __forceinline__ void init(State& c, f32x4& hl, int i, float c0) {
    c[i] = c0;
    hl[i] = 0.f;
  }
  static __device__ __forceinline__ void prepare(State&, const EncArgs&, bool, int) {}
  static __device__ __forceinline__ void seed(const State&, f32x4 (&)[4], int) {}
  template <bool SAVE>
  static __device__ __forceinline__ float update(State& c, const f32x4 (&acc)[4], int i, float, f32x4 (&sv)[SAVED_Q]) {
    const float ig = sigmoidf_(acc[0][i]), fg = sigmoidf_(acc[1][i]), gg = tanhf(acc[2][i]), og = sigmoidf_(acc[3][i]);
    c[i] = fg * c[i] + ig * gg;
    if constexpr (SAVE) { sv[0][i] = ig; sv[1][i] = fg; sv[2][i] = gg; sv[3][i] = og; sv[4][i] = c[i]; }
    return og * tanhf(c[i]);
  }
  static __device__ __forceinline__ void finish(const State& c, const EncArgs& a, int64_t o, int i) { a.c_T[o] = c[i]; }

  // ---- reverse
  struct BwdState {
    const float *c0, *g_cT;
    const float* dc_in;              // [U][H], as dh_in
    float* dc_out;                   // [U][H]: d c_{tb - 1}
  };
  static void chunk_state(BwdState& st, const float*, const float*, const float* c0, const float* g_cT, const float* dc_in,
                          float* dc_out) {
    st = BwdState{c0, g_cT, dc_in, dc_out};
  }
  // G = 4H is a multiple of 64 and row m of either dW reads panel column m; d_b_hh is not looked at
  static void launch_dw(DwArgs d, const float* h_out, const float* h0, float* d_w_ih, float* d_w_hh, float* d_b, float*,
                        hipStream_t s) {
    const int H = d.H, E = d.s.E;
    d.msplit = d.G; d.mshift = 0;
    if (d_w_hh) {
      DwArgs x = d;
      x.h_out = h_out; x.h0 = h0;
      x.out = d_w_hh; x.ldo = H; x.N = H;
      hipLaunchKernelGGL((seq_dw_kernel<false, false>), dim3(d.G / DW_T, (H + DW_T - 1) / DW_T), dim3(256), 0, s, x);
    }
    if (d_w_ih || d_b) {
      DwArgs x = d;
      x.out = d_w_ih; x.ldo = E + 1; x.N = E;
      x.d_wr = d_w_ih ? d_w_ih + E : nullptr;
      x.d_b = d_b;
      hipLaunchKernelGGL((seq_dw_kernel<true, false>), dim3(d.G / DW_T, d_w_ih ? (E + DW_T - 1) / DW_T : 1), dim3(256), 0, s, x);
    }
  }
};

// ------------------------------------------------------------------------------------------------ reverse chain
template <int TPW>
__global__ __launch_bounds__(NT) void lstm_bwd_chain_kernel(const BwdArgs<LstmCell> a) {
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
        gt[j][q] = on[j] ? sv[acc_index(blockIdx.x, a.T, t, ntiles, jt[j], LstmCell::SAVED_Q, q, lane)] : zero4;
  };
  auto load_c = [&](int t, f32x4 (&cv)[TPW]) {      // c_t; t = -1: c0 (or zero)
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      cv[j] = zero4;
      if (!on[j]) continue;
      if (t >= 0) {
        cv[j] = sv[acc_index(blockIdx.x, a.T, t, ntiles, jt[j], LstmCell::SAVED_Q, 4, lane)];
      } else if (a.st.c0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) cv[j][i] = a.st.c0[(int64_t)uc[i] * H + jt[j] * 16 + r];
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
      if (a.st.dc_in && live[i]) dcn[j][i] = a.st.dc_in[o];
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
          if (a.st.g_cT && live[i]) dcin += a.st.g_cT[(int64_t)uc[i] * H + hid];
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
      a.st.dc_out[o] = dcn[j][i];
    }
  }
}

}  // namespace

extern "C" int recnn_lstm_workspace_bytes(int n_users, int T, int hidden, int variant, int64_t* h_bytes) {
  return workspace_bytes_impl<LstmCell>("lstm_workspace_bytes", n_users, T, hidden, variant, h_bytes);
}

extern "C" int recnn_lstm_encode(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                                 int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_ih,
                                 const float* w_hh, const float* b_ih, const float* b_hh, const float* h0, const float* c0, float* h_out,
                                 float* h_T, float* c_T, int variant, void* workspace, void* stream) {
  return encode_impl<LstmCell>("lstm_encode", false, items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden,
                               w_ih, w_hh, b_ih, b_hh, h0, c0, h_out, h_T, c_T, variant, workspace, nullptr, stream);
}

extern "C" int recnn_lstm_train_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int variant, int64_t* saved_bytes,
                                                int64_t* bwd_bytes) {
  return train_workspace_bytes_impl<LstmCell>("lstm_train_workspace_bytes", n_users, T, hidden, emb_dim, variant, saved_bytes, bwd_bytes);
}

extern "C" int recnn_lstm_encode_train(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                                       int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden,
                                       const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* h0,
                                       const float* c0, float* h_out, float* h_T, float* c_T, int variant, void* workspace, void* saved,
                                       void* stream) {
  return encode_impl<LstmCell>("lstm_encode_train", true, items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim,
                               hidden, w_ih, w_hh, b_ih, b_hh, h0, c0, h_out, h_T, c_T, variant, workspace, saved, stream);
}

extern "C" int recnn_lstm_table_grad_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int n_items, int64_t* bytes) {
  return table_grad_workspace_bytes_impl<LstmCell>("lstm_table_grad_workspace_bytes", n_users, T, hidden, emb_dim, n_items, bytes);
}

extern "C" int recnn_lstm_backward(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                                   int t0, int T, const float* table, int n_items, int emb_dim, int hidden, const float* w_hh,
                                   const void* saved, const float* h_out, const float* h0, const float* c0, const float* g_h,
                                   const float* g_hT, const float* g_cT, float* d_w_ih, float* d_w_hh, float* d_b, float* d_h0,
                                   float* d_c0, void* workspace, void* stream) {
  return backward_impl<LstmCell>(lstm_bwd_chain_kernel<1>, lstm_bwd_chain_kernel<2>, items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, nullptr, w_hh, saved,
                                 h_out, h0, c0, g_h, g_hT, g_cT, d_w_ih, d_w_hh, d_b, nullptr, d_h0, d_c0, nullptr, workspace, nullptr,
                                 stream);
}

extern "C" int recnn_lstm_backward_table(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                                         int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden,
                                         const float* w_ih, const float* w_hh, const void* saved, const float* h_out, const float* h0,
                                         const float* c0, const float* g_h, const float* g_hT, const float* g_cT, float* d_w_ih,
                                         float* d_w_hh, float* d_b, float* d_h0, float* d_c0, float* d_table, void* workspace,
                                         void* table_workspace, void* stream) {
  RECNN_REQUIRE(d_table, "lstm_backward_table: null pointer (d_table; recnn_lstm_backward is the call without it)");
  return backward_impl<LstmCell>(lstm_bwd_chain_kernel<1>, lstm_bwd_chain_kernel<2>, items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, w_ih, w_hh, saved,
                                 h_out, h0, c0, g_h, g_hT, g_cT, d_w_ih, d_w_hh, d_b, nullptr, d_h0, d_c0, d_table, workspace,
                                 table_workspace, stream);
}
