// seq_bwd.h -- the reverse half of the two state encoders (seq_chain.h is the forward half): the W_hh
// transpose, the reverse chain's arguments, the workspace layout and the checked host call, shared by the cells of lstm.hip / gru.hip.
//
//   reverse chain     one workgroup owns the same 16 users for all steps of a launch and walks them downwards.  Wave w owns hidden
//                     tiles w and w + 8 as in the forward, so a lane meets the (user, hidden unit) pairs whose gates it saved: the
//                     gate derivatives are lane-local.  The panel [16][4H] of a step -- four quantities per pair, both cells -- is
//                     staged in LDS (double-buffered: one barrier per step) and dh_rec[16, H] = panel . W_hh runs on
//                     v_mfma_f32_16x16x4_f32 with the contraction cut by W_hh's row blocks into one accumulator each per hidden
//                     tile, added in a fixed order: independent MFMA chains per wave and hidden tile, and an accumulator tile is
//                     again the lane's own (user, hidden unit) set, so dh_rec and the cell's carry never leave registers inside a
//                     launch.  W_hh is read from a transposed copy [H, NG H] made once per backward call: the contraction index is
//                     contiguous and a lane loads 16 bytes, the forward's access pattern.
//                     T is cut into launches of LSTM_CHUNK steps (the panel workspace is per chunk); dh and the carry pass through
//                     [U, H] buffers in stream order.  A launch adds nothing and reorders nothing, so the cut changes no bit.
//                     Rows past the batch write zeros into the panel and nothing to global memory.
//                     The chain KERNEL is each cell's own (lstm_bwd_chain_kernel, gru_bwd_chain_kernel): one template with the
//                     gate derivatives, loads and carry as cell hooks computed the same bits but ran the GRU's backward 0.2-0.7 %
//                     slower than its own kernel (other hook shapes: up to 1.8 %), so this family stays per cell; everything
//                     around it is here.
//   weight and table gradients: seq_grad.h.
//
// What a Cell supplies here, besides the constants of seq_chain.h: BWD[2] (the names of its two backward calls), BwdState (the
// kernel arguments of its own tensors), chunk_state (the hand-over pointers of a chunk launch), launch_dw (its seq_dw_kernel
// launches), and its chain kernel for one and two hidden tiles per wave, handed to backward_impl.
#pragma once
#include "seq_grad.h"

namespace {

// W_hh [G][H] -> W_hh^T [H][G]
__global__ __launch_bounds__(256) void whh_transpose_kernel(const float* __restrict__ w, int H, int G, float* __restrict__ wt) {
  flat_walk<1>((int64_t)H * G, [&](int64_t i, Width<1>) {
    const int j = (int)(i / G), k = (int)(i - (int64_t)j * G);
    wt[i] = w[(int64_t)k * H + j];
  });
}

template <class Cell>
struct BwdArgs {
  int U, T, H;                       // T: steps of the whole call (saved, h_out and g_h are [.., T, ..])
  int tb, Tc;                        // this launch walks the call's steps tb + Tc - 1 down to tb
  const float* saved;
  const float* w_hhT;                // [H][NG H]
  typename Cell::BwdState st;
  const float *g_h, *g_hT;
  const float* dh_in;                // [U][H] from the launch of the later chunk; NULL: zeros (the call's last chunk)
  float* dh_out;                     // [U][H]: d h_{tb - 1}
  float* da;                         // [user tiles * 16][da_T][4H]: this chunk's panels; NULL: not wanted
  int da_T;
};

inline size_t bwd_lds(int H) { return (size_t)2 * MT * (4 * H + PAD) * sizeof(float); }

// workspace of a backward call: W_hh^T [H][NG H], the hand-over buffers (dh, and dc for a cell with two states), one chunk of panels
struct BwdWs {
  int64_t wt, dh, dc, da, total;    // byte offsets; dc means something for NSTATE == 2 only (else it is da: never handed on)
};
template <class Cell>
inline BwdWs bwd_ws(int n_users, int T, int H) {
  BwdWs w;
  const int64_t state = ((int64_t)n_users * H * 4 + 15) & ~(int64_t)15;
  w.wt = 0;
  w.dh = (int64_t)H * Cell::NG * H * 4;
  w.dc = w.dh + state;
  w.da = w.dh + Cell::NSTATE * state;
  w.total = w.da + (int64_t)user_tiles(n_users) * MT * chunk_steps(T) * 4 * H * 4;
  return w;
}

// recnn_<cell>_train_workspace_bytes and recnn_<cell>_table_grad_workspace_bytes
template <class Cell>
int train_workspace_bytes_impl(const char* what, int n_users, int T, int hidden, int emb_dim, int variant, int64_t* saved_bytes,
                               int64_t* bwd_bytes) {
  RECNN_REQUIRE(saved_bytes && bwd_bytes, "%s: null pointer", what);
  RECNN_LSTM_DIMS_OK(what, emb_dim, hidden);
  RECNN_REQUIRE(n_users >= 0 && T >= 0 && (variant == 0 || variant == 1), "%s: need n_users >= 0, T >= 0, variant 0 or 1", what);
  *saved_bytes = acc_bytes(n_users, T, hidden, Cell::SAVED_Q);
  *bwd_bytes = bwd_ws<Cell>(n_users, T, hidden).total;
  return 0;
}
template <class Cell>
int table_grad_workspace_bytes_impl(const char* what, int n_users, int T, int hidden, int emb_dim, int n_items, int64_t* bytes) {
  RECNN_REQUIRE(bytes, "%s: null pointer", what);
  RECNN_LSTM_DIMS_OK(what, emb_dim, hidden);
  RECNN_REQUIRE(n_users >= 0 && T >= 0 && n_items >= 1 && (int64_t)n_users * T < (1LL << 31),
                "%s: need n_users >= 0, T >= 0, n_items >= 1 and n_users * T < 2^31", what);
  *bytes = table_ws(n_users, T, Cell::NG * hidden, emb_dim, n_items).total;
  return 0;
}

// recnn_<cell>_backward (d_table == NULL: w_ih and table_workspace are not looked at) and recnn_<cell>_backward_table.
// c0, g_cT, d_c0: cells with NSTATE = 2.  A cell with one bias gradient takes it as d_b_ih.
template <class Cell>
int backward_impl(void (*chain1)(BwdArgs<Cell>), void (*chain2)(BwdArgs<Cell>), const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users, int t0, int T,
                  const float* table, int n_items, int emb_dim, int hidden, const float* w_ih, const float* w_hh, const void* saved,
                  const float* h_out, const float* h0, const float* c0, const float* g_h, const float* g_hT, const float* g_cT,
                  float* d_w_ih, float* d_w_hh, float* d_b_ih, float* d_b_hh, float* d_h0, float* d_c0, float* d_table, void* workspace,
                  void* table_workspace, void* stream) {
  const char *what = Cell::BWD[0], *what_t = Cell::BWD[1];
  RECNN_REQUIRE(store_ok(items, ratings, user_off, slots, table) && w_hh && saved && h_out && workspace, "%s: null pointer", what);
  RECNN_REQUIRE(Cell::NSTATE == 1 || (h0 == nullptr) == (c0 == nullptr), "%s: h0 and c0 come together", what);
  RECNN_LSTM_DIMS_OK(what, emb_dim, hidden);
  RECNN_REQUIRE(n_users >= 0 && t0 >= 0 && T >= 1 && n_items > 0, "%s: need n_users, t0 >= 0, T >= 1 and n_items > 0", what);
  RECNN_REQUIRE(aligned16(table, w_hh, saved, h_out, h0, workspace),
                "%s: table, w_hh, saved, h_out, h0 and workspace must be 16-byte aligned", what);
  if (d_table) {
    RECNN_REQUIRE(w_ih && table_workspace, "%s: null pointer (w_ih, table_workspace)", what_t);
    RECNN_REQUIRE(aligned16(d_table, table_workspace), "%s: d_table and table_workspace must be 16-byte aligned", what_t);
    RECNN_REQUIRE((int64_t)n_users * T < (1LL << 31), "%s: n_users * T must stay below 2^31", what_t);
  }
  const hipStream_t s = (hipStream_t)stream;
  void (*const chain)(BwdArgs<Cell>) = hidden > 16 * NWV ? chain2 : chain1;
  if (n_users == 0) {
    if (d_table) RECNN_HIP(hipMemsetAsync(d_table, 0, (size_t)n_items * emb_dim * sizeof(float), s));
    return 0;
  }
  const int H = hidden, G = Cell::NG * H, P = 4 * H;
  const BwdWs w = bwd_ws<Cell>(n_users, T, H);
  char* ws = (char*)workspace;
  float* wt = (float*)(ws + w.wt);
  float* dh = (float*)(ws + w.dh);
  const bool want_w = d_w_ih || d_w_hh || d_b_ih || d_b_hh;
  const size_t lds = bwd_lds(H);
  if (int rc = raise_lds(chain, lds)) return rc;
  hipLaunchKernelGGL(whh_transpose_kernel, dim3(grid_for((int64_t)H * G, 256, 2048)), dim3(256), 0, s, w_hh, H, G, wt);

  BwdArgs<Cell> a{};
  a.U = n_users; a.T = T; a.H = H;
  a.saved = (const float*)saved;
  a.w_hhT = wt;
  a.g_h = g_h; a.g_hT = g_hT;
  a.da = want_w || d_table ? (float*)(ws + w.da) : nullptr;
  a.da_T = chunk_steps(T);
  DwArgs d{};
  d.s = SeqStore{items, ratings, user_off, slots, n_users, table, n_items, emb_dim};
  d.t0 = t0;
  d.U = n_users; d.T = T; d.H = H; d.da_T = a.da_T;
  d.G = G; d.lda = P;
  d.da = a.da;
  // the table gradient's operands that do not depend on da: the packed W_ih^T and the inverted index of the call's positions
  TableGrad tg{};
  if (d_table) RECNN_HIP(table_grad_prepare(tg, d.s, t0, T, G, P, a.da_T, a.da, w_ih, table_workspace, s));
  const int nchunks = (T + LSTM_CHUNK - 1) / LSTM_CHUNK;
  for (int ci = nchunks - 1; ci >= 0; --ci) {
    const bool first = ci == nchunks - 1;       // the launch of the call's last steps
    a.tb = ci * LSTM_CHUNK;
    a.Tc = chunk_steps(T - a.tb);
    a.dh_in = first ? nullptr : dh;
    a.dh_out = ci == 0 && d_h0 ? d_h0 : dh;
    Cell::chunk_state(a.st, h_out, h0, c0, g_cT, first ? nullptr : (float*)(ws + w.dc), ci == 0 && d_c0 ? d_c0 : (float*)(ws + w.dc));
    hipLaunchKernelGGL(chain, dim3(user_tiles(n_users)), dim3(NT), lds, s, a);
    if (d_table) table_grad_chunk(tg, a.tb, a.Tc, s);
    if (!want_w) continue;
    d.tb = a.tb; d.Tc = a.Tc;
    d.accumulate = !first;
    Cell::launch_dw(d, h_out, h0, d_w_ih, d_w_hh, d_b_ih, d_b_hh, s);
  }
  if (d_table) table_grad_finish(tg, d_table, s);
  return recnn_check_hip(hipGetLastError(), d_table ? what_t : what);
}

}  // namespace
