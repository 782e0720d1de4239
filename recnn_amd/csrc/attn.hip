// attn.hip -- the causal self-attention state encoder of the dynamic-length path: one layer of multi-head attention over
// a user's history, forward and backward, and the recnn_attn_* entry points.  Where the LSTM and the GRU (seq_chain.h) are a chain of
// T dependent steps, every step here is independent of the others: the work is parallel over (user, head, block of steps).
//
//   the layer        x_t = [table[item_t] | rating_t], [q_t | k_t | v_t] = W_in x_t + b_in, per head a of width d = H / heads:
//                      s(t, j) = (q_t . k_j) / sqrt(d) - m_a (t - j) for j in [max(0, t - window + 1), t], p = softmax_j s,
//                      o_t = sum_j p(t, j) v_j,  h_t = W_o o_t + b_o.         m_a = 2^(-8 (a + 1) / heads) (ALiBi) or 0.
//   linear kernels   attn_dev.h describes them: the in-projection is its gathered linear (rows read through the store, the rating
//                    as the chain's first link), the out-projection and dO = g_h W_o (over a transposed copy of W_o) its dense linear.
//   forward          one workgroup per (user, head, 64 query rows), heaviest blocks first; wave w owns 16 query rows.  Key tiles of 64
//                    lie on absolute multiples of 64 from the call's step 0 and are walked upwards from the first one the block's window
//                    reaches to the diagonal one; K and V tiles pass through LDS.  The products are computed transposed -- S^T = K Q^T,
//                    O^T = V^T P^T -- so that a lane holds, for ONE query (lane & 15), four keys per 16-key block in the accumulator of
//                    S^T, which is as it stands the B operand of the P V product: P never crosses lanes or LDS, and the running
//                    maximum, the running sum and the rescale factor of a query are the lane's own (two xor-shuffles fold the four
//                    lane groups).  Masking is a select on the score before the maximum.  A tile that is fully masked for a row leaves
//                    (max, sum, o) of the row as they were: the maximum stays -inf and is replaced by 0 in the exponent.
//   backward         dO = g_h W_o; P is recomputed from q, k and the saved log-sum-exp, which is kept in its two parts -- the row maximum m and
//                    l = sum exp(s - m) -- and used as exp(s - m) / l: rounding m + log l to one float would put up to half an ulp
//                    of a number of the scores' size (1e-6 at |s| = 20) into every probability of the row.  delta(t) = sum_j p(t, j) dP(t, j) is summed
//                    from the SAME dP bits that dS = p (dP - delta) then subtracts it from (a first sweep of the query owner; both owners
//                    compute dP as the same chain of products): where the softmax is peaked, dP - delta cancels, and the errors of dP
//                    cancel with it as they do in autograd's softmax backward.  The usual delta = rowsum(dO o) reaches the same number
//                    by another route, its error does not cancel, and the gradient bounds of the tests are missed (measured: 1.23
//                    bounds at U = 1, T = 63).  Then two launches, no float atomics, no hand-off between
//                    workgroups: the query owner (the forward's loop; dQ^T += K^T dS^T) and the key owner (one workgroup per 64 keys,
//                    its K and V fragments in registers, sweeping the query tiles in its reach upwards; Q, dO, lse and delta tiles in
//                    LDS; dV^T += dO^T P, dK^T += Q^T dS).  dqkv is written [U, T, 3H]; the weight gradients are the tile of
//                    seq_dw_kernel (seq_grad.h) over segments of the call's samples, the parts added in order (attn_dw_kernel of attn_dev.h);
//                    the table gradient is seq_grad.h's dX contraction and scatter-sum with da = dqkv.
//   append           recnn_attn_append: the layer on the n new steps of sessions whose keys and values live in a KV cache;
//                    the in-projection reads [n_rows, n] ids and ratings as a store whose histories are the rows, attn_dev.h's
//                    attn_cache_kernel is the forward above with its key tiles staged from the cache.
// Every sum has a fixed order that depends on nothing but (t, j): equal calls give equal bits, a user's bits do not depend on the batch,
// and h[:, :a] of a longer call equals the shorter call's.
#include "attn_dev.h"

namespace {

int attn_encode_impl(const char* what, const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                     int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden, int n_heads, int window,
                     int alibi, const float* w_in, const float* b_in, const float* w_o, const float* b_o, float* h_out, void* keep,
                     void* stream) {
  RECNN_REQUIRE(store_ok(items, ratings, user_off, slots, table) && w_in && b_in && w_o && b_o && h_out && keep, "%s: null pointer", what);
  RECNN_ATTN_DIMS_OK(what, emb_dim, hidden, n_heads);
  RECNN_ATTN_SIZE_OK(what, n_users, T);
  RECNN_REQUIRE(t0 >= 0 && T >= 1 && n_items > 0 && window >= 0, "%s: need t0 >= 0, T >= 1, n_items > 0 and window >= 0 (0: none)", what);
  RECNN_REQUIRE(aligned16(table, w_o, h_out, keep), "%s: table, w_o, h_out and the workspace / saved must be 16-byte aligned", what);
  if (n_users == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  const AttnWs w = attn_ws(n_users, T, hidden, n_heads);
  char* kp = (char*)keep;
  LinArgs l{};
  l.s = SeqStore{items, ratings, user_off, slots, n_users, table, n_items, emb_dim};
  l.t0 = t0; l.T = T; l.rows = n_users * T;
  l.K = emb_dim; l.w = w_in; l.ldw = emb_dim + 1; l.b = b_in;
  l.out = (float*)(kp + w.qkv); l.N = 3 * hidden;
  if (int rc = launch_linear(l, s)) return rc;
  AttnArgs a = attn_args(n_users, T, hidden, n_heads, window, alibi);
  a.qkv = (const float*)(kp + w.qkv);
  a.o = (float*)(kp + w.o);
  a.lse = (float*)(kp + w.lse);
  launch_query<0>(a, s);
  DenseLinArgs p{};
  p.rows = n_users * T; p.K = hidden; p.N = hidden;
  p.x = a.o; p.w = w_o; p.ldw = hidden; p.b = b_o;
  p.out = h_out;
  if (int rc = launch_dense_linear(p, false, s)) return rc;
  return recnn_check_hip(hipGetLastError(), what);
}

int attn_backward_impl(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users, int t0,
                       int T, const float* table, int n_items, int emb_dim, int hidden, int n_heads, int window, int alibi,
                       const float* w_in, const float* w_o, const void* saved, const float* g_h, float* d_w_in, float* d_b_in,
                       float* d_w_o, float* d_b_o, float* d_table, bool with_table, void* workspace, void* table_workspace,
                       void* stream) {
  const char* what = with_table ? "attn_backward_table" : "attn_backward";
  if (with_table)
    RECNN_REQUIRE(d_table && w_in && table_workspace,
                  "%s: null pointer (d_table, w_in, table_workspace; recnn_attn_backward is the call without them)", what);
  RECNN_REQUIRE(store_ok(items, ratings, user_off, slots, table) && w_o && saved && g_h && workspace, "%s: null pointer", what);
  RECNN_ATTN_DIMS_OK(what, emb_dim, hidden, n_heads);
  RECNN_ATTN_SIZE_OK(what, n_users, T);
  RECNN_REQUIRE(t0 >= 0 && T >= 1 && n_items > 0 && window >= 0, "%s: need t0 >= 0, T >= 1, n_items > 0 and window >= 0 (0: none)", what);
  RECNN_REQUIRE(aligned16(table, w_o, saved, g_h, workspace), "%s: table, w_o, saved, g_h and workspace must be 16-byte aligned", what);
  if (with_table) RECNN_REQUIRE(aligned16(d_table, table_workspace), "%s: d_table and table_workspace must be 16-byte aligned", what);
  const hipStream_t s = (hipStream_t)stream;
  if (n_users == 0) {
    if (with_table) RECNN_HIP(hipMemsetAsync(d_table, 0, (size_t)n_items * emb_dim * sizeof(float), s));
    return 0;
  }
  const int H = hidden, G = 3 * H;
  const AttnWs sv = attn_ws(n_users, T, H, n_heads);
  const AttnBwdWs w = attn_bwd_ws(n_users, T, H, emb_dim, n_heads);
  const char* sp = (const char*)saved;
  char* ws = (char*)workspace;
  const float* o = (const float*)(sp + sv.o);
  float* dqkv = (float*)(ws + w.dqkv);
  const SeqStore st{items, ratings, user_off, slots, n_users, table, n_items, emb_dim};
  // the table gradient's operands that do not depend on dqkv: the packed W_in^T and the inverted index of the call's positions
  TableGrad tg{};
  if (with_table) RECNN_HIP(table_grad_prepare(tg, st, t0, T, G, G, T, dqkv, w_in, table_workspace, s));
  // the weight gradients: the parts of one tensor's tile launch are summed before the next launch reuses the buffer (stream order)
  const int S = n_users * T;
  float* part = (float*)(ws + w.parts);
  // d_w_o[m, n] = sum_s g_h[s, m] o[s, n] and d_b_o[m] = sum_s g_h[s, m]
  launch_weight_grad(nullptr, t0, T, S, g_h, H, o, H, H, H, part, d_w_o, d_b_o, s);
  if (d_w_in || d_b_in || with_table) {
    hipLaunchKernelGGL(whh_transpose_kernel, dim3(grid_for((int64_t)H * H, 256, 2048)), dim3(256), 0, s, w_o, H, H, (float*)(ws + w.wt));
    DenseLinArgs p{};
    p.rows = S; p.K = H; p.N = H;
    p.x = g_h; p.w = (const float*)(ws + w.wt); p.ldw = H;
    p.out = (float*)(ws + w.d_o);
    if (int rc = launch_dense_linear(p, false, s)) return rc;
    AttnArgs a = attn_args(n_users, T, H, n_heads, window, alibi);
    a.qkv = (const float*)(sp + sv.qkv);
    a.lse = (float*)(sp + sv.lse);                  // (read only)
    a.d_o = p.out;
    a.delta = (const float*)(ws + w.delta);
    a.delta_out = (float*)(ws + w.delta);
    a.dqkv = dqkv;
    launch_query<1>(a, s);
    launch_key(a, s);
    launch_query<2>(a, s);
    if (with_table) {
      table_grad_chunk(tg, 0, T, s);
      table_grad_finish(tg, d_table, s);
    }
    // d_w_in (its rating column included) and d_b_in: da = dqkv, X rows gathered through the store
    launch_weight_grad(&st, t0, T, S, dqkv, G, nullptr, emb_dim, G, emb_dim, part, d_w_in, d_b_in, s);
  }
  return recnn_check_hip(hipGetLastError(), what);
}

}  // namespace

extern "C" int recnn_attn_workspace_bytes(int n_users, int T, int hidden, int n_heads, int64_t* bytes) {
  const char* what = "attn_workspace_bytes";
  RECNN_REQUIRE(bytes, "%s: null pointer", what);
  RECNN_ATTN_DIMS_OK(what, 8, hidden, n_heads);
  RECNN_ATTN_SIZE_OK(what, n_users, T);
  *bytes = attn_ws(n_users, T, hidden, n_heads).total;
  return 0;
}

extern "C" int recnn_attn_encode(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                                 int t0, int T, const float* table, int n_items, int emb_dim, int hidden, int n_heads, int window,
                                 int alibi, const float* w_in, const float* b_in, const float* w_o, const float* b_o, float* h_out,
                                 void* workspace, void* stream) {
  return attn_encode_impl("attn_encode", items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, n_heads, window,
                          alibi, w_in, b_in, w_o, b_o, h_out, workspace, stream);
}

extern "C" int recnn_kv_min_capacity(int window, int n, int* capacity) {
  const char* what = "kv_min_capacity";
  RECNN_REQUIRE(capacity, "%s: null pointer", what);
  RECNN_REQUIRE(window >= 1 && window < AT_NO_WINDOW && n >= 1 && n < AT_NO_WINDOW, "%s: need window and n in 1 .. 2^30 - 1 (got window=%d, n=%d)",
                what, window, n);
  *capacity = kv_min_capacity(window, n);
  return 0;
}

extern "C" int recnn_kv_append_workspace_bytes(int n_rows, int n, int hidden, int64_t* bytes) {
  const char* what = "kv_append_workspace_bytes";
  RECNN_REQUIRE(bytes, "%s: null pointer", what);
  RECNN_REQUIRE(hidden >= 16 && hidden % 16 == 0 && hidden <= 256, "%s: hidden must be a multiple of 16 up to 256 (got %d)", what, hidden);
  RECNN_REQUIRE(n >= 1 && n_rows >= 0 && n_rows <= 65535 && (int64_t)n_rows * n < (1LL << 31),
                "%s: need n >= 1, n_rows in 0 .. 65535 and n_rows * n < 2^31 (got n_rows=%d, n=%d)", what, n_rows, n);
  *bytes = append_ws(n_rows, n, hidden).total;
  return 0;
}

extern "C" int recnn_attn_append(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_rows,
                                 int n, const float* table, int n_items, int emb_dim, int hidden, int n_heads, int window, int alibi,
                                 const float* w_in, const float* b_in, const float* w_o, const float* b_o, float* kv, int n_sessions,
                                 int capacity, const int32_t* pos, const int32_t* rows, float* h_out, void* workspace, void* stream) {
  const char* what = "attn_append";
  RECNN_REQUIRE(store_ok(items, ratings, user_off, slots, table) && w_in && b_in && w_o && b_o && h_out && workspace, "%s: null pointer", what);
  RECNN_ATTN_DIMS_OK(what, emb_dim, hidden, n_heads);
  RECNN_KV_CACHE_OK(what, n_rows, n, n_sessions, capacity, window, kv, pos, rows);
  RECNN_REQUIRE(n_items > 0, "%s: need n_items > 0", what);
  RECNN_REQUIRE(aligned16(table, w_o, h_out, workspace), "%s: table, w_o, h_out and the workspace must be 16-byte aligned", what);
  if (n_rows == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  const AppendWs w = append_ws(n_rows, n, hidden);
  char* ws = (char*)workspace;
  float* qkv = (float*)(ws + w.qkv);
  float* o = (float*)(ws + w.o);
  LinArgs l{};
  l.s = SeqStore{items, ratings, user_off, slots, n_rows, table, n_items, emb_dim};
  l.t0 = 0; l.T = n; l.rows = n_rows * n;
  l.K = emb_dim; l.w = w_in; l.ldw = emb_dim + 1; l.b = b_in;
  l.out = qkv; l.N = 3 * hidden;
  if (int rc = launch_linear(l, s)) return rc;
  launch_cache_attention(qkv, o, n_rows, n, hidden, n_heads, window, alibi, kv, n_sessions, capacity, pos, rows, s);
  DenseLinArgs p{};
  p.rows = n_rows * n; p.K = hidden; p.N = hidden;
  p.x = o; p.w = w_o; p.ldw = hidden; p.b = b_o;
  p.out = h_out;
  if (int rc = launch_dense_linear(p, false, s)) return rc;
  return recnn_check_hip(hipGetLastError(), what);
}

extern "C" int recnn_attn_train_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int n_heads, int64_t* saved_bytes,
                                                int64_t* bwd_bytes) {
  const char* what = "attn_train_workspace_bytes";
  RECNN_REQUIRE(saved_bytes && bwd_bytes, "%s: null pointer", what);
  RECNN_ATTN_DIMS_OK(what, emb_dim, hidden, n_heads);
  RECNN_ATTN_SIZE_OK(what, n_users, T);
  *saved_bytes = attn_ws(n_users, T, hidden, n_heads).total;
  *bwd_bytes = attn_bwd_ws(n_users, T, hidden, emb_dim, n_heads).total;
  return 0;
}

extern "C" int recnn_attn_encode_train(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                                       int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden, int n_heads,
                                       int window, int alibi, const float* w_in, const float* b_in, const float* w_o, const float* b_o,
                                       float* h_out, void* saved, void* stream) {
  return attn_encode_impl("attn_encode_train", items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, n_heads,
                          window, alibi, w_in, b_in, w_o, b_o, h_out, saved, stream);
}

extern "C" int recnn_attn_backward(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots, int n_users,
                                   int t0, int T, const float* table, int n_items, int emb_dim, int hidden, int n_heads, int window,
                                   int alibi, const float* w_o, const void* saved, const float* g_h, float* d_w_in, float* d_b_in,
                                   float* d_w_o, float* d_b_o, void* workspace, void* stream) {
  return attn_backward_impl(items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, n_heads, window, alibi,
                            nullptr, w_o, saved, g_h, d_w_in, d_b_in, d_w_o, d_b_o, nullptr, false, workspace, nullptr, stream);
}

extern "C" int recnn_attn_table_grad_workspace_bytes(int n_users, int T, int hidden, int emb_dim, int n_items, int64_t* bytes) {
  const char* what = "attn_table_grad_workspace_bytes";
  RECNN_REQUIRE(bytes, "%s: null pointer", what);
  RECNN_LSTM_DIMS_OK(what, emb_dim, hidden);
  RECNN_REQUIRE(n_users >= 0 && T >= 0 && n_items >= 1 && (int64_t)n_users * T < (1LL << 31),
                "%s: need n_users >= 0, T >= 0, n_items >= 1 and n_users * T < 2^31", what);
  *bytes = table_ws(n_users, T, 3 * hidden, emb_dim, n_items).total;
  return 0;
}

extern "C" int recnn_attn_backward_table(const int32_t* items, const float* ratings, const int64_t* user_off, const int32_t* slots,
                                         int n_users, int t0, int T, const float* table, int n_items, int emb_dim, int hidden, int n_heads,
                                         int window, int alibi, const float* w_in, const float* w_o, const void* saved, const float* g_h,
                                         float* d_w_in, float* d_b_in, float* d_w_o, float* d_b_o, float* d_table, void* workspace,
                                         void* table_workspace, void* stream) {
  return attn_backward_impl(items, ratings, user_off, slots, n_users, t0, T, table, n_items, emb_dim, hidden, n_heads, window, alibi, w_in,
                            w_o, saved, g_h, d_w_in, d_b_in, d_w_o, d_b_o, d_table, true, workspace, table_workspace, stream);
}
