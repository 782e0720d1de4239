// gather.hip -- replay sampler + embedding gather (gfx950).
//
// Replaces, bit-exactly, the collate of the reference:
//   recnn/data/utils.py:7-10     rolling_window        (sliding windows of length F+1 per user)
//   recnn/data/utils.py:161-187  prepare_batch_static_size (concatenate windows over users)
//   recnn/data/utils.py:51-81    batch_tensor_embeddings   (emb[items], view, cat, done scatter)
// The [B, F+1] item/rating windows are never materialised: a batch row r is located by a binary
// search over the per-user row prefix sum, and the window is read straight from the CSR store.
//
// HBM-bound copy kernel.  One workgroup builds R consecutive batch rows.  Consecutive rows of one
// user share F of their F+1 embedding rows (sliding window) and state / next_state / action of one
// row share all of them, so each distinct (row, slot) embedding line is fetched ONCE (16-byte coalesced
// loads, (R+F)..R*(F+1) lines of E floats per workgroup) by the threads that own it and stored straight
// to every output that uses it with the widest store the output alignment allows (gather_dev.h).
#include "gather_dev.h"
#include "recnn_hip_debug.h"

// ------------------------------------------------------------------ plan: row prefix sums
__global__ __launch_bounds__(1024) void frame_plan_kernel(const int64_t* __restrict__ user_off,
                                                          const int32_t* __restrict__ users, int n, int frame,
                                                          int32_t* __restrict__ row_off, const int32_t* __restrict__ cursor,
                                                          int cursor_stride) {
  __shared__ int sc[1024];
  __shared__ int carry;
  const int tid = threadIdx.x;
  if (cursor) users += (int64_t)(*cursor) * cursor_stride;  // device-side batch cursor (graph replay)
  if (tid == 0) { carry = 0; row_off[0] = 0; }
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    int i = base + tid;
    int v = 0;
    if (i < n) {
      int u = users[i];
      int len = (int)(user_off[u + 1] - user_off[u]);
      v = max(len - frame, 0);
    }
    sc[tid] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // inclusive Hillis-Steele scan
      int t = tid >= o ? sc[tid - o] : 0;
      __syncthreads();
      sc[tid] += t;
      __syncthreads();
    }
    if (i < n) row_off[i + 1] = carry + sc[tid];
    __syncthreads();
    if (tid == 0) carry += sc[1023];
    __syncthreads();
  }
}

extern "C" int recnn_frame_plan(const int64_t* user_off, const int32_t* batch_users, int n_users, int frame,
                                int32_t* row_off, const int32_t* cursor, int cursor_stride, void* stream) {
  RECNN_REQUIRE(user_off && batch_users && row_off && n_users >= 0 && frame > 0, "frame_plan: bad arguments");
  hipLaunchKernelGGL(frame_plan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, user_off, batch_users, n_users, frame,
                     row_off, cursor, cursor_stride);
  return recnn_check_hip(hipGetLastError(), "frame_plan");
}

// ------------------------------------------------------------------ per-epoch plan table
// One workgroup per batch of the epoch permutation: prefix sums of the batch users' window counts (256 users per pass),
// then every batch row looks itself up once: plan[batch][row] = (CSR offset of the window start << 1) | last-window flag,
// -1 past the batch's last row.  The gather of a step then reaches a row's window with ONE load (GatherArgs.plan).
__global__ __launch_bounds__(256) void frame_plan_rows_kernel(const int64_t* __restrict__ user_off, const int32_t* __restrict__ perm, int n,
                                                              int frame, int rows, int64_t* __restrict__ plan) {
  extern __shared__ __attribute__((aligned(16))) unsigned char plan_smem[];
  long long* s_start = (long long*)plan_smem;      // [n]
  int* s_off = (int*)(s_start + n);                // [n + 1]
  int* sc = s_off + n + 1;                         // [256]
  __shared__ int carry;
  const int tid = threadIdx.x;
  const int32_t* users = perm + (int64_t)blockIdx.x * n;
  if (tid == 0) { carry = 0; s_off[0] = 0; }
  __syncthreads();
  for (int base = 0; base < n; base += 256) {
    const int i = base + tid;
    int v = 0;
    if (i < n) {
      const int u = users[i];
      const long long o0 = user_off[u];
      v = max((int)(user_off[u + 1] - o0) - frame, 0);
      s_start[i] = o0;
    }
    sc[tid] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive Hillis-Steele scan
      const int t = tid >= o ? sc[tid - o] : 0;
      __syncthreads();
      sc[tid] += t;
      __syncthreads();
    }
    if (i < n) s_off[i + 1] = carry + sc[tid];
    __syncthreads();
    if (tid == 0) carry += sc[255];
    __syncthreads();
  }
  const int total = s_off[n];
  int64_t* out = plan + (int64_t)blockIdx.x * rows;
  for (int r = tid; r < rows; r += 256) {
    long long p = -1;
    if (r < total) {
      int lo = 0, hi = n;     // largest i with s_off[i] <= r
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s_off[mid] <= r) lo = mid; else hi = mid;
      }
      const int t = r - s_off[lo];
      p = ((s_start[lo] + t) << 1) | (t == s_off[lo + 1] - s_off[lo] - 1 ? 1 : 0);
    }
    out[r] = p;
  }
}

extern "C" int recnn_frame_plan_rows(const int64_t* user_off, const int32_t* perm, int users_per_batch, int n_batches, int frame, int rows,
                                     int64_t* plan, void* stream) {
  RECNN_REQUIRE(user_off && perm && plan && users_per_batch > 0 && n_batches > 0 && frame > 0 && rows > 0, "frame_plan_rows: bad arguments");
  const size_t lds = (size_t)users_per_batch * 8 + (size_t)(users_per_batch + 1 + 256) * 4;
  RECNN_REQUIRE(lds <= 64 * 1024, "frame_plan_rows: at most ~5000 users per batch (%d given)", users_per_batch);
  hipLaunchKernelGGL(frame_plan_rows_kernel, dim3(n_batches), dim3(256), lds, (hipStream_t)stream, user_off, perm, users_per_batch, frame, rows,
                     plan);
  return recnn_check_hip(hipGetLastError(), "frame_plan_rows");
}

// ------------------------------------------------------------------ dense epoch plan: every window of every user, once
// The reference trains on ALL L - F windows of every user of a batch (recnn/data/utils.py:161-187: rolling_window over each
// user's whole history, concatenated); a fixed-row batch that keeps only the first `rows` rows of its users drops the rest.
// Here the windows of the epoch's user SEQUENCE are concatenated in sequence order and cut into batches of `rows` rows: batch
// b = global rows [b rows, (b + 1) rows), a user's windows continue in the next batch, `done` marks each user's last window
// (utils.py:70-71) wherever it falls.  skip0 = windows of the first sequence entry already consumed by the previous epoch's last
// batch (the leftover of an epoch is carried, so that over consecutive epochs every (user, window) is visited exactly once per
// epoch).  Two launches: prefix sums of the window counts over the sequence, then one thread per plan row.
__global__ __launch_bounds__(1024) void frame_plan_seq_kernel(const int64_t* __restrict__ user_off, const int32_t* __restrict__ seq, int n,
                                                              int frame, int skip0, int32_t* __restrict__ row_off) {
  __shared__ int sc[1024];
  __shared__ int carry;
  const int tid = threadIdx.x;
  if (tid == 0) { carry = 0; row_off[0] = 0; }
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int i = base + tid;
    int v = 0;
    if (i < n) {
      const int u = seq[i];
      v = max((int)(user_off[u + 1] - user_off[u]) - frame - (i == 0 ? skip0 : 0), 0);
    }
    sc[tid] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // inclusive Hillis-Steele scan
      const int t = tid >= o ? sc[tid - o] : 0;
      __syncthreads();
      sc[tid] += t;
      __syncthreads();
    }
    if (i < n) row_off[i + 1] = carry + sc[tid];
    __syncthreads();
    if (tid == 0) carry += sc[1023];
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void frame_plan_dense_kernel(const int64_t* __restrict__ user_off, const int32_t* __restrict__ seq,
                                                               const int32_t* __restrict__ row_off, int n, int frame, int skip0, int rows,
                                                               int64_t n_rows, int64_t* __restrict__ plan) {
  const int total = row_off[n];
  const int64_t usable = (int64_t)(total / rows) * rows;      // whole batches of this epoch
  for (int64_t g0 = (int64_t)blockIdx.x * 256 + threadIdx.x; g0 < n_rows; g0 += (int64_t)gridDim.x * 256) {
    long long p = -1;
    // plan slots past the epoch's last whole batch repeat its first batches: a caller that lets the device cursor run past the
    // epoch (raw recnn_engine_graph_run without the host's epoch logic) reads valid rows, not garbage
    const int64_t g = (g0 < usable || usable == 0) ? g0 : (g0 - usable) % usable;
    if (g < total) {
      int lo = 0, hi = n;               // largest i with row_off[i] <= g   (row_off non-decreasing, row_off[n] > g)
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (row_off[mid] <= g) lo = mid; else hi = mid;
      }
      const int u = seq[lo];
      const long long o0 = user_off[u];
      const int t = (int)(g - row_off[lo]) + (lo == 0 ? skip0 : 0);
      const int last = (int)(user_off[u + 1] - o0) - frame - 1;
      p = ((o0 + t) << 1) | (t == last ? 1 : 0);
    }
    plan[g0] = p;
  }
}

extern "C" int recnn_frame_plan_dense(const int64_t* user_off, const int32_t* seq, int n_seq, int skip0, int frame, int rows,
                                      int32_t* row_off, int64_t n_rows, int64_t* plan, void* stream) {
  RECNN_REQUIRE(user_off && seq && row_off && plan && n_seq > 0 && skip0 >= 0 && frame > 0 && rows > 0 && n_rows > 0, "frame_plan_dense: bad arguments");
  hipLaunchKernelGGL(frame_plan_seq_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, user_off, seq, n_seq, frame, skip0, row_off);
  int grid = (int)((n_rows + 255) / 256);
  if (grid > 16384) grid = 16384;
  hipLaunchKernelGGL(frame_plan_dense_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, user_off, seq, row_off, n_seq, frame, skip0, rows,
                     n_rows, plan);
  return recnn_check_hip(hipGetLastError(), "frame_plan_dense");
}

// ------------------------------------------------------------------ gather
template <int R, int W>
__global__ __launch_bounds__(256) void frame_gather_kernel(const GatherArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  frame_gather_body<R, W>(a, blockIdx.x, smem_raw);
}

// n consecutive batches of the epoch plan in ONE launch (blockIdx.y = batch j: cursor look-ahead + j, outputs j * rows rows
// further down): the batches of a whole policy cycle for the cycle-batched frozen-network forwards (engine.hip).  bf16 rows only.
__global__ __launch_bounds__(256) void frame_gather_multi_kernel(const GatherArgs a0) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  GatherArgs a = a0;
  const int j = blockIdx.y;
  const int64_t r0 = (int64_t)j * a.rows;
  a.cursor_add += j;
  a.state_h += r0 * a.ld_h; a.action_h += r0 * a.ld_h;
  if (a.next_h) a.next_h += r0 * a.ld_h;            // (NULL: no next rows, the next ratings go to tail_n -- gather.h)
  else a.tail_n += r0 * a.ld_tail;
  a.reward += r0; a.done += r0;
  frame_gather_body<4, 4>(a, blockIdx.x, smem_raw);
}

// ------------------------------------------------------------------ cycle gather: long row runs per workgroup
// The body of the cycle launch in the form the engine's window mode runs (bf16 rows from the epoch plan, no next rows: state rows,
// action rows, the next ratings r1..rF into tail_n; gather.h).  R consecutive plan rows of one batch per workgroup: a user's run of
// n windows owns n + F distinct embedding lines, so a long run reads each line ONCE per workgroup (R = 4: 3.5 lines per row,
// R = 32: 1.3) and stores it to every (row, slot) of the run that holds it -- up to F state slots and the action row.  Wave 0 reads
// the R plan entries and lists the distinct lines in LDS (CSR offset of the item; first row, first slot, rows of the run that follow);
// after ONE barrier every thread takes 8 fp32 of a line, rounds them as the generic body does (pack_bf2) and writes 16 bytes per
// destination; the last wave writes each row's ratings, reward and done from one lane.
// Measured on the ten-batch launch (profiles/NOTES_gather_cycle.md): R = 8 / 16 / 32 with 16-byte stores 18.4 / 15.4 / 14.3 us, with
// 8-byte stores 18.1 / 15.5 / 17.4, the generic body 26.3 -- 32 rows and 16-byte stores stayed, the rest is gone.
constexpr int GC_MAXF1 = 16;                     // frame + 1 <= 16: a row's ratings live in one lane's registers
constexpr int GC_ROWS = 32;                      // rows per workgroup
constexpr int GC_CHUNK = 8;                      // floats per chunk of a line: one 16-byte bf16 store per destination

// n bf16 roundings of v[OFF ..] to d, by the widest stores d's alignment allows (the same bits as n f2bf stores)
template <int OFF>
__device__ __forceinline__ void store_bf_run(bf16_t* d, const float (&v)[GC_MAXF1 + 4], const int n) {
  const uintptr_t al = (uintptr_t)d;
#pragma unroll
  for (int k = 0; k < GC_MAXF1; k += 4) {
    if (!(al & 7) && k + 4 <= n) {
      *(uint2*)(d + k) = make_uint2(pack_bf2(v[OFF + k], v[OFF + k + 1]), pack_bf2(v[OFF + k + 2], v[OFF + k + 3]));
    } else {
#pragma unroll
      for (int h = k; h < k + 4; h += 2) {
        if (!(al & 3) && h + 2 <= n) {
          *(uint32_t*)(d + h) = pack_bf2(v[OFF + h], v[OFF + h + 1]);
        } else {
          if (h < n) d[h] = f2bf(v[OFF + h]);
          if (h + 1 < n) d[h + 1] = f2bf(v[OFF + h + 1]);
        }
      }
    }
  }
}

static size_t gather_runs_lds_bytes(const GatherArgs& a, int R) {
  return (size_t)R * 8 + (size_t)R * (a.frame + 1) * (8 + 4) + 16;     // worst case: every row a user's only window
}

template <int R>
__global__ __launch_bounds__(256) void frame_gather_multi_kernel_runs(const GatherArgs a) {
  static_assert(R <= 32, "wave 0 lists the lines with one row per lane and room to shift; the row index takes 8 bits of the line word");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int F = a.frame, E = a.emb, F1 = F + 1;
  long long* s_plan = (long long*)smem_raw;      // [R] the rows' plan entries
  long long* s_off = s_plan + R;                 // [R * F1] per distinct line: CSR offset of its item
  int* s_meta = (int*)(s_off + R * F1);          // [R * F1] first row | first slot << 8 | rows of the run after it << 16
  int* s_total = s_meta + R * F1;                // distinct lines of the workgroup
  const int tid = threadIdx.x, set = blockIdx.y, row0 = blockIdx.x * R;

  if (tid < 64) {
    int cur = 0;
    if (a.cursor) {
      cur = *a.cursor + a.cursor_add + set;
      if (a.cursor_mod > 0 && cur >= a.cursor_mod) cur -= a.cursor_mod;
    }
    const int r = tid;
    long long p = -1;
    if (r < R && row0 + r < a.rows) p = a.plan[(int64_t)cur * a.plan_stride + row0 + r];
    const bool valid = p >= 0;
    const long long src = p >> 1;
    // a run: consecutive windows of one user -- the previous row is valid, not the user's last, and one item earlier
    const long long psrc = __shfl_up(src, 1, 64);
    const int pgo = __shfl_up(valid && !(p & 1) ? 1 : 0, 1, 64);
    const bool cont = r > 0 && valid && pgo && src == psrc + 1;
    const int cnt = valid ? (cont ? 1 : F1) : 0;
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (r >= o) incl += t;
    }
    const int base = incl - cnt;
    const unsigned long long cm = __ballot(cont);
    const int follow = __builtin_ctzll(~((cm >> r) >> 1));       // rows after r that continue its run (rows >= R never do)
    if (r < R) {
      s_plan[r] = p;
      for (int i = 0; i < cnt; ++i) {
        const int j = cont ? F : i;
        s_off[base + i] = src + j;
        s_meta[base + i] = r | (j << 8) | (follow << 16);
      }
    }
    if (r == 63) *s_total = incl;
  }
  __syncthreads();

  const int64_t out0 = (int64_t)set * a.rows + row0;           // batch `set` lands set * rows rows below the given outputs
  const int FE = F * E;
  if (tid >= 192 && tid - 192 < R) {
    const int r = tid - 192;
    const long long p = s_plan[r];
    if (p >= 0) {
      const long long src = p >> 1;
      const int64_t row = out0 + r;
      float rt[GC_MAXF1 + 4];
#pragma unroll
      for (int k = 0; k < GC_MAXF1 + 4; ++k) rt[k] = k < F1 ? a.ratings[src + k] : 0.f;
      float rew = 0.f;
#pragma unroll
      for (int k = 1; k < GC_MAXF1; ++k) rew = k == F ? rt[k] : rew;
      a.reward[row] = rew;
      a.done[row] = (p & 1) ? 1.f : 0.f;
      store_bf_run<0>(a.state_h + row * a.ld_h + FE, rt, F);
      store_bf_run<1>(a.tail_n + row * a.ld_tail, rt, F);
    }
  }

  // ---- embedding lines: chunk c (GC_CHUNK floats) of line l; U chunks per thread in flight (ids, then lines, then stores)
  constexpr int U = 4;
  const int total = *s_total;
  const int EC = E / GC_CHUNK, dl = 256 / EC, dc = 256 - dl * EC;
  int l = tid / EC, c = tid - l * EC;
  bf16_t* const st = a.state_h + out0 * a.ld_h;
  bf16_t* const ac = a.action_h + out0 * a.ld_h;
  const int64_t back = a.ld_h - E;                              // one row down, one slot back
  while (l < total) {
    int m[U], ee[U], item[U];
    float4 v[U], w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      m[u] = -1;
      if (l < total) {
        m[u] = s_meta[l];
        ee[u] = c * GC_CHUNK;
        item[u] = a.items[s_off[l]];
      }
      l += dl; c += dc;
      if (c >= EC) { c -= EC; ++l; }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (m[u] >= 0) {
        const float* t = a.table + (int64_t)item[u] * E + ee[u];
        v[u] = *(const float4*)t;
        w[u] = *(const float4*)(t + 4);
      }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (m[u] < 0) continue;
      const int r = m[u] & 255, j = (m[u] >> 8) & 255, follow = m[u] >> 16;
      const int n = min(follow, j) + 1;                          // row r + k holds the line in slot j - k
      const uint4 h = make_uint4(pack_bf2(v[u].x, v[u].y), pack_bf2(v[u].z, v[u].w), pack_bf2(w[u].x, w[u].y), pack_bf2(w[u].z, w[u].w));
      int k = 0;
      if (j == F) {                                              // the row's action; the rows after it hold it as state
        *(uint4*)(ac + r * a.ld_h + ee[u]) = h;
        k = 1;
      }
      bf16_t* d = st + (r + k) * a.ld_h + (j - k) * E + ee[u];
      for (; k < n; ++k, d += back) *(uint4*)d = h;
    }
  }
}

// what frame_gather_multi_kernel_runs covers (everything else: the generic body, frame_gather_multi_kernel)
static bool gather_runs_ok(const GatherArgs& a, int R) {
  const auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  return a.plan && a.state_h && a.action_h && !a.state && !a.x3 && !a.next_h && a.tail_n && a.frame + 1 <= GC_MAXF1 && a.emb % GC_CHUNK == 0 &&
         al16(a.state_h) && al16(a.action_h) && (a.ld_h * 2) % 16 == 0 && gather_runs_lds_bytes(a, R) <= 48 * 1024;
}

template <int R> static int launch_gather_runs(const GatherArgs& a, int n_sets, hipStream_t s) {
  hipLaunchKernelGGL((frame_gather_multi_kernel_runs<R>), dim3((a.rows + R - 1) / R, n_sets), dim3(256), gather_runs_lds_bytes(a, R), s, a);
  return recnn_check_hip(hipGetLastError(), "frame_gather_multi (runs)");
}

int frame_gather_multi_launch(const GatherArgs& a, int n_sets, hipStream_t s, int cycle_body) {
  const size_t lds = frame_gather_lds_bytes(a, 4);
  if (lds > 48 * 1024 || !a.state_h || a.state || (a.emb % 4) || a.rows <= 0 || n_sets <= 0 || n_sets > 65535) {
    recnn_set_error("frame_gather_multi: needs the bf16-only gather with a tile that fits 48 KB of LDS");
    return RECNN_E_UNSUPPORTED;
  }
  if (!a.next_h && (!a.tail_n || a.x3 || a.ld_tail < a.frame)) {
    recnn_set_error("frame_gather_multi: without next rows the next ratings need a bf16 array of at least `frame` columns");
    return RECNN_E_INVALID;
  }
  if (cycle_body && gather_runs_ok(a, GC_ROWS)) return launch_gather_runs<GC_ROWS>(a, n_sets, s);
  hipLaunchKernelGGL(frame_gather_multi_kernel, dim3((a.rows + 3) / 4, n_sets), dim3(256), lds, s, a);
  return recnn_check_hip(hipGetLastError(), "frame_gather_multi");
}

// The cycle gather on caller-supplied device buffers (csrc/recnn_hip_debug.h): shapes and alignments out of the engine's reach.
extern "C" int recnn_debug_gather_cycle(const recnn_debug_gather_cycle_args* d, int64_t sizeof_args, void* stream) {
  RECNN_REQUIRE(d && sizeof_args == (int64_t)sizeof(*d), "debug_gather_cycle: null pointer or another layout of the argument block");
  RECNN_REQUIRE(d->items && d->ratings && d->table && d->plan && d->state_h && d->action_h && d->reward && d->done, "debug_gather_cycle: null pointer");
  RECNN_REQUIRE(d->rows > 0 && d->frame > 0 && d->emb > 0 && d->plan_stride >= d->rows, "debug_gather_cycle: bad sizes");
  RECNN_REQUIRE(((uintptr_t)d->table & 15) == 0 && ((uintptr_t)d->state_h & 7) == 0 && ((uintptr_t)d->action_h & 7) == 0 && (d->ld_h * 2) % 8 == 0 &&
                (!d->next_h || ((uintptr_t)d->next_h & 7) == 0), "debug_gather_cycle: the table needs 16-byte, the rows 8-byte alignment");
  GatherArgs a;
  memset(&a, 0, sizeof(a));
  a.items = d->items; a.ratings = d->ratings; a.table = d->table;
  a.plan = d->plan; a.plan_stride = d->plan_stride;
  a.cursor = d->cursor; a.cursor_add = d->cursor_add; a.cursor_mod = d->cursor_mod;
  a.rows = d->rows; a.frame = d->frame; a.emb = d->emb;
  a.state_h = (bf16_t*)d->state_h; a.action_h = (bf16_t*)d->action_h; a.next_h = (bf16_t*)d->next_h; a.ld_h = d->ld_h;
  a.tail_n = (bf16_t*)d->tail_n; a.ld_tail = d->ld_tail;
  a.reward = d->reward; a.done = d->done;
  return frame_gather_multi_launch(a, d->n_sets, (hipStream_t)stream, d->gather_cycle);
}

size_t frame_gather_lds_bytes(const GatherArgs& a, int R) {
  const int F1 = a.frame + 1;
  (void)F1;
  size_t lds = (size_t)R * 8 + (size_t)R * 4 + 16;      // per-row window offsets and flags (no line staging since round 2)
  if (a.inline_plan && !a.plan) lds += (size_t)a.n_users * 8 + (size_t)(a.n_users + 1 + 4) * 4;
  return lds;
}

template <int R> static int launch_gather(const GatherArgs& a, int W, hipStream_t s) {
  const size_t lds = frame_gather_lds_bytes(a, R);
  if (lds > 160 * 1024) { recnn_set_error("frame_gather: tile does not fit LDS (%zu bytes)", lds); return RECNN_E_UNSUPPORTED; }
  dim3 grid((a.rows + R - 1) / R), block(256);
  hipError_t e = hipSuccess;
  if (W == 4) {
    if (lds > 48 * 1024) e = hipFuncSetAttribute((const void*)frame_gather_kernel<R, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) hipLaunchKernelGGL((frame_gather_kernel<R, 4>), grid, block, lds, s, a);
  } else if (W == 2) {
    if (lds > 48 * 1024) e = hipFuncSetAttribute((const void*)frame_gather_kernel<R, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) hipLaunchKernelGGL((frame_gather_kernel<R, 2>), grid, block, lds, s, a);
  } else {
    if (lds > 48 * 1024) e = hipFuncSetAttribute((const void*)frame_gather_kernel<R, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) hipLaunchKernelGGL((frame_gather_kernel<R, 1>), grid, block, lds, s, a);
  }
  if (e != hipSuccess) return recnn_check_hip(e, "frame_gather attr");
  return recnn_check_hip(hipGetLastError(), "frame_gather");
}


extern "C" int recnn_frame_gather(const int32_t* items, const float* ratings, const int64_t* user_off,
                                  const int32_t* batch_users, const int32_t* row_off, int n_users, int rows, int frame,
                                  int emb_dim, const float* table, float* state, int64_t ld_state, float* next_state,
                                  int64_t ld_next, float* action, int64_t ld_action, float* reward, float* done,
                                  const int32_t* cursor, int cursor_stride, void* stream) {
  RECNN_REQUIRE(items && ratings && user_off && batch_users && table, "frame_gather: null input");
  RECNN_REQUIRE(row_off || n_users <= 1024, "frame_gather: more than 1024 users per batch need a recnn_frame_plan row_off");
  RECNN_REQUIRE(state && next_state && action && reward && done, "frame_gather: null output");
  RECNN_REQUIRE(frame > 0 && emb_dim > 0 && (emb_dim % 4) == 0, "frame_gather: emb_dim must be a positive multiple of 4");
  RECNN_REQUIRE(((uintptr_t)table & 15) == 0, "frame_gather: table must be 16-byte aligned");
  RECNN_REQUIRE(n_users >= 0 && rows >= 0, "frame_gather: negative sizes");
  if (rows == 0) return 0;
  RECNN_REQUIRE(n_users > 0, "frame_gather: rows requested from an empty user list");
  GatherArgs a;
  memset(&a, 0, sizeof(a));
  a.items = items; a.ratings = ratings; a.user_off = user_off; a.users = batch_users; a.row_off = row_off;
  a.n_users = n_users; a.rows = rows; a.frame = frame; a.emb = emb_dim; a.table = table;
  a.state = state; a.ld_state = ld_state; a.next_state = next_state; a.ld_next = ld_next;
  a.action = action; a.ld_action = ld_action; a.reward = reward; a.done = done;
  a.cursor = cursor; a.cursor_stride = cursor_stride;
  a.inline_plan = row_off == nullptr;
  return frame_gather_launch(a, (hipStream_t)stream);
}

int frame_gather_launch(GatherArgs a, hipStream_t stream) {
  float* state = a.state; float* next_state = a.next_state; float* action = a.action;
  const int64_t ld_state = a.ld_state, ld_next = a.ld_next, ld_action = a.ld_action;
  const int emb_dim = a.emb;
  // widest store every output row start supports
  auto al = [](const void* p, int64_t ld) {
    uintptr_t x = (uintptr_t)p | (uintptr_t)(ld * 4);
    return (x & 15) == 0 ? 4 : ((x & 7) == 0 ? 2 : 1);
  };
  int W = 4;
  if (state) {  // fp32 rows may be omitted (bf16 twins only) by the engine's own sampler
    W = al(state, ld_state);
    int w2 = al(next_state, ld_next); if (w2 < W) W = w2;
    int w3 = al(action, ld_action); if (w3 < W) W = w3;
  } else if (!a.state_h) {
    recnn_set_error("frame_gather: no output rows");
    return RECNN_E_INVALID;
  }
  if (emb_dim % W) W = 1;
  if (a.state_h && !a.next_h) { recnn_set_error("frame_gather: the per-batch gather writes next rows"); return RECNN_E_INVALID; }
  if (a.state_h && W != 4) { recnn_set_error("frame_gather: bf16 twin rows need 16-byte aligned fp32 rows"); return RECNN_E_INVALID; }
  // (4 rows per workgroup: 2 and 8 were measured in round 2 -- 7.0 / 9.6 us against 7.2 -- and are gone)
  return launch_gather<4>(a, W, stream);
}

// ------------------------------------------------------------------ pack a canonical batch
__global__ __launch_bounds__(256) void pack_batch_kernel(const float* __restrict__ state, int64_t ld_state,
                                                         const float* __restrict__ action, int64_t ld_action,
                                                         const float* __restrict__ next_state, int64_t ld_next, int rows, int S,
                                                         int A, float* __restrict__ xs, float* __restrict__ xn, int64_t ld_x) {
  const int r = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;  // column in the packed row
  if (r >= rows || c >= A + S) return;
  if (c < A) {
    xs[(int64_t)r * ld_x + c] = action[(int64_t)r * ld_action + c];
  } else {
    xs[(int64_t)r * ld_x + c] = state[(int64_t)r * ld_state + (c - A)];
    xn[(int64_t)r * ld_x + c] = next_state[(int64_t)r * ld_next + (c - A)];
  }
}

extern "C" int recnn_pack_batch(const float* state, int64_t ld_state, const float* action, int64_t ld_action,
                                const float* next_state, int64_t ld_next, int rows, int state_dim, int action_dim, float* xs,
                                float* xn, int64_t ld_x, void* stream) {
  RECNN_REQUIRE(state && action && next_state && xs && xn, "pack_batch: null pointer");
  RECNN_REQUIRE(rows >= 0 && state_dim > 0 && action_dim > 0 && ld_x >= state_dim + action_dim, "pack_batch: bad sizes");
  if (rows == 0) return 0;
  dim3 grid((state_dim + action_dim + 255) / 256, rows), block(256);
  hipLaunchKernelGGL(pack_batch_kernel, grid, block, 0, (hipStream_t)stream, state, ld_state, action, ld_action, next_state,
                     ld_next, rows, state_dim, action_dim, xs, xn, ld_x);
  return recnn_check_hip(hipGetLastError(), "pack_batch");
}

// ------------------------------------------------------------------ packed fp32 rows -> bf16 twins
// (engine, bf16 mode, batch not produced by the engine's own sampler): one pass over xs and xn.
__global__ __launch_bounds__(256) void rows_to_bf16_kernel(const float* __restrict__ xs, const float* __restrict__ xn,
                                                           bf16_t* __restrict__ hs, bf16_t* __restrict__ hn, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 a = ((const float4*)xs)[i], b = ((const float4*)xn)[i];
    ((uint2*)hs)[i] = make_uint2(pack_bf2(a.x, a.y), pack_bf2(a.z, a.w));
    ((uint2*)hn)[i] = make_uint2(pack_bf2(b.x, b.y), pack_bf2(b.z, b.w));
  }
}
int rows_to_bf16_launch(const float* xs, const float* xn, bf16_t* hs, bf16_t* hn, int rows, int64_t ld, hipStream_t s) {
  const int64_t n4 = (int64_t)rows * ld / 4;
  if (n4 <= 0) return 0;
  int grid = (int)((n4 + 255) / 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(rows_to_bf16_kernel, dim3(grid), dim3(256), 0, s, xs, xn, hs, hn, n4);
  return recnn_check_hip(hipGetLastError(), "rows_to_bf16_kernel");
}
