// slate.hip -- a candidate slate diversified on the GPU (gfx950): the similarity matrix of a row's candidates, the greedy maximal-
// marginal-relevance pick over it (Carbonell & Goldstein 1998) and the slate's intra-list distance, one launch each.  DESIGN.md
// section 25.
//
//   X [K <= 64][128] = table[ids[b, :]] (a slot whose id is outside [0, N) is empty: it reads nothing),  G = X X^T,  n_i = G_ii
//   IP   S_ij = G_ij          COS  S_ij = G_ij / (sqrt(n_i) sqrt(n_j)), 0 where a norm is 0          L2  S_ij = -max((n_i + n_j) - 2 G_ij, 0)
//   entries of an empty slot are 0.
//
// One workgroup of four waves owns a row.  Its K table rows go to LDS (register-staged, 16 bytes per lane, all of a thread's loads
// in flight together) at a stride of 136 floats: the fragment read below -- lane (fr, fg) takes the 16 bytes at [16 T + fr][k0 + 4 fg]
// -- then touches sixteen different 4-bank slots in each of ds_read_b128's lane groups.  G is cut into 16 x 16 tiles, one accumulator
// each, v_mfma_f32_16x16x4_f32 with both operands from that LDS image; a tile and its mirror image are computed once (ten tiles
// at K = 64, two or three per wave) and stored to both places.
//
// Bits: G_ij is one fmaf chain from +0 over the products x_i[k] x_j[k] in the order k0 = 0, 16, .., 112; e = 0..3; fg = 0..3 at
// k = k0 + 4 fg + e -- fixed by the instruction sequence, the same for every tile of every wave, and no function of B, K or the slot.
// Which of (i, j) and (j, i) a wave computes changes nothing: the chain of G_ji has the commuted products in the same order, and
// every step from G to S is a correctly rounded operation that commutes in (i, j); the other one is a copy.  n_i is the diagonal of
// the same chain.  So S is bitwise symmetric and S_ij depends on the two table rows alone.
//
// S takes the place of X in LDS (every wave is past its last fragment read at the barrier before the first S store), so a workgroup
// holds 35 KB and four of them share a CU.
//
// Selection (rerank): after one barrier wave 0 runs the k steps with lane = slot: the order of slot_before as one 64-bit key
// (slot_key, select_dev.h), its wave maximum over DPP row operations, the smallest slot among the lanes that hold it, then one LDS row
// read of S (row s = column s) to update m_j = max over the chosen s of S_js.  No atomics, no workspace.
#include "common.h"
#include "select_dev.h"   // slot_key: slot_before's order as a key; no floating-point arithmetic in it

// Every value below is stated operation by operation, each one correctly rounded: nothing may fuse.  Plain operators, not HIP's
// __fmul_rn / __fsub_rn: those are header functions compiled with contraction allowed, and once inlined a product and the difference
// that takes it do fuse.  Under the compiler's defaults `/` and sqrtf are the correctly rounded quotient and root.
#pragma clang fp contract(off)

namespace {
constexpr int SL_E = 128;        // embedding width
constexpr int SL_SLOTS = 64;     // largest K
constexpr int SL_XP = SL_E + 8;  // floats per LDS row of X
constexpr int SL_SP = SL_SLOTS + 4;   // floats per LDS row of S
constexpr int SL_MAX_ROWS = 1 << 20;  // rows per launch (256 threads each: the grid stays below 2^32 threads)
enum { SL_IP = 0, SL_L2 = 1, SL_COS = 2 };
enum Mode { M_SIM, M_PICK, M_ILD };

struct SlateArgs {
  const float* table; int N;
  const void* ids; int64_t ld_ids; int K; int ids64;
  int kind; int64_t row0;
  float* sim;                                                   // M_SIM: [B][K][K]
  const float* rel; int64_t ld_rel; float lam, mu; int normalize; int k_out;   // M_PICK
  float* out_score; int64_t* out_ids; int32_t* out_slot;        // [B][k_out]
  double* ild;                                                  // M_ILD: [B]
};

// ai, aj: what norm_term() made of n_i and n_j
__device__ inline float norm_term(int kind, float n) { return kind == SL_COS ? sqrtf(n) : n; }      // sqrt(n) == 0 exactly when n == 0
__device__ inline float sim_value(int kind, float g, float ai, float aj) {
  if (kind == SL_IP) return g;
  if (kind == SL_COS) return (ai == 0.f || aj == 0.f) ? 0.f : g / (ai * aj);
  return 0.f - fmaxf((ai + aj) - 2.f * g, 0.f);     // 0 - x: a zero distance is +0
}

// the largest key of the wave, in every lane: DPP row operations, a lane without a source takes 0 (below every key)
template <int CTRL, int ROW_MASK = 0xF> __device__ inline uint64_t dpp_take64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROW_MASK, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROW_MASK, 0xF, false);
  return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t max_u64(uint64_t x, uint64_t y) { return x > y ? x : y; }
__device__ inline uint64_t wave_max_u64(uint64_t v) {
  v = max_u64(v, dpp_take64<0xB1>(v));         // quad_perm [1,0,3,2]
  v = max_u64(v, dpp_take64<0x4E>(v));         // quad_perm [2,3,0,1]
  v = max_u64(v, dpp_take64<0x141>(v));        // row_half_mirror
  v = max_u64(v, dpp_take64<0x140>(v));        // row_mirror: every lane of a 16-lane row holds the row's
  v = max_u64(v, dpp_take64<0x142, 0xA>(v));   // row_bcast15 into rows 1 and 3
  v = max_u64(v, dpp_take64<0x143, 0xC>(v));   // row_bcast31 into rows 2 and 3: lane 63 holds the wave's
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
  return ((uint64_t)hi << 32) | lo;
}

__device__ inline float dist_value(int kind, float s) {
  if (kind == SL_COS) return 1.f - s;
  if (kind == SL_L2) return sqrtf(-s);
  return -s;
}

template <int MODE>
__global__ __launch_bounds__(256) void slate_kernel(const SlateArgs a) {
  __shared__ __attribute__((aligned(16))) float Xs[SL_SLOTS * SL_XP];
  float* Ss = Xs;                          // [SL_SLOTS][SL_SP], once X has been read
  static_assert(SL_SP <= SL_XP, "S takes X's place");
  __shared__ float Ns[SL_SLOTS];           // norm_term(n_i)
  __shared__ int Is[SL_SLOTS];             // the id of a slot, -1 for an empty one (and for the slots past K)
  __shared__ double Rd[4];
  __shared__ int Rc[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int64_t b = a.row0 + blockIdx.x;
  const int K = a.K, K16 = (K + 15) & ~15, T = K16 >> 4;

  // ---- gather: thread (r0, k4) takes the 16 bytes at column 4 k4 of rows r0, r0 + 8, ..
  {
    const int k4 = tid & 31, r0 = tid >> 5;
    f32x4 v[SL_SLOTS / 8];
#pragma unroll
    for (int i = 0; i < SL_SLOTS / 8; ++i) {
      const int row = r0 + 8 * i;
      int64_t id = -1;
      if (row < K) {
        const int64_t o = b * a.ld_ids + row;
        id = a.ids64 ? ((const int64_t*)a.ids)[o] : (int64_t)((const int32_t*)a.ids)[o];
      }
      const bool ok = (uint64_t)id < (uint64_t)a.N;
      v[i] = ok ? *(const f32x4*)(a.table + id * SL_E + k4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
      if (k4 == 0) Is[row] = ok ? (int)id : -1;
    }
#pragma unroll
    for (int i = 0; i < SL_SLOTS / 8; ++i) {
      const int row = r0 + 8 * i;
      if (row < K16) *(f32x4*)&Xs[row * SL_XP + k4 * 4] = v[i];
    }
  }
  __syncthreads();

  // ---- G: its T x T tiles of 16 x 16 are symmetric, so each unordered pair {I, J} is computed once: wave w takes (w, w), (w, w + 1)
  // and, for w < 2, (w, w + 2), tile indices mod 4 -- ten tiles at T = 4, three on the longest wave.  acc[s][r] = G[16 w + 4 fg + r][16 J_s + fr]
  f32x4 acc[3];
  int Js[3];
  bool on[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    Js[s] = (wave + s) & 3;
    on[s] = wave < T && Js[s] < T && (s < 2 || wave < 2);      // wave-uniform
  }
  if (on[0]) {
    const float* xa = Xs + (wave * 16 + fr) * SL_XP + fg * 4;
    const float* xb = Xs + fr * SL_XP + fg * 4;
#pragma unroll 2
    for (int k0 = 0; k0 < SL_E; k0 += 16) {
      const f32x4 av = *(const f32x4*)(xa + k0);
      f32x4 bv[3];
#pragma unroll
      for (int s = 0; s < 3; ++s)
        if (on[s]) bv[s] = *(const f32x4*)(xb + Js[s] * 16 * SL_XP + k0);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int s = 0; s < 3; ++s)
          if (on[s]) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[s][e], acc[s], 0, 0, 0);
    }
    // the diagonal: lane (fr, fg = fr / 4) holds G_ii of row i = 16 w + fr in register fr % 4 of the tile (w, w)
    if (fg == (fr >> 2)) {
      float n = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r == (fr & 3)) n = acc[0][r];
      Ns[wave * 16 + fr] = norm_term(a.kind, n);
    }
  }
  __syncthreads();                          // the norms are complete, and no wave reads X any more
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    if (!on[s]) continue;
    const int j = Js[s] * 16 + fr;
    const float nj = Ns[j];
    const bool okj = Is[j] >= 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = wave * 16 + fg * 4 + r;
      const float v = (okj && Is[i] >= 0) ? sim_value(a.kind, acc[s][r], Ns[i], nj) : 0.f;
      Ss[i * SL_SP + j] = v;
      if (s > 0) Ss[j * SL_SP + i] = v;     // the mirrored tile
    }
  }
  __syncthreads();

  if constexpr (MODE == M_SIM) {
    float* out = a.sim + b * K * K;
    for (int c = tid; c < K * K; c += 256) {
      const int i = c / K, j = c - i * K;
      out[c] = Ss[i * SL_SP + j];
    }
  } else if constexpr (MODE == M_ILD) {
    double sum = 0.0;
    int cnt = 0;
    for (int c = tid; c < K * K; c += 256) {
      const int i = c / K, j = c - i * K;
      if (i < j && Is[i] >= 0 && Is[j] >= 0) {
        sum += (double)dist_value(a.kind, Ss[i * SL_SP + j]);
        ++cnt;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sum += __shfl_xor(sum, o, 64);
      cnt += __shfl_xor(cnt, o, 64);
    }
    if (lane == 0) { Rd[wave] = sum; Rc[wave] = cnt; }
    __syncthreads();
    if (tid == 0) {
      const int pairs = (Rc[0] + Rc[1]) + (Rc[2] + Rc[3]);
      a.ild[b] = pairs ? ((Rd[0] + Rd[1]) + (Rd[2] + Rd[3])) / (double)pairs : __builtin_nan("");
    }
  } else {
    if (wave != 0) return;
    // ---- lane = slot
    int cid = Is[lane];                     // the slot's id while it can still be chosen, -1 afterwards (and for an empty slot)
    float r = 0.f;
    if (cid >= 0) r = a.rel[b * a.ld_rel + lane];
    if (a.normalize) {
      const bool fin = cid >= 0 && __builtin_isfinite(r);
      float mn = fin ? r : INFINITY, mx = fin ? r : -INFINITY;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      }
      mn = mn + 0.f;             // one zero: a minimum of -0 and +0 is +0 whichever the reduction met first
      mx = mx + 0.f;
      if (fin) r = mx == mn ? 0.f : (r - mn) / (mx - mn);
    }
    const float lr = a.lam * r;
    float m = 0.f;
    float* os = a.out_score + b * a.k_out;
    int64_t* oi = a.out_ids + b * a.k_out;
    int32_t* ol = a.out_slot + b * a.k_out;
    int t = 0;
    for (; t < a.k_out; ++t) {
      const float q = t == 0 ? lr : lr - a.mu * m;
      const uint64_t key = slot_key(q, cid);
      const uint64_t best = wave_max_u64(key);
      if (best == 0) break;                 // every slot left is empty or chosen
      const int bs = __ffsll((long long)__ballot(key == best)) - 1;      // equal keys: the smaller slot
      const float bq = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, q), bs));
      const int bi = 0x7FFFFFFF - (int)(uint32_t)best;
      if (lane == 0) { os[t] = bq; oi[t] = bi; ol[t] = bs; }
      if (lane == bs) cid = -1;
      const float s = lane < K ? Ss[bs * SL_SP + lane] : 0.f;     // row s of S = its column s, bit for bit
      m = (t == 0 || s > m) ? s : m;
    }
    if (lane == 0)
      for (; t < a.k_out; ++t) { os[t] = -INFINITY; oi[t] = -1; ol[t] = -1; }
  }
}

template <int MODE> int launch_slate(SlateArgs a, int64_t B, hipStream_t st) {
  for (int64_t r0 = 0; r0 < B; r0 += SL_MAX_ROWS) {
    a.row0 = r0;
    const int64_t rows = B - r0 < SL_MAX_ROWS ? B - r0 : SL_MAX_ROWS;
    hipLaunchKernelGGL((slate_kernel<MODE>), dim3((unsigned)rows), dim3(256), 0, st, a);
    if (int rc = recnn_check_hip(hipGetLastError(), "slate_kernel")) return rc;
  }
  return 0;
}

int slate_check(const char* fn, const float* table, int n_items, const void* ids, int64_t ld_ids, int n_rows, int n_cand,
                int ids_are_int64, int kind, SlateArgs* a) {
  RECNN_REQUIRE(table && (ids || n_rows == 0), "%s: null pointer", fn);
  RECNN_REQUIRE(n_rows >= 0 && n_items > 0, "%s: need n_rows >= 0 and n_items > 0", fn);
  RECNN_REQUIRE(n_cand >= 1 && n_cand <= SL_SLOTS, "%s: n_candidates must be from 1 to %d (got %d)", fn, SL_SLOTS, n_cand);
  RECNN_REQUIRE(kind == SL_IP || kind == SL_L2 || kind == SL_COS, "%s: kind must be 0 (IP), 1 (L2) or 2 (COS), got %d", fn, kind);
  RECNN_REQUIRE(aligned16(table), "%s: table must be 16-byte aligned", fn);
  RECNN_REQUIRE(ids_are_int64 == 0 || ids_are_int64 == 1, "%s: ids_are_int64 must be 0 (int32) or 1 (int64)", fn);
  RECNN_REQUIRE(((uintptr_t)ids & (ids_are_int64 ? 7 : 3)) == 0 && (ld_ids >= n_cand || n_rows <= 1),
                "%s: ids must be aligned to their element with a row stride ld_ids of at least n_candidates", fn);
  *a = SlateArgs{};
  a->table = table; a->N = n_items; a->ids = ids; a->ld_ids = ld_ids; a->K = n_cand; a->ids64 = ids_are_int64; a->kind = kind;
  return 0;
}
}  // namespace

extern "C" int recnn_slate_similarity(const float* table, int n_items, const void* ids, int64_t ld_ids, int n_rows, int n_candidates,
                                      int ids_are_int64, int kind, float* out, void* stream) {
  SlateArgs a;
  if (int rc = slate_check("slate_similarity", table, n_items, ids, ld_ids, n_rows, n_candidates, ids_are_int64, kind, &a)) return rc;
  RECNN_REQUIRE((out && ((uintptr_t)out & 3) == 0) || n_rows == 0, "slate_similarity: out is null or misaligned");
  if (n_rows == 0) return 0;
  a.sim = out;
  return launch_slate<M_SIM>(a, n_rows, (hipStream_t)stream);
}

extern "C" int recnn_slate_rerank(const float* table, int n_items, const void* ids, int64_t ld_ids, int n_rows, int n_candidates,
                                  int ids_are_int64, int kind, const float* rel, int64_t ld_rel, float lam, int normalize, int k,
                                  float* out_score, int64_t* out_ids, int32_t* out_slot, void* stream) {
  SlateArgs a;
  if (int rc = slate_check("slate_rerank", table, n_items, ids, ld_ids, n_rows, n_candidates, ids_are_int64, kind, &a)) return rc;
  RECNN_REQUIRE(k >= 1 && k <= n_candidates, "slate_rerank: need 1 <= k <= n_candidates (got k = %d, n_candidates = %d)", k, n_candidates);
  RECNN_REQUIRE(lam >= 0.f && lam <= 1.f, "slate_rerank: lam must be in [0, 1] (got %g)", (double)lam);
  RECNN_REQUIRE(normalize == 0 || normalize == 1, "slate_rerank: normalize must be 0 or 1");
  RECNN_REQUIRE((rel && out_score && out_ids && out_slot) || n_rows == 0, "slate_rerank: null pointer");
  RECNN_REQUIRE(((uintptr_t)rel & 3) == 0 && (ld_rel >= n_candidates || n_rows <= 1),
                "slate_rerank: rel must be 4-byte aligned with a row stride ld_rel of at least n_candidates");
  if (n_rows == 0) return 0;
  a.rel = rel; a.ld_rel = ld_rel; a.lam = lam; a.mu = 1.f - lam; a.normalize = normalize; a.k_out = k;
  a.out_score = out_score; a.out_ids = out_ids; a.out_slot = out_slot;
  return launch_slate<M_PICK>(a, n_rows, (hipStream_t)stream);
}

extern "C" int recnn_slate_ild(const float* table, int n_items, const void* ids, int64_t ld_ids, int n_rows, int n_candidates,
                               int ids_are_int64, int kind, double* out, void* stream) {
  SlateArgs a;
  if (int rc = slate_check("slate_ild", table, n_items, ids, ld_ids, n_rows, n_candidates, ids_are_int64, kind, &a)) return rc;
  RECNN_REQUIRE((out && ((uintptr_t)out & 7) == 0) || n_rows == 0, "slate_ild: out is null or misaligned");
  if (n_rows == 0) return 0;
  a.ild = out;
  return launch_slate<M_ILD>(a, n_rows, (hipStream_t)stream);
}
