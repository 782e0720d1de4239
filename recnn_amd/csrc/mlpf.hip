// mlpf.hip -- a whole FROZEN network (target actor, target critic, the actor between its optimizer steps) on 128-row panels
// of a policy cycle's batches: all three layers in one workgroup, weights streamed once per 128 rows.  bf16, gfx950.
//
//   Actor   h1 = drop(relu(x W1^T + b1)); h2 = drop(relu(h1 W2^T + b2)); out = h2 W3^T + b3 (+ clip(noise))   recnn/nn/models.py:66-73
//   Critic  h1 = relu([state | action] W1^T + b1); h2 = relu(h1 W2^T + b2); q = h2 . w3 + b3               recnn/nn/models.py:207-213
//
// Cycle mode (engine.hip) applies these networks to M = cycle x rows rows at once.  Doing that with the per-step kernels (a
// tiled layer-1 GEMM, then 32-row tail panels that each restart a 128-192 KB weight stream) spent as long on the 16 % of
// the FLOPs after layer 1 as on layer 1 itself.  Here a 16-wave workgroup owns 128 rows x all 256 hidden columns (waves as
// 4 row groups x 4 column groups, wave tile 32 x 64: six fragment reads per eight MFMAs):
//   layer 1   64-k slabs of A (16 KB) + W1 (32 KB) through a 3-slot ring over the whole 144 KB, two slabs ahead;
//   then      the activation panel (4 sub-panels of 32 rows in mlp_panel.h's swizzled layout: 64 KB) takes the ring's first
//             64 KB, W2's four and W3's two 32 KB slabs stream through a 3-slot ring in the other 96 KB;
//   critic    q dots from the h2 panel (8 rows per wave).
// Per output element the arithmetic is the per-step kernels' (l1gemm.hip + mlpt.hip = mlps.hip): k ascending in MFMA steps of
// 32 from a zero accumulator, the segments in order (up to four: [s' | a'] of a target critic is three shifted windows of the
// cycle's state / action / next-rating arrays and the target actor's output), weights as the first MFMA operand, the same epilogues
// (mlp_panel.h), the same q-dot lane map and reduction tree -- so `run()` in cycle mode equals the eager step loop bit for bit.
#include <cstddef>
#include <cstring>
#include <type_traits>
#include "mlp_panel.h"
#include "split.h"
#include "recnn_hip_debug.h"

namespace {
constexpr int NW = 16;
constexpr int W_BYTES = HP * 128;                // 32 KB: one 64-k slab of a 256-row weight matrix
constexpr int NST1 = 3;
constexpr int LDS_TOTAL = 160 * 1024;
// FR = rows per workgroup: 128 (waves as 4 row groups x 4 column groups, wave tile 32 x 64), or 64 (2 x 8, wave tile 32 x 32) for the
// launches of SHORT cycle segments (round 6): a launch lasts as long as one workgroup does (one workgroup per CU, <= 256 of them), and a
// request that starts or ends inside a policy cycle -- the driver's 20 steps are segments of 6 + 10 + 4 -- pays two launches per
// segment whatever its length; half the rows per workgroup is 0.7 of the time (tools/frozen_trace.py: 48.5k against 69.6k clocks) while
// the launch still fits one round.
template <int FR> struct FrozenPlan {
  static constexpr int WMG = FR / 32, WNG = NW / WMG;            // row groups x column groups of the 16 waves
  static constexpr int TNH = HP / WNG / 16;                      // 16-column blocks per wave in the hidden layers: 4 | 2
  static constexpr int TN3 = 128 / WNG / 16;                     // ... in the actor's output layer: 2 | 1
  static constexpr int A_BYTES = FR * 128;                       // one 64-k slab of the rows: 16 | 8 KB
  static constexpr int STAGE1 = A_BYTES + W_BYTES;               // 48 | 40 KB
  static constexpr int PANEL_BYTES = WMG * 2 * PANEL_HALF;       // 32-row sub-panels: 64 | 32 KB
  static constexpr int WR_OFF = PANEL_BYTES;                     // the later layers' ring: 3 x 32 KB behind the panel
  static constexpr int CONST_OFF = NST1 * STAGE1;                // 144 | 120 KB: b1 | b2 | b3 or w3 (fp32, 1 KB each) while layer 1 runs --
  static constexpr int A_WAVES = FR / 8;                         //   inside the later ring's third stage in both plans
  static_assert(CONST_OFF + 3 * 1024 <= LDS_TOTAL && PANEL_BYTES + 3 * W_BYTES <= LDS_TOTAL, "the two LDS plans share one allocation");
  static_assert(CONST_OFF >= WR_OFF + 2 * W_BYTES, "the constants must survive the later layers' first two slabs");
};
}  // namespace

template <int FR>
__global__ __launch_bounds__(NW * 64) void mlp_frozen_kernel(const FrozenBatch batch) {
  using PL = FrozenPlan<FR>;
  constexpr int WNG = PL::WNG, TNH = PL::TNH, TN3 = PL::TN3, A_BYTES = PL::A_BYTES, STAGE1 = PL::STAGE1, WR_OFF = PL::WR_OFF, CONST_OFF = PL::CONST_OFF;
  const FrozenProb& P = batch.p[blockIdx.y];
  const int m0 = blockIdx.x * FR;
  if (m0 >= P.rows) return;
  // pull this problem's kernel-argument lines into the scalar cache, all in flight together
  kernarg_prefetch<sizeof(FrozenProb)>(blockIdx.y * sizeof(FrozenProb));
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const unsigned lds0 = (unsigned)(size_t)lds;
  const int tid = threadIdx.x, lane = tid & 63;
  // (debug: phase stamps by thread 0 -- tools/frozen_trace.py)
  unsigned long long* const trw = batch.trace ? batch.trace + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 16 : nullptr;
  auto stamp = [&](int k) { if (trw && tid == 0) TRACE_STAMP(trw, k); };
  stamp(0);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WNG, wn = wave % WNG;    // rows 32 wm .. + 31, hidden columns 16 TNH wn .. + 16 TNH - 1
  const int fr = lane & 15, fg = lane >> 4;
  const bool actor = P.W3 != nullptr;
  const int sw = (fr >> 1) & 7;

  // ---- the biases (and a critic's last-layer row) through the stream itself: three 1 KB transfers (waves 0..2) into the 16 KB
  // that layer 1's ring leaves free; the epilogues read them from LDS.  (Held in registers across the k loop they cost 28
  // VGPRs the kernel does not have -- the first version spilled; fetched by ordinary loads after layer 1 they cost a memory
  // latency on every workgroup's critical path.)
  if (wave < 3) {
    const float* src = wave == 0 ? P.b1 : (wave == 1 ? P.b2 : (actor ? P.b3 : P.w3row));
    const int nvalid = wave < 2 ? P.H : (actor ? P.out_dim : P.H);
    dma_s((unsigned)(min(lane * 4, nvalid - 4) * 4), src, lds0 + CONST_OFF + wave * 1024);
  }
  float b3s = 0.f;                                // critic: b3 through the scalar cache
  if (!actor) sload_dword(b3s, P.b3);
  int32_t step_now = 0;
  if (P.mask_mode == RECNN_MASK_HASH && P.step_ptr) sload_dword(step_now, P.step_ptr);

  // ------------------------------------------------------------------ layer 1
  // slab = A rows (one instruction per wave: rows 8 wave .. + 7) + 256 W1 rows (two per wave: rows l_row, l_row + 128); chunk c
  // of slab row r at position c ^ ((r >> 1) & 7)
  // up to four contraction segments: slab t belongs to the segment whose cumulative slab count first exceeds t.  The boundaries are
  // scalars (an absent segment's equals nt, which no issue reaches); the segment table stays in the kernel arguments
  const int nb1 = P.K[0] / 64;
  const int nb2 = nb1 + (P.nseg > 1 ? P.K[1] / 64 : 0);
  const int nb3 = nb2 + (P.nseg > 2 ? P.K[2] / 64 : 0);
  const int nt = nb3 + (P.nseg > 3 ? P.K[3] / 64 : 0);
  const int l_row = wave * 8 + (lane >> 3);
  const int l_c = ((lane & 7) ^ ((l_row >> 1) & 7)) * 16;
  const int gr_a = min(m0 + l_row, P.rows - 1);
  unsigned voff_a = (unsigned)(gr_a * (int)P.lda[0] * 2 + l_c);
  unsigned voff_w = (unsigned)(l_row * (int)P.ldw1 * 2 + l_c);
  const char* a_base = (const char*)P.A[0];
  const char* w_base = (const char*)P.W1 + (int64_t)P.w1_col[0] * 2;
  const int64_t w_half = (int64_t)128 * P.ldw1 * 2;
  const unsigned wave_kb = wave * 1024;
  int issued = 0;
  auto issue_l1 = [&]() {
    if (issued == nb1 || issued == nb2 || issued == nb3) {   // next contraction segment: re-base the three streams
      const bool g1 = issued == nb1, g2 = issued == nb2;     // (segments have at least one slab each: at most one boundary matches)
      const int lda = (int)(g1 ? P.lda[1] : (g2 ? P.lda[2] : P.lda[3]));
      const int col = g1 ? P.w1_col[1] : (g2 ? P.w1_col[2] : P.w1_col[3]);
      voff_a = (unsigned)(gr_a * lda * 2 + l_c);
      a_base = (const char*)(g1 ? P.A[1] : (g2 ? P.A[2] : P.A[3]));
      w_base = (const char*)P.W1 + (int64_t)col * 2;
    }
    const unsigned sb = lds0 + (issued % NST1) * STAGE1 + wave_kb;
    ++issued;
    if (FR == 128 || wave < PL::A_WAVES) dma_s(voff_a, a_base, sb);      // (64 rows: one instruction each from waves 0..7)
    dma_s(voff_w, w_base, sb + A_BYTES);
    dma_s(voff_w, w_base + w_half, sb + A_BYTES + NW * 1024);
    a_base += 128;
    w_base += 128;
  };
  issue_l1();
  issue_l1();                                     // (layer 1 has at least 2 slabs)

  f32x4 acc[2][TNH];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TNH; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int t = 0; t < nt; ++t) {
    if (t + 1 >= nt) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (FR == 128 || wave < PL::A_WAVES) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");     // (waves 8..15 of the 64-row plan issue two instructions per slab)
    __builtin_amdgcn_s_barrier();                 // slab t landed for every wave; the stage of slab t - 1 (= slab t + 2's) is free
    if (t == 0) stamp(1);
    if (t == 8) stamp(2);
    if (t == 16) stamp(3);
    if (t + 2 < nt) issue_l1();
    const unsigned char* sa = lds + (t % NST1) * STAGE1;
    const unsigned char* sb = sa + A_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int pos = ((ks * 4 + fg) ^ sw) * 16;
      uint4 a[2], b[TNH];
#pragma unroll
      for (int tm = 0; tm < 2; ++tm) a[tm] = *(const uint4*)(sa + (wm * 32 + tm * 16 + fr) * 128 + pos);
#pragma unroll
      for (int tn = 0; tn < TNH; ++tn) b[tn] = *(const uint4*)(sb + (wn * (16 * TNH) + tn * 16 + fr) * 128 + pos);
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < TNH; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, b[tn]), __builtin_bit_cast(bf16x8, a[tm]), acc[tm][tn], 0, 0, 0);
    }
  }
  // ---- every argument field used from here on, into registers once: requested here, so that the wait below (the last fragment reads')
  // covers them, and pinned -- the phases behind layer 1 are short latency chains, and a kernel-argument load with its lgkmcnt(0)
  // between a phase's LDS reads and their use (the epilogues had 14, the output stage about 90: P.out, P.ldo, P.addend ... per block)
  // waits for all of them (mlpt.hip got the same fix in round 6)
  // (pinned in two statements of eleven: a statement's fields are all requested before its one wait; pinned one by one, every load
  // was waited for on its own)
  int H = P.H, rows = P.rows, out_dim = P.out_dim, store_row0 = P.store_row0, rows_per_set = P.rows_per_set, mask_mode = P.mask_mode;
  int step_add = P.step_add, ldw2 = (int)P.ldw2;
  uint32_t seed = P.seed, stream1 = P.stream1, stream2 = P.stream2;
  asm volatile("" : "+s"(H), "+s"(rows), "+s"(out_dim), "+s"(store_row0), "+s"(rows_per_set), "+s"(mask_mode), "+s"(step_add), "+s"(ldw2), "+s"(seed),
               "+s"(stream1), "+s"(stream2));
  int64_t ldo = P.ldo, ld_add = P.ld_add, ldh = P.ldh;
  const char* W2 = (const char*)P.W2;
  const char* W3 = (const char*)P.W3;
  bf16_t* h1 = (bf16_t*)P.h1;
  bf16_t* h2 = (bf16_t*)P.h2;
  bf16_t* out = (bf16_t*)P.out;
  float* qout = P.q;
  const float* addend = P.addend;
  float add_clip = P.add_clip;
  asm volatile("" : "+s"(ldo), "+s"(ld_add), "+s"(ldh), "+s"(W2), "+s"(W3), "+s"(h1), "+s"(h2), "+s"(out), "+s"(qout), "+s"(addend), "+s"(add_clip));
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(step_now) : : "memory");   // (also the mask step requested at entry)
  __builtin_amdgcn_s_barrier();                   // every wave is done with layer 1's ring: the second LDS plan takes over
  stamp(4);

  // ---- the later layers' stream: slab c = W2's k-slab c (c < 4), then (actor) W3's two double slabs; ring stage c % 3
  const unsigned voff_sq = (unsigned)(l_row * ldw2 * 2 + l_c);   // W2 / W3 share the pitch (mlpf_launch)
  const int npost = actor ? 6 : 4;
  int posted = 0;
  auto issue_post = [&]() {
    if (posted >= npost) return;
    const int c = posted++;
    const unsigned wb = lds0 + WR_OFF + (c % 3) * W_BYTES + wave_kb;
    if (c < 4) {
      const char* b0 = W2 + c * 128;
      dma_s(voff_sq, b0, wb);
      dma_s(voff_sq, b0 + (int64_t)256 * ldw2, wb + NW * 1024);
    } else {                                      // W3: k-slabs 2 p and 2 p + 1 of its 128 rows as image rows 0..127 / 128..255
      const char* b0 = W3 + 2 * (c - 4) * 128;
      dma_s(voff_sq, b0, wb);
      dma_s(voff_sq, b0 + 128, wb + NW * 1024);
    }
  };
  issue_post();
  issue_post();
  int consumed = 0;
  // next slab of the later layers: waits until it has landed for every wave (2 instructions per wave and slab: at most one
  // younger slab outstanding), refills the stage the previous slab occupied
  auto next_post = [&]() -> const unsigned char* {
    const int c = consumed++;
    if (posted - c - 1 >= 1) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    issue_post();
    return lds + WR_OFF + (c % 3) * W_BYTES;
  };

  // ---- h1 = dropout(relu(acc + b1)) into this wave's sub-panel (rows 32 wm ..), columns 64 wn ..
  unsigned char* spanel = lds + wm * (2 * PANEL_HALF);
  const int sm0 = m0 + wm * 32;                   // first row of the sub-panel
  int mset = 0, mrow0 = sm0;
  if (rows_per_set > 0) { mset = sm0 / rows_per_set; mrow0 = sm0 - mset * rows_per_set; }
  const int32_t step0 = step_now + step_add + mset;
  const bool hash = mask_mode == RECNN_MASK_HASH;
  const uint32_t key1 = hash ? mask_key(seed, step0, stream1) : 0u;
  const uint32_t key2 = hash ? mask_key(seed, step0, stream2) : 0u;
  const float* cst = (const float*)(lds + CONST_OFF);
  // the mask mode as a compile-time constant under ONE uniform branch per epilogue (this kernel sees hash masks or none: mlpf_launch): as a
  // run-time value every element carried the external-mask, hash-mask and no-mask paths (2,280 instructions and 20 spilled registers in
  // the 128-row form; the two target networks take the no-mask path, the shorter one)
  auto epilogue = [&](const f32x4 (&bv)[TNH], uint32_t key) {
    if (hash) hidden_epilogue<TNH>(acc, bv, H, rows - (sm0 - mrow0), mrow0, wn, fr, fg, RECNN_MASK_HASH, nullptr, 0, key, spanel);
    else hidden_epilogue<TNH>(acc, bv, H, rows - (sm0 - mrow0), mrow0, wn, fr, fg, RECNN_MASK_NONE, nullptr, 0, 0u, spanel);
  };
  {
    f32x4 b1v[TNH];
#pragma unroll
    for (int tn = 0; tn < TNH; ++tn) {
      const int n = wn * (16 * TNH) + tn * 16 + fg * 4;
      b1v[tn] = (n + 3 < H) ? *(const f32x4*)(cst + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    epilogue(b1v, key1);
  }
  stamp(5);
  // the later layers' constants (after the epilogue: the accumulators' registers are free again)
  f32x4 b2v[TNH];
#pragma unroll
  for (int tn = 0; tn < TNH; ++tn) {
    const int n = wn * (16 * TNH) + tn * 16 + fg * 4;
    b2v[tn] = (n + 3 < H) ? *(const f32x4*)(cst + 256 + n) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float v3[TN3][4];                               // actor: b3 of this lane's output columns 16 TN3 wn + 16 tn + 4 fg + r
  float w3v[4];                                   // critic: w3 of columns 4 lane .. 4 lane + 3
#pragma unroll
  for (int tn = 0; tn < TN3; ++tn)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int no = wn * (16 * TN3) + tn * 16 + fg * 4 + r;
      v3[tn][r] = (actor && no < out_dim) ? cst[512 + no] : 0.f;
    }
#pragma unroll
  for (int r = 0; r < 4; ++r) w3v[r] = (!actor && lane * 4 + r < H) ? cst[512 + lane * 4 + r] : 0.f;
  // (the constants sit in what becomes the later layers' ring stage 2: every wave has read them -- the lgkmcnt(0) of
  // next_post -- before the first rendezvous below lets slab 2 be requested)

  // ------------------------------------------------------------------ layer 2
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < TNH; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int q = 0; q < 4; ++q) {
    const unsigned char* st = next_post();        // (its barrier also completes the h1 panel for q = 0)
    if (q == 0 && h1 && m0 + FR > store_row0) {   // (a workgroup wholly below the first stored row skips the pass)
#pragma unroll
      for (int sp = 0; sp < PL::WMG; ++sp) panel_to_global<NW>(lds + sp * (2 * PANEL_HALF), h1, ldh, m0 + sp * 32, rows, tid, store_row0);
    }
    const unsigned char* sa = spanel + (q >> 1) * PANEL_HALF;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int posa = ((((q & 1) * 8) + ks * 4 + fg) ^ fr) * 16;
      const int posb = ((ks * 4 + fg) ^ sw) * 16;
      uint4 a[2], b[TNH];
#pragma unroll
      for (int tm = 0; tm < 2; ++tm) a[tm] = *(const uint4*)(sa + (tm * 16 + fr) * 256 + posa);
#pragma unroll
      for (int tn = 0; tn < TNH; ++tn) b[tn] = *(const uint4*)(st + (wn * (16 * TNH) + tn * 16 + fr) * 128 + posb);
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < TNH; ++tn)
          acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, b[tn]), __builtin_bit_cast(bf16x8, a[tm]), acc[tm][tn], 0, 0, 0);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                   // everyone is done reading the h1 panel
  stamp(6);
  epilogue(b2v, key2);
  stamp(7);

  if (actor) {
    // ---------------------------------------------------------------- layer 3: 128 x 128 outputs, wave tile 32 x 32
    f32x4 o[2][TN3];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < TN3; ++j) o[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < 2; ++p) {
      const unsigned char* st = next_post();      // (completes the h2 panel for p = 0)
      if (p == 0 && h2 && m0 + FR > store_row0) {
#pragma unroll
        for (int sp = 0; sp < PL::WMG; ++sp) panel_to_global<NW>(lds + sp * (2 * PANEL_HALF), h2, ldh, m0 + sp * 32, rows, tid, store_row0);
      }
#pragma unroll
      for (int hq = 0; hq < 2; ++hq) {            // k quarter q = 2 p + hq of the panel against image rows hq * 128 + output column
        const int q = 2 * p + hq;
        const unsigned char* sa = spanel + (q >> 1) * PANEL_HALF;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int posa = ((((q & 1) * 8) + ks * 4 + fg) ^ fr) * 16;
          const int posb = ((ks * 4 + fg) ^ sw) * 16;
          uint4 a[2], b[TN3];
#pragma unroll
          for (int tm = 0; tm < 2; ++tm) a[tm] = *(const uint4*)(sa + (tm * 16 + fr) * 256 + posa);
#pragma unroll
          for (int tn = 0; tn < TN3; ++tn) b[tn] = *(const uint4*)(st + (hq * 128 + wn * (16 * TN3) + tn * 16 + fr) * 128 + posb);
#pragma unroll
          for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN3; ++tn)
              o[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, b[tn]), __builtin_bit_cast(bf16x8, a[tm]), o[tm][tn], 0, 0, 0);
        }
      }
    }
    stamp(8);
    // out = o + b3 (+ clip(addend)) as bf16.  The presence of an addend and a full 128-column output are uniform: decided once, not per
    // element; one 64-bit row offset per row block instead of one per element.  Narrower outputs keep the column tests and the rule
    // that padded columns hold bf16 +0.
    auto out_stage = [&](auto FULLc, auto ADDc) {
      constexpr bool FULL = decltype(FULLc)::value, ADD = decltype(ADDc)::value;
#pragma unroll
      for (int tm = 0; tm < 2; ++tm) {
        const int m = sm0 + tm * 16 + fr;
        const bool mrow = m < rows;
        bf16_t* const orow = out + (int64_t)m * ldo;
        const float* const arow = ADD ? addend + (int64_t)m * ld_add : nullptr;
#pragma unroll
        for (int tn = 0; tn < TN3; ++tn) {
          const int no = wn * (16 * TN3) + tn * 16 + fg * 4;
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool ncol = FULL || no + r < out_dim;
            v[r] = o[tm][tn][r] + v3[tn][r];
            if (ADD && ncol && mrow) {
              const float z = arow[no + r];
              v[r] += fminf(fmaxf(z, -add_clip), add_clip);
            }
            if (!ncol) v[r] = 0.f;
          }
          uint2 packed = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
          if (!FULL && no + 3 >= out_dim) {                    // (padded columns hold bf16 +0, not -0)
            if (no + 0 >= out_dim) packed.x &= 0xFFFF0000u;
            if (no + 1 >= out_dim) packed.x &= 0x0000FFFFu;
            if (no + 2 >= out_dim) packed.y &= 0xFFFF0000u;
            if (no + 3 >= out_dim) packed.y &= 0x0000FFFFu;
          }
          if (mrow) {
            if (FULL || no + 3 < out_dim) {
              *(uint2*)(orow + no) = packed;
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (no + r < out_dim) orow[no + r] = (bf16_t)((r < 2 ? packed.x : packed.y) >> ((r & 1) * 16));
            }
          }
        }
      }
    };
    if (out_dim == 128) {
      if (addend) out_stage(std::true_type{}, std::true_type{});
      else out_stage(std::true_type{}, std::false_type{});
    } else {
      if (addend) out_stage(std::false_type{}, std::true_type{});
      else out_stage(std::false_type{}, std::false_type{});
    }
    stamp(9);
    return;
  }

  // ------------------------------------------------------------------ critic head: q[m] = h2[m, :] . w3 + b3, 8 rows per wave
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b3s) : : "memory");
  __builtin_amdgcn_s_barrier();                   // h2 panel complete
  if (h2 && m0 + FR > store_row0) {
#pragma unroll
    for (int sp = 0; sp < PL::WMG; ++sp) panel_to_global<NW>(lds + sp * (2 * PANEL_HALF), h2, ldh, m0 + sp * 32, rows, tid, store_row0);
  }
#pragma unroll
  for (int i = 0; i < FR / NW; ++i) {           // (unrolled: the rows' panel reads and reduction trees interleave)
    const int prow = wave * (FR / NW) + i;        // row of the 128-row panel
    const unsigned char* pp = lds + (prow >> 5) * (2 * PANEL_HALF);
    const int row = prow & 31;
    const int c = ((((lane * 4) & 127) >> 3) ^ (row & 15));
    const uint2 hv = *(const uint2*)(pp + ((lane * 4) >> 7) * PANEL_HALF + row * 256 + c * 16 + ((lane * 4) & 7) * 2);
    const float hf[4] = {bf2f((bf16_t)(hv.x & 0xFFFFu)), bf2f((bf16_t)(hv.x >> 16)), bf2f((bf16_t)(hv.y & 0xFFFFu)), bf2f((bf16_t)(hv.y >> 16))};
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) s += lane * 4 + j < H ? hf[j] * w3v[j] : 0.f;
    s = wave_sum(s);
    if (lane == 0 && m0 + prow < rows && qout) qout[m0 + prow] = s + b3s;
  }
  stamp(9);
}
static unsigned long long* g_frozen_trace = nullptr;
extern "C" void recnn_debug_frozen_trace(void* p) { g_frozen_trace = (unsigned long long*)p; }   // read at launch (= graph capture) time

int mlpf_init() {
  int rc = recnn_check_hip(hipFuncSetAttribute((const void*)mlp_frozen_kernel<128>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_TOTAL), "mlp_frozen attr");
  if (!rc) rc = recnn_check_hip(hipFuncSetAttribute((const void*)mlp_frozen_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_TOTAL), "mlp_frozen<64> attr");
  return rc;
}

int mlpf_launch(const FrozenBatch& b, int nprob, hipStream_t s, int panel_rows) {
  RECNN_REQUIRE(nprob >= 1 && nprob <= FROZEN_MAX_GROUP, "mlp_frozen: 1..%d problems per launch", FROZEN_MAX_GROUP);
  RECNN_REQUIRE(panel_rows == 128 || panel_rows == 64, "mlp_frozen: 128 or 64 rows per workgroup");
  int rows = 0;
  for (int i = 0; i < nprob; ++i) {
    const FrozenProb& p = b.p[i];
    if (p.rows > rows) rows = p.rows;
    RECNN_REQUIRE(p.rows > 0 && p.H >= 8 && p.H <= HP && (p.H & 7) == 0 && p.out_dim <= 128, "mlp_frozen: hidden <= 256 (multiple of 8), out_dim <= 128");
    RECNN_REQUIRE(p.nseg >= 1 && p.nseg <= FROZEN_MAX_SEG && p.W1 && p.W2 && p.b1 && p.b2 && p.b3, "mlp_frozen: bad problem");
    int k64 = 0;
    for (int g = 0; g < p.nseg; ++g) {
      RECNN_REQUIRE(p.A[g] && p.K[g] > 0 && p.K[g] % 64 == 0 && p.lda[g] % 8 == 0 && (((uintptr_t)p.A[g]) & 15) == 0 && (p.w1_col[g] & 7) == 0 &&
                        p.w1_col[g] >= 0 && p.w1_col[g] + p.K[g] <= p.ldw1 && (int64_t)p.rows * p.lda[g] * 2 < (1ll << 31),
                    "mlp_frozen: segment %d must be 16-byte aligned with K a multiple of 64 (and < 2 GB)", g);
      k64 += p.K[g] / 64;
    }
    RECNN_REQUIRE(k64 >= 2, "mlp_frozen: layer 1 needs at least 128 k");
    RECNN_REQUIRE(p.ldw1 % 8 == 0 && p.ldw2 % 8 == 0 && (((uintptr_t)p.W1 | (uintptr_t)p.W2) & 15) == 0, "mlp_frozen: bad weight pitches");
    // (whatever H and out_dim: the stream reads HP rows of W1 / W2 and 128 of W3, HP columns of W2 / W3, and the panel stores write HP
    //  columns of h1 / h2, those at and beyond H as +0 -- the arrays must be that large; their pitches are what can be checked here)
    RECNN_REQUIRE(p.ldw2 >= HP, "mlp_frozen: W2 (and W3) must hold %d columns per row, zero or not beyond H", HP);
    RECNN_REQUIRE((!p.h1 && !p.h2) || (p.ldh >= HP && p.ldh % 8 == 0), "mlp_frozen: stored activations take %d columns per row (a pitch that is a multiple of 8)", HP);
    RECNN_REQUIRE(p.mask_mode == RECNN_MASK_NONE || p.mask_mode == RECNN_MASK_HASH, "mlp_frozen: hash dropout masks only");
    RECNN_REQUIRE(p.store_row0 >= 0 && p.store_row0 <= p.rows, "mlp_frozen: the first stored activation row lies outside the problem");
    RECNN_REQUIRE(p.rows_per_set == 0 || p.rows_per_set % 32 == 0, "mlp_frozen: batches must be multiples of 32 rows");
    if (p.W3) RECNN_REQUIRE(p.out && p.ldw3 == p.ldw2 && (((uintptr_t)p.W3) & 15) == 0 && p.ldo % 4 == 0, "mlp_frozen: actor needs W3 (same pitch as W2) and an output");
    // (b3 reaches LDS in groups of four floats, the last group shifted back to end at out_dim: a width that is no multiple of 4 would put
    //  the last columns' biases two places off -- the engine's action widths are multiples of 8)
    if (p.W3) RECNN_REQUIRE(p.out_dim >= 4 && p.out_dim % 4 == 0, "mlp_frozen: the actor's output width must be a multiple of 4");
    else RECNN_REQUIRE(p.w3row && p.q, "mlp_frozen: critic needs its last layer's row and a Q output");
  }
  FrozenBatch bb = b;
  bb.trace = g_frozen_trace;
  if (panel_rows == 64) hipLaunchKernelGGL(mlp_frozen_kernel<64>, dim3((rows + 63) / 64, nprob), dim3(NW * 64), LDS_TOTAL, s, bb);
  else hipLaunchKernelGGL(mlp_frozen_kernel<128>, dim3((rows + 127) / 128, nprob), dim3(NW * 64), LDS_TOTAL, s, bb);
  return recnn_check_hip(hipGetLastError(), "mlp_frozen_kernel");
}

// One problem on caller-supplied device buffers (csrc/recnn_hip_debug.h): the kernel's edge cases -- two and three layer-1 slabs, every
// segment boundary, narrow outputs, an addend without masks -- are out of the engine's reach (its networks give 21 or 23 slabs).
extern "C" int recnn_debug_frozen_forward(const recnn_debug_frozen_args* a, int64_t sizeof_args, void* stream) {
  RECNN_REQUIRE(a && sizeof_args == (int64_t)sizeof(*a), "debug_frozen_forward: null pointer or another layout of the argument block");
  RECNN_REQUIRE(a->nseg >= 1 && a->nseg <= FROZEN_MAX_SEG, "debug_frozen_forward: 1..%d segments", FROZEN_MAX_SEG);
  int rc = mlpf_init();
  if (rc) return rc;
  FrozenBatch fb;
  memset(&fb, 0, sizeof(fb));
  FrozenProb& p = fb.p[0];
  for (int g = 0; g < a->nseg; ++g) { p.A[g] = a->A[g]; p.lda[g] = a->lda[g]; p.K[g] = a->K[g]; p.w1_col[g] = a->w1_col[g]; }
  p.nseg = a->nseg;
  p.W1 = a->W1; p.ldw1 = a->ldw1; p.W2 = a->W2; p.ldw2 = a->ldw2; p.W3 = a->W3; p.ldw3 = a->ldw3;
  p.b1 = a->b1; p.b2 = a->b2; p.b3 = a->b3; p.w3row = a->w3row;
  p.rows = a->rows; p.H = a->H; p.out_dim = a->out_dim;
  p.mask_mode = a->mask_mode; p.seed = a->seed; p.stream1 = a->stream1; p.stream2 = a->stream2;
  p.step_ptr = nullptr; p.step_add = a->step; p.rows_per_set = a->rows_per_set;
  p.h1 = a->h1; p.h2 = a->h2; p.ldh = a->ldh; p.store_row0 = a->store_row0;
  p.out = a->out; p.ldo = a->ldo; p.addend = a->addend; p.ld_add = a->ld_add; p.add_clip = a->add_clip; p.q = a->q;
  return mlpf_launch(fb, 1, (hipStream_t)stream, a->panel_rows);
}
