// engine_plan.hip -- the launch plans of a DDPG / TD3 step (split out of engine.hip in round 5): optimizer layouts, GEMM / MLP problem
// builders, the per-engine tuning entry points, the phases of a step (forward in its four schedules: fused row panels, split, cycle-batched
// frozen networks, split bf16; value backward; policy loss and its backward chain; finish), the batch buffer sets, and step_impl.
// recnn/nn/update/ddpg.py:58-104, td3.py:66-150, misc.py:25-44 are what the sequence of launches replaces; state and the interface to the
// other units are engine_internal.h.
#include "engine_internal.h"

// ------------------------------------------------------------------------------------ layouts
namespace recnn_eng {

bool value_panel_ok(const recnn_engine* e);

NetLayout make_layout(const recnn_engine* e, int ni, int rows) {
  const Net& n = e->net[ni];
  NetLayout L;
  memset(&L, 0, sizeof(L));
  const int H = e->H;
  const int tiles_m = (rows + 31) / 32;
  const int nblk_hb = (rows + HEAD_ROWS_PER_BLOCK - 1) / HEAD_ROWS_PER_BLOCK;
  const int rr[6] = {H, 1, H, 1, n.out_dim, 1};
  const int cc[6] = {n.in_dim, H, H, H, H, n.out_dim};
  int blk = 0;
  for (int i = 0; i < 6; ++i) {
    TensorSeg& t = L.t[i];
    t.p_off = n.off[i];
    t.rows = rr[i];
    t.cols = cc[i];
    t.sh_off = n.sh_off[i];
    t.sh_ld = i == W1 ? n.ld_w1 : (i == W2 ? n.ld_w2 : n.ld_w3);
    t.col_rot = (i == W1 && n.critic) ? e->A : 0;
    t.gpart = n.gp[i];
    t.blk0 = blk;
    const int64_t ne = (int64_t)t.rows * t.cols;
    blk += opt_blocks(ne);
    t.small = opt_is_small(ne);
    t.nslab = 1;
    t.slab_stride = 0;
  }
  L.nblk = blk;
  L.n_params = n.n_params;
  if (rows > 0 && n.gp[W1]) {
    auto sp = [&](int mx) { int s = rows / 128; if (s < 1) s = 1; return s > mx ? mx : s; };
    L.t[W1].nslab = sp(e->tune.dw_splits); L.t[W1].slab_stride = (int64_t)H * n.in_dim;
    L.t[W2].nslab = sp(SP_W2); L.t[W2].slab_stride = (int64_t)H * H;
    L.t[B1].nslab = tiles_m; L.t[B1].slab_stride = H;
    if (n.critic) {
      const bool half = e->half_panels && e->panel_bwd_done && !e->unit_bwd;   // mlpt.hip ran 16-row panels: half-panel sums, taken in pairs
      const int nhead = (value_panel_ok(e) || half) ? tiles_m : nblk_hb;  // bwd.hip emits one partial per 32 rows, head.hip per 16
      L.t[W3].nslab = nhead; L.t[W3].slab_stride = H;
      L.t[B2].nslab = nhead; L.t[B2].slab_stride = H;
      L.t[B3].nslab = nhead; L.t[B3].slab_stride = 1;
      if (half) L.t[B1].pair = L.t[W3].pair = L.t[B2].pair = L.t[B3].pair = 1;
    } else {
      L.t[W3].nslab = sp(SP_W3); L.t[W3].slab_stride = (int64_t)e->A * H;
      L.t[B2].nslab = tiles_m; L.t[B2].slab_stride = H;
      L.t[B3].nslab = tiles_m; L.t[B3].slab_stride = e->A;
    }
  }
  for (int i = 0; i < 6; ++i) {
    TensorSeg& t = L.t[i];
    const int64_t ne = (int64_t)t.rows * t.cols;
    t.vec4 = !t.small && ne % 4 == 0 && t.p_off % 4 == 0 && (t.nslab <= 1 || t.slab_stride % 4 == 0) &&
             (((uintptr_t)t.gpart) & 15) == 0;
  }
  return L;
}

// byte offset of logical column `col` (a multiple of 32 for split rows) inside a compute-type row
inline int64_t tc_off(const recnn_engine* e, int col) { return (int64_t)(e->x3 ? 2 * col : col) * e->esz; }
inline char* sh_ptr(const recnn_engine* e, int ni, int which) {
  const Net& n = e->net[ni];
  return n.shadow + n.sh_off[which] * e->esz;
}

// (the finished per-rank gradient always goes to the bound arena; a collective copies it into the peer buffer itself, with
// system-scope stores)
inline float* g_produce(const recnn_engine* e, int ni) { return e->net[ni].g; }
// where its optimizer reads the gradient: a critic's, in region mode, straight from the collective's out[] (system-scope loads,
// ApplyArgs.g_sys); everything else from the bound arena, where the collective launch delivers the sums
inline bool g_direct(const recnn_engine* e, int ni) { return e->comm && e->comm_region && e->net[ni].critic; }
inline float* g_consume(const recnn_engine* e, int ni) { return g_direct(e, ni) ? comm_out(e->comm, e->comm_off[ni]) : e->net[ni].g; }
int net_allreduce(recnn_engine* e, int ni, const char* name, hipStream_t s);

// The optimizer / soft-update description of network `ni` (shared by apply_kernel launches and the fused dW epilogue).
int fill_apply_args(recnn_engine* e, int ni, const NetLayout& L, bool do_adam, int opt_idx, float grad_scale, bool clip, int target_ni,
                    float tau, ApplyArgs* out) {
  Net& n = e->net[ni];
  ApplyArgs& a = *out;
  memset(&a, 0, sizeof(a));
  a.p = n.p; a.g = g_consume(e, ni); a.m = n.m; a.v = n.v;
  a.g_sys = g_direct(e, ni);
  a.shadow = n.shadow;
  a.tc_bf16 = e->cfg.dtype;
  a.do_adam = do_adam;
  a.t_ptr = n.t_ptr;
  a.t_add = e->run_t_off[ni];
  if (do_adam) {
    RECNN_REQUIRE(n.g && n.m && n.v && n.t_ptr, "apply: network %d has no optimizer state bound", ni);
    a.lr = e->hy.lr[opt_idx]; a.beta1 = e->hy.beta1[opt_idx]; a.beta2 = e->hy.beta2[opt_idx];
    a.eps = e->hy.eps[opt_idx]; a.weight_decay = e->hy.weight_decay[opt_idx];
    a.opt_kind = e->hy.opt_kind[opt_idx];
    if (a.opt_kind == RECNN_OPT_RANGER) {
      RECNN_REQUIRE(n.slow, "apply: network %d runs Ranger but has no Lookahead slow-weight arena bound (recnn_engine_bind_slow)", ni);
      a.slow = n.slow; a.la_alpha = e->hy.la_alpha[opt_idx]; a.la_k = e->hy.la_k[opt_idx]; a.nsma_thr = e->hy.nsma_threshold[opt_idx];
    }
  }
  a.grad_scale = grad_scale;
  a.g_out = n.g;
  a.l1part = clip ? n.l1part : nullptr;
  a.n_l1 = clip ? L.nblk : 0;
  a.coef_out = clip ? e->coef_out : nullptr;
  if (target_ni >= 0) {
    a.tgt_p = e->net[target_ni].p;
    a.tgt_shadow = e->net[target_ni].shadow;
    a.tau = tau;
  }
  return 0;
}

int apply_net(recnn_engine* e, int ni, int rows, bool do_adam, int opt_idx, float grad_scale, bool clip, int target_ni,
              float tau, hipStream_t s, bool from_slabs) {
  Net& n = e->net[ni];
  // (recnn_engine_state_grads: this launch rewrites the shadow of `ni` -- the critic's serves both gradients, the actor's the policy loss's)
  if (ni == RECNN_NET_VALUE1) e->sg_ok = 0;
  else if (ni == RECNN_NET_VALUE2) e->sg_ok &= ~1;   // (TD3: critic 2 serves the value losses' gradient only)
  else if (ni == RECNN_NET_POLICY) e->sg_ok &= ~2;
  NetLayout L = make_layout(e, ni, rows);
  ApplyArgs a;
  int rc = fill_apply_args(e, ni, L, do_adam, opt_idx, grad_scale, clip, target_ni, tau, &a);
  if (rc) return rc;
  a.from_slabs = from_slabs && do_adam && rows > 0;
  if (e->comm && a.from_slabs) {   // data parallel: the exchange runs inside this launch (comm_fused_ok checked by the caller)
    if ((rc = comm_port(e->comm, e->comm_off[ni], &a.comm))) return rc;
    a.comm_nwg = L.nblk;
    a.g = n.g; a.g_sys = 0;
  }
  const GatherArgs* pg = (do_adam && ni == RECNN_NET_VALUE1) ? e->pregather : nullptr;
  return slot(e, do_adam ? (n.critic ? (pg ? "adam_critic+gather" : "adam_critic") : "adam_actor") : "shadow_refresh", 0, s,
              [&] { return apply_launch(L, a, s, pg); }, !do_adam && target_ni < 0);
}

// ---- what a problem is: stated once, whatever the schedule that launches it ----------------
constexpr int POL = RECNN_NET_POLICY, TPOL = RECNN_NET_TARGET_POLICY;
constexpr int VAL[2] = {RECNN_NET_VALUE1, RECNN_NET_VALUE2}, TVAL[2] = {RECNN_NET_TARGET_VALUE1, RECNN_NET_TARGET_VALUE2};

// Dropout of one hidden layer: none, an external keep-mask [max_rows, H] per stream, or the counter-based hash keyed by (seed, stream,
// *step_ptr + step_add).  The kernel structs name these fields their own way (stream / stream_id / stream1, stream2; mask / mask1, mask2):
// every builder copies from here.  A network's second hidden layer takes the stream after its first's (mask2_idx).
struct MaskSel {
  int mode = RECNN_MASK_NONE;
  const uint8_t* ext = nullptr; int64_t pitch = 0;
  uint32_t seed = 0, stream = 0;
  const int32_t* step_ptr = nullptr; int step_add = 0;
};
MaskSel mask_sel(const recnn_engine* e, int mask_idx, int step_add, bool hash_only = false) {
  MaskSel m;
  const int mode = e->cfg.mask_mode;
  if (mask_idx < 0 || mode == RECNN_MASK_NONE || (hash_only && mode != RECNN_MASK_HASH)) return m;
  m.mode = mode;
  if (mode == RECNN_MASK_EXTERNAL) {
    m.ext = e->ext_masks + (int64_t)mask_idx * e->cfg.max_rows * e->H; m.pitch = e->H;
  } else {
    m.seed = e->cfg.seed; m.stream = (uint32_t)mask_idx; m.step_ptr = e->counters; m.step_add = step_add;
  }
  return m;
}
inline int mask2_idx(int mask_idx) { return mask_idx < 0 ? -1 : mask_idx + 1; }

// A network's weights as the forward and backward launches read them: the compute-type shadows of W1 / W2 (/ W3: an actor's), the
// canonical fp32 biases, a critic's last layer as its canonical fp32 row.  (critic <=> out_dim == 1: net_dims gives a critic one output
// and an actor A of them, and the launch that asks by out_dim -- x3tail.hip -- only runs at A == 128.)
struct NetView {
  const char *W1, *W2, *W3; int64_t ldw1, ldw2, ldw3;
  const float *b1, *b2, *b3, *w3row;
};
NetView net_view(const recnn_engine* e, int ni) {
  const Net& n = e->net[ni];
  NetView v;
  v.W1 = sh_ptr(e, ni, W1); v.ldw1 = n.ld_w1;
  v.W2 = sh_ptr(e, ni, W2); v.ldw2 = n.ld_w2;
  v.W3 = n.critic ? nullptr : sh_ptr(e, ni, W3); v.ldw3 = n.critic ? 0 : n.ld_w3;
  v.b1 = n.p + n.off[B1]; v.b2 = n.p + n.off[B2]; v.b3 = n.p + n.off[B3];
  v.w3row = n.critic ? n.p + n.off[W3] : nullptr;
  return v;
}

// One application of a network in a step: what it reads, its dropout streams, where its results go.  Every schedule turns a role into a
// problem of its own launches (fill_fwd per layer, fill_mlp, fill_l1 + fill_tail, fill_x3tail, ph_frozen_batched's fill).
struct Role {
  int ni;
  const void* A0; int64_t lda0; int K0; int col0;                            // layer-1 input: first segment, its first W1-shadow column
  const void* A1 = nullptr; int64_t lda1 = 0; int K1 = 0; int col1 = 0;      // optional second segment, contracted after the first
  int mask_idx = -1;   // dropout stream of the first hidden layer (second: + 1); -1 = eval mode
  int step_add = 0;    // mask key step on top of the device counter
  void* h1 = nullptr; void* h2 = nullptr;                                    // hidden activations ...
  bool keep = false;   // ... which a backward reads: the row-panel launches store them too (layer-by-layer launches always do)
  void* out = nullptr; int64_t ldo = 0;                                      // an actor's output
  const float* addend = nullptr; int64_t ld_add = 0; float add_clip = 0.f;   // ... + clipped noise (TD3's target action)
  float* q = nullptr;  // a critic's Q per row (b3 included)
};

// The buffers the roles live in: the step's own, or a whole policy cycle's (cycle mode: n batches side by side, M = n * rows rows).
struct StepBufs {
  char *xs, *xn;                                       // packed rows [action | state], pitch e->ldx
  char *tp_h1, *tp_h2, *pa_h1, *pa_h2, *ga, *tq_h1[2], *tq_h2[2];
  float* tq[2];
  const float* noise;
  int step_add;
};
StepBufs step_bufs(const recnn_engine* e) {
  StepBufs b;
  b.xs = e->xcs; b.xn = e->xcn;
  b.tp_h1 = e->tp.h1; b.tp_h2 = e->tp.h2; b.pa_h1 = e->pa.h1; b.pa_h2 = e->pa.h2; b.ga = e->gen_action;
  for (int c = 0; c < 2; ++c) { b.tq_h1[c] = e->tq[c].h1; b.tq_h2[c] = e->tq[c].h2; b.tq[c] = e->tqv[c]; }
  b.noise = e->ext_noise ? e->ext_noise : e->noise_buf;
  b.step_add = e->run_off;
  return b;
}
// ... of the cycle whose first batch is step run_off0 of the run; the actor's operands from batch actor_set0 on (its batches may be dealt
// out over two launches).  (bf16 only: 2 bytes per element.)
StepBufs cycle_bufs(const recnn_engine* e, int rows, int run_off0, int actor_set0 = 0) {
  const int64_t r0 = (int64_t)actor_set0 * rows;
  StepBufs b;
  b.xs = e->m_xs + r0 * e->ldx * 2; b.xn = e->m_xn;
  b.tp_h1 = e->m_tp_h1; b.tp_h2 = e->m_tp_h2;
  b.pa_h1 = e->m_pa_h1 + r0 * e->Hp * 2; b.pa_h2 = e->m_pa_h2 + r0 * e->Hp * 2; b.ga = e->m_ga + r0 * e->Ap * 2;
  for (int c = 0; c < 2; ++c) {
    b.tq_h1[c] = e->m_tq_h1[c]; b.tq[c] = e->m_tq[c];
    b.tq_h2[c] = c == 0 ? e->m_tp_h2 : e->m_tp_h1;     // (layer-by-layer form: the target actor's panels are done with by then)
  }
  b.noise = e->ext_noise ? e->ext_noise : e->m_noise;
  b.step_add = run_off0 + actor_set0;
  return b;
}

// target actor on s': next_action into the action slot of the packed next rows (+ TD3's clipped noise, td3.py:74-78)
Role role_target_actor(const recnn_engine* e, const StepBufs& b) {
  Role r{TPOL, b.xn + tc_off(e, e->A), e->ldx, e->K1a, 0};
  r.step_add = b.step_add;
  r.h1 = b.tp_h1; r.h2 = b.tp_h2; r.out = b.xn; r.ldo = e->ldx;
  if (e->td3) { r.addend = b.noise; r.ld_add = e->A; r.add_clip = e->hy.noise_clip; }
  return r;
}
// actor on s: gen_action, activations kept for the policy step's backward
Role role_actor(const recnn_engine* e, const StepBufs& b) {
  Role r{POL, b.xs + tc_off(e, e->A), e->ldx, e->K1a, 0};
  r.mask_idx = e->td3 ? 4 : 2; r.step_add = b.step_add;
  r.h1 = b.pa_h1; r.h2 = b.pa_h2; r.keep = true; r.out = b.ga; r.ldo = e->Ap;
  return r;
}
// learning critic c on [action | state]
Role role_critic(const recnn_engine* e, const StepBufs& b, int c) {
  Role r{VAL[c], b.xs, e->ldx, e->K1c, 0};
  r.mask_idx = 2 * c; r.step_add = b.step_add;
  r.h1 = e->cv[c].h1; r.h2 = e->cv[c].h2; r.keep = true; r.q = e->q[c];
  return r;
}
// target critic c on [next_action | next_state].  whole: the packed row as one segment; otherwise the state part first, then the action
// columns (the order of mlps.hip's chained form, whose state part does not wait for the target actor)
Role role_target_critic(const recnn_engine* e, const StepBufs& b, int c, bool whole) {
  Role r{TVAL[c], b.xn, e->ldx, e->K1c, 0};
  if (!whole) {
    r.A0 = b.xn + tc_off(e, e->A); r.K0 = e->K1a; r.col0 = e->A;
    r.A1 = b.xn; r.lda1 = e->ldx; r.K1 = e->Ap; r.col1 = 0;
  }
  r.step_add = b.step_add;
  r.h1 = b.tq_h1[c]; r.h2 = b.tq_h2[c]; r.q = b.tq[c];
  return r;
}
// policy-loss critic: critic 1 on [pi(s) | s], two contraction segments over the rotated W1 shadow.  (gen_action is zero padded to Ap
// columns, so segment 0 may run over the padded width: the W1 shadow columns it meets there are multiplied by zeros.)
Role role_policy_critic(const recnn_engine* e, const char* xs, const char* ga, int step_add) {
  Role r{RECNN_NET_VALUE1, ga, e->Ap, e->Ap, 0};
  r.A1 = xs + tc_off(e, e->A); r.lda1 = e->ldx; r.K1 = e->K1a; r.col1 = e->A;
  r.mask_idx = e->td3 ? 6 : 4; r.step_add = step_add;
  r.h1 = e->pc.h1; r.h2 = e->pc.h2;
  return r;
}
// ... of the PREVIOUS step of this run, riding in this step's forward (run graphs: nothing of this or later steps depends on it, the
// weights are as that step's optimizer left them = the current ones): that step's batch and mask key, Q into that step's pl_part slot
Role role_deferred_critic(const recnn_engine* e) {
  const recnn_engine::PendingPc& pp = e->pending_pc;
  Role r = role_policy_critic(e, pp.xs, pp.ga, pp.run_off);
  r.q = e->pl_part_base + (int64_t)pp.slot * e->pl_cap;
  return r;
}
// the partial sums of a step's policy loss (sums of Q, b3 included) as the loss history will read them
int note_policy_parts(recnn_engine* e, int slot, int parts) {
  RECNN_REQUIRE(parts > 0 && parts <= e->pl_cap, "policy loss: %d partial sums do not fit %d", parts, e->pl_cap);
  if (slot < LOSS_HIST_MAX) { e->hist_pol_count[slot] = parts; e->hist_pol_add[slot] = 0; }
  return 0;
}

// ---- GEMM problem builders ---------------------------------------------------------------
struct FwdSpec {
  int ni;               // network whose weights are used
  int layer;            // 1, 2, 3
  const void* A; int64_t lda; int a_f32; int K;         // segment 0 input
  const void* A2 = nullptr; int64_t lda2 = 0; int K2 = 0; int b2_col = 0;  // optional second segment (B column offset)
  int b_col = 0;        // column offset into the W shadow for segment 0
  void* C; int64_t ldc; int c_f32;
  int relu;
  int mask_idx;         // -1 = none
  int step_add = -1;    // mask key step on top of the device counter; -1 = e->run_off
  const float* addend = nullptr; int64_t ld_add = 0; float add_clip = 0.f;
};

double fill_fwd(const recnn_engine* e, const FwdSpec& f, int rows, GemmProb* p) {
  const Net& n = e->net[f.ni];
  gemm_prob_init(p);
  const int wi = f.layer == 1 ? W1 : (f.layer == 2 ? W2 : W3);
  const int bi = wi + 1;
  const int ldw = f.layer == 1 ? n.ld_w1 : (f.layer == 2 ? n.ld_w2 : n.ld_w3);
  char* w = sh_ptr(e, f.ni, wi);
  p->seg[0].A = f.A; p->seg[0].lda = f.lda; p->seg[0].K = f.K;
  p->seg[0].B = w + tc_off(e, f.b_col); p->seg[0].ldb = ldw;
  p->nseg = 1;
  if (f.A2) {
    p->seg[1].A = f.A2; p->seg[1].lda = f.lda2; p->seg[1].K = f.K2;
    p->seg[1].B = w + tc_off(e, f.b2_col); p->seg[1].ldb = ldw;
    p->nseg = 2;
  }
  p->M = rows;
  p->N = f.layer == 3 ? n.out_dim : e->H;
  p->C = f.C; p->ldc = f.ldc; p->c_f32 = f.c_f32;
  p->bias = n.p + n.off[bi];
  p->relu = f.relu;
  const MaskSel m = mask_sel(e, f.mask_idx, f.step_add < 0 ? e->run_off : f.step_add);
  p->mask_mode = m.mode; p->mask = m.ext; p->ld_mask = m.pitch;
  p->seed = m.seed; p->stream_id = m.stream; p->step_ptr = m.step_ptr; p->step_add = m.step_add;
  p->addend = f.addend; p->ld_add = f.ld_add; p->add_clip = f.add_clip;
  const double kreal = f.layer == 1 ? n.in_dim : e->H;
  return 2.0 * rows * p->N * kreal;
}
// layer 1 of a role from its input segments, layer 2 from its h1, layer 3 (an actor's) from its h2
FwdSpec role_layer(const recnn_engine* e, const Role& r, int layer) {
  const int Hp = e->Hp;
  FwdSpec f{r.ni, layer, layer == 1 ? r.A0 : (layer == 2 ? r.h1 : r.h2), layer == 1 ? r.lda0 : Hp, 0, layer == 1 ? r.K0 : Hp};
  f.c_f32 = 0; f.step_add = r.step_add;
  if (layer == 1) {
    f.b_col = r.col0;
    if (r.A1) { f.A2 = r.A1; f.lda2 = r.lda1; f.K2 = r.K1; f.b2_col = r.col1; }
    f.C = r.h1; f.ldc = Hp; f.relu = 1; f.mask_idx = r.mask_idx;
  } else if (layer == 2) {
    f.C = r.h2; f.ldc = Hp; f.relu = 1; f.mask_idx = mask2_idx(r.mask_idx);
  } else {
    f.C = r.out; f.ldc = r.ldo; f.relu = 0; f.mask_idx = -1;
    f.addend = r.addend; f.ld_add = r.ld_add; f.add_clip = r.add_clip;
  }
  return f;
}

struct Group {
  GemmLaunch L;
  double flops = 0.0;
  recnn_engine* eng;
  Group(recnn_engine* e, int mode, int a_f32, int b_f32) : eng(e) {
    memset(&L, 0, sizeof(L));
    L.dtype = e->cfg.dtype; L.mode = mode;
    L.a_f32 = e->bf16 ? a_f32 : 0;
    L.b_f32 = e->bf16 ? b_f32 : 0;
    L.nprob = 0;
    L.tune = &e->gtune;
  }
  GemmProb* add() { return &L.batch.p[L.nprob++]; }
  GemmProb* add(double fl) { flops += fl; return &L.batch.p[L.nprob++]; }
  int run(hipStream_t s, const char* name = "gemm") {
    return slot(eng, name, flops, s, [&] { return gemm_launch(&L, s); });
  }
};

GemmProb* add_layer(Group& g, const Role& r, int layer, int rows) {
  GemmProb* p = g.add();
  g.flops += fill_fwd(g.eng, role_layer(g.eng, r, layer), rows, p);
  return p;
}
// One layer of several roles as one GEMM launch (layer 3: of those that have an output, the actors).  dot: one more layer-2 problem whose
// sums of Q -- the last layer's dot, b3 included -- come out of the epilogue as partial sums in dot->q (a policy-loss critic);
// *dot_parts = how many it wrote, -1 if the group had no room for it.
int fwd_layer(recnn_engine* e, int rows, int layer, const Role* r, int n, const char* name, hipStream_t s, const Role* dot = nullptr,
              int* dot_parts = nullptr) {
  Group g(e, GEMM_FWD, 0, 0);
  for (int i = 0; i < n; ++i)
    if (layer < 3 || r[i].out) add_layer(g, r[i], layer, rows);
  int di = -1;
  if (dot && g.L.nprob < GEMM_MAX_GROUP) {
    const NetView v = net_view(e, dot->ni);
    di = g.L.nprob;
    GemmProb* p = add_layer(g, *dot, 2, rows);
    p->dot_w = v.w3row; p->dot_bias = v.b3; p->dot_part = dot->q;
  }
  const int rc = g.run(s, name);
  if (!rc && dot_parts) *dot_parts = di >= 0 ? g.L.batch.p[di].dot_parts : -1;
  return rc;
}

// dX problem: C[rows, N] = (A[rows, Kc] * Wshadow[Kc, N(+col0)]) * scale*[yref>0]
double fill_dx(const recnn_engine* e, GemmProb* p, int rows, const void* A, int64_t lda, int Kc, int ni, int which, int col0,
             int N, void* C, int64_t ldc, const void* yref, int64_t ldy, float* colsum) {
  const Net& n = e->net[ni];
  gemm_prob_init(p);
  const int ldw = which == W1 ? n.ld_w1 : (which == W2 ? n.ld_w2 : n.ld_w3);
  p->seg[0].A = A; p->seg[0].lda = lda; p->seg[0].K = Kc;
  p->seg[0].B = sh_ptr(e, ni, which) + tc_off(e, col0); p->seg[0].ldb = ldw;
  p->M = rows; p->N = N;
  p->C = C; p->ldc = ldc; p->c_f32 = 0;
  p->yref = yref; p->ldy = ldy;
  p->dx_scale = yref ? (e->cfg.mask_mode != RECNN_MASK_NONE ? 2.0f : 1.0f) : 1.0f;
  p->colsum = colsum;
  const double kreal = (which == W3) ? n.out_dim : e->H;
  return 2.0 * rows * N * kreal;
}

// dW problem: slabs[s][M, valid] = dZ[rows, M]^T * X[rows, N]
double fill_dw(const recnn_engine* e, GemmProb* p, int rows, const void* dz, int64_t ldz, int M, const void* X, int64_t ldx_,
             int valid_cols, int rot, float* slabs, int splits, int64_t slab_stride) {
  gemm_prob_init(p);
  p->seg[0].A = dz; p->seg[0].lda = ldz; p->seg[0].K = rows;
  p->seg[0].B = X; p->seg[0].ldb = ldx_;
  p->M = M; p->N = valid_cols;
  p->C = slabs; p->ldc = valid_cols; p->c_f32 = 1;
  p->dw_splits = splits; p->dw_slab_stride = slab_stride;
  p->dw_valid_cols = valid_cols; p->dw_col_rot = rot;
  return 2.0 * rows * M * valid_cols;
}

int check_ready(recnn_engine* e, int rows) {
  RECNN_REQUIRE(e, "engine: null");
  RECNN_REQUIRE(rows > 0 && rows <= e->cfg.max_rows, "engine: rows=%d outside [1, %d]", rows, e->cfg.max_rows);
  RECNN_REQUIRE(e->xs && e->xn, "engine: batch buffers not bound");
  RECNN_REQUIRE(e->hyper_set, "engine: hyper-parameters not set");
  for (int ni = 0; ni < RECNN_NET_COUNT; ++ni)
    if (net_used(e, ni)) RECNN_REQUIRE(e->net[ni].bound, "engine: network %d not bound", ni);
  if (e->cfg.mask_mode == RECNN_MASK_EXTERNAL) RECNN_REQUIRE(e->ext_masks, "engine: external masks not bound");
  return 0;
}

// ---- per-engine tuning (include/recnn_hip.h recnn_engine_tuning): every field selects among schedules / tile shapes that
// produce the same numbers.  What the measured-slower variants of earlier rounds taught is recorded in profiles/NOTES_r01_r05.md 5c, not kept in
// the binary: the optimizer in the dW launch's epilogue (26.7 vs 18.7 us), an XCD-affine workgroup map of the fused forward
// (-11 MB of HBM traffic, +6 us), the cycle gather on a side branch of the run graph (67.5 vs 61.5 us/step), the learning
// critic's step forward as one fused launch in cycle mode (67.4 vs 65.1 us/step), padded leading dimensions (no effect).
//   fused_mlp: 0 = never, 1 = groups of >= 3 networks (a single network only occupies 64 CUs and streams its whole W1 per
//     workgroup: the tiled kernels are faster there), 2 = every forward
//   split_fwd: 0 = the fused row-panel kernel (mlps.hip) everywhere; 1 (default) = run graphs of at least cycle_min_len steps
//     run in CYCLE MODE (capture_run: the batches of a policy cycle gathered at once, the frozen networks applied to all of
//     them by mlpf.hip, per-step launches = split forward of the learning critics: l1gemm.hip + mlpt.hip); 2 = split forward and
//     cycle mode everywhere.  Measured (round 3, DDPG 2048 rows): sustained 61.2-61.5 us/step in cycle mode vs 62.9-63.2 fused;
//     a 20-step graph (the driver's command) 74.7 vs 69.9 -- three partial cycles do not pay there.
//   bwd_panel: 0 = head + dX launches, 1 = row-panel launch (bwd.hip), 2 = inside the critic's forward workgroup (mlps.hip)
extern "C" void recnn_engine_tuning_init(recnn_engine_tuning* t) {
  if (!t) return;
  memset(t, 0, sizeof(*t));
  t->fused_mlp = 1; t->chain_target_critic = 1; t->bwd_panel = 2; t->policy_chain = 1;
  t->split_fwd = 1; t->cycle_min_len = 20; t->cycle_min_seg = 4; t->frozen_fused = 1; t->frozen_gemm = 1;
  t->graph_run = -1; t->pregather = 1; t->defer_policy_fwd = 1;
  t->sampler_f32_rows = 0; t->dw_splits = 8; t->comm_fused = 1; t->l1_big = 1;
  t->gemm_variant = -1; t->gemm_v0_threshold = 512; t->gemm_dma = 1; t->gemm_dma_depth = 1; t->gemm_dma_waves = 8;
  t->gemm_waves = 8; t->dw_dma = 2; t->x3_tail = 1; t->x3_fwd = 2; t->dw_fuse = 1; t->tail_half = 1; t->l1_ws = 1; t->frozen_half = 1;
  t->frozen_window = 1;
  t->run_align = 1; t->frozen_acts_policy_only = 1;
  t->gather_cycle = 1;
  t->policy_fused = 3;
}
extern "C" int recnn_engine_set_tuning(recnn_engine* e, const recnn_engine_tuning* t) {
  RECNN_REQUIRE(e && t, "set_tuning: null pointer");
  e->tune = *t;
  recnn_engine_tuning& u = e->tune;
  u.dw_splits = u.dw_splits < 1 ? 1 : (u.dw_splits > SP_W1_MAX ? SP_W1_MAX : u.dw_splits);
  u.cycle_min_len = u.cycle_min_len < 2 ? 2 : u.cycle_min_len;
  u.cycle_min_seg = u.cycle_min_seg < 1 ? 1 : u.cycle_min_seg;
  u.l1_big = u.l1_big == 2 ? 2 : 1;
  sync_gemm_tune(e);
  drop_graphs(e);
  return 0;
}
extern "C" int recnn_engine_get_tuning(recnn_engine* e, recnn_engine_tuning* t) {
  RECNN_REQUIRE(e && t, "get_tuning: null pointer");
  *t = e->tune;
  return 0;
}

// bf16 value side on the fully fused path: target critics chained inside the forward launch (Q and Q' arrive as
// per-row scalars), critic head + first backward GEMM in one row-panel launch (bwd.hip)
bool value_chain_ok(const recnn_engine* e) {
  return e->tune.fused_mlp && e->tune.chain_target_critic && e->bf16 && e->Hp == 256 && e->Ap == 128 && e->A == e->Ap;
}
bool value_panel_ok(const recnn_engine* e) { return value_chain_ok(e) && e->tune.bwd_panel; }

bool fused_mlp_ok(const recnn_engine* e, int nprob) {
  return e->tune.fused_mlp && e->bf16 && e->Hp == 256 && e->Ap == 128 && (nprob >= 3 || e->tune.fused_mlp >= 2);
}

// a role's whole network as a problem of the fused row-panel launch (mlps.hip)
double fill_mlp(const recnn_engine* e, const Role& f, int rows, MlpProb* p) {
  const Net& n = e->net[f.ni];
  const NetView v = net_view(e, f.ni);
  memset(p, 0, sizeof(*p));
  p->A[0] = f.A0; p->lda[0] = f.lda0; p->K[0] = f.K0; p->w1_col[0] = f.col0;
  p->nseg = 1;
  if (f.A1) { p->A[1] = f.A1; p->lda[1] = f.lda1; p->K[1] = f.K1; p->w1_col[1] = f.col1; p->nseg = 2; }
  p->W1 = v.W1; p->ldw1 = v.ldw1; p->W2 = v.W2; p->ldw2 = v.ldw2; p->W3 = v.W3; p->ldw3 = v.ldw3;
  p->b1 = v.b1; p->b2 = v.b2; p->b3 = v.b3; p->w3row = v.w3row;
  p->rows = rows; p->H = e->H; p->out_dim = n.out_dim;
  const MaskSel m1 = mask_sel(e, f.mask_idx, f.step_add), m2 = mask_sel(e, mask2_idx(f.mask_idx), f.step_add);
  p->mask_mode = m1.mode; p->mask1 = m1.ext; p->mask2 = m2.ext; p->ld_mask = m1.pitch;
  p->seed = m1.seed; p->stream1 = m1.stream; p->stream2 = m2.stream; p->step_ptr = m1.step_ptr; p->step_add = m1.step_add;
  p->h1 = f.keep ? f.h1 : nullptr; p->h2 = f.keep ? f.h2 : nullptr; p->ldh = e->Hp;
  p->out = f.out; p->ldo = f.ldo;
  p->q = f.q;
  p->cbwd_idx = -1;
  p->addend = f.addend; p->ld_add = f.ld_add; p->add_clip = f.add_clip;
  return 2.0 * rows * ((double)e->H * n.in_dim + (double)e->H * e->H + (double)n.out_dim * e->H);
}

// ---- the TD head of the learning critics (recnn/nn/update/misc.py:6-7,33-39, td3.py:83-93), whichever launch evaluates it:
// y = r + (1 - done) gamma min_t Q'_t clamped to [lo, hi] (TD3: not clamped), d_c = 2 (Q_c - y) / rows, loss partials; value_bwd: the
// small tensors' gradient partial sums go to the critics' slabs
struct TdDesc {
  int nc;
  const float *reward, *done;
  float gamma, lo, hi;
  float *expected, *target_q;
  float *tq[2], *q[2], *delta[2], *loss_part[2];
  bool train; float scale;                                         // the backward's relu gates times 2 when dropout is active
  float *dw3_part[2], *db2_part[2], *db1_part[2], *db3_part[2];    // NULL: no parameter gradients wanted
};
int td_desc(recnn_engine* e, bool value_bwd, TdDesc* d) {
  memset(d, 0, sizeof(*d));
  d->nc = e->n_critic;
  d->reward = e->reward; d->done = e->done; d->gamma = e->hy.gamma;
  d->lo = e->td3 ? -INFINITY : e->hy.min_value;
  d->hi = e->td3 ? INFINITY : e->hy.max_value;
  d->expected = e->expected; d->target_q = e->target_q;
  d->train = e->cfg.mask_mode != RECNN_MASK_NONE;
  d->scale = d->train ? 2.0f : 1.0f;
  for (int c = 0; c < d->nc; ++c) {
    const Net& v = e->net[VAL[c]];
    d->tq[c] = e->tqv[c]; d->q[c] = e->q[c]; d->delta[c] = e->delta[c]; d->loss_part[c] = e->loss_part[c];
    if (value_bwd) {
      RECNN_REQUIRE(v.g, "value backward: network %d has no gradient arena bound", VAL[c]);
      d->dw3_part[c] = v.gp[W3]; d->db2_part[c] = v.gp[B2]; d->db1_part[c] = v.gp[B1]; d->db3_part[c] = v.gp[B3];
    }
  }
  return 0;
}
// ... into critic c's problem of the split forward's tail launch (mlpt.hip)
void td_write(const TdDesc& d, int c, TailProb* p) {
  p->n_target = d.nc;
  for (int t = 0; t < d.nc; ++t) p->tq[t] = d.tq[t];
  p->reward = d.reward; p->done = d.done; p->gamma = d.gamma; p->lo = d.lo; p->hi = d.hi;
  if (c == 0) { p->expected = d.expected; p->target_q = d.target_q; }
  p->delta_out = d.delta[c]; p->loss_part = d.loss_part[c];
  p->scale = d.scale;
  p->dw3_part = d.dw3_part[c]; p->db2_part = d.db2_part[c]; p->db1_part = d.db1_part[c]; p->db3_part = d.db3_part[c];
}
// ... into the head the target actor's workgroup evaluates inside the fused forward (mlps.hip); Q arrives through the hand-off slots
void td_write(const TdDesc& d, const recnn_engine* e, MlpHead* h) {
  h->n_critic = d.nc;
  for (int c = 0; c < d.nc; ++c) {
    h->q_slot[c] = e->q_slot[c];
    h->delta_out[c] = d.delta[c]; h->loss_part[c] = d.loss_part[c];
    h->db3_part[c] = d.db3_part[c];
  }
  h->reward = d.reward; h->done = d.done; h->gamma = d.gamma; h->lo = d.lo; h->hi = d.hi;
  h->expected = d.expected; h->target_q = d.target_q;
}
// ... into critic c's problem of the row-panel backward launch (bwd.hip, mode 0)
void td_write(const TdDesc& d, int c, BwdPanelProb* b) {
  b->q = d.q[c]; b->n_target = d.nc;
  for (int t = 0; t < d.nc; ++t) b->tq[t] = d.tq[t];
  b->reward = d.reward; b->done = d.done; b->gamma = d.gamma; b->lo = d.lo; b->hi = d.hi;
  if (c == 0) { b->expected = d.expected; b->target_q = d.target_q; }
  b->delta_out = d.delta[c]; b->loss_part = d.loss_part[c];
  b->scale = d.scale;
  b->dw3_part = d.dw3_part[c]; b->db2_part = d.db2_part[c]; b->db3_part = d.db3_part[c]; b->colsum = d.db1_part[c];
}
// ... into the head launch (head.hip)
void td_write(const TdDesc& d, HeadArgs* h) {
  h->n_target = d.nc; h->n_critic = d.nc;
  for (int c = 0; c < d.nc; ++c) {
    h->q[c] = d.q[c]; h->delta[c] = d.delta[c]; h->loss_part[c] = d.loss_part[c];
    h->dw3_part[c] = d.dw3_part[c]; h->db2_part[c] = d.db2_part[c]; h->db3_part[c] = d.db3_part[c];
  }
  h->reward = d.reward; h->done = d.done; h->gamma = d.gamma; h->lo = d.lo; h->hi = d.hi;
  h->expected = d.expected; h->target_q = d.target_q;
  h->train = d.train;
}

// ------------------------------------------------------------------------------------ phases
// TD3's target-action noise (td3.py:74-78) for n_sets consecutive batches of `rows` rows, batch j under the key of step + step_add + j;
// nothing to launch for DDPG or when the caller supplies the noise
int ph_td3_noise(recnn_engine* e, float* out, int rows, int step_add, int n_sets, hipStream_t s) {
  if (!e->td3 || e->ext_noise) return 0;
  return slot(e, "td3_noise", 0, s, [&] { return noise_fill_launch(out, (int64_t)rows * e->A, e->hy.noise_std, e->cfg.seed, e->counters, step_add, s, n_sets); });
}

// The head launch: TD target, Q, dQ, loss partials (+ with value_bwd: dz2 and the last layer's gradient partials) from the layer-2
// activations of the critics and target critics.  tq_ready: Q' per row came out of an earlier launch.
int ph_td_head(recnn_engine* e, int rows, bool value_bwd, bool tq_ready, hipStream_t s) {
  TdDesc td;
  int rc;
  if ((rc = td_desc(e, value_bwd, &td))) return rc;
  HeadArgs h;
  memset(&h, 0, sizeof(h));
  h.rows = rows; h.H = e->H; h.tc_bf16 = e->cfg.dtype; h.ld_h = e->Hp;
  td_write(td, &h);
  for (int c = 0; c < td.nc; ++c) {
    const NetView t = net_view(e, TVAL[c]), v = net_view(e, VAL[c]);
    h.th2[c] = e->tq[c].h2; h.tw3[c] = t.w3row; h.tb3[c] = t.b3;
    if (tq_ready) h.tq_in[c] = e->tqv[c];
    h.ch2[c] = e->cv[c].h2; h.cw3[c] = v.w3row; h.cb3[c] = v.b3;
    if (value_bwd) h.dz2[c] = e->dzc2[c];
  }
  h.policy_mode = 0;
  h.do_bwd = value_bwd;
  const GatherArgs* hg = (value_bwd && e->head_gather) ? e->head_gather : nullptr;   // (armed by step_impl: the next step's gather rides here)
  if ((rc = slot(e, hg ? "head_td_target+gather" : "head_td_target", 0, s, [&] { return head_launch(h, s, hg); }, hg == nullptr))) return rc;
  if (hg) e->head_gather = nullptr;         // consumed
  return 0;
}

// The policy loss's backward seed d = -1/B for every row through the critic's last two layers: dz_e2 and dz_e1 in one row-panel launch
// (bwd.hip, mode 1), no critic parameter gradients
int ph_head_dx_pcritic(recnn_engine* e, int rows, hipStream_t s) {
  BwdPanelBatch bb;
  memset(&bb, 0, sizeof(bb));
  BwdPanelProb& b = bb.p[0];
  const NetView v = net_view(e, RECNN_NET_VALUE1);
  b.rows = rows; b.H = e->H; b.mode = 1; b.delta_const = -1.0f / (float)rows;
  b.h2 = e->pc.h2; b.ldh = e->Hp; b.w3 = v.w3row; b.scale = e->cfg.mask_mode != RECNN_MASK_NONE ? 2.0f : 1.0f;
  b.dz2 = e->dze2; b.W2 = v.W2; b.ldw2 = v.ldw2; b.h1 = e->pc.h1; b.dz1 = e->dze1;
  return slot(e, "head_dx_pcritic", 2.0 * rows * (double)e->H * e->H, s, [&] { return bwd_panel_launch(bb, 1, s); });
}

// ---- split forward (split.h): a role's layer 1 as a problem of the tiled launch (l1gemm.hip), its layers 2 / 3 of the tail launch (mlpt.hip)
void fill_l1(const recnn_engine* e, L1Prob* p, const Role& f, int rows) {
  const NetView v = net_view(e, f.ni);
  memset(p, 0, sizeof(*p));
  p->A[0] = f.A0; p->lda[0] = f.lda0; p->K[0] = f.K0; p->w1_col[0] = f.col0; p->nseg = 1;
  if (f.A1) { p->A[1] = f.A1; p->lda[1] = f.lda1; p->K[1] = f.K1; p->w1_col[1] = f.col1; p->nseg = 2; }
  p->W1 = v.W1; p->ldw1 = v.ldw1;
  p->b1 = v.b1;
  p->rows = rows; p->H = e->H;
  const MaskSel m = mask_sel(e, f.mask_idx, f.step_add);
  p->mask_mode = m.mode; p->mask = m.ext; p->ld_mask = m.pitch;
  p->seed = m.seed; p->stream = m.stream; p->step_ptr = m.step_ptr; p->step_add = m.step_add;
  p->h1 = f.h1; p->ldh = e->Hp;
}
// (TailProb and the split-bf16 type's X3TailProb name what they share alike)
template <class P> void fill_layers23(const recnn_engine* e, P* p, const Role& f, int rows) {
  const NetView v = net_view(e, f.ni);
  memset(p, 0, sizeof(*p));
  p->h1 = f.h1; p->ldh = e->Hp;
  p->W2 = v.W2; p->ldw2 = v.ldw2; p->W3 = v.W3; p->ldw3 = v.ldw3;
  p->b2 = v.b2; p->b3 = v.b3; p->w3row = v.w3row;
  p->rows = rows; p->H = e->H; p->out_dim = e->net[f.ni].out_dim;
  const MaskSel m = mask_sel(e, mask2_idx(f.mask_idx), f.step_add);
  p->mask_mode = m.mode; p->mask2 = m.ext; p->ld_mask = m.pitch;
  p->seed = m.seed; p->stream2 = m.stream; p->step_ptr = m.step_ptr; p->step_add = m.step_add;
  p->h2 = f.keep ? f.h2 : nullptr;
  p->out = f.out; p->ldo = f.ldo;
  p->addend = f.addend; p->ld_add = f.ld_add; p->add_clip = f.add_clip;
  p->q = f.q;
}
void fill_tail(const recnn_engine* e, TailProb* p, int kind, const Role& f, int rows) {
  fill_layers23(e, p, f, rows);
  p->kind = kind;
}

// The forward of one step, split (e->tune.split_fwd): frozen networks first (target actor -> target critics on its action; the
// actor), then the learning critics with the TD head and their layer-2 backward in their own workgroups.  Six launches here;
// inside run graphs the frozen half is hoisted out of the step and applied to a whole policy cycle at once (capture_run).
int ph_forward_split(recnn_engine* e, int rows, bool value_side, bool actor_side, bool value_bwd, hipStream_t s, bool frozen_done = false) {
  const int A = e->A, nc = e->n_critic;
  const StepBufs B = step_bufs(e);
  const double l1_fl_a = 2.0 * rows * (double)e->H * e->S, l1_fl_c = 2.0 * rows * (double)e->H * (e->S + A);
  const double t_fl_a = 2.0 * rows * ((double)e->H * e->H + (double)A * e->H), t_fl_c = 2.0 * rows * ((double)e->H * e->H + e->H);
  int rc = 0;
  if (!frozen_done && value_side && (rc = ph_td3_noise(e, e->noise_buf, rows, e->run_off, 1, s))) return rc;
  if (!frozen_done) {  // ---- frozen networks: target actor on s', actor on s
    L1Batch lb;
    TailBatch tb;
    int np = 0;
    double fl = 0, tfl = 0;
    if (value_side) {
      const Role r = role_target_actor(e, B);
      fill_l1(e, &lb.p[np], r, rows); fill_tail(e, &tb.p[np++], TAIL_ACTOR, r, rows);
      fl += l1_fl_a; tfl += t_fl_a;
    }
    if (actor_side) {
      const Role r = role_actor(e, B);
      fill_l1(e, &lb.p[np], r, rows); fill_tail(e, &tb.p[np++], TAIL_ACTOR, r, rows);
      fl += l1_fl_a; tfl += t_fl_a;
    }
    if (np && (rc = slot(e, "l1_actors", fl, s, [&] { return l1gemm_launch(lb, np, 0, s, e->tune.l1_ws); }))) return rc;
    if (np && (rc = slot(e, "tail_actors", tfl, s, [&] { return mlpt_launch(tb, np, s); }))) return rc;
  }
  e->panel_bwd_done = false;
  e->split_critics = false;
  e->unit_bwd = false;
  e->half_panels = false;
  if (!value_side) return 0;
  // 16-row panels for the learning critics' tail (tuning.tail_half): whole 32-row pairs only, and the consumers of its panel sums must
  // be the pair-aware ones (the optimizer launches; not grad_reduce's callers that read gp[] directly -- there are none)
  // ... and only while the launch still fits the machine in ONE round of workgroups (one 152 KB workgroup per CU): 2 nc (rows / 32) half panels
  // + rows / 32 panels of the deferred policy-loss critic <= 256.  DDPG at 2048 rows: 192 (53.9 vs 57.3 us/step); TD3 at 4096 rows would be
  // 640 -- measured 130.5 vs 124.1 us/step with 32-row panels (profiles/NOTES_r06.md)
  const bool half = e->tune.tail_half && value_bwd && rows % 32 == 0 && (2 * nc + 1) * (rows / 32) <= 256;
  if (!frozen_done) {  // ---- target critics on [next_state | next_action]
    L1Batch lb;
    TailBatch tb;
    double fl = 0, tfl = 0;
    for (int c = 0; c < nc; ++c) {
      const Role r = role_target_critic(e, B, c, false);
      fill_l1(e, &lb.p[c], r, rows); fill_tail(e, &tb.p[c], TAIL_CRITIC_Q, r, rows);
      fl += l1_fl_c; tfl += t_fl_c;
    }
    if ((rc = slot(e, "l1_target_critic", fl, s, [&] { return l1gemm_launch(lb, nc, 0, s, e->tune.l1_ws); }))) return rc;
    if ((rc = slot(e, "tail_target_critic", tfl, s, [&] { return mlpt_launch(tb, nc, s); }))) return rc;
  }
  {  // ---- learning critics (+ the previous step's policy-loss forward riding along: same weights, the previous batch)
    L1Batch lb;
    TailBatch tb;
    int np = 0;
    double fl = 0, tfl = 0;
    TdDesc td;
    if ((rc = td_desc(e, value_bwd, &td))) return rc;
    for (int c = 0; c < nc; ++c) {
      const Role r = role_critic(e, B, c);
      fill_l1(e, &lb.p[np], r, rows);
      TailProb* p = &tb.p[np++];
      fill_tail(e, p, TAIL_CRITIC_LEARN, r, rows);
      td_write(td, c, p);
      p->half_panels = half;
      p->dz2 = e->dzc2[c]; p->dz1 = e->dzc1[c];
      fl += l1_fl_c; tfl += t_fl_c + 2.0 * rows * (double)e->H * e->H;
    }
    if (e->pending_pc.on && np < L1_MAX_GROUP) {
      const Role r = role_deferred_critic(e);
      fill_l1(e, &lb.p[np], r, rows); fill_tail(e, &tb.p[np++], TAIL_CRITIC_Q, r, rows);
      fl += l1_fl_c; tfl += t_fl_c;
      e->pending_pc.on = false;
    }
    // 64 x 64 tiles while they fit two rounds of workgroups; beyond that (TD3 at 4096 rows: 3 problems x 256 tiles = three rounds of 8 us)
    // the 128 x 128 form -- a quarter of the workgroups, twice the stream each: one round (122.35 -> 120.1 us/step, A/B in one call)
    const int tiles64 = np * ((rows + 63) / 64) * 4;
    const int big = tiles64 > 512 ? 1 : 0;
    if ((rc = slot(e, "l1_critic", fl, s, [&] { return l1gemm_launch(lb, np, big, s, e->tune.l1_ws); }))) return rc;
    if ((rc = slot(e, "tail_critic", tfl, s, [&] { return mlpt_launch(tb, np, s); }))) return rc;
  }
  e->panel_bwd_done = true;     // dz2 / dz1 (already times the per-row loss seed) and the small tensors' panel sums exist
  e->split_critics = true;
  e->half_panels = half;
  return 0;
}

// layers 2 (+ 3) of a role as a problem of the split-bf16 row-panel launch (x3tail.hip)
void fill_x3tail(const recnn_engine* e, X3TailProb* p, const Role& f, int rows) { fill_layers23(e, p, f, rows); }
bool x3_tail_ok(const recnn_engine* e) {
  return e->x3 && e->tune.x3_tail && e->H == 256 && e->Hp == 512 && e->A == 128 && e->net[RECNN_NET_POLICY].ld_w2 == e->net[RECNN_NET_POLICY].ld_w3;
}


// The forward of one step in the split-bf16 type (x3.h): layer-by-layer GEMM launches like the fp32 path, arranged so that every
// launch is as full as the data dependencies allow (each launch streams its tiles at one CU's L2 -> LDS rate: time = bytes / CUs):
//   L1  {target actor(s'), critic(s, a), actor(s), target critic STATE part (raw fp32, 1290 of its 1418 k: it does not depend on
//        the target actor), [the previous step's policy-loss critic on [pi(s) | s]: deferred, run graphs]}
//   L2  {target actor, critic, actor, [deferred policy-loss critic, the loss summed in the epilogue]}
//   L3  {target actor -> next_action (+ TD3 noise), actor -> gen_action}
//   L1' target critic: relu(state part + next_action W1[:, action columns]^T + b1)      (k = 128)
//   L2' target critic        then the head launch (TD target, Q dots, loss partials, dz2).
// recnn/nn/update/misc.py:27-39, td3.py:73-93, ddpg.py:78-79 (deferred), same arithmetic as ph_forward's generic branch up to the
// summation order of the target critic's layer 1.
int ph_forward_x3(recnn_engine* e, int rows, bool value_side, bool actor_side, bool value_bwd, hipStream_t s) {
  const int A = e->A, Hp = e->Hp, nc = e->n_critic;
  const int ldp = e->Hl > 256 ? e->Hl : 256;     // row pitch of the fp32 layer-1 parts
  int rc;
  const bool pend = e->pending_pc.on;
  const int pend_slot = e->pending_pc.slot;
  Role pc{};                                     // the deferred policy-loss critic on [pi(s) | s] of the previous batch
  if (pend) pc = role_deferred_critic(e);
  e->pending_pc.on = false;
  // DDPG's first launch is exactly one round of 64 x 128 tiles on 256 CUs without the deferred policy-loss critic (4 problems x 64
  // tiles); a fifth problem would cost a whole second round (measured 44.6 us against ~28).  It rides with the target critic's
  // k = 128 launch and panel tail instead, which fill a quarter of the machine.  (TD3's first launch is two rounds either way.)
  const bool pend_late = pend && value_side && !e->td3 && x3_tail_ok(e);
  const StepBufs B = step_bufs(e);
  Role net[4], tc[2] = {};                       // target actor, critics, actor: the order of every launch that carries them
  int nn = 0;
  if (value_side) {
    net[nn++] = role_target_actor(e, B);
    for (int c = 0; c < nc; ++c) {
      net[nn] = role_critic(e, B, c);
      net[nn++].q = nullptr;                     // (Q comes out of the head launch here)
      tc[c] = role_target_critic(e, B, c, false);
    }
  }
  if (actor_side) net[nn++] = role_actor(e, B);
  auto pc_tail = [&](X3TailProb* p) -> int {     // ... its sums of Q per panel into that step's policy-loss slot
    fill_x3tail(e, p, pc, rows);
    p->q = nullptr; p->q_part = pc.q;
    return note_policy_parts(e, pend_slot, ((rows + 31) / 32) * x3tail_parts_per_panel());
  };
  {  // ---- L1
    Group g(e, GEMM_FWD, 0, 0);
    for (int i = 0; i < nn; ++i) add_layer(g, net[i], 1, rows);
    for (int c = 0; c < nc && value_side; ++c) {   // state columns of the target critic's W1 shadow ([action | state] order): raw fp32, no bias
      FwdSpec f{tc[c].ni, 1, tc[c].A0, tc[c].lda0, 0, tc[c].K0};
      f.b_col = tc[c].col0;
      f.C = e->tc_part[c]; f.ldc = ldp; f.c_f32 = 1; f.relu = 0; f.mask_idx = -1;
      GemmProb* p = g.add();
      fill_fwd(e, f, rows, p);
      p->bias = nullptr;
      g.flops += 2.0 * rows * (double)e->H * e->S;
    }
    if (pend && !pend_late && g.L.nprob < GEMM_MAX_GROUP) add_layer(g, pc, 1, rows);
    if ((rc = g.run(s, "fwd_l1"))) return rc;
  }
  const bool tails = x3_tail_ok(e);
  if (value_side && (rc = ph_td3_noise(e, e->noise_buf, rows, e->run_off, 1, s))) return rc;
  if (tails) {
    // ---- layers 2 + 3 of everything whose layer 1 exists, ONE launch of 32-row panels (x3tail.hip): target actor -> next_action
    // (+ TD3 noise), critics -> h2 (the head and the backward read it), actor -> h2, gen_action, deferred policy-loss critic -> sums of Q
    X3TailBatch tb;
    int np = 0;
    double fl = 0;
    const double fl2 = 2.0 * rows * (double)e->H * e->H;
    for (int i = 0; i < nn; ++i) {
      fill_x3tail(e, &tb.p[np++], net[i], rows);
      fl += net[i].out ? fl2 + 2.0 * rows * (double)e->H * A : fl2;
    }
    if (pend && !pend_late) {
      if ((rc = pc_tail(&tb.p[np++]))) return rc;
      fl += fl2;
    }
    if (np && (rc = slot(e, "x3_tail", fl, s, [&] { return x3tail_launch(tb, np, s); }))) return rc;
  } else {
    int parts = -1;   // L2: the deferred policy-loss critic rides here, -mean Q from the epilogue's partial dots
    if ((rc = fwd_layer(e, rows, 2, net, nn, "fwd_l2", s, pend ? &pc : nullptr, &parts))) return rc;
    if (parts >= 0 && (rc = note_policy_parts(e, pend_slot, parts))) return rc;
    if ((rc = fwd_layer(e, rows, 3, net, nn, "fwd_l3_actors", s))) return rc;
  }
  e->panel_bwd_done = false;
  e->split_critics = false;
  e->half_panels = false;
  e->unit_bwd = false;
  if (!value_side) return 0;
  {  // ---- target critics: the action part on top of the state part
    Group g(e, GEMM_FWD, 0, 0);
    for (int c = 0; c < nc; ++c) {
      FwdSpec f{tc[c].ni, 1, tc[c].A1, tc[c].lda1, 0, tc[c].K1};
      f.b_col = tc[c].col1;
      f.C = tc[c].h1; f.ldc = Hp; f.c_f32 = 0; f.relu = 1; f.mask_idx = -1;
      f.addend = e->tc_part[c]; f.ld_add = ldp; f.add_clip = INFINITY;
      g.flops += 2.0 * rows * (double)e->H * A;
      fill_fwd(e, f, rows, g.add());
    }
    if (pend_late) add_layer(g, pc, 1, rows);
    if ((rc = g.run(s, "fwd_l1_target_critic"))) return rc;
  }
  if (tails) {   // Q'(s', a') per row: layer 2 and the last layer's dot in one panel launch
    X3TailBatch tb;
    for (int c = 0; c < nc; ++c) fill_x3tail(e, &tb.p[c], tc[c], rows);
    int np = nc;
    if (pend_late && (rc = pc_tail(&tb.p[np++]))) return rc;
    if ((rc = slot(e, "x3_tail_target_critic", np * 2.0 * rows * (double)e->H * e->H, s, [&] { return x3tail_launch(tb, np, s); }))) return rc;
  } else if ((rc = fwd_layer(e, rows, 2, tc, nc, "fwd_l2_target_critic", s))) {
    return rc;
  }
  return ph_td_head(e, rows, value_bwd, tails, s);   // (+ dz2 and the last layer's gradient partials)
}

// Forward of the value side (+ optionally the actor forward, which is independent of it).
int ph_forward(recnn_engine* e, int rows, bool value_side, bool actor_side, bool value_bwd, hipStream_t s) {
  const int A = e->A, Hp = e->Hp, nc = e->n_critic;
  int rc;
  if (e->x3) return ph_forward_x3(e, rows, value_side, actor_side, value_bwd, s);
  if (e->tune.split_fwd >= 2 && value_chain_ok(e) && e->tune.bwd_panel >= 2 && e->H % 8 == 0) return ph_forward_split(e, rows, value_side, actor_side, value_bwd, s);
  const StepBufs B = step_bufs(e);
  bool chained = false;  // target critics computed inside the first fused launch
  bool fwd_did_bwd = false;  // ... and the critics' head + layer-2 backward too
  // chained target critics add nc producer problems, so a value-side launch always has >= 3 problems
  const bool can_chain = value_side && value_chain_ok(e);
  const int n_first = (value_side ? 1 + nc : 0) + (actor_side ? 1 : 0) + (can_chain ? nc : 0);
  if (fused_mlp_ok(e, n_first)) {
    // whole networks per launch: {target actor, critic(s), actor}
    if (value_side && (rc = ph_td3_noise(e, e->noise_buf, rows, e->run_off, 1, s))) return rc;
    MlpBatch mb;
    memset(&mb, 0, sizeof(mb));
    int np = 0;
    double fl = 0;
    chained = can_chain;
    const bool in_fwd_bwd = chained && e->tune.bwd_panel >= 2 && mlp_waves() == 16;
    fwd_did_bwd = in_fwd_bwd;
    TdDesc td;
    if (in_fwd_bwd && (rc = td_desc(e, value_bwd, &td))) return rc;
    if (chained) {
      // producers first (launch order = dispatch order): state part of each target critic's layer 1, nothing else of the network
      for (int c = 0; c < nc; ++c) {
        Role r = role_target_critic(e, B, c, false);
        r.A1 = nullptr;                          // (the action part: in the target actor's workgroup, MlpTail below)
        MlpProb* p = &mb.p[np++];
        fill_mlp(e, r, rows, p);
        p->W2 = nullptr; p->W3 = nullptr; p->q = nullptr;
        p->part_out = e->tc_part[c]; p->part_flag = e->tc_flag[c];
        fl += 2.0 * rows * (double)e->H * e->S;
      }
    }
    if (value_side) {
      // launch order = dispatch order, and a workgroup may only wait for workgroups dispatched before it: the critics
      // (whose Q(s, a) the head in the target actor's workgroup picks up) come BEFORE the target actor, like the
      // target critics' layer-1 producers -- otherwise a batch with more panels than CUs would dead-lock (bounded)
      for (int c = 0; c < nc; ++c) {
        MlpProb* pc = &mb.p[np++];
        fl += fill_mlp(e, role_critic(e, B, c), rows, pc);
        if (in_fwd_bwd) {
          MlpCriticBwd& cb = mb.cbwd[c];
          pc->cbwd_idx = c;
          cb.enabled = 1;
          cb.q_slot = e->q_slot[c];
          cb.scale = td.scale;
          cb.dz2 = e->dzc2[c]; cb.dz1 = e->dzc1[c];   // UNIT tensors: the dW launch applies the per-row seed e->delta[c]
          fl += 2.0 * rows * (double)e->H * e->H;
        }
      }
      MlpProb* pt = &mb.p[np++];
      fl += fill_mlp(e, role_target_actor(e, B), rows, pt);
      if (in_fwd_bwd) td_write(td, e, &mb.head);
      if (chained) {
        pt->n_tail = nc;
        for (int c = 0; c < nc; ++c) {
          const NetView t = net_view(e, TVAL[c]);
          MlpTail& T = mb.tail[c];
          T.part = e->tc_part[c]; T.flag = e->tc_flag[c];
          T.W1a = t.W1; T.ldw1 = t.ldw1;
          T.W2 = t.W2; T.ldw2 = t.ldw2;
          T.b1 = t.b1; T.b2 = t.b2; T.b3 = t.b3; T.w3row = t.w3row;
          T.q = B.tq[c];
          fl += 2.0 * rows * ((double)e->H * A + (double)e->H * e->H + e->H);
        }
      }
    }
    if (actor_side) fl += fill_mlp(e, role_actor(e, B), rows, &mb.p[np++]);
    if (e->pending_pc.on && np < MLP_MAX_GROUP) {   // the launch has idle CUs once its short workgroups are done
      fl += fill_mlp(e, role_deferred_critic(e), rows, &mb.p[np++]);
      e->pending_pc.on = false;
    }
    mb.err = (int32_t*)(e->losses + 4);
    if ((rc = slot(e, "mlp_fwd_nets", fl, s, [&] { return mlp_launch(mb, np, s); }))) return rc;
  } else {
    // layer by layer: packed rows (compute type) in, tc hidden out; layer 3 of the actors: next_action into the action slot of the packed
    // next rows, gen_action
    Role net[4];
    int nn = 0;
    if (value_side) {
      net[nn++] = role_target_actor(e, B);
      for (int c = 0; c < nc; ++c) net[nn++] = role_critic(e, B, c);
    }
    if (actor_side) net[nn++] = role_actor(e, B);
    if ((rc = fwd_layer(e, rows, 1, net, nn, "fwd_l1", s))) return rc;
    if ((rc = fwd_layer(e, rows, 2, net, nn, "fwd_l2", s))) return rc;
    if (value_side && (rc = ph_td3_noise(e, e->noise_buf, rows, e->run_off, 1, s))) return rc;
    if ((rc = fwd_layer(e, rows, 3, net, nn, "fwd_l3_actors", s))) return rc;
  }
  if (chained) {
    // nothing left to launch for the target critics
  } else if (value_side) {   // target critics on [next_action | next_state]
    Role tc[2] = {};
    for (int c = 0; c < nc; ++c) tc[c] = role_target_critic(e, B, c, true);
    if (fused_mlp_ok(e, nc)) {
      MlpBatch mb;
      memset(&mb, 0, sizeof(mb));
      double fl = 0;
      for (int c = 0; c < nc; ++c) {
        fl += fill_mlp(e, tc[c], rows, &mb.p[c]);
        mb.p[c].h2 = tc[c].h2; mb.p[c].q = nullptr;     // (the head launch takes Q' from the layer-2 activations)
      }
      if ((rc = slot(e, "mlp_fwd_target_critic", fl, s, [&] { return mlp_launch(mb, nc, s); }))) return rc;
    } else {
      if ((rc = fwd_layer(e, rows, 1, tc, nc, "fwd_l1_target_critic", s))) return rc;
      if ((rc = fwd_layer(e, rows, 2, tc, nc, "fwd_l2_target_critic", s))) return rc;
    }
  }
  e->panel_bwd_done = false;
  e->split_critics = false;
  e->half_panels = false;
  e->unit_bwd = false;
  if (value_side && fwd_did_bwd) {
    // nothing left to launch here: losses, the per-row seed and the UNIT dz2 / dz1 came out of the forward launch; the dW
    // launch scales them and adds the bias / last-layer partial sums
    e->panel_bwd_done = true;
    e->unit_bwd = true;
  } else if (value_side && chained && e->tune.bwd_panel) {
    // critic head + dz2 + dz1 in one row-panel launch (bwd.hip); Q comes from the forward launch, Q' from its tails
    BwdPanelBatch bb;
    memset(&bb, 0, sizeof(bb));
    TdDesc td;
    if ((rc = td_desc(e, value_bwd, &td))) return rc;
    double fl = 0;
    for (int c = 0; c < nc; ++c) {
      BwdPanelProb& b = bb.p[c];
      const NetView v = net_view(e, VAL[c]);
      b.rows = rows; b.H = e->H; b.mode = 0;
      td_write(td, c, &b);
      b.h2 = e->cv[c].h2; b.ldh = Hp; b.w3 = v.w3row;
      b.dz2 = e->dzc2[c];
      b.W2 = v.W2; b.ldw2 = v.ldw2;
      b.h1 = e->cv[c].h1; b.dz1 = e->dzc1[c];
      fl += 2.0 * rows * (double)e->H * e->H;
    }
    if ((rc = slot(e, "head_dx_critic", fl, s, [&] { return bwd_panel_launch(bb, nc, s); }))) return rc;
    e->panel_bwd_done = true;
  } else if (value_side) {
    return ph_td_head(e, rows, value_bwd, chained, s);
  }
  return 0;
}

// Backward of the critic(s): dz1 (unless the forward launch produced it), then the weight-gradient GEMMs as split-batch slabs
// (summed by the slab-reducing Adam launch, or by grad_reduce into the flat arenas when `reduce`: the phase API / data parallel).
int ph_value_backward(recnn_engine* e, int rows, bool reduce, hipStream_t s, bool dx_only) {
  const int Hp = e->Hp, H = e->H, nc = e->n_critic;
  int rc;
  if (!e->panel_bwd_done) {
    Group g(e, GEMM_DX, 0, 0);
    for (int c = 0; c < nc; ++c)
      g.flops += fill_dx(e, g.add(), rows, e->dzc2[c], Hp, Hp, VAL[c], W2, 0, H, e->dzc1[c], Hp, e->cv[c].h1, Hp, e->net[VAL[c]].gp[B1]);
    if ((rc = g.run(s, "dx_critic_l2"))) return rc;
  }
  if (dx_only) return 0;     // (the weight gradients follow in dw_adam_kernel: ph_value_dwadam)
  NetLayout L0 = make_layout(e, VAL[0], rows);
  {
    Group g(e, GEMM_DW, 0, 0);  // dW2 = dz2^T h1 and dW1 = dz1^T [a|s], split over the batch into slabs
    DwVec vec;
    memset(&vec, 0, sizeof(vec));
    for (int c = 0; c < nc; ++c) {
      GemmProb* p = g.add();
      g.flops += fill_dw(e, p, rows, e->dzc2[c], Hp, H, e->cv[c].h1, Hp, H, 0, e->net[VAL[c]].gp[W2], L0.t[W2].nslab,
                         L0.t[W2].slab_stride);
      if (e->unit_bwd) p->a_row_scale = e->delta[c];
    }
    for (int c = 0; c < nc; ++c) {
      GemmProb* p = g.add();
      g.flops += fill_dw(e, p, rows, e->dzc1[c], Hp, H, e->xcs, e->ldx, e->S + e->A, e->S, e->net[VAL[c]].gp[W1],
                         L0.t[W1].nslab, L0.t[W1].slab_stride);
      if (e->unit_bwd) p->a_row_scale = e->delta[c];
    }
    if (e->unit_bwd) {  // dW3 / db2 / db1 partial sums per 32-row panel ride on this launch
      vec.n = nc;
      for (int c = 0; c < nc; ++c) {
        Net& v = e->net[VAL[c]];
        DwVecProb& q = vec.p[c];
        q.rows = rows; q.H = H; q.delta = e->delta[c]; q.h2 = e->cv[c].h2; q.u2 = e->dzc2[c]; q.U = e->dzc1[c]; q.ldh = Hp;
        q.dw3_part = v.gp[W3]; q.db2_part = v.gp[B2]; q.colsum = v.gp[B1];
      }
      g.L.vec = &vec;
    }
    if ((rc = g.run(s, "dw_critic"))) return rc;
  }
  for (int c = 0; c < nc && reduce; ++c) {
    NetLayout L = make_layout(e, VAL[c], rows);
    if ((rc = slot(e, "grad_reduce_critic", 0, s, [&] { return grad_reduce_launch(L, g_produce(e, VAL[c]), nullptr, s); }))) return rc;
  }
  return 0;
}

// Policy loss through the (updated) critic 1; optionally the gradient chain back into the actor.
// need_rows: per-row Q(s, pi(s)) wanted (debug / learn=False logging) -> head kernel; otherwise, on the fused bf16 path,
// the loss is summed in the layer-2 GEMM's epilogue and the backward seed comes from the row-panel kernel (bwd.hip).
int ph_policy(recnn_engine* e, int rows, bool backward, bool with_l1, hipStream_t s, bool need_rows) {
  const int A = e->A, Hp = e->Hp, H = e->H, Ap = e->Ap;
  const int V1 = RECNN_NET_VALUE1;
  const NetView v = net_view(e, V1);
  const bool train = e->cfg.mask_mode != RECNN_MASK_NONE;
  int rc;
  // (split bf16: the loss of a step without backward comes from the layer-2 epilogue's partial dots; with backward the head kernel
  // produces the seed dz_e2 as well -- either way the step's partial sums land in its pl_part slot)
  const bool x3_dot = e->x3 && !need_rows && !backward;
  const bool use_dot = (!need_rows && value_panel_ok(e) && !fused_mlp_ok(e, 1)) || x3_dot;
  bool chain_done = false;
  e->pl_dot_parts = 0;
  // critic on [gen_action | state] of the current batch with the UPDATED weights
  Role pcr = role_policy_critic(e, e->xcs, e->gen_action, e->run_off);
  pcr.keep = true;
  if (fused_mlp_ok(e, 1)) {   // one launch, two layer-1 contraction segments
    MlpBatch mb;
    memset(&mb, 0, sizeof(mb));
    const double fl = fill_mlp(e, pcr, rows, &mb.p[0]);
    if ((rc = slot(e, "mlp_fwd_pcritic", fl, s, [&] { return mlp_launch(mb, 1, s); }))) return rc;
  } else {
    // tuning.policy_fused bit 0: layer 1 on the per-step tiled kernel wherever the step's learning critics ran on it (one problem of
    // 64 x 64 tiles, the deferred forward's problem of the "l1_critic" launch on this step's batch: the same h1 bit for bit)
    const bool l1_tiled = (e->tune.policy_fused & 1) && use_dot && !e->x3 && !e->comm && e->tune.policy_chain && e->split_critics &&
                          e->tune.bwd_panel >= 2 && H % 8 == 0;
    if (l1_tiled) {
      L1Batch lb;
      fill_l1(e, &lb.p[0], pcr, rows);
      const double fl = 2.0 * rows * (double)H * (e->S + A);
      if ((rc = slot(e, "l1_pcritic", fl, s, [&] { return l1gemm_launch(lb, 1, 0, s, e->tune.l1_ws); }))) return rc;
    } else if ((rc = fwd_layer(e, rows, 1, &pcr, 1, "fwd_l1_pcritic", s))) {
      return rc;
    }
    if (use_dot) {          // the loss from the layer-2 epilogue's partial dots, into the step's pl_part slot
      pcr.q = e->pl_part;
      if ((rc = fwd_layer(e, rows, 2, nullptr, 0, "fwd_l2_pcritic", s, &pcr, &e->pl_dot_parts))) return rc;
      if ((rc = note_policy_parts(e, e->run_off, e->pl_dot_parts))) return rc;
    } else if ((rc = fwd_layer(e, rows, 2, &pcr, 1, "fwd_l2_pcritic", s))) {
      return rc;
    }
  }
  if (use_dot) {
    if (!backward) return 0;
    Net& pn0 = e->net[POL];
    RECNN_REQUIRE(pn0.g, "policy backward: the actor has no gradient arena bound");
    if (e->tune.policy_chain) {
      // the whole chain dz_e2 -> dz_e1 -> dact -> dz_p2 -> dz_p1 on a row panel that never leaves the CU (bwd.hip)
      BwdChainArgs c;
      memset(&c, 0, sizeof(c));
      const NetView a = net_view(e, POL);
      c.rows = rows; c.H = H; c.A = A; c.delta_const = -1.0f / (float)rows; c.scale = train ? 2.0f : 1.0f; c.ldh = Hp;
      c.e2 = e->pc.h2; c.e1 = e->pc.h1; c.w3c = v.w3row;
      c.W2c = v.W2; c.ldw2c = v.ldw2;
      c.W1c = v.W1; c.ldw1c = v.ldw1;
      c.W3a = a.W3; c.ldw3a = a.ldw3;
      c.W2a = a.W2; c.ldw2a = a.ldw2;
      c.p2 = e->pa.h2; c.p1 = e->pa.h1;
      c.dact = e->dag; c.ldact = Ap; c.dzp2 = e->dzp2; c.dzp1 = e->dzp1;
      c.db3_part = pn0.gp[B3]; c.db2_part = pn0.gp[B2]; c.db1_part = pn0.gp[B1];
      const double fl = 2.0 * rows * ((double)H * H + (double)H * A + (double)A * H + (double)H * H);
      if ((rc = slot(e, "bwd_chain_policy", fl, s, [&] { return bwd_chain_launch(c, s); }))) return rc;
      chain_done = true;
      e->dze1_ok = false;   // dz_e2 / dz_e1 stayed on chip (ph_state_grads makes them when it is asked for the policy loss's gradient)
    } else {
      if ((rc = ph_head_dx_pcritic(e, rows, s))) return rc;
    }
  } else {
    HeadArgs h;
    memset(&h, 0, sizeof(h));
    h.rows = rows; h.H = H; h.tc_bf16 = e->cfg.dtype; h.ld_h = Hp;
    h.n_target = 0; h.n_critic = 1; h.policy_mode = 1;
    h.ch2[0] = e->pc.h2; h.cw3[0] = v.w3row; h.cb3[0] = v.b3;
    h.q[0] = e->qpi; h.loss_part[0] = e->loss_part[2];
    if (e->x3 && !need_rows) {    // the step's policy-loss partial sums (sum of Q incl. b3 per block) in its pl_part slot
      const int nblk = (rows + HEAD_ROWS_PER_BLOCK - 1) / HEAD_ROWS_PER_BLOCK;
      h.loss_part[0] = e->pl_part;
      e->pl_dot_parts = nblk;
      if (e->run_off < LOSS_HIST_MAX) { e->hist_pol_count[e->run_off] = nblk; e->hist_pol_add[e->run_off] = 0; }
    }
    h.do_bwd = backward;          // d(policy_loss)/dQ = -1/B for every row; no critic parameter gradients
    h.train = train;
    h.delta_const = -1.0f / (float)rows;
    h.dz2[0] = e->dze2;
    if ((rc = slot(e, "head_policy_loss", 0, s, [&] { return head_launch(h, s); }))) return rc;
  }
  if (!backward) return 0;
  if (!chain_done) e->dze1_ok = true;
  Net& pn = e->net[POL];
  RECNN_REQUIRE(pn.g, "policy backward: the actor has no gradient arena bound");
  auto dx1 = [&](const char* nm, const void* Ain, int64_t lda, int Kc, int ni, int which, int N, void* C, int64_t ldc, const void* yref,
                 float* colsum) {
    Group g(e, GEMM_DX, 0, 0);
    g.flops += fill_dx(e, g.add(), rows, Ain, lda, Kc, ni, which, 0, N, C, ldc, yref, Hp, colsum);
    return g.run(s, nm);
  };
  // critic: dz_e1 = (dz_e2 W2) * 2[e1>0];   dact = dz_e1 * W1[:, action columns]  (shadow columns 0..A-1)
  if (!chain_done) {
  if (!use_dot && (rc = dx1("dx_pcritic_l2", e->dze2, Hp, Hp, V1, W2, H, e->dze1, Hp, e->pc.h1, nullptr))) return rc;
  if ((rc = dx1("dx_pcritic_action", e->dze1, Hp, Hp, V1, W1, A, e->dag, Ap, nullptr, pn.gp[B3]))) return rc;
  // actor: dz_p2 = (dact W3) * 2[p2>0];  dz_p1 = (dz_p2 W2) * 2[p1>0]
  if ((rc = dx1("dx_actor_l3", e->dag, Ap, Ap, POL, W3, H, e->dzp2, Hp, e->pa.h2, pn.gp[B2]))) return rc;
  if ((rc = dx1("dx_actor_l2", e->dzp2, Hp, Hp, POL, W2, H, e->dzp1, Hp, e->pa.h1, pn.gp[B1]))) return rc;
  }
  NetLayout L = make_layout(e, POL, rows);
  // tuning.policy_fused bit 1: the three weight gradients without slabs -- dwadam.hip's tiles with a gradient-only epilogue sum the batch
  // slices on chip in grad_reduce_kernel's order and write the flat gradient; the clip quirk's per-block |g| sums then come from that
  // arena (l1_blocks_kernel: grad_reduce_kernel's block map and summation order).  Same eligibility as the row-panel chain above.
  if ((e->tune.policy_fused & 2) && chain_done && !e->x3 && !e->comm && e->cfg.dtype == RECNN_BF16 && dwgrad_ok(L, rows)) {
    DwGradNet n;
    memset(&n, 0, sizeof(n));
    n.L = L; n.rows = rows;
    n.w[0].dz = e->dzp1; n.w[0].ldz = Hp; n.w[0].x = e->xcs + tc_off(e, A); n.w[0].ldx = e->ldx; n.w[0].tensor = W1;
    n.w[1].dz = e->dzp2; n.w[1].ldz = Hp; n.w[1].x = e->pa.h1; n.w[1].ldx = Hp; n.w[1].tensor = W2;
    n.w[2].dz = e->dag; n.w[2].ldz = Ap; n.w[2].x = e->pa.h2; n.w[2].ldx = Hp; n.w[2].tensor = W3;
    const double fl = 2.0 * rows * ((double)H * e->S + (double)H * H + (double)A * H);
    if ((rc = slot(e, "dwgrad_actor", fl, s, [&] { return dwgrad_launch(n, g_produce(e, RECNN_NET_POLICY), s); }))) return rc;
    if (!with_l1) return 0;
    return slot(e, "l1_norm_actor", 0, s, [&] { return l1_blocks_launch(L, g_produce(e, RECNN_NET_POLICY), pn.l1part, s); });
  }
  {
    Group g(e, GEMM_DW, 0, 0);
    g.flops += fill_dw(e, g.add(), rows, e->dag, Ap, A, e->pa.h2, Hp, H, 0, pn.gp[W3], L.t[W3].nslab, L.t[W3].slab_stride);
    g.flops += fill_dw(e, g.add(), rows, e->dzp2, Hp, H, e->pa.h1, Hp, H, 0, pn.gp[W2], L.t[W2].nslab, L.t[W2].slab_stride);
    g.flops += fill_dw(e, g.add(), rows, e->dzp1, Hp, H, e->xcs + tc_off(e, A), e->ldx, e->S, 0, pn.gp[W1], L.t[W1].nslab,
                       L.t[W1].slab_stride);
    if ((rc = g.run(s, "dw_actor"))) return rc;
  }
  return slot(e, "grad_reduce_actor", 0, s, [&] { return grad_reduce_launch(L, g_produce(e, RECNN_NET_POLICY), with_l1 ? pn.l1part : nullptr, s); });
}

// The input gradient of the step (state_grad.hip; recnn_engine_state_grads): d loss / d state through layer 1.
//   which 0: gV1 = dz_c1[0] * W1c1[:, state columns]                              (value loss 1; the critic the value backward used)
//   which 1: gP  = dz_e1 * W1c1[:, state columns] + dz_p1 * W1a                   (policy loss; the updated critic 1, then the actor)
//   which 2: gV2 = dz_c1[1] * W1c2[:, state columns]                              (TD3: value loss 2, critic 2 likewise)
//   which 3: gV1 + gV2 in one launch, two segments, critic 1 first                (TD3: what one backward through the encoder needs)
// W comes from the compute-type SHADOWS: they hold exactly the numbers the forward and the backward multiplied with (bf16: the master
// rounded to nearest even by the optimizer / refresh launch), they keep the pre-step critic until the refresh that follows the value
// optimizer, and their rows are 16-byte aligned and zero padded whatever S is -- the master's rows (stride S + A floats) are not.
// Where the fused forward left UNIT tensors, each critic's segment carries its own per-row seed (delta[c]), as its dW launch does.
int ph_state_grads(recnn_engine* e, int rows, int which, float* out, int64_t ld_out, hipStream_t s) {
  const int A = e->A, H = e->H, S = e->S, V1 = RECNN_NET_VALUE1;
  const Net& v = e->net[V1];
  const Net& p = e->net[POL];
  const int vec = 16 / e->esz;
  RECNN_REQUIRE(A + ru(S, vec) <= v.ld_w1 && ru(S, vec) <= p.ld_w1, "state_grads: shadow rows shorter than the state columns");
  RECNN_REQUIRE(which == 0 || which == 1 || e->n_critic == 2, "state_grads: which=%d needs the second critic", which);
  int rc;
  StateGradArgs a;
  memset(&a, 0, sizeof(a));
  a.rows = rows; a.S = S; a.K = H; a.out = out; a.ld_out = ld_out;
  const char* w1c = sh_ptr(e, V1, W1) + tc_off(e, A);   // the shadow is rotated to [action | state]
  // critic c's value-loss segment; the fused forward left UNIT tensors: the per-row seed d is applied in the launch, as the dW launch does
  auto value_seg = [&](int c) {
    const Net& vc = e->net[VAL[c]];
    return StateGradSeg{e->dzc1[c], e->Hp, sh_ptr(e, VAL[c], W1) + tc_off(e, A), vc.ld_w1, e->unit_bwd ? e->delta[c] : nullptr};
  };
  const char* name = "state_grad_value";
  if (which == 0 || which == 2) {
    a.nseg = 1;
    a.seg[0] = value_seg(which / 2);
  } else if (which == 3) {
    RECNN_REQUIRE(A + ru(S, vec) <= e->net[VAL[1]].ld_w1, "state_grads: shadow rows shorter than the state columns");
    a.nseg = 2;
    a.seg[0] = value_seg(0);
    a.seg[1] = value_seg(1);
    name = "state_grad_value12";
  } else {
    if (!e->dze1_ok) {
      // the row-panel chain kept the critic's dz on chip: the same two tensors from the same activations and weights
      if ((rc = ph_head_dx_pcritic(e, rows, s))) return rc;
      e->dze1_ok = true;
    }
    a.nseg = 2;
    a.seg[0] = StateGradSeg{e->dze1, e->Hp, w1c, v.ld_w1, nullptr};
    a.seg[1] = StateGradSeg{e->dzp1, e->Hp, sh_ptr(e, POL, W1), p.ld_w1, nullptr};
    name = "state_grad_policy";
  }
  return slot(e, name, 2.0 * rows * (double)S * H * a.nseg, s, [&] { return state_grad_launch(a, e->cfg.dtype, s); });
}

int ph_finish(recnn_engine* e, int rows, bool ticked_value, bool ticked_policy, hipStream_t s) {
  if (e->run_off >= 0 && e->run_off < LOSS_HIST_MAX) e->hist_half[e->run_off] = e->half_panels;
  if (e->run_skip_finish) return 0;  // inside a run graph: the last step's finalize ticks the counters for the whole run
  LossFinalizeArgs a;
  memset(&a, 0, sizeof(a));
  const int nblk = (rows + HEAD_ROWS_PER_BLOCK - 1) / HEAD_ROWS_PER_BLOCK;
  const int nc = e->n_critic;
  const int nval = (value_panel_ok(e) || e->half_panels) ? (rows + BWD_ROWS - 1) / BWD_ROWS : nblk;
  for (int c = 0; c < nc; ++c) { a.part[c] = e->loss_part[c]; a.n_part[c] = nval; a.scale[c] = 1.0f / (float)rows; a.pair[c] = e->half_panels; }
  a.part[nc] = e->loss_part[2]; a.n_part[nc] = nblk; a.scale[nc] = -1.0f / (float)rows;
  if (e->pl_dot_parts > 0) {  // policy loss = -(sum of the layer-2 epilogue's partial dots, b3 included) / B
    a.part[nc] = e->pl_part; a.n_part[nc] = e->pl_dot_parts;
  }
  a.n = nc + 1;
  a.out = e->losses;
  a.host_out = e->h_stage;
  // run_tick = {1, 1, 1} outside run graphs; the last step of a run adds the whole run's counts
  a.tick_inc[a.n_tick] = e->run_tick[0]; a.tick[a.n_tick++] = e->counters;  // mask-key step
  if (ticked_value) {
    a.tick_inc[a.n_tick] = e->run_tick[1]; a.tick[a.n_tick++] = e->net[RECNN_NET_VALUE1].t_ptr;
    if (e->td3) { a.tick_inc[a.n_tick] = e->run_tick[1]; a.tick[a.n_tick++] = e->net[RECNN_NET_VALUE2].t_ptr; }
  }
  const bool run_final = e->run_tick[0] > 1;  // last step of a run graph: the actor took run_tick[2] steps during the run
  if (run_final ? e->run_tick[2] > 0 : ticked_policy) { a.tick_inc[a.n_tick] = e->run_tick[2]; a.tick[a.n_tick++] = e->net[RECNN_NET_POLICY].t_ptr; }
  if (e->has_sampler && e->use_sampler) { a.wrap_ptr = e->smp.cursor; a.wrap_mod = e->smp.n_batches; a.wrap_inc = e->run_tick[0]; }
  a.ring = e->loss_ring; a.ring_mask = LOSS_RING - 1;
  if (run_final && e->run_off >= 1 && e->run_off < LOSS_HIST_MAX) {
    // losses of the run's earlier steps from their kept partial sums (the step counter is not ticked yet)
    LossHistoryArgs h;
    memset(&h, 0, sizeof(h));
    h.n_steps = e->run_off; h.n = nc + 1;
    for (int i = 0; i < e->run_off; ++i) h.pair_steps |= (unsigned long long)(e->hist_half[i] ? 1 : 0) << i;
    for (int c = 0; c < nc; ++c) { h.part[c] = e->loss_part_base[c]; h.stride[c] = e->loss_part_stride; h.n_part[c] = nval; h.scale[c] = 1.0f / (float)rows; }
    h.scale[nc] = -1.0f / (float)rows;
    if (value_panel_ok(e) || e->x3) {   // policy loss from the layer-2 epilogue's partial dots / the deferred forward's per-row Q
      h.part[nc] = e->pl_part_base; h.stride[nc] = e->pl_cap;
      for (int i = 0; i < e->run_off; ++i) { h.pol_count[i] = e->hist_pol_count[i]; h.pol_add[i] = e->hist_pol_add[i]; }
    } else {                   // ... from the head kernel's per-block partial sums (fp32 / generic path)
      h.part[nc] = e->loss_part_base[2]; h.stride[nc] = e->loss_part_stride;
      for (int i = 0; i < e->run_off; ++i) { h.pol_count[i] = nblk; h.pol_add[i] = 0; }
    }
    h.b3 = e->net[RECNN_NET_VALUE1].p + e->net[RECNN_NET_VALUE1].off[B3];
    h.step_ctr = e->counters; h.ring = e->loss_ring; h.ring_mask = LOSS_RING - 1;
    int hrc = slot(e, "loss_history", 0, s, [&] { return loss_history_launch(h, s); }, false);
    if (hrc) return hrc;
  }
  return slot(e, "loss_finalize", 0, s, [&] { return loss_finalize_launch(a, s); }, false);
}

}  // namespace recnn_eng

namespace recnn_eng {
int ph_policy_l1(recnn_engine* e, hipStream_t s) {
  Net& pn = e->net[RECNN_NET_POLICY];
  NetLayout L = make_layout(e, RECNN_NET_POLICY, 0);
  return slot(e, "l1_norm_actor", 0, s, [&] {
    return l1_blocks_launch(L, g_consume(e, RECNN_NET_POLICY), pn.l1part, s);
  });
}

// rows > 0: fused single-GPU path, Adam sums the gradient slabs itself (no separate reduction launch)
int value_apply(recnn_engine* e, bool soft, float grad_scale, hipStream_t s, int rows) {
  int rc;
  for (int c = 0; c < e->n_critic; ++c)
    if ((rc = apply_net(e, VAL[c], rows, true, 1, grad_scale, false, soft ? TVAL[c] : -1, e->hy.soft_tau, s, rows > 0)))
      return rc;
  return 0;
}

// The critics' weight gradients with the optimizer step in the epilogue (dwadam.hip): ONE launch instead of ph_value_backward +
// value_apply, no gradient slabs.  Taken when the step's backward tensors came from the split forward's tail (mlpt.hip: dz2 / dz1
// already carry the per-row loss seed, the small tensors' panel sums exist) on the single-GPU bf16 step; bit-identical to the two launches.
bool dwadam_ok(const recnn_engine* e, int rows) {
  if (!e->tune.dw_fuse || e->comm || e->unit_bwd || e->H != 256) return false;
  if (e->x3) {
    // split bf16: the head launch wrote dz2 (times the loss seed) and the small tensors' partial sums; dz1 comes from the dX launch that
    // ph_value_dwadam issues first.  (The generic split-bf16 forward only: Hp = 512 physical.)
    if (e->cfg.dtype != RECNN_BF16X3 || e->panel_bwd_done || e->Hp != 512) return false;
  } else if (e->cfg.dtype != RECNN_BF16 || !e->panel_bwd_done || e->Hp != 256) return false;
  for (int c = 0; c < e->n_critic; ++c) {
    const Net& n = e->net[VAL[c]];
    if (!n.g || !n.m || !n.v || !n.critic) return false;
    const NetLayout L = make_layout(e, VAL[c], rows);
    if (!dwadam_tensor_ok(L, W1, rows, e->x3) || !dwadam_tensor_ok(L, W2, rows, e->x3)) return false;
    if (!L.t[B1].small || !L.t[B2].small || !L.t[W3].small || !L.t[B3].small) return false;
  }
  return true;
}

int ph_value_dwadam(recnn_engine* e, int rows, bool soft, hipStream_t s) {
  DwAdamBatch b;
  memset(&b, 0, sizeof(b));
  double fl = 0;
  int rc;
  if (!e->panel_bwd_done && (rc = ph_value_backward(e, rows, false, s, true))) return rc;   // (split bf16: the critics' dX launch)
  for (int c = 0; c < e->n_critic; ++c) {
    DwAdamNet& n = b.n[c];
    n.L = make_layout(e, VAL[c], rows);
    if ((rc = fill_apply_args(e, VAL[c], n.L, true, 1, 1.0f, false, soft ? TVAL[c] : -1, e->hy.soft_tau, &n.a))) return rc;
    n.a.from_slabs = 1;
    n.rows = rows;
    n.w[0].dz = e->dzc2[c]; n.w[0].ldz = e->Hp; n.w[0].x = e->cv[c].h1; n.w[0].ldx = e->Hp; n.w[0].tensor = W2;
    n.w[1].dz = e->dzc1[c]; n.w[1].ldz = e->Hp; n.w[1].x = e->xcs; n.w[1].ldx = e->ldx; n.w[1].tensor = W1;
    fl += 2.0 * rows * (double)e->H * (e->H + e->S + e->A);
  }
  return slot(e, "dwadam_critic", fl, s, [&] { return dwadam_launch(b, e->n_critic, s); }, false);
}

int policy_apply(recnn_engine* e, bool soft, float grad_scale, hipStream_t s, bool have_l1) {
  int rc;
  if (!have_l1 && (rc = ph_policy_l1(e, s))) return rc;
  // TD3 never soft-updates the target policy (td3.py:136-141); DDPG does (ddpg.py:98-100).
  const int tgt = (soft && !e->td3) ? RECNN_NET_TARGET_POLICY : -1;
  return apply_net(e, RECNN_NET_POLICY, 0, true, 0, grad_scale, true, tgt, e->hy.soft_tau, s);
}

// per-step slot of the loss partial sums (run graphs: step i of the run; everything else: slot 0)
void use_hist_slot(recnn_engine* e, int i) {
  for (int c = 0; c < 3; ++c) e->loss_part[c] = e->loss_part_base[c] + (int64_t)i * e->loss_part_stride;
  e->pl_part = e->pl_part_base + (int64_t)i * e->pl_cap;
}

// batch buffer set k (0: the bound / first set, 1: the look-ahead set of bf16 sampler mode)
void use_set(recnn_engine* e, int k) {
  e->cur_set = k;
  if (k == 0) {
    e->xcs = e->twins ? e->xsh : (char*)e->xs;
    e->xcn = e->twins ? e->xnh : (char*)e->xn;
    e->reward = e->reward0; e->done = e->done0;
    e->gen_action = e->gen_action0;
  } else {
    e->xcs = e->xsh2; e->xcn = e->xnh2; e->reward = e->reward2; e->done = e->done2;
    e->gen_action = e->gen_action2;
  }
}
bool lookahead_ok(const recnn_engine* e) {
  return e->has_sampler && e->twins && !e->tune.sampler_f32_rows && (e->smp.users_per_batch <= 1024 || e->smp.plan) && e->tune.pregather;
}

// gather of the batch `cursor_add` steps ahead of the device cursor into buffer set `set`
GatherArgs gather_args(const recnn_engine* e, int rows, int set, int cursor_add) {
  const recnn_sampler& m = e->smp;
  const bool inl = m.users_per_batch <= 1024;   // the gather plans its rows itself: one launch less
  GatherArgs g;
  memset(&g, 0, sizeof(g));
  g.items = m.items; g.ratings = m.ratings; g.user_off = m.user_off; g.users = m.perm;
  g.row_off = inl ? nullptr : m.row_off;
  g.n_users = m.users_per_batch; g.rows = rows; g.frame = m.frame; g.emb = m.emb_dim; g.table = m.table;
  g.state = e->xs + e->A; g.ld_state = e->ldx32;
  g.next_state = e->xn + e->A; g.ld_next = e->ldx32;
  g.action = e->xs; g.ld_action = e->ldx32;
  g.reward = set ? e->reward2 : e->reward0; g.done = set ? e->done2 : e->done0;
  g.cursor = m.cursor; g.cursor_stride = m.users_per_batch;
  g.cursor_add = cursor_add; g.cursor_mod = m.n_batches;
  g.inline_plan = inl;
  if (m.plan && rows <= m.plan_rows) { g.plan = m.plan; g.plan_stride = m.plan_rows; }
  if (e->twins) {  // the compute-type twins of the packed rows are written by the same kernel
    char* hs = set ? e->xsh2 : e->xsh;
    char* hn = set ? e->xnh2 : e->xnh;
    const int acol = e->x3 ? 2 * e->A : e->A;   // (split rows: the state columns start at physical column 2 A)
    g.state_h = (bf16_t*)hs + acol; g.next_h = (bf16_t*)hn + acol; g.action_h = (bf16_t*)hs;
    g.ld_h = e->ldx;
    g.x3 = e->x3;
    // Nothing reads the fp32 rows when the engine samples its own batches in bf16: materialise the batch in
    // the compute type only (recnn_tune_sampler_f32_rows(1) restores the fp32 copies, e.g. for inspection).
    if (!e->tune.sampler_f32_rows) { g.state = nullptr; g.next_state = nullptr; g.action = nullptr; }
  }
  return g;
}

int frame_gather_packed(recnn_engine* e, int rows, hipStream_t s) {
  const recnn_sampler& m = e->smp;
  const bool inl = m.users_per_batch <= 1024 || (m.plan && rows <= m.plan_rows);
  if (!inl) {
    int rc = slot(e, "frame_plan", 0, s, [&] {
      return recnn_frame_plan(m.user_off, m.perm, m.users_per_batch, m.frame, m.row_off, m.cursor, m.users_per_batch, s);
    });
    if (rc) return rc;
  }
  return slot(e, "frame_gather", 0, s, [&] { return frame_gather_launch(gather_args(e, rows, e->cur_set, e->run_off), s); });
}

// Make the step's batch available in the compute type: built by the sampler, or converted from the bound fp32 rows.
int stage_batch(recnn_engine* e, int rows, hipStream_t s) {
  if (e->has_sampler && e->use_sampler) return frame_gather_packed(e, rows, s);
  if (e->bf16)
    return slot(e, "rows_to_bf16", 0, s, [&] {
      return rows_to_bf16_launch(e->xs, e->xn, (bf16_t*)e->xsh, (bf16_t*)e->xnh, rows, e->ldx, s);
    });
  if (e->x3)   // (padding columns of the split rows rest at zero: the workspace is zero-initialised and nothing writes them)
    return slot(e, "rows_to_x3", 0, s, [&] {
      return rows_to_x3_launch(e->xs, e->xn, (bf16_t*)e->xsh, (bf16_t*)e->xnh, rows, e->S + e->A, e->ldx32, e->ldx, s);
    });
  return 0;
}

// ---- cycle mode: batch j of the cycle = rows j * rows .. (j + 1) * rows - 1 of the m_* arrays
void use_mset(recnn_engine* e, int j, int rows) {
  const int64_t r0 = (int64_t)j * rows;
  e->xcs = e->m_xs + r0 * e->ldx * 2; e->xcn = e->m_xn + r0 * e->ldx * 2;
  e->reward = e->m_reward + r0; e->done = e->m_done + r0;
  e->gen_action = e->m_ga + r0 * e->Ap * 2;
  e->pa.h1 = e->m_pa_h1 + r0 * e->Hp * 2; e->pa.h2 = e->m_pa_h2 + r0 * e->Hp * 2;
  for (int c = 0; c < e->n_critic; ++c) e->tqv[c] = e->m_tq[c] + r0;
}
void leave_mset(recnn_engine* e) {
  e->pa = e->pa0;
  for (int c = 0; c < 2; ++c) e->tqv[c] = e->tqv0[c];
  use_set(e, 0);
}
bool cycle_ok(const recnn_engine* e, int rows) {
  return e->tune.split_fwd && lookahead_ok(e) && value_chain_ok(e) && e->tune.bwd_panel >= 2 && e->H % 8 == 0 && rows % 32 == 0 && e->m_xs != nullptr &&
         !e->ext_noise && e->cfg.mask_mode != RECNN_MASK_EXTERNAL;   // (external masks / noise describe ONE batch)
}

// The FROZEN networks on all n * rows rows of the cycle's batches (gathered by ph_gather_cycle into the current copy):
// target actor -> next_action (+ TD3 noise) -> target critics -> Q', and the actor -> gen_action (+ its activations for the
// policy step's backward).  recnn/nn/update/misc.py:28-31, td3.py:73-81 (target side), ddpg.py:66-69 / td3.py:104-110 (actor).
void select_mbuf(recnn_engine* e, int b) {
  e->m_xs = e->m_xs_b[b]; e->m_reward = e->m_reward_b[b]; e->m_done = e->m_done_b[b];
  // window mode: only a segment that steps through the fused forward has next rows (its steps' e->xcn); nothing of a batched
  // segment reads e->xcn -- the frozen launches take m_tail_n / m_na, the per-step launches the state rows
  e->m_xn = e->win ? e->m_xn_short : e->m_xn_b[b];
  e->m_tail_n = e->m_tail_n_b[b]; e->m_na = e->m_na_b[b];
}

// tuning.frozen_window applies to the bf16 cycle schedule with the fused frozen launches.  Every reader of the cycle's next rows is
// covered: the batched frozen launches (ph_frozen_batched: windows) -- their tiled form (frozen_fused 0) reads whole rows and makes the
// mode ineligible --; the fused forward of segments shorter than cycle_min_seg (m_xn_short: they must fit it); the per-step launches of
// a batched segment, the data-parallel exchange and TD3's noise addend (indexed by row) do not read them.
bool window_ok(const recnn_engine* e, int rows) {
  return e->tune.frozen_window && e->bf16 && e->tune.frozen_fused && e->win_tail > 0 && cycle_ok(e, rows) && e->has_sampler &&
         e->smp.emb_dim == e->A && e->smp.frame * e->smp.emb_dim == e->K1a - e->win_tail && e->tune.cycle_min_seg - 1 <= recnn_engine::SHORT_SETS;
}
// the cycle's packed next rows for everything that is not window mode: allocated (and zeroed, like the workspace) on first use
static int ensure_mxn(recnn_engine* e) {
  if (e->m_xn_own || !e->bf16) return 0;
  const size_t each = (size_t)ru((int64_t)recnn_engine::MSET_MAX * e->Bc * e->ldx * 2, 256);
  RECNN_HIP(hipMalloc((void**)&e->m_xn_own, 2 * each));
  RECNN_HIP(hipMemset(e->m_xn_own, 0, 2 * each));
  e->m_xn_b[0] = e->m_xn_own; e->m_xn_b[1] = e->m_xn_own + each;
  return 0;
}
int begin_cycle_mode(recnn_engine* e, int rows) {
  e->win = window_ok(e, rows);
  const int rc = e->win ? 0 : ensure_mxn(e);
  select_mbuf(e, 0);
  return rc;
}

// the batches of run steps run_off0 .. run_off0 + n - 1 into copy `b` of the cycle arrays: one launch
int ph_gather_cycle(recnn_engine* e, int rows, int n, int run_off0, int b, hipStream_t s, bool batched) {
  GatherArgs g = gather_args(e, rows, 0, run_off0);
  g.state_h = (bf16_t*)e->m_xs_b[b] + e->A; g.action_h = (bf16_t*)e->m_xs_b[b];
  RECNN_REQUIRE(e->win || e->m_xn_b[b], "cycle gather: the packed next rows are not allocated (begin_cycle_mode)");
  if (!e->win) g.next_h = (bf16_t*)e->m_xn_b[b] + e->A;
  else if (!batched) { RECNN_REQUIRE(n <= recnn_engine::SHORT_SETS, "cycle gather: %d batches of a short segment", n); g.next_h = (bf16_t*)e->m_xn_short + e->A; }
  else { g.next_h = nullptr; g.tail_n = (bf16_t*)e->m_tail_n_b[b]; g.ld_tail = e->win_tail; }
  g.reward = e->m_reward_b[b]; g.done = e->m_done_b[b];
  return slot(e, "frame_gather_cycle", 0, s, [&] { return frame_gather_multi_launch(g, n, s, e->tune.gather_cycle); });
}

int ph_frozen_batched(recnn_engine* e, int rows, int n, int run_off0, hipStream_t s, bool ends_on_policy) {
  const int A = e->A, nc = e->n_critic;
  const int M = n * rows;
  int rc;
  // the cycle's batches in one launch (batch j: the key of step run_off0 + j)
  if ((rc = ph_td3_noise(e, e->m_noise, rows, run_off0, n, s))) return rc;
  const double l1_fl_a = 2.0 * M * (double)e->H * e->S, l1_fl_c = 2.0 * M * (double)e->H * (e->S + A);
  const double t_fl_a = 2.0 * M * ((double)e->H * e->H + (double)A * e->H), t_fl_c = 2.0 * M * ((double)e->H * e->H + e->H);
  const StepBufs CB = cycle_bufs(e, rows, run_off0);
  const Role ta = role_target_actor(e, CB), ac = role_actor(e, CB);
  Role tc[2] = {};
  for (int c = 0; c < nc; ++c) tc[c] = role_target_critic(e, CB, c, false);
  if (e->tune.frozen_fused) {
    // a role's whole network on prows rows of the cycle as a problem of the frozen launch (mlpf.hip): hash masks only
    auto fill = [&](FrozenProb* p, const Role& f, int prows) {
      const NetView v = net_view(e, f.ni);
      memset(p, 0, sizeof(*p));
      p->A[0] = f.A0; p->lda[0] = f.lda0; p->K[0] = f.K0; p->w1_col[0] = f.col0; p->nseg = 1;
      if (f.A1) { p->A[1] = f.A1; p->lda[1] = f.lda1; p->K[1] = f.K1; p->w1_col[1] = f.col1; p->nseg = 2; }
      p->W1 = v.W1; p->ldw1 = v.ldw1; p->W2 = v.W2; p->ldw2 = v.ldw2; p->W3 = v.W3; p->ldw3 = v.ldw3;
      p->b1 = v.b1; p->b2 = v.b2; p->b3 = v.b3; p->w3row = v.w3row;
      p->rows = prows; p->H = e->H; p->out_dim = e->net[f.ni].out_dim;
      const MaskSel m1 = mask_sel(e, f.mask_idx, f.step_add, true), m2 = mask_sel(e, mask2_idx(f.mask_idx), f.step_add, true);
      p->mask_mode = m1.mode; p->seed = m1.seed; p->stream1 = m1.stream; p->stream2 = m2.stream;
      p->step_ptr = m1.step_ptr; p->step_add = m1.step_add;
      if (m1.mode != RECNN_MASK_NONE) p->rows_per_set = rows;
      p->h1 = f.keep ? f.h1 : nullptr; p->h2 = f.keep ? f.h2 : nullptr; p->ldh = e->Hp;
      p->out = f.out; p->ldo = f.ldo;
      p->addend = f.addend; p->ld_add = f.ld_add; p->add_clip = f.add_clip;
      p->q = f.q;
    };
    // Two launches (the target critics need the target actor's output).  A launch is 128-row workgroups at ONE per CU, so what
    // counts is how many rounds of 256 it takes: {target actor, actor} = 2 x 160 workgroups at 10 x 2048 rows = two rounds
    // with the second three quarters empty.  The actor depends on nothing here, so its batches are dealt out over both
    // launches to fill them: as many whole batches next to the target actor as fit the first round, the rest next to the
    // target critics (DDPG, 10 x 2048 rows: 160 + 96 and 160 + 64 workgroups = two full rounds instead of three).
    // Round 6: 64-row workgroups last 0.70 of a 128-row one's time (tools/frozen_trace.py: 48.5k against 69.6k clocks) -- a gain while the
    // launch still fits the same number of rounds, i.e. for the SHORT segments of a run that starts or ends inside a policy cycle (the
    // driver's 20 steps: 6 + 10 + 4).  All (rows per workgroup of launch 1, actor batches in launch 1, rows per workgroup of launch 2)
    // are priced as rounds x duration; ties go to the 128-row form and to the larger first share.
    const int cus = 256;
    int sets_a = n, fr_a = 128, fr_b = 128;
    if (rows % 128 == 0) {
      float best = 1e30f;
      for (int fa = 128; fa >= (e->tune.frozen_half ? 64 : 128); fa -= 64)
        for (int fb = 128; fb >= (e->tune.frozen_half ? 64 : 128); fb -= 64)
          for (int sa = n; sa >= 0; --sa) {
            const int wa = (n + sa) * (rows / fa), wb = (nc * n + (n - sa)) * (rows / fb);
            const float cost = (float)((wa + cus - 1) / cus) * (fa == 64 ? 0.70f : 1.0f) + (float)((wb + cus - 1) / cus) * (fb == 64 ? 0.70f : 1.0f);
            if (cost < best - 1e-6f) { best = cost; sets_a = sa; fr_a = fa; fr_b = fb; }
          }
    }
    auto actor_part = [&](FrozenProb* p, int set0, int nsets) {      // the actor on batches set0 .. set0 + nsets - 1
      fill(p, role_actor(e, cycle_bufs(e, rows, run_off0, set0)), nsets * rows);
      if (e->tune.frozen_acts_policy_only) {
        // h1 / h2 have one reader: the backward of the policy step (bwd_chain / the actor's dW), on the segment's LAST batch
        const int pol_set = n - 1 - set0;                            // ... as a batch of this part
        if (!ends_on_policy || pol_set < 0 || pol_set >= nsets) p->h1 = p->h2 = nullptr;
        else p->store_row0 = pol_set * rows;
      }
    };
    // Window mode (tuning.frozen_window): no next rows exist.  s' = [e1..eF | r1..rF | 0] of a transition is, column for column,
    // [state row from its second embedding on | action row | next ratings]: three contraction segments with constant offsets into
    // m_xs and m_tail_n, against the same W1 columns in the same ascending k order -- the same bits as the materialised row.
    const bool win = e->win;
    const int64_t aoff = (int64_t)A * 2;
    const int FE = e->K1a - e->win_tail;                             // frame x emb embedding columns of a state
    auto window = [&](FrozenProb* p, int col0) {
      p->A[0] = e->m_xs + aoff + (int64_t)A * 2; p->lda[0] = e->ldx; p->K[0] = FE - A; p->w1_col[0] = col0;            // e1..e(F-1)
      p->A[1] = e->m_xs; p->lda[1] = e->ldx; p->K[1] = A; p->w1_col[1] = col0 + FE - A;                               // eF = the action
      p->A[2] = e->m_tail_n; p->lda[2] = e->win_tail; p->K[2] = e->win_tail; p->w1_col[2] = col0 + FE;                // r1..rF, zeros
      p->nseg = 3;
    };
    FrozenBatch fb;
    int np = 0;
    fill(&fb.p[np], ta, M);                                          // target actor on s' -> next_action into the rows' action slot
    if (win) { window(&fb.p[np], 0); fb.p[np].out = e->m_na; fb.p[np].ldo = e->Ap; }    // ... or into its own compact array
    ++np;
    if (sets_a > 0) actor_part(&fb.p[np++], 0, sets_a);              // actor on s -> gen_action, activations kept for the policy step
    if ((rc = slot(e, "frozen_actors", l1_fl_a + t_fl_a + (l1_fl_a + t_fl_a) * sets_a / n, s, [&] { return mlpf_launch(fb, np, s, fr_a); }))) return rc;
    FrozenBatch fc;
    int nq = 0;
    for (int c = 0; c < nc; ++c) {                                  // target critics on [s' | next_action]: state part first
      fill(&fc.p[nq], tc[c], M);
      if (win) {
        window(&fc.p[nq], A);
        fc.p[nq].A[3] = e->m_na; fc.p[nq].lda[3] = e->Ap; fc.p[nq].K[3] = e->Ap; fc.p[nq].w1_col[3] = 0; fc.p[nq].nseg = 4;
      }
      ++nq;
    }
    if (sets_a < n) actor_part(&fc.p[nq++], sets_a, n - sets_a);
    return slot(e, "frozen_target_critics", nc * (l1_fl_c + t_fl_c) + (l1_fl_a + t_fl_a) * (n - sets_a) / n, s, [&] { return mlpf_launch(fc, nq, s, fr_b); });
  }

  // The tiled form: layer 1 of a whole cycle as GEMMs (l1gemm.hip), the later layers either likewise (tuning.frozen_gemm) or as tail panels.
  // Layer 2 / 3 of a role as a problem of the layer-1 kernel (K = 256): per output element the arithmetic of the row-panel tail kernel (k
  // ascending in steps of 32 from a zero accumulator, + bias, relu, dropout / + clipped noise, round to bf16), without 1280 workgroups each
  // starting a 192 KB weight stream for 32 rows.  (Written out here: this borrowed use of L1Prob has no second caller.)
  auto later = [&](L1Prob* p, const Role& r, int layer) {
    const NetView v = net_view(e, r.ni);
    Role g{r.ni, layer == 2 ? r.h1 : r.h2, e->Hp, e->Hp, 0};
    g.h1 = layer == 2 ? r.h2 : r.out; g.mask_idx = layer == 2 ? mask2_idx(r.mask_idx) : -1; g.step_add = r.step_add;
    fill_l1(e, p, g, M);
    p->W1 = layer == 2 ? v.W2 : v.W3; p->ldw1 = layer == 2 ? v.ldw2 : v.ldw3; p->b1 = layer == 2 ? v.b2 : v.b3;
    if (layer == 3) {
      p->H = A; p->w_rows = e->Ap; p->no_relu = 1; p->ldh = r.ldo;
      p->addend = r.addend; p->ld_add = r.ld_add; p->add_clip = r.add_clip;
    }
  };
  {
    L1Batch lb;
    fill_l1(e, &lb.p[0], ta, M);
    fill_l1(e, &lb.p[1], ac, M);
    lb.p[1].rows_per_set = rows;
    if ((rc = slot(e, "l1_frozen_actors", 2 * l1_fl_a, s, [&] { return l1gemm_launch(lb, 2, e->tune.l1_big, s); }))) return rc;
    if (e->tune.frozen_gemm) {
      L1Batch l2;
      later(&l2.p[0], ta, 2);
      later(&l2.p[1], ac, 2);
      l2.p[1].rows_per_set = rows;
      if ((rc = slot(e, "l2_frozen_actors", 4.0 * M * (double)e->H * e->H, s, [&] { return l1gemm_launch(l2, 2, e->tune.l1_big, s); }))) return rc;
      L1Batch l3;
      later(&l3.p[0], ta, 3);
      later(&l3.p[1], ac, 3);
      if ((rc = slot(e, "l3_frozen_actors", 4.0 * M * (double)A * e->H, s, [&] { return l1gemm_launch(l3, 2, e->tune.l1_big, s); }))) return rc;
    } else {
      TailBatch tb;
      fill_tail(e, &tb.p[0], TAIL_ACTOR, ta, M);
      fill_tail(e, &tb.p[1], TAIL_ACTOR, ac, M);
      tb.p[1].rows_per_set = rows;
      if ((rc = slot(e, "tail_frozen_actors", 2 * t_fl_a, s, [&] { return mlpt_launch(tb, 2, s); }))) return rc;
    }
  }
  {
    L1Batch lb;
    for (int c = 0; c < nc; ++c) fill_l1(e, &lb.p[c], tc[c], M);
    if ((rc = slot(e, "l1_frozen_target_critic", nc * l1_fl_c, s, [&] { return l1gemm_launch(lb, nc, e->tune.l1_big, s); }))) return rc;
    if (e->tune.frozen_gemm) {
      L1Batch l2;
      for (int c = 0; c < nc; ++c) later(&l2.p[c], tc[c], 2);
      if ((rc = slot(e, "l2_frozen_target_critic", nc * 2.0 * M * (double)e->H * e->H, s, [&] { return l1gemm_launch(l2, nc, e->tune.l1_big, s); }))) return rc;
      for (int c = 0; c < nc; ++c) {
        const NetView t = net_view(e, TVAL[c]);
        if ((rc = slot(e, "q_frozen_target_critic", 2.0 * M * e->H, s, [&] { return qdot_launch(tc[c].h2, e->Hp, t.w3row, t.b3, e->H, M, tc[c].q, s); }))) return rc;
      }
    } else {
      TailBatch tb;
      for (int c = 0; c < nc; ++c) fill_tail(e, &tb.p[c], TAIL_CRITIC_Q, tc[c], M);
      if ((rc = slot(e, "tail_frozen_target_critic", nc * t_fl_c, s, [&] { return mlpt_launch(tb, nc, s); }))) return rc;
    }
  }
  return 0;
}

// The critics' exchange can run inside their optimizer launch when every workgroup's element range is made of whole float4
// groups of the arena (all tensor offsets and all but the last tensor's sizes multiples of 4) and there is a flag slot per
// workgroup.
bool comm_fused_ok(recnn_engine* e, int rows) {
  if (!e->comm || !e->comm_region || !e->tune.comm_fused) return false;
  for (int c = 0; c < e->n_critic; ++c) {
    const NetLayout L = make_layout(e, VAL[c], rows);
    if (L.nblk > COMM_MAX_WG || !L.t[W1].nslab) return false;
    for (int t = 0; t < 6; ++t) {
      if (L.t[t].p_off & 3) return false;
      if (t < 5 && (((int64_t)L.t[t].rows * L.t[t].cols) & 3)) return false;
    }
  }
  return true;
}

int net_allreduce(recnn_engine* e, int ni, const char* name, hipStream_t s) {
  Net& n = e->net[ni];
  return slot(e, name, 0, s, [&] {
    return e->comm_region ? comm_allreduce_region(e->comm, e->comm_off[ni], n.g, g_direct(e, ni) ? nullptr : n.g, n.n_params, s) : comm_allreduce_launch(e->comm, n.g, n.n_params, s);
  });
}

// The whole step.  `policy_step` is decided by the caller (host counter), everything else is on-device.
// pregathered: the batch of this step is already in the current buffer set (put there by the previous step's
// optimizer launch); gather_next: this step's critic optimizer launch also gathers the NEXT batch into the other set.
int step_impl(recnn_engine* e, int rows, bool learn, bool policy_step, hipStream_t s, bool pregathered, bool gather_next,
              bool defer_policy_fwd, bool frozen_done) {
  int rc;
  e->sg_ok = 0;   // (recnn_engine_state_grads belongs to the phase API: a whole step leaves nothing it may read)
  if (!pregathered && (rc = stage_batch(e, rows, s))) return rc;
  // Split bf16 with the fused dW + optimizer launch: that launch (147 KB of LDS per workgroup) cannot carry the look-ahead gather the
  // way apply_gather_kernel does, so the critic HEAD launch does -- armed here, consumed inside ph_forward (if no head launch takes it,
  // the optimizer launch carries it as before and the two-launch form stays)
  GatherArgs ga_head;
  bool head_ride = false;
  if (learn && gather_next && e->x3 && !e->comm && e->tune.dw_fuse && e->H == 256 && e->Hp == 512) {
    const NetLayout L0 = make_layout(e, RECNN_NET_VALUE1, rows);
    if (dwadam_tensor_ok(L0, W1, rows, 1) && dwadam_tensor_ok(L0, W2, rows, 1)) {
      ga_head = gather_args(e, rows, e->cur_set ^ 1, e->run_off + 1);
      e->head_gather = &ga_head;
      head_ride = true;
    }
  }
  if (frozen_done) {   // cycle mode: the batch is in place and the frozen networks have been applied to it (ph_frozen_batched)
    if ((rc = ph_forward_split(e, rows, true, true, learn, s, true))) return rc;
  } else if ((rc = ph_forward(e, rows, true, true, learn, s))) return rc;
  if (learn) {
    // The critic's soft update reads the just-updated weights and nothing reads the target before the
    // next step, so on policy steps it is fused into the critic's optimizer pass (ddpg.py:95-97) -- which itself is the
    // epilogue of the weight-gradient launch on the bf16 unit-backward path (dwopt.hip), a separate Adam launch otherwise.
    GatherArgs ga;
    const bool rode = head_ride && e->head_gather == nullptr;     // the head launch took the next step's gather
    e->head_gather = nullptr;
    if (gather_next && !rode) { ga = gather_args(e, rows, e->cur_set ^ 1, e->run_off + 1); e->pregather = &ga; }
    if (e->comm) {
      // data parallel: finished gradients into the flat arenas, summed over the ranks by one launch per arena, then the
      // replicated optimizer step on grad / world (recnn_amd/parallel.py; the arithmetic of the global batch mean)
      if (comm_fused_ok(e, rows)) {
        // ... with the exchange inside the critics' optimizer launches (optim.hip exchange_grads): the launches of the
        // single-GPU step
        rc = ph_value_backward(e, rows, false, s);
        if (!rc) rc = value_apply(e, policy_step, e->comm_scale, s, rows);
      } else {
        rc = ph_value_backward(e, rows, true, s);
        for (int c = 0; c < e->n_critic && !rc; ++c) rc = net_allreduce(e, VAL[c], "allreduce_critic", s);
        if (!rc) rc = value_apply(e, policy_step, e->comm_scale, s);
      }
    } else if ((!gather_next || rode) && dwadam_ok(e, rows)) {
      rc = ph_value_dwadam(e, rows, policy_step, s);
    } else {
      rc = ph_value_backward(e, rows, false, s);
      if (!rc) rc = value_apply(e, policy_step, 1.0f, s, rows);
    }
    e->pregather = nullptr;
    if (rc) return rc;
  }
  const bool pol = learn && policy_step;
  if (defer_policy_fwd && !pol && learn) {
    // run graphs: the next step's forward launch carries this step's policy-loss forward (see ph_forward)
    e->pending_pc.on = true; e->pending_pc.xs = e->xcs; e->pending_pc.ga = e->gen_action;
    e->pending_pc.run_off = e->run_off; e->pending_pc.slot = e->run_off;
    e->hist_pol_count[e->run_off] = rows; e->hist_pol_add[e->run_off] = 0;
  } else if ((rc = ph_policy(e, rows, pol, !e->comm, s, !learn))) {
    return rc;
  }
  if (pol && e->comm) {   // the L1 clip quirk acts on the REDUCED actor gradient
    if ((rc = net_allreduce(e, RECNN_NET_POLICY, "allreduce_actor", s))) return rc;
    if ((rc = policy_apply(e, true, e->comm_scale, s, false))) return rc;
  } else if (pol && (rc = policy_apply(e, true, 1.0f, s, true))) {
    return rc;
  }
  return ph_finish(e, rows, learn, pol, s);
}
}  // namespace recnn_eng

