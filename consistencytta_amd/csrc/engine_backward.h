// What the backward passes of the U-Net (engine_unet_train.h) and of the VAE decoder (engine_vae.hip) share: the gradient
// context, the leaf operators (data gradients, GroupNorm backward) and the weight-gradient jobs, which launch from the plan
// of wgrad_plan.hip.  Gradients are ACCUMULATED into the caller's fp32 tensors (same names / shapes as the state dict),
// i.e. `.grad` semantics; the caller zeroes them.  Activation gradients travel in bf16.
#pragma once
#include "engine_common.h"
#include "wgrad_plan.h"

// Weight-gradient jobs (transposed im2col, the split-M GEMM, the scatter into the caller's gradient tensors) of a handle
// that owns one of these run on a SECOND stream: the data-gradient chain on the caller's stream is the critical path of the
// backward pass, its thin batch-9 launches leave CUs idle, and a layer's weight gradient depends on nothing that comes
// after it.  Each job owns one of NS scratch slots (dY^T is written by the main stream, everything else by the side
// stream); events order slot reuse and the joins at block boundaries.  Option "wgrad_stream" = 0 keeps everything on one
// stream.  (The U-Net has one; the VAE decoder's jobs run on the caller's stream out of its arena.)
struct WgradSide {
  static constexpr int NS = 2;
  hipStream_t stream = nullptr;
  Arena slot[NS];
  char* base = nullptr;
  hipEvent_t ready[NS] = {nullptr, nullptr}, freed[NS] = {nullptr, nullptr}, joined = nullptr;
  bool in_use[NS] = {false, false};
  bool dirty = false;     // side stream has work the main stream has not joined yet
  hipStream_t joined_on = nullptr;   // the main stream that last joined the side stream (see unet_backward_begin_impl)
  bool was_capturing = false;        // whether the previous backward was recorded into a hipGraph capture
  int next = 0;
  bool enabled = false;
};

// The engines' contexts derive from this one; a forward pass uses B and gn_need only.
struct GradCtx : RunCtx {
  int B;
  size_t gn_need = 0;                          // largest GroupNorm scratch a call of this pass asked for
  int norm_groups = 0;                         // groups of the engine's GroupNorm layers
  const GradTable* grads = nullptr;            // the caller's gradient tensors
  bool params = false;                         // parameter gradients are wanted (VAE forward: keep what they read)
  const char* who = "";                        // entry name in error texts
  WgradSide* side = nullptr;                   // null: weight-gradient jobs run on c.stream out of c.arena
  const ctta_wgrad_policy* policy = nullptr;   // the engine's weight-gradient policy
};

static ctta_status grad_ptr(GradCtx& c, const std::string& key, float** out) {
  *out = nullptr;
  if (c.dry) return CTTA_OK;
  auto it = c.grads->map.find(key);
  if (it == c.grads->map.end() || !it->second) {
    ctta_set_error("%s: no gradient tensor for '%s'", c.who, key.c_str());
    return CTTA_ERR_MISSING_KEY;
  }
  *out = it->second;
  return CTTA_OK;
}

// ------------------------------------------------------------------------------ data gradients, norms
static ctta_status conv_dgrad(GradCtx& c, const ConvLayer& D, const bf16_t* dy, int Hdy, int Wdy, bf16_t* dx, int Hout,
                              int Wout, bool accumulate) {
  ctta_conv_desc d;
  desc_init(&d);
  d.x0 = dy; d.c0 = D.cin_pad;
  d.batch = c.B; d.hi = Hdy; d.wi = Wdy; d.ho = Hout; d.wo = Wout;
  d.kh = D.kh; d.kw = D.kw; d.pad_h = d.pad_w = D.pad;
  d.w = D.p.w; d.k_pad = D.p.k_pad; d.n = D.p.n;
  d.out = dx; d.ldc = D.cout; d.accumulate = accumulate ? 1 : 0;
  RUN(c, ctta_conv_gemm(&d, c.stream));
  return CTTA_OK;
}
// dx [rows][ldx] (first n_out columns written) (+)= dy[:, :k] * W   with dy row stride dy_ld
static ctta_status linear_dgrad(GradCtx& c, const PackedW& D, const bf16_t* dy, int dy_k, int dy_ld, int64_t rows, bf16_t* dx,
                                int n_out, int ldx, bool accumulate) {
  ctta_conv_desc d;
  desc_init(&d);
  d.x0 = dy; d.c0 = dy_k; d.x_stride = dy_ld;
  d.batch = 1; d.hi = (int)rows; d.wi = 1; d.ho = (int)rows; d.wo = 1;
  d.w = D.w; d.k_pad = D.k_pad; d.n = n_out;
  d.out = dx; d.ldc = ldx; d.accumulate = accumulate ? 1 : 0;
  RUN(c, ctta_conv_gemm(&d, c.stream));
  return CTTA_OK;
}

// d gamma / d beta are added to the caller's tensors when the context wants parameter gradients
static ctta_status gn_backward(GradCtx& c, const GNLayer& g, const bf16_t* x, const bf16_t* dy, bf16_t* dx, int hw,
                               const float* stats, bool silu, bool accumulate_dx) {
  const size_t need = ctta_groupnorm_bwd_scratch_floats(c.B, hw, g.c, c.norm_groups);
  if (need > c.gn_need) c.gn_need = need;
  if (!c.dry && need > c.gn_scratch_floats) { ctta_set_error("groupnorm backward scratch too small"); return CTTA_ERR_INVALID; }
  float *dg = nullptr, *db = nullptr;
  if (c.params) {
    CTTA_TRY(grad_ptr(c, g.key + "weight", &dg));
    CTTA_TRY(grad_ptr(c, g.key + "bias", &db));
  }
  RUN(c, ctta_groupnorm_bwd(x, dy, dx, c.B, hw, g.c, c.norm_groups, stats, g.gamma, g.beta, silu ? 1 : 0, accumulate_dx ? 1 : 0,
                            dg, db, dg ? 1 : 0, c.gn_scratch, c.stream));
  return CTTA_OK;
}

// ------------------------------------------------------------------------------ weight-gradient jobs
// One weight-gradient job: `w` is the context its launches use -- with a side object a scratch slot as arena (and the side
// stream when enabled), without one the caller's own arena between a mark and a release.
struct WgJob {
  GradCtx w;
  int slot = 0;
  bool async = false;
  size_t mark = 0;
};
static ctta_status wg_begin(GradCtx& c, WgJob* j) {
  j->w = c;
  if (!c.side) { j->mark = c.arena->mark(); return CTTA_OK; }
  WgradSide& W = *c.side;
  j->slot = W.next;
  W.next = (W.next + 1) % WgradSide::NS;
  // ("wgrad_stream" is read per job: switched off between two backward passes -- bench.py's profiled step, whose per-launch
  // event brackets must not overlap -- the jobs run on the caller's stream in the same slots; the handle's arena policy,
  // W.enabled, was fixed when it was created)
  j->async = !c.dry && W.enabled && W.stream != nullptr && ctta_opt(CTTA_OPT_WGRAD_STREAM) != 0;
  j->w.arena = &W.slot[j->slot];
  W.slot[j->slot].reset();
  if (!j->async && !c.dry && W.in_use[j->slot]) {      // a side-stream job of an earlier pass may still own the slot
    CTTA_CHECK_HIP(hipStreamWaitEvent(c.stream, W.freed[j->slot], 0));
    W.in_use[j->slot] = false;
  }
  if (j->async) {
    j->w.stream = W.stream;
    // the slot's previous job must have drained before the main stream writes dY^T into it.  Jobs that read their operands
    // in place (ctta_wgrad_tn) never touch the slot from the main stream, but they keep this wait: it is the back-pressure
    // that lets the main stream run at most two jobs ahead of the side stream.  Without it the main stream races to the
    // block's wg_join and idles there while the side stream drains alone: 92.4 vs 83.9 ms per pipelined step (round 4).
    if (W.in_use[j->slot]) CTTA_CHECK_HIP(hipStreamWaitEvent(c.stream, W.freed[j->slot], 0));
  }
  return CTTA_OK;
}
// dY^T is in the slot (written on the main stream): hand over to the side stream
static ctta_status wg_handoff(GradCtx& c, WgJob& j) {
  if (!j.async) return CTTA_OK;
  WgradSide& W = *c.side;
  CTTA_CHECK_HIP(hipEventRecord(W.ready[j.slot], c.stream));
  CTTA_CHECK_HIP(hipStreamWaitEvent(W.stream, W.ready[j.slot], 0));
  return CTTA_OK;
}
static ctta_status wg_end(GradCtx& c, WgJob& j) {
  if (!c.side) c.arena->release(j.mark);
  if (!j.async) return CTTA_OK;
  WgradSide& W = *c.side;
  CTTA_CHECK_HIP(hipEventRecord(W.freed[j.slot], W.stream));
  W.in_use[j.slot] = true;
  W.dirty = true;
  return CTTA_OK;
}
// the main stream waits for every weight-gradient job issued so far (block boundaries: the caller may start the
// all-reduce of the block's gradients; before the embedding MLPs, which read d temb)
static ctta_status wg_join(GradCtx& c) {
  if (c.dry || !c.side || !c.side->dirty) return CTTA_OK;
  WgradSide& W = *c.side;
  CTTA_CHECK_HIP(hipEventRecord(W.joined, W.stream));
  CTTA_CHECK_HIP(hipStreamWaitEvent(c.stream, W.joined, 0));
  W.dirty = false;
  W.joined_on = c.stream;
  return CTTA_OK;
}

// One layer's geometry as the plan takes it: x NHWC with `C` channels at H x W (ups: before the x2), dy [B * ho * wo][N].
// (layer_wgrad fills in what depends on the job and on the pack map.)
static ctta_wgrad_geom wgrad_geom(int B, int kh, int kw, int C, int H, int W, bool ups, int stride, int pad, int N, int nb) {
  ctta_wgrad_geom g;
  memset(&g, 0, sizeof(g));
  g.kh = kh; g.kw = kw; g.c = C; g.batch = B;
  g.hi = ups ? 2 * H : H; g.wi = ups ? 2 * W : W; g.upsample = ups ? 1 : 0;
  g.ho = (g.hi + 2 * pad - kh) / stride + 1; g.wo = (g.wi + 2 * pad - kw) / stride + 1;
  g.stride = stride; g.pad = pad; g.n = N; g.nb = nb;
  return g;
}

// Runs the plan's route: *slabs_p [S][N][ld] in the job's scratch, or NULL after a direct route (the kernel added its tiles
// straight into the gradient tensors of `dm`: nothing to scatter).  `cm` is the main context: dY lives in its arena, and a
// dY^T copy is written by ITS stream, so wg_handoff comes after that transpose and before the job's first own launch.
static ctta_status wgrad_launch(GradCtx& cm, WgJob& job, const ctta_wgrad_geom& g, const ctta_wgrad_plan_info& pl,
                                const bf16_t* x, const bf16_t* dy, const PackMap* dm, float** slabs_p) {
  GradCtx& c = job.w;
  Arena& A = *c.arena;
  const int C = g.c, N = g.n, B = g.batch, S = pl.splits, mp = pl.mp, ld = pl.ld, K = g.kh * g.kw * C;
  const int M = B * g.ho * g.wo;
  const int64_t stride = (int64_t)N * ld;
  bf16_t *q = nullptr, *pt = nullptr, *xu = nullptr;
  float* slabs = nullptr;
  if (pl.q) { q = A.get<bf16_t>((size_t)pl.q); ALLOC_OR_FAIL(q); }
  if (pl.pt) { pt = A.get<bf16_t>((size_t)pl.pt); ALLOC_OR_FAIL(pt); }
  if (pl.slabs) { slabs = A.get<float>((size_t)pl.slabs); ALLOC_OR_FAIL(slabs); }
  if (pl.xu) { xu = A.get<bf16_t>((size_t)pl.xu); ALLOC_OR_FAIL(xu); }
  *slabs_p = slabs;
  float *gw = nullptr, *gb = nullptr;
  if (!slabs) {
    CTTA_TRY(grad_ptr(c, dm->wkey, &gw));
    if (!dm->bkey.empty()) CTTA_TRY(grad_ptr(c, dm->bkey, &gb));
  }
  if (pt) RUN(cm, ctta_transpose_bf16(dy, 0, M, N, N, 0, pt, 0, mp, 1, cm.stream));
  CTTA_TRY(wg_handoff(cm, job));
  if (xu) {
    RUN(c, ctta_upsample2_nearest(x, xu, B, g.hi / 2, g.wi / 2, C, c.stream));
    x = xu;
  }
  switch (pl.route) {
    case CTTA_WGRAD_TN:
      RUN(c, ctta_wgrad_tn(dy, N, N, x, C, C, M, mp, S, K, slabs, stride, ld, c.stream));
      break;
    case CTTA_WGRAD_TN_DIRECT:
      RUN(c, ctta_wgrad_tn_direct(dy, N, N, x, C, C, M, mp, dm->k_ident > 0 ? dm->k_ident : K, dm->n, dm->ro,
                                  dm->k_ident > 0 ? nullptr : dm->co, gw, dm->n_bias, dm->bidx, gb, c.stream));
      break;
    case CTTA_WGRAD_IMPLICIT_INPLACE:
      RUN(c, ctta_wgrad_implicit_inplace(dy, N, N, mp, x, C, C, B, g.hi, g.wi, 9, M, S, K, g.nb, slabs, stride, ld, c.stream));
      break;
    case CTTA_WGRAD_IMPLICIT_DIRECT:
      RUN(c, ctta_wgrad_implicit_direct(dy, N, N, mp, x, C, C, B, g.hi, g.wi, M, dm->k_ident, dm->n, dm->ro, gw, dm->n_bias, dm->bidx,
                                        gb, c.stream));
      break;
    case CTTA_WGRAD_IMPLICIT_DYT:
      RUN(c, ctta_wgrad_implicit(pt, N, mp, x, C, C, B, g.hi, g.wi, 9, M, S, K, g.nb, slabs, stride, ld, c.stream));
      break;
    default: {   // CTTA_WGRAD_IM2COL_T
      RUN(c, ctta_im2col_t(x, C, B, g.hi, g.wi, g.upsample, g.ho, g.wo, g.kh, g.kw, g.stride, g.pad, g.pad, 1, q, mp, g.nb, c.stream));
      ctta_conv_desc d;
      desc_init(&d);
      d.x0 = pt; d.c0 = pl.seg; d.x_stride = mp;
      d.batch = 1; d.hi = N; d.wi = 1; d.ho = N; d.wo = 1;
      d.w = q; d.k_pad = mp; d.n = pl.sums_apart ? K : pl.rows;
      d.out = slabs; d.ldc = ld; d.out_f32 = 1;
      d.groups = S; d.x_group_stride = pl.seg; d.w_group_stride = pl.seg; d.out_group_stride = stride;
      if (job.async) ctta_conv_suppress_splitk(1);   // the handle's split-K slabs belong to the main stream's launches
      const ctta_status gst = c.dry ? CTTA_OK : ctta_conv_gemm(&d, c.stream);
      if (job.async) ctta_conv_suppress_splitk(0);
      CTTA_TRY(gst);
      if (pl.sums_apart) RUN(c, ctta_wgrad_rowsum(pt, N, mp, M, S, g.ho * g.wo, g.nb, slabs, stride, ld, K, c.stream));
    }
  }
  return CTTA_OK;
}

// slab rows [row0, row0 + m.n) -> weight / bias gradients of the layer described by `m` (split slabs folded in slab
// order: no atomics)
static ctta_status scatter_wgrad(GradCtx& c, const float* slabs, const ctta_wgrad_geom& g, const ctta_wgrad_plan_info& pl,
                                 const PackMap& m, int row0 = 0) {
  const int64_t stride = (int64_t)g.n * pl.ld;
  const float* base = slabs + (size_t)row0 * pl.ld;
  const int k_rows = g.kh * g.kw * g.c;
  float *gw, *gb = nullptr;
  CTTA_TRY(grad_ptr(c, m.wkey, &gw));
  if (!m.bkey.empty()) CTTA_TRY(grad_ptr(c, m.bkey, &gb));
  // weight rows and (same launch) the bias column of the slabs
  const bool bias_here = !m.bkey.empty() && m.n_bias <= m.n;
  const int bcol = bias_here ? k_rows : -1;
  RUN(c, ctta_wgrad_scatter_rows_bias(base, pl.splits, stride, pl.ld, m.k_ident > 0 ? m.k_ident : k_rows, m.n, m.ro,
                                      m.k_ident > 0 ? nullptr : m.co, gw, bcol, m.n_bias, m.bidx, gb, 1, c.stream));
  if (!m.bkey.empty() && !bias_here)
    RUN(c, ctta_col_scatter(base, pl.splits, stride, pl.ld, k_rows, 1, m.n_bias, m.bidx, gb, 0, 1, c.stream));
  return CTTA_OK;
}

// The whole job of one layer: plan, launch, scatter into the gradients of `m` (and of `m2`, whose rows follow m's in a fused
// operand).  `more` runs inside the job, after the scatter, with the job's context and the slabs.
struct WgradDone { const ctta_wgrad_geom& g; const ctta_wgrad_plan_info& pl; const float* slabs; };
template <typename More>
static ctta_status layer_wgrad(GradCtx& c, ctta_wgrad_geom g, const PackMap& m, const PackMap* m2, const bf16_t* x,
                               const bf16_t* dy, More more) {
  if (!c.params) return CTTA_OK;   // the caller wants no parameter gradients of the base network (U-Net: frozen-base mode)
  WgJob job;
  CTTA_TRY(wg_begin(c, &job));
  // the DIRECT form needs the whole slab row to belong to one pack map whose rows the kernel can place itself: the 1x1
  // kernel scatters through a linear's column map too, the 3x3 one needs the identity map of a convolution
  const PackMap* dm = g.nb == 0 && !m2 ? &m : nullptr;
  g.direct_ok = dm && m.n <= g.n && (m.bkey.empty() || m.n_bias <= m.n) && (g.kh * g.kw == 1 || m.k_ident > 0);
  g.run_async = job.async ? 1 : 0;
  g.keeps_dy = c.side && c.side->enabled ? 1 : 0;
  ctta_wgrad_plan_info pl;
  CTTA_TRY(ctta_wgrad_plan(&g, c.policy, &pl));
  float* slabs;
  CTTA_TRY(wgrad_launch(c, job, g, pl, x, dy, dm, &slabs));
  if (slabs) CTTA_TRY(scatter_wgrad(job.w, slabs, g, pl, m));      // NULL: the kernel added into the gradients itself
  if (m2) CTTA_TRY(scatter_wgrad(job.w, slabs, g, pl, *m2, m.n));
  CTTA_TRY(more(job.w, WgradDone{g, pl, slabs}));
  return wg_end(c, job);
}

// dW / db of one convolution.  x: the layer's input, NHWC with L.cin_pad channels at H x W (ups: before the x2); dy has
// L.p.n channels
static ctta_status conv_wgrad(GradCtx& c, const ConvLayer& L, const PackMap& m, const bf16_t* x, int H, int W, bool ups,
                              const bf16_t* dy) {
  return layer_wgrad(c, wgrad_geom(c.B, L.kh, L.kw, L.cin_pad, H, W, ups, L.stride, L.pad, L.p.n, 0), m, nullptr, x, dy,
                     [](GradCtx&, const WgradDone&) { return CTTA_OK; });
}
// linear y = x W^T (+b): x [rows][x_ld] (the first k_rows columns are the GEMM K), dy [rows][N]; m2: fused [q | k]
static ctta_status linear_wgrad(GradCtx& c, const PackMap& m, const PackMap* m2, const bf16_t* x, int x_ld, int64_t rows,
                                const bf16_t* dy, int N) {
  return layer_wgrad(c, wgrad_geom(1, 1, 1, x_ld, (int)rows, 1, false, 1, 0, N, 0), m, m2, x, dy,
                     [](GradCtx&, const WgradDone&) { return CTTA_OK; });
}
