// U-Net engine: builds the layer graph of UNet2DConditionGuidedModel / UNet2DConditionModel
// from a config + state dict, pre-packs weights for conv_gemm, and runs the forward pass on a
// private activation arena.  Reference call order:
//   unet_2d_condition_guided.py:716-945 (forward), unet_2d_blocks.py:912-972 (CrossAttnDown),
//   :1027-1058 (Down), :588-609 (Mid), :2017-2078 (CrossAttnUp), :2129-2159 (Up),
//   resnet.py:549-597 (ResnetBlock2D), transformer_2d.py:218-332, attention.py:276-334.
//
// Data layout in HBM: activations NHWC bf16, i.e. a (B, H*W, C) token matrix, so the
// transformer blocks run on the conv activations without any permute.  The transformer's
// hidden width `inner = heads * (C // heads)` (255/510/1020 in the light config) is padded to a
// multiple of 64 (`cp`), heads are padded from dh to 64 lanes (`hp = heads*64`) by zero rows /
// columns placed at weight-packing time, so no kernel ever sees an odd width.
#include "engine_backward.h"

#include <stdlib.h>

#include <math.h>

__global__ void add_silu_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                float* __restrict__ out, float* __restrict__ sum_out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = a[i] + (b ? b[i] : 0.f);
  if (sum_out) sum_out[i] = v;
  out[i] = v / (1.0f + expf(-v));
}
// (B,L) u8 keep-mask -> additive bias (1-m)*-10000 (unet_2d_condition_guided.py:793-795)
__global__ void mask_bias_kernel(const uint8_t* __restrict__ m, float* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (1.0f - (m[i] ? 1.0f : 0.0f)) * -10000.0f;
}
// (B,L,X) f32 -> (B,Lp,Xp) bf16, zero padded
__global__ void pack_enc_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int B, int L,
                                int X, int Lp, int Xp) {
  const long long total = (long long)B * Lp * Xp;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(i % Xp);
    const long long r = i / Xp;
    const int l = (int)(r % Lp);
    const int b = (int)(r / Lp);
    dst[i] = (l < L && x < X) ? f2bf(src[((size_t)b * L + l) * X + x]) : (bf16_t)0;
  }
}
// (n, c, kh, kw) f32 -> (n, kh, kw, c) f32 for the direct small-N convolution
__global__ void repack_small_w_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, int c,
                                      int khw) {
  const int total = n * c * khw;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int cc = i % c;
  const int t = (i / c) % khw;
  const int nn = i / (c * khw);
  dst[i] = src[((size_t)nn * c + cc) * khw + t];
}

// Training-only companions of a conv / linear: the data-gradient operand and the pack map that
// routes the weight-gradient slab back into the state-dict layout.
struct ConvTrain { ConvLayer d; PackMap m; };
struct LinTrain { PackedW d; PackMap m; };

struct Resnet {
  int cin = 0, cout = 0, temb_off = 0;
  GNLayer n1, n2;
  ConvLayer c1, c2, sc;
  bool has_sc = false;
  std::string key;
  ConvTrain t1, t2, tsc;
  // tensors the training forward keeps for the backward pass
  struct Saved { const bf16_t *x = nullptr, *a = nullptr, *t1 = nullptr, *a2 = nullptr; float *st1 = nullptr, *st2 = nullptr; int H = 0, W = 0; } sv;
};

struct LNLayer { float* gamma = nullptr; float* beta = nullptr; std::string key; };

// LoRA adapter of one attention projection (lora.hip): y = W x + up(down(x)).  Packed through the maps of the base layer at
// the same site, zeros in every padded row / column: a = down.weight as [r][k_pad], b = up.weight as [n_pad][r], both fp32.
// The activations these read carry exact zeros in their padded columns (products with zero weight rows, LayerNorm's
// explicit zeros), so padding contributes nothing.  kmap / nmap (device) send a padded column back to its place in the
// parameter, or to -1: the weight-gradient kernel drops padding through them.
struct LoraSite {
  std::string key;   // "...attn1.processor.to_q_lora."
  float *a = nullptr, *b = nullptr;
  int32_t *kmap = nullptr, *nmap = nullptr;
  int k = 0, n = 0, k_pad = 0, n_pad = 0;
  float* d = nullptr;   // down(x) [rows][r] of the training forward, kept for the backward pass
  // per-request adapters (ctta_unet_adapter_bank): `slots` copies of a / b in the same packed layout, zeros where never loaded
  float *bank_a = nullptr, *bank_b = nullptr;
};

struct Transformer {
  int c = 0, heads = 0, dh = 0, inner = 0, cp = 0, hp = 0, ffh = 0, ffp = 0;
  GNLayer norm;
  PackedW proj_in, qk1, v1, out1, q2, k2, v2, out2, ff1, ff2, proj_out;
  LNLayer ln1, ln2, ln3;
  bf16_t *k2c = nullptr, *vt2c = nullptr;   // persistent cross-attention K / V^T of the text states (text cache)
  bf16_t* ffn_stream = nullptr;             // ff1 / ff2 as per-wave weight streams of the fused feed-forward (ffn_fused.hip)
  bool want_proj_stream = false;
  bf16_t* front_stream = nullptr;           // ... and attn2.to_out as its front projection
  bf16_t* proj_stream = nullptr;            // ... and proj_out as its tail projection (when its width is the block's padded inner width)
  LinTrain t_proj_in, t_q1, t_k1, t_v1, t_out1, t_q2, t_k2, t_v2, t_out2, t_ff1, t_ff2, t_proj_out;
  LoraSite lq1, lk1, lv1, lo1, lq2, lk2, lv2, lo2;   // used when the handle has adapters (ctta_unet::lora_r > 0)
  struct Saved {
    const bf16_t *x = nullptr, *g = nullptr, *s0 = nullptr, *n1 = nullptr, *qk = nullptr, *vt = nullptr, *att1 = nullptr,
                 *s1 = nullptr, *n2 = nullptr, *q2 = nullptr, *k2 = nullptr, *vt2 = nullptr, *att2 = nullptr, *s2 = nullptr,
                 *n3 = nullptr, *f = nullptr, *gg = nullptr, *s3 = nullptr;
    float *st = nullptr, *lse1 = nullptr, *lse2 = nullptr;   // GroupNorm stats, attention log-sum-exps
    int H = 0, W = 0;
  } sv;
};

struct Level {
  std::vector<Resnet> res;
  std::vector<Transformer> att;
  bool has_sampler = false;
  ConvLayer sampler;
  ConvTrain tsampler;
};

// One entry per layer the training forward ran, replayed in reverse by the backward pass.
struct TapeOp {
  enum Kind { CONV_IN, SKIP_PUSH, RESNET, TRANSFORMER, DOWNSAMPLE, CONCAT, UPSAMPLE } kind;
  Resnet* R = nullptr;
  Transformer* T = nullptr;
  Level* Lv = nullptr;
  const bf16_t* x = nullptr;   // layer input (samplers, conv_in)
  int H = 0, W = 0, ch = 0, skc = 0, skip_idx = -1;
  int block = 0;   // 0 conv_in (+ embeddings), 1..n down blocks, n+1 mid, n+2.. up blocks
};

struct ctta_unet : EngineBase {
  ctta_unet_config cfg;
  std::vector<Level> down, up;
  Resnet mid_r0, mid_r1;
  Transformer mid_att;
  ConvLayer conv_in;
  GNLayer norm_out;
  ConvLayer conv_out;            // bf16 pack for conv_gemm (round 3: 256x32 MFMA tile, ~4x the direct kernel at batch 32)
  float* conv_out_w = nullptr;   // fp32 [cout][3][3][c0] for the direct small-N kernel (CTTA_CONV_OUT_DIRECT=1)
  float* conv_out_b = nullptr;
  // embeddings (fp32)
  float *freqs = nullptr, *t_w1 = nullptr, *t_b1 = nullptr, *t_w2 = nullptr, *t_b2 = nullptr;
  float *g_proj = nullptr, *g_w1 = nullptr, *g_b1 = nullptr, *g_w2 = nullptr, *g_b2 = nullptr;
  float *temb_w = nullptr, *temb_b = nullptr;
  int temb_dim = 0, temb_total = 0, cin_pad = 0, xp = 0;
  int lora_r = 0;   // rank of the attention-projection adapters; 0: the weight table named none, and no launch differs
  // ctta_unet_set_lora: which passes take the fused site kernels (lora.hip) where those take the shapes -- bit 0 the
  // backward groups, bit 1 the forward groups -- and the adapter strength y = W x + lora_scale * up(down(x)); read by the
  // next forward, whose values its backward uses (ts below).  The forward groups are off by default: ctta_lora_sites_fwd
  // measured slower than the launches it replaces (profiles/lora_step.txt).
  int lora_fused = 1;
  float lora_scale = 1.0f;
  // Per-request adapters: one allocation behind every site's bank_a / bank_b, and the caller's device arrays of
  // ctta_unet_set_adapter_rows (read by the kernels, never by the host).  row_slot == nullptr: no launch differs.
  float* bank_base = nullptr;
  int bank_slots = 0;
  const int32_t* row_slot = nullptr;
  const float* row_scale = nullptr;
  // Text cache: the cross-attention K / V^T projections of the text states (32 small GEMMs per forward) live in
  // persistent buffers; a caller that queries the same handle again with the SAME text states and mask (the second CFG
  // teacher query of a distillation step, every query of the Heun teacher loop) says so with ctta_unet_reuse_text and
  // the forward skips them.  Invalidated by ctta_unet_load_weights.
  char* tc_base = nullptr;
  bool tc_valid = false, tc_reuse_next = false;
  int tc_B = 0, tc_L = 0;
  // ---- training state (cfg.enable_training)
  ConvTrain t_conv_in, t_conv_out;
  std::vector<TapeOp> tape;
  struct TrainSaved {
    bool valid = false;
    int B = 0, L = 0, Lp = 0, n_skips = 0;
    size_t arena_off = 0;
    const float *tfeat = nullptr, *t_h1pre = nullptr, *t_h1 = nullptr, *gfeat = nullptr, *g_h1pre = nullptr,
                *g_h1 = nullptr, *emb = nullptr, *emb_silu = nullptr;
    const bf16_t *enc_bf = nullptr, *xin = nullptr, *h_last = nullptr, *a_out = nullptr;
    const float *mask_bias = nullptr, *st_out = nullptr;
    int lora_fused = 1;
    float lora_scale = 1.0f;
  } ts;
  WgradSide wg;   // the weight-gradient side stream and its scratch slots (engine_backward.h)
  struct BackwardState {   // between ctta_unet_backward_begin / _next calls
    bool active = false;
    bf16_t* dh = nullptr;
    std::vector<bf16_t*> dskip;
    float* dtemb_all = nullptr;
    size_t pos = 0;
  } bw;
};

struct UCtx : GradCtx {
  ctta_unet* U;
  bool reuse_text = false;
  int L, Lp;
  const float* temb_all;
  const bf16_t* enc_bf;
  const float* mask_bias;
  bool train = false;
  bool lora_fused = false;   // the forward groups (bit 1 of the handle's setting)
  float lora_scale = 1.0f;
  const int32_t* row_slot = nullptr;   // per-request adapters: the rows kernels read the sites' banks through these
  const float* row_scale = nullptr;
};

static ctta_status make_resnet(ctta_unet* U, const std::string& p, int cin, int cout, Resnet* R) {
  WeightStore& ws = U->store;
  R->cin = cin; R->cout = cout; R->key = p;
  const bool tr = U->cfg.enable_training != 0;
  CTTA_TRY(make_gn(ws, p + "norm1.", cin, &R->n1));
  CTTA_TRY(make_conv(ws, p + "conv1.", cout, cin, cin, 3, 3, 1, 1, &R->c1, true, tr ? &R->t1.m : nullptr));
  CTTA_TRY(make_gn(ws, p + "norm2.", cout, &R->n2));
  CTTA_TRY(make_conv(ws, p + "conv2.", cout, cout, cout, 3, 3, 1, 1, &R->c2, true, tr ? &R->t2.m : nullptr));
  R->has_sc = cin != cout;
  if (R->has_sc) CTTA_TRY(make_conv(ws, p + "conv_shortcut.", cout, cin, cin, 1, 1, 1, 0, &R->sc, true, tr ? &R->tsc.m : nullptr));
  if (tr) {
    CTTA_TRY(make_conv_dgrad_from(ws, R->c1, cout, cin, &R->t1.d));
    CTTA_TRY(make_conv_dgrad_from(ws, R->c2, cout, cout, &R->t2.d));
    if (R->has_sc) CTTA_TRY(make_conv_dgrad_from(ws, R->sc, cout, cin, &R->tsc.d));
  }
  // time_emb_proj rows live in one concatenated fp32 table -> one small GEMM per forward
  R->temb_off = U->temb_total;
  CTTA_TRY(ws.add_copy_into(p + "time_emb_proj.weight", (int64_t)cout * U->temb_dim,
                            U->temb_w + (size_t)R->temb_off * U->temb_dim));
  CTTA_TRY(ws.add_copy_into(p + "time_emb_proj.bias", cout, U->temb_b + R->temb_off));
  U->temb_total += cout;
  return CTTA_OK;
}

static ctta_status make_ln(WeightStore& ws, const std::string& p, int d, LNLayer* L) {
  L->key = p;
  CTTA_TRY(ws.add_vector(p + "weight", d, &L->gamma));
  CTTA_TRY(ws.add_vector(p + "bias", d, &L->beta));
  return CTTA_OK;
}

static ctta_status make_lora_site(ctta_unet* U, const std::string& key, int n_src, int k_src, const std::vector<int32_t>& rows,
                                  const std::vector<int32_t>& cols, LoraSite* S) {
  WeightStore& ws = U->store;
  const int r = U->lora_r, n_pad = (int)rows.size(), k_pad = (int)cols.size();
  S->key = key; S->k = k_src; S->n = n_src; S->k_pad = k_pad; S->n_pad = n_pad;
  std::vector<WeightStore::Seg> sa, sb;
  auto push = [](std::vector<WeightStore::Seg>& v, int src, int dst, int count) {
    if (!v.empty() && v.back().src_start + v.back().count == src && v.back().dst_start + v.back().count == dst) v.back().count += count;
    else v.push_back({src, dst, count});
  };
  for (int j = 0; j < r; ++j)
    for (int k = 0; k < k_pad; ++k)
      if (cols[k] >= 0) push(sa, j * k_src + cols[k], j * k_pad + k, 1);
  for (int n = 0; n < n_pad; ++n)
    if (rows[n] >= 0) push(sb, rows[n] * r, n * r, r);
  CTTA_TRY(ws.add_vector(key + "down.weight", r * k_src, r * k_pad, sa, &S->a));
  CTTA_TRY(ws.add_vector(key + "up.weight", n_src * r, n_pad * r, sb, &S->b));
  CTTA_TRY(ws.upload(cols, &S->kmap));
  CTTA_TRY(ws.upload(rows, &S->nmap));
  return CTTA_OK;
}

static ctta_status make_transformer(ctta_unet* U, const std::string& p, int c, int heads, Transformer* T) {
  WeightStore& ws = U->store;
  const int dh = c / heads, inner = heads * dh;   // unet_2d_blocks.py:873-875
  CTTA_REQUIRE(dh >= 1 && dh <= 64, "attention head dim %d outside [1,64]", dh);
  const int cp = round_up(inner, 64), hp = heads * 64;
  const int ffh = inner * 4, ffp = round_up(ffh, 64);
  const int X = U->cfg.cross_attention_dim, xp = U->xp;
  T->c = c; T->heads = heads; T->dh = dh; T->inner = inner; T->cp = cp; T->hp = hp; T->ffh = ffh; T->ffp = ffp;
  CTTA_TRY(make_gn(ws, p + "norm.", c, &T->norm));
  const std::string t = p + "transformer_blocks.0.";
  const auto hmap = head_pad_map(heads, dh);
  const auto in_cols = identity_map(inner, cp);
  const bool tr = U->cfg.enable_training != 0;
  // forward pack (+ pack map and data-gradient pack when training)
  auto lin = [&](const std::string& wkey, const std::string& bkey, int n_src, int k_src,
                 const std::vector<int32_t>& rows, const std::vector<int32_t>& cols, PackedW* P, LinTrain* LT,
                 bf16_t* pre = nullptr, bool need_dgrad = true) -> ctta_status {
    CTTA_TRY(make_linear(ws, wkey, bkey, n_src, k_src, rows, cols, P, pre, tr ? &LT->m : nullptr));
    if (tr && need_dgrad) CTTA_TRY(make_linear_dgrad_from(ws, P->w, P->n, P->k_pad, &LT->d));
    return CTTA_OK;
  };
  CTTA_TRY(lin(p + "proj_in.weight", p + "proj_in.bias", inner, c, identity_map(inner, cp),
               identity_map(c, round_up(c, 64)), &T->proj_in, &T->t_proj_in));
  {  // self-attention q and k packed back to back -> one fused [q | k] GEMM
    bf16_t* qk = ws.arena.get<bf16_t>((size_t)2 * hp * cp);
    if (!qk) { ctta_set_error("weight store exhausted"); return CTTA_ERR_NOMEM; }
    PackedW pq, pk;
    CTTA_TRY(lin(t + "attn1.to_q.weight", "", inner, inner, hmap, in_cols, &pq, &T->t_q1, qk));
    CTTA_TRY(lin(t + "attn1.to_k.weight", "", inner, inner, hmap, in_cols, &pk, &T->t_k1, qk + (size_t)hp * cp));
    T->qk1.w = qk; T->qk1.bias = nullptr; T->qk1.n = 2 * hp; T->qk1.k_pad = cp;
  }
  CTTA_TRY(lin(t + "attn1.to_v.weight", "", inner, inner, hmap, in_cols, &T->v1, &T->t_v1));
  CTTA_TRY(lin(t + "attn1.to_out.0.weight", t + "attn1.to_out.0.bias", inner, inner, identity_map(inner, cp), hmap,
               &T->out1, &T->t_out1));
  CTTA_TRY(lin(t + "attn2.to_q.weight", "", inner, inner, hmap, in_cols, &T->q2, &T->t_q2));
  // the text states carry no gradient: no data-gradient packs for attn2.to_k / to_v
  CTTA_TRY(lin(t + "attn2.to_k.weight", "", inner, X, hmap, identity_map(X, xp), &T->k2, &T->t_k2, nullptr, false));
  CTTA_TRY(lin(t + "attn2.to_v.weight", "", inner, X, hmap, identity_map(X, xp), &T->v2, &T->t_v2, nullptr, false));
  CTTA_TRY(lin(t + "attn2.to_out.0.weight", t + "attn2.to_out.0.bias", inner, inner, identity_map(inner, cp), hmap,
               &T->out2, &T->t_out2));
  {  // GEGLU projection (attention.py:430-432), rows interleaved in 16-blocks [16 value][16 gate] so that the fused
     // GEMM epilogue finds value and gate of a hidden unit in adjacent accumulator fragments
    std::vector<int32_t> rows(2 * ffp, -1);
    for (int i = 0; i < ffh; ++i) { rows[(i / 16) * 32 + i % 16] = i; rows[(i / 16) * 32 + 16 + i % 16] = ffh + i; }
    CTTA_TRY(lin(t + "ff.net.0.proj.weight", t + "ff.net.0.proj.bias", 2 * ffh, inner, rows, in_cols, &T->ff1, &T->t_ff1));
  }
  CTTA_TRY(lin(t + "ff.net.2.weight", t + "ff.net.2.bias", inner, ffh, identity_map(inner, cp), identity_map(ffh, ffp),
               &T->ff2, &T->t_ff2));
  // 256- / 512-wide blocks: the inference forward runs ff1 -> GEGLU -> ff2 + residual as ONE row-tile launch (ctta_ffn_geglu)
  // that streams both matrices in its own layout; the copy is re-derived from the packed operands after every (re)load
  if (ctta_ffn_geglu_supported(cp, ffp) && T->ff1.k_pad >= cp && T->ff2.k_pad >= ffp) {
    T->ffn_stream = reinterpret_cast<bf16_t*>(ws.arena.get<unsigned char>(ctta_ffn_pack_bytes(cp, ffp)));
    if (!T->ffn_stream) { ctta_set_error("weight store exhausted (feed-forward weight streams)"); return CTTA_ERR_NOMEM; }
    const bf16_t *w1 = T->ff1.w, *w2 = T->ff2.w;
    const int k1 = T->ff1.k_pad, k2 = T->ff2.k_pad;
    bf16_t* dst = T->ffn_stream;
    ws.jobs.push_back([=](const WeightTable&, hipStream_t s) -> ctta_status { return ctta_ffn_pack(w1, k1, w2, k2, cp, ffp, dst, s); });
    T->want_proj_stream = true;
  }
  if (U->lora_r > 0) {   // adapters: the output side of q / k / v and the input side of to_out are head padded
    const auto out_rows = identity_map(inner, cp), x_cols = identity_map(X, xp);
    CTTA_TRY(make_lora_site(U, t + "attn1.processor.to_q_lora.", inner, inner, hmap, in_cols, &T->lq1));
    CTTA_TRY(make_lora_site(U, t + "attn1.processor.to_k_lora.", inner, inner, hmap, in_cols, &T->lk1));
    CTTA_TRY(make_lora_site(U, t + "attn1.processor.to_v_lora.", inner, inner, hmap, in_cols, &T->lv1));
    CTTA_TRY(make_lora_site(U, t + "attn1.processor.to_out_lora.", inner, inner, out_rows, hmap, &T->lo1));
    CTTA_TRY(make_lora_site(U, t + "attn2.processor.to_q_lora.", inner, inner, hmap, in_cols, &T->lq2));
    CTTA_TRY(make_lora_site(U, t + "attn2.processor.to_k_lora.", inner, X, hmap, x_cols, &T->lk2));
    CTTA_TRY(make_lora_site(U, t + "attn2.processor.to_v_lora.", inner, X, hmap, x_cols, &T->lv2));
    CTTA_TRY(make_lora_site(U, t + "attn2.processor.to_out_lora.", inner, inner, out_rows, hmap, &T->lo2));
  }
  CTTA_TRY(make_ln(ws, t + "norm1.", inner, &T->ln1));
  CTTA_TRY(make_ln(ws, t + "norm2.", inner, &T->ln2));
  CTTA_TRY(make_ln(ws, t + "norm3.", inner, &T->ln3));
  CTTA_TRY(lin(p + "proj_out.weight", p + "proj_out.bias", c, inner, identity_map(c, round_up(c, 4)), in_cols,
               &T->proj_out, &T->t_proj_out));
  if (T->want_proj_stream && T->out2.n == cp && T->out2.k_pad == hp && T->out2.bias && ctta_ffn_proj_pack_bytes(cp, hp)) {
    T->front_stream = reinterpret_cast<bf16_t*>(ws.arena.get<unsigned char>(ctta_ffn_proj_pack_bytes(cp, hp)));
    if (!T->front_stream) { ctta_set_error("weight store exhausted (front projection weight stream)"); return CTTA_ERR_NOMEM; }
    const bf16_t* w0 = T->out2.w;
    bf16_t* dst = T->front_stream;
    ws.jobs.push_back([=](const WeightTable&, hipStream_t s) -> ctta_status { return ctta_ffn_proj_pack(w0, hp, hp, cp, dst, s); });
  }
  if (T->want_proj_stream && T->proj_out.n == cp && T->proj_out.k_pad == cp && c == cp) {
    T->proj_stream = reinterpret_cast<bf16_t*>(ws.arena.get<unsigned char>(ctta_ffn_proj_pack_bytes(cp, cp)));
    if (!T->proj_stream) { ctta_set_error("weight store exhausted (projection weight stream)"); return CTTA_ERR_NOMEM; }
    const bf16_t* w3 = T->proj_out.w;
    bf16_t* dst = T->proj_stream;
    ws.jobs.push_back([=](const WeightTable&, hipStream_t s) -> ctta_status { return ctta_ffn_proj_pack(w3, cp, cp, cp, dst, s); });
  }
  return CTTA_OK;
}

// ------------------------------------------------------------------------------------ run
// GroupNorm (+SiLU); the training forward also keeps (mean, rstd) per (sample, group) for the backward pass
static ctta_status gn(UCtx& c, const GNLayer& g, const bf16_t* x, bf16_t* y, int hw, float eps, bool silu,
                      float** stats_out = nullptr) {
  const int groups = c.U->cfg.norm_num_groups;
  size_t need = ctta_groupnorm_scratch_floats(c.B, hw, g.c, groups);
  if (c.train) {
    const size_t nb = ctta_groupnorm_bwd_scratch_floats(c.B, hw, g.c, groups);
    if (nb > need) need = nb;
  }
  if (need > c.gn_need) c.gn_need = need;
  float* st = nullptr;
  if (c.train && stats_out) {   // (mean, rstd) per (sample, group), emitted by the forward's own fold
    st = c.arena->get<float>((size_t)c.B * groups * 2); ALLOC_OR_FAIL(st);
    *stats_out = st;
  }
  return run_gn(c, g, x, y, c.B, hw, groups, eps, silu, st);
}

static ctta_status run_resnet(UCtx& c, Resnet& R, const bf16_t* x, int H, int W, bf16_t** out_p) {
  Arena& A = *c.arena;
  const size_t M = (size_t)c.B * H * W;
  bf16_t* out = A.get<bf16_t>(M * R.cout); ALLOC_OR_FAIL(out);
  const size_t mk = A.mark();
  bf16_t* a = A.get<bf16_t>(M * R.cin); ALLOC_OR_FAIL(a);
  CTTA_TRY(gn(c, R.n1, x, a, H * W, c.U->cfg.norm_eps, true, &R.sv.st1));
  bf16_t* t1 = A.get<bf16_t>(M * R.cout); ALLOC_OR_FAIL(t1);
  CTTA_TRY(run_conv2d(c, R.c1, a, c.B, H, W, false, t1, c.temb_all + R.temb_off, c.U->temb_total, nullptr, 0));
  bf16_t* a2 = A.get<bf16_t>(M * R.cout); ALLOC_OR_FAIL(a2);
  CTTA_TRY(gn(c, R.n2, t1, a2, H * W, c.U->cfg.norm_eps, true, &R.sv.st2));
  if (c.train) { R.sv.x = x; R.sv.a = a; R.sv.t1 = t1; R.sv.a2 = a2; R.sv.H = H; R.sv.W = W; }
  const bf16_t* res = x;
  if (R.has_sc) {
    bf16_t* r = A.get<bf16_t>(M * R.cout); ALLOC_OR_FAIL(r);
    CTTA_TRY(run_conv2d(c, R.sc, x, c.B, H, W, false, r, nullptr, 0, nullptr, 0));
    res = r;
  }
  CTTA_TRY(run_conv2d(c, R.c2, a2, c.B, H, W, false, out, nullptr, 0, res, R.cout));
  A.release(mk);
  *out_p = out;
  return CTTA_OK;
}

static ctta_status run_attention(UCtx& c, const bf16_t* q, int q_ld, const bf16_t* k, int k_ld, int k_rows,
                                 const bf16_t* vt, int vt_ld, const float* bias, bf16_t* out, int out_ld,
                                 int heads, int nq, int nk, int dh, float** lse_out = nullptr) {
  float* lse = nullptr;
  if (c.train && lse_out) {   // the backward pass rebuilds the probabilities from the row log-sum-exp
    lse = c.arena->get<float>((size_t)c.B * heads * nq); ALLOC_OR_FAIL(lse);
    *lse_out = lse;
  }
  RUN(c, ctta_attention_lse(q, q_ld, k, k_ld, k_rows, vt, vt_ld, bias, out, out_ld, c.B, heads, nq, nk,
                            1.0f / sqrtf((float)dh), lse, c.stream));
  return CTTA_OK;
}

// The adapter term of one site, behind its base launch: d = x a^T (kept by the training forward), then y += scale * d b^T,
// or the same into the transposed V^T [batch][hp][vt_ld] where `vt_tokens` > 0.  Everything comes from the arena.
struct LoraDst { LoraSite* S; bf16_t* y; int ldy; int vt_tokens; };

static ctta_status lora_forward_one(UCtx& c, const LoraDst& D, const bf16_t* x, int ldx, int64_t rows, float* d) {
  const int r = c.U->lora_r;
  LoraSite& S = *D.S;
  if (c.row_slot) {   // a different adapter per sample: the sample's slot of the site's bank, its scale (or the handle's)
    const int slots = c.U->bank_slots;
    const int64_t sa = (int64_t)r * S.k_pad, sb = (int64_t)S.n_pad * r;
    RUN(c, ctta_lora_down_rows(x, ldx, rows, S.k_pad, S.bank_a, sa, slots, r, rows / c.B, c.row_slot, d, c.stream));
    if (D.vt_tokens > 0)
      RUN(c, ctta_lora_up_add_t_rows(D.y, D.ldy, (int64_t)S.n_pad * D.ldy, c.B, D.vt_tokens, S.n_pad, d, D.vt_tokens, S.bank_b, sb,
                                     slots, r, c.row_slot, c.row_scale, c.lora_scale, c.stream));
    else
      RUN(c, ctta_lora_up_add_rows(D.y, D.ldy, rows, S.n_pad, d, S.bank_b, sb, slots, r, rows / c.B, c.row_slot, c.row_scale,
                                   c.lora_scale, c.stream));
    return CTTA_OK;
  }
  RUN(c, ctta_lora_down(x, ldx, rows, S.k_pad, S.a, 0, r, d, c.stream));
  if (D.vt_tokens > 0)
    RUN(c, ctta_lora_up_add_t(D.y, D.ldy, (int64_t)S.n_pad * D.ldy, c.B, D.vt_tokens, S.n_pad, d, D.vt_tokens, S.b, r, c.lora_scale,
                              c.stream));
  else
    RUN(c, ctta_lora_up_add(D.y, D.ldy, rows, S.n_pad, d, S.b, 0, r, c.lora_scale, c.stream));
  return CTTA_OK;
}

// One to three sites on one input: ONE ctta_lora_sites_fwd launch where the fused kernels take the shapes (rank <= 4; a
// V^T destination of 8 | tokens), the per-site launches otherwise -- a V^T site the fused kernel refuses (always the last of
// its group) leaves the group and runs alone.  Either route allocates the same d buffers, and the values are bit-identical.
static ctta_status lora_forward(UCtx& c, const LoraDst* dst, int n, const bf16_t* x, int ldx, int64_t rows) {
  const int r = c.U->lora_r;
  float* d[3];
  int np[3];
  for (int i = 0; i < n; ++i) {
    d[i] = c.arena->get<float>((size_t)rows * r); ALLOC_OR_FAIL(d[i]);
    if (c.train) dst[i].S->d = d[i];
    np[i] = dst[i].S->n_pad;
  }
  const int k_pad = dst[0].S->k_pad;
  int nf = 0;   // sites [0, nf) go through the fused launch
  if (c.lora_fused) {
    const LoraDst& T = dst[n - 1];
    if (ctta_lora_sites_supported(k_pad, np, n, r, T.vt_tokens, T.ldy, (int64_t)T.S->n_pad * T.ldy)) nf = n;
    else if (n > 1 && T.vt_tokens > 0 && ctta_lora_sites_supported(k_pad, np, n - 1, r, 0, 0, 0)) nf = n - 1;
  }
  if (nf > 0) {
    ctta_lora_fwd_site fs[3];
    for (int i = 0; i < nf; ++i) {
      LoraSite& S = *dst[i].S;
      fs[i] = {S.a, S.b, dst[i].y, d[i], dst[i].ldy, S.n_pad, dst[i].vt_tokens, (int64_t)S.n_pad * dst[i].ldy};
    }
    RUN(c, ctta_lora_sites_fwd(x, ldx, rows, k_pad, r, c.lora_scale, fs, nf, c.stream));
  }
  for (int i = nf; i < n; ++i) CTTA_TRY(lora_forward_one(c, dst[i], x, ldx, rows, d[i]));
  return CTTA_OK;
}

static ctta_status run_transformer(UCtx& c, Transformer& T, const bf16_t* x, int H, int W,
                                   bf16_t** out_p) {
  Arena& A = *c.arena;
  const int N = H * W;
  const size_t M = (size_t)c.B * N;
  const int cp = T.cp, hp = T.hp;
  const bool lora = c.U->lora_r > 0;
  bf16_t* out = A.get<bf16_t>(M * T.c); ALLOC_OR_FAIL(out);
  const size_t mk = A.mark();
  bf16_t* g = A.get<bf16_t>(M * T.c); ALLOC_OR_FAIL(g);
  CTTA_TRY(gn(c, T.norm, x, g, N, 1e-6f, false, &T.sv.st));   // transformer_2d.py:149 hard-codes eps=1e-6
  bf16_t* s0 = A.get<bf16_t>(M * cp); ALLOC_OR_FAIL(s0);
  CTTA_TRY(run_linear(c, T.proj_in, g, T.c, M, s0, cp, nullptr, 0));
  bf16_t* n = A.get<bf16_t>(M * cp); ALLOC_OR_FAIL(n);
  RUN(c, ctta_layernorm(s0, n, M, T.inner, cp, T.ln1.gamma, T.ln1.beta, 1e-5f, c.stream));
  // --- self-attention
  bf16_t* qk = A.get<bf16_t>(M * 2 * hp); ALLOC_OR_FAIL(qk);
  CTTA_TRY(run_linear(c, T.qk1, n, cp, M, qk, 2 * hp, nullptr, 0));
  const int vt_ld = round_up(N, 8);
  bf16_t* vt = A.get<bf16_t>((size_t)c.B * hp * vt_ld); ALLOC_OR_FAIL(vt);
  CTTA_TRY(run_vt(c, T.v1, n, c.B, N, N, vt, vt_ld));
  if (lora) {   // q, k, v read n once; the [q | k] buffer is addressed by halves through ldy = 2 * hp
    const LoraDst g1[3] = {{&T.lq1, qk, 2 * hp, 0}, {&T.lk1, qk + hp, 2 * hp, 0}, {&T.lv1, vt, vt_ld, N}};
    CTTA_TRY(lora_forward(c, g1, 3, n, cp, M));
  }
  bf16_t* att = A.get<bf16_t>(M * hp); ALLOC_OR_FAIL(att);
  CTTA_TRY(run_attention(c, qk, 2 * hp, qk + hp, 2 * hp, N, vt, vt_ld, nullptr, att, hp, T.heads, N, N, T.dh, &T.sv.lse1));
  bf16_t* s1 = A.get<bf16_t>(M * cp); ALLOC_OR_FAIL(s1);
  CTTA_TRY(run_linear(c, T.out1, att, hp, M, s1, cp, s0, cp));
  if (lora) { const LoraDst g = {&T.lo1, s1, cp, 0}; CTTA_TRY(lora_forward(c, &g, 1, att, hp, M)); }
  // --- cross-attention against the text states
  bf16_t* const n1 = n;
  bf16_t* const att1 = att;
  if (c.train) {   // the backward pass needs every LayerNorm / attention output: no buffer reuse
    n = A.get<bf16_t>(M * cp); ALLOC_OR_FAIL(n);
    att = A.get<bf16_t>(M * hp); ALLOC_OR_FAIL(att);
  }
  RUN(c, ctta_layernorm(s1, n, M, T.inner, cp, T.ln2.gamma, T.ln2.beta, 1e-5f, c.stream));
  bf16_t* const n2 = n;
  bf16_t* q2 = A.get<bf16_t>(M * hp); ALLOC_OR_FAIL(q2);
  CTTA_TRY(run_linear(c, T.q2, n, cp, M, q2, hp, nullptr, 0));
  if (lora) { const LoraDst g = {&T.lq2, q2, hp, 0}; CTTA_TRY(lora_forward(c, &g, 1, n, cp, M)); }
  bf16_t* k2 = T.k2c;
  bf16_t* vt2 = T.vt2c;
  if (!k2 || c.dry) {   // sizing pass / no text cache: arena buffers
    k2 = A.get<bf16_t>((size_t)c.B * c.Lp * hp); ALLOC_OR_FAIL(k2);
    vt2 = A.get<bf16_t>((size_t)c.B * hp * c.Lp); ALLOC_OR_FAIL(vt2);
  }
  if (!c.reuse_text) {
    CTTA_TRY(run_linear(c, T.k2, c.enc_bf, c.U->xp, (int64_t)c.B * c.Lp, k2, hp, nullptr, 0));
    CTTA_TRY(run_vt(c, T.v2, c.enc_bf, c.B, c.Lp, c.Lp, vt2, c.Lp));
    if (lora) {   // into the text cache where there is one: it holds K / V^T with the adapter term
      const LoraDst g2[2] = {{&T.lk2, k2, hp, 0}, {&T.lv2, vt2, c.Lp, c.Lp}};
      CTTA_TRY(lora_forward(c, g2, 2, c.enc_bf, c.U->xp, (int64_t)c.B * c.Lp));
    }
  }
  CTTA_TRY(run_attention(c, q2, hp, k2, hp, c.Lp, vt2, c.Lp, c.mask_bias, att, hp, T.heads, N, c.L, T.dh, &T.sv.lse2));
  bf16_t* s2 = A.get<bf16_t>(M * cp); ALLOC_OR_FAIL(s2);
  // the fused feed-forward (inference forward, widths 256 / 512, enough rows to fill its tiles) also takes attn2.to_out + residual
  // and norm3 in front and proj_out + residual behind: five launches in one, s2 the only intermediate that reaches HBM
  // With adapters attn2.to_out is its own launch (its adapter term has to land before norm3), so the fused feed-forward
  // runs without its front projection; and the sizing pass of such a handle takes the unfused branch, the larger one
  // (ctta_ffn_geglu_wanted is not monotone in M: a smaller batch may take it).
  const bool ffn_fused = !c.train && T.ffn_stream && !(lora && c.dry) && ctta_ffn_geglu_wanted(cp, T.ffp, (int64_t)M);
  const bool ffn_front = ffn_fused && T.front_stream && !lora;
  if (!ffn_front) {
    CTTA_TRY(run_linear(c, T.out2, att, hp, M, s2, cp, s1, cp));
    if (lora) { const LoraDst g = {&T.lo2, s2, cp, 0}; CTTA_TRY(lora_forward(c, &g, 1, att, hp, M)); }
    // --- GEGLU feed-forward
    if (c.train) { n = A.get<bf16_t>(M * cp); ALLOC_OR_FAIL(n); }
    RUN(c, ctta_layernorm(s2, n, M, T.inner, cp, T.ln3.gamma, T.ln3.beta, 1e-5f, c.stream));
  }
  bf16_t* f = nullptr;
  bf16_t* gg = nullptr;
  if (c.train) {   // the backward pass needs the pre-activation: unfused
    f = A.get<bf16_t>(M * 2 * T.ffp); ALLOC_OR_FAIL(f);
    CTTA_TRY(run_linear(c, T.ff1, n, cp, M, f, 2 * T.ffp, nullptr, 0));
    gg = A.get<bf16_t>(M * T.ffp); ALLOC_OR_FAIL(gg);
    RUN(c, ctta_geglu(f, gg, M, T.ffp, 1, c.stream));
  } else if (ffn_fused) {
    // ff1 -> GEGLU -> ff2 + residual (-> proj_out + block input) in one launch: neither the projection, the hidden activations
    // nor (with the tail) the feed-forward result reach HBM
    ctta_ffn_desc fd;
    ctta_ffn_desc_init(&fd);
    fd.x = n; fd.ld_x = cp; fd.M = (int64_t)M; fd.cp = cp; fd.ffp = T.ffp; fd.packed = T.ffn_stream;
    fd.b1 = T.ff1.bias; fd.b2 = T.ff2.bias; fd.res = s2; fd.res_ld = cp;
    if (ffn_front) {
      fd.front_packed = T.front_stream; fd.front_bias = T.out2.bias; fd.att = att; fd.att_ld = hp; fd.front_k = hp;
      fd.front_res = s1; fd.front_res_ld = cp; fd.s2_out = s2; fd.s2_ld = cp;
      fd.ln_gamma = T.ln3.gamma; fd.ln_beta = T.ln3.beta; fd.ln_d = T.inner; fd.ln_eps = 1e-5f;
      c.gn_ready_x = nullptr;      // (what run_linear(out2) did: a linear ends the producer -> GroupNorm adjacency)
    }
    if (T.proj_stream) {
      fd.proj_packed = T.proj_stream; fd.proj_bias = T.proj_out.bias; fd.proj_res = x; fd.proj_res_ld = T.c;
      fd.out = out; fd.ldc = T.c; fd.n_valid = T.proj_out.n;
      RUN(c, ctta_ffn_block(&fd, c.stream));
    } else {
      bf16_t* s3f = A.get<bf16_t>(M * cp); ALLOC_OR_FAIL(s3f);
      fd.out = s3f; fd.ldc = cp; fd.n_valid = T.ff2.n;
      RUN(c, ctta_ffn_block(&fd, c.stream));
      CTTA_TRY(run_linear(c, T.proj_out, s3f, cp, M, out, T.c, x, T.c));
    }
    A.release(mk);
    *out_p = out;
    return CTTA_OK;
  } else {         // value * gelu(gate) in the GEMM epilogue: the (M, 2*ffp) projection never reaches HBM
    gg = A.get<bf16_t>(M * T.ffp); ALLOC_OR_FAIL(gg);
    ctta_conv_desc d;
    desc_init(&d);
    d.x0 = n; d.c0 = cp;
    d.batch = 1; d.hi = (int)M; d.wi = 1; d.ho = (int)M; d.wo = 1;
    d.w = T.ff1.w; d.k_pad = T.ff1.k_pad; d.n = T.ff1.n; d.bias = T.ff1.bias;
    d.out = gg; d.ldc = T.ffp; d.out_act = 4;
    RUN(c, ctta_conv_gemm(&d, c.stream));
  }
  bf16_t* s3 = A.get<bf16_t>(M * cp); ALLOC_OR_FAIL(s3);
  CTTA_TRY(run_linear(c, T.ff2, gg, T.ffp, M, s3, cp, s2, cp));
  CTTA_TRY(run_linear(c, T.proj_out, s3, cp, M, out, T.c, x, T.c));
  if (c.train) {
    Transformer::Saved& S = T.sv;
    S.x = x; S.g = g; S.s0 = s0; S.n1 = n1; S.qk = qk; S.vt = vt; S.att1 = att1; S.s1 = s1; S.n2 = n2; S.q2 = q2;
    S.k2 = k2; S.vt2 = vt2; S.att2 = att; S.s2 = s2; S.n3 = n; S.f = f; S.gg = gg; S.s3 = s3; S.H = H; S.W = W;
  }
  A.release(mk);
  *out_p = out;
  return CTTA_OK;
}

struct Skip { bf16_t* p; int c; };

static ctta_status unet_forward_impl(ctta_unet* U, bool dry, const float* sample, const float* timesteps,
                                     const double* guidance, const float* enc, const uint8_t* mask, int B,
                                     int L, float* out, hipStream_t stream, size_t* gn_need, bool train = false) {
  const ctta_unet_config& cfg = U->cfg;
  UCtx c;
  c.train = train;
  U->ts.valid = false;
  U->tape.clear();
  U->bind(c, stream, dry, cfg.debug_taps != 0, cfg.norm_num_groups);
  c.U = U; c.B = B; c.L = L; c.Lp = round_up(L, 8);
  c.lora_fused = (U->lora_fused & 2) != 0; c.lora_scale = U->lora_scale;
  if (U->row_slot && !train) {   // per-request adapters: the per-site rows launches, whatever bit 1 says
    c.row_slot = U->row_slot; c.row_scale = U->row_scale; c.lora_fused = false;
  }
  c.reuse_text = !dry && !train && U->tc_reuse_next && U->tc_valid && U->tc_base && U->tc_B == B && U->tc_L == L;
  U->tc_reuse_next = false;
  // a forward that re-projects the text states overwrites the cache as it goes: the cache is valid again only when this
  // call has finished (line `tc_valid = true` at the end), so a call that fails half way cannot leave mixed K / V behind
  if (!dry && !c.reuse_text && !train) U->tc_valid = false;
  Arena& A = U->arena;
  A.reset();
  A.no_release = cfg.debug_taps != 0 || train;   // the backward pass reads every intermediate
  const int H = cfg.height, W = cfg.width;
  const int T = U->temb_dim, c0 = cfg.block_out_channels[0];

  // ---- 1. time / guidance embeddings in fp32 (embeddings.py; unet...guided.py:803-816)
  float* tfeat = A.get<float>((size_t)B * c0); ALLOC_OR_FAIL(tfeat);
  float* h1 = A.get<float>((size_t)B * T); ALLOC_OR_FAIL(h1);
  float* et = A.get<float>((size_t)B * T); ALLOC_OR_FAIL(et);
  float* eg = nullptr;
  RUN(c, ctta_time_features(timesteps, U->freqs, c0, cfg.flip_sin_to_cos, tfeat, B, stream));
  // hidden = SiLU(linear_1(x)); the training forward keeps the pre-activation for SiLU'
  auto mlp_hidden = [&](const float* x, const float* w, const float* b, int k, float* hid, const float** pre_out) -> ctta_status {
    if (!train) { RUN(c, ctta_linear_f32(x, w, b, hid, B, T, k, 0, 1, stream)); return CTTA_OK; }
    float* pre = A.get<float>((size_t)B * T); ALLOC_OR_FAIL(pre);
    RUN(c, ctta_linear_f32(x, w, b, pre, B, T, k, 0, 0, stream));
    if (!dry) {
      hipLaunchKernelGGL(add_silu_kernel, dim3((B * T + 255) / 256), dim3(256), 0, stream, pre, (const float*)nullptr, hid,
                         (float*)nullptr, B * T);
      CTTA_LAUNCH_CHECK();
    }
    *pre_out = pre;
    return CTTA_OK;
  };
  CTTA_TRY(mlp_hidden(tfeat, U->t_w1, U->t_b1, c0, h1, &U->ts.t_h1pre));
  RUN(c, ctta_linear_f32(h1, U->t_w2, U->t_b2, et, B, T, T, 0, 0, stream));
  U->ts.tfeat = tfeat; U->ts.t_h1 = h1;
  if (cfg.guided) {
    float* gfeat = A.get<float>((size_t)B * T); ALLOC_OR_FAIL(gfeat);
    float* g1 = A.get<float>((size_t)B * T); ALLOC_OR_FAIL(g1);
    eg = A.get<float>((size_t)B * T); ALLOC_OR_FAIL(eg);
    RUN(c, ctta_fourier_features(guidance, U->g_proj, T / 2, cfg.flip_sin_to_cos, gfeat, B, stream));
    CTTA_TRY(mlp_hidden(gfeat, U->g_w1, U->g_b1, T, g1, &U->ts.g_h1pre));
    RUN(c, ctta_linear_f32(g1, U->g_w2, U->g_b2, eg, B, T, T, 0, 0, stream));
    U->ts.gfeat = gfeat; U->ts.g_h1 = g1;
  }
  float* emb = A.get<float>((size_t)B * T); ALLOC_OR_FAIL(emb);
  float* emb_silu = A.get<float>((size_t)B * T); ALLOC_OR_FAIL(emb_silu);
  if (!dry) {
    hipLaunchKernelGGL(add_silu_kernel, dim3((B * T + 255) / 256), dim3(256), 0, stream, et, eg, emb_silu, emb, B * T);
    CTTA_LAUNCH_CHECK();
  }
  U->ts.emb = emb; U->ts.emb_silu = emb_silu;
  add_tap(c, "emb", emb, B, T, 1, 1, T, true);
  // every resnet's Linear(SiLU(emb)) (resnet.py:572-573) in one batch
  float* temb_all = A.get<float>((size_t)B * U->temb_total); ALLOC_OR_FAIL(temb_all);
  RUN(c, ctta_linear_f32(emb_silu, U->temb_w, U->temb_b, temb_all, B, U->temb_total, T, 0, 0, stream));
  c.temb_all = temb_all;

  // ---- text states and mask bias
  bf16_t* enc_bf = A.get<bf16_t>((size_t)B * c.Lp * U->xp); ALLOC_OR_FAIL(enc_bf);
  float* mbias = nullptr;
  if (mask) { mbias = A.get<float>((size_t)B * L); ALLOC_OR_FAIL(mbias); }
  if (!dry) {
    const long long total = (long long)B * c.Lp * U->xp;
    if (!c.reuse_text) {   // only the K / V^T projections read the packed text states
      hipLaunchKernelGGL(pack_enc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, enc, enc_bf, B,
                         L, cfg.cross_attention_dim, c.Lp, U->xp);
      CTTA_LAUNCH_CHECK();
    }
    if (mask) {
      hipLaunchKernelGGL(mask_bias_kernel, dim3((B * L + 255) / 256), dim3(256), 0, stream, mask, mbias, B * L);
      CTTA_LAUNCH_CHECK();
    }
  }
  c.enc_bf = enc_bf; c.mask_bias = mbias;
  U->ts.enc_bf = enc_bf; U->ts.mask_bias = mbias;
  int cur_block = 0;
  auto tape = [&](TapeOp op) { op.block = cur_block; if (train) U->tape.push_back(op); };

  // ---- 2. conv_in
  bf16_t* xin = A.get<bf16_t>((size_t)B * H * W * U->cin_pad); ALLOC_OR_FAIL(xin);
  RUN(c, ctta_nchw_f32_to_nhwc_bf16(sample, xin, B, cfg.in_channels, H, W, U->cin_pad, 1.0f, stream));
  bf16_t* h = A.get<bf16_t>((size_t)B * H * W * c0); ALLOC_OR_FAIL(h);
  CTTA_TRY(run_conv2d(c, U->conv_in, xin, B, H, W, false, h, nullptr, 0, nullptr, 0));
  add_tap(c, "conv_in", h, B, c0, H, W, c0);
  int ch = c0, hh = H, ww = W;
  std::vector<Skip> skips;
  int n_skips = 0;
  U->ts.xin = xin;
  { TapeOp op; op.kind = TapeOp::CONV_IN; op.x = xin; op.H = H; op.W = W; tape(op); }
  auto push_skip = [&](bf16_t* p, int cc) {
    skips.push_back({p, cc});
    TapeOp op; op.kind = TapeOp::SKIP_PUSH; op.skip_idx = n_skips++; op.ch = cc; op.H = hh; op.W = ww; tape(op);
  };
  auto tape_res = [&](Resnet& R) { TapeOp op; op.kind = TapeOp::RESNET; op.R = &R; op.H = hh; op.W = ww; tape(op); };
  auto tape_att = [&](Transformer& Tr) { TapeOp op; op.kind = TapeOp::TRANSFORMER; op.T = &Tr; op.H = hh; op.W = ww; tape(op); };
  push_skip(h, ch);

  // ---- 3. down
  for (int i = 0; i < cfg.n_levels; ++i) {
    Level& Lv = U->down[i];
    cur_block = 1 + i;
    const std::string p = "down_blocks." + std::to_string(i) + ".";
    for (size_t j = 0; j < Lv.res.size(); ++j) {
      CTTA_TRY(run_resnet(c, Lv.res[j], h, hh, ww, &h));
      tape_res(Lv.res[j]);
      ch = Lv.res[j].cout;
      add_tap(c, p + "resnets." + std::to_string(j), h, B, ch, hh, ww, ch);
      if (!Lv.att.empty()) {
        CTTA_TRY(run_transformer(c, Lv.att[j], h, hh, ww, &h));
        tape_att(Lv.att[j]);
        add_tap(c, p + "attentions." + std::to_string(j), h, B, ch, hh, ww, ch);
      }
      push_skip(h, ch);
    }
    if (Lv.has_sampler) {
      const int ho = (hh + 2 - 3) / 2 + 1, wo = (ww + 2 - 3) / 2 + 1;
      bf16_t* d = A.get<bf16_t>((size_t)B * ho * wo * ch); ALLOC_OR_FAIL(d);
      CTTA_TRY(run_conv2d(c, Lv.sampler, h, B, hh, ww, false, d, nullptr, 0, nullptr, 0));
      { TapeOp op; op.kind = TapeOp::DOWNSAMPLE; op.Lv = &Lv; op.x = h; op.H = hh; op.W = ww; op.ch = ch; tape(op); }
      h = d; hh = ho; ww = wo;
      add_tap(c, p + "downsamplers.0", h, B, ch, hh, ww, ch);
      push_skip(h, ch);
    }
  }
  // ---- 4. mid
  cur_block = 1 + cfg.n_levels;
  CTTA_TRY(run_resnet(c, U->mid_r0, h, hh, ww, &h));
  tape_res(U->mid_r0);
  CTTA_TRY(run_transformer(c, U->mid_att, h, hh, ww, &h));
  tape_att(U->mid_att);
  CTTA_TRY(run_resnet(c, U->mid_r1, h, hh, ww, &h));
  tape_res(U->mid_r1);
  add_tap(c, "mid_block", h, B, ch, hh, ww, ch);
  // ---- 5. up
  for (int i = 0; i < cfg.n_levels; ++i) {
    Level& Lv = U->up[i];
    cur_block = 2 + cfg.n_levels + i;
    const std::string p = "up_blocks." + std::to_string(i) + ".";
    for (size_t j = 0; j < Lv.res.size(); ++j) {
      const Skip sk = skips.back();
      skips.pop_back();
      const size_t M = (size_t)B * hh * ww;
      bf16_t* cat = A.get<bf16_t>(M * (ch + sk.c)); ALLOC_OR_FAIL(cat);
      // torch.cat([h, skip], 1).  With the statistics fusion on, the pass that writes the concatenation also sums it for the
      // resnet's norm1 (the one GroupNorm input no convolution epilogue produces): one read of the two sources instead of
      // concat + a statistics pass over its output
      if (!c.dry && c.gn_fpart && c.gn_groups > 0 && (ch + sk.c) % c.gn_groups == 0) {
        int chunks = 0;
        CTTA_TRY(ctta_concat_channels_gn(h, ch, sk.p, sk.c, cat, B, hh * ww, c.gn_groups, c.gn_fpart, (int64_t)c.gn_fpart_floats,
                                         &chunks, stream));
        c.gn_ready_x = cat; c.gn_ready_chunks = chunks; c.gn_ready_c = ch + sk.c;
      } else {
        RUN(c, ctta_concat_channels(h, ch, sk.p, sk.c, cat, (int64_t)M, stream));
      }
      CTTA_REQUIRE(Lv.res[j].cin == ch + sk.c, "internal: skip width mismatch");
      { TapeOp op; op.kind = TapeOp::CONCAT; op.ch = ch; op.skc = sk.c; op.skip_idx = (int)skips.size(); op.H = hh; op.W = ww; tape(op); }
      CTTA_TRY(run_resnet(c, Lv.res[j], cat, hh, ww, &h));
      tape_res(Lv.res[j]);
      ch = Lv.res[j].cout;
      add_tap(c, p + "resnets." + std::to_string(j), h, B, ch, hh, ww, ch);
      if (!Lv.att.empty()) {
        CTTA_TRY(run_transformer(c, Lv.att[j], h, hh, ww, &h));
        tape_att(Lv.att[j]);
        add_tap(c, p + "attentions." + std::to_string(j), h, B, ch, hh, ww, ch);
      }
    }
    if (Lv.has_sampler) {   // Upsample2D: nearest x2 fused into the conv's gather
      bf16_t* u = A.get<bf16_t>((size_t)B * 4 * hh * ww * ch); ALLOC_OR_FAIL(u);
      CTTA_TRY(run_conv2d(c, Lv.sampler, h, B, hh, ww, true, u, nullptr, 0, nullptr, 0));
      { TapeOp op; op.kind = TapeOp::UPSAMPLE; op.Lv = &Lv; op.x = h; op.H = hh; op.W = ww; op.ch = ch; tape(op); }
      h = u; hh *= 2; ww *= 2;
      add_tap(c, p + "upsamplers.0", h, B, ch, hh, ww, ch);
    }
  }
  CTTA_REQUIRE(hh == H && ww == W && ch == c0, "internal: up path did not return to the input extent");
  // ---- 6. out
  bf16_t* a = A.get<bf16_t>((size_t)B * H * W * c0); ALLOC_OR_FAIL(a);
  float* st_out = nullptr;
  CTTA_TRY(gn(c, U->norm_out, h, a, H * W, cfg.norm_eps, true, &st_out));
  if (cfg.out_channels % 4 != 0) {     // the direct fp32-weight kernel of round 2 (290 us at batch 32) for odd channel counts
    RUN(c, ctta_conv_small_n(a, c0, B, H, W, 3, 3, 1, 1, U->conv_out_w, U->conv_out_b, cfg.out_channels, 0,
                             0.f, 0, out, nullptr, stream));
  } else {   // conv_gemm on the matrix pipe (N = 8 of a 32-wide tile), fp32 [pixel][channel] result, then the NCHW hop
    float* o_nhwc = A.get<float>((size_t)B * H * W * U->conv_out.p.n); ALLOC_OR_FAIL(o_nhwc);
    ctta_conv_desc d;
    desc_init(&d);
    d.x0 = a; d.c0 = c0;
    d.batch = B; d.hi = H; d.wi = W; d.ho = H; d.wo = W;
    d.kh = 3; d.kw = 3; d.pad_h = d.pad_w = 1;
    d.w = U->conv_out.p.w; d.k_pad = U->conv_out.p.k_pad; d.n = U->conv_out.p.n; d.bias = U->conv_out.p.bias;
    d.out = o_nhwc; d.ldc = U->conv_out.p.n; d.out_f32 = 1;
    RUN(c, ctta_conv_gemm(&d, stream));
    RUN(c, ctta_nhwc_f32_to_nchw_f32(o_nhwc, out, B, cfg.out_channels, H * W, U->conv_out.p.n, stream));
  }
  if (train) {
    U->ts.h_last = h; U->ts.a_out = a; U->ts.st_out = st_out;
    U->ts.B = B; U->ts.L = L; U->ts.Lp = c.Lp; U->ts.n_skips = n_skips; U->ts.arena_off = A.off;
    U->ts.lora_fused = U->lora_fused; U->ts.lora_scale = U->lora_scale;
    U->ts.valid = !dry;
  }
  if (gn_need) *gn_need = c.gn_need;
  if (!dry && U->tc_base) { U->tc_valid = true; U->tc_B = B; U->tc_L = L; }
  return CTTA_OK;
}

#include "engine_unet_train.h"


// ------------------------------------------------------------------------------------ create
static ctta_status unet_build(ctta_unet* U) {
  const ctta_unet_config& cfg = U->cfg;
  WeightStore& ws = U->store;
  const int n = cfg.n_levels;
  const int* boc = cfg.block_out_channels;
  const int T = boc[0] * 4;
  U->temb_dim = T;
  U->cin_pad = round_up(cfg.in_channels, 32);
  U->xp = round_up(cfg.cross_attention_dim, 64);
  // total rows of the concatenated time_emb_proj table
  int total = 0;
  for (int i = 0; i < n; ++i) total += cfg.layers_per_block[i] * boc[i];
  for (int i = 0; i < n; ++i) total += (cfg.layers_per_block[n - 1 - i] + 1) * boc[n - 1 - i];
  total += 2 * boc[n - 1];
  U->temb_w = ws.arena.get<float>((size_t)total * T);
  U->temb_b = ws.arena.get<float>((size_t)total);
  if (!U->temb_w || !U->temb_b) { ctta_set_error("weight store exhausted"); return CTTA_ERR_NOMEM; }
  U->temb_total = 0;

  const bool tr = cfg.enable_training != 0;
  CTTA_TRY(make_conv(ws, "conv_in.", boc[0], cfg.in_channels, U->cin_pad, 3, 3, 1, 1, &U->conv_in, true,
                     tr ? &U->t_conv_in.m : nullptr));
  CTTA_TRY(ws.add_vector("time_embedding.linear_1.weight", T * boc[0], &U->t_w1));
  CTTA_TRY(ws.add_vector("time_embedding.linear_1.bias", T, &U->t_b1));
  CTTA_TRY(ws.add_vector("time_embedding.linear_2.weight", T * T, &U->t_w2));
  CTTA_TRY(ws.add_vector("time_embedding.linear_2.bias", T, &U->t_b2));
  if (cfg.guided) {
    CTTA_TRY(ws.add_vector("guidance_proj.weight", T / 2, &U->g_proj));
    CTTA_TRY(ws.add_vector("guidance_embedding.linear_1.weight", T * T, &U->g_w1));
    CTTA_TRY(ws.add_vector("guidance_embedding.linear_1.bias", T, &U->g_b1));
    CTTA_TRY(ws.add_vector("guidance_embedding.linear_2.weight", T * T, &U->g_w2));
    CTTA_TRY(ws.add_vector("guidance_embedding.linear_2.bias", T, &U->g_b2));
  }
  {  // sinusoid frequency table exp(-ln(10000) * i / (half - shift)), embeddings.py:43-49
    const int half = boc[0] / 2;
    std::vector<float> f(half);
    for (int i = 0; i < half; ++i) {
      const float exponent = (-logf(10000.0f) * (float)i) / ((float)half - cfg.freq_shift);
      f[i] = (float)exp((double)exponent);
    }
    U->freqs = ws.arena.get<float>(half);
    if (!U->freqs) { ctta_set_error("weight store exhausted"); return CTTA_ERR_NOMEM; }
    CTTA_CHECK_HIP(hipMemcpy(U->freqs, f.data(), half * sizeof(float), hipMemcpyHostToDevice));
  }

  U->down.resize(n);
  int out_c = boc[0];
  for (int i = 0; i < n; ++i) {
    const int in_c = out_c;
    out_c = boc[i];
    Level& Lv = U->down[i];
    const std::string p = "down_blocks." + std::to_string(i) + ".";
    const int nl = cfg.layers_per_block[i];
    if (cfg.down_cross[i]) {
      Lv.att.resize(nl);
      for (int j = 0; j < nl; ++j)
        CTTA_TRY(make_transformer(U, p + "attentions." + std::to_string(j) + ".", out_c, cfg.heads[i], &Lv.att[j]));
    }
    Lv.res.resize(nl);
    for (int j = 0; j < nl; ++j)
      CTTA_TRY(make_resnet(U, p + "resnets." + std::to_string(j) + ".", j == 0 ? in_c : out_c, out_c, &Lv.res[j]));
    if (i != n - 1) {
      Lv.has_sampler = true;
      CTTA_TRY(make_conv(ws, p + "downsamplers.0.conv.", out_c, out_c, out_c, 3, 3, 2, 1, &Lv.sampler, true,
                         tr ? &Lv.tsampler.m : nullptr));
      if (tr) CTTA_TRY(make_conv_dgrad_from(ws, Lv.sampler, out_c, out_c, &Lv.tsampler.d));
    }
  }
  U->up.resize(n);
  out_c = boc[n - 1];
  for (int i = 0; i < n; ++i) {
    const int prev_c = out_c;
    out_c = boc[n - 1 - i];
    const int in_c = boc[n - 1 - (i + 1 < n ? i + 1 : n - 1)];
    const int nl = cfg.layers_per_block[n - 1 - i] + 1;
    Level& Lv = U->up[i];
    const std::string p = "up_blocks." + std::to_string(i) + ".";
    if (cfg.up_cross[i]) {
      Lv.att.resize(nl);
      for (int j = 0; j < nl; ++j)
        CTTA_TRY(make_transformer(U, p + "attentions." + std::to_string(j) + ".", out_c, cfg.heads[n - 1 - i], &Lv.att[j]));
    }
    Lv.res.resize(nl);
    for (int j = 0; j < nl; ++j) {
      const int skip_c = (j == nl - 1) ? in_c : out_c;
      const int rin = (j == 0) ? prev_c : out_c;
      CTTA_TRY(make_resnet(U, p + "resnets." + std::to_string(j) + ".", rin + skip_c, out_c, &Lv.res[j]));
    }
    if (i != n - 1) {
      Lv.has_sampler = true;
      CTTA_TRY(make_conv(ws, p + "upsamplers.0.conv.", out_c, out_c, out_c, 3, 3, 1, 1, &Lv.sampler, true,
                         tr ? &Lv.tsampler.m : nullptr));
      if (tr) CTTA_TRY(make_conv_dgrad_from(ws, Lv.sampler, out_c, out_c, &Lv.tsampler.d));
    }
  }
  CTTA_TRY(make_transformer(U, "mid_block.attentions.0.", boc[n - 1], cfg.heads[n - 1], &U->mid_att));
  CTTA_TRY(make_resnet(U, "mid_block.resnets.0.", boc[n - 1], boc[n - 1], &U->mid_r0));
  CTTA_TRY(make_resnet(U, "mid_block.resnets.1.", boc[n - 1], boc[n - 1], &U->mid_r1));
  CTTA_REQUIRE(U->temb_total == total, "internal: time_emb_proj table size");
  CTTA_TRY(make_gn(ws, "conv_norm_out.", boc[0], &U->norm_out));
  {
    const int co = cfg.out_channels, ci = boc[0];
    CTTA_TRY(make_conv(ws, "conv_out.", co, ci, ci, 3, 3, 1, 1, &U->conv_out, true, nullptr));
    U->conv_out_w = ws.arena.get<float>((size_t)co * ci * 9);
    if (!U->conv_out_w) { ctta_set_error("weight store exhausted"); return CTTA_ERR_NOMEM; }
    float* dst = U->conv_out_w;
    ws.jobs.push_back([=](const WeightTable& wt, hipStream_t s) -> ctta_status {
      const ctta_tensor* t = wt.find("conv_out.weight");
      if (!t) { ctta_set_error("missing state-dict key 'conv_out.weight'"); return CTTA_ERR_MISSING_KEY; }
      if (tensor_numel(t) != (int64_t)co * ci * 9) { ctta_set_error("size mismatch for 'conv_out.weight'"); return CTTA_ERR_INVALID; }
      const int total_e = co * ci * 9;
      hipLaunchKernelGGL(repack_small_w_kernel, dim3((total_e + 255) / 256), dim3(256), 0, s, t->data, dst, co, ci, 9);
      CTTA_LAUNCH_CHECK();
      return CTTA_OK;
    });
    CTTA_TRY(ws.add_vector("conv_out.bias", co, &U->conv_out_b));
    if (tr) {   // conv_out runs on the direct small-N kernel in the forward; the backward uses conv_gemm
      CTTA_REQUIRE(co <= 8, "unet_create: training supports out_channels <= 8");
      CTTA_TRY(make_conv_dgrad(ws, "conv_out.", co, ci, 3, 3, 1, &U->t_conv_out.d, 8));
      std::vector<int32_t> ro(8, -1);
      for (int r = 0; r < co; ++r) ro[r] = r * ci * 9;
      PackMap& m = U->t_conv_out.m;
      m.wkey = "conv_out.weight"; m.bkey = "conv_out.bias"; m.n = 8; m.n_bias = co; m.bidx = nullptr;
      m.k_ident = ci * 9;
      CTTA_TRY(ws.upload(ro, &m.ro));
    }
  }
  return CTTA_OK;
}

extern "C" ctta_status ctta_unet_create(const ctta_unet_config* cfg, const ctta_tensor* weights, int n_weights,
                                        void* stream, ctta_unet** out) {
  CTTA_REQUIRE(cfg && weights && out, "unet_create: null pointer");
  CTTA_REQUIRE(cfg->n_levels >= 1 && cfg->n_levels <= CTTA_MAX_LEVELS, "unet_create: n_levels=%d", cfg->n_levels);
  CTTA_REQUIRE(cfg->in_channels > 0 && cfg->out_channels > 0 &&
                   (cfg->out_channels == 1 || cfg->out_channels == 2 || cfg->out_channels == 4 || cfg->out_channels == 8),
               "unet_create: out_channels=%d unsupported (1,2,4,8)", cfg->out_channels);
  for (int i = 0; i < cfg->n_levels; ++i) {
    CTTA_REQUIRE(cfg->block_out_channels[i] % 8 == 0, "unet_create: block_out_channels must be multiples of 8");
    CTTA_REQUIRE(cfg->block_out_channels[i] % cfg->norm_num_groups == 0,
                 "unet_create: channels %d not divisible by norm_num_groups %d", cfg->block_out_channels[i], cfg->norm_num_groups);
  }
  const int div = 1 << (cfg->n_levels - 1);
  CTTA_REQUIRE(cfg->height % div == 0 && cfg->width % div == 0,
               "unet_create: sample extent %dx%d must be a multiple of %d", cfg->height, cfg->width, div);
  CTTA_REQUIRE(cfg->max_batch >= 1 && cfg->max_text_len >= 1, "unet_create: bad max_batch/max_text_len");
  hipStream_t s = (hipStream_t)stream;
  ctta_unet* U = new ctta_unet();
  U->cfg = *cfg;
  // A weight table that names adapter tensors ("..._lora.down.weight" / "..._lora.up.weight") gives the handle adapters at
  // every attention projection; the rank is read from the first one's shape.  A table that lacks one of the eight tensors
  // of an attention fails in load_weights with that key named.
  for (int i = 0; i < n_weights && U->lora_r == 0; ++i) {
    const char* nm = weights[i].name;
    if (!nm || !strstr(nm, "_lora.") || weights[i].ndim != 2) continue;
    const size_t len = strlen(nm);
    if (len > 11 && !strcmp(nm + len - 11, "down.weight")) U->lora_r = (int)weights[i].shape[0];
    else if (len > 9 && !strcmp(nm + len - 9, "up.weight")) U->lora_r = (int)weights[i].shape[1];
  }
  if (U->lora_r < 0 || U->lora_r > 16) {
    ctta_set_error("unet_create: adapter rank %d outside [1,16]", U->lora_r);
    delete U;
    return CTTA_ERR_INVALID;
  }
  ctta_status st = U->store.init(cfg->enable_training ? estimate_store_bytes_training(weights, n_weights)
                                                      : estimate_store_bytes(weights, n_weights));
  if (st == CTTA_OK) st = unet_build(U);
  if (st == CTTA_OK) st = U->load_weights(weights, n_weights, s);
  size_t gn_need = 0;
  if (st == CTTA_OK) {   // sizing pass: no launches, measures the arena and the GN scratch
    U->arena.dry = true;
    U->arena.no_release = cfg->debug_taps != 0;
    st = unet_forward_impl(U, true, nullptr, nullptr, nullptr, nullptr, (const uint8_t*)1, cfg->max_batch,
                           cfg->max_text_len, nullptr, s, &gn_need);
    if (st == CTTA_OK && cfg->enable_training) {   // training forward + backward need the larger arena
      {   // known before the dry run: with the side stream on, the backward releases nothing (unet_backward_begin_impl)
        U->wg.enabled = ctta_opt(CTTA_OPT_WGRAD_STREAM) != 0;   // 0 at creation: one stream, and the backward releases its arena blocks
      }
      size_t gn2 = 0;
      st = unet_forward_impl(U, true, nullptr, nullptr, nullptr, nullptr, (const uint8_t*)1, cfg->max_batch,
                             cfg->max_text_len, nullptr, s, &gn2, true);
      if (gn2 > gn_need) gn_need = gn2;
      for (Arena& a : U->wg.slot) { a.dry = true; a.reset(); a.peak = 0; }
      if (st == CTTA_OK) st = unet_backward_impl(U, true, nullptr, nullptr, s, nullptr);
      U->ts.valid = false;
    }
  }
  if (st == CTTA_OK && cfg->enable_training) {   // scratch slots + stream + events of the weight-gradient side stream
    WgradSide& W = U->wg;
    size_t slot_bytes = 0;
    for (Arena& a : W.slot) if (a.peak > slot_bytes) slot_bytes = a.peak;
    slot_bytes = (slot_bytes + 4095) & ~(size_t)4095;
    if (hipMalloc((void**)&W.base, slot_bytes * WgradSide::NS + 4096) != hipSuccess) {
      ctta_set_error("unet_create: hipMalloc of the weight-gradient scratch (%zu bytes) failed", slot_bytes * 2);
      st = CTTA_ERR_NOMEM;
    } else {
      for (int i = 0; i < WgradSide::NS; ++i) {
        W.slot[i].dry = false; W.slot[i].base = W.base + (size_t)i * slot_bytes; W.slot[i].cap = slot_bytes; W.slot[i].reset();
        if (hipEventCreateWithFlags(&W.ready[i], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&W.freed[i], hipEventDisableTiming) != hipSuccess) st = CTTA_ERR_HIP;
      }
      if (hipEventCreateWithFlags(&W.joined, hipEventDisableTiming) != hipSuccess ||
          hipStreamCreateWithFlags(&W.stream, hipStreamNonBlocking) != hipSuccess) st = CTTA_ERR_HIP;
      if (st != CTTA_OK) ctta_set_error("unet_create: could not create the weight-gradient stream / events");
    }
  }
  if (st == CTTA_OK)
    st = U->allocate_after_dry_run("unet_create", gn_need,
                                   (size_t)cfg->max_batch * (cfg->height * cfg->width / 16 + 1) * cfg->norm_num_groups * 2, true, s);
  if (st == CTTA_OK) {   // text cache: K [B][Lp][hp] + V^T [B][hp][Lp] per transformer block
    std::vector<Transformer*> ts;
    for (Level& Lv : U->down) for (Transformer& T : Lv.att) ts.push_back(&T);
    ts.push_back(&U->mid_att);
    for (Level& Lv : U->up) for (Transformer& T : Lv.att) ts.push_back(&T);
    const size_t lp = (size_t)round_up(cfg->max_text_len, 8);
    size_t total = 0;
    for (Transformer* T : ts) total += 2 * (((size_t)cfg->max_batch * lp * T->hp * sizeof(bf16_t) + 255) & ~(size_t)255);
    if (hipMalloc((void**)&U->tc_base, total + 256) != hipSuccess) {
      U->tc_base = nullptr;   // no cache: the forward falls back to arena buffers (sized by the dry run either way)
    } else {
      char* q = U->tc_base;
      for (Transformer* T : ts) {
        const size_t one = ((size_t)cfg->max_batch * lp * T->hp * sizeof(bf16_t) + 255) & ~(size_t)255;
        T->k2c = reinterpret_cast<bf16_t*>(q); q += one;
        T->vt2c = reinterpret_cast<bf16_t*>(q); q += one;
      }
    }
  }
  if (st != CTTA_OK) { ctta_unet_destroy(U); return st; }
  *out = U;
  return CTTA_OK;
}

extern "C" void ctta_unet_destroy(ctta_unet* U) {
  if (!U) return;
  U->destroy_base();
  if (U->tc_base) (void)hipFree(U->tc_base);
  if (U->bank_base) (void)hipFree(U->bank_base);
  if (U->wg.stream) { (void)hipStreamSynchronize(U->wg.stream); (void)hipStreamDestroy(U->wg.stream); }
  for (int i = 0; i < WgradSide::NS; ++i) {
    if (U->wg.ready[i]) (void)hipEventDestroy(U->wg.ready[i]);
    if (U->wg.freed[i]) (void)hipEventDestroy(U->wg.freed[i]);
  }
  if (U->wg.joined) (void)hipEventDestroy(U->wg.joined);
  if (U->wg.base) (void)hipFree(U->wg.base);
  delete U;
}

extern "C" ctta_status ctta_unet_load_weights(ctta_unet* U, const ctta_tensor* weights, int n_weights, void* stream) {
  CTTA_REQUIRE(U && weights, "unet_load_weights: null pointer");
  U->tc_valid = false;   // the cached K / V^T were projected with the old weights
  return U->load_weights(weights, n_weights, (hipStream_t)stream);
}

// Re-packs the adapter tensors alone: the fp32 copies make_lora_site registered (keys with "_lora."); every base pack stays.
extern "C" ctta_status ctta_unet_load_adapters(ctta_unet* U, const ctta_tensor* weights, int n_weights, void* stream) {
  CTTA_REQUIRE(U && weights, "unet_load_adapters: null pointer");
  CTTA_REQUIRE(U->lora_r > 0, "unet_load_adapters: the handle has no adapters (its weight table named none at creation)");
  WeightTable wt;
  wt.map.clear();
  for (int i = 0; i < n_weights; ++i) {
    const char* nm = weights[i].name;
    if (!nm || !strstr(nm, "_lora.")) continue;
    const size_t len = strlen(nm);
    int r = U->lora_r;
    if (weights[i].ndim == 2 && len > 11 && !strcmp(nm + len - 11, "down.weight")) r = (int)weights[i].shape[0];
    else if (weights[i].ndim == 2 && len > 9 && !strcmp(nm + len - 9, "up.weight")) r = (int)weights[i].shape[1];
    CTTA_REQUIRE(r == U->lora_r, "unet_load_adapters: '%s' has rank %d, the handle's adapters have rank %d", nm, r, U->lora_r);
    wt.map[nm] = &weights[i];
  }
  U->tc_valid = false;   // the cached K / V^T hold the old adapters' term
  return U->store.run_adapters(wt, (hipStream_t)stream);
}

extern "C" ctta_status ctta_unet_set_lora(ctta_unet* U, int fused, float scale) {
  CTTA_REQUIRE(U, "unet_set_lora: null handle");
  CTTA_REQUIRE(scale == scale && scale - scale == 0.f, "unet_set_lora: scale must be finite");
  CTTA_REQUIRE(fused >= 0 && fused <= 3, "unet_set_lora: fused=%d (bit 0: backward groups, bit 1: forward groups)", fused);
  if (scale != U->lora_scale) U->tc_valid = false;   // the cached K / V^T hold scale * the adapter term
  U->lora_fused = fused;
  U->lora_scale = scale;
  return CTTA_OK;
}

// ---- per-request adapters.  The bank is ONE allocation carved into per-site A [slots][r][k_pad] / B [slots][n_pad][r]; a slot
// is loaded with the copy segments make_lora_site registered for the handle's own a / b, rebased into the slot.
static void lora_sites_of(ctta_unet* U, std::vector<LoraSite*>* out) {
  auto of = [&](Transformer& T) {
    for (LoraSite* S : {&T.lq1, &T.lk1, &T.lv1, &T.lo1, &T.lq2, &T.lk2, &T.lv2, &T.lo2}) out->push_back(S);
  };
  for (Level& Lv : U->down) for (Transformer& T : Lv.att) of(T);
  of(U->mid_att);
  for (Level& Lv : U->up) for (Transformer& T : Lv.att) of(T);
}

extern "C" ctta_status ctta_unet_adapter_bank(ctta_unet* U, int slots, void* stream) {
  CTTA_REQUIRE(U, "unet_adapter_bank: null handle");
  CTTA_REQUIRE(U->lora_r > 0, "unet_adapter_bank: the handle has no adapters (its weight table named none at creation)");
  CTTA_REQUIRE(slots >= 1 && slots <= 64, "unet_adapter_bank: %d slots outside [1,64]", slots);
  if (U->bank_base) {
    CTTA_REQUIRE(slots == U->bank_slots, "unet_adapter_bank: the handle already has a bank of %d slots (asked for %d); a bank is allocated once per handle",
                 U->bank_slots, slots);
    return CTTA_OK;
  }
  std::vector<LoraSite*> sites;
  lora_sites_of(U, &sites);
  const int r = U->lora_r;
  auto padded = [](size_t floats) { return (floats + 63) & ~(size_t)63; };   // 256-byte steps: every site's bank is 16-byte aligned
  size_t total = 0;
  for (LoraSite* S : sites) total += padded((size_t)slots * r * S->k_pad) + padded((size_t)slots * S->n_pad * r);
  float* base = nullptr;
  if (hipMalloc((void**)&base, total * sizeof(float)) != hipSuccess) {
    ctta_set_error("unet_adapter_bank: hipMalloc of %zu bytes failed", total * sizeof(float));
    return CTTA_ERR_NOMEM;
  }
  if (hipMemsetAsync(base, 0, total * sizeof(float), (hipStream_t)stream) != hipSuccess) {
    (void)hipFree(base);
    ctta_set_error("unet_adapter_bank: hipMemset of the bank failed");
    return CTTA_ERR_HIP;
  }
  float* q = base;
  for (LoraSite* S : sites) {
    S->bank_a = q; q += padded((size_t)slots * r * S->k_pad);
    S->bank_b = q; q += padded((size_t)slots * S->n_pad * r);
  }
  U->bank_base = base;
  U->bank_slots = slots;
  return CTTA_OK;
}

extern "C" ctta_status ctta_unet_load_adapter_slot(ctta_unet* U, int slot, const ctta_tensor* weights, int n_weights, void* stream) {
  CTTA_REQUIRE(U && weights, "unet_load_adapter_slot: null pointer");
  CTTA_REQUIRE(U->lora_r > 0, "unet_load_adapter_slot: the handle has no adapters (its weight table named none at creation)");
  CTTA_REQUIRE(U->bank_base, "unet_load_adapter_slot: the handle has no adapter bank (ctta_unet_adapter_bank)");
  CTTA_REQUIRE(slot >= 0 && slot < U->bank_slots, "unet_load_adapter_slot: slot %d outside [0,%d)", slot, U->bank_slots);
  WeightTable wt;
  wt.map.clear();
  for (int i = 0; i < n_weights; ++i) {
    const char* nm = weights[i].name;
    if (!nm || !strstr(nm, "_lora.")) continue;
    const size_t len = strlen(nm);
    int r = U->lora_r;
    if (weights[i].ndim == 2 && len > 11 && !strcmp(nm + len - 11, "down.weight")) r = (int)weights[i].shape[0];
    else if (weights[i].ndim == 2 && len > 9 && !strcmp(nm + len - 9, "up.weight")) r = (int)weights[i].shape[1];
    CTTA_REQUIRE(r == U->lora_r, "unet_load_adapter_slot: '%s' has rank %d, the handle's adapters have rank %d", nm, r, U->lora_r);
    wt.map[nm] = &weights[i];
  }
  // the handle's own packed a / b -> the same place of this slot of the site's bank
  std::vector<LoraSite*> sites;
  lora_sites_of(U, &sites);
  const size_t r = (size_t)U->lora_r;
  std::vector<WeightStore::Rebase> rb;
  for (LoraSite* S : sites) {
    rb.push_back({S->a, r * S->k_pad, S->bank_a + (size_t)slot * r * S->k_pad});
    rb.push_back({S->b, (size_t)S->n_pad * r, S->bank_b + (size_t)slot * S->n_pad * r});
  }
  U->tc_valid = false;   // the cached K / V^T hold the rows' adapter terms
  return U->store.run_adapters(wt, (hipStream_t)stream, &rb);
}

extern "C" ctta_status ctta_unet_set_adapter_rows(ctta_unet* U, const int32_t* slot_of_sample, const float* scale_of_sample) {
  CTTA_REQUIRE(U, "unet_set_adapter_rows: null handle");
  CTTA_REQUIRE(!slot_of_sample || U->bank_base, "unet_set_adapter_rows: the handle has no adapter bank (ctta_unet_adapter_bank)");
  CTTA_REQUIRE(slot_of_sample || !scale_of_sample, "unet_set_adapter_rows: scale_of_sample without slot_of_sample");
  U->tc_valid = false;   // the cached K / V^T hold the adapter terms of whatever was bound before
  U->row_slot = slot_of_sample;
  U->row_scale = scale_of_sample;
  return CTTA_OK;
}

extern "C" ctta_status ctta_unet_reuse_text(ctta_unet* U, int reuse) {
  CTTA_REQUIRE(U, "unet_reuse_text: null handle");
  U->tc_reuse_next = reuse != 0;
  return CTTA_OK;
}

extern "C" ctta_status ctta_unet_forward(ctta_unet* U, const float* sample, const float* timesteps,
                                         const double* guidance, const float* enc, const uint8_t* mask, int batch,
                                         int text_len, float* out, void* stream) {
  CTTA_REQUIRE(U && sample && timesteps && enc && out, "unet_forward: null pointer");
  CTTA_REQUIRE(!U->cfg.guided || guidance, "unet_forward: guidance is required by the guided U-Net");
  CTTA_REQUIRE(batch >= 1 && batch <= U->cfg.max_batch, "unet_forward: batch %d outside [1,%d]", batch, U->cfg.max_batch);
  CTTA_REQUIRE(text_len >= 1 && text_len <= U->cfg.max_text_len, "unet_forward: text_len %d outside [1,%d]", text_len,
               U->cfg.max_text_len);
  WsBind bind(U->splitws);
  return unet_forward_impl(U, false, sample, timesteps, guidance, enc, mask, batch, text_len, out, (hipStream_t)stream,
                           nullptr);
}

extern "C" size_t ctta_unet_arena_bytes(const ctta_unet* U) { return U ? U->arena_bytes() : 0; }
extern "C" int ctta_unet_num_taps(const ctta_unet* U) { return (int)taps_of(U).size(); }
extern "C" ctta_status ctta_unet_tap_info(const ctta_unet* U, int i, const char** name, int dims[4]) { return tap_info(taps_of(U), i, name, dims); }
extern "C" ctta_status ctta_unet_tap_read(ctta_unet* U, int i, float* dst, void* stream) { return tap_read(taps_of(U), i, dst, stream); }
