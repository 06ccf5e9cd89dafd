// Backward pass of the student U-Net for the consistency-distillation step (included by
// engine_unet.hip; same translation unit).  The reference gets these gradients from torch autograd
// over UNet2DConditionGuidedModel.forward (train.py:332-346 -> accelerator.backward(loss)); here the
// tape the training forward recorded is replayed in reverse with hand-written operators:
//   * data gradients   : conv_gemm against the re-packed (rotated / transposed) weights,
//   * weight gradients : one split-M GEMM  dW[k][n] = sum_m Q[k][m] * dY^T[n][m]  per layer, where
//                        Q = im2col(X)^T plus an all-ones row (bias gradient) and, for the resnets'
//                        conv1, one indicator row per sample (time-embedding gradient),
//   * attention        : flash-style backward (ctta_attention_bwd_inplace): probabilities rebuilt from the forward's
//                        log-sum-exp, dV = P^T dO, dP = dO V^T, dS = P (dP - D) scale, dQ = dS K, dK = dS^T Q,
//   * norms / GEGLU / embedding MLP: the kernels in backward.hip.
// The leaf operators and the weight-gradient jobs (plan, launch, scatter, side stream) are engine_backward.h's, shared
// with the VAE decoder; this file keeps the U-Net's blocks.  Gradients are ACCUMULATED into the caller's fp32 tensors (same names / shapes as the state dict),
// i.e. `.grad` semantics; the caller zeroes them.  Activation gradients travel in bf16.

struct BCtx : UCtx {
  float* dtemb_all = nullptr;   // [B][temb_total] fp32, filled from the conv1 indicator rows
};

// conv1 of a resnet: the shared job with one indicator row per sample behind the bias row (nb = B), whose slab columns
// are d temb; then time_emb_proj's own gradients
static ctta_status conv1_wgrad(BCtx& c, const Resnet& R, const bf16_t* x, int H, int W, const bf16_t* dy) {
  const ConvLayer& L = R.c1;
  const int K = L.kh * L.kw * L.cin_pad;
  return layer_wgrad(c, wgrad_geom(c.B, L.kh, L.kw, L.cin_pad, H, W, false, L.stride, L.pad, L.p.n, c.B), R.t1.m, nullptr, x, dy,
                     [&](GradCtx& w, const WgradDone& d) -> ctta_status {
    // d temb[b][off + n] = sum over the sample's pixels of dY: columns K+1 .. K+B of the slab
    RUN(w, ctta_col_scatter(d.slabs, d.pl.splits, (int64_t)d.g.n * d.pl.ld, d.pl.ld, K + 1, c.B, L.cout, nullptr,
                            c.dtemb_all + R.temb_off, c.U->temb_total, 0, w.stream));
    // temb = time_emb_proj(SiLU(emb)): its weight / bias gradients need only this resnet's rows of d temb, which the
    // scatter above just produced (same stream, in order)
    float *gw, *gb;
    CTTA_TRY(grad_ptr(w, R.key + "time_emb_proj.weight", &gw));
    CTTA_TRY(grad_ptr(w, R.key + "time_emb_proj.bias", &gb));
    RUN(w, ctta_linear_f32_bwd(c.U->ts.emb_silu, c.U->temb_w, c.dtemb_all + R.temb_off, c.U->temb_total, nullptr, nullptr, gw, gb,
                               c.B, R.cout, c.U->temb_dim, 0, 1, w.stream));
    return CTTA_OK;
  });
}

// dx = dx_add + dL/dx (dx_add NULL: plain).  The transformer's running token-stream gradient moves to a NEW buffer at every
// LayerNorm: the previous one stays as it was for the weight-gradient jobs that read it in place on the side stream.
static ctta_status ln_backward(BCtx& c, const LNLayer& l, const bf16_t* x, const bf16_t* dy, const bf16_t* dx_add, bf16_t* dx,
                               int64_t rows, int d, int ld) {
  float *dg, *db;
  Arena& A = *c.arena;
  const size_t mk = A.mark();
  if (!c.params) {
    // frozen base: the kernel forms d gamma / d beta on its way to dx whatever the caller wants; they go to a throwaway row
    // of the arena (never read), without the partial table and so without the fold launch
    dg = A.get<float>((size_t)2 * ld); ALLOC_OR_FAIL(dg);
    db = dg + ld;
    RUN(c, ctta_layernorm_bwd_ws(x, dy, dx_add, dx, rows, d, ld, l.gamma, 1e-5f, dg, db, nullptr, 0, c.stream));
    A.release(mk);
    return CTTA_OK;
  }
  CTTA_TRY(grad_ptr(c, l.key + "weight", &dg));
  CTTA_TRY(grad_ptr(c, l.key + "bias", &db));
  // the partial table of d gamma / d beta comes from THIS handle's arena and goes back at once: everything that may later
  // be placed on top of it is written by kernels enqueued on c.stream behind the fold
  const size_t nf = ctta_layernorm_bwd_scratch_floats(rows, ld);
  float* part = nf ? A.get<float>(nf) : nullptr;
  if (nf && !part) { ctta_set_error("arena exhausted (layernorm backward partials)"); return CTTA_ERR_NOMEM; }
  RUN(c, ctta_layernorm_bwd_ws(x, dy, dx_add, dx, rows, d, ld, l.gamma, 1e-5f, dg, db, part, nf, c.stream));
  A.release(mk);
  return CTTA_OK;
}

// Adapter backward of one to three projection sites y = W x + scale * up(down(x)) on ONE input x, behind the base layers' own
// data gradients:  dD = dY B,  dB += scale dY^T D,  dA += scale dD^T X,  dX += scale dD A  (dx NULL: the input carries no
// gradient -- the text states); dD stays unscaled.  The parameter gradients are formed when the gradient table names the
// site's two tensors.  Where the fused kernels take the shapes (ctta_lora_sites_supported) the group is ONE
// ctta_lora_sites_bwd call -- one read-modify-write of dx with the per-site launches' rounding sequence, so every data
// gradient downstream keeps its bits; otherwise each site runs down + 2 x wgrad + up_add.  All launches run on the main
// stream out of ONE arena block whose size covers both routes (the route may change between the sizing pass and a call).
struct LoraGrad { LoraSite* S; const bf16_t* dy; int lddy; };

static ctta_status lora_backward(BCtx& c, const LoraGrad* sites, int n, const bf16_t* x, int ldx, int64_t rows, bf16_t* dx,
                                 int lddx) {
  const int r = c.U->lora_r;
  const float scale = c.U->ts.lora_scale;
  Arena& A = *c.arena;
  float *ga[3] = {nullptr, nullptr, nullptr}, *gb[3] = {nullptr, nullptr, nullptr};
  bool want[3], any = dx != nullptr;
  int np[3];
  for (int i = 0; i < n; ++i) {
    LoraSite& S = *sites[i].S;
    want[i] = c.dry;
    if (!c.dry) {
      auto ia = c.grads->map.find(S.key + "down.weight"), ib = c.grads->map.find(S.key + "up.weight");
      const bool ha = ia != c.grads->map.end() && ia->second, hb = ib != c.grads->map.end() && ib->second;
      if (ha != hb) {
        ctta_set_error("%s: no gradient tensor for '%s%s'", c.who, S.key.c_str(), ha ? "up.weight" : "down.weight");
        return CTTA_ERR_MISSING_KEY;
      }
      want[i] = ha;
      if (ha) { ga[i] = ia->second; gb[i] = ib->second; }
    }
    any = any || want[i];
    np[i] = S.n_pad;
  }
  if (!any) return CTTA_OK;
  const int k_pad = sites[0].S->k_pad;
  // per-site route: dD and the larger of the two partial tables per site, each rounded up to 64 floats
  auto up64 = [](size_t v) { return (v + 63) / 64 * 64; };
  size_t per_site = 0;
  for (int i = 0; i < n; ++i) {
    size_t nf = ctta_lora_wgrad_scratch_floats(rows, np[i], r);
    const size_t nk = ctta_lora_wgrad_scratch_floats(rows, k_pad, r);
    if (nk > nf) nf = nk;
    per_site += up64((size_t)rows * r) + up64(nf);
  }
  const bool can_fuse = ctta_lora_sites_supported(k_pad, np, n, r, 0, 0, 0) != 0;
  const size_t fused_floats = can_fuse ? ctta_lora_sites_bwd_scratch_floats(rows, k_pad, np[0], n, r) : 0;
  float* block = A.get<float>(per_site > fused_floats ? per_site : fused_floats); ALLOC_OR_FAIL(block);
  if (can_fuse && (c.U->ts.lora_fused & 1)) {
    ctta_lora_bwd_site bs[3];
    for (int i = 0; i < n; ++i) {
      LoraSite& S = *sites[i].S;
      bs[i] = {sites[i].dy, S.a, S.b, S.d, nullptr, ga[i], gb[i], S.kmap, S.nmap, (int64_t)S.k, 1, 1, (int64_t)r, sites[i].lddy, S.n_pad};
    }
    RUN(c, ctta_lora_sites_bwd(x, ldx, dx, lddx, rows, k_pad, r, scale, bs, n, block, c.stream));
    return CTTA_OK;
  }
  float* q = block;
  for (int i = 0; i < n; ++i) {
    LoraSite& S = *sites[i].S;
    if (!want[i] && !dx) continue;
    float* dd = q; q += up64((size_t)rows * r);
    float* part = q;
    size_t nf = ctta_lora_wgrad_scratch_floats(rows, S.n_pad, r);
    const size_t nk = ctta_lora_wgrad_scratch_floats(rows, S.k_pad, r);
    q += up64(nk > nf ? nk : nf);
    RUN(c, ctta_lora_down(sites[i].dy, sites[i].lddy, rows, S.n_pad, S.b, 1, r, dd, c.stream));
    if (want[i]) {
      RUN(c, ctta_lora_wgrad(S.d, sites[i].dy, sites[i].lddy, rows, S.n_pad, r, scale, gb[i], 1, r, S.nmap, part, c.stream));
      RUN(c, ctta_lora_wgrad(dd, x, ldx, rows, S.k_pad, r, scale, ga[i], S.k, 1, S.kmap, part, c.stream));
    }
    if (dx) RUN(c, ctta_lora_up_add(dx, lddx, rows, S.k_pad, dd, S.a, 1, r, scale, c.stream));
  }
  return CTTA_OK;
}

// ------------------------------------------------------------------------------ resnet
// out = conv2(silu(gn2(t1))) + shortcut(x),  t1 = conv1(silu(gn1(x))) + temb   (resnet.py:549-597)
static ctta_status bwd_resnet(BCtx& c, Resnet& R, const bf16_t* dout, bf16_t** dx_p) {
  Arena& A = *c.arena;
  const Resnet::Saved& S = R.sv;
  const int H = S.H, W = S.W;
  const size_t M = (size_t)c.B * H * W;
  bf16_t* dx = A.get<bf16_t>(M * R.cin); ALLOC_OR_FAIL(dx);
  const size_t mk = A.mark();
  bf16_t* da2 = A.get<bf16_t>(M * R.cout); ALLOC_OR_FAIL(da2);
  CTTA_TRY(conv_dgrad(c, R.t2.d, dout, H, W, da2, H, W, false));
  CTTA_TRY(conv_wgrad(c, R.c2, R.t2.m, S.a2, H, W, false, dout));
  bf16_t* dt1 = A.get<bf16_t>(M * R.cout); ALLOC_OR_FAIL(dt1);
  CTTA_TRY(gn_backward(c, R.n2, S.t1, da2, dt1, H * W, S.st2, true, false));
  CTTA_TRY(conv1_wgrad(c, R, S.a, H, W, dt1));   // + d temb and time_emb_proj's weight / bias gradients
  bf16_t* da = A.get<bf16_t>(M * R.cin); ALLOC_OR_FAIL(da);
  CTTA_TRY(conv_dgrad(c, R.t1.d, dt1, H, W, da, H, W, false));
  if (R.has_sc) {
    CTTA_TRY(conv_dgrad(c, R.tsc.d, dout, H, W, dx, H, W, false));
    CTTA_TRY(conv_wgrad(c, R.sc, R.tsc.m, S.x, H, W, false, dout));
  } else {
    RUN(c, ctta_add_slices(dout, R.cout, nullptr, 0, dx, R.cin, (int64_t)M, R.cin, c.stream));
  }
  CTTA_TRY(gn_backward(c, R.n1, S.x, da, dx, H * W, S.st1, true, true));
  A.release(mk);
  *dx_p = dx;
  return CTTA_OK;
}

// ------------------------------------------------------------------------------ attention
// q [B][nq][ldq], k [B][krows][ldk] (head h at columns h*64), vt [B][hp][vt_ld]; out / dO [B*nq][hp].
// Writes dq [B*nq][lddq], dk [B*krows][lddk], dv [B*krows][hp] for keys < nk (head-padded lanes come
// out zero).  Flash-style (no score matrix): Q, K, dO are read where they lie and V as the forward keeps it
// (transposed) -- ctta_attention_bwd_inplace takes the operands it needs in the other orientation out of its own LDS tiles
// through transposing reads.
static ctta_status bwd_attention(BCtx& c, int heads, int dh, const bf16_t* q, int ldq, const bf16_t* k, int ldk, int krows,
                                 const bf16_t* vt, int vt_ld, const float* bias, int nq, int nk, const bf16_t* out,
                                 const bf16_t* dO, int hp, const float* lse, bf16_t* dq, int lddq, bf16_t* dk, int lddk,
                                 bf16_t* dv) {
  CTTA_REQUIRE(vt_ld % 8 == 0 && vt_ld >= nk, "bwd_attention: vt_ld=%d is not what the forward takes (nk=%d)", vt_ld, nk);
  Arena& A = *c.arena;
  const int B = c.B;
  const size_t mk = A.mark();
  float* dsum = A.get<float>((size_t)B * heads * nq); ALLOC_OR_FAIL(dsum);
  float* part = nullptr;
  int64_t part_floats = 0;
  if (nk <= 128) {   // cross-attention: room for 32 query splits of the dk/dv kernel
    part_floats = (int64_t)32 * 2 * B * krows * hp;
    part = A.get<float>((size_t)part_floats); ALLOC_OR_FAIL(part);
  }
  RUN(c, ctta_attention_bwd_inplace(q, ldq, k, ldk, krows, vt, vt_ld, bias, out, hp, dO, hp, lse, dsum, dq, lddq, dk, lddk, dv, hp,
                                    B, heads, nq, nk, 1.0f / sqrtf((float)dh), part, part_floats, c.stream));
  A.release(mk);
  return CTTA_OK;
}

// ------------------------------------------------------------------------------ transformer
// transformer_2d.py:218-332 + attention.py:276-334 in reverse (see run_transformer for the forward)
static ctta_status bwd_transformer(BCtx& c, Transformer& T, const bf16_t* dout, bf16_t** dx_p) {
  Arena& A = *c.arena;
  const Transformer::Saved& S = T.sv;
  const int N = S.H * S.W;
  const int64_t M = (int64_t)c.B * N;
  const int cp = T.cp, hp = T.hp, ffp = T.ffp;
  const int vt_ld = round_up(N, 8);
  const bool lora = c.U->lora_r > 0;
  bf16_t* dx = A.get<bf16_t>((size_t)M * T.c); ALLOC_OR_FAIL(dx);
  const size_t mk = A.mark();
  // out = proj_out(s3) + x
  bf16_t* ds = A.get<bf16_t>((size_t)M * cp); ALLOC_OR_FAIL(ds);   // running gradient of the token stream
  bf16_t* ds_next[3];                                              // ... after ln3, ln2, ln1 (never rewritten in place)
  for (int i = 0; i < 3; ++i) { ds_next[i] = A.get<bf16_t>((size_t)M * cp); ALLOC_OR_FAIL(ds_next[i]); }
  CTTA_TRY(linear_dgrad(c, T.t_proj_out.d, dout, T.c, T.c, M, ds, cp, cp, false));
  CTTA_TRY(linear_wgrad(c, T.t_proj_out.m, nullptr, S.s3, cp, M, dout, T.proj_out.n));
  {  // s3 = ff2(geglu(ff1(ln3(s2)))) + s2
    const size_t m2 = A.mark();
    bf16_t* dgg = A.get<bf16_t>((size_t)M * ffp); ALLOC_OR_FAIL(dgg);
    CTTA_TRY(linear_dgrad(c, T.t_ff2.d, ds, cp, cp, M, dgg, ffp, ffp, false));
    CTTA_TRY(linear_wgrad(c, T.t_ff2.m, nullptr, S.gg, ffp, M, ds, cp));
    bf16_t* df = A.get<bf16_t>((size_t)M * 2 * ffp); ALLOC_OR_FAIL(df);
    RUN(c, ctta_geglu_bwd(S.f, dgg, df, M, ffp, 1, c.stream));
    bf16_t* dn = A.get<bf16_t>((size_t)M * cp); ALLOC_OR_FAIL(dn);
    CTTA_TRY(linear_dgrad(c, T.t_ff1.d, df, 2 * ffp, 2 * ffp, M, dn, cp, cp, false));
    CTTA_TRY(linear_wgrad(c, T.t_ff1.m, nullptr, S.n3, cp, M, df, 2 * ffp));
    CTTA_TRY(ln_backward(c, T.ln3, S.s2, dn, ds, ds_next[0], M, T.inner, cp));
    ds = ds_next[0];
    A.release(m2);
  }
  {  // s2 = out2(attn(q2(ln2(s1)), k2(enc), v2(enc))) + s1
    const size_t m2 = A.mark();
    const int Lp = c.Lp;
    bf16_t* datt = A.get<bf16_t>((size_t)M * hp); ALLOC_OR_FAIL(datt);
    CTTA_TRY(linear_dgrad(c, T.t_out2.d, ds, cp, cp, M, datt, hp, hp, false));
    if (lora) { const LoraGrad g = {&T.lo2, ds, cp}; CTTA_TRY(lora_backward(c, &g, 1, S.att2, hp, M, datt, hp)); }
    CTTA_TRY(linear_wgrad(c, T.t_out2.m, nullptr, S.att2, hp, M, ds, cp));
    bf16_t* dq = A.get<bf16_t>((size_t)M * hp); ALLOC_OR_FAIL(dq);
    const size_t kv = (size_t)c.B * Lp * hp;
    bf16_t* dk = A.get<bf16_t>(kv); ALLOC_OR_FAIL(dk);
    bf16_t* dv = A.get<bf16_t>(kv); ALLOC_OR_FAIL(dv);
    if (!c.dry) {   // rows of padded text positions are never written by the per-head GEMMs
      CTTA_CHECK_HIP(ctta_zero_async(dk, kv * sizeof(bf16_t), c.stream));
      CTTA_CHECK_HIP(ctta_zero_async(dv, kv * sizeof(bf16_t), c.stream));
    }
    CTTA_TRY(bwd_attention(c, T.heads, T.dh, S.q2, hp, S.k2, hp, Lp, S.vt2, Lp, c.mask_bias, N, c.L, S.att2, datt, hp, S.lse2,
                           dq, hp, dk, hp, dv));
    bf16_t* dn = A.get<bf16_t>((size_t)M * cp); ALLOC_OR_FAIL(dn);
    CTTA_TRY(linear_dgrad(c, T.t_q2.d, dq, hp, hp, M, dn, cp, cp, false));
    if (lora) {   // dn has its one owner (the line above) before the adapter adds into it; the text states take no gradient
      const LoraGrad gq = {&T.lq2, dq, hp};
      CTTA_TRY(lora_backward(c, &gq, 1, S.n2, cp, M, dn, cp));
      const LoraGrad gkv[2] = {{&T.lk2, dk, hp}, {&T.lv2, dv, hp}};
      CTTA_TRY(lora_backward(c, gkv, 2, c.enc_bf, c.U->xp, (int64_t)c.B * Lp, nullptr, 0));
    }
    CTTA_TRY(linear_wgrad(c, T.t_q2.m, nullptr, S.n2, cp, M, dq, hp));
    CTTA_TRY(linear_wgrad(c, T.t_k2.m, nullptr, c.enc_bf, c.U->xp, (int64_t)c.B * Lp, dk, hp));
    CTTA_TRY(linear_wgrad(c, T.t_v2.m, nullptr, c.enc_bf, c.U->xp, (int64_t)c.B * Lp, dv, hp));
    CTTA_TRY(ln_backward(c, T.ln2, S.s1, dn, ds, ds_next[1], M, T.inner, cp));
    ds = ds_next[1];
    A.release(m2);
  }
  {  // s1 = out1(attn(q1(n1), k1(n1), v1(n1))) + s0,  n1 = ln1(s0)
    const size_t m2 = A.mark();
    bf16_t* datt = A.get<bf16_t>((size_t)M * hp); ALLOC_OR_FAIL(datt);
    CTTA_TRY(linear_dgrad(c, T.t_out1.d, ds, cp, cp, M, datt, hp, hp, false));
    if (lora) { const LoraGrad g = {&T.lo1, ds, cp}; CTTA_TRY(lora_backward(c, &g, 1, S.att1, hp, M, datt, hp)); }
    CTTA_TRY(linear_wgrad(c, T.t_out1.m, nullptr, S.att1, hp, M, ds, cp));
    bf16_t* dqk = A.get<bf16_t>((size_t)M * 2 * hp); ALLOC_OR_FAIL(dqk);
    bf16_t* dv = A.get<bf16_t>((size_t)M * hp); ALLOC_OR_FAIL(dv);
    CTTA_TRY(bwd_attention(c, T.heads, T.dh, S.qk, 2 * hp, S.qk + hp, 2 * hp, N, S.vt, vt_ld, nullptr, N, N, S.att1, datt, hp,
                           S.lse1, dqk, 2 * hp, dqk + hp, 2 * hp, dv));
    bf16_t* dn = A.get<bf16_t>((size_t)M * cp); ALLOC_OR_FAIL(dn);
    CTTA_TRY(linear_dgrad(c, T.t_q1.d, dqk, hp, 2 * hp, M, dn, cp, cp, false));
    CTTA_TRY(linear_dgrad(c, T.t_k1.d, dqk + hp, hp, 2 * hp, M, dn, cp, cp, true));
    CTTA_TRY(linear_dgrad(c, T.t_v1.d, dv, hp, hp, M, dn, cp, cp, true));
    if (lora) {   // behind the owner (q, accumulate = false) and the two accumulating data gradients: one write of dn
      const LoraGrad g1[3] = {{&T.lq1, dqk, 2 * hp}, {&T.lk1, dqk + hp, 2 * hp}, {&T.lv1, dv, hp}};
      CTTA_TRY(lora_backward(c, g1, 3, S.n1, cp, M, dn, cp));
    }
    CTTA_TRY(linear_wgrad(c, T.t_q1.m, &T.t_k1.m, S.n1, cp, M, dqk, 2 * hp));
    CTTA_TRY(linear_wgrad(c, T.t_v1.m, nullptr, S.n1, cp, M, dv, hp));
    CTTA_TRY(ln_backward(c, T.ln1, S.s0, dn, ds, ds_next[2], M, T.inner, cp));
    ds = ds_next[2];
    A.release(m2);
  }
  // s0 = proj_in(gn(x))
  bf16_t* dg = A.get<bf16_t>((size_t)M * T.c); ALLOC_OR_FAIL(dg);
  CTTA_TRY(linear_dgrad(c, T.t_proj_in.d, ds, cp, cp, M, dg, T.c, T.c, false));
  CTTA_TRY(linear_wgrad(c, T.t_proj_in.m, nullptr, S.g, T.c, M, ds, cp));
  RUN(c, ctta_add_slices(dout, T.c, nullptr, 0, dx, T.c, M, T.c, c.stream));
  CTTA_TRY(gn_backward(c, T.norm, S.x, dg, dx, N, S.st, false, true));
  A.release(mk);
  *dx_p = dx;
  return CTTA_OK;
}

// ------------------------------------------------------------------------------ embeddings
static ctta_status bwd_embeddings(BCtx& c) {
  ctta_unet* U = c.U;
  Arena& A = *c.arena;
  const ctta_unet::TrainSaved& S = U->ts;
  const int B = c.B, T = U->temb_dim, total = U->temb_total, c0 = U->cfg.block_out_channels[0];
  // temb_all = Linear(SiLU(emb)) over the concatenated time_emb_proj table (its weight gradients were taken per resnet)
  if (!c.params) return CTTA_OK;   // frozen base: d emb feeds parameter gradients only
  float* demb = A.get<float>((size_t)B * T); ALLOC_OR_FAIL(demb);
  RUN(c, ctta_linear_f32_bwd(S.emb_silu, U->temb_w, c.dtemb_all, total, S.emb, demb, nullptr, nullptr, B, total, T, 0, 0,
                             c.stream));
  // emb = linear_2(SiLU(linear_1(feat)))  for the time (and guidance) branch; d emb feeds both
  auto mlp = [&](const std::string& name, const float* feat, int k, const float* hpre, const float* hid, const float* w1,
                 const float* w2) -> ctta_status {
    float *gw1, *gb1, *gw2, *gb2;
    CTTA_TRY(grad_ptr(c, name + "linear_1.weight", &gw1));
    CTTA_TRY(grad_ptr(c, name + "linear_1.bias", &gb1));
    CTTA_TRY(grad_ptr(c, name + "linear_2.weight", &gw2));
    CTTA_TRY(grad_ptr(c, name + "linear_2.bias", &gb2));
    float* dh = A.get<float>((size_t)B * T); ALLOC_OR_FAIL(dh);
    RUN(c, ctta_linear_f32_bwd(hid, w2, demb, T, hpre, dh, gw2, gb2, B, T, T, 0, 1, c.stream));
    RUN(c, ctta_linear_f32_bwd(feat, w1, dh, T, nullptr, nullptr, gw1, gb1, B, T, k, 0, 1, c.stream));
    return CTTA_OK;
  };
  CTTA_TRY(mlp("time_embedding.", S.tfeat, c0, S.t_h1pre, S.t_h1, U->t_w1, U->t_w2));
  if (U->cfg.guided) CTTA_TRY(mlp("guidance_embedding.", S.gfeat, T, S.g_h1pre, S.g_h1, U->g_w1, U->g_w2));
  return CTTA_OK;
}

// ------------------------------------------------------------------------------ whole network
// The backward pass is resumable block by block (out head, up blocks, mid block, down blocks, then conv_in + the
// embedding MLPs): after each step all parameter gradients of that block are final, so the caller can start the
// data-parallel all-reduce of that block's slice of the flat gradient buffer while the next block computes.
static void bctx_init(BCtx& c, ctta_unet* U, bool dry, const GradTable* grads, hipStream_t stream) {
  const ctta_unet::TrainSaved& S = U->ts;
  U->bind(c, stream, dry, false, 0);   // the backward emits no fused GroupNorm statistics
  c.U = U; c.B = S.B; c.L = S.L; c.Lp = S.Lp; c.train = true;
  c.enc_bf = S.enc_bf; c.mask_bias = S.mask_bias;
  c.grads = grads; c.who = "unet_backward"; c.norm_groups = U->cfg.norm_num_groups;
  // Per parameter kind: a table that names no base parameter (adapter tensors only) is the frozen-base mode -- no base
  // weight-gradient job is launched anywhere in the network (convolutions, linears, norms, embeddings); one that names any
  // base parameter asks for all of them, as ever.  Adapter gradients follow their own names (lora_backward).
  c.params = dry || U->lora_r == 0;
  if (!c.params)
    for (const auto& kv : grads->map)
      if (kv.first.find("_lora.") == std::string::npos) { c.params = true; break; }
  c.side = &U->wg; c.policy = &kWgradPolicyUnet;
  c.dtemb_all = U->bw.dtemb_all;
}

static ctta_status unet_backward_begin_impl(ctta_unet* U, bool dry, const bf16_t* dpred, const GradTable* grads,
                                            hipStream_t stream) {
  const ctta_unet_config& cfg = U->cfg;
  const ctta_unet::TrainSaved& S = U->ts;
  Arena& A = U->arena;
  A.off = S.arena_off;
  // With the weight-gradient side stream on, a linear layer's dY is read in place by the SIDE stream some time after the main
  // stream has moved on: nothing the backward allocates is released before the next training forward resets the arena
  // (the dry run sizes it under the same policy; a few GB more at batch 9 -- HBM is what this part has).
  A.no_release = U->wg.enabled;
  const int B = S.B, H = cfg.height, W = cfg.width, c0 = cfg.block_out_channels[0];
  U->bw.dtemb_all = A.get<float>((size_t)B * U->temb_total); ALLOC_OR_FAIL(U->bw.dtemb_all);
  U->bw.dskip.assign((size_t)S.n_skips, nullptr);
  U->bw.pos = U->tape.size();
  BCtx c;
  bctx_init(c, U, dry, grads, stream);
  if (!dry) {
    // Every earlier backward ended with wg_join: when that join was on THIS stream, everything the side stream did for
    // it is ordered before what this call enqueues, so no scratch slot is "in use" any more.  Without this the first
    // jobs of a backward waited on `freed` events recorded by the previous one -- harmless eagerly, but inside a hipGraph
    // capture that is a dependency on uncaptured work (hipErrorStreamCaptureIsolation).
    // The same when this call is the first one inside / after a capture: events recorded on the other side of that
    // boundary must not be waited on (torch's graph context synchronises the device when it opens and closes).
    WgradSide& Wg = U->wg;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &cs);
    const bool capturing = cs == hipStreamCaptureStatusActive;
    if (!Wg.dirty && (Wg.joined_on == stream || capturing != Wg.was_capturing))
      for (int i = 0; i < WgradSide::NS; ++i) Wg.in_use[i] = false;
    Wg.was_capturing = capturing;
  }
  // ---- conv_out, conv_norm_out
  const size_t M0 = (size_t)B * H * W;
  bf16_t* dh = A.get<bf16_t>(M0 * c0); ALLOC_OR_FAIL(dh);
  const size_t mk = A.mark();
  bf16_t* da = A.get<bf16_t>(M0 * c0); ALLOC_OR_FAIL(da);
  CTTA_TRY(conv_dgrad(c, U->t_conv_out.d, dpred, H, W, da, H, W, false));
  ConvLayer co;   // geometry of conv_out for the weight gradient (the forward runs it on the small-N kernel)
  co.cin_pad = c0; co.cout = cfg.out_channels; co.kh = co.kw = 3; co.stride = 1; co.pad = 1; co.p.n = 8;
  CTTA_TRY(conv_wgrad(c, co, U->t_conv_out.m, S.a_out, H, W, false, dpred));
  CTTA_TRY(gn_backward(c, U->norm_out, S.h_last, da, dh, H * W, S.st_out, true, false));
  A.release(mk);
  CTTA_TRY(wg_join(c));   // the out head's gradients are final when this call returns
  U->bw.dh = dh;
  U->bw.active = true;
  return CTTA_OK;
}

// replays the tape entries of ONE block (all entries at the current position that share its block id); the last
// step also runs the embedding MLPs.  *block_done = id of the finished block, *finished = 1 after the last step.
static ctta_status unet_backward_next_impl(ctta_unet* U, bool dry, const GradTable* grads, hipStream_t stream,
                                           int* block_done, int* finished) {
  const ctta_unet::TrainSaved& S = U->ts;
  Arena& A = U->arena;
  BCtx c;
  bctx_init(c, U, dry, grads, stream);
  if (!dry) {
    // begin / every earlier next ended with wg_join on this stream: no scratch slot is in use any more, and the `freed`
    // events of the previous call must not be waited on when this call is captured into its OWN hipGraph (segmented
    // capture of the data-parallel step: they were recorded in another capture).
    WgradSide& Wg = U->wg;
    if (!Wg.dirty && Wg.joined_on == stream)
      for (int i = 0; i < WgradSide::NS; ++i) Wg.in_use[i] = false;
  }
  const int B = S.B;
  bf16_t* dh = U->bw.dh;
  std::vector<bf16_t*>& dskip = U->bw.dskip;
  CTTA_REQUIRE(U->bw.pos > 0, "unet_backward_next: nothing left to replay");
  const int block = U->tape[U->bw.pos - 1].block;
  while (U->bw.pos > 0 && U->tape[U->bw.pos - 1].block == block) {
    TapeOp& op = U->tape[--U->bw.pos];
    const size_t M = (size_t)B * op.H * op.W;
    switch (op.kind) {
      case TapeOp::RESNET: CTTA_TRY(bwd_resnet(c, *op.R, dh, &dh)); break;
      case TapeOp::TRANSFORMER: CTTA_TRY(bwd_transformer(c, *op.T, dh, &dh)); break;
      case TapeOp::UPSAMPLE: {   // y = conv(nearest_x2(x)): dx = 2x2 sum-pool of the conv data gradient
        bf16_t* dx = A.get<bf16_t>(M * op.ch); ALLOC_OR_FAIL(dx);
        const size_t mk = A.mark();
        bf16_t* dup = A.get<bf16_t>(M * 4 * op.ch); ALLOC_OR_FAIL(dup);
        CTTA_TRY(conv_dgrad(c, op.Lv->tsampler.d, dh, 2 * op.H, 2 * op.W, dup, 2 * op.H, 2 * op.W, false));
        RUN(c, ctta_pool2_sum(dup, dx, B, op.H, op.W, op.ch, 0, stream));
        CTTA_TRY(conv_wgrad(c, op.Lv->sampler, op.Lv->tsampler.m, op.x, op.H, op.W, true, dh));
        A.release(mk);
        dh = dx;
        break;
      }
      case TapeOp::DOWNSAMPLE: {   // stride-2 conv: zero-insert dY, then a stride-1 data-gradient conv
        bf16_t* dx = A.get<bf16_t>(M * op.ch); ALLOC_OR_FAIL(dx);
        const size_t mk = A.mark();
        const int ho = (op.H + 2 - 3) / 2 + 1, wo = (op.W + 2 - 3) / 2 + 1;
        bf16_t* dz = A.get<bf16_t>(M * op.ch); ALLOC_OR_FAIL(dz);
        RUN(c, ctta_zero_insert2(dh, dz, B, ho, wo, op.H, op.W, op.ch, stream));
        CTTA_TRY(conv_dgrad(c, op.Lv->tsampler.d, dz, op.H, op.W, dx, op.H, op.W, false));
        CTTA_TRY(conv_wgrad(c, op.Lv->sampler, op.Lv->tsampler.m, op.x, op.H, op.W, false, dh));
        A.release(mk);
        dh = dx;
        break;
      }
      case TapeOp::CONCAT: {   // torch.cat([h, skip], 1): split the gradient
        bf16_t* d0 = A.get<bf16_t>(M * op.ch); ALLOC_OR_FAIL(d0);
        bf16_t* d1 = A.get<bf16_t>(M * op.skc); ALLOC_OR_FAIL(d1);
        const int ld = op.ch + op.skc;
        RUN(c, ctta_add_slices(dh, ld, nullptr, 0, d0, op.ch, (int64_t)M, op.ch, stream));
        RUN(c, ctta_add_slices(dh + op.ch, ld, nullptr, 0, d1, op.skc, (int64_t)M, op.skc, stream));
        dskip[op.skip_idx] = d1;
        dh = d0;
        break;
      }
      case TapeOp::SKIP_PUSH: {
        bf16_t* ds = dskip[op.skip_idx];
        CTTA_REQUIRE(ds, "internal: skip %d has no gradient", op.skip_idx);
        RUN(c, ctta_add_slices(dh, op.ch, ds, op.ch, dh, op.ch, (int64_t)M, op.ch, stream));
        break;
      }
      case TapeOp::CONV_IN:
        CTTA_TRY(conv_wgrad(c, U->conv_in, U->t_conv_in.m, op.x, op.H, op.W, false, dh));
        break;
    }
  }
  U->bw.dh = dh;
  *block_done = block;
  *finished = 0;
  CTTA_TRY(wg_join(c));     // this block's weight gradients (and d temb rows) are complete
  if (U->bw.pos == 0) {
    CTTA_TRY(bwd_embeddings(c));
    *finished = 1;
    U->bw.active = false;
  }
  return CTTA_OK;
}

static ctta_status unet_backward_impl(ctta_unet* U, bool dry, const bf16_t* dpred, const GradTable* grads,
                                      hipStream_t stream, size_t* gn_need) {
  CTTA_TRY(unet_backward_begin_impl(U, dry, dpred, grads, stream));
  int block = 0, fin = 0;
  while (!fin) CTTA_TRY(unet_backward_next_impl(U, dry, grads, stream, &block, &fin));
  if (gn_need) *gn_need = 0;
  return CTTA_OK;
}

extern "C" ctta_status ctta_unet_forward_train(ctta_unet* U, const float* sample, const float* timesteps,
                                               const double* guidance, const float* enc, const uint8_t* mask, int batch,
                                               int text_len, float* out, void* stream) {
  CTTA_REQUIRE(U && sample && timesteps && enc && out, "unet_forward_train: null pointer");
  CTTA_REQUIRE(U->cfg.enable_training, "unet_forward_train: handle was created without enable_training");
  CTTA_REQUIRE(!U->row_slot, "unet_forward_train: per-request adapter rows are bound (ctta_unet_set_adapter_rows); training mixes no adapters, unbind them first");
  CTTA_REQUIRE(!U->cfg.guided || guidance, "unet_forward_train: guidance is required by the guided U-Net");
  CTTA_REQUIRE(batch >= 1 && batch <= U->cfg.max_batch, "unet_forward_train: batch %d outside [1,%d]", batch, U->cfg.max_batch);
  CTTA_REQUIRE(text_len >= 1 && text_len <= U->cfg.max_text_len, "unet_forward_train: text_len %d outside [1,%d]", text_len,
               U->cfg.max_text_len);
  WsBind bind(U->splitws);
  return unet_forward_impl(U, false, sample, timesteps, guidance, enc, mask, batch, text_len, out, (hipStream_t)stream,
                           nullptr, true);
}

extern "C" ctta_status ctta_unet_backward(ctta_unet* U, const void* dout_nhwc, const ctta_tensor* grads, int n_grads,
                                          void* stream) {
  CTTA_REQUIRE(U && dout_nhwc && grads, "unet_backward: null pointer");
  CTTA_REQUIRE(U->cfg.enable_training, "unet_backward: handle was created without enable_training");
  CTTA_REQUIRE(U->ts.valid, "unet_backward: no training forward to differentiate (call ctta_unet_forward_train first)");
  GradTable gt;
  gt.build(grads, n_grads);
  WsBind bind(U->splitws);
  const ctta_status st = unet_backward_impl(U, false, (const bf16_t*)dout_nhwc, &gt, (hipStream_t)stream, nullptr);
  U->ts.valid = false;   // one backward per training forward
  return st;
}

// Block-wise variant for overlapping the data-parallel gradient all-reduce with the backward pass:
//   begin (out head) -> next ... next until *finished.  Block ids: 0 = conv_in + embedding MLPs, 1..n = down blocks,
//   n+1 = mid block, n+2..2n+1 = up blocks, 2n+2 = conv_norm_out + conv_out (final after `begin`).
extern "C" ctta_status ctta_unet_backward_begin(ctta_unet* U, const void* dout_nhwc, const ctta_tensor* grads, int n_grads,
                                                void* stream) {
  CTTA_REQUIRE(U && dout_nhwc && grads, "unet_backward_begin: null pointer");
  CTTA_REQUIRE(U->cfg.enable_training, "unet_backward_begin: handle was created without enable_training");
  CTTA_REQUIRE(U->ts.valid, "unet_backward_begin: no training forward to differentiate (call ctta_unet_forward_train first)");
  GradTable gt;
  gt.build(grads, n_grads);
  U->ts.valid = false;
  WsBind bind(U->splitws);
  return unet_backward_begin_impl(U, false, (const bf16_t*)dout_nhwc, &gt, (hipStream_t)stream);
}
extern "C" ctta_status ctta_unet_backward_next(ctta_unet* U, const ctta_tensor* grads, int n_grads, void* stream,
                                               int* block_done, int* finished) {
  CTTA_REQUIRE(U && grads && block_done && finished, "unet_backward_next: null pointer");
  CTTA_REQUIRE(U->bw.active, "unet_backward_next: call ctta_unet_backward_begin first");
  GradTable gt;
  gt.build(grads, n_grads);
  WsBind bind(U->splitws);
  return unet_backward_next_impl(U, false, &gt, (hipStream_t)stream, block_done, finished);
}
