// The plan of one ctta_conv_gemm call (conv_plan.h): check the descriptor, fill ConvParams, choose the tile, schedule the
// launches.  No HIP call in this file: process state comes in through ConvPlanEnv, so the rules run -- and are tested --
// on a host without a GPU (ctta_conv_plan, tests/test_conv_plan_cpu.py).
#include "conv_plan.h"

namespace {

// Settled constants (their A/B switches went with round 6; the sweeps and A/Bs that fixed them are in profiles/ and LABNOTES.md)
constexpr int kSplitkMinNk = 32;       // K tiles from which a launch with few output tiles is split over K
constexpr int kSplitkTiles = 192;      // ... "few": fewer output tiles than this
constexpr int kSplitkTarget = 512;     // workgroups a split launch aims for
constexpr int kSplitkMax = 8;          // most splits
constexpr int kSplitkMinSteps = 8;     // K tiles every split keeps at least
constexpr int kBigTileMinK = 512;      // the 256x256x64 tile from this K up (straight-line epilogue, profiles/sweep_r02*.json)

// The split-K factor of a launch of `tiles` (< kSplitkTiles) output tiles that walk nk K tiles; below 2: no split
long long splitk_factor(long long tiles, long long nk) {
  long long s = kSplitkTarget / tiles;
  if (s > kSplitkMax) s = kSplitkMax;
  if (s > nk / kSplitkMinSteps) s = nk / kSplitkMinSteps;
  return s;
}

// What the rules look at besides the descriptor and ConvParams
struct Problem {
  long long M, K;
  int groups;
  bool geglu, scalar_store;
  long long x_bytes, w_bytes;
};

// ---- check ---------------------------------------------------------------------------------------------------------
ctta_status check_desc(const ctta_conv_desc* d) {
  CTTA_REQUIRE(d && d->x0 && d->w && d->out, "conv_gemm: null pointer");
  CTTA_REQUIRE(d->c0 > 0 && d->c0 % 8 == 0 && d->c1 % 8 == 0 && d->c1 >= 0,
               "conv_gemm: channel counts must be multiples of 8 (c0=%d c1=%d)", d->c0, d->c1);
  CTTA_REQUIRE(d->n > 0, "conv_gemm: n=%d must be positive", d->n);
  const bool scalar_store = d->ldc % 4 != 0;
  CTTA_REQUIRE(scalar_store || d->n % 4 == 0 ||
                   (!d->bias && !d->rowvec && !d->res && !d->accumulate && !d->out_limit && (d->n + 3) / 4 * 4 <= d->ldc),
               "conv_gemm: n=%d must be a multiple of 4 for this epilogue", d->n);
  CTTA_REQUIRE(!scalar_store || (!d->rowvec && !d->res && !d->accumulate && !d->out2 && !d->out_limit && d->out_offset == 0),
               "conv_gemm: scalar-store mode (ldc %% 4 != 0) supports only bias/bias_m epilogues");
  CTTA_REQUIRE(!d->out2 || !d->out_f32, "conv_gemm: out2 needs a bf16 primary output");
  CTTA_REQUIRE(d->k_pad % 64 == 0, "conv_gemm: k_pad=%d must be a multiple of 64", d->k_pad);
  CTTA_REQUIRE(d->kh >= 1 && d->kw >= 1 && d->stride_h >= 1 && d->stride_w >= 1 && d->dil_h >= 1 &&
                   d->dil_w >= 1, "conv_gemm: bad kernel geometry");
  CTTA_REQUIRE(!d->upsample || (d->hi % 2 == 0 && d->wi % 2 == 0), "conv_gemm: odd upsample extent");
  CTTA_REQUIRE(d->out_offset % 4 == 0, "conv_gemm: out_offset must be a multiple of 4");
  CTTA_REQUIRE(!d->res || d->res_ld % 4 == 0, "conv_gemm: res_ld must be a multiple of 4");
  CTTA_REQUIRE(!d->rowvec || d->rowvec_ld % 4 == 0, "conv_gemm: rowvec_ld must be a multiple of 4");
  CTTA_REQUIRE(d->out_act != 4 || (d->n % 32 == 0 && !d->rowvec && !d->res && !d->accumulate && !d->out2 && !d->out_f32 &&
                                   d->groups <= 1 && d->out_limit == 0 && d->out_offset == 0 && d->bias_m == nullptr &&
                                   d->alpha == 1.0f && d->ldc % 4 == 0 && d->ldc >= d->n / 2),
               "conv_gemm: the fused GEGLU epilogue takes bias only, n %% 32 == 0 and an output of half the width");
  return CTTA_OK;
}

// ---- params: descriptor -> ConvParams geometry and epilogue flags ------------------------------------------------------
ctta_status fill_params(const ctta_conv_desc* d, ConvParams& p, Problem& pr) {
  pr.scalar_store = d->ldc % 4 != 0;
  pr.geglu = d->out_act == 4;
  const bool scalar_store = pr.scalar_store, geglu = pr.geglu;
  memset(&p, 0, sizeof(p));
  p.x0 = (const bf16_t*)d->x0; p.x1 = (const bf16_t*)d->x1;
  p.c0 = d->c0; p.c1 = d->x1 ? d->c1 : 0; p.ct = p.c0 + p.c1;
  p.xs0 = d->x_stride > 0 ? d->x_stride : d->c0;
  CTTA_REQUIRE(p.xs0 >= d->c0 && p.xs0 % 8 == 0, "conv_gemm: x_stride=%d must be >= c0 and a multiple of 8", p.xs0);
  const long long M = (long long)d->batch * d->ho * d->wo;
  CTTA_REQUIRE(M > 0 && M < (1LL << 31), "conv_gemm: M out of range");
  p.M = (int)M; p.hi = d->hi; p.wi = d->wi; p.ups = d->upsample ? 1 : 0;
  p.hs = p.ups ? d->hi / 2 : d->hi; p.ws = p.ups ? d->wi / 2 : d->wi;
  p.ho = d->ho; p.wo = d->wo; p.howo = d->ho * d->wo;
  p.howo_inv = p.howo == 1 ? 0xFFFFFFFFu : (unsigned)((1ULL << 32) / (unsigned)p.howo);
  p.wo_inv = p.wo == 1 ? 0xFFFFFFFFu : (unsigned)((1ULL << 32) / (unsigned)p.wo);
  p.kh = d->kh; p.kw = d->kw; p.taps = d->kh * d->kw;
  p.sh = d->stride_h; p.sw = d->stride_w; p.ph = d->pad_h; p.pw = d->pad_w;
  p.dh = d->dil_h; p.dw = d->dil_w;
  p.w = (const bf16_t*)d->w; p.k_pad = d->k_pad; p.n = d->n;
  const long long K = (long long)p.taps * p.ct;
  CTTA_REQUIRE(K <= d->k_pad, "conv_gemm: K=%lld exceeds k_pad=%d", K, d->k_pad);
  p.bias = d->bias; p.bias_m = d->bias_m; p.rowvec = d->rowvec; p.rowvec_ld = d->rowvec_ld;
  p.res = (const bf16_t*)d->res; p.res_ld = d->res_ld;
  p.in_act = d->in_act; p.in_slope = d->in_slope; p.out_act = d->out_act; p.out_slope = d->out_slope;
  p.out2 = (bf16_t*)d->out2; p.out2_slope = d->out2_slope; p.scalar_store = scalar_store ? 1 : 0;
  p.alpha = d->alpha; p.accumulate = d->accumulate;
  p.out = d->out; p.ldc = d->ldc; p.out_f32 = d->out_f32;
  p.obs = d->out_batch_stride ? d->out_batch_stride : (long long)p.howo * d->ldc;
  p.out_offset = d->out_offset; p.out_limit = d->out_limit;
  p.xgs = d->x_group_stride; p.wgs = d->w_group_stride; p.ogs = d->out_group_stride;
  pr.M = M; pr.K = K;
  pr.groups = d->groups > 0 ? d->groups : 1;
  pr.x_bytes = (((long long)d->batch * p.hs * p.ws - 1) * p.xs0 + p.c0) * 2;
  pr.w_bytes = (long long)d->n * d->k_pad * 2;

  p.plain_out = (d->out_limit == 0 && d->out_offset == 0 && p.obs == (long long)p.howo * d->ldc) ? 1 : 0;
  p.wide_store = (!d->out_f32 && !scalar_store && d->ldc % 4 == 0 && d->n % 4 == 0 &&
                  (p.plain_out || (!geglu && p.obs % 4 == 0 && d->out_offset % 4 == 0 && d->out_limit % 4 == 0)) &&
                  (!d->res || d->res_ld % 4 == 0) && (!d->rowvec || d->rowvec_ld % 4 == 0))
                     ? 1 : 0;
  p.wide_f32 = (d->out_f32 && !scalar_store && d->ldc % 4 == 0 && d->n % 4 == 0 && p.plain_out && !d->res && !d->accumulate &&
                !d->out2 && d->out_act == 0 && d->alpha == 1.0f && !d->rowvec && !d->bias_m && !geglu && !d->gn_part) ? 1 : 0;
  p.epi_fast_geglu = (geglu && p.wide_store && p.plain_out &&
                      M * (long long)d->ldc * 2 < 0x7FFFFF00LL) ? 1 : 0;
  // (a per-sample strided, shifted, clipped destination -- the ConvTranspose upsamplers -- takes it too since round 6: one
  // descriptor per sample does the clipping; its rows cover the sample: (howo + 1) * ldc elements at most)
  const bool strided_ok = !p.plain_out && !d->res && !d->accumulate && !d->gn_part && !d->rowvec && d->out_limit > 0 &&
                          d->out_limit * 2 < 0x7FFFFF00LL && ((long long)p.howo + 1) * d->ldc * 2 < 0x7FFFFF00LL;
  p.epi_fast = (p.wide_store && (p.plain_out ? M * (long long)d->ldc * 2 < 0x7FFFFF00LL : strided_ok) &&
                (!d->res || M * (long long)d->res_ld * 2 < 0x7FFFFF00LL) && !geglu && !d->bias_m && !(d->gn_part && (d->accumulate || d->out2)) && !(d->accumulate && d->out2) &&
                (d->out_act == 0 || (d->out_act == 3 && d->out_slope >= 0.f && d->out_slope <= 1.f)) &&
                (!d->out2 || (d->out2_slope >= 0.f && d->out2_slope <= 1.f))) ? 1 : 0;
  p.epi_act = (d->alpha != 1.0f || d->out_act == 3) ? 1 : 0;
  if (p.epi_act && d->gn_part) p.epi_fast = 0;   // the statistics instantiations carry no scale / activation
  return CTTA_OK;
}

// the descriptor fast path (MODE 2) of a tile with K tiles of bk
bool fast_ok(const ctta_conv_desc* d, const ConvParams& p, const Problem& pr, int bk) {
  return p.ct % bk == 0 && p.taps <= 32 && p.c1 == 0 && !d->in_act && pr.x_bytes < 0xFFFFFF00LL && pr.w_bytes < 0xFFFFFF00LL &&
         (!p.ups || (d->kh == 3 && d->kw == 3 && d->pad_h == 1 && d->pad_w == 1 && d->stride_h == 1 &&
                     d->stride_w == 1 && d->dil_h == 1 && d->dil_w == 1));
}

// stride-1 1-D conv with Cin == Cout == 32: weight fragments straight from cache (k = tap*C + c).  Measured on MI355X
// (profiles/): 1.7x over the generic kernel at C=32; at C=64 an LDS weight ring only ties and at C=128 the
// activation tile limits the CU to one workgroup and loses 2x, so those widths stay on conv_gemm_kernel.
bool halo_eligible(const ctta_conv_desc* d, const ConvParams& p, int groups) {
  const int C = p.c0;
  if (C != 32 || p.c1 != 0 || d->n != C || groups != 1) return false;
  if (d->kh != 1 || d->hi != 1 || d->ho != 1 || d->stride_w != 1 || d->upsample || d->in_act) return false;
  if (d->wo != d->wi || p.xs0 != C || p.taps < 2) return false;
  if (d->ldc % 4 != 0 || d->out_limit != 0 || d->out_offset != 0) return false;
  return (size_t)(256 + (p.taps - 1) * p.dw) * (C + 8) * 2 <= 64 * 1024;
}

// ---- choose tile -----------------------------------------------------------------------------------------------------
// Tile choice from the on-device sweep (tools/sweep_conv.py, profiles/sweep_r01*.json).  kBigTile (256x256x64, 8 waves of
// 128x64) is judged first: it halves the L1->LDS bytes per FLOP, which is what bounds the 128-wide tiles (64 B/clk/CU vs
// 512 MFMA-cycles).
// 0: no; 1: the 256x256x64 tile, one tile per workgroup; 2: the deep case below (stream-K where the workspace allows, else 1)
int want_big_tile(long long M, int N, long long K, int groups) {
  const long long t256 = ((M + 255) / 256) * ((N + 255) / 256) * groups;
  // one workgroup per CU: 288 tiles (the distillation teacher's batch 18 at level 0) are two rounds of the 256 CUs with the
  // second one 12 % full -- 659-741 TFLOP/s against 828-910 on the thin-grid tile (profiles/sweep_r03.txt, t18 rows)
  // (a ragged last row tile that alone opens a round is cut off into its own small launch: judge the rest)
  long long tq = t256;
  const long long t_cut = (M / 256) * ((N + 255) / 256) * groups;
  if (M % 256 != 0 && groups == 1 && t_cut >= 1 && (t_cut + 255) / 256 < (t256 + 255) / 256) tq = t_cut;
  const long long rounds = (tq + 255) / 256;
  const bool fills = tq >= 1024 || tq * 10 >= rounds * 256 * 7;
  if (N >= 256 && (N % 256 == 0 || N >= 1024) && K >= kBigTileMinK && t256 >= 192 && fills) return 1;
  // Round 6 (profiles/sweep_r06_streamk_v3_coop_fold.txt, weights cold): a DEEP launch (K >= 8192) with 64 .. 191 big tiles is
  // bound by the bytes its workgroups stage per CU-clock, and the small tiles that fill every CU stage the most per FLOP.  On
  // the big tile: as stream-K (one persistent launch, one workgroup per CU, partial tiles folded in the launch) 4608 x 1024 x
  // 9216 822 TFLOP/s, 4096 x 1024 x 9216 845, 4096 x 1024 x 18432 1063, 18432 x 512 x 9216 1014; with the two-pass split-K
  // (7-8 splits) 764 / 727 / 982 / 968; round 5's choices (64x128x64, 3-stage ring, + split-K) 628 / 737 / 757 / 686.
  // Not when the 128x128x64 tile fills its 512 slots evenly (8192 x 1024 x 9216: 1049 vs 1050), which pick_variant tests first;
  // not below 64 tiles (2304 x 1024 x 9216: 548 vs 676 -- the fold traffic does not shrink with M).
  const long long t128 = ((M + 127) / 128) * ((N + 127) / 128) * groups;
  const bool even128 = t128 >= 400 && t128 < 1024 && t128 * 100 >= ((t128 + 511) / 512) * 512 * 85;
  return (N >= 512 && N % 256 == 0 && K >= 8192 && groups == 1 && t256 >= 64 && t256 < 192 && !even128) ? 2 : 0;
}
// Returns a register-staged id (1..8); choose_tile adds kTwinLds / kTwinFast for the direct-to-LDS twins.
int pick_variant(long long M, int N, long long K, int groups) {
  if (N <= 32) {                                           // 256x32; few row tiles (the per-sample cross-attention
    const long long t256 = ((M + 255) / 256) * groups;     // K / V^T projections: 18..180 workgroups walking K = 1024
    return t256 >= 512 ? kTile256x32x64 : kTile64x64x64;   // one latency-bound tile at a time): 64x64 quadruples them
  }
  if (N <= 64) return K >= 512 ? kTile128x64x64 : kTile64x64x64;
  const long long t128 = ((M + 127) / 128) * ((N + 127) / 128) * groups;
  if (t128 < 200) return kTile64x64x64;                    // too few 128x128 tiles to fill 256 CUs
  // 128x128x64 when its tiles fill the CUs about evenly (two resident workgroups per CU: 512 slots).  The batch-32 level-2
  // linears (M = 8192, t128 = 512: 736-824 vs 588-682 TFLOP/s on the thin-grid tile) and the Heun teacher's batch 16 at
  // level 1 (t128 = 512: 1024 vs 740, 1109 vs 786, 928 vs 665) take it; batch 18 (t128 = 576 = 2.25 tiles per slot pair)
  // and batch 9 (288) do NOT: 723 vs 866, 665 vs 768 -- profiles/sweep_r03.txt, u32 / t16 / t18 rows.
  if (t128 >= 400 && t128 < 1024 && K >= 512 && t128 * 100 >= ((t128 + 511) / 512) * 512 * 85) return kTile128x128x64;
  if (t128 < 1024 && (K < 4096 || t128 < 400 || N <= 512)) return kTile64x128x64;   // thin grids (distillation micro-batch): 64x128x64 doubles the workgroups
  // batch 18 at level 0 (M = 73728, N = 256: 1152 tiles = 2.25 rounds of 512 slots): the thin-grid tile beats 128x128x32
  // (828-910 vs 730, round 3) -- and from K = 2048 up 128x128x64 beats both (round 6, profiles/sweep_r06_streamk_v3_coop_fold.txt:
  // K = 4608 942 vs 798 on the 3-stage ring, K = 2304 866 vs 746-779)
  if (t128 < 1536 && K >= 1024 && N <= 512) return K >= 2048 ? kTile128x128x64 : kTile64x128x64;
  if (K >= 4096) return N >= 256 ? kTile128x128x64 : kTile64x128x64;
  if (K > 1536) return M >= 400000 ? kTile64x128x64 : kTile128x128x32;
  return N >= 256 ? kTile128x128x32 : kTile64x128x64;      // (re-swept with the wide-store epilogue)
}

// The variant id of the launch: the forced d->tile, or what the rules pick.
int choose_tile(const ctta_conv_desc* d, const ConvParams& p, const Problem& pr, ConvPlanEnv& env) {
  const long long M = pr.M, K = pr.K;
  const int groups = pr.groups;
  const bool geglu = pr.geglu;
  if (d->tile > 0 && d->tile <= kNumVariants) return d->tile;
  const int big = (!d->in_act && !geglu && fast_ok(d, p, pr, kTiles[kBigTile - 1].bk)) ? want_big_tile(M, d->n, K, groups) : 0;
  if (big) {
    // stream-K needs a workspace with a live header
    if (big == 2 && env.splitk_on() && env.streamk && env.workspace() && env.ws_hdr && !env.stamps) return kBigTileSk;
    // (round 1 sent short-K launches with a residual / second output / accumulate to the 256x128x32 tile because the
    // big tile's rolled epilogue could not hide behind another workgroup; with the straight-line epilogue the big tile
    // wins there too: profiles/sweep_r02_epi.json, 670 vs 626 TFLOP/s at K = 768)
    return kBigTile;
  }
  int vid = pick_variant(M, d->n, K, groups);
  // fused GEGLU: 128x128x32 through the wide-store epilogue (its read-back loop is rolled, so the 16-fragment tile
  // keeps its accumulators in registers); the direct epilogue only exists in the <= 8-fragment tiles (64x128x64)
  // (round 3, after the GELU rewrite: 256x128x32 with 8 waves of 64x64 wins from K = 512 up and on the batch-9 / 16
  // shapes -- 796 vs 727, 919 vs 795, 625 vs 591 TFLOP/s, profiles/sweep_r03.txt; the K = 256 batch-32 launch stays)
  if (geglu) vid = !p.wide_store ? kTile64x128x64 : ((K >= 512 || M < 100000) && fast_ok(d, p, pr, 32)) ? kTile256x128x32 : kTile128x128x32;
  // deep and narrow (few 128x128 tiles, long K): the 128x128 tile with split-K beats small tiles that only
  // exist to create workgroups (measured: M=1152, N=1024, K=9216 at 176 TFLOP/s on 64x64 tiles)
  // M = 1024 / 1152 (teacher batches, level 3): 64x128x64 + split-K 502-523 vs 414-450 TFLOP/s on 128x128x64;
  // M = 576 (batch 9, level 3): 128x64x64 346 vs 295
  // round 5 (profiles/sweep_r05_thin.txt, weights cold): a K step of these launches takes ~1750 clocks whatever the
  // tile (one K tile in flight per workgroup, ~2 workgroups per CU: tools/thin_timeline.py), so the tile that does
  // the most work per step while split-K still fills one round of the CUs wins: M <= 640: 64x128x64 with the 3-stage
  // ring and 7 splits (504 workgroups on 512 slots) 373 vs 304 TFLOP/s on 128x64x64; M <= 1280: 128x128x64 with 7
  // splits 571 vs 420 on 64x128x64
  bool thin_ring = false;
  const long long t128 = ((M + 127) / 128) * ((d->n + 127) / 128);
  if (env.splitk_on() && groups == 1 && K >= 4096 && d->n >= 256 && t128 < 192 && !pr.scalar_store && !geglu &&
      d->out_limit == 0 && d->out_offset == 0) {
    thin_ring = M <= 640;
    vid = M <= 640 ? kTile64x128x64 : kTile128x128x64;
  }
  if (!d->in_act && vid <= 8) vid += fast_ok(d, p, pr, kTiles[vid - 1].bk) ? kTwinFast : kTwinLds;
  // 64 < N <= 128 with enough rows: the 256x128x32 tile (8 waves of 64x64) stages 25 % fewer bytes per FLOP than
  // 128x128 / 64x128 and, with the wide-store epilogue, wins from K = 384 up (sweep: +12..22 %)
  const long long t28 = ((M + 255) / 256) * groups;
  if (!geglu && !d->in_act && d->n > 64 && d->n <= 128 && K >= 384 && t28 >= 512 && fast_ok(d, p, pr, 32) &&
      vid != kTile128x128x64 + kTwinFast) {
    vid = kTile256x128x32;
    // ... and from K = 1024 up with >= 2 rounds of 512-row tiles: 512x128x64 (8 waves of 128x64 = the big tile's wave
    // shape, all 160 KB of LDS): 978 vs 937-959 (K = 1152), 1074 vs 961 (K = 2304), 895 vs 806 (k = 11 conv1d) TFLOP/s
    if (K >= 1024 && (M + 511) / 512 * groups >= 512 && fast_ok(d, p, pr, 64)) vid = kTile512x128x64;
  }
  // K-heavy launches on the 64x128x64 tile whose workgroups fill whole rounds at TWO per CU: the 3-stage ring (72 KB of
  // LDS instead of 48: two K tiles in flight while one is consumed -- inside the pipeline the weights of these layers
  // arrive cold from HBM, 1.3 us per K step with one tile in flight).  Teacher loop at batch 16 (M = 4096 x N = 1024:
  // 512 workgroups; M = 16384 x N = 512: 1024): 67.7 -> 70.1 U-Net queries/s.  Batch 9 / 18 (576, 1152 workgroups: 1.1 and
  // 2.25 rounds of 512 slots where the 2-stage tile has 768) lose 2.3 ms of the distillation step with it, so the rule
  // looks at the round fill, like the tile rules above (A/B of round 3).
  // (the same move for the 128x128x64 tile -- 128x128x32 with a 3-stage ring, 48 KB -- measured slower at batch 32 and 16:
  // 25.4 vs 24.8 ms and 14.7 vs 14.5 ms per U-Net forward, tools/r3_probe35.sh)
  if (d->tile <= 0 && vid == kTile64x128x64 + kTwinFast && K >= 4096 && !geglu) {
    long long wgs = ((M + 63) / 64) * ((d->n + 127) / 128) * groups;
    if (wgs < kSplitkTiles && groups == 1 && env.splitk_on()) {      // the split-K factor the schedule will choose
      const long long sp = splitk_factor(wgs, (K + 63) / 64);
      if (sp > 1) wgs *= sp;
    }
    const long long rounds = (wgs + 511) / 512;
    if ((wgs >= 512 && wgs * 100 >= rounds * 512 * 85) || (thin_ring && wgs > 384 && wgs <= 512)) vid = kTile64x128x64Ring3;
  }
  return vid;
}

// what the chosen (or forced) tile cannot do
ctta_status check_tile(const ctta_conv_desc* d, const ConvParams& p, const Problem& pr, int vid) {
  const TileShape& v = kTiles[vid - 1];
  CTTA_REQUIRE(!(v.mode != 0 && d->in_act), "conv_gemm: in_act needs a register-staged variant (tile 1..8)");
  if (pr.geglu) {   // direct epilogue: <= 8-fragment tiles (64x64, 64x128, 128x64, 256x32); wide-store: also the 128x128 tiles
    const int frags = (v.bm / v.wm / 16) * (v.bn / v.wn / 16);     // accumulator fragments per wave
    CTTA_REQUIRE(frags <= 8 || (p.wide_store && frags <= 16),
                 "conv_gemm: the fused GEGLU epilogue needs a tile with <= 8 fragments per wave (or, wide-store, <= 16): got %s",
                 v.name);
  }
  CTTA_REQUIRE(v.mode != 2 || fast_ok(d, p, pr, v.bk),
               "conv_gemm: variant %s needs (c0+c1) %% BK == 0, one source and <= 32 taps", v.name);
  CTTA_REQUIRE((pr.K + v.bk - 1) / v.bk * v.bk <= d->k_pad, "conv_gemm: k_pad too small for BK");
  return CTTA_OK;
}

// ---- schedule --------------------------------------------------------------------------------------------------------
// Stream-K: one persistent launch, at most one workgroup per CU slot; every workgroup walks an equal share of the (tile, K
// step) items and the partial tiles are folded inside the launch in K order (ConvParams::sk_hdr, conv_gemm_sk_kernel)
// (no GroupNorm statistics from this launch: split tiles leave through the fold, not through the statistics epilogue;
// gn_nchunk stays 0 and the caller runs its statistics pass)
ctta_status schedule_streamk(const Problem& pr, ConvPlanEnv& env, ConvPlan& pl) {
  const TileShape& v = kTiles[pl.vid - 1];
  ConvParams& p = pl.p;
  CTTA_REQUIRE(pr.groups == 1 && !pr.geglu, "conv_gemm: stream-K variant %s takes ungrouped launches without the fused GEGLU", v.name);
  CTTA_REQUIRE(env.workspace() && env.ws_hdr, "conv_gemm: stream-K needs a workspace whose header was zeroed (ctta_conv_bind_workspace_ex)");
  const long long T = (long long)pl.gx * pl.gy;
  CTTA_REQUIRE(2 * T <= SK_MAX_GRID, "conv_gemm: stream-K takes at most %d output tiles (got %lld)", SK_MAX_GRID / 2, T);
  const size_t slot = (size_t)v.bm * v.bn * 4;
  const size_t hdr = (size_t)SK_HDR_WORDS * 4;
  CTTA_REQUIRE(env.ws_bytes > hdr + 2 * slot, "conv_gemm: workspace too small for stream-K");
  const long long items = T * p.nk;
  const int per_cu = (int)((160 * 1024) / ((size_t)v.stages * (v.bm + v.bn) * v.bk * 2));
  long long G = (long long)env.cu_count * (per_cu < 1 ? 1 : per_cu > 2 ? 2 : per_cu);
  if (env.streamk_grid > 0) G = env.streamk_grid;
  if (G > items / 4) G = items / 4;          // >= 4 K steps per workgroup
  if (G > SK_MAX_GRID) G = SK_MAX_GRID;
  if (G < 1) G = 1;
  if (hdr + (size_t)2 * G * slot > env.ws_bytes) G = (long long)((env.ws_bytes - hdr) / (2 * slot));   // two slots per workgroup
  if (G >= 8) G &= ~7LL;      // whole rounds of the 8 XCDs (the chunk arithmetic of the kernel needs it)
  // XCD chunks (conv_gemm_sk_kernel): the most chunks of whole tiles whose largest is within 6 % of the mean
  int nch = 1;
  for (int c = 8; c > 1; c >>= 1) {
    if (G % 8 != 0 || T < c) continue;
    const long long big = (T + c - 1) / c;
    if (big * c * 100 <= T * 106 && (T / c) * p.nk >= 4 * (G / c)) { nch = c; break; }
  }
  if (!env.xcd) nch = 1;
  p.sk_chunks = nch;
  p.m_tiles = (int)pl.gx; p.n_tiles = (int)pl.gy; p.sk_tiles = (int)T;
  p.sk_m_inner = pr.w_bytes > pr.x_bytes ? 1 : 0;       // weight-dominated: the row tiles of one weight slab run next to each other
  pl.gx = (unsigned)G; pl.gy = 1; pl.gz = 1;
  return CTTA_OK;
}

// One tile per workgroup: split-K, the ragged tail, the tile order, GroupNorm partials
void schedule_tiles(const ctta_conv_desc* d, const Problem& pr, ConvPlanEnv& env, ConvPlan& pl) {
  const TileShape& v = kTiles[pl.vid - 1];
  ConvParams& p = pl.p;
  const long long M = pr.M;
  const int groups = pr.groups;
  const bool geglu = pr.geglu;
  // split-K: deep, narrow problems (the 1024-channel levels at small batch: M <= 2304, K = 9216 / 18432) launch
  // too few workgroups to fill 256 CUs; split the K walk over blockIdx.z and reduce in a second pass
  const long long tiles = (long long)pl.gx * pl.gy;
  const int ld = (d->n + 3) / 4 * 4;
  int splits = 1;
  if (env.splitk_on() && groups == 1 && !pr.scalar_store && !geglu && d->out_limit == 0 && d->out_offset == 0 &&
      tiles < kSplitkTiles && p.nk >= kSplitkMinNk && env.workspace() && env.ws_bytes > (size_t)SK_HDR_WORDS * 4) {
    splits = (int)splitk_factor(tiles, p.nk);
    if (splits < 1) splits = 1;
    // (the slabs start behind the stream-K header, which stays untouched)
    if ((long long)splits * M * ld * 4 > (long long)(env.ws_bytes - (size_t)SK_HDR_WORDS * 4)) splits = 1;
  }
  // Ragged last row tile of a 256-row-tile launch: when it alone opens another round of the CUs, it leaves this launch
  // (one row tile fewer) and runs as a second launch with 64x64 tiles behind it (the same rows, the same epilogue; rows
  // are independent, so this is exact).  M = 163872, N = 512: 1282 -> 1280 big tiles = 5 rounds instead of 5 + a round
  // of two half-idle workgroups, plus ~16 small workgroups.
  int tail_rows = 0;
  {
    const long long slots = 256LL * (pl.vid == kTile256x128x32 ? 2 : 1);
    const long long t_all = (long long)pl.gx * pl.gy, t_cut = (long long)(pl.gx - 1) * pl.gy;
    if (d->tile <= 0 && v.bm == 256 && v.mode != 0 && splits == 1 && groups == 1 && M % 256 != 0 && pl.gx > 1 &&
        !geglu && !d->gn_part && !env.stamps && (t_all + slots - 1) / slots > (t_cut + slots - 1) / slots) {
      tail_rows = (int)(M % 256);
      pl.gx -= 1;
    }
  }
  // (launches whose weights outweigh their activations take the weight-slab mapping below instead, whatever their row tiles)
  const bool slab_pref = groups == 1 && pl.gy >= 2 && pr.w_bytes > pr.x_bytes && tail_rows == 0;
  if (splits == 1 && groups == 1 && env.xcd && pl.gx >= 64 && !slab_pref) {
    p.m_tiles = (int)pl.gx; p.n_tiles = (int)pl.gy;
    p.xcd_per = (p.m_tiles + 7) / 8;
    // few N tiles: visit them back to back per M tile (the input tile is read once per XCD); many N tiles (wide
    // linears: the weight matrix is far larger than L2): keep one weight slice hot and walk the XCD's M range
    p.n_inner = (p.n_tiles <= 4 || pr.w_bytes <= (2LL << 20)) ? 1 : 0;   // a <= 2 MB weight matrix stays L2-resident anyway
    pl.gx = (unsigned)(8 * p.xcd_per * p.n_tiles); pl.gy = 1; pl.gz = 1;
  }
  if (d->gn_part && d->gn_groups > 0 && d->gn_hw > 0 && splits == 1 && groups == 1 && p.wide_store && !geglu) {
    // GroupNorm partials from the epilogue: whole tiles per sample, whole groups per tile, a lane's 4 channels in one group
    const int cpg = d->n % d->gn_groups == 0 ? d->n / d->gn_groups : 0;
    const int tn = v.bn / v.wn;
    if (cpg >= 4 && (cpg & (cpg - 1)) == 0 && v.bn % cpg == 0 && d->gn_hw % v.bm == 0 && M % d->gn_hw == 0) {
      const int sub = cpg > tn ? cpg / tn : 1;
      const int nchunk = d->gn_hw / v.bm * v.wm * sub;
      if ((long long)(M / d->gn_hw) * nchunk * d->gn_groups * 2 <= (long long)d->gn_part_floats) {
        p.gn_part = (float*)d->gn_part; p.gn_cpg = cpg; p.gn_G = d->gn_groups; p.gn_hw = d->gn_hw;
        p.gn_nchunk = nchunk;
      }
    }
  }
  // Weight-slab affinity (see ConvParams::slab_total): every split-K launch, and unsplit launches whose few row tiles the
  // M-range mapping above does not take (grid.x < 64) when the weights outweigh the activations and there are slabs enough
  // to give every XCD its own.
  bool slab = false;
  if (groups == 1 && env.xcd && p.xcd_per == 0) {
    if (splits > 1) slab = true;
    else if (pl.gy >= 2 && (long long)pl.gx * pl.gy >= 16 && pr.w_bytes > pr.x_bytes && tail_rows == 0) slab = true;
  }
  if (slab && splits == 1) {
    p.m_tiles = (int)pl.gx; p.n_tiles = (int)pl.gy;
    p.slab_total = p.m_tiles * p.n_tiles;
    p.slab_per = (p.slab_total + 7) / 8;
    pl.gx = (unsigned)(8 * p.slab_per); pl.gy = 1; pl.gz = 1;
  }
  if (splits > 1) {
    ConvParams& q = pl.q;
    q = p;   // first pass: raw partial sums (q.out: the workspace behind its header, bound at the launch)
    q.nk_split = (p.nk + splits - 1) / splits;
    splits = (p.nk + q.nk_split - 1) / q.nk_split;   // every split owns at least one K-tile
    q.ksplit = splits;
    q.bias = nullptr; q.bias_m = nullptr; q.rowvec = nullptr; q.res = nullptr; q.out_act = 0; q.alpha = 1.0f;
    q.accumulate = 0; q.out2 = nullptr; q.out = nullptr; q.ldc = ld; q.out_f32 = 1; q.obs = (long long)p.howo * ld;
    q.wide_store = 0;
    q.wide_f32 = conv_wide_f32_ok(v.bm, v.bn, v.bk, v.wm, v.wn, v.mode, v.stages) ? 1 : 0;
    q.ogs = (long long)M * ld;
    pl.gz = (unsigned)splits;
    if (slab) {
      q.m_tiles = (int)pl.gx; q.n_tiles = (int)pl.gy;
      q.slab_total = q.m_tiles * q.n_tiles * splits;
      q.slab_per = (q.slab_total + 7) / 8;
      pl.gx = (unsigned)(8 * q.slab_per); pl.gy = 1; pl.gz = 1;
    }
    const long long total = M * (ld / 4);
    pl.ld = ld;
    pl.finish_blocks = (int)((total + 255) / 256);
    if (pl.finish_blocks > 4096) pl.finish_blocks = 4096;
  } else if (tail_rows > 0) {
    // 64x64x64, descriptor staging where a K tile never straddles a tap
    pl.tail_vid = kTile64x64x64 + ((v.mode == 2 && fast_ok(d, p, pr, 64)) ? kTwinFast : kTwinLds);
    const TileShape& tv = kTiles[pl.tail_vid - 1];
    ConvParams& t = pl.t;
    t = p;
    t.m_off = (int)(M - tail_rows);
    t.xcd_per = 0; t.m_tiles = 0; t.n_tiles = 0; t.n_inner = 0; t.slab_total = 0; t.slab_per = 0;
    t.nk = (int)((pr.K + tv.bk - 1) / tv.bk);
    t.nk_split = t.nk;
    pl.tail_gx = (unsigned)((tail_rows + tv.bm - 1) / tv.bm);
    pl.tail_gy = (unsigned)((d->n + tv.bn - 1) / tv.bn);
  }
  pl.splits = splits;
  pl.tail_rows = tail_rows;
}

}  // namespace

ctta_status ctta_conv_make_plan(const ctta_conv_desc* d, ConvPlanEnv& env, ConvPlan& pl) {
  CTTA_TRY(check_desc(d));
  memset(&pl, 0, sizeof(pl));
  Problem pr;
  CTTA_TRY(fill_params(d, pl.p, pr));
  ConvParams& p = pl.p;
  pl.M = pr.M; pl.K = pr.K; pl.groups = pr.groups;
  pl.splits = 1;
  if (d->tile <= 0 && halo_eligible(d, p, pr.groups)) {
    pl.halo = true;
    pl.prof_code = kHaloProfCode;
    pl.gx = (unsigned)((p.wo + 255) / 256); pl.gy = (unsigned)d->batch; pl.gz = 1;
    return CTTA_OK;
  }
  pl.vid = choose_tile(d, p, pr, env);
  CTTA_TRY(check_tile(d, p, pr, pl.vid));
  const TileShape& v = kTiles[pl.vid - 1];
  pl.kind = v.kind;
  if (!conv_wide_f32_ok(v.bm, v.bn, v.bk, v.wm, v.wn, v.mode, v.stages)) p.wide_f32 = 0;
  p.x_bytes = (unsigned)pr.x_bytes; p.w_bytes = (unsigned)pr.w_bytes;
  p.nk = (int)((pr.K + v.bk - 1) / v.bk);
  p.ksplit = 1; p.nk_split = p.nk;
  pl.prof_code = pl.vid + ((p.epi_fast || p.epi_fast_geglu) ? 0 : 100);   // +100: generic epilogue
  pl.gx = (unsigned)((pr.M + v.bm - 1) / v.bm); pl.gy = (unsigned)((d->n + v.bn - 1) / v.bn); pl.gz = (unsigned)pr.groups;
  if (v.kind >= 2) return schedule_streamk(pr, env, pl);
  schedule_tiles(d, pr, env, pl);
  return CTTA_OK;
}

// ------------------------------------------------------------------------------------------
extern "C" ctta_status ctta_conv_plan(const ctta_conv_desc* d, const ctta_conv_plan_env* e, ctta_conv_plan_info* out) {
  CTTA_REQUIRE(e && out, "ctta_conv_plan: null pointer");
  ConvPlanEnv env;
  memset(&env, 0, sizeof(env));
  env.cu_count = e->cu_count;
  env.xcd = e->xcd; env.splitk = e->splitk; env.streamk = e->streamk; env.streamk_grid = e->streamk_grid;
  env.no_splitk = e->suppress_splitk != 0;
  env.stamps = e->stamps_bound != 0;
  env.ws_ok = e->workspace_bytes > 0; env.ws_bytes = (size_t)e->workspace_bytes; env.ws_hdr = env.ws_ok && e->workspace_header_zeroed;
  ConvPlan pl;
  memset(out, 0, sizeof(*out));
  CTTA_TRY(ctta_conv_make_plan(d, env, pl));
  const ConvParams& p = pl.p;
  const ConvParams& f = pl.splits > 1 ? pl.q : pl.p;      // what the (first) tile launch runs with
  out->variant = pl.vid; out->kind = pl.kind; out->halo = pl.halo ? 1 : 0; out->prof_code = pl.prof_code;
  out->grid_x = (int)pl.gx; out->grid_y = (int)pl.gy; out->grid_z = (int)pl.gz;
  out->splits = pl.splits; out->nk = f.nk; out->nk_split = f.nk_split; out->finish_blocks = pl.finish_blocks;
  out->tail_rows = pl.tail_rows; out->tail_variant = pl.tail_vid;
  out->tail_grid_x = (int)pl.tail_gx; out->tail_grid_y = (int)pl.tail_gy; out->tail_nk = pl.t.nk;
  out->xcd_per = f.xcd_per; out->m_tiles = f.m_tiles; out->n_tiles = f.n_tiles; out->n_inner = f.n_inner;
  out->slab_total = f.slab_total; out->slab_per = f.slab_per;
  out->sk_chunks = p.sk_chunks; out->sk_m_inner = p.sk_m_inner;
  out->gn_nchunk = p.gn_nchunk;
  out->plain_out = p.plain_out; out->wide_store = p.wide_store; out->wide_f32 = p.wide_f32; out->splitk_wide_f32 = pl.splits > 1 ? pl.q.wide_f32 : 0;
  out->epi_fast = p.epi_fast; out->epi_fast_geglu = p.epi_fast_geglu; out->epi_act = p.epi_act;
  return CTTA_OK;
}
