// The plan of one layer's weight gradient (wgrad_plan.h).  No HIP call in this file: the rules run -- and are tested -- on a
// host without a GPU (ctta_wgrad_plan, tests/test_wgrad_plan_cpu.py).
//
// dW[k][n] = sum_m Q[k][m] * dY^T[n][m] as a split-M GEMM into slabs[s][n][r]: one row per OUTPUT channel n, r = (cin, kh, kw)
// index of the weight row, then the bias column, then `nb` per-sample columns -- the state dict's own row layout, so the
// scatter is a coalesced streaming add.  x is the layer input in NHWC (a linear is the 1x1 case with batch = 1, hi = rows).
#include "wgrad_plan.h"

namespace {

// splits doubled while the launch stays under `target` workgroups and `cap` splits and every split keeps `min_m` positions
int splits_for(int64_t tiles, int64_t M, int target, int cap, int min_m) {
  int S = 1;
  while (tiles * S < target && S < cap && M / (2 * S) >= min_m) S *= 2;
  return S;
}
int64_t tiles_of(int a, int ta, int b, int tb) { return (int64_t)((a + ta - 1) / ta) * ((b + tb - 1) / tb); }

}  // namespace

extern "C" ctta_status ctta_wgrad_plan(const ctta_wgrad_geom* g, const ctta_wgrad_policy* pol, ctta_wgrad_plan_info* out) {
  CTTA_REQUIRE(g && pol && out, "ctta_wgrad_plan: null pointer");
  memset(out, 0, sizeof(*out));
  const int taps = g->kh * g->kw, C = g->c, N = g->n, nb = g->nb;
  const int64_t M = (int64_t)g->batch * g->ho * g->wo;
  CTTA_REQUIRE(taps > 0 && C > 0 && N > 0 && nb >= 0 && M > 0 && M < (1LL << 31) - 4096,
               "ctta_wgrad_plan: bad geometry (taps=%d c=%d n=%d nb=%d positions=%lld)", taps, C, N, nb, (long long)M);
  const int K = taps * C;
  out->rows = K + 1 + nb;
  out->ld = round_up(out->rows, 4);
  const bool direct = pol->direct && g->direct_ok && nb == 0;
  int S;
  if (taps == 1 && !g->upsample && g->stride == 1 && g->pad == 0 && nb == 0 && C % 8 == 0 && N % 8 == 0) {
    // 1x1 layers: both operands read WHERE THEY LIE by ctta_wgrad_tn (no dY^T, no X^T copy).  On a side stream this needs dY
    // to stay valid until the join: the U-Net's backward releases nothing while its side stream is on, and no dY is
    // rewritten in place (the transformer's token-stream gradient moves to a new buffer at every LayerNorm backward).
    // 128 x 128 tiles; the U-Net's level-0 / level-1 linears have 4..16 tiles over 9 216..36 864 rows.  256 workgroups, at
    // most 32 splits of >= 128 rows: pipelined step 77.5 -> 76.2 ms against 512 / 64, too narrow (64 workgroups, 8
    // splits) loses 4 ms (profiles/ab_r05_wgrad_splits.txt).  Not the implicit kernel: its 1-tap tiling reads LDS once per MFMA.
    S = splits_for(tiles_of(N, 128, C, 128), M, 256, 32, 128);
    out->route = S == 1 && direct ? CTTA_WGRAD_TN_DIRECT : CTTA_WGRAD_TN;
  } else if ((!g->upsample || pol->upsample_copy) && g->stride == 1 && g->ho == g->hi && g->wo == g->wi && taps == 9 && g->kh == 3 &&
             g->pad == 1 && ctta_wgrad_implicit_supported(9, C, g->hi, g->wi, C, N) != 0) {
    // 3x3 stride-1 layers inside the implicit kernel's range: the layer input read in place through LDS transpose reads
    // (wgrad_gemm.hip), 64 x 64 (x 9 taps) tiles.  dY is read in place too when the kernel can (n % 8, per-sample columns
    // only over whole 64-position chunks) and dY outlives the job: no convolution's dY is rewritten by the main stream
    // later, so that is the handle's arena policy.  Otherwise over a dY^T copy.
    S = splits_for(tiles_of(N, 64, C, 64), M, pol->implicit_target, pol->implicit_cap, 256);
    const bool inplace = N % 8 == 0 && (nb == 0 || (g->ho * g->wo) % 64 == 0) && (!g->run_async || g->keeps_dy);
    out->route = !inplace ? CTTA_WGRAD_IMPLICIT_DYT : S == 1 && direct ? CTTA_WGRAD_IMPLICIT_DIRECT : CTTA_WGRAD_IMPLICIT_INPLACE;
    out->upsample_copy = g->upsample ? 1 : 0;
  } else {
    // everything else (stride-2 / upsampling samplers, the U-Net's 8-channel conv_in, widths the implicit kernel does not
    // take): both operands made m-contiguous -- dY^T and im2col^T, whose rows are (channel, tap), the all-ones row, then the
    // per-sample indicator rows -- and multiplied by conv_gemm, 128 x 128 tiles.  The GEMM produces the K weight columns
    // only; the bias column (and the per-sample columns behind it) are row sums of dY^T (ctta_wgrad_rowsum): as GEMM rows
    // they cost a whole extra tile column (N = 257 ran 3 column tiles of 128 for 2 tiles of work).
    S = splits_for(tiles_of(out->rows, 128, N, 128), M, 256, 16, 256);
    out->route = CTTA_WGRAD_IM2COL_T;
  }
  out->splits = S;
  out->mp = (int)round_up64(M, 64 * S);
  out->seg = out->mp / S;
  const bool direct_route = out->route == CTTA_WGRAD_TN_DIRECT || out->route == CTTA_WGRAD_IMPLICIT_DIRECT;
  out->slabs = direct_route ? 0 : (int64_t)S * N * out->ld;
  if (out->route == CTTA_WGRAD_IM2COL_T) {
    out->q = (int64_t)out->rows * out->mp;
    out->sums_apart = (nb == 0 || (g->ho * g->wo) % 8 == 0) && out->mp % (8 * S) == 0;
  }
  if (out->route == CTTA_WGRAD_IM2COL_T || out->route == CTTA_WGRAD_IMPLICIT_DYT) out->pt = (int64_t)N * out->mp;
  if (out->upsample_copy) out->xu = M * C;
  return CTTA_OK;
}

extern "C" ctta_status ctta_wgrad_engine_policy(int engine, ctta_wgrad_policy* out) {
  CTTA_REQUIRE(out && (engine == 0 || engine == 1), "ctta_wgrad_engine_policy: engine must be 0 (U-Net) or 1 (VAE decoder)");
  *out = engine == 0 ? kWgradPolicyUnet : kWgradPolicyVae;
  return CTTA_OK;
}
