// Paired metrics of the evaluation suite (audioldm_eval/eval.py:137-179), batched over the pairs of a chunk:
//   ctta_lsd        log-spectral distance of ssr_eval.metrics.AudioMetrics.lsd (behind eval.py:154,160-162) on two magnitude
//                   spectrograms: mean over frames of sqrt(mean over bins of log10(T^2 / (E + 1e-12)^2 + 1e-12)^2)
//   ctta_ssim_mean  skimage.metrics.structural_similarity with its defaults (uniform win x win window, K1 = 0.01, K2 = 0.03,
//                   sample covariance), the mean over the positions whose whole window lies inside the image (eval.py:177 on
//                   the normalised mels, AudioMetrics.ssim on the magnitude spectrograms)
//   ctta_psnr_mse   the mean squared difference under skimage.metrics.peak_signal_noise_ratio (eval.py:172)
// ssr_eval and skimage are pip dependencies of the reference, not part of its tree: the definitions are the published ones,
// restated in float64 numpy in tests/paired_metrics_ref.py.
// The inputs are fp32; every sum, the window moments and the per-pixel SSIM are formed in fp64 (uxx - ux^2 on magnitudes of
// order 10^2 loses in fp32 the digits C2 is compared against), and every sum runs in a fixed order: per-frame / per-row /
// per-tile partial results go to a workspace, a second launch adds them per pair.  No floating-point atomics, so two calls
// give the same bits.  Per-pair extents travel by value in the kernel arguments (at most CTTA_PAIR_MAX pairs per call).
// All of it is HBM- and latency-bound work on a few MB beside the STFT that feeds it.
#include "common.h"

#include <math.h>

// a == b must give a / b == 1 exactly (identical images score 1.0 as in numpy): no fused multiply-adds in this file
#pragma clang fp contract(off)

struct PairLens {
  int v[CTTA_PAIR_MAX];
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// 256 partial sums of a workgroup, added as a fixed binary tree; the total is valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// stage 2 of all three metrics: out[p] = (sum of the pair's partials) / ((len - sub) * unit); the pair has
// ceil((len - sub) / th) * tx partials at ws[p * stride]
__global__ __launch_bounds__(256) void pair_reduce_kernel(const double* __restrict__ ws, long long stride, PairLens lens, int sub,
                                                          int th, int tx, double unit, double* __restrict__ out) {
  __shared__ double red[256];
  const int p = blockIdx.x, n = lens.v[p] - sub;
  const int cnt = (n + th - 1) / th * tx;
  const double* w = ws + (size_t)p * stride;
  double acc = 0.0;
  for (int i = threadIdx.x; i < cnt; i += 256) acc += w[i];
  const double total = block_sum_f64(acc, red);
  if (threadIdx.x == 0) out[p] = total / ((double)n * unit);
}

// one wave per frame: sqrt(mean over bins of log10(T^2 / (E + 1e-12)^2 + 1e-12)^2)
__global__ __launch_bounds__(256) void lsd_frames_kernel(const float* __restrict__ est, const float* __restrict__ tgt,
                                                         int frames_max, int bins, PairLens frames, double* __restrict__ ws) {
  const int p = blockIdx.y, t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= frames.v[p]) return;
  const size_t row = ((size_t)p * frames_max + t) * bins;
  double acc = 0.0;
  for (int k = lane; k < bins; k += 64) {
    const double e = (double)est[row + k] + 1e-12, g = (double)tgt[row + k];
    const double l = log10((g * g) / (e * e) + 1e-12);
    acc += l * l;
  }
  acc = wave_sum_f64(acc);
  if (lane == 0) ws[(size_t)p * frames_max + t] = sqrt(acc / (double)bins);
}

extern "C" ctta_status ctta_lsd(const float* est, const float* tgt, int pairs, int frames_max, int bins, const int32_t* frames,
                                double* lsd, double* ws, void* stream) {
  CTTA_REQUIRE(est && tgt && frames && lsd && ws, "lsd: null pointer");
  CTTA_REQUIRE(pairs >= 1 && pairs <= CTTA_PAIR_MAX && frames_max >= 1 && bins >= 1,
               "lsd: pairs=%d (1..%d), frames_max=%d, bins=%d", pairs, CTTA_PAIR_MAX, frames_max, bins);
  PairLens L;
  for (int p = 0; p < pairs; ++p) {
    CTTA_REQUIRE(frames[p] >= 1 && frames[p] <= frames_max, "lsd: pair %d has %d frames (1..%d)", p, frames[p], frames_max);
    L.v[p] = frames[p];
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lsd_frames_kernel, dim3((frames_max + 3) / 4, pairs), dim3(256), 0, s, est, tgt, frames_max, bins, L, ws);
  CTTA_LAUNCH_CHECK();
  hipLaunchKernelGGL(pair_reduce_kernel, dim3(pairs), dim3(256), 0, s, ws, (long long)frames_max, L, 0, 1, 1, 1.0, lsd);
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}

// one wave per row: sum over the row of (x - y)^2
__global__ __launch_bounds__(256) void sqdiff_rows_kernel(const float* __restrict__ x, const float* __restrict__ y, int h_max,
                                                          int W, PairLens hv, double* __restrict__ ws) {
  const int p = blockIdx.y, r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= hv.v[p]) return;
  const size_t row = ((size_t)p * h_max + r) * W;
  double acc = 0.0;
  for (int c = lane; c < W; c += 64) {
    const double d = (double)x[row + c] - (double)y[row + c];
    acc += d * d;
  }
  acc = wave_sum_f64(acc);
  if (lane == 0) ws[(size_t)p * h_max + r] = acc;
}

extern "C" ctta_status ctta_psnr_mse(const float* x, const float* y, int pairs, int h_max, int w, const int32_t* h_valid,
                                     double* mse, double* ws, void* stream) {
  CTTA_REQUIRE(x && y && h_valid && mse && ws, "psnr_mse: null pointer");
  CTTA_REQUIRE(pairs >= 1 && pairs <= CTTA_PAIR_MAX && h_max >= 1 && w >= 1, "psnr_mse: pairs=%d (1..%d), h_max=%d, w=%d", pairs,
               CTTA_PAIR_MAX, h_max, w);
  PairLens L;
  for (int p = 0; p < pairs; ++p) {
    CTTA_REQUIRE(h_valid[p] >= 1 && h_valid[p] <= h_max, "psnr_mse: pair %d has %d rows (1..%d)", p, h_valid[p], h_max);
    L.v[p] = h_valid[p];
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sqdiff_rows_kernel, dim3((h_max + 3) / 4, pairs), dim3(256), 0, s, x, y, h_max, w, L, ws);
  CTTA_LAUNCH_CHECK();
  hipLaunchKernelGGL(pair_reduce_kernel, dim3(pairs), dim3(256), 0, s, ws, (long long)h_max, L, 0, 1, 1, (double)w, mse);
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}

// A workgroup takes a tile of SS_TH x SS_TW window positions: the (SS_TH + win - 1) x (SS_TW + win - 1) pixels under them go
// to LDS, the five moments (x, y, xx, yy, xy) are summed along the rows first (hs), then down the columns as running sums
// (window r + 1 = window r + the row entering - the row leaving), three positions per thread.
constexpr int SS_TH = 24, SS_TW = 32, SS_WIN_MAX = 11;
constexpr int SS_IH = SS_TH + SS_WIN_MAX - 1, SS_IW = SS_TW + SS_WIN_MAX - 1;

__global__ __launch_bounds__(256) void ssim_tiles_kernel(const float* __restrict__ x, const float* __restrict__ y, int h_max, int W,
                                                         PairLens hv, int win, double c1, double c2, double cov_norm, int tiles_x,
                                                         long long ws_stride, double* __restrict__ ws) {
  __shared__ float sx[SS_IH][SS_IW], sy[SS_IH][SS_IW];
  __shared__ double hs[5][SS_IH][SS_TW];
  __shared__ double red[256];
  const int p = blockIdx.z, tid = threadIdx.x;
  const int oh = hv.v[p] - win + 1, ow = W - win + 1;        // window positions of this pair's image
  const int r0 = blockIdx.y * SS_TH, c0 = blockIdx.x * SS_TW;
  if (r0 >= oh) return;                                       // a shorter pair of the chunk (whole workgroup)
  const int th = min(SS_TH, oh - r0), tw = min(SS_TW, ow - c0);
  const int ih = th + win - 1, iw = tw + win - 1;             // r0 + ih <= H, c0 + iw <= W
  const size_t base = (size_t)p * h_max * W;
  for (int i = tid; i < ih * iw; i += 256) {
    const int r = i / iw, c = i - r * iw;
    const size_t src = base + (size_t)(r0 + r) * W + c0 + c;
    sx[r][c] = x[src];
    sy[r][c] = y[src];
  }
  __syncthreads();
  for (int i = tid; i < ih * tw; i += 256) {
    const int r = i / tw, c = i - r * tw;
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < win; ++k) {
      const double a = (double)sx[r][c + k], b = (double)sy[r][c + k];
      m[0] += a; m[1] += b; m[2] += a * a; m[3] += b * b; m[4] += a * b;
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) hs[j][r][c] = m[j];
  }
  __syncthreads();
  const int c = tid & (SS_TW - 1), o0 = (tid / SS_TW) * 3, o1 = min(o0 + 3, th);
  double acc = 0.0;
  if (c < tw && o0 < th) {
    const double np_ = (double)(win * win);   // divided by, not multiplied with a rounded 1 / 49: a constant window has ux * ux == uxx
    double m[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      double v = 0.0;
      for (int k = 0; k < win; ++k) v += hs[j][o0 + k][c];
      m[j] = v;
    }
    for (int o = o0;;) {
      const double ux = m[0] / np_, uy = m[1] / np_, uxx = m[2] / np_, uyy = m[3] / np_, uxy = m[4] / np_;
      const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
      const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2, b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
      acc += (a1 * a2) / (b1 * b2);
      if (++o >= o1) break;
#pragma unroll
      for (int j = 0; j < 5; ++j) m[j] += hs[j][o + win - 1][c] - hs[j][o - 1][c];
    }
  }
  const double total = block_sum_f64(acc, red);
  if (tid == 0) ws[(size_t)p * ws_stride + (size_t)blockIdx.y * tiles_x + blockIdx.x] = total;
}

extern "C" int64_t ctta_ssim_tiles(int h, int w, int win) {
  if (win < 1 || h < win || w < win) return 0;
  return cdiv64(h - win + 1, SS_TH) * cdiv64(w - win + 1, SS_TW);
}

extern "C" ctta_status ctta_ssim_mean(const float* x, const float* y, int pairs, int h_max, int w, const int32_t* h_valid,
                                      int win, double data_range, int sample_covariance, double* ssim, double* ws,
                                      void* stream) {
  CTTA_REQUIRE(x && y && h_valid && ssim && ws, "ssim_mean: null pointer");
  CTTA_REQUIRE(win >= 3 && win <= SS_WIN_MAX && (win & 1), "ssim_mean: win=%d must be odd, 3..%d", win, SS_WIN_MAX);
  CTTA_REQUIRE(pairs >= 1 && pairs <= CTTA_PAIR_MAX && h_max >= win && w >= win,
               "ssim_mean: pairs=%d (1..%d); h_max=%d and w=%d must hold one %dx%d window", pairs, CTTA_PAIR_MAX, h_max, w, win, win);
  CTTA_REQUIRE(data_range > 0.0 && (sample_covariance == 0 || sample_covariance == 1),
               "ssim_mean: data_range=%g must be positive, sample_covariance=%d in {0, 1}", data_range, sample_covariance);
  PairLens L;
  for (int p = 0; p < pairs; ++p) {
    CTTA_REQUIRE(h_valid[p] >= win && h_valid[p] <= h_max, "ssim_mean: pair %d has %d rows (%d..%d)", p, h_valid[p], win, h_max);
    L.v[p] = h_valid[p];
  }
  const int tiles_x = (int)cdiv64(w - win + 1, SS_TW), tiles_y = (int)cdiv64(h_max - win + 1, SS_TH);
  CTTA_REQUIRE(tiles_y <= 65535, "ssim_mean: h_max=%d is more than %d rows", h_max, 65535 * SS_TH);
  const double np_ = (double)(win * win), c1 = (0.01 * data_range) * (0.01 * data_range),
               c2 = (0.03 * data_range) * (0.03 * data_range);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ssim_tiles_kernel, dim3(tiles_x, tiles_y, pairs), dim3(256), 0, s, x, y, h_max, w, L, win, c1, c2,
                     sample_covariance ? np_ / (np_ - 1.0) : 1.0, tiles_x, (long long)tiles_x * tiles_y, ws);
  CTTA_LAUNCH_CHECK();
  hipLaunchKernelGGL(pair_reduce_kernel, dim3(pairs), dim3(256), 0, s, ws, (long long)tiles_x * tiles_y, L, win - 1, SS_TH,
                     tiles_x, (double)(w - win + 1), ssim);
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}
