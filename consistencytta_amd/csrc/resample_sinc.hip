// Band-limited resampling of the file loaders (tools/torch_tools.py:54-75 `read_wav_file`, tools/t2a_dataset.py:111-122,
// audioldm_eval/datasets/load_mel.py:25-28, metrics/fad.py:33-34) for a ragged batch of clips:
//   ctta_resample_sinc  resampy.resample(x, sr_orig, sr_new, filter="kaiser_best") (torch_tools.py:66)
//   ctta_wave_prepare   the tail of read_wav_file (torch_tools.py:69-73): mean removal, peak 0.5, cut / pad, peak 0.5 again
// resampy is a pip dependency of the reference, not part of its tree: the arithmetic is the published definition of version
// 0.4.2 (core.resample + interpn.resample_f), restated in float64 numpy in tests/resampy_ref.py.
//
// resampy is not an exact polyphase filter: it interpolates linearly in a 32769-entry table and walks the table with the
// TRUNCATED integer stride int(scale * num_table), so the weights are a discontinuous function of the output position.
// The position arithmetic below is therefore the float64 expressions of interpn.resample_f, evaluated as written and
// without contraction (t * time_increment - n must not become one fused operation); fp32 cannot hold t * time_increment
// of a 10 s clip at all.  Table entries and samples are fp32 (PCM16 / 32768 is exact), a weight is formed in fp64 from two
// neighbouring entries and every product is added to an fp64 sum: left wing first, then the right wing, tap by tap, one
// thread per output -- an order that does not depend on the tiling, so a clip gives the same bits alone or in any batch.
//
// A workgroup owns RS_RUN consecutive outputs of one clip and stages the input span they touch into LDS (4.2 KB for
// 44100 -> 16000); the table (128 KB) stays in global memory and is gathered through the caches: neighbouring outputs
// start at offsets inside one stride (185 entries = 740 B) and advance together, so a wave's gather touches a few lines.
// A run whose span would not fit RS_SPAN floats is cut into shorter runs by the workgroup itself; where fewer than
// RS_MIN_RUN outputs would fit (ratios below about 1 / 30) the samples are read from global memory instead.
#include "common.h"

#include <math.h>

// positions: the reference's separate IEEE operations (see above); sums use explicit fma()
#pragma clang fp contract(off)

constexpr int RS_RUN = 256;      // outputs per workgroup = threads
constexpr int RS_SPAN = 4096;    // staged input samples (16 KB of LDS)
constexpr int RS_MIN_RUN = 32;   // shorter staged runs would leave most of the workgroup idle: not staged then

__device__ __forceinline__ int rs_floor_pos(int t, double time_increment) { return (int)((double)t * time_increment); }

__global__ __launch_bounds__(RS_RUN) void resample_sinc_kernel(const float* x, float* y, const ctta_resample_clip* __restrict__ clips,
                                                               const float* __restrict__ win, int n_win, int num_table) {
  __shared__ float sx[RS_SPAN];
  const ctta_resample_clip c = clips[blockIdx.y];
  const int t_begin = blockIdx.x * RS_RUN;
  if (t_begin >= c.n_out) return;                             // a shorter clip of the batch (whole workgroup)
  const int t_end = min(t_begin + RS_RUN, c.n_out);
  const int tid = threadIdx.x;
  const int step = c.index_step;
  const int wing = n_win / step;                              // no wing has more taps: (n_win - offset) / step, offset >= 0
  const float* xc = x + c.x_off;
  // outputs per pass so that (run - 1) * time_increment + 2 * wing + 3 samples fit the staging buffer
  const double room = ((double)RS_SPAN - 2.0 * (double)wing - 3.0) / c.time_increment;
  const int run = room >= (double)(RS_RUN - 1) || room < (double)(RS_MIN_RUN - 1) ? RS_RUN : (int)room + 1;
  const double gain = (double)c.gain, ntab = (double)num_table;
  for (int t0 = t_begin; t0 < t_end; t0 += run) {
    const int t1 = min(t0 + run, t_end);
    const int lo = max(0, rs_floor_pos(t0, c.time_increment) - wing + 1);
    const int hi = min(c.n_in, rs_floor_pos(t1 - 1, c.time_increment) + wing + 1);
    const bool staged = hi - lo <= RS_SPAN;                   // uniform over the workgroup; false for a full run that has no room
    __syncthreads();                                          // the previous pass has finished reading sx
    if (staged)
      for (int i = tid; i < hi - lo; i += RS_RUN) sx[i] = xc[lo + i];
    __syncthreads();
    const int t = t0 + tid;
    if (t >= t1) continue;
    const double time_register = (double)t * c.time_increment;
    const int n = (int)time_register;
    double acc = 0.0;
    double frac = c.scale * (time_register - (double)n);
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const double index_frac = frac * ntab;
      const int offset = (int)index_frac;
      const double eta = index_frac - (double)offset;
      // left wing: x[n - i], i < n + 1; right wing: x[n + 1 + k], k < n_in - n - 1
      const int taps = max(0, min(side == 0 ? n + 1 : c.n_in - n - 1, (n_win - offset) / step));
      const int first = side == 0 ? n : n + 1, dir = side == 0 ? -1 : 1;
      if (staged) {
        const float* s = sx + (first - lo);
        for (int i = 0, j = offset; i < taps; ++i, j += step) {
          const double w0 = (double)win[j], w1 = (double)win[min(j + 1, n_win - 1)];   // delta[n_win - 1] = 0
          acc = fma(gain * (w0 + eta * (w1 - w0)), (double)s[dir * i], acc);
        }
      } else {
        const float* s = xc + first;
        for (int i = 0, j = offset; i < taps; ++i, j += step) {
          const double w0 = (double)win[j], w1 = (double)win[min(j + 1, n_win - 1)];
          acc = fma(gain * (w0 + eta * (w1 - w0)), (double)s[dir * i], acc);
        }
      }
      frac = c.scale - frac;
    }
    y[c.y_off + t] = (float)acc;
  }
}

extern "C" ctta_status ctta_resample_sinc(const float* x, float* y, const ctta_resample_clip* clips, int n_clips, int max_n_out,
                                          const float* win, int n_win, int num_table, void* stream) {
  CTTA_REQUIRE(x && y && clips && win, "resample_sinc: null pointer");
  CTTA_REQUIRE(n_clips >= 1 && n_clips <= 65535 && max_n_out >= 1, "resample_sinc: n_clips=%d (1..65535), max_n_out=%d", n_clips,
               max_n_out);
  CTTA_REQUIRE(num_table >= 1 && n_win > num_table, "resample_sinc: a table of %d entries at %d per zero crossing", n_win, num_table);
  hipLaunchKernelGGL(resample_sinc_kernel, dim3((unsigned)cdiv64(max_n_out, RS_RUN), n_clips), dim3(RS_RUN), 0, (hipStream_t)stream, x,
                     y, clips, win, n_win, num_table);
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}

constexpr int WP_THREADS = 1024;

// WP_THREADS partial results of a workgroup, combined as a fixed binary tree; valid in every thread after the call
template <bool MAX>
__device__ __forceinline__ double wp_block_reduce(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();                                            // red may still be read from the previous reduction
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = WP_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = MAX ? fmax(red[tid], red[tid + o]) : red[tid] + red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// One workgroup per clip, three sweeps over samples that the resampler has just left in L2: the fp64 sum (thread i adds
// samples i, i + 1024, ... in that order, then the tree), the two maxima of |y - mean| (whole clip, kept segment), the output.
__global__ __launch_bounds__(WP_THREADS) void wave_prepare_kernel(const float* __restrict__ y, const ctta_resample_clip* __restrict__ clips,
                                                                  int segment, float* __restrict__ out, double* __restrict__ ws) {
  __shared__ double red[WP_THREADS];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = clips[p].n_out, keep = min(n, segment);
  const float* yc = y + clips[p].y_off;
  float* oc = out + (size_t)p * segment;
  double acc = 0.0;
  for (int i = tid; i < n; i += WP_THREADS) acc += (double)yc[i];
  const double mean = wp_block_reduce<false>(acc, red) / (double)n;
  double m_all = 0.0, m_keep = 0.0;
  for (int i = tid; i < n; i += WP_THREADS) {
    const double a = fabs((double)yc[i] - mean);
    m_all = fmax(m_all, a);
    if (i < keep) m_keep = fmax(m_keep, a);
  }
  const double peak = wp_block_reduce<true>(m_all, red);
  // wav / (max|wav| + 1e-8) / 2 is monotone in |wav|: the peak of the kept segment is the scaled peak of its |y - mean|
  const double peak_keep = wp_block_reduce<true>(m_keep, red) / (peak + 1e-8) / 2.0;
  for (int i = tid; i < segment; i += WP_THREADS)
    oc[i] = i < keep ? (float)((((double)yc[i] - mean) / (peak + 1e-8) / 2.0) / (peak_keep + 1e-8) / 2.0) : 0.0f;
  if (tid == 0) {
    ws[3 * p] = mean;
    ws[3 * p + 1] = peak;
    ws[3 * p + 2] = peak_keep;
  }
}

extern "C" ctta_status ctta_wave_prepare(const float* y, const ctta_resample_clip* clips, int n_clips, int segment, float* out,
                                         double* ws, void* stream) {
  CTTA_REQUIRE(y && clips && out && ws, "wave_prepare: null pointer");
  CTTA_REQUIRE(n_clips >= 1 && segment >= 1, "wave_prepare: n_clips=%d, segment=%d", n_clips, segment);
  hipLaunchKernelGGL(wave_prepare_kernel, dim3(n_clips), dim3(WP_THREADS), 0, (hipStream_t)stream, y, clips, segment, out, ws);
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}
