// Mix augmentation of the training batch: tools/torch_tools.py:98-123 (augment) over tools/mix.py:4-51 (a_weight,
// compute_gain, mix), as called by the train split's collate (tools/t2a_dataset.py:51-69).
//
// Three launches, no atomics, no host synchronisation (capturable in a hipGraph), bit-deterministic:
//   1. mix_frame_energy_kernel -- one workgroup per (clip, frame): periodic-Hann window, n_fft-point complex radix-2 FFT
//      in LDS (fp32, twiddles from a float64 host table), E = sum_k A_k |X_k|^2 for k <= n_fft/2 (or mean(x^2) in RMSE
//      mode), gain = 10 log10(max(E, 10^(min_db/10))) in float64.  The energy is summed from the spectrum, not as the
//      quadratic form x^T Q x: with A_0 = 1e-8 at DC that form cancels catastrophically in fp32 for bass-heavy clips.
//   2. mix_pairs_kernel -- one workgroup per (pair, chunk of samples): the pair's clip indices come from a DEVICE int32
//      array (new pairs can be copied into a captured graph), each workgroup reduces both clips' frame gains to their
//      maxima, forms t and 1/sqrt(t^2 + (1-t)^2) in float64, writes its chunk of the unnormalised mixture and its max |.|.
//   3. mix_normalise_kernel -- one workgroup per (pair, chunk): max of the partials of the pair's group, (x / m) / 2.
//      Pairs are split into n_groups equal consecutive groups, each normalised on its own (one collate per group).
#include "common.h"

#include <math.h>

#include <vector>

namespace {

constexpr int kMixThreads = 256;
constexpr int kMixChunk = 4096;   // samples per workgroup in the pair / normalise kernels

struct MixTables {
  std::vector<float> window, aw;
  std::vector<float2> tw;
};

__device__ __forceinline__ float max_nan(float a, float b) {   // torch.max / np.max: a NaN anywhere is the result
  return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b);
}

// block-wide reductions over 256 threads; every thread gets the result
__device__ __forceinline__ float block_sum(float v, float* red) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float block_max(float v, float* red) {
  for (int o = 32; o >= 1; o >>= 1) v = max_nan(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return max_nan(max_nan(red[0], red[1]), max_nan(red[2], red[3]));
}

}  // namespace

struct ctta_mixer {
  int fs = 0, mode = 0, n_fft = 0, log2n = 0, stride = 0;
  float min_db = 0.f;
  double floor_e = 0.0;
  int max_clips = 0, max_samples = 0, max_pairs = 0, max_frames = 0, max_chunks = 0;
  float* window = nullptr;    // [n_fft] periodic Hann
  float2* tw = nullptr;       // [n_fft/2] exp(-2 pi i k / n_fft)
  float* aw = nullptr;        // [n_fft/2 + 1] 10^(a_weight_dB / 10)
  float* gain = nullptr;      // [max_clips][max_frames] per-frame gains (dB) of the last ctta_mixer_mix
  float* partial = nullptr;   // [max_pairs][max_chunks] max |mixture| per chunk
};

// ---------------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(kMixThreads) void mix_frame_energy_kernel(
    const float* __restrict__ wav, int64_t ld, int n_fft, int log2n, int stride, int rmse, const float* __restrict__ window,
    const float2* __restrict__ tw, const float* __restrict__ aw, double floor_e, float* __restrict__ gain_db, int gain_ld) {
  extern __shared__ float2 buf[];   // [n_fft]
  __shared__ float red[4];
  const int f = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const float* x = wav + (size_t)c * ld + (size_t)f * stride;
  float acc = 0.f;
  if (rmse) {
    for (int n = tid; n < n_fft; n += kMixThreads) acc += x[n] * x[n];
  } else {
    // windowed frame into bit-reversed order, then in-place decimation-in-time butterflies
    for (int n = tid; n < n_fft; n += kMixThreads)
      buf[__brev((unsigned)n) >> (32 - log2n)] = make_float2(window[n] * x[n], 0.f);
    __syncthreads();
    const int half = n_fft >> 1;
    for (int s = 0; s < log2n; ++s) {
      const int m = 1 << s;
      for (int j = tid; j < half; j += kMixThreads) {
        const int pos = j & (m - 1);
        const int i0 = ((j >> s) << (s + 1)) + pos, i1 = i0 + m;
        const float2 w = tw[pos << (log2n - 1 - s)];
        const float2 a = buf[i0], b = buf[i1];
        const float br = w.x * b.x - w.y * b.y, bi = w.x * b.y + w.y * b.x;
        buf[i0] = make_float2(a.x + br, a.y + bi);
        buf[i1] = make_float2(a.x - br, a.y - bi);
      }
      __syncthreads();
    }
    for (int k = tid; k <= half; k += kMixThreads) {
      const float2 X = buf[k];
      acc += aw[k] * (X.x * X.x + X.y * X.y);
    }
  }
  const float e = block_sum(acc, red);
  if (tid == 0) {
    double E = rmse ? (double)e / n_fft : (double)e;
    if (E == E) E = fmax(E, floor_e);   // np.maximum keeps a NaN
    gain_db[(size_t)c * gain_ld + f] = (float)(10.0 * log10(E));
  }
}

__global__ __launch_bounds__(kMixThreads) void mix_pairs_kernel(
    const float* __restrict__ wav, int64_t ld, int n_clips, int n_samples, const int* __restrict__ pairs,
    const float* __restrict__ gain_db, int gain_ld, int n_frames, double r, float* __restrict__ dst, int64_t dst_ld,
    int dst_row0, float* __restrict__ partial, int n_chunks, float* __restrict__ t_out, float* __restrict__ g_out) {
  __shared__ float red[4];
  const int c = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
  const int i = pairs[2 * p], j = pairs[2 * p + 1];
  // an index outside the batch (a bad device pair array) yields a NaN row instead of an out-of-bounds read
  const bool ok = i >= 0 && i < n_clips && j >= 0 && j < n_clips;
  float g1 = -INFINITY, g2 = -INFINITY;
  if (ok)
    for (int f = tid; f < n_frames; f += kMixThreads) {
      g1 = max_nan(g1, gain_db[(size_t)i * gain_ld + f]);
      g2 = max_nan(g2, gain_db[(size_t)j * gain_ld + f]);
    }
  g1 = block_max(g1, red);
  g2 = block_max(g2, red);
  const double t = 1.0 / (1.0 + pow(10.0, ((double)g1 - (double)g2) / 20.0) * (1.0 - r) / r);
  const double den = sqrt(t * t + (1.0 - t) * (1.0 - t));
  const float a = ok ? (float)(t / den) : __builtin_nanf(""), b = ok ? (float)((1.0 - t) / den) : __builtin_nanf("");
  const float* s1 = wav + (size_t)(ok ? i : 0) * ld;
  const float* s2 = wav + (size_t)(ok ? j : 0) * ld;
  float* out = dst + (size_t)(dst_row0 + p) * dst_ld;
  const int lo = c * kMixChunk, hi = min(lo + kMixChunk, n_samples);
  float m = 0.f;
  for (int n = lo + tid; n < hi; n += kMixThreads) {
    const float y = s1[n] * a + s2[n] * b;
    out[n] = y;
    m = max_nan(m, fabsf(y));
  }
  m = block_max(m, red);
  if (tid == 0) {
    partial[(size_t)p * n_chunks + c] = m;
    if (c == 0 && t_out) t_out[p] = ok ? (float)t : __builtin_nanf("");
    if (c == 0 && g_out) {
      g_out[2 * p] = g1;
      g_out[2 * p + 1] = g2;
    }
  }
}

__global__ __launch_bounds__(kMixThreads) void mix_normalise_kernel(float* __restrict__ dst, int64_t dst_ld, int dst_row0,
                                                                    int n_samples, const float* __restrict__ partial,
                                                                    int n_chunks, int pairs_per_group) {
  __shared__ float red[4];
  const int c = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
  const int g = p / pairs_per_group;
  const float* pp = partial + (size_t)g * pairs_per_group * n_chunks;
  float m = 0.f;
  for (int q = tid; q < pairs_per_group * n_chunks; q += kMixThreads) m = max_nan(m, pp[q]);
  m = block_max(m, red);
  float* out = dst + (size_t)(dst_row0 + p) * dst_ld;
  const int lo = c * kMixChunk, hi = min(lo + kMixChunk, n_samples);
  for (int n = lo + tid; n < hi; n += kMixThreads) out[n] = out[n] / m * 0.5f;   // all-silent group: 0 / 0 = NaN
}

// ---------------------------------------------------------------------------------------------------- host
static MixTables mix_tables(int fs, int n_fft, float min_db) {
  MixTables T;
  const int half = n_fft / 2;
  T.window.resize(n_fft);
  T.tw.resize(half);
  T.aw.resize(half + 1);
  for (int n = 0; n < n_fft; ++n) T.window[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * n / n_fft));   // np.hanning(N + 1)[:-1]
  for (int k = 0; k < half; ++k) {
    const double ang = 2.0 * M_PI * k / n_fft;
    T.tw[k] = make_float2((float)cos(ang), (float)-sin(ang));
  }
  // mix.py:4-15: the A-weighting curve (dB) on linspace(0, fs // 2, n_fft / 2 + 1), f^2 := 1 at DC, clamped at min_db
  const double step = (double)(fs / 2) / half;
  for (int k = 0; k <= half; ++k) {
    const double f = k == half ? (double)(fs / 2) : k * step;
    const double f2 = k == 0 ? 1.0 : f * f;
    double w = 2.0 + 20.0 * (2 * log10(12194.0) + 2 * log10(f2) - log10(f2 + 12194.0 * 12194.0) - log10(f2 + 20.6 * 20.6) -
                             0.5 * log10(f2 + 107.7 * 107.7) - 0.5 * log10(f2 + 737.9 * 737.9));
    w = fmax(w, (double)min_db);
    T.aw[k] = (float)pow(10.0, w / 10.0);
  }
  return T;
}

static int mix_frames(const ctta_mixer* M, int n_samples) {
  return n_samples < M->n_fft ? 0 : (n_samples - M->n_fft) / M->stride + 1;
}

extern "C" void ctta_mixer_destroy(ctta_mixer* M) {
  if (!M) return;
  for (void* p : {(void*)M->window, (void*)M->tw, (void*)M->aw, (void*)M->gain, (void*)M->partial})
    if (p) (void)hipFree(p);
  delete M;
}

extern "C" ctta_status ctta_mixer_create(int fs, int mode, float min_db, int max_clips, int max_samples, int max_pairs,
                                         ctta_mixer** out) {
  CTTA_REQUIRE(out, "mixer_create: null out");
  CTTA_REQUIRE(fs == 16000 || fs == 44100, "mixer_create: invalid fs %d (16000 or 44100)", fs);
  CTTA_REQUIRE(mode == 0 || mode == 1, "mixer_create: invalid mode %d (0 = A-weighting, 1 = RMSE)", mode);
  CTTA_REQUIRE(isfinite(min_db), "mixer_create: min_db must be finite");
  const int n_fft = fs == 16000 ? 2048 : 4096;
  CTTA_REQUIRE(max_clips >= 1 && max_pairs >= 1 && max_samples >= n_fft,
               "mixer_create: max_clips %d / max_pairs %d must be >= 1 and max_samples %d >= n_fft %d", max_clips,
               max_pairs, max_samples, n_fft);
  ctta_mixer* M = new ctta_mixer();
  M->fs = fs; M->mode = mode; M->min_db = min_db; M->n_fft = n_fft; M->stride = n_fft / 2;
  M->log2n = fs == 16000 ? 11 : 12;
  M->floor_e = pow(10.0, (double)min_db / 10.0);
  M->max_clips = max_clips; M->max_samples = max_samples; M->max_pairs = max_pairs;
  M->max_frames = mix_frames(M, max_samples);
  M->max_chunks = (max_samples + kMixChunk - 1) / kMixChunk;
  const MixTables T = mix_tables(fs, n_fft, min_db);
  bool ok = hipMalloc((void**)&M->window, T.window.size() * 4) == hipSuccess &&
            hipMalloc((void**)&M->tw, T.tw.size() * sizeof(float2)) == hipSuccess &&
            hipMalloc((void**)&M->aw, T.aw.size() * 4) == hipSuccess &&
            hipMalloc((void**)&M->gain, (size_t)max_clips * M->max_frames * 4) == hipSuccess &&
            hipMalloc((void**)&M->partial, (size_t)max_pairs * M->max_chunks * 4) == hipSuccess;
  if (ok)
    ok = hipMemcpy(M->window, T.window.data(), T.window.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(M->tw, T.tw.data(), T.tw.size() * sizeof(float2), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(M->aw, T.aw.data(), T.aw.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    ctta_set_error("mixer_create: device allocation / upload failed");
    ctta_mixer_destroy(M);
    return CTTA_ERR_NOMEM;
  }
  *out = M;
  return CTTA_OK;
}

extern "C" int ctta_mixer_frames(const ctta_mixer* M, int n_samples) { return M ? mix_frames(M, n_samples) : 0; }

static ctta_status mix_energy(ctta_mixer* M, const float* wav, int n_clips, int n_samples, int64_t ld, float* gain_db,
                              int gain_ld, hipStream_t s) {
  const int frames = mix_frames(M, n_samples);
  const size_t lds = M->mode == 1 ? 0 : (size_t)M->n_fft * sizeof(float2);
  hipLaunchKernelGGL(mix_frame_energy_kernel, dim3(frames, n_clips), dim3(kMixThreads), lds, s, wav, ld, M->n_fft, M->log2n,
                     M->stride, M->mode, M->window, M->tw, M->aw, M->floor_e, gain_db, gain_ld);
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}

extern "C" ctta_status ctta_mixer_gain_db(ctta_mixer* M, const float* wav, int n_clips, int n_samples, int64_t ld,
                                          float* gain_db, void* stream) {
  CTTA_REQUIRE(M && wav && gain_db, "mixer_gain_db: null pointer");
  CTTA_REQUIRE(n_clips >= 1 && n_samples >= M->n_fft && ld >= n_samples,
               "mixer_gain_db: %d clips of %d samples (ld %lld): need >= 1 clip of >= n_fft %d samples", n_clips,
               n_samples, (long long)ld, M->n_fft);
  return mix_energy(M, wav, n_clips, n_samples, ld, gain_db, mix_frames(M, n_samples), (hipStream_t)stream);
}

extern "C" ctta_status ctta_mixer_mix(ctta_mixer* M, const float* wav, int n_clips, int n_samples, int64_t ld,
                                      const int32_t* pairs, int n_pairs, int n_groups, double r, float* dst, int64_t dst_ld,
                                      int dst_row0, float* t_out, float* g_out, void* stream) {
  CTTA_REQUIRE(M && wav && pairs && dst, "mixer_mix: null pointer");
  CTTA_REQUIRE(n_clips >= 1 && n_clips <= M->max_clips && n_samples >= M->n_fft && n_samples <= M->max_samples &&
                   ld >= n_samples && dst_ld >= n_samples,
               "mixer_mix: %d clips of %d samples (ld %lld, dst_ld %lld) outside the handle's limits (%d clips, %d..%d samples)",
               n_clips, n_samples, (long long)ld, (long long)dst_ld, M->max_clips, M->n_fft, M->max_samples);
  CTTA_REQUIRE(n_pairs >= 1 && n_pairs <= M->max_pairs && dst_row0 >= 0,
               "mixer_mix: %d pairs (handle limit %d), dst_row0 %d", n_pairs, M->max_pairs, dst_row0);
  CTTA_REQUIRE(n_groups >= 0 && (n_groups == 0 || n_pairs % n_groups == 0),
               "mixer_mix: %d pairs do not split into %d equal groups", n_pairs, n_groups);
  CTTA_REQUIRE(r > 0.0 && r <= 1.0, "mixer_mix: r %g outside (0, 1]", r);
  hipStream_t s = (hipStream_t)stream;
  const int frames = mix_frames(M, n_samples), chunks = (n_samples + kMixChunk - 1) / kMixChunk;
  CTTA_TRY(mix_energy(M, wav, n_clips, n_samples, ld, M->gain, M->max_frames, s));
  hipLaunchKernelGGL(mix_pairs_kernel, dim3(chunks, n_pairs), dim3(kMixThreads), 0, s, wav, ld, n_clips, n_samples, pairs,
                     M->gain, M->max_frames, frames, r, dst, dst_ld, dst_row0, M->partial, chunks, t_out, g_out);
  CTTA_LAUNCH_CHECK();
  if (n_groups > 0) {
    hipLaunchKernelGGL(mix_normalise_kernel, dim3(chunks, n_pairs), dim3(kMixThreads), 0, s, dst, dst_ld, dst_row0, n_samples,
                       M->partial, chunks, n_pairs / n_groups);
    CTTA_LAUNCH_CHECK();
  }
  return CTTA_OK;
}
