// Seeded sampler noise: Philox4x32-10 keyed per request, addressed by (sample, draw, latent element), so a request's
// draws do not depend on its row, on the batch size or on what was drawn before (include/ctta.h).
// ALU-bound: one thread makes one Philox block (ten rounds of two 32x32->64 multiplies) = four consecutive w, and stores
// it as one 16-byte vector.  No fast-math intrinsic anywhere: logf, sqrtf and sincospif are the library's precise forms.
#include "common.h"

#include <math.h>
#include <stdint.h>

static int grid_for(long long total_vec) {
  long long b = (total_vec + 255) / 256;
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return (int)b;
}

// Philox4x32-10 as published (Salmon et al., SC'11): counter c[4], key (k0, k1); the key is bumped by the Weyl constants
// between rounds.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                               uint32_t k1, uint32_t x[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// u(x) = ((x >> 9) + 0.5) * 2^-23: 23 bits plus a half, exact in fp32, strictly inside (0, 1)
__device__ __forceinline__ float unit_open(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// Box-Muller on one pair of words: radius from xa, angle 2 pi u(xb) through sincospif(2 u) -- 2 u is exact, so the angle
// carries no argument rounding
__device__ __forceinline__ void normal_pair(uint32_t xa, uint32_t xb, float& za, float& zb) {
  const float r = sqrtf(-2.0f * logf(unit_open(xa)));
  float s, c;
  sincospif(2.0f * unit_open(xb), &s, &c);
  za = r * c;
  zb = r * s;
}

// out (draws, batch, C, H, W) as vectors of four w.  The Philox block index is q >> 2 with q = (h * C + c) * W + w: rows
// are the OUTER index of the stream, so a latent of H rows draws the first H rows of a taller one's.
template <bool NORMAL>
__global__ void philox_fill_kernel(const int64_t* __restrict__ seeds, const int32_t* __restrict__ samples, int batch,
                                   unsigned draw0, int channels, int height, int wv, float scale, uint4* __restrict__ out,
                                   long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long t = i;
    const int w4 = (int)(t % wv); t /= wv;
    const int h = (int)(t % height); t /= height;
    const int c = (int)(t % channels); t /= channels;
    const int b = (int)(t % batch);
    const unsigned d = draw0 + (unsigned)(t / batch);
    const unsigned long long seed = (unsigned long long)seeds[b];
    const unsigned m = samples ? (unsigned)samples[b] : 0u;
    const uint32_t block = (uint32_t)(((unsigned long long)h * channels + c) * wv + w4);      // < 2^32: C*H*W < 2^34
    uint32_t x[4];
    philox4x32_10(block, d, m, 0u /* domain tag: sampler noise */, (uint32_t)seed, (uint32_t)(seed >> 32), x);
    if (NORMAL) {
      float z0, z1, z2, z3;
      normal_pair(x[0], x[1], z0, z1);
      normal_pair(x[2], x[3], z2, z3);
      z0 = scale * z0; z1 = scale * z1; z2 = scale * z2; z3 = scale * z3;                     // a rounding of its own
      out[i] = make_uint4(__float_as_uint(z0), __float_as_uint(z1), __float_as_uint(z2), __float_as_uint(z3));
    } else {
      out[i] = make_uint4(x[0], x[1], x[2], x[3]);
    }
  }
}

template <bool NORMAL>
static ctta_status philox_fill(const char* who, const int64_t* seeds, const int32_t* samples, int batch, int draw0,
                               int draws, int channels, int height, int width, float scale, void* out, void* stream) {
  CTTA_REQUIRE(seeds && out, "%s: seeds and out are both required", who);
  CTTA_REQUIRE(batch > 0 && draws > 0 && channels > 0 && height > 0 && width > 0,
               "%s: empty tensor (batch=%d draws=%d C=%d H=%d W=%d)", who, batch, draws, channels, height, width);
  CTTA_REQUIRE(draw0 >= 0, "%s: draw0=%d is negative", who, draw0);
  CTTA_REQUIRE(width % 4 == 0, "%s: width=%d must be a multiple of 4 (one Philox block serves four w)", who, width);
  CTTA_REQUIRE((long long)channels * height <= ((1ll << 34) - 1) / width,      // int * int cannot overflow 64 bits
               "%s: C*H*W = %d*%d*%d needs more than 32 bits of block index (limit 2^34 elements)", who, channels, height, width);
  const long long per = (long long)channels * height * width;
  const long long rows = (long long)draws * batch;                  // < 2^62
  CTTA_REQUIRE(rows <= (1ll << 62) / per, "%s: output of %lld latents is too large", who, rows);
  const long long total = rows * (per / 4);
  hipLaunchKernelGGL((philox_fill_kernel<NORMAL>), dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, seeds, samples,
                     batch, (unsigned)draw0, channels, height, width / 4, scale, (uint4*)out, total);
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}

extern "C" ctta_status ctta_philox_normal(const int64_t* seeds, const int32_t* samples, int batch, int draw0, int draws,
                                          int channels, int height, int width, float scale, float* out, void* stream) {
  return philox_fill<true>("philox_normal", seeds, samples, batch, draw0, draws, channels, height, width, scale, out, stream);
}

extern "C" ctta_status ctta_philox_words(const int64_t* seeds, const int32_t* samples, int batch, int draw0, int draws,
                                         int channels, int height, int width, int32_t* out, void* stream) {
  return philox_fill<false>("philox_words", seeds, samples, batch, draw0, draws, channels, height, width, 1.0f, out, stream);
}
