// LoRA adapter operators of the attention projections (diffusers LoRAAttnProcessor, attention_processor.py:508-613):
//   y = W x + scale * up(down(x)),  down: Linear(in, r, bias=False), up: Linear(r, out, bias=False), rank r in [1, 16].
// The base product W x stays the conv_gemm launch it is; these kernels add the rank-r term beside it, forward and backward:
//   ctta_lora_down     D[M][r] (fp32)  = X[M][K] (bf16) * A^T         forward D = X A^T, backward dD = dY B
//   ctta_lora_up_add   Y[M][N] (bf16) += scale * D * B^T               forward Y += D B^T, backward dX += dD A
//   ctta_lora_up_add_t the same into a transposed result V^T[b][n][token] (how the engines keep attention values)
//   ctta_lora_down_rows / _up_add_rows / _up_add_t_rows   the three forward operators with one adapter PER SAMPLE, from a bank
//   ctta_lora_wgrad    G (fp32)       += scale * sum_m D[m][j] X[m][k]  dA = dD^T X, dB = dY^T D
//   ctta_lora_sites_fwd / _bwd         the same for one to three sites on ONE input at rank <= 4 (end of this file)
// All are skinny and memory bound (r << K): no matrix pipe, bf16 rows move as 16-byte vectors, sums are fp32.  No float
// atomics anywhere: a row's dot products are folded across lanes in a fixed order, sums over rows go through per-slab
// partial sums that a second launch folds in slab order, so gradients are bit-reproducible.
//
// Adapter matrices are fp32 and come in either orientation (a flag), so one packed copy of A and one of B serve the
// forward and the backward pass: [r][K] / [K][r] for the down operand, [N][r] / [r][N] for the up operand.
//
// PADDED COLUMNS.  The engines keep activations in padded layouts (width rounded up to 64, heads padded from dh to 64
// lanes).  The contract here: the kernels read EVERY column they are given, and the PACKED ADAPTER holds zeros in every
// padded row and column; the activations' padded columns must be finite (the engines write exact zeros there: they are
// products with zero weight rows), so they contribute exactly 0.  ctta_lora_wgrad drops padded columns through its
// column map instead (they have no place in the gradient tensor).
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------- down
// LPR lanes share one row; each takes 8 columns per pass.  KMAJOR: a[k][r], else a[r][k].
template <int RMAX, int LPR, bool KMAJOR>
__global__ __launch_bounds__(256) void lora_down_kernel(const bf16_t* __restrict__ x, int ldx, int64_t M, int K,
                                                        const float* __restrict__ a, int r, float* __restrict__ d) {
  const int lr = threadIdx.x % LPR;
  const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  float acc[RMAX];
#pragma unroll
  for (int j = 0; j < RMAX; ++j) acc[j] = 0.f;
  if (row < M) {
    const bf16_t* xr = x + row * ldx;
    for (int k0 = lr * 8; k0 < K; k0 += LPR * 8) {
      float f[8];
      unpack8(*reinterpret_cast<const uint4*>(xr + k0), f);
#pragma unroll
      for (int j = 0; j < RMAX; ++j) {
        if (j < r) {
          if constexpr (KMAJOR) {
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[j] = fmaf(f[i], a[(size_t)(k0 + i) * r + j], acc[j]);
          } else {
            const float4 w0 = *reinterpret_cast<const float4*>(a + (size_t)j * K + k0);
            const float4 w1 = *reinterpret_cast<const float4*>(a + (size_t)j * K + k0 + 4);
            acc[j] = fmaf(f[0], w0.x, acc[j]); acc[j] = fmaf(f[1], w0.y, acc[j]);
            acc[j] = fmaf(f[2], w0.z, acc[j]); acc[j] = fmaf(f[3], w0.w, acc[j]);
            acc[j] = fmaf(f[4], w1.x, acc[j]); acc[j] = fmaf(f[5], w1.y, acc[j]);
            acc[j] = fmaf(f[6], w1.z, acc[j]); acc[j] = fmaf(f[7], w1.w, acc[j]);
          }
        }
      }
    }
  }
  // every lane of the wave takes part in the fold (rows past M carry zeros)
#pragma unroll
  for (int j = 0; j < RMAX; ++j)
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
  if (row < M && lr == 0) {
#pragma unroll
    for (int j = 0; j < RMAX; ++j)
      if (j < r) d[row * r + j] = acc[j];
  }
}

// ---------------------------------------------------------------------------------------------- up_add
// A block is 32 column threads (8 output columns each) by 8 row lanes and walks UP_ROWS rows: a thread keeps its
// [8][r] slice of b in registers for all of its rows, so a row costs one 16-byte load, r broadcast loads of d and one
// 16-byte store.  RMAJOR: b[r][N], else b[N][r].  A thread whose eight sums are all zero stores nothing, so zero adapters
// leave Y bit for bit as it was.
constexpr int UP_ROWS = 64;
template <int RMAX, bool RMAJOR>
__global__ __launch_bounds__(256) void lora_up_add_kernel(bf16_t* __restrict__ y, int ldy, int64_t M, int N,
                                                          const float* __restrict__ d, const float* __restrict__ b,
                                                          int r, float scale) {
  const int c8 = (blockIdx.y * 32 + threadIdx.x % 32) * 8;
  if (c8 >= N) return;
  float bw[RMAX][8];
#pragma unroll
  for (int j = 0; j < RMAX; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i)
      bw[j][i] = j < r ? (RMAJOR ? b[(size_t)j * N + c8 + i] : b[(size_t)(c8 + i) * r + j]) * scale : 0.f;
  const int64_t m0 = (int64_t)blockIdx.x * UP_ROWS;
  const int64_t m1 = m0 + UP_ROWS < M ? m0 + UP_ROWS : M;
  for (int64_t row = m0 + threadIdx.x / 32; row < m1; row += 8) {
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
    for (int j = 0; j < RMAX; ++j) {
      if (j < r) {
        const float dv = d[row * r + j];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(dv, bw[j][i], acc[i]);
      }
    }
    bool any = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) any = any || acc[i] != 0.f;
    if (!any) continue;
    uint4* p = reinterpret_cast<uint4*>(y + row * ldy + c8);
    float f[8];
    unpack8(*p, f);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] += acc[i];
    *p = pack8(f);
  }
}

// yt[bb][n][tok] += scale * sum_j d[(bb * d_tokens + tok) * r + j] * b[n][j]; VEC: 8 tokens per thread
template <int RMAX, bool VEC>
__global__ __launch_bounds__(256) void lora_up_add_t_kernel(bf16_t* __restrict__ yt, int ldt, int64_t batch_stride, int batch,
                                                            int tokens, int N, const float* __restrict__ d, int d_tokens,
                                                            const float* __restrict__ b, int r, float scale) {
  constexpr int W = VEC ? 8 : 1;
  const int tc = tokens / W;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)batch * N * tc) return;
  const int t0 = (int)(idx % tc) * W;
  const int n = (int)((idx / tc) % N);
  const int bb = (int)(idx / ((int64_t)tc * N));
  const float* dr = d + ((size_t)bb * d_tokens + t0) * r;
  float acc[W];
#pragma unroll
  for (int i = 0; i < W; ++i) acc[i] = 0.f;
#pragma unroll
  for (int j = 0; j < RMAX; ++j) {
    if (j < r) {
      const float bv = b[(size_t)n * r + j] * scale;
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] = fmaf(dr[(size_t)i * r + j], bv, acc[i]);
    }
  }
  bf16_t* p = yt + (size_t)bb * batch_stride + (size_t)n * ldt + t0;
  if constexpr (VEC) {
    bool any = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) any = any || acc[i] != 0.f;
    if (!any) return;
    float f[8];
    unpack8(*reinterpret_cast<uint4*>(p), f);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] += acc[i];
    *reinterpret_cast<uint4*>(p) = pack8(f);
  } else {
    if (acc[0] != 0.f) *p = f2bf(bf2f(*p) + acc[0]);
  }
}

// ---------------------------------------------------------------------------------------------- per-sample adapters
// The three forward operators above with one adapter PER SAMPLE: `bank` holds n_slots packed matrices slot_stride floats
// apart, sample = row / rows_per_sample (the batch index of the transposed form) looks its slot up in a device array, and
// a slot outside [0, n_slots) is "no adapter": nothing of the bank is read, d gets zeros, y keeps its bits.  For a valid
// slot a row's arithmetic is that of the kernels above (same lanes per row, same chains, same fold, the same bw = b * scale),
// so the bits are those of a launch with that slot's matrix and scale.
__device__ __forceinline__ bool slot_valid(int slot, int n_slots) { return (unsigned)slot < (unsigned)n_slots; }

// A wave may hold rows of several samples: every row picks its own a; the fold stays inside the row's LPR lanes.
template <int RMAX, int LPR>
__global__ __launch_bounds__(256) void lora_down_rows_kernel(const bf16_t* __restrict__ x, int ldx, int64_t M, int K,
                                                             const float* __restrict__ bank, int64_t slot_stride, int n_slots,
                                                             int r, int64_t rps, const int32_t* __restrict__ slot_of_sample,
                                                             float* __restrict__ d) {
  const int lr = threadIdx.x % LPR;
  const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
  float acc[RMAX];
#pragma unroll
  for (int j = 0; j < RMAX; ++j) acc[j] = 0.f;
  if (row < M) {
    const int slot = slot_of_sample[row / rps];
    if (slot_valid(slot, n_slots)) {
      const float* __restrict__ a = bank + (size_t)slot * slot_stride;
      const bf16_t* xr = x + row * ldx;
      for (int k0 = lr * 8; k0 < K; k0 += LPR * 8) {
        float f[8];
        unpack8(*reinterpret_cast<const uint4*>(xr + k0), f);
#pragma unroll
        for (int j = 0; j < RMAX; ++j) {
          if (j < r) {
            const float4 w0 = *reinterpret_cast<const float4*>(a + (size_t)j * K + k0);
            const float4 w1 = *reinterpret_cast<const float4*>(a + (size_t)j * K + k0 + 4);
            acc[j] = fmaf(f[0], w0.x, acc[j]); acc[j] = fmaf(f[1], w0.y, acc[j]);
            acc[j] = fmaf(f[2], w0.z, acc[j]); acc[j] = fmaf(f[3], w0.w, acc[j]);
            acc[j] = fmaf(f[4], w1.x, acc[j]); acc[j] = fmaf(f[5], w1.y, acc[j]);
            acc[j] = fmaf(f[6], w1.z, acc[j]); acc[j] = fmaf(f[7], w1.w, acc[j]);
          }
        }
      }
    }
  }
  // every lane of the wave takes part in the fold (rows past M and rows without an adapter carry zeros)
#pragma unroll
  for (int j = 0; j < RMAX; ++j)
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
  if (row < M && lr == 0) {
#pragma unroll
    for (int j = 0; j < RMAX; ++j)
      if (j < r) d[row * r + j] = acc[j];
  }
}

// The grid is laid out per sample: blockIdx.x = sample * blocks_per_sample + block, so a block's UP_ROWS rows are one
// sample's and its [8][r] slice of that sample's b stays in registers as above.  B * ceil(rps / 64) slices are read in
// all, the fewest any layout reads (a slice per sample a block touches).  A block of a sample without an adapter returns.
template <int RMAX>
__global__ __launch_bounds__(256) void lora_up_add_rows_kernel(bf16_t* __restrict__ y, int ldy, int64_t M, int N,
                                                               const float* __restrict__ d, const float* __restrict__ bank,
                                                               int64_t slot_stride, int n_slots, int r, int64_t rps, int bps,
                                                               const int32_t* __restrict__ slot_of_sample,
                                                               const float* __restrict__ scale_of_sample, float scale) {
  const int c8 = (blockIdx.y * 32 + threadIdx.x % 32) * 8;
  if (c8 >= N) return;
  const int64_t sample = blockIdx.x / bps;
  const int slot = slot_of_sample[sample];
  if (!slot_valid(slot, n_slots)) return;
  if (scale_of_sample) scale = scale_of_sample[sample];
  const float* __restrict__ b = bank + (size_t)slot * slot_stride;
  float bw[RMAX][8];
#pragma unroll
  for (int j = 0; j < RMAX; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) bw[j][i] = j < r ? b[(size_t)(c8 + i) * r + j] * scale : 0.f;
  const int64_t s1 = (sample + 1) * rps < M ? (sample + 1) * rps : M;
  const int64_t m0 = sample * rps + (int64_t)(blockIdx.x % bps) * UP_ROWS;
  const int64_t m1 = m0 + UP_ROWS < s1 ? m0 + UP_ROWS : s1;
  for (int64_t row = m0 + threadIdx.x / 32; row < m1; row += 8) {
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
    for (int j = 0; j < RMAX; ++j) {
      if (j < r) {
        const float dv = d[row * r + j];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(dv, bw[j][i], acc[i]);
      }
    }
    bool any = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) any = any || acc[i] != 0.f;
    if (!any) continue;
    uint4* p = reinterpret_cast<uint4*>(y + row * ldy + c8);
    float f[8];
    unpack8(*p, f);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] += acc[i];
    *p = pack8(f);
  }
}

template <int RMAX, bool VEC>
__global__ __launch_bounds__(256) void lora_up_add_t_rows_kernel(bf16_t* __restrict__ yt, int ldt, int64_t batch_stride, int batch,
                                                                 int tokens, int N, const float* __restrict__ d, int d_tokens,
                                                                 const float* __restrict__ bank, int64_t slot_stride, int n_slots,
                                                                 int r, const int32_t* __restrict__ slot_of_sample,
                                                                 const float* __restrict__ scale_of_sample, float scale) {
  constexpr int W = VEC ? 8 : 1;
  const int tc = tokens / W;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)batch * N * tc) return;
  const int t0 = (int)(idx % tc) * W;
  const int n = (int)((idx / tc) % N);
  const int bb = (int)(idx / ((int64_t)tc * N));
  const int slot = slot_of_sample[bb];
  if (!slot_valid(slot, n_slots)) return;
  if (scale_of_sample) scale = scale_of_sample[bb];
  const float* __restrict__ b = bank + (size_t)slot * slot_stride;
  const float* dr = d + ((size_t)bb * d_tokens + t0) * r;
  float acc[W];
#pragma unroll
  for (int i = 0; i < W; ++i) acc[i] = 0.f;
#pragma unroll
  for (int j = 0; j < RMAX; ++j) {
    if (j < r) {
      const float bv = b[(size_t)n * r + j] * scale;
#pragma unroll
      for (int i = 0; i < W; ++i) acc[i] = fmaf(dr[(size_t)i * r + j], bv, acc[i]);
    }
  }
  bf16_t* p = yt + (size_t)bb * batch_stride + (size_t)n * ldt + t0;
  if constexpr (VEC) {
    bool any = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) any = any || acc[i] != 0.f;
    if (!any) return;
    float f[8];
    unpack8(*reinterpret_cast<uint4*>(p), f);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] += acc[i];
    *reinterpret_cast<uint4*>(p) = pack8(f);
  } else {
    if (acc[0] != 0.f) *p = f2bf(bf2f(*p) + acc[0]);
  }
}

// ---------------------------------------------------------------------------------------------- wgrad
// part[s][j][k] = sum over the rows of slab s of d[m][j] * x[m][k].  A block is CT column threads (8 columns each) by
// 256 / CT row groups; the row groups' sums meet in LDS and are added in row-group order.
template <int RMAX>
__global__ __launch_bounds__(256) void lora_wgrad_partial_kernel(const float* __restrict__ d, const bf16_t* __restrict__ x,
                                                                 int ldx, int64_t M, int K, int r, int ct, int64_t rows_per_slab,
                                                                 float* __restrict__ part) {
  __shared__ float red[256 * 8];
  const int tx = threadIdx.x % ct, rg = threadIdx.x / ct, n_rg = 256 / ct;
  const int k0 = (blockIdx.x * ct + tx) * 8;
  const bool active = k0 < K;
  const int64_t m0 = (int64_t)blockIdx.y * rows_per_slab;
  const int64_t m1 = m0 + rows_per_slab < M ? m0 + rows_per_slab : M;
  float acc[RMAX][8];
#pragma unroll
  for (int j = 0; j < RMAX; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[j][i] = 0.f;
  if (active) {
    for (int64_t m = m0 + rg; m < m1; m += n_rg) {
      float f[8];
      unpack8(*reinterpret_cast<const uint4*>(x + m * ldx + k0), f);
#pragma unroll
      for (int j = 0; j < RMAX; ++j) {
        if (j < r) {
          const float dv = d[m * r + j];
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[j][i] = fmaf(dv, f[i], acc[j][i]);
        }
      }
    }
  }
  float* dst = part + (size_t)blockIdx.y * r * K;
#pragma unroll
  for (int j = 0; j < RMAX; ++j) {
    if (j < r) {   // uniform across the block
#pragma unroll
      for (int i = 0; i < 8; ++i) red[(rg * ct + tx) * 8 + i] = acc[j][i];
      __syncthreads();
      if ((int)threadIdx.x < ct * 8) {
        const int k = blockIdx.x * ct * 8 + threadIdx.x;
        if (k < K) {
          float s = 0.f;
          for (int g = 0; g < n_rg; ++g) s += red[g * ct * 8 + threadIdx.x];
          dst[(size_t)j * K + k] = s;
        }
      }
      __syncthreads();
    }
  }
}

// g[j * gs_r + col(k) * gs_k] += scale * (part[0] + part[1] + ...)[j][k]; columns the map sends to -1 are dropped
__global__ __launch_bounds__(256) void lora_wgrad_fold_kernel(const float* __restrict__ part, int slabs, int K, int r, float scale,
                                                              float* __restrict__ g, int64_t gs_r, int64_t gs_k,
                                                              const int32_t* __restrict__ col_map) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= r * K) return;
  const int j = idx / K, k = idx % K;
  const int col = col_map ? col_map[k] : k;
  if (col < 0) return;
  float s = 0.f;
  for (int i = 0; i < slabs; ++i) s += part[(size_t)i * r * K + idx];
  g[j * gs_r + col * gs_k] += scale * s;
}

int wgrad_slabs(int64_t m) {
  const int64_t s = (m + 255) / 256;
  return (int)(s < 1 ? 1 : s > 512 ? 512 : s);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

#define LORA_RMAX_DISPATCH(r, CALL) \
  do {                              \
    if ((r) <= 4) { CALL(4); } else { CALL(16); } \
  } while (0)

extern "C" ctta_status ctta_lora_down(const void* x, int ldx, int64_t m, int k, const float* a, int a_kmajor, int r, float* d,
                                      void* stream) {
  CTTA_REQUIRE(x && a && d, "lora_down: null pointer");
  CTTA_REQUIRE(r >= 1 && r <= 16, "lora_down: rank %d outside [1,16]", r);
  CTTA_REQUIRE(m >= 0 && k >= 8 && k % 8 == 0 && ldx >= k && ldx % 8 == 0, "lora_down: m=%lld k=%d ldx=%d (k, ldx multiples of 8, ldx >= k)",
               (long long)m, k, ldx);
  CTTA_REQUIRE(aligned16(x) && aligned16(a), "lora_down: x and a must be 16-byte aligned");
  if (m == 0) return CTTA_OK;
  hipStream_t s = (hipStream_t)stream;
  const bf16_t* xp = (const bf16_t*)x;
#define LAUNCH_LPR(RM, LPR)                                                                                            \
  do {                                                                                                                 \
    const dim3 grid((unsigned)cdiv64(m, 256 / LPR));                                                                   \
    if (a_kmajor) hipLaunchKernelGGL((lora_down_kernel<RM, LPR, true>), grid, dim3(256), 0, s, xp, ldx, m, k, a, r, d); \
    else hipLaunchKernelGGL((lora_down_kernel<RM, LPR, false>), grid, dim3(256), 0, s, xp, ldx, m, k, a, r, d);         \
  } while (0)
#define CALL(RM)                             \
  do {                                       \
    if (k <= 64) LAUNCH_LPR(RM, 8);          \
    else if (k <= 128) LAUNCH_LPR(RM, 16);   \
    else if (k <= 256) LAUNCH_LPR(RM, 32);   \
    else LAUNCH_LPR(RM, 64);                 \
  } while (0)
  LORA_RMAX_DISPATCH(r, CALL);
#undef CALL
#undef LAUNCH_LPR
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}

extern "C" ctta_status ctta_lora_up_add(void* y, int ldy, int64_t m, int n, const float* d, const float* b, int b_rmajor, int r,
                                        float scale, void* stream) {
  CTTA_REQUIRE(y && d && b, "lora_up_add: null pointer");
  CTTA_REQUIRE(r >= 1 && r <= 16, "lora_up_add: rank %d outside [1,16]", r);
  CTTA_REQUIRE(m >= 0 && n >= 8 && n % 8 == 0 && ldy >= n && ldy % 8 == 0, "lora_up_add: m=%lld n=%d ldy=%d (n, ldy multiples of 8, ldy >= n)",
               (long long)m, n, ldy);
  CTTA_REQUIRE(aligned16(y), "lora_up_add: y must be 16-byte aligned");
  if (m == 0) return CTTA_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)cdiv64(m, UP_ROWS), (unsigned)((n / 8 + 31) / 32));
#define CALL(RM)                                                                                                                  \
  do {                                                                                                                            \
    if (b_rmajor) hipLaunchKernelGGL((lora_up_add_kernel<RM, true>), grid, dim3(256), 0, s, (bf16_t*)y, ldy, m, n, d, b, r, scale); \
    else hipLaunchKernelGGL((lora_up_add_kernel<RM, false>), grid, dim3(256), 0, s, (bf16_t*)y, ldy, m, n, d, b, r, scale);         \
  } while (0)
  LORA_RMAX_DISPATCH(r, CALL);
#undef CALL
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}

extern "C" ctta_status ctta_lora_up_add_t(void* yt, int ldt, int64_t batch_stride, int batch, int tokens, int n, const float* d,
                                          int d_tokens, const float* b, int r, float scale, void* stream) {
  CTTA_REQUIRE(yt && d && b, "lora_up_add_t: null pointer");
  CTTA_REQUIRE(r >= 1 && r <= 16, "lora_up_add_t: rank %d outside [1,16]", r);
  CTTA_REQUIRE(batch >= 0 && tokens >= 1 && n >= 1 && ldt >= tokens && d_tokens >= tokens && batch_stride >= (int64_t)n * ldt,
               "lora_up_add_t: batch=%d tokens=%d n=%d ldt=%d d_tokens=%d batch_stride=%lld", batch, tokens, n, ldt, d_tokens,
               (long long)batch_stride);
  if (batch == 0) return CTTA_OK;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = tokens % 8 == 0 && ldt % 8 == 0 && batch_stride % 8 == 0 && aligned16(yt);
  const dim3 grid((unsigned)cdiv64((int64_t)batch * n * (vec ? tokens / 8 : tokens), 256));
#define CALL(RM)                                                                                                              \
  do {                                                                                                                        \
    if (vec) hipLaunchKernelGGL((lora_up_add_t_kernel<RM, true>), grid, dim3(256), 0, s, (bf16_t*)yt, ldt, batch_stride, batch, \
                                tokens, n, d, d_tokens, b, r, scale);                                                         \
    else hipLaunchKernelGGL((lora_up_add_t_kernel<RM, false>), grid, dim3(256), 0, s, (bf16_t*)yt, ldt, batch_stride, batch,    \
                            tokens, n, d, d_tokens, b, r, scale);                                                             \
  } while (0)
  LORA_RMAX_DISPATCH(r, CALL);
#undef CALL
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}

// ---- per-sample adapters: the dispatch rules (lanes per row by k, RMAX by r, the vector path of the transposed form) are
// those of the three entry points above, so a row with a valid slot gets their bits
extern "C" ctta_status ctta_lora_down_rows(const void* x, int ldx, int64_t m, int k, const float* a_bank, int64_t slot_stride,
                                           int n_slots, int r, int64_t rows_per_sample, const int32_t* slot_of_sample, float* d,
                                           void* stream) {
  CTTA_REQUIRE(x && a_bank && d && slot_of_sample, "lora_down_rows: null pointer");
  CTTA_REQUIRE(r >= 1 && r <= 16, "lora_down_rows: rank %d outside [1,16]", r);
  CTTA_REQUIRE(m >= 0 && k >= 8 && k % 8 == 0 && ldx >= k && ldx % 8 == 0, "lora_down_rows: m=%lld k=%d ldx=%d (k, ldx multiples of 8, ldx >= k)",
               (long long)m, k, ldx);
  CTTA_REQUIRE(n_slots >= 1 && slot_stride >= (int64_t)r * k && slot_stride % 4 == 0 && rows_per_sample >= 1,
               "lora_down_rows: n_slots=%d slot_stride=%lld (a multiple of 4, at least r * k) rows_per_sample=%lld", n_slots,
               (long long)slot_stride, (long long)rows_per_sample);
  CTTA_REQUIRE(aligned16(x) && aligned16(a_bank), "lora_down_rows: x and a_bank must be 16-byte aligned");
  if (m == 0) return CTTA_OK;
  hipStream_t s = (hipStream_t)stream;
  const bf16_t* xp = (const bf16_t*)x;
#define LAUNCH_LPR(RM, LPR)                                                                                                \
  hipLaunchKernelGGL((lora_down_rows_kernel<RM, LPR>), dim3((unsigned)cdiv64(m, 256 / LPR)), dim3(256), 0, s, xp, ldx, m, k, \
                     a_bank, slot_stride, n_slots, r, rows_per_sample, slot_of_sample, d)
#define CALL(RM)                             \
  do {                                       \
    if (k <= 64) LAUNCH_LPR(RM, 8);          \
    else if (k <= 128) LAUNCH_LPR(RM, 16);   \
    else if (k <= 256) LAUNCH_LPR(RM, 32);   \
    else LAUNCH_LPR(RM, 64);                 \
  } while (0)
  LORA_RMAX_DISPATCH(r, CALL);
#undef CALL
#undef LAUNCH_LPR
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}

extern "C" ctta_status ctta_lora_up_add_rows(void* y, int ldy, int64_t m, int n, const float* d, const float* b_bank,
                                             int64_t slot_stride, int n_slots, int r, int64_t rows_per_sample,
                                             const int32_t* slot_of_sample, const float* scale_of_sample, float scale,
                                             void* stream) {
  CTTA_REQUIRE(y && d && b_bank && slot_of_sample, "lora_up_add_rows: null pointer");
  CTTA_REQUIRE(r >= 1 && r <= 16, "lora_up_add_rows: rank %d outside [1,16]", r);
  CTTA_REQUIRE(m >= 0 && n >= 8 && n % 8 == 0 && ldy >= n && ldy % 8 == 0, "lora_up_add_rows: m=%lld n=%d ldy=%d (n, ldy multiples of 8, ldy >= n)",
               (long long)m, n, ldy);
  CTTA_REQUIRE(n_slots >= 1 && slot_stride >= (int64_t)n * r && rows_per_sample >= 1,
               "lora_up_add_rows: n_slots=%d slot_stride=%lld (at least n * r) rows_per_sample=%lld", n_slots, (long long)slot_stride,
               (long long)rows_per_sample);
  CTTA_REQUIRE(aligned16(y), "lora_up_add_rows: y must be 16-byte aligned");
  if (m == 0) return CTTA_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t samples = cdiv64(m, rows_per_sample);
  const int64_t bps = cdiv64(rows_per_sample < m ? rows_per_sample : m, UP_ROWS);
  CTTA_REQUIRE(samples * bps <= 0x7fffffff, "lora_up_add_rows: %lld samples of %lld rows exceed the grid", (long long)samples,
               (long long)rows_per_sample);
  const dim3 grid((unsigned)(samples * bps), (unsigned)((n / 8 + 31) / 32));
#define CALL(RM)                                                                                                                 \
  hipLaunchKernelGGL((lora_up_add_rows_kernel<RM>), grid, dim3(256), 0, s, (bf16_t*)y, ldy, m, n, d, b_bank, slot_stride, n_slots, \
                     r, rows_per_sample, (int)bps, slot_of_sample, scale_of_sample, scale)
  LORA_RMAX_DISPATCH(r, CALL);
#undef CALL
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}

extern "C" ctta_status ctta_lora_up_add_t_rows(void* yt, int ldt, int64_t batch_stride, int batch, int tokens, int n,
                                               const float* d, int d_tokens, const float* b_bank, int64_t slot_stride, int n_slots,
                                               int r, const int32_t* slot_of_sample, const float* scale_of_sample, float scale,
                                               void* stream) {
  CTTA_REQUIRE(yt && d && b_bank && slot_of_sample, "lora_up_add_t_rows: null pointer");
  CTTA_REQUIRE(r >= 1 && r <= 16, "lora_up_add_t_rows: rank %d outside [1,16]", r);
  CTTA_REQUIRE(batch >= 0 && tokens >= 1 && n >= 1 && ldt >= tokens && d_tokens >= tokens && batch_stride >= (int64_t)n * ldt,
               "lora_up_add_t_rows: batch=%d tokens=%d n=%d ldt=%d d_tokens=%d batch_stride=%lld", batch, tokens, n, ldt, d_tokens,
               (long long)batch_stride);
  CTTA_REQUIRE(n_slots >= 1 && slot_stride >= (int64_t)n * r, "lora_up_add_t_rows: n_slots=%d slot_stride=%lld (at least n * r)",
               n_slots, (long long)slot_stride);
  if (batch == 0) return CTTA_OK;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = tokens % 8 == 0 && ldt % 8 == 0 && batch_stride % 8 == 0 && aligned16(yt);
  const dim3 grid((unsigned)cdiv64((int64_t)batch * n * (vec ? tokens / 8 : tokens), 256));
#define CALL(RM)                                                                                                                  \
  do {                                                                                                                            \
    if (vec) hipLaunchKernelGGL((lora_up_add_t_rows_kernel<RM, true>), grid, dim3(256), 0, s, (bf16_t*)yt, ldt, batch_stride, batch, \
                                tokens, n, d, d_tokens, b_bank, slot_stride, n_slots, r, slot_of_sample, scale_of_sample, scale);  \
    else hipLaunchKernelGGL((lora_up_add_t_rows_kernel<RM, false>), grid, dim3(256), 0, s, (bf16_t*)yt, ldt, batch_stride, batch,   \
                            tokens, n, d, d_tokens, b_bank, slot_stride, n_slots, r, slot_of_sample, scale_of_sample, scale);      \
  } while (0)
  LORA_RMAX_DISPATCH(r, CALL);
#undef CALL
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}

extern "C" size_t ctta_lora_wgrad_scratch_floats(int64_t m, int k, int r) {
  if (m < 1 || k < 8 || k % 8 || r < 1 || r > 16) return 0;
  return (size_t)wgrad_slabs(m) * r * k;
}

extern "C" ctta_status ctta_lora_wgrad(const float* d, const void* x, int ldx, int64_t m, int k, int r, float scale, float* g,
                                       int64_t g_stride_r, int64_t g_stride_k, const int32_t* col_map, float* scratch,
                                       void* stream) {
  CTTA_REQUIRE(d && x && g && scratch, "lora_wgrad: null pointer");
  CTTA_REQUIRE(r >= 1 && r <= 16, "lora_wgrad: rank %d outside [1,16]", r);
  CTTA_REQUIRE(m >= 0 && k >= 8 && k % 8 == 0 && ldx >= k && ldx % 8 == 0, "lora_wgrad: m=%lld k=%d ldx=%d (k, ldx multiples of 8, ldx >= k)",
               (long long)m, k, ldx);
  CTTA_REQUIRE(aligned16(x), "lora_wgrad: x must be 16-byte aligned");
  if (m == 0) return CTTA_OK;
  hipStream_t s = (hipStream_t)stream;
  const int slabs = wgrad_slabs(m);
  const int64_t rows_per_slab = cdiv64(m, slabs);
  const int ct = k <= 64 ? 8 : k <= 128 ? 16 : 32;
  const dim3 grid((unsigned)((k / 8 + ct - 1) / ct), (unsigned)slabs);
#define CALL(RM) \
  hipLaunchKernelGGL((lora_wgrad_partial_kernel<RM>), grid, dim3(256), 0, s, d, (const bf16_t*)x, ldx, m, k, r, ct, rows_per_slab, scratch)
  LORA_RMAX_DISPATCH(r, CALL);
#undef CALL
  CTTA_LAUNCH_CHECK();
  hipLaunchKernelGGL(lora_wgrad_fold_kernel, dim3((unsigned)((r * k + 255) / 256)), dim3(256), 0, s, scratch, slabs, k, r, scale, g,
                     g_stride_r, g_stride_k, col_map);
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}

// ================================================================================================== fused site kernels
// Rank <= 4, one to three sites on one input.  What the per-site launches above cost at the engines' shapes (profiles/
// lora_step.txt): a thousand small launches per training step, X read once per site, and a weight-gradient kernel whose
// 144 slabs of 256 rows leave CUs idle while each thread walks 32 dependent row loads.  Here a call walks X once for all
// its sites, slabs are sized so that 36864 rows give two workgroups per CU, and the r <= 4 accumulators stay in registers.
// The per-site VALUES are bit for bit those of the kernels above: the same lanes share a row (sites_lpr == the LPR
// ctta_lora_down picks), the folds and fmaf chains are the same.  Measured (same file, second section): the backward is
// 3.4x faster than its launches; the forward kernel is SLOWER than its own (it re-reads A and B through L1 for every row),
// so the engine takes it only on request (ctta_unet_set_lora bit 1).
namespace {

constexpr int SITES_MAX = 3;
constexpr int SITES_W_MAX = 1536;   // three passes of 64 lanes x 8 columns
constexpr int FWD_TILE = 64;        // rows between two barriers of the transposed destination

struct FwdSites { ctta_lora_fwd_site s[SITES_MAX]; };
struct BwdSites { ctta_lora_bwd_site s[SITES_MAX]; };

int sites_lpr(int k) { return k <= 64 ? 8 : k <= 128 ? 16 : k <= 256 ? 32 : 64; }

// rows per slab: a multiple of 8 (a transposed destination moves 8 tokens at a time), at least 32, and at most 512 slabs
int64_t sites_rps(int64_t rows) {
  const int64_t q = ((rows + 511) / 512 + 7) / 8 * 8;
  return q < 32 ? 32 : q;
}

// row n of b [n][r] as four floats (zeros behind r)
__device__ __forceinline__ void load_brow(const float* __restrict__ b, int64_t n, int r, float out[4]) {
  if (r == 4) {
    const float4 v = *reinterpret_cast<const float4*>(b + n * 4);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = j < r ? b[n * r + j] : 0.f;
  }
}

template <int NS, int LPR>
__global__ __launch_bounds__(256) void lora_sites_fwd_kernel(const bf16_t* __restrict__ x, int ldx, int64_t M, int K, int r,
                                                             float scale, int rps, FwdSites S) {
  __shared__ float ds[NS][FWD_TILE][4];   // D of the tile's rows, for the transposed destinations
  constexpr int G = 256 / LPR;
  const int lr = threadIdx.x % LPR, g = threadIdx.x / LPR;
  const int64_t m0 = (int64_t)blockIdx.x * rps;
  const int64_t m1 = m0 + rps < M ? m0 + rps : M;
  bool any_t = false;
#pragma unroll
  for (int s = 0; s < NS; ++s) any_t = any_t || S.s[s].tokens > 0;
  for (int64_t t0 = m0; t0 < m1; t0 += FWD_TILE) {
    const int64_t t1 = t0 + FWD_TILE < m1 ? t0 + FWD_TILE : m1;
    // the first 16 bytes of the next row are asked for before this row's arithmetic: two row loads in flight per thread
    uint4 nxt = make_uint4(0, 0, 0, 0);
    const bool pre = lr * 8 < K;
    if (pre && t0 + g < t1) nxt = *reinterpret_cast<const uint4*>(x + (t0 + g) * ldx + lr * 8);
    for (int64_t rb = t0; rb < t1; rb += G) {   // uniform trip count: every lane takes part in the fold
      const int64_t row = rb + g;
      const bool active = row < t1;
      float acc[NS][4];
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[s][j] = 0.f;
      const uint4 cur = nxt;
      if (pre && row + G < t1) nxt = *reinterpret_cast<const uint4*>(x + (row + G) * ldx + lr * 8);
      if (active) {
        const bf16_t* xr = x + row * ldx;
        for (int k0 = lr * 8; k0 < K; k0 += LPR * 8) {
          float f[8];
          unpack8(k0 == lr * 8 ? cur : *reinterpret_cast<const uint4*>(xr + k0), f);
#pragma unroll
          for (int s = 0; s < NS; ++s) {
            const float* __restrict__ a = S.s[s].a;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (j < r) {
                const float4 w0 = *reinterpret_cast<const float4*>(a + (size_t)j * K + k0);
                const float4 w1 = *reinterpret_cast<const float4*>(a + (size_t)j * K + k0 + 4);
                acc[s][j] = fmaf(f[0], w0.x, acc[s][j]); acc[s][j] = fmaf(f[1], w0.y, acc[s][j]);
                acc[s][j] = fmaf(f[2], w0.z, acc[s][j]); acc[s][j] = fmaf(f[3], w0.w, acc[s][j]);
                acc[s][j] = fmaf(f[4], w1.x, acc[s][j]); acc[s][j] = fmaf(f[5], w1.y, acc[s][j]);
                acc[s][j] = fmaf(f[6], w1.z, acc[s][j]); acc[s][j] = fmaf(f[7], w1.w, acc[s][j]);
              }
            }
          }
        }
      }
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int o = LPR / 2; o > 0; o >>= 1) acc[s][j] += __shfl_xor(acc[s][j], o, 64);
      if (!active) continue;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const ctta_lora_fwd_site& T = S.s[s];
        if (lr == 0) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j < r) {
              if (T.d) T.d[row * r + j] = acc[s][j];
              if (T.tokens > 0) ds[s][(int)(row - t0)][j] = acc[s][j];
            }
          }
        }
        if (T.tokens > 0) continue;
        bf16_t* yr = reinterpret_cast<bf16_t*>(T.y) + row * T.ldy;
        for (int c8 = lr * 8; c8 < T.n_pad; c8 += LPR * 8) {
          float bw[8][4];
#pragma unroll
          for (int i = 0; i < 8; ++i) load_brow(T.b, c8 + i, r, bw[i]);
          float o8[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) o8[i] = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j < r) {
#pragma unroll
              for (int i = 0; i < 8; ++i) o8[i] = fmaf(acc[s][j], bw[i][j] * scale, o8[i]);
            }
          }
          bool any = false;
#pragma unroll
          for (int i = 0; i < 8; ++i) any = any || o8[i] != 0.f;
          if (!any) continue;
          uint4* p = reinterpret_cast<uint4*>(yr + c8);
          float f[8];
          unpack8(*p, f);
#pragma unroll
          for (int i = 0; i < 8; ++i) f[i] += o8[i];
          *p = pack8(f);
        }
      }
    }
    if (!any_t) continue;   // uniform across the block
    __syncthreads();
    const int ntg = (int)(t1 - t0) / 8;   // slabs, tiles and token counts are multiples of 8: a group of 8 rows is one sample's
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const ctta_lora_fwd_site& T = S.s[s];
      if (T.tokens <= 0) continue;
      for (int idx = threadIdx.x; idx < ntg * T.n_pad; idx += 256) {
        const int tg = idx % ntg, n = idx / ntg;
        const int64_t row0 = t0 + tg * 8;
        const int64_t bb = row0 / T.tokens;
        const int tok0 = (int)(row0 - bb * T.tokens);
        float bv[4];
        load_brow(T.b, n, r, bv);
        float o8[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o8[i] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < r) {
            const float w = bv[j] * scale;
#pragma unroll
            for (int i = 0; i < 8; ++i) o8[i] = fmaf(ds[s][tg * 8 + i][j], w, o8[i]);
          }
        }
        bool any = false;
#pragma unroll
        for (int i = 0; i < 8; ++i) any = any || o8[i] != 0.f;
        if (!any) continue;
        uint4* p = reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(T.y) + bb * T.batch_stride + (int64_t)n * T.ldy + tok0);
        float f[8];
        unpack8(*p, f);
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] += o8[i];
        *p = pack8(f);
      }
    }
    __syncthreads();
  }
}

// ---- backward, first launch: one site per blockIdx.y.  dD = dY B for the slab's rows (the lanes, chains and fold of
// lora_down_kernel<.., KMAJOR>) and, from the same read of dY, the slab's partial sum of dY^T D.  lg = log2(lanes per row).
template <int P>
__global__ __launch_bounds__(256) void lora_sites_bwd_dy_kernel(int64_t M, int N, int r, int rps, int lg, int slabs,
                                                                float* __restrict__ dd_base, float* __restrict__ part_b, BwdSites S) {
  __shared__ float red[256 * 8];
  const ctta_lora_bwd_site& T = S.s[blockIdx.y];
  const int lpr = 1 << lg, G = 256 >> lg;
  const int lr = threadIdx.x & (lpr - 1), g = threadIdx.x >> lg;
  const int64_t m0 = (int64_t)blockIdx.x * rps;
  const int64_t m1 = m0 + rps < M ? m0 + rps : M;
  const bf16_t* __restrict__ dy = reinterpret_cast<const bf16_t*>(T.dy);
  float* __restrict__ dd = T.dd ? T.dd : dd_base + (size_t)blockIdx.y * M * r;
  const bool want = T.ga != nullptr;
  float aw[P][4][8];
#pragma unroll
  for (int p = 0; p < P; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 8; ++i) aw[p][j][i] = 0.f;
#pragma unroll 1
  for (int64_t rb = m0; rb < m1; rb += G) {
    const int64_t row = rb + g;
    const bool active = row < m1;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
      float dv[4] = {0.f, 0.f, 0.f, 0.f};
      if (want) load_brow(T.d, row, r, dv);
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const int k0 = (lr + p * lpr) * 8;
        if (k0 < N) {
          float f[8];
          unpack8(*reinterpret_cast<const uint4*>(dy + row * T.lddy + k0), f);
          float bw[8][4];
#pragma unroll
          for (int i = 0; i < 8; ++i) load_brow(T.b, k0 + i, r, bw[i]);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j < r) {
#pragma unroll
              for (int i = 0; i < 8; ++i) acc[j] = fmaf(f[i], bw[i][j], acc[j]);
#pragma unroll
              for (int i = 0; i < 8; ++i) aw[p][j][i] = fmaf(dv[j], f[i], aw[p][j][i]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      for (int o = lpr >> 1; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
    if (active && lr == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < r) dd[row * r + j] = acc[j];
    }
  }
  if (!want) return;   // uniform across the block
  // the row groups' sums meet in LDS and are added in row-group order
  float* dst = part_b + ((size_t)blockIdx.y * slabs + blockIdx.x) * r * N;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if (p * lpr * 8 >= N) break;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < r) {
#pragma unroll
        for (int i = 0; i < 8; ++i) red[(g * lpr + lr) * 8 + i] = aw[p][j][i];
        __syncthreads();
        for (int t = threadIdx.x; t < lpr * 8; t += 256) {   // 64 lanes per row: two columns per thread
          const int k = p * lpr * 8 + t;
          if (k < N) {
            float s = 0.f;
            for (int q = 0; q < G; ++q) s += red[q * lpr * 8 + t];
            dst[(size_t)j * N + k] = s;
          }
        }
        __syncthreads();
      }
    }
  }
}

// ---- backward, second launch: blockIdx.y is a chunk of ct * 8 columns of X / dX.  One read of X feeds every site's partial
// sum of dD^T X; one read-modify-write of dX takes every site's scale * dD A.
// The sites are added in site order and the sum is ROUNDED TO bf16 AFTER EACH SITE, on purpose: that is what one
// ctta_lora_up_add launch per site does to dX, so the whole data-gradient chain behind this call keeps the bits of the
// unfused route (a single rounding at the end would be more accurate and would move every base gradient downstream).
template <int NS>
__global__ __launch_bounds__(256) void lora_sites_bwd_x_kernel(const bf16_t* __restrict__ x, int ldx, bf16_t* __restrict__ dx, int lddx,
                                                               int64_t M, int K, int r, float scale, int rps, int lg, int slabs,
                                                               const float* __restrict__ dd_base, float* __restrict__ part_a, BwdSites S) {
  __shared__ float red[256 * 8];
  const int ct = 1 << lg, G = 256 >> lg;
  const int lr = threadIdx.x & (ct - 1), g = threadIdx.x >> lg;
  const int k0 = (blockIdx.y * ct + lr) * 8;
  const bool col_ok = k0 < K;
  const int64_t m0 = (int64_t)blockIdx.x * rps;
  const int64_t m1 = m0 + rps < M ? m0 + rps : M;
  bool any_want = false;
  const float* dds[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    any_want = any_want || S.s[s].ga != nullptr;
    dds[s] = S.s[s].dd ? S.s[s].dd : dd_base + (size_t)s * M * r;
  }
  // scale * a[j][k0 + i], the operand ctta_lora_up_add(b_rmajor = 1) multiplies with, for the chunk's columns: in LDS (as
  // two conflict-free float4 planes per (site, j)), because 32 registers per site beside the 32 accumulators per site
  // would leave one wave per SIMD at three sites
  __shared__ float4 as4[NS * 4 * 2 * 64];
  if (dx) {
    for (int e = threadIdx.x; e < NS * 4 * 2 * ct; e += 256) {
      const int l = e % ct, h = (e / ct) % 2, j = (e / ct / 2) % 4, s = e / ct / 8;
      const int c = (blockIdx.y * ct + l) * 8 + h * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < K && j < r) {
        v = *reinterpret_cast<const float4*>(S.s[s].a + (size_t)j * K + c);
        v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
      }
      as4[e] = v;
    }
    __syncthreads();
  }
  float aw[NS][4][8];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 8; ++i) aw[s][j][i] = 0.f;
  if (col_ok) {
#pragma unroll 2
    for (int64_t row = m0 + g; row < m1; row += G) {
      float xf[8];
      if (any_want) unpack8(*reinterpret_cast<const uint4*>(x + row * ldx + k0), xf);
      float f[8];
      uint4* p = dx ? reinterpret_cast<uint4*>(dx + row * lddx + k0) : nullptr;
      if (dx) unpack8(*p, f);
      bool changed = false;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        float dv[4];
        load_brow(dds[s], row, r, dv);
        if (dx) {
          float o8[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) o8[i] = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j < r) {
              const float4 w0 = as4[((s * 4 + j) * 2) * ct + lr], w1 = as4[((s * 4 + j) * 2 + 1) * ct + lr];
              o8[0] = fmaf(dv[j], w0.x, o8[0]); o8[1] = fmaf(dv[j], w0.y, o8[1]);
              o8[2] = fmaf(dv[j], w0.z, o8[2]); o8[3] = fmaf(dv[j], w0.w, o8[3]);
              o8[4] = fmaf(dv[j], w1.x, o8[4]); o8[5] = fmaf(dv[j], w1.y, o8[5]);
              o8[6] = fmaf(dv[j], w1.z, o8[6]); o8[7] = fmaf(dv[j], w1.w, o8[7]);
            }
          }
          bool any = false;
#pragma unroll
          for (int i = 0; i < 8; ++i) any = any || o8[i] != 0.f;
          if (any) {
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] += o8[i];
            const uint4 q = pack8(f);   // this site's rounding
            unpack8(q, f);
            changed = true;
          }
        }
        if (S.s[s].ga) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j < r) {
#pragma unroll
              for (int i = 0; i < 8; ++i) aw[s][j][i] = fmaf(dv[j], xf[i], aw[s][j][i]);
            }
          }
        }
      }
      if (changed) *p = pack8(f);   // f holds bf16 values: exact
    }
  }
  if (!any_want) return;   // uniform across the block
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (!S.s[s].ga) continue;
    float* dst = part_a + ((size_t)s * slabs + blockIdx.x) * r * K;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < r) {
#pragma unroll
        for (int i = 0; i < 8; ++i) red[(g * ct + lr) * 8 + i] = aw[s][j][i];
        __syncthreads();
        for (int e = threadIdx.x; e < ct * 8; e += 256) {   // 64 lanes per row: two columns per thread
          const int k = blockIdx.y * ct * 8 + e;
          if (k < K) {
            float t = 0.f;
            for (int q = 0; q < G; ++q) t += red[q * ct * 8 + e];
            dst[(size_t)j * K + k] = t;
          }
        }
        __syncthreads();
      }
    }
  }
}

// ---- backward, third launch: every gradient tensor of the call.  blockIdx.y is the job (site x {gb, ga}); the slabs are
// added in slab order, four loads in flight.  g = fl(g + fl(scale * sum)): the product is rounded on its own, so a
// non-zero g receives exactly what a zeroed one does.
struct FoldJob { const float* part; float* g; const int32_t* map; int64_t sr, sk; int K; };
struct FoldJobs { FoldJob j[2 * SITES_MAX]; };
__global__ __launch_bounds__(256) void lora_sites_fold_kernel(int slabs, int r, float scale, FoldJobs J) {
  const FoldJob& F = J.j[blockIdx.y];
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= r * F.K) return;
  const int j = idx / F.K, k = idx % F.K;
  const int col = F.map ? F.map[k] : k;
  if (col < 0) return;
  const size_t st = (size_t)r * F.K;
  const float* p = F.part + idx;
  float s = 0.f;
  int i = 0;
  for (; i + 4 <= slabs; i += 4) {
    const float v0 = p[(size_t)i * st], v1 = p[(size_t)(i + 1) * st], v2 = p[(size_t)(i + 2) * st], v3 = p[(size_t)(i + 3) * st];
    s += v0; s += v1; s += v2; s += v3;
  }
  for (; i < slabs; ++i) s += p[(size_t)i * st];
  float* q = F.g + j * F.sr + col * F.sk;
  *q = __fadd_rn(*q, __fmul_rn(scale, s));
}

}  // namespace

extern "C" int ctta_lora_sites_supported(int k_pad, const int* n_pad, int n_sites, int r, int vt_tokens, int vt_ldt,
                                         int64_t vt_batch_stride) {
  if (!n_pad || n_sites < 1 || n_sites > SITES_MAX || r < 1 || r > 4) return 0;
  if (k_pad < 8 || k_pad % 8 || k_pad > SITES_W_MAX) return 0;
  for (int s = 0; s < n_sites; ++s)
    if (n_pad[s] < 8 || n_pad[s] % 8 || n_pad[s] > SITES_W_MAX || n_pad[s] != n_pad[0]) return 0;
  if (vt_tokens < 0) return 0;
  if (vt_tokens > 0 && (vt_tokens % 8 || vt_ldt % 8 || vt_ldt < vt_tokens || vt_batch_stride % 8)) return 0;
  return 1;
}

extern "C" ctta_status ctta_lora_sites_fwd(const void* x, int ldx, int64_t rows, int k_pad, int r, float scale,
                                           const ctta_lora_fwd_site* sites, int n_sites, void* stream) {
  CTTA_REQUIRE(x && sites, "lora_sites_fwd: null pointer");
  CTTA_REQUIRE(n_sites >= 1 && n_sites <= SITES_MAX && r >= 1 && r <= 4, "lora_sites_fwd: %d sites of rank %d (1..3 sites, rank 1..4)", n_sites, r);
  CTTA_REQUIRE(rows >= 0 && ldx >= k_pad && ldx % 8 == 0 && aligned16(x), "lora_sites_fwd: rows=%lld k_pad=%d ldx=%d", (long long)rows, k_pad, ldx);
  FwdSites S;
  memset(&S, 0, sizeof(S));
  int np[SITES_MAX];
  int vt_tokens = 0, vt_ldt = 0;
  int64_t vt_bs = 0;
  for (int s = 0; s < n_sites; ++s) {
    const ctta_lora_fwd_site& T = sites[s];
    CTTA_REQUIRE(T.a && T.b && T.y && aligned16(T.a) && aligned16(T.b) && aligned16(T.y), "lora_sites_fwd: site %d: null or unaligned pointer", s);
    np[s] = T.n_pad;
    if (T.tokens > 0) {
      CTTA_REQUIRE(rows % T.tokens == 0 && T.ldy >= T.tokens && T.batch_stride >= (int64_t)T.n_pad * T.ldy && T.tokens % 8 == 0 &&
                   T.ldy % 8 == 0 && T.batch_stride % 8 == 0,
                   "lora_sites_fwd: site %d: tokens=%d ldt=%d batch_stride=%lld rows=%lld", s, T.tokens, T.ldy, (long long)T.batch_stride, (long long)rows);
      vt_tokens = T.tokens; vt_ldt = T.ldy; vt_bs = T.batch_stride;
    } else {
      CTTA_REQUIRE(T.tokens == 0 && T.ldy >= T.n_pad && T.ldy % 8 == 0, "lora_sites_fwd: site %d: n_pad=%d ldy=%d", s, T.n_pad, T.ldy);
    }
    S.s[s] = T;
  }
  CTTA_REQUIRE(ctta_lora_sites_supported(k_pad, np, n_sites, r, vt_tokens, vt_ldt, vt_bs), "lora_sites_fwd: shapes outside the fused kernels (ctta_lora_sites_supported)");
  if (rows == 0) return CTTA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int rps = (int)sites_rps(rows);
  const dim3 grid((unsigned)cdiv64(rows, rps));
  const bf16_t* xp = (const bf16_t*)x;
#define LAUNCH(NS, LPR) hipLaunchKernelGGL((lora_sites_fwd_kernel<NS, LPR>), grid, dim3(256), 0, st, xp, ldx, rows, k_pad, r, scale, rps, S)
#define BY_LPR(NS)                                      \
  do {                                                  \
    switch (sites_lpr(k_pad)) {                         \
      case 8: LAUNCH(NS, 8); break;                     \
      case 16: LAUNCH(NS, 16); break;                   \
      case 32: LAUNCH(NS, 32); break;                   \
      default: LAUNCH(NS, 64); break;                   \
    }                                                   \
  } while (0)
  if (n_sites == 1) BY_LPR(1);
  else if (n_sites == 2) BY_LPR(2);
  else BY_LPR(3);
#undef BY_LPR
#undef LAUNCH
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}

// [dD of every site][partials of gb][partials of ga]; sized for the largest slab count any smaller row count can have, so
// the figure never shrinks as rows grow
extern "C" size_t ctta_lora_sites_bwd_scratch_floats(int64_t rows, int k_pad, int n_pad, int n_sites, int r) {
  if (rows < 1 || n_sites < 1 || n_sites > SITES_MAX || r < 1 || r > 4) return 0;
  if (k_pad < 8 || k_pad % 8 || k_pad > SITES_W_MAX || n_pad < 8 || n_pad % 8 || n_pad > SITES_W_MAX) return 0;
  const int64_t sl = (rows + 31) / 32 < 512 ? (rows + 31) / 32 : 512;
  return (size_t)n_sites * ((size_t)(rows * r + 3) / 4 * 4 + (size_t)sl * r * (n_pad + k_pad));
}

extern "C" ctta_status ctta_lora_sites_bwd(const void* x, int ldx, void* dx, int lddx, int64_t rows, int k_pad, int r, float scale,
                                           const ctta_lora_bwd_site* sites, int n_sites, float* scratch, void* stream) {
  CTTA_REQUIRE(sites && scratch, "lora_sites_bwd: null pointer");
  CTTA_REQUIRE(n_sites >= 1 && n_sites <= SITES_MAX && r >= 1 && r <= 4, "lora_sites_bwd: %d sites of rank %d (1..3 sites, rank 1..4)", n_sites, r);
  CTTA_REQUIRE(rows >= 0 && aligned16(scratch), "lora_sites_bwd: rows=%lld", (long long)rows);
  BwdSites S;
  memset(&S, 0, sizeof(S));
  int np[SITES_MAX];
  bool any_want = false;
  for (int s = 0; s < n_sites; ++s) {
    const ctta_lora_bwd_site& T = sites[s];
    CTTA_REQUIRE(T.dy && T.a && T.b && aligned16(T.dy) && aligned16(T.a) && aligned16(T.b) && (!T.dd || aligned16(T.dd)),
                 "lora_sites_bwd: site %d: null or unaligned pointer", s);
    CTTA_REQUIRE((T.ga != nullptr) == (T.gb != nullptr), "lora_sites_bwd: site %d: ga and gb come together", s);
    CTTA_REQUIRE(!T.ga || (T.d && aligned16(T.d)), "lora_sites_bwd: site %d: parameter gradients need the forward's d", s);
    CTTA_REQUIRE(T.lddy >= T.n_pad && T.lddy % 8 == 0, "lora_sites_bwd: site %d: n_pad=%d lddy=%d", s, T.n_pad, T.lddy);
    np[s] = T.n_pad;
    any_want = any_want || T.ga;
    S.s[s] = T;
  }
  CTTA_REQUIRE(ctta_lora_sites_supported(k_pad, np, n_sites, r, 0, 0, 0), "lora_sites_bwd: shapes outside the fused kernels (ctta_lora_sites_supported)");
  CTTA_REQUIRE(!dx || (lddx >= k_pad && lddx % 8 == 0 && aligned16(dx)), "lora_sites_bwd: k_pad=%d lddx=%d", k_pad, lddx);
  CTTA_REQUIRE(!any_want || (x && ldx >= k_pad && ldx % 8 == 0 && aligned16(x)), "lora_sites_bwd: k_pad=%d ldx=%d", k_pad, ldx);
  if (rows == 0) return CTTA_OK;
  hipStream_t st = (hipStream_t)stream;
  const int n = np[0];
  const int rps = (int)sites_rps(rows);
  const int slabs = (int)cdiv64(rows, rps);
  float* dd_base = scratch;
  float* part_b = scratch + (size_t)n_sites * ((size_t)(rows * r + 3) / 4 * 4);
  float* part_a = part_b + (size_t)n_sites * slabs * r * n;
  auto lg2 = [](int v) { int l = 0; while ((1 << l) < v) ++l; return l; };
  const int lpr_n = sites_lpr(n), passes = (n + lpr_n * 8 - 1) / (lpr_n * 8);
#define LAUNCH(P)                                                                                                                \
  hipLaunchKernelGGL((lora_sites_bwd_dy_kernel<P>), dim3((unsigned)slabs, (unsigned)n_sites), dim3(256), 0, st, rows, n, r, rps, \
                     lg2(lpr_n), slabs, dd_base, part_b, S)
  if (passes == 1) LAUNCH(1);
  else if (passes == 2) LAUNCH(2);
  else LAUNCH(3);
#undef LAUNCH
  CTTA_LAUNCH_CHECK();
  if (dx || any_want) {
    const int ct = sites_lpr(k_pad);
    const dim3 grid((unsigned)slabs, (unsigned)((k_pad / 8 + ct - 1) / ct));
#define LAUNCH(NS)                                                                                                              \
  hipLaunchKernelGGL((lora_sites_bwd_x_kernel<NS>), grid, dim3(256), 0, st, (const bf16_t*)x, ldx, (bf16_t*)dx, lddx, rows, k_pad, r, \
                     scale, rps, lg2(ct), slabs, dd_base, part_a, S)
    if (n_sites == 1) LAUNCH(1);
    else if (n_sites == 2) LAUNCH(2);
    else LAUNCH(3);
#undef LAUNCH
    CTTA_LAUNCH_CHECK();
  }
  if (any_want) {
    FoldJobs J;
    memset(&J, 0, sizeof(J));
    int nj = 0, kmax = 0;
    for (int s = 0; s < n_sites; ++s) {
      const ctta_lora_bwd_site& T = sites[s];
      if (!T.ga) continue;
      J.j[nj++] = {part_b + (size_t)s * slabs * r * n, T.gb, T.n_map, T.gb_stride_r, T.gb_stride_k, n};
      J.j[nj++] = {part_a + (size_t)s * slabs * r * k_pad, T.ga, T.k_map, T.ga_stride_r, T.ga_stride_k, k_pad};
    }
    kmax = n > k_pad ? n : k_pad;
    hipLaunchKernelGGL(lora_sites_fold_kernel, dim3((unsigned)((r * kmax + 255) / 256), (unsigned)nj), dim3(256), 0, st, slabs, r, scale, J);
    CTTA_LAUNCH_CHECK();
  }
  return CTTA_OK;
}
