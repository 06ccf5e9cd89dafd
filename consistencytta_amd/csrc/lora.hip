// LoRA adapter operators of the attention projections (diffusers LoRAAttnProcessor, attention_processor.py:508-613):
//   y = W x + scale * up(down(x)),  down: Linear(in, r, bias=False), up: Linear(r, out, bias=False), rank r in [1, 16].
// The base product W x stays the conv_gemm launch it is; these kernels add the rank-r term beside it, forward and backward:
//   ctta_lora_down     D[M][r] (fp32)  = X[M][K] (bf16) * A^T         forward D = X A^T, backward dD = dY B
//   ctta_lora_up_add   Y[M][N] (bf16) += scale * D * B^T               forward Y += D B^T, backward dX += dD A
//   ctta_lora_up_add_t the same into a transposed result V^T[b][n][token] (how the engines keep attention values)
//   ctta_lora_wgrad    G (fp32)       += scale * sum_m D[m][j] X[m][k]  dA = dD^T X, dB = dY^T D
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
