// Implicit-GEMM convolution / linear / batched matmul on the gfx950 matrix cores.
//
//   out[m][n] = alpha * ( sum_k X[m][k] * W[n][k] + bias[n] + rowvec[b(m)][n] + res[m][n] )
//
// m runs over output pixels (b, oh, ow) of an NHWC bf16 tensor, k over (kh, kw, c) of the
// receptive field (gathered on the fly: zero padding, stride, dilation, optional x2 nearest
// upsample, optional two-source channel concat), n over output channels.  W is pre-packed
// bf16 [n][k_pad] (K contiguous), so both MFMA operands are K-contiguous 16-byte fragments.
//
// This one kernel family is every conv2d / conv1d / ConvTranspose1d / Linear / QK^T / PV of
// the reference path:
//   F.conv2d   resnet.py:549-597, modules.py:155-175,  Upsample2D resnet.py:126-161 (fused),
//   F.conv1d / conv_transpose1d  hifigan/models.py:56-63,101-117 (ConvTranspose1d is run as
//   `stride` phase-convolutions written through an output remap),
//   F.linear   attention.py:276-334, attention_processor.py:1107-1136, torch.bmm modules.py:204-230.
//
// CDNA4 mapping: 256-thread workgroups (4 wave64), v_mfma_f32_16x16x32_bf16 with the WEIGHT
// tile as the A operand and the PIXEL tile as the B operand, so each lane ends up holding 4
// consecutive output channels of one pixel (8-byte packed bf16 stores along NHWC's fastest
// axis).  Global -> register -> LDS staging with a 2-deep LDS ring and the next tile's
// global loads issued before the current tile's MFMAs (one barrier per K-step).  LDS rows are
// padded by 16 B to spread ds_read_b128 over banks.
#include "conv_gemm_kernel.h"
#include "conv_plan.h"

#include <stdlib.h>

CTTA_CONV_VARIANTS_ALL(CTTA_CONV_DECLARE)
CTTA_CONV_VARIANTS_KIND(CTTA_CONV_DECLARE_K)

// ------------------------------------------------------------------------------------------
// 1-D "halo" convolution for the narrowest layers (C = Cin = Cout = 32, stride 1): the HiFi-GAN ResBlock
// convolutions of the last upsampling stage (hifigan/models.py:56-63), 5.2 M positions x 32 channels at B=32.  As an implicit
// GEMM these layers re-gather every input row once per tap from L2 (k = 3/7/11 times) while producing
// only C output channels per row -- the generic kernel is L2-bandwidth bound there.  Here a workgroup
// stages its BL output positions plus the (k-1)*dilation halo ONCE in LDS; the taps are row offsets into
// that tile, the weight fragments (A operands, [n][k_pad] packing shared with conv_gemm) stream straight
// from L1/L2 into registers one (tap, 32-channel chunk) ahead of the MFMAs.  Same MFMA roles and the same
// epilogue as conv_gemm_kernel: weights = A (rows = Cout), positions = B (cols), lane owns 4 consecutive Cout.
template <int C, int BL>
__global__ __launch_bounds__(256) void conv1d_halo_kernel(const ConvParams p) {
  constexpr int RS = C + 8;      // LDS row stride (bf16): C*2 + 16 bytes -> conflict-free ds_read_b128 over 16 rows
  constexpr int NCB = C / 16;    // Cout blocks
  constexpr int NCH = C / 32;    // 32-channel chunks per tap
  constexpr int PB = BL / 64;    // position blocks per wave
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 15, lg = lane >> 4;
  const int b = blockIdx.y, l0 = blockIdx.x * BL;
  const int L = p.wo;
  const int nrows = BL + (p.taps - 1) * p.dw;
  const bf16_t* xb = p.x0 + (size_t)b * L * p.xs0;
  for (int idx = tid; idx < nrows * (C / 8); idx += 256) {
    const int r = idx / (C / 8), cc = idx - r * (C / 8);
    const int pos = l0 - p.pw + r;
    uint4 v = make_uint4(0, 0, 0, 0);
    if ((unsigned)pos < (unsigned)L) v = *reinterpret_cast<const uint4*>(xb + (size_t)pos * p.xs0 + cc * 8);
    *reinterpret_cast<uint4*>(xs + r * RS + cc * 8) = v;
  }
  f32x4_t acc[NCB][PB];
#pragma unroll
  for (int i = 0; i < NCB; ++i)
#pragma unroll
    for (int j = 0; j < PB; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const bf16_t* wl = p.w + (size_t)lq * p.k_pad + lg * 8;
  bf16x8_t a_cur[NCB], a_nxt[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
    a_cur[cb] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(wl + (size_t)cb * 16 * p.k_pad));
  __syncthreads();
  const bf16_t* xw = xs + (wave * (BL / 4) + lq) * RS + lg * 8;
  const int nsteps = p.taps * NCH;
  for (int st = 0; st < nsteps; ++st) {
    const int tap = st / NCH, ch = st - tap * NCH;
    if (st + 1 < nsteps) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
        a_nxt[cb] = __builtin_bit_cast(
            bf16x8_t, *reinterpret_cast<const uint4*>(wl + (size_t)cb * 16 * p.k_pad + (size_t)(st + 1) * 32));
    }
    const bf16_t* xr = xw + (tap * p.dw) * RS + ch * 32;
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
      const bf16x8_t bf = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(xr + pb * 16 * RS));
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) acc[cb][pb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_cur[cb], bf, acc[cb][pb], 0, 0, 0);
    }
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) a_cur[cb] = a_nxt[cb];
  }
  if (p.wide_store) {   // same transposed store as conv_gemm_kernel: 16 positions x C channels per wave at a time
    constexpr int RSF = C * 4 + 16;
    constexpr int LPR = C / 4, RPW = 64 / LPR;
    unsigned char* stg = smem_raw + (size_t)wave * 16 * RSF;
    const int col4 = lane % LPR, prow = lane / LPR;
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias) bias4 = *reinterpret_cast<const float4*>(p.bias + col4 * 4);
    __syncthreads();   // the input tile is dead
#pragma unroll
    for (int pb = 0; pb < PB; ++pb) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const f32x4_t a = acc[cb][pb];
        *reinterpret_cast<float4*>(stg + lq * RSF + (cb * 16 + lg * 4) * 4) = make_float4(a[0], a[1], a[2], a[3]);
      }
      __syncthreads();
#pragma unroll
      for (int r = prow; r < 16; r += RPW) {
        const int l = l0 + wave * (BL / 4) + pb * 16 + r;
        if (l < L) epilogue_wide4(p, *reinterpret_cast<const float4*>(stg + r * RSF + col4 * 16), bias4, b * L + l, col4 * 4, 0);
      }
      if (pb + 1 < PB) __syncthreads();
    }
    return;
  }
#pragma unroll
  for (int pb = 0; pb < PB; ++pb) {
    const int l = l0 + wave * (BL / 4) + pb * 16 + lq;
    if (l < L) {
      const int m = b * L + l;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) epilogue_store(p, acc[cb][pb], m, cb * 16 + lg * 4, b, l, 0);
    }
  }
}

// ------------------------------------------------------------------------------------------
// split-K second pass: sums the fp32 partial slabs [S][M][ld] and runs the fused epilogue of the original launch
__global__ __launch_bounds__(256) void splitk_finish_kernel(const ConvParams p, const float* __restrict__ slabs, int S,
                                                            long long slab_stride, int ld) {
  const int n4 = (p.n + 3) / 4;
  const long long total = (long long)p.M * n4;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int m = (int)(i / n4), n = (int)(i - (long long)m * n4) * 4;
    const float* src = slabs + (size_t)m * ld + n;
    float4 a = *reinterpret_cast<const float4*>(src);
    // the partial sums are requested four slabs at a time and added in slab order (the plain loop waits for every load
    // before it asks for the next: S - 1 serial round trips per lane)
    int s2 = 1;
    for (; s2 + 4 <= S; s2 += 4) {
      float4 q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) q[u] = *reinterpret_cast<const float4*>(src + (size_t)(s2 + u) * slab_stride);
#pragma unroll
      for (int u = 0; u < 4; ++u) { a.x += q[u].x; a.y += q[u].y; a.z += q[u].z; a.w += q[u].w; }
    }
    for (; s2 < S; ++s2) {
      const float4 q = *reinterpret_cast<const float4*>(src + (size_t)s2 * slab_stride);
      a.x += q.x; a.y += q.y; a.z += q.z; a.w += q.w;
    }
    const int b = m / p.howo;
    epilogue_store(p, (f32x4_t){a.x, a.y, a.z, a.w}, m, n, b, m - (long long)b * p.howo, 0);
  }
}
// Split-K workspace.  Every engine handle owns one (SplitWs in engine_common.h) and binds it to the calling host
// thread for the duration of each entry point (ctta_conv_bind_workspace), so handles running on different streams
// or host threads never share partial-sum slabs.  Raw ctta_conv_gemm callers that bound nothing get a lazily
// allocated workspace PER DEVICE (mutex-guarded); launches that share it must be ordered on one stream.
// The first SK_HDR_WORDS 32-bit words of a workspace are the stream-K header (ConvParams::sk_hdr): zero when the workspace is
// created, kept consistent by the stream-K launches themselves afterwards.  Partial slabs / slots start behind it.
static const size_t kSplitWsBytes = (size_t)192 << 20;
static thread_local float* t_ws = nullptr;
static thread_local size_t t_ws_bytes = 0;
static thread_local int t_ws_hdr = 0;     // the bound workspace's header was zeroed by its owner: stream-K launches may use it
extern "C" void ctta_conv_bind_workspace(void* ws, size_t bytes) { t_ws = (float*)ws; t_ws_bytes = ws ? bytes : 0; t_ws_hdr = 0; }
extern "C" void ctta_conv_bind_workspace_ex(void* ws, size_t bytes, int header_zeroed) {
  t_ws = (float*)ws; t_ws_bytes = ws ? bytes : 0; t_ws_hdr = (ws && header_zeroed) ? 1 : 0;
}
extern "C" void ctta_conv_bound_workspace(void** ws, size_t* bytes) { if (ws) *ws = t_ws; if (bytes) *bytes = t_ws_bytes; }
extern "C" int ctta_conv_bound_workspace_header(void) { return t_ws_hdr; }
extern "C" size_t ctta_conv_workspace_bytes(void) { return kSplitWsBytes; }
extern "C" size_t ctta_conv_workspace_header_bytes(void) { return (size_t)SK_HDR_WORDS * 4; }
#include <mutex>
static float* splitk_workspace(size_t* bytes, bool* hdr_ok = nullptr) {
  if (t_ws) { *bytes = t_ws_bytes; if (hdr_ok) *hdr_ok = t_ws_hdr != 0; return t_ws; }
  static std::mutex mu;
  static float* per_dev[64] = {nullptr};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  if (!per_dev[dev]) {
    if (hipMalloc((void**)&per_dev[dev], kSplitWsBytes) != hipSuccess) per_dev[dev] = nullptr;
    else if (hipMemset(per_dev[dev], 0, (size_t)SK_HDR_WORDS * 4) != hipSuccess) { (void)hipFree(per_dev[dev]); per_dev[dev] = nullptr; }
  }
  *bytes = kSplitWsBytes;
  if (hdr_ok) *hdr_ok = per_dev[dev] != nullptr;
  return per_dev[dev];
}
// ------------------------------------------------------------------------------------------
// The launch side of the tile table (conv_plan.h: CTTA_CONV_TILE_TABLE holds the shapes, the ids and their names)
struct Variant {
  void (*launch)(const ConvParams&, dim3, hipStream_t);
  ctta_status (*prepare)();
};
#define VARIANT(BM, BN, BK, WM, WN, G, S) {launch_variant<BM, BN, BK, WM, WN, G, S, 0>, prepare_variant<BM, BN, BK, WM, WN, G, S, 0>},
#define VARIANT_K(BM, BN, BK, WM, WN, G, S, KIND, TAG) \
  {launch_variant<BM, BN, BK, WM, WN, G, S, KIND>, prepare_variant<BM, BN, BK, WM, WN, G, S, KIND>},
static const Variant kVariants[] = {CTTA_CONV_TILE_TABLE(VARIANT, VARIANT_K)};
static_assert(sizeof(kVariants) / sizeof(kVariants[0]) == kNumVariants, "one launcher per tile");

extern "C" int ctta_conv_gemm_num_variants(void) { return kNumVariants; }
extern "C" const char* ctta_conv_gemm_variant_name(int id) {
  return (id >= 1 && id <= kNumVariants) ? kTiles[id - 1].name : "auto";
}

static const bf16_t* zero_page() {   // 256 zero bytes per device (source of out-of-range chunks in the LDS-direct paths)
  static std::mutex mu;
  static bf16_t* per_dev[64] = {nullptr};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  if (!per_dev[dev]) {
    bf16_t* z = nullptr;
    if (hipMalloc((void**)&z, 256) != hipSuccess) return nullptr;
    if (hipMemset(z, 0, 256) != hipSuccess) { (void)hipFree(z); return nullptr; }
    per_dev[dev] = z;
  }
  return per_dev[dev];
}

static thread_local unsigned long long* t_stamps = nullptr;
extern "C" void ctta_conv_debug_stamps(void* buf) { t_stamps = (unsigned long long*)buf; }
unsigned long long* ctta_debug_stamps_current() { return t_stamps; }
static thread_local int t_no_splitk = 0;
extern "C" void ctta_conv_suppress_splitk(int on) { t_no_splitk = on ? 1 : 0; }

static thread_local int t_last_gn_chunks = 0;
extern "C" int ctta_conv_last_gn_chunks(void) { return t_last_gn_chunks; }

// The plan's view of this process: options, thread state, and the workspace on first use (which may allocate it)
static void lookup_workspace(ConvPlanEnv* e) {
  bool hdr = false;
  e->ws = splitk_workspace(&e->ws_bytes, &hdr);
  e->ws_ok = e->ws != nullptr;
  e->ws_hdr = hdr;
}
static ConvPlanEnv live_env() {
  ConvPlanEnv e;
  memset(&e, 0, sizeof(e));
  e.cu_count = ctta_cu_count();
  e.xcd = ctta_opt(CTTA_OPT_XCD); e.splitk = ctta_opt(CTTA_OPT_SPLITK);
  e.streamk = ctta_opt(CTTA_OPT_STREAMK); e.streamk_grid = ctta_opt(CTTA_OPT_STREAMK_GRID);
  e.no_splitk = t_no_splitk != 0;
  e.stamps = t_stamps != nullptr;
  e.lookup = lookup_workspace;
  return e;
}

// Plan (conv_plan.hip: check, params, choose tile, schedule), then launch: the only step that touches the device.
extern "C" ctta_status ctta_conv_gemm(const ctta_conv_desc* d, void* stream) {
  t_last_gn_chunks = 0;
  ConvPlanEnv env = live_env();
  ConvPlan pl;
  CTTA_TRY(ctta_conv_make_plan(d, env, pl));
  t_last_gn_chunks = pl.p.gn_nchunk;
  hipStream_t s = (hipStream_t)stream;
  pl.p.stamps = pl.q.stamps = pl.t.stamps = t_stamps;
  const bool prof = ctta_prof_active();
  if (pl.halo) {
    if (prof) ctta_prof_begin(0, pl.prof_code, pl.M, d->n, pl.K, pl.groups, s);
    const size_t smem = (size_t)(256 + (pl.p.taps - 1) * pl.p.dw) * (32 + 8) * 2;
    conv1d_halo_kernel<32, 256><<<dim3(pl.gx, pl.gy), dim3(256), smem, s>>>(pl.p);
    if (prof) ctta_prof_end(s);
    CTTA_LAUNCH_CHECK();
    return CTTA_OK;
  }
  const Variant& v = kVariants[pl.vid - 1];
  pl.p.zero = pl.q.zero = pl.t.zero = zero_page();
  CTTA_REQUIRE(pl.p.zero, "conv_gemm: could not allocate the zero page");
  CTTA_TRY(v.prepare());
  const dim3 grid(pl.gx, pl.gy, pl.gz);
  if (prof) ctta_prof_begin(0, pl.prof_code, pl.M, d->n, pl.K, pl.groups, s);
  if (pl.kind >= 2) {
    pl.p.sk_hdr = reinterpret_cast<unsigned*>(env.ws);
    pl.p.sk_slots = env.ws + SK_HDR_WORDS;
    v.launch(pl.p, grid, s);
  } else if (pl.splits > 1) {
    float* slabs = env.ws + SK_HDR_WORDS;       // the stream-K header stays untouched
    pl.q.out = slabs;
    v.launch(pl.q, grid, s);
    splitk_finish_kernel<<<dim3(pl.finish_blocks), dim3(256), 0, s>>>(pl.p, slabs, pl.splits, pl.M * pl.ld, pl.ld);
  } else {
    v.launch(pl.p, grid, s);
    if (pl.tail_rows > 0) {
      const Variant& tv = kVariants[pl.tail_vid - 1];
      CTTA_TRY(tv.prepare());
      tv.launch(pl.t, dim3(pl.tail_gx, pl.tail_gy, 1), s);
    }
  }
  if (prof) ctta_prof_end(s);
  CTTA_LAUNCH_CHECK();
  return CTTA_OK;
}
