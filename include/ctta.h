/*
 * ctta.h -- C ABI of the MI355X-native ConsistencyTTA hot path (libctta_hip.so).
 *
 * The reference (Bai-YT/ConsistencyTTA) has no FFI: its "plugin boundary" for this path is
 * the PyTorch nn.Module protocol.  Each entry point below replaces one of
 * those module calls and cites it.  All pointers are raw DEVICE pointers unless marked
 * host; all calls are asynchronous on `stream` (a hipStream_t passed as void*), borrow
 * their arguments for the duration of the call only, and return a ctta_status (no
 * exceptions cross the boundary; ctta_last_error() gives the message for this thread).
 * Handles own their pre-packed bf16 weights and activation arena and are freed by
 * *_destroy.  One handle per (device, model); calls on one handle must not overlap.
 *
 * Layout contract at the boundary: fp32, the reference's own layouts (NCHW latents/mel,
 * (B,L,X) text states, (B,L) uint8 mask).  Internally activations are NHWC bf16 with fp32
 * accumulation (the reference's own GPU recipe is bf16 autocast, inference.py:190).
 */
#ifndef CTTA_H
#define CTTA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  CTTA_OK = 0,
  CTTA_ERR_INVALID = 1,     /* bad argument / unsupported shape (reference: ValueError/assert) */
  CTTA_ERR_HIP = 2,         /* a HIP runtime call failed */
  CTTA_ERR_MISSING_KEY = 3, /* weight table lacks a state-dict key (reference: load_state_dict) */
  CTTA_ERR_NOMEM = 4
} ctta_status;

const char* ctta_last_error(void);
int ctta_version(void);

/* Library options -- the only switches of the library (nothing in it reads the environment; there is no other global state
 * than this table and the per-thread bindings documented below).  Process-wide plain ints, read by the call that uses
 * them; set them before the handles they concern are created or between calls, not while another host thread is inside
 * the library.  Names, defaults and what each one trades:
 *   "xcd"          1  blockIdx -> tile order that keeps the tiles sharing operands on one XCD's L2 (0: plain 2-D grids)
 *   "splitk"       1  deep thin GEMMs (few output tiles, long K) are cut over K: two-pass split-K or stream-K (0: never)
 *   "streamk"      1  ... as ONE persistent launch that folds its partial tiles itself, where the tile rules choose it
 *                     (0: two-pass split-K only); needs a workspace with a zeroed header (ctta_conv_bind_workspace_ex)
 *   "streamk_grid" 0  tuning: workgroups of a stream-K launch (0: one per CU slot)
 *   "wgrad_stream" 1  weight-gradient launches of ctta_unet_backward* go to the handle's side stream (0: everything on the
 *                     caller's stream -- what a per-launch profile needs; read at every backward call)
 *   "gn_fuse"      1  GroupNorm statistics come from the producing convolution's epilogue (= ctta_set_gn_fuse)
 *   "fused_res"    1  HiFi-GAN ResBlock units run as fused pair kernels (0: one conv_gemm launch per convolution)
 *   "ffn_fuse"     1  the inference forward runs the 256-wide transformer feed-forward as one row-tile kernel
 *                     (ctta_ffn_geglu; 0: ff1 + GEGLU epilogue and ff2 as two conv_gemm launches); read when a handle is built
 * Every option is exercised in its non-default position by tests/test_options_gpu.py. */
ctta_status ctta_set_option(const char* name, int value);
ctta_status ctta_get_option(const char* name, int* value);
int ctta_num_options(void);
const char* ctta_option_name(int i);
int ctta_option_default(int i);

/* One entry of a state dict: reference key name, fp32 device data, shape. */
typedef struct {
  const char* name;
  const float* data;
  int ndim;
  int64_t shape[4];
} ctta_tensor;

/* ------------------------------------------------------------------------------------ *
 * U-Net.  Replaces UNet2DConditionGuidedModel.forward
 * (diffusers/models/unet_2d_condition_guided.py:716-945) and, with guided=0, the teacher
 * UNet2DConditionModel.forward (unet_2d_condition.py:668-907).
 * ------------------------------------------------------------------------------------ */
#define CTTA_MAX_LEVELS 4
typedef struct {
  int in_channels, out_channels;
  int n_levels;                             /* len(block_out_channels), <= 4 */
  int block_out_channels[CTTA_MAX_LEVELS];
  int heads[CTTA_MAX_LEVELS];               /* config "attention_head_dim" = head COUNT */
  int layers_per_block[CTTA_MAX_LEVELS];
  int down_cross[CTTA_MAX_LEVELS];          /* 1: CrossAttnDownBlock2D, 0: DownBlock2D */
  int up_cross[CTTA_MAX_LEVELS];            /* 1: CrossAttnUpBlock2D,   0: UpBlock2D   */
  int cross_attention_dim;
  int norm_num_groups;
  float norm_eps;
  int flip_sin_to_cos;
  float freq_shift;
  int guided;                               /* 1: guidance Fourier branch present */
  int max_batch, height, width, max_text_len; /* arena sizing */
  int debug_taps;                           /* 1: keep every named intermediate (tests) */
  int enable_training;                      /* 1: also build the data-gradient packs and size the arena for
                                               ctta_unet_forward_train + ctta_unet_backward */
} ctta_unet_config;

typedef struct ctta_unet ctta_unet;

/* LoRA: a weight table that names adapter tensors (`...attn{1,2}.processor.to_{q,k,v,out}_lora.{down,up}.weight`, diffusers
 * LoRAAttnProcessor) gives the handle adapters at every attention projection, y = W x + scale * up(down(x)); the rank
 * (1..16) is read from their shapes, and a table that lacks one of an attention's eight tensors fails with that key named.
 * The adapters are a separately reloadable part of the handle: ctta_unet_load_weights repacks them with the rest,
 * ctta_unet_load_adapters repacks them alone (an optimizer / EMA step on the adapters, a swap of one adapter set for another
 * on a serving handle).  `scale` and the choice of kernels are per-handle settings (ctta_unet_set_lora; defaults: the fused
 * site kernels of csrc/lora.hip in the backward where they take the shapes -- rank <= 4 -- and scale 1).  In ctta_unet_backward*, a gradient
 * table that names adapter tensors only is the frozen-base mode: no base weight gradient is formed.  A handle without
 * adapters runs what it always ran. */
ctta_status ctta_unet_create(const ctta_unet_config* cfg, const ctta_tensor* weights,
                             int n_weights, void* stream, ctta_unet** out);
void ctta_unet_destroy(ctta_unet* h);
/* Re-reads (re-packs) all weights from a new table, e.g. after an optimizer/EMA step. */
ctta_status ctta_unet_load_weights(ctta_unet* h, const ctta_tensor* weights, int n_weights,
                                   void* stream);
/* Re-packs the adapter tensors only: names without `_lora.` are ignored and every base pack stays as it is; the text cache
 * is dropped (the cached K / V^T hold the adapter term).  Fails with the key named when one of an attention's eight
 * tensors is missing, and when the handle has no adapters or a tensor's rank differs from the handle's. */
ctta_status ctta_unet_load_adapters(ctta_unet* h, const ctta_tensor* weights, int n_weights, void* stream);
/* Per-handle adapter settings, read by the next ctta_unet_forward / _forward_train (a backward uses the values of the
 * forward_train it belongs to).  `fused` selects, per pass, one ctta_lora_sites_* launch per group of sites on one input
 * where ctta_lora_sites_supported says so: bit 0 the backward groups, bit 1 the forward groups; 0: the per-site launches
 * everywhere.  Forward and data gradients are bit-identical either way; the adapter weight gradients differ in their
 * summation order only.  A change of `scale` drops the text cache.  Defaults (1, 1.0f): the fused backward measured 3.4x
 * faster than its launches, the fused forward slower than its own (profiles/lora_step.txt), so it is opt-in (fused = 3). */
ctta_status ctta_unet_set_lora(ctta_unet* h, int fused, float scale);
/* Per-request adapters: one batch, a different adapter (and strength) per row.  diffusers' LoRAAttnProcessor carries one
 * adapter set and takes one `scale` per call (attention_processor.py:508-613, `__call__(..., scale=)`); a server that offers
 * several fine-tunes of one base checkpoint wants both per row, with the base GEMMs shared by the whole batch.
 *   ctta_unet_adapter_bank     : gives a handle with adapters (created from a table that named some) a zero-filled bank of
 *       `slots` in [1, 64] adapter sets: per site A [slots][r][k_pad] and B [slots][n_pad][r] beside the handle's own pair.
 *       Once per handle -- a second call with the same count changes nothing, with another count it fails -- and freed with
 *       the handle.  A slot that was never loaded is all zeros and behaves as the base model.
 *   ctta_unet_load_adapter_slot: packs one adapter set into one slot through the site maps of the handle's own adapters.  The
 *       rules of ctta_unet_load_adapters: names without `_lora.` are ignored, a missing tensor of an attention's eight is
 *       named, a rank other than the handle's fails.  Neither the handle's own adapters nor any base pack is touched; the
 *       text cache is dropped.
 *   ctta_unet_set_adapter_rows : binds DEVICE arrays of at least `batch` entries (of every later forward): slot_of_sample
 *       int32 -- a slot of the bank, or -1 (any value outside the bank) for the base model -- and scale_of_sample float, or
 *       NULL: every row takes the handle's scale (ctta_unet_set_lora).  The caller keeps the arrays alive; their CONTENTS are
 *       read when the kernels run, so a captured graph serves another mapping on its next replay without being recorded
 *       again.  slot_of_sample NULL unbinds: the handle is back on its single-adapter path, launch for launch.  Binding,
 *       rebinding and unbinding drop the text cache.  The cache holds K / V^T WITH the rows' adapter terms: a caller that
 *       rewrites the arrays' contents between two forwards must not ask for ctta_unet_reuse_text across that change (the
 *       handle cannot see the rewrite).
 * With rows bound, ctta_unet_forward runs the per-site ctta_lora_*_rows launches at every site (whatever bit 1 of `fused`
 * says; there is no fused rows form), the handle's own adapters are not applied, and ctta_unet_forward_train fails: training
 * mixes no adapters. */
ctta_status ctta_unet_adapter_bank(ctta_unet* h, int slots, void* stream);
ctta_status ctta_unet_load_adapter_slot(ctta_unet* h, int slot, const ctta_tensor* weights, int n_weights, void* stream);
ctta_status ctta_unet_set_adapter_rows(ctta_unet* h, const int32_t* slot_of_sample, const float* scale_of_sample);
/* sample (B,C,H,W) f32; timesteps (B) f32; guidance (B) f64 or NULL when !guided;
 * enc (B,L,X) f32; mask (B,L) u8 (1 = keep) or NULL; out (B,Cout,H,W) f32. */
/* One-shot hint for the NEXT ctta_unet_forward / _forward_train on this handle: reuse != 0 promises that its
 * encoder_hidden_states and encoder_attention_mask (and batch / text_len) are those of the previous forward on the handle,
 * so the cross-attention K / V projections of the text states (attention_processor.py:1107-1111: `to_k` / `to_v` of
 * encoder_hidden_states, 32 small GEMMs per forward) are taken from the handle's text cache instead of recomputed -- the
 * second CFG teacher query of a distillation step, every query of a Heun teacher loop.  Ignored when nothing valid is cached
 * (first forward, other batch / length, after ctta_unet_load_weights).  Results are bit-identical either way. */
ctta_status ctta_unet_reuse_text(ctta_unet* h, int reuse);
ctta_status ctta_unet_forward(ctta_unet* h, const float* sample, const float* timesteps,
                              const double* guidance, const float* enc, const uint8_t* mask,
                              int batch, int text_len, float* out, void* stream);
size_t ctta_unet_arena_bytes(const ctta_unet* h);
/* Distillation step (train.py:332-346: loss = model(...); accelerator.backward(loss)).
 * forward_train = forward that keeps every activation the backward pass needs; backward takes
 * dL/d(out) as NHWC bf16 [B][H*W][8] (ctta_snr_mse_grad writes exactly that) and ACCUMULATES
 * dL/d(param) into `grads`: fp32 tensors with the names / shapes of the state dict (`.grad`
 * semantics; guidance_proj.weight has requires_grad=False in the reference and gets none). */
ctta_status ctta_unet_forward_train(ctta_unet* h, const float* sample, const float* timesteps,
                                    const double* guidance, const float* enc, const uint8_t* mask,
                                    int batch, int text_len, float* out, void* stream);
ctta_status ctta_unet_backward(ctta_unet* h, const void* dout_nhwc, const ctta_tensor* grads,
                               int n_grads, void* stream);
/* The same backward pass, resumable block by block, so that the data-parallel all-reduce of a finished
 * block's gradients (accelerate/DDP's bucketed all-reduce, train.py:377-379) overlaps with the remaining
 * backward work: `begin` finishes block 2n+2 (conv_norm_out, conv_out); every `next` finishes one more
 * block and reports its id -- n+2+i = up_blocks.i, n+1 = mid_block, 1+i = down_blocks.i, 0 = conv_in +
 * time/guidance embedding MLPs (last, *finished = 1). */
ctta_status ctta_unet_backward_begin(ctta_unet* h, const void* dout_nhwc, const ctta_tensor* grads,
                                     int n_grads, void* stream);
ctta_status ctta_unet_backward_next(ctta_unet* h, const ctta_tensor* grads, int n_grads, void* stream,
                                    int* block_done, int* finished);
/* Debug taps (only when cfg.debug_taps): named NCHW fp32 copies of intermediates. */
int ctta_unet_num_taps(const ctta_unet* h);
ctta_status ctta_unet_tap_info(const ctta_unet* h, int i, const char** name, int dims[4]);
ctta_status ctta_unet_tap_read(ctta_unet* h, int i, float* dst_nchw, void* stream);

/* ------------------------------------------------------------------------------------ *
 * VAE decoder + vocoder.  Replaces AutoencoderKL.decode_first_stage
 * (audioldm/variational_autoencoder/autoencoder.py:103-106 -> Decoder.forward
 * modules.py:650-683) and AutoencoderKL.decode_to_waveform (autoencoder.py:108-111 ->
 * vocoder_infer hifigan/utilities.py:76-91 -> Generator.forward hifigan/models.py:101-117).
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int z_channels, embed_dim, ch, out_ch, n_levels, num_res_blocks;
  int ch_mult[CTTA_MAX_LEVELS];
  float scale_factor;
  int max_batch, latent_h, latent_w;
  int debug_taps;
  int enable_grad;   /* 1: also build the data-gradient packs and size the arena for
                        ctta_vae_decode_with_grad + ctta_vae_decode_backward (decoder only);
                        2: the differentiable forward also keeps every convolution's input, and
                        ctta_vae_decode_backward_params forms the parameter gradients too */
} ctta_vae_config;

typedef struct ctta_vae ctta_vae;
ctta_status ctta_vae_create(const ctta_vae_config* cfg, const ctta_tensor* weights,
                            int n_weights, void* stream, ctta_vae** out);
void ctta_vae_destroy(ctta_vae* h);
/* z (B,zc,T,F) f32 -> mel (B,out_ch,4T,4F) f32 */
ctta_status ctta_vae_decode(ctta_vae* h, const float* z, int batch, float* mel, void* stream);
/* decode_first_stage(z, allow_grad=True) (autoencoder.py:103-106 as called by CLAPLoss, tools/losses.py:294-296):
 * the same decode, keeping what the input gradient needs; ctta_vae_decode_backward then turns d loss / d mel
 * (B,1,4T,4F) f32 into d loss / d z (B,zc,T,F) f32 -- the decoder is frozen, no parameter gradients.  One forward
 * may be pending per handle; the backward consumes it.  Requires cfg.enable_grad. */
ctta_status ctta_vae_decode_with_grad(ctta_vae* h, const float* z, int batch, float* mel, void* stream);
ctta_status ctta_vae_decode_backward(ctta_vae* h, const float* grad_mel, int batch, float* grad_z, void* stream);
/* Fine-tuning the decoder (AudioLCM_FTVAE): on a handle created with enable_grad = 2 the same backward also ACCUMULATES
 * d loss / d parameter into `grads`, fp32 tensors with the state dict's names and shapes (`.grad` semantics, as
 * ctta_unet_backward): every decoder.* and post_quant_conv.* key.  grad_z may be NULL.  Consumes the pending forward. */
ctta_status ctta_vae_decode_backward_params(ctta_vae* h, const float* grad_mel, int batch, float* grad_z,
                                            const ctta_tensor* grads, int n_grads, void* stream);
/* a new state dict into an existing handle (forward packs, data-gradient packs, conv_out's fp32 taps), e.g. after an
 * optimizer step on the decoder; a pending differentiable forward is dropped */
ctta_status ctta_vae_load_weights(ctta_vae* h, const ctta_tensor* weights, int n_weights, void* stream);
size_t ctta_vae_arena_bytes(const ctta_vae* h);
int ctta_vae_num_taps(const ctta_vae* h);
ctta_status ctta_vae_tap_info(const ctta_vae* h, int i, const char** name, int dims[4]);
ctta_status ctta_vae_tap_read(ctta_vae* h, int i, float* dst_nchw, void* stream);

#define CTTA_MAX_UPS 8
/* VAE encoder: AutoencoderKL.encode_first_stage (autoencoder.py:80-89 -> Encoder.forward modules.py:519-543 +
 * quant_conv), the training-side latent encoder of tools/train_utils.py:155-162.  Same ctta_vae_config as the decoder
 * (out_ch = the mel's channel count 1; latent_h/_w = the LATENT extent, the mel is 2^(n_levels-1) times larger).
 * mel (B,1,T,F) f32 -> moments (B, 2*embed_dim, T/s, F/s) f32 = [mean | logvar] of the diagonal Gaussian posterior;
 * sampling (DiagonalGaussianDistribution.sample, distributions.py:37-41) stays with the caller's RNG. */
typedef struct ctta_vae_encoder ctta_vae_encoder;
ctta_status ctta_vae_encoder_create(const ctta_vae_config* cfg, const ctta_tensor* weights, int n_weights,
                                    void* stream, ctta_vae_encoder** out);
void ctta_vae_encoder_destroy(ctta_vae_encoder* h);
ctta_status ctta_vae_encoder_load_weights(ctta_vae_encoder* h, const ctta_tensor* weights, int n_weights,
                                          void* stream);
ctta_status ctta_vae_encode(ctta_vae_encoder* h, const float* mel, int batch, float* moments, void* stream);
int ctta_vae_encoder_num_taps(const ctta_vae_encoder* h);
ctta_status ctta_vae_encoder_tap_info(const ctta_vae_encoder* h, int i, const char** name, int dims[4]);
ctta_status ctta_vae_encoder_tap_read(ctta_vae_encoder* h, int i, float* dst_nchw, void* stream);

/* Waveform -> log-mel front-end of the training step: tools/torch_tools.py:126-135 (wav_to_fbank) with
 * audioldm/audio/stft.py:132-186 (TacotronSTFT: reflect pad, conv1d STFT at hop `hop_length`, magnitude, mel
 * filterbank (librosa.filters.mel, Slaney scale / area norm), log(clamp(x, 1e-5))) and torch_tools.py:38-51 (_pad_spec).
 * wav (B, n_samples) f32 (clipped to [-1, 1], NaN -> 0 like get_mel_from_wav) -> fbank (B, target_length, n_mels) f32
 * and, when logmag != NULL, the log-magnitude spectrogram (B, target_length, filter_length/2) f32.  Frames past
 * n_samples/hop + 1 are zero (not log(1e-5)), exactly as the reference pads. */
typedef struct ctta_mel_frontend ctta_mel_frontend;
ctta_status ctta_mel_frontend_create(int filter_length, int hop_length, int win_length, int n_mels,
                                     int sampling_rate, float mel_fmin, float mel_fmax, int max_batch,
                                     int max_samples, ctta_mel_frontend** out);
void ctta_mel_frontend_destroy(ctta_mel_frontend* h);
ctta_status ctta_wav_to_fbank(ctta_mel_frontend* h, const float* wav, int batch, int n_samples,
                              int target_length, float* fbank, float* logmag, void* stream);

/* Mix augmentation of the training batch (csrc/mix_augment.hip).  The handle owns the fp32 periodic-Hann, twiddle and
 * A-weight tables (computed on the host in float64, uploaded once) and a workspace for max_clips clips of up to
 * max_samples samples and max_pairs pairs.  fs is 16000 (n_fft 2048) or 44100 (n_fft 4096), anything else is
 * CTTA_ERR_INVALID (tools/mix.py:19-24 raises); mode 0 = "A_weighting", 1 = "RMSE".  Calls on one handle must not overlap.
 * ctta_mixer_frames: frames of a clip, (n_samples - n_fft) / (n_fft / 2) + 1 (0 when shorter than n_fft).
 * ctta_mixer_gain_db replaces tools/mix.py:18-43 (compute_gain) for n_clips clips at once: wav [n_clips][ld] f32 ->
 * gain_db [n_clips][frames] f32, 10 log10(max(E, 10^(min_db/10))) per frame (no padding, partial tail dropped).
 * ctta_mixer_mix replaces tools/torch_tools.py:117-123 over tools/mix.py:46-51 (mix at ratio r): for pair p with clip indices
 * pairs[2p], pairs[2p+1] (DEVICE int32, read by the kernel: a captured graph takes new pairs) the mixture
 * (s1 t + s2 (1 - t)) / sqrt(t^2 + (1 - t)^2), t = 1 / (1 + 10^((g1 - g2)/20) (1 - r)/r) with g the clip's maximum frame
 * gain, is written to dst row dst_row0 + p.  n_groups > 0 splits the pairs into that many equal consecutive groups and
 * divides each group by its own max |.|, then by 2 (torch_tools.py:121, one collate per group; an all-silent group is
 * 0/0 = NaN as in the reference); n_groups = 0 leaves the mixtures unnormalised (mix.py's mix).  t_out [n_pairs] and
 * g_out [n_pairs][2] (f32, may be NULL) receive t and (g1, g2).  A pair index outside [0, n_clips) gives a NaN row.
 * dst rows must not overlap the source rows.  Three launches, no host synchronisation, deterministic. */
typedef struct ctta_mixer ctta_mixer;
ctta_status ctta_mixer_create(int fs, int mode, float min_db, int max_clips, int max_samples, int max_pairs,
                              ctta_mixer** out);
void ctta_mixer_destroy(ctta_mixer* h);
int ctta_mixer_frames(const ctta_mixer* h, int n_samples);
ctta_status ctta_mixer_gain_db(ctta_mixer* h, const float* wav, int n_clips, int n_samples, int64_t ld, float* gain_db,
                               void* stream);
ctta_status ctta_mixer_mix(ctta_mixer* h, const float* wav, int n_clips, int n_samples, int64_t ld, const int32_t* pairs,
                           int n_pairs, int n_groups, double r, float* dst, int64_t dst_ld, int dst_row0, float* t_out,
                           float* g_out, void* stream);

/* ------------------------------------------------------------------------------------ *
 * Text encoder.  Replaces `self.text_encoder(input_ids=, attention_mask=)[0]` of
 * models/audio_distilled_model.py:208-214 (transformers T5EncoderModel, FLAN-T5-large; weights in the
 * T5EncoderModel state-dict layout: shared.weight, encoder.block.N.layer.{0.SelfAttention.{q,k,v,o},
 * 0.layer_norm, 1.DenseReluDense.{wi_0,wi_1,wo}, 1.layer_norm}.weight, block 0's relative_attention_bias,
 * encoder.final_layer_norm.weight).  gated-gelu feed-forward, d_kv = 64.
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int vocab_size, d_model, d_kv, d_ff, num_layers, num_heads;
  int rel_buckets, rel_max_distance;   /* relative_attention_num_buckets / _max_distance */
  float eps;                           /* layer_norm_epsilon */
  int max_batch, max_len;              /* arena sizing */
} ctta_t5_config;
typedef struct ctta_t5 ctta_t5;
ctta_status ctta_t5_create(const ctta_t5_config* cfg, const ctta_tensor* weights, int n_weights, void* stream,
                           ctta_t5** out);
void ctta_t5_destroy(ctta_t5* h);
/* input_ids (B, L) int64, attention_mask (B, L) uint8 (1 = token, 0 = padding; every row needs one token)
 * -> last_hidden_state (B, L, d_model) f32 */
ctta_status ctta_t5_encode(ctta_t5* h, const int64_t* input_ids, const uint8_t* attention_mask, int batch, int len,
                           float* last_hidden_state, void* stream);
size_t ctta_t5_arena_bytes(const ctta_t5* h);

typedef struct {
  int num_mels, upsample_initial_channel, n_ups, n_kernels;
  int upsample_rates[CTTA_MAX_UPS], upsample_kernel_sizes[CTTA_MAX_UPS];
  int resblock_kernel_sizes[4];
  int resblock_dilations[4][3];
  int max_batch, max_frames;
  int debug_taps;
  int enable_grad;   /* 1: ctta_hifigan_forward_with_grad + ctta_hifigan_backward are available */
} ctta_hifigan_config;

typedef struct ctta_hifigan ctta_hifigan;
ctta_status ctta_hifigan_create(const ctta_hifigan_config* cfg, const ctta_tensor* weights,
                                int n_weights, void* stream, ctta_hifigan** out);
void ctta_hifigan_destroy(ctta_hifigan* h);
int64_t ctta_hifigan_out_len(const ctta_hifigan* h, int frames);
/* mel (B,frames,num_mels) f32 (== (B,1,T,F) NCHW mel) -> wav (B,out_len) f32 in (-1,1),
 * BEFORE the reference's batch-global centring. */
ctta_status ctta_hifigan_forward(ctta_hifigan* h, const float* mel, int batch, int frames,
                                 float* wav, void* stream);
/* vocoder_infer(..., allow_grad=True) (hifigan/utilities.py:79-81): the same forward keeping every LeakyReLU mask;
 * ctta_hifigan_backward turns d loss / d wav (B,out_len) f32 (`wav` = the forward's output, for tanh') into
 * d loss / d mel (B,frames,num_mels) f32.  The generator is frozen.  Requires cfg.enable_grad. */
ctta_status ctta_hifigan_forward_with_grad(ctta_hifigan* h, const float* mel, int batch, int frames, float* wav,
                                           void* stream);
ctta_status ctta_hifigan_backward(ctta_hifigan* h, const float* grad_wav, const float* wav, int batch, int frames,
                                  float* grad_mel, void* stream);
/* vocoder_infer post-processing (utilities.py:83-86): wav -= (max+min)/2 over the WHOLE
 * batch, *32768, truncation to int16.  `scratch` >= 2 floats of device memory.
 * centred (float, may be NULL) and pcm (int16, may be NULL) receive the results. */
ctta_status ctta_wav_finalize(const float* wav, int64_t n, float* scratch, float* centred,
                              int16_t* pcm, void* stream);
/* The same in two halves for a batch SHARDED over ranks: the centring uses the extrema of the whole batch
 * (hifigan/utilities.py:85 `(wavs.max() + wavs.min()) / 2` on the full tensor), so every rank computes its local
 * (max, min) -> max_min[2] (device floats), the caller MAX-reduces (max, -min) over ranks (dist_util.global_wav_extrema_),
 * and ctta_wav_center applies the reduced pair.  scratch >= 2 floats. */
ctta_status ctta_wav_extrema(const float* wav, int64_t n, float* scratch, float* max_min, void* stream);
ctta_status ctta_wav_center(const float* wav, int64_t n, const float* max_min, float* scratch, float* centred,
                            int16_t* pcm, void* stream);
size_t ctta_hifigan_arena_bytes(const ctta_hifigan* h);
int ctta_hifigan_num_taps(const ctta_hifigan* h);
ctta_status ctta_hifigan_tap_info(const ctta_hifigan* h, int i, const char** name, int dims[4]);
ctta_status ctta_hifigan_tap_read(ctta_hifigan* h, int i, float* dst_ncl, void* stream);

/* ------------------------------------------------------------------------------------ *
 * Heun solver elementwise steps with PER-SAMPLE sigmas.  Replace
 * HeunDiscreteScheduler.{scale_model_input,add_noise,step}
 * (diffusers/schedulers/scheduling_heun_discrete.py:151-172,364-385,273-362), v-prediction.
 * x etc. are (B, n_per_sample) f32; sigma arrays are (B) f32 on device.
 * ------------------------------------------------------------------------------------ */
ctta_status ctta_heun_scale_model_input(const float* x, const float* sigma, float* out,
                                        int batch, int64_t n_per_sample, void* stream);
ctta_status ctta_heun_add_noise(const float* x0, const float* noise, const float* sigma,
                                float* out, int batch, int64_t n_per_sample, void* stream);
/* 1st-order half: prev = x + d*(sigma_next-sigma), d = (x - x0_hat)/sigma; writes d. */
ctta_status ctta_heun_step_first(const float* v, const float* x, const float* sigma,
                                 const float* sigma_next, float* prev, float* deriv,
                                 int batch, int64_t n_per_sample, void* stream);
/* 2nd-order half: d2 at (x_hat, sigma_next); prev = x_stored + (d_prev+d2)/2*(sigma_next-sigma) */
ctta_status ctta_heun_step_second(const float* v, const float* x_hat, const float* x_stored,
                                  const float* deriv_prev, const float* sigma,
                                  const float* sigma_next, float* prev, int batch,
                                  int64_t n_per_sample, void* stream);
/* AudioDistilledModel._query_teacher CFG combine (models/audio_distilled_model.py:313-319):
 * out = (1-w)*uncond + w*cond, per-sample w (B) f32. */
ctta_status ctta_cfg_combine(const float* uncond, const float* cond, const float* w, float* out,
                             int batch, int64_t n_per_sample, void* stream);
/* One sampler step between two U-Net queries of the few-step consistency sampler
 * (easy_inference/consistencytta.py:152-197; scheduling_heun_discrete.py:151-172,364-385) in one pass over (B, n) f32:
 *   x0  = uncond == NULL ? cond : (1 - w_post[b]) * uncond + w_post[b] * cond      (post-CFG combine)
 *   z   = x0 + noise * sigma[b]                                                    (add_noise)
 *   out = z / sqrt(sigma[b]^2 + 1)                                                 (scale_model_input)
 * `out` holds copies * B rows: the result is written `copies` (1 or 2) times, stacked along the batch (the 2B-row input of
 * a CFG query).  sigma and w_post are (B) f32 on device; w_post may be NULL when uncond is.  Bit-identical to torch's
 * (1 - w) * u + w * c, then ctta_heun_add_noise, then ctta_heun_scale_model_input, then a concatenation. */
ctta_status ctta_consistency_renoise(const float* cond, const float* uncond, const float* w_post, const float* noise,
                                     const float* sigma, float* out, int copies, int batch, int64_t n_per_sample,
                                     void* stream);
/* The same step with a source clip: the masked sampler of audioldm/ldm.py:718-805, whose step ends with
 * img = img_orig * mask + (1 - mask) * img (audioldm/latent_diffusion/ddim.py:210-216), in the few-step consistency
 * sampler's terms -- the known region is blended into x0 between two queries.  One pass over (B, n) f32:
 *   x0  = uncond == NULL ? cond : (1 - w_post[b]) * uncond + w_post[b] * cond      (as ctta_consistency_renoise)
 *   x0  = keep[b, p] * src + (1 - keep[b, p]) * x0                                 (ddim.py:216; p = position in the plane)
 *   z   = x0 + noise * sigma[b];   out = z / sqrt(sigma[b]^2 + 1)                  (written `copies` = 1 or 2 times)
 * keep is (B, hw) f32, 1 = keep the source (ldm.py:764-768), shared by the n_per_sample / hw channels of a row; hw % 4 == 0
 * and n_per_sample % hw == 0.  src is (B, n); src and keep are both required.  cond == NULL (then uncond must be NULL too)
 * means x0 = 0 before the blend: the sampler's start, where keep * src plus noise is the first input.  Bit-identical to
 * torch's (1 - w) * u + w * c, torch's keep * src + (1 - keep) * x0, ctta_heun_add_noise, ctta_heun_scale_model_input
 * and a concatenation.
 * ctta_cfg_combine_keep: the last query's post-CFG combine (uncond may be NULL: out is the blend of cond) and the same
 * blend, without the re-noising. */
ctta_status ctta_consistency_edit_renoise(const float* cond, const float* uncond, const float* w_post, const float* src,
                                          const float* keep, const float* noise, const float* sigma, float* out,
                                          int copies, int batch, int64_t n_per_sample, int64_t hw, void* stream);
ctta_status ctta_cfg_combine_keep(const float* uncond, const float* cond, const float* w, const float* src,
                                  const float* keep, float* out, int batch, int64_t n_per_sample, int64_t hw, void* stream);
/* The same step for a clip longer than the student's window (the `duration` of audioldm/pipeline.py:49-50,94-95 in the
 * few-step sampler's terms): the student is queried on n_windows overlapping windows of window_h rows of ONE long latent of
 * latent_h rows, as rows of one batch, and between two queries the windows' x0 estimates are fused into one long x0,
 * re-noised with one long draw and cut into the next windows.  cond / uncond are (batch * n_windows, C, window_h, W), row
 * b * n_windows + k; noise and x0_long are (batch, C, latent_h, W); out is (copies * batch * n_windows, C, window_h, W), the
 * same row order stacked `copies` (1 or 2) times.  Per long element (b, c, h, x), over the windows k that cover row h
 * (starts[k] <= h < starts[k] + window_h), in ascending k, every multiply and every add rounded on its own:
 *   x_k = uncond == NULL ? cond : (1 - w_post[b]) * uncond + w_post[b] * cond      (as ctta_consistency_renoise)
 *   acc = weights[k0][h - starts[k0]] * x_k0;   acc = acc + weights[k][h - starts[k]] * x_k   (k > k0)
 *   z   = acc + noise * sigma[b];   o = z / sqrt(sigma[b]^2 + 1)
 * and o is written to out at (b * n_windows + k, c, h - starts[k], x) for every covering k and every copy; acc is written
 * to x0_long when that is given.  One pass over the long elements: every window element is written exactly once.
 * starts is a HOST array of n_windows (<= 16) int32, copied into the launch arguments: it begins with 0, ends with
 * latent_h - window_h, increases strictly and leaves no gap (starts[k + 1] <= starts[k] + window_h).  weights is
 * (n_windows, window_h) f32 on the device; sigma and w_post are (batch) f32 on the device; width % 4 == 0.
 * cond == NULL (then uncond must be NULL too) means x0 = 0: the sampler's start, pure noise cut into windows.
 * noise == NULL and out == NULL together: the sampler's end, only x0_long (then required) is written.  uncond and w_post
 * are given together or not at all. */
ctta_status ctta_window_fuse_renoise(const float* cond, const float* uncond, const float* w_post, const int32_t* starts,
                                     const float* weights, const float* noise, const float* sigma, float* x0_long,
                                     float* out, int copies, int batch, int n_windows, int channels, int window_h,
                                     int latent_h, int width, void* stream);
/* ctta_window_fuse_renoise with a long source clip: the masked sampler's blend (audioldm/ldm.py:718-805, ddim.py:210-216)
 * on the fused x0 of a clip of another `duration` (pipeline.py:49-50,94-95).  Every layout and rule of
 * ctta_window_fuse_renoise carries over; src_long is (batch, C, latent_h, W) f32 and keep is (batch, latent_h * W) f32, one
 * plane per clip shared by its channels, 1 = keep the source, fractions allowed; both are required.  Per long element
 * (b, c, h, x), every multiply and every add rounded on its own:
 *   acc = the weighted overlap-add of ctta_window_fuse_renoise      (cond == NULL: every x_k = 0)
 *   x0  = keep[b][h * W + x] * src_long + (1 - keep[b][h * W + x]) * acc            (torch's mul, rsub, mul, add)
 *   z   = x0 + noise * sigma[b];   o = z / sqrt(sigma[b]^2 + 1)
 * o goes to out at every covering window and every copy, x0 to x0_long when that is given.  cond == NULL is the sampler's
 * start, keep * src plus noise cut into windows; noise == NULL and out == NULL together is its end, only x0_long (then
 * required) is written.  One window of latent_h == window_h rows is ctta_consistency_edit_renoise / ctta_cfg_combine_keep
 * bit for bit; keep == 0 with a finite source is ctta_window_fuse_renoise up to the sign of a zero. */
ctta_status ctta_window_fuse_edit_renoise(const float* cond, const float* uncond, const float* w_post,
                                          const int32_t* starts, const float* weights, const float* src_long,
                                          const float* keep, const float* noise, const float* sigma, float* x0_long,
                                          float* out, int copies, int batch, int n_windows, int channels, int window_h,
                                          int latent_h, int width, void* stream);
/* Seeded sampler noise: what torch.randn at easy_inference/consistencytta.py's noise draw becomes when a request carries
 * a seed.  Philox4x32-10 as published (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), one
 * block per four consecutive w of a (C, H, W) latent:
 *   q       = (h * C + c) * W + w                      (rows are the OUTER index: H rows are the first H of a taller draw)
 *   key     = (seed & 0xffffffff, seed >> 32)          (seed: the request's int64 taken as uint64)
 *   counter = (q >> 2, d, m, 0)                        (d: draw index, m: sample index, 0: domain tag "sampler noise")
 * and the block's words x0..x3 serve q & 3 = 0..3.  With u(x) = ((x >> 9) + 0.5) * 2^-23 and r(x) = sqrtf(-2 logf(u(x))):
 *   z0 = r(x0) * cos(2 pi u(x1)),  z1 = r(x0) * sin(2 pi u(x1)),  z2 = r(x2) * cos(2 pi u(x3)),  z3 = r(x2) * sin(2 pi u(x3))
 * the angle through sincospif(2 u) (2 u is exact in fp32), no fast-math intrinsic; |z| <= sqrt(-2 ln 2^-24) = 5.768.
 * seeds is (batch) int64 and samples (batch) int32 (NULL: all zeros), both on the DEVICE and read when the kernel runs: a
 * captured launch picks up what the buffers hold at replay.  out is (draws, batch, C, H, W) and holds the draws
 * d = draw0 .. draw0 + draws - 1 of every row, in ONE launch; ctta_philox_normal writes scale * z (f32, the product
 * rounded on its own), ctta_philox_words the raw words.  Refused before any launch: width % 4 != 0, a non-positive extent,
 * draw0 < 0, C * H * W >= 2^34 (q >> 2 is a 32-bit counter word), seeds or out NULL. */
ctta_status ctta_philox_normal(const int64_t* seeds, const int32_t* samples, int batch, int draw0, int draws, int channels,
                               int height, int width, float scale, float* out, void* stream);
ctta_status ctta_philox_words(const int64_t* seeds, const int32_t* samples, int batch, int draw0, int draws, int channels,
                              int height, int width, int32_t* out, void* stream);
/* get_loss with MSELoss('instance') and SNR clamp (models/audio_consistency_model.py:250-266,
 * tools/losses.py:28-33): loss = mean_b( mean((pred-target)^2) * min(sigma^-2, gamma) ).
 * gamma <= 0 disables the weighting.  loss: 1 float on device. */
ctta_status ctta_snr_mse_loss(const float* pred, const float* target, const float* sigma,
                              float gamma, float* per_instance, float* loss, int batch,
                              int64_t n_per_sample, void* stream);
/* Stage-1 guided distillation pieces: per-sample linear combination out = a[b]*x + b[b]*y
 * (optionally clamped to [-clamp, clamp]) -- DDPMScheduler/DDIMScheduler.add_noise (scheduling_ddpm.py:420-443) and the
 * v-prediction terms of DDIMScheduler.step (scheduling_ddim.py:243-370) -- and the MSE with explicit per-instance weights
 * of AudioGDM.forward's get_loss (models/audio_guided_model.py:92-117). */
ctta_status ctta_lincomb2_rows(const float* x, const float* y, const float* a, const float* b, float* out,
                               int batch, int64_t n_per_sample, float clamp, void* stream);
/* The DDIM solver of stage-2 consistency distillation (AudioLCM with use_edm=False, models/audio_consistency_model.py:
 * 72-75,313-340) as one-pass primitives with PER-SAMPLE coefficients ((B) f32 on device: sqrt(alphas_cumprod[t]),
 * sqrt(1 - alphas_cumprod[t]) and the same two at the previous timestep).
 * ctta_ddim_step: DDIMScheduler.step with eta = 0 (diffusers/schedulers/scheduling_ddim.py:243-370, batched timesteps):
 *   x0 = sqrt_a_t * sample - sqrt_1m_a_t * v            (v_prediction, :310-314)
 *   x0 = (sample - sqrt_1m_a_t * v) / sqrt_a_t          (epsilon, :305-306; as (1/sqrt_a_t) * sample + (-sqrt_1m_a_t/sqrt_a_t) * v)
 *   x0 clamped to [-clamp, clamp] when clamp > 0 (:321-324); eps = sqrt_a_t * v + sqrt_1m_a_t * sample (v_prediction) or v;
 *   prev_sample = sqrt_a_prev * x0 + sqrt_1m_a_prev * eps (:345-349).
 * model_output is (B, n_per_sample) when cfg_w is NULL; otherwise (2B, n_per_sample) = [uncond | cond] and
 * v = (1 - cfg_w[b]) * uncond + cfg_w[b] * cond first (models/audio_distilled_model.py:313-319).  pred_original_sample may be
 * NULL.  Bit-identical to ctta_cfg_combine followed by three ctta_lincomb2_rows (the chain DDIMScheduler.step launches).
 * ctta_ddim_noising: DDIMScheduler.add_noise (:372-393) with the last-step select of the distillation step
 * (models/audio_consistency_model.py:312-319): out = last[b] != 0 ? noise * init_sigma : sqrt_a * x0 + sqrt_1m_a * noise;
 * last (B) f32 may be NULL (plain add_noise). */
enum { CTTA_DDIM_V_PREDICTION = 0, CTTA_DDIM_EPSILON = 1 };
ctta_status ctta_ddim_step(const float* model_output, const float* cfg_w, const float* sample, const float* sqrt_a_t,
                           const float* sqrt_1m_a_t, const float* sqrt_a_prev, const float* sqrt_1m_a_prev,
                           int prediction_type, float clamp, float* prev_sample, float* pred_original_sample,
                           int batch, int64_t n_per_sample, void* stream);
ctta_status ctta_ddim_noising(const float* x0, const float* noise, const float* sqrt_a, const float* sqrt_1m_a,
                              const float* last, float init_sigma, float* out, int batch, int64_t n_per_sample,
                              void* stream);
ctta_status ctta_weighted_mse_loss(const float* pred, const float* target, const float* weights,
                                   float* per_instance, float* loss, int batch, int64_t n_per_sample,
                                   void* stream);
ctta_status ctta_weighted_mse_grad(const float* pred, const float* target, const float* weights, float loss_scale,
                                   int batch, int c, int hw, int c_pad, void* dpred_nhwc, void* stream);

/* ------------------------------------------------------------------------------------ *
 * Fused two-shadow EMA.  Replaces do_ema_update (tools/train_utils.py:255-282) as called by
 * AudioLCM.update_ema (models/audio_consistency_model.py:221-227): for each shadow s_k:
 * s_k += (1-decay_k)*(p - s_k), fp32, in place.  shadow_b/decay_b may be NULL/0.
 * ------------------------------------------------------------------------------------ */
ctta_status ctta_ema_update2(const float* param, float* shadow_a, double decay_a, float* shadow_b,
                             double decay_b, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------ *
 * Operator-level entry points (used by the engines; exported for per-op parity tests and
 * micro-benchmarks).  bf16 tensors are uint16_t bit patterns, NHWC.
 * ------------------------------------------------------------------------------------ */
typedef struct {
  const void* x0; int c0;     /* NHWC bf16 source, channel count (== row stride unless x_stride) */
  const void* x1; int c1;     /* optional second source, concatenated after x0's channels */
  int batch, hi, wi;          /* LOGICAL input extent (after the optional x2 upsample) */
  int upsample;               /* 1: sources are (hi/2, wi/2), nearest-upsampled on the fly */
  int ho, wo;
  int kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
  const void* w;              /* packed bf16 [n_rows >= n][k_pad], k = (kh,kw,c), zero padded */
  int k_pad;                  /* row stride of w, multiple of 64 */
  int n;                      /* valid output channels; multiple of 4 unless the epilogue is
                                 plain (no bias/rowvec/res/accumulate) and round_up(n,4) <= ldc */
  const float* bias;          /* [n] or NULL */
  const float* bias_m;        /* per output ROW (pixel) bias [m] or NULL (transposed products) */
  const float* rowvec; int rowvec_ld;   /* + rowvec[b*ld + n] (time-embedding shift) or NULL */
  const void* res; int res_ld;          /* + res[m*ld + n] bf16 or NULL */
  int in_act;                 /* on the A operand: 0 none, 1 leaky_relu(in_slope) */
  float in_slope;
  int out_act;                /* 0 none, 1 silu, 2 tanh, 3 leaky_relu(out_slope), 4 fused GEGLU (bias only, n % 32 == 0,
                                 out of half the width; out_batch_stride is honoured, out_offset / out_limit are not taken) */
  float out_slope;
  float alpha;                /* v = alpha*(acc + bias + rowvec + res [+ old out]) */
  int accumulate;             /* 1: add the existing output before scaling */
  void* out; int ldc;         /* bf16 (or f32 when out_f32) [m][ldc]; ldc %% 4 != 0 selects
                                 element-wise stores (tiny Cout, bias-only epilogue) */
  int out_f32;
  void* out2; float out2_slope; /* optional 2nd bf16 output = leaky_relu(out, out2_slope), same indexing */
  int64_t out_batch_stride;   /* 0 -> ho*wo*ldc */
  int64_t out_offset;         /* element offset added inside a batch (ConvTranspose remap) */
  int64_t out_limit;          /* >0: store only if 0 <= idx_in_batch < out_limit */
  /* batched GEMM (grid.z): extra strides in elements; 0 = shared */
  int groups; int64_t x_group_stride, w_group_stride, out_group_stride;
  int tile;                   /* 0 = auto; else force a kernel variant id (tuning) */
  int x_stride;               /* 0 -> c0; else row stride of x0 in elements (column slice of a wider matrix) */
  /* GroupNorm statistics of the output from the epilogue (saves GroupNorm's own read pass over the tensor): when
   * gn_part != NULL, gn_groups divides n and gn_hw (rows per sample) divides the row count, every workgroup writes
   * (sum, sum of squares) per channel group of its tile to gn_part [batch][chunks][gn_groups][2] fp32, chunks = gn_hw /
   * tile rows.  Only some launches can do it (plain bf16 output through the wide-store epilogue, whole tiles per sample,
   * no split-K): ctta_conv_last_gn_chunks() tells the caller whether -- and with how many chunks -- it happened.
   * CONTRACT of the partials: they are the sums of the output values in fp32 BEFORE their rounding to bf16 (after alpha and
   * the output activation), i.e. what a GroupNorm computed in fp32 on the unrounded convolution result sees -- not the sums
   * of the stored bf16 numbers, from which they differ by zero-mean rounding noise of 2^-9 relative per element.  Every
   * epilogue code that writes partials (the straight-line waves and the generic column-edge waves of one launch) sums the
   * same quantity; tests/test_conv_forms_gpu.py holds each entry to the float64 sums of it. */
  void* gn_part; int gn_groups; int gn_hw;
  int64_t gn_part_floats;     /* capacity of gn_part; launches whose partials would not fit write none */
} ctta_conv_desc;

ctta_status ctta_conv_gemm(const ctta_conv_desc* d, void* stream);
/* chunks per sample of the GroupNorm partials the calling thread's LAST ctta_conv_gemm wrote (0: none were written) */
int ctta_conv_last_gn_chunks(void);
/* Split-K partial sums (deep, narrow problems: < 192 output tiles and K >= 1024) go through a device workspace.
 * Threading contract: every engine handle (ctta_unet / ctta_vae / ctta_hifigan / ctta_t5 ...) owns its own workspace
 * and binds it to the calling host thread inside each of its entry points, so different handles may run on different
 * streams or host threads concurrently.  A RAW ctta_conv_gemm caller is served from one lazily allocated workspace per
 * device: launches that share it must be ordered on ONE stream -- or the caller binds its own buffer of
 * ctta_conv_workspace_bytes() bytes for the calling thread (NULL unbinds). */
void ctta_conv_bind_workspace(void* ws, size_t bytes);
/* The same with a promise about the workspace's first ctta_conv_workspace_header_bytes() bytes: header_zeroed != 0 says they were
 * zero when the buffer was created and have only been touched by this library since.  Stream-K launches (one persistent
 * launch that folds its partial tiles itself: start tickets, an epoch and one flag word per workgroup live there; the launches
 * leave the header consistent for the next one) are only taken with such a workspace; the engine handles bind theirs this
 * way, ctta_conv_bind_workspace() promises nothing and keeps the two-pass split-K.  The per-device default workspace is
 * created with a zero header. */
void ctta_conv_bind_workspace_ex(void* ws, size_t bytes, int header_zeroed);
int ctta_conv_bound_workspace_header(void);
size_t ctta_conv_workspace_header_bytes(void);
/* The calling thread's current binding (NULL / 0 when none).  Engine / STFT / mel / T5 entry points bind their own
 * handle's workspace while they enqueue work and RESTORE the caller's binding on return (round 3; before, they left the
 * thread unbound and later raw launches silently fell back to the shared per-device workspace). */
void ctta_conv_bound_workspace(void** ws, size_t* bytes);
/* on != 0: launches issued by the calling host thread take no split-K path until switched off again (used for GEMMs that
 * an engine enqueues on a second stream of the same handle, which must not share the handle's partial-sum slabs) */
void ctta_conv_suppress_splitk(int on);
/* Diagnostic: while `buf` is non-NULL every conv_gemm workgroup launched from this host thread writes six 64-bit words
 * {HW_ID register, s_memtime at entry, after the first K-tile landed, after the main loop, after the epilogue's last
 * store was issued, before the first K-tile request} to buf[6 * linear workgroup index] (tools/tile_timeline.py).  buf: >= 48 bytes per workgroup. */
void ctta_conv_debug_stamps(void* buf);
/* Diagnostic: while `buf` is non-NULL the self-attention forward launches of this host thread (no bias, nk % 64 == 0) run an
 * instrumented twin that writes, per workgroup, 4 waves x 64 key tiles x 6 s_memtime stamps (low 32 bits: tile top, after
 * the barrier, after the LDS-DMA issue, after the next tile's scores, after the softmax, after P V) followed by the four
 * waves' HW_ID and XCC_ID registers: (4 * 64 * 6 + 8) 32-bit words per workgroup (tools/attn_timeline.py). */
void ctta_attention_debug_stamps(void* buf);
size_t ctta_conv_workspace_bytes(void);
int ctta_conv_gemm_num_variants(void);
const char* ctta_conv_gemm_variant_name(int id);
/* The PLAN of a ctta_conv_gemm call, without a device: which kernel the dispatch rules pick for descriptor `d` and how they
 * schedule it, in an environment the caller describes.  ctta_conv_gemm launches from the same plan, built from the live
 * process.  Pointers in `d` are only tested against NULL.  Returns the status, and leaves the ctta_last_error() text, that
 * ctta_conv_gemm would give for the descriptor. */
typedef struct {
  int cu_count;                       /* compute units of the device */
  int xcd, splitk, streamk, streamk_grid;   /* values of the options of these names (ctta_get_option) */
  int suppress_splitk;                /* ctta_conv_suppress_splitk is on */
  int stamps_bound;                   /* ctta_conv_debug_stamps has a buffer */
  int64_t workspace_bytes;            /* the split-K workspace the launch would find (bound, or the per-device default); 0: none */
  int workspace_header_zeroed;        /* ... and whether stream-K may use it (ctta_conv_bind_workspace_ex) */
} ctta_conv_plan_env;
typedef struct {
  int variant, kind, halo;            /* tile id (0 with halo), its kind (2: stream-K), 1: the C = 32 conv1d halo kernel */
  int prof_code;                      /* variant code of the launch's profiler record */
  int grid_x, grid_y, grid_z;         /* grid of the (first) launch */
  int splits, nk, nk_split;           /* two-pass split-K factor (1: none), K tiles, K tiles per split */
  int finish_blocks;                  /* workgroups of the split-K second pass */
  int tail_rows, tail_variant;        /* ragged last row tile cut off into a second launch: its rows and tile (0: none) */
  int tail_grid_x, tail_grid_y, tail_nk;
  int xcd_per, m_tiles, n_tiles, n_inner;   /* XCD-aware tile order */
  int slab_total, slab_per;           /* weight-slab affinity */
  int sk_chunks, sk_m_inner;          /* stream-K: XCD chunks, tile order */
  int gn_nchunk;                      /* GroupNorm partial chunks per sample (0: the launch writes none) */
  int plain_out, wide_store, wide_f32, splitk_wide_f32, epi_fast, epi_fast_geglu, epi_act;   /* epilogue flags */
} ctta_conv_plan_info;
ctta_status ctta_conv_plan(const ctta_conv_desc* d, const ctta_conv_plan_env* env, ctta_conv_plan_info* out);
/* The PLAN of one layer's weight gradient in the engines' backward passes, without a device: which of the weight-gradient
 * kernels below runs for a layer geometry, over how many position splits, and what scratch it takes.  ctta_unet_backward* and
 * ctta_vae_decode_backward_params launch from the same plan, each under its own policy (ctta_wgrad_engine_policy). */
typedef struct {
  int kh, kw, c;                      /* taps and input channels (the row stride of x) */
  int batch, hi, wi, upsample;        /* input extent AFTER the x2 nearest upsampling, if any */
  int ho, wo, stride, pad;            /* output extent: dY is [batch * ho * wo][n] */
  int n;                              /* output channels */
  int nb;                             /* per-sample columns behind the bias column (time-embedding gradient); 0: none */
  int direct_ok;                      /* the layer's pack map lets a one-split kernel add into the gradient tensors itself */
  int run_async, keeps_dy;            /* the job runs on a side stream; the handle keeps dY alive until that stream is joined */
} ctta_wgrad_geom;
typedef struct {
  int implicit_target, implicit_cap;  /* implicit kernel: workgroups a launch aims for, most splits */
  int direct;                         /* one-split launches add straight into the gradient tensors */
  int upsample_copy;                  /* x2-upsampling convolutions: implicit kernel over an x2 copy (0: im2col^T) */
} ctta_wgrad_policy;
enum { CTTA_WGRAD_TN = 0, CTTA_WGRAD_TN_DIRECT, CTTA_WGRAD_IMPLICIT_INPLACE, CTTA_WGRAD_IMPLICIT_DIRECT,
       CTTA_WGRAD_IMPLICIT_DYT, CTTA_WGRAD_IM2COL_T };
typedef struct {
  int route;                          /* CTTA_WGRAD_* */
  int splits, mp, seg;                /* position splits, padded positions (multiple of 64 * splits), positions per split */
  int rows, ld;                       /* slab columns in use (k + 1 + nb) and the slab row stride */
  int sums_apart;                     /* im2col^T: bias / per-sample columns from ctta_wgrad_rowsum, not from the GEMM */
  int upsample_copy;                  /* the kernel reads an x2 copy of the input (xu) */
  int64_t slabs, q, pt, xu;           /* elements of the scratch buffers: fp32 slabs, im2col^T, dY^T, x2 copy (0: not made) */
} ctta_wgrad_plan_info;
ctta_status ctta_wgrad_plan(const ctta_wgrad_geom* g, const ctta_wgrad_policy* policy, ctta_wgrad_plan_info* out);
/* engine 0: the U-Net's policy, 1: the VAE decoder's */
ctta_status ctta_wgrad_engine_policy(int engine, ctta_wgrad_policy* out);

/* Fused HiFi-GAN ResBlock unit (hifigan/models.py:56-63) for C = 32 / 64 / 128 / 256 channels, odd k <= 11 (C = 512: k = 3 / 7 / 11):
 *   out = act( alpha * ( [old out +] x + conv2(leaky_relu(conv1(leaky_relu(x, slope)) + b1, slope)) + b2 ) )
 * conv1: k taps, dilation `dil`; conv2: k taps, dilation 1; "same" zero padding; x / out bf16 [batch][len][channels].
 * The intermediate never leaves LDS.  Weights are FRAGMENT-MAJOR copies ([n/16][k*channels/32][64][8] bf16) of the
 * packed [n][k_pad] operands, made by ctta_frag_pack (k_valid = k * channels).  out_slope > 0 applies a final
 * leaky_relu.  ctta_resunit_supported reports whether a (channels, k, dil) combination fits the kernel.  out must not alias x.
 * One sample is addressed with signed 32-bit byte offsets: len is refused once the rows that the last tile stages (its
 * positions, the conv1 / conv2 halo and the rest of its last load batch) would reach 2^31 bytes into the sample, i.e. a
 * little under 2^30 / channels positions (C = 512, k = 3, dil = 1: at most 2 097 120; the exact rule is resunit_max_len in resunit.hip). */
int ctta_resunit_supported(int channels, int k, int dil);
ctta_status ctta_frag_pack(const void* packed, int n, int k_pad, int k_valid, void* dst, void* stream);
ctta_status ctta_resunit_conv1d(const void* x, int batch, int len, int channels, int k, int dil,
                                const void* w1_frag, const float* b1, const void* w2_frag, const float* b2,
                                float slope, void* out, int accumulate, float alpha, float out_slope, void* stream);
/* The three units of one ResBlock chained in ONE launch (C = 32 / 64, k in {3, 5, 7}): x_{u+1} = x_u + unit_u(x_u) with the
 * residual stream kept in LDS between units (rounded to bf16 after every unit, as ctta_resunit_conv1d stores it), the last
 * unit finished by the same epilogue as ctta_resunit_conv1d.  Bit-identical to three ctta_resunit_conv1d calls.
 * dils / w1_frag / b1 / w2_frag / b2: HOST arrays of three entries (device pointers inside).  out must not alias x.
 * len is refused once ceil(len / T) * T * channels * 2 bytes (T = 256 / 128 positions per workgroup at 32 / 64 channels)
 * would pass 2^31: at most 2^25 / 2^24 positions. */
int ctta_reschain_supported(int channels, int k, const int* dils);
ctta_status ctta_reschain_conv1d(const void* x, int batch, int len, int channels, int k, const int* dils,
                                 const void* const* w1_frag, const float* const* b1, const void* const* w2_frag,
                                 const float* const* b2, float slope, void* out, int accumulate, float alpha,
                                 float out_slope, void* stream);

/* Fused GEGLU feed-forward of a transformer block (diffusers/models/attention.py:276-334, 383-386, 430-432: ff.net.0.proj ->
 * chunk -> value * gelu(gate) -> ff.net.2, plus the residual) for the 256- and 512-wide levels, ONE launch:
 *   out[m][0..n_valid) = res[m][..] + b2 + W2 . ( (W1v . x[m] + b1v) * gelu(W1g . x[m] + b1g) )
 * x: bf16 [M][ld_x] (the LayerNorm output, cp = 256 or 512 columns used); the hidden activations (ffp columns) never leave the
 * CU.  With ln_gamma != NULL x is the LayerNorm's INPUT and the rows are normalised over their first ln_d columns while they
 * are staged (norm3 of the block, attention.py:329-334; same arithmetic and summation order as ctta_layernorm: bit-identical
 * to running it first) -- the normalised tensor never exists in HBM either.
 * `packed` = ctta_ffn_pack's per-wave weight streams (ctta_ffn_pack_bytes bytes) made from the conv_gemm operands of the two
 * linears: ff1 [2*ffp][k_pad1] with its rows in 16-blocks [16 value][16 gate] (what the out_act = 4 epilogue takes), ff2
 * [cp][k_pad2].  b1 follows ff1's row order.  Bit-identical to ctta_conv_gemm(out_act = 4) + ctta_conv_gemm(res).
 * ctta_ffn_geglu_supported: 1 when (cp, ffp) fits the kernel and option "ffn_fuse" is on (asked when a handle is built: it then
 * keeps the weight streams); ctta_ffn_geglu_wanted: 1 when M rows of a fitting (cp, ffp) fill the kernel's row tiles (one
 * workgroup per CU) well enough to beat the two launches (asked per forward; a pure function of its arguments). */
int ctta_ffn_geglu_supported(int cp, int ffp);
int ctta_ffn_geglu_wanted(int cp, int ffp, int64_t M);
size_t ctta_ffn_pack_bytes(int cp, int ffp);
ctta_status ctta_ffn_pack(const void* w1_packed, int k_pad1, const void* w2_packed, int k_pad2, int cp, int ffp, void* dst,
                          void* stream);
ctta_status ctta_ffn_geglu(const void* x, int ld_x, int64_t M, int cp, int ffp, const void* packed, const float* b1,
                           const float* b2, const void* res, int res_ld, void* out, int ldc, int n_valid,
                           const float* ln_gamma, const float* ln_beta, int ln_d, float ln_eps, void* stream);
/* The same launch by descriptor, with two optional neighbours of the feed-forward inside the workgroup:
 * TAIL PROJECTION (proj_packed != NULL; proj_out of the Transformer2DModel + the block's input as residual, transformer_2d.py):
 *   out[m][0..n_valid) = proj_res[m][..] + proj_bias + Wp . bf16( res[m] + b2 + W2 . (...) )
 * the feed-forward result is rounded to bf16 (what the separate launch would store), becomes the operand of one more cp x cp
 * GEMM and never reaches HBM; `out` / `ldc` / `n_valid` then describe the projection's output.
 * FRONT PROJECTION (front_packed != NULL; attn2.to_out + residual and norm3, attention.py:318-334):
 *   s2[m] = front_res[m] + front_bias + W0 . att[m][0..front_k)      (bf16, stored to s2_out: the feed-forward's residual)
 *   x[m]  = LayerNorm(s2[m])   (ln_gamma / ln_beta / ln_d / ln_eps; the normalised rows exist in LDS only)
 * `x` / `ld_x` / `res` / `res_ld` are ignored.  The streams of both projections are made by ctta_ffn_proj_pack from their
 * conv_gemm operands [cp][k_pad] (k = cp for the tail, k = the head-padded attention width for the front).
 * Bit-identical to the separate launches (ctta_conv_gemm x 4 + ctta_layernorm). */
typedef struct {
  const void* x; int ld_x; int64_t M; int cp, ffp;
  const void* packed; const float* b1; const float* b2;
  const void* res; int res_ld;
  void* out; int ldc; int n_valid;
  const float* ln_gamma; const float* ln_beta; int ln_d; float ln_eps;
  const void* proj_packed; const float* proj_bias; const void* proj_res; int proj_res_ld;
  const void* front_packed; const float* front_bias; const void* att; int att_ld; int front_k;
  const void* front_res; int front_res_ld; void* s2_out; int s2_ld;
} ctta_ffn_desc;
void ctta_ffn_desc_init(ctta_ffn_desc* d);
size_t ctta_ffn_proj_pack_bytes(int cp, int k);
ctta_status ctta_ffn_proj_pack(const void* w_packed, int k_pad, int k, int cp, void* dst, void* stream);
ctta_status ctta_ffn_block(const ctta_ffn_desc* d, void* stream);

/* Direct convolution for tiny Cout (<= 8): bf16 NHWC in, fp32 weights [n][kh][kw][c],
 * fp32 planar (NCHW) out, optional input leaky-relu and output tanh. */
ctta_status ctta_conv_small_n(const void* x, int c, int batch, int hi, int wi, int kh, int kw,
                              int pad_h, int pad_w, const float* w, const float* bias, int n,
                              int in_act, float in_slope, int out_act, float* out_nchw,
                              void* out_bf16_nhwc, void* stream);

/* fp32 weight matrix -> packed bf16 [n_rows][k_pad]: dst[r][k] = src[row_off[r]+col_off[k]]
 * (zero when either offset < 0, or when aux_limit > 0 and row_aux[r]+col_aux[k] >= aux_limit).
 * All index arrays are DEVICE int32. */
ctta_status ctta_pack_weight(const float* src, const int32_t* row_off, const int32_t* col_off,
                             const int32_t* row_aux, const int32_t* col_aux, int aux_limit,
                             int n_rows, int k_pad, void* dst, void* stream);

/* Table-driven variants used by the engines' (re)load path: all pack jobs / all fp32 copies of a
 * state dict in ONE launch each.  `jobs` / `segs` are DEVICE arrays; jobs must be sorted by block0
 * (block0 = first thread block of the job, CTTA_PACK_ELEMS_PER_BLOCK outputs per block). */
#define CTTA_PACK_ELEMS_PER_BLOCK 2048
#define CTTA_COPY_ELEMS_PER_BLOCK 16384
typedef struct {
  const float* src;
  const int32_t *row_off, *col_off, *row_aux, *col_aux;
  int aux_limit, n_rows, k_pad, block0;
  void* dst;
  int src_row_len;     /* > 0: every source row is the contiguous range [row_off[r], row_off[r] + src_row_len) and
                          all col_off < src_row_len: eligible for ctta_pack_weight_rows_multi */
  int rows_per_block;  /* ctta_pack_weight_rows_multi only: rows a block stages (<= 64; block0 counts such blocks) */
} ctta_pack_job;
typedef struct {
  const float* src;
  float* dst;
  int count;
} ctta_copy_seg;
ctta_status ctta_pack_weight_multi(const ctta_pack_job* jobs, int n_jobs, int total_blocks, void* stream);
/* Same result for jobs with src_row_len > 0.  A block of `threads` (256 / 512 / 1024) threads stages
 * rows_per_block source rows (rows_per_block * src_row_len <= lds_floats floats of dynamic shared memory), read once
 * and coalesced, and permutes them from LDS -- the strided (cin, kh, kw) -> (kh, kw, cin) gather of a conv weight
 * otherwise touches every cache line kh*kw times.  Callers launch one table per LDS class so that short rows keep
 * several blocks per CU. */
ctta_status ctta_pack_weight_rows_multi(const ctta_pack_job* jobs, int n_jobs, int total_blocks, int lds_floats,
                                        int threads, void* stream);
/* Table-driven bf16 transposes (one 64x64 tile per block): dst[c][r] = src[r][c] for r < rows, c < cols, zero for
 * rows <= r < wcols; only the first wcols columns of a dst row are written.  Used to derive the data-gradient
 * operands (W^T, rotated conv taps) from the freshly packed forward operands without re-reading fp32 weights. */
typedef struct {
  const void* src;
  void* dst;
  int rows, cols, src_ld, dst_ld, wcols, block0, tiles_r;
} ctta_tpose_job;
ctta_status ctta_transpose_multi(const ctta_tpose_job* jobs, int n_jobs, int total_blocks, void* stream);
ctta_status ctta_copy_segments_multi(const ctta_copy_seg* segs, int n_segs, void* stream);

ctta_status ctta_nchw_f32_to_nhwc_bf16(const float* src, void* dst, int batch, int c, int h,
                                       int w, int c_pad, float scale, void* stream);
/* (B, HW, c_stride) fp32 rows -> (B, C, HW) fp32: the last hop of UNet2DCondition*Model.forward's `sample` (conv_out's
 * [pixel][channel] result of ctta_conv_gemm to the reference's NCHW, unet_2d_condition_guided.py:940-945) */
ctta_status ctta_nhwc_f32_to_nchw_f32(const float* src, float* dst, int batch, int c, int hw, int c_stride, void* stream);
ctta_status ctta_nhwc_bf16_to_nchw_f32(const void* src, float* dst, int batch, int c, int h,
                                       int w, int c_stride, void* stream);
ctta_status ctta_rows_f32_to_bf16(const float* src, void* dst, int64_t rows, int cols,
                                  int cols_pad, void* stream);
ctta_status ctta_concat_channels(const void* a, int ca, const void* b, int cb, void* dst,
                                 int64_t pixels, void* stream);
/* The same concatenation, also leaving the GroupNorm partial sums of the result ([batch][*nchunk][groups][2], what
 * ctta_groupnorm_from_partials reads; chunking and summation order of ctta_groupnorm's own first pass, so the normalised tensor
 * is bit-identical to concat + ctta_groupnorm): unet_2d_blocks.py:2053 + resnet.py:553 in one pass over the two sources. */
ctta_status ctta_concat_channels_gn(const void* a, int ca, const void* b, int cb, void* dst, int batch, int hw, int groups,
                                    float* partials, int64_t partials_floats, int* nchunk_out, void* stream);

/* GroupNorm over NHWC bf16 (+ optional SiLU): F.group_norm semantics (biased variance).
 * scratch: fp32 device buffer of ctta_groupnorm_scratch_floats(...) floats. */
size_t ctta_groupnorm_scratch_floats(int batch, int hw, int c, int groups);
ctta_status ctta_groupnorm(const void* x, void* y, int batch, int hw, int c, int groups,
                           const float* gamma, const float* beta, float eps, int silu,
                           float* scratch, void* stream);
/* Same, and also writes (mean, rstd) per (sample, group) to stats [B][G][2] when stats != NULL: what
 * ctta_groupnorm_bwd needs, for free from the forward's own fp64 fold. */
ctta_status ctta_groupnorm_stats_out(const void* x, void* y, int batch, int hw, int c, int groups,
                                     const float* gamma, const float* beta, float eps, int silu,
                                     float* scratch, float* stats, void* stream);
/* Same normalisation from partial sums that a convolution's epilogue already wrote (ctta_conv_desc.gn_part, `nchunk` =
 * ctta_conv_last_gn_chunks()): finalize + apply, no statistics pass over x.  scratch: >= batch * 2 * c floats. */
ctta_status ctta_groupnorm_from_partials(const void* x, void* y, int batch, int hw, int c, int groups,
                                         const float* gamma, const float* beta, float eps, int silu,
                                         const float* partials, int nchunk, float* scratch, float* stats, void* stream);
/* LayerNorm over rows of a padded bf16 matrix: dims [rows][ld], true width d (pad -> 0). */
ctta_status ctta_layernorm(const void* x, void* y, int64_t rows, int d, int ld,
                           const float* gamma, const float* beta, float eps, void* stream);
/* GEGLU: in [rows][2*hp] = [value | gate] -> out [rows][hp] = value * gelu_erf(gate) */
ctta_status ctta_geglu(const void* in, void* out, int64_t rows, int hp, int interleaved, void* stream);
/* Row softmax: fp32 scores [rows][cols] * scale -> bf16 probabilities [rows][cols] */
ctta_status ctta_softmax_rows(const float* s, void* p, int64_t rows, int cols, float scale,
                              void* stream);

/* Multi-head attention, head dim padded to 64 (pad lanes must be zero):
 * q [B][nq][..] row stride q_ld, head h at column h*64; k [B][k_rows >= nk][..] likewise; vt is V
 * TRANSPOSED: [B][heads*64][vt_ld] (keys contiguous).  bias (B, nk) f32 additive per key or NULL.
 * softmax(q k^T * scale + bias) v  ->  out [B][nq][out_ld], head h at column h*64. */
/* Same with a relative-position table added to the scores: rel_bias_log2 [heads][nq+nk-1], entry
 * (key - query + nq - 1), ALREADY multiplied by log2(e); q / out batches are q_rows rows apart (T5 self-attention). */
ctta_status ctta_attention_rel(const void* q, int q_ld, int q_rows, const void* k, int k_ld, int k_rows,
                               const void* vt, int vt_ld, const float* key_bias, const float* rel_bias_log2,
                               void* out, int out_ld, int batch, int heads, int nq, int nk, float scale, void* stream);
ctta_status ctta_attention(const void* q, int q_ld, const void* k, int k_ld, int k_rows, const void* vt,
                           int vt_ld, const float* bias, void* out, int out_ld, int batch,
                           int heads, int nq, int nk, float scale, void* stream);
/* Same, and (when lse != NULL) also writes the log2-domain log-sum-exp of every query row,
 * lse[b][head][q] = log2(sum_k exp2(s*scale*log2e + bias*log2e)), which ctta_attention_bwd_inplace needs. */
ctta_status ctta_attention_lse(const void* q, int q_ld, const void* k, int k_ld, int k_rows,
                               const void* vt, int vt_ld, const float* bias, void* out, int out_ld,
                               int batch, int heads, int nq, int nk, float scale, float* lse,
                               void* stream);
/* Backward of the attention above (autograd of F.scaled_dot_product_attention,
 * attention_processor.py:1127-1129) without materialising the scores.  Every operand is read where it lies:
 *   q, k, vt, bias  exactly as the forward took them (vt [B][heads*64][vt_ld], vt_ld >= nk and a multiple of 8)
 *   out / dout      forward output and its gradient [B*nq][*_ld]
 *   lse             from ctta_attention_lse;  dsum [B][heads][nq] fp32 scratch (D = rowsum(dout*out))
 * Writes dq [B*nq][dq_ld], dk / dv [B*k_rows][*_ld] for keys < nk (head h at columns h*64).
 * partial (optional fp32 scratch of partial_floats): with few keys (cross-attention) the query walk of
 * the dk/dv kernel is split over up to 32 workgroups whose fp32 partial sums are folded afterwards;
 * needs 2 * splits * batch * k_rows * heads*64 floats, fewer splits are used if it is smaller. */
ctta_status ctta_attention_bwd_inplace(const void* q, int q_ld, const void* k, int k_ld, int k_rows, const void* vt,
                                       int vt_ld, const float* bias, const void* out, int out_ld, const void* dout,
                                       int do_ld, const float* lse, float* dsum, void* dq, int dq_ld, void* dk, int dk_ld,
                                       void* dv, int dv_ld, int batch, int heads, int nq, int nk, float scale,
                                       float* partial, int64_t partial_floats, void* stream);

/* Window attention of the CLAP audio tower (Swin, laion_clap/clap_module/htsat.py:336-361): the flash kernels above with a
 * FULL additive bias table full_bias_log2 [n_bias_batches][heads][nq][nk] (already multiplied by log2 e; relative-position
 * bias per head plus the shifted-window mask, one table per window position); batch item b reads table b % n_bias_batches.
 * Heads are padded to 64 lanes like everywhere else.  lse may be NULL in the forward.  The backward takes the operands of
 * ctta_attention_bwd_inplace with the table in place of the per-key bias; it has no split path. */
ctta_status ctta_attention_fullbias(const void* q, int q_ld, const void* k, int k_ld, int k_rows, const void* vt,
                                    int vt_ld, const float* full_bias_log2, int n_bias_batches, void* out, int out_ld,
                                    int batch, int heads, int nq, int nk, float scale, float* lse, void* stream);
ctta_status ctta_attention_fullbias_bwd_inplace(const void* q, int q_ld, const void* k, int k_ld, int k_rows, const void* vt,
                                                int vt_ld, const float* full_bias_log2, int n_bias_batches,
                                                const void* out, int out_ld, const void* dout, int do_ld, const float* lse,
                                                float* dsum, void* dq, int dq_ld, void* dk, int dk_ld, void* dv, int dv_ld,
                                                int batch, int heads, int nq, int nk, float scale, void* stream);

/* ------------------------------------------------------------------------------------ *
 * CLAP fine-tuning stage (tools/losses.py:259-316): glue kernels of the audio tower.
 * ------------------------------------------------------------------------------------ */
/* torchaudio.functional.resample(sinc_interp_kaiser) as a polyphase FIR (tools/losses.py:299-303):
 * y[b][n*up + p] = sum_j kernels[p][j] * x[b][n*down + j - width], zero outside [0, len); kernels fp32 [up][taps] built by
 * the host from the published window formula; out_len = ceil(up * len / down).  _bwd is the adjoint (d y -> d x). */
ctta_status ctta_resample_poly(const float* x, int batch, int len, const float* kernels, int up, int down, int width,
                               int taps, float* y, int64_t out_len, void* stream);
ctta_status ctta_resample_poly_bwd(const float* dy, int batch, int64_t out_len, const float* kernels, int up, int down,
                                   int width, int taps, float* dx, int len, void* stream);
/* |STFT| with input gradient for MultiResolutionSTFTLoss (tools/losses.py:146-169 `stft`, :187-256): torch.stft(center,
 * reflect padding, periodic Hann window of win_length centred in fft_size) -> sqrt(clamp(re^2 + im^2, 1e-8)), laid out
 * (batch, frames, fft_size / 2 + 1) with frames = n_samples / hop_size + 1.  The reference computes in float64; here both
 * GEMM operands are split into three bf16 parts (fp32-grade).  ctta_stft_magnitude_bwd maps d|STFT| of the LAST
 * ctta_stft_magnitude call on the handle to d wav (batch, n_samples).  One handle per resolution; not thread-safe. */
typedef struct ctta_stft ctta_stft;
ctta_status ctta_stft_create(int fft_size, int hop_size, int win_length, int max_batch, int max_samples, ctta_stft** out);
void ctta_stft_destroy(ctta_stft* h);
int ctta_stft_frames(const ctta_stft* h, int n_samples);
ctta_status ctta_stft_magnitude(ctta_stft* h, const float* wav, int batch, int n_samples, float* mag, void* stream);
ctta_status ctta_stft_magnitude_bwd(ctta_stft* h, const float* dmag, int batch, int n_samples, float* dwav, void* stream);

/* Spectrogram(power 2) + LogmelFilterBank (dB, amin) of htsat.py:684-697 on a ctta_mel_frontend handle: (batch, n_samples)
 * fp32 -> logmel [batch][n_samples / hop + 1][n_mels] fp32; _bwd maps d logmel to d wav for the last forward call. */
ctta_status ctta_wav_to_logmel_db(ctta_mel_frontend* h, const float* wav, int batch, int n_samples, float amin,
                                  float* logmel, void* stream);
ctta_status ctta_wav_to_logmel_db_bwd(ctta_mel_frontend* h, const float* dlogmel, int batch, int n_samples, float amin,
                                      float* dwav, void* stream);
/* bn0 (eval: per-mel-bin scale / shift) + bicubic stretch of the frame axis (tap tables [out_frames][4] from the host) +
 * fold into the (spec_size x spec_size) image, htsat.py:913-925,856-878 -> NHWC bf16 [batch][S][S][cpad] (channel 0).
 * _bwd: gradient of the patch-embedding conv in token layout [batch][(S/patch)^2][ld >= patch^2] fp32 -> d logmel, with the
 * transposed tap list in CSR form (rt_ptr [frames + 1], rt_tt, rt_w). */
ctta_status ctta_htsat_image(const float* logmel, int batch, int frames, int mel_bins, const float* bn_scale,
                             const float* bn_shift, const int32_t* tap_idx, const float* tap_w, int out_frames,
                             int spec_size, int cpad, void* image_nhwc, void* stream);
ctta_status ctta_htsat_image_bwd(const float* dtokens, int dtokens_ld, int patch, int batch, int frames, int mel_bins,
                                 const float* bn_scale, const int32_t* rt_ptr, const int32_t* rt_tt, const float* rt_w,
                                 int spec_size, float* dlogmel, void* stream);
/* dst[r][:] = src[idx[r]][:] over bf16 rows (idx < 0: zeros): window partition / cyclic shift / patch merging and their
 * inverses are all row permutations of the token matrix (htsat.py:259-287,471-492,517-537). */
ctta_status ctta_gather_rows(const void* src, int src_ld, const int32_t* idx, void* dst, int dst_ld, int64_t n_rows,
                             int row_elems, void* stream);
/* nn.GELU (erf) on bf16 and its backward from the pre-activation (htsat.py:156-174) */
ctta_status ctta_gelu(const void* x, void* y, int64_t n, void* stream);
ctta_status ctta_gelu_bwd(const void* x, const void* dy, void* dx, int64_t n, void* stream);
/* mean over the token axis: bf16 [batch][tokens][ld] -> fp32 [batch][channels], and its backward (htsat.py:818-819) */
ctta_status ctta_mean_tokens(const void* x, int batch, int tokens, int channels, int ld, float* y, void* stream);
ctta_status ctta_mean_tokens_bwd(const float* dy, int batch, int tokens, int channels, int ld, void* dx, void* stream);

/* Evaluation-suite classifier glue (PANNs Cnn14, audioldm_eval/feature_extractors/panns/models.py:168-323; the twelve 3x3
 * convolutions run on ctta_conv_gemm with BatchNorm folded in, the front end on ctta_wav_to_logmel_db):
 *   ctta_logmel_to_image  bn0 in eval mode (models.py:276-278: scale / shift per mel bin) of logmel fp32 [batch][frames][mel_bins]
 *                         -> image bf16 [batch][frames][mel_bins][8], channel 0 live;
 *   ctta_avgpool2         F.avg_pool2d(2) (models.py:71-72) on NHWC bf16 [batch][hi][wi][c] -> [batch][hi/2][wi/2][c], c % 8 == 0,
 *                         a trailing odd row / column dropped as torch does;
 *   ctta_cnn14_head       mean over frequency, then max over time + mean over time (models.py:305-309):
 *                         bf16 [batch][frames][freq][c] -> fp32 [batch][c]. */
ctta_status ctta_logmel_to_image(const float* logmel, int batch, int frames, int mel_bins, const float* scale,
                                 const float* shift, void* image, void* stream);
ctta_status ctta_avgpool2(const void* x, void* y, int batch, int hi, int wi, int c, void* stream);
ctta_status ctta_cnn14_head(const void* x, int batch, int frames, int freq, int c, float* y, void* stream);

/* VGGish for the Frechet Audio Distance (audioldm_eval/metrics/fad.py:39-79; the model is harritaylor/torchvggish, its input
 * stage TensorFlow models' vggish_input.py / mel_features.py / vggish_params.py):
 *   ctta_vggish_frontend_create  a ctta_mel_frontend handle with the VGGish basis (periodic Hann of 400 samples, zero-extended
 *                                512-point DFT) and mel matrix (64 HTK bands, 125-7500 Hz, no area norm, DC row zero) for up
 *                                to max_batch clips of max_samples samples at 16 kHz; ctta_mel_frontend_destroy frees it, the
 *                                other ctta_mel_frontend entries refuse it;
 *   ctta_wav_to_vggish_logmel    wav (batch, n_samples) f32, taken as it is (no padding, clipping or NaN scrubbing) -> frames
 *                                of 400 samples at hop 160 -> ln(|rfft| @ mel + 0.01) -> logmel f32
 *                                [batch][n_examples * 96][64] = [batch * n_examples][96][64], n_examples =
 *                                (1 + (n_samples - 400) / 160) / 96; only frames inside an example are computed;
 *                                CTTA_ERR_INVALID below 15600 samples (no example);
 *   ctta_maxpool2                F.max_pool2d(2, 2) (torchvggish `VGG.features`) on NHWC bf16 [batch][hi][wi][c] ->
 *                                [batch][hi/2][wi/2][c], c % 8 == 0, a trailing odd row / column dropped as torch does. */
ctta_status ctta_vggish_frontend_create(int max_batch, int max_samples, ctta_mel_frontend** out);
ctta_status ctta_wav_to_vggish_logmel(ctta_mel_frontend* h, const float* wav, int batch, int n_samples, float* logmel,
                                      void* stream);
ctta_status ctta_maxpool2(const void* x, void* y, int batch, int hi, int wi, int c, void* stream);

/* |librosa.stft(x, n_fft = n_dft, hop_length = hop_size, window = periodic Hann of n_dft samples, center = True)| as
 * ssr_eval.metrics.AudioMetrics computes it for `lsd` and `ssim_stft` (behind audioldm_eval/eval.py:137-162; n_dft =
 * int(2048 / (44100 / sr)) = 743 at 16 kHz, 1486 at 32 kHz).  ctta_stft_create requires fft_size % 64 == 0; this entry takes
 * any 16 <= n_dft <= 8192, odd ones included: frames and basis rows hold n_dft samples followed by zeros up to the GEMM's K
 * multiple (the layout of the VGGish front end's 400-in-512 basis), the bins are k / n_dft, n_dft / 2 + 1 of them.  Centre
 * padding of n_dft / 2 samples on both sides, reflect (pad_zero = 0: librosa 0.9, which ssr_eval was released against) or
 * zeros (pad_zero = 1: librosa 0.10); frames = n_samples / hop_size + 1; for an odd n_dft the last frame ends one sample past
 * the padding, which is continued by the same rule.  The handle goes to ctta_stft_magnitude (same split-bf16 arithmetic,
 * (batch, frames, n_dft / 2 + 1) output) and gives sqrt(re^2 + im^2) WITHOUT the loss path's 1e-8 clamp;
 * ctta_stft_magnitude_bwd refuses it. */
ctta_status ctta_stft_create_dft(int n_dft, int hop_size, int pad_zero, int max_batch, int max_samples, ctta_stft** out);

/* Paired metrics of the evaluation suite (audioldm_eval/eval.py:137-179; ssr_eval and skimage are pip dependencies of the
 * reference: built from the published definitions), batched over at most CTTA_PAIR_MAX pairs per call.  Inputs are fp32
 * device tensors padded to the chunk's longest pair, the per-pair extents are HOST int32 arrays, outputs are fp64 device
 * arrays [pairs].  All sums run in fp64 and in a fixed order (partials in the caller's device workspace `ws`, added by a
 * second launch): the same inputs give the same bits.
 *   ctta_lsd        eval.py:154,160-162 -> AudioMetrics.lsd on magnitude spectrograms est / tgt [pairs][frames_max][bins],
 *                   frames[p] valid frames: mean_t sqrt(mean_f log10(tgt^2 / (est + 1e-12)^2 + 1e-12)^2); ws: pairs *
 *                   frames_max doubles;
 *   ctta_ssim_mean  eval.py:177 / AudioMetrics.ssim -> skimage.metrics.structural_similarity(x, y, win_size = win, data_range)
 *                   on images [pairs][h_max][w] with h_valid[p] valid rows: uniform window, K1 = 0.01, K2 = 0.03, sample
 *                   covariance (win^2 / (win^2 - 1)) when sample_covariance, mean over the positions whose whole window lies
 *                   inside the image; win odd, 3..11; ws: pairs * ctta_ssim_tiles(h_max, w, win) doubles;
 *   ctta_psnr_mse   eval.py:172 -> the mean of (x - y)^2 under skimage.metrics.peak_signal_noise_ratio (an exact 0 for identical
 *                   images: the caller skips such a pair, eval.py:173-175); ws: pairs * h_max doubles.
 * CTTA_ERR_INVALID for an image smaller than one window, a pair without frames, more than CTTA_PAIR_MAX pairs. */
#define CTTA_PAIR_MAX 256
ctta_status ctta_lsd(const float* est, const float* tgt, int pairs, int frames_max, int bins, const int32_t* frames, double* lsd,
                     double* ws, void* stream);
int64_t ctta_ssim_tiles(int h, int w, int win);
ctta_status ctta_ssim_mean(const float* x, const float* y, int pairs, int h_max, int w, const int32_t* h_valid, int win,
                           double data_range, int sample_covariance, double* ssim, double* ws, void* stream);
ctta_status ctta_psnr_mse(const float* x, const float* y, int pairs, int h_max, int w, const int32_t* h_valid, double* mse,
                          double* ws, void* stream);

/* The file loaders' resampler and waveform normalisation for a ragged batch of clips (tools/torch_tools.py:54-75
 * `read_wav_file`; the same call in tools/t2a_dataset.py:111-122, audioldm_eval/datasets/load_mel.py:25-28 and
 * metrics/fad.py:33-34).  resampy is a pip dependency of the reference, not part of its tree: built from the published
 * definition of version 0.4.2 (core.resample + interpn.resample_f), restated in float64 numpy in tests/resampy_ref.py.
 * One ctta_resample_clip per clip, filled by the host (consistencytta_amd/audio.py `resample_clip`) and read from DEVICE memory:
 *   ctta_resample_sinc  torch_tools.py:66 -> resampy.resample(x, sr_orig, sr_new, filter): clip p reads n_in samples at
 *                       x + x_off and writes n_out at y + y_off (x and y may be one arena; a clip's input and output must
 *                       not overlap).  `win`: the filter's half window, n_win fp32 entries at num_table entries per zero
 *                       crossing, UNSCALED (the clip's gain carries sample_ratio when down-sampling); delta[j] = win[j + 1] -
 *                       win[j], 0 at the end.  Output t: time_register = t * time_increment, n = int(time_register), frac =
 *                       scale * (time_register - n), offset = int(frac * num_table), eta = frac * num_table - offset, all in
 *                       fp64 as separate operations; left wing sum_i (win + eta * delta)[offset + i * index_step] * x[n - i],
 *                       i < min(n + 1, (n_win - offset) / index_step); right wing the same with frac := scale - frac on
 *                       x[n + 1 + k], k < min(n_in - n - 1, (n_win - offset) / index_step).  Weights and sums in fp64, in
 *                       that order: a clip's output does not depend on the rest of the batch.  max_n_out >= every n_out
 *                       sizes the grid.
 *   ctta_wave_prepare   torch_tools.py:69-73 on clip p's n_out samples at y + y_off: wav - mean; / (max|wav| + 1e-8) / 2;
 *                       cut or zero-padded to `segment`; / (max|.| of the kept segment + 1e-8) / 2 -> out [n_clips][segment].
 *                       Mean and maxima in fp64 in a fixed order, the element arithmetic in fp64 rounded once to fp32.
 *                       ws: 3 * n_clips doubles, left holding each clip's mean, first peak and second peak.
 * Both only enqueue on `stream` (no allocation, no synchronisation). */
typedef struct ctta_resample_clip {
  int64_t x_off, y_off;      /* element offset of the clip's first sample in x / y */
  int32_t n_in, n_out;       /* n_out = int(n_in * sr_new / sr_orig) >= 1 */
  double time_increment;     /* 1.0 / (float(sr_new) / sr_orig) */
  double scale;              /* min(1, sample_ratio) */
  float gain;                /* sample_ratio when < 1, else 1 */
  int32_t index_step;        /* int(scale * num_table): truncated */
} ctta_resample_clip;
ctta_status ctta_resample_sinc(const float* x, float* y, const ctta_resample_clip* clips, int n_clips, int max_n_out,
                               const float* win, int n_win, int num_table, void* stream);
ctta_status ctta_wave_prepare(const float* y, const ctta_resample_clip* clips, int n_clips, int segment, float* out, double* ws,
                              void* stream);

/* Small fp32 linear: y[m][n] = act_out(sum_k act_in(x[m][k]) * w[n][k] + b[n]); m <= 1024.
 * act: 0 none, 1 silu. */
ctta_status ctta_linear_f32(const float* x, const float* w, const float* b, float* y, int m,
                            int n, int k, int act_in, int act_out, void* stream);
/* Sinusoidal timestep features (embeddings.py:25-65) and Gaussian Fourier features
 * (embeddings.py:239-249) in one launch.  freqs: [dim/2] f32 table. */
ctta_status ctta_time_features(const float* t, const float* freqs, int dim, int flip, float* out,
                               int batch, void* stream);
ctta_status ctta_fourier_features(const double* w, const float* weight, int half, int flip,
                                  float* out, int batch, void* stream);

/* ------------------------------------------------------------------------------------ *
 * Backward-pass operators of the distillation step (student U-Net); torch-autograd semantics of
 * the reference modules.  All contractions run on ctta_conv_gemm; these are the glue kernels.
 * ------------------------------------------------------------------------------------ */
/* dst[g][c][r] = src[g][r][col0 + c] (r < rows), zero for rows <= r < dst_ld */
ctta_status ctta_transpose_bf16(const void* src, int64_t src_group_stride, int rows, int cols, int src_ld,
                                int col0, void* dst, int64_t dst_group_stride, int dst_ld, int groups,
                                void* stream);
/* Q[(ch*taps + tap)][m] = X[pixel(m, tap)][ch] (transposed im2col, channel-major rows = the (cin,kh,kw) order
 * of a conv weight row; rows padded to m_pad); when
 * indicator_batches >= 0 appends 1 + indicator_batches rows: all-ones, then per-sample indicators. */
ctta_status ctta_im2col_t(const void* x, int c, int batch, int hi, int wi, int upsample, int ho, int wo,
                          int kh, int kw, int stride, int pad_h, int pad_w, int dil_w, void* dst, int m_pad,
                          int indicator_batches, void* stream);
/* grad_w[row_off[n] + col_off[k]] (+)= sum_s slabs[s][k][n]: inverse of ctta_pack_weight
 * (col_off NULL = identity; negative offsets are skipped) */
ctta_status ctta_wgrad_scatter(const float* slabs, int n_slabs, int64_t slab_stride, int ldn, int k_rows,
                               int n_cols, const int32_t* row_off, const int32_t* col_off,
                               const int32_t* row_aux, const int32_t* col_aux, int aux_limit, float* grad,
                               int accumulate, void* stream);
/* same contraction for row-major slabs [S][n_rows][ldk] (k contiguous):
 * grad_w[row_off[n] + col_off[k]] (+)= sum_s slabs[s][n][k] */
/* Implicit weight-gradient GEMM (csrc/wgrad_gemm.hip): slabs[s][n][c * taps + t] = sum over split s's positions m of
 * dY^T[n][m] * X[pixel(m, tap t)][c] -- the product ctta_im2col_t + ctta_conv_gemm compute, without materialising im2col(X)^T.
 * dyt: bf16 [n][mp] (ctta_transpose_bf16 of dY, zero beyond m_valid); x: bf16 NHWC (batch, h, w) with x_ld elements per
 * pixel, c channels used; taps = 9: 3x3, stride 1, pad 1, a power-of-two width from 2 to 64 with h * w a multiple of 64,
 * columns in (cin, kh, kw) order; taps = 1: a linear layer
 * (batch * h * w = rows).  bias_col >= 0 also writes the row sums of dY^T into column bias_col (bias gradient) and, for
 * sample_cols > 0, per-sample sums into the columns behind it (d temb).  mp % (64 * splits) == 0.
 * ctta_wgrad_implicit_supported: whether a geometry is inside the kernel's range (CTTA_WGRAD_IMPLICIT=0 turns it off). */
int ctta_wgrad_implicit_supported(int taps, int c, int h, int w, int x_ld, int n);
/* ctta_wgrad_implicit with dY [m_valid][ldy] read where it lies (taps = 9 only): no transposed copy, bias / per-sample
 * columns summed inside the kernel. */
ctta_status ctta_wgrad_implicit_inplace(const void* dy, int ldy, int n, int mp, const void* x, int x_ld, int c, int batch, int h,
                                        int w, int taps, int m_valid, int splits, int bias_col, int sample_cols, float* slabs,
                                        int64_t slab_stride, int ld, void* stream);
/* Weight gradient of a linear layer with BOTH operands read in place (no transposed copies):
 * slabs[s][r][k] = sum over split s's rows m of dY[m][r] * X[m][k]; dy [m_valid][ldy] (n columns used), x [m_valid][ldx]
 * (c columns used), row-major bf16; rows beyond m_valid count as zero up to mp (mp %% (64 * splits) == 0).  bias_col >= c
 * also writes the column sums of dY into slabs[s][r][bias_col].  Replaces autograd's grad_weight / grad_bias of F.linear
 * (diffusers/models/attention.py:276-334, attention_processor.py:1107-1136) in the student's backward pass. */
ctta_status ctta_wgrad_tn(const void* dy, int ldy, int n, const void* x, int ldx, int c, int m_valid, int mp, int splits,
                          int bias_col, float* slabs, int64_t slab_stride, int ld, void* stream);
/* The same two products with ONE split and the tile added STRAIGHT into the layer's gradient tensors through the pack map
 * (autograd's accumulate into .grad, tools/train_utils.py:166): grad_w[row_off[n] + col(k)] += dW[n][k] for k < k_cols, rows with
 * row_off[n] < 0 skipped (padding), col = col_off[k] (< 0 skipped) or the identity when col_off is NULL;
 * grad_b[bias_idx[n] or n] += column sum of dY for n < n_bias (grad_b NULL: no bias).  No fp32 slab, no scatter launch; the
 * same bits as slab + ctta_wgrad_scatter_rows_bias(accumulate = 1) with one slab. */
ctta_status ctta_wgrad_tn_direct(const void* dy, int ldy, int n, const void* x, int ldx, int c, int m_valid, int mp,
                                 int k_cols, int n_rows, const int32_t* row_off, const int32_t* col_off, float* grad_w,
                                 int n_bias, const int32_t* bias_idx, float* grad_b, void* stream);
ctta_status ctta_wgrad_implicit_direct(const void* dy, int ldy, int n, int mp, const void* x, int x_ld, int c, int batch,
                                       int h, int w, int m_valid, int k_cols, int n_rows, const int32_t* row_off,
                                       float* grad_w, int n_bias, const int32_t* bias_idx, float* grad_b, void* stream);
/* the row sums alone: slabs[s][r][bias_col] = sum over split s of dY^T[r][m] (+ per-sample sums in the sample_cols columns
 * behind it): bias gradient / d temb of the layers whose weight-gradient product runs on ctta_conv_gemm */
ctta_status ctta_wgrad_rowsum(const void* dyt, int n, int mp, int m_valid, int splits, int hw, int sample_cols, float* slabs,
                              int64_t slab_stride, int ld, int bias_col, void* stream);
ctta_status ctta_wgrad_implicit(const void* dyt, int n, int mp, const void* x, int x_ld, int c, int batch, int h, int w,
                                int taps, int m_valid, int splits, int bias_col, int sample_cols, float* slabs,
                                int64_t slab_stride, int ld, void* stream);
ctta_status ctta_wgrad_scatter_rows(const float* slabs, int n_slabs, int64_t slab_stride, int ldk, int k_cols,
                                    int n_rows, const int32_t* row_off, const int32_t* col_off, float* grad,
                                    int accumulate, void* stream);
/* dst[j*dst_stride + idx[n]] (+)= sum_s slabs[s][n][col + j], j < n_cols (bias / per-sample columns) */
/* ctta_wgrad_scatter_rows that also folds column `bias_col` of the slabs into grad_bias[bias_idx[n]] for n < n_bias (the
 * layer's bias gradient in the same launch; bias_col < 0: none) */
ctta_status ctta_wgrad_scatter_rows_bias(const float* slabs, int n_slabs, int64_t slab_stride, int ldk, int k_cols, int n_rows,
                                         const int32_t* row_off, const int32_t* col_off, float* grad, int bias_col, int n_bias,
                                         const int32_t* bias_idx, float* grad_bias, int accumulate, void* stream);
ctta_status ctta_col_scatter(const float* slabs, int n_slabs, int64_t slab_stride, int ldk, int col, int n_cols,
                             int n_rows, const int32_t* idx, float* dst, int64_t dst_stride, int accumulate,
                             void* stream);
ctta_status ctta_row_scatter(const float* slabs, int n_slabs, int64_t slab_stride, int ldn, int row,
                             int n_cols, const int32_t* idx, float* dst, int accumulate, void* stream);
/* out (+)= res + alpha * g * (act > 0 ? 1 : slope): LeakyReLU backward on the saved activation, residual folded in */
ctta_status ctta_lrelu_bwd(const void* g, const void* act, float slope, float alpha, const void* res, void* out,
                           int64_t n, int accumulate, void* stream);
/* data gradient of a 1-output-channel conv (w fp32 [tap][c]); gy is scaled by (1 - y_tanh^2) when y_tanh != NULL and
 * the result by leaky_relu'(act) when act != NULL; dx NHWC bf16 */
ctta_status ctta_conv_cout1_dgrad(const float* gy, const float* y_tanh, const float* w, int batch, int h, int wd,
                                  int kh, int kw, int pad_h, int pad_w, int c, const void* act, float slope,
                                  void* dx, void* stream);
/* weight and bias gradient of the same 1-output-channel conv (at most 9 taps, c a multiple of 8 up to 2048):
 * dw[c][tap] (+)= sum_m gy[m] * a[pixel(m, tap)][c] in the state dict's (1, c, kh, kw) order, db[0] (+)= sum_m gy[m]
 * (db may be NULL); gy fp32 (batch, h, wd), a NHWC bf16 with c channels.  Per-workgroup partial rows in `scratch`
 * (ctta_conv_cout1_wgrad_scratch_floats floats) are folded in a fixed order: no atomics, the same bits every run. */
size_t ctta_conv_cout1_wgrad_scratch_floats(int batch, int h, int wd, int kh, int kw, int c);
ctta_status ctta_conv_cout1_wgrad(const float* gy, const void* a, int batch, int h, int wd, int kh, int kw, int pad_h,
                                  int pad_w, int c, float* dw, float* db, int accumulate, float* scratch, void* stream);
/* post_quant_conv's parameter gradients (1x1 conv of z / scale, embed_dim zin <= 16 -> z_channels zout <= 32):
 * dw[o][e] (+)= sum_pix dzin[pix][o] * (z[b][e][hw] * inv_scale), db[o] (+)= sum_pix dzin[pix][o] (db may be NULL);
 * dzin NHWC bf16 with ld elements per pixel, z fp32 (batch, zin, hw).  Same fixed-order fold through `scratch`. */
size_t ctta_post_quant_wgrad_scratch_floats(int batch, int hw, int zin, int zout);
ctta_status ctta_post_quant_wgrad(const void* dzin, int ld, const float* z, float inv_scale, int batch, int zin, int zout,
                                  int hw, float* dw, float* db, int accumulate, float* scratch, void* stream);
/* GroupNorm(+SiLU) backward; stats [B][G][2] = (mean, rstd) from ctta_groupnorm_stats */
size_t ctta_groupnorm_bwd_scratch_floats(int batch, int hw, int c, int groups);
ctta_status ctta_groupnorm_stats(const void* x, int batch, int hw, int c, int groups, float eps, float* stats,
                                 void* stream);
ctta_status ctta_groupnorm_bwd(const void* x, const void* dy, void* dx, int batch, int hw, int c, int groups,
                               const float* stats, const float* gamma, const float* beta, int silu,
                               int accumulate_dx, float* dgamma, float* dbeta, int accumulate_param,
                               float* scratch, void* stream);
/* LayerNorm backward (statistics recomputed); dgamma/dbeta are ACCUMULATED into (one fp32 atomic per block and column; a
   matrix of fewer than 16 blocks' worth of rows, <= 120, runs as one block and is bit-reproducible) */
ctta_status ctta_layernorm_bwd(const void* x, const void* dy, void* dx, int64_t rows, int d, int ld,
                               const float* gamma, float eps, int accumulate_dx, float* dgamma, float* dbeta,
                               void* stream);
/* dx = dx_add + dL/dx with a separate output (dx_add may be NULL, or equal dx = the in-place accumulate above) */
ctta_status ctta_layernorm_bwd_add(const void* x, const void* dy, const void* dx_add, void* dx, int64_t rows, int d, int ld,
                                   const float* gamma, float eps, float* dgamma, float* dbeta, void* stream);
/* The same with a CALLER-OWNED partial table for d gamma / d beta (per-block sums, a sliced fold and a fold of the slices,
   all in a fixed order and without float atomics: two runs give the same bits); scratch may be NULL (atomics path).  The
   library holds no workspace of its own for this call. */
size_t ctta_layernorm_bwd_scratch_floats(int64_t rows, int ld);
ctta_status ctta_layernorm_bwd_ws(const void* x, const void* dy, const void* dx_add, void* dx, int64_t rows, int d, int ld,
                                  const float* gamma, float eps, float* dgamma, float* dbeta, float* scratch,
                                  size_t scratch_floats, void* stream);
ctta_status ctta_geglu_bwd(const void* f, const void* dout, void* df, int64_t rows, int hp, int interleaved,
                           void* stream);
ctta_status ctta_add_slices(const void* a, int lda, const void* b, int ldb, void* out, int ldo, int64_t rows,
                            int cols, void* stream);
ctta_status ctta_zero_insert2(const void* dy, void* dz, int batch, int ho, int wo, int hz, int wz, int c,
                              void* stream);
/* out (batch, 2h, 2w, c) = nearest x2 of x (batch, h, w, c), NHWC bf16, c a multiple of 8 (pool2_sum's forward twin) */
ctta_status ctta_upsample2_nearest(const void* x, void* out, int batch, int h, int w, int c, void* stream);
ctta_status ctta_pool2_sum(const void* dup, void* dx, int batch, int h, int w, int c, int accumulate,
                           void* stream);
ctta_status ctta_softmax_bias_rows(const float* s, int lds, const float* bias, int rows_per_bias, void* p,
                                   int64_t rows, int cols, int ldp, float scale, void* stream);
ctta_status ctta_softmax_bwd_rows(const void* p, const float* dp, int lddp, void* ds, int64_t rows, int cols,
                                  int ldp, float scale, void* stream);
ctta_status ctta_linear_f32_bwd(const float* x, const float* w, const float* dy, int dy_ld,
                                const float* xpre_silu, float* dx, float* dw, float* db, int m, int n, int k,
                                int accumulate_dx, int accumulate_param, void* stream);
/* d/dpred of get_loss (MSE 'instance' x SNR clamp, models/audio_consistency_model.py:250-266) as NHWC bf16 */
ctta_status ctta_snr_mse_grad(const float* pred, const float* target, const float* sigma, float gamma,
                              float loss_scale, int batch, int c, int hw, int c_pad, void* dpred_nhwc,
                              void* stream);
/* torch.optim.AdamW step (tools/train_utils.py:59-63): decoupled weight decay, bias correction by `step` */
ctta_status ctta_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                            float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                            float grad_scale, void* stream);
/* The optimizer tail of one training step as ONE pass over the training state: optimizer.step() -> optimizer.zero_grad() ->
 * update_ema() (tools/train_utils.py:177-183, 255-282).  param / grad / both shadows are the flat fp32 buffers of n_all
 * elements (trainable prefix of n_train elements first, see AudioLCM.prepare_training); exp_avg / exp_avg_sq cover the
 * prefix.  Reads p, g, m, v, shadow_a, shadow_b; writes p, m, v, both shadows and g = 0.  do_step = 0 leaves p, m, v alone
 * (the reference skips the update on a NaN loss, train_utils.py:167-172, but still zeroes the gradients and moves the
 * shadows).  shadow_b may be NULL.  Per element the same fp32 operations in the same order as ctta_adamw_step followed by
 * ctta_ema_update2: bit-identical state.  n_train and n_all must be multiples of 4, all buffers 16-byte aligned. */
ctta_status ctta_adamw_ema2_zero(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n_train, int64_t n_all,
                                 float* shadow_a, double decay_a, float* shadow_b, double decay_b, int do_step, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                                 void* stream);

/* LoRA adapters of the attention projections (csrc/lora.hip; diffusers LoRAAttnProcessor): y = W x + scale * up(down(x)) with
 * rank r in [1, 16].  The base product stays a conv_gemm launch; these add the rank-r term, forward and backward.  Adapter
 * matrices are fp32 and taken in either orientation, so one packed A [r][k] and one packed B [n][r] serve both passes.
 * Activations are bf16 in the engines' padded layouts: k, n and the leading dimensions are multiples of 8, the pointers
 * 16-byte aligned.  The kernels read every column they are given; the packed adapter holds zeros in its padded rows and
 * columns and the activations' padded columns are finite, so padding contributes exactly 0.  No float atomics: results are
 * bit-reproducible.
 *   down     : d[m][r] (fp32) = x[m][k] * a^T; a is [r][k], or [k][r] when a_kmajor (the backward's dD = dY * B)
 *   up_add   : y[m][n] = bf16(float(y) + scale * d * b^T); b is [n][r], or [r][n] when b_rmajor (the backward's
 *              dX += dD * A).  Elements whose added term is zero keep their bits.
 *   up_add_t : the same into a transposed result yt[batch][n][tokens] (row stride ldt, batch stride batch_stride), the
 *              rows of d being (batch, d_tokens >= tokens); b is [n][r]
 *   wgrad    : g[j * g_stride_r + col(kk) * g_stride_k] += scale * sum_m d[m][j] * x[m][kk], col = col_map[kk] (device
 *              int32, -1 = padded column, dropped) or kk when col_map is NULL.  g is any fp32 address (no alignment
 *              rule).  dA = dD^T X: strides (K, 1); dB = dY^T D: strides (1, r).  Per-slab partial sums in `scratch`
 *              (ctta_lora_wgrad_scratch_floats floats) are folded in slab order. */
ctta_status ctta_lora_down(const void* x, int ldx, int64_t m, int k, const float* a, int a_kmajor, int r, float* d,
                           void* stream);
ctta_status ctta_lora_up_add(void* y, int ldy, int64_t m, int n, const float* d, const float* b, int b_rmajor, int r,
                             float scale, void* stream);
ctta_status ctta_lora_up_add_t(void* yt, int ldt, int64_t batch_stride, int batch, int tokens, int n, const float* d,
                               int d_tokens, const float* b, int r, float scale, void* stream);
/* The three forward operators with one adapter PER SAMPLE (a batch whose rows ask for different fine-tunes over one base
 * model; diffusers gives a call one strength, attention_processor.py:508-613 `LoRAAttnProcessor.__call__(..., scale=)`, and
 * one adapter set -- here both are looked up per row).  A *bank* is n_slots packed matrices slot_stride floats apart, each in
 * the layout and under the padded-column contract above: a_bank slots are [r][k] (slot_stride a multiple of 4, >= r * k),
 * b_bank slots are [n][r].  sample = row / rows_per_sample (the batch index of the transposed form); slot_of_sample is a
 * DEVICE int32 array, scale_of_sample a DEVICE float array or NULL, both read when the kernel runs, so a captured graph
 * serves whatever they hold at replay.
 *   down_rows     : d[row][:] = x[row] * a_bank[slot]^T where slot is in [0, n_slots), d[row][:] = 0 otherwise
 *   up_add_rows   : y[row] += s * d[row] * b_bank[slot]^T, s = scale_of_sample[sample] when the array is given, `scale`
 *                   otherwise (not their product)
 *   up_add_t_rows : the same into yt[batch][n][tokens], tokens / d_tokens as ctta_lora_up_add_t
 * A slot outside [0, n_slots) -- -1, the documented "base model", or any index too large -- reads nothing of the bank and
 * stores nothing to y: no value in a device array makes a kernel read outside the bank.  For a valid slot a row's result is
 * BIT FOR BIT that of ctta_lora_down / _up_add / _up_add_t on that row with that slot's matrix and that scale (same lanes
 * per row by k, same fold and fmaf chains, same rank dispatch, same b * scale pre-multiply, same "store nothing where all
 * eight sums are zero").  The grid of up_add_rows is per sample, so rows_per_sample need not be a multiple of anything. */
ctta_status ctta_lora_down_rows(const void* x, int ldx, int64_t m, int k, const float* a_bank, int64_t slot_stride, int n_slots,
                                int r, int64_t rows_per_sample, const int32_t* slot_of_sample, float* d, void* stream);
ctta_status ctta_lora_up_add_rows(void* y, int ldy, int64_t m, int n, const float* d, const float* b_bank, int64_t slot_stride,
                                  int n_slots, int r, int64_t rows_per_sample, const int32_t* slot_of_sample,
                                  const float* scale_of_sample, float scale, void* stream);
ctta_status ctta_lora_up_add_t_rows(void* yt, int ldt, int64_t batch_stride, int batch, int tokens, int n, const float* d,
                                    int d_tokens, const float* b_bank, int64_t slot_stride, int n_slots, int r,
                                    const int32_t* slot_of_sample, const float* scale_of_sample, float scale, void* stream);
size_t ctta_lora_wgrad_scratch_floats(int64_t m, int k, int r);
ctta_status ctta_lora_wgrad(const float* d, const void* x, int ldx, int64_t m, int k, int r, float scale, float* g,
                            int64_t g_stride_r, int64_t g_stride_k, const int32_t* col_map, float* scratch, void* stream);

/* Fused forms for rank <= 4: one to three sites that share ONE input (q / k / v of a self-attention on its LayerNorm output,
 * k / v of a cross-attention on the text states, or a single site).  Same layouts and padded-column contract as above; a is
 * [r][k_pad], b is [n_pad][r].  Per site the results are BIT FOR BIT those of the per-site launches they replace (same lanes
 * per row, same fold order, same fmaf chains, the same "store nothing where all eight sums are zero" rule).
 *   sites_fwd : per site D = X A^T (stored to `d` when given), Y += scale * D B^T; X is read once per call.  A site with
 *               tokens > 0 writes the transposed yt[batch][n_pad][tokens] (row stride ldy, batch stride batch_stride),
 *               rows = batch * tokens, as ctta_lora_up_add_t does.
 *   sites_bwd : per site dD = dY B (kept in `dd` when given, else in scratch); dX += scale * dD A over all sites in ONE
 *               read-modify-write of dx (sites in order, rounded to bf16 after each: the bits of one ctta_lora_up_add per
 *               site; dx NULL: the input takes no gradient); gb += scale * dY^T D and ga += scale * dD^T X where the site
 *               gives both gradient tensors (strides and column maps as ctta_lora_wgrad takes them; `d` is the forward's D),
 *               through per-slab partial sums in scratch and ONE fold launch, slabs in slab order: two runs give the same
 *               bits, and into a non-zero G the result is fl(G + what a zeroed G receives).  dY and X are read once each.
 * ctta_lora_sites_supported: 1 where the fused kernels take the shapes (pure host function): r in [1, 4], 1..3 sites of one
 * n_pad, k_pad and n_pad multiples of 8 up to 1536, and for a transposed destination (vt_tokens > 0) tokens, row stride and
 * batch stride multiples of 8.  Callers use the per-site launches otherwise. */
typedef struct {
  const float* a;
  const float* b;
  void* y;              /* bf16 destination */
  float* d;             /* fp32 [rows][r] or NULL */
  int ldy, n_pad;
  int tokens;           /* > 0: transposed destination */
  int64_t batch_stride;
} ctta_lora_fwd_site;
typedef struct {
  const void* dy;       /* bf16 [rows][lddy] */
  const float* a;
  const float* b;
  const float* d;       /* the forward's D; read when ga / gb are given */
  float* dd;            /* fp32 [rows][r] or NULL */
  float* ga;            /* both or neither */
  float* gb;
  const int32_t* k_map; /* ga's column map over k_pad (NULL: identity) */
  const int32_t* n_map; /* gb's column map over n_pad */
  int64_t ga_stride_r, ga_stride_k, gb_stride_r, gb_stride_k;
  int lddy, n_pad;
} ctta_lora_bwd_site;
int ctta_lora_sites_supported(int k_pad, const int* n_pad, int n_sites, int r, int vt_tokens, int vt_ldt, int64_t vt_batch_stride);
ctta_status ctta_lora_sites_fwd(const void* x, int ldx, int64_t rows, int k_pad, int r, float scale,
                                const ctta_lora_fwd_site* sites, int n_sites, void* stream);
size_t ctta_lora_sites_bwd_scratch_floats(int64_t rows, int k_pad, int n_pad, int n_sites, int r);
ctta_status ctta_lora_sites_bwd(const void* x, int ldx, void* dx, int lddx, int64_t rows, int k_pad, int r, float scale,
                                const ctta_lora_bwd_site* sites, int n_sites, float* scratch, void* stream);

/* Opt-in launch profiler (bench.py's live roofline leg): when enabled, every conv_gemm (kind 0)
 * and attention (kind 1) launch is bracketed by hipEvents on its own stream.  collect() waits
 * for the recorded launches, returns their summed duration / executed FLOPs / count, optionally
 * appends one CSV line per launch (kind,variant,m,n,k,groups,ms,tflops) and clears the log. */
/* GroupNorm statistics from the producing convolution's epilogue (default on; option "gn_fuse" = 0 /
 * ctta_set_gn_fuse(0) turn it off, process-wide, taking effect at the next engine call).  Off: a sample's result is
 * bit-identical at every batch size; on: at a fixed batch size (LABNOTES.md 4). */
void ctta_set_gn_fuse(int on);
int ctta_get_gn_fuse(void);
void ctta_prof_enable(int on);
ctta_status ctta_prof_collect(int kind, double* total_ms, double* total_flops, int64_t* launches,
                              const char* csv_path);

#ifdef __cplusplus
}
#endif
#endif /* CTTA_H */
