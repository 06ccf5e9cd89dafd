"""Evaluation suite of the reference (`audioldm_eval/`): the PANNs Cnn14 classifier on the HIP path and the metric
arithmetic on its features.

  * `Cnn14` -- audioldm_eval/feature_extractors/panns/models.py:168-323 in eval mode: waveform -> power STFT -> dB log-mel
    -> bn0 -> six ConvBlocks (conv3x3, BatchNorm, ReLU, twice; 2x2 average pooling) -> mean over frequency, max + mean over
    time -> fc1 + ReLU (the "2048" embedding) -> fc_audioset ("logits").  The twelve convolutions (40 GFLOP per 10 s clip)
    run on ctta_conv_gemm with BatchNorm folded into weights / bias and ReLU in the epilogue, the front end on
    ctta_wav_to_logmel_db (the torchlibrosa Spectrogram + LogmelFilterBank the CLAP tower already uses); state-dict keys are
    the reference's, so `Cnn14_16k_mAP=0.438.pth` loads as it is.
  * `calculate_fid` / `calculate_isc` / `calculate_kid` / `calculate_kl` -- audioldm_eval/metrics/{fid,isc,kid,kl}.py: same
    names, arguments, dictionary keys and random streams (np.random.RandomState(rng_seed)); host arithmetic on (N, 2048) /
    (N, 527) feature matrices, as in the reference (numpy / scipy there too).
  * `VGGish` -- the embedding model of the Frechet Audio Distance (metrics/fad.py:39-79).  The reference takes it from
    `torch.hub` (harritaylor/torchvggish, fad.py:53), so its sources are not in the reference tree; it is built here from the
    published definition (TensorFlow models' vggish_input.py / mel_features.py / vggish_params.py and torchvggish's `VGG`):
    16 kHz waveform -> 400-sample Hann frames at hop 160 -> |rfft_512| -> 64 HTK mel bands -> ln(x + 0.01) -> patches of
    96 frames -> six 3x3 convolutions with ReLU and four 2x2 max-poolings -> three Linear layers -> 128 numbers per 0.96 s.
    The front end runs on ctta_wav_to_vggish_logmel, the convolutions and the two wide Linear layers on ctta_conv_gemm, the
    pooling on ctta_maxpool2, the last Linear in fp32 on ctta_linear_f32; state-dict keys are torchvggish's, so the released
    `vggish-10086976.pth` loads as it is.
  * `calculate_fid` / `calculate_isc` / `calculate_kid` / `calculate_kl` / `calculate_fad` -- audioldm_eval/metrics/{fid,isc,
    kid,kl,fad}.py: same names, dictionary keys and random streams; `load_audio_task` is fad.py's own file loader.
  * `EvaluationHelper` -- audioldm_eval/eval.py:58-349: `get_featuresdict`, `calculate_metrics` on two directories of .wav
    files (or two lists of waveforms), the CLAP scores through `consistencytta_amd.clap.CLAP_Module`, the Frechet Audio
    Distance through a `VGGish` passed as `vggish_model`, the paired metrics with `paired_metrics=True`.
  * `MelPairedDataset`, `calculate_lsd`, `calculate_psnr_ssim` -- datasets/load_mel.py:32-120 and eval.py:137-179: `lsd` /
    `ssim_stft` / `psnr` / `ssim`, clip by clip between a generated file and the ground-truth file of the same name.  The
    reference takes the arithmetic from two pip packages outside its tree, `ssr_eval.metrics.AudioMetrics` and
    `skimage.metrics`; it is built here from the published definitions (restated in float64 numpy in
    tests/paired_metrics_ref.py): |librosa.stft| at n_fft = int(2048 / (44100 / sr)) = 743 (16 kHz) or 1486 (32 kHz), hop
    sr / 100, periodic Hann window, on ctta_stft_create_dft + ctta_stft_magnitude (split-bf16 GEMM); the log-spectral distance
    on ctta_lsd; skimage's `structural_similarity` (uniform 7x7 window, K1 = 0.01, K2 = 0.03, sample covariance, mean over the
    positions whose window lies inside the image) on ctta_ssim_mean with fp64 moments; the mean squared error under
    `peak_signal_noise_ratio` on ctta_psnr_mse; the normalised mels from `TacotronSTFT.fbank`.  Pairs are batched through the
    kernels in chunks.  Three choices depend on the versions of those packages and are constructor arguments of
    `EvaluationHelper`: `stft_pad_mode="reflect"` (librosa 0.9, which ssr_eval was released against; "constant" is librosa
    0.10), `stft_ssim_data_range=2.0` (skimage infers it from the float dtype of the spectrograms) and the frame count
    1 + len // hop, which for the odd n_fft = 743 takes the last frame one sample past the centre padding.

The four paired keys are computed only by a helper built with `paired_metrics=True`; otherwise they are reported as NaN, exactly
like a key the reference leaves out (eval.py:297-299 `out.get(key, nan)`), and so is frechet_audio_distance when no
`vggish_model` is given.  Resampling of files whose rate is not an integer multiple of the target (`resampy`,
load_mel.py:25-28, fad.py:33-34) is refused loudly by default; `EvaluationHelper(resample="kaiser_best")` and the loaders'
`resampler="kaiser_best"` send such files through `audio.resample`, the HIP restatement of resampy 0.4.2's kaiser_best
(built from the published definition; the package is not part of the reference tree), and the CLAP scores' 48 kHz
conversion with them.  Integer multiples keep the reference's striding either way.
"""
import os
from collections import OrderedDict

import numpy as np
import scipy.linalg
import torch

from . import _native as N
from . import spec
from .audio import TacotronSTFT
from .clap import PackedLinear, _check_cuda, _conv, _desc
from .modules import _ParamTree

__all__ = ["Cnn14", "VGGish", "EvaluationHelper", "calculate_fid", "calculate_isc", "calculate_kid", "calculate_kl",
           "calculate_fad", "read_centered_wav", "pad_short_audio", "load_audio_task", "MelPairedDataset", "WaveDataset"]


# ------------------------------------------------------------------------------------------------ classifier
class _FrontendHandle:
    """The ctta_mel_frontend handle of a model: created on first use by the model's `_create_frontend(max_batch,
    max_samples, handle)`, re-created when a larger batch or a longer clip arrives, destroyed with the model."""

    _fe = _fe_key = None

    def __del__(self):
        try:
            self._release_frontend()
        except Exception:
            pass

    def _release_frontend(self):
        if self._fe is not None:
            N.lib().ctta_mel_frontend_destroy(self._fe)
            self._fe = self._fe_key = None

    def _frontend(self, B, L):
        key = self._fe_key
        if self._fe is None or B > key[0] or L > key[1]:
            Bm, Lm = (max(B, key[0]), max(L, key[1])) if key else (B, L)
            self._release_frontend()
            h = N.c_void_p()
            N.check(self._create_frontend(Bm, Lm, h))
            self._fe, self._fe_key = h, (Bm, Lm)
        return self._fe


class Cnn14(_FrontendHandle, _ParamTree):
    """`Cnn14(features_list, sample_rate, window_size, hop_size, mel_bins, fmin, fmax, classes_num)` of the reference,
    eval mode (no SpecAugment, mixup or dropout: eval.py:83 calls `.eval()`), without the checkpoint download of its
    constructor (models.py:236-253): load the released state dict with `load_state_dict(torch.load(...)["model"])`."""

    def __init__(self, features_list=("2048", "logits"), sample_rate=16000, window_size=512, hop_size=160, mel_bins=64,
                 fmin=50, fmax=8000, classes_num=527):
        super().__init__()
        self.features_list = list(features_list)
        self.cfg = dict(sample_rate=sample_rate, n_fft=window_size, hop=hop_size, mel_bins=mel_bins, fmin=fmin, fmax=fmax,
                        classes_num=classes_num, widths=list(spec.CNN14_16K_CONFIG["widths"]))
        self._register(spec.cnn14_param_spec(self.cfg))
        self.requires_grad_(False)
        self._packed = self._packed_ver = None
        self._fe = self._fe_key = None

    @property
    def device(self):
        return self.get_parameter("fc1.weight").device

    def load_state_dict(self, state_dict, strict=True):
        """A released checkpoint also holds `num_batches_tracked` counters (structural here); torchlibrosa's frozen STFT /
        mel matrices are accepted and ignored -- the front end derives its own."""
        keep = OrderedDict((k, v) for k, v in state_dict.items() if not k.endswith("num_batches_tracked"))
        if strict:
            for k in spec.CNN14_STRUCTURAL:
                keep.setdefault(k, self.get_parameter(k).detach())
        return super().load_state_dict(keep, strict=strict)

    def init_deterministic(self, seed=0, prefix="cnn14."):
        with torch.no_grad():
            for k, p in self.named_parameters():
                if k not in spec.CNN14_STRUCTURAL:
                    p.copy_(torch.from_numpy(spec.cnn14_det_weight(prefix + k, tuple(p.shape), seed)).to(p.device))
        return self

    def _create_frontend(self, max_batch, max_samples, h):
        c = self.cfg
        return N.lib().ctta_mel_frontend_create(c["n_fft"], c["hop"], c["n_fft"], c["mel_bins"], c["sample_rate"],
                                                float(c["fmin"]), float(c["fmax"]), max_batch, max_samples, h)

    def _pack(self):
        ver = self._weights_version()
        if self._packed is not None and self._packed_ver == ver:
            return self._packed
        sd = {k: p.detach() for k, p in self.named_parameters()}
        for k, p in sd.items():
            _check_cuda(p, "parameter '%s'" % k)

        def bn_affine(p):        # BatchNorm2d in eval mode, eps 1e-5 (nn.BatchNorm2d default, models.py:53-54,224)
            scale = sd[p + "weight"].float() / torch.sqrt(sd[p + "running_var"].float() + 1e-5)
            return scale, sd[p + "bias"].float() - sd[p + "running_mean"].float() * scale

        P = {}
        P["bn0"] = tuple(t.contiguous() for t in bn_affine("bn0."))
        cin = 1
        for i, c in enumerate(self.cfg["widths"]):
            p = "conv_block%d." % (i + 1)
            for j, ci in ((1, cin), (2, c)):
                cp = max(8, ci)                              # NHWC channel count of the layer's input (1 -> 8)
                colmap = [-1] * (9 * cp)
                for t in range(9):
                    for ch in range(ci):
                        colmap[t * cp + ch] = ch * 9 + t     # (cout, cin, kh, kw) rows -> (kh, kw, c) columns
                scale, shift = bn_affine(p + "bn%d." % j)
                w = sd[p + "conv%d.weight" % j].float().reshape(c, ci * 9) * scale[:, None]
                P[p + "conv%d" % j] = PackedLinear(w, shift, list(range(c)), colmap, need_grad=False)
            cin = c
        self._packed, self._packed_ver = P, ver
        return P

    def forward(self, input, mixup_lambda=None):
        """input: (batch_size, data_length) waveform at cfg['sample_rate'] on the GPU -> {"logits", "2048",
        "clipwise_output"} fp32, the reference's output dictionary (models.py:315-321)."""
        if self.training:
            raise N.CttaError("Cnn14 is built for evaluation only (the reference calls .eval(), eval.py:83): SpecAugment, "
                              "mixup and dropout of the training mode are not implemented")
        wav = input.contiguous().float()
        _check_cuda(wav, "waveform")
        P = self._pack()
        c = self.cfg
        B, L = wav.shape
        L_ = N.lib()
        s = N.stream_ptr()
        frames, F = L // c["hop"] + 1, c["mel_bins"]
        if frames < 32 or F < 32:
            raise ValueError("%d frames x %d mel bins: five 2x2 poolings need at least 32 of each" % (frames, F))
        lm = torch.empty(B, frames, F, dtype=torch.float32, device=wav.device)
        N.check(L_.ctta_wav_to_logmel_db(self._frontend(B, L), N.ptr(wav), B, L, 1e-10, N.ptr(lm), s))
        x = torch.empty(B, frames, F, 8, dtype=torch.bfloat16, device=wav.device)
        N.check(L_.ctta_logmel_to_image(N.ptr(lm), B, frames, F, N.ptr(P["bn0"][0]), N.ptr(P["bn0"][1]), N.ptr(x), s))
        H, W, cp = frames, F, 8
        for i, width in enumerate(c["widths"]):
            p = "conv_block%d." % (i + 1)
            for j in (1, 2):
                W_ = P[p + "conv%d" % j]
                y = torch.empty(B, H, W, width, dtype=torch.bfloat16, device=wav.device)
                _conv(_desc(x0=x, c0=cp, batch=B, hi=H, wi=W, ho=H, wo=W, kh=3, kw=3, pad_h=1, pad_w=1, w=W_.w,
                            k_pad=W_.k_pad, n=W_.n, bias=W_.bias, out=y, ldc=width, out_act=3, out_slope=0.0))   # ReLU
                x, cp = y, width
            if i < len(c["widths"]) - 1:      # pool_size (2, 2); conv_block6 pools (1, 1) = identity (models.py:302)
                y = torch.empty(B, H // 2, W // 2, width, dtype=torch.bfloat16, device=wav.device)
                N.check(L_.ctta_avgpool2(N.ptr(x), N.ptr(y), B, H, W, width, s))
                x, H, W = y, H // 2, W // 2
        pooled = torch.empty(B, cp, dtype=torch.float32, device=wav.device)
        N.check(L_.ctta_cnn14_head(N.ptr(x), B, H, W, cp, N.ptr(pooled), s))
        sd = dict(self.named_parameters())
        emb = torch.empty(B, cp, dtype=torch.float32, device=wav.device)
        logits = torch.empty(B, c["classes_num"], dtype=torch.float32, device=wav.device)
        for r0 in range(0, B, 1024):          # ctta_linear_f32 takes <= 1024 rows
            r1 = min(B, r0 + 1024)
            N.check(L_.ctta_linear_f32(N.ptr(pooled[r0:r1]), N.ptr(sd["fc1.weight"]), N.ptr(sd["fc1.bias"]), N.ptr(emb[r0:r1]),
                                       r1 - r0, cp, cp, 0, 0, s))
        emb.clamp_(min=0)                     # F.relu_ (models.py:313)
        for r0 in range(0, B, 1024):
            r1 = min(B, r0 + 1024)
            N.check(L_.ctta_linear_f32(N.ptr(emb[r0:r1]), N.ptr(sd["fc_audioset.weight"]), N.ptr(sd["fc_audioset.bias"]),
                                       N.ptr(logits[r0:r1]), r1 - r0, c["classes_num"], cp, 0, 0, s))
        return {"logits": logits, "2048": emb, "clipwise_output": torch.sigmoid(logits)}


class VGGish(_FrontendHandle, _ParamTree):
    """torchvggish's `VGG` as metrics/fad.py:46-60 configures it (`use_pca=False, use_activation=False`: no PCA / quantisation
    post-processor, the ReLU behind the last Linear removed), eval mode, without the hub download: load the released state
    dict with `load_state_dict(torch.load("vggish-10086976.pth"))`."""

    def __init__(self, use_pca=False, use_activation=False):
        super().__init__()
        if use_pca:
            raise N.CttaError("VGGish(use_pca=True): the PCA / quantisation post-processor is not built (fad.py:54-55 "
                              "switches it off)")
        self.use_activation = bool(use_activation)
        self.cfg = dict(spec.VGGISH_CONFIG)
        self._register(spec.vggish_param_spec())
        self.requires_grad_(False)
        self._packed = self._packed_ver = None
        self._fe = self._fe_key = None

    @property
    def device(self):
        return self.get_parameter("embeddings.4.weight").device

    def load_state_dict(self, state_dict, strict=True):
        """torchvggish keys; the `pproc.*` PCA tables of a hub-built model are accepted and ignored."""
        keep = OrderedDict((k, v) for k, v in state_dict.items() if not k.startswith("pproc."))
        return super().load_state_dict(keep, strict=strict)

    def init_deterministic(self, seed=0, prefix="vggish."):
        with torch.no_grad():
            for k, p in self.named_parameters():
                p.copy_(torch.from_numpy(spec.vggish_det_weight(prefix + k, tuple(p.shape), seed)).to(p.device))
        return self

    def n_examples(self, n_samples):
        """96-frame examples of a clip of `n_samples` samples (vggish_input.waveform_to_examples: frames of 400 at hop 160
        without padding, examples at hop 96, the incomplete tail dropped)."""
        c = self.cfg
        if n_samples < c["window"]:
            return 0
        return (1 + (n_samples - c["window"]) // c["hop"]) // c["example_frames"]

    def _create_frontend(self, max_batch, max_samples, h):
        return N.lib().ctta_vggish_frontend_create(max_batch, max_samples, h)

    def _pack(self):
        ver = self._weights_version()
        if self._packed is not None and self._packed_ver == ver:
            return self._packed
        sd = {k: p.detach() for k, p in self.named_parameters()}
        for k, p in sd.items():
            _check_cuda(p, "parameter '%s'" % k)
        P = {}
        for i, ci, co in self.cfg["convs"]:
            cp = max(8, ci)                                  # NHWC channel count of the layer's input (1 -> 8)
            colmap = [-1] * (9 * cp)
            for t in range(9):
                for ch in range(ci):
                    colmap[t * cp + ch] = ch * 9 + t         # (cout, cin, kh, kw) rows -> (kh, kw, c) columns
            w = sd["features.%d.weight" % i].float().reshape(co, ci * 9)
            P["features.%d" % i] = PackedLinear(w, sd["features.%d.bias" % i], list(range(co)), colmap, need_grad=False)
        for i, ci, co in self.cfg["linears"][:2]:
            # torchvggish flattens (N, 512, 6, 4) in (frame, mel, channel) order: the NHWC activation as it lies in memory
            P["embeddings.%d" % i] = PackedLinear(sd["embeddings.%d.weight" % i].float(), sd["embeddings.%d.bias" % i],
                                                  list(range(co)), list(range(ci)), need_grad=False)
        P["unit"] = (torch.ones(self.cfg["mel_bins"], dtype=torch.float32, device=self.device),
                     torch.zeros(self.cfg["mel_bins"], dtype=torch.float32, device=self.device))
        self._packed, self._packed_ver = P, ver
        return P

    def logmel_examples(self, wav):
        """(B, L) fp32 at 16 kHz on the GPU -> (B * n_examples, 96, 64) fp32 log-mel patches, clip-major."""
        wav = wav.contiguous().float()
        _check_cuda(wav, "waveform")
        if wav.dim() != 2:
            raise ValueError("VGGish takes a (batch, samples) waveform, got %s" % (tuple(wav.shape),))
        B, L = wav.shape
        c = self.cfg
        ne = self.n_examples(L)
        if ne < 1:
            raise ValueError("%d samples hold no %d-frame example: 15600 samples at least" % (L, c["example_frames"]))
        lm = torch.empty(B, ne * c["example_frames"], c["mel_bins"], dtype=torch.float32, device=wav.device)
        clips = max(1, self.MAX_EXAMPLES // ne)
        for b0 in range(0, B, clips):
            b1 = min(B, b0 + clips)
            N.check(N.lib().ctta_wav_to_vggish_logmel(self._frontend(b1 - b0, L), N.ptr(wav[b0:b1]), b1 - b0, L,
                                                      N.ptr(lm[b0:b1]), N.stream_ptr()))
        return lm.view(B * ne, c["example_frames"], c["mel_bins"])

    MAX_EXAMPLES = 512      # examples per pass of the network: bounds the activations (0.4 GB behind the first convolution)

    def _features(self, lm, P):
        """lm (n, 96, 64) fp32 -> the `features` stack: bf16 (n, 6 * 4 * 512), NHWC, which is torchvggish's flatten order
        (`transpose(1, 3)`, `transpose(1, 2)`, `view`: frame, mel, channel)."""
        c = self.cfg
        L_ = N.lib()
        s = N.stream_ptr()
        dev = lm.device
        n, H, W = lm.shape
        x = torch.empty(n, H, W, 8, dtype=torch.bfloat16, device=dev)
        N.check(L_.ctta_logmel_to_image(N.ptr(lm), n, H, W, N.ptr(P["unit"][0]), N.ptr(P["unit"][1]), N.ptr(x), s))
        cp = 8
        for i, ci, co in c["convs"]:
            W_ = P["features.%d" % i]
            y = torch.empty(n, H, W, co, dtype=torch.bfloat16, device=dev)
            _conv(_desc(x0=x, c0=cp, batch=n, hi=H, wi=W, ho=H, wo=W, kh=3, kw=3, pad_h=1, pad_w=1, w=W_.w, k_pad=W_.k_pad,
                        n=W_.n, bias=W_.bias, out=y, ldc=co, out_act=3, out_slope=0.0))                            # ReLU
            x, cp = y, co
            if i in c["pool_after"]:
                y = torch.empty(n, H // 2, W // 2, co, dtype=torch.bfloat16, device=dev)
                N.check(L_.ctta_maxpool2(N.ptr(x), N.ptr(y), n, H, W, co, s))
                x, H, W = y, H // 2, W // 2
        return x.view(n, H * W * cp)

    def _embeddings(self, x, out, P):
        """bf16 (n, 12288) -> the `embeddings` stack without its last ReLU: out (n, 128) fp32.  The two wide layers are 1x1
        launches of the convolution family with ReLU; the last one runs in fp32, so the embedding is not rounded to bf16."""
        c = self.cfg
        L_ = N.lib()
        s = N.stream_ptr()
        n = x.shape[0]
        for i, ci, co in c["linears"][:2]:
            W_ = P["embeddings.%d" % i]
            assert x.shape[1] == W_.k_pad, (tuple(x.shape), W_.k_pad)
            y = torch.empty(n, co, dtype=torch.bfloat16, device=x.device)
            _conv(_desc(x0=x, c0=W_.k_pad, batch=1, hi=n, wi=1, ho=n, wo=1, w=W_.w, k_pad=W_.k_pad, n=W_.n, bias=W_.bias, out=y,
                        ldc=co, out_act=3, out_slope=0.0))
            x = y
        i, ci, co = c["linears"][2]
        x32 = x.float()
        w, b = self.get_parameter("embeddings.%d.weight" % i), self.get_parameter("embeddings.%d.bias" % i)
        for r0 in range(0, n, 1024):                         # ctta_linear_f32 takes <= 1024 rows
            r1 = min(n, r0 + 1024)
            N.check(L_.ctta_linear_f32(N.ptr(x32[r0:r1]), N.ptr(w), N.ptr(b), N.ptr(out[r0:r1]), r1 - r0, co, ci, 0, 0, s))

    def forward(self, wav):
        """wav: (B, L) fp32 waveform at 16 kHz on the GPU -> (B * n_examples(L), 128) fp32 embeddings, clip-major rows
        (what `model.forward(audio, sr)` of fad.py:76 returns per file, stacked)."""
        if self.training:
            raise N.CttaError("VGGish is built for evaluation only (fad.py:60 calls .eval())")
        P = self._pack()
        lm = self.logmel_examples(wav)
        total = lm.shape[0]
        out = torch.empty(total, self.cfg["embedding"], dtype=torch.float32, device=lm.device)
        for e0 in range(0, total, self.MAX_EXAMPLES):
            e1 = min(total, e0 + self.MAX_EXAMPLES)
            self._embeddings(self._features(lm[e0:e1], P), out[e0:e1], P)
        if self.use_activation:
            out.clamp_(min=0)
        return out


# ------------------------------------------------------------------------------------------------ metrics
def _frechet_distance(f1, f2, what, imag_error):
    """Frechet distance between the Gaussians fitted to two (N, D) numpy feature sets: the stable form shared by
    metrics/fid.py:20-65 and metrics/fad.py:81-144 (they differ in the exception an imaginary square root raises)."""
    eps = 1e-6
    mu1, sigma1 = np.atleast_1d(np.mean(f1, axis=0)), np.atleast_2d(np.cov(f1, rowvar=False))
    mu2, sigma2 = np.atleast_1d(np.mean(f2, axis=0)), np.atleast_2d(np.cov(f2, rowvar=False))
    assert mu1.shape == mu2.shape, "Training and test mean vectors have different lengths"
    assert sigma1.shape == sigma2.shape, "Training and test covariances have different dimensions"
    diff = mu1 - mu2
    covmean, _ = scipy.linalg.sqrtm(sigma1.dot(sigma2), disp=False)        # the product might be almost singular
    if not np.isfinite(covmean).all():
        print("WARNING: %s calculation produces singular product; adding %g to the covariance diagonal" % (what, eps))
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = scipy.linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):                                           # numerical error: slight imaginary component
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise imag_error("Imaginary component {}".format(np.max(np.abs(covmean.imag))))
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


def calculate_fid(featuresdict_1, featuresdict_2, feat_layer_name):
    """metrics/fid.py:7-67: Frechet distance between the Gaussians fitted to two (N, D) feature sets."""
    features_1, features_2 = featuresdict_1[feat_layer_name], featuresdict_2[feat_layer_name]
    assert torch.is_tensor(features_1) and features_1.dim() == 2
    assert torch.is_tensor(features_2) and features_2.dim() == 2
    return {"frechet_distance": _frechet_distance(features_1.cpu().numpy(), features_2.cpu().numpy(), "fid", AssertionError)}


def calculate_fad(embds_gen, embds_gt):
    """metrics/fad.py:146-168 behind the embeddings: (N, 128) VGGish embeddings of the generated and the ground-truth set
    (tensors or arrays) -> {"frechet_audio_distance"}; -1 when a side is empty, like the reference."""
    g = embds_gen.detach().cpu().numpy() if torch.is_tensor(embds_gen) else np.asarray(embds_gen)
    t = embds_gt.detach().cpu().numpy() if torch.is_tensor(embds_gt) else np.asarray(embds_gt)
    if len(g) == 0:
        print("[Frechet Audio Distance] generated dir is empty, exitting...")
        return -1
    if len(t) == 0:
        print("[Frechet Audio Distance] ground truth dir is empty, exitting...")
        return -1
    return {"frechet_audio_distance": _frechet_distance(g, t, "fad", ValueError)}


def calculate_isc(featuresdict, feat_layer_name, rng_seed, samples_shuffle, splits):
    """metrics/isc.py:5-32: inception score of (N, C) logits over `splits` consecutive chunks (float64)."""
    features = featuresdict[feat_layer_name]
    assert torch.is_tensor(features) and features.dim() == 2
    n = features.shape[0]
    features = features.cpu()
    if samples_shuffle:
        rng = np.random.RandomState(rng_seed)
        features = features[rng.permutation(n), :]
    features = features.double()
    p, log_p = features.softmax(dim=1), features.log_softmax(dim=1)
    scores = []
    for i in range(splits):
        lo, hi = i * n // splits, (i + 1) * n // splits
        p_chunk, log_p_chunk = p[lo:hi, :], log_p[lo:hi, :]
        q_chunk = p_chunk.mean(dim=0, keepdim=True)
        kl = p_chunk * (log_p_chunk - q_chunk.log())
        scores.append(kl.sum(dim=1).mean().exp().item())
    return {"inception_score_mean": float(np.mean(scores)), "inception_score_std": float(np.std(scores))}


def polynomial_kernel(X, Y, degree=3, gamma=None, coef0=1):
    if gamma in [None, "none", "null", "None"]:
        gamma = 1.0 / X.shape[1]
    return (np.matmul(X, Y.T) * gamma + coef0) ** degree


def polynomial_mmd(features_1, features_2, degree, gamma, coef0):
    """metrics/kid.py:68-104: unbiased MMD^2 estimate under the polynomial kernel."""
    k_xx = polynomial_kernel(features_1, features_1, degree=degree, gamma=gamma, coef0=coef0)
    k_yy = polynomial_kernel(features_2, features_2, degree=degree, gamma=gamma, coef0=coef0)
    k_xy = polynomial_kernel(features_1, features_2, degree=degree, gamma=gamma, coef0=coef0)
    m = k_xx.shape[0]
    assert k_xx.shape == (m, m) and k_xy.shape == (m, m) and k_yy.shape == (m, m)
    kt_xx_sum = (k_xx.sum(axis=1) - np.diagonal(k_xx)).sum()
    kt_yy_sum = (k_yy.sum(axis=1) - np.diagonal(k_yy)).sum()
    k_xy_sum = k_xy.sum(axis=0).sum()
    mmd2 = (kt_xx_sum + kt_yy_sum) / (m * (m - 1))
    mmd2 -= 2 * k_xy_sum / (m * m)
    return mmd2


def calculate_kid(featuresdict_1, featuresdict_2, subsets, subset_size, degree, gamma, coef0, rng_seed, feat_layer_name):
    """metrics/kid.py:8-60: kernel inception distance over `subsets` random subsets drawn without replacement."""
    features_1, features_2 = featuresdict_1[feat_layer_name], featuresdict_2[feat_layer_name]
    assert torch.is_tensor(features_1) and features_1.dim() == 2
    assert torch.is_tensor(features_2) and features_2.dim() == 2
    assert features_1.shape[1] == features_2.shape[1]
    for other in (features_2, features_1):
        if subset_size > len(other):
            print("WARNING: subset size (%d) is larger than feature length (%d). Using %d for both datasets"
                  % (subset_size, len(other), len(other)))
            subset_size = len(other)
    features_1, features_2 = features_1.cpu().numpy(), features_2.cpu().numpy()
    mmds = np.zeros(subsets)
    rng = np.random.RandomState(rng_seed)
    for i in range(subsets):
        f1 = features_1[rng.choice(len(features_1), subset_size, replace=False)]
        f2 = features_2[rng.choice(len(features_2), subset_size, replace=False)]
        mmds[i] = polynomial_mmd(f1, f2, degree, gamma, coef0)
    return {"kernel_inception_distance_mean": float(np.mean(mmds)), "kernel_inception_distance_std": float(np.std(mmds))}


def calculate_kl(featuresdict_1, featuresdict_2, feat_layer_name, same_name=True):
    """metrics/kl.py:36-114: KL(target || prediction) of the classifier's distributions, files paired by base name;
    returns (metrics, per-file reference KL, paths of the first set) like the reference."""
    if not same_name:
        return ({"kullback_leibler_divergence_sigmoid": float(-1), "kullback_leibler_divergence_softmax": float(-1)},
                None, None)
    EPS = 1e-6
    features_1, features_2 = featuresdict_1[feat_layer_name].cpu(), featuresdict_2[feat_layer_name].cpu()
    paths_1 = [os.path.basename(x) for x in featuresdict_1["file_path_"]]
    paths_2 = [os.path.basename(x) for x in featuresdict_2["file_path_"]]
    key_to_feats_1 = {p: f for p, f in zip(paths_1, features_1)}
    key_to_feats_2 = {p: f for p, f in zip(paths_2, features_2)}
    f1, f2 = [], []
    for key, feat_2 in key_to_feats_2.items():
        if key not in key_to_feats_1:
            print("%s is not in the generation result" % key)
            continue
        f1.append(key_to_feats_1[key])
        f2.append(feat_2)
    features_1, features_2 = torch.stack(f1, dim=0), torch.stack(f2, dim=0)
    kl_div = torch.nn.functional.kl_div
    kl_ref = kl_div((features_1.softmax(dim=1) + EPS).log(), features_2.softmax(dim=1), reduction="none") / len(features_1)
    kl_ref = torch.mean(kl_ref, dim=-1)
    kl_softmax = kl_div((features_1.softmax(dim=1) + EPS).log(), features_2.softmax(dim=1), reduction="sum") / len(features_1)
    kl_sigmoid = kl_div((features_1.sigmoid() + EPS).log(), features_2.sigmoid(), reduction="sum") / len(features_1)
    return ({"kullback_leibler_divergence_sigmoid": float(kl_sigmoid),
             "kullback_leibler_divergence_softmax": float(kl_softmax)}, kl_ref, paths_1)


# ------------------------------------------------------------------------------------------------ files
def pad_short_audio(audio, min_samples=32000):
    """datasets/load_mel.py:9-14."""
    if audio.shape[-1] < min_samples:
        audio = torch.nn.functional.pad(audio, (0, min_samples - audio.shape[-1]), mode="constant", value=0.0)
    return audio


def _check_resampler(resampler):
    if resampler not in (None, "kaiser_best"):
        raise ValueError("resampler must be None (refuse such files) or 'kaiser_best', got %r" % (resampler,))


def _resample_host(audio, orig_sr, target_sr, resampler):
    """resampy.resample(audio, orig_sr, target_sr, filter=resampler) (load_mel.py:25-28, fad.py:33-34) for one host clip:
    up to the current GPU as fp32, `audio.resample`, back as float64."""
    from .audio import resample
    x = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).cuda()
    return resample([x], orig_sr, target_sr, filter=resampler)[0].cpu().numpy().astype(np.float64)


def read_centered_wav(audio_file, target_sr, resampler=None):
    """datasets/load_mel.py:17-29 with scipy.io.wavfile in place of soundfile: first channel mix-down, integer-ratio
    decimation by plain striding (as the reference does), mean removed; PCM widths scaled to [-1, 1) like soundfile.
    Any other rate is refused unless `resampler="kaiser_best"`, which resamples it as the reference does, on the GPU."""
    _check_resampler(resampler)
    from scipy.io import wavfile
    orig_sr, audio = wavfile.read(audio_file)
    if audio.dtype.kind == "i":
        audio = audio.astype(np.float64) / float(2 ** (8 * audio.dtype.itemsize - 1))
    elif audio.dtype.kind == "u":                            # 8-bit PCM is unsigned
        audio = (audio.astype(np.float64) - 128.0) / 128.0
    else:
        audio = audio.astype(np.float64)
    if audio.ndim > 1:
        audio = audio.mean(axis=1)                           # librosa.to_mono
    if orig_sr != target_sr and orig_sr % target_sr == 0:
        audio = audio[..., ::(orig_sr // target_sr)]
    elif orig_sr != target_sr and resampler is not None:
        audio = _resample_host(audio, orig_sr, target_sr, resampler)
    elif orig_sr != target_sr:
        raise N.CttaError("%s: %d Hz is not an integer multiple of %d Hz; the reference resamples such files with resampy "
                          "(kaiser_best) -- pass resampler='kaiser_best' or resample the directory first"
                          % (audio_file, orig_sr, target_sr))
    return audio - audio.mean()


def load_audio_task(fname, target_sr=16000, target_length=1000, resampler=None):
    """metrics/fad.py:22-36, the Frechet Audio Distance's own loader, with scipy.io.wavfile in place of soundfile: samples as
    int16 / 32768, MEAN over the channels, integer-ratio decimation by plain striding, cut to `target_length` centiseconds;
    the mean is NOT removed (unlike `read_centered_wav`: the two loaders differ in the reference too).  float64 array.
    `resampler`: as in `read_centered_wav`."""
    from scipy.io import wavfile
    _check_resampler(resampler)
    orig_sr, audio = wavfile.read(fname)
    if audio.dtype != np.int16:
        raise N.CttaError("%s holds %s samples: only 16-bit PCM is read (the reference converts other widths with soundfile's "
                          "dtype='int16' read, which is not rebuilt)" % (fname, audio.dtype))
    audio = audio / 32768.0
    if audio.ndim > 1:
        audio = np.mean(audio, axis=1)
    if orig_sr % target_sr == 0:
        audio = audio[::(orig_sr // target_sr)]
    elif resampler is not None:
        audio = _resample_host(audio, orig_sr, target_sr, resampler)
    else:
        raise N.CttaError("%s: %d Hz is not an integer multiple of %d Hz; the reference resamples such files with resampy "
                          "(kaiser_best) -- pass resampler='kaiser_best' or resample the directory first"
                          % (fname, orig_sr, target_sr))
    return audio[:int(target_length * target_sr / 100)]


class WaveDataset:
    """datasets/load_mel.py:123-151: sorted .wav files of a directory -> (waveform (1, n) fp32, base name)."""

    def __init__(self, datadir, sr=16000, target_length=1000, limit_num=None, resampler=None):
        _check_resampler(resampler)
        self.resampler = resampler
        self.datalist = sorted(os.path.join(datadir, x) for x in os.listdir(datadir))
        self.datalist = [x for x in self.datalist if x.endswith(".wav")]
        if limit_num is not None:
            self.datalist = self.datalist[:limit_num]
        self.sr, self.target_length = sr, target_length

    def __len__(self):
        return len(self.datalist)

    def __getitem__(self, index):
        filename = self.datalist[index]
        audio = torch.from_numpy(read_centered_wav(filename, self.sr, self.resampler)).float()[None]
        audio = pad_short_audio(audio[..., :int(self.sr * self.target_length / 100)], min_samples=32000)
        if audio.shape[-1] < 1:
            raise ValueError("empty file %s" % filename)
        return audio, os.path.basename(filename)


def _normalised_mels(stft, audios):
    """datasets/load_mel.py:100-120 for a list of float64 waveforms: clip to [-1, 1], `stft.fbank` (the natural log of the
    clamped mel magnitudes) -> log10 -> clip((20 x - 20 + 100) / 100, 0, 1).  Clips of equal length share a launch.  Returns
    one (n_mels, frames) fp32 GPU tensor per waveform (a transposed view of the front end's (frames, n_mels) rows)."""
    out = [None] * len(audios)
    order = sorted(range(len(audios)), key=lambda i: len(audios[i]))
    i = 0
    while i < len(order):
        n = len(audios[order[i]])
        j = i
        while j < len(order) and j - i < 32 and len(audios[order[j]]) == n:
            j += 1
        wav = torch.from_numpy(np.stack([audios[order[k]] for k in range(i, j)])).float().clip(-1, 1)
        fb, _ = stft.fbank(wav, want_logmag=False)
        mel = fb / float(np.log(10.0))                       # normalize_fun=torch.log10 on the same clamp(m, 1e-5)
        mel = (((mel * 20) - 20) + 100) / 100
        mel = torch.clip(mel, min=0, max=1.0)
        for k in range(i, j):
            out[order[k]] = mel[k - i].t()
        i = j
    return out


class MelPairedDataset:
    """datasets/load_mel.py:32-120: the .wav files two directories have in common, by base name (sorted; the reference
    iterates a set) -> (generated mel, ground-truth mel, base name, (generated audio, ground-truth audio)).  The mels are the
    normalised (n_mels, frames) float32 arrays of `get_mel_from_wav`, cut to the shorter of the two; the audio is what
    `read_centered_wav` returns, whole.  `_stft`: a `TacotronSTFT` on the GPU (None: no mels).  `fbin_mean`, `fbin_std` and
    `augment` are accepted and unused, as in the reference.  `EvaluationHelper` reads the audio through `audio_pair` and
    batches the mels itself instead of indexing pair by pair."""

    def __init__(self, datadir1, datadir2, _stft, sr=16000, fbin_mean=None, fbin_std=None, augment=False, limit_num=None,
                 resampler=None):
        _check_resampler(resampler)
        self.resampler = resampler
        lists = []
        for d in (datadir1, datadir2):
            files = [x for x in sorted(os.path.join(d, x) for x in os.listdir(d)) if x.endswith(".wav")]
            lists.append(files[:limit_num] if limit_num is not None else files)
        d1, d2 = ({os.path.basename(x): x for x in files} for files in lists)
        keys = sorted(set(d1) & set(d2))
        self.datalist1, self.datalist2 = [d1[k] for k in keys], [d2[k] for k in keys]
        self._stft, self.sr, self.augment = _stft, sr, augment

    def __len__(self):
        return len(self.datalist1)

    def name(self, index):
        return os.path.basename(self.datalist1[index])

    def audio_pair(self, index):
        return (read_centered_wav(self.datalist1[index], self.sr, self.resampler),
                read_centered_wav(self.datalist2[index], self.sr, self.resampler))

    def get_mel_from_wav(self, audio):
        return _normalised_mels(self._stft, [np.asarray(audio, dtype=np.float64)])[0].cpu().numpy(), None

    def get_mel_from_file(self, audio_file):
        audio = read_centered_wav(audio_file, self.sr, self.resampler)
        melspec, energy = self.get_mel_from_wav(audio) if self._stft is not None else (None, None)
        return melspec, energy, audio

    def __getitem__(self, index):
        mel1, _, audio1 = self.get_mel_from_file(self.datalist1[index])
        mel2, _, audio2 = self.get_mel_from_file(self.datalist2[index])
        if mel1 is not None:
            min_len = min(mel1.shape[-1], mel2.shape[-1])
            mel1, mel2 = mel1[..., :min_len], mel2[..., :min_len]
        return mel1, mel2, self.name(index), (audio1, audio2)


class _DftMagnitude:
    """|librosa.stft(x, n_fft, hop, window="hann", center=True, pad_mode)| on a ctta_stft_create_dft handle, which grows with
    the largest batch and the longest clip it has seen."""

    def __init__(self, n_fft, hop, pad_mode):
        if pad_mode not in ("reflect", "constant"):
            raise ValueError("stft_pad_mode must be 'reflect' (librosa 0.9) or 'constant' (librosa 0.10), got %r" % (pad_mode,))
        self.n_fft, self.hop, self.pad_zero = int(n_fft), int(hop), int(pad_mode == "constant")
        self._h = self._key = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _release(self):
        if self._h is not None:
            N.lib().ctta_stft_destroy(self._h)
            self._h = self._key = None

    def __call__(self, wav):
        """(B, n) fp32 on the GPU -> (B, 1 + n // hop, 1 + n_fft // 2) fp32."""
        _check_cuda(wav, "waveform")
        B, n = wav.shape
        key = self._key
        if self._h is None or B > key[0] or n > key[1] or key[2] != wav.device:
            Bm, nm = (max(B, key[0]), max(n, key[1])) if key and key[2] == wav.device else (B, n)
            self._release()
            h = N.c_void_p()
            with torch.cuda.device(wav.device):
                N.check(N.lib().ctta_stft_create_dft(self.n_fft, self.hop, self.pad_zero, Bm, nm, h))
            self._h, self._key = h, (Bm, nm, wav.device)
        mag = torch.empty(B, n // self.hop + 1, self.n_fft // 2 + 1, dtype=torch.float32, device=wav.device)
        with torch.cuda.device(wav.device):
            N.check(N.lib().ctta_stft_magnitude(self._h, N.ptr(wav), B, n, N.ptr(mag), N.stream_ptr()))
        return mag


def _lengths(values):
    return (N.c_int32 * len(values))(*values)


def _ssim_mean(x, y, rows, win, data_range):
    """ctta_ssim_mean on two (P, h_max, w) fp32 GPU tensors with `rows[p]` valid rows -> P float64 numbers on the host."""
    P, h_max, w = x.shape
    L_ = N.lib()
    out = torch.empty(P, dtype=torch.float64, device=x.device)
    ws = torch.empty(P * max(1, L_.ctta_ssim_tiles(h_max, w, win)), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        N.check(L_.ctta_ssim_mean(N.ptr(x), N.ptr(y), P, h_max, w, _lengths(rows), win, float(data_range), 1, N.ptr(out),
                                  N.ptr(ws), N.stream_ptr()))
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ driver
class EvaluationHelper:
    """eval.py:58-349 for the metrics this build computes.  `clap_model`: a `consistencytta_amd.clap.CLAP_Module` (or None
    to skip the three CLAP scores); the reference constructs one from `ckpt/music_audioset_epoch_15_esc_90.14.pt`.
    `vggish_model`: a `VGGish` holding the released torchvggish weights (or None to leave `frechet_audio_distance` NaN); the
    reference downloads one through `torch.hub` (eval.py:65, metrics/fad.py:53).  `paired_metrics=True` computes `lsd`,
    `ssim_stft`, `psnr` and `ssim` (eval.py:137-179) on the HIP path; the default leaves them NaN.  Their version-dependent
    choices: `stft_pad_mode` -- the centre padding of the LSD's |librosa.stft|, "reflect" (librosa 0.9, which `ssr_eval` was
    released against) or "constant" (librosa 0.10); `stft_ssim_data_range` -- the data range of `ssim_stft`, 2.0 being what
    skimage infers for a float image.  `resample="kaiser_best"`: files whose rate is not an integer multiple of the target
    are resampled as the reference does (resampy's kaiser_best on the HIP path, `audio.resample`) instead of refused, and
    the CLAP scores' 16 -> 48 kHz conversion uses it too; None keeps both as they were."""

    KEYS = ["frechet_distance", "frechet_audio_distance", "lsd", "psnr", "kullback_leibler_divergence_sigmoid",
            "kullback_leibler_divergence_softmax", "ssim", "ssim_stft", "inception_score_mean", "inception_score_std",
            "kernel_inception_distance_mean", "kernel_inception_distance_std", "gt_text_clap_score", "gen_text_clap_score",
            "gen_gt_clap_score"]

    PAIR_CHUNK = 32         # pairs per pass of the paired metrics: 64 clips through the STFT (0.5 GB of frames at 10 s, 16 kHz)
    SSIM_WIN = 7            # skimage's default win_size

    def __init__(self, sampling_rate, device, backbone="cnn14", mel_model=None, clap_model=None, vggish_model=None,
                 paired_metrics=False, stft_pad_mode="reflect", stft_ssim_data_range=2.0, resample=None):
        self.device, self.backbone, self.sampling_rate = device, backbone, sampling_rate
        if sampling_rate not in (16000, 32000):
            raise ValueError("We only support the evaluation on 16kHz and 32kHz sampling rates.")
        if mel_model is None:
            c = spec.CNN14_16K_CONFIG if sampling_rate == 16000 else spec.CNN14_32K_CONFIG
            mel_model = Cnn14(features_list=["2048", "logits"], sample_rate=c["sample_rate"], window_size=c["n_fft"],
                              hop_size=c["hop"], mel_bins=c["mel_bins"], fmin=c["fmin"], fmax=c["fmax"],
                              classes_num=c["classes_num"]).to(device)
        self.mel_model = mel_model.eval()
        self.clap_model = clap_model
        self.vggish_model = vggish_model.eval() if vggish_model is not None else None
        self.paired_metrics = bool(paired_metrics)
        _check_resampler(resample)
        self.resample = resample
        self.stft_pad_mode, self.stft_ssim_data_range = stft_pad_mode, float(stft_ssim_data_range)
        if self.stft_ssim_data_range <= 0.0:
            raise ValueError("stft_ssim_data_range must be positive, got %r" % (stft_ssim_data_range,))
        # AudioMetrics(rate) of ssr_eval: n_fft = int(2048 / (44100 / rate)), hop = int(rate / 100) (eval.py:66)
        self._lsd_stft = _DftMagnitude(int(2048 / (44100 / sampling_rate)), int(sampling_rate / 100), stft_pad_mode)
        self._stft = None       # eval.py:89-98, built with the first paired pass

    def file_init_check(self, dir):
        assert os.path.exists(dir), "The path does not exist %s" % dir
        assert len(os.listdir(dir)) > 1, "There is no files in %s" % dir

    def get_filename_intersection_ratio(self, dir1, dir2, threshold=0.99, limit_num=None):
        k1 = {os.path.basename(x) for x in os.listdir(dir1) if x.endswith(".wav")}
        k2 = {os.path.basename(x) for x in os.listdir(dir2) if x.endswith(".wav")}
        both = k1 & k2
        return len(both) / len(k1) > threshold and len(both) / len(k2) > threshold

    def get_featuresdict(self, dataloader):
        """eval.py:310-330: an iterable of (waveform (1, n) or (n,), file name) -> {"2048", "logits", "clipwise_output":
        (N, .) CPU tensors, "file_path_": names}.  Clips of equal length go through the classifier together."""
        items = [(w.reshape(-1).float(), name) for w, name in dataloader]
        feats = {}
        order = sorted(range(len(items)), key=lambda i: items[i][0].numel())
        i = 0
        with torch.no_grad():
            while i < len(order):
                n = items[order[i]][0].numel()
                j = i
                while j < len(order) and j - i < 32 and items[order[j]][0].numel() == n:
                    j += 1
                out = self.mel_model(torch.stack([items[order[k]][0] for k in range(i, j)]).to(self.device))
                for k in range(i, j):
                    feats[order[k]] = {key: v[k - i].cpu() for key, v in out.items()}
                i = j
        res = {key: torch.stack([feats[i][key] for i in range(len(items))]) for key in ("2048", "logits", "clipwise_output")}
        res["file_path_"] = [name for _, name in items]
        return res

    def get_vggish_embeddings(self, datadir, target_length=1000):
        """metrics/fad.py:62-79: the VGGish embeddings of every .wav file of a directory, loaded by `load_audio_task` at
        16 kHz whatever the helper's own rate is (fad.py:62), stacked in file order -> (N, 128) CPU tensor.  Clips of equal
        length go through the model together; a file too short for one 0.96 s example contributes no rows."""
        from scipy.io import wavfile
        m = self.vggish_model
        paths = [os.path.join(datadir, f) for f in sorted(os.listdir(datadir)) if f.endswith(".wav")]
        limit = int(target_length * 16000 / 100)

        def length(path):                                    # samples `load_audio_task` will return, from the header alone
            sr, data = wavfile.read(path, mmap=True)
            if sr % 16000 == 0:
                return min(-(-data.shape[0] // (sr // 16000)), limit)
            return min(int(data.shape[0] * 16000 / sr), limit) if self.resample is not None else limit   # else: it raises

        lengths = [length(p) for p in paths]
        order = sorted((i for i in range(len(paths)) if m.n_examples(lengths[i]) > 0), key=lambda i: lengths[i])
        embds = {}
        i = 0
        with torch.no_grad():
            while i < len(order):                            # one batch of files in host memory at a time
                j = i
                while j < len(order) and j - i < 32 and lengths[order[j]] == lengths[order[i]]:
                    j += 1
                waves = [torch.from_numpy(load_audio_task(paths[order[k]], 16000, target_length, self.resample)).float()
                         for k in range(i, j)]
                out = m(torch.stack(waves).to(self.device)).cpu()
                rows = out.shape[0] // (j - i)
                for k in range(i, j):
                    embds[order[k]] = out[(k - i) * rows:(k - i + 1) * rows]
                i = j
        if not embds:
            return torch.zeros(0, m.cfg["embedding"])
        return torch.cat([embds[i] for i in sorted(embds)])

    @staticmethod
    def captions_from_dataset_json(dataset_json_path):
        """{generated file name: caption} as `T2APairedDataset` pairs them (tools/t2a_dataset.py:79-87,118-119): line i of the
        json-lines file holds the caption of `output_<i>.wav`."""
        import json
        if not os.path.isfile(dataset_json_path):
            raise AssertionError("%s is not a file." % dataset_json_path)
        with open(dataset_json_path) as f:
            rows = [json.loads(line) for line in f if line.strip()]
        return {"output_%d.wav" % i: r["captions"] for i, r in enumerate(rows)}

    def calculate_metrics(self, dataset_json_path, generate_files_path, groundtruth_path, mel_path=None, same_name=True,
                          target_length=1000, limit_num=None, captions=None, subset_size=None):
        """eval.py:181-308 (same positional order) on two directories of identically named .wav files.  The captions of the
        CLAP scores come from `dataset_json_path` as in the reference (or from `captions`: {file name: text}); `mel_path`
        (pre-computed generated mels for the reference's optional mel metrics) is accepted and unused.  Returns the
        reference's dictionary, rounded to 4 digits; `lsd` / `ssim_stft` / `psnr` / `ssim` are NaN unless the helper was built
        with `paired_metrics=True`, and so is `frechet_audio_distance` without a `vggish_model`."""
        if captions is None and dataset_json_path is not None:
            captions = self.captions_from_dataset_json(dataset_json_path)
        gen_files = sorted(f for f in os.listdir(generate_files_path) if f.endswith(".wav"))
        gt_files = sorted(f for f in os.listdir(groundtruth_path) if f.endswith(".wav"))
        if gen_files != gt_files:
            raise ValueError("Generated and groundtruth diretories have different files.\nGenerated: %s;\nGround truth: %s."
                             % (gen_files, gt_files))
        sr = self.sampling_rate
        gen = WaveDataset(generate_files_path, sr, limit_num=limit_num, target_length=target_length, resampler=self.resample)
        gt = WaveDataset(groundtruth_path, sr, limit_num=limit_num, target_length=1000, resampler=self.resample)
        featuresdict_2 = self.get_featuresdict(gt[i] for i in range(len(gt)))
        featuresdict_1 = self.get_featuresdict(gen[i] for i in range(len(gen)))
        out = {}
        if self.vggish_model is not None:                    # eval.py:232-236 -> FrechetAudioDistance.score (fad.py:146-168)
            fad = calculate_fad(self.get_vggish_embeddings(generate_files_path, target_length=target_length),
                                self.get_vggish_embeddings(groundtruth_path, target_length=1000))
            out.update(fad if isinstance(fad, dict) else {"frechet_audio_distance": float(fad)})
        if self.clap_model is not None and captions is not None:
            out.update(self.clap_scores([gt[i] for i in range(len(gt))], [gen[i] for i in range(len(gen))], captions))
        metric_kl, _, _ = calculate_kl(featuresdict_1, featuresdict_2, "logits", same_name)
        out.update(metric_kl)
        out.update(calculate_isc(featuresdict_1, feat_layer_name="logits", splits=10, samples_shuffle=True, rng_seed=2020))
        out.update(calculate_kid(featuresdict_1, featuresdict_2, feat_layer_name="2048", degree=3, gamma=None, subsets=100,
                                 subset_size=len(gen) if subset_size is None else subset_size, coef0=1, rng_seed=2020))
        out.update(calculate_fid(featuresdict_1, featuresdict_2, feat_layer_name="2048"))
        if self.paired_metrics:                              # eval.py:222-228,238-240,259-263
            paired = MelPairedDataset(generate_files_path, groundtruth_path, self.mel_stft(), sr, limit_num=limit_num,
                                      resampler=self.resample)
            out.update(self.calculate_lsd(paired, same_name=same_name))
            out.update(self.calculate_psnr_ssim(paired, same_name=same_name))
        return {key: round(out.get(key, float("nan")), 4) for key in self.KEYS}

    def mel_stft(self):
        """The `TacotronSTFT` of eval.py:89-98 on the helper's device."""
        if self._stft is None:
            c = {16000: (512, 160, 512, 64, 16000, 50, 8000), 32000: (1024, 320, 1024, 64, 32000, 50, 14000)}[self.sampling_rate]
            self._stft = TacotronSTFT(*c).to(self.device)
        return self._stft

    def _pair_chunks(self, pairs, want_mel):
        """Lists of at most PAIR_CHUNK (generated mel, ground-truth mel, name, (generated audio, ground-truth audio)) items.
        A `MelPairedDataset` is read through `audio_pair` and its mels come from one batched front-end pass per chunk (GPU
        tensors); any other iterable of such tuples (a DataLoader over the dataset, as in the reference) is taken as it is."""
        if isinstance(pairs, MelPairedDataset):
            for i0 in range(0, len(pairs), self.PAIR_CHUNK):
                idx = list(range(i0, min(len(pairs), i0 + self.PAIR_CHUNK)))
                audio = [pairs.audio_pair(i) for i in idx]
                m1 = m2 = [None] * len(idx)
                if want_mel:
                    stft = pairs._stft if pairs._stft is not None else self.mel_stft()
                    m1 = _normalised_mels(stft, [a for a, _ in audio])
                    m2 = _normalised_mels(stft, [a for _, a in audio])
                yield [(m1[k], m2[k], pairs.name(i), audio[k]) for k, i in enumerate(idx)]
            return
        buf = []
        for item in pairs:
            buf.append(item)
            if len(buf) == self.PAIR_CHUNK:
                yield buf
                buf = []
        if buf:
            yield buf

    def calculate_lsd(self, pairs, same_name=True, time_offset=160 * 7):
        """eval.py:137-162 -> {"lsd", "ssim_stft"}, the means over all pairs of `AudioMetrics.lsd` and `AudioMetrics.ssim` on
        the magnitude spectrograms.  Per pair (float64 on the host, as the reference): the generated audio from `time_offset`
        on, (a - mean) / max|a| on both sides with the maximum taken before the mean is removed, both cut to the shorter.  The
        pairs of a chunk that share a length go through the STFT, ctta_lsd and ctta_ssim_mean together."""
        if not same_name:
            return {"lsd": -1, "ssim_stft": -1}
        lsd_avg, ssim_avg = [], []
        hop = self._lsd_stft.hop
        for chunk in self._pair_chunks(pairs, want_mel=False):
            by_len = {}
            for _, _, name, (a1, a2) in chunk:
                a1, a2 = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (a1, a2))
                if a1.shape[0] <= time_offset:
                    raise ValueError("%s: %d generated samples, not more than the time offset of %d" % (name, a1.shape[0], time_offset))
                a1 = a1[time_offset:]
                a1 = (a1 - a1.mean()) / np.abs(a1).max()
                a2 = (a2 - a2.mean()) / np.abs(a2).max()
                n = min(a1.shape[0], a2.shape[0])
                if 1 + n // hop < self.SSIM_WIN:
                    raise ValueError("%s: %d samples are %d frames, fewer than one %dx%d window of ssim_stft"
                                     % (name, n, 1 + n // hop, self.SSIM_WIN, self.SSIM_WIN))
                by_len.setdefault(n, []).append((a1[:n], a2[:n]))
            for n, group in sorted(by_len.items()):
                P = len(group)
                wav = torch.from_numpy(np.stack([a for a, _ in group] + [a for _, a in group])).float().to(self.device)
                mag = self._lsd_stft(wav)                    # (2 P, frames, bins): generated first, ground truth behind
                frames, bins = mag.shape[1], mag.shape[2]
                out = torch.empty(P, dtype=torch.float64, device=mag.device)
                ws = torch.empty(P * frames, dtype=torch.float64, device=mag.device)
                with torch.cuda.device(mag.device):
                    N.check(N.lib().ctta_lsd(N.ptr(mag[:P]), N.ptr(mag[P:]), P, frames, bins, _lengths([frames] * P), N.ptr(out),
                                             N.ptr(ws), N.stream_ptr()))
                lsd_avg += out.cpu().tolist()
                ssim_avg += _ssim_mean(mag[:P], mag[P:], [frames] * P, self.SSIM_WIN, self.stft_ssim_data_range).tolist()
        return {"lsd": float(np.mean(lsd_avg)), "ssim_stft": float(np.mean(ssim_avg))}

    def calculate_psnr_ssim(self, pairs, same_name=True):
        """eval.py:164-179 -> {"psnr", "ssim"}: skimage's `peak_signal_noise_ratio` (data range 1, inferred for a non-negative
        float image) and `structural_similarity(data_range=1.)` of the normalised mels, the means over the pairs whose PSNR is
        finite: a pair of identical mels is left out of both, as in the reference.  The mels of a chunk are padded to its
        longest pair and go through ctta_psnr_mse and ctta_ssim_mean together, as (frames, n_mels) images: both metrics are
        the same on a transposed image."""
        if not same_name:
            return {"psnr": -1, "ssim": -1}
        psnr_avg, ssim_avg = [], []
        win = self.SSIM_WIN
        for chunk in self._pair_chunks(pairs, want_mel=True):
            imgs, rows, names = [], [], []
            for m1, m2, name, _ in chunk:
                m1, m2 = (torch.as_tensor(m).float() for m in (m1, m2))
                m1, m2 = (m.reshape(m.shape[-2], m.shape[-1]).t().to(self.device) for m in (m1, m2))      # (frames, n_mels)
                if m1.shape[1] != m2.shape[1]:
                    raise ValueError("%s: mels of %d and %d bands" % (name, m1.shape[1], m2.shape[1]))
                h = min(m1.shape[0], m2.shape[0])
                if h < win or m1.shape[1] < win:
                    raise ValueError("%s: a mel of %d frames x %d bands holds no %dx%d window" % (name, h, m1.shape[1], win, win))
                imgs.append((m1, m2))
                rows.append(h)
                names.append(name)
            P, h_max, w = len(imgs), max(rows), imgs[0][0].shape[1]
            x = torch.zeros(2, P, h_max, w, dtype=torch.float32, device=self.device)
            for k, (m1, m2) in enumerate(imgs):
                x[0, k, :rows[k]] = m1[:rows[k]]
                x[1, k, :rows[k]] = m2[:rows[k]]
            mse = torch.empty(P, dtype=torch.float64, device=self.device)
            ws = torch.empty(P * h_max, dtype=torch.float64, device=self.device)
            with torch.cuda.device(x.device):
                N.check(N.lib().ctta_psnr_mse(N.ptr(x[0]), N.ptr(x[1]), P, h_max, w, _lengths(rows), N.ptr(mse), N.ptr(ws),
                                              N.stream_ptr()))
            ssim = _ssim_mean(x[0], x[1], rows, win, 1.0)
            for k, err in enumerate(mse.cpu().tolist()):
                if err == 0.0:
                    print("Infinite value encountered in psnr %s " % names[k])
                    continue
                psnr_avg.append(10.0 * np.log10(1.0 / err))
                ssim_avg.append(float(ssim[k]))
        return {"psnr": float(np.mean(psnr_avg)), "ssim": float(np.mean(ssim_avg))}

    def _clap_wave(self, w, seconds=10.0):
        """What `T2APairedDataset` hands the CLAP tower (tools/t2a_dataset.py:111-125 -> tools/torch_tools.py:54-75): the clip at
        48 kHz, mean removed, scaled to peak 0.5, cut / zero-padded to the segment length, scaled again.  The reference
        resamples with `resampy` (kaiser_best), which is not in its tree.  A helper built with `resample="kaiser_best"` does
        the same on the HIP path (`audio.resample` + `data.wave_prepare`, fp64 normalisation rounded once like the reference's
        `.float()`); by default the Kaiser-windowed sinc resampler of the CLAP loss (tools/losses.py:299-303 =
        `clap.Resampler`) does it and the normalisation is fp32 -- a stated deviation of the filter, not of the pipeline."""
        from .clap import Resampler
        w = w.reshape(1, -1).float().to(self.device)
        if self.resample is not None:
            from .audio import resample
            from .data import wave_prepare
            w = w[0].contiguous()
            if self.sampling_rate != 48000:
                w = resample([w], self.sampling_rate, 48000, filter=self.resample)[0]
            return wave_prepare(w, [0], [w.shape[0]], int(round(seconds * 48000)))
        if self.sampling_rate != 48000:
            if getattr(self, "_to48k", None) is None:
                self._to48k = Resampler(orig_freq=self.sampling_rate, new_freq=48000)
            w = self._to48k(w)
        w = w - w.mean()
        w = w / (w.abs().max() + 1e-8) / 2
        seg = int(round(seconds * 48000))
        w = w[:, :seg] if w.shape[1] >= seg else torch.nn.functional.pad(w, (0, seg - w.shape[1]))
        return w / (w.abs().max() + 1e-8) / 2

    def clap_scores(self, gt_items, gen_items, captions, seconds=10.0):
        """eval.py:29-55,238-253: clamped cosine similarities of CLAP embeddings (audio at 48 kHz as `_clap_wave` prepares
        it, captions through the text tower), x 100."""
        cos = torch.nn.functional.cosine_similarity
        sims = {"gt_text": [], "gen_text": [], "gen_gt": []}
        with torch.no_grad():
            for (gw, name), (xw, _) in zip(gt_items, gen_items):
                g = self.clap_model.get_audio_embedding_from_data(x=self._clap_wave(gw, seconds), use_tensor=True)
                x = self.clap_model.get_audio_embedding_from_data(x=self._clap_wave(xw, seconds), use_tensor=True)
                t = self.clap_model.get_text_embedding([captions[name]], use_tensor=True)
                sims["gt_text"].append(cos(g, t, dim=1).clamp(min=0))
                sims["gen_text"].append(cos(x, t, dim=1).clamp(min=0))
                sims["gen_gt"].append(cos(x, g, dim=1).clamp(min=0))
        return {k + "_clap_score": torch.cat(v).mean().item() * 100.0 for k, v in sims.items()}

    def main(self, dataset_json_path, generated_files_path, groundtruth_path, mel_path=None, target_length=1000,
             limit_num=None, captions=None):
        """eval.py:336-349, keyword- and position-compatible with the reference's callers (inference.py:230,
        evaluate_existing.py:54); `dataset_json_path=None` skips the CLAP scores unless `captions` is given."""
        self.file_init_check(generated_files_path)
        self.file_init_check(groundtruth_path)
        same_name = self.get_filename_intersection_ratio(generated_files_path, groundtruth_path, limit_num=limit_num)
        return self.calculate_metrics(dataset_json_path, generated_files_path, groundtruth_path, mel_path, same_name,
                                      target_length, limit_num, captions)
