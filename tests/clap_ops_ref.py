"""float64 CPU references of the CLAP tower's front-end and glue operators, the cases the operator tests run, and the
bounds those tests hold the kernels to (tests/test_clap_ops_gpu.py, tests/test_clap_ops_cpu.py).

Every reference is the plain definition of the operator in float64; the only kernel arithmetic restated here is what
the kernels document about themselves: the three-way bf16 split of the STFT operands (`split3`, `kernel_basis_f32`) and
the two bf16 roundings of the log-mel backward (`logmel_db_bwd_rounded_ref`).

Where a bound is "measured", the figure is the worst error on an MI355X (LABNOTES.md section XVI has every figure) and
the bound is the stated multiple of it; bounds that follow from a number format are written as that format's step.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import clap as oclap
from oracle import mel as omel

FRONT_CFG = dict(n_fft=1024, hop=480, mel_bins=64, sample_rate=48000, fmin=50, fmax=14000)
AMIN = 1e-10
LOGMEL_LENGTHS = (513, 600, 1024, 1447, 4801)
LOGMEL_MAX_BATCH, LOGMEL_MAX_SAMPLES = 3, 6000          # the handle is larger than every call made on it

# ---- bounds (LABNOTES.md section XVI has every measured figure)
# forward log-mel, per element in dB: measured worst 7.6e-6 dB (the floor of silent frames comes out one fp32 step
# below -100; live values are within 4.4e-6), x4.  Dropping the smallest of the six split products costs
# 7.5e-5 .. 2.5e-4 dB on the same inputs (tests/test_clap_ops_cpu.py asserts that this exceeds the bound).
LOGMEL_FWD_DB = 3.1e-5
# log-mel backward, per element relative to max |ref| (over all samples, and again over the halo samples alone).
# Against the reference with the kernel's two bf16 roundings restated: measured worst 1.4e-5, x4.  Most cases sit at
# 3e-7; the worst one holds an element of d re whose bf16 rounding falls the other way, because the kernel's fp32 STFT
# and the float64 one differ in the last bits.  Against the plain float64 gradient: measured 3.6e-3, x2 -- what bf16 costs.
LOGMEL_BWD_ROUNDED = 5.5e-5
LOGMEL_BWD_PLAIN = 7.2e-3
# image backward (fp32 in and out), per element relative to max |ref|.  Against float64 autograd of F.interpolate:
# measured worst 1.38e-5, x4 -- the float32 tap positions (scale * i rounded at 2^-24 of up to 150 frames), the same
# as torch's own float32 bicubic.  Against the same operator built from the host's float32 taps in float64 arithmetic,
# where only the kernel's own sums remain: measured worst 4.4e-7, x4.
IMAGE_BWD = 5.5e-5
IMAGE_BWD_TAPS = 1.8e-6
# _Frontend end to end against the float32 oracle under autograd: rel-L2 of d wav (measured worst 2.19e-3, x2) and the
# per-element error over the halo samples relative to max |ref| there (measured 4.5e-3 at L = 9000, x4)
FRONTEND_GRAD_REL_L2 = 4.4e-3
FRONTEND_GRAD_HALO = 1.8e-2
# window attention against float64 on the bf16-rounded operands.  Forward: one bf16 output rounding of the element plus
# `ATTN_FWD_ABS` of max |ref| (the bf16 probabilities of the P V product; measured worst 1.2e-3, x4).  LSE absolute in
# log2 units (measured 7.0e-7, x4).  Gradients per element relative to that operand's max |ref| (measured dq 4.8e-3,
# dk 3.7e-3, dv 4.6e-3, x4).
ATTN_FWD_ABS = 4.8e-3
ATTN_LSE_ABS = 2.8e-6
ATTN_BWD = dict(dq=1.9e-2, dk=1.5e-2, dv=1.8e-2)

IMAGE_GEOMETRIES = [(64, 64, 4, 2), (64, 64, 4, 19), (64, 64, 4, 63), (64, 64, 4, 64), (128, 64, 4, 150)]   # (S, F, ps, frames)
ATTN_CASES = [(2, 32, 4, 6, 1), (4, 16, 16, 8, 4), (2, 32, 16, 5, 1), (8, 32, 64, 4, 4), (32, 32, 64, 2, 1),
              (4, 32, 64, 16, 16)]                                                        # (heads, hd, n, nw, nbb)
KAISER = dict(lowpass_filter_width=64, rolloff=0.9475937167399596, beta=14.769656459379492)
RESAMPLE_CASES = [(16000, 48000, 5000), (16000, 48000, 333), (48000, 16000, 4001), (2, 3, 1000), (48000, 16000, 17),
                  (16000, 48000, 7)]


def bf16_round64(x):
    """float64 -> the nearest bf16 value (through float32, as the kernels hold the value), back in float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def det64(name, shape, seed):
    from consistencytta_amd import spec
    return torch.from_numpy(spec.det_uniform(name, shape, seed)).to(torch.float64)


# ------------------------------------------------------------------------------------------------ log-mel front end
def logmel_inputs(L, B=2):
    """Uniform +-0.4 noise (float32 values); row 1 is exact zeros from L / 3 on once the clip holds silent frames."""
    wav = (det64("clapops.wav.%d" % L, (B, L), 11) * 0.4).to(torch.float32)
    if L >= 2400:
        wav[1, L // 3:] = 0.0
    return wav


def basis64(cfg):
    """The oracle's float32 DFT basis and mel matrix, cast to float64: (re [cutoff][N], im [cutoff][N], W [cutoff][mels])."""
    re, im = oclap.dft_basis(cfg["n_fft"], cfg["n_fft"])
    melw = omel.mel_filterbank(cfg["sample_rate"], cfg["n_fft"], cfg["mel_bins"], cfg["fmin"], cfg["fmax"]).T.astype(np.float32)
    return re.double(), im.double(), torch.from_numpy(melw).double()


def frames64(wav, cfg):
    """(B, L) -> (B, frames, n_fft): reflect padding by n_fft / 2, centred frames every hop."""
    half = cfg["n_fft"] // 2
    x = F.pad(wav.double()[:, None, :], (half, half), mode="reflect")[:, 0]
    return x.unfold(1, cfg["n_fft"], cfg["hop"])


def stft64(wav, cfg):
    re_w, im_w, _ = basis64(cfg)
    fr = frames64(wav, cfg)
    return fr @ re_w.t(), fr @ im_w.t()


def mel_power64(wav, cfg):
    re, im = stft64(wav, cfg)
    return (re ** 2 + im ** 2) @ basis64(cfg)[2]


def logmel_db_ref(wav, cfg=FRONT_CFG, amin=AMIN):
    """`oracle.clap.spectrogram_power` + `logmel` in float64 (differentiable): (B, L) -> (B, frames, mels) in dB."""
    return 10.0 * torch.log10(torch.clamp(mel_power64(wav, cfg), min=amin))


def logmel_db_bwd_ref(wav, dlogmel, cfg=FRONT_CFG, amin=AMIN):
    w = wav.double().clone().requires_grad_(True)
    (logmel_db_ref(w, cfg, amin) * dlogmel.double()).sum().backward()
    return w.grad


def kernel_basis_f32(cfg):
    """The basis as `ctta_mel_frontend_create` forms it: float32(cos | -sin of the exact angle) * float32(periodic Hann),
    the product in float32.  Rows [re ; im], (2 * cutoff, n_fft) float32."""
    N = cfg["n_fft"]
    k = np.arange(N // 2 + 1)[:, None]
    n = np.arange(N)[None, :]
    ang = 2.0 * np.pi * ((k * n) % N).astype(np.float64) / N
    win = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)).astype(np.float32)
    return torch.from_numpy(np.concatenate([np.cos(ang).astype(np.float32) * win, (-np.sin(ang)).astype(np.float32) * win]))


def split3(x32):
    """The kernels' three-way bf16 split of a float32 tensor (x = p0 + p1 + p2 to 24 bits), each part in float64."""
    p0 = x32.to(torch.bfloat16).to(torch.float32)
    r1 = x32 - p0
    p1 = r1.to(torch.bfloat16).to(torch.float32)
    p2 = (r1 - p1).to(torch.bfloat16).to(torch.float32)
    return p0.double(), p1.double(), p2.double()


SPLIT_PASSES = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))     # (waveform part, basis part), as the kernel orders them


def logmel_db_split_emulated(wav, cfg=FRONT_CFG, amin=AMIN, drop=None):
    """The forward with the STFT as the six split products x_i * b_j (i + j <= 2) accumulated in float64; `drop` leaves
    one pass out.  Returns (dB log-mel, Frobenius norm of each pass's contribution)."""
    cutoff = cfg["n_fft"] // 2 + 1
    half = cfg["n_fft"] // 2
    xp = F.pad(wav[:, None, :], (half, half), mode="reflect")[:, 0]
    xs = [p.unfold(1, cfg["n_fft"], cfg["hop"]) for p in split3(xp)]
    bs = split3(kernel_basis_f32(cfg))
    ft, norms = 0.0, []
    for p, (i, j) in enumerate(SPLIT_PASSES):
        term = xs[i] @ bs[j].t()
        norms.append(float(term.norm()))
        if p != drop:
            ft = ft + term
    power = ft[..., :cutoff] ** 2 + ft[..., cutoff:] ** 2
    return 10.0 * torch.log10(torch.clamp(power @ basis64(cfg)[2], min=amin)), norms


def logmel_db_bwd_rounded_ref(wav, dlogmel, cfg=FRONT_CFG, amin=AMIN):
    """The log-mel backward with the two roundings `mel_power_db_bwd_kernel` / `ctta_wav_to_logmel_db_bwd` document,
    everything else in float64: d re / d im are rounded to bf16, and they multiply only the LEADING bf16 part of the
    basis (`kernel_basis_f32` rounded to nearest even).  Overlap-add and the reflect padding's adjoint come from
    autograd of the framing."""
    re_w, im_w, melw = basis64(cfg)
    N = cfg["n_fft"]
    cutoff = N // 2 + 1
    w = wav.double().clone().requires_grad_(True)
    fr = frames64(w, cfg)
    with torch.no_grad():
        re, im = fr @ re_w.t(), fr @ im_w.t()
        mel = (re ** 2 + im ** 2) @ melw
        gm = torch.where(mel > amin, dlogmel.double() * (10.0 / math.log(10.0)) / mel.clamp_min(1e-300), torch.zeros_like(mel))
        dp = gm @ melw.t()
        dre, dim = bf16_round64(2.0 * re * dp), bf16_round64(2.0 * im * dp)
        b0 = kernel_basis_f32(cfg).to(torch.bfloat16).to(torch.float64)
        dframes = dre @ b0[:cutoff] + dim @ b0[cutoff:]
    (fr * dframes).sum().backward()
    return w.grad


def halo_mask(L, n_fft=1024):
    """Samples [0, n_fft/2 + 1) and [L - n_fft/2, L): where the adjoint of the reflect padding adds its mirrored terms."""
    m = torch.zeros(L, dtype=torch.bool)
    m[:n_fft // 2 + 1] = True
    m[max(L - n_fft // 2, 0):] = True
    return m


def silent_frames(wav, cfg=FRONT_CFG):
    """(B, frames) bool: frames whose every mel value is exactly 0."""
    return (mel_power64(wav, cfg) == 0).all(-1)


# ------------------------------------------------------------------------------------------------ log-mel -> image
def image_inputs(S, Fq, ps, frames, B=2):
    tag = "clapops.img.%d.%d" % (S, frames)
    lm = (det64(tag + ".lm", (B, frames, Fq), 1) * 30.0 - 40.0).to(torch.float32)          # dB-like values
    scale = (0.1 + 0.05 * det64(tag + ".a", (Fq,), 2)).to(torch.float32)
    shift = (0.5 * det64(tag + ".c", (Fq,), 3)).to(torch.float32)
    return lm, scale, shift


def stretch_matrix(t_in, t_out):
    """The host's float32 tap table (`consistencytta_amd.clap.bicubic_taps`) as a dense [t_out][t_in] float64 matrix."""
    from consistencytta_amd.clap import bicubic_taps
    idx, w = bicubic_taps(t_in, t_out)
    m = torch.zeros(t_out, t_in, dtype=torch.float64)
    m.index_put_((torch.arange(t_out)[:, None].expand(-1, 4), torch.from_numpy(idx).long()), torch.from_numpy(w).double(),
                 accumulate=True)
    return m


def image_ref(lm, scale, shift, S, host_taps=False):
    """bn0 affine per mel bin, bicubic stretch of the frame axis (align_corners=True) to S * (S / F) frames, and the
    fold of `oracle.clap.wav_to_image`: (B, T, F) -> (B, S, S) float64 (differentiable).  `host_taps` stretches with the
    host's float32 tap table instead of F.interpolate."""
    B, T, Fq = lm.shape
    ratio = S // Fq
    tt = S * ratio
    x = (lm.double() * scale.double() + shift.double())[:, None]
    if T < tt and host_taps:
        x = torch.einsum("ot,bctf->bcof", stretch_matrix(T, tt), x)
    elif T < tt:
        x = F.interpolate(x, (tt, Fq), mode="bicubic", align_corners=True)
    x = x.permute(0, 1, 3, 2).reshape(B, 1, Fq, ratio, tt // ratio).permute(0, 1, 3, 2, 4)
    return x.reshape(B, Fq * ratio, tt // ratio)


def tokens_to_image(dtok, S, ps):
    """[B][(S/ps)^2][>= ps*ps] token layout -> (B, S, S): pixel (row, col) at patch (row/ps, col/ps), entry (row%ps)*ps + col%ps."""
    B, G = dtok.shape[0], S // ps
    return dtok[:, :, :ps * ps].reshape(B, G, G, ps, ps).permute(0, 1, 3, 2, 4).reshape(B, S, S)


def image_bwd_ref(lm, scale, shift, S, ps, dtok, host_taps=False):
    x = lm.double().clone().requires_grad_(True)
    (image_ref(x, scale, shift, S, host_taps) * tokens_to_image(dtok.double(), S, ps)).sum().backward()
    return x.grad


# ------------------------------------------------------------------------------------------------ window attention
def attention_inputs(heads, hd, n, nw, nbb):
    """bf16-valued q, k, v, dout (nw, heads, n, hd) and bias (nbb, heads, n, n), all float64.  With 16 bias batches the
    odd ones carry a shifted-window style -100 mask, and batch 3 masks keys n*3/4.. for EVERY query."""
    tag = "clapops.wa.%d.%d.%d.%d.%d" % (heads, hd, n, nw, nbb)
    q, k, v, go = (bf16_round64(det64(tag + "." + nm, (nw, heads, n, hd), s) * 1.5) for s, nm in enumerate(("q", "k", "v", "go")))
    bias = det64(tag + ".bias", (nbb, heads, n, n), 7) * 2.0
    dead = None
    if nbb == 16:
        region = (torch.arange(n) >= n * 5 // 8).to(torch.float64)
        block = torch.where(region[:, None] != region[None, :], torch.tensor(-100.0, dtype=torch.float64),
                            torch.tensor(0.0, dtype=torch.float64))
        bias[1::2] += block
        dead = (3, n * 3 // 4)
        bias[3] -= block                                       # batch 3: only the all-query mask below
        bias[3, :, :, dead[1]:] = -100.0
    return q, k, v, go, bias.to(torch.float32).double(), dead


def window_attention_ref(q, k, v, bias, scale):
    """softmax(q k^T scale + bias[b % nbb]) v in float64; also the log2-domain log-sum-exp per row, the kernel's
    `lse = max + log2(sum exp2(s * scale * log2e + bias * log2e - max))`."""
    nw, nbb = q.shape[0], bias.shape[0]
    s = (q @ k.transpose(-1, -2)) * scale + bias[torch.arange(nw) % nbb]
    return s.softmax(-1) @ v, torch.logsumexp(s, -1) / math.log(2.0)


def window_attention_bwd_ref(q, k, v, bias, scale, go):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    out, _ = window_attention_ref(q, k, v, bias, scale)
    (out * go).sum().backward()
    return q.grad, k.grad, v.grad


# ------------------------------------------------------------------------------------------------ glue
def resample64(x, orig_freq, new_freq, **kw):
    """`oracle.clap.resample` with its float32 filter table cast to float64 and the sums in float64 (differentiable)."""
    kernels, width, orig, new = oclap.sinc_resample_kernel(orig_freq, new_freq, **kw)
    length = x.shape[-1]
    xp = F.pad(x.double().reshape(-1, length), (width, width + orig))
    y = F.conv1d(xp[:, None], kernels.double(), stride=orig).transpose(1, 2).reshape(xp.shape[0], -1)
    return y[:, :int(math.ceil(new * length / orig))]


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
