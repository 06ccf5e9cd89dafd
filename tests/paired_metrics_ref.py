"""The four paired metrics of the evaluation suite (`lsd`, `ssim_stft`, `psnr`, `ssim`; audioldm_eval/eval.py:137-179) restated
in numpy from their published definitions (TEST INFRASTRUCTURE ONLY).  The reference takes them from two pip packages that are
not part of its tree: `ssr_eval.metrics.AudioMetrics` (LSD and SSIM on |librosa.stft|) and `skimage.metrics`
(`peak_signal_noise_ratio`, `structural_similarity`, which calls `scipy.ndimage.uniform_filter` as this file does).

Every function takes `dtype`: float64 is the reference the HIP path is compared against, float32 is the same formula in the
number format of the kernels' inputs -- the distance between the two is what the tests derive their bounds from.

Stated choices (constructor arguments of `EvaluationHelper`, defaults as here):
  * n_fft = int(2048 / (44100 / sr)): 743 at 16 kHz, 1486 at 32 kHz; hop = int(sr / 100); periodic Hann window of n_fft samples;
  * centre padding of n_fft // 2 samples, "reflect" (librosa 0.9, which ssr_eval was released against) or "constant" (0.10);
    frames = 1 + len // hop: for an odd n_fft the last frame ends one sample past the padding, which continues by the same rule;
  * the SSIM of the spectrograms infers data_range from the float dtype: R = 2; the SSIM of the mels is given R = 1."""
import numpy as np
from scipy.ndimage import uniform_filter

from oracle import mel as omel

TIME_OFFSET = 160 * 7


def n_fft_of(sr):
    return int(2048 / (44100 / sr))


def hop_of(sr):
    return int(sr / 100)


def hann_periodic(n, dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)).astype(dtype)


def padded(a, n_fft, hop, pad_mode):
    """The centre-padded signal every frame of `stft_frames` is cut from: n_fft // 2 samples on the left, enough on the right
    for frame len // hop (n_fft // 2, one more for an odd n_fft when hop divides len)."""
    a = np.asarray(a)
    frames = 1 + len(a) // hop
    left = n_fft // 2
    right = max(n_fft // 2, (frames - 1) * hop + n_fft - left - len(a))
    return np.pad(a, (left, right), mode=pad_mode), frames


def stft_frames(a, n_fft, hop, pad_mode="reflect", dtype=np.float64):
    """(frames, n_fft): the windowed frames whose rfft is the spectrogram."""
    if pad_mode not in ("reflect", "constant"):
        raise ValueError(pad_mode)
    p, frames = padded(np.asarray(a, dtype=dtype), n_fft, hop, pad_mode)
    idx = np.arange(frames)[:, None] * hop + np.arange(n_fft)[None, :]
    return p[idx] * hann_periodic(n_fft, dtype)[None, :]


def stft_magnitude(a, n_fft, hop, pad_mode="reflect", dtype=np.float64):
    """|librosa.stft(a, n_fft, hop, center=True, pad_mode)| laid out (frames, 1 + n_fft // 2), written as the DFT sum itself
    (a matrix product with the cos / sin tables, angles reduced exactly), not through an FFT."""
    fr = stft_frames(a, n_fft, hop, pad_mode, dtype)
    k = np.arange(1 + n_fft // 2)[None, :]
    n = np.arange(n_fft)[:, None]
    ang = 2.0 * np.pi * ((k * n) % n_fft).astype(np.float64) / n_fft
    re = fr @ np.cos(ang).astype(dtype)
    im = fr @ (-np.sin(ang)).astype(dtype)
    return np.sqrt(re * re + im * im)


def lsd(est, target, dtype=np.float64):
    """AudioMetrics.lsd on (frames, bins) magnitudes: mean_t sqrt(mean_f log10(T^2 / (E + 1e-12)^2 + 1e-12)^2)."""
    e, t = np.asarray(est, dtype=dtype), np.asarray(target, dtype=dtype)
    eps = dtype(1e-12)
    ratio = np.log10(t ** 2 / ((e + eps) ** 2) + eps) ** 2
    return float(np.mean(np.sqrt(np.mean(ratio, axis=-1, dtype=dtype)), dtype=dtype))


def ssim_map(x, y, data_range, win=7, sample_covariance=True, dtype=np.float64):
    """skimage.metrics.structural_similarity's per-pixel map S, cropped to the positions whose window lies inside the image."""
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    if min(x.shape) < win or x.shape != y.shape:
        raise ValueError("win_size exceeds image extent")
    npx = win * win
    cov_norm = dtype(npx / (npx - 1.0) if sample_covariance else 1.0)
    ux, uy = uniform_filter(x, size=win), uniform_filter(y, size=win)
    uxx, uyy, uxy = uniform_filter(x * x, size=win), uniform_filter(y * y, size=win), uniform_filter(x * y, size=win)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = dtype((0.01 * data_range) ** 2), dtype((0.03 * data_range) ** 2)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    pad = (win - 1) // 2
    return s[pad:s.shape[0] - pad, pad:s.shape[1] - pad]


def ssim(x, y, data_range, win=7, sample_covariance=True, dtype=np.float64):
    return float(ssim_map(x, y, data_range, win, sample_covariance, dtype).mean(dtype=np.float64))


def mse(x, y):
    return float(np.mean((np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64)) ** 2, dtype=np.float64))


def psnr(x, y, data_range=1.0):
    """skimage.metrics.peak_signal_noise_ratio: 10 log10(R^2 / mse), inf for identical images."""
    err = mse(x, y)
    return float("inf") if err == 0.0 else float(10.0 * np.log10(data_range ** 2 / err))


def mel_config(sr):
    return {16000: (512, 160, 512, 64, 16000, 50, 8000), 32000: (1024, 320, 1024, 64, 32000, 50, 14000)}[sr]


def normalised_mel(audio, sr=16000, dtype=np.float64, perturb=None):
    """datasets/load_mel.py:100-120: clip to [-1, 1] -> TacotronSTFT mel magnitudes (reflect padding of filter_length / 2, periodic
    Hann, Slaney mel matrix) -> clip((20 log10(clamp(m, 1e-5)) - 20 + 100) / 100, 0, 1), (n_mels, frames)."""
    n_fft, hop, _, n_mels, _, fmin, fmax = mel_config(sr)
    a = np.clip(np.asarray(audio, dtype=dtype), -1, 1)
    mag = stft_magnitude(a, n_fft, hop, "reflect", dtype)                    # (frames, bins); n_fft is even: the plain centre padding
    if perturb is not None:
        mag = perturb(mag)
    m = omel.mel_filterbank(sr, n_fft, n_mels, fmin, fmax).astype(dtype) @ mag.T
    db = 20 * np.log10(np.maximum(m, dtype(1e-5))) - 20
    return np.clip((db + 100) / 100, 0, 1).astype(dtype)


def lsd_audio_pair(gen, gt, time_offset=TIME_OFFSET):
    """eval.py:146-152 on float64 audio: the offset on the generated side, (a - mean) / max|a| with the maximum taken BEFORE the
    mean is removed, both cut to the shorter."""
    a1 = np.asarray(gen, dtype=np.float64)[time_offset:]
    a2 = np.asarray(gt, dtype=np.float64)
    if len(a1) < 1:
        raise ValueError("the generated clip is not longer than the time offset")
    a1 = (a1 - a1.mean()) / np.abs(a1).max()
    a2 = (a2 - a2.mean()) / np.abs(a2).max()
    n = min(len(a1), len(a2))
    return a1[:n], a2[:n]


def paired_metrics(pairs, sr=16000, pad_mode="reflect", stft_ssim_data_range=2.0, time_offset=TIME_OFFSET, dtype=np.float64,
                   perturb=None):
    """`pairs`: (generated, ground truth) float64 audio as `read_centered_wav` returns it -> the four keys as eval.py reports
    them.  `perturb(mag)` (optional) is applied to every STFT magnitude: the tests model the kernels' split-bf16 error with it."""
    n_fft, hop = n_fft_of(sr), hop_of(sr)
    lsds, ssim_stfts, psnrs, ssims = [], [], [], []
    for gen, gt in pairs:
        a1, a2 = lsd_audio_pair(gen, gt, time_offset)
        a1, a2 = a1.astype(np.float32), a2.astype(np.float32)               # the number format the audio reaches the STFT in
        e, t = stft_magnitude(a1, n_fft, hop, pad_mode, dtype), stft_magnitude(a2, n_fft, hop, pad_mode, dtype)
        if perturb is not None:
            e, t = perturb(e), perturb(t)
        lsds.append(lsd(e, t, dtype))
        ssim_stfts.append(ssim(e, t, stft_ssim_data_range, dtype=dtype))
        m1, m2 = (normalised_mel(np.asarray(a, dtype=np.float64).astype(np.float32), sr, dtype, perturb) for a in (gen, gt))
        n = min(m1.shape[-1], m2.shape[-1])
        m1, m2 = m1[:, :n].astype(np.float32), m2[:, :n].astype(np.float32)  # the mels are float32 arrays in the reference
        p = psnr(m1, m2)
        if np.isinf(p):
            continue
        psnrs.append(p)
        ssims.append(ssim(m1, m2, 1.0, dtype=dtype))
    return {"lsd": float(np.mean(lsds)), "ssim_stft": float(np.mean(ssim_stfts)), "psnr": float(np.mean(psnrs)),
            "ssim": float(np.mean(ssims))}
