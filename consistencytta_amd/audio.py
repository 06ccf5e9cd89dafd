"""Waveform -> log-mel front-end mirrors: `audioldm.audio.stft.TacotronSTFT` (stft.py:132-186) and
`tools.torch_tools.wav_to_fbank` (torch_tools.py:126-135), backed by the HIP front-end (csrc/mel_frontend.hip):
reflect pad, STFT as a split-bf16 MFMA GEMM against the windowed DFT basis, magnitude, Slaney mel filterbank,
log(clamp(x, 1e-5)), frame padding.  Same call signatures as the reference; the arithmetic runs on the GPU only.

Also the loaders' band-limited resampler, `resampy.resample(..., filter="kaiser_best")` of `tools/torch_tools.py:66`, on
csrc/resample_sinc.hip: `resampy_filter`, `resample` (below)."""
import numpy as np
import torch
from torch import nn

from . import _native as N


class TacotronSTFT(nn.Module):
    def __init__(self, filter_length=1024, hop_length=160, win_length=1024, n_mel_channels=64, sampling_rate=16000,
                 mel_fmin=0.0, mel_fmax=8000.0):
        super().__init__()
        self.filter_length, self.hop_length, self.win_length = int(filter_length), int(hop_length), int(win_length)
        self.n_mel_channels, self.sampling_rate = int(n_mel_channels), int(sampling_rate)
        self.mel_fmin, self.mel_fmax = float(mel_fmin), float(mel_fmax)
        self.register_buffer("_device_anchor", torch.zeros(1), persistent=False)
        self._h = None
        self._h_key = None

    @property
    def device(self):
        return self._device_anchor.device

    def _release(self):
        if getattr(self, "_h", None):
            N.lib().ctta_mel_frontend_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _ensure(self, B, T):
        key = self._h_key
        if self._h is None or B > key[0] or T > key[1] or key[2] != self.device:
            self._release()
            Bm = max(B, key[0]) if key else B
            Tm = max(T, key[1]) if key else T
            h = N.c_void_p()
            with torch.cuda.device(self.device):
                N.check(N.lib().ctta_mel_frontend_create(self.filter_length, self.hop_length, self.win_length,
                                                         self.n_mel_channels, self.sampling_rate, self.mel_fmin,
                                                         self.mel_fmax, Bm, Tm, h))
            self._h, self._h_key = h, (Bm, Tm, self.device)
        return self._h

    def fbank(self, y, target_length=None, want_logmag=True):
        """y (B, T) -> fbank (B, frames|target_length, n_mels) [, log-magnitudes (B, ., filter_length/2)]."""
        if self.device.type != "cuda":
            raise N.CttaError("TacotronSTFT is on %s: the HIP front-end has no CPU path (call .cuda())" % self.device)
        if y.ndim != 2:
            raise ValueError("waveforms must be (batch, samples), got %s" % (tuple(y.shape),))
        y = y.detach().to(device=self.device, dtype=torch.float32).contiguous()
        B, T = y.shape
        frames = T // self.hop_length + 1
        target = int(target_length) if target_length is not None else frames
        h = self._ensure(B, T)
        fb = torch.empty(B, target, self.n_mel_channels, dtype=torch.float32, device=self.device)
        lm = torch.empty(B, target, self.filter_length // 2, dtype=torch.float32, device=self.device) if want_logmag else None
        with torch.cuda.device(self.device):
            N.check(N.lib().ctta_wav_to_fbank(h, N.ptr(y), B, T, target, N.ptr(fb), N.ptr(lm), N.stream_ptr()))
        return fb, lm

    def mel_spectrogram(self, y, normalize_fun=torch.log):
        """(B, T) in [-1, 1] -> mel_output (B, n_mel_channels, frames), log-magnitudes (B, filter_length/2, frames).
        The reference also returns the per-frame energy and the 513th (Nyquist) log-magnitude row; neither is used on
        the ConsistencyTTA path (`_pad_spec` drops the odd bin) and they are not produced here (energy is None)."""
        if normalize_fun is not torch.log:
            raise NotImplementedError("only the natural-log compression the reference uses is built")
        assert torch.min(y.data) >= -1, torch.min(y.data)
        assert torch.max(y.data) <= 1, torch.max(y.data)
        fb, lm = self.fbank(y)
        return fb.transpose(1, 2), lm.transpose(1, 2), None


def wav_to_fbank(waveforms, target_length=1024, fn_STFT=None):
    """tools/torch_tools.py:126-135: clip / nan_to_num, mel spectrogram, transpose to (B, frames, n_mels), pad or cut to
    `target_length` frames.  Returns (fbank, log_magnitudes_stft)."""
    assert fn_STFT is not None
    return fn_STFT.fbank(waveforms, target_length)


# --------------------------------------------------------------------------------------------------- resampy on the HIP path
# `resampy.resample(wav, cur_sr, tar_sr, filter="kaiser_best")` of tools/torch_tools.py:66 (also tools/t2a_dataset.py:111-122,
# audioldm_eval/datasets/load_mel.py:25-28, metrics/fad.py:33-34).  resampy is a pip package outside the reference tree and is
# not installed where this was built: everything below follows the published definition of version 0.4.2 (the one
# environment.yml pins; core.resample, filters.sinc_window, interpn.resample_f), restated in float64 numpy in
# tests/resampy_ref.py, and was never compared with the package itself.
_RESAMPY_FILTERS = {"kaiser_best": (64, 9, 14.769656459379492, 0.9475937167399596)}   # = tools/losses.py:303-304
_RESAMPY_TABLES = {}
_RESAMPY_DEVICE_TABLES = {}


def _filter_key(name):
    if isinstance(name, str):
        if name not in _RESAMPY_FILTERS:
            raise ValueError("filter %r is not built (only 'kaiser_best', or a (num_zeros, precision, beta, rolloff) tuple)" % name)
        return _RESAMPY_FILTERS[name]
    num_zeros, precision, beta, rolloff = name
    return int(num_zeros), int(precision), float(beta), float(rolloff)


def resampy_filter(name="kaiser_best"):
    """filters.sinc_window of resampy 0.4.2 with a Kaiser window: the right half of the windowed sinc as (win float64 of
    num_zeros * 2**precision + 1 entries, num_table = 2**precision).  `name`: "kaiser_best" or a tuple (num_zeros,
    precision, beta, rolloff)."""
    key = _filter_key(name)
    if key not in _RESAMPY_TABLES:
        num_zeros, precision, beta, rolloff = key
        num_table = 2 ** precision
        n = num_table * num_zeros
        sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
        _RESAMPY_TABLES[key] = (np.kaiser(2 * n + 1, beta)[n:] * sinc_win, num_table)
    return _RESAMPY_TABLES[key]


def _device_table(filter, device):
    """(fp32 table on `device`, n_win, num_table) -- uploaded once per filter and device."""
    key = (_filter_key(filter), device)
    if key not in _RESAMPY_DEVICE_TABLES:
        win, num_table = resampy_filter(filter)
        _RESAMPY_DEVICE_TABLES[key] = (torch.from_numpy(win.astype("float32")).to(device), int(win.shape[0]), num_table)
    return _RESAMPY_DEVICE_TABLES[key]


def resample_length(n_in, sr_orig, sr_new):
    """resampy 0.4.2's output length, int(n_in * sr_new / sr_orig); ValueError below one sample, like resampy."""
    n_out = int(n_in * sr_new / sr_orig)
    if n_out < 1:
        raise ValueError("Input signal length=%d is too small to resample from %s->%s" % (n_in, sr_orig, sr_new))
    return n_out


def resample_clip(n_in, sr_orig, sr_new, num_table=512, x_off=0, y_off=0):
    """The ctta_resample_clip of one clip: the host scalars of core.resample, in its own float64 expressions."""
    sample_ratio = float(sr_new) / sr_orig
    scale = min(1.0, sample_ratio)
    return N.ResampleClip(x_off=int(x_off), y_off=int(y_off), n_in=int(n_in), n_out=resample_length(n_in, sr_orig, sr_new),
                          time_increment=1.0 / sample_ratio, scale=scale, gain=sample_ratio if sample_ratio < 1 else 1.0,
                          index_step=int(scale * num_table))


def clip_table(descs, device):
    """A list of ctta_resample_clip -> its device copy (uint8 tensor; one upload)."""
    raw = bytes().join(bytes(d) for d in descs)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def resample_launch(x, y, clips, n_clips, max_n_out, filter="kaiser_best"):
    """ctta_resample_sinc on fp32 device buffers `x` / `y` (they may be one arena) and a device table of `n_clips`
    ctta_resample_clip (tensor or raw pointer): one launch for the ragged batch, on the current stream."""
    win, n_win, num_table = _device_table(filter, y.device)
    cp = N.ptr(clips) if torch.is_tensor(clips) else N.c_void_p(clips)
    with torch.cuda.device(y.device):
        N.check(N.lib().ctta_resample_sinc(N.ptr(x), N.ptr(y), cp, int(n_clips), int(max_n_out), N.ptr(win), n_win, num_table,
                                           N.stream_ptr()))


def resample(x, sr_orig, sr_new, filter="kaiser_best"):
    """resampy.resample(x, sr_orig, sr_new, filter=filter) per clip on the GPU.  `x`: a (B, L) fp32 CUDA tensor or a list
    of 1-D CUDA tensors; `sr_orig`: one rate or one per clip.  Returns a (B, n_out) tensor for a tensor input with one
    output length, else a list of 1-D tensors (views of one buffer).  A clip already at `sr_new` is returned as it is
    (resampy would filter it; read_wav_file never calls it then).  The whole batch is one launch."""
    as_list = not torch.is_tensor(x)
    clips = list(x) if as_list else x
    if not as_list and x.ndim != 2:
        raise ValueError("waveforms must be (batch, samples) or a list of 1-D tensors, got %s" % (tuple(x.shape),))
    B = len(clips)
    rates = [int(r) for r in sr_orig] if isinstance(sr_orig, (list, tuple)) else [int(sr_orig)] * B
    if len(rates) != B:
        raise ValueError("%d rates for %d clips" % (len(rates), B))
    for c in clips:
        if not torch.is_tensor(c) or c.ndim != 1:
            raise ValueError("every clip must be a 1-D tensor")
        if not c.is_cuda:
            raise N.CttaError("clip on %s: the HIP resampler has no CPU path (call .cuda())" % c.device)
    todo = [b for b in range(B) if rates[b] != int(sr_new)]
    if not todo:
        return x
    _, num_table = resampy_filter(filter)
    dev = clips[0].device
    if as_list:
        flat = torch.cat([clips[b].detach().to(device=dev, dtype=torch.float32) for b in todo])
        lens = [int(clips[b].shape[0]) for b in todo]
        x_offs = [sum(lens[:i]) for i in range(len(todo))]
    else:
        flat = x.detach().to(dtype=torch.float32).contiguous()
        x_offs = [b * x.shape[1] for b in todo]
        lens = [int(x.shape[1])] * len(todo)
    descs, y_off = [], 0
    for i, b in enumerate(todo):
        descs.append(resample_clip(lens[i], rates[b], sr_new, num_table, x_offs[i], y_off))
        y_off += descs[-1].n_out
    y = torch.empty(y_off, dtype=torch.float32, device=dev)
    resample_launch(flat, y, clip_table(descs, dev), len(descs), max(d.n_out for d in descs), filter)
    outs = list(clips)
    for d, b in zip(descs, todo):
        outs[b] = y[d.y_off:d.y_off + d.n_out]
    if not as_list and len(todo) == B and len({d.n_out for d in descs}) == 1:
        return y.view(B, descs[0].n_out)
    return outs
