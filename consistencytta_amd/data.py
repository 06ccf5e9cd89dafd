"""Mix augmentation of the training batch, mirroring the reference's names and signatures: `tools/mix.py:4-51`
(a_weight, compute_gain, mix), `tools/torch_tools.py:85-123` (uncapitalize, mix_wavs_and_captions, augment) and the
train split's collate (`tools/t2a_dataset.py:51-69`, built with augment=True by train.py:173-176).

The pair draw and the captions stay on the host and use Python's global `random` exactly as the reference does, so the
same seed selects the same pairs.  Everything numerical runs on the GPU (csrc/mix_augment.hip): per-frame A-weighted
(or RMSE) gains, the loudness-balanced pair mix and the per-batch normalisation.  There is no CPU path: numpy or CPU
tensor inputs are copied to the current CUDA device and the results copied back.

The HIP stage cannot run in DataLoader worker processes, so the loader keeps augment=False and the training loop calls
`collate(captions, waveforms)` on the raw batch before `wav_to_fbank`.

The file loader in front of it, `tools/torch_tools.py:54-75` (`read_wav_file`): `read_wav_batch` / `read_wav_file` read the
files on the host and resample (resampy's kaiser_best, `audio.resample`) and normalise (`wave_prepare`) the ragged batch on
the GPU (csrc/resample_sinc.hip), for the same reason in the same place: the loader hands out paths, the loop reads them."""
import itertools
import random

import numpy as np
import torch

from . import _native as N
from . import audio

_MODES = {"A_weighting": 0, "RMSE": 1}


def _n_fft(fs):
    if fs == 16000:
        return 2048
    if fs == 44100:
        return 4096
    raise ValueError("Invalid fs {}".format(fs))


def a_weight(fs, n_fft, min_db=-80.0):
    """tools/mix.py:4-15: the A-weighting curve (dB) on the rfft bins, f^2 := 1 at DC, clamped below at min_db.
    float64 host table (the device tables are built from the same formula in csrc/mix_augment.hip)."""
    freq_sq = np.linspace(0, fs // 2, n_fft // 2 + 1) ** 2
    freq_sq[0] = 1.0
    weight = 2.0 + 20.0 * (2 * np.log10(12194) + 2 * np.log10(freq_sq) - np.log10(freq_sq + 12194 ** 2)
                           - np.log10(freq_sq + 20.6 ** 2) - 0.5 * np.log10(freq_sq + 107.7 ** 2)
                           - 0.5 * np.log10(freq_sq + 737.9 ** 2))
    return np.maximum(weight, min_db)


def uncapitalize(s):
    """tools/torch_tools.py:85-89"""
    return s[:1].lower() + s[1:] if s else ""


class Mixer:
    """Owner of one ctta_mixer handle for (device, fs, mode, min_db); the handle grows when a call needs more clips,
    samples or pairs than it was made for (like audio.TacotronSTFT._ensure).  Growing frees and re-allocates device
    memory, so warm a shape up eagerly before capturing it in a graph."""

    def __init__(self, device, fs=16000, mode="A_weighting", min_db=-80.0):
        if mode not in _MODES:
            raise ValueError("Invalid mode {}".format(mode))
        self.n_fft = _n_fft(fs)
        self.device = torch.device(device)
        self.fs, self.mode, self.min_db = int(fs), mode, float(min_db)
        self._h = None
        self._key = (0, 0, 0)

    def _release(self):
        if getattr(self, "_h", None):
            N.lib().ctta_mixer_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def handle(self, clips, samples, pairs=1):
        c, s, p = self._key
        if self._h is None or clips > c or samples > s or pairs > p:
            self._release()
            c, s, p = max(clips, c), max(samples, s), max(pairs, p)
            h = N.c_void_p()
            with torch.cuda.device(self.device):
                N.check(N.lib().ctta_mixer_create(self.fs, _MODES[self.mode], self.min_db, c, s, p, h))
            self._h, self._key = h, (c, s, p)
        return self._h

    def frames(self, samples):
        return max(0, (samples - self.n_fft) // (self.n_fft // 2) + 1)

    def gain_db(self, wav):
        """wav (B, L) fp32 on self.device -> per-frame gains (B, frames) fp32, dB."""
        B, L = wav.shape
        self._check_len(L)
        self._check_src(wav)
        out = torch.empty(B, self.frames(L), dtype=torch.float32, device=self.device)
        h = self.handle(B, L)
        with torch.cuda.device(self.device):
            N.check(N.lib().ctta_mixer_gain_db(h, N.ptr(wav), B, L, L, N.ptr(out), N.stream_ptr()))
        return out

    def mix(self, wav, pairs, dst, dst_row0=0, groups=1, r=0.5, t_out=None, g_out=None):
        """Mixes wav's rows pairs[p] = (i, j) into dst[dst_row0 + p]; groups = 0 leaves them unnormalised."""
        B, L = wav.shape
        self._check_len(L)
        self._check_src(wav)
        if pairs.dtype != torch.int32 or pairs.device != self.device or pairs.ndim != 2 or pairs.shape[1] != 2 \
                or not pairs.is_contiguous():
            raise ValueError("pairs must be a contiguous (n, 2) int32 tensor on %s" % self.device)
        n = pairs.shape[0]
        for o, need in ((t_out, n), (g_out, 2 * n)):
            if o is not None and (o.dtype != torch.float32 or o.device != self.device or not o.is_contiguous()
                                  or o.numel() < need):
                raise ValueError("t_out / g_out must be contiguous fp32 tensors of >= %d / %d elements on %s"
                                 % (n, 2 * n, self.device))
        if dst.dtype != torch.float32 or dst.device != self.device or not dst.is_contiguous() or dst.shape[1] != L \
                or dst.shape[0] < dst_row0 + n:
            raise ValueError("dst must be a contiguous fp32 (>= %d, %d) tensor on %s" % (dst_row0 + n, L, self.device))
        if dst.data_ptr() == wav.data_ptr() and dst_row0 < B:
            raise ValueError("mixture rows overlap the source rows")
        if groups and n % groups:
            raise ValueError("%d pairs do not split into %d equal groups" % (n, groups))
        h = self.handle(B, L, n)
        with torch.cuda.device(self.device):
            N.check(N.lib().ctta_mixer_mix(h, N.ptr(wav), B, L, L, N.ptr(pairs), n, int(groups), float(r),
                                           N.ptr(dst), L, int(dst_row0), N.ptr(t_out), N.ptr(g_out),
                                           N.stream_ptr()))
        return dst

    def _check_len(self, L):
        _check_len(L, self.n_fft)

    def _check_src(self, wav):   # rows are passed with leading dimension L
        if wav.dtype != torch.float32 or wav.device != self.device or not wav.is_contiguous():
            raise ValueError("waveforms must be a contiguous fp32 (B, L) tensor on %s" % self.device)


def _check_len(L, n_fft):
    if L < n_fft:   # the reference's np.max of an empty gain list raises ValueError too
        raise ValueError("a clip of %d samples is shorter than n_fft = %d: it has no frame" % (L, n_fft))


_MIXERS = {}


def mixer(device=None, fs=16000, mode="A_weighting", min_db=-80.0):
    """The per-(device, fs, mode, min_db) Mixer of this process."""
    device = torch.device(device if device is not None else "cuda")
    if device.type != "cuda":
        raise N.CttaError("the mix augmentation runs on the GPU only (got device %s)" % device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device, int(fs), mode, float(min_db))
    if key not in _MIXERS:
        _MIXERS[key] = Mixer(device, fs, mode, min_db)
    return _MIXERS[key]


def _to_device(x, dim):
    """numpy / torch -> (fp32 contiguous CUDA tensor, device, back-converter to the input's type)."""
    if isinstance(x, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        back = lambda y: y.cpu().numpy().astype(np.float64)   # noqa: E731  (the reference's numpy results are float64)
    elif torch.is_tensor(x):
        t = x.detach()
        back = (lambda y: y) if t.is_cuda else (lambda y: y.cpu())
    else:
        raise TypeError("expected a numpy array or a torch tensor, got %s" % type(x).__name__)
    if t.ndim != dim:
        raise ValueError("expected %d-D input, got shape %s" % (dim, tuple(t.shape)))
    dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return t.to(device=dev, dtype=torch.float32).contiguous(), dev, back


def compute_gain(sound, fs, min_db=-80.0, mode="A_weighting"):
    """tools/mix.py:18-43: per-frame gain (dB) of `sound` (1-D, or (B, L) for a batch), frames of n_fft at stride
    n_fft / 2 without padding.  Returns the input's type (numpy float64 or a torch fp32 tensor)."""
    _check_len(sound.shape[-1], _n_fft(fs))
    if mode not in _MODES:
        raise ValueError("Invalid mode {}".format(mode))
    one = (sound.ndim == 1)
    x, dev, back = _to_device(sound[None] if one else sound, 2)
    g = mixer(dev, fs, mode, min_db).gain_db(x)
    return back(g[0] if one else g)


def mix(sound1, sound2, r, fs):
    """tools/mix.py:46-51: the loudness-balanced mixture of two equal-length 1-D clips (A-weighted gains)."""
    if tuple(sound1.shape) != tuple(sound2.shape) or sound1.ndim != 1:
        raise ValueError("mix needs two 1-D clips of equal length, got %s and %s" % (tuple(sound1.shape), tuple(sound2.shape)))
    _check_len(sound1.shape[0], _n_fft(fs))
    if torch.is_tensor(sound1):
        both = torch.stack([sound1.detach().float(), sound2.detach().to(sound1.device).float()])
    else:
        both = np.stack([np.asarray(sound1, np.float32), np.asarray(sound2, np.float32)])
    x, dev, back = _to_device(both, 2)
    out = torch.empty(1, x.shape[1], dtype=torch.float32, device=dev)
    pairs = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
    mixer(dev, fs).mix(x, pairs, out, groups=0, r=r)
    return back(out[0])


def mix_wavs_and_captions(wave1, wave2, caption1, caption2):
    """tools/torch_tools.py:92-95"""
    mixed_sound = mix(wave1, wave2, 0.5, 16000).reshape(1, -1)
    return mixed_sound, f"{caption1} and {uncapitalize(caption2)}"


def draw_pairs(n, num_items=None):
    """torch_tools.py:103-113: all pairs i < j in itertools.combinations order, shuffled with the global `random`,
    the first num_items kept (all of them if there are fewer)."""
    if num_items is None:
        num_items = n // 2
    combinations = list(itertools.combinations(list(range(n)), 2))
    random.shuffle(combinations)
    return combinations if len(combinations) < num_items else combinations[:num_items]


def pair_captions(texts, pairs):
    """torch_tools.py:117: "x and y" for each host pair (i, j)."""
    return [f"{texts[i]} and {uncapitalize(texts[j])}" for i, j in pairs]


def _pair_tensor(pairs, dev):
    if torch.is_tensor(pairs):
        if pairs.dtype != torch.int32 or pairs.device != dev or pairs.ndim != 2 or pairs.shape[1] != 2:
            raise ValueError("a device pair tensor must be (n, 2) int32 on %s" % dev)
        return pairs.contiguous()
    return torch.tensor([list(p) for p in pairs], dtype=torch.int32).reshape(-1, 2).to(dev)


def _check_host_pairs(pairs, lo, hi):
    for i, j in pairs:
        if not (lo <= i < hi and lo <= j < hi):
            raise ValueError("pair (%d, %d) outside clips [%d, %d)" % (i, j, lo, hi))


def augment(waveforms, texts, num_items=None, pairs=None):
    """torch_tools.py:98-123: mixes num_items (default len(texts) // 2) random pairs of the batch, normalised together
    by one max |.| and halved.  Returns (fp32 CUDA mixtures (n, L), captions).

    pairs: host list of (i, j), or an (n, 2) int32 CUDA tensor, replaces the draw (no `random` call).  With a device
    tensor no value is read on the host (the graph-capture path) and the captions are None: build them from the host
    pairs with `pair_captions`."""
    x, dev, _ = _to_device(waveforms, 2)
    if pairs is None:
        pairs = draw_pairs(len(texts), num_items)
    if not torch.is_tensor(pairs):
        _check_host_pairs(pairs, 0, x.shape[0])
    captions = None if torch.is_tensor(pairs) else pair_captions(texts, pairs)
    p = _pair_tensor(pairs, dev)
    out = torch.empty(p.shape[0], x.shape[1], dtype=torch.float32, device=dev)
    if p.shape[0]:
        mixer(dev).mix(x, p, out, groups=1)
    return out, captions


def collate(captions, waveforms, augment=True, out=None, groups=1, pairs=None):
    """The train split's collate (t2a_dataset.py:51-69) on a raw batch: (captions, waveforms (B, L)) ->
    (captions + mixed captions, (B + n, L) fp32 CUDA batch) with the B source rows copied unchanged and the n mixtures
    written straight into the tail rows.

    groups > 1 treats the batch as `groups` consecutive loader batches of B / groups clips (the fused micro-batch):
    each draws its own B / groups // 2 pairs, in group order, and is normalised on its own, exactly as that many
    collates would; their mixtures follow all source rows, group by group.
    out: optional preallocated (B + n, L) fp32 CUDA tensor (its first B rows may already hold the waveforms).
    pairs: host list or (n, 2) int32 CUDA tensor of batch-global clip indices replacing the draw (captions are then
    None for a device tensor, see augment)."""
    if waveforms.ndim != 2 or len(captions) != waveforms.shape[0]:
        raise ValueError("%d captions for waveforms of shape %s" % (len(captions), tuple(waveforms.shape)))
    if augment:
        _check_len(waveforms.shape[1], 2048)
        if groups < 1 or waveforms.shape[0] % groups:
            raise ValueError("a batch of %d does not split into %d equal loader batches" % (waveforms.shape[0], groups))
    x, dev, _ = _to_device(waveforms, 2)
    B, L = x.shape
    captions = list(captions)
    if not augment:
        if out is None:
            return captions, x.clone() if x is waveforms else x
        out[:B].copy_(x)
        return captions, out
    bg = B // groups
    if pairs is None:
        pairs = [(i + g * bg, j + g * bg) for g in range(groups) for i, j in draw_pairs(bg, bg // 2)]
    n = pairs.shape[0] if torch.is_tensor(pairs) else len(pairs)
    if n % groups:
        raise ValueError("%d pairs do not split into %d groups" % (n, groups))
    if not torch.is_tensor(pairs):
        per = n // groups
        for g in range(groups):
            _check_host_pairs(pairs[g * per:(g + 1) * per], g * bg, (g + 1) * bg)
    mixed_captions = None if torch.is_tensor(pairs) else pair_captions(captions, pairs)
    if out is None:
        out = torch.empty(B + n, L, dtype=torch.float32, device=dev)
    elif out.shape[0] != B + n or out.shape[1] != L or out.dtype != torch.float32 or out.device != dev:
        raise ValueError("out must be an fp32 (%d, %d) tensor on %s" % (B + n, L, dev))
    if out.data_ptr() != x.data_ptr():
        out[:B].copy_(x)
    if n:
        mixer(dev).mix(out[:B], _pair_tensor(pairs, dev), out, dst_row0=B, groups=groups)
    return (captions + mixed_captions if mixed_captions is not None else None), out


# ------------------------------------------------------------------------------------------------------- the file loader
def read_mono(filename):
    """`sf.read` + `librosa.to_mono` of torch_tools.py:56-58 through scipy.io.wavfile (there is no soundfile here), with the
    rules of `audioldm_eval.read_centered_wav`: integer PCM scaled to [-1, 1), unsigned 8-bit re-centred, the mean over the
    channels.  Returns (float64 samples, rate)."""
    from scipy.io import wavfile
    sr, wav = wavfile.read(filename)
    if wav.dtype.kind == "i":
        wav = wav.astype(np.float64) / float(2 ** (8 * wav.dtype.itemsize - 1))
    elif wav.dtype.kind == "u":
        wav = (wav.astype(np.float64) - 128.0) / 128.0
    else:
        wav = wav.astype(np.float64)
    if wav.ndim > 1:
        wav = wav.mean(axis=1)
    return wav, int(sr)


def wave_prepare(flat, offsets, lengths, segment_length, clips=None):
    """torch_tools.py:69-73 for clips lying in one fp32 CUDA buffer (`flat[offsets[b]:offsets[b] + lengths[b]]`): mean
    removal, peak 0.5, cut / zero-pad to `segment_length`, peak 0.5 again -> (B, segment_length) fp32.  One launch
    (ctta_wave_prepare).  `clips`: a device table of ctta_resample_clip already holding these offsets (y_off) and lengths
    (n_out), tensor or raw pointer; built and uploaded here when None."""
    if not flat.is_cuda:
        raise N.CttaError("waveforms on %s: the HIP loader has no CPU path (call .cuda())" % flat.device)
    if flat.dtype != torch.float32 or not flat.is_contiguous():
        raise ValueError("the sample buffer must be a contiguous fp32 tensor")
    B, seg = len(lengths), int(segment_length)
    if min(lengths) < 1:
        raise ValueError("an empty clip has no mean")
    if clips is None:
        clips = audio.clip_table([N.ResampleClip(y_off=int(o), n_out=int(n)) for o, n in zip(offsets, lengths)], flat.device)
    out = torch.empty(B, seg, dtype=torch.float32, device=flat.device)
    ws = torch.empty(3 * B, dtype=torch.float64, device=flat.device)
    cp = N.ptr(clips) if torch.is_tensor(clips) else N.c_void_p(clips)
    with torch.cuda.device(flat.device):
        N.check(N.lib().ctta_wave_prepare(N.ptr(flat), cp, B, seg, N.ptr(out), N.ptr(ws), N.stream_ptr()))
    return out


def read_wav_batch(filenames, segment_length, target_sr=16000, device=None, filter="kaiser_best"):
    """`read_wav_file` (tools/torch_tools.py:54-75) for a list of files of any lengths and rates -> (B, segment_length) fp32 on
    the GPU: what `collate` and `audio.wav_to_fbank` take.  `target_sr` may be a list of rates, resampled to in turn as the
    reference does (t2a_dataset.py:111-122 passes [16000, 48000]).

    The files are read and mixed down on the host; everything numerical runs on the GPU.  All samples and every stage's
    clip descriptors go up in ONE copy into an arena that also holds the stages' outputs; then one ctta_resample_sinc
    per rate stage (clips already at the stage's rate stay where they are) and one ctta_wave_prepare.  The resampler
    follows the published definition of resampy 0.4.2 (see `audio.resample`); the package itself is not installed where
    this was built, so parity with it is by definition, not by comparison."""
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise N.CttaError("the file loader's arithmetic runs on the GPU only (got device %s)" % dev)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    stages = [int(r) for r in target_sr] if isinstance(target_sr, (list, tuple)) else [int(target_sr)]
    _, num_table = audio.resampy_filter(filter)
    waves, rates = zip(*(read_mono(f) for f in filenames))
    B = len(waves)
    # arena, in fp32 elements: [the clip tables of every stage and of the normalisation | samples | stage outputs]
    size = N.ctypes.sizeof(N.ResampleClip)
    offs, lens, cur = [0] * B, [len(w) for w in waves], list(rates)
    end = 0
    for b in range(B):
        offs[b], end = end, end + lens[b]
    n_samples = end
    tables = []                                               # (first descriptor, count, max_n_out) per launched stage
    descs = []
    for sr in stages:
        first = len(descs)
        for b in range(B):
            if cur[b] != sr:
                d = audio.resample_clip(lens[b], cur[b], sr, num_table, offs[b], end)
                descs.append(d)
                offs[b], lens[b], cur[b], end = end, d.n_out, sr, end + d.n_out
        if len(descs) > first:
            tables.append((first, len(descs) - first, max(d.n_out for d in descs[first:])))
    final = len(descs)
    descs += [N.ResampleClip(y_off=offs[b], n_out=lens[b]) for b in range(B)]
    head = -(-len(descs) * size // 16) * 16                   # the samples start 16-byte aligned
    shift = head // 4
    for d in descs:
        d.x_off += shift
        d.y_off += shift
    host = np.empty(head + 4 * n_samples, dtype=np.uint8)
    host[:len(descs) * size] = np.frombuffer(bytes().join(bytes(d) for d in descs), dtype=np.uint8)
    host[head:].view(np.float32)[:] = np.concatenate(waves)
    arena = torch.empty(head + 4 * end, dtype=torch.uint8, device=dev)
    arena[:host.shape[0]].copy_(torch.from_numpy(host))
    samples = arena.view(torch.float32)
    for first, count, max_n_out in tables:
        audio.resample_launch(samples, samples, arena.data_ptr() + first * size, count, max_n_out, filter)
    return wave_prepare(samples, None, lens, segment_length, clips=arena.data_ptr() + final * size)


def read_wav_file(filename, segment_length, target_sr=16000, device=None):
    """tools/torch_tools.py:54-75 -> (1, segment_length) fp32 on the GPU (`read_wav_batch` of one file)."""
    return read_wav_batch([filename], segment_length, target_sr, device)
