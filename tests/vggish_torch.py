"""Restatement of VGGish for the tests, written from its published definition (TensorFlow models' vggish_input.py /
mel_features.py / vggish_params.py and the harritaylor/torchvggish `VGG` module that audioldm_eval/metrics/fad.py:53 loads):
the input stage in float64 numpy like the original, the network in fp32 torch on the CPU.  `emulate_bf16=True` rounds weights
and the activations between layers to bf16 (fp32 accumulation, the last Linear left unrounded): the rounding points of the HIP
path, used to derive the tests' bounds on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F

SAMPLE_RATE = 16000
WINDOW, HOP, N_FFT = 400, 160, 512
N_MELS, MEL_MIN_HZ, MEL_MAX_HZ = 64, 125.0, 7500.0
LOG_OFFSET = 0.01
EXAMPLE_FRAMES = 96
CONVS = ((0, 1, 64), (3, 64, 128), (6, 128, 256), (8, 256, 256), (11, 256, 512), (13, 512, 512))
POOL_AFTER = (0, 3, 8, 13)
LINEARS = ((0, 12288, 4096), (2, 4096, 4096), (4, 4096, 128))


def hertz_to_mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_matrix():
    """(257, 64): triangles in the HTK mel domain over the rfft bin centres, no area normalisation, DC row zero."""
    bins_mel = hertz_to_mel(np.linspace(0.0, SAMPLE_RATE / 2.0, N_FFT // 2 + 1))
    edges = np.linspace(hertz_to_mel(MEL_MIN_HZ), hertz_to_mel(MEL_MAX_HZ), N_MELS + 2)
    m = np.empty((N_FFT // 2 + 1, N_MELS))
    for i in range(N_MELS):
        lower, centre, upper = edges[i:i + 3]
        m[:, i] = np.maximum(0.0, np.minimum((bins_mel - lower) / (centre - lower), (upper - bins_mel) / (upper - centre)))
    m[0, :] = 0.0
    return m


def n_examples(n_samples):
    return 0 if n_samples < WINDOW else (1 + (n_samples - WINDOW) // HOP) // EXAMPLE_FRAMES


def logmel_examples(wav, dtype=np.float64):
    """(L,) waveform at 16 kHz -> (n_examples, 96, 64) log-mel patches, every step in `dtype`."""
    x = np.asarray(wav, dtype=dtype)
    n_frames = 0 if x.shape[0] < WINDOW else 1 + (x.shape[0] - WINDOW) // HOP
    idx = HOP * np.arange(n_frames)[:, None] + np.arange(WINDOW)[None, :]
    window = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(WINDOW) / WINDOW)).astype(dtype)
    frames = x[idx] * window
    if dtype == np.float64:
        mag = np.abs(np.fft.rfft(frames, N_FFT))
    else:                                   # numpy's FFT computes in float64: an explicit DFT matrix product in `dtype`
        n, k = np.arange(WINDOW)[:, None], np.arange(N_FFT // 2 + 1)[None, :]
        ang = 2 * np.pi * ((n * k) % N_FFT) / N_FFT
        re, im = frames @ np.cos(ang).astype(dtype), frames @ (-np.sin(ang)).astype(dtype)
        mag = np.sqrt(re * re + im * im)
    logmel = np.log(mag @ mel_matrix().astype(dtype) + dtype(LOG_OFFSET))
    n_ex = n_frames // EXAMPLE_FRAMES
    return logmel[:n_ex * EXAMPLE_FRAMES].reshape(n_ex, EXAMPLE_FRAMES, N_MELS)


def _r(t, on):
    return t.to(torch.bfloat16).to(torch.float32) if on else t


def embed(sd, patches, emulate_bf16=False, use_activation=False, chunk=40):
    """torchvggish `VGG.forward` without the post-processor: (n, 96, 64) patches -> (n, 128) fp32 embeddings."""
    out = []
    x_all = torch.as_tensor(np.asarray(patches), dtype=torch.float32)[:, None]
    with torch.no_grad():
        for c0 in range(0, x_all.shape[0], chunk):
            x = _r(x_all[c0:c0 + chunk], emulate_bf16)
            for i, _, _ in CONVS:
                x = F.relu(F.conv2d(x, _r(sd["features.%d.weight" % i], emulate_bf16), sd["features.%d.bias" % i], padding=1))
                x = _r(x, emulate_bf16)
                if i in POOL_AFTER:
                    x = F.max_pool2d(x, 2, 2)
            x = x.transpose(1, 3).transpose(1, 2).contiguous().view(x.shape[0], -1)       # (frame, mel, channel) order
            for i, _, _ in LINEARS[:2]:
                x = _r(F.relu(F.linear(x, _r(sd["embeddings.%d.weight" % i], emulate_bf16), sd["embeddings.%d.bias" % i])),
                       emulate_bf16)
            i = LINEARS[2][0]
            x = F.linear(x, sd["embeddings.%d.weight" % i], sd["embeddings.%d.bias" % i])
            out.append(F.relu(x) if use_activation else x)
    return torch.cat(out)


def forward(sd, wav, **kw):
    """(B, L) waveforms -> (B * n_examples, 128), clip-major rows."""
    wav = np.asarray(wav, dtype=np.float64)
    return embed(sd, np.concatenate([logmel_examples(w) for w in wav]), **kw)


_WEIGHTS = {}


def det_state_dict(seed=5):
    """The deterministic test weights over torchvggish's keys (shared by the tests of a session, never modified)."""
    from consistencytta_amd import spec
    if seed not in _WEIGHTS:
        _WEIGHTS[seed] = {k: torch.from_numpy(spec.vggish_det_weight("vggish." + k, s, seed))
                          for k, s in spec.vggish_param_spec().items()}
    return _WEIGHTS[seed]
