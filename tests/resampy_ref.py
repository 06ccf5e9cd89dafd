"""float64 numpy restatement of `resampy.resample(x, sr_orig, sr_new, filter="kaiser_best")` as published in resampy 0.4.2
(`core.resample`, `filters.sinc_window`, `interpn.resample_f`), the version the reference's environment.yml pins, and of the
rest of `tools/torch_tools.py:54-75` (`read_wav_file`).  resampy is a pip package outside the reference tree and is not
installed where these tests run, so nothing here was compared with the package itself and no fixture comes from it: the
definition is pinned against facts that hold by construction (tests/test_resample_cpu.py) and the HIP path against this
file (tests/test_resample_gpu.py).  Not collected by pytest."""
import numpy as np

KAISER_BEST = (64, 9, 14.769656459379492, 0.9475937167399596)        # num_zeros, precision, beta, rolloff


def sinc_window(num_zeros=64, precision=9, beta=KAISER_BEST[2], rolloff=KAISER_BEST[3]):
    """filters.sinc_window with window = scipy.signal.windows.kaiser(., beta) (= numpy.kaiser): the right half of the
    windowed sinc, num_zeros * 2**precision + 1 float64 entries; returns (win, num_table)."""
    num_table = 2 ** precision
    n = num_table * num_zeros
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
    taper = np.kaiser(2 * n + 1, beta)[n:]
    return taper * sinc_win, num_table


def plan(n_in, sr_orig, sr_new, num_table=512):
    """The scalars of core.resample: (n_out, sample_ratio, scale, time_increment, index_step)."""
    sample_ratio = float(sr_new) / sr_orig
    n_out = int(n_in * sr_new / sr_orig)
    scale = min(1.0, sample_ratio)
    return n_out, sample_ratio, scale, 1.0 / sample_ratio, int(scale * num_table)


def resample(x, sr_orig, sr_new, positions=None, filter=KAISER_BEST):
    """-> (y, A, taps) at the outputs `positions` (default: all n_out of them): y[t] as resampy computes it in float64,
    A[t] = sum |w_i x_i| over its taps and the number of taps.  ValueError when n_out < 1, like resampy."""
    x = np.asarray(x, dtype=np.float64)
    win, num_table = sinc_window(*filter)
    n_in = x.shape[0]
    n_out, sample_ratio, scale, time_increment, index_step = plan(n_in, sr_orig, sr_new, num_table)
    if n_out < 1:
        raise ValueError("Input signal length=%d is too small to resample from %s->%s" % (n_in, sr_orig, sr_new))
    if sample_ratio < 1:
        win = sample_ratio * win
    delta = np.diff(win, append=win[-1])
    n_win = win.shape[0]
    ts = np.arange(n_out) if positions is None else np.asarray(positions, dtype=np.int64)
    y, A, taps = np.zeros(len(ts)), np.zeros(len(ts)), np.zeros(len(ts), dtype=np.int64)
    for o, t in enumerate(ts):
        time_register = float(t) * time_increment
        n = int(time_register)
        frac = scale * (time_register - n)
        index_frac = frac * num_table
        offset = int(index_frac)
        eta = index_frac - offset
        i = np.arange(max(0, min(n + 1, (n_win - offset) // index_step)))
        w = win[offset + i * index_step] + eta * delta[offset + i * index_step]
        p = w * x[n - i]
        frac = scale - frac
        index_frac = frac * num_table
        offset = int(index_frac)
        eta = index_frac - offset
        k = np.arange(max(0, min(n_in - n - 1, (n_win - offset) // index_step)))
        w = win[offset + k * index_step] + eta * delta[offset + k * index_step]
        q = w * x[n + k + 1]
        y[o] = p.sum() + q.sum()
        A[o] = np.abs(p).sum() + np.abs(q).sum()
        taps[o] = len(i) + len(k)
    return y, A, taps


def bound(y, A, taps):
    """The per-output bound of an fp32-table, fp32-sample evaluation against `resample`: one rounding per product and per
    addition, a few ulps for the table entry and the interpolated, scaled weight, one rounding for the store."""
    return (taps + 8) * 2.0 ** -24 * A + 2.0 ** -24 * np.abs(y)


def wave_prepare(wav, segment):
    """torch_tools.py:69-73 in float64: mean removal, peak 0.5, cut / zero-pad to `segment`, peak 0.5 again -> (segment,)."""
    wav = np.asarray(wav, dtype=np.float64)
    wav = wav - wav.mean()
    wav = wav / (np.abs(wav).max() + 1e-8) / 2
    out = np.zeros(segment)
    out[:min(segment, len(wav))] = wav[:segment]
    return out / (np.abs(out).max() + 1e-8) / 2


def read_mono(path):
    """soundfile.read + librosa.to_mono through scipy.io.wavfile: integer PCM scaled to [-1, 1), unsigned 8-bit re-centred,
    the mean over the channels -> (float64 samples, rate)."""
    from scipy.io import wavfile
    sr, a = wavfile.read(path)
    if a.dtype.kind == "i":
        a = a.astype(np.float64) / float(2 ** (8 * a.dtype.itemsize - 1))
    elif a.dtype.kind == "u":
        a = (a.astype(np.float64) - 128.0) / 128.0
    else:
        a = a.astype(np.float64)
    return (a.mean(axis=1) if a.ndim > 1 else a), sr


def read_wav_file(path, segment, target_sr=16000):
    """torch_tools.py:54-75 on the float64 resampler -> (wave (segment,) float64, E, P): E the largest per-output bound of the
    resampled clip (0 without a resampling stage; a second stage passes the first one's E on times its largest sum of
    |weights| and adds its own), P the resampled clip's peak after mean removal."""
    wav, cur = read_mono(path)
    E = 0.0
    for tar in (target_sr if isinstance(target_sr, list) else [target_sr]):
        if cur != tar:
            carried = E * float(resample(np.ones(len(wav)), cur, tar)[1].max()) if E else 0.0
            wav, A, taps = resample(wav, cur, tar)
            E = carried + float(bound(wav, A, taps).max())
            cur = tar
    return wave_prepare(wav, segment), E, float(np.abs(wav - wav.mean()).max())
