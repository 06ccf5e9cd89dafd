"""resampy's kaiser_best on the HIP path (tools/torch_tools.py:54-75 `read_wav_file`): ctta_resample_sinc and
ctta_wave_prepare, `audio.resample`, `data.read_wav_file` / `read_wav_batch` and the evaluation suite's `resample=` switch
against the float64 numpy restatement of resampy 0.4.2's published definition (tests/resampy_ref.py).  resampy is not
installed where these tests run, so the restatement, not the package, is the reference.

Inputs are random int16 / 32768 (exact in fp32).  Every output t is held to the bound the reference itself yields,

    |y_gpu - y_ref| <= (taps_t + 8) * 2^-24 * A_t + 2^-24 * |y_ref|,      A_t = sum |w_i x_i| over the taps of output t:

one fp32 rounding per product, at most taps_t roundings in the sum, a few ulps for the fp32 table entry and the interpolated,
scaled weight, one rounding for the store.  A tap that is off by one table index or one sample misses it by orders of
magnitude (neighbouring weights differ by about 5e-4, the bound is about 1e-5 of A_t)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resampy_ref as R  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from consistencytta_amd import audio, data  # noqa: E402
from consistencytta_amd import audioldm_eval as E  # noqa: E402
from gpu_util import DEV, sync  # noqa: E402

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
_REF = {}


def pcm(tag, n, channels=None):
    """Random int16 samples (seeded by the tag)."""
    rng = np.random.RandomState(sum(ord(c) * (i + 1) for i, c in enumerate(tag)) % (2 ** 31))
    return rng.randint(-32768, 32768, size=(n,) if channels is None else (n, channels)).astype(np.int16)


def clip(tag, n):
    return (pcm(tag, n).astype(np.float64) / 32768.0).astype(np.float32)


def ref(tag, n, sr_orig, sr_new, positions=None):
    """The restatement on clip(tag, n), computed once per case and shared."""
    key = (tag, n, sr_orig, sr_new, None if positions is None else len(positions))
    if key not in _REF:
        _REF[key] = R.resample(clip(tag, n).astype(np.float64), sr_orig, sr_new, positions=positions)
    return _REF[key]


def on_gpu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def assert_within_bound(got, want, what):
    y, A, taps = want
    err, bound = np.abs(np.asarray(got, dtype=np.float64) - y), R.bound(y, A, taps)
    worst = int(np.argmax(err - bound))
    print("%s: %d outputs, taps %d..%d, max error %.3g, smallest bound %.3g, largest error / bound %.3g"
          % (what, len(y), taps.min(), taps.max(), err.max(), bound.min(), (err / np.maximum(bound, 1e-300)).max()))
    assert err.shape == bound.shape and np.all(err <= bound), (what, worst, err[worst], bound[worst])


def run_single(tag, n, sr_orig, sr_new):
    got = audio.resample(on_gpu(clip(tag, n))[None], sr_orig, sr_new)
    sync()
    assert torch.is_tensor(got) and got.dtype == torch.float32 and got.shape == (1, R.plan(n, sr_orig, sr_new)[0])
    return got[0].cpu().numpy()


@pytest.mark.parametrize("tag,n,sr_orig,sr_new", [
    ("short", 50, 44100, 16000),        # shorter than one wing: both wings are cut by both ends of the signal in one output
    ("one-out", 3, 44100, 16000),       # one output
    ("one-in", 1, 16000, 48000),        # three outputs of one sample
    ("int3", 1500, 48000, 16000),       # time_increment == 3.0: every output on an integer position, frac == 0
    ("int160", 4410, 44100, 16000),     # every 160th output on an integer position; several workgroups
    ("up", 2000, 11025, 16000),         # scale == 1, index_step == 512, gain == 1
    ("x16", 8000, 16000, 1000),         # index_step 32: a workgroup's 256 outputs span more input than it stages, two passes each
    ("x32", 10000, 16000, 500),         # index_step 16: not even one output's 4099-sample span fits the staging buffer, samples read from memory
])
def test_resample_against_the_restatement(tag, n, sr_orig, sr_new):
    want = ref(tag, n, sr_orig, sr_new)
    assert_within_bound(run_single(tag, n, sr_orig, sr_new), want, "%s %d: %d -> %d" % (tag, n, sr_orig, sr_new))
    if tag == "short":
        assert want[2].max() <= 50 < 32769 // 185             # no output has a full wing (177 taps)
    if tag == "one-out":
        assert len(want[0]) == 1
    if tag == "one-in":
        assert len(want[0]) == 3
    if tag == "int3":
        assert 1.0 / (16000.0 / 48000) == 3.0
    if tag == "up":
        assert want[2].max() == 127
    if tag == "x16":
        assert len(want[0]) == 500 and want[2].max() > 2000
    if tag == "x32":
        assert len(want[0]) == 312 and want[2].max() > 4093


def test_too_short_a_clip_raises_before_any_launch():
    with pytest.raises(ValueError):
        audio.resample(on_gpu(clip("two", 2))[None], 44100, 16000)
    x = on_gpu(clip("same", 64))[None]
    assert audio.resample(x, 16000, 16000) is x               # equal rates: the input, as read_wav_file never resamples then


def test_long_clip_needs_float64_positions():
    """10 s at 44100 -> 16000, compared at every 97th output and the last 400: fp32 cannot hold t * time_increment there (a
    position near 441000 has an fp32 spacing of 1 / 32 sample, i.e. 16 table entries)."""
    n = 441000
    pos = np.unique(np.concatenate([np.arange(0, 160000, 97), np.arange(160000 - 400, 160000)]))
    want = ref("long", n, 44100, 16000, positions=pos)
    got = run_single("long", n, 44100, 16000)
    assert got.shape == (160000,)
    assert_within_bound(got[pos], want, "long 441000: 44100 -> 16000")
    assert want[2].max() == 353


def test_ragged_batch_equals_each_clip_alone():
    cases = [("short", 50, 44100), ("rag-b", 4410, 22050), ("up", 2000, 11025)]
    clips = [on_gpu(clip(tag, n)) for tag, n, _ in cases]
    got = audio.resample(clips, [sr for _, _, sr in cases], 16000)
    sync()
    assert isinstance(got, list) and [g.shape[0] for g in got] == [18, 3200, 2902]
    for (tag, n, sr), g, x in zip(cases, got, clips):
        assert_within_bound(g.cpu().numpy(), ref(tag, n, sr, 16000), "ragged %s" % tag)
        alone = audio.resample(x[None], sr, 16000)
        assert torch.equal(alone[0], g), tag                  # bit for bit: a clip does not see the rest of the batch
    # a clip already at the target rate stays as it is inside a list
    mixed = audio.resample([clips[0], clips[1]], [44100, 16000], 16000)
    assert mixed[1] is clips[1] and torch.equal(mixed[0], got[0])


def test_wave_prepare_against_the_float64_pipeline():
    seg = 700
    rng = np.random.RandomState(7)
    tail_peak = rng.uniform(-0.3, 0.3, 1000)
    tail_peak[900] = 0.9                                      # the peak lies in the part that is cut off: the second scale is not 1
    ys = [rng.uniform(-0.8, 0.8, 300) + 0.1,                  # n < segment: zero padding
          tail_peak,                                          # n > segment
          rng.uniform(-0.5, 0.5, seg) - 0.2,                  # n == segment
          np.zeros(500)]                                      # all zero: zeros, no NaN
    ys = [y.astype(np.float32) for y in ys]
    lens = [len(y) for y in ys]
    offs = [3 + sum(lens[:i]) + 5 * i for i in range(len(ys))]
    flat = np.zeros(offs[-1] + lens[-1] + 9, np.float32)
    for o, y in zip(offs, ys):
        flat[o:o + len(y)] = y
    got = data.wave_prepare(on_gpu(flat), offs, lens, seg)
    sync()
    got = got.cpu().numpy()
    assert got.shape == (4, seg) and got.dtype == np.float32 and np.all(np.isfinite(got))
    for b, y in enumerate(ys):
        want = R.wave_prepare(y.astype(np.float64), seg)
        err = float(np.abs(got[b] - want).max())
        print("wave_prepare clip %d (n = %d): max error %.3g" % (b, lens[b], err))
        assert err <= ULP
    assert np.all(got[0, 300:] == 0.0) and np.all(got[3] == 0.0)
    assert abs(float(np.abs(got[2]).max()) - 0.5) < 1e-6      # each scaling leaves a peak of 0.5
    first = (tail_peak.astype(np.float32).astype(np.float64) - tail_peak.astype(np.float32).astype(np.float64).mean())
    assert np.abs(first[:seg]).max() < 0.5 * np.abs(first).max()


@pytest.fixture(scope="module")
def wav_files(tmp_path_factory):
    from scipy.io import wavfile
    d = tmp_path_factory.mktemp("resample_wavs")
    wavfile.write(str(d / "stereo22k.wav"), 22050, pcm("stereo22k", 3000, 2))
    wavfile.write(str(d / "mono44k.wav"), 44100, pcm("mono44k", 5001))
    wavfile.write(str(d / "mono16k.wav"), 16000, pcm("mono16k", 1000))
    return {k: str(d / (k + ".wav")) for k in ("stereo22k", "mono44k", "mono16k")}


def _assert_prepared(got, path, seg, target_sr, what):
    """|difference| <= 3 E / P + 4 * 2^-24 with E the largest per-output bound of the resampled clip and P its peak after mean
    removal: the scale 1 / (2 P) meets an error of at most 2 E (sample and mean), the perturbation of P an amplitude of 0.5."""
    key = (path, seg, str(target_sr))
    if key not in _REF:
        _REF[key] = R.read_wav_file(path, seg, target_sr)
    want, E_, P = _REF[key]
    assert P >= 0.25
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("%s: max error %.3g, bound %.3g (E = %.3g, P = %.3g)" % (what, err, 3 * E_ / P + 4 * ULP, E_, P))
    assert got.shape == want.shape and err <= 3 * E_ / P + 4 * ULP


def test_read_wav_file_and_batch(wav_files):
    seg = 2000                                                # 3000 at 22050 -> 2176 (cut), 5001 at 44100 -> 1814 (padded)
    names = ["stereo22k", "mono44k", "mono16k"]
    batch = data.read_wav_batch([wav_files[k] for k in names], seg)
    sync()
    assert batch.shape == (3, seg) and batch.dtype == torch.float32 and batch.is_cuda
    for b, k in enumerate(names):
        _assert_prepared(batch[b].cpu().numpy(), wav_files[k], seg, 16000, "read_wav_batch %s" % k)
        one = data.read_wav_file(wav_files[k], seg)
        assert one.shape == (1, seg) and torch.equal(one[0], batch[b]), k
    assert float(batch[1, 1814:].abs().max()) == 0.0 and float(batch[1, 1813].abs()) > 0.0


def test_read_wav_file_through_two_rates(wav_files):
    seg = 6000                                                # 2176 * 3 = 6528 (cut), 1814 * 3 = 5442 (padded), 3000 (padded)
    names = ["stereo22k", "mono44k", "mono16k"]
    batch = data.read_wav_batch([wav_files[k] for k in names], seg, [16000, 48000])
    sync()
    for b, k in enumerate(names):
        _assert_prepared(batch[b].cpu().numpy(), wav_files[k], seg, [16000, 48000], "two rates %s" % k)


class _Stub:
    def eval(self):
        return self


def test_evaluation_switch_for_a_22050_hz_file(wav_files):
    path = wav_files["stereo22k"]
    with pytest.raises(N.CttaError):
        E.read_centered_wav(path, 16000)
    with pytest.raises(N.CttaError):
        E.load_audio_task(path, 16000)
    mono, sr = R.read_mono(path)
    key = ("eval22k",)
    if key not in _REF:
        _REF[key] = R.resample(mono, sr, 16000)
    y, A, taps = _REF[key]
    got = E.read_centered_wav(path, 16000, resampler="kaiser_best")
    assert got.dtype == np.float64 and got.shape == y.shape
    assert_within_bound(got, (y - y.mean(), A, taps), "read_centered_wav 22050 -> 16000")
    task = E.load_audio_task(path, 16000, target_length=10, resampler="kaiser_best")      # 0.1 s: cut to 1600
    assert task.shape == (1600,)
    assert_within_bound(task, (y[:1600], A[:1600], taps[:1600]), "load_audio_task 22050 -> 16000")
    ds = E.WaveDataset(os.path.dirname(path), sr=16000, target_length=10, resampler="kaiser_best")
    w, name = ds[[os.path.basename(p) for p in ds.datalist].index("stereo22k.wav")]
    assert name == "stereo22k.wav" and tuple(w.shape) == (1, 32000)
    assert_within_bound(w[0, :1600].numpy(), ((y - y.mean())[:1600], A[:1600], taps[:1600]), "WaveDataset 22050 -> 16000")
    with pytest.raises(ValueError):
        E.read_centered_wav(path, 16000, resampler="kaiser_fast")


def test_clap_wave_with_and_without_the_switch(wav_files):
    from consistencytta_amd.clap import Resampler
    seconds = 0.05                                            # 2400 samples at 48 kHz; 1000 at 16 kHz -> 3000, cut
    w = torch.from_numpy(clip("clap", 1000))
    h = E.EvaluationHelper(16000, DEV, mel_model=_Stub(), resample="kaiser_best")
    got = h._clap_wave(w, seconds)
    sync()
    assert got.shape == (1, 2400) and got.dtype == torch.float32
    y, A, taps = R.resample(clip("clap", 1000).astype(np.float64), 16000, 48000)
    E_, P = float(R.bound(y, A, taps).max()), float(np.abs(y - y.mean()).max())
    assert P >= 0.25
    err = float(np.abs(got[0].cpu().numpy().astype(np.float64) - R.wave_prepare(y, 2400)).max())
    print("_clap_wave: max error %.3g, bound %.3g" % (err, 3 * E_ / P + 4 * ULP))
    assert err <= 3 * E_ / P + 4 * ULP
    # the default is what it was: clap.Resampler and the fp32 normalisation
    h0 = E.EvaluationHelper(16000, DEV, mel_model=_Stub())
    x = Resampler(orig_freq=16000, new_freq=48000)(w.reshape(1, -1).float().to(DEV))
    x = x - x.mean()
    x = x / (x.abs().max() + 1e-8) / 2
    x = x[:, :2400]
    x = x / (x.abs().max() + 1e-8) / 2
    assert torch.equal(h0._clap_wave(w, seconds), x)
