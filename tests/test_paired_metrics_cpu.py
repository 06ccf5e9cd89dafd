"""Host side of the paired metrics (audioldm_eval/eval.py:137-179): the float64 restatement the GPU tests compare against
(tests/paired_metrics_ref.py) checked against facts that hold by construction, the pairing of `MelPairedDataset`, the helper's
constructor arguments and the library's entry points.  Nothing here needs a GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import abi
import cases  # noqa: E402
import paired_metrics_ref as R  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from consistencytta_amd import audioldm_eval as E  # noqa: E402

PAIRED_SYMBOLS = ("ctta_stft_create_dft", "ctta_lsd", "ctta_ssim_mean", "ctta_psnr_mse")


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def _image(tag, H, W):
    wav = cases.eval_waves("paired.cpu." + tag, 1, 16000).numpy()[0].astype(np.float64)
    return R.stft_magnitude(wav, 743, 160)[:H, :W]


def test_stft_lengths_of_the_lsd():
    assert int(2048 / (44100 / 16000)) == 743 and R.n_fft_of(16000) == 743 and R.n_fft_of(32000) == 1486
    assert R.hop_of(16000) == 160 and R.hop_of(32000) == 320
    assert R.TIME_OFFSET == 1120


def test_ssim_of_an_image_with_itself_is_exactly_one():
    for R_ in (1.0, 2.0):
        x = _image("self", 40, 50)
        assert R.ssim(x, x.copy(), R_) == 1.0
        assert R.ssim(x.astype(np.float32), x.astype(np.float32), R_, dtype=np.float32) == 1.0
    with pytest.raises(ValueError):
        R.ssim(x[:6], x[:6], 1.0)


def test_ssim_of_constant_images_is_the_luminance_term():
    """Zero variance and covariance on both sides: the contrast / structure factor is C2 / C2 and S = (2 a b + C1) / (a^2 + b^2 + C1)."""
    for data_range, a, c in ((1.0, 0.5, 0.25), (2.0, 120.0, 30.0), (2.0, 0.0, 0.125)):
        x = np.full((12, 15), a)
        b, c1 = a + c, (0.01 * data_range) ** 2
        want = (2 * a * b + c1) / (a * a + b * b + c1)
        assert abs(R.ssim(x, x + c, data_range) - want) <= 1e-12
    # a window that straddles structure is below the constant-image value
    y = _image("lum", 12, 15)
    assert R.ssim(y, y + 30.0, 2.0) < 1.0


def test_ssim_window_and_covariance_normalisation():
    """One 7 x 7 window written out: sample covariance (49 / 48), K1 = 0.01, K2 = 0.03."""
    x, y = _image("w.x", 7, 7), _image("w.y", 7, 7)
    ux, uy = x.mean(), y.mean()
    vx, vy, vxy = x.var(ddof=1), y.var(ddof=1), ((x - ux) * (y - uy)).sum() / 48.0
    c1, c2 = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2
    want = (2 * ux * uy + c1) * (2 * vxy + c2) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    assert R.ssim_map(x, y, 2.0).shape == (1, 1)
    assert abs(R.ssim(x, y, 2.0) - want) <= 1e-9 * abs(want)
    assert R.ssim_map(_image("w.x", 20, 31), _image("w.y", 20, 31), 2.0).shape == (14, 25)


def test_psnr_of_a_shifted_image():
    x = np.clip(_image("psnr", 64, 101) / 50.0, 0, 0.8)
    for d in (0.1, 1e-3):
        assert abs(R.psnr(x, x + d) - (-20 * np.log10(d))) <= 1e-9
    assert np.isinf(R.psnr(x, x.copy())) and R.mse(x, x.copy()) == 0.0


def test_lsd_of_a_scaled_copy():
    e = _image("lsd", 101, 372)
    for c in (4.0, 0.25, 1.7):
        assert abs(R.lsd(e, c * e) - abs(2 * np.log10(c))) <= 1e-9
    assert R.lsd(e, e) <= 1e-9
    z = e.copy()
    z[::3, ::5] = 0.0                                       # the guards: log10(t^2 / 1e-24 + 1e-12) of about 24 in a fifth of the bins of
    assert np.isfinite(R.lsd(z, e)) and R.lsd(z, e) > 3.0 and np.isfinite(R.lsd(e, z))      # every third frame: 24 / sqrt(5) / 3


@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
@pytest.mark.parametrize("n_fft,hop,L", [(743, 160, 16000), (743, 160, 16037), (1486, 320, 32000), (512, 160, 8000)])
def test_stft_restatement_equals_rfft_of_the_windowed_frames(n_fft, hop, L, pad_mode):
    """The DFT sum of the restatement against numpy.fft.rfft of frames cut by hand from the explicitly padded signal."""
    wav = cases.eval_waves("paired.cpu.stft", 1, L).numpy()[0].astype(np.float64)
    half, frames = n_fft // 2, 1 + L // hop
    need = (frames - 1) * hop + n_fft                        # an odd n_fft with hop | L: one sample past the n_fft // 2 padding
    extra = max(0, need - (L + 2 * half))
    assert extra == (1 if (n_fft % 2 and L % hop == 0) else 0)
    if pad_mode == "reflect":
        p = np.concatenate([wav[1:half + 1][::-1], wav, wav[-2:-(half + extra) - 2:-1]])
    else:
        p = np.concatenate([np.zeros(half), wav, np.zeros(half + extra)])
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    want = np.abs(np.stack([np.fft.rfft(p[f * hop:f * hop + n_fft] * win) for f in range(frames)]))
    got = R.stft_magnitude(wav, n_fft, hop, pad_mode)
    assert got.shape == (frames, n_fft // 2 + 1)
    assert float(np.abs(got - want).max()) <= 1e-10 * float(want.max())


def test_normalised_mel_range_and_shape():
    wav = cases.eval_waves("paired.cpu.mel", 1, 16000).numpy()[0]
    m = R.normalised_mel(wav, 16000)
    assert m.shape == (64, 101) and float(m.min()) >= 0.0 and float(m.max()) <= 1.0 and float(m.std()) > 0.01
    assert float(R.normalised_mel(np.zeros(16000), 16000).max()) == 0.0         # clamp(1e-5): (20 * -5 - 20 + 100) / 100 = -0.2 -> 0


def test_lsd_audio_pair_follows_the_reference():
    gen = np.arange(3000, dtype=np.float64) % 17 - 3.0
    gt = np.arange(2500, dtype=np.float64) % 13 - 9.0
    a1, a2 = R.lsd_audio_pair(gen, gt)
    assert a1.shape == a2.shape == (1880,)
    g = gen[1120:]
    np.testing.assert_allclose(a1, ((g - g.mean()) / np.abs(g).max())[:1880], rtol=0, atol=1e-15)   # the maximum BEFORE the mean
    np.testing.assert_allclose(a2, ((gt - gt.mean()) / np.abs(gt).max())[:1880], rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        R.lsd_audio_pair(gen[:1120], gt)


def test_mel_paired_dataset_pairs_by_base_name(tmp_path):
    from scipy.io import wavfile
    d1, d2 = tmp_path / "a", tmp_path / "b"
    d1.mkdir()
    d2.mkdir()
    tone = (np.sin(np.arange(4800) * 0.05) * 9000).astype(np.int16)
    for name in ("x.wav", "y.wav", "only1.wav", "notes.txt"):
        wavfile.write(str(d1 / name), 16000, tone[:1600])
    for name in ("y.wav", "x.wav", "only2.wav"):
        wavfile.write(str(d2 / name), 48000, tone)
    ds = E.MelPairedDataset(str(d1), str(d2), None, 16000)
    assert len(ds) == 2 and [ds.name(i) for i in range(2)] == ["x.wav", "y.wav"]
    mel1, mel2, name, (a1, a2) = ds[0]
    assert mel1 is None and mel2 is None and name == "x.wav"
    assert a1.shape == (1600,) and a2.shape == (1600,) and abs(a1.mean()) < 1e-12      # whole file, strided by 3, mean removed
    assert len(E.MelPairedDataset(str(d1), str(d2), None, 16000, limit_num=1)) == 0     # only1.wav against only2.wav


def test_helper_arguments_and_unpaired_result():
    class Stub:
        def eval(self):
            return self

    h = E.EvaluationHelper(16000, "cpu", mel_model=Stub())
    assert h.paired_metrics is False and h.stft_pad_mode == "reflect" and h.stft_ssim_data_range == 2.0
    assert (h._lsd_stft.n_fft, h._lsd_stft.hop) == (743, 160)
    h32 = E.EvaluationHelper(32000, "cpu", mel_model=Stub(), paired_metrics=True, stft_pad_mode="constant", stft_ssim_data_range=1.0)
    assert (h32._lsd_stft.n_fft, h32._lsd_stft.hop, h32._lsd_stft.pad_zero) == (1486, 320, 1)
    assert h.calculate_lsd([], same_name=False) == {"lsd": -1, "ssim_stft": -1}
    assert h.calculate_psnr_ssim([], same_name=False) == {"psnr": -1, "ssim": -1}
    with pytest.raises(ValueError):
        E.EvaluationHelper(16000, "cpu", mel_model=Stub(), stft_pad_mode="edge")
    with pytest.raises(ValueError):
        E.EvaluationHelper(16000, "cpu", mel_model=Stub(), stft_ssim_data_range=0.0)
    with pytest.raises(ValueError, match="time offset"):
        h.calculate_lsd([(None, None, "a.wav", (np.ones(1000), np.ones(4000)))])


def test_paired_entry_points_are_declared_and_exported(built_lib):
    abi.assert_bound(tuple(PAIRED_SYMBOLS) + ("ctta_ssim_tiles",), built_lib)
    assert N.FUNCTIONS["ctta_ssim_tiles"].c_restype == "int64_t"
    assert built_lib.ctta_ssim_tiles(7, 7, 7) == 1 and built_lib.ctta_ssim_tiles(30, 38, 7) == 1
    assert built_lib.ctta_ssim_tiles(31, 39, 7) == 4 and built_lib.ctta_ssim_tiles(6, 9, 7) == 0
    assert N.CONSTANTS["CTTA_PAIR_MAX"] == 256
