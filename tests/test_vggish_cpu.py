"""Host side of the Frechet Audio Distance (audioldm_eval/metrics/fad.py): the VGGish parameter table, the example count, the
distance arithmetic, the metric's own file loader and the library's entry points.  Nothing here needs a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import vggish_torch as VT  # noqa: E402
import abi
from consistencytta_amd import _native as N  # noqa: E402
from consistencytta_amd import audioldm_eval as E  # noqa: E402
from consistencytta_amd import spec  # noqa: E402

VGGISH_SYMBOLS = ("ctta_vggish_frontend_create", "ctta_wav_to_vggish_logmel", "ctta_maxpool2")


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def test_param_spec_lists_the_released_keys():
    sd = spec.vggish_param_spec()
    want = [("features.0", (64, 1, 3, 3)), ("features.3", (128, 64, 3, 3)), ("features.6", (256, 128, 3, 3)),
            ("features.8", (256, 256, 3, 3)), ("features.11", (512, 256, 3, 3)), ("features.13", (512, 512, 3, 3)),
            ("embeddings.0", (4096, 12288)), ("embeddings.2", (4096, 4096)), ("embeddings.4", (128, 4096))]
    keys = []
    for p, shape in want:
        keys += [p + ".weight", p + ".bias"]
        assert tuple(sd[p + ".weight"]) == shape and tuple(sd[p + ".bias"]) == (shape[0],)
    assert list(sd) == keys and len(sd) == 18
    w = spec.vggish_det_weight("vggish.features.3.weight", (128, 64, 3, 3), 5)
    assert w.dtype == np.float32 and float(np.abs(w).max()) <= np.sqrt(6.0 / 576)
    assert float(np.abs(spec.vggish_det_weight("vggish.features.3.bias", (128,), 5)).max()) <= 0.05


@pytest.mark.parametrize("n_samples,want", [(15599, 0), (15600, 1), (32000, 2), (160000, 10), (0, 0), (399, 0)])
def test_n_examples(n_samples, want):
    assert E.VGGish().n_examples(n_samples) == want
    assert VT.n_examples(n_samples) == want
    if n_samples:
        assert VT.logmel_examples(np.zeros(n_samples)).shape == (want, 96, 64)


def test_vggish_rejects_the_post_processor():
    with pytest.raises(RuntimeError):
        E.VGGish(use_pca=True)


def _sets():
    u = lambda name, shape: spec.det_uniform("vggish.fad." + name, shape, 21).astype(np.float64)
    mix = u("mix", (128, 128)) * 0.2 + np.eye(128)
    a = (u("a", (200, 128)) * 1.5) @ mix + 0.3
    b = (u("b", (200, 128)) * 1.2) @ mix.T - 0.2
    return a.astype(np.float32), b.astype(np.float32)


def test_calculate_fad_is_the_frechet_distance():
    a, b = _sets()
    trace = float(np.trace(np.cov(a, rowvar=False)))
    same = E.calculate_fad(a, a.copy())
    assert set(same) == {"frechet_audio_distance"} and abs(same["frechet_audio_distance"]) <= 1e-6 * trace
    fad = E.calculate_fad(torch.from_numpy(a), torch.from_numpy(b))["frechet_audio_distance"]
    fid = E.calculate_fid({"x": torch.from_numpy(a)}, {"x": torch.from_numpy(b)}, "x")["frechet_distance"]
    assert isinstance(fad, float) and fad > 0.0
    assert abs(fad - fid) <= 1e-9 * abs(fid)
    assert abs(E.calculate_fad(a, b)["frechet_audio_distance"] - fad) <= 1e-9 * abs(fad)      # arrays or tensors
    # written out: |mu1 - mu2|^2 + tr(S1) + tr(S2) - 2 tr(sqrt(S1 S2)), through the eigenvalues of S1 S2
    s1, s2 = np.cov(a, rowvar=False), np.cov(b, rowvar=False)
    d = a.mean(0).astype(np.float64) - b.mean(0).astype(np.float64)
    direct = d @ d + np.trace(s1) + np.trace(s2) - 2 * np.sqrt(np.linalg.eigvals(s1 @ s2).real.clip(min=0)).sum()
    assert abs(fad - direct) <= 1e-6 * abs(direct)
    assert E.calculate_fad(np.zeros((0, 128), np.float32), b) == -1
    assert E.calculate_fad(a, torch.zeros(0, 128)) == -1


def test_load_audio_task_follows_the_reference_loader(tmp_path):
    from scipy.io import wavfile
    rng = np.random.RandomState(3)
    stereo = (rng.randint(-9000, 9000, size=(48000, 2)) + np.array([1200, 300])).astype(np.int16)
    wavfile.write(str(tmp_path / "st16.wav"), 16000, stereo)
    w = E.load_audio_task(str(tmp_path / "st16.wav"))
    want = (stereo / 32768.0).mean(axis=1)
    assert w.dtype == np.float64 and w.shape == (48000,)
    np.testing.assert_array_equal(w, want)                       # int16 / 32768, mean over the channels
    assert abs(w.mean() - 750.0 / 32768.0) < 2e-3                  # the DC offset stays
    assert abs(E.read_centered_wav(str(tmp_path / "st16.wav"), 16000).mean()) < 1e-12    # ... unlike the classifier's loader
    np.testing.assert_array_equal(E.load_audio_task(str(tmp_path / "st16.wav"), target_length=100), want[:16000])
    mono48 = rng.randint(-20000, 20000, size=(96000,)).astype(np.int16)
    wavfile.write(str(tmp_path / "m48.wav"), 48000, mono48)
    np.testing.assert_array_equal(E.load_audio_task(str(tmp_path / "m48.wav")), mono48[::3] / 32768.0)
    np.testing.assert_array_equal(E.load_audio_task(str(tmp_path / "m48.wav"), target_length=50), (mono48[::3] / 32768.0)[:8000])
    np.testing.assert_array_equal(E.load_audio_task(str(tmp_path / "m48.wav"), target_sr=48000, target_length=150),
                                  (mono48 / 32768.0)[:72000])
    wavfile.write(str(tmp_path / "m22.wav"), 22050, mono48[:22050])
    with pytest.raises(RuntimeError, match="not an integer multiple"):
        E.load_audio_task(str(tmp_path / "m22.wav"))
    for name, data in (("f32.wav", (mono48[:16000] / 32768.0).astype(np.float32)), ("i32.wav", mono48[:16000].astype(np.int32) << 16),
                       ("u8.wav", (mono48[:16000] >> 8).astype(np.int16).astype(np.uint8))):
        wavfile.write(str(tmp_path / name), 16000, data)           # other sample formats are refused, not converted
        with pytest.raises(RuntimeError, match="16-bit PCM"):
            E.load_audio_task(str(tmp_path / name))


def test_restatement_and_spec_agree_on_the_published_constants():
    """The helper the GPU tests compare against carries the constants of vggish_params.py on its own; they must be the ones
    `spec.VGGISH_CONFIG` gives the HIP path.  The rest is a self-check of the helper's mel matrix: 64 bands between 125 and
    7500 Hz, DC row zero, no area normalisation, and the log of silence is ln(0.01)."""
    c = spec.VGGISH_CONFIG
    assert (c["sample_rate"], c["window"], c["hop"], c["n_fft"]) == (VT.SAMPLE_RATE, VT.WINDOW, VT.HOP, VT.N_FFT)
    assert (c["mel_bins"], c["fmin"], c["fmax"], c["log_offset"]) == (VT.N_MELS, VT.MEL_MIN_HZ, VT.MEL_MAX_HZ, VT.LOG_OFFSET)
    assert c["example_frames"] == c["example_hop"] == VT.EXAMPLE_FRAMES
    assert tuple(c["convs"]) == VT.CONVS and tuple(c["pool_after"]) == VT.POOL_AFTER and tuple(c["linears"]) == VT.LINEARS
    m = VT.mel_matrix()
    assert m.shape == (257, 64) and float(m[0].max()) == 0.0 and float(m.min()) >= 0.0 and float(m.max()) <= 1.0
    hz = np.linspace(0, 8000, 257)
    assert float(m[hz < 125].max()) == 0.0 and float(m[hz > 7500].max()) == 0.0
    assert (m.argmax(0)[1:] >= m.argmax(0)[:-1]).all()
    np.testing.assert_allclose(VT.logmel_examples(np.zeros(15600)), np.log(0.01), rtol=0, atol=1e-15)


def test_vggish_entry_points_are_declared_and_exported(built_lib):
    abi.assert_bound(VGGISH_SYMBOLS, built_lib)
    assert built_lib.ctta_version() == 100
