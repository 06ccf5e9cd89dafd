"""Host side of the mix augmentation (consistencytta_amd/data.py): the pair draw with Python's global `random` and the
captions equal the reference's (tests/golden/mix_augment.npz, made by the reference's tools.torch_tools.augment), the
A-weight table matches tools/mix.py's, and invalid rates and too-short clips fail before any device work."""
import random

import numpy as np
import pytest

import abi
from consistencytta_amd import _native as N
from consistencytta_amd import data

MIX_SYMBOLS = ("ctta_mixer_create", "ctta_mixer_destroy", "ctta_mixer_frames", "ctta_mixer_gain_db", "ctta_mixer_mix")


@pytest.fixture(scope="module")
def built_lib():
    import os
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


@pytest.mark.parametrize("k", [0, 1])
def test_pair_draw_and_captions_equal_the_reference(golden, k):
    g = golden("mix_augment")
    texts = [str(s) for s in g["texts_a"]]
    random.seed(int(g["seeds_a"][k]))
    pairs = data.draw_pairs(len(texts), 3)
    assert [tuple(p) for p in g["a%d_pairs" % k].tolist()] == pairs
    assert data.pair_captions(texts, pairs) == [str(s) for s in g["a%d_captions" % k]]
    random.seed(7)
    texts_b = [str(s) for s in g["texts_b"]]
    pairs_b = data.draw_pairs(2)
    assert pairs_b == [tuple(p) for p in g["b_pairs"].tolist()]
    assert data.pair_captions(texts_b, pairs_b) == [str(s) for s in g["b_captions"]]


def test_draw_consumes_random_like_the_reference():
    """num_items larger than the number of pairs keeps them all; the draw advances `random` by one shuffle."""
    random.seed(3)
    assert sorted(data.draw_pairs(3, 10)) == [(0, 1), (0, 2), (1, 2)]
    after = random.random()
    random.seed(3)
    random.shuffle([0, 1, 2])
    assert random.random() == after


def test_uncapitalize():
    assert data.uncapitalize("") == ""
    assert data.uncapitalize("Dog barks") == "dog barks"
    assert data.uncapitalize("É") == "é"


def test_a_weight_matches_the_reference_table(golden):
    g = golden("mix_augment")
    np.testing.assert_allclose(data.a_weight(16000, 2048), g["aweight_16k"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(data.a_weight(44100, 4096), g["aweight_44k"], rtol=0, atol=1e-12)
    assert data.a_weight(16000, 2048)[0] == -80.0


def test_invalid_rate_and_short_clip_raise_value_error():
    with pytest.raises(ValueError, match="Invalid fs"):
        data.compute_gain(np.zeros(8192, np.float32), 22050)
    with pytest.raises(ValueError, match="Invalid fs"):
        data.mix(np.zeros(8192, np.float32), np.zeros(8192, np.float32), 0.5, 8000)
    with pytest.raises(ValueError, match="shorter than n_fft"):
        data.compute_gain(np.zeros(2047, np.float32), 16000)
    with pytest.raises(ValueError, match="shorter than n_fft"):
        data.compute_gain(np.zeros(4095, np.float32), 44100)
    with pytest.raises(ValueError, match="shorter than n_fft"):
        data.mix(np.zeros(1000, np.float32), np.zeros(1000, np.float32), 0.5, 16000)
    with pytest.raises(ValueError, match="shorter than n_fft"):
        data.collate(["a", "b"], np.zeros((2, 1000), np.float32))
    with pytest.raises(ValueError, match="equal loader batches"):
        data.collate(["a"] * 6, np.zeros((6, 4096), np.float32), groups=4)
    with pytest.raises(ValueError, match="Invalid mode"):
        data.compute_gain(np.zeros(4096, np.float32), 16000, mode="C_weighting")


def test_mixer_is_gpu_only():
    with pytest.raises(N.CttaError):
        data.mixer("cpu")


def test_library_rejects_invalid_mixer_arguments(built_lib):
    h = N.c_void_p()
    assert built_lib.ctta_mixer_create(22050, 0, -80.0, 2, 4096, 1, h) == 1
    assert b"invalid fs" in built_lib.ctta_last_error()
    assert built_lib.ctta_mixer_create(16000, 2, -80.0, 2, 4096, 1, h) == 1
    assert built_lib.ctta_mixer_create(16000, 0, -80.0, 2, 2047, 1, h) == 1
    assert not h.value


def test_mixer_entry_points_are_declared_and_exported(built_lib):
    abi.assert_bound(MIX_SYMBOLS, built_lib)
    assert built_lib.ctta_version() == 100
