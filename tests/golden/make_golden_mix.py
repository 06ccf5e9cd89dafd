"""Fixture for the mix augmentation of the training batch (consistencytta_amd/data.py, csrc/mix_augment.hip), produced
by the REFERENCE's own `tools.mix` and `tools.torch_tools.augment` (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mix.py

The inputs are regenerated in the tests by `test_wave` below.  Every case seeds Python's global `random` itself before
calling the reference's `augment`, which draws its pairs from it; the pairs are recorded from the reference's own
calls of `mix` (the clips are distinct, so a row identifies its index).  The reference computes in float64; gains,
t and the A-weight tables are stored as float64, the mixtures as float32 (their values are <= 0.5, float32 keeps
them to 3e-8, and float64 would not fit the fixture size): case A seed 0 in full, seed 1 every 4th sample, case B
the first 32768 samples and every 8th sample."""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from consistencytta_amd import spec  # noqa: E402

TEXTS_A = ["A dog barks twice", "Rain falls on a tin roof", "", "Birds chirp nearby", "a man speaks",
           "Éclair wrappers rustle"]
KINDS_A = ["tone", "low", "tone", "silent", "tone", "tone"]
TEXTS_B = ["Church bells ring", "Thunder rumbles in the distance"]
KINDS_B = ["tone", "low"]
SEEDS_A = (0, 1234)
L_A, L_B = 32768, 163840


def test_wave(B, L, tag, kinds):
    """Deterministic clips of different loudness: 'tone' = a chirp with bursts over decaying noise, 'low' = a 30 Hz
    sine with faint noise (energy far below the A-weighting's passband), 'silent' = zeros.  No NaN."""
    t = np.arange(L) / 16000.0
    out = []
    for b in range(B):
        n = spec.det_uniform(tag + ".n%d" % b, (L,), 37).astype(np.float64)
        if kinds[b] == "silent":
            x = np.zeros(L)
        elif kinds[b] == "low":
            x = 0.6 * np.sin(2 * np.pi * 30.0 * t) + 0.002 * n
        else:
            amp = (0.6, 0.05, 0.25, 0.9, 0.12, 0.4)[b % 6]
            env = 0.55 + 0.45 * np.sin(2 * np.pi * (0.7 + 0.3 * b) * t) ** 2
            x = amp * env * np.sin(2 * np.pi * (300 + 650 * b + 400 * t) * t) + 0.1 * amp * n * np.exp(-2 * t)
        out.append(x.astype(np.float32))
    return torch.from_numpy(np.stack(out))


def load_reference():
    import make_golden_mel
    _, TT = make_golden_mel.load_reference_stft()   # stubs librosa / soundfile / resampy, maps the `tools` package
    import importlib
    return importlib.import_module("tools.mix"), TT


def run_augment(M, TT, wav, texts, num_items, seed):
    """The reference's augment with `random` seeded; returns (pairs, captions, t, (g1, g2), mixtures)."""
    rows = wav.numpy()
    rec = []
    orig = TT.mix

    def recording_mix(s1, s2, r, fs):
        i = [k for k in range(rows.shape[0]) if np.array_equal(rows[k], s1)]
        j = [k for k in range(rows.shape[0]) if np.array_equal(rows[k], s2)]
        assert len(i) == 1 and len(j) == 1
        g1, g2 = np.max(M.compute_gain(s1, fs)), np.max(M.compute_gain(s2, fs))
        rec.append((i[0], j[0], 1.0 / (1 + np.power(10, (g1 - g2) / 20.) * (1 - r) / r), g1, g2))
        return orig(s1, s2, r, fs)

    TT.mix = recording_mix
    try:
        random.seed(seed)
        mixed, captions = TT.augment(wav, list(texts), num_items=num_items)
    finally:
        TT.mix = orig
    pairs = np.array([(a, b) for a, b, _, _, _ in rec], dtype=np.int32)
    t = np.array([x[2] for x in rec], dtype=np.float64)
    g = np.array([(x[3], x[4]) for x in rec], dtype=np.float64)
    return pairs, np.array(captions), t, g, mixed.numpy()


def main():
    M, TT = load_reference()
    out = {"seeds_a": np.array(SEEDS_A), "texts_a": np.array(TEXTS_A), "texts_b": np.array(TEXTS_B),
           "aweight_16k": M.a_weight(16000, 2048), "aweight_44k": M.a_weight(44100, 4096)}
    wa = test_wave(6, L_A, "mixA", KINDS_A)
    for mode, tag in (("A_weighting", "a"), ("RMSE", "rmse")):
        for fs, ftag in ((16000, "16k"), (44100, "44k")):
            out["gain_%s%s" % (tag, ftag)] = np.stack([M.compute_gain(w, fs, mode=mode) for w in wa.numpy()])
    for k, seed in enumerate(SEEDS_A):
        pairs, caps, t, g, mixed = run_augment(M, TT, wa, TEXTS_A, 3, seed)
        out["a%d_pairs" % k], out["a%d_captions" % k], out["a%d_t" % k], out["a%d_g" % k] = pairs, caps, t, g
        out["a%d_mix" % k] = (mixed if k == 0 else mixed[:, ::4]).astype(np.float32)
    wb = test_wave(2, L_B, "mixB", KINDS_B)
    out["gain_b_a16k"] = np.stack([M.compute_gain(w, 16000) for w in wb.numpy()])
    pairs, caps, t, g, mixed = run_augment(M, TT, wb, TEXTS_B, 1, 7)
    out["b_pairs"], out["b_captions"], out["b_t"], out["b_g"] = pairs, caps, t, g
    out["b_mix_head"] = mixed[0, :32768].astype(np.float32)
    out["b_mix_sub"] = mixed[0, ::8].astype(np.float32)
    path = os.path.join(HERE, "mix_augment.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    for k, v in out.items():
        print("  %-14s %-10s %s" % (k, v.dtype, v.shape))


if __name__ == "__main__":
    main()
