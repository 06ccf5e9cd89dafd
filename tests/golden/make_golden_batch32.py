"""Fixture pinning BASELINE.json configs[1] at its benchmarked size (batch 32, L = 32, ragged masks) to the REFERENCE's
own modules (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_batch32.py

Same recipe as `golden_pipeline` in make_golden.py: the guided light U-Net (one query, w = 4, no post-CFG), then
`decode_first_stage`, then `vocoder`, on the inputs of `cases.batch32_inputs()`.  Clips are independent in the
reference too, so each of the 32 clips runs alone at B = 1 in fp32 on the CPU.

The whole batch is 90 MB of outputs, so `pipeline_batch32.npz` keeps:
  * for the clips of `cases.batch32_clips` (rows 0 and 31 and the shortest mask): latent and mel in full, and the float
    waveform's first 16 384 samples plus every 8th sample, all float16 (like `pipeline_light.npz`'s waveform; relative
    rounding <= 2^-11) so that the file stays under 1 MiB;
  * for every clip: a `cases.sample_index(numel, 512)` sample of latent, mel and waveform, the full fp64 L2 norm and
    the absolute maximum of each;
  * the batch-global centre (max + min) / 2 over all 32 waveforms, with max and min: what `vocoder_infer`
    (hifigan/utilities.py:76-91) subtracts before the int16 conversion;
  * fp64 sums of `enc` and `noise` and the mask lengths, so that a change of torch's RNG fails as "inputs changed".
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import cases  # noqa: E402
import ref_import  # noqa: E402
from consistencytta_amd import spec  # noqa: E402
from make_golden import ref_unet, ref_vae, save  # noqa: E402

WAV_HEAD, WAV_STRIDE = 16384, 8


def compute(ns):
    """Runs the 32 clips; returns the inputs, the per-clip outputs (latent, mel, waveform) and the scale factor."""
    X = cases.batch32_inputs()
    outs = []
    with torch.no_grad():
        m = ref_unet(ns, spec.LIGHT_UNET_CONFIG, True)
        vae, sf = ref_vae(ns, spec.VAE_DDCONFIG, spec.HIFIGAN_16K_64)
        for b in range(X["noise"].shape[0]):
            s = ref_import.make_heun(ns)
            s.set_timesteps(18)
            z_N = X["noise"][b:b + 1] * s.init_noise_sigma
            z_in = s.scale_model_input(z_N, s.timesteps[0])
            lat = m(z_in, s.timesteps[0], guidance=4.0, encoder_hidden_states=X["enc"][b:b + 1],
                    encoder_attention_mask=X["mask"][b:b + 1]).sample
            mel = vae.decode_first_stage(lat.float())
            wav = vae.vocoder(mel.squeeze(1).permute(0, 2, 1)).squeeze(1).float()
            outs.append((lat[0].numpy(), mel[0].numpy(), wav[0].numpy()))
            print("clip %2d (%2d tokens): |latent| %.4f |mel| %.4f |wav| %.4f" % (
                b, int(X["lens"][b]), np.linalg.norm(outs[-1][0]), np.linalg.norm(outs[-1][1]),
                np.linalg.norm(outs[-1][2])), flush=True)
    return X, outs, sf


def write(X, outs, sf, name="pipeline_batch32"):
    lens = X["lens"].numpy()
    clips = cases.batch32_clips(lens)
    out = dict(lens=lens, enc_sum=np.float64(X["enc"].double().sum()), noise_sum=np.float64(X["noise"].double().sum()),
               clips=np.array(clips, dtype=np.int64), scale_factor=sf, wav_head_len=WAV_HEAD, wav_stride=WAV_STRIDE)
    for key, j in (("latent", 0), ("mel", 1)):
        out[key] = np.stack([outs[b][j] for b in clips]).astype(np.float16)
    out["wav_head"] = np.stack([outs[b][2][:WAV_HEAD] for b in clips]).astype(np.float16)
    out["wav_strided"] = np.stack([outs[b][2][::WAV_STRIDE] for b in clips]).astype(np.float16)
    for key, j in (("latent", 0), ("mel", 1), ("wav", 2)):
        flat = [outs[b][j].reshape(-1) for b in range(len(outs))]
        idx = cases.sample_index(flat[0].size)
        out[key + "_samples"] = np.stack([f[idx] for f in flat]).astype(np.float32)
        out[key + "_norm"] = np.array([np.linalg.norm(f.astype(np.float64)) for f in flat])
        out[key + "_absmax"] = np.array([float(np.abs(f).max()) for f in flat])
    wav_all = torch.from_numpy(np.stack([o[2] for o in outs]))
    hi, lo = wav_all.max(), wav_all.min()
    out.update(wav_max=float(hi), wav_min=float(lo), wav_centre=float((hi + lo) / 2))     # fp32, as vocoder_infer
    save(name, **out)
    return out


if __name__ == "__main__":
    torch.set_num_threads(os.cpu_count())
    write(*compute(ref_import.load()))
