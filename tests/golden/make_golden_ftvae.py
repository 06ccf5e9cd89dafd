"""Fixture for the VAE fine-tuning stage (models/audio_consistency_model_ftvae.py), from the REFERENCE's own modules
(build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ftvae.py

tests/golden/ftvae_tiny.npz holds
  * the reference AutoencoderKL's decoder.* / post_quant_conv.* gradients (torch autograd through
    `decode_first_stage(z, allow_grad=True)` with those parameters requiring grad) of loss = (mel * direction).sum() for the
    tiny decoder, z = cases.vae_inputs(2, 16, 16, "vae_grad"), scale_factor 0.9: tensors of up to WHOLE elements whole, larger
    ones as their L2 norm plus a strided sample of WHOLE entries (cases.sample_index);
  * the key list (and shapes) of the reference `AudioLCM_FTVAE.state_dict()` for the tiny U-Nets and that VAE;
  * what the reference's `load_pretrained` leaves in every parameter after loading `synthetic_checkpoint(keys, shapes)`:
    every tensor filled with a number derived from its key (`key_code`), the `loss.vae.*` duplicates first and different
    from their `vae.*` twins, and the `vae.*` twins named in LONE removed so that only the duplicate can fill them; NaN
    stands for "not loaded: left as constructed" (the VAE's encoder and vocoder).

What is the reference's code and what is a stand-in: AudioLCM_FTVAE, AudioLCM, AutoencoderKL and the U-Nets are the
reference's; FLAN-T5 and the scheduler download are stubbed as in make_golden_distill.py; `tools.losses.CLAPLoss` is replaced
by its own constructor without the two lines that build `laion_clap.CLAP_Module` and load its checkpoint
(tools/losses.py:270-273), so the key list has the `loss.vae.*` entries and no `loss.clap.*` ones.
"""
import json
import os
import sys
import tempfile
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import cases  # noqa: E402
from consistencytta_amd import spec  # noqa: E402

WHOLE = 1024
SCALE = 0.9
DEC = ("decoder.", "post_quant_conv.")
LONE = ("vae.decoder.conv_out.bias", "vae.post_quant_conv.weight", "vae.decoder.mid.attn_1.q.weight")


def key_code(key):
    """The number a synthetic checkpoint holds in every element of tensor `key` (exact in fp32, never 0)."""
    return float(zlib.crc32(key.encode()) % 65521 + 1)


def synthetic_checkpoint(keys, shapes):
    """{key: constant tensor}: `loss.*` entries first (the reference's loop must not depend on the order), without LONE."""
    order = sorted((k for k in keys if k not in LONE), key=lambda k: not k.startswith("loss."))
    shape = dict(zip(keys, shapes))
    return {k: torch.full(tuple(int(d) for d in shape[k] if d > 0), key_code(k)) for k in order}


def pack_shapes(tensors):
    out = np.zeros((len(tensors), 4), dtype=np.int64)
    for i, t in enumerate(tensors):
        out[i, :t.ndim] = tuple(t.shape)
    return out


def main():
    import make_golden
    from make_golden_distill import load_reference_audiolcm
    ns, AudioLCM, TU = load_reference_audiolcm()

    # ---- 1. decoder / post_quant_conv gradients of the reference VAE
    vae, _ = make_golden.ref_vae(ns, cases.TINY_VAE_DD, cases.TINY_HIFIGAN)
    vae.scale_factor = SCALE
    vae.decoder.requires_grad_(True)
    vae.post_quant_conv.requires_grad_(True)
    z = cases.vae_inputs(2, 16, 16, "vae_grad")
    mel = vae.decode_first_stage(z, allow_grad=True)
    direction = cases.t(spec.det_uniform("vae_grad.dir", tuple(mel.shape), 9))
    (mel * direction).sum().backward()
    out = dict(mel=mel.detach().numpy(), scale_factor=np.float64(SCALE), whole=np.int64(WHOLE))
    names, norms, samples, offsets = [], [], [], [0]
    for k, p in vae.named_parameters():
        if not k.startswith(DEC):
            assert p.grad is None, k
            continue
        g = p.grad.detach().reshape(-1)
        names.append(k)
        norms.append(float(g.double().norm()))
        samples.append((g if g.numel() <= WHOLE else g[torch.from_numpy(cases.sample_index(g.numel(), WHOLE))]).numpy())
        offsets.append(offsets[-1] + samples[-1].size)
    assert names == list(spec.vae_decoder_param_spec(cases.TINY_VAE_DD).keys())
    out.update(grad_names=np.array(names), grad_norms=np.array(norms, dtype=np.float64),
               grad_samples=np.concatenate(samples).astype(np.float32), grad_offsets=np.array(offsets, dtype=np.int64))
    vae.requires_grad_(False)
    vae.zero_grad(set_to_none=True)

    # ---- 2. the reference AudioLCM_FTVAE: state-dict keys, load_pretrained
    import models.audio_consistency_model as RM

    class ClapLossNoTower(torch.nn.Module):      # tools/losses.py:260-276 without :270-273
        def __init__(self, vae, reduction="instance", mse_weight=1., clap_weight=1.):
            super().__init__()
            self.vae, self.reduction, self.sr = vae, reduction, 16000
            self.mse_weight, self.clap_weight = mse_weight, clap_weight
    RM.CLAPLoss = ClapLossNoTower
    from models.audio_consistency_model_ftvae import AudioLCM_FTVAE
    full = dict(json.load(open(ns.light_config_path)))
    full.update(cases.TINY_UNET)
    tmp = os.path.join(tempfile.mkdtemp(), "tiny_light.json")
    json.dump(full, open(tmp, "w"))

    torch.manual_seed(0)
    model = AudioLCM_FTVAE(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                           unet_model_config_path=tmp, snr_gamma=5.0, use_edm=True, teacher_guidance_scale=-1,
                           num_diffusion_steps=18, vae=vae, loss_type="clap", target_ema_decay=0.95, ema_decay=0.999)
    sd = model.state_dict()
    keys = list(sd.keys())
    assert any(k.startswith("loss.vae.decoder.") for k in keys) and any(k.startswith("vae.ema_decoder.") for k in keys)
    shapes = pack_shapes(list(sd.values()))
    out.update(keys=np.array(keys), shapes=shapes)
    ckpt = synthetic_checkpoint(keys, shapes)
    assert all(("loss." + k) in ckpt and k not in ckpt for k in LONE)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    model.load_pretrained(ckpt)
    loaded_names, loaded_codes = [], []
    for k, p in model.named_parameters():          # every parameter once, under its first name
        p = p.detach()
        const = float(p.min()) == float(p.max())
        assert const or torch.equal(p, before[k]), k          # loaded from the checkpoint, or left as constructed
        loaded_names.append(k)
        loaded_codes.append(float(p.reshape(-1)[0]) if const and not torch.equal(p, before[k]) else float("nan"))
    out.update(loaded_names=np.array(loaded_names), loaded_codes=np.array(loaded_codes, dtype=np.float64))
    path = os.path.join(HERE, "ftvae_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB;", len(names), "gradient tensors,", len(keys), "keys,",
          len(loaded_names), "parameters after load_pretrained")


if __name__ == "__main__":
    main()
