"""Fixture pinning the distillation step at the REAL widths:
the reference's own `models.AudioLCM` at `configs/tango_diffusion_light.json` (559 M-parameter
U-Nets), B=2 latents of the real (8, 256, 16) shape, its internal random draws recorded, loss
AND the student's gradients from torch autograd (build container only, ≈3 min of CPU):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_distill_light.py
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_distill_light.py --batch 9 --text-len 32 \
        --tag distill_full --out distill_light_b9 --draw-seed 9 --bf16-samples

The full gradient is 2.2 GB, so the fixture keeps, for every parameter tensor of the student,
its L2 norm and a deterministic strided sample of up to 512 entries (`sample_index`): a
per-block relative L2 over the samples is an unbiased estimate of the block's relative L2.
Follows `models/audio_consistency_model.py:239-427` and `tools/train_utils.py:166`.

The default run (B = 2, L = 16) RECORDS the reference's own random draws (time indices, noise, guidance) and stores
them.  With `--draw-seed` the draws are INJECTED instead: `torch.randint`, `randn_like` and `rand` inside
`AudioLCM.forward` return `cases.distill_draws(B, seed)` (asserting the call shapes and ranges of
audio_consistency_model.py:284,312,326), which a test rebuilds from the seed; the fixture then keeps only the time
indices, the guidance scales and an fp64 checksum of the noise (at B = 9 the noise alone is 1.2 MB).  The injected
time indices include 0 (the `last_mask` branch, where `z_gaussian` replaces `z_noisy`, :315-317) and the largest one,
the guidance scales values near 0 and near 6.  With `--bf16-samples` the gradient samples are stored as bfloat16 bit
patterns (`grad_samples_bf16`, relative rounding <= 2^-9), which keeps the B = 9 file under 1 MiB.

Measured with 8 CPU threads: B = 2, L = 16 takes 223 s of CPU (78 s wall), peak RSS 14 GB; B = 9, L = 32 (configs[3]'s
per-GPU batch, the size of `_lcm_light(9, 32, "distill_full")` in test_train_gpu.py) 775 s of CPU (200 s wall), peak
RSS 24 GB.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import cases  # noqa: E402
from consistencytta_amd import spec  # noqa: E402
from make_golden_distill import load_reference_audiolcm  # noqa: E402

H, W = 256, 16


sample_index = cases.sample_index


def main(B=2, L=16, tag="distill_light", out_name="distill_light", draw_seed=None, bf16_samples=False):
    ns, AudioLCM, TU = load_reference_audiolcm()
    cfg = spec.LIGHT_UNET_CONFIG
    torch.manual_seed(0)
    model = AudioLCM(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                     unet_model_config_path=ns.light_config_path, snr_gamma=5.0, use_edm=True,
                     teacher_guidance_scale=-1, num_diffusion_steps=18, vae=torch.nn.Identity(), loss_type="mse",
                     target_ema_decay=0.95, ema_decay=0.999)
    model.teacher_unet.load_state_dict(cases.unet_weights(cfg, False, 0))
    model.student_unet.load_state_dict(cases.unet_weights(cfg, True, 1))
    model.student_target_unet.load_state_dict(cases.unet_weights(cfg, True, 2))
    model.student_ema_unet.load_state_dict(cases.unet_weights(cfg, True, 3))
    P = cases.prompt_states(cfg, B, L, tag)
    model.get_prompt_embeds = lambda prompt, use_cf, num_samples_per_prompt=1: (
        P["embeds_cf"], P["mask_cf"], P["embeds"], P["mask"])
    model.encode_text_classifier_free = lambda prompt, n: (P["embeds_cf"], P["mask_cf"], P["embeds"], P["mask"])
    z0 = cases.t(spec.det_uniform(tag + ".z0", (B, 8, H, W), 14)) * 0.9

    rec = {}
    o_randint, o_randn_like, o_rand = torch.randint, torch.randn_like, torch.rand

    if draw_seed is None:
        def randint(*a, **k):
            v = o_randint(*a, **k)
            rec.setdefault("randint", v.clone())
            return v

        def randn_like(x, *a, **k):
            v = o_randn_like(x, *a, **k)
            rec.setdefault("randn_like", v.clone())
            return v

        def rand(*a, **k):
            v = o_rand(*a, **k)
            rec.setdefault("rand", v.clone())
            return v
    else:
        assert model.max_rand_guidance_scale == 6
        ti, noise, u = cases.distill_draws(B, draw_seed)
        n_steps = (len(model.noise_scheduler.timesteps) - 1) // 2

        def randint(low, high, size, **k):          # get_random_timestep (:284): randint(0, 17, (B,)) * 2
            assert (low, high, tuple(size)) == (0, n_steps, (B,)) and "randint" not in rec, (low, high, size)
            rec["randint"] = ti.clone()
            return ti.clone().to(k.get("device", "cpu"))

        def randn_like(x, *a, **k):                 # gaussian_noise (:312)
            assert tuple(x.shape) == (B, 8, H, W) and x.dtype == torch.float32 and "randn_like" not in rec
            rec["randn_like"] = noise.clone()
            return noise.clone().to(x.device)

        def rand(*a, **k):                          # random guidance scale (:326): rand(B) * 6
            assert a == (B,) and not k and "rand" not in rec, (a, k)
            rec["rand"] = u.clone()
            return u.clone()

    model.train()
    torch.manual_seed(4321)
    torch.randint, torch.randn_like, torch.rand = randint, randn_like, rand
    try:
        loss = model(z0, None, ["a"] * B)
    finally:
        torch.randint, torch.randn_like, torch.rand = o_randint, o_randn_like, o_rand
    assert sorted(rec) == ["rand", "randint", "randn_like"], sorted(rec)
    loss.backward()          # accelerator.backward(loss) on one process (tools/train_utils.py:166)

    out = dict(train_loss=np.float64(float(loss)), time_inds=rec["randint"].numpy(),
               noise=rec["randn_like"].numpy(), guidance=rec["rand"].numpy() * 6)
    if draw_seed is not None:
        out["draw_seed"] = np.int64(draw_seed)
        out["noise_sum"] = np.float64(rec["randn_like"].double().sum())
        del out["noise"]
    names, norms, samples, offsets = [], [], [], [0]
    for k, p in model.student_unet.named_parameters():
        if p.grad is None:
            assert not p.requires_grad, k
            continue
        g = p.grad.detach().reshape(-1)
        names.append(k)
        norms.append(float(g.double().norm()))
        samples.append(g[torch.from_numpy(sample_index(g.numel()))].numpy())
        offsets.append(offsets[-1] + samples[-1].size)
    out["grad_names"] = np.array(names)
    out["grad_norms"] = np.array(norms, dtype=np.float64)
    samples = np.concatenate(samples).astype(np.float32)
    if bf16_samples:
        out["grad_samples_bf16"] = torch.from_numpy(samples).to(torch.bfloat16).view(torch.int16).numpy()
    else:
        out["grad_samples"] = samples
    out["grad_offsets"] = np.array(offsets, dtype=np.int64)
    for p in model.teacher_unet.parameters():
        assert p.grad is None
    path = os.path.join(HERE, out_name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB; loss", float(loss), "tensors", len(names),
          "time_inds", out["time_inds"], "guidance", out["guidance"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--text-len", type=int, default=16)
    ap.add_argument("--tag", default="distill_light", help="name prefix of the seeded prompt states and latents")
    ap.add_argument("--out", default="distill_light", help="fixture name (written as tests/golden/<out>.npz)")
    ap.add_argument("--draw-seed", type=int, default=None, help="inject cases.distill_draws(B, seed) instead of recording")
    ap.add_argument("--bf16-samples", action="store_true", help="store the gradient samples as bfloat16 bit patterns")
    a = ap.parse_args()
    torch.set_num_threads(os.cpu_count())
    main(a.batch, a.text_len, a.tag, a.out, a.draw_seed, a.bf16_samples)
