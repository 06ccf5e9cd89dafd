"""One CLAP fine-tuning step with the VAE decoder frozen (AudioLCM, the perceptual leg of bench.py) beside the same step with
the decoder trained as well (AudioLCM_FTVAE), at bench.py's sizes: light U-Nets, full-width VAE decoder + HiFi-GAN,
HTSAT-base, batch 4, 10.24 s clips, random weights.  The set-up restates that leg's (bench.py, distill_leg(perceptual=True))
rather than calling it, so both models are built and timed by the same lines; bench.py's own figure is a different
process and is not the baseline here.  Eager `train_step` loops in one process on one box:
frozen / FTVAE / frozen again, `--warmup` steps then `--steps` timed ones each, ending in a device synchronise.

    python tools/ftvae_step_bench.py [--batch 4] [--steps 10] [--warmup 3] [--out profiles/ftvae_step.txt]
"""
import argparse
import os
import socket
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from consistencytta_amd import clap as clap_mod  # noqa: E402
from consistencytta_amd import modules, spec  # noqa: E402
from consistencytta_amd.models import AudioLCM, AudioLCM_FTVAE  # noqa: E402
from consistencytta_amd.optim import WarmupSchedule  # noqa: E402

DEV = "cuda:0"


def build(cls, B, L=77):
    vae = modules.AutoencoderKL(ddconfig=spec.VAE_DDCONFIG, embed_dim=8, scale_factor=0.9227914214134216)
    vae.to(DEV)
    vae.init_random_(seed=12)
    vae.eval().requires_grad_(False)
    clap = clap_mod.CLAP_Module(enable_fusion=False, amodel="HTSAT-base")
    clap.to(DEV)
    clap.model.init_random_(seed=13)
    m = cls(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
            unet_model_config_path="tango_diffusion_light.json", unet_config=spec.LIGHT_UNET_CONFIG, snr_gamma=5.0, use_edm=True,
            teacher_guidance_scale=-1, num_diffusion_steps=18, vae=vae, loss_type="clap", clap_module=clap, target_ema_decay=0.95,
            ema_decay=0.999)
    m.to(DEV)
    m.teacher_unet.init_random_(seed=10)
    m.student_unet.init_random_(seed=11)
    with torch.no_grad():
        for dst in (m.student_target_unet, m.student_ema_unet):
            for p, q in zip(dst.parameters(), m.student_unet.parameters()):
                p.copy_(q)
    m.train()
    opt = m.prepare_training(lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, broadcast=False)
    sched = WarmupSchedule(opt, "linear", num_warmup_steps=1000, num_training_steps=100000)
    g = torch.Generator(device="cpu").manual_seed(5)
    z0 = (torch.randn(B, 8, 256, 16, generator=g) * 0.9).to(DEV)
    enc = (torch.randn(B, L, 1024, generator=g) * 0.25).to(DEV)
    lens = torch.randint(6, L + 1, (B,), generator=g)
    mask = (torch.arange(L)[None, :] < lens[:, None]).to(DEV)
    unc, umask = torch.zeros_like(enc), torch.zeros_like(mask)
    umask[:, 0] = True
    P = {"embeds_cf": torch.cat([unc, enc]), "mask_cf": torch.cat([umask, mask]), "embeds": enc, "mask": mask}
    ids = torch.randint(4, 50000, (B, 77), generator=g)
    tl = torch.randint(5, 30, (B,), generator=g)
    tmask = (torch.arange(77)[None, :] < tl[:, None]).long()
    ids = torch.where(tmask == 1, ids, torch.ones_like(ids))
    P["clap_text_features"] = clap.model.get_text_embedding({"input_ids": ids.to(DEV), "attention_mask": tmask.to(DEV)})
    gt = (torch.rand(B, 160000, generator=g) * 2 - 1).to(DEV) * 0.3
    return m, opt, sched, z0, P, gt


def timed(cls, a):
    torch.cuda.reset_peak_memory_stats()
    m, opt, sched, z0, P, gt = build(cls, a.batch)
    torch.manual_seed(100)
    losses = [m.train_step(z0, P, opt, sched, gt_wav=gt) for _ in range(a.warmup)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses += [m.train_step(z0, P, opt, sched, gt_wav=gt) for _ in range(a.steps)]
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    assert all(v == v for v in losses), "NaN loss"
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    del m, opt
    torch.cuda.empty_cache()
    return dt * 1e3, peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ftvae_step_bench needs a GPU: nothing is measured without one")
    lines = ["# CLAP fine-tuning step, batch %d, eager train_step, %d timed steps after %d; box %s, %s"
             % (a.batch, a.steps, a.warmup, socket.gethostname(), torch.cuda.get_device_name(0)),
             "%-36s %12s %22s" % ("model", "ms / step", "torch GiB (no arenas)")]
    for name, cls in (("AudioLCM (decoder frozen)", AudioLCM), ("AudioLCM_FTVAE (decoder trained)", AudioLCM_FTVAE),
                      ("AudioLCM (decoder frozen), again", AudioLCM)):
        ms, peak = timed(cls, a)
        lines.append("%-36s %12.2f %22.2f" % (name, ms, peak))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
