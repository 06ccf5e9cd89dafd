"""What LoRA adapters cost and save at the project's sizes (light U-Net, latent 256 x 16), measured in ONE process on one
box, every variant built and timed by the same lines and the plain path timed again at the end (drift of the box):

  forward  the inference forward at batch 32: plain U-Net / with rank-4 adapters / after merge_lora_() / plain again
  step     the stage-1 `AudioGDM.train_step` at batch 9: full fine-tuning / LoRA / full fine-tuning again

Times are hipEvent brackets around `--steps` calls after `--warmup` calls of the same shapes; random weights.

    python tools/lora_bench.py [--steps 10] [--warmup 3] [--out profiles/lora_step.txt]
"""
import argparse
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from consistencytta_amd import modules, spec  # noqa: E402
from consistencytta_amd.models import AudioGDM  # noqa: E402

DEV = "cuda:0"
CFG = spec.LIGHT_UNET_CONFIG


def event_ms(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def texts(B, L, g):
    enc = (torch.randn(B, L, CFG["cross_attention_dim"], generator=g) * 0.25).to(DEV)
    lens = torch.randint(6, L + 1, (B,), generator=g)
    return enc, (torch.arange(L)[None, :] < lens[:, None]).to(DEV)


def randomise_up_(net, g):
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.endswith("_lora.up.weight"):
                p.copy_((torch.randn(p.shape, generator=g) * 0.02).to(DEV))


def forward_rows(a):
    B, L = a.forward_batch, 32
    g = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn(B, 8, 256, 16, generator=g).to(DEV)
    t = (torch.rand(B, generator=g) * 999).to(DEV)
    w = (torch.rand(B, generator=g) * 6).to(DEV)
    enc, mask = texts(B, L, g)
    net = modules.UNet2DConditionGuidedModel.from_config(CFG).to(DEV)
    net.init_random_(seed=11)
    net.eval().requires_grad_(False)

    def run():
        # reuse_text=False: every call projects the text states, adapters included
        return net(x, t, guidance=w, encoder_hidden_states=enc, encoder_attention_mask=mask, reuse_text=False).sample

    rows = [("plain U-Net", event_ms(run, a.warmup, a.steps))]
    net.enable_lora_(4)
    randomise_up_(net, g)
    rows.append(("rank-4 adapters", event_ms(run, a.warmup, a.steps)))
    net.merge_lora_()
    rows.append(("after merge_lora_()", event_ms(run, a.warmup, a.steps)))
    rows.append(("after merge_lora_(), again", event_ms(run, a.warmup, a.steps)))
    del net
    torch.cuda.empty_cache()
    return rows


def step_ms(a, lora):
    B, L = a.step_batch, 32
    g = torch.Generator(device="cpu").manual_seed(5)
    m = AudioGDM(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                 unet_model_config_path="tango_diffusion_light.json", unet_config=CFG, snr_gamma=5.0, teacher_guidance_scale=-1,
                 ema_decay=0.999, use_lora=lora)
    m.to(DEV)
    m.teacher_unet.init_random_(seed=10)
    m.student_unet.init_random_(seed=11)
    if lora:
        m.setup_lora()
        randomise_up_(m.student_unet, g)
    m._rebuild_ema_student()
    m.train()
    opt = m.prepare_training(lr=1e-5, weight_decay=1e-2, broadcast=False)
    z0 = (torch.randn(B, 8, 256, 16, generator=g) * 0.9).to(DEV)
    enc, mask = texts(B, L, g)
    unc, umask = torch.zeros_like(enc), torch.zeros_like(mask)
    umask[:, 0] = True
    P = {"embeds_cf": torch.cat([unc, enc]), "mask_cf": torch.cat([umask, mask]), "embeds": enc, "mask": mask}
    torch.manual_seed(100)
    losses = []
    ms = event_ms(lambda: losses.append(m.train_step(z0, P, opt, None)), a.warmup, a.steps)
    assert all(v == v for v in losses), "NaN loss"
    n_train, n_all = opt.n, opt.flat.numel()
    del m, opt
    torch.cuda.empty_cache()
    return ms, n_train, n_all


def kernel_rows(a, m, k=256, r=4):
    """the adapter kernels alone at the level-0 shape of the light U-Net (width 256, m = batch x 4096 tokens), with the
    bytes each has to move and the rate that makes"""
    from consistencytta_amd import _native as N
    L = N.lib()
    g = torch.Generator(device="cpu").manual_seed(9)
    x = torch.randn(m, k, generator=g).to(torch.bfloat16).to(DEV)
    y = torch.randn(m, k, generator=g).to(torch.bfloat16).to(DEV)
    wa = (torch.randn(r, k, generator=g) * 0.25).to(DEV)
    wb = (torch.randn(k, r, generator=g) * 0.02).to(DEV)
    d = torch.empty(m, r, device=DEV)
    grad = torch.zeros(r, k, device=DEV)
    scratch = torch.empty(L.ctta_lora_wgrad_scratch_floats(m, k, r), device=DEV)
    s = N.stream_ptr()
    calls = (("ctta_lora_down", m * k * 2 + m * r * 4,
              lambda: N.check(L.ctta_lora_down(N.ptr(x), k, m, k, N.ptr(wa), 0, r, N.ptr(d), s))),
             ("ctta_lora_up_add", 2 * m * k * 2 + m * r * 4,
              lambda: N.check(L.ctta_lora_up_add(N.ptr(y), k, m, k, N.ptr(d), N.ptr(wb), 0, r, 1.0, s))),
             ("ctta_lora_wgrad (2 launches)", m * k * 2 + m * r * 4,
              lambda: N.check(L.ctta_lora_wgrad(N.ptr(d), N.ptr(x), k, m, k, r, 1.0, N.ptr(grad), k, 1, None, N.ptr(scratch), s))))
    return [(name, event_ms(fn, a.warmup, 5 * a.steps) * 1e3, nbytes) for name, nbytes, fn in calls]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forward-batch", type=int, default=32)
    ap.add_argument("--step-batch", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_bench needs a GPU: nothing is measured without one")
    lines = ["# LoRA on the light U-Net, %d timed calls after %d, hipEvent brackets; box %s, %s"
             % (a.steps, a.warmup, socket.gethostname(), torch.cuda.get_device_name(0)),
             "# inference forward, batch %d, latent 256 x 16, 32 text states" % a.forward_batch,
             "%-36s %12s" % ("variant", "ms / call")]
    for name, ms in forward_rows(a):
        lines.append("%-36s %12.3f" % (name, ms))
        print(lines[-1], flush=True)
    lines += ["# stage-1 train_step (AudioGDM, eager, one process), batch %d" % a.step_batch,
              "%-36s %12s %16s" % ("variant", "ms / step", "trained / all")]
    for name, lora in (("full fine-tuning", False), ("LoRA rank 4", True), ("full fine-tuning, again", False)):
        ms, n_train, n_all = step_ms(a, lora)
        lines.append("%-36s %12.2f %16s" % (name, ms, "%d / %d" % (n_train, n_all)))
        print(lines[-1], flush=True)
    for batch in (a.step_batch, a.forward_batch):
        lines += ["# adapter kernels alone, %d rows (batch %d x 4096 tokens) x 256 columns, rank 4" % (batch * 4096, batch),
                  "%-36s %12s %12s" % ("kernel", "us / call", "GB/s")]
        for name, us, nbytes in kernel_rows(a, batch * 4096):
            lines.append("%-36s %12.1f %12.0f" % (name, us, nbytes / us * 1e-3))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
