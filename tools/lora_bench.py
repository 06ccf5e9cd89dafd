"""What LoRA adapters cost and save at the project's sizes (light U-Net, latent 256 x 16), measured in ONE process on one
box, every variant built and timed by the same lines; each adapter line runs as off / on / off with `lora_fused`, and the
plain path is timed again at the end, so the drift of the box is visible:

  forward  the inference forward at batch 32: plain U-Net / rank-4 adapters, per-site launches / fused site kernels /
           per-site launches again / after merge_lora_()
  step     the stage-1 `AudioGDM.train_step` at batch 9: full fine-tuning / LoRA with per-site launches and a full re-pack
           of the handle after every optimizer step (what the code did before the adapter-only reload) / LoRA with the
           fused kernels and the adapter-only reload / the first again / full fine-tuning again; and the two reloads alone
  kernels  ctta_lora_sites_fwd / _bwd for the q / k / v group against the launches they replace, with the bytes each must
           move and the floor those bytes make at the box's streaming rate (tools/stream_bench.py's EMA pass)

Times are hipEvent brackets around `--steps` calls after `--warmup` calls of the same shapes; random weights.

    python tools/lora_bench.py [--steps 10] [--warmup 3] [--out profiles/lora_step.txt]     (--out appends a dated section)
"""
import argparse
import datetime
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
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
    for name, fused in (("rank-4 adapters, per-site launches", False), ("rank-4 adapters, fused site kernels", True),
                        ("rank-4 adapters, per-site launches, again", False)):
        net.lora_fused = 3 if fused else False        # 3: the forward groups too (the default fuses the backward alone)
        rows.append((name, event_ms(run, a.warmup, a.steps)))
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
    n_train, n_all = opt.n, opt.flat.numel()
    stu = m.student_unet
    rows = []
    if not lora:
        rows.append(("", event_ms(lambda: losses.append(m.train_step(z0, P, opt, None)), a.warmup, a.steps)))
    else:
        def step(full_reload):
            losses.append(m.train_step(z0, P, opt, None))
            if full_reload:                        # a base change: the next call re-packs all 560 M parameters
                stu.mark_weights_changed()
        for name, fused in ((", per-site launches + full reload", False), (", fused backward + adapter reload", True),
                            (", fused forward and backward + adapter reload", 3),
                            (", per-site launches + full reload, again", False)):
            stu.lora_fused = fused
            rows.append((name, event_ms(lambda: step(not fused), a.warmup, a.steps)))
        # the two reloads alone, on the student's handle
        from consistencytta_amd import _native as N
        L = N.lib()
        full, keep1 = N.tensor_table(stu._table())
        ad, keep2 = N.tensor_table({k: v for k, v in stu._table().items() if "_lora." in k})
        rows.append((": ctta_unet_load_weights alone", event_ms(
            lambda: N.check(L.ctta_unet_load_weights(stu._h_unet, full, len(full), N.stream_ptr())), a.warmup, a.steps)))
        rows.append((": ctta_unet_load_adapters alone", event_ms(
            lambda: N.check(L.ctta_unet_load_adapters(stu._h_unet, ad, len(ad), N.stream_ptr())), a.warmup, a.steps)))
    assert all(v == v for v in losses), "NaN loss"
    del m, opt
    torch.cuda.empty_cache()
    return rows, n_train, n_all


def stream_rate():
    """bytes / us of the two-shadow EMA pass (tools/stream_bench.py: 20 B per element) at 64 M elements"""
    from consistencytta_amd import _native as N
    from stream_bench import timed
    L = N.lib()
    n = 64 * 1024 * 1024
    p, sa, sb = (torch.randn(n, device=DEV) * 0.02 for _ in range(3))
    fn = lambda: N.check(L.ctta_ema_update2(N.ptr(p), N.ptr(sa), 0.95, N.ptr(sb), 0.999, n, N.stream_ptr()))  # noqa: E731
    fn()
    torch.cuda.synchronize()
    return 20.0 * n / (timed(fn) * 1e3)


def kernel_rows(a, m, k=256, r=4):
    """the q / k / v group at the level-0 shape of the light U-Net (width 256, m = batch x 4096 tokens): the fused calls
    against the per-site launches they replace, with the bytes each must move"""
    from consistencytta_amd import _native as N
    L = N.lib()
    g = torch.Generator(device="cpu").manual_seed(9)
    s = N.stream_ptr()
    x = torch.randn(m, k, generator=g).to(torch.bfloat16).to(DEV)
    ys = [torch.randn(m, k, generator=g).to(torch.bfloat16).to(DEV) for _ in range(3)]      # Y forward, dY backward
    dx = torch.randn(m, k, generator=g).to(torch.bfloat16).to(DEV)
    wa = [(torch.randn(r, k, generator=g) * 0.25).to(DEV) for _ in range(3)]
    wb = [(torch.randn(k, r, generator=g) * 0.02).to(DEV) for _ in range(3)]
    d = [torch.randn(m, r, generator=g).to(DEV) for _ in range(3)]
    dd = [torch.empty(m, r, device=DEV) for _ in range(3)]
    ga = [torch.zeros(r, k, device=DEV) for _ in range(3)]
    gb = [torch.zeros(k, r, device=DEV) for _ in range(3)]
    part = torch.empty(L.ctta_lora_wgrad_scratch_floats(m, k, r), device=DEV)
    scratch = torch.empty(L.ctta_lora_sites_bwd_scratch_floats(m, k, k, 3, r), device=DEV)
    fs = (N.LoraFwdSite * 3)()
    bs = (N.LoraBwdSite * 3)()
    for i in range(3):
        fs[i].a, fs[i].b, fs[i].y, fs[i].d, fs[i].ldy, fs[i].n_pad = N.ptr(wa[i]), N.ptr(wb[i]), N.ptr(ys[i]), N.ptr(d[i]), k, k
        bs[i].dy, bs[i].a, bs[i].b, bs[i].d, bs[i].ga, bs[i].gb = (N.ptr(t) for t in (ys[i], wa[i], wb[i], d[i], ga[i], gb[i]))
        bs[i].ga_stride_r, bs[i].ga_stride_k, bs[i].gb_stride_r, bs[i].gb_stride_k, bs[i].lddy, bs[i].n_pad = k, 1, 1, r, k, k

    def fwd_unfused():
        for i in range(3):
            N.check(L.ctta_lora_down(N.ptr(x), k, m, k, N.ptr(wa[i]), 0, r, N.ptr(d[i]), s))
            N.check(L.ctta_lora_up_add(N.ptr(ys[i]), k, m, k, N.ptr(d[i]), N.ptr(wb[i]), 0, r, 1.0, s))

    def bwd_unfused():
        for i in range(3):
            N.check(L.ctta_lora_down(N.ptr(ys[i]), k, m, k, N.ptr(wb[i]), 1, r, N.ptr(dd[i]), s))
            N.check(L.ctta_lora_wgrad(N.ptr(d[i]), N.ptr(ys[i]), k, m, k, r, 1.0, N.ptr(gb[i]), 1, r, None, N.ptr(part), s))
            N.check(L.ctta_lora_wgrad(N.ptr(dd[i]), N.ptr(x), k, m, k, r, 1.0, N.ptr(ga[i]), k, 1, None, N.ptr(part), s))
            N.check(L.ctta_lora_up_add(N.ptr(dx), k, m, k, N.ptr(dd[i]), N.ptr(wa[i]), 1, r, 1.0, s))

    act = m * k * 2
    calls = (("forward: 3 x (down + up_add)", fwd_unfused, 3 * act + 6 * act),
             ("forward: ctta_lora_sites_fwd", lambda: N.check(L.ctta_lora_sites_fwd(N.ptr(x), k, m, k, r, 1.0, fs, 3, s)), act + 6 * act),
             ("forward: 3 x (down + up_add), again", fwd_unfused, 3 * act + 6 * act),
             ("backward: 3 x (down + 2 wgrad + up_add)", bwd_unfused, 3 * (2 * act + act + 2 * act)),
             ("backward: ctta_lora_sites_bwd", lambda: N.check(L.ctta_lora_sites_bwd(
                 N.ptr(x), k, N.ptr(dx), k, m, k, r, 1.0, bs, 3, N.ptr(scratch), s)), 3 * act + act + 2 * act),
             ("backward: 3 x (down + 2 wgrad + up_add), again", bwd_unfused, 3 * (2 * act + act + 2 * act)))
    return [(name, event_ms(fn, a.warmup, 5 * a.steps) * 1e3, nbytes) for name, fn, nbytes in calls]


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
    lines = ["# %s: LoRA on the light U-Net, %d timed calls after %d, hipEvent brackets; box %s, %s"
             % (datetime.date.today().isoformat(), a.steps, a.warmup, socket.gethostname(), torch.cuda.get_device_name(0)),
             "# inference forward, batch %d, latent 256 x 16, 32 text states" % a.forward_batch,
             "%-52s %12s" % ("variant", "ms / call")]
    for name, ms in forward_rows(a):
        lines.append("%-52s %12.3f" % (name, ms))
        print(lines[-1], flush=True)
    lines += ["# stage-1 train_step (AudioGDM, eager, one process), batch %d" % a.step_batch,
              "%-52s %12s %16s" % ("variant", "ms / step", "trained / all")]
    for name, lora in (("full fine-tuning", False), ("LoRA rank 4", True), ("full fine-tuning, again", False)):
        rows, n_train, n_all = step_ms(a, lora)
        for tail, ms in rows:
            lines.append("%-52s %12.2f %16s" % (name + tail, ms, "%d / %d" % (n_train, n_all)))
            print(lines[-1], flush=True)
    rate = stream_rate()
    lines.append("# streaming rate of this box (two-shadow EMA pass, 64 M elements): %.0f GB/s" % (rate * 1e-3))
    for batch in (a.step_batch, a.forward_batch):
        lines += ["# the q / k / v group alone, %d rows (batch %d x 4096 tokens) x 256 columns, rank 4" % (batch * 4096, batch),
                  "%-52s %12s %12s %12s" % ("launches", "us / call", "GB/s", "floor us")]
        for name, us, nbytes in kernel_rows(a, batch * 4096):
            lines.append("%-52s %12.1f %12.0f %12.1f" % (name, us, nbytes / us * 1e-3, nbytes / rate))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
