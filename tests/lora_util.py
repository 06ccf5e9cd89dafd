"""What the LoRA GPU tests share: the fixture's models, rebuilt from `cases` / `lora_cases`, and the gradient comparison."""
import torch

import cases
import lora_cases as LC
from consistencytta_amd import modules, spec
from gpu_util import DEV


def unet(cfg, adapters=True, zero_up=False):
    """the fixture's student: base weights of seed 1, adapters of `lora_cases.lora_weights` (`zero_up`: every up = 0)"""
    m = modules.UNet2DConditionGuidedModel.from_config(cfg)
    m.load_state_dict(cases.unet_weights(cfg, True, 1))
    if adapters:
        m.enable_lora_(LC.RANK)
        ad = LC.lora_weights(cfg)
        if zero_up:
            ad = {k: (torch.zeros_like(v) if k.endswith("up.weight") else v) for k, v in ad.items()}
        info = m.load_state_dict(ad, strict=False)
        assert not info.unexpected_keys
    return m.to(DEV).eval()


def unet_inputs(cfg):
    x, ts, gs, enc, mask = cases.unet_inputs(cfg, LC.B, LC.H, LC.W, LC.L, "lora")
    return dict(sample=x.to(DEV), timestep=ts.to(DEV), guidance=gs.to(DEV), encoder_hidden_states=enc.to(DEV),
                encoder_attention_mask=mask.to(DEV))


def gdm():
    """the fixture's AudioGDM(use_lora=True): teacher seed 0, student seed 1 + adapters, EMA student = a copy"""
    from consistencytta_amd.models import AudioGDM
    cfg = LC.LORA_TINY_LIGHT
    m = AudioGDM(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                 unet_model_config_path="tiny_light.json", unet_config=cfg, snr_gamma=5.0, teacher_guidance_scale=-1,
                 ema_decay=0.999, use_lora=True)
    m.teacher_unet.load_state_dict(cases.unet_weights(cfg, False, 0))
    m.student_unet.load_state_dict(cases.unet_weights(cfg, True, 1))
    m.setup_lora()
    m.student_unet.load_state_dict(LC.lora_weights(cfg), strict=False)
    m._rebuild_ema_student()
    m.to(DEV)
    P = {k: v.to(DEV) for k, v in cases.prompt_states(cfg, LC.B, LC.L, "distill").items()}
    z0 = (cases.t(spec.det_uniform("distill.z0", (LC.B, 8, LC.H, LC.W), 14)) * 0.9).to(DEV)
    return m, P, z0


def draws(g):
    return dict(time_inds=torch.from_numpy(g["time_inds"]), gaussian_noise=torch.from_numpy(g["noise"]).to(DEV),
                guidance_scale=torch.from_numpy(g["guidance"]))


def adapter_grad_error(net, g, tag):
    """pooled rel-L2 of every adapter gradient vs the fixture; prints it, and the worst tensors one by one"""
    num = den = 0.0
    per = []
    n = 0
    for k, p in net.named_parameters():
        if "_lora." not in k:
            continue
        ref = torch.from_numpy(g["grad." + k]).double()
        got = p.grad.detach().cpu().double()
        assert bool(torch.isfinite(got).all()), k
        e, r = float((got - ref).norm()), float(ref.norm())
        num += e * e
        den += r * r
        per.append((e / max(r, 1e-30), e, r, k))
        n += 1
    assert n == 256
    rel = (num / den) ** 0.5
    print("%s: adapter gradients vs the reference, pooled rel_l2 %.3e over %d tensors" % (tag, rel, n))
    for v, e, r, k in sorted(per, reverse=True)[:5]:
        print("    rel_l2 %.3e (|err| %.3e, |ref| %.3e)  %s" % (v, e, r, k))
    return rel
