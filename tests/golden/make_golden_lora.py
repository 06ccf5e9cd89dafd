"""Fixture for LoRA on stage 1, produced by the REFERENCE's own `models.AudioGDM(use_lora=True)` -> `setup_lora()` ->
diffusers `LoRAAttnProcessor` (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lora.py

Writes lora_gdm_tiny.npz.  Weights, adapter values and inputs are functions of (name, shape, seed) (`cases`, `lora_cases`)
and are not stored; the file holds what the reference computed from them:
  keys                      the student's state-dict keys after setup_lora(), in order
  unet_out                  UNet2DConditionGuidedModel + adapters on fixed inputs (light-style config)
  unet_out_full             the same for the config whose inner width equals the channel count (file name without "light")
  adapter_effect            rel-L2 between unet_out and the output with every `up` zeroed (asserted >= 4 x 2.5e-2, so
                            that a path which ignores the adapters cannot pass the forward bound)
  loss, time_inds, noise, guidance      AudioGDM.forward on the recorded draws
  grad.<key>                d loss / d <adapter tensor>, all 256 of them
  inference_4steps          4-step DDIM inference(use_ema=True)
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import cases  # noqa: E402
import lora_cases as LC  # noqa: E402
import make_golden_distill as mgd  # noqa: E402
import make_golden_gdm as mgg  # noqa: E402
from consistencytta_amd import spec  # noqa: E402


def build(AudioGDM, ns, cfg, file_name):
    full = dict(json.load(open(ns.light_config_path)))
    full.update(cfg)
    tmp = os.path.join(tempfile.mkdtemp(), file_name)
    json.dump(full, open(tmp, "w"))
    torch.manual_seed(0)
    model = AudioGDM(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                     unet_model_config_path=tmp, snr_gamma=5.0, teacher_guidance_scale=-1, ema_decay=0.999, use_lora=True)
    # the order of load_state_dict_from_tango (audio_guided_model.py:53-85): base weights, setup_lora(), then the EMA
    # student rebuilt as a copy.  The guided student has keys the teacher lacks, so the networks are loaded one by one.
    model.teacher_unet.load_state_dict(cases.unet_weights(cfg, False, 0))
    model.student_unet.load_state_dict(cases.unet_weights(cfg, True, 1))
    model.setup_lora()
    info = model.student_unet.load_state_dict(LC.lora_weights(cfg), strict=False)
    assert not info.unexpected_keys and all("_lora." not in k for k in info.missing_keys), info
    from copy import deepcopy
    model.student_ema_unet = deepcopy(model.student_unet)
    model.student_ema_unet.requires_grad_(False)
    return model


def unet_out(unet, cfg):
    x, ts, gs, enc, mask = cases.unet_inputs(cfg, LC.B, LC.H, LC.W, LC.L, "lora")
    with torch.no_grad():
        return unet(x, ts, guidance=gs, encoder_hidden_states=enc, encoder_attention_mask=mask).sample


def main():
    DDPM, DDIM, D = mgg.load_reference_schedulers()
    ns, _, _ = mgd.load_reference_audiolcm()
    D.DDPMScheduler, D.DDIMScheduler = DDPM, DDIM
    DDPM.from_pretrained = classmethod(lambda cls, *a, **k: DDPM(**mgg.SD21))
    sys.modules.pop("models.audio_guided_model", None)
    from models.audio_guided_model import AudioGDM
    out = {}

    # ---- forward-only case: inner width == channel count
    cfg_f = LC.LORA_TINY_FULL
    m_f = build(AudioGDM, ns, cfg_f, "tiny_full.json")
    assert not m_f.lightweight
    out["unet_out_full"] = unet_out(m_f.student_unet, cfg_f).numpy()

    # ---- light-style case
    cfg = LC.LORA_TINY_LIGHT
    model = build(AudioGDM, ns, cfg, "tiny_light.json")
    assert model.lightweight
    keys = list(model.student_unet.state_dict().keys())
    assert list(model.student_ema_unet.state_dict().keys()) == keys
    trainable = [k for k, p in model.student_unet.named_parameters() if p.requires_grad]
    assert len(trainable) == 256 and all("_lora." in k for k in trainable)
    out["keys"] = np.array(keys)
    out["n_adapter_params"] = sum(p.numel() for p in model.student_unet.parameters() if p.requires_grad)
    y = unet_out(model.student_unet, cfg)
    out["unet_out"] = y.numpy()
    saved = {k: p.detach().clone() for k, p in model.student_unet.named_parameters() if k.endswith("up.weight")}
    with torch.no_grad():
        for k, p in model.student_unet.named_parameters():
            if k in saved:
                p.zero_()
        y0 = unet_out(model.student_unet, cfg)
        for k, p in model.student_unet.named_parameters():
            if k in saved:
                p.copy_(saved[k])
    effect = float((y - y0).norm() / y.norm())
    assert effect >= 4 * 2.5e-2, "adapters change the prediction by only %.3e rel-L2: raise lora_cases.UP_STD" % effect
    out["adapter_effect"] = effect

    P = cases.prompt_states(cfg, LC.B, LC.L, "distill")
    model.get_prompt_embeds = lambda prompt, use_cf, num_samples_per_prompt=1: (
        P["embeds_cf"], P["mask_cf"], P["embeds"], P["mask"])
    model.encode_text_classifier_free = lambda prompt, n: (P["embeds_cf"], P["mask_cf"], P["embeds"], P["mask"])
    z0 = cases.t(spec.det_uniform("distill.z0", (LC.B, 8, LC.H, LC.W), 14)) * 0.9
    rec = {}
    o_randint, o_randn_like, o_rand = torch.randint, torch.randn_like, torch.rand

    def recording(name, fn):
        def wrapped(*a, **k):
            vv = fn(*a, **k)
            rec.setdefault(name, vv.clone())
            return vv
        return wrapped

    torch.manual_seed(4321)
    torch.randint, torch.randn_like, torch.rand = (recording("randint", o_randint), recording("randn_like", o_randn_like),
                                                   recording("rand", o_rand))
    try:
        model.train()
        model.teacher_unet.eval()
        model.student_ema_unet.eval()
        loss = model(z0, ["a"] * LC.B)
    finally:
        torch.randint, torch.randn_like, torch.rand = o_randint, o_randn_like, o_rand
    loss.backward()
    out["loss"] = float(loss.detach())
    out["time_inds"] = rec["randint"].numpy()
    out["noise"] = rec["randn_like"].numpy()
    out["guidance"] = rec["rand"].numpy() * 6
    for k, p in model.student_unet.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
            out["grad." + k] = p.grad.numpy()
        else:
            assert p.grad is None, k
    model.update_ema()     # the reference's EMA update accepts the pair (same keys on both sides)

    import models.audio_guided_model as AGM
    lat = cases.t(spec.det_uniform("gdm.inf_noise", (LC.B, 8, 256, 16), 16)) * np.float32(np.sqrt(3.0))
    AGM.randn_tensor = lambda shape, generator=None, device=None, dtype=None: lat.clone()
    model2 = build(AudioGDM, ns, cfg, "tiny_light.json")      # fresh EMA copy (the update above moved the first one)
    model2.get_prompt_embeds = model.get_prompt_embeds
    model2.encode_text_classifier_free = model.encode_text_classifier_free
    model2.eval()
    sched = DDIM(set_alpha_to_one=False, **mgg.SD21)
    with torch.no_grad():
        z = model2.inference(["a"] * LC.B, sched, guidance_scale_input=3.0, guidance_scale_post=1.0, num_steps=4, use_ema=True)
    out["inference_4steps"] = z.numpy()
    path = os.path.join(HERE, "lora_gdm_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    print({k: (vv if np.ndim(vv) == 0 or np.size(vv) < 8 else np.shape(vv)) for k, vv in out.items() if not k.startswith("grad.")})


if __name__ == "__main__":
    torch.set_num_threads(os.cpu_count())
    main()
