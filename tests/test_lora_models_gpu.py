"""AudioGDM(use_lora=True) on the HIP path against the reference's own AudioGDM with LoRA (tests/golden/make_golden_lora.py,
recorded random draws): loss, adapter gradients, one training step, DDIM inference.  (AudioGDM has no graphed inference
loop, so there is no graphed-vs-eager case.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
import lora_util as LU  # noqa: E402
from consistencytta_amd import scheduler, spec  # noqa: E402
from gpu_util import DEV, rel_l2  # noqa: E402

REL_L2 = 2.5e-2


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_loss_and_adapter_gradients_against_the_reference(golden):
    """loss within 5e-2 relative; pooled rel-L2 of the adapter gradients <= 4e-2 (measured 1.1e-2 on an MI355X)"""
    g = golden("lora_gdm_tiny")
    m, P, z0 = LU.gdm()
    m.train()
    loss = m(z0, P, **LU.draws(g))
    ref = float(g["loss"])
    val = float(loss.detach())
    print("stage-1 LoRA loss hip %.6f ref %.6f" % (val, ref))
    assert loss.requires_grad and abs(val - ref) <= 5e-2 * ref
    loss.backward()
    torch.cuda.synchronize()
    assert LU.adapter_grad_error(m.student_unet, g, "AudioGDM.forward().backward()") <= 4e-2
    assert all(p.grad is None for k, p in m.student_unet.named_parameters() if "_lora." not in k)


def test_one_train_step_moves_the_adapters_only(golden):
    g = golden("lora_gdm_tiny")
    m, P, z0 = LU.gdm()
    m.train()
    opt = m.prepare_training(lr=1e-4, weight_decay=1e-2, broadcast=False)
    n = opt.n
    assert n == 55872 == m.student_unet.n_trainable() and opt.exp_avg.numel() == n and opt.n_tail == n
    stu, ema = opt.flat, m.student_ema_unet._flat
    assert stu.numel() == ema.numel() > n and torch.equal(_bits(stu), _bits(ema))
    stu0, ema0 = stu.detach().clone(), ema.detach().clone()
    val = m.train_step(z0, P, opt, None, **LU.draws(g))
    torch.cuda.synchronize()
    assert abs(val - float(g["loss"])) <= 5e-2 * float(g["loss"]) and opt.step_count == 1
    # the adapter segment moved (weight decay applies to it: the adapters are the only trainable parameters) ...
    assert not torch.equal(stu[:n], stu0[:n]) and float(opt.exp_avg.abs().max()) > 0
    assert bool((stu[:n] != stu0[:n]).float().mean() > 0.9)
    # ... the base segment of the student and of the EMA copy is bitwise what it was
    assert torch.equal(_bits(stu[n:]), _bits(stu0[n:])) and torch.equal(_bits(ema[n:]), _bits(ema0[n:]))
    # the EMA adapters moved by (1 - decay) * (student - ema), bit for bit (as the stage-1 step test holds the full model)
    assert not torch.equal(ema[:n], ema0[:n])
    assert torch.equal(ema[:n], ema0[:n] + (1 - m.ema_decay) * (stu[:n] - ema0[:n]))
    assert float(opt.grad.abs().max()) == 0.0
    # the next forward of either network sees the new adapters
    x = LU.unet_inputs(m.student_unet._cfg)
    m.eval()
    a, b = m.student_unet(**x).sample, m.student_ema_unet(**x).sample
    assert bool(torch.isfinite(a).all()) and not torch.equal(a, b)


def test_ddim_inference_against_the_reference(golden):
    g = golden("lora_gdm_tiny")
    m, P, _ = LU.gdm()
    m.eval()
    sched = scheduler.DDIMScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    lat = (cases.t(spec.det_uniform("gdm.inf_noise", (3, 8, 256, 16), 16)) * np.float32(np.sqrt(3.0))).to(DEV)
    z = m.inference(P, sched, guidance_scale_input=3.0, guidance_scale_post=1.0, num_steps=4, use_ema=True, noise=lat)
    l2 = rel_l2(z, torch.from_numpy(g["inference_4steps"]))
    print("stage-1 LoRA 4-step DDIM inference rel_l2 %.3e" % l2)
    assert l2 <= 2 * REL_L2
