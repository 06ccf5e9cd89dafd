"""Task-level parity: models.AudioLCM on the HIP path against fixtures
produced by the reference's own models.AudioLCM (tests/golden/make_golden_distill.py), with the
reference's internal random draws replayed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
from consistencytta_amd import scheduler, spec  # noqa: E402
from consistencytta_amd.models import AudioLCM  # noqa: E402
from gpu_util import DEV, rel_err, rel_l2  # noqa: E402

REL_L2 = 2.5e-2
# relative L2 difference between the gradients of two `forward().backward()` runs of the `_gdm()` case: the largest of the
# ten pairs among five runs on an MI355X (6.3e-9 ... 1.28e-8, LABNOTES.md)
GDM_GRAD_REPEAT_REL_L2 = 1.28e-8


def _model():
    cfg = cases.TINY_UNET
    m = AudioLCM(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                 unet_model_config_path="tiny_light.json", unet_config=cfg, snr_gamma=5.0, use_edm=True,
                 teacher_guidance_scale=-1, num_diffusion_steps=18, vae=None, loss_type="mse",
                 target_ema_decay=0.95, ema_decay=0.999)
    m.teacher_unet.load_state_dict(cases.unet_weights(cfg, False, 0))
    m.student_unet.load_state_dict(cases.unet_weights(cfg, True, 1))
    m.student_target_unet.load_state_dict(cases.unet_weights(cfg, True, 2))
    m.student_ema_unet.load_state_dict(cases.unet_weights(cfg, True, 3))
    m.to(DEV)
    P = {k: v.to(DEV) for k, v in cases.prompt_states(cfg, 3, 6, "distill").items()}
    z0 = (cases.t(spec.det_uniform("distill.z0", (3, 8, 32, 8), 14)) * 0.9).to(DEV)
    return m, P, z0


def test_distillation_forward_losses_and_teacher_query(golden):
    g = golden("distill_tiny")
    m, P, z0 = _model()
    m.train()   # as in train_one_epoch; frozen sub-nets stay in eval mode
    loss = m(z0, None, P, time_inds=torch.from_numpy(g["time_inds"]) * 2,
             gaussian_noise=torch.from_numpy(g["noise"]).to(DEV), guidance_scale=torch.from_numpy(g["guidance"]))
    ref = float(g["train_loss"])
    print("distillation loss hip %.6f ref %.6f" % (float(loss), ref))
    assert abs(float(loss) - ref) <= 5e-2 * ref     # a squared bf16 error budget: 2 * REL_L2
    m.eval()
    vl = m(z0, None, P, validation_mode=2, run_teacher=True, gaussian_noise=torch.from_numpy(g["val_noise"]).to(DEV),
           guidance_scale=torch.from_numpy(g["val_guidance"]))
    got = np.array([float(v) for v in vl])
    print("validation losses hip", got, "ref", g["val_losses"])
    np.testing.assert_allclose(got, g["val_losses"], rtol=6e-2)
    assert m.noise_scheduler.state_in_first_order
    ts = m.noise_scheduler.timesteps[torch.tensor([0, 6, 32])]
    zq = cases.t(spec.det_uniform("distill.zq", (3, 8, 32, 8), 15)).to(DEV)
    q = m._query_teacher(zq, ts, P["embeds_cf"], P["mask_cf"], torch.tensor([0.5, 3.0, 5.5]))
    # CFG extrapolation (1-w)*u + w*c amplifies the bf16 round-off of u and c by about |1-w| + w (10x at w = 5.5)
    l2 = rel_l2(q, torch.from_numpy(g["query_teacher"]))
    print("CFG teacher query rel_l2 %.3e (w up to 5.5)" % l2)
    assert l2 <= 3 * REL_L2


def test_inference_student_multistep_and_heun_teacher(golden):
    g = golden("distill_tiny")
    m, P, _ = _model()
    m.eval()
    sched = scheduler.HeunDiscreteScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    noise = (cases.t(spec.det_uniform("distill.inf_noise", (3, 8, 256, 16), 16)) * np.float32(np.sqrt(3.0))).to(DEV)
    stu, tea, _, _ = m.inference(P, sched, guidance_scale_input=4.0, guidance_scale_post=1.0, num_steps=1, use_edm=True,
                                 use_ema=True, query_teacher=True, num_teacher_steps=3, return_all=True, noise=noise)
    l2s, l2t = rel_l2(stu, torch.from_numpy(g["inf_student_1step"])), rel_l2(tea, torch.from_numpy(g["inf_teacher_3steps"]))
    print("inference 1-step rel_l2 %.3e, Heun teacher (5 CFG queries) rel_l2 %.3e" % (l2s, l2t))
    assert l2s <= REL_L2 and l2t <= 2 * REL_L2      # the teacher chains 5 U-Net evaluations
    assert sched.state_in_first_order
    # 2-step generation with post-CFG: replay the reference's re-noising draw
    ren = torch.from_numpy(g["inf_renoise"]).to(DEV)
    orig = torch.randn_like
    torch.randn_like = lambda x, *a, **k: ren.clone()
    try:
        stu2 = m.inference(P, sched, guidance_scale_input=3.0, guidance_scale_post=2.0, num_steps=2, use_edm=True,
                           use_ema=False, noise=noise)
    finally:
        torch.randn_like = orig
    l2 = rel_l2(stu2, torch.from_numpy(g["inf_student_2step_cfg"]))
    print("inference 2-step + post-CFG rel_l2 %.3e" % l2)
    assert l2 <= 2 * REL_L2


def test_update_ema_matches_reference_and_resyncs_engines(golden):
    g = golden("distill_tiny")
    m, P, z0 = _model()
    key = str(g["ema_key"])
    m.train()
    x, ts, gs, enc, mask = cases.unet_inputs(cases.TINY_UNET, 1, 16, 8, 4, "ema")
    args = dict(encoder_hidden_states=enc.to(DEV), encoder_attention_mask=mask.to(DEV))
    before = m.student_target_unet(x.to(DEV), ts.to(DEV), guidance=gs.to(DEV), **args).sample.clone()
    m.update_ema()
    sd_t, sd_e = m.student_target_unet.state_dict(), m.student_ema_unet.state_dict()
    assert torch.equal(sd_t[key][:4].cpu(), torch.from_numpy(g["ema_target_after"]))    # bit-exact
    assert torch.equal(sd_e[key][:4].cpu(), torch.from_numpy(g["ema_ema_after"]))
    after = m.student_target_unet(x.to(DEV), ts.to(DEV), guidance=gs.to(DEV), **args).sample
    assert not torch.equal(before, after)     # the engine re-packed the updated shadow weights
    m.eval()
    with pytest.raises(AssertionError):
        m.update_ema()                         # "EMA update should only be called during training"


def test_teacher_loop_hipgraph_matches_eager(golden):
    """Config 3: the Heun teacher loop replayed from one captured hipGraph gives the eager loop's result exactly,
    and that result matches the reference's own AudioLCM.inference (3 Heun steps = 5 CFG teacher queries)."""
    g = golden("distill_tiny")
    m, P, _ = _model()
    m.eval()
    sched = scheduler.HeunDiscreteScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    noise = (cases.t(spec.det_uniform("distill.inf_noise", (3, 8, 256, 16), 16)) * np.float32(np.sqrt(3.0))).to(DEV)
    kw = dict(guidance_scale_input=4.0, guidance_scale_post=1.0, num_steps=1, use_edm=True, use_ema=True,
              query_teacher=True, return_all=True, noise=noise)
    _, eager, _, _ = m.inference(P, sched, num_teacher_steps=3, **kw)
    _, graphed, _, _ = m.inference(P, sched, num_teacher_steps=3, graph_teacher=True, **kw)
    assert torch.equal(eager, graphed)
    assert rel_l2(graphed, torch.from_numpy(g["inf_teacher_3steps"])) <= 2 * REL_L2
    assert sched.state_in_first_order
    # a longer schedule (more replays of the same graph) and a second call (new capture) stay consistent
    _, e2, _, _ = m.inference(P, sched, num_teacher_steps=6, **kw)
    _, g2, _, _ = m.inference(P, sched, num_teacher_steps=6, graph_teacher=True, **kw)
    assert torch.equal(e2, g2)


def test_heun_teacher_loop_at_real_size_graph_equals_eager(tmp_path):
    """VERDICT r3 next #4 -- BASELINE configs[2] at its REAL size (models/audio_consistency_model.py:499-524): light teacher
    U-Net, 8 prompts (CFG batch 16), L = 32, 6 Heun steps = 11 CFG queries.  (i) With the defaults (the 3-stage ring rule
    for the K >= 4096 layers and the text-state K / V cache both active at exactly this batch) the hipGraph-replayed loop
    must equal the eager loop BIT FOR BIT, and so must a second capture; (ii) a second process without the text cache
    (every query re-projects K / V) must agree with (i): bit-identical -- a cached projection is the same kernel's output
    (until round 5 that process also switched the 3-stage ring off through an environment knob; the library reads no
    environment any more); (iii) finite, non-trivial output."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    res = []
    for tag, env, extra in (("default", {}, []), ("plain", {}, ["notextcache"])):
        out = str(tmp_path / (tag + ".pt"))
        p = subprocess.run([sys.executable, os.path.join(here, "teacher_loop_worker.py"), out, "6"] + extra,
                           env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        assert p.returncode == 0, p.stdout.decode(errors="replace")[-3000:]
        res.append(torch.load(out))
    a, b = res
    for r in res:
        assert torch.isfinite(r["eager"]).all() and float(r["eager"].std()) > 0
        assert torch.equal(r["eager"], r["graphed"]) and torch.equal(r["graphed"], r["graphed2"])
    d = float((a["eager"] - b["eager"]).norm() / b["eager"].norm())
    print("configs[2] real size: defaults vs (no text cache): rel diff %.3e; student %.3e"
          % (d, float((a["student"] - b["student"]).norm() / b["student"].norm())))
    assert torch.equal(a["eager"], b["eager"]) and torch.equal(a["student"], b["student"])


# ------------------------------------------------------------------------------------------------
# Stage-1 guided distillation: DDPM / DDIM schedulers and models.AudioGDM
def _gdm():
    from consistencytta_amd.models import AudioGDM
    cfg = cases.TINY_UNET
    m = AudioGDM(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                 unet_model_config_path="tiny_light.json", unet_config=cfg, snr_gamma=5.0, teacher_guidance_scale=-1,
                 ema_decay=0.999)
    m.teacher_unet.load_state_dict(cases.unet_weights(cfg, False, 0))
    m.student_unet.load_state_dict(cases.unet_weights(cfg, True, 1))
    m.student_ema_unet.load_state_dict(cases.unet_weights(cfg, True, 3))
    m.to(DEV)
    P = {k: v.to(DEV) for k, v in cases.prompt_states(cfg, 3, 6, "distill").items()}
    z0 = (cases.t(spec.det_uniform("distill.z0", (3, 8, 32, 8), 14)) * 0.9).to(DEV)
    return m, P, z0


def test_ddpm_ddim_schedulers_against_reference_golden(golden):
    g = golden("gdm_tiny")
    x = (cases.t(spec.det_uniform("gdm.x", (3, 8, 16, 4), 1)) * 2).to(DEV)
    noise = cases.t(spec.det_uniform("gdm.n", (3, 8, 16, 4), 2)).to(DEV)
    v = cases.t(spec.det_uniform("gdm.v", (3, 8, 16, 4), 3)).to(DEV)
    ddpm = scheduler.DDPMScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    np.testing.assert_array_equal(ddpm.timesteps[:5].numpy(), g["ddpm_timesteps_head"])
    np.testing.assert_allclose(ddpm.alphas_cumprod.numpy(), g["alphas_cumprod"], rtol=1e-6)
    t_train = torch.tensor([999, 400, 0])
    assert rel_err(ddpm.add_noise(x, noise, t_train), torch.from_numpy(g["ddpm_add_noise"])) < 1e-6
    assert ddpm.init_noise_sigma == 1.0 and ddpm.scale_model_input(x, 5) is x
    ddim = scheduler.DDIMScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    for n in (50, 5):
        ddim.set_timesteps(n)
        np.testing.assert_array_equal(ddim.timesteps.numpy(), g["ddim_timesteps_%d" % n])
    assert rel_err(ddim.step(v, torch.from_numpy(g["ddim_t"]), x).prev_sample, torch.from_numpy(g["ddim_step"])) < 1e-6
    assert rel_err(ddim.step(v, 600, x).prev_sample, torch.from_numpy(g["ddim_step_scalar_t"])) < 1e-6
    assert rel_err(ddim.add_noise(x, noise, t_train.to(DEV)), torch.from_numpy(g["ddim_add_noise"])) < 1e-6
    with pytest.raises(ValueError):
        scheduler.DDIMScheduler().step(v, 5, x)          # set_timesteps not called


def test_ddpm_ancestral_step_against_reference_golden(golden):
    """DDPMScheduler.step (scheduling_ddpm.py:285-418) on the HIP elementwise kernel vs the reference's own step with
    its recorded noise: full 1000-step schedule, 50/20/10-step schedules, epsilon + clipping, fixed_large variance,
    rows with t == 0 (no noise) and prev_t < 0 (alpha_prev = 1)."""
    g = golden("ddpm_step")
    x = (cases.t(spec.det_uniform("ddpm.x", (4, 8, 16, 4), 1)) * 2).to(DEV)
    v = cases.t(spec.det_uniform("ddpm.v", (4, 8, 16, 4), 3)).to(DEV)
    sd21 = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                prediction_type="v_prediction", clip_sample=False)
    for tag, kw, steps in (("v_full", sd21, None), ("v_50", sd21, 50),
                           ("eps_clip", dict(sd21, prediction_type="epsilon", clip_sample=True), 20),
                           ("v_large", dict(sd21, variance_type="fixed_large"), 10)):
        s = scheduler.DDPMScheduler(**kw)
        if steps:
            s.set_timesteps(steps)
        r = s.step(v, torch.from_numpy(g[tag + "_t"]), x, variance_noise=torch.from_numpy(g[tag + "_noise"]).to(DEV))
        assert rel_err(r.prev_sample, torch.from_numpy(g[tag + "_prev"])) < 2e-6, tag
        assert rel_err(r.pred_original_sample, torch.from_numpy(g[tag + "_x0"])) < 2e-6, tag
    s = scheduler.DDPMScheduler(**sd21)
    s.set_timesteps(50)
    assert rel_err(s.step(v, 0, x).prev_sample, torch.from_numpy(g["scalar_t_prev"])) < 2e-6
    # own noise: drawn for the t > 0 rows only, reproducible through the generator
    gen = torch.Generator(device=DEV).manual_seed(3)
    a = s.step(v, torch.tensor([980, 0, 20, 500]), x, generator=gen).prev_sample
    gen.manual_seed(3)
    b = s.step(v, torch.tensor([980, 0, 20, 500]), x, generator=gen).prev_sample
    assert torch.equal(a, b) and not torch.equal(a[0], s.step(v, torch.tensor([980, 0, 20, 500]), x).prev_sample[0])


def test_stage1_guided_distillation_loss_backward_and_inference(golden):
    """AudioGDM.forward vs the reference's own AudioGDM (recorded random draws), its gradients vs torch autograd over
    the oracle, one fused train_step, and the 4-step DDIM inference vs the reference."""
    from oracle import distill
    g = golden("gdm_tiny")
    m, P, z0 = _gdm()
    m.train()
    kw = dict(time_inds=torch.from_numpy(g["gdm_time_inds"]), gaussian_noise=torch.from_numpy(g["gdm_noise"]).to(DEV),
              guidance_scale=torch.from_numpy(g["gdm_guidance"]))
    loss = m(z0, P, **kw)
    ref = float(g["gdm_loss"])
    print("stage-1 loss hip %.6f ref %.6f" % (float(loss), ref))
    assert loss.requires_grad and abs(float(loss) - ref) <= 5e-2 * ref
    loss.backward()
    torch.cuda.synchronize()
    # oracle gradients
    cfg = cases.TINY_UNET
    student = {k: v.clone().requires_grad_(k != "guidance_proj.weight") for k, v in cases.unet_weights(cfg, True, 1).items()}
    n = distill.Nets(cfg, cases.unet_weights(cfg, False, 0), student, None, cases.unet_weights(cfg, True, 3))
    Pc = cases.prompt_states(cfg, 3, 6, "distill")
    z0c = cases.t(spec.det_uniform("distill.z0", (3, 8, 32, 8), 14)) * 0.9
    distill.gdm_loss(n, Pc, z0c, torch.from_numpy(g["gdm_noise"]), torch.from_numpy(g["gdm_time_inds"]),
                     torch.from_numpy(g["gdm_guidance"])).backward()
    num = den = 0.0
    for k, p in m.student_unet.named_parameters():
        if p.requires_grad:
            num += float((p.grad.cpu() - student[k].grad).norm()) ** 2
            den += float(student[k].grad.norm()) ** 2
    rel = (num / den) ** 0.5
    print("stage-1 gradients vs oracle autograd: rel_l2 %.3e" % rel)
    assert rel <= 4e-2
    # fused step
    for p in m.student_unet.parameters():
        p.grad = None
    opt = m.prepare_training(lr=1e-4, weight_decay=1e-2, broadcast=False)
    before = opt.flat.detach().clone()
    ema_before = m.student_ema_unet._flat.detach().clone()
    val = m.train_step(z0, P, opt, None, **kw)
    assert abs(val - float(loss)) <= 1e-5 * abs(val) and not torch.equal(opt.flat, before)
    assert not torch.equal(m.student_ema_unet._flat, ema_before) and float(opt.grad.abs().max()) == 0.0
    # inference (fresh model: the step above changed the weights)
    m2, P2, _ = _gdm()
    m2.eval()
    sched = scheduler.DDIMScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    lat = (cases.t(spec.det_uniform("gdm.inf_noise", (3, 8, 256, 16), 16)) * np.float32(np.sqrt(3.0))).to(DEV)
    z = m2.inference(P2, sched, guidance_scale_input=3.0, guidance_scale_post=1.0, num_steps=4, use_ema=True, noise=lat)
    l2 = rel_l2(z, torch.from_numpy(g["gdm_inference_4steps"]))
    print("stage-1 4-step DDIM inference rel_l2 %.3e" % l2)
    assert l2 <= 2 * REL_L2


def test_stage1_train_step_is_forward_backward_adamw_and_ema(golden):
    """AudioGDM.train_step pinned against the pieces it is made of, on the recorded draws of `gdm_tiny`: model 1 runs
    `forward(...).backward()`; model 2, from identical weights, runs `train_step`.  Same loss bit for bit; one AdamW step
    whose first moment is (1 - beta1) x model 1's gradient; the gradient buffer zeroed; the EMA shadow moved by
    (1 - ema_decay) * (p_after - shadow_before), bit for bit (the kernel's own unfused fp32 arithmetic, as
    test_update_ema_matches_reference_and_resyncs_engines holds it against the reference).
    Gradient bound: two `forward().backward()` runs of this very case differ by GDM_GRAD_REPEAT_REL_L2 in relative L2
    (the atomics of the normalisation-layer reductions add in arrival order; LABNOTES.md); twice that is allowed, and never
    more than 1e-6.  The moment is compared in the form the kernel computes it, fl32((1 - beta1) * g) with 1 - beta1 in
    fp32 -- one fp32 multiply, which torch repeats bit for bit on model 1's gradient: dividing exp_avg back by (1 - beta1)
    would add the rounding of that multiply and of the division (6.3e-8 measured, the same on every run) to a comparison
    whose bound is 2.6e-8."""
    g = golden("gdm_tiny")
    kw = dict(time_inds=torch.from_numpy(g["gdm_time_inds"]), gaussian_noise=torch.from_numpy(g["gdm_noise"]).to(DEV),
              guidance_scale=torch.from_numpy(g["gdm_guidance"]))
    m1, P, z0 = _gdm()
    m1.train()
    opt1 = m1.prepare_training(lr=1e-4, weight_decay=1e-2, broadcast=False)
    loss1 = m1(z0, P, **kw)
    loss1.backward()
    torch.cuda.synchronize()
    grad1 = opt1.grad[:opt1.n].clone()
    assert float(grad1.abs().max()) > 0 and opt1.step_count == 0

    m2, P2, _ = _gdm()
    m2.train()
    opt2 = m2.prepare_training(lr=1e-4, weight_decay=1e-2, broadcast=False)
    assert torch.equal(opt2.flat, opt1.flat)
    ema_before = m2.student_ema_unet._flat.detach().clone()
    val = m2.train_step(z0, P2, opt2, None, **kw)
    torch.cuda.synchronize()
    assert val == float(loss1.detach())                                   # bit for bit
    assert opt2.step_count == 1 and float(opt2.grad.abs().max()) == 0.0
    beta1 = np.float32(opt2.param_groups[0]["betas"][0])
    want = grad1 * float(np.float32(1.0) - beta1)                         # exp_avg after one step from zero moments
    rel = float((opt2.exp_avg - want).norm() / want.norm())
    bound = min(2 * GDM_GRAD_REPEAT_REL_L2, 1e-6)
    print("stage-1 train_step: loss %.8f, gradient vs forward().backward() rel_l2 %.3e (bound %.1e)" % (val, rel, bound))
    assert rel <= bound
    assert not torch.equal(opt2.flat, opt1.flat)
    ema_after = m2.student_ema_unet._flat
    assert not torch.equal(ema_after, ema_before)
    assert torch.equal(ema_after, ema_before + (1 - m2.ema_decay) * (opt2.flat - ema_before))


def test_whole_pipeline_hipgraph_matches_eager():
    """ConsistencyTTA.capture_graph: one hipGraph for U-Net -> VAE decoder -> HiFi-GAN -> int16; replays with new inputs
    must equal the eager pipeline bit for bit."""
    from consistencytta_amd import modules
    from consistencytta_amd.models import ConsistencyTTA
    cfg = cases.TINY_UNET
    vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    pipe = ConsistencyTTA(unet_config=cfg, vae=vae)
    pipe.to(DEV)
    pipe.unet.init_deterministic(1)
    vae.init_deterministic(2)
    pipe.eval().requires_grad_(False)
    B, L = 2, 7
    gen = pipe.capture_graph(B, L, cfg_scale_input=4.0, cross_attention_dim=cfg["cross_attention_dim"], latent=(8, 32, 16))
    for seed in (1, 2):
        x, _, _, enc, mask = cases.unet_inputs(cfg, B, 32, 16, L, "graph%d" % seed)
        pcm = gen(enc.to(DEV), mask.to(DEV), x.to(DEV)).clone()
        lat = pipe.generate_latent(enc.to(DEV), mask.to(DEV), x.to(DEV), 4.0, 1.0, 1)
        mel = vae.decode_first_stage(lat)
        ref = vae.decode_to_waveform(mel)
        assert torch.equal(gen.outputs[0], lat) and torch.equal(gen.outputs[1], mel)
        assert np.array_equal(pcm.cpu().numpy(), ref)


def test_three_stage_batch_pipeline_equals_the_eager_pipeline_two_calls_later():
    """Round 4 -- ConsistencyTTA.capture_pipeline: U-Net(batch i), VAE decoder(batch i-1) and HiFi-GAN(batch i-2) as three
    hipGraphs on three streams per call.  Five different batches fed in a row: call j returns the int16 waveforms of
    batch j-2, bit-identical to the eager pipeline on that batch (the hand-over copies at the call boundary carry the
    right batch to the right stage)."""
    from consistencytta_amd import modules
    from consistencytta_amd.models import ConsistencyTTA
    cfg = cases.TINY_UNET
    vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    pipe = ConsistencyTTA(unet_config=cfg, vae=vae)
    pipe.to(DEV)
    pipe.unet.init_deterministic(1)
    vae.init_deterministic(2)
    pipe.eval().requires_grad_(False)
    B, L = 2, 7
    gen = pipe.capture_pipeline(B, L, cfg_scale_input=4.0, cross_attention_dim=cfg["cross_attention_dim"], latent=(8, 32, 16),
                                candidates=3)
    assert gen.depth == 2 and set(gen.placement_ms) == {"u", "v"}
    batches, refs = [], []
    for seed in range(5):
        x, _, _, enc, mask = cases.unet_inputs(cfg, B, 32, 16, L, "pipe%d" % seed)
        batches.append((enc.to(DEV), mask.to(DEV), x.to(DEV)))
        lat = pipe.generate_latent(*batches[-1], 4.0, 1.0, 1)
        refs.append(vae.decode_to_waveform(vae.decode_first_stage(lat)))
    assert not np.array_equal(refs[0], refs[1])
    outs = []
    for b in batches + batches[-1:] * 2:                  # two extra calls drain the pipeline
        outs.append(gen(*b).cpu().numpy().copy())
    for j, ref in enumerate(refs):
        assert np.array_equal(outs[j + 2], ref), j


def test_batch32_graph_and_three_stage_pipeline_equal_eager_bit_for_bit(golden):
    """The forms bench.py times for BASELINE.json configs[1] -- `capture_graph(32, 32, cfg_scale_input=4.0)` and
    `capture_pipeline(32, 32, cfg_scale_input=4.0)`, the arguments of bench.py -- at the light widths, on the batch of
    `cases.batch32_inputs()` that test_engines_gpu.py pins against the reference's own modules: their int16 output equals
    the eager pipeline's bit for bit.  The pipeline gets three different batches (the fixture's batch, a row-permuted
    copy of it, a fresh draw) and is drained; every output must be its own batch's, two calls later."""
    from gpu_util import light_pipeline, run_light_pipeline
    pipe = light_pipeline(float(golden("pipeline_batch32")["scale_factor"]))
    X = cases.batch32_inputs()
    B, L = X["enc"].shape[:2]
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(7))
    gen = torch.Generator().manual_seed(4)
    lens = torch.randint(6, L + 1, (B,), generator=gen)
    batches = [(X["enc"], X["mask"], X["noise"]), (X["enc"][perm], X["mask"][perm], X["noise"][perm]),
               (torch.randn(B, L, 1024, generator=gen) * 0.25, torch.arange(L)[None, :] < lens[:, None],
                torch.randn(B, 8, 256, 16, generator=gen))]
    batches = [tuple(t.to(DEV) for t in b) for b in batches]
    refs = []
    for b in batches:
        lat, mel, _ = run_light_pipeline(pipe, *b)
        refs.append(pipe.vae.decode_to_waveform(mel))
    assert refs[0].shape == (B, 163872) and not np.array_equal(refs[0], refs[1])
    graph = pipe.capture_graph(B, L, cfg_scale_input=4.0)
    for b, ref in zip(batches, refs):
        assert np.array_equal(graph(*b).cpu().numpy(), ref)
    del graph
    gen3 = pipe.capture_pipeline(B, L, cfg_scale_input=4.0)
    outs = []
    for b in batches + batches[-1:] * 2:                  # two extra calls drain the pipeline
        outs.append(gen3(*b).cpu().numpy().copy())
    for j, ref in enumerate(refs):
        assert np.array_equal(outs[j + 2], ref), j


class _FakeTokenizer:
    """Whitespace tokenizer with T5's calling convention (the sentencepiece model is not available offline)."""
    model_max_length = 512

    def __call__(self, prompt, max_length=None, padding=True, truncation=True, return_tensors="pt"):
        max_length = max_length or self.model_max_length
        rows = [[(sum(map(ord, w)) % 500) + 2 for w in p.split()][:max_length - 1] + [1] for p in prompt]
        width = max_length if padding == "max_length" else max(len(r) for r in rows)
        ids = torch.zeros(len(rows), width, dtype=torch.long)
        mask = torch.zeros(len(rows), width, dtype=torch.long)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r)
            mask[i, :len(r)] = 1
        return type("Batch", (), {"input_ids": ids, "attention_mask": mask})()


def test_prompt_to_waveform_with_the_hip_text_encoder():
    """easy_inference ConsistencyTTA.forward (consistencytta.py:135-200) end to end on the HIP engines: tokenizer (host)
    -> T5 encoder -> CFG batch -> U-Net -> VAE -> HiFi-GAN; equals the embedding-level entry point fed with the oracle's
    T5 states within the path tolerance, for cfg_scale_post = 1 and > 1."""
    from consistencytta_amd import modules, text_encoder
    from consistencytta_amd.models import ConsistencyTTA
    from oracle import t5 as ot5
    cfg = dict(cases.TINY_UNET, cross_attention_dim=cases.TINY_T5["d_model"])
    vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    te = text_encoder.T5EncoderModel(cases.TINY_T5)
    tsd = cases.t5_weights(cases.TINY_T5)
    te.load_state_dict(tsd)
    pipe = ConsistencyTTA(unet_config=cfg, vae=vae, text_encoder=te, tokenizer=_FakeTokenizer())
    pipe.to(DEV)
    pipe.unet.init_deterministic(1)
    vae.init_deterministic(2)
    pipe.eval().requires_grad_(False)
    prompts = ["a dog barks twice", "rain"]
    emb_cf, mask_cf, emb, mask = pipe.encode_text_classifier_free(prompts, 1)
    assert emb.shape == (2, 5, 256) and emb_cf.shape == (4, 5, 256) and mask.dtype == torch.bool
    tok = _FakeTokenizer()(prompts)
    with torch.no_grad():
        ref = ot5.t5_encode(cases.TINY_T5, tsd, tok.input_ids, tok.attention_mask)
    assert rel_l2(emb, ref) <= REL_L2
    for post in (1.0, 2.0):
        torch.manual_seed(5)
        pcm = pipe(prompts, cfg_scale_input=4.0, cfg_scale_post=post, num_steps=1)
        assert pcm.dtype == np.int16 and pcm.shape[0] == 2
        torch.manual_seed(5)
        noise = torch.randn((2, 8, 256, 16), device=DEV)
        kw = dict(uncond_states=emb_cf[:2], uncond_mask=mask_cf[:2]) if post > 1 else {}
        again = pipe.forward_from_embeds(emb, mask, noise, 4.0, post, 1, **kw)
        assert np.array_equal(pcm, again)


def test_released_checkpoint_layout_round_trip(tmp_path):
    """`unet_state_dict.pt` + `vae_state_dict.pt` ({"state_dict", "scale_factor"}) as easy_inference/consistencytta.py:22-42
    reads them: written from one pipeline with torch.save, loaded by from_checkpoint_dir, same waveform bit for bit."""
    from consistencytta_amd import modules
    from consistencytta_amd.models import ConsistencyTTA
    cfg = cases.TINY_UNET
    vae = modules.AutoencoderKL(embed_dim=8, scale_factor=0.9227914214134216)
    a = ConsistencyTTA(unet_config=cfg, vae=vae)
    a.unet.init_deterministic(1)
    vae.init_deterministic(2)
    torch.save(a.unet.state_dict(), tmp_path / "unet_state_dict.pt")
    torch.save({"state_dict": vae.state_dict(), "scale_factor": vae.scale_factor}, tmp_path / "vae_state_dict.pt")
    b = ConsistencyTTA.from_checkpoint_dir(str(tmp_path), unet_config=cfg, device=DEV)
    a.to(DEV).eval().requires_grad_(False)
    assert list(b.vae.state_dict().keys()) == list(vae.state_dict().keys()) and b.vae.scale_factor == vae.scale_factor
    x, _, _, enc, mask = cases.unet_inputs(cfg, 1, 32, 16, 5, "ckpt")
    wa = a.forward_from_embeds(enc.to(DEV), mask.to(DEV), x.to(DEV), 4.0, 1.0, 1)
    wb = b.forward_from_embeds(enc.to(DEV), mask.to(DEV), x.to(DEV), 4.0, 1.0, 1)
    assert wa.dtype == np.int16 and np.array_equal(wa, wb)
