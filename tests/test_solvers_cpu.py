"""The DDIM solver and the Karras sigmas of stage-2 distillation, host side (no GPU): `AudioLCM(use_edm=False)` and
`AudioLCM(use_karras=True)` construct with the reference's scheduler, tables and init_noise_sigma
(models/audio_consistency_model.py:72-84), run directories carrying either flag load, the Karras tables of
`HeunDiscreteScheduler` match the reference's (scheduling_heun_discrete.py:204-208,229-267), and the CPU restatement
the GPU tests lean on (tests/solver_oracle.py) reproduces the reference's own training loss in both modes.
Fixture: tests/golden/make_golden_solvers.py."""
import argparse
import os

import numpy as np
import pytest
import torch

import cases
import solver_oracle as so
from consistencytta_amd import scheduler, spec
from consistencytta_amd.models import AudioLCM


def _lcm(**flags):
    return AudioLCM(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                    unet_model_config_path="tiny_light.json", unet_config=cases.TINY_UNET, snr_gamma=5.0,
                    teacher_guidance_scale=-1, num_diffusion_steps=18, vae=None, loss_type="mse", target_ema_decay=0.95,
                    ema_decay=0.999, **flags)


def test_audiolcm_constructs_in_every_solver_mode(golden):
    g = golden("solvers_tiny")
    ddim_ts = np.arange(17, -1, -1) * 55                                  # 935, 880, ..., 55, 0
    assert np.array_equal(g["ddim.noise_scheduler_timesteps"], ddim_ts)
    for flags in (dict(use_edm=False), dict(use_edm=False, use_karras=True), dict()):   # use_edm defaults to False
        m = _lcm(**flags)
        s = m.noise_scheduler
        assert type(s) is scheduler.DDIMScheduler and not m.use_edm
        assert s.timesteps.dtype == torch.int64 and np.array_equal(s.timesteps.numpy(), ddim_ts)
        assert s.init_noise_sigma == 1.0 == float(g["ddim.init_noise_sigma"]) and s.num_inference_steps == 18
        assert not hasattr(s, "use_karras_sigmas")                      # Karras without Heun has no effect (:77-82)
        # compute_snr (:215-219 -> audio_distilled_model.py:165-192)
        ac = s.alphas_cumprod
        np.testing.assert_allclose(m.compute_snr(s.timesteps, None).numpy(), (ac / (1 - ac))[s.timesteps].numpy(), rtol=1e-6)
    m = _lcm(use_edm=True, use_karras=True)
    s = m.noise_scheduler
    assert type(s) is scheduler.HeunDiscreteScheduler and s.use_karras_sigmas and m.use_edm and m.use_karras
    assert s.timesteps.dtype == torch.float64 and len(s.timesteps) == 35 and len(s.sigmas) == 36
    assert np.abs(s.timesteps.numpy() - g["heun_karras.noise_scheduler_timesteps"]).max() <= 1e-9
    np.testing.assert_allclose(float(s.init_noise_sigma), float(g["heun_karras.init_noise_sigma"]), rtol=1e-6)
    np.testing.assert_allclose(m.compute_snr(None, torch.tensor([0, 4])).numpy(), s.sigmas[[0, 4]].numpy() ** -2.0, rtol=1e-6)
    # the Heun / uniform mode is what it was
    s = _lcm(use_edm=True).noise_scheduler
    assert type(s) is scheduler.HeunDiscreteScheduler and not s.use_karras_sigmas
    assert np.array_equal(s.timesteps.numpy(), golden("heun")["timesteps_18"])


@pytest.mark.parametrize("flags", [dict(use_edm=False, use_karras=False), dict(use_edm=True, use_karras=True)])
def test_run_directory_with_either_flag_builds(tmp_path, flags):
    from consistencytta_amd import checkpoint as ck
    run = str(tmp_path / "run")
    args = argparse.Namespace(stage=2, text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                              unet_model_name=None, unet_model_config="tiny_light.json", snr_gamma=5.0,
                              freeze_text_encoder=True, uncondition=False, use_lora=False, target_ema_decay=0.95,
                              ema_decay=0.999, num_diffusion_steps=18, teacher_guidance_scale=-1, loss_type="mse",
                              finetune_vae=False, output_dir=run, **flags)
    ck.write_args_summary(run, args)
    m = _lcm(**flags)
    for i, net in enumerate((m.teacher_unet, m.student_unet, m.student_target_unet, m.student_ema_unet)):
        net.init_deterministic(seed=20 + i)
    path = os.path.join(run, "pytorch_model_2.bin")
    torch.save(m.state_dict(), path)
    m2, ta = ck.build_model_from_run(path, os.path.join(run, "summary.jsonl"), vae=None, stage=2, unet_config=cases.TINY_UNET)
    assert ta.use_edm == flags["use_edm"] and ta.use_karras == flags["use_karras"] and not m2.training
    assert type(m2.noise_scheduler) is type(m.noise_scheduler)
    assert np.array_equal(m2.noise_scheduler.timesteps.numpy(), m.noise_scheduler.timesteps.numpy())
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("how", ["constructor", "assigned"])
def test_karras_tables_match_reference(golden, how):
    g, gh = golden("solvers_tiny"), golden("heun")
    if how == "constructor":
        s = scheduler.HeunDiscreteScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler",
                                                            use_karras_sigmas=True)
    else:       # the reference switches it on after construction (audio_consistency_model.py:80, inference.py:167)
        s = scheduler.HeunDiscreteScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
        assert np.array_equal(s.timesteps.numpy(), np.concatenate([[999.], np.repeat(np.arange(998., -1, -1), 2)]))
        s.use_karras_sigmas = True
    for n in (2, 18, 200):
        s.set_timesteps(n)
        ts, ref = s.timesteps.numpy(), g["karras_timesteps_%d" % n]
        assert s.timesteps.dtype == torch.float64 and s.sigmas.dtype == torch.float32 and ts.shape == ref.shape
        np.testing.assert_allclose(s.sigmas.numpy(), g["karras_sigmas_%d" % n], rtol=1e-6, atol=0)
        dev = np.abs(ts - ref).max()
        print("Karras N=%d: max |timestep - reference| %.3e, first %.13f" % (n, dev, ts[0]))
        assert dev <= 1e-9
        assert abs(ts[0] - 998.9999997466181) <= 1e-9 and ts[0] != 999.0 and ts[-1] == 0.0
        assert np.array_equal(s._timesteps_host, ts) and np.array_equal(s._sigmas_host, s.sigmas.numpy())
    s.set_timesteps(18)
    assert len(s.timesteps) == 35 and len(s.sigmas) == 36 and s.state_in_first_order
    np.testing.assert_allclose(s.timesteps.numpy()[:3], [998.9999997466181, 957.1340889625562, 957.1340889625562], atol=1e-9, rtol=0)
    np.testing.assert_allclose(s.sigmas.numpy()[:3], [14.614647, 11.420151, 11.420151], rtol=1e-6)
    np.testing.assert_allclose(s.sigmas.numpy()[-3:], [0.029167533, 0.029167533, 0], rtol=1e-6)
    assert list(s.index_for_timestep(s.timesteps[[0, 1, 2, 34]])) == [0, 2, 2, 34]
    # ... and with the flag off the tables are the uniform ones again
    s.use_karras_sigmas = False
    for n in (1, 2, 18, 200):
        s.set_timesteps(n)
        assert np.array_equal(s.timesteps.numpy(), gh["timesteps_%d" % n])
        np.testing.assert_allclose(s.sigmas.numpy(), gh["sigmas_%d" % n], rtol=1e-6, atol=0)


@pytest.mark.parametrize("mode", list(so.MODES))
def test_cpu_restatement_reproduces_reference_training_loss(golden, mode):
    """tests/solver_oracle.py read the semantics of both modes correctly: its loss on the reference's recorded draws is
    the reference's own (2e-4 relative: two fp32 evaluation orders of the same U-Nets)."""
    g = golden("solvers_tiny")
    cfg = cases.TINY_UNET
    P = cases.prompt_states(cfg, 3, 6, "distill")
    z0 = cases.t(spec.det_uniform("distill.z0", (3, 8, 32, 8), 14)) * 0.9
    noise, w = torch.from_numpy(g[mode + ".noise"]), torch.from_numpy(g[mode + ".guidance"])
    inds = torch.from_numpy(g[mode + ".time_inds"]).to(torch.int64)
    with torch.no_grad():
        if mode == "ddim":
            loss = so.ddim_distill_loss(so.nets_tiny(), P, z0, noise, inds, w)
        else:
            loss = so.heun_karras_distill_loss(so.nets_tiny(), P, z0, noise, inds * 2, w, g["karras_timesteps_18"],
                                               g["karras_sigmas_18"])
    ref = float(g[mode + ".train_loss"])
    print("%s: restated loss %.8f reference %.8f (rel %.2e)" % (mode, float(loss), ref, abs(float(loss) - ref) / ref))
    assert abs(float(loss) - ref) <= 2e-4 * ref
