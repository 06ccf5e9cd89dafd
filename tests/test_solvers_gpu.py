"""The DDIM solver (`AudioLCM(use_edm=False)`, the reference's default) and Heun on Karras sigmas
(`AudioLCM(use_edm=True, use_karras=True)`) on the HIP path, against fixtures produced by the reference's own
`models.AudioLCM` in both modes (tests/golden/make_golden_solvers.py), with the reference's draws replayed: training and
validation losses, the student's gradients (tiny and light widths), generation (student, teacher, a captured teacher
loop, a model sampled with the other solver's scheduler), the captured training step in its three forms, the optimizer
step, and the one-pass DDIM primitives (`ctta_ddim_step`, `ctta_ddim_noising`) against the launches they fuse.
Every tolerance is the one the Heun / uniform path is held to (test_models_gpu.py, test_train_gpu.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
import solver_oracle as so  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from consistencytta_amd import scheduler, spec  # noqa: E402
from consistencytta_amd.models import AudioLCM  # noqa: E402
from gpu_util import DEV, rel_l2  # noqa: E402

REL_L2 = 2.5e-2                 # test_models_gpu.py:15
GRAD_REL_L2 = 8e-2              # test_train_gpu.py:21-22
GRAD_REL_L2_ALL = 4e-2
MODES = list(so.MODES)


def _build(mode, cfg, path):
    m = AudioLCM(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                 unet_model_config_path=path, unet_config=cfg, snr_gamma=5.0, teacher_guidance_scale=-1,
                 num_diffusion_steps=18, vae=None, loss_type="mse", target_ema_decay=0.95, ema_decay=0.999, **so.MODES[mode])
    m.teacher_unet.load_state_dict(cases.unet_weights(cfg, False, 0))
    m.student_unet.load_state_dict(cases.unet_weights(cfg, True, 1))
    m.student_target_unet.load_state_dict(cases.unet_weights(cfg, True, 2))
    m.student_ema_unet.load_state_dict(cases.unet_weights(cfg, True, 3))
    return m.to(DEV)


def _lcm(mode):
    m = _build(mode, cases.TINY_UNET, "tiny_light.json")
    P = {k: v.to(DEV) for k, v in cases.prompt_states(cases.TINY_UNET, 3, 6, "distill").items()}
    z0 = (cases.t(spec.det_uniform("distill.z0", (3, 8, 32, 8), 14)) * 0.9).to(DEV)
    return m, P, z0


def _order(mode):
    return 2 if so.MODES[mode]["use_edm"] else 1     # `time_inds=` is the index of t_{n+1} in noise_scheduler.timesteps


def _block_of(key):
    head, _, rest = key.partition(".")
    return head + "." + rest.split(".")[0] if head in ("down_blocks", "up_blocks") else head


def _check_student_grads(tag, m, g, pre=""):
    """The student's gradients against the reference's autograd (per tensor: norm + strided sample, the format of
    distill_light*.npz): per block the relative L2 over the samples <= GRAD_REL_L2_ALL, per tensor the deviation of the
    full norm <= GRAD_REL_L2 (test_train_gpu.py `_check_student_grads`)."""
    names = [str(k) for k in g[pre + "grad_names"]]
    params = dict(m.student_unet.named_parameters())
    assert names == [k for k, p in params.items() if p.requires_grad]
    assert params["guidance_proj.weight"].grad is None
    off, norms = g[pre + "grad_offsets"], g[pre + "grad_norms"]
    samples = torch.from_numpy(g[pre + "grad_samples_bf16"]).view(torch.bfloat16).double().numpy()
    blocks, worst_norm = {}, ("", 0.0)
    for i, k in enumerate(names):
        gr = params[k].grad.detach().reshape(-1)
        idx = torch.from_numpy(cases.sample_index(gr.numel())).to(DEV)
        got = gr[idx].double().cpu().numpy()
        ref = samples[off[i]:off[i + 1]]
        b = blocks.setdefault(_block_of(k), [0.0, 0.0])
        b[0] += float(((got - ref) ** 2).sum())
        b[1] += float((ref ** 2).sum())
        nrel = abs(float(gr.double().norm()) - norms[i]) / max(norms[i], 1e-30)
        if nrel > worst_norm[1]:
            worst_norm = (k, nrel)
    tot_e, tot_n = sum(b[0] for b in blocks.values()), sum(b[1] for b in blocks.values())
    for name, (e, n) in blocks.items():
        print("  %-28s sampled grad rel_l2 %.3e" % (name, (e / max(n, 1e-300)) ** 0.5))
    print("%s, all blocks: sampled rel_l2 %.3e ; worst per-tensor norm deviation %s %.3e"
          % (tag, (tot_e / tot_n) ** 0.5, worst_norm[0], worst_norm[1]))
    for name, (e, n) in blocks.items():
        assert (e / max(n, 1e-300)) ** 0.5 <= GRAD_REL_L2_ALL, (tag, name)
    assert worst_norm[1] <= GRAD_REL_L2, (tag, worst_norm)
    for name in ("teacher_unet", "student_target_unet", "student_ema_unet"):
        assert all(p.grad is None for p in getattr(m, name).parameters())


# ------------------------------------------------------------------------------------------------ check 4
@pytest.mark.parametrize("mode", MODES)
def test_distillation_losses_and_gradients_match_reference(golden, mode):
    g = golden("solvers_tiny")
    pre = mode + "."
    m, P, z0 = _lcm(mode)
    m.train()
    loss = m(z0, None, P, time_inds=torch.from_numpy(g[pre + "time_inds"]).to(torch.int64) * _order(mode),
             gaussian_noise=torch.from_numpy(g[pre + "noise"]).to(DEV), guidance_scale=torch.from_numpy(g[pre + "guidance"]))
    ref = float(g[pre + "train_loss"])
    print("%s: distillation loss hip %.6f ref %.6f (rel %.2e)" % (mode, float(loss), ref, abs(float(loss) - ref) / ref))
    assert loss.requires_grad and abs(float(loss) - ref) <= 5e-2 * ref
    loss.backward()
    torch.cuda.synchronize()
    _check_student_grads(mode + " tiny", m, g, pre)
    m.zero_grad()
    m.eval()
    vl = m(z0, None, P, validation_mode=2, run_teacher=True, gaussian_noise=torch.from_numpy(g[pre + "val_noise"]).to(DEV),
           guidance_scale=torch.from_numpy(g[pre + "val_guidance"]))
    got = np.array([float(v) for v in vl])
    print("%s: validation losses hip" % mode, got, "ref", g[pre + "val_losses"])
    np.testing.assert_allclose(got, g[pre + "val_losses"], rtol=6e-2)
    if so.MODES[mode]["use_edm"]:
        assert m.noise_scheduler.state_in_first_order


@pytest.mark.parametrize("mode", MODES)
def test_distillation_step_at_light_widths_matches_reference(golden, mode):
    g = golden("solvers_light_" + mode)
    ti, noise, u = so.light_draws(mode)
    assert np.array_equal(ti.numpy(), g["time_inds"]) and np.array_equal((u * 6).numpy(), g["guidance"])
    assert abs(float(noise.double().sum()) - float(g["noise_sum"])) <= 1e-9 * float(noise.double().abs().sum()), \
        "injected draws changed: noise"
    cfg = spec.LIGHT_UNET_CONFIG
    m = _build(mode, cfg, "tango_diffusion_light.json")
    P = {k: v.to(DEV) for k, v in cases.prompt_states(cfg, 2, 16, "distill_light").items()}
    z0 = (cases.t(spec.det_uniform("distill_light.z0", (2, 8, 256, 16), 14)) * 0.9).to(DEV)
    m.train()
    loss = m(z0, None, P, time_inds=ti * _order(mode), gaussian_noise=noise.to(DEV), guidance_scale=u * 6)
    ref = float(g["train_loss"])
    print("%s: light-width distillation loss hip %.6f ref %.6f (rel %.2e)" % (mode, float(loss), ref, abs(float(loss) - ref) / ref))
    assert abs(float(loss) - ref) <= 5e-2 * ref
    loss.backward()
    torch.cuda.synchronize()
    _check_student_grads(mode + " light B=2", m, g)


# ------------------------------------------------------------------------------------------------ check 5
def _inference_scheduler(mode):
    if not so.MODES[mode]["use_edm"]:
        return scheduler.DDIMScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    s = scheduler.HeunDiscreteScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    s.use_karras_sigmas = True            # inference.py:167
    return s


@pytest.mark.parametrize("mode", MODES)
def test_inference_student_and_teacher_match_reference(golden, mode):
    g = golden("solvers_tiny")
    pre = mode + "."
    m, P, _ = _lcm(mode)
    m.eval()
    noise = so.inf_noise(3).to(DEV)
    edm = so.MODES[mode]["use_edm"]
    sched = _inference_scheduler(mode)
    _, tea, _, _ = m.inference(P, sched, guidance_scale_input=4.0, guidance_scale_post=1.0, num_steps=1, use_edm=edm,
                               use_ema=True, query_teacher=True, num_teacher_steps=3, return_all=True, noise=noise)
    with so.RenoiseInjector() as inj:
        stu2 = m.inference(P, sched, guidance_scale_input=3.0, guidance_scale_post=2.0, num_steps=2, use_edm=edm,
                           use_ema=False, noise=noise)
    assert inj.k == 1
    l2t = rel_l2(so.strided(tea), torch.from_numpy(g[pre + "inf_teacher_3steps"]))
    l2s = rel_l2(so.strided(stu2), torch.from_numpy(g[pre + "inf_student_2step_cfg"]))
    print("%s: 2-step student + post-CFG rel_l2 %.3e, 3-step teacher rel_l2 %.3e" % (mode, l2s, l2t))
    assert l2s <= 2 * REL_L2 and l2t <= 2 * REL_L2
    # the captured teacher loop = the eager loop, for the fixture's schedule and for a longer one
    for steps in (3, 7):
        _, eager, _, _ = m.inference(P, sched, guidance_scale_input=4.0, num_steps=1, use_edm=edm, query_teacher=True,
                                     num_teacher_steps=steps, return_all=True, noise=noise)
        _, graphed, _, _ = m.inference(P, sched, guidance_scale_input=4.0, num_steps=1, use_edm=edm, query_teacher=True,
                                       num_teacher_steps=steps, return_all=True, noise=noise, graph_teacher=True)
        assert torch.equal(eager, graphed), (mode, steps, rel_l2(graphed, eager))
        if steps == 3:
            assert torch.equal(eager, tea)
    if edm:
        assert sched.state_in_first_order


def test_inference_of_a_heun_model_with_a_ddim_scheduler_matches_reference(golden):
    """The scheduler is the CALLER's choice, the re-noising stride the model's (audio_consistency_model.py:497-499): a
    use_edm=True model with a DDIMScheduler and num_steps=4 re-noises at every second of 750, 500, 250, 0."""
    g = golden("solvers_tiny")
    m, P, _ = _lcm("heun_karras")
    m.eval()
    sched = scheduler.DDIMScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    seen, add_noise = [], sched.add_noise
    sched.add_noise = lambda x, n, t: (seen.append(int(t)), add_noise(x, n, t))[1]
    with so.RenoiseInjector() as inj:
        stu = m.inference(P, sched, guidance_scale_input=3.0, guidance_scale_post=1.0, num_steps=4, use_edm=False,
                          use_ema=True, noise=so.inf_noise(3).to(DEV))
    assert inj.k == 2 and seen == [500, 0] == list(g["mixed.renoise_timesteps"])
    l2 = rel_l2(so.strided(stu), torch.from_numpy(g["mixed.student_4steps"]))
    print("use_edm=True model, DDIM scheduler, 4 steps: rel_l2 %.3e" % l2)
    assert l2 <= 2 * REL_L2
    # the other way round runs too: a DDIM-distilled model sampled with the Heun scheduler (stride 1 on its table)
    m2, P2, _ = _lcm("ddim")
    m2.eval()
    heun = scheduler.HeunDiscreteScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    out, tea, _, _ = m2.inference(P2, heun, guidance_scale_input=3.0, num_steps=2, use_edm=True, query_teacher=True,
                                  num_teacher_steps=2, return_all=True, noise=so.inf_noise(3).to(DEV))
    assert torch.isfinite(out).all() and torch.isfinite(tea).all() and heun.state_in_first_order


# ------------------------------------------------------------------------------------------------ check 6
def _batches(mode, n, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        out.append(dict(z=(torch.randn(3, 8, 32, 8, generator=gen) * 0.9).to(DEV),
                        kw=dict(time_inds=torch.randint(0, 17, (3,), generator=gen) * _order(mode),
                                gaussian_noise=torch.randn(3, 8, 32, 8, generator=gen).to(DEV),
                                guidance_scale=torch.rand(3, generator=gen) * 6)))
    out[1]["kw"]["time_inds"][0] = 0                      # the largest timestep: noise * init_noise_sigma
    out[2]["kw"]["time_inds"][1] = 16 * _order(mode)      # t_n = 0: the target is z_0 of THAT batch
    return out


def _pair(mode):
    m1, P, _ = _lcm(mode)
    m1.train()
    o1 = m1.prepare_training(lr=1e-4, weight_decay=1e-4, broadcast=False)
    m2, _, _ = _lcm(mode)
    m2.train()
    o2 = m2.prepare_training(lr=1e-4, weight_decay=1e-4, broadcast=False)
    return m1, o1, m2, o2, P


NETS = ("student_unet", "student_target_unet", "student_ema_unet")


def _same_weights(m1, m2):
    for name in NETS:
        getattr(m2, name)._flat.copy_(getattr(m1, name)._flat)
        getattr(m2, name).mark_weights_changed()


def _eager(m1, P, b):
    with torch.no_grad():
        loss, pred, target, sig, gamma = m1._forward_impl(b["z"], None, P, False, True, b["kw"]["time_inds"],
                                                          b["kw"]["gaussian_noise"], b["kw"]["guidance_scale"], True)
        m1._student_backward(pred, target, sig, gamma, 1.0, None)
    return loss


def _tail(*pairs):
    for o, m in pairs:
        o.step(grad_scale=1.0)
        o.zero_grad()
        m.update_ema()


@pytest.mark.parametrize("mode", MODES)
def test_captured_step_monolithic_equals_eager(mode):
    batches = _batches(mode, 5, 31)
    m1, o1, m2, o2, P = _pair(mode)
    gs = m2.capture_train_graph(o2, batches[4]["z"], P, segmented=False, **batches[4]["kw"])
    assert float(o2.grad.abs().max()) == 0.0 and o2.step_count == 0
    for i, b in enumerate(batches[:4]):
        _same_weights(m1, m2)
        loss = _eager(m1, P, b)
        gs._refresh(b["z"], b["kw"]["time_inds"], b["kw"]["gaussian_noise"], b["kw"]["guidance_scale"])
        gs.replay()
        torch.cuda.synchronize()
        l_e, l_g = float(loss), float(gs.loss.item())
        rel = float((o1.grad - o2.grad).norm() / o1.grad.norm())
        print("%s monolithic, batch %d: eager loss %.9g graph loss %.9g, gradient rel diff %.2e" % (mode, i, l_e, l_g, rel))
        assert l_e == l_g and np.isfinite(l_e)
        assert float(o1.grad.norm()) > 0 and rel <= 1e-7
        _tail((o1, m1), (o2, m2))
    _same_weights(m1, m2)
    v1 = m1.train_step(batches[0]["z"], P, o1, None, **batches[0]["kw"])
    v2 = gs.step(batches[0]["z"], None, **batches[0]["kw"])
    assert v1 == v2 and o2.step_count == o1.step_count == 5 and float(o2.grad.abs().max()) == 0.0


@pytest.mark.parametrize("mode", MODES)
def test_captured_step_segmented_with_bucket_allreduce_equals_eager(mode):
    """One graph per backward block (bucket_min_elems=1) with the bucketed gradient all-reduce issued between the
    replays, on one rank with a real RCCL process group (CTTA_FORCE_COLLECTIVES=1), as the data-parallel step runs it."""
    import os
    import torch.distributed as dist
    from consistencytta_amd import dist_util as du
    batches = _batches(mode, 5, 37)
    m1, o1, m2, o2, P = _pair(mode)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29583")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    os.environ["CTTA_FORCE_COLLECTIVES"] = "1"
    try:
        gs = m2.capture_train_graph(o2, batches[4]["z"], P, bucket_min_elems=1, **batches[4]["kw"])
        assert gs.segmented and len(gs.segments) > 1 and all(len(bs) == 1 for _, bs in gs.segments)
        blocks = [b for _, bs in gs.segments for b in bs]
        for i, b in enumerate(batches[:4]):
            _same_weights(m1, m2)
            loss = _eager(m1, P, b)
            gs._refresh(b["z"], b["kw"]["time_inds"], b["kw"]["gaussian_noise"], b["kw"]["guidance_scale"])
            buckets = du.GradientBuckets(o2.grad, m2.student_unet.block_ranges(), min_elems=1)
            assert buckets.enabled
            seen = []
            gs.replay(lambda blk: (seen.append(blk), buckets.ready(blk)))
            assert buckets.wait() == 1 and seen == blocks
            torch.cuda.synchronize()
            l_e, l_g = float(loss), float(gs.loss.item())
            rel = float((o1.grad - o2.grad).norm() / o1.grad.norm())
            print("%s segmented, batch %d: eager loss %.9g graph loss %.9g, gradient rel diff %.2e" % (mode, i, l_e, l_g, rel))
            assert l_e == l_g and np.isfinite(l_e) and rel <= 1e-7
            _tail((o1, m1), (o2, m2))
        # the data-parallel public entry points (GradientBuckets, AnyRankFlag) from equal states
        _same_weights(m1, m2)
        v1 = m1.train_step(batches[1]["z"], P, o1, None, **batches[1]["kw"])
        v2 = gs.step(batches[1]["z"], None, **batches[1]["kw"])
        torch.cuda.synchronize()
        assert v1 == v2 and o1.step_count == o2.step_count == 5 and float(o2.grad.abs().max()) == 0.0
    finally:
        os.environ["CTTA_FORCE_COLLECTIVES"] = "0"
        if created:
            dist.destroy_process_group()


@pytest.mark.parametrize("mode", MODES)
def test_captured_step_with_pipelined_teacher_equals_eager(mode):
    batches = _batches(mode, 6, 41)
    m1, o1, m2, o2, P = _pair(mode)
    gs = m2.capture_train_graph(o2, batches[5]["z"], P, segmented=False, pipeline_teacher=True, **batches[5]["kw"])
    assert gs.pipelined and gs.teacher_graph is not None and float(o2.grad.abs().max()) == 0.0
    assert gs.feed(batches[0]["z"], **batches[0]["kw"]) is False            # primes the pipeline
    for i in range(4):
        b = batches[i]
        _same_weights(m1, m2)
        loss = _eager(m1, P, b)
        assert gs.feed(batches[i + 1]["z"], **batches[i + 1]["kw"]) is True  # batch i becomes current, i + 1 goes to the teacher
        gs.replay()
        torch.cuda.synchronize()
        l_e, l_g = float(loss), float(gs.loss.item())
        rel = float((o1.grad - o2.grad).norm() / o1.grad.norm())
        print("%s pipelined, batch %d: eager loss %.9g graph loss %.9g, gradient rel diff %.2e" % (mode, i, l_e, l_g, rel))
        assert l_e == l_g and np.isfinite(l_e) and rel <= 1e-7
        _tail((o1, m1), (o2, m2))
    _same_weights(m1, m2)
    v1 = m1.train_step(batches[4]["z"], P, o1, None, **batches[4]["kw"])
    v2 = gs.step(batches[0]["z"], None, **batches[0]["kw"])
    assert v1 == v2 and o1.step_count == o2.step_count == 5
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ check 7
def _rows(name, B, n, seed):
    return cases.t(spec.det_uniform(name, (B, n), seed)).to(DEV)


def _vec(v):
    return torch.as_tensor(np.asarray(v, dtype=np.float32)).to(DEV)


def _lincomb(x, y, a, b, clamp=0.0):
    out = torch.empty_like(x)
    N.check(N.lib().ctta_lincomb2_rows(N.ptr(x), N.ptr(y), N.ptr(a), N.ptr(b), N.ptr(out), x.shape[0], x.shape[1],
                                       float(clamp), N.stream_ptr()))
    return out


@pytest.mark.parametrize("B,n", [(3, 8 * 32 * 8), (9, 8 * 256 * 16), (18, 8 * 256 * 16)])
@pytest.mark.parametrize("pred_type", ["v_prediction", "epsilon"])
@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("clamp", [0.0, 1.0])
def test_one_pass_ddim_step_equals_the_four_launch_chain(B, n, pred_type, cfg, clamp):
    L_ = N.lib()
    s = scheduler.DDIMScheduler(**dict(scheduler.SD21_SCHEDULER_CONFIG, set_alpha_to_one=False, prediction_type=pred_type,
                                       clip_sample=clamp > 0, clip_sample_range=clamp or 1.0))
    s.set_timesteps(50)
    t = s.timesteps[torch.arange(B) * 49 // max(B - 1, 1)]              # distinct timesteps per row, 980 ... 0
    assert len(set(t.tolist())) == B and int(t[-1]) == 0                # the last row steps to "prev < 0"
    x = _rows("ddimk.x", B, n, 1) * 2
    mo = _rows("ddimk.v", 2 * B if cfg else B, n, 2)
    w = _vec(np.linspace(0.0, 6.0, B)) if cfg else None
    # the chain stage 1 launches: ctta_cfg_combine, then DDIMScheduler.step's three ctta_lincomb2_rows
    if cfg:
        v = torch.empty_like(x)
        N.check(L_.ctta_cfg_combine(N.ptr(mo[:B]), N.ptr(mo[B:]), N.ptr(w), N.ptr(v), B, n, N.stream_ptr()))
    else:
        v = mo
    ref = s.step(v.view(B, 8, -1, 8), t, x.view(B, 8, -1, 8))
    prev, x0 = s.step_fused(mo.view(-1, 8, n // 64, 8), t, x.view(B, 8, -1, 8), cfg_w=w, want_x0=True)
    torch.cuda.synchronize()
    assert torch.equal(prev, ref.prev_sample) and torch.equal(x0, ref.pred_original_sample)
    assert torch.equal(s.step_fused(mo.view(-1, 8, n // 64, 8), t, x.view(B, 8, -1, 8), cfg_w=w), ref.prev_sample)
    if clamp > 0:
        assert float(x0.abs().max()) == clamp                           # the clamp is active on these inputs
    # ... and spelled out with raw launches and the four coefficient vectors
    c = s.step_coeffs(t, B)
    sa, sb, sap, sbp = (_vec(q) for q in c.numpy())
    if pred_type == "v_prediction":
        x0r = _lincomb(x, v, sa, _vec(-c[1].numpy()), clamp)
        eps = _lincomb(v, x, sa, sb)
    else:
        x0r = _lincomb(x, v, _vec((1.0 / c[0]).numpy()), _vec((-c[1] / c[0]).numpy()), clamp)
        eps = v
    assert torch.equal(prev.view(B, n), _lincomb(x0r, eps, sap, sbp))


@pytest.mark.parametrize("B,n", [(3, 8 * 32 * 8), (9, 8 * 256 * 16), (18, 8 * 256 * 16)])
def test_one_pass_noising_equals_add_noise_and_where(B, n):
    s = scheduler.DDIMScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    s.set_timesteps(18)
    t = s.timesteps[torch.arange(B) % 18]
    x = (_rows("ddimk.z0", B, n, 3) * 0.9).view(B, 8, -1, 8)
    nz = (_rows("ddimk.nz", B, n, 4) * np.float32(np.sqrt(3.0))).view(B, 8, -1, 8)
    last = t == int(s.timesteps.max())
    assert 0 < int(last.sum()) < B
    for init_sigma in (1.0, 14.6146):
        ref = torch.where(last.reshape(-1, 1, 1, 1).to(DEV), nz * init_sigma, s.add_noise(x, nz, t))
        got = s.add_noise_last(x, nz, t, last.to(DEV, torch.float32), init_sigma=init_sigma)
        assert torch.equal(got, ref)
    assert torch.equal(s.add_noise_last(x, nz, t), s.add_noise(x, nz, t))       # no flags: plain add_noise


def test_ddim_primitives_refuse_bad_arguments():
    L_ = N.lib()
    B, n = 2, 64
    x, v, out = _rows("ddimk.e1", B, n, 5), _rows("ddimk.e2", B, n, 6), torch.empty(B, n, device=DEV)
    c = _vec(np.full(B, 0.5))
    st = N.stream_ptr()
    null = N.c_void_p(0)
    ok = lambda rc: rc == 0       # noqa: E731
    assert ok(L_.ctta_ddim_step(N.ptr(v), null, N.ptr(x), N.ptr(c), N.ptr(c), N.ptr(c), N.ptr(c), 0, 0.0, N.ptr(out), null, B, n, st))
    assert ok(L_.ctta_ddim_noising(N.ptr(x), N.ptr(v), N.ptr(c), N.ptr(c), null, 1.0, N.ptr(out), B, n, st))
    torch.cuda.synchronize()
    before = out.clone()
    bad = [L_.ctta_ddim_step(null, null, N.ptr(x), N.ptr(c), N.ptr(c), N.ptr(c), N.ptr(c), 0, 0.0, N.ptr(out), null, B, n, st),
           L_.ctta_ddim_step(N.ptr(v), null, null, N.ptr(c), N.ptr(c), N.ptr(c), N.ptr(c), 0, 0.0, N.ptr(out), null, B, n, st),
           L_.ctta_ddim_step(N.ptr(v), null, N.ptr(x), null, N.ptr(c), N.ptr(c), N.ptr(c), 0, 0.0, N.ptr(out), null, B, n, st),
           L_.ctta_ddim_step(N.ptr(v), null, N.ptr(x), N.ptr(c), N.ptr(c), N.ptr(c), N.ptr(c), 0, 0.0, null, null, B, n, st),
           L_.ctta_ddim_step(N.ptr(v), null, N.ptr(x), N.ptr(c), N.ptr(c), N.ptr(c), N.ptr(c), 0, 0.0, N.ptr(out), null, B, n - 2, st),
           L_.ctta_ddim_step(N.ptr(v), null, N.ptr(x), N.ptr(c), N.ptr(c), N.ptr(c), N.ptr(c), 2, 0.0, N.ptr(out), null, B, n, st),
           L_.ctta_ddim_noising(null, N.ptr(v), N.ptr(c), N.ptr(c), null, 1.0, N.ptr(out), B, n, st),
           L_.ctta_ddim_noising(N.ptr(x), N.ptr(v), N.ptr(c), null, null, 1.0, N.ptr(out), B, n, st),
           L_.ctta_ddim_noising(N.ptr(x), N.ptr(v), N.ptr(c), N.ptr(c), null, 1.0, null, B, n, st),
           L_.ctta_ddim_noising(N.ptr(x), N.ptr(v), N.ptr(c), N.ptr(c), null, 1.0, N.ptr(out), B, n - 1, st)]
    assert all(rc != 0 for rc in bad), bad
    with pytest.raises(N.CttaError, match="multiple of 4"):
        N.check(L_.ctta_ddim_noising(N.ptr(x), N.ptr(v), N.ptr(c), N.ptr(c), null, 1.0, N.ptr(out), B, n - 1, st))
    torch.cuda.synchronize()
    assert torch.equal(out, before)                                     # an error status, not a launch
    s = scheduler.DDIMScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    s.set_timesteps(18)
    with pytest.raises(RuntimeError):
        s.step_fused(torch.zeros(2, 8, 4, 4), 55, torch.zeros(2, 8, 4, 4))          # CPU tensors: no CPU path


# ------------------------------------------------------------------------------------------------ check 8
@pytest.mark.parametrize("mode", MODES)
def test_train_step_moves_student_and_both_shadows(mode):
    m, P, z0 = _lcm(mode)
    m.train()
    opt = m.prepare_training(lr=1e-4, weight_decay=1e-4, broadcast=False)
    before = {name: getattr(m, name)._flat.detach().clone() for name in NETS}
    teacher = [p.detach().clone() for p in m.teacher_unet.parameters()]
    torch.manual_seed(5)
    losses = [m.train_step(z0, P, opt) for _ in range(3)]               # the model's own draws
    torch.cuda.synchronize()
    print("%s: train_step losses" % mode, losses)
    assert all(np.isfinite(v) and v > 0 for v in losses) and opt.step_count == 3
    for name in NETS:
        assert not torch.equal(getattr(m, name)._flat, before[name]), name
        assert torch.isfinite(getattr(m, name)._flat).all()
    assert all(torch.equal(a, b) for a, b in zip(teacher, m.teacher_unet.parameters()))
    assert float(opt.grad.abs().max()) == 0.0
