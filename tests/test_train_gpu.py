"""Backward pass of the student U-Net: every parameter gradient the HIP engine
produces is compared with torch autograd over the CPU oracle's forward (fp32), on the tiny
config of the golden cases.

Tolerance: activations and activation-gradients travel in bf16 (fp32 accumulation), the oracle is
fp32 end to end.  Per parameter tensor the relative L2 error must stay below GRAD_REL_L2; the
error over the whole concatenated gradient below GRAD_REL_L2_ALL.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from consistencytta_amd import modules, spec  # noqa: E402
from gpu_util import DEV, bf16_round  # noqa: E402
from oracle import nets as onets  # noqa: E402

GRAD_REL_L2 = 8e-2
GRAD_REL_L2_ALL = 4e-2


def _oracle_grads(cfg, sd, x, ts, gs, enc, mask, dout, guided=True):
    params = {k: v.clone().requires_grad_(k != "guidance_proj.weight") for k, v in sd.items()}
    out = onets.unet_forward(cfg, params, x, ts, gs if guided else None, enc, mask)
    (out * dout).sum().backward()
    return out.detach(), {k: p.grad for k, p in params.items() if p.requires_grad}


def _compare(grads_hip, grads_ref):
    num = den = 0.0
    worst = ("", 0.0)
    rows = []
    for k, r in grads_ref.items():
        g = grads_hip[k].detach().float().cpu()
        e = float((g - r).norm())
        n = float(r.norm())
        num += e * e
        den += n * n
        rel = e / max(n, 1e-30)
        rows.append((rel, k, n))
        if rel > worst[1]:
            worst = (k, rel)
    rows.sort(reverse=True)
    for rel, k, n in rows[:12]:
        print("  %-70s rel_l2 %.3e  |ref| %.3e" % (k, rel, n))
    total = (num / den) ** 0.5
    print("all parameters: rel_l2 %.3e ; worst %s %.3e" % (total, worst[0], worst[1]))
    return total, worst


@pytest.mark.parametrize("B,H,W,L", [(2, 32, 8, 7), (3, 16, 8, 5)])
def test_unet_parameter_gradients_match_autograd(B, H, W, L):
    cfg = cases.TINY_UNET
    sd = cases.unet_weights(cfg, True, 1)
    x, ts, gs, enc, mask = cases.unet_inputs(cfg, B, H, W, L, "train_tiny")
    dout = bf16_round(cases.t(spec.det_uniform("train.dout", (B, cfg["out_channels"], H, W), 21))) * 0.01
    ref_out, ref = _oracle_grads(cfg, sd, x, ts, gs, enc, mask, dout)

    m = modules.UNet2DConditionGuidedModel.from_config(cfg)
    m.load_state_dict(sd)
    m = m.to(DEV)
    out = m.forward_train(x.to(DEV), ts.to(DEV), gs.to(DEV), enc.to(DEV), mask.to(DEV))
    rel_out = float((out.cpu() - ref_out).norm() / ref_out.norm())
    assert rel_out < 2.5e-2, rel_out
    m.backward(dout.to(DEV))
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in m.named_parameters() if p.requires_grad}
    assert set(grads) == set(ref)
    assert m.get_parameter("guidance_proj.weight").grad is None       # embeddings.py:229 requires_grad=False
    total, worst = _compare(grads, ref)
    assert np.isfinite(total) and total <= GRAD_REL_L2_ALL
    assert worst[1] <= GRAD_REL_L2, worst

    # .grad semantics: a second forward/backward accumulates
    m.forward_train(x.to(DEV), ts.to(DEV), gs.to(DEV), enc.to(DEV), mask.to(DEV))
    m.backward(dout.to(DEV))
    torch.cuda.synchronize()
    k0 = "down_blocks.1.resnets.0.conv1.weight"
    assert float((grads[k0].cpu() - 2 * ref[k0]).norm() / (2 * ref[k0]).norm()) <= GRAD_REL_L2
    # and the plain forward still works on the training handle
    with torch.no_grad():
        out2 = m(x.to(DEV), ts.to(DEV), guidance=gs.to(DEV), encoder_hidden_states=enc.to(DEV),
                 encoder_attention_mask=mask.to(DEV)).sample
    # (not bit-equal: the inference forward fuses GEGLU into the GEMM epilogue, the training forward keeps the
    # pre-activation for the backward pass)
    assert float((out2 - out).norm() / out.norm()) < 2.5e-2      # two bf16 evaluation orders: the engines' stated tolerance


def test_backward_requires_a_training_forward():
    cfg = cases.TINY_UNET
    m = modules.UNet2DConditionGuidedModel.from_config(cfg).init_deterministic(1).to(DEV)
    x, ts, gs, enc, mask = cases.unet_inputs(cfg, 1, 16, 8, 4, "train_err")
    m.enable_training = True
    m(x.to(DEV), ts.to(DEV), guidance=gs.to(DEV), encoder_hidden_states=enc.to(DEV))
    from consistencytta_amd import _native as N
    with pytest.raises(N.CttaError, match="no training forward"):
        m.backward(torch.zeros(1, cfg["out_channels"], 16, 8))


# ------------------------------------------------------------------------------------------------
# The whole distillation step (SURVEY §8 a15 + a18 + a20): loss with a grad_fn, fused AdamW, EMA.
def _lcm():
    from consistencytta_amd.models import AudioLCM
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


def _oracle_distill_grads(g):
    """torch autograd through oracle.distill.distill_loss w.r.t. the student's parameters, with the
    reference's recorded random draws (the fixture made by the reference's own AudioLCM.forward)."""
    from oracle import distill
    cfg = cases.TINY_UNET
    student = {k: v.clone().requires_grad_(k != "guidance_proj.weight") for k, v in cases.unet_weights(cfg, True, 1).items()}
    n = distill.Nets(cfg, cases.unet_weights(cfg, False, 0), student, cases.unet_weights(cfg, True, 2),
                     cases.unet_weights(cfg, True, 3))
    P = cases.prompt_states(cfg, 3, 6, "distill")
    z0 = cases.t(spec.det_uniform("distill.z0", (3, 8, 32, 8), 14)) * 0.9
    noise, inds, w = torch.from_numpy(g["noise"]), torch.from_numpy(g["time_inds"]) * 2, torch.from_numpy(g["guidance"])
    with torch.no_grad():   # teacher / target side carries no gradient (audio_consistency_model.py:314-351)
        ts, sig = distill._tables()
        z_np1_scaled, t_np1, zhat, zhat_scaled, t_n, s_np1 = distill._teacher_two_queries(n, P, z0, noise, inds, w, ts, sig)
        target = onets.unet_forward(cfg, n.target, zhat_scaled, t_n, w, P["embeds"], P["mask"])
        target = torch.where((t_n == 0).reshape(-1, 1, 1, 1), z0, target)
    from oracle import heun
    pred = onets.unet_forward(cfg, student, z_np1_scaled, t_np1, w, P["embeds"], P["mask"])
    loss = heun.snr_mse_loss(pred, target, s_np1, 5.0)
    loss.backward()
    return float(loss), {k: p.grad for k, p in student.items() if p.requires_grad}


def test_distillation_loss_backward_matches_oracle_autograd(golden):
    g = golden("distill_tiny")
    ref_loss, ref = _oracle_distill_grads(g)
    assert abs(ref_loss - float(g["train_loss"])) <= 2e-4 * ref_loss     # oracle == reference's own forward
    m, P, z0 = _lcm()
    m.train()
    loss = m(z0, None, P, time_inds=torch.from_numpy(g["time_inds"]) * 2,
             gaussian_noise=torch.from_numpy(g["noise"]).to(DEV), guidance_scale=torch.from_numpy(g["guidance"]))
    assert loss.requires_grad and loss.grad_fn is not None
    assert abs(float(loss) - ref_loss) <= 5e-2 * ref_loss
    loss.backward()                                          # accelerator.backward(loss), train_utils.py:166
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in m.student_unet.named_parameters() if p.requires_grad}
    total, worst = _compare(grads, ref)
    # the student's input differs from the oracle's by the teacher's bf16 error too: a slightly wider budget
    assert np.isfinite(total) and total <= 1.5 * GRAD_REL_L2_ALL
    for name in ("teacher_unet", "student_target_unet", "student_ema_unet"):
        assert all(p.grad is None for p in getattr(m, name).parameters())
    # eval / no_grad calls stay graph-free
    with torch.no_grad():
        l2 = m(z0, None, P, time_inds=torch.from_numpy(g["time_inds"]) * 2,
               gaussian_noise=torch.from_numpy(g["noise"]).to(DEV), guidance_scale=torch.from_numpy(g["guidance"]))
    assert not l2.requires_grad


def test_train_step_adamw_and_ema_match_torch(golden):
    """train_step = backward + fused AdamW + lr schedule + two-shadow EMA.  Given the gradients the
    engine produced, the parameter update must equal torch.optim.AdamW's and the shadows the
    reference's do_ema_update (tools/train_utils.py:255-282), to fp32 round-off."""
    from consistencytta_amd.optim import WarmupSchedule
    g = golden("distill_tiny")
    m, P, z0 = _lcm()
    m.train()
    opt = m.prepare_training(lr=1e-3, weight_decay=1e-2, broadcast=False)
    sched = WarmupSchedule(opt, "linear", num_warmup_steps=2, num_training_steps=10)
    # shadow copies on the CPU driven by torch's own optimizer
    cpu = {k: p.detach().cpu().clone().requires_grad_(p.requires_grad) for k, p in m.student_unet.named_parameters()}
    topt = torch.optim.AdamW([p for p in cpu.values() if p.requires_grad], lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2,
                             eps=1e-8)
    tsched = torch.optim.lr_scheduler.LambdaLR(topt, sched._factor)
    tgt = {k: p.detach().cpu().clone() for k, p in m.student_target_unet.named_parameters()}
    ema = {k: p.detach().cpu().clone() for k, p in m.student_ema_unet.named_parameters()}
    kw = dict(time_inds=torch.from_numpy(g["time_inds"]) * 2, gaussian_noise=torch.from_numpy(g["noise"]).to(DEV),
              guidance_scale=torch.from_numpy(g["guidance"]))
    for it in range(3):
        # the engine's gradients for this step, captured through the autograd-compatible path
        loss = m(z0, None, P, **kw)
        loss.backward()
        torch.cuda.synchronize()
        for k, p in m.student_unet.named_parameters():
            if p.requires_grad:
                cpu[k].grad = p.grad.detach().cpu().clone()
        opt.zero_grad()
        value = m.train_step(z0, P, opt, sched, **kw)
        assert abs(value - float(loss)) <= 1e-6 * abs(value) + 1e-9
        topt.step()
        tsched.step()
        with torch.no_grad():
            for k in tgt:
                tgt[k] += np.float32(1. - 0.95) * (cpu[k].detach() - tgt[k])
                ema[k] += np.float32(1. - 0.999) * (cpu[k].detach() - ema[k])
        torch.cuda.synchronize()
        worst = 0.0
        for k, p in m.student_unet.named_parameters():
            d = float((p.detach().cpu() - cpu[k].detach()).abs().max())
            worst = max(worst, d / (float(cpu[k].detach().abs().max()) + 1e-12))
        print("step %d: loss %.6f  max relative parameter difference vs torch.optim.AdamW %.3e" % (it, value, worst))
        assert worst <= 2e-5          # deterministic engine -> same gradients in both passes; fp32 update round-off
        for name, refsd in (("student_target_unet", tgt), ("student_ema_unet", ema)):
            for k, p in getattr(m, name).named_parameters():
                assert float((p.detach().cpu() - refsd[k]).abs().max()) <= 1e-6 * (1 + float(refsd[k].abs().max())), (name, k)
        assert abs(opt.param_groups[0]["lr"] - topt.param_groups[0]["lr"]) < 1e-12
        assert float(opt.grad.abs().max()) == 0.0            # zero_grad
    # frozen Fourier projection never moves (embeddings.py:229)
    k = "guidance_proj.weight"
    assert torch.equal(m.student_unet.get_parameter(k).detach().cpu(), cases.unet_weights(cases.TINY_UNET, True, 1)[k])
    # the engines picked the new weights up: the next loss differs from the first one
    assert abs(m.train_step(z0, P, opt, sched, **kw) - float(g["train_loss"])) > 1e-6


def test_fused_optimizer_tail_gives_the_same_training_state_as_the_three_launches(golden, monkeypatch):
    """AudioLCM.train_step ends with AdamW -> zero_grad -> EMA x 2 (tools/train_utils.py:177-183).  From the second step on
    (the first one validates the flat-buffer layout of the four networks) that tail is ONE launch, ctta_adamw_ema2_zero;
    CTTA_FUSED_TAIL=0 keeps the three.  Here the tail alone, on the model's own buffers: the SAME gradient, weights, moments
    and schedule go through `_optimizer_tail` both ways (the whole step cannot be compared bit for bit across two runs: the
    backward folds some partials with fp32 atomics, and AdamW turns 1e-8 of gradient noise into lr-sized steps).  Student,
    target and EMA weights, both moments, the learning rate and the step count come out bit-identical, the gradient buffer
    zero, and the fused form really ran -- also with do_step = False, the NaN-loss skip."""
    from consistencytta_amd.optim import WarmupSchedule
    g = golden("distill_tiny")
    kw = dict(time_inds=torch.from_numpy(g["time_inds"]) * 2, gaussian_noise=torch.from_numpy(g["noise"]).to(DEV),
              guidance_scale=torch.from_numpy(g["guidance"]))
    m, P, z0 = _lcm()
    m.train()
    opt = m.prepare_training(lr=1e-3, weight_decay=1e-2, broadcast=False)
    sched = WarmupSchedule(opt, "linear", num_warmup_steps=2, num_training_steps=10)
    m.train_step(z0, P, opt, sched, **kw)            # validates the layout (three launches), leaves real moments behind
    nets = (m.student_unet, m.student_target_unet, m.student_ema_unet)
    gen = torch.Generator().manual_seed(3)
    grad = (torch.randn(opt.grad.numel(), generator=gen) * 1e-3).to(DEV)
    grad[opt.n:] = 0

    def snapshot():
        return ([n_._flat.clone() for n_ in nets], opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count,
                opt.param_groups[0]["lr"], dict(sched.__dict__) if hasattr(sched, "__dict__") else None)

    def restore(s_):
        for n_, f in zip(nets, s_[0]):
            n_._flat.copy_(f)
        opt.exp_avg.copy_(s_[1]); opt.exp_avg_sq.copy_(s_[2])
        opt.step_count = s_[3]
        opt.param_groups[0]["lr"] = s_[4]
        if s_[5] is not None:
            sched.__dict__.update(s_[5])

    start = snapshot()
    can_fuse = opt.n % 4 == 0 and opt.flat.numel() % 4 == 0
    for do_step in (True, False):
        results = []
        for fused in ("1", "0"):
            monkeypatch.setenv("CTTA_FUSED_TAIL", fused)
            restore(start)
            opt.grad.copy_(grad)
            calls = []
            real = opt.step_zero_ema
            opt.step_zero_ema = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
            m._optimizer_tail(opt, sched, 0.5, do_step)
            opt.step_zero_ema = real
            torch.cuda.synchronize()
            if can_fuse:
                assert len(calls) == (1 if fused == "1" else 0), (fused, calls)
            assert not bool(opt.grad.any())
            results.append(snapshot())
        a, b = results
        assert a[3] == b[3] == start[3] + (1 if do_step else 0) and a[4] == b[4]
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        for x, y in zip(a[0], b[0]):
            assert torch.equal(x, y)
        assert not torch.equal(a[0][1], start[0][1])                     # the shadows moved ...
        assert torch.equal(a[0][0], start[0][0]) == (not do_step)        # ... and the student only when the step was taken


def test_blockwise_backward_with_rccl_buckets_equals_monolithic(golden):
    """The overlapped data-parallel path on one GPU: a 1-rank RCCL process group with CTTA_FORCE_COLLECTIVES=1 makes
    train_step run the block-wise backward and issue the bucketed all-reduces; the parameters after one optimisation
    step must equal those of the plain (monolithic backward, no collective) step.  (Only one step is compared
    element-wise: the bf16 re-pack of the updated weights is discontinuous, so the last-bit noise of the LayerNorm
    atomics can flip a rounding and, through AdamW's normalisation, move a near-zero-gradient element by ~lr in the
    next step; the second step is checked through its loss.)"""
    import os
    import torch.distributed as dist
    from consistencytta_amd import dist_util as du
    g = golden("distill_tiny")
    kw = dict(time_inds=torch.from_numpy(g["time_inds"]) * 2, gaussian_noise=torch.from_numpy(g["noise"]).to(DEV),
              guidance_scale=torch.from_numpy(g["guidance"]))

    def run(force):
        m, P, z0 = _lcm()
        m.train()
        opt = m.prepare_training(lr=1e-3, weight_decay=1e-2, broadcast=False)
        os.environ["CTTA_FORCE_COLLECTIVES"] = "1" if force else "0"
        try:
            losses = [m.train_step(z0, P, opt, None, **kw)]
            torch.cuda.synchronize()
            flat1 = opt.flat.detach().clone()
            losses.append(m.train_step(z0, P, opt, None, **kw))
        finally:
            os.environ["CTTA_FORCE_COLLECTIVES"] = "0"
        torch.cuda.synchronize()
        return losses, flat1, m.student_unet.block_ranges(), opt.n

    ref_losses, ref_flat, ranges, n = run(False)
    # block ranges tile the trainable prefix of the flat buffer exactly
    spans = sorted(ranges.values())
    assert spans[0][0] == 0 and spans[-1][1] == n and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert set(ranges) == set(range(0, 2 * 4 + 3))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29581")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        losses, flat, _, _ = run(True)
    finally:
        if created:
            dist.destroy_process_group()
    assert abs(losses[0] - ref_losses[0]) <= 1e-6 * abs(ref_losses[0])
    assert abs(losses[1] - ref_losses[1]) <= 2e-3 * abs(ref_losses[1])
    worst = float((flat - ref_flat).abs().max() / ref_flat.abs().max())
    print("block-wise + RCCL vs monolithic: max relative parameter difference after one step %.3e" % worst)
    assert worst <= 5e-6      # LayerNorm gamma/beta gradients use fp32 atomics: last-bit run-to-run differences


def test_graph_captured_distillation_step_equals_eager_train_step(golden):
    """VERDICT r2 missing #2: the distillation micro-step captured into ONE hipGraph (AudioLCM.capture_train_graph: noising,
    two CFG teacher queries + Heun, target network, student training forward on its side stream and backward with the
    weight-gradient side stream, loss; AdamW / EMA eager behind it) against the eager `train_step`: same draws -> the same
    loss bit for bit and the same gradient up to the LayerNorm-atomics round-off (1e-7), from identical parameters, for
    three DIFFERENT draws (the static timestep / sigma / guidance tensors must really be refreshed before each replay;
    one draw takes the pure-noise branch of the noising step, one has t_n = 0 where the target becomes z_0)."""
    g = golden("distill_tiny")
    gen = torch.Generator().manual_seed(7)
    draws = [dict(time_inds=torch.from_numpy(g["time_inds"]) * 2, gaussian_noise=torch.from_numpy(g["noise"]).to(DEV),
                  guidance_scale=torch.from_numpy(g["guidance"]))]
    for _ in range(2):
        draws.append(dict(time_inds=torch.randint(0, 17, (3,), generator=gen) * 2,
                          gaussian_noise=torch.randn(3, 8, 32, 8, generator=gen).to(DEV),
                          guidance_scale=torch.rand(3, generator=gen) * 6))
    draws[2]["time_inds"][0] = 0          # the largest timestep: the pure-noise branch of the noising step
    draws[1]["time_inds"][1] = 32         # t_n = 0: the target is replaced by z_0
    m1, P, z0 = _lcm()
    m1.train()
    o1 = m1.prepare_training(lr=1e-4, weight_decay=1e-4, broadcast=False)
    m2, _, _ = _lcm()
    m2.train()
    o2 = m2.prepare_training(lr=1e-4, weight_decay=1e-4, broadcast=False)
    gs = m2.capture_train_graph(o2, z0, P, **draws[0])
    assert float(o2.grad.abs().max()) == 0.0 and o2.step_count == 0          # capturing moved nothing
    assert torch.equal(o2.flat, m2.student_unet._flat)
    nets = ("student_unet", "student_target_unet", "student_ema_unet")
    for it, kw in enumerate(draws):
        # same parameters on both sides (one AdamW step amplifies the 1e-8 LayerNorm-atomics noise of a gradient through
        # its sign-like first update, so free-running copies drift apart chaotically: 2e-6 in the loss after one step,
        # 4e-4 after two -- measured, eager vs eager behaves the same)
        for name in nets:
            getattr(m2, name)._flat.copy_(getattr(m1, name)._flat)
            getattr(m2, name).mark_weights_changed()
        with torch.no_grad():
            loss, pred, target, sig, gamma = m1._forward_impl(z0, None, P, False, True, kw["time_inds"], kw["gaussian_noise"],
                                                              kw["guidance_scale"], True)
            m1._student_backward(pred, target, sig, gamma, 1.0, None)
        gs._refresh(z0, kw["time_inds"], kw["gaussian_noise"], kw["guidance_scale"])
        gs.graph.replay()
        torch.cuda.synchronize()
        l_e, l_g = float(loss), float(gs.loss.item())
        rel = float((o1.grad - o2.grad).norm() / o1.grad.norm())
        print("draw %d: eager loss %.9g graph loss %.9g, gradient rel diff %.2e" % (it, l_e, l_g, rel))
        assert l_e == l_g and np.isfinite(l_e)
        assert float(o1.grad.norm()) > 0 and rel <= 1e-7
        for o, m in ((o1, m1), (o2, m2)):      # the eager tail of the step, identically on both sides
            o.step(grad_scale=1.0)
            o.zero_grad()
            m.update_ema()
    # the public entry points end to end: one more step each from (nearly) equal states
    v1 = m1.train_step(z0, P, o1, None, **draws[0])
    v2 = gs.step(z0, None, **draws[0])
    assert np.isfinite(v1) and abs(v1 - v2) <= 1e-3 * abs(v1) and o2.step_count == o1.step_count == 4
    assert float(o2.grad.abs().max()) == 0.0
    with pytest.raises(N.CttaError, match="pre-computed text states"):
        m2.capture_train_graph(o2, z0, ["a", "b", "c"])


def test_segmented_step_graph_with_rccl_buckets_equals_monolithic_graph_and_eager(golden):
    """the distillation micro-step captured as 1 + n hipGraphs (forward + loss + out head | one graph
    per backward block) with the bucketed gradient all-reduce issued BETWEEN the replays -- the form the data-parallel
    step runs (tools/train_utils.py:152-183 under DDP).  On one rank with a real RCCL process group
    (CTTA_FORCE_COLLECTIVES=1: every block's slice of the flat gradient buffer goes through ncclAllReduce on RCCL's
    stream) the segmented replay must reproduce the monolithic replay and the eager step: loss bit-identical, gradient
    to the LayerNorm-atomics round-off, for two different draws; the public `step` then moves the parameters like the
    eager `train_step`."""
    import os
    import torch.distributed as dist
    g = golden("distill_tiny")
    gen = torch.Generator().manual_seed(11)
    draws = [dict(time_inds=torch.from_numpy(g["time_inds"]) * 2, gaussian_noise=torch.from_numpy(g["noise"]).to(DEV),
                  guidance_scale=torch.from_numpy(g["guidance"])),
             dict(time_inds=torch.randint(0, 17, (3,), generator=gen) * 2,
                  gaussian_noise=torch.randn(3, 8, 32, 8, generator=gen).to(DEV), guidance_scale=torch.rand(3, generator=gen) * 6)]
    models = []
    for _ in range(3):
        m, P, z0 = _lcm()
        m.train()
        models.append((m, m.prepare_training(lr=1e-4, weight_decay=1e-4, broadcast=False)))
    (m_e, o_e), (m_g, o_g), (m_s, o_s) = models
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29583")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    os.environ["CTTA_FORCE_COLLECTIVES"] = "1"
    try:
        mono = m_g.capture_train_graph(o_g, z0, P, segmented=False, **draws[0])
        # default: segmented under (forced) collectives; bucket_min_elems=1: one graph per block (the tiny model's blocks
        # are far below the 16 M-element merge rule, which is exercised at real size in the B = 9 test below)
        seg = m_s.capture_train_graph(o_s, z0, P, bucket_min_elems=1, **draws[0])
        assert seg.segmented and not mono.segmented
        n_levels = len(cases.TINY_UNET["block_out_channels"])
        blocks = [b for _, bs in seg.segments for b in bs]
        assert all(len(bs) == 1 for _, bs in seg.segments)
        assert blocks == [2 * n_levels + 2] + list(range(2 * n_levels + 1, -1, -1)), blocks
        assert float(o_s.grad.abs().max()) == 0.0 and o_s.step_count == 0
        from consistencytta_amd import dist_util as du
        for it, kw in enumerate(draws):
            with torch.no_grad():
                loss, pred, target, sig, gamma = m_e._forward_impl(z0, None, P, False, True, kw["time_inds"],
                                                                   kw["gaussian_noise"], kw["guidance_scale"], True)
                m_e._student_backward(pred, target, sig, gamma, 1.0, None)
            mono._refresh(z0, kw["time_inds"], kw["gaussian_noise"], kw["guidance_scale"])
            mono.replay()
            seg._refresh(z0, kw["time_inds"], kw["gaussian_noise"], kw["guidance_scale"])
            buckets = du.GradientBuckets(o_s.grad, m_s.student_unet.block_ranges(), min_elems=1)
            assert buckets.enabled
            seen = []
            seg.replay(lambda b: (seen.append(b), buckets.ready(b)))
            assert buckets.wait() == 1 and seen == blocks
            torch.cuda.synchronize()
            l_e, l_g, l_s = float(loss), float(mono.loss.item()), float(seg.loss.item())
            r_g = float((o_e.grad - o_g.grad).norm() / o_e.grad.norm())
            r_s = float((o_e.grad - o_s.grad).norm() / o_e.grad.norm())
            print("draw %d: loss eager %.9g mono %.9g segmented %.9g; gradient rel diff mono %.2e segmented %.2e"
                  % (it, l_e, l_g, l_s, r_g, r_s))
            assert l_e == l_g == l_s and np.isfinite(l_e)
            assert float(o_e.grad.norm()) > 0 and r_g <= 1e-7 and r_s <= 1e-7
            for o in (o_e, o_g, o_s):
                o.zero_grad()
        # the public entry point: same parameters in, one optimizer step each
        before = o_e.flat.detach().clone()
        v_e = m_e.train_step(z0, P, o_e, None, **draws[1])
        v_s = seg.step(z0, None, **draws[1])
        torch.cuda.synchronize()
        assert v_e == v_s and o_s.step_count == o_e.step_count == 1
        d_e, d_s = o_e.flat - before, o_s.flat - before
        upd = float((d_e - d_s).norm() / d_e.norm())
        print("segmented step vs eager train_step: parameter update rel diff %.3e" % upd)
        assert upd <= 1e-3 and float(o_s.grad.abs().max()) == 0.0
        assert torch.equal(m_s.student_unet._flat, o_s.flat)
        with pytest.raises(N.CttaError, match="segmented=True"):
            mono.step(z0, None, **draws[0])
    finally:
        os.environ["CTTA_FORCE_COLLECTIVES"] = "0"
        if created:
            dist.destroy_process_group()


def test_pipelined_teacher_step_graph_equals_eager_on_a_sequence_of_batches(golden):
    """Round 4: `capture_train_graph(pipeline_teacher=True)` -- the frozen teacher's two CFG queries + Heun step of batch
    i + 1 run as their own hipGraph on a second stream beside the student / target / backward graph of batch i
    (audio_consistency_model.py:268-311 has no dependence on the student's weights).  Three DIFFERENT batches with
    different draws, fed one call ahead: every replayed micro-step must give the eager step's loss bit for bit and its
    gradient to the LayerNorm-atomics round-off -- i.e. the rotation of the input sets (one device copy) hands each
    batch's teacher outputs, timesteps, sigmas and guidance to the right main-graph replay.  Monolithic and segmented."""
    g = golden("distill_tiny")
    gen = torch.Generator().manual_seed(23)
    batches = []
    for i in range(4):
        batches.append(dict(z=(torch.randn(3, 8, 32, 8, generator=gen) * 0.9).to(DEV),
                            kw=dict(time_inds=torch.randint(0, 17, (3,), generator=gen) * 2,
                                    gaussian_noise=torch.randn(3, 8, 32, 8, generator=gen).to(DEV),
                                    guidance_scale=torch.rand(3, generator=gen) * 6)))
    batches[1]["kw"]["time_inds"][0] = 0           # pure-noise branch
    batches[2]["kw"]["time_inds"][1] = 32          # t_n = 0: the target is z_0 of THAT batch
    nets = ("student_unet", "student_target_unet", "student_ema_unet")
    for segmented in (False, True):
        m1, P, _ = _lcm()
        m1.train()
        o1 = m1.prepare_training(lr=1e-4, weight_decay=1e-4, broadcast=False)
        m2, _, _ = _lcm()
        m2.train()
        o2 = m2.prepare_training(lr=1e-4, weight_decay=1e-4, broadcast=False)
        gs = m2.capture_train_graph(o2, batches[3]["z"], P, segmented=segmented, pipeline_teacher=True, bucket_min_elems=1,
                                    **batches[3]["kw"])
        assert gs.pipelined and gs.teacher_graph is not None and float(o2.grad.abs().max()) == 0.0
        assert gs.feed(batches[0]["z"], **batches[0]["kw"]) is False            # primes the pipeline
        for i in range(3):
            b = batches[i]
            for name in nets:
                getattr(m2, name)._flat.copy_(getattr(m1, name)._flat)
                getattr(m2, name).mark_weights_changed()
            with torch.no_grad():
                loss, pred, target, sig, gamma = m1._forward_impl(b["z"], None, P, False, True, b["kw"]["time_inds"],
                                                                  b["kw"]["gaussian_noise"], b["kw"]["guidance_scale"], True)
                m1._student_backward(pred, target, sig, gamma, 1.0, None)
            assert gs.feed(batches[i + 1]["z"], **batches[i + 1]["kw"]) is True  # batch i becomes current, i + 1 goes to the teacher
            gs.replay()
            torch.cuda.synchronize()
            l_e, l_g = float(loss), float(gs.loss.item())
            rel = float((o1.grad - o2.grad).norm() / o1.grad.norm())
            print("%s, batch %d: eager loss %.9g pipelined %.9g, gradient rel diff %.2e"
                  % ("segmented" if segmented else "monolithic", i, l_e, l_g, rel))
            assert l_e == l_g and np.isfinite(l_e) and rel <= 1e-7
            for o, m in ((o1, m1), (o2, m2)):
                o.step(grad_scale=1.0)
                o.zero_grad()
                m.update_ema()
        # the public entry point: `step(z_next)` trains on the batch fed before (batch 3 here) and queues z_next
        for name in nets:
            getattr(m2, name)._flat.copy_(getattr(m1, name)._flat)
            getattr(m2, name).mark_weights_changed()
        v1 = m1.train_step(batches[3]["z"], P, o1, None, **batches[3]["kw"])
        v2 = gs.step(batches[0]["z"], None, **batches[0]["kw"])
        assert v1 == v2 and o1.step_count == o2.step_count == 4
        torch.cuda.synchronize()
        del gs


def test_pipelined_step_trains_every_batch_once_with_feed_and_drain(golden):
    """the reference trains every batch exactly once (tools/train_utils.py:150-183).  With the pipelined
    teacher, `feed(b0); step(b1); step(b2); drain()` is that loop: the losses are the eager `train_step` losses of
    b0, b1, b2 in order (same draws, parameters evolving identically), `drain()` with nothing waiting returns None, and
    the pipeline can be primed again afterwards."""
    gen = torch.Generator().manual_seed(29)
    batches = []
    for i in range(3):
        batches.append(dict(z=(torch.randn(3, 8, 32, 8, generator=gen) * 0.9).to(DEV),
                            kw=dict(time_inds=torch.randint(0, 17, (3,), generator=gen) * 2,
                                    gaussian_noise=torch.randn(3, 8, 32, 8, generator=gen).to(DEV),
                                    guidance_scale=torch.rand(3, generator=gen) * 6)))
    m1, P, _ = _lcm()
    m1.train()
    o1 = m1.prepare_training(lr=1e-4, weight_decay=1e-4, broadcast=False)
    m2, _, _ = _lcm()
    m2.train()
    o2 = m2.prepare_training(lr=1e-4, weight_decay=1e-4, broadcast=False)
    gs = m2.capture_train_graph(o2, batches[0]["z"], P, segmented=False, pipeline_teacher=True, **batches[0]["kw"])
    assert gs.drain() is None                                   # nothing fed yet
    init = o1.flat.detach().clone()
    assert torch.equal(init, o2.flat)
    eager = [m1.train_step(b["z"], P, o1, None, **b["kw"]) for b in batches]
    got = []
    assert gs.feed(batches[0]["z"], **batches[0]["kw"]) is False
    got.append(gs.step(batches[1]["z"], None, **batches[1]["kw"]))     # trains on batch 0
    got.append(gs.step(batches[2]["z"], None, **batches[2]["kw"]))     # trains on batch 1
    got.append(gs.drain())                                               # trains on batch 2, feeds nothing
    torch.cuda.synchronize()
    print("eager losses", eager, "feed/step/step/drain losses", got)
    assert o1.step_count == o2.step_count == 3 and gs.drain() is None
    assert got[0] == eager[0]
    # later steps start from parameters that differ by AdamW's amplification of the LayerNorm-atomics round-off (a gradient
    # entry near zero may change sign: +-lr on that entry); the three batches' losses differ by 2.5x .. 18x, so 2e-3 tells
    # "the right batch" from "another batch" with a wide margin
    for a, b in zip(got[1:], eager[1:]):
        assert abs(a - b) <= 2e-3 * abs(b)
    d1, d2 = o1.flat - init, o2.flat - init
    upd = float((d1 - d2).norm() / d1.norm())
    print("three optimizer steps, eager vs feed/step/step/drain: parameter update rel diff %.3e" % upd)
    assert upd <= 5e-2
    assert gs.feed(batches[0]["z"], **batches[0]["kw"]) is False    # a fresh pipeline
    assert gs.drain() is not None
    del gs


def test_pipelined_teacher_with_eager_main_and_changing_prompts(golden):
    """Round 4: (i) a batch's TEXT STATES travel with it through the pipeline (double-buffered like the latents): three batches
    with three different prompt sets, fed one call ahead, give the eager step's loss bit for bit; (ii) `main_eager` -- only the
    teacher phase is a hipGraph, the rest of the step eager launches, the form the waveform-domain losses of configs[4] take
    (bench.py `perceptual_distill`) -- equals the eager `_forward_impl` + backward on every batch as well (loss bit-identical,
    gradient to round-off); exercised here with the latent-space loss so that the comparison is exact."""
    cfg = cases.TINY_UNET
    gen = torch.Generator().manual_seed(41)
    batches = []
    for i in range(4):
        batches.append(dict(z=(torch.randn(3, 8, 32, 8, generator=gen) * 0.9).to(DEV),
                            P={k: v.to(DEV) for k, v in cases.prompt_states(cfg, 3, 6, "pp%d" % i).items()},
                            kw=dict(time_inds=torch.randint(0, 17, (3,), generator=gen) * 2,
                                    gaussian_noise=torch.randn(3, 8, 32, 8, generator=gen).to(DEV),
                                    guidance_scale=torch.rand(3, generator=gen) * 6)))
    nets = ("student_unet", "student_target_unet", "student_ema_unet")
    for eager_main in (False, True):
        m1, _, _ = _lcm()
        m1.train()
        o1 = m1.prepare_training(lr=1e-4, weight_decay=1e-4, broadcast=False)
        m2, _, _ = _lcm()
        m2.train()
        o2 = m2.prepare_training(lr=1e-4, weight_decay=1e-4, broadcast=False)
        gs = m2.capture_train_graph(o2, batches[3]["z"], batches[3]["P"], segmented=False, pipeline_teacher=True,
                                    main_eager=eager_main, **batches[3]["kw"])
        assert gs.main_eager == eager_main and (gs.graph is None) == eager_main
        assert gs.feed(batches[0]["z"], prompt=batches[0]["P"], **batches[0]["kw"]) is False
        for i in range(3):
            b = batches[i]
            for name in nets:
                getattr(m2, name)._flat.copy_(getattr(m1, name)._flat)
                getattr(m2, name).mark_weights_changed()
            with torch.no_grad():
                loss, pred, target, sig, gamma = m1._forward_impl(b["z"], None, b["P"], False, True, b["kw"]["time_inds"],
                                                                  b["kw"]["gaussian_noise"], b["kw"]["guidance_scale"], True)
                m1._student_backward(pred, target, sig, gamma, 1.0, None)
            assert gs.feed(batches[i + 1]["z"], prompt=batches[i + 1]["P"], **batches[i + 1]["kw"]) is True
            gs.replay()
            torch.cuda.synchronize()
            rel = float((o1.grad - o2.grad).norm() / o1.grad.norm())
            print("main_eager=%s, batch %d: eager loss %.9g pipelined %.9g, gradient rel diff %.2e"
                  % (eager_main, i, float(loss), float(gs.loss.item()), rel))
            assert float(loss) == float(gs.loss.item()) and rel <= 1e-7
            for o, m in ((o1, m1), (o2, m2)):
                o.step(grad_scale=1.0)
                o.zero_grad()
                m.update_ema()
        del gs


def test_step_graph_with_a_fixed_teacher_guidance_scale_equals_eager(golden):
    """with teacher_guidance_scale = 3 the eager `_forward_impl` conditions student and target on
    w = 3 (audio_consistency_model.py:300-311: the random draw exists only for scale -1); the captured step must do the
    same whatever `guidance_scale` the caller passes."""
    g = golden("distill_tiny")
    kw = dict(time_inds=torch.from_numpy(g["time_inds"]) * 2, gaussian_noise=torch.from_numpy(g["noise"]).to(DEV))
    pair = []
    for _ in range(2):
        m, P, z0 = _lcm()
        m.teacher_guidance_scale = 3
        m.train()
        pair.append((m, m.prepare_training(lr=1e-4, weight_decay=1e-4, broadcast=False)))
    (m1, o1), (m2, o2) = pair
    gs = m2.capture_train_graph(o2, z0, P, segmented=False, guidance_scale=torch.from_numpy(g["guidance"]), **kw)
    with torch.no_grad():
        loss, pred, target, sig, gamma = m1._forward_impl(z0, None, P, False, True, kw["time_inds"], kw["gaussian_noise"],
                                                          None, True)
        m1._student_backward(pred, target, sig, gamma, 1.0, None)
    gs._refresh(z0, kw["time_inds"], kw["gaussian_noise"], torch.from_numpy(g["guidance"]))   # a draw the model must ignore
    gs.replay()
    torch.cuda.synchronize()
    assert float(gs.w.min()) == float(gs.w.max()) == 3.0
    rel = float((o1.grad - o2.grad).norm() / o1.grad.norm())
    print("fixed w = 3: eager loss %.9g graph loss %.9g, gradient rel diff %.2e" % (float(loss), float(gs.loss.item()), rel))
    assert float(loss) == float(gs.loss.item()) and rel <= 1e-7


def test_gradient_accumulation_matches_one_big_step(golden):
    """accumulation_steps=2 with the same micro-batch twice: the accumulated, 1/2-scaled gradient equals the single
    micro-step gradient, so the parameters after the boundary step equal those of a plain step (up to bf16 rounding of
    the scaled loss gradient), and nothing moves before the boundary."""
    g = golden("distill_tiny")
    kw = dict(time_inds=torch.from_numpy(g["time_inds"]) * 2, gaussian_noise=torch.from_numpy(g["noise"]).to(DEV),
              guidance_scale=torch.from_numpy(g["guidance"]))
    m1, P, z0 = _lcm()
    m1.train()
    o1 = m1.prepare_training(lr=1e-4, weight_decay=0.0, broadcast=False)
    before = o1.flat.detach().clone()
    m1.train_step(z0, P, o1, None, **kw)
    m2, _, _ = _lcm()
    m2.train()
    o2 = m2.prepare_training(lr=1e-4, weight_decay=0.0, broadcast=False)
    m2.train_step(z0, P, o2, None, accumulation_steps=2, **kw)
    torch.cuda.synchronize()
    assert torch.equal(o2.flat, before) and float(o2.grad.abs().max()) > 0      # no update, gradients kept
    ema_before = m2.student_ema_unet._flat.detach().clone()
    m2.train_step(z0, P, o2, None, accumulation_steps=2, **kw)
    torch.cuda.synchronize()
    assert float(o2.grad.abs().max()) == 0.0 and not torch.equal(m2.student_ema_unet._flat, ema_before)
    d1, d2 = (o1.flat - before), (o2.flat - before)
    rel = float((d1 - d2).norm() / d1.norm())
    print("accumulated (2 x 1/2) vs single step: relative difference of the parameter update %.3e" % rel)
    assert rel < 5e-2        # AdamW's first step is lr*sign-like: tiny gradient differences flip a few near-zero elements


def test_fused_accumulation_one_big_micro_batch_equals_the_accumulated_micro_steps(golden):
    """Round 4 (bench.py `grad_accum_5_fused`): train.sh accumulates 5 micro-batches of 9 per optimizer step because the
    reference's GPUs cannot hold more; with 288 GB the same 45 samples run as ONE micro-batch.  Same samples, same
    per-sample draws: the loss is the mean of the micro-losses and the gradient AdamW consumes is the accumulated one up
    to fp32 / bf16 summation order (a sample's forward does not depend on its batch mates; the loss is a batch mean)."""
    gen = torch.Generator().manual_seed(31)
    cfg = cases.TINY_UNET
    n_micro, b = 3, 2
    Pbig = {k: v.to(DEV) for k, v in cases.prompt_states(cfg, n_micro * b, 6, "fusedacc").items()}
    zbig = (torch.randn(n_micro * b, 8, 32, 8, generator=gen) * 0.9).to(DEV)
    draws = dict(time_inds=torch.randint(0, 17, (n_micro * b,), generator=gen) * 2,
                 gaussian_noise=torch.randn(n_micro * b, 8, 32, 8, generator=gen).to(DEV),
                 guidance_scale=torch.rand(n_micro * b, generator=gen) * 6)

    def shard(i):
        lo, hi = i * b, (i + 1) * b
        n = n_micro * b
        P = {"embeds_cf": torch.cat([Pbig["embeds_cf"][:n][lo:hi], Pbig["embeds_cf"][n:][lo:hi]]),
             "mask_cf": torch.cat([Pbig["mask_cf"][:n][lo:hi], Pbig["mask_cf"][n:][lo:hi]]),
             "embeds": Pbig["embeds"][lo:hi], "mask": Pbig["mask"][lo:hi]}
        return P, zbig[lo:hi], {k: v[lo:hi] for k, v in draws.items()}

    seen = {}

    def run(fused):
        m, _, _ = _lcm()
        m.train()
        opt = m.prepare_training(lr=1e-4, weight_decay=0.0, broadcast=False)
        orig = opt.step

        def step(grad_scale=1.0):
            seen[fused] = opt.grad.detach().clone()
            return orig(grad_scale=grad_scale)
        opt.step = step
        if fused:
            losses = [m.train_step(zbig, Pbig, opt, None, **draws)]
        else:
            losses = []
            for i in range(n_micro):
                P, z, kw = shard(i)
                losses.append(m.train_step(z, P, opt, None, accumulation_steps=n_micro, **kw))
        torch.cuda.synchronize()
        return float(np.mean(losses))

    l_acc, l_fused = run(False), run(True)
    rel = float((seen[True] - seen[False]).norm() / seen[False].norm())
    print("accumulated %d x %d vs one batch of %d: loss %.7f vs %.7f, gradient rel diff %.3e" % (n_micro, b, n_micro * b, l_acc, l_fused, rel))
    assert abs(l_acc - l_fused) <= 1e-5 * abs(l_acc)
    assert rel <= 1e-2        # the micro-steps round (1/n) * dL/dpred to bf16 per micro-batch, the fused step rounds dL/dpred of the batch mean


def test_real_training_step_from_waveforms(golden):
    """The reference's inner loop end to end (tools/train_utils.py:150-183): waveforms -> wav_to_fbank -> VAE
    encode_first_stage -> get_first_stage_encoding -> distillation step, all on the HIP path."""
    import make_golden_mel as mg
    from consistencytta_amd import audio
    m, P, _ = _lcm()
    dd = cases.TINY_VAE_DD
    vae = modules.AutoencoderKL(ddconfig=dd, embed_dim=8, scale_factor=0.9227914214134216,
                                hifigan_config=cases.TINY_HIFIGAN)
    sd = dict(cases.vae_weights(dd))
    sd.update(cases.vae_encoder_weights(dd))
    sd.update(cases.hifigan_weights(cases.TINY_HIFIGAN))
    vae.load_state_dict(sd)
    vae.to(DEV).eval().requires_grad_(False)
    stft = audio.TacotronSTFT(1024, 160, 1024, 32, 16000, 0, 8000).to(DEV)     # 32 mel bins -> latent (B, 8, 32, 8)
    wav = mg.test_wave(3, 20320, "train_wav").nan_to_num().clip(-1, 1)
    with torch.no_grad():
        mel, _ = audio.wav_to_fbank(wav, 128, stft)
        z0 = vae.get_first_stage_encoding(vae.encode_first_stage(mel.unsqueeze(1)))
    assert tuple(z0.shape) == (3, 8, 32, 8) and bool(torch.isfinite(z0).all())
    m.train()
    opt = m.prepare_training(lr=1e-5, weight_decay=1e-4, broadcast=False)
    before = opt.flat.detach().clone()
    loss = m.train_step(z0, P, opt, None)
    assert loss == loss and loss > 0 and not torch.equal(opt.flat, before)


# ------------------------------------------------------------------------------------------------
# Perceptual losses on the differentiable decode (tools/losses.py MelLoss / CLAPLoss path).
def _tiny_vae(scale_factor):
    from consistencytta_amd import modules
    v = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=scale_factor,
                              hifigan_config=cases.TINY_HIFIGAN)
    sd = dict(cases.vae_weights(cases.TINY_VAE_DD))
    sd.update(cases.hifigan_weights(cases.TINY_HIFIGAN))
    v.load_state_dict(sd)
    return v.to(DEV).eval().requires_grad_(False), sd


def test_mel_loss_against_reference_golden(golden):
    from consistencytta_amd import losses
    g = golden("melloss_tiny")
    vae, _ = _tiny_vae(float(g["scale_factor"]))
    pred = (cases.vae_inputs(2, 16, 16, "melloss.pred") * 0.5).to(DEV).requires_grad_(True)
    target = (cases.vae_inputs(2, 16, 16, "melloss.target") * 0.5).to(DEV)
    inst = losses.MelLoss(vae=vae, reduction="instance")(pred, target, None, None)
    (inst * torch.from_numpy(g["weights"]).to(DEV)).mean().backward()
    ref = torch.from_numpy(g["instance_loss"])
    assert float((inst.detach().cpu() - ref).abs().max()) <= 2e-2 * float(ref.abs().max())
    gr = torch.from_numpy(g["grad_pred"])
    rel = float((pred.grad.cpu() - gr).norm() / gr.norm())
    print("MelLoss d/d latent vs the reference's autograd: rel_l2 %.3e" % rel)
    assert rel <= 2.5e-2
    with pytest.raises(RuntimeError):
        losses.CLAPLoss(vae=vae)


def test_distillation_with_mel_loss_backward_matches_oracle_autograd(golden):
    """AudioLCM(loss_type='mel'): the loss graph runs student U-Net -> frozen VAE decoder (HIP backward) -> MelLoss;
    parameter gradients against torch autograd over the oracle with the reference's recorded random draws."""
    from consistencytta_amd.models import AudioLCM
    from oracle import distill
    g = golden("distill_tiny")
    sf = 0.9227914214134216
    vae, vsd = _tiny_vae(sf)
    cfg = cases.TINY_UNET
    m = AudioLCM(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                 unet_model_config_path="tiny_light.json", unet_config=cfg, snr_gamma=5.0, use_edm=True,
                 teacher_guidance_scale=-1, num_diffusion_steps=18, vae=vae, loss_type="mel",
                 target_ema_decay=0.95, ema_decay=0.999)
    m.teacher_unet.load_state_dict(cases.unet_weights(cfg, False, 0))
    m.student_unet.load_state_dict(cases.unet_weights(cfg, True, 1))
    m.student_target_unet.load_state_dict(cases.unet_weights(cfg, True, 2))
    m.student_ema_unet.load_state_dict(cases.unet_weights(cfg, True, 3))
    m.to(DEV)
    P = {k: v.to(DEV) for k, v in cases.prompt_states(cfg, 3, 6, "distill").items()}
    z0 = (cases.t(spec.det_uniform("distill.z0", (3, 8, 32, 8), 14)) * 0.9).to(DEV)
    m.train()
    draws = dict(time_inds=torch.from_numpy(g["time_inds"]) * 2, gaussian_noise=torch.from_numpy(g["noise"]).to(DEV),
                 guidance_scale=torch.from_numpy(g["guidance"]))
    loss = m(z0, None, P, **draws)
    assert loss.requires_grad
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad for k, p in m.student_unet.named_parameters() if p.requires_grad}
    assert all(p.grad is None for p in vae.parameters())

    # oracle
    student = {k: v.clone().requires_grad_(k != "guidance_proj.weight") for k, v in cases.unet_weights(cfg, True, 1).items()}
    n = distill.Nets(cfg, cases.unet_weights(cfg, False, 0), student, cases.unet_weights(cfg, True, 2),
                     cases.unet_weights(cfg, True, 3))
    Pc = cases.prompt_states(cfg, 3, 6, "distill")
    z0c = z0.cpu()
    noise, inds, w = torch.from_numpy(g["noise"]), torch.from_numpy(g["time_inds"]) * 2, torch.from_numpy(g["guidance"])
    with torch.no_grad():
        ts, sig = distill._tables()
        z_np1_scaled, t_np1, zhat, zhat_scaled, t_n, s_np1 = distill._teacher_two_queries(n, Pc, z0c, noise, inds, w, ts, sig)
        target = onets.unet_forward(cfg, n.target, zhat_scaled, t_n, w, Pc["embeds"], Pc["mask"])
        target = torch.where((t_n == 0).reshape(-1, 1, 1, 1), z0c, target)
    pred = onets.unet_forward(cfg, student, z_np1_scaled, t_np1, w, Pc["embeds"], Pc["mask"])
    inst = distill.mel_loss_instances(cases.TINY_VAE_DD, vsd, pred, target, sf)
    ref_loss = (inst * torch.clamp(s_np1.float() ** -2, max=5.0)).mean()
    ref_loss.backward()
    ref = {k: p.grad for k, p in student.items() if p.requires_grad}
    print("mel-loss distillation: loss %.6f (oracle %.6f)" % (float(loss), float(ref_loss)))
    assert abs(float(loss) - float(ref_loss)) <= 5e-2 * float(ref_loss)
    total, worst = _compare(grads, ref)
    assert np.isfinite(total) and total <= 1.5 * GRAD_REL_L2_ALL

    # one full optimizer step through the same path
    for p in m.student_unet.parameters():
        p.grad = None
    opt = m.prepare_training(lr=1e-5, weight_decay=1e-4, broadcast=False)
    before = m.student_unet.flatten_parameters_().clone()
    value = m.train_step(z0, P, opt, **draws)
    assert abs(value - float(ref_loss)) <= 5e-2 * float(ref_loss)
    assert float((m.student_unet.flatten_parameters_() - before).abs().max()) > 0


def test_multi_resolution_stft_loss_runs_through_the_differentiable_vocoder():
    """MultiResolutionSTFTLoss (tools/losses.py:187-256): latent -> mel -> waveform with allow_grad=True on the HIP
    engines, three STFT resolutions on csrc/stft_loss.hip.  Value against oracle/losses.py (torch.stft in float64, the
    reference's recipe) over the oracle's fp32 waveforms; the
    latent gradient must exist and be finite (its LeakyReLU-mask sensitivity is covered in test_engines_gpu.py)."""
    from consistencytta_amd import losses
    from oracle import nets
    sf = 0.9227914214134216
    vae, sd = _tiny_vae(sf)
    pred = (cases.vae_inputs(2, 16, 16, "stftloss.pred") * 0.5).to(DEV).requires_grad_(True)
    target = (cases.vae_inputs(2, 16, 16, "stftloss.target") * 0.5).to(DEV)
    crit = losses.MultiResolutionSTFTLoss(vae=vae, reduction="instance", factor_sc=0.1, factor_mag=0.1, factor_mse=.8).to(DEV)
    inst = crit(pred, target, None, None)
    inst.mean().backward()
    assert inst.shape == (2,) and torch.isfinite(inst).all()
    assert torch.isfinite(pred.grad).all() and float(pred.grad.abs().max()) > 0

    from oracle import losses as olosses
    with torch.no_grad():   # the oracle's fp32 decode + vocoder, then the reference's own torch.stft recipe
        wavs = [nets.mel_to_waveform(cases.TINY_HIFIGAN, sd, nets.vae_decode(cases.TINY_VAE_DD, sd, z.detach().cpu(), sf))[1]
                for z in (pred, target)]
        ref = olosses.multi_resolution_stft_loss(pred.detach().cpu(), target.cpu(), wavs[0], wavs[1], factor_sc=0.1,
                                                 factor_mag=0.1, factor_mse=.8)
    print("stft loss", inst.detach().cpu().numpy(), "oracle", ref.numpy())
    assert float((inst.detach().cpu() - ref).abs().max()) <= 5e-2 * float(ref.abs().max())


@pytest.mark.parametrize("loss_type", ["mel", "stft"])
def test_waveform_loss_step_as_a_replayed_graph_equals_the_eager_step(golden, loss_type):
    """`capture_train_graph(pipeline_teacher=True, main_eager=False)` with a waveform-domain loss (round 6; the CLAP form at the
    real widths is in tests/test_clap_gpu.py): the decode, the loss module and torch's backward through them are recorded in the
    main hipGraph.  At the toy size, for the two losses that need no CLAP towers: the replay gives the eager step's loss and
    the student's gradient, twice in a row."""
    from consistencytta_amd.models import AudioLCM
    g = golden("distill_tiny")
    vae, _ = _tiny_vae(0.9227914214134216)
    cfg = cases.TINY_UNET
    m = AudioLCM(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                 unet_model_config_path="tiny_light.json", unet_config=cfg, snr_gamma=5.0, use_edm=True,
                 teacher_guidance_scale=-1, num_diffusion_steps=18, vae=vae, loss_type=loss_type,
                 target_ema_decay=0.95, ema_decay=0.999)
    m.teacher_unet.load_state_dict(cases.unet_weights(cfg, False, 0))
    m.student_unet.load_state_dict(cases.unet_weights(cfg, True, 1))
    m.student_target_unet.load_state_dict(cases.unet_weights(cfg, True, 2))
    m.student_ema_unet.load_state_dict(cases.unet_weights(cfg, True, 3))
    m.to(DEV)
    m.train()
    P = {k: v.to(DEV) for k, v in cases.prompt_states(cfg, 3, 6, "distill").items()}
    # (the STFT loss runs the vocoder: 64 mel bins = a latent 16 wide; the mel loss keeps the fixture's 32 x 8 latent and draws)
    zs = (3, 8, 16, 16) if loss_type == "stft" else (3, 8, 32, 8)
    z0 = (cases.t(spec.det_uniform("distill.z0", zs, 14)) * 0.9).to(DEV)
    noise = torch.from_numpy(g["noise"]) if loss_type == "mel" else cases.t(spec.det_uniform("distill.noise16", zs, 15))
    kw = dict(time_inds=torch.from_numpy(g["time_inds"]) * 2, gaussian_noise=noise.to(DEV),
              guidance_scale=torch.from_numpy(g["guidance"]))
    opt = m.prepare_training(lr=1e-5, weight_decay=1e-4, broadcast=False)
    with torch.no_grad():
        loss, pred, target, sig, gamma = m._forward_impl(z0, None, P, False, True, kw["time_inds"], kw["gaussian_noise"],
                                                         kw["guidance_scale"], True)
        m._student_backward(pred, target, sig, gamma, 1.0, None)
    torch.cuda.synchronize()
    g_eager, l_eager = opt.grad.clone(), float(loss)
    opt.zero_grad()
    gs = m.capture_train_graph(opt, z0, P, segmented=False, pipeline_teacher=True, main_eager=False, **kw)
    assert gs.main_eager is False and gs.graph is not None
    assert gs.feed(z0, prompt=P, **kw) is False
    for rnd in range(2):
        assert gs.feed(z0, prompt=P, **kw) is True
        gs.replay()
        torch.cuda.synchronize()
        rel = float((opt.grad - g_eager).norm() / g_eager.norm())
        print("replayed %s-loss step %d: loss %.7f (eager %.7f), gradient rel diff %.2e" % (loss_type, rnd, float(gs.loss.item()), l_eager, rel))
        assert abs(float(gs.loss.item()) - l_eager) <= 1e-5 * abs(l_eager) and rel <= 1e-4
        opt.zero_grad()


# ------------------------------------------------------------------------------------------------
# The distillation step at the REAL widths (559 M-parameter light U-Nets, latent 8 x 256 x 16): loss and student
# gradients against the reference's own AudioLCM + torch autograd (tests/golden/make_golden_distill_light.py).
def _lcm_light(B, L, tag):
    from consistencytta_amd.models import AudioLCM
    cfg = spec.LIGHT_UNET_CONFIG
    m = AudioLCM(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                 unet_model_config_path="tango_diffusion_light.json", unet_config=cfg, snr_gamma=5.0, use_edm=True,
                 teacher_guidance_scale=-1, num_diffusion_steps=18, vae=None, loss_type="mse",
                 target_ema_decay=0.95, ema_decay=0.999)
    m.teacher_unet.load_state_dict(cases.unet_weights(cfg, False, 0))
    m.student_unet.load_state_dict(cases.unet_weights(cfg, True, 1))
    m.student_target_unet.load_state_dict(cases.unet_weights(cfg, True, 2))
    m.student_ema_unet.load_state_dict(cases.unet_weights(cfg, True, 3))
    m.to(DEV)
    P = {k: v.to(DEV) for k, v in cases.prompt_states(cfg, B, L, tag).items()}
    z0 = (cases.t(spec.det_uniform(tag + ".z0", (B, 8, 256, 16), 14)) * 0.9).to(DEV)
    return m, P, z0


def _block_of(key):
    head, _, rest = key.partition(".")
    return head + "." + rest.split(".")[0] if head in ("down_blocks", "up_blocks") else head


def _fixture_grad_samples(g):
    """The strided gradient samples of a distill_light*.npz fixture, fp64 (stored as fp32, or as bfloat16 bit patterns)."""
    if "grad_samples_bf16" in g.files:
        return torch.from_numpy(g["grad_samples_bf16"]).view(torch.bfloat16).double().numpy()
    return g["grad_samples"].astype(np.float64)


def _check_student_grads(tag, m, g):
    """The student's gradients against a distill_light*.npz fixture: per block (`_block_of`) the relative L2 over the
    strided 512-entry samples <= GRAD_REL_L2_ALL, per tensor the deviation of the full norm <= GRAD_REL_L2."""
    sample_index = cases.sample_index
    names = [str(k) for k in g["grad_names"]]
    params = dict(m.student_unet.named_parameters())
    assert names == [k for k, p in params.items() if p.requires_grad]
    off, samples, norms = g["grad_offsets"], _fixture_grad_samples(g), g["grad_norms"]
    blocks, worst_norm = {}, ("", 0.0)
    for i, k in enumerate(names):
        gr = params[k].grad.detach().reshape(-1)
        idx = torch.from_numpy(sample_index(gr.numel())).to(DEV)
        got = gr[idx].double().cpu().numpy()
        ref = samples[off[i]:off[i + 1]]
        b = blocks.setdefault(_block_of(k), [0.0, 0.0])
        b[0] += float(((got - ref) ** 2).sum())
        b[1] += float((ref ** 2).sum())
        nrel = abs(float(gr.double().norm()) - norms[i]) / max(norms[i], 1e-30)
        if nrel > worst_norm[1]:
            worst_norm = (k, nrel)
    tot_e = sum(b[0] for b in blocks.values())
    tot_n = sum(b[1] for b in blocks.values())
    for name, (e, n) in blocks.items():
        print("  %-28s sampled grad rel_l2 %.3e" % (name, (e / max(n, 1e-300)) ** 0.5))
    print("%s, all blocks: sampled rel_l2 %.3e ; worst per-tensor norm deviation %s %.3e"
          % (tag, (tot_e / tot_n) ** 0.5, worst_norm[0], worst_norm[1]))
    for name, (e, n) in blocks.items():
        assert (e / max(n, 1e-300)) ** 0.5 <= GRAD_REL_L2_ALL, (tag, name)
    assert worst_norm[1] <= GRAD_REL_L2, (tag, worst_norm)


def test_distillation_step_at_light_widths_matches_reference(golden):
    """`AudioLCM.forward` + backward at `tango_diffusion_light.json` widths (the code path the
    bench times: split-K deep-level GEMMs, wgrad scatter, 64x64 K/V tiles) vs the reference's loss and autograd
    gradients.  The fixture holds every tensor's gradient norm and a strided 512-entry sample of it; tolerances:
    loss 5e-2 relative, per-block sampled-gradient relative L2 4e-2, per-tensor norm 8e-2."""
    g = golden("distill_light")
    m, P, z0 = _lcm_light(2, 16, "distill_light")
    m.train()
    kw = dict(time_inds=torch.from_numpy(g["time_inds"]) * 2, gaussian_noise=torch.from_numpy(g["noise"]).to(DEV),
              guidance_scale=torch.from_numpy(g["guidance"]))
    loss = m(z0, None, P, **kw)
    ref_loss = float(g["train_loss"])
    print("light-width distillation loss hip %.6f ref %.6f" % (float(loss), ref_loss))
    assert abs(float(loss) - ref_loss) <= 5e-2 * ref_loss
    loss.backward()
    torch.cuda.synchronize()
    _check_student_grads("B=2 light eager", m, g)
    for name in ("teacher_unet", "student_target_unet", "student_ema_unet"):
        assert all(p.grad is None for p in getattr(m, name).parameters())


def test_distillation_step_b9_matches_reference_eager_and_pipelined_graph(golden):
    """BASELINE configs[3] at its benchmarked size (per-GPU batch 9, L = 32: stream-K and two-pass split-K on the deep
    levels, the ragged masks of a real batch) against the reference's own AudioLCM + autograd
    (`distill_light_b9.npz`, make_golden_distill_light.py --draw-seed): the random draws were injected into the
    reference and are rebuilt here from the seed (time indices 0 and 16 -- the `last_mask` branch and the largest index --
    guidance scales near 0 and near 6).  The eager step, then the pipelined-teacher graph (the form bench.py's
    distillation leg replays) on the same draws, at the bounds of the B = 2 test."""
    g = golden("distill_light_b9")
    B = 9
    ti, noise, u = cases.distill_draws(B, int(g["draw_seed"]))
    assert np.array_equal(ti.numpy(), g["time_inds"]), "injected draws changed: time indices"
    assert np.array_equal((u * 6).numpy(), g["guidance"]), "injected draws changed: guidance"
    assert abs(float(noise.double().sum()) - float(g["noise_sum"])) <= 1e-9 * float(noise.double().abs().sum()), \
        "injected draws changed: noise"
    assert 0 in ti and 16 in ti
    m, P, z0 = _lcm_light(B, 32, "distill_full")
    m.train()
    kw = dict(time_inds=ti * 2, gaussian_noise=noise.to(DEV), guidance_scale=u * 6)
    ref_loss = float(g["train_loss"])
    loss = m(z0, None, P, **kw)
    print("B=9 light distillation loss hip %.6f ref %.6f" % (float(loss), ref_loss))
    assert abs(float(loss) - ref_loss) <= 5e-2 * ref_loss
    loss.backward()
    torch.cuda.synchronize()
    _check_student_grads("B=9 light eager", m, g)
    opt = m.prepare_training(lr=1e-5, weight_decay=1e-4, broadcast=False)
    gs = m.capture_train_graph(opt, z0, P, segmented=False, pipeline_teacher=True, **kw)
    assert float(opt.grad.abs().max()) == 0.0
    gs.feed(z0, **kw)
    assert gs.feed(z0, **kw) is True                 # the first feed becomes the current set
    gs.replay()
    torch.cuda.synchronize()
    print("B=9 light distillation loss, pipelined-teacher graph %.6f ref %.6f" % (float(gs.loss.item()), ref_loss))
    assert abs(float(gs.loss.item()) - ref_loss) <= 5e-2 * ref_loss
    _check_student_grads("B=9 light pipelined-teacher graph", m, g)
    opt.zero_grad()
    del gs


def test_distillation_step_full_batch_is_deterministic_and_blockwise_exact():
    """BASELINE configs[3] at its real size (per-GPU batch 9, L = 32): two identical steps give bit-identical losses
    and gradients outside the LayerNorm affine atomics, and the block-wise (overlappable) backward equals the
    monolithic one, and the captured forms equal the eager step -- properties of the engine itself; the same size
    against the reference's own step is test_distillation_step_b9_matches_reference_eager_and_pipelined_graph."""
    m, P, z0 = _lcm_light(9, 32, "distill_full")
    m.train()
    gen = torch.Generator().manual_seed(5)
    kw = dict(time_inds=torch.randint(0, 17, (9,), generator=gen) * 2,
              gaussian_noise=torch.randn(9, 8, 256, 16, generator=gen).to(DEV),
              guidance_scale=torch.rand(9, generator=gen) * 6)
    opt = m.prepare_training(lr=1e-5, weight_decay=1e-4, broadcast=False)

    def grads(blockwise):
        opt.zero_grad()
        with torch.no_grad():
            loss, pred, target, sig, gamma = m._forward_impl(z0, None, P, False, True, kw["time_inds"],
                                                             kw["gaussian_noise"], kw["guidance_scale"], True)
            seen = []
            m._student_backward(pred, target, sig, gamma, 1.0, seen.append if blockwise else None)
        torch.cuda.synchronize()
        return float(loss), opt.grad.detach().clone(), seen

    l1, g1, _ = grads(False)
    l2, g2, _ = grads(False)
    l3, g3, seen = grads(True)
    assert np.isfinite(l1) and l1 == l2 == l3
    assert seen[0] == 10 and sorted(seen) == list(range(11))         # out head first, every block reported once
    ref = float(g1.norm())
    assert np.isfinite(ref) and ref > 0
    d12, d13 = float((g1 - g2).norm()) / ref, float((g1 - g3).norm()) / ref
    print("B=9 light: loss %.6f, |grad| %.4e, run-to-run rel diff %.2e, block-wise vs monolithic %.2e" % (l1, ref, d12, d13))
    # Only the LayerNorm gamma/beta fp32 atomics may differ in the last bit: 1.5e-8 measured with BOTH stream overlaps on
    # (the default: CTTA_TWO_STREAM / option "wgrad_stream").  The 1.5e-7..3.8e-7 once seen with a second hardware queue were the
    # v_pk_fma_f32 op_sel hazard (LABNOTES.md 5), gone since the library is built with -fno-slp-vectorize.
    assert d12 <= 1e-7 and d13 <= 1e-7
    # the hipGraph-captured step at THIS size (what bench.py times) against the eager one -- loss bit
    # for bit and the whole 559 M-element gradient, for the monolithic capture and for the segmented one (1 + 11 graphs,
    # the data-parallel form); a second, different draw checks that the static tensors are really refreshed.
    for segmented in (False, True):
        gs = m.capture_train_graph(opt, z0, P, segmented=segmented, **kw)
        assert float(opt.grad.abs().max()) == 0.0
        gen2 = torch.Generator().manual_seed(6)
        kw2 = dict(time_inds=torch.randint(0, 17, (9,), generator=gen2) * 2,
                   gaussian_noise=torch.randn(9, 8, 256, 16, generator=gen2).to(DEV),
                   guidance_scale=torch.rand(9, generator=gen2) * 6)
        for draw in (kw, kw2):
            opt.zero_grad()
            with torch.no_grad():
                loss, pred, target, sig, gamma = m._forward_impl(z0, None, P, False, True, draw["time_inds"],
                                                                 draw["gaussian_noise"], draw["guidance_scale"], True)
                m._student_backward(pred, target, sig, gamma, 1.0, None)
            torch.cuda.synchronize()
            g_e, l_e = opt.grad.detach().clone(), float(loss)
            opt.zero_grad()
            gs._refresh(z0, draw["time_inds"], draw["gaussian_noise"], draw["guidance_scale"])
            seen = []
            gs.replay(seen.append if segmented else None)
            torch.cuda.synchronize()
            d = float((opt.grad - g_e).norm() / g_e.norm())
            print("B=9 light, %s graph: loss %.9g vs eager %.9g, gradient rel diff %.2e"
                  % ("segmented" if segmented else "monolithic", float(gs.loss.item()), l_e, d))
            assert float(gs.loss.item()) == l_e and d <= 1e-7
            assert not segmented or (seen[0] == 10 and sorted(seen) == list(range(11)))
            # at this size the merge rule applies: out head + up3 + up2 share the first graph, then one graph per bucket
            assert not segmented or [bs for _, bs in gs.segments] == [(10, 9, 8), (7,), (6,), (5,), (4,), (3,), (2,), (1, 0)]
        opt.zero_grad()
        del gs
    # the PIPELINED teacher (the form bench.py's headline distillation number runs) at this size --
    # the whole gradient against the eager step, for both draws fed one call ahead
    gs = m.capture_train_graph(opt, z0, P, segmented=False, pipeline_teacher=True, **kw)
    gs.feed(z0, **kw)
    for draw, nxt in ((kw, kw2), (kw2, kw)):
        torch.cuda.synchronize()     # the eager reference below uses the SAME teacher handle as the teacher graph in flight
        opt.zero_grad()
        with torch.no_grad():
            loss, pred, target, sig, gamma = m._forward_impl(z0, None, P, False, True, draw["time_inds"],
                                                             draw["gaussian_noise"], draw["guidance_scale"], True)
            m._student_backward(pred, target, sig, gamma, 1.0, None)
        torch.cuda.synchronize()
        g_e, l_e = opt.grad.detach().clone(), float(loss)
        opt.zero_grad()
        assert gs.feed(z0, **nxt) is True           # `draw` becomes the current set, `nxt` goes to the teacher stream
        gs.replay()
        torch.cuda.synchronize()
        d = float((opt.grad - g_e).norm() / g_e.norm())
        print("B=9 light, pipelined teacher: loss %.9g vs eager %.9g, gradient rel diff %.2e" % (float(gs.loss.item()), l_e, d))
        assert float(gs.loss.item()) == l_e and d <= 1e-7
    opt.zero_grad()
    del gs
