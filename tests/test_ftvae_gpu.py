"""Fine-tuning the VAE decoder on the HIP path (AudioLCM_FTVAE): the decoder's parameter gradients against torch autograd
over the CPU oracle, the in-place weight reload of the decoder handle, and the training step that moves U-Net and decoder
together."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
from consistencytta_amd import modules, optim, spec  # noqa: E402
from gpu_util import DEV, det, rel_l2  # noqa: E402
from oracle import nets as onets  # noqa: E402

# the project's gradient contract (tests/test_train_gpu.py)
GRAD_REL_L2 = 8e-2
GRAD_REL_L2_ALL = 4e-2
MEL_REL_L2 = 2.5e-2
SCALE = 0.9
DEC = ("decoder.", "post_quant_conv.")
# gradients that are zero in exact arithmetic: softmax shift invariance; biases in front of a GroupNorm with one channel per
# group (ch = 32)
ZERO_GRADS = {"decoder.mid.attn_1.k.bias", "decoder.up.0.block.0.nin_shortcut.bias"} | {
    "decoder.up.0.block.%d.conv%d.bias" % (b, c) for b in range(3) for c in (1, 2)}


def _vae(trainable, sd=None, encoder=False):
    vsd = dict(cases.vae_weights(cases.TINY_VAE_DD)) if sd is None else dict(sd)
    if encoder:
        vsd.update(cases.vae_encoder_weights(cases.TINY_VAE_DD))
    vsd.update(cases.hifigan_weights(cases.TINY_HIFIGAN))
    vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=SCALE, hifigan_config=cases.TINY_HIFIGAN)
    vae.load_state_dict(vsd)
    vae.to(DEV).eval().requires_grad_(False)
    if trainable:
        vae.train_decoder_()
    return vae, vsd


def rms(t):
    return float(t.detach().double().pow(2).mean().sqrt())


def _oracle_grads(z):
    vsd = dict(cases.vae_weights(cases.TINY_VAE_DD))
    params = {k: v.clone().requires_grad_(k.startswith(DEC)) for k, v in vsd.items()}
    zo = z.clone().requires_grad_(True)
    mel = onets.vae_decode(cases.TINY_VAE_DD, params, zo, SCALE)
    direction = cases.t(spec.det_uniform("vae_grad.dir", tuple(mel.shape), 9))
    (mel * direction).sum().backward()
    grads = {k: p.grad.detach() for k, p in params.items() if k.startswith(DEC)}
    return z, direction, mel.detach(), grads, zo.grad.detach()


@pytest.fixture(scope="module")
def oracle_grads():
    """(z, direction, mel, {name: gradient}, grad_z) of loss = (mel * direction).sum() under torch autograd on the CPU oracle."""
    return _oracle_grads(cases.vae_inputs(2, 16, 16, "vae_grad"))


def _check_grads(got, ref, tiny, med, factor, what):
    num = den = 0.0
    worst = ("", 0.0)
    for k, r in ref.items():
        g, r = got[k], r * factor
        assert g.shape == r.shape and torch.isfinite(g).all(), k
        if k in tiny:
            assert rms(g) <= 2.5e-2 * med * factor, (what, k, rms(g))
        else:
            e = rel_l2(g, r)
            worst = max(worst, (k, e), key=lambda t: t[1])
            assert e <= GRAD_REL_L2, (what, k, e)
        num += float((g.double() - r.double()).norm()) ** 2
        den += float(r.double().norm()) ** 2
    print("%s: worst tensor %s %.3e, whole %.3e" % (what, worst[0], worst[1], (num / den) ** 0.5))
    assert (num / den) ** 0.5 <= GRAD_REL_L2_ALL


def test_decoder_parameter_gradients_match_the_oracle(oracle_grads):
    z, direction, mel_ref, ref, gz_ref = oracle_grads
    assert len(ref) == 114
    med = float(np.median([rms(g) for g in ref.values()]))
    tiny = {k for k, g in ref.items() if rms(g) < 1e-3 * med}
    assert tiny == ZERO_GRADS, sorted(tiny ^ ZERO_GRADS)

    vae, _ = _vae(True)
    frozen = {k for k, p in vae.named_parameters() if not p.requires_grad}
    assert all(not k.startswith(DEC) for k in frozen) and any(k.startswith("vocoder.") for k in frozen)
    zd = z.to(DEV).requires_grad_(True)
    mel = vae.decode_first_stage(zd, allow_grad=True)
    assert type(mel.grad_fn).__name__ == "_VaeDecodeWithParamGradBackward"
    err_mel = rel_l2(mel, mel_ref)
    (mel * direction.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    got = {k: p.grad.detach().cpu().clone() for k, p in vae.named_parameters() if k.startswith(DEC)}
    gz = zd.grad.detach().clone()

    def check(got, factor, what):
        _check_grads(got, ref, tiny, med, factor, what)

    print("mel rel_l2 %.3e, grad_z rel_l2 %.3e" % (err_mel, rel_l2(gz, gz_ref)))
    assert err_mel <= MEL_REL_L2
    check(got, 1.0, "first backward")
    assert all(p.grad is None for k, p in vae.named_parameters() if not k.startswith(DEC))

    # a second forward / backward ACCUMULATES; a latent that does not require grad still reaches the parameters
    mel2 = vae.decode_first_stage(z.to(DEV), allow_grad=True)
    (mel2 * direction.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    check({k: p.grad.detach().cpu() for k, p in vae.named_parameters() if k.startswith(DEC)}, 2.0, "accumulated")

    # the data gradient is the frozen decoder's, and a frozen decoder still takes that path
    fz, _ = _vae(False)
    zf = z.to(DEV).requires_grad_(True)
    melf = fz.decode_first_stage(zf, allow_grad=True)
    assert type(melf.grad_fn).__name__ == "_VaeDecodeWithGradBackward"
    (melf * direction.to(DEV)).sum().backward()
    assert torch.equal(melf.detach(), mel.detach())
    assert rel_l2(gz, zf.grad) <= 1e-6
    assert all(p.grad is None for p in fz.parameters())
    assert fz.decode_first_stage(z.to(DEV), allow_grad=True).grad_fn is None


def test_decoder_parameter_gradients_at_a_width_the_implicit_kernel_refuses():
    """Latent 16 x 12: widths 12, 24 and 48 are no powers of two, so every 3x3 layer -- the two upsampling ones with their
    input at half the extent, conv_in with its padded channels -- takes the im2col^T + conv_gemm + row-sum route of
    `vconv_wgrad`, and the arena is sized for it.  Same reference, same bounds as at 16 x 16."""
    from consistencytta_amd import _native as N
    assert N.lib().ctta_wgrad_implicit_supported(9, 32, 64, 48, 32, 32) == 0 and N.lib().ctta_wgrad_implicit_supported(9, 128, 16, 12, 128, 128) == 0
    z, direction, mel_ref, ref, gz_ref = _oracle_grads(cases.vae_inputs(2, 16, 12, "vae_grad12"))
    med = float(np.median([rms(g) for g in ref.values()]))
    tiny = {k for k, g in ref.items() if rms(g) < 1e-3 * med}
    assert tiny == ZERO_GRADS, sorted(tiny ^ ZERO_GRADS)
    vae, _ = _vae(True)
    zd = z.to(DEV).requires_grad_(True)
    mel = vae.decode_first_stage(zd, allow_grad=True)
    assert rel_l2(mel, mel_ref) <= MEL_REL_L2
    (mel * direction.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    _check_grads({k: p.grad.detach().cpu() for k, p in vae.named_parameters() if k.startswith(DEC)}, ref, tiny, med, 1.0, "16 x 12")
    fz, _ = _vae(False)
    zf = z.to(DEV).requires_grad_(True)
    (fz.decode_first_stage(zf, allow_grad=True) * direction.to(DEV)).sum().backward()
    assert rel_l2(zd.grad, zf.grad) <= 1e-6


def test_decoder_handle_reloads_weights_in_place():
    """ctta_vae_load_weights: after the parameters moved, the decode equals a freshly created handle's bit for bit and the
    handle is the same one; an optimizer step through raw pointers (FusedAdamW) is seen too."""
    vae, vsd = _vae(True)
    z = cases.vae_inputs(2, 16, 16, "vae_reload").to(DEV)
    mel0 = vae.decode_first_stage(z)
    h0 = vae._eng["vae"][0].h.value
    with torch.no_grad():
        for k, p in vae.named_parameters():
            if k.startswith(DEC):
                p.add_(0.05 * det("reload." + k, tuple(p.shape), 3).to(DEV))
    mel1 = vae.decode_first_stage(z)
    assert vae._eng["vae"][0].h.value == h0 and not torch.equal(mel1, mel0)
    fresh, _ = _vae(False, {k: p.detach().cpu() for k, p in vae.named_parameters() if k.startswith(DEC)})
    assert torch.equal(fresh.decode_first_stage(z), mel1)
    # the differentiable handle too, through an optimizer step
    opt = optim.FusedAdamW(vae, lr=1e-3, weight_decay=0.0)
    assert opt.n == sum(p.numel() for k, p in vae.named_parameters() if k.startswith(DEC))
    direction = det("reload.dir", tuple(mel1.shape), 4).to(DEV)
    (vae.decode_first_stage(z, allow_grad=True) * direction).sum().backward()
    hg = vae._eng["vae"][1].h.value
    before = opt.flat[:opt.n].clone()
    opt.step()
    opt.zero_grad()
    assert float((opt.flat[:opt.n] - before).abs().max()) > 0
    melg = vae.decode_first_stage(z, allow_grad=True)
    mel2 = vae.decode_first_stage(z)
    assert vae._eng["vae"][1].h.value == hg and vae._eng["vae"][0].h.value == h0
    fresh2, _ = _vae(False, {k: p.detach().cpu() for k, p in vae.named_parameters() if k.startswith(DEC)})
    want = fresh2.decode_first_stage(z)
    assert torch.equal(mel2, want) and torch.equal(melg.detach(), want) and not torch.equal(mel2, mel1)
    # the data-gradient packs and conv_out's fp32 taps were repacked too: grad_z through the reloaded handle is a fresh
    # handle's (the frozen path of a VAE built from the new weights)
    zr = z.clone().requires_grad_(True)
    (vae.decode_first_stage(zr, allow_grad=True) * direction).sum().backward()
    zq = z.clone().requires_grad_(True)
    (fresh2.decode_first_stage(zq, allow_grad=True) * direction).sum().backward()
    assert vae._eng["vae"][1].h.value == hg and rel_l2(zr.grad, zq.grad) <= 1e-6
    vae_old, _ = _vae(False, vsd)
    zo = z.clone().requires_grad_(True)
    (vae_old.decode_first_stage(zo, allow_grad=True) * direction).sum().backward()
    assert rel_l2(zr.grad, zo.grad) > 1e-4                  # ... and not the old weights'


# ------------------------------------------------------------------------------------------------ AudioLCM_FTVAE
def _ftvae(seeds=(1, 2, 3)):
    """The sizes of test_audiolcm_clap_finetune_step_runs_and_moves_the_student: tiny U-Net, VAE, HiFi-GAN and CLAP."""
    from consistencytta_amd import clap as C
    from consistencytta_amd.models import AudioLCM_FTVAE
    ucfg = cases.TINY_UNET
    clap = C.CLAP_Module(audio_cfg=dict(cases.TINY_HTSAT, spec_size=128), text_cfg=cases.TINY_ROBERTA,
                         clip_samples=3 * (64 * 160 + 32))
    clap.to(DEV)
    clap.model.init_random_(seed=3)
    vae, _ = _vae(False, encoder=True)
    m = AudioLCM_FTVAE(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                       unet_model_config_path="tiny_light.json", unet_config=ucfg, snr_gamma=5.0, use_edm=True,
                       teacher_guidance_scale=-1, num_diffusion_steps=18, vae=vae, loss_type="clap", clap_module=clap)
    m.teacher_unet.load_state_dict(cases.unet_weights(ucfg, False, 0))
    for net, seed in zip((m.student_unet, m.student_target_unet, m.student_ema_unet), seeds):
        net.load_state_dict(cases.unet_weights(ucfg, True, seed))
    m.to(DEV)
    m.train()
    B = 2
    P = {k: v.to(DEV) for k, v in cases.prompt_states(ucfg, B, 6, "ftvae").items()}
    P["clap_text_features"] = torch.nn.functional.normalize(det("ftvae.text", (B, 512), 4), dim=-1).to(DEV)
    z0 = (cases.t(spec.det_uniform("ftvae.z0", (B, 8, 16, 16), 14)) * 0.9).to(DEV)
    gt = (det("ftvae.gt", (B, 9000), 5) * 0.3).to(DEV)
    gen = torch.Generator().manual_seed(11)
    kw = dict(time_inds=torch.randint(2, 15, (B,), generator=gen) * 2,
              gaussian_noise=torch.randn(B, 8, 16, 16, generator=gen).to(DEV), guidance_scale=torch.rand(B, generator=gen) * 6)
    return m, P, z0, gt, kw


def _dec_flat(vae):
    return torch.cat([p.detach().reshape(-1) for k, p in vae.named_parameters() if k.startswith(DEC)]).clone()


def _ema_flat(m):
    return torch.cat([p.detach().reshape(-1) for mod in (m.ema_vae_decoder, m.ema_vae_pqconv) for p in mod.parameters()]).clone()


def test_ftvae_train_step_moves_unet_and_decoder_together():
    m, P, z0, gt, kw = _ftvae()
    vae = m.vae
    assert m.training and vae.decoder.training and not m.ema_vae_decoder.training and not vae.vocoder.training
    assert all(p.requires_grad for k, p in vae.named_parameters() if k.startswith(DEC))
    assert not any(p.requires_grad for mod in (m.ema_vae_decoder, m.ema_vae_pqconv) for p in mod.parameters())
    m.check_eval_mode()
    opt = m.prepare_training(lr=1e-4, weight_decay=0.0, broadcast=False)
    assert opt.vae_optimizer.n == _dec_flat(vae).numel()
    frozen0 = {k: p.detach().clone() for k, p in vae.named_parameters() if not k.startswith(DEC)}
    assert any(k.startswith("encoder.") for k in frozen0) and any(k.startswith("quant_conv.") for k in frozen0)
    dec0, ema0, stu0 = _dec_flat(vae), _ema_flat(m), opt.flat.detach().clone()
    assert torch.equal(dec0, ema0)
    v1 = m.train_step(z0, P, opt, None, gt_wav=gt, **kw)
    torch.cuda.synchronize()
    assert np.isfinite(v1) and v1 > 0
    dec1, ema1 = _dec_flat(vae), _ema_flat(m)
    moved = float((dec1 - dec0).abs().max())
    print("FTVAE step: loss %.5f, decoder max change %.3e, student max change %.3e" % (v1, moved, float((opt.flat - stu0).abs().max())))
    assert moved > 0 and float((opt.flat - stu0).abs().max()) > 0
    for lo, hi in ((0, dec0.numel() - 72), (dec0.numel() - 72, dec0.numel())):      # the decoder; post_quant_conv (64 + 8)
        assert float((dec1[lo:hi] - dec0[lo:hi]).abs().max()) > 0
    want = ema0 + (1.0 - m.ema_decay) * (dec1 - ema0)
    assert float((ema1 - want).abs().max()) <= 1e-6 * float(want.abs().max())
    for k, p in vae.named_parameters():
        if not k.startswith(DEC):
            assert torch.equal(p.detach(), frozen0[k]), k
    assert float(opt.vae_optimizer.grad.abs().max()) == 0.0             # zero_grad ran
    m.check_eval_mode()
    # use_ema decodes through the EMA copies, on a handle of their own
    z = cases.vae_inputs(2, 16, 16, "ftvae.ema").to(DEV)
    mel, mel_ema = vae.decode_first_stage(z), vae.decode_first_stage(z, use_ema=True)
    assert not torch.equal(mel, mel_ema)
    sd = {"decoder." + k: p.detach().cpu() for k, p in m.ema_vae_decoder.named_parameters()}
    sd.update({"post_quant_conv." + k: p.detach().cpu() for k, p in m.ema_vae_pqconv.named_parameters()})
    loaded, _ = _vae(False, sd)
    assert torch.equal(loaded.decode_first_stage(z), mel_ema)
    # a NaN loss: neither parameter set moves, both EMAs do
    stu1, ema_stu1 = opt.flat.detach().clone(), m.student_ema_unet._flat.detach().clone()
    bad = dict(kw, gaussian_noise=torch.full_like(kw["gaussian_noise"], float("nan")))
    v2 = m.train_step(z0, P, opt, None, gt_wav=gt, **bad)
    torch.cuda.synchronize()
    assert np.isnan(v2)
    assert torch.equal(_dec_flat(vae), dec1) and torch.equal(opt.flat, stu1)
    assert not torch.equal(_ema_flat(m), ema1) and not torch.equal(m.student_ema_unet._flat, ema_stu1)
    assert torch.isfinite(_ema_flat(m)).all() and float(opt.vae_optimizer.grad.abs().max()) == 0.0


def test_ftvae_loss_decreases_over_twenty_fixed_draw_steps():
    m, P, z0, gt, kw = _ftvae(seeds=(1, 1, 1))
    opt = m.prepare_training(lr=2e-4, weight_decay=0.0, broadcast=False)
    losses = [m.train_step(z0, P, opt, None, gt_wav=gt, **kw) for _ in range(20)]
    print("FTVAE clap loss over 20 fixed-draw steps: %.5f -> %.5f (min %.5f)" % (losses[0], losses[-1], min(losses)))
    assert all(np.isfinite(v) for v in losses)
    assert np.mean(losses[-3:]) < 0.9 * np.mean(losses[:3])


def test_ftvae_refuses_what_it_does_not_cover(monkeypatch):
    from consistencytta_amd import dist_util
    m, P, z0, gt, kw = _ftvae()
    opt = m.prepare_training(lr=1e-4, weight_decay=0.0, broadcast=False)
    with pytest.raises(NotImplementedError, match="FTVAE"):
        m.capture_train_graph(opt, z0, P)
    monkeypatch.setattr(dist_util.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist_util.dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="FTVAE"):
        m.train_step(z0, P, opt, None, gt_wav=gt, **kw)
    with pytest.raises(NotImplementedError, match="FTVAE"):
        m.prepare_training(lr=1e-4, broadcast=False)
