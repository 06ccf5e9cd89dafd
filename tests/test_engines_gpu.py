"""End-to-end parity of the HIP engines (through the nn.Module mirrors and the C ABI) against
(a) the committed fixtures produced by the reference's own modules and (b) the CPU oracle,
layer by layer via debug taps.

Tolerance contract (north_star: "within a stated fp32 mel-spectrogram tolerance"): the
engines compute in bf16 with fp32 accumulation (the reference's own GPU recipe is bf16
autocast, inference.py:190) and are compared with the reference's fp32 CPU outputs:
    relative L2 error  ||hip - ref|| / ||ref||  <=  REL_L2   and
    max abs error / max|ref|                   <=  REL_MAX
with the constants below.  Random-init networks (no checkpoint on either box) amplify bf16
round-off more than trained ones, so these bounds are conservative for real weights.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
from consistencytta_amd import _native as N, modules, scheduler, spec  # noqa: E402
from gpu_util import DEV, light_pipeline, rel_err, rel_l2, run_light_pipeline  # noqa: E402
from oracle import nets as onets  # noqa: E402

REL_L2 = 2.5e-2
REL_MAX = 6e-2


def _load(module, sd):
    module.load_state_dict({k: v for k, v in sd.items()})
    return module.to(DEV).eval().requires_grad_(False)


def _report(tag, got, ref):
    l2, mx = rel_l2(got, ref), rel_err(got, ref)
    print("%-40s rel_l2 %.3e  rel_max %.3e" % (tag, l2, mx))
    return l2, mx


def _check(tag, got, ref, l2_tol=REL_L2, max_tol=REL_MAX):
    l2, mx = _report(tag, got, ref)
    assert np.isfinite(l2) and l2 <= l2_tol and mx <= max_tol, "%s: rel_l2 %.3e rel_max %.3e" % (tag, l2, mx)


def test_unet_tiny_against_reference_golden_and_oracle_taps(golden):
    g = golden("unet_tiny")
    cfg = cases.TINY_UNET
    sd = cases.unet_weights(cfg, True)
    m = modules.UNet2DConditionGuidedModel.from_config(cfg)
    assert list(m.state_dict().keys()) == [str(k) for k in g["keys"]]   # reference key names AND order
    m.debug_taps = True
    _load(m, sd)
    x, ts, gs, enc, mask = cases.unet_inputs(cfg, 2, 32, 8, 7, "unet_tiny")
    out = m(x.to(DEV), ts.to(DEV), guidance=gs.to(DEV), encoder_hidden_states=enc.to(DEV),
            encoder_attention_mask=mask.to(DEV)).sample
    # layer-by-layer localisation against the oracle
    taps = {}
    with torch.no_grad():
        ref = onets.unet_forward(cfg, sd, x, ts, gs, enc, mask, taps=taps)
    worst = 0.0
    for name, t in m.read_taps().items():
        r = taps[name]
        if r.ndim == 2:
            r = r[:, :, None, None]
        l2, _ = _report("tap " + name, t, r)
        worst = max(worst, l2)
    assert worst <= REL_L2
    _check("unet_tiny vs oracle", out, ref)
    _check("unet_tiny vs reference golden", out, torch.from_numpy(g["guided"]))
    # scalar (Python float) timestep / guidance path, smaller extent -> new handle
    x2, _, _, enc2, mask2 = cases.unet_inputs(cfg, 2, 16, 8, 5, "unet_tiny_s", False)
    out2 = m(x2.to(DEV), 999.0, guidance=4.0, encoder_hidden_states=enc2.to(DEV),
             encoder_attention_mask=mask2.to(DEV)).sample
    _check("unet_tiny scalar t/w vs reference golden", out2, torch.from_numpy(g["guided_scalar"]))
    # teacher (no guidance branch); `guidance=` is swallowed like the reference's **kwargs
    mt = _load(modules.UNet2DConditionModel.from_config(cfg), cases.unet_weights(cfg, False))
    out3 = mt(x.to(DEV), ts.to(DEV), enc.to(DEV), encoder_attention_mask=mask.to(DEV), guidance=1.0).sample
    _check("teacher unet vs reference golden", out3, torch.from_numpy(g["teacher"]))


def test_unet_batch_independence_and_determinism():
    cfg = cases.TINY_UNET
    m = _load(modules.UNet2DConditionGuidedModel.from_config(cfg), cases.unet_weights(cfg, True))
    x, ts, gs, enc, mask = cases.unet_inputs(cfg, 4, 16, 8, 9, "unet_bi")
    args = dict(encoder_hidden_states=enc.to(DEV), encoder_attention_mask=mask.to(DEV))
    a = m(x.to(DEV), ts.to(DEV), guidance=gs.to(DEV), **args).sample
    b = m(x.to(DEV), ts.to(DEV), guidance=gs.to(DEV), **args).sample
    assert torch.equal(a, b)                                    # no atomics on the data path
    one = m(x[2:3].to(DEV), ts[2:3].to(DEV), guidance=gs[2:3].to(DEV), encoder_hidden_states=enc[2:3].to(DEV),
            encoder_attention_mask=mask[2:3].to(DEV)).sample
    assert torch.equal(one[0], a[2])                            # clips are independent: batch shards exactly


def test_unet_light_config1_against_reference_golden(golden):
    g = golden("unet_light")
    cfg = spec.LIGHT_UNET_CONFIG
    m = modules.UNet2DConditionGuidedModel.from_config(cfg)
    assert sum(p.numel() for p in m.parameters()) == int(g["n_params"])
    _load(m, cases.unet_weights(cfg, True))
    x, _, _, enc, mask = cases.unet_inputs(cfg, 1, 256, 16, 16, "unet_light", False)
    x = x / 1.7 * cases.SIGMA_MAX / ((cases.SIGMA_MAX ** 2 + 1) ** 0.5)
    out = m(x.to(DEV), 999.0, guidance=4.0, encoder_hidden_states=enc.to(DEV),
            encoder_attention_mask=mask.to(DEV)).sample
    _check("unet_light (559M params) vs reference golden", out, torch.from_numpy(g["out"]))


def _vae(dd, hcfg, taps=False):
    v = modules.AutoencoderKL(ddconfig=dd, embed_dim=8, scale_factor=1.0, hifigan_config=hcfg)
    sd = dict(cases.vae_weights(dd))
    sd.update(cases.hifigan_weights(hcfg))
    v.debug_taps = taps
    return _load(v, sd), sd


def test_vae_and_hifigan_tiny(golden):
    g = golden("vae_tiny")
    v, sd = _vae(cases.TINY_VAE_DD, cases.TINY_HIFIGAN, taps=True)
    v.scale_factor = float(g["scale_factor"])
    z = cases.vae_inputs(2, 16, 8, "vae_tiny")
    mel = v.decode_first_stage(z.to(DEV))
    taps = {}
    with torch.no_grad():
        ref = onets.vae_decode(cases.TINY_VAE_DD, sd, z, v.scale_factor, taps=taps)
    for name, t in v._read_taps("vae").items():
        _report("vae tap " + name, t, taps[name])
    _check("vae_tiny mel vs oracle", mel, ref)
    _check("vae_tiny mel vs reference golden", mel, torch.from_numpy(g["mel"]))
    mel_in = cases.mel_inputs(2, 24, 64, "hifigan_tiny")
    wav = v.vocode(mel_in.to(DEV))
    taps = {}
    with torch.no_grad():
        onets.hifigan_forward(cases.TINY_HIFIGAN, sd, mel_in.squeeze(1).permute(0, 2, 1), taps=taps)
    n_ups = len(cases.TINY_HIFIGAN["upsample_rates"])
    for name, t in v._read_taps("voc").items():
        if name.startswith("lrelu."):   # the engine stores leaky_relu(x) where x has no other consumer
            slope = 0.01 if name == "lrelu.stage.%d" % (n_ups - 1) else 0.1
            ref = torch.nn.functional.leaky_relu(taps[name[len("lrelu."):]], slope)
        else:
            ref = taps[name]
        l2, _ = _report("hifigan tap " + name, t.squeeze(2), ref)
        assert l2 <= REL_L2
    _check("hifigan_tiny wav vs reference golden", wav, torch.from_numpy(g["wav"]))
    pcm = v.decode_to_waveform(mel_in.to(DEV))
    assert pcm.dtype == np.int16 and pcm.shape == g["pcm"].shape
    scale = float(np.abs(g["pcm"].astype(np.int64)).max())
    assert np.abs(pcm.astype(np.int64) - g["pcm"].astype(np.int64)).max() <= REL_MAX * scale + 2


def test_vae_and_hifigan_full_width(golden):
    g = golden("vae_full")
    v, sd = _vae(spec.VAE_DDCONFIG, spec.HIFIGAN_16K_64)
    v.scale_factor = float(g["scale_factor"])
    mel = v.decode_first_stage(cases.vae_inputs(1, 64, 16, "vae_full").to(DEV))
    _check("vae full-width mel vs reference golden", mel, torch.from_numpy(g["mel"]))
    wav = v.vocode(cases.mel_inputs(1, 64, 64, "hifigan_full").to(DEV))
    assert wav.shape == g["wav"].shape
    _check("hifigan full-width wav vs reference golden", wav, torch.from_numpy(g["wav"]))


def test_scheduler_mirror_matches_reference_tables_and_steps(golden):
    g = golden("heun")
    s = scheduler.HeunDiscreteScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    for n in (1, 2, 18, 200):
        s.set_timesteps(n, device=DEV)
        assert np.array_equal(s.timesteps.cpu().numpy(), g["timesteps_%d" % n])
        # sigmas come from fp32 torch.linspace/cumprod on the HOST cpu: last-bit differences between
        # CPU models (FMA / vector width) are the reference's own, hence 1e-6 instead of equality
        np.testing.assert_allclose(s.sigmas.cpu().numpy(), g["sigmas_%d" % n], rtol=1e-6, atol=0)
        assert abs(float(s.init_noise_sigma) - float(g["init_sigma_%d" % n])) <= 1e-6 * float(g["init_sigma_%d" % n])
    s.set_timesteps(18, device=DEV)
    idx = torch.from_numpy(g["idx"])
    x = (cases.t(spec.det_uniform("heun.x", (3, 8, 16, 4), 1)) * 3).to(DEV)
    v1 = cases.t(spec.det_uniform("heun.v1", (3, 8, 16, 4), 2)).to(DEV)
    v2 = cases.t(spec.det_uniform("heun.v2", (3, 8, 16, 4), 3)).to(DEV)
    t_a, t_b = s.timesteps[idx], s.timesteps[idx + 2]
    assert rel_err(s.scale_model_input(x, t_a), torch.from_numpy(g["scaled"])) < 2e-6
    first = s.step(v1, t_a, x).prev_sample
    assert not s.state_in_first_order
    assert rel_err(first, torch.from_numpy(g["step1"])) < 2e-6
    assert rel_err(s.scale_model_input(first, t_b), torch.from_numpy(g["scaled2"])) < 2e-6
    second = s.step(v2, t_b, first).prev_sample
    assert s.state_in_first_order
    assert rel_err(second, torch.from_numpy(g["step2"])) < 8e-6


def test_pipeline_config1_end_to_end(golden):
    """BASELINE.json config 1 (easy_inference recipe, B=1, 1 step, w=4): latent, mel and
    waveform against the reference modules' outputs."""
    from consistencytta_amd.models import ConsistencyTTA
    g = golden("pipeline_light")
    cfg = spec.LIGHT_UNET_CONFIG
    v, _ = _vae(spec.VAE_DDCONFIG, spec.HIFIGAN_16K_64)
    v.scale_factor = float(g["scale_factor"])
    pipe = ConsistencyTTA(unet_config=cfg, vae=v)
    _load(pipe.unet, cases.unet_weights(cfg, True))
    _, _, _, enc, mask = cases.unet_inputs(cfg, 1, 256, 16, 16, "pipe", False)
    noise = cases.t(spec.det_uniform("pipe.noise", (1, 8, 256, 16), 9)) * np.float32(np.sqrt(3.0))
    lat = pipe.generate_latent(enc.to(DEV), mask.to(DEV), noise.to(DEV), cfg_scale_input=4.0, cfg_scale_post=1.0,
                               num_steps=1)
    _check("pipeline latent", lat, torch.from_numpy(g["latent"]))
    mel = v.decode_first_stage(lat)
    _check("pipeline mel (the north_star tolerance)", mel, torch.from_numpy(g["mel"]))
    wav = v.vocode(mel)
    assert wav.shape[1] == 163872
    ref_head = torch.from_numpy(g["wav_head"])
    _check("pipeline waveform head", wav[:, :ref_head.shape[1]], ref_head)
    assert bool(torch.isfinite(wav).all()) and float(wav.abs().max()) <= 1.0


def test_pipeline_batch32_shards_into_single_clip_runs(golden):
    """BASELINE.json configs[1] at its full size (batch 32, light U-Net + VAE decoder + HiFi-GAN, L=32 with ragged
    masks) through a size-independent property: every clip of the batch equals the same clip run alone (the shape
    the config-1 golden pins against the reference) -- clips are independent, so a batch shards over ranks with no
    data-path collective.  Tile shapes and split-K differ between M = 32 x 4096 and M = 4096, so the
    fp32 accumulation ORDER differs; on this random-init network any such change (split-K off, another tile, another
    batch size -- tools/order_noise.py) moves the bf16 result by the same 9.2e-3 relative L2 in the latent (1.9e-2
    mel, 1.6e-2 waveform): the bf16 rounding-noise floor, below the 1.2e-2 / 1.9e-2 distance to the fp32 reference.
    The tolerances are that floor with 2x margin; a replay of the batch itself is bit-exact."""
    pipe = light_pipeline(float(golden("pipeline_light")["scale_factor"]))
    X = cases.batch32_inputs()
    B = X["noise"].shape[0]

    def run(sel):
        return run_light_pipeline(pipe, X["enc"][sel], X["mask"][sel], X["noise"][sel])
    full = run(slice(0, B))
    again = run(slice(0, B))
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    assert full[2].shape == (B, 163872) and bool(torch.isfinite(full[2]).all())
    for i in (0, 17, 31):
        one = run(slice(i, i + 1))
        for tag, a, b, tol in (("latent", full[0][i:i + 1], one[0], 2e-2), ("mel", full[1][i:i + 1], one[1], 3e-2),
                               ("waveform", full[2][i:i + 1], one[2], 3e-2)):
            err = rel_l2(a.float().cpu(), b.float().cpu())
            print("clip %d %s: batch-32 vs alone rel_l2 %.2e" % (i, tag, err))
            assert err < tol, (i, tag, err)


# Per-clip outlier bound of the batch-32 test: on this random-init network the distance to the reference is the bf16
# rounding noise, statistically the same for every clip, and a 512-entry sample estimates a clip's relative L2 to about
# 5 % -- measured, the worst of the 32 clips is 1.10x the batch median in the latent and 1.11x in the mel.  A clip above
# 1.3x its batch mates' median has an error of its own: one valid token masked out of clip 17's 14 makes 1.80x in the
# latent and 1.49x in the mel, and no other clip moves.
OUTLIER = 1.3


def test_pipeline_batch32_against_reference_golden(golden):
    """BASELINE.json configs[1] at the size bench.py times (batch 32, L = 32, ragged masks: the 256x256x64 conv tile,
    the FFN GEGLU kernel, the eight-wave HiFi-GAN unit forms at 1024 mel frames) against the reference's own modules,
    clip by clip (tests/golden/make_golden_batch32.py).  The clips stored in full (rows 0 and 31 and the shortest mask)
    are checked at the REL_L2 / REL_MAX contract; every one of the 32 clips by the relative L2 of a
    512-entry strided sample and by its full norm, and by how far that distance stands out from the other clips' (OUTLIER),
    so an error confined to one row of the batch fails here; the int16
    output of decode_to_waveform (batch-global centring) at the stored positions within the bound of
    test_vae_and_hifigan_tiny."""
    g = golden("pipeline_batch32")
    X = cases.batch32_inputs()
    assert np.array_equal(X["lens"].numpy(), g["lens"]), "inputs changed: mask lengths"
    for k in ("enc", "noise"):
        got = float(X[k].double().sum())
        assert abs(got - float(g[k + "_sum"])) <= 1e-9 * float(X[k].double().abs().sum()), "inputs changed: " + k
    clips = [int(c) for c in g["clips"]]
    assert clips == cases.batch32_clips(g["lens"])
    pipe = light_pipeline(float(g["scale_factor"]))
    lat, mel, wav = run_light_pipeline(pipe, X["enc"], X["mask"], X["noise"])
    B = lat.shape[0]
    assert wav.shape == (B, 163872)
    head, stride = int(g["wav_head_len"]), int(g["wav_stride"])
    for j, b in enumerate(clips):
        tag = "batch32 clip %d (%d tokens)" % (b, int(g["lens"][b]))
        _check(tag + " latent", lat[b], torch.from_numpy(g["latent"][j].astype(np.float32)))
        _check(tag + " mel", mel[b], torch.from_numpy(g["mel"][j].astype(np.float32)))
        _check(tag + " waveform head", wav[b, :head], torch.from_numpy(g["wav_head"][j].astype(np.float32)))
        _check(tag + " waveform 1-in-%d" % stride, wav[b, ::stride], torch.from_numpy(g["wav_strided"][j].astype(np.float32)))
    worst, bad = {}, []
    for key, got in (("latent", lat), ("mel", mel), ("wav", wav)):
        l2s = []
        flat = got.reshape(B, -1).float()
        idx = torch.from_numpy(cases.sample_index(flat.shape[1])).to(DEV)
        sampled = flat[:, idx].double().cpu().numpy()
        ref = g[key + "_samples"].astype(np.float64)
        norms = flat.double().norm(dim=1).cpu().numpy()
        absmax = flat.abs().amax(dim=1).double().cpu().numpy()
        for b in range(B):
            l2 = float(np.linalg.norm(sampled[b] - ref[b]) / np.linalg.norm(ref[b]))
            dn = abs(norms[b] - g[key + "_norm"][b]) / g[key + "_norm"][b]
            dm = abs(absmax[b] - g[key + "_absmax"][b]) / g[key + "_absmax"][b]
            l2s.append(l2)
            if l2 > worst.get(key, (0, -1.0))[1]:
                worst[key] = (b, l2)
            if not (np.isfinite(l2) and l2 <= REL_L2 and dn <= REL_L2 and dm <= REL_MAX):
                bad.append("clip %d %s: sampled rel_l2 %.3e, norm deviation %.3e, absmax deviation %.3e" % (b, key, l2, dn, dm))
        med = float(np.median(l2s))
        print("batch32 %-6s sampled rel_l2 over the clips: median %.3e, worst %.3e (clip %d, %.2fx the median)"
              % (key, med, worst[key][1], worst[key][0], worst[key][1] / med))
        if key != "wav":     # the waveform's distance is mostly bf16 order noise of its own (the vocoder's), alike for all
            bad += ["clip %d %s: sampled rel_l2 %.3e is %.2fx the batch median %.3e" % (b, key, l2s[b], l2s[b] / med, med)
                    for b in range(B) if l2s[b] > OUTLIER * med]
    assert not bad, bad
    # decode_to_waveform: vocoder_infer's int16 with the batch-global (max + min) / 2 centre of all 32 clips
    pcm = pipe.vae.decode_to_waveform(mel)
    assert pcm.dtype == np.int16 and pcm.shape == (B, 163872)
    centre = np.float32(g["wav_centre"])

    def ref_pcm(w):
        return ((w.astype(np.float32) - centre) * np.float32(32768)).astype(np.int16).astype(np.int64)
    n = pcm.shape[1]
    pairs = [(pcm[:, cases.sample_index(n)], ref_pcm(g["wav_samples"]))]
    for j, b in enumerate(clips):
        pairs += [(pcm[b, :head], ref_pcm(g["wav_head"][j])), (pcm[b, ::stride], ref_pcm(g["wav_strided"][j]))]
    for got, ref in pairs:
        scale = float(np.abs(ref).max())
        err = float(np.abs(got.astype(np.int64) - ref).max())
        print("batch32 int16 waveform: max abs error %.0f of %.0f" % (err, scale))
        assert err <= REL_MAX * scale + 2


def test_vae_encoder_against_reference_golden_and_oracle_taps(golden):
    """AutoencoderKL.encode_first_stage / get_first_stage_encoding on the HIP encoder: posterior
    moments vs the reference's own fixture, layer by layer vs the oracle, and the sampled, scaled latent."""
    g = golden("vae_encoder_tiny")
    dd = cases.TINY_VAE_DD
    sd = dict(cases.vae_weights(dd))
    sd.update(cases.vae_encoder_weights(dd))
    sd.update(cases.hifigan_weights(cases.TINY_HIFIGAN))
    v = modules.AutoencoderKL(ddconfig=dd, embed_dim=8, scale_factor=float(g["scale_factor"]),
                              hifigan_config=cases.TINY_HIFIGAN)
    v.debug_taps = True
    _load(v, sd)
    mel = cases.mel_inputs(2, 64, 16, "vaeenc_tiny") * 2.0 - 4.0
    post = v.encode_first_stage(mel.to(DEV))
    taps = {}
    with torch.no_grad():
        ref = onets.vae_encode(dd, sd, mel, taps=taps)
    worst = 0.0
    for name, t in v.read_encoder_taps().items():
        l2, _ = _report("enc tap " + name, t, taps[name])
        worst = max(worst, l2)
    assert worst <= REL_L2
    _check("vae encoder moments vs oracle", post.parameters, ref)
    _check("vae encoder moments vs reference golden", post.parameters, torch.from_numpy(g["moments"]))
    # sampling: the reference draws torch.randn(mean.shape) on the CPU and moves it; replay the recorded draw
    noise = torch.from_numpy(g["noise"])
    orig = torch.randn
    torch.randn = lambda *a, **k: noise.clone()
    try:
        z = v.get_first_stage_encoding(post)
    finally:
        torch.randn = orig
    _check("scaled posterior sample vs reference golden", z, torch.from_numpy(g["z"]))
    assert tuple(z.shape) == (2, 8, 16, 4)
    # round trip through the decoder stays finite and has the mel's shape
    rec = v.decode_first_stage(z)
    assert tuple(rec.shape) == tuple(mel.shape) and bool(torch.isfinite(rec).all())


def test_vae_encoder_full_width_against_reference_golden(golden):
    g = golden("vae_encoder_full")
    dd = spec.VAE_DDCONFIG
    v = modules.AutoencoderKL(ddconfig=dd, embed_dim=8, scale_factor=float(g["scale_factor"]))
    sd = dict(cases.vae_weights(dd))
    sd.update(cases.vae_encoder_weights(dd))
    sd.update(cases.hifigan_weights(spec.HIFIGAN_16K_64))
    _load(v, sd)
    mel = cases.mel_inputs(1, 128, 64, "vaeenc_full") * 2.0 - 4.0
    post = v.encode_first_stage(mel.to(DEV))
    _check("full-width vae encoder moments vs reference golden", post.parameters, torch.from_numpy(g["moments"]))
    with pytest.raises(ValueError):
        v.encode_first_stage(torch.zeros(1, 1, 30, 64, device=DEV))     # extent not a multiple of 4


def test_mel_frontend_against_reference_golden(golden):
    """wav_to_fbank on the HIP front-end vs the reference's TacotronSTFT + tools.torch_tools.wav_to_fbank fixture.
    Tolerance: the log-mel is compared in ABSOLUTE terms (it is a logarithm; 0.005 = 0.5 % in linear mel energy); the
    three-way split-bf16 STFT (fp32-grade products) keeps even near-silent bins within it."""
    import make_golden_mel as mg
    from consistencytta_amd import audio
    g = golden("mel_frontend")
    stft = audio.TacotronSTFT(1024, 160, 1024, 64, 16000, 0, 8000).to(DEV)
    fb, lm = audio.wav_to_fbank(mg.test_wave(2, 40000, "mel").to(DEV), 256, stft)
    ref = torch.from_numpy(g["fbank"])
    err = float((fb.cpu() - ref).abs().max())
    print("log-mel max abs error %.3e (range %.1f .. %.1f)" % (err, float(ref.min()), float(ref.max())))
    assert tuple(fb.shape) == (2, 256, 64) and err < 5e-3
    assert float(fb[:, 251:].abs().max()) == 0.0                       # zero padding past the last frame
    assert float((lm.cpu()[:, ::8, ::8] - torch.from_numpy(g["logmag_sub"])).abs().max()) < 5e-2
    fb2, _ = audio.wav_to_fbank(mg.test_wave(1, 163840, "mel_full"), 1024, stft)     # CPU waveform (dataloader) is moved
    err2 = float((fb2.cpu() - torch.from_numpy(g["fbank_full"])).abs().max())
    print("10.24 s clip: log-mel max abs error %.3e" % err2)
    assert tuple(fb2.shape) == (1, 1024, 64) and err2 < 5e-3
    mel, logm, _ = stft.mel_spectrogram(mg.test_wave(1, 16000, "mel_s").nan_to_num().clip(-1, 1).to(DEV))
    assert tuple(mel.shape) == (1, 64, 101) and tuple(logm.shape) == (1, 512, 101)
    with pytest.raises(N.CttaError):
        audio.TacotronSTFT().fbank(torch.zeros(1, 16000))            # module on the CPU: no fallback


@pytest.mark.parametrize("B,H,W,L,mask_mode", [(1, 8, 8, 1, "none"), (2, 16, 8, 3, "row_all_masked"), (3, 8, 16, 9, "ragged"),
                                               (1, 40, 8, 33, "ragged")])
def test_unet_edge_cases_against_oracle(B, H, W, L, mask_mode):
    """Smallest extent the 4-level U-Net accepts, a single text token, a row whose mask keeps nothing (the reference adds
    -10000 to every key of that row: a uniform softmax), ragged masks, odd text lengths beyond the 32-token arena
    default, batch 1 -- all vs the CPU oracle."""
    cfg = cases.TINY_UNET
    sd = cases.unet_weights(cfg, True)
    m = _load(modules.UNet2DConditionGuidedModel.from_config(cfg), sd)
    x, ts, gs, enc, mask = cases.unet_inputs(cfg, B, H, W, L, "edge_%s_%d" % (mask_mode, L))
    if mask_mode == "none":
        mask = None
    elif mask_mode == "row_all_masked":
        mask = mask.clone()
        mask[-1] = False
    out = m(x.to(DEV), ts.to(DEV), guidance=gs.to(DEV), encoder_hidden_states=enc.to(DEV),
            encoder_attention_mask=None if mask is None else mask.to(DEV)).sample
    with torch.no_grad():
        ref = onets.unet_forward(cfg, sd, x, ts, gs, enc, mask)
    _check("unet edge %s B=%d %dx%d L=%d" % (mask_mode, B, H, W, L), out, ref)


def test_unet_rejects_bad_extents_and_shapes():
    cfg = cases.TINY_UNET
    m = _load(modules.UNet2DConditionGuidedModel.from_config(cfg), cases.unet_weights(cfg, True))
    x, ts, gs, enc, mask = cases.unet_inputs(cfg, 1, 12, 8, 4, "edge_bad")          # 12 is not a multiple of 8
    with pytest.raises(N.CttaError, match="multiple of 8"):
        m(x.to(DEV), ts.to(DEV), guidance=gs.to(DEV), encoder_hidden_states=enc.to(DEV))
    x, ts, gs, enc, mask = cases.unet_inputs(cfg, 1, 16, 8, 4, "edge_bad2")
    with pytest.raises(ValueError):
        m(x.to(DEV), ts.to(DEV), guidance=gs.to(DEV), encoder_hidden_states=enc[:, :, :-1].to(DEV))   # wrong feature dim
    with pytest.raises(ValueError):
        m(x[:, :4].to(DEV), ts.to(DEV), guidance=gs.to(DEV), encoder_hidden_states=enc.to(DEV))        # wrong channels
    with pytest.raises(N.CttaError, match="no CPU path"):
        m(x, ts, guidance=gs, encoder_hidden_states=enc)                                                # CPU tensors


def _vocoder_masks(v):
    """The engine's saved LeakyReLU outputs (debug taps of the differentiable forward) as oracle mask sites."""
    masks = {}
    for name, t in v._read_taps("voc").items():
        if name.startswith("mask."):
            masks[name[len("mask."):]] = t.squeeze(2).cpu()
        elif name.startswith("lrelu."):
            masks[name[len("lrelu."):]] = t.squeeze(2).cpu()
    return masks


def test_differentiable_decode_gradients_against_reference_golden(golden):
    """decode_first_stage(allow_grad=True) -> decode_to_waveform(allow_grad=True) (CLAPLoss, tools/losses.py:294-298;
    SURVEY §8f rank 2).  Forward values and the decoder's latent gradient are compared directly.  The vocoder is
    piecewise linear (46 LeakyReLUs deep), so its input gradient is discontinuous in the activations: bf16 storage
    flips the sign of ~1 % of near-zero activations per site and each flip moves a gradient entry by 90 %.  Its backward
    OPERATOR is therefore checked exactly -- against the oracle's autograd with the engine's own masks prescribed
    (tolerance = bf16 round-off) -- and the unconstrained comparison with the fp32 reference carries the flip noise
    (the same magnitude separates an fp32 run from one with bf16-rounded activations on the CPU)."""
    g = golden("vae_grad_tiny")
    v, sd = _vae(cases.TINY_VAE_DD, cases.TINY_HIFIGAN, taps=True)
    v.scale_factor = float(g["scale_factor"])
    z = cases.vae_inputs(2, 16, 16, "vae_grad")
    zd = z.to(DEV).requires_grad_(True)
    mel = v.decode_first_stage(zd, allow_grad=True)
    assert mel.requires_grad
    mel.retain_grad()
    wav = v.decode_to_waveform(mel, allow_grad=True)
    direction = cases.t(spec.det_uniform("vae_grad.direction", tuple(wav.shape), 21))
    (wav * direction.to(DEV)).sum().backward()
    _check("differentiable mel vs reference", mel.detach(), torch.from_numpy(g["mel"]))
    _check("differentiable wav vs reference", wav.detach(), torch.from_numpy(g["wav"]))
    _check("d/d mel vs reference autograd (flip noise)", mel.grad, torch.from_numpy(g["grad_mel"]), l2_tol=0.3, max_tol=0.5)
    _check("d/d z vs reference autograd (flip noise)", zd.grad, torch.from_numpy(g["grad_z"]), l2_tol=0.3, max_tol=0.5)
    # same graph on the oracle with the engine's masks: mel gradient, then through the (smooth) decoder to z
    masks = _vocoder_masks(v)
    zo = z.clone().requires_grad_(True)
    melo = onets.vae_decode(cases.TINY_VAE_DD, sd, zo, v.scale_factor)
    melo.retain_grad()
    wo = onets.hifigan_forward(cases.TINY_HIFIGAN, sd, melo.squeeze(1).permute(0, 2, 1), lrelu_masks=masks).squeeze(1)
    wo = wo - (wo.max() + wo.min()) / 2
    (wo * direction).sum().backward()
    _check("d/d mel vs oracle autograd, engine masks", mel.grad, melo.grad, l2_tol=3e-2, max_tol=8e-2)
    _check("d/d z vs oracle autograd, engine masks", zd.grad, zo.grad, l2_tol=3e-2, max_tol=8e-2)

    # vocoder alone: same mel on both sides
    mel_in = cases.mel_inputs(2, 24, 64, "hifigan_tiny")
    md = mel_in.to(DEV).requires_grad_(True)
    v2, _ = _vae(cases.TINY_VAE_DD, cases.TINY_HIFIGAN, taps=True)   # taps keep the shapes the handle was sized for
    wd = modules._VocodeWithGrad.apply(md, v2)
    dirv = cases.t(spec.det_uniform("vae_grad.dirv", tuple(wd.shape), 22))
    (wd * dirv.to(DEV)).sum().backward()
    mo = mel_in.clone().requires_grad_(True)
    wo = onets.hifigan_forward(cases.TINY_HIFIGAN, sd, mo.squeeze(1).permute(0, 2, 1), lrelu_masks=_vocoder_masks(v2)).squeeze(1)
    (wo * dirv).sum().backward()
    _check("vocoder wav (grad forward) vs oracle", wd.detach(), wo.detach())
    _check("vocoder d/d mel vs oracle autograd, engine masks", md.grad, mo.grad, l2_tol=3e-2, max_tol=8e-2)

    # decoder alone (GroupNorm / SiLU / softmax: smooth, compared directly)
    zo = z.clone().requires_grad_(True)
    melo = onets.vae_decode(cases.TINY_VAE_DD, sd, zo, v.scale_factor)
    dirm = cases.t(spec.det_uniform("vae_grad.dirm", tuple(melo.shape), 23))
    (melo * dirm).sum().backward()
    z2 = z.to(DEV).requires_grad_(True)
    mel2 = v.decode_first_stage(z2, allow_grad=True)
    (mel2 * dirm.to(DEV)).sum().backward()
    _check("decoder d/d z vs oracle autograd", z2.grad, zo.grad)

    # plain decodes (own handle) do not disturb a pending differentiable one -- MelLoss decodes input AND target;
    # a second differentiable decode does: loud error on the stale graph, not stale gradients
    z3 = z.to(DEV).requires_grad_(True)
    mel3 = v.decode_first_stage(z3, allow_grad=True)
    plain = v.decode_first_stage(z.to(DEV), allow_grad=True)      # no grad wanted -> plain path
    assert not plain.requires_grad
    (mel3 * dirm.to(DEV)).sum().backward()
    _check("decoder d/d z with a plain decode in between", z3.grad, zo.grad)
    mel4 = v.decode_first_stage(z.to(DEV).requires_grad_(True), allow_grad=True)
    v.decode_first_stage(z.to(DEV).requires_grad_(True), allow_grad=True)
    with pytest.raises(N.CttaError):
        mel4.sum().backward()


def test_t5_encoder_against_transformers_golden_and_oracle(golden):
    """The text encoder (models/audio_distilled_model.py:97-98,208-214) on the HIP engine vs the
    installed transformers' own T5EncoderModel (fixture) and the oracle: ragged masks, a length that is not a multiple
    of 8, a sequence spanning every relative-position bucket, FLAN-T5-large's widths; key order; error behaviour."""
    from consistencytta_amd import text_encoder
    from oracle import t5 as ot5
    g = golden("t5_encoder")
    for name, cfg, B, L, tag in (("tiny", cases.TINY_T5, 3, 13, "t5_tiny"), ("tiny_long", cases.TINY_T5, 2, 150, "t5_long"),
                                 ("wide", cases.WIDE_T5, 2, 16, "t5_wide")):
        m = text_encoder.T5EncoderModel(cfg)
        assert list(m.state_dict().keys()) == list(spec.t5_encoder_param_spec(cfg).keys())
        sd = cases.t5_weights(cfg)
        m.load_state_dict(sd)
        m.to(DEV).eval()
        ids, mask = cases.t5_inputs(cfg, B, L, tag)
        out = m(input_ids=ids.to(DEV), attention_mask=mask.to(DEV))
        assert out[0] is out.last_hidden_state and tuple(out[0].shape) == (B, L, cfg["d_model"])
        with torch.no_grad():
            ref = ot5.t5_encode(cfg, sd, ids, mask)
        valid = mask.bool()
        # padded positions are computed by the reference too (and consumed nowhere): compared as well
        _check("t5 %s vs oracle" % name, out[0], ref)
        _check("t5 %s vs transformers" % name, out[0], torch.from_numpy(g[name]))
        _check("t5 %s valid tokens vs transformers" % name, out[0].cpu()[valid], torch.from_numpy(g[name])[valid])
        # smaller batch / shorter length on the same handle; batch independence
        out1 = m(input_ids=ids[:1, :L - 3].to(DEV), attention_mask=torch.ones(1, L - 3, dtype=torch.long, device=DEV))
        with torch.no_grad():
            ref1 = ot5.t5_encode(cfg, sd, ids[:1, :L - 3], torch.ones(1, L - 3, dtype=torch.long))
        _check("t5 %s shorter call vs oracle" % name, out1[0], ref1)
    with pytest.raises(N.CttaError):
        m(input_ids=ids, attention_mask=mask)                       # CPU tensors: no CPU path
    with pytest.raises(IndexError):
        m(input_ids=torch.full((1, 4), cfg["vocab_size"], device=DEV), attention_mask=torch.ones(1, 4, device=DEV))
    with pytest.raises(ValueError):
        m(input_ids=ids.to(DEV), attention_mask=torch.zeros_like(mask).to(DEV))


@pytest.mark.parametrize("guided", [True, False])
def test_unet_forward_is_bit_identical_whatever_the_batch_mates(guided):
    """Data-parallel training shards a batch by sample, so a sample's activations must not depend on who shares its
    launch.  (a) At a FIXED batch size a sample's rows are bit-identical whatever its mates and its position -- the
    property sharding needs (every rank runs the same micro-batch size).  (b) Across batch sizes (tile choice, split-K and
    the small fp32 MLP kernels all change with the batch size; a 1-ulp difference in the time embedding once flipped bf16
    roundings downstream and showed up as 1e-3 in the 2-rank gradient test): bit-identical with GroupNorm's statistics
    pass on its own kernel (ctta_set_gn_fuse(0): rounds 1-2), bf16 round-off with the statistics in the conv epilogue
    (round 3 default: the per-tile partial sums depend on the tile shape in the last fp32 bits)."""
    cfg = cases.TINY_UNET
    cls = modules.UNet2DConditionGuidedModel if guided else modules.UNet2DConditionModel
    net = _load(cls.from_config(cfg), cases.unet_weights(cfg, guided, 1))
    B, L = 8, 6
    P = cases.prompt_states(cfg, B, L, "mates")
    z = (cases.t(spec.det_uniform("mates.z", (B, 8, 32, 8), 14)) * 0.9).to(DEV)
    t = torch.tensor([3.0, 400.0, 77.0, 950.0, 10.0, 500.0, 640.0, 999.0], device=DEV)
    w = torch.tensor([1.0, 2.5, 4.0, 0.3, 0.7, 5.0, 3.3, 2.0], device=DEV)
    enc, mask = P["embeds"].to(DEV), P["mask"].to(DEV)

    def run_idx(idx):
        idx = torch.as_tensor(idx, device=DEV)
        kw = dict(encoder_hidden_states=enc[idx], encoder_attention_mask=mask[idx])
        if guided:
            kw["guidance"] = w[idx]
        with torch.no_grad():
            return net(z[idx], t[idx], **kw).sample.clone()

    def run(lo, hi):
        return run_idx(list(range(lo, hi)))
    from consistencytta_amd import _native as N_
    L_ = N_.lib()
    assert L_.ctta_get_gn_fuse() == 1
    try:
        full = run(0, B)
        # (a) fixed size: other mates, other positions
        perm = [5, 2, 7, 0, 3, 6, 1, 4]
        got = run_idx(perm)
        for pos, s_ in enumerate(perm):
            assert torch.equal(got[pos], full[s_]), "sample %d at position %d of a permuted batch differs" % (s_, pos)
        four = run(0, 4)
        assert torch.equal(run_idx([3, 7, 0, 5])[2], four[0]) and torch.equal(run_idx([6, 1, 4, 2])[1], four[1])
        # (b) across sizes: bf16 round-off
        for lo, hi in [(0, 4), (4, 8), (2, 5), (0, 7)] + [(s_, s_ + 1) for s_ in range(B)]:
            sub = run(lo, hi)
            err = float((sub - full[lo:hi]).norm() / full[lo:hi].norm())
            assert err <= 2e-3, "samples %d..%d: rel L2 %.2e vs their rows of the batch-8 forward" % (lo, hi - 1, err)
        # ... and bit for bit with the statistics on their own pass
        L_.ctta_set_gn_fuse(0)
        full0 = run(0, B)
        for lo, hi in [(0, 4), (4, 8), (2, 5), (0, 7)] + [(s_, s_ + 1) for s_ in range(B)]:
            assert torch.equal(run(lo, hi), full0[lo:hi]), "samples %d..%d differ from their rows of the batch-8 forward" % (lo, hi - 1)
        assert float((full0 - full).norm() / full.norm()) <= 2e-3
    finally:
        L_.ctta_set_gn_fuse(1)


def test_text_cache_reuses_cross_attention_kv_only_for_unchanged_text_states():
    """ctta_unet_reuse_text (round 3): a second query with the SAME text-state tensors skips the 2 x (number of transformer
    blocks) K / V projection GEMMs and is bit-identical to a cold module; an in-place change of the text states, a new
    tensor object, other weights or a capture without the caller's word all recompute."""
    import ctypes
    from consistencytta_amd import _native as N_
    cfg = cases.TINY_UNET
    sd = cases.unet_weights(cfg, False, 1)
    net = _load(modules.UNet2DConditionModel.from_config(cfg), sd)
    cold = _load(modules.UNet2DConditionModel.from_config(cfg), sd)
    B, L = 4, 6
    P = cases.prompt_states(cfg, B, L, "tcache")
    enc, mask = P["embeds"].to(DEV).contiguous(), P["mask"].to(DEV)
    z = [(cases.t(spec.det_uniform("tcache.z%d" % i, (B, 8, 32, 8), 14 + i)) * 0.9).to(DEV) for i in range(3)]
    t = [torch.tensor([3.0, 400.0, 77.0, 950.0], device=DEV) + i for i in range(3)]
    L_ = N_.lib()

    def launches(fn):
        L_.ctta_prof_enable(1)
        out = fn()
        torch.cuda.synchronize()
        L_.ctta_prof_enable(0)
        ms, fl, cnt = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        N_.check(L_.ctta_prof_collect(0, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(cnt), None))
        return out, cnt.value

    def q(m, i, e=enc, **kw):
        with torch.no_grad():
            return m(z[i], t[i], e, encoder_attention_mask=mask, **kw).sample.clone()
    o0, n0 = launches(lambda: q(net, 0))
    o1, n1 = launches(lambda: q(net, 1))                       # same tensors: K / V from the cache
    n_blocks = sum(1 for k in sd if k.endswith("attn2.to_k.weight"))
    assert n_blocks >= 3 and n0 - n1 == 2 * n_blocks, (n0, n1, n_blocks)
    assert torch.equal(o1, q(cold, 1, e=enc.clone()))
    _, n1f = launches(lambda: q(net, 1, reuse_text=False))    # the caller can always refuse
    assert n1f == n0
    enc.mul_(1.25)                                             # in-place change: version counter moved -> recompute
    o2, n2 = launches(lambda: q(net, 2))
    assert n2 == n0 and torch.equal(o2, q(cold, 2, e=enc.clone()))
    o2b, n2b = launches(lambda: q(net, 2, e=enc.clone()))      # equal content, other object -> recompute (and same numbers)
    assert n2b == n0 and torch.equal(o2b, o2)
    new_sd = {k: (v * 1.01 if k.endswith("attn2.to_k.weight") else v) for k, v in sd.items()}
    net.load_state_dict(new_sd)
    net.to(DEV)
    e3 = enc.clone()
    q(net, 0, e=e3)
    cold2 = _load(modules.UNet2DConditionModel.from_config(cfg), new_sd)
    o3, n3 = launches(lambda: q(net, 1, e=e3))
    assert n3 == n1 and torch.equal(o3, q(cold2, 1, e=e3.clone()))     # new weights were re-projected once, then reused


def test_vocoder_input_gradient_predicts_the_finite_difference_along_itself():
    """a finite-difference check of the vocoder's input gradient that does not depend on the reference's
    activation signs.  f(mel) = <vocode(mel), w> is piecewise linear; along d = g / |g| (g = the engine's gradient) the
    central difference (f(mel + eps d) - f(mel - eps d)) / (2 eps) must equal <g, d> = |g| up to the kinks crossed (a few %
    at eps = 0.2 .. 0.5 of a mel whose rms is 0.87) -- steps below 0.1 drown in the bf16 forward noise (measured ratios
    0.85 / 1.24 at eps = 0.02 / 0.05, 1.001 / 0.977 / 0.970 at 0.1 / 0.2 / 0.5).  A gradient with wrong masks, a missing
    branch of the MRF sum or a wrong scale fails this by tens of percent."""
    mel_in = cases.mel_inputs(2, 24, 64, "hifigan_tiny")
    v, _ = _vae(cases.TINY_VAE_DD, cases.TINY_HIFIGAN, taps=True)
    md = mel_in.to(DEV).requires_grad_(True)
    wav = modules._VocodeWithGrad.apply(md, v)
    w = cases.t(spec.det_uniform("vae_grad.dirv", tuple(wav.shape), 22)).to(DEV)
    (wav * w).sum().backward()
    g = md.grad.clone()
    d = g / g.norm()
    analytic = float((g.double() * d.double()).sum())

    def f(m):
        with torch.no_grad():
            return float((modules._VocodeWithGrad.apply(m, v).double() * w.double()).sum())
    for eps in (0.2, 0.5):
        fd = (f(mel_in.to(DEV) + eps * d) - f(mel_in.to(DEV) - eps * d)) / (2 * eps)
        print("eps %.1f: finite difference %.4f, <g, d> %.4f, ratio %.4f" % (eps, fd, analytic, fd / analytic))
        assert abs(fd / analytic - 1.0) <= 0.08
