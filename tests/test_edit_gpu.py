"""Audio editing with the consistency student (ConsistencyTTA.edit_latent, capture_edit_graph, edit_from_embeds): the two
kernels against the unfused sequence they replace, bit for bit; the sampler's identities; the eager path against the plain
torch restatement tests/edit_ref.py; the captured path against the eager one; the waveform entry against its manual chain.
No tolerance anywhere: the feature is an exact composition of steps that other tests pin to the reference, plus one blend."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
import edit_ref  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from consistencytta_amd import spec  # noqa: E402

DEV = "cuda:0"
B, L, LATENT = 2, 7, (8, 32, 16)
H, W = LATENT[1:]
W_IN = 4.0
NULL = N.c_void_p(0)


def _pipe(**kw):
    from consistencytta_amd import modules
    from consistencytta_amd.models import ConsistencyTTA
    cfg = dict(cases.TINY_UNET)
    vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    pipe = ConsistencyTTA(unet_config=cfg, vae=vae, **kw)
    pipe.to(DEV)
    pipe.unet.init_deterministic(1)
    vae.init_deterministic(2)
    sd = vae.state_dict()
    sd.update(cases.vae_encoder_weights(cases.TINY_VAE_DD))
    vae.load_state_dict(sd)
    pipe.eval().requires_grad_(False)
    return pipe, cfg


@pytest.fixture(scope="module")
def shared():
    """One pipe for the tests that only run eager calls (a capture gets its own)."""
    return _pipe()


def _noise(steps, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((steps, B) + LATENT, generator=g).to(DEV)


def _source(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B,) + LATENT, generator=g) * 0.8).to(DEV)


def _states(cfg, tag):
    _, _, _, enc, mask = cases.unet_inputs(cfg, B, H, W, L, tag)
    return enc.to(DEV), mask.to(DEV)


def _uncond(cfg, tag):
    u = cases.t(spec.det_uniform(tag + ".unc", (B, L, cfg["cross_attention_dim"]), 12)) * 0.5
    m = torch.zeros(B, L, dtype=torch.bool)
    m[:, :2] = True
    return u.to(DEV), m.to(DEV)


def _half_mask(rows=B):
    keep = torch.ones(rows, 1, H, W)
    keep[:, :, H // 2:] = 0
    return keep.to(DEV)


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


# --------------------------------------------------------------------------------------------------- 1: the kernels
def _edit_renoise(cond, unc, w, src, keep, nz, sig, copies, n, hw, out, batch=3):
    return N.lib().ctta_consistency_edit_renoise(N.ptr(cond), N.ptr(unc), N.ptr(w) if w is not None else NULL, N.ptr(src),
                                                 N.ptr(keep), N.ptr(nz), N.ptr(sig), N.ptr(out), copies, batch, n, hw,
                                                 N.stream_ptr())


def _combine_keep(unc, cond, w, src, keep, n, hw, out, batch=3):
    return N.lib().ctta_cfg_combine_keep(N.ptr(unc), N.ptr(cond), N.ptr(w) if w is not None else NULL, N.ptr(src),
                                         N.ptr(keep), N.ptr(out), batch, n, hw, N.stream_ptr())


def _kernel_inputs(hw, channels):
    n = hw * channels
    g = torch.Generator().manual_seed(hw + channels)
    c, u, nz, src = (torch.randn(3, n, generator=g).to(DEV) for _ in range(4))
    sig = torch.tensor([14.6146, 0.0, 0.7], dtype=torch.float32, device=DEV)
    w = torch.tensor([1.0, 2.0, 0.5], dtype=torch.float32, device=DEV)
    values = torch.tensor([0.0, 1.0, 0.25])
    keep = torch.stack([values[(torch.arange(hw) + b) % 3] for b in range(3)]).to(DEV)      # 0, 1, 0.25 in every plane
    keep_rows = keep[:, None, :].expand(3, channels, hw).reshape(3, n)                        # the plane under every channel
    return n, c, u, nz, src, sig, w, keep, keep_rows


@pytest.mark.parametrize("channels", [1, 8])
@pytest.mark.parametrize("hw", [4, 4 * 257, 512])
def test_edit_kernels_equal_the_unfused_sequence_bit_for_bit(hw, channels):
    """torch's (1 - w) * u + w * c, torch's keep * src + (1 - keep) * x0, ctta_heun_add_noise, ctta_heun_scale_model_input,
    torch.cat against the one-pass kernel: copies 1 and 2; cond alone, uncond + cond, and cond == NULL (x0 = 0); per-row w
    in {1, 2, 0.5}, per-row sigmas (sigma_max, 0, an inner one), mask values 0, 1 and 0.25 in one plane of hw entries under
    `channels` channels.  The output buffer starts as NaN and is followed by 256 sentinel floats."""
    L_ = N.lib()
    n, c, u, nz, src, sig, w, keep, keep_rows = _kernel_inputs(hw, channels)
    for mode in ("cond", "cfg", "zero"):
        x0 = {"cond": c, "cfg": (1 - w[:, None]) * u + w[:, None] * c, "zero": torch.zeros_like(c)}[mode]
        x0 = keep_rows * src + (1 - keep_rows) * x0
        z, ref1 = torch.empty_like(c), torch.empty_like(c)
        N.check(L_.ctta_heun_add_noise(N.ptr(x0), N.ptr(nz), N.ptr(sig), N.ptr(z), 3, n, N.stream_ptr()))
        N.check(L_.ctta_heun_scale_model_input(N.ptr(z), N.ptr(sig), N.ptr(ref1), 3, n, N.stream_ptr()))
        assert bool(torch.isfinite(ref1).all())
        cond, unc, ww = {"cond": (c, None, None), "cfg": (c, u, w), "zero": (None, None, None)}[mode]
        for copies in (1, 2):
            ref = torch.cat([ref1] * copies)
            buf = torch.full((copies * 3 * n + 256,), float("nan"), device=DEV)
            buf[copies * 3 * n:] = 12345.0
            N.check(_edit_renoise(cond, unc, ww, src, keep, nz, sig, copies, n, hw, buf))
            got = buf[:copies * 3 * n].view(copies * 3, n)
            assert not bool(torch.isnan(got).any()), (mode, copies)
            assert torch.equal(_bits(got), _bits(ref)), (mode, copies)
            assert bool((buf[copies * 3 * n:] == 12345.0).all()), (mode, copies)
        if mode == "zero":
            continue
        buf = torch.full((3 * n + 256,), float("nan"), device=DEV)
        buf[3 * n:] = 12345.0
        N.check(_combine_keep(unc, cond, ww, src, keep, n, hw, buf))
        assert torch.equal(_bits(buf[:3 * n].view(3, n)), _bits(x0)), mode
        assert bool((buf[3 * n:] == 12345.0).all()), mode


def test_edit_kernels_refuse_before_launch():
    Bk, n, hw = 3, 16, 8
    c, nz, src = (torch.ones(Bk, n, device=DEV) for _ in range(3))
    keep = torch.ones(Bk, hw, device=DEV)
    sig = torch.ones(Bk, device=DEV)
    buf = torch.full((2 * Bk * n + 256,), float("nan"), device=DEV)
    assert _edit_renoise(c, None, None, src, keep, nz, sig, 1, 12, 6, buf) != 0
    with pytest.raises(N.CttaError, match="multiple of 4"):
        N.check(_edit_renoise(c, None, None, src, keep, nz, sig, 1, 12, 6, buf))             # hw % 4 != 0
    with pytest.raises(N.CttaError, match="no multiple of hw"):
        N.check(_edit_renoise(c, None, None, src, keep, nz, sig, 1, 12, 8, buf))             # n % hw != 0
    with pytest.raises(N.CttaError, match="copies"):
        N.check(_edit_renoise(c, None, None, src, keep, nz, sig, 3, n, hw, buf))
    with pytest.raises(N.CttaError):
        N.check(_edit_renoise(c, c, None, src, keep, nz, sig, 1, n, hw, buf))                # uncond without w_post
    with pytest.raises(N.CttaError):
        N.check(_edit_renoise(None, c, sig, src, keep, nz, sig, 1, n, hw, buf))              # uncond without cond
    with pytest.raises(N.CttaError, match="src and keep"):
        N.check(_edit_renoise(c, None, None, src, None, nz, sig, 1, n, hw, buf))             # src without keep
    with pytest.raises(N.CttaError, match="src and keep"):
        N.check(_edit_renoise(c, None, None, None, keep, nz, sig, 1, n, hw, buf))
    with pytest.raises(N.CttaError, match="multiple of 4"):
        N.check(_combine_keep(None, c, None, src, keep, 12, 6, buf))
    with pytest.raises(N.CttaError, match="no multiple of hw"):
        N.check(_combine_keep(None, c, None, src, keep, 12, 8, buf))
    with pytest.raises(N.CttaError):
        N.check(_combine_keep(c, c, None, src, keep, n, hw, buf))                            # uncond without w
    with pytest.raises(N.CttaError, match="src and keep"):
        N.check(_combine_keep(None, c, None, src, None, n, hw, buf))
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())                                                      # nothing was launched


# ------------------------------------------------------------------------------------------ 2: the sampler's identities
@pytest.mark.parametrize("steps,post", [(1, 1.0), (3, 1.0), (1, 2.0), (3, 2.0)])
def test_nothing_kept_at_full_strength_is_plain_generation(shared, steps, post):
    pipe, cfg = shared
    enc, mask = _states(cfg, "edit2")
    noise, src = _noise(steps, 100 + steps), _source(7)
    kw = {}
    if post > 1:
        unc, unc_mask = _uncond(cfg, "edit2")
        kw = dict(uncond_states=unc, uncond_mask=unc_mask)
    plain = pipe.generate_latent(enc, mask, noise[0], W_IN, post, steps, step_noise=noise[1:], **kw)
    for keep in (torch.zeros(B, 1, H, W, device=DEV), None):
        got = pipe.edit_latent(enc, mask, noise[0], src, keep, 1.0, W_IN, post, steps, step_noise=noise[1:], **kw)
        assert torch.equal(got, plain)


def test_everything_kept_returns_the_source_whatever_the_prompt(shared):
    pipe, cfg = shared
    noise, src = _noise(3, 110), _source(8)
    for tag, keep in (("edit3a", torch.ones(B, 1, H, W, device=DEV)), ("edit3b", torch.ones(1, 1, H, W, device=DEV))):
        enc, mask = _states(cfg, tag)
        got = pipe.edit_latent(enc, mask, noise[0], src, keep, 1.0, W_IN, 1.0, 3, step_noise=noise[1:])
        assert torch.equal(got, src)


def test_half_time_mask_keeps_one_half_and_regenerates_the_other(shared):
    pipe, cfg = shared
    enc, mask = _states(cfg, "edit4")
    noise, src = _noise(3, 120), _source(9)
    plain = pipe.generate_latent(enc, mask, noise[0], W_IN, 1.0, 3, step_noise=noise[1:])
    got = pipe.edit_latent(enc, mask, noise[0], src, _half_mask(1), 1.0, W_IN, 1.0, 3, step_noise=noise[1:])
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got[:, :, :H // 2], src[:, :, :H // 2])
    new = got[:, :, H // 2:]
    assert not torch.equal(new, src[:, :, H // 2:]) and not torch.equal(new, plain[:, :, H // 2:])
    assert float((new - src[:, :, H // 2:]).abs().max()) > 1e-3 and float((new - plain[:, :, H // 2:]).abs().max()) > 1e-6
    torch.manual_seed(4)                                 # the internal draws: torch.randn_like per re-noising step
    a = pipe.edit_latent(enc, mask, noise[0], src, _half_mask(1), 1.0, W_IN, 1.0, 3)
    torch.manual_seed(4)
    draws = torch.stack([torch.randn_like(noise[0]), torch.randn_like(noise[0])])
    b = pipe.edit_latent(enc, mask, noise[0], src, _half_mask(1), 1.0, W_IN, 1.0, 3, step_noise=draws)
    assert torch.equal(a, b) and not torch.equal(a, got)


# ------------------------------------------------------------------------------- 3: the eager path against the restatement
@pytest.mark.parametrize("strength,post", [(1.0, 1.0), (0.5, 1.0), (1.0, 2.0), (0.5, 2.0), (1.0, 2.3), (0.5, 2.3), (1.0, 1.3),
                                           (0.5, 1.3)])
def test_eager_edit_equals_the_plain_torch_restatement(shared, strength, post):
    """Two non-dyadic post scales.  2.3: fp32(1 - 2.3) happens to equal fp32(1) - fp32(2.3), so the kernels combine.
    1.3: it does not, and the combine stays torch's own in front of the kernels (models._post_cfg_fusable)."""
    from consistencytta_amd.models import _post_cfg_fusable
    assert _post_cfg_fusable(2.0) and _post_cfg_fusable(2.3) and not _post_cfg_fusable(1.3)
    pipe, cfg = shared
    steps = 4
    r = max(1, int(strength * steps))
    enc, mask = _states(cfg, "edit5")
    unc, unc_mask = _uncond(cfg, "edit5")
    noise, src = _noise(r, 130), _source(10)
    keep = _half_mask()
    keep[1, :, :4] = 0.25                                # a soft edge in one row of the batch

    def query(z_in, t):
        if post > 1:
            zh = pipe.unet(torch.cat([z_in] * 2), t, guidance=W_IN, encoder_hidden_states=torch.cat([unc, enc]),
                           encoder_attention_mask=torch.cat([unc_mask, mask])).sample
            u, c = zh.chunk(2)
            return (1 - post) * u + post * c
        return pipe.unet(z_in, t, guidance=W_IN, encoder_hidden_states=enc, encoder_attention_mask=mask).sample

    times, sigmas = edit_ref.schedule(pipe.scheduler, steps)
    want = edit_ref.edit_sampler(query, times, sigmas, noise[0], src, keep, strength, noise[1:])
    kw = dict(uncond_states=unc, uncond_mask=unc_mask) if post > 1 else {}
    got = pipe.edit_latent(enc, mask, noise[0], src, keep, strength, W_IN, post, steps, step_noise=noise[1:], **kw)
    assert bool(torch.isfinite(want).all())
    assert torch.equal(got, want)
    if strength < 1:                                     # another start, another result
        full = pipe.edit_latent(enc, mask, noise[0], src, keep, 1.0, W_IN, post, steps,
                                step_noise=_noise(steps, 131)[1:], **kw)
        assert not torch.equal(full, got)


# ------------------------------------------------------------------------------------------------ 4: the captured path
def _eager_edit(pipe, enc, mask, noise, src, keep, strength, post, steps, unc=None, unc_mask=None):
    kw = dict(uncond_states=unc, uncond_mask=unc_mask) if post > 1 else {}
    lat = pipe.edit_latent(enc, mask, noise[0], src, keep, strength, W_IN, post, steps, step_noise=noise[1:], **kw)
    mel = pipe.vae.decode_first_stage(lat.float())
    return lat.clone(), mel.clone(), pipe.vae.decode_to_waveform(mel)


@pytest.mark.parametrize("steps,strength,post", [(4, 1.0, 1.0), (4, 0.5, 2.0), (2, 1.0, 1.3)])
def test_captured_edit_graph_equals_the_eager_path(steps, strength, post):
    """post = 1.3 keeps torch's combine inside the captured sequence (models._post_cfg_fusable)."""
    pipe, cfg = _pipe()
    r = max(1, int(strength * steps))
    unc, unc_mask = _uncond(cfg, "edit6") if post > 1 else (None, None)
    soft = _half_mask(1)
    soft[:, :, :3, 8:] = 0.5
    inputs = [_states(cfg, "edit6_0") + (_noise(r, 140), _source(11), _half_mask()),
              _states(cfg, "edit6_1") + (_noise(r, 141), _source(12), soft),              # another mask, (1, 1, H, W)
              _states(cfg, "edit6_2") + (_noise(r, 142), _source(13), None)]
    refs = [_eager_edit(pipe, e, m, nz, s, k, strength, post, steps, unc, unc_mask) for e, m, nz, s, k in inputs]
    assert not np.array_equal(refs[0][2], refs[1][2])
    gen = pipe.capture_edit_graph(B, L, cfg_scale_input=W_IN, cross_attention_dim=cfg["cross_attention_dim"], latent=LATENT,
                                  num_steps=steps, strength=strength, cfg_scale_post=post, uncond_states=unc,
                                  uncond_mask=unc_mask)
    assert gen.queries == r
    for args, (lat, mel, pcm) in zip(inputs, refs):
        before = [None if a is None else a.clone() for a in args]
        out = gen(*args)
        assert torch.equal(_bits(gen.outputs[0]), _bits(lat))
        assert torch.equal(_bits(gen.outputs[1]), _bits(mel))
        assert np.array_equal(out.cpu().numpy(), pcm)
        for a, b in zip(args, before):                   # copied in, never held or written
            assert a is None or torch.equal(a, b)
    with pytest.raises(ValueError):
        gen(*inputs[0][:3], inputs[0][3][:, :, :-1], inputs[0][4])                        # another source shape
    with pytest.raises(ValueError):
        gen(*inputs[0][:4], torch.ones(B, H, W, device=DEV))                              # a mask without its channel axis
    if r > 1:
        with pytest.raises(ValueError):
            gen(inputs[0][0], inputs[0][1], inputs[0][2][0], inputs[0][3], inputs[0][4])  # one draw where r are due


# ----------------------------------------------------------------------------------------------- 5: the waveform entry
def test_edit_from_embeds_equals_the_manual_chain():
    import make_golden_mel as mg
    from consistencytta_amd import audio, modules
    pipe, cfg = _pipe()
    assert pipe.stft is None
    enc, mask = _states(cfg, "edit7")
    noise = _noise(2, 150)
    wav = mg.test_wave(B, 20320, "edit7")                # 128 frames of hop 160; holds a NaN and samples past 1
    keep = pipe.latent_keep_mask(B, (H, W), time_mask_ratio_start_and_end=(0.25, 0.75))
    got = pipe.edit_from_embeds(enc, mask, noise[0], wav, keep, 1.0, W_IN, 1.0, 2, step_noise=noise[1:])
    assert isinstance(pipe.stft, audio.TacotronSTFT) and pipe.stft.n_mel_channels == 64      # created on first use

    stft = audio.TacotronSTFT(1024, 160, 1024, 64, 16000, 0, 8000).to(DEV)
    mel, _ = audio.wav_to_fbank(wav, target_length=128, fn_STFT=stft)
    src = pipe.vae.get_first_stage_encoding(pipe.vae.encode(mel[:, None]).mode())
    assert tuple(src.shape) == (B,) + LATENT and bool(torch.isfinite(src).all())
    lat = pipe.edit_latent(enc, mask, noise[0], src, keep, 1.0, W_IN, 1.0, 2, step_noise=noise[1:])
    want = pipe.vae.decode_to_waveform(pipe.vae.decode_first_stage(lat))[:, :int(16000 * 9.5)]
    assert np.array_equal(got, want)
    plain = pipe.forward_from_embeds(enc, mask, noise[0], W_IN, 1.0, 2, step_noise=noise[1:])
    assert got.shape == plain.shape and got.dtype == plain.dtype and not np.array_equal(got, plain)

    given, _ = _pipe(stft=stft)                          # the constructor's keyword; a variation of the whole clip
    assert given.stft is stft
    vary = given.edit_from_embeds(enc, mask, noise[0], wav, None, 0.5, W_IN, 1.0, 2)
    lat = given.edit_latent(enc, mask, noise[0], src, None, 0.5, W_IN, 1.0, 2)
    assert np.array_equal(vary, given.vae.decode_to_waveform(given.vae.decode_first_stage(lat))[:, :int(16000 * 9.5)])

    with pytest.raises(ValueError, match="mel bins"):    # a front end whose bins are not 4 x the latent's
        _pipe(stft=audio.TacotronSTFT(1024, 160, 1024, 32, 16000, 0, 8000))[0].edit_from_embeds(
            enc, mask, noise[0], wav, keep, 1.0, W_IN, 1.0, 2, step_noise=noise[1:])

    bare = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    sd = dict(cases.vae_weights(cases.TINY_VAE_DD))
    sd.update(cases.hifigan_weights(cases.TINY_HIFIGAN))
    bare.load_state_dict(sd)                             # a decoder-only checkpoint
    pipe.vae = bare.to(DEV).eval().requires_grad_(False)
    with pytest.raises(RuntimeError, match="no encoder weights"):
        pipe.edit_from_embeds(enc, mask, noise[0], wav, keep, 1.0, W_IN, 1.0, 2, step_noise=noise[1:])


# --------------------------------------------------------------------------------------------------- 6: prompts in
class _WhitespaceTokenizer:
    """Whitespace tokenizer with T5's calling convention (the sentencepiece model is not available offline): ids in
    [2, 502), EOS = 1, pad = 0."""
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


def test_edit_from_prompts_is_text_encoding_then_edit_from_embeds():
    """`edit` at the model's own latent (8, 256, 16): the ratios become the mask, the draws come from the global RNG in
    `forward`'s order, post-CFG takes the uncond half of encode_text_classifier_free; without a masked span a strength
    below 1 runs without a mask."""
    import make_golden_mel as mg
    from consistencytta_amd import modules, text_encoder
    from consistencytta_amd.models import ConsistencyTTA
    te = text_encoder.T5EncoderModel(cases.TINY_T5)
    te.load_state_dict(cases.t5_weights(cases.TINY_T5))
    cfg = dict(cases.TINY_UNET, cross_attention_dim=cases.TINY_T5["d_model"])
    vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    pipe = ConsistencyTTA(unet_config=cfg, vae=vae, text_encoder=te, tokenizer=_WhitespaceTokenizer())
    pipe.to(DEV)
    pipe.unet.init_deterministic(1)
    vae.init_deterministic(2)
    pipe.eval().requires_grad_(False)
    prompts = ["a dog barks twice near the mill", "rain"]
    wav = mg.test_wave(2, 40000, "edit8").nan_to_num().clip(-1, 1)
    for strength, post, ratios in ((1.0, 2.0, (0.25, 0.75)), (0.5, 1.0, (1.0, 1.0))):
        torch.manual_seed(21)
        got = pipe.edit(prompts, wav, time_mask_ratio_start_and_end=ratios, strength=strength, cfg_scale_input=W_IN,
                        cfg_scale_post=post, num_steps=2)
        torch.manual_seed(21)
        embeds_cf, mask_cf, embeds, mask = pipe.encode_text_classifier_free(prompts, 1)
        noise = torch.randn((2, 8, 256, 16), device=embeds.device, dtype=torch.float32)
        keep = None if strength < 1 else pipe.latent_keep_mask(2, (256, 16), time_mask_ratio_start_and_end=ratios)
        kw = dict(uncond_states=embeds_cf[:2], uncond_mask=mask_cf[:2]) if post > 1 else {}
        want = pipe.edit_from_embeds(embeds, mask, noise, wav, keep, strength, W_IN, post, 2, **kw)
        assert got.dtype == np.int16 and got.shape == (2, int(16000 * 9.5)) and np.array_equal(got, want)
    with pytest.raises(ValueError, match="source_wav"):
        pipe.edit(prompts, wav[:1])
