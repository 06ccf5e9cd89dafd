"""Long and short clips with the consistency student (ConsistencyTTA.generate_long_latent, generate_long_from_embeds,
capture_long_graph): the one-pass step kernel against the unfused chain it replaces, bit for bit; its refusals; the eager
sampler against `generate_latent` (one window) and against the plain torch restatement tests/long_ref.py (several); windows
with their own text states; the captured path against the eager one; the waveform entry against its manual chain, chunked
and not; and the VAE decoder and HiFi-GAN away from 256 rows, at real width, against the fp32 oracle with the bounds of
tests/test_engines_gpu.py.  Everything but the last is exact: the feature is a composition of steps other tests pin to the
reference, plus one weighted overlap-add."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
import edit_ref  # noqa: E402
import long_ref  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from consistencytta_amd import spec  # noqa: E402
from consistencytta_amd.models import LONG_DECODE_ROWS, LONG_MAX_LATENT_H, _long_latent_h  # noqa: E402

DEV = "cuda:0"
B, L, C, WH, W = 2, 7, 8, 32, 16
W_IN = 4.0
NULL = N.c_void_p(0)
INVALID = 1
KERNEL_PLANS = [(80, 32, 8), (48, 32, 24), (40, 32, 24), (32, 32, 8)]


def _pipe(**kw):
    from consistencytta_amd import modules
    from consistencytta_amd.models import ConsistencyTTA
    cfg = dict(cases.TINY_UNET)
    vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    pipe = ConsistencyTTA(unet_config=cfg, vae=vae, **kw)
    pipe.to(DEV)
    pipe.unet.init_deterministic(1)
    vae.init_deterministic(2)
    pipe.eval().requires_grad_(False)
    return pipe, cfg


@pytest.fixture(scope="module")
def shared():
    """One pipe for the tests that only run eager calls (a capture gets its own)."""
    return _pipe()


def _noise(steps, Ht, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((steps, B, C, Ht, W), generator=g).to(DEV)


def _states(cfg, tag, rows=B):
    _, _, _, enc, mask = cases.unet_inputs(cfg, rows, WH, W, L, tag)
    return enc.to(DEV), mask.to(DEV)


def _uncond(cfg, tag, rows=B):
    u = cases.t(spec.det_uniform(tag + ".unc", (rows, L, cfg["cross_attention_dim"]), 12)) * 0.5
    m = torch.zeros(rows, L, dtype=torch.bool)
    m[:, :2] = True
    return u.to(DEV), m.to(DEV)


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


# --------------------------------------------------------------------------------------------------- 1: the kernel
def _fuse(cond, unc, w, starts, weights, nz, sig, x0_long, out, copies, batch, n, channels, wh, Ht, width):
    host = (N.c_int32 * len(starts))(*starts)
    return N.lib().ctta_window_fuse_renoise(N.ptr(cond), N.ptr(unc), N.ptr(w), host, N.ptr(weights), N.ptr(nz), N.ptr(sig),
                                            N.ptr(x0_long), N.ptr(out), copies, batch, n, channels, wh, Ht, width,
                                            N.stream_ptr())


def _guarded(numel):
    """A NaN buffer of `numel` floats followed by 256 sentinel floats."""
    buf = torch.full((numel + 256,), float("nan"), device=DEV)
    buf[numel:] = 12345.0
    return buf


@pytest.mark.parametrize("channels", [1, 8])
@pytest.mark.parametrize("width", [4, 16])
@pytest.mark.parametrize("plan", KERNEL_PLANS)
def test_window_fuse_kernel_equals_the_unfused_sequence_bit_for_bit(plan, width, channels):
    """Slices, torch's (1 - w) * u + w * c per window, torch's weighted sum over the windows of a row (mul, then add in
    ascending window order), ctta_heun_add_noise, ctta_heun_scale_model_input on the long tensor, the cut into windows and
    torch.cat against the one-pass kernel: copies 1 and 2; cond alone, uncond + cond, cond == NULL (x0 = 0); per-row w in
    {1, 2, 0.5}, per-row sigmas (sigma_max, 0, an inner one); the end form, which writes x0_long alone.  `out` and `x0_long`
    start as NaN and are each followed by 256 sentinel floats."""
    from consistencytta_amd.models import ConsistencyTTA
    L_ = N.lib()
    Ht, wh0, overlap = plan
    starts, weights = ConsistencyTTA.long_plan(Ht, wh0, overlap)
    ref_starts, ref_weights = long_ref.plan(Ht, wh0, overlap)
    assert starts == ref_starts and torch.equal(weights, ref_weights)
    n, wh = weights.shape
    wdev = weights.to(DEV)
    Bk = 3
    g = torch.Generator().manual_seed(Ht + width + channels)
    c, u = (torch.randn(Bk * n, channels, wh, width, generator=g).to(DEV) for _ in range(2))
    nz = torch.randn(Bk, channels, Ht, width, generator=g).to(DEV)
    sig = torch.tensor([14.6146, 0.0, 0.7], dtype=torch.float32, device=DEV)
    w = torch.tensor([1.0, 2.0, 0.5], dtype=torch.float32, device=DEV)
    wr = w.repeat_interleave(n).view(-1, 1, 1, 1)                   # row b * n + k takes w[b]
    n_long, n_win = Bk * channels * Ht * width, Bk * n * channels * wh * width
    for mode in ("cond", "cfg", "zero"):
        xw = {"cond": c, "cfg": (1 - wr) * u + wr * c, "zero": torch.zeros_like(c)}[mode]
        x0 = long_ref.fuse(xw, ref_starts, ref_weights, Ht)
        z, scaled = torch.empty_like(x0), torch.empty_like(x0)
        N.check(L_.ctta_heun_add_noise(N.ptr(x0), N.ptr(nz), N.ptr(sig), N.ptr(z), Bk, x0[0].numel(), N.stream_ptr()))
        N.check(L_.ctta_heun_scale_model_input(N.ptr(z), N.ptr(sig), N.ptr(scaled), Bk, x0[0].numel(), N.stream_ptr()))
        ref1 = long_ref.cut(scaled, ref_starts, wh)
        assert bool(torch.isfinite(ref1).all()) and tuple(ref1.shape) == tuple(c.shape)
        cond, unc, ww = {"cond": (c, None, None), "cfg": (c, u, w), "zero": (None, None, None)}[mode]
        for copies in (1, 2):
            for with_long in (False, True):
                out, lng = _guarded(copies * n_win), _guarded(n_long)
                N.check(_fuse(cond, unc, ww, starts, wdev, nz, sig, lng if with_long else None, out, copies, Bk, n, channels,
                              wh, Ht, width))
                got = out[:copies * n_win].view((copies * Bk * n,) + tuple(c.shape[1:]))
                assert not bool(torch.isnan(got).any()), (mode, copies)
                assert torch.equal(_bits(got), _bits(torch.cat([ref1] * copies))), (mode, copies)
                assert bool((out[copies * n_win:] == 12345.0).all()), (mode, copies)
                if with_long:
                    assert torch.equal(_bits(lng[:n_long].view_as(x0)), _bits(x0)), (mode, copies)
                else:
                    assert bool(torch.isnan(lng[:n_long]).all())
                assert bool((lng[n_long:] == 12345.0).all()), (mode, copies)
        lng = _guarded(n_long)                                       # the end: nothing is re-noised
        N.check(_fuse(cond, unc, ww, starts, wdev, None, None, lng, None, 1, Bk, n, channels, wh, Ht, width))
        assert not bool(torch.isnan(lng[:n_long]).any()), mode
        assert torch.equal(_bits(lng[:n_long].view_as(x0)), _bits(x0)), mode
        assert bool((lng[n_long:] == 12345.0).all()), mode


def test_window_fuse_kernel_refuses_before_launch():
    Bk, ch, wh, Ht, width = 2, 2, 32, 80, 8
    starts = [0, 24, 48]
    n = len(starts)
    c, u = (torch.ones(Bk * n, ch, wh, width, device=DEV) for _ in range(2))
    nz = torch.ones(Bk, ch, Ht, width, device=DEV)
    weights = torch.ones(17, wh, device=DEV)
    sig, w = torch.ones(Bk, device=DEV), torch.ones(Bk, device=DEV)
    out = torch.full((2 * c.numel() + 256,), float("nan"), device=DEV)
    lng = torch.full((nz.numel() + 256,), float("nan"), device=DEV)

    def call(cond=c, unc=None, ww=None, st=starts, noise=nz, sigma=sig, x0_long=lng, o=out, copies=1, n_=None, Ht_=Ht,
             width_=width):
        return _fuse(cond, unc, ww, st, weights, noise, sigma, x0_long, o, copies, Bk, len(st) if n_ is None else n_, ch, wh,
                     Ht_, width_)

    assert call() == 0                                   # the arguments every refusal below departs from
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[:c.numel()]).any())
    out.fill_(float("nan"))
    lng.fill_(float("nan"))
    refusals = [
        (dict(st=[8, 24, 48]), r"starts\[0\]"),
        (dict(st=[0, 24, 40]), "last start"),
        (dict(st=[0, 24, 48], Ht_=88), "last start"),
        (dict(st=[0, 24, 24, 48]), "strictly increasing"),
        (dict(st=[0, 30, 24, 48]), "strictly increasing"),
        (dict(st=[0, 8, 48]), "gap"),
        (dict(st=list(range(0, 51, 3))), "n_windows"),   # 17 windows
        (dict(st=[0, 24, 48], n_=0), "n_windows"),
        (dict(width_=6), "width"),
        (dict(copies=0), "copies"),
        (dict(copies=3), "copies"),
        (dict(unc=u), "uncond and w_post"),
        (dict(ww=w), "uncond and w_post"),
        (dict(cond=None, unc=u, ww=w), "uncond without cond"),
        (dict(noise=None), "noise and out"),
        (dict(o=None), "noise and out"),
        (dict(noise=None, o=None, x0_long=None), "x0_long"),
        (dict(sigma=None), "sigma"),
    ]
    for kw, what in refusals:
        assert call(**kw) == INVALID, kw
        with pytest.raises(N.CttaError, match=what):
            N.check(call(**kw))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(lng).all())                    # nothing was launched


# ------------------------------------------------------------------------------------------ 2: the sampler, one window
STEPS_POST = [(s, p) for s in (1, 2, 4) for p in (1.0, 2.0, 1.3)]


def _kw(cfg, post, tag, rows=B):
    if post <= 1:
        return {}
    unc, unc_mask = _uncond(cfg, tag, rows)
    return dict(uncond_states=unc, uncond_mask=unc_mask)


@pytest.mark.parametrize("steps,post", STEPS_POST)
def test_one_window_of_the_models_height_is_plain_generation(shared, steps, post):
    pipe, cfg = shared
    enc, mask = _states(cfg, "long2")
    noise = _noise(steps, WH, 200 + steps)
    kw = _kw(cfg, post, "long2")
    plain = pipe.generate_latent(enc, mask, noise[0], W_IN, post, steps, step_noise=noise[1:], **kw)
    got = pipe.generate_long_latent(enc, mask, noise[0], W_IN, post, steps, overlap=8, window_h=WH, step_noise=noise[1:], **kw)
    assert bool(torch.isfinite(plain).all()) and torch.equal(got, plain)


# ---------------------------------------------------------------------------- 3: the eager path against the restatement
def _query(pipe, enc_rows, mask_rows, post, unc_rows=None, unc_mask_rows=None):
    """The guided student with its post-CFG combine on B * n window rows, plain torch around pipe.unet."""
    def query(z_in, t):
        if post > 1:
            zh = pipe.unet(torch.cat([z_in] * 2), t, guidance=W_IN, encoder_hidden_states=torch.cat([unc_rows, enc_rows]),
                           encoder_attention_mask=torch.cat([unc_mask_rows, mask_rows])).sample
            u, c = zh.chunk(2)
            return (1 - post) * u + post * c
        return pipe.unet(z_in, t, guidance=W_IN, encoder_hidden_states=enc_rows, encoder_attention_mask=mask_rows).sample
    return query


@pytest.mark.parametrize("steps,post", STEPS_POST)
@pytest.mark.parametrize("Ht,overlap", [(80, 8), (48, 24)])
def test_eager_long_latent_equals_the_plain_torch_restatement(shared, Ht, overlap, steps, post):
    """post = 1.3 keeps torch's combine in front of the kernel (models._post_cfg_fusable)."""
    from consistencytta_amd.models import _post_cfg_fusable
    assert _post_cfg_fusable(2.0) and not _post_cfg_fusable(1.3)
    pipe, cfg = shared
    n = len(long_ref.plan(Ht, WH, overlap)[0])
    assert n == 3
    enc, mask = _states(cfg, "long3")
    noise = _noise(steps, Ht, 210 + steps)
    kw = _kw(cfg, post, "long3")
    rep = lambda x: None if x is None else x.repeat_interleave(n, 0)                         # noqa: E731
    query = _query(pipe, rep(enc), rep(mask), post, rep(kw.get("uncond_states")), rep(kw.get("uncond_mask")))
    times, sigmas = edit_ref.schedule(pipe.scheduler, steps)
    want = long_ref.long_sampler(query, times, sigmas, noise[0], WH, overlap, noise[1:])
    got = pipe.generate_long_latent(enc, mask, noise[0], W_IN, post, steps, overlap=overlap, window_h=WH,
                                    step_noise=noise[1:], **kw)
    assert tuple(got.shape) == (B, C, Ht, W) and bool(torch.isfinite(want).all())
    assert torch.equal(got, want)


def test_internal_draws_are_long_draws_from_the_global_generator(shared):
    pipe, cfg = shared
    enc, mask = _states(cfg, "long3b")
    noise = _noise(1, 80, 220)
    torch.manual_seed(5)
    a = pipe.generate_long_latent(enc, mask, noise[0], W_IN, 1.0, 3, overlap=8, window_h=WH)
    torch.manual_seed(5)
    draws = torch.stack([torch.randn_like(noise[0]), torch.randn_like(noise[0])])
    b = pipe.generate_long_latent(enc, mask, noise[0], W_IN, 1.0, 3, overlap=8, window_h=WH, step_noise=draws)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------- 4: windows with their own text states
@pytest.mark.parametrize("post", [1.0, 2.0])
def test_per_window_text_states(shared, post):
    """B * n rows of text states give every window its own: equal to the repeated form when the rows are the repeats; when
    one window's states differ, a one-step call changes the rows that window covers and no others."""
    pipe, cfg = shared
    Ht, overlap, n = 80, 8, 3
    enc, mask = _states(cfg, "long4")
    noise = _noise(2, Ht, 230)
    kw = _kw(cfg, post, "long4")
    args = dict(overlap=overlap, window_h=WH)
    for steps in (1, 2):
        base = pipe.generate_long_latent(enc, mask, noise[0], W_IN, post, steps, step_noise=noise[1:steps], **kw, **args)
        enc_n, mask_n = enc.repeat_interleave(n, 0), mask.repeat_interleave(n, 0)
        kw_n = {k: v.repeat_interleave(n, 0) for k, v in kw.items()}
        same = pipe.generate_long_latent(enc_n, mask_n, noise[0], W_IN, post, steps, step_noise=noise[1:steps], **kw_n, **args)
        assert torch.equal(same, base)
    other, _ = _states(cfg, "long4_other")
    enc_n = enc.repeat_interleave(n, 0)
    enc_n[1 * n + 2] = other[1]                          # clip 1, window 2: rows 48 .. 79
    base = pipe.generate_long_latent(enc, mask, noise[0], W_IN, post, 1, **kw, **args)
    got = pipe.generate_long_latent(enc_n, mask.repeat_interleave(n, 0), noise[0], W_IN, post, 1, **kw, **args)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1, :, :48], base[1, :, :48])
    assert not torch.equal(got[1, :, 48:], base[1, :, 48:])
    assert float((got[1, :, 56:] - base[1, :, 56:]).abs().max()) > 1e-6


# ------------------------------------------------------------------------------------------------ 5: the captured path
DURATION = 3.0                                           # 80 rows: three windows of 32 with 8 shared


def _eager_long(pipe, enc, mask, noise, post, steps, kw, duration=DURATION, overlap=8, **extra):
    return pipe.generate_long_from_embeds(enc, mask, noise[0], duration, W_IN, post, steps, step_noise=noise[1:],
                                          overlap=overlap, window_h=WH, **kw, **extra)


@pytest.mark.parametrize("steps,post", [(4, 1.0), (2, 2.0), (1, 1.3)])
def test_captured_long_graph_equals_the_eager_path(steps, post):
    pipe, cfg = _pipe()
    kw = _kw(cfg, post, "long5")
    inputs = [_states(cfg, "long5_0") + (_noise(steps, 80, 240),), _states(cfg, "long5_1") + (_noise(steps, 80, 241),)]
    refs = []
    for enc, mask, noise in inputs:
        lat = pipe.generate_long_latent(enc, mask, noise[0], W_IN, post, steps, overlap=8, window_h=WH, step_noise=noise[1:],
                                        **kw)
        refs.append((lat.clone(), _eager_long(pipe, enc, mask, noise, post, steps, kw)))
    assert refs[0][1].shape == (B, int(16000 * DURATION)) and not np.array_equal(refs[0][1], refs[1][1])
    gen = pipe.capture_long_graph(B, L, DURATION, cfg_scale_input=W_IN, num_steps=steps, cfg_scale_post=post, overlap=8,
                                  window_h=WH, cross_attention_dim=cfg["cross_attention_dim"], latent_cw=(C, W), **kw)
    assert gen.latent_h == 80
    for (enc, mask, noise), (lat, pcm) in list(zip(inputs, refs)) + [(inputs[0], refs[0])]:
        before = [a.clone() for a in (enc, mask, noise)]
        out = gen(enc, mask, noise)
        assert out.dtype == torch.int16 and tuple(out.shape) == pcm.shape
        assert torch.equal(_bits(gen.outputs[0]), _bits(lat))
        assert np.array_equal(out.cpu().numpy(), pcm)
        for a, b in zip((enc, mask, noise), before):     # copied in, never held or written
            assert torch.equal(a, b)
    with pytest.raises(ValueError):
        gen(inputs[0][0], inputs[0][1], inputs[0][2][:, :, :, :32])                          # window-sized noise


# ----------------------------------------------------------------------------------------------- 6: the waveform entry
def test_generate_long_from_embeds_equals_the_manual_chain_chunked_or_not(shared):
    pipe, cfg = shared
    duration, Ht = 3.3, 88                               # no multiple of 2.5 s; 84.48 rows round up to 88: four windows
    enc, mask = _states(cfg, "long6")
    noise = _noise(2, Ht, 250)
    got = _eager_long(pipe, enc, mask, noise, 1.0, 2, {}, duration)
    lat = pipe.generate_long_latent(enc, mask, noise[0], W_IN, 1.0, 2, overlap=8, window_h=WH, step_noise=noise[1:])
    assert tuple(lat.shape) == (B, C, Ht, W)
    full = pipe.vae.decode_to_waveform(pipe.vae.decode_first_stage(lat))
    assert int(16000 * duration) == 52800 <= full.shape[1]
    assert got.dtype == np.int16 and got.shape == (B, 52800) and np.array_equal(got, full[:, :52800])
    # one clip per decoder call: the centring still spans the batch
    chunked = _eager_long(pipe, enc, mask, noise, 1.0, 2, {}, duration, _chunk_rows=Ht)
    assert np.array_equal(chunked, got)
    with pytest.raises(ValueError, match="noise"):
        _eager_long(pipe, enc, mask, noise, 1.0, 2, {}, 3.0)


# ------------------------------------------------------------------ 7: the decoder away from 256 rows, at real width, B = 1
def test_vae_decoder_and_hifigan_at_264_rows_against_the_oracle():
    """A 264 x 16 latent is 4224 tokens in the VAE mid-block: none of the 4096 / 2048 / 1024 row-softmax forms and no
    multiple of 256; its mel has 1056 frames.  Same helper and bounds as the full-width comparisons of test_engines_gpu."""
    from oracle import nets as onets
    from test_engines_gpu import REL_L2, REL_MAX, _check, _vae
    assert (REL_L2, REL_MAX) == (2.5e-2, 6e-2)
    assert _long_latent_h(10.24) == 264 <= LONG_MAX_LATENT_H and LONG_DECODE_ROWS // 264 >= 1      # what a 10.24 s clip asks for
    v, sd = _vae(spec.VAE_DDCONFIG, spec.HIFIGAN_16K_64)
    z = cases.vae_inputs(1, 264, 16, "vae_long")
    mel = v.decode_first_stage(z.to(DEV))
    assert tuple(mel.shape) == (1, 1, 1056, 64)
    with torch.no_grad():
        ref = onets.vae_decode(spec.VAE_DDCONFIG, sd, z, v.scale_factor)
    _check("vae 264 x 16 mel vs oracle", mel, ref)
    mel_in = cases.mel_inputs(1, 1056, 64, "hifigan_long")
    wav = v.vocode(mel_in.to(DEV))
    with torch.no_grad():
        wref = onets.hifigan_forward(spec.HIFIGAN_16K_64, sd, mel_in.squeeze(1).permute(0, 2, 1)).squeeze(1)
    assert tuple(wav.shape) == tuple(wref.shape) and wav.shape[1] >= 1056 * 160            # plus the transposed convs' tails
    _check("hifigan 1056 frames wav vs oracle", wav, wref)
