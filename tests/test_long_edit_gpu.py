"""Editing long clips with the consistency student (ConsistencyTTA.edit_long_latent, edit_long_from_embeds, extend,
capture_long_edit_graph): the one-pass step kernel against the unfused chain it replaces, bit for bit; its two reductions
(one window is the edit kernels, keep == 0 is the plain fusion); its refusals; the eager sampler against the plain torch
restatement tests/long_edit_ref.py; the sampler's identities; the captured path against the eager one; the waveform entries
against their manual chains.  No tolerance anywhere: the feature is an exact composition of steps other tests pin to the
reference, plus one blend on the fused latent."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
import edit_ref  # noqa: E402
import long_edit_ref  # noqa: E402
import long_ref  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from consistencytta_amd import spec  # noqa: E402

DEV = "cuda:0"
B, L, C, WH, W = 2, 7, 8, 32, 16
W_IN = 4.0
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
    sd = vae.state_dict()
    sd.update(cases.vae_encoder_weights(cases.TINY_VAE_DD))
    vae.load_state_dict(sd)
    pipe.eval().requires_grad_(False)
    return pipe, cfg


@pytest.fixture(scope="module")
def shared():
    """One pipe for the tests that only run eager calls (a capture gets its own)."""
    return _pipe()


def _noise(steps, Ht, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((steps, B, C, Ht, W), generator=g).to(DEV)


def _source(Ht, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B, C, Ht, W), generator=g) * 0.8).to(DEV)


def _states(cfg, tag, rows=B):
    _, _, _, enc, mask = cases.unet_inputs(cfg, rows, WH, W, L, tag)
    return enc.to(DEV), mask.to(DEV)


def _uncond(cfg, tag, rows=B):
    u = cases.t(spec.det_uniform(tag + ".unc", (rows, L, cfg["cross_attention_dim"]), 12)) * 0.5
    m = torch.zeros(rows, L, dtype=torch.bool)
    m[:, :2] = True
    return u.to(DEV), m.to(DEV)


def _kw(cfg, post, tag):
    if post <= 1:
        return {}
    unc, unc_mask = _uncond(cfg, tag)
    return dict(uncond_states=unc, uncond_mask=unc_mask)


def _time_mask(Ht, a, b, rows=B):
    """1 = keep; rows [a, b) are regenerated."""
    keep = torch.ones(rows, 1, Ht, W)
    keep[:, :, a:b] = 0
    return keep.to(DEV)


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


# --------------------------------------------------------------------------------------------------- 1: the kernel
def _fuse_edit(cond, unc, w, starts, weights, src, keep, nz, sig, x0_long, out, copies, batch, n, channels, wh, Ht, width):
    host = (N.c_int32 * len(starts))(*starts)
    return N.lib().ctta_window_fuse_edit_renoise(N.ptr(cond), N.ptr(unc), N.ptr(w), host, N.ptr(weights), N.ptr(src),
                                                 N.ptr(keep), N.ptr(nz), N.ptr(sig), N.ptr(x0_long), N.ptr(out), copies,
                                                 batch, n, channels, wh, Ht, width, N.stream_ptr())


def _fuse_plain(cond, unc, w, starts, weights, nz, sig, x0_long, out, copies, batch, n, channels, wh, Ht, width):
    host = (N.c_int32 * len(starts))(*starts)
    return N.lib().ctta_window_fuse_renoise(N.ptr(cond), N.ptr(unc), N.ptr(w), host, N.ptr(weights), N.ptr(nz), N.ptr(sig),
                                            N.ptr(x0_long), N.ptr(out), copies, batch, n, channels, wh, Ht, width,
                                            N.stream_ptr())


def _guarded(numel):
    """A NaN buffer of `numel` floats followed by 256 sentinel floats."""
    buf = torch.full((numel + 256,), float("nan"), device=DEV)
    buf[numel:] = 12345.0
    return buf


def _keep_planes(Bk, Ht, width, starts):
    """(Bk, Ht * width): per clip, ones down to a row boundary that lies inside the first overlap (two rows past the second
    window's start, one row later per clip), a four-row fractional ramp, zeros below; the last clip's plane also ramps over
    the columns, so a float4 holds four different values."""
    keep = torch.zeros(Bk, Ht, width)
    for b in range(Bk):
        edge = (starts[1] if len(starts) > 1 else 10) + 2 + b
        keep[b, :edge] = 1
        keep[b, edge:edge + 4] = torch.tensor([0.8, 0.6, 0.4, 0.2]).view(4, 1)
    keep[Bk - 1] *= torch.linspace(0.25, 1.0, width).view(1, width)
    assert bool((keep == 0).any()) and bool((keep == 1).any()) and bool(((keep > 0) & (keep < 1)).any())
    return keep.reshape(Bk, Ht * width).to(DEV)


def _kernel_inputs(plan, width, channels):
    from consistencytta_amd.models import ConsistencyTTA
    Ht, wh0, overlap = plan
    starts, weights = ConsistencyTTA.long_plan(Ht, wh0, overlap)
    ref_starts, ref_weights = long_ref.plan(Ht, wh0, overlap)
    assert starts == ref_starts and torch.equal(weights, ref_weights)
    n, wh = weights.shape
    Bk = 3
    g = torch.Generator().manual_seed(Ht + width + channels + 1)
    c, u = (torch.randn(Bk * n, channels, wh, width, generator=g).to(DEV) for _ in range(2))
    nz, src = (torch.randn(Bk, channels, Ht, width, generator=g).to(DEV) for _ in range(2))
    sig = torch.tensor([14.6146, 0.0, 0.7], dtype=torch.float32, device=DEV)
    w = torch.tensor([1.0, 2.0, 0.5], dtype=torch.float32, device=DEV)
    keep = _keep_planes(Bk, Ht, width, starts)
    return Bk, Ht, n, wh, starts, weights, weights.to(DEV), c, u, nz, src, sig, w, keep


def _windows(mode, c, u, w, n):
    wr = w.repeat_interleave(n).view(-1, 1, 1, 1)                   # row b * n + k takes w[b]
    return {"cond": c, "cfg": (1 - wr) * u + wr * c, "zero": torch.zeros_like(c)}[mode]


def _args(mode, c, u, w):
    return {"cond": (c, None, None), "cfg": (c, u, w), "zero": (None, None, None)}[mode]


@pytest.mark.parametrize("channels", [1, 8])
@pytest.mark.parametrize("width", [4, 16])
@pytest.mark.parametrize("plan", KERNEL_PLANS)
def test_window_fuse_edit_kernel_equals_the_unfused_sequence_bit_for_bit(plan, width, channels):
    """torch's (1 - w) * u + w * c per window, long_ref.fuse, torch's keep * src + (1 - keep) * x0 on the long tensor,
    ctta_heun_add_noise, ctta_heun_scale_model_input, the cut into windows and torch.cat against the one-pass kernel:
    copies 1 and 2; cond alone, uncond + cond, cond == NULL (the start); per-row w in {1, 2, 0.5}, per-row sigmas (sigma_max,
    0, an inner one); with and without x0_long; the end form, which writes x0_long alone.  The planes hold 0, 1 and
    fractions with their row boundary inside an overlap.  `out` and `x0_long` start as NaN and are each followed by 256
    sentinel floats."""
    L_ = N.lib()
    Bk, Ht, n, wh, starts, weights, wdev, c, u, nz, src, sig, w, keep = _kernel_inputs(plan, width, channels)
    keep4 = keep.view(Bk, 1, Ht, width)
    n_long, n_win = Bk * channels * Ht * width, Bk * n * channels * wh * width
    for mode in ("cond", "cfg", "zero"):
        x0 = long_ref.fuse(_windows(mode, c, u, w, n), starts, weights, Ht)
        x0 = keep4 * src + (1 - keep4) * x0
        z, scaled = torch.empty_like(x0), torch.empty_like(x0)
        N.check(L_.ctta_heun_add_noise(N.ptr(x0), N.ptr(nz), N.ptr(sig), N.ptr(z), Bk, x0[0].numel(), N.stream_ptr()))
        N.check(L_.ctta_heun_scale_model_input(N.ptr(z), N.ptr(sig), N.ptr(scaled), Bk, x0[0].numel(), N.stream_ptr()))
        ref1 = long_ref.cut(scaled, starts, wh)
        assert bool(torch.isfinite(ref1).all()) and tuple(ref1.shape) == tuple(c.shape)
        cond, unc, ww = _args(mode, c, u, w)
        for copies in (1, 2):
            for with_long in (False, True):
                out, lng = _guarded(copies * n_win), _guarded(n_long)
                N.check(_fuse_edit(cond, unc, ww, starts, wdev, src, keep, nz, sig, lng if with_long else None, out, copies,
                                   Bk, n, channels, wh, Ht, width))
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
        N.check(_fuse_edit(cond, unc, ww, starts, wdev, src, keep, None, None, lng, None, 1, Bk, n, channels, wh, Ht, width))
        assert not bool(torch.isnan(lng[:n_long]).any()), mode
        assert torch.equal(_bits(lng[:n_long].view_as(x0)), _bits(x0)), mode
        assert bool((lng[n_long:] == 12345.0).all()), mode


# --------------------------------------------------------------------------------------------------- 2: the reductions
@pytest.mark.parametrize("channels,width", [(1, 4), (8, 16)])
def test_one_window_is_the_edit_kernels_bit_for_bit(channels, width):
    """latent_h == window_h: a step is ctta_consistency_edit_renoise, the end is ctta_cfg_combine_keep."""
    L_ = N.lib()
    Bk, Ht, n, wh, starts, weights, wdev, c, u, nz, src, sig, w, keep = _kernel_inputs((32, 32, 8), width, channels)
    assert n == 1 and wh == Ht and bool((weights == 1).all())
    per, hw = channels * Ht * width, Ht * width
    for mode in ("cond", "cfg", "zero"):
        cond, unc, ww = _args(mode, c, u, w)
        for copies in (1, 2):
            want, got = torch.empty(copies * Bk * per, device=DEV), torch.empty(copies * Bk * per, device=DEV)
            N.check(L_.ctta_consistency_edit_renoise(N.ptr(cond), N.ptr(unc), N.ptr(ww), N.ptr(src), N.ptr(keep), N.ptr(nz),
                                                     N.ptr(sig), N.ptr(want), copies, Bk, per, hw, N.stream_ptr()))
            N.check(_fuse_edit(cond, unc, ww, starts, wdev, src, keep, nz, sig, None, got, copies, Bk, 1, channels, wh, Ht,
                               width))
            assert bool(torch.isfinite(want).all()) and torch.equal(_bits(got), _bits(want)), (mode, copies)
        if mode == "zero":
            continue
        want, got = torch.empty(Bk * per, device=DEV), torch.empty(Bk * per, device=DEV)
        N.check(L_.ctta_cfg_combine_keep(N.ptr(unc), N.ptr(cond), N.ptr(ww), N.ptr(src), N.ptr(keep), N.ptr(want), Bk, per, hw,
                                         N.stream_ptr()))
        N.check(_fuse_edit(cond, unc, ww, starts, wdev, src, keep, None, None, got, None, 1, Bk, 1, channels, wh, Ht, width))
        assert torch.equal(_bits(got), _bits(want)), mode


@pytest.mark.parametrize("plan", [(80, 32, 8), (48, 32, 24)])
def test_a_zero_plane_is_the_plain_fusion_as_values(plan):
    """0 * src + 1 * x0 is x0 for a finite source, but for the sign of a zero: the blend turns the fusion's -0 into +0, so
    the floats are compared, not the bits."""
    Bk, Ht, n, wh, starts, weights, wdev, c, u, nz, src, sig, w, _ = _kernel_inputs(plan, 16, 8)
    zero = torch.zeros(Bk, Ht * 16, device=DEV)
    n_long, n_win = Bk * 8 * Ht * 16, Bk * n * 8 * wh * 16
    for mode in ("cond", "cfg", "zero"):
        cond, unc, ww = _args(mode, c, u, w)
        outs = []
        for fuse in (lambda *a: _fuse_plain(cond, unc, ww, starts, wdev, *a),
                     lambda *a: _fuse_edit(cond, unc, ww, starts, wdev, src, zero, *a)):
            out, lng, end = torch.empty(2 * n_win, device=DEV), torch.empty(n_long, device=DEV), torch.empty(n_long, device=DEV)
            N.check(fuse(nz, sig, lng, out, 2, Bk, n, 8, wh, Ht, 16))
            N.check(fuse(None, None, end, None, 1, Bk, n, 8, wh, Ht, 16))
            outs.append((out, lng, end))
        for a, b in zip(*outs):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), mode


# --------------------------------------------------------------------------------------------------- 3: the refusals
def test_window_fuse_edit_kernel_refuses_before_launch():
    Bk, ch, wh, Ht, width = 2, 2, 32, 80, 8
    starts = [0, 24, 48]
    n = len(starts)
    c, u = (torch.ones(Bk * n, ch, wh, width, device=DEV) for _ in range(2))
    nz, src = (torch.ones(Bk, ch, Ht, width, device=DEV) for _ in range(2))
    keep = torch.full((Bk, Ht * width), 0.5, device=DEV)
    weights = torch.ones(17, wh, device=DEV)
    sig, w = torch.ones(Bk, device=DEV), torch.ones(Bk, device=DEV)
    out = torch.full((2 * c.numel() + 256,), float("nan"), device=DEV)
    lng = torch.full((nz.numel() + 256,), float("nan"), device=DEV)

    def call(cond=c, unc=None, ww=None, st=starts, s=src, k=keep, noise=nz, sigma=sig, x0_long=lng, o=out, copies=1, n_=None,
             Ht_=Ht, width_=width):
        return _fuse_edit(cond, unc, ww, st, weights, s, k, noise, sigma, x0_long, o, copies, Bk, len(st) if n_ is None else n_,
                          ch, wh, Ht_, width_)

    assert call() == 0                                   # the arguments every refusal below departs from
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[:c.numel()]).any()) and not bool(torch.isnan(lng[:nz.numel()]).any())
    out.fill_(float("nan"))
    lng.fill_(float("nan"))
    refusals = [
        (dict(s=None), "src_long and keep"),
        (dict(k=None), "src_long and keep"),
        (dict(s=None, k=None), "src_long and keep"),
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


# ------------------------------------------------------------------------------- 4: the eager path against the restatement
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


SAMPLER_CASES = [(4, 1.0, 1.0), (4, 0.5, 2.0), (2, 1.0, 1.3), (1, 1.0, 1.0)]


@pytest.mark.parametrize("steps,strength,post", SAMPLER_CASES)
@pytest.mark.parametrize("Ht,overlap", [(80, 8), (48, 24)])
def test_eager_long_edit_equals_the_plain_torch_restatement(shared, Ht, overlap, steps, strength, post):
    """post = 1.3 keeps torch's combine in front of the kernel (models._post_cfg_fusable); the mask's edge lies inside an
    overlap and one clip has a soft edge."""
    from consistencytta_amd.models import _post_cfg_fusable
    assert _post_cfg_fusable(2.0) and not _post_cfg_fusable(1.3)
    pipe, cfg = shared
    n = len(long_ref.plan(Ht, WH, overlap)[0])
    assert n == 3
    r = max(1, int(strength * steps))
    enc, mask = _states(cfg, "ledit4")
    noise, src = _noise(r, Ht, 310 + steps), _source(Ht, 20)
    keep = _time_mask(Ht, 28, Ht)                         # rows 24 .. 31 (80) / 16 .. 31 (48) lie under more than one window
    keep[1, :, 24:28] = 0.25
    kw = _kw(cfg, post, "ledit4")
    rep = lambda x: None if x is None else x.repeat_interleave(n, 0)                         # noqa: E731
    query = _query(pipe, rep(enc), rep(mask), post, rep(kw.get("uncond_states")), rep(kw.get("uncond_mask")))
    times, sigmas = edit_ref.schedule(pipe.scheduler, steps)
    want = long_edit_ref.long_edit_sampler(query, times, sigmas, noise[0], src, keep, WH, overlap, strength, noise[1:])
    got = pipe.edit_long_latent(enc, mask, noise[0], src, keep, strength, W_IN, post, steps, overlap=overlap, window_h=WH,
                                step_noise=noise[1:], **kw)
    assert tuple(got.shape) == (B, C, Ht, W) and bool(torch.isfinite(want).all())
    assert torch.equal(got, want)


# --------------------------------------------------------------------------------------------------- 5: behaviour
def test_everything_kept_returns_the_source_whatever_the_prompt(shared):
    pipe, cfg = shared
    noise, src = _noise(3, 80, 320), _source(80, 21)
    for tag, keep in (("ledit5a", torch.ones(B, 1, 80, W, device=DEV)), ("ledit5b", torch.ones(1, 1, 80, W, device=DEV))):
        enc, mask = _states(cfg, tag)
        got = pipe.edit_long_latent(enc, mask, noise[0], src, keep, 1.0, W_IN, 1.0, 3, overlap=8, window_h=WH,
                                    step_noise=noise[1:])
        assert torch.equal(got, src)


def test_a_time_mask_keeps_its_rows_and_regenerates_the_others(shared):
    """Rows [0, 32) of 80 are regenerated: the kept rows -- under the second and third windows, with the seam of the first
    overlap at their edge -- come back exactly."""
    pipe, cfg = shared
    enc, mask = _states(cfg, "ledit5c")
    noise, src = _noise(3, 80, 321), _source(80, 22)
    keep = pipe.latent_keep_mask(1, (80, W), time_mask_ratio_start_and_end=(0.0, 0.4))
    assert float(keep[0, 0, 31].max()) == 0 and float(keep[0, 0, 32].min()) == 1
    plain = pipe.generate_long_latent(enc, mask, noise[0], W_IN, 1.0, 3, overlap=8, window_h=WH, step_noise=noise[1:])
    got = pipe.edit_long_latent(enc, mask, noise[0], src, keep, 1.0, W_IN, 1.0, 3, overlap=8, window_h=WH,
                                step_noise=noise[1:])
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got[:, :, 32:], src[:, :, 32:])
    new = got[:, :, :32]
    assert float((new - src[:, :, :32]).abs().max()) > 1e-3 and float((new - plain[:, :, :32]).abs().max()) > 1e-6


@pytest.mark.parametrize("steps,post", [(1, 1.0), (3, 1.0), (3, 2.0), (2, 1.3)])
def test_nothing_kept_at_full_strength_is_long_generation(shared, steps, post):
    pipe, cfg = shared
    enc, mask = _states(cfg, "ledit5d")
    noise, src = _noise(steps, 80, 330 + steps), _source(80, 23)
    kw = _kw(cfg, post, "ledit5d")
    plain = pipe.generate_long_latent(enc, mask, noise[0], W_IN, post, steps, overlap=8, window_h=WH, step_noise=noise[1:],
                                      **kw)
    for keep in (None, torch.zeros(B, 1, 80, W, device=DEV)):
        got = pipe.edit_long_latent(enc, mask, noise[0], src, keep, 1.0, W_IN, post, steps, overlap=8, window_h=WH,
                                    step_noise=noise[1:], **kw)
        assert bool(torch.isfinite(plain).all()) and torch.equal(got, plain)


@pytest.mark.parametrize("steps,strength,post", SAMPLER_CASES)
def test_one_window_of_the_models_height_is_edit_latent_bit_for_bit(shared, steps, strength, post):
    pipe, cfg = shared
    r = max(1, int(strength * steps))
    enc, mask = _states(cfg, "ledit5e")
    noise, src = _noise(r, WH, 340 + steps), _source(WH, 24)
    keep = _time_mask(WH, 16, WH)
    keep[1, :, :4] = 0.25
    kw = _kw(cfg, post, "ledit5e")
    for k in (keep, None):
        want = pipe.edit_latent(enc, mask, noise[0], src, k, strength, W_IN, post, steps, step_noise=noise[1:], **kw)
        got = pipe.edit_long_latent(enc, mask, noise[0], src, k, strength, W_IN, post, steps, overlap=8, window_h=WH,
                                    step_noise=noise[1:], **kw)
        assert bool(torch.isfinite(want).all()) and torch.equal(_bits(got), _bits(want))


def test_internal_draws_are_long_draws_from_the_global_generator(shared):
    pipe, cfg = shared
    enc, mask = _states(cfg, "ledit5f")
    noise, src = _noise(1, 80, 350), _source(80, 25)
    keep = _time_mask(80, 0, 40, 1)
    torch.manual_seed(5)
    a = pipe.edit_long_latent(enc, mask, noise[0], src, keep, 1.0, W_IN, 1.0, 3, overlap=8, window_h=WH)
    torch.manual_seed(5)
    draws = torch.stack([torch.randn_like(noise[0]), torch.randn_like(noise[0])])
    b = pipe.edit_long_latent(enc, mask, noise[0], src, keep, 1.0, W_IN, 1.0, 3, overlap=8, window_h=WH, step_noise=draws)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 6: the captured path
DURATION = 3.0                                           # 80 rows: three windows of 32 with 8 shared
SAMPLES = int(16000 * DURATION)


def _eager(pipe, enc, mask, noise, src, keep, strength, post, steps, kw):
    lat = pipe.edit_long_latent(enc, mask, noise[0], src, keep, strength, W_IN, post, steps, overlap=8, window_h=WH,
                                step_noise=noise[1:], **kw)
    _, pcm = pipe._decode_long(lat)
    return lat.clone(), pcm[:, :SAMPLES].cpu().numpy()


def _capture(pipe, cfg, steps, strength, post, kw, **extra):
    return pipe.capture_long_edit_graph(B, L, DURATION, num_steps=steps, strength=strength, cfg_scale_input=W_IN,
                                        cfg_scale_post=post, overlap=8, window_h=WH,
                                        cross_attention_dim=cfg["cross_attention_dim"], latent_cw=(C, W), **kw, **extra)


@pytest.mark.parametrize("steps,strength,post", [(4, 1.0, 1.0), (4, 0.5, 2.0), (2, 1.0, 1.3)])
def test_captured_long_edit_graph_equals_the_eager_path(steps, strength, post):
    """Three replays: another source and another mask each time ((B, 1, Ht, W), (1, 1, Ht, W) with a soft edge, None)."""
    pipe, cfg = _pipe()
    r = max(1, int(strength * steps))
    kw = _kw(cfg, post, "ledit6")
    soft = _time_mask(80, 0, 28, 1)
    soft[:, :, 28:31, 8:] = 0.5
    inputs = [_states(cfg, "ledit6_0") + (_noise(r, 80, 360), _source(80, 26), _time_mask(80, 28, 80)),
              _states(cfg, "ledit6_1") + (_noise(r, 80, 361), _source(80, 27), soft),
              _states(cfg, "ledit6_2") + (_noise(r, 80, 362), _source(80, 28), None)]
    refs = [_eager(pipe, e, m, nz, s, k, strength, post, steps, kw) for e, m, nz, s, k in inputs]
    assert refs[0][1].shape == (B, SAMPLES) and not np.array_equal(refs[0][1], refs[1][1])
    gen = _capture(pipe, cfg, steps, strength, post, kw)
    assert gen.queries == r and gen.latent_h == 80
    for args, (lat, pcm) in list(zip(inputs, refs)) + [(inputs[0], refs[0])]:
        before = [None if a is None else a.clone() for a in args]
        out = gen(*args)
        assert out.dtype == torch.int16 and tuple(out.shape) == pcm.shape
        assert torch.equal(_bits(gen.outputs[0]), _bits(lat))
        assert np.array_equal(out.cpu().numpy(), pcm)
        for a, b in zip(args, before):                   # copied in, never held or written
            assert a is None or torch.equal(a, b)
    with pytest.raises(ValueError):
        gen(*inputs[0][:3], inputs[0][3][:, :, :32], inputs[0][4])                        # a window-sized source
    with pytest.raises(ValueError):
        gen(*inputs[0][:4], torch.ones(B, 80, W, device=DEV))                             # a mask without its channel axis
    if r > 1:
        with pytest.raises(ValueError):
            gen(inputs[0][0], inputs[0][1], inputs[0][2][0], inputs[0][3], inputs[0][4])  # one draw where r are due


def test_seeded_capture_equals_the_noise_fed_capture_given_seeded_noise():
    pipe, cfg = _pipe()
    steps, strength = 4, 0.5
    enc, mask = _states(cfg, "ledit6s")
    src, keep = _source(80, 29), _time_mask(80, 28, 80, 1)
    seeds, samples = [11, 2 ** 40 + 5], [0, 3]
    noise = pipe.seeded_noise(seeds, 2, (C, 80, W), samples)
    fed = _capture(pipe, cfg, steps, strength, 1.0, {})
    want = fed(enc, mask, noise, src, keep).clone()
    lat = fed.outputs[0].clone()
    seeded = _capture(pipe, cfg, steps, strength, 1.0, {}, seeded=True)
    got = seeded(enc, mask, seeds, src, keep, samples=samples)
    assert torch.equal(_bits(seeded.outputs[0]), _bits(lat)) and torch.equal(got, want)
    seeded(enc, mask, [12, 2 ** 40 + 5], src, keep, samples=samples)
    assert not torch.equal(seeded.outputs[0][0], lat[0])                                    # another seed, another clip


# ----------------------------------------------------------------------------------------------- 7: the waveform entries
def _encode_chunked(pipe, wav, rows, per):
    """The source latent by hand: fbank at 4 * rows frames, the encoder's posterior mean, `per` clips per encoder call."""
    from consistencytta_amd import audio
    stft = audio.TacotronSTFT(1024, 160, 1024, 64, 16000, 0, 8000).to(DEV)
    parts = []
    for i in range(0, wav.shape[0], per):
        mel, _ = audio.wav_to_fbank(wav[i:i + per], target_length=4 * rows, fn_STFT=stft)
        parts.append(pipe.vae.get_first_stage_encoding(pipe.vae.encode(mel[:, None]).mode()))
    return torch.cat(parts)


def test_edit_long_from_embeds_equals_the_manual_chain_chunked_or_not():
    import make_golden_mel as mg
    pipe, cfg = _pipe()
    duration, Ht = 3.3, 88                               # 84.48 rows round up to 88: four windows
    enc, mask = _states(cfg, "ledit7")
    noise = _noise(2, Ht, 370)
    wav = mg.test_wave(B, 40000, "ledit7")               # 2.5 s, padded to the clip; holds a NaN and samples past 1
    keep = pipe.latent_keep_mask(B, (Ht, W), time_mask_ratio_start_and_end=(0.5, 1.0))
    for chunk_rows, per in ((None, B), (Ht, 1)):
        extra = {} if chunk_rows is None else dict(_chunk_rows=chunk_rows)
        got = pipe.edit_long_from_embeds(enc, mask, noise[0], wav, duration, keep, 1.0, W_IN, 1.0, 2, step_noise=noise[1:],
                                         overlap=8, window_h=WH, **extra)
        src = _encode_chunked(pipe, wav, Ht, per)
        assert tuple(src.shape) == (B, C, Ht, W) and bool(torch.isfinite(src).all())
        lat = pipe.edit_long_latent(enc, mask, noise[0], src, keep, 1.0, W_IN, 1.0, 2, overlap=8, window_h=WH,
                                    step_noise=noise[1:])
        assert torch.equal(lat[:, :, :44], src[:, :, :44])
        _, pcm = pipe._decode_long(lat, **({} if chunk_rows is None else dict(chunk_rows=chunk_rows)))
        want = pcm.cpu().numpy()[:, :int(16000 * duration)]
        assert got.dtype == np.int16 and got.shape == (B, 52800) and np.array_equal(got, want)
    with pytest.raises(ValueError, match="noise"):
        pipe.edit_long_from_embeds(enc, mask, noise[0], wav, 3.0, keep, overlap=8, window_h=WH)
    with pytest.raises(ValueError, match="keep_mask"):
        pipe.edit_long_from_embeds(enc, mask, noise[0], wav, duration, keep[:, :, :80], overlap=8, window_h=WH)


def _prompt_pipe():
    from test_edit_gpu import _WhitespaceTokenizer
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
    sd = vae.state_dict()
    sd.update(cases.vae_encoder_weights(cases.TINY_VAE_DD))
    vae.load_state_dict(sd)
    return pipe.eval().requires_grad_(False)


def test_extend_and_edit_long_are_their_pieces_put_together():
    """`extend`: a 2 s source (50 rows) in a 3 s clip (80 rows), at the start (kept rows [0, 48)) and at the end (row 30,
    kept rows [32, 80)): the source encoded at its own extent, written into a zero latent, one plane for the batch, then
    `edit_long_latent`, `_decode_long` and the cut.  Draws from the global generator in `generate_long`'s order, or seeded.
    `edit_long`: text encoding, the ratios as a mask over the clip's rows, `edit_long_from_embeds`."""
    import make_golden_mel as mg
    pipe = _prompt_pipe()
    prompts = ["a dog barks twice near the mill", "rain"]
    wav = mg.test_wave(2, 32000 + 100, "ledit8").nan_to_num().clip(-1, 1)
    args = dict(cfg_scale_input=W_IN, num_steps=2, overlap=8, window_h=WH)
    for at, r0, k0, k1, post, seeds in ((0.0, 0, 0, 48, 2.0, None), (1.2, 30, 32, 80, 1.0, [7, 8])):
        torch.manual_seed(31)
        got = pipe.extend(prompts, wav, DURATION, source_at=at, cfg_scale_post=post, seeds=seeds, **args)
        torch.manual_seed(31)
        embeds_cf, mask_cf, embeds, mask = pipe.encode_text_classifier_free(prompts, 1)
        if seeds is None:
            noise, kw = torch.randn((2, C, 80, W), device=embeds.device, dtype=torch.float32), {}
        else:
            draws = pipe.seeded_noise(seeds, 2, (C, 80, W))
            noise, kw = draws[0], dict(step_noise=draws[1:])
        if post > 1:
            kw.update(uncond_states=embeds_cf[:2], uncond_mask=mask_cf[:2])
        # the encoder takes rows in multiples of 4: 50 rows are filled up to 52 with zero samples on the side that borders
        # generated audio, and the two rows are dropped again
        left = 2 if r0 + 50 == 80 else 0
        padded = torch.nn.functional.pad(wav[:, :50 * 640], (left * 640, (2 - left) * 640))
        part = _encode_chunked(pipe, padded, 52, 2)[:, :, left:left + 50]
        assert tuple(part.shape) == (2, C, 50, W) and bool(torch.isfinite(part).all())
        src = torch.zeros(2, C, 80, W, device=DEV)
        src[:, :, r0:r0 + 50] = part
        keep = torch.zeros(1, 1, 80, W, device=DEV)
        keep[:, :, k0:k1] = 1
        lat = pipe.edit_long_latent(embeds, mask, noise, src, keep, 1.0, W_IN, post, 2, overlap=8, window_h=WH, **kw)
        assert torch.equal(lat[:, :, k0:k1], src[:, :, k0:k1])
        want = pipe._decode_long(lat)[1].cpu().numpy()[:, :SAMPLES]
        assert got.dtype == np.int16 and got.shape == (2, SAMPLES) and np.array_equal(got, want)
    for strength, post, ratios in ((1.0, 2.0, (0.25, 0.75)), (0.5, 1.0, (1.0, 1.0))):
        torch.manual_seed(32)
        got = pipe.edit_long(prompts, wav, DURATION, time_mask_ratio_start_and_end=ratios, strength=strength,
                             cfg_scale_post=post, **args)
        torch.manual_seed(32)
        embeds_cf, mask_cf, embeds, mask = pipe.encode_text_classifier_free(prompts, 1)
        noise = torch.randn((2, C, 80, W), device=embeds.device, dtype=torch.float32)
        keep = None if strength < 1 else pipe.latent_keep_mask(2, (80, W), time_mask_ratio_start_and_end=ratios)
        kw = dict(uncond_states=embeds_cf[:2], uncond_mask=mask_cf[:2]) if post > 1 else {}
        want = pipe.edit_long_from_embeds(embeds, mask, noise, wav, DURATION, keep, strength, W_IN, post, 2, overlap=8,
                                          window_h=WH, **kw)
        assert got.dtype == np.int16 and got.shape == (2, SAMPLES) and np.array_equal(got, want)
    with pytest.raises(ValueError, match="source_wav"):
        pipe.edit_long(prompts, wav[:1], DURATION)
    with pytest.raises(ValueError, match="source_wav"):
        pipe.extend(prompts, wav[:1], DURATION)
