"""Host-side halves of long and short clips (ConsistencyTTA.long_plan, generate_long_latent and friends): the window plan
against its stated properties, the restatement's formulas and three layouts worked out by hand, every refusal raised before
anything is launched (host tensors throughout: there is no CPU path behind the checks), the export of the kernel, and the
restatement tests/long_ref.py on a dummy query."""
import pytest
import torch

import abi
import cases
import edit_ref
import long_ref
from consistencytta_amd import _native as N
from consistencytta_amd import scheduler
from consistencytta_amd.models import ConsistencyTTA, _long_latent_h

LONG_PLAN = ConsistencyTTA.long_plan                      # what the restatement restates: without it nothing here stands
PLANS = [(768, 256, 64), (80, 32, 8), (48, 32, 24), (40, 32, 24), (32, 32, 8), (64, 256, 64)]


def _pipe():
    from consistencytta_amd import modules
    vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    return ConsistencyTTA(unet_config=cases.TINY_UNET, vae=vae).eval().requires_grad_(False)


@pytest.mark.parametrize("latent_h,window_h,overlap", PLANS)
def test_long_plan_covers_the_clip_with_weights_that_sum_to_one(latent_h, window_h, overlap):
    starts, weights = ConsistencyTTA.long_plan(latent_h, window_h, overlap)
    assert weights.dtype == torch.float32 and all(isinstance(s, int) for s in starts)
    if latent_h <= window_h:                             # one window of latent_h rows
        assert starts == [0] and tuple(weights.shape) == (1, latent_h) and bool((weights == 1).all())
        return
    n = len(starts)
    assert tuple(weights.shape) == (n, window_h)
    assert starts[0] == 0 and starts[-1] == latent_h - window_h
    assert all(0 < b - a <= window_h for a, b in zip(starts, starts[1:]))          # strictly increasing, no gap
    assert n == -(-(latent_h - window_h) // (window_h - overlap)) + 1
    total = torch.zeros(latent_h, dtype=torch.float64)
    cover = torch.zeros(latent_h, dtype=torch.int64)
    for k, s in enumerate(starts):
        total[s:s + window_h] += weights[k].double()
        cover[s:s + window_h] += 1
    assert int(cover.min()) >= 1
    assert float((total - 1).abs().max()) <= 3 * 2.0 ** -24
    assert bool((weights > 0).all()) and bool((weights <= 1).all())
    for k, s in enumerate(starts):                       # rows under one window weigh exactly 1
        alone = cover[s:s + window_h] == 1
        assert bool((weights[k][alone] == 1.0).all())
    ref_starts, ref_weights = long_ref.plan(latent_h, window_h, overlap)           # the restatement agrees
    assert starts == ref_starts and torch.equal(weights, ref_weights)
    if (latent_h, window_h, overlap) == (768, 256, 64):  # span 512, step 192: 4 windows; 512 k / 3 rounded half up
        assert starts == [0, 171, 341, 512]
    if (latent_h, window_h, overlap) == (48, 32, 24):    # span 16, step 8: 3 windows; rows 16-31 lie under all three
        assert starts == [0, 8, 16]
        assert bool((cover[16:32] == 3).all()) and int(cover.max()) == 3
    if (latent_h, window_h, overlap) == (80, 32, 8):     # span 48, step 24: 3 windows 24 apart, 8 rows shared
        assert starts == [0, 24, 48]
        assert float(weights[0][24]) == pytest.approx(8 / 9) and float(weights[1][0]) == pytest.approx(1 / 9)


@pytest.mark.parametrize("args", [(100, 32, 8), (80, 36, 8), (80, 32, 32), (80, 32, -1), (1032, 256, 64), (0, 32, 8),
                                  (1024, 32, 0), (512, 32, 8)])
def test_long_plan_refuses_what_the_kernel_and_the_decoder_cannot_take(args):
    """Rows that are no multiples of 8, an overlap outside [0, window_h), more than 1024 rows, more than 16 windows."""
    with pytest.raises(ValueError):
        ConsistencyTTA.long_plan(*args)


def test_duration_maps_to_latent_rows_and_is_bounded():
    assert _long_latent_h(2.5) == 64 and _long_latent_h(10.0) == 256 and _long_latent_h(10.24) == 264
    assert _long_latent_h(30.72) == 792 and _long_latent_h(40.0) == 1024 and _long_latent_h(7.3) == 192
    for bad in (2.4, 0.0, -1.0, 40.5, float("nan")):
        with pytest.raises(ValueError, match="duration"):
            _long_latent_h(bad)


def test_long_entries_refuse_bad_arguments_before_any_launch():
    """Host tensors throughout: anything past the checks meets the missing CPU path (CttaError)."""
    pipe = _pipe()
    B, H, W, Ht = 2, 32, 16, 80
    _, _, _, enc, mask = cases.unet_inputs(cases.TINY_UNET, B, H, W, 5, "long_cpu")
    noise = torch.zeros(B, 8, Ht, W)

    def call(**kw):
        args = dict(noise=noise, num_steps=2, overlap=8, window_h=32, step_noise=None, encoder_states=enc, encoder_mask=mask)
        args.update(kw)
        return pipe.generate_long_latent(args.pop("encoder_states"), args.pop("encoder_mask"), args.pop("noise"), 4.0, **args)

    with pytest.raises(N.CttaError):                     # everything in order: the checks pass
        call()
    with pytest.raises(N.CttaError):
        call(step_noise=torch.zeros(1, B, 8, Ht, W))
    for n in (0, 2):
        with pytest.raises(ValueError, match="step_noise"):
            call(step_noise=torch.zeros(n, B, 8, Ht, W))
    with pytest.raises(ValueError, match="step_noise"):
        call(step_noise=torch.zeros(1, B, 8, H, W))      # window-sized draws where long ones are due
    with pytest.raises(ValueError, match="noise"):
        call(noise=torch.zeros(8, Ht, W))
    with pytest.raises(ValueError, match="multiples of 8"):
        call(noise=torch.zeros(B, 8, 84, W))
    with pytest.raises(ValueError, match="multiples of 8"):
        call(window_h=36)
    with pytest.raises(ValueError, match="overlap"):
        call(overlap=32)
    with pytest.raises(ValueError, match="overlap"):
        call(overlap=-8)
    with pytest.raises(ValueError, match="at most 1024"):
        call(noise=torch.zeros(1, 8, 1032, W))
    with pytest.raises(ValueError, match="windows"):
        call(noise=torch.zeros(1, 8, 512, W), overlap=8)
    with pytest.raises(ValueError, match="num_steps"):
        call(num_steps=0, step_noise=None)
    with pytest.raises(ValueError, match="encoder_states"):
        call(encoder_states=torch.cat([enc, enc[:1]]))   # 3 rows: neither B nor B * n
    with pytest.raises(N.CttaError):                     # B * n rows: every window its own
        call(encoder_states=enc.repeat_interleave(3, 0), encoder_mask=mask.repeat_interleave(3, 0))
    with pytest.raises(ValueError, match="uncond_states"):
        call(cfg_scale_post=2.0)
    for bad in (2.4, 41.0):
        with pytest.raises(ValueError, match="duration"):
            pipe.generate_long_from_embeds(enc, mask, noise, bad)
        with pytest.raises(ValueError, match="duration"):
            pipe.generate_long(["rain"], bad)
        with pytest.raises(ValueError, match="duration"):
            pipe.capture_long_graph(B, 5, bad)
    with pytest.raises(ValueError, match="noise"):       # 3.0 s is 80 rows; 3.5 s is 96
        pipe.generate_long_from_embeds(enc, mask, noise, 3.5, window_h=32, overlap=8)
    with pytest.raises(N.CttaError):
        pipe.generate_long_from_embeds(enc, mask, noise, 3.0, 4.0, num_steps=1, window_h=32, overlap=8)


def test_window_fuse_kernel_is_declared_exported_and_bound():
    assert "ctta_window_fuse_renoise" in abi.declared_symbols()
    abi.assert_bound(("ctta_window_fuse_renoise",))


# ------------------------------------------------------------------------------------- the restatement on a dummy query
def _dummy(Ht):
    g = torch.Generator().manual_seed(6)
    noise = torch.randn(2, 8, Ht, 16, generator=g)
    steps = torch.randn(3, 2, 8, Ht, 16, generator=g)
    sch = scheduler.HeunDiscreteScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    return noise, steps, sch


def test_restated_cut_and_fuse_are_inverse_on_one_latent():
    """Windows cut from ONE long tensor fuse back to it up to the rounding of the weights (they sum to 1 per row), and
    exactly where one window covers a row."""
    noise, _, _ = _dummy(80)
    starts, weights = long_ref.plan(80, 32, 8)
    assert (starts, weights.tolist()) == (LONG_PLAN(80, 32, 8)[0], LONG_PLAN(80, 32, 8)[1].tolist())
    wins = long_ref.cut(noise, starts, 32)
    assert tuple(wins.shape) == (6, 8, 32, 16) and torch.equal(wins[4], noise[1, :, 24:56])      # row b * n + k
    back = long_ref.fuse(wins, starts, weights, 80)
    assert torch.equal(back[:, :, :24], noise[:, :, :24]) and torch.equal(back[:, :, 32:48], noise[:, :, 32:48])
    assert float((back - noise).abs().max()) <= 8 * 2.0 ** -24 * float(noise.abs().max())


@pytest.mark.parametrize("num_steps", [1, 4])
def test_restatement_with_one_window_is_the_plain_sampler(num_steps):
    noise, steps, sch = _dummy(32)
    query = lambda z, t: 0.3 * z + 0.001 * t - 0.2                                          # noqa: E731
    times, sigmas = edit_ref.schedule(sch, num_steps)
    plain = edit_ref.plain_sampler(query, times, sigmas, noise, steps[:num_steps - 1])
    for window_h in (32, 64):                            # latent_h == window_h, latent_h < window_h
        out = long_ref.long_sampler(query, times, sigmas, noise, window_h, 8, steps[:num_steps - 1])
        assert torch.equal(out, plain)


def test_restatement_with_a_pointwise_query_does_not_see_the_windows():
    """A query that treats every element alike gives every window the same estimate of a shared row, so the fusion is the
    plain sampler up to the rounding of the weights; a query that depends on the row within the window does not."""
    noise, steps, sch = _dummy(80)
    times, sigmas = edit_ref.schedule(sch, 2)
    point = lambda z, t: 0.3 * z - 0.2                                                      # noqa: E731
    plain = edit_ref.plain_sampler(point, times, sigmas, noise, steps[:1])
    out = long_ref.long_sampler(point, times, sigmas, noise, 32, 8, steps[:1])
    assert float((out - plain).abs().max()) <= 1e-5 * float(plain.abs().max())
    ramp = torch.arange(32.0).view(1, 1, 32, 1)
    rowwise = lambda z, t: 0.3 * z + 0.01 * ramp                                            # noqa: E731
    times, sigmas = edit_ref.schedule(sch, 1)            # one query: the windows' estimates, cross-faded
    out = long_ref.long_sampler(rowwise, times, sigmas, noise, 32, 8)
    flat = edit_ref.plain_sampler(lambda z, t: 0.3 * z, times, sigmas, noise)
    seam = (out - flat)[0, 0, :, 0]
    assert float(seam[23]) == pytest.approx(0.23, abs=1e-4) and float(seam[32]) == pytest.approx(0.08, abs=1e-4)
    assert 0.08 < float(seam[27]) < 0.28                 # rows 24-31: a cross-fade between 0.24 .. 0.31 and 0.00 .. 0.07
