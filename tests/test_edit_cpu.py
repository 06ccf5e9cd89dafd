"""Host-side halves of audio editing (ConsistencyTTA.edit_latent and friends): the keep mask against the reference's three
lines, every refusal of the sampler on host tensors (raised before anything is launched: there is no CPU path behind them),
the export of the two kernels, and the restatement tests/edit_ref.py on a linear dummy query."""
import pytest
import torch

import abi
import cases
import edit_ref
from consistencytta_amd import _native as N
from consistencytta_amd import scheduler

B, H, W = 2, 32, 16


def _pipe():
    from consistencytta_amd import modules
    from consistencytta_amd.models import ConsistencyTTA
    vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    return ConsistencyTTA(unet_config=cases.TINY_UNET, vae=vae).eval().requires_grad_(False)


def _reference_mask(batch, h, w, time_ratios, freq_ratios):
    """audioldm/ldm.py:764-768, restated."""
    mask = torch.ones(batch, h, w)
    mask[:, int(h * time_ratios[0]):int(h * time_ratios[1]), :] = 0
    mask[:, :, int(w * freq_ratios[0]):int(w * freq_ratios[1])] = 0
    return mask[:, None, ...]


@pytest.mark.parametrize("time_ratios,freq_ratios", [((0.10, 0.15), (1.0, 1.0)), ((0.25, 0.75), (1.0, 1.0)),
                                                     ((1.0, 1.0), (0.75, 1.0)), ((0.25, 0.75), (0.75, 1.0)),
                                                     ((1.0, 1.0), (1.0, 1.0))])
def test_keep_mask_follows_the_reference_lines(time_ratios, freq_ratios):
    from consistencytta_amd.models import ConsistencyTTA
    got = ConsistencyTTA.latent_keep_mask(B, (H, W), time_mask_ratio_start_and_end=time_ratios,
                                          freq_mask_ratio_start_and_end=freq_ratios)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, 1, H, W)
    assert torch.equal(got, _reference_mask(B, H, W, time_ratios, freq_ratios))
    if time_ratios == (0.10, 0.15):                      # int(3.2) .. int(4.8): row 3 alone
        assert torch.equal(got[0, 0, :, 0] == 0, torch.arange(H) == 3)
    if time_ratios == freq_ratios == (1.0, 1.0):
        assert bool((got == 1).all())
    if freq_ratios == (0.75, 1.0) and time_ratios == (0.25, 0.75):
        assert float(got.sum()) == B * 16 * 12


def test_keep_mask_defaults_and_explicit_rows():
    from consistencytta_amd.models import ConsistencyTTA
    assert bool((ConsistencyTTA.latent_keep_mask(1, (H, W)) == 1).all())
    rows = torch.zeros(H)
    rows[:5] = 0.25
    got = ConsistencyTTA.latent_keep_mask(B, (H, W), time_keep=rows, freq_mask_ratio_start_and_end=(0.0, 0.5))
    want = rows.view(1, 1, H, 1).expand(B, 1, H, W).clone()
    want[..., :8] = 0
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        ConsistencyTTA.latent_keep_mask(B, (H, W), freq_keep=torch.ones(H))


@pytest.mark.parametrize("ratios", [(-0.1, 0.5), (0.5, 1.2), (0.6, 0.4)])
def test_keep_mask_refuses_ratios_outside_the_unit_interval_or_out_of_order(ratios):
    from consistencytta_amd.models import ConsistencyTTA
    with pytest.raises(ValueError):
        ConsistencyTTA.latent_keep_mask(B, (H, W), time_mask_ratio_start_and_end=ratios)
    with pytest.raises(ValueError):
        ConsistencyTTA.latent_keep_mask(B, (H, W), freq_mask_ratio_start_and_end=ratios)


def test_edit_latent_refuses_bad_arguments_before_any_launch():
    """Host tensors throughout: anything past the checks would raise something else (there is no CPU path)."""
    pipe = _pipe()
    x, _, _, enc, mask = cases.unet_inputs(cases.TINY_UNET, B, H, W, 5, "edit_cpu")
    src = torch.zeros_like(x)

    def call(**kw):
        args = dict(noise=x, src_latent=src, keep_mask=None, strength=1.0, num_steps=4, step_noise=None)
        args.update(kw)
        return pipe.edit_latent(enc, mask, args.pop("noise"), args.pop("src_latent"), cfg_scale_input=4.0, **args)

    draws = lambda n: torch.zeros((n,) + tuple(x.shape))                                    # noqa: E731
    # num_steps = 4: strength 1.0, 0.5, 0.3 -> r = 4, 2, 1 -> 3, 1, 0 re-noising draws
    for strength, want in ((1.0, 3), (0.5, 1), (0.3, 0)):
        for n in {0, 1, 2, 3, 4} - {want}:
            with pytest.raises(ValueError, match="step_noise"):
                call(strength=strength, step_noise=draws(n))
        with pytest.raises(N.CttaError):                 # the right count passes the checks and meets the missing CPU path
            call(strength=strength, step_noise=draws(want))
    with pytest.raises(ValueError, match="step_noise"):
        call(step_noise=torch.zeros_like(x))
    for bad in (torch.zeros(B, 8, H, W + 4), torch.zeros(B + 1, 8, H, W), torch.zeros(8, H, W)):
        with pytest.raises(ValueError, match="src_latent"):
            call(src_latent=bad)
    for bad in (torch.ones(B, H, W), torch.ones(B, 8, H, W), torch.ones(B + 1, 1, H, W), torch.ones(1, 1, W, H)):
        with pytest.raises(ValueError, match="keep_mask"):
            call(keep_mask=bad)
    for strength in (0.0, 1.5, -0.5):
        with pytest.raises(ValueError, match="strength"):
            call(strength=strength)
    for good in (torch.ones(B, 1, H, W), torch.ones(1, 1, H, W)):
        with pytest.raises(N.CttaError):
            call(keep_mask=good)
    with pytest.raises(ValueError, match="step_noise"):
        pipe.edit_from_embeds(enc, mask, x, torch.zeros(B, 20320), strength=0.5, num_steps=4, step_noise=draws(3))


def test_edit_kernels_are_exported_and_bound():
    abi.assert_bound(("ctta_consistency_edit_renoise", "ctta_cfg_combine_keep"))


# ------------------------------------------------------------------------------------- the restatement on a dummy query
def _dummy():
    g = torch.Generator().manual_seed(5)
    noise, src = torch.randn(B, 8, H, W, generator=g), torch.randn(B, 8, H, W, generator=g)
    steps = torch.randn(3, B, 8, H, W, generator=g)
    query = lambda z, t: 0.3 * z + 0.001 * t - 0.2                                          # noqa: E731
    sch = scheduler.HeunDiscreteScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    return noise, src, steps, query, sch


def test_restated_schedule_is_the_samplers():
    sch = _dummy()[4]
    times, sigmas = edit_ref.schedule(sch, 4)
    assert times[0] == 999.0 and times == sorted(times, reverse=True) and len(set(times)) == 4
    assert abs(float(sigmas[0]) - cases.SIGMA_MAX) < 1e-3 and list(sigmas) == sorted(sigmas, reverse=True)
    assert edit_ref.schedule(sch, 1) == ([999.0], [sigmas[0]])


@pytest.mark.parametrize("strength", [1.0, 0.5])
def test_restatement_with_everything_kept_returns_the_source(strength):
    noise, src, steps, query, sch = _dummy()
    times, sigmas = edit_ref.schedule(sch, 4)
    r = max(1, int(strength * 4))
    out = edit_ref.edit_sampler(query, times, sigmas, noise, src, torch.ones(1, 1, H, W), strength, steps[:r - 1])
    assert torch.equal(out, src)


@pytest.mark.parametrize("num_steps", [1, 4])
def test_restatement_with_nothing_kept_is_the_plain_sampler(num_steps):
    noise, src, steps, query, sch = _dummy()
    times, sigmas = edit_ref.schedule(sch, num_steps)
    plain = edit_ref.plain_sampler(query, times, sigmas, noise, steps[:num_steps - 1])
    for keep in (torch.zeros(B, 1, H, W), None):
        out = edit_ref.edit_sampler(query, times, sigmas, noise, src, keep, 1.0, steps[:num_steps - 1])
        assert torch.equal(out, plain)
    half = torch.ones(1, 1, H, W)
    half[:, :, H // 2:] = 0
    out = edit_ref.edit_sampler(query, times, sigmas, noise, src, half, 1.0, steps[:num_steps - 1])
    assert torch.equal(out[:, :, :H // 2], src[:, :, :H // 2]) and not torch.equal(out[:, :, H // 2:], src[:, :, H // 2:])
    if num_steps > 1:           # strength < 1 starts from the source: another result
        vary = edit_ref.edit_sampler(query, times, sigmas, noise, src, None, 0.5, steps[:1])
        assert not torch.equal(vary, plain)
