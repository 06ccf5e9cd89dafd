"""Host-side halves of long-clip editing (ConsistencyTTA.edit_long_latent, extend and friends): the export of the kernel, the
refusals of its C entry (they come before any launch, so they hold without a GPU and on pointers that are never read), the
input rules at long shapes, the row arithmetic of `extend` worked out by hand, and the restatement tests/long_edit_ref.py on a
dummy query against the two restatements it joins."""
import pytest
import torch

import abi
import cases
import edit_ref
import long_edit_ref
import long_ref
from consistencytta_amd import _native as N
from consistencytta_amd import scheduler
from consistencytta_amd.models import ConsistencyTTA, _check_edit_inputs, _extend_rows

INVALID = 1
SOME = N.c_void_p(4096)                                   # a device pointer's stand-in: refused calls never read it


def _pipe():
    from consistencytta_amd import modules
    vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    return ConsistencyTTA(unet_config=cases.TINY_UNET, vae=vae).eval().requires_grad_(False)


def test_window_fuse_edit_kernel_is_declared_exported_and_bound():
    assert "ctta_window_fuse_edit_renoise" in abi.declared_symbols()
    abi.assert_bound(("ctta_window_fuse_edit_renoise",))


def test_c_entry_refuses_null_and_invalid_arguments_on_the_host():
    """Every call here is refused: none reaches a launch."""
    def call(cond=SOME, unc=None, ww=None, st=(0, 24, 48), weights=SOME, src=SOME, keep=SOME, noise=SOME, sigma=SOME,
             x0_long=SOME, out=SOME, copies=1, n_=None, Ht=80, width=8):
        host = (N.c_int32 * max(1, len(st)))(*st) if st is not None else None
        return N.lib().ctta_window_fuse_edit_renoise(cond, unc, ww, host, weights, src, keep, noise, sigma, x0_long, out,
                                                     copies, 2, len(st) if n_ is None and st is not None else (n_ or 0), 2, 32,
                                                     Ht, width, None)

    refusals = [
        (dict(src=None), "src_long and keep"),
        (dict(keep=None), "src_long and keep"),
        (dict(src=None, keep=None), "src_long and keep"),
        (dict(st=None, n_=3), "starts and weights"),
        (dict(weights=None), "starts and weights"),
        (dict(st=(8, 24, 48)), r"starts\[0\]"),
        (dict(st=(0, 24, 40)), "last start"),
        (dict(Ht=88), "last start"),
        (dict(st=(0, 24, 24, 48)), "strictly increasing"),
        (dict(st=(0, 8, 48)), "gap"),
        (dict(st=tuple(range(0, 51, 3))), "n_windows"),
        (dict(n_=0), "n_windows"),
        (dict(width=6), "width"),
        (dict(copies=0), "copies"),
        (dict(copies=3), "copies"),
        (dict(unc=SOME), "uncond and w_post"),
        (dict(ww=SOME), "uncond and w_post"),
        (dict(cond=None, unc=SOME, ww=SOME), "uncond without cond"),
        (dict(noise=None), "noise and out"),
        (dict(out=None), "noise and out"),
        (dict(noise=None, out=None, x0_long=None), "x0_long"),
        (dict(sigma=None), "sigma"),
    ]
    for kw, what in refusals:
        assert call(**kw) == INVALID, kw
        with pytest.raises(N.CttaError, match="window_fuse_edit_renoise: .*" + what):
            N.check(call(**kw))


def test_edit_input_rules_hold_at_long_shapes():
    B, C, Ht, W = 2, 8, 80, 16
    noise, src = torch.zeros(B, C, Ht, W), torch.zeros(B, C, Ht, W)
    assert _check_edit_inputs(noise, src, None, 1.0, 4) == 4
    assert _check_edit_inputs(noise, src, torch.ones(1, 1, Ht, W), 0.5, 4) == 2
    assert _check_edit_inputs(torch.zeros(2, B, C, Ht, W), src, torch.ones(B, 1, Ht, W), 0.5, 4) == 2
    assert _check_edit_inputs(noise, src, None, 0.1, 4) == 1
    for bad in (torch.zeros(B, C, 32, W), torch.zeros(B, C, Ht, 8), None):
        with pytest.raises(ValueError, match="src_latent"):
            _check_edit_inputs(noise, bad, None, 1.0, 4)
    for bad in (torch.ones(B, 1, 32, W), torch.ones(B, Ht, W), torch.ones(3, 1, Ht, W), torch.ones(B, C, Ht, W)):
        with pytest.raises(ValueError, match="keep_mask"):
            _check_edit_inputs(noise, src, bad, 1.0, 4)
    for bad in (0.0, 1.5, -0.5):
        with pytest.raises(ValueError, match="strength"):
            _check_edit_inputs(noise, src, None, bad, 4)
    with pytest.raises(ValueError, match="num_steps"):
        _check_edit_inputs(noise, src, None, 1.0, 0)


def test_long_edit_entries_refuse_bad_arguments_before_any_launch():
    """Host tensors throughout: anything past the checks meets the missing CPU path (CttaError)."""
    pipe = _pipe()
    B, W, Ht = 2, 16, 80
    _, _, _, enc, mask = cases.unet_inputs(cases.TINY_UNET, B, 32, W, 5, "long_edit_cpu")
    noise, src = torch.zeros(B, 8, Ht, W), torch.zeros(B, 8, Ht, W)

    def call(**kw):
        args = dict(noise=noise, src_latent=src, keep_mask=None, strength=1.0, num_steps=2, overlap=8, window_h=32,
                    step_noise=None, encoder_states=enc, encoder_mask=mask)
        args.update(kw)
        return pipe.edit_long_latent(args.pop("encoder_states"), args.pop("encoder_mask"), args.pop("noise"),
                                     args.pop("src_latent"), args.pop("keep_mask"), args.pop("strength"), 4.0, **args)

    with pytest.raises(N.CttaError):                     # everything in order: the checks pass
        call()
    with pytest.raises(N.CttaError):
        call(keep_mask=torch.ones(1, 1, Ht, W), strength=0.5, num_steps=4, step_noise=torch.zeros(1, B, 8, Ht, W))
    with pytest.raises(ValueError, match="step_noise"):
        call(strength=0.5, num_steps=4, step_noise=torch.zeros(3, B, 8, Ht, W))            # r = 2: one draw is due
    with pytest.raises(ValueError, match="noise"):
        call(noise=torch.zeros(8, Ht, W))
    with pytest.raises(ValueError, match="src_latent"):
        call(src_latent=torch.zeros(B, 8, 32, W))
    with pytest.raises(ValueError, match="keep_mask"):
        call(keep_mask=torch.ones(B, 1, 32, W))
    with pytest.raises(ValueError, match="strength"):
        call(strength=0.0)
    with pytest.raises(ValueError, match="multiples of 8"):
        call(window_h=36)
    with pytest.raises(ValueError, match="overlap"):
        call(overlap=32)
    with pytest.raises(ValueError, match="windows"):
        call(noise=torch.zeros(1, 8, 512, W), src_latent=torch.zeros(1, 8, 512, W), overlap=8)
    with pytest.raises(ValueError, match="encoder_states"):
        call(encoder_states=torch.cat([enc, enc[:1]]))
    with pytest.raises(N.CttaError):                     # B * n rows: every window its own
        call(encoder_states=enc.repeat_interleave(3, 0), encoder_mask=mask.repeat_interleave(3, 0))
    with pytest.raises(ValueError, match="uncond_states"):
        call(cfg_scale_post=2.0)
    wav = torch.zeros(B, 32000)
    for bad in (2.4, 41.0):
        with pytest.raises(ValueError, match="duration"):
            pipe.edit_long_from_embeds(enc, mask, noise, wav, bad)
        with pytest.raises(ValueError, match="duration"):
            pipe.edit_long(["rain"], wav[:1], bad)
        with pytest.raises(ValueError, match="duration"):
            pipe.extend(["rain"], wav[:1], bad)
        with pytest.raises(ValueError, match="duration"):
            pipe.capture_long_edit_graph(B, 5, bad)
    with pytest.raises(ValueError, match="noise"):       # 3.0 s is 80 rows; 3.5 s is 96
        pipe.edit_long_from_embeds(enc, mask, noise, wav, 3.5, window_h=32, overlap=8)
    with pytest.raises(ValueError, match="source_wav"):
        pipe.edit_long_from_embeds(enc, mask, noise, wav[:1], 3.0, window_h=32, overlap=8)
    with pytest.raises(ValueError, match="strength"):
        pipe.capture_long_edit_graph(B, 5, 3.0, strength=0.0)


def test_extend_row_arithmetic():
    """A row is 640 samples (4 mel frames of 160): 25 rows per second of source, whatever the clip's 25.6."""
    assert _extend_rows(32000, 80, 0.0, 2) == (50, 0, 0, 48)          # 2 s at 0 in a 3 s clip: the right side borders
    assert _extend_rows(32000, 80, 1.2, 2) == (50, 30, 32, 80)        # ends with the clip: only the left side borders
    assert _extend_rows(32000, 80, 0.4, 2) == (50, 10, 12, 58)        # both sides
    assert _extend_rows(32000 + 639, 80, 0.0, 0) == (50, 0, 0, 50)    # a part row is dropped; no junction rows
    assert _extend_rows(51200, 80, 0.0, 2) == (80, 0, 0, 80)          # the whole clip: nothing borders
    assert _extend_rows(5120, 80, 0.0, 5) == (8, 0, 0, 3)
    assert _extend_rows(5120, 80, 1.0, 5)[2:] == (30, 30)             # junctions wider than the source: nothing kept
    with pytest.raises(ValueError, match="at least 8"):
        _extend_rows(5119, 80, 0.0, 2)                   # 7 rows
    with pytest.raises(ValueError, match="before the clip"):
        _extend_rows(32000, 80, -0.1, 2)
    with pytest.raises(ValueError, match="do not fit"):
        _extend_rows(32000, 80, 1.24, 2)                 # row 31: rows [31, 81)
    with pytest.raises(ValueError, match="junction_rows"):
        _extend_rows(32000, 80, 0.0, -1)
    pipe = _pipe()
    for at, T in ((-0.1, 32000), (1.24, 32000), (0.0, 5119)):          # raised before the text encoder is asked for
        with pytest.raises(ValueError):
            pipe.extend(["rain"], torch.zeros(1, T), 3.0, source_at=at)


# ------------------------------------------------------------------------------------- the restatement on a dummy query
def _dummy(Ht):
    g = torch.Generator().manual_seed(16)
    noise = torch.randn(2, 8, Ht, 16, generator=g)
    steps = torch.randn(3, 2, 8, Ht, 16, generator=g)
    src = torch.randn(2, 8, Ht, 16, generator=g) * 0.8
    sch = scheduler.HeunDiscreteScheduler.from_pretrained("stabilityai/stable-diffusion-2-1", subfolder="scheduler")
    return noise, steps, src, sch


def _query(z, t):
    return 0.3 * z + 0.001 * t - 0.2


@pytest.mark.parametrize("num_steps", [1, 2, 4])
def test_restatement_that_keeps_nothing_is_the_long_sampler(num_steps):
    noise, steps, src, sch = _dummy(80)
    times, sigmas = edit_ref.schedule(sch, num_steps)
    want = long_ref.long_sampler(_query, times, sigmas, noise, 32, 8, steps[:num_steps - 1])
    for keep in (None, torch.zeros(1, 1, 80, 16)):
        got = long_edit_ref.long_edit_sampler(_query, times, sigmas, noise, src, keep, 32, 8, 1.0, steps[:num_steps - 1])
        assert torch.equal(got, want)                    # values: the blend turns a -0 into +0
    keep = torch.zeros(2, 1, 80, 16)
    keep[:, :, :40] = 1
    got = long_edit_ref.long_edit_sampler(_query, times, sigmas, noise, src, keep, 32, 8, 1.0, steps[:num_steps - 1])
    assert torch.equal(got[:, :, :40], src[:, :, :40])   # kept rows come back exactly
    assert torch.equal(got[:, :, 40:], want[:, :, 40:])  # and a pointwise query does not carry them into the others


@pytest.mark.parametrize("strength", [1.0, 0.5, 0.25])
def test_restatement_with_one_window_is_the_edit_sampler(strength):
    noise, steps, src, sch = _dummy(32)
    times, sigmas = edit_ref.schedule(sch, 4)
    r = max(1, int(strength * 4))
    keep = torch.ones(2, 1, 32, 16)
    keep[:, :, 16:] = 0
    keep[1, :, :4] = 0.25
    for k in (keep, None):
        want = edit_ref.edit_sampler(_query, times, sigmas, noise, src, k, strength, steps[:r - 1])
        for window_h in (32, 64):                        # latent_h == window_h, latent_h < window_h
            got = long_edit_ref.long_edit_sampler(_query, times, sigmas, noise, src, k, window_h, 8, strength, steps[:r - 1])
            assert torch.equal(got, want)
