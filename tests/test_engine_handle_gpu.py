"""The engine handles' shared lifecycle on the GPU (tiny configs of tests/golden/cases.py only): the tap accessors'
host-side argument checks, capacity reuse through the module mirrors -- the handle address a captured graph would hold
stays put when a smaller call follows a larger one -- and a create that fails its validation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cases  # noqa: E402
from consistencytta_amd import _native as N, modules, text_encoder  # noqa: E402
from gpu_util import DEV, rel_err, rel_l2  # noqa: E402
from oracle import nets as onets  # noqa: E402

REL_L2, REL_MAX = 2.5e-2, 6e-2      # the engines' parity contract (test_engines_gpu.py)


def _load(module, sd):
    module.load_state_dict(dict(sd))
    return module.to(DEV).eval().requires_grad_(False)


def _unet(taps=False):
    m = modules.UNet2DConditionGuidedModel.from_config(cases.TINY_UNET)
    m.debug_taps = taps
    return _load(m, cases.unet_weights(cases.TINY_UNET, True))


def _vae(taps=False, z_channels=None):
    dd = cases.TINY_VAE_DD if z_channels is None else dict(cases.TINY_VAE_DD, z_channels=z_channels)
    sd = dict(cases.vae_weights(dd))
    sd.update(cases.vae_encoder_weights(dd))
    sd.update(cases.hifigan_weights(cases.TINY_HIFIGAN))
    v = modules.AutoencoderKL(ddconfig=dd, embed_dim=8, scale_factor=1.0, hifigan_config=cases.TINY_HIFIGAN)
    v.debug_taps = taps
    return _load(v, sd), sd


def _unet_call(m, B, tag="handle_unet"):
    x, ts, gs, enc, mask = cases.unet_inputs(cases.TINY_UNET, 2, 16, 8, 9, tag)
    return m(x[:B].to(DEV), ts[:B].to(DEV), guidance=gs[:B].to(DEV), encoder_hidden_states=enc[:B].to(DEV),
             encoder_attention_mask=mask[:B].to(DEV)).sample


# prefix of the C accessors, the call that runs one tiny forward at batch B, where the mirror keeps the handle it used
def _tap_cases():
    z = cases.vae_inputs(2, 16, 8, "handle_vae").to(DEV)
    mel_dec = cases.mel_inputs(2, 24, 64, "handle_voc").to(DEV)
    mel_enc = (cases.mel_inputs(2, 64, 16, "handle_enc") * 2.0 - 4.0).to(DEV)
    return {
        "unet": ("ctta_unet", lambda m, B: _unet_call(m, B), lambda m: m._h_unet),
        "vae": ("ctta_vae", lambda v, B: v.decode_first_stage(z[:B]), lambda v: v._h_vae),
        "vae_encoder": ("ctta_vae_encoder", lambda v, B: v.encode_first_stage(mel_enc[:B]).parameters, lambda v: v._enc.h),
        "hifigan": ("ctta_hifigan", lambda v, B: v.vocode(mel_dec[:B]), lambda v: v._h_voc),
    }


@pytest.mark.parametrize("which", ["unet", "vae", "vae_encoder", "hifigan"])
def test_tap_accessors_check_their_index_and_read_every_tap(which):
    """Host-side argument checks that return a status: no out-of-range pointer ever reaches a kernel."""
    prefix, call, handle = _tap_cases()[which]
    m = _unet(taps=True) if which == "unet" else _vae(taps=True)[0]
    call(m, 1)
    L, h = N.lib(), handle(m)
    num = getattr(L, prefix + "_num_taps")(h)
    assert num > 0
    info = getattr(L, prefix + "_tap_info")
    for bad in (-1, num):
        name, dims = N.c_char_p(), (N.c_int * 4)()
        assert info(h, bad, name, dims) != 0
        assert L.ctta_last_error() == b"tap index out of range"
    taps = N.read_taps(prefix, h, DEV)
    assert len(taps) == num
    for i, (tname, t) in enumerate(taps.items()):
        name, dims = N.c_char_p(), (N.c_int * 4)()
        N.check(info(h, i, name, dims))
        assert name.value.decode() == tname and tuple(t.shape) == tuple(dims) and dims[0] == 1
        assert bool(torch.isfinite(t).all()), tname


def _t5_case():
    m = text_encoder.T5EncoderModel(cases.TINY_T5)
    m.load_state_dict(cases.t5_weights(cases.TINY_T5))
    m.to(DEV).eval()
    ids, _ = cases.t5_inputs(cases.TINY_T5, 2, 13, "handle_t5")
    ids = ids.to(DEV)
    return m, lambda m, B: m(input_ids=ids[:B], attention_mask=torch.ones_like(ids[:B])).last_hidden_state, lambda m: m._engine.h


@pytest.mark.parametrize("which", ["unet", "vae", "vae_encoder", "hifigan", "t5"])
def test_smaller_call_reuses_the_handle_and_matches_its_row_of_the_larger_one(which):
    """B=2 then B=1 through the mirror: the native handle is the same object (the address a captured graph holds), and
    the B=1 result equals row 0 of the B=2 call bit for bit, the property and the tolerance of
    test_unet_batch_independence_and_determinism."""
    if which == "t5":
        m, call, handle = _t5_case()
    else:
        _, call, handle = _tap_cases()[which]
        m = _unet() if which == "unet" else _vae()[0]
    two = call(m, 2).clone()
    h2 = handle(m)
    addr = h2.value
    one = call(m, 1)
    assert handle(m) is h2 and h2.value == addr and addr
    diff = float((one[0] - two[0]).abs().max())
    print("%s: max |B=1 - row 0 of B=2| = %.3e (rel L2 %.3e)" % (which, diff, rel_l2(one[:1], two[:1])))
    assert torch.equal(one[0], two[0])


def test_vae_create_that_fails_validation_leaves_the_stream_usable():
    """enable_grad needs z_channels % 8 == 0: the create returns its error (and holds no handle); a valid create on the
    same stream then succeeds and decodes correctly."""
    bad, _ = _vae(z_channels=4)
    z_bad = torch.zeros(1, 8, 16, 8, device=DEV, requires_grad=True)
    with pytest.raises(N.CttaError, match="vae_create: enable_grad needs z_channels % 8 == 0"):
        bad.decode_first_stage(z_bad, allow_grad=True)
    assert bad._eng["vae"][1].h is None
    v, sd = _vae()
    z = cases.vae_inputs(2, 16, 8, "handle_vae")
    mel = v.decode_first_stage(z.to(DEV))
    with torch.no_grad():
        ref = onets.vae_decode(cases.TINY_VAE_DD, sd, z, v.scale_factor)
    l2, mx = rel_l2(mel, ref), rel_err(mel, ref)
    print("decode after the failed create: rel_l2 %.3e rel_max %.3e" % (l2, mx))
    assert np.isfinite(l2) and l2 <= REL_L2 and mx <= REL_MAX
