"""Host side of the fused LoRA site kernels, the per-call adapter strength and the adapter-only reload: the exported
symbols, the pure host functions (`ctta_lora_sites_supported`, `ctta_lora_sites_bwd_scratch_floats`), the split of a
module's weight version into a base and an adapter part, and `cross_attention_kwargs`."""
import pytest
import torch

import abi
import lora_cases as LC
from consistencytta_amd import _native as N
from consistencytta_amd import modules, spec

NEW = ("ctta_lora_sites_supported", "ctta_lora_sites_fwd", "ctta_lora_sites_bwd", "ctta_lora_sites_bwd_scratch_floats",
       "ctta_unet_set_lora", "ctta_unet_load_adapters")
FULL = dict(spec.LIGHT_UNET_CONFIG, block_out_channels=[320, 640, 1280, 1280], attention_head_dim=[5, 10, 20, 20])


def _up64(v):
    return (v + 63) // 64 * 64


def _supported(L, k_pad, n_pads, r, vt=(0, 0, 0)):
    arr = (N.c_int * len(n_pads))(*n_pads)
    return L.ctta_lora_sites_supported(k_pad, arr, len(n_pads), r, *vt)


def site_shapes(cfg, r):
    """(key, k_pad, n_pad) of every adapter site: the engines' padded widths (identity padding to 64, heads in 64 lanes)"""
    boc, heads, _ = spec.unet_levels(cfg)
    hp_of = {}
    for c, h in zip(boc, heads):
        hp_of[h * (c // h)] = h * 64
    table = spec.lora_param_spec(cfg, r)
    out = []
    for k, shape in table.items():
        if not k.endswith("down.weight"):
            continue
        k_src = shape[1]
        n_src = table[k[:-len("down.weight")] + "up.weight"][0]
        if ".to_out_lora." in k:
            out.append((k, hp_of[k_src], _up64(n_src)))
        else:
            out.append((k, _up64(k_src), hp_of[n_src]))
    return out


def test_the_new_symbols_are_exported():
    abi.assert_bound(NEW)


@pytest.mark.parametrize("cfg", [spec.LIGHT_UNET_CONFIG, FULL], ids=["light", "full"])
def test_every_site_of_the_light_and_full_unets_is_supported_up_to_rank_4(cfg):
    L = N.lib()
    seen = set()
    for r in (1, 2, 3, 4):
        shapes = site_shapes(cfg, r)
        assert len(shapes) == 128
        for key, k_pad, n_pad in shapes:
            seen.add((k_pad, n_pad))
            assert _supported(L, k_pad, [n_pad], r) == 1, (key, k_pad, n_pad, r)
            # the groups the engine forms: q / k / v of attn1 on one input, k / v of attn2 on the text states
            assert _supported(L, k_pad, [n_pad] * 3, r) == 1 and _supported(L, k_pad, [n_pad] * 2, r) == 1
    widths = {w for kn in seen for w in kn}
    assert {1024} <= widths and (widths & {256, 512, 320, 640, 1280})
    for key, k_pad, n_pad in site_shapes(cfg, 4):
        for r in (5, 16):
            assert _supported(L, k_pad, [n_pad], r) == 0


def test_supported_refuses_what_the_kernels_do_not_take():
    L = N.lib()
    assert _supported(L, 256, [256], 4) == 1
    assert _supported(L, 256, [256] * 4, 4) == 0 and _supported(L, 256, [], 4) == 0       # 1..3 sites
    assert _supported(L, 252, [256], 4) == 0 and _supported(L, 256, [252], 4) == 0        # multiples of 8
    assert _supported(L, 256, [256, 512], 4) == 0                                         # one n_pad per group
    assert _supported(L, 256, [256], 0) == 0
    # a transposed destination: tokens, row stride and batch stride multiples of 8 (the tiny U-Net's 4-token level is not)
    assert _supported(L, 256, [256], 4, (64, 64, 256 * 64)) == 1
    assert _supported(L, 256, [256], 4, (4, 8, 256 * 8)) == 0
    assert _supported(L, 256, [256], 4, (16, 20, 256 * 20)) == 0
    assert _supported(L, 256, [256], 4, (16, 16, 256 * 16 + 4)) == 0


def test_bwd_scratch_is_zero_for_bad_arguments_and_never_shrinks_with_rows():
    L = N.lib()
    f = L.ctta_lora_sites_bwd_scratch_floats
    assert f(0, 256, 256, 1, 4) == 0 and f(10, 252, 256, 1, 4) == 0 and f(10, 256, 252, 1, 4) == 0
    assert f(10, 256, 256, 0, 4) == 0 and f(10, 256, 256, 4, 4) == 0 and f(10, 256, 256, 1, 5) == 0
    assert f(10, 256, 256, 1, 0) == 0
    for n_sites, r, k, n in ((1, 1, 64, 64), (3, 4, 256, 256), (2, 3, 1024, 1280)):
        prev = 0
        rows = list(range(1, 300)) + list(range(16000, 16800, 7)) + [36864, 36865, 131072, 131073, 10 ** 6]
        for m in rows:
            v = f(m, k, n, n_sites, r)
            assert v >= n_sites * (m * r + r * (k + n)) and v >= prev, (m, n_sites, r)
            prev = v


def _lora_unet():
    m = modules.UNet2DConditionGuidedModel.from_config(LC.LORA_TINY_LIGHT)
    m.enable_lora_(LC.RANK)
    return m


def test_an_adapter_only_load_moves_the_adapter_part_of_the_version_alone():
    m = _lora_unet()
    base0, ad0 = m._weights_versions()
    assert m._weights_version() == base0 + ad0
    info = m.load_state_dict(LC.lora_weights(LC.LORA_TINY_LIGHT), strict=False)
    assert not info.unexpected_keys
    base1, ad1 = m._weights_versions()
    assert base1 == base0 and ad1 != ad0
    # what the fused optimizer / EMA passes call on a module with adapters, and on one without
    m.mark_weights_changed(adapters_only=True)
    base2, ad2 = m._weights_versions()
    assert base2 == base1 and ad2 != ad1
    m.mark_weights_changed()
    base3, ad3 = m._weights_versions()
    assert base3 != base2 and ad3 == ad2
    # a base tensor written through torch moves the base part
    with torch.no_grad():
        m.conv_in.weight.add_(1.0)
    assert m._weights_versions()[0] != base3 and m._weights_versions()[1] == ad3
    # a module without adapters has an empty adapter part
    plain = modules.UNet2DConditionGuidedModel.from_config(LC.LORA_TINY_LIGHT)
    assert plain._weights_versions()[1] == 0


def test_defaults_and_cross_attention_kwargs():
    m = _lora_unet()
    assert m.lora_scale == 1.0 and m.lora_fused is True
    assert m._call_lora_scale(None) is None and m._call_lora_scale({}) is None
    assert m._call_lora_scale({"scale": 0.5}) == 0.5
    x = torch.zeros(1, 8, 32, 8)
    enc = torch.zeros(1, 6, LC.LORA_TINY_LIGHT["cross_attention_dim"])
    with pytest.raises(NotImplementedError, match="gligen"):
        m(x, 1.0, 1.0, enc, cross_attention_kwargs={"scale": 0.5, "gligen": {}})
    t = modules.UNet2DConditionModel.from_config(LC.LORA_TINY_LIGHT)
    with pytest.raises(NotImplementedError, match="attention_bias"):
        t(x, 1.0, enc, cross_attention_kwargs={"attention_bias": 1})


def test_merge_folds_the_modules_scale():
    m = _lora_unet().init_deterministic(3)      # the base weights are torch.empty until set: heap leftovers may hold NaN
    m.load_state_dict(LC.lora_weights(LC.LORA_TINY_LIGHT), strict=False)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m.lora_scale = 0.5
    m.merge_lora_()
    assert "lora_scale" in modules._UNetBase.merge_lora_.__doc__
    site = "mid_block.attentions.0.transformer_blocks.0.attn1."
    want = sd[site + "to_q.weight"] + 0.5 * (sd[site + "processor.to_q_lora.up.weight"] @ sd[site + "processor.to_q_lora.down.weight"])
    assert torch.allclose(m.state_dict()[site + "to_q.weight"], want, rtol=0, atol=1e-7)
