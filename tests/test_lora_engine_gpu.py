"""The U-Net engine with LoRA adapters against the reference's `UNet2DConditionGuidedModel` + `LoRAAttnProcessor`
(tests/golden/make_golden_lora.py), and the equivalences the adapter path must keep."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import lora_cases as LC  # noqa: E402
import lora_util as LU  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from gpu_util import DEV, rel_err, rel_l2  # noqa: E402

REL_L2, REL_MAX = 2.5e-2, 6e-2          # the tiny U-Net's bounds in test_engines_gpu.py


@pytest.mark.parametrize("name,cfg,key", [("light", LC.LORA_TINY_LIGHT, "unet_out"), ("full", LC.LORA_TINY_FULL, "unet_out_full")])
def test_forward_with_adapters_against_the_reference(golden, name, cfg, key):
    g = golden("lora_gdm_tiny")
    assert float(g["adapter_effect"]) >= 4 * REL_L2          # a path that ignores the adapters cannot pass
    m = LU.unet(cfg)
    out = m(**LU.unet_inputs(cfg)).sample
    ref = torch.from_numpy(g[key])
    l2, mx = rel_l2(out, ref), rel_err(out, ref)
    print("U-Net + adapters (%s): rel_l2 %.3e rel_max %.3e" % (name, l2, mx))
    assert l2 <= REL_L2 and mx <= REL_MAX
    if name == "light":     # ... and the same weights without the adapters miss it
        plain = LU.unet(cfg, adapters=False)(**LU.unet_inputs(cfg)).sample
        assert rel_l2(plain, ref) > 2 * REL_L2


def test_zero_up_equals_no_adapters_and_text_cache_and_merge(golden):
    g = golden("lora_gdm_tiny")
    cfg = LC.LORA_TINY_LIGHT
    inp = LU.unet_inputs(cfg)
    plain = LU.unet(cfg, adapters=False)(**inp).sample
    zero = LU.unet(cfg, zero_up=True)(**inp).sample
    assert torch.equal(zero, plain), "adapters with up = 0 changed the output"
    # text cache: the cached cross-attention K / V^T hold the adapter term
    m = LU.unet(cfg)
    first = m(**inp).sample.clone()
    cached = m(**inp).sample.clone()                         # same text tensors: taken from the cache
    fresh = m(reuse_text=False, **inp).sample
    assert torch.equal(first, cached) and torch.equal(first, fresh)
    assert not torch.equal(first, plain)
    # merged: a plain U-Net again, within the forward bound of the reference
    ref = torch.from_numpy(g["unet_out"])
    m.merge_lora_()
    assert m.lora_rank == 0 and len(list(m.parameters())) == 945 - 256
    merged = m(**inp).sample
    l2 = rel_l2(merged, ref)
    print("merged adapters: rel_l2 %.3e vs the reference, %.3e vs the adapter path" % (l2, rel_l2(merged, first)))
    assert l2 <= REL_L2


def test_backward_of_adapters_only(golden):
    """forward_train + backward with a gradient table that names adapter tensors only (the frozen-base mode), on the
    loss gradient of the fixture's AudioGDM step.  Pooled rel-L2 of the 256 adapter gradients vs the reference's autograd:
    measured 1.1e-2 on an MI355X (bound 4e-2, the project's bound for stage-1 gradients)."""
    g = golden("lora_gdm_tiny")
    m, P, z0 = LU.gdm()
    m.train()
    with torch.no_grad():
        loss, *saved = m._forward_impl(z0, P, True, **LU.draws(g))
        m._student_backward(*saved)
    torch.cuda.synchronize()
    net = m.student_unet
    rel = LU.adapter_grad_error(net, g, "engine backward")
    assert rel <= 4e-2
    assert all(p.grad is None for k, p in net.named_parameters() if "_lora." not in k), "a base parameter got a .grad"
    # a second pass accumulates (`.grad` semantics): twice the gradient
    once = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    with torch.no_grad():
        loss, *saved = m._forward_impl(z0, P, True, **LU.draws(g))
        m._student_backward(*saved)
    torch.cuda.synchronize()
    assert all(torch.equal(p.grad, 2 * once[k]) for k, p in net.named_parameters() if p.grad is not None)


def test_gradient_table_with_base_and_adapter_names_does_both(golden):
    """the same step with the base un-frozen: every base parameter gets its gradient, and the adapter gradients are bit for
    bit those of the frozen-base mode (the same launches on the same operands form them)"""
    g = golden("lora_gdm_tiny")

    def grads(unfreeze):
        m, P, z0 = LU.gdm()
        m.train()
        if unfreeze:
            for k, p in m.student_unet.named_parameters():
                p.requires_grad_(k != "guidance_proj.weight")
        with torch.no_grad():
            loss, *saved = m._forward_impl(z0, P, True, **LU.draws(g))
            m._student_backward(*saved)
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in m.student_unet.named_parameters() if p.grad is not None}

    frozen, both = grads(False), grads(True)
    assert len(frozen) == 256 and len(both) == 945 - 1
    assert all(torch.equal(both[k], frozen[k]) for k in frozen)
    base = [k for k in both if k not in frozen]
    assert all(bool(torch.isfinite(both[k]).all()) for k in base)
    assert sum(float(both[k].abs().max()) > 0 for k in base) >= len(base) - 2


def test_incomplete_adapter_table_names_the_missing_key():
    cfg = LC.LORA_TINY_LIGHT
    m = LU.unet(cfg)
    inp = LU.unet_inputs(cfg)
    victim = "mid_block.attentions.0.transformer_blocks.0.attn2.processor.to_v_lora.up.weight"
    table = m._table()
    del table[victim]
    tab, keep = N.tensor_table(table)
    h = N.c_void_p()
    st = N.lib().ctta_unet_create(m._native_config(LC.B, LC.H, LC.W, 32), tab, len(tab), N.stream_ptr(), h)
    assert st != 0 and victim in N.lib().ctta_last_error().decode()
    assert float(m(**inp).sample.abs().max()) > 0             # the module's own handle is unaffected
