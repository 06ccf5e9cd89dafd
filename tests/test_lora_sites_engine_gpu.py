"""The U-Net engine on the fused LoRA site kernels, the per-call adapter strength, and the adapter-only reload.

The tiny configs mix fused sites with the fallback: their deepest level has 4 tokens, so its V^T destination stays on
ctta_lora_up_add_t while q / k of the same group, and every other group, take the fused launches.

`lora_fused` is True by default (the backward groups); ALL = 3 adds the forward groups, which these tests switch on so that
both fused passes run.  Bounds: fused against unfused is bit for bit in the forward and in every base gradient (the fused
kernels keep the per-site rounding sequence); the adapter gradients differ in summation order only, pooled rel-L2 <= 1e-5 (the project's figure for that, tests/test_dist_gpu.py); against the reference fixture the
bound stays 4e-2."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import lora_cases as LC  # noqa: E402
import lora_util as LU  # noqa: E402
from consistencytta_amd import _native as N  # noqa: E402
from gpu_util import DEV  # noqa: E402

ORDER_ONLY = 1e-5
ALL = 3      # lora_fused: backward groups (bit 0, the default) and forward groups (bit 1)
CFGS = [("light", LC.LORA_TINY_LIGHT), ("full", LC.LORA_TINY_FULL)]


def pooled(a, b, keys):
    num = sum(float((a[k].double() - b[k].double()).norm()) ** 2 for k in keys)
    den = sum(float(b[k].double().norm()) ** 2 for k in keys)
    return (num / den) ** 0.5


def unet_with(cfg, adapters):
    """the fixture's student with the given adapter tensors"""
    m = LU.unet(cfg)
    info = m.load_state_dict(adapters, strict=False)
    assert not info.unexpected_keys
    return m


def half_up(ad):
    return {k: (v * 0.5 if k.endswith("up.weight") else v) for k, v in ad.items()}


class Counting:
    """counting wrappers on the loaded library object's attributes: handle -> number of calls, per entry"""

    def __init__(self, *names):
        self.names, self.calls, self.orig = names, {n: [] for n in names}, {}

    def __enter__(self):
        L = N.lib()
        for n in self.names:
            self.orig[n] = getattr(L, n)

            def wrapped(h, *a, _n=n):
                self.calls[_n].append(h.value if hasattr(h, "value") else h)
                return self.orig[_n](h, *a)
            setattr(L, n, wrapped)
        return self

    def __exit__(self, *exc):
        for n in self.names:
            setattr(N.lib(), n, self.orig[n])

    def count(self, name, module):
        return self.calls[name].count(module._h_unet.value)


@pytest.mark.parametrize("name,cfg", CFGS)
def test_fused_forward_is_bit_for_bit_the_unfused_one(name, cfg):
    inp = LU.unet_inputs(cfg)
    m = LU.unet(cfg)
    assert m.lora_fused is True and m.lora_scale == 1.0
    default = m(**inp).sample.clone()
    m.lora_fused = ALL
    fused = m(reuse_text=False, **inp).sample.clone()
    assert torch.equal(default, fused)
    m.lora_fused = False
    unfused = m(reuse_text=False, **inp).sample.clone()
    assert torch.equal(fused, unfused)
    assert not torch.equal(fused, LU.unet(cfg, adapters=False)(**inp).sample)


def _step_grads(g, fused, unfreeze, scale=1.0, adapters=None):
    m, P, z0 = LU.gdm()
    net = m.student_unet
    if adapters is not None:
        net.load_state_dict(adapters, strict=False)
    net.lora_fused, net.lora_scale = (ALL if fused else False), scale
    m.train()
    if unfreeze:
        for k, p in net.named_parameters():
            p.requires_grad_(k != "guidance_proj.weight")
    with torch.no_grad():
        loss, *saved = m._forward_impl(z0, P, True, **LU.draws(g))
        m._student_backward(*saved)
    torch.cuda.synchronize()
    return net, {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


_BOTH = {}


def _both_routes(g):
    """the fixture's step with the base unfrozen, on the fused and on the unfused route: computed once, read by the tests below"""
    if not _BOTH:
        _BOTH["fused"] = _step_grads(g, True, True)
        _BOTH["unfused"] = _step_grads(g, False, True)
    return _BOTH["fused"], _BOTH["unfused"]


def test_fused_backward_keeps_every_base_gradient_bit_for_bit(golden):
    """Every base gradient of the fused route `torch.equal` to the unfused route's: the fused kernels keep the per-site
    rounding sequence of dX, and no base gradient is formed with float atomics (LayerNorm's gamma / beta fold and the
    embedding MLPs' d emb add their partial sums in a fixed order), so two runs of one route give the same bits too."""
    (net_f, fused), (net_u, unfused) = _both_routes(golden("lora_gdm_tiny"))
    assert len(fused) == len(unfused) == 945 - 1
    base = [k for k in fused if "_lora." not in k]
    assert len(base) == 688
    bad = [k for k in base if not torch.equal(fused[k], unfused[k])]
    print("base gradients that differ between the fused and the unfused route: %d of %d" % (len(bad), len(base)))
    assert not bad, "base gradients differ between the fused and the unfused route: %s" % bad[:5]


def test_fused_backward_keeps_the_adapter_gradients(golden):
    """the adapter gradients agree to summation order; the fixture's bound holds on the fused route"""
    g = golden("lora_gdm_tiny")
    (net_f, fused), (net_u, unfused) = _both_routes(g)
    lora = [k for k in fused if "_lora." in k]
    assert len(lora) == 256
    rel = pooled(fused, unfused, lora)
    print("adapter gradients, fused vs unfused: pooled rel_l2 %.3e" % rel)
    assert rel <= ORDER_ONLY
    assert LU.adapter_grad_error(net_f, g, "fused engine backward") <= 4e-2


def test_base_gradients_repeat_bit_for_bit(golden):
    """two runs of the same step on the same route: every gradient has the same bits (no float atomics on the way)"""
    g = golden("lora_gdm_tiny")
    (net_f, fused), _ = _both_routes(g)
    _, again = _step_grads(g, True, True)
    bad = [k for k in fused if not torch.equal(fused[k], again[k])]
    assert not bad, "gradients differ between two runs of one route: %s" % bad[:5]


@pytest.mark.parametrize("name,cfg", CFGS)
def test_scale_in_the_forward(name, cfg):
    inp = LU.unet_inputs(cfg)
    ad = LC.lora_weights(cfg)
    m = LU.unet(cfg)
    m.lora_fused = ALL
    one = m(**inp).sample.clone()
    # a scale change between two calls with the same text tensors: the text cache is dropped -> a fresh handle's result
    m.lora_scale = 0.5
    half = m(**inp).sample.clone()
    fresh = LU.unet(cfg)
    fresh.lora_fused, fresh.lora_scale = ALL, 0.5
    assert torch.equal(half, fresh(**inp).sample) and not torch.equal(half, one)
    # scale 0.5 == adapters with up * 0.5 at scale 1, bit for bit (halving fp32 is exact)
    assert torch.equal(half, unet_with(cfg, half_up(ad))(**inp).sample)
    # per call, as diffusers' cross_attention_kwargs={"scale": s}; it does not persist
    m.lora_scale = 1.0
    assert torch.equal(m(cross_attention_kwargs={"scale": 0.5}, **inp).sample, half)
    assert torch.equal(m(**inp).sample, one) and m.lora_scale == 1.0
    # scale 0: the plain U-Net
    plain = LU.unet(cfg, adapters=False)(**inp).sample
    assert torch.equal(m(cross_attention_kwargs={"scale": 0.0}, **inp).sample, plain)
    m.lora_scale = 0.0
    assert torch.equal(m(**inp).sample, plain)
    # and the unfused route takes the scale the same way
    m.lora_scale, m.lora_fused = 0.5, False
    assert torch.equal(m(reuse_text=False, **inp).sample, half)


def test_scale_in_the_backward(golden):
    g = golden("lora_gdm_tiny")
    ad = LC.lora_weights(LC.LORA_TINY_LIGHT)
    _, scaled = _step_grads(g, True, False, scale=0.5)
    _, halved = _step_grads(g, True, False, scale=1.0, adapters=half_up(ad))
    ups = [k for k in scaled if k.endswith("up.weight")]
    downs = [k for k in scaled if k.endswith("down.weight")]
    assert len(ups) == len(downs) == 128 and len(scaled) == 256
    r_up = pooled(scaled, {k: 0.5 * halved[k] for k in ups}, ups)
    r_down = pooled(scaled, halved, downs)
    print("scale 0.5 vs up * 0.5: grad(up) %.3e grad(down) %.3e" % (r_up, r_down))
    assert r_up <= ORDER_ONLY and r_down <= ORDER_ONLY
    # the unfused route at the same scale
    _, unf = _step_grads(g, False, False, scale=0.5)
    assert pooled(scaled, unf, ups + downs) <= ORDER_ONLY


def _two_steps(g, force_full):
    m, P, z0 = LU.gdm()
    m.train()
    opt = m.prepare_training(lr=1e-4, weight_decay=1e-2, broadcast=False)
    with Counting("ctta_unet_load_weights", "ctta_unet_load_adapters") as c:
        for _ in range(2):
            m.train_step(z0, P, opt, None, **LU.draws(g))
            if force_full:
                m.student_unet.mark_weights_changed()       # a base change: the next call re-packs everything
        torch.cuda.synchronize()
        full, ad = c.count("ctta_unet_load_weights", m.student_unet), c.count("ctta_unet_load_adapters", m.student_unet)
    return opt.flat.detach().clone(), m.student_ema_unet._flat.detach().clone(), full, ad


def test_train_steps_reload_the_adapters_alone(golden):
    g = golden("lora_gdm_tiny")
    stu, ema, full, ad = _two_steps(g, False)
    assert full == 0 and ad >= 1, (full, ad)
    stu2, ema2, full2, ad2 = _two_steps(g, True)
    assert full2 >= 1
    assert torch.equal(stu.view(torch.int32), stu2.view(torch.int32)) and torch.equal(ema.view(torch.int32), ema2.view(torch.int32))


def test_hot_swap_of_a_second_adapter_set():
    cfg = LC.LORA_TINY_LIGHT
    inp = LU.unet_inputs(cfg)
    second = LC.lora_weights(cfg, seed=1)
    m = LU.unet(cfg)
    first_out = m(**inp).sample.clone()
    with Counting("ctta_unet_load_weights", "ctta_unet_load_adapters") as c:
        h0 = m._h_unet.value
        m.load_state_dict(second, strict=False)
        swapped = m(**inp).sample.clone()
        assert m._h_unet.value == h0
        assert c.count("ctta_unet_load_weights", m) == 0 and c.count("ctta_unet_load_adapters", m) == 1
    assert torch.equal(swapped, unet_with(cfg, second)(**inp).sample) and not torch.equal(swapped, first_out)


def test_adapter_table_errors():
    cfg = LC.LORA_TINY_LIGHT
    inp = LU.unet_inputs(cfg)
    L = N.lib()
    m = LU.unet(cfg)
    out = m(**inp).sample.clone()
    victim = "mid_block.attentions.0.transformer_blocks.0.attn2.processor.to_v_lora.up.weight"
    table = {k: v for k, v in m._table().items() if "_lora." in k}
    del table[victim]
    tab, keep = N.tensor_table(table)
    assert L.ctta_unet_load_adapters(m._h_unet, tab, len(tab), N.stream_ptr()) != 0
    assert victim in L.ctta_last_error().decode()
    # another rank
    wrong = {k: (v[:2].contiguous() if k.endswith("down.weight") else v[:, :2].contiguous()) for k, v in m._table().items() if "_lora." in k}
    tab, keep = N.tensor_table(wrong)
    assert L.ctta_unet_load_adapters(m._h_unet, tab, len(tab), N.stream_ptr()) != 0
    assert "rank" in L.ctta_last_error().decode()
    assert torch.equal(m(reuse_text=False, **inp).sample, out)       # the handle kept its adapters
    # a handle without adapters
    plain = LU.unet(cfg, adapters=False)
    plain(**inp)
    tab, keep = N.tensor_table({k: v for k, v in m._table().items() if "_lora." in k})
    assert L.ctta_unet_load_adapters(plain._h_unet, tab, len(tab), N.stream_ptr()) != 0
    assert "no adapters" in L.ctta_last_error().decode()
    assert L.ctta_unet_set_lora(plain._h_unet, 1, float("nan")) != 0
