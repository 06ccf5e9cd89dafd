"""Per-request adapters through the engine and the Python layers: one batch, a different adapter and strength per row.

The reference of a row is the single-adapter path of the parent design: the same inputs at the SAME batch size through
`lora_util.unet(cfg)` loaded with that row's adapter and `lora_scale` = that row's strength, compared at the same row
position with `torch.equal` (a sample's bits are not promised across batch sizes while gn_fuse is on).  A row without an
adapter is compared with the module that has no adapters at all.

The capture test runs on the tiny pipeline of test_serving_gpu.py at that file's latent (8, 32, 16): its vocoder takes
64 mel bins, i.e. a latent 16 wide, so a latent 8 wide cannot pass `vae.vocode`."""
import functools

import numpy as np
import pytest
import torch

import cases
import lora_cases as LC
import lora_util as LU
import test_serving_gpu as SV
from consistencytta_amd import _native as N
from gpu_util import DEV

pytestmark = pytest.mark.gpu

CFGS = {"light": LC.LORA_TINY_LIGHT, "full": LC.LORA_TINY_FULL}
BATCH = 4
ROWS = ["a1", None, "a0", "a2"]
SCALES = [1.0, 1.0, 0.5, 2.0]
SEED = {"a0": 0, "a1": 1, "a2": 2}


def inputs(cfg, H=LC.H, tag="lora"):
    x, ts, gs, enc, mask = cases.unet_inputs(cfg, BATCH, H, LC.W, LC.L, tag)
    return dict(sample=x.to(DEV), timestep=ts.to(DEV), guidance=gs.to(DEV), encoder_hidden_states=enc.to(DEV),
                encoder_attention_mask=mask.to(DEV))


def bank_unet(cfg, names=("a0", "a1", "a2")):
    m = LU.unet(cfg)
    for n in names:
        m.add_adapter(n, LC.lora_weights(cfg, SEED[n]))
    return m


@functools.lru_cache(maxsize=None)
def single_adapter_rows(name, H=LC.H):
    """row i of the batch through today's single-adapter module with ROWS[i] / SCALES[i]; the base module for None"""
    cfg = CFGS[name]
    inp = inputs(cfg, H)
    base = LU.unet(cfg, adapters=False)(**inp).sample.clone()
    ref = LU.unet(cfg)
    out = []
    for i, (a, s) in enumerate(zip(ROWS, SCALES)):
        if a is None:
            out.append(base[i])
            continue
        ref.load_state_dict(LC.lora_weights(cfg, SEED[a]), strict=False)
        ref.lora_scale = s
        out.append(ref(**inp).sample[i].clone())
    return base, torch.stack(out)


@pytest.mark.parametrize("name", sorted(CFGS))
def test_mixed_batch_equals_the_single_adapter_path_row_by_row(name):
    cfg = CFGS[name]
    base, want = single_adapter_rows(name)
    m = bank_unet(cfg)
    assert m.adapter_names() == ["a0", "a1", "a2"]
    got = m(adapter_rows=ROWS, adapter_scales=SCALES, **inputs(cfg)).sample
    for i, a in enumerate(ROWS):
        assert torch.equal(got[i], want[i]), (name, i, a, float((got[i] - want[i]).abs().max()))
        assert (a is None) == torch.equal(got[i], base[i]), "row %d: the table was ignored" % i
    # the same mapping as device arrays, taken as they are (slot 7 is outside the bank: the base model)
    slots = torch.tensor([m.adapter_slot("a1"), 7, m.adapter_slot("a0"), m.adapter_slot("a2")], dtype=torch.int32, device=DEV)
    scales = torch.tensor(SCALES, device=DEV)
    dev = m(adapter_rows=slots, adapter_scales=scales, **inputs(cfg)).sample
    assert torch.equal(dev, got)
    # strengths left out: every row takes the module's lora_scale
    m.lora_scale = 2.0
    d2 = m(adapter_rows=[None, None, None, "a2"], **inputs(cfg)).sample
    assert torch.equal(d2[3], want[3]) and torch.equal(d2[0], base[0])


def test_text_cache_follows_the_mapping():
    cfg = CFGS["light"]
    inp = inputs(cfg)                                     # the SAME tensors in every call: the module may reuse the text cache
    m = LU.unet(cfg)
    plain = m(**inp).sample.clone()                       # before any bank exists
    for n in ("a0", "a1", "a2"):
        m.add_adapter(n, LC.lora_weights(cfg, SEED[n]))
    other = dict(rows=["a0", "a0", None, "a1"], scales=[2.0, 1.0, 1.0, 0.25])
    a = m(adapter_rows=ROWS, adapter_scales=SCALES, **inp).sample.clone()
    assert m._text_key is not None
    b = m(adapter_rows=ROWS, adapter_scales=SCALES, **inp).sample.clone()      # same text, same mapping: from the cache
    assert torch.equal(a, b)
    c = m(adapter_rows=other["rows"], adapter_scales=other["scales"], **inp).sample.clone()
    fresh = bank_unet(cfg)(adapter_rows=other["rows"], adapter_scales=other["scales"], **inp).sample
    assert torch.equal(c, fresh) and not torch.equal(c, a)
    # device arrays rewritten in place (torch sees the write): no reuse across the change
    slots = torch.tensor([m.adapter_slot(n) if n else -1 for n in ROWS], dtype=torch.int32, device=DEV)
    scales = torch.tensor(SCALES, device=DEV)
    assert torch.equal(m(adapter_rows=slots, adapter_scales=scales, **inp).sample, a)
    slots.copy_(torch.tensor([m.adapter_slot(n) if n else -1 for n in other["rows"]], dtype=torch.int32))
    scales.copy_(torch.tensor(other["scales"]))
    assert torch.equal(m(adapter_rows=slots, adapter_scales=scales, **inp).sample, c)
    # a replaced adapter reaches the bank at the next forward; removal zeroes the slot
    m.add_adapter("a1", LC.lora_weights(cfg, SEED["a2"]))
    m.remove_adapter("a0")
    base, want = single_adapter_rows("light")
    r = m(adapter_rows=[None, None, None, "a1"], adapter_scales=[1.0, 1.0, 1.0, 2.0], **inp).sample
    assert torch.equal(r[3], want[3]) and torch.equal(r[2], base[2])              # "a1" now holds what row 3 of ROWS asks for
    z = m(adapter_rows=torch.tensor([0, 0, 0, 0], dtype=torch.int32, device=DEV), **inp).sample      # slot 0 was a0's
    assert torch.equal(z, base)
    # unbound: the module as it was before any bank existed
    assert torch.equal(m(**inp).sample, plain)
    assert torch.equal(m(**inp).sample, plain)


@pytest.mark.parametrize("steps,post", [(1, 1.0), (2, 2.0)])
def test_one_captured_graph_serves_every_mapping(steps, post):
    pipe, cfg = SV._pipe()
    pipe.unet.enable_lora_(LC.RANK)
    pipe.requires_grad_(False)
    for n, seed in SEED.items():
        pipe.unet.add_adapter(n, LC.lora_weights(cfg, seed))
    enc, mask = SV._states(cfg, "rows_serve", LC.L)
    noise = SV._noise(steps, 77)
    kw = {}
    unc = unc_mask = None
    if post > 1:
        unc, unc_mask = SV._uncond(cfg, 1, "rows_serve", LC.L)
        kw = dict(uncond_states=unc.expand(SV.B, -1, -1), uncond_mask=unc_mask.expand(SV.B, -1))
    X = dict(adapters=["a0", None], adapter_scales=[0.5, None])
    Y = dict(adapters=["a2", "a1"])
    eager = {}
    for tag, sel in (("X", X), ("Y", Y), ("base", {})):
        lat = pipe.generate_latent(enc, mask, noise[0], SV.W_IN, post, steps, step_noise=noise[1:], **kw, **sel).clone()
        pcm = pipe.forward_from_embeds(enc, mask, noise[0], SV.W_IN, post, steps, step_noise=noise[1:], **kw, **sel)
        eager[tag] = (lat, pcm)
    assert not torch.equal(eager["X"][0], eager["Y"][0]) and not torch.equal(eager["X"][0], eager["base"][0])
    assert torch.equal(eager["X"][0][1], eager["base"][0][1])                      # row 1 of X asks for the base model
    gen = pipe.capture_graph(SV.B, LC.L, cfg_scale_input=SV.W_IN, cross_attention_dim=cfg["cross_attention_dim"],
                             latent=SV.LATENT, num_steps=steps, cfg_scale_post=post, uncond_states=unc, uncond_mask=unc_mask,
                             adapters=True)
    first = None
    for tag, sel in (("X", X), ("Y", Y), ("X", X), ("base", {})):                  # one graph, no recapture
        out = gen(enc, mask, noise, **sel).cpu().numpy()
        assert torch.equal(SV._bits(gen.outputs[0]), SV._bits(eager[tag][0])), tag
        assert np.array_equal(out, eager[tag][1]), tag
        if first is None:
            first = out.copy()
    assert np.array_equal(gen(enc, mask, noise, **X).cpu().numpy(), first)
    with pytest.raises(KeyError, match="unknown adapter"):
        gen(enc, mask, noise, adapters=["nobody", None])
    plain = pipe.capture_graph(SV.B, LC.L, cfg_scale_input=SV.W_IN, cross_attention_dim=cfg["cross_attention_dim"],
                               latent=SV.LATENT, num_steps=steps, cfg_scale_post=post, uncond_states=unc, uncond_mask=unc_mask)
    with pytest.raises(ValueError, match="without adapters=True"):
        plain(enc, mask, noise, adapters=["a0", None])


def test_training_forward_refuses_bound_rows_and_a_rebuilt_handle_still_serves_the_bank():
    cfg = CFGS["light"]
    _, want = single_adapter_rows("light")
    m = bank_unet(cfg)
    a = m(adapter_rows=ROWS, adapter_scales=SCALES, **inputs(cfg)).sample.clone()
    assert torch.equal(a, want)
    h0 = m._h_unet
    # another latent extent: the handle is rebuilt, the bank is uploaded to the new one
    _, want16 = single_adapter_rows("light", 16)
    b = m(adapter_rows=ROWS, adapter_scales=SCALES, **inputs(cfg, 16)).sample
    assert m._h_unet is not h0 and torch.equal(b, want16)
    assert torch.equal(m(adapter_rows=ROWS, adapter_scales=SCALES, **inputs(cfg)).sample, a)
    # a ninth adapter outgrows the bank of 8 slots: a larger bank on a new handle, the old slots as they were
    h1 = m._h_unet
    for i in range(6):
        m.add_adapter("more%d" % i, LC.lora_weights(cfg, SEED["a0"], up_std=0.01 * (i + 1)))
    assert m.adapter_slots == 16 and m._h_unet is None
    assert torch.equal(m(adapter_rows=ROWS, adapter_scales=SCALES, **inputs(cfg)).sample, a)
    assert m._h_unet is not h1
    # a training handle with rows bound refuses forward_train and says why
    t = bank_unet(cfg)
    t.enable_training = True
    inp = inputs(cfg)
    t(adapter_rows=ROWS, adapter_scales=SCALES, **inp)
    args = (inp["sample"], inp["timestep"], inp["guidance"], inp["encoder_hidden_states"], inp["encoder_attention_mask"])
    with pytest.raises(N.CttaError, match="adapter rows are bound"):
        t.forward_train(*args)
    t.unbind_adapter_rows()
    assert t.forward_train(*args).shape == inp["sample"].shape


def test_the_c_entries_refuse_what_the_header_says_they_refuse():
    from collections import OrderedDict
    L = N.lib()
    cfg = CFGS["light"]
    inp = inputs(cfg)
    plain = LU.unet(cfg, adapters=False)
    plain(**inp)
    assert L.ctta_unet_adapter_bank(plain._h_unet, 4, N.stream_ptr()) != 0
    assert b"no adapters" in L.ctta_last_error()
    m = LU.unet(cfg)
    m(**inp)
    h = m._h_unet
    slots = torch.zeros(BATCH, dtype=torch.int32, device=DEV)
    assert L.ctta_unet_set_adapter_rows(h, N.ptr(slots), None) != 0 and b"no adapter bank" in L.ctta_last_error()
    for bad in (0, 65):
        assert L.ctta_unet_adapter_bank(h, bad, N.stream_ptr()) != 0 and b"[1,64]" in L.ctta_last_error()
    N.check(L.ctta_unet_adapter_bank(h, 3, N.stream_ptr()))
    N.check(L.ctta_unet_adapter_bank(h, 3, N.stream_ptr()))                       # the same count again: nothing to do
    assert L.ctta_unet_adapter_bank(h, 4, N.stream_ptr()) != 0 and b"once per handle" in L.ctta_last_error()
    sd = OrderedDict((k, v.to(DEV)) for k, v in LC.lora_weights(cfg, 1).items())
    table, keep = N.tensor_table(sd)
    for bad in (-1, 3):
        assert L.ctta_unet_load_adapter_slot(h, bad, table, len(table), N.stream_ptr()) != 0
        assert b"outside [0,3)" in L.ctta_last_error()
    gone = sorted(sd)[5]
    short, keep2 = N.tensor_table(OrderedDict((k, v) for k, v in sd.items() if k != gone))
    assert L.ctta_unet_load_adapter_slot(h, 0, short, len(short), N.stream_ptr()) != 0
    assert gone.encode() in L.ctta_last_error()
    wrong = OrderedDict(sd)
    wrong[gone] = torch.zeros(sd[gone].shape[0], LC.RANK + 1, device=DEV) if gone.endswith("up.weight") else \
        torch.zeros(LC.RANK + 1, sd[gone].shape[1], device=DEV)
    wtab, keep3 = N.tensor_table(wrong)
    assert L.ctta_unet_load_adapter_slot(h, 0, wtab, len(wtab), N.stream_ptr()) != 0
    assert b"rank %d" % (LC.RANK + 1) in L.ctta_last_error() and gone.encode() in L.ctta_last_error()
    # names without `_lora.` are ignored; a full set goes in, and row 0 then equals the single-adapter path with it
    extra = OrderedDict(sd, **{"conv_in.weight": torch.zeros(3, device=DEV)})
    etab, keep4 = N.tensor_table(extra)
    N.check(L.ctta_unet_load_adapter_slot(h, 2, etab, len(etab), N.stream_ptr()))
    N.check(L.ctta_unet_set_adapter_rows(h, N.ptr(torch.full_like(slots, 2)), None))
    N.check(L.ctta_unet_set_adapter_rows(h, None, None))
    assert L.ctta_unet_set_adapter_rows(h, None, N.ptr(torch.ones(BATCH, device=DEV))) != 0
