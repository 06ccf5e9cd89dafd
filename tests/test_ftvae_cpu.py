"""Host side of AudioLCM_FTVAE (models/audio_consistency_model_ftvae.py of the reference): class selection from a run's
summary, the train / eval / requires_grad pattern, `load_pretrained`'s key routing, the flat-buffer order of a trainable
decoder, and the C ABI of the two new engine entries."""
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import abi
import cases
from consistencytta_amd import checkpoint as ck
from consistencytta_amd import modules

DEC = ("decoder.", "post_quant_conv.")


def _vae():
    vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    vae.init_deterministic(3)
    return vae.eval().requires_grad_(False)


def _clap():
    from consistencytta_amd import clap as C
    return C.CLAP_Module(audio_cfg=dict(cases.TINY_HTSAT, spec_size=128), text_cfg=cases.TINY_ROBERTA, clip_samples=3 * (64 * 160 + 32))


def _ftvae(**kw):
    from consistencytta_amd.models import AudioLCM_FTVAE
    args = dict(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                unet_model_config_path="tiny_light.json", unet_config=cases.TINY_UNET, snr_gamma=5.0, use_edm=True,
                teacher_guidance_scale=-1, num_diffusion_steps=18, vae=_vae(), loss_type="clap", clap_module=_clap())
    args.update(kw)
    return AudioLCM_FTVAE(**args)


def test_header_and_signatures_agree_on_the_engine_entries():
    abi.assert_bound(("ctta_vae_decode_backward_params", "ctta_vae_load_weights"))


def test_modes_and_frozen_sets_follow_the_reference():
    with pytest.raises(AssertionError):
        _ftvae(loss_type="mse")
    m = _ftvae()
    vae = m.vae
    assert vae.ema_decoder is m.ema_vae_decoder and vae.ema_post_quant_conv is m.ema_vae_pqconv
    assert not any(k.startswith("ema_") for k, _ in vae.named_parameters())        # the VAE's flat buffers hold its own tensors only
    for k, p in vae.named_parameters():
        assert p.requires_grad == k.startswith(DEC), k
    assert not any(p.requires_grad for mod in (m.ema_vae_decoder, m.ema_vae_pqconv) for p in mod.parameters())
    for (k, a), (_, b) in zip(vae.decoder.state_dict().items(), m.ema_vae_decoder.state_dict().items()):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr(), k
    m.train()
    assert m.training and m.student_unet.training and vae.decoder.training
    assert not (vae.training or vae.vocoder.training or vae.encoder.training or m.ema_vae_decoder.training or m.teacher_unet.training)
    m.check_eval_mode()
    m.eval()
    assert not vae.decoder.training and not m.student_unet.training
    m.check_eval_mode()
    m.train()
    m.ema_vae_decoder.train()
    with pytest.raises(AssertionError, match="ema_vae_decoder is not in eval mode"):
        m.check_eval_mode()
    m.train()
    next(m.ema_vae_pqconv.parameters()).requires_grad_(True)
    with pytest.raises(AssertionError, match="ema_vae_pqconv is not frozen"):
        m.check_eval_mode()
    # trainable prefix of the flat buffers = decoder.* then post_quant_conv.*, the EMA holders' own order
    names = {id(p): k for k, p in vae.named_parameters()}
    order = [names[id(p)] for p in vae._flat_order()]
    n = sum(1 for k in order if k.startswith(DEC))
    assert n == 114 and all(k.startswith(DEC) for k in order[:n]) and order[n - 2].startswith("post_quant_conv.")
    want = ["decoder." + k for k, _ in m.ema_vae_decoder.named_parameters()] + ["post_quant_conv." + k for k, _ in m.ema_vae_pqconv.named_parameters()]
    assert order[:n] == want
    assert vae.n_trainable() == sum(p.numel() for mod in (m.ema_vae_decoder, m.ema_vae_pqconv) for p in mod.parameters())
    assert vae.train_decoder_(False).decoder_trainable() is False and vae._flat_order()[0] is next(vae.parameters())


def test_load_pretrained_routes_the_decoder_keys():
    """audio_consistency_model_ftvae.py:69-91: `vae.decoder.*` / `vae.post_quant_conv.*` / `ema_vae_decoder.*` /
    `ema_vae_pqconv.*` by name; a `loss.vae.*` duplicate fills only what no `vae.*` twin brought (whatever the order)."""
    m = _ftvae()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    assert any(k.startswith("vae.decoder.") for k in sd) and any(k.startswith("ema_vae_pqconv.") for k in sd)
    mark = {}
    for k in list(sd):
        if k.startswith(("vae.decoder.", "vae.post_quant_conv.")):
            sd[k] = torch.full_like(sd[k], 2.0)
            sd["loss." + k] = torch.full_like(sd[k], 9.0)       # the twin: must lose
        elif k.startswith("ema_vae_decoder."):
            sd[k] = torch.full_like(sd[k], 3.0)
        elif k.startswith("ema_vae_pqconv."):
            sd[k] = torch.full_like(sd[k], 4.0)
        elif k.startswith("vae.encoder."):
            mark[k] = sd[k] = torch.full_like(sd[k], 7.0)       # `vae.*` outside the decoder is never loaded
    lone = "vae.decoder.conv_out.bias"                          # only the loss.* copy of this one is in the checkpoint
    del sd[lone]
    # loss.vae.* entries first: they still only fill the gaps
    sd = dict(sorted(sd.items(), key=lambda kv: not kv[0].startswith("loss.")))
    fresh = _ftvae()
    enc0 = {k: p.detach().clone() for k, p in fresh.vae.named_parameters() if k.startswith("encoder.")}
    fresh.load_pretrained(sd)
    for k, p in fresh.vae.named_parameters():
        if k.startswith(DEC):
            assert float(p.flatten()[0]) == (9.0 if "vae." + k == lone else 2.0), k
        elif k.startswith("encoder."):
            assert torch.equal(p.detach(), enc0[k]), k
    assert all(float(p.flatten()[0]) == 3.0 for p in fresh.ema_vae_decoder.parameters())
    assert all(float(p.flatten()[0]) == 4.0 for p in fresh.ema_vae_pqconv.parameters())
    assert fresh.vae.ema_decoder is fresh.ema_vae_decoder


def test_build_model_from_run_picks_the_class(tmp_path):
    from consistencytta_amd.models import AudioLCM, AudioLCM_FTVAE
    run = str(tmp_path / "run")
    m = _ftvae()
    for ft in (True, False):
        args = Namespace(stage=2, text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
                         unet_model_name=None, unet_model_config="tiny_light.json", snr_gamma=5.0, freeze_text_encoder=True,
                         uncondition=False, use_edm=True, use_karras=False, use_lora=False, target_ema_decay=0.95, ema_decay=0.999,
                         num_diffusion_steps=18, teacher_guidance_scale=-1, loss_type="clap", finetune_vae=ft,
                         output_dir=run + str(int(ft)))
        ck.write_args_summary(args.output_dir, args)
        assert json.loads(open(os.path.join(args.output_dir, "summary.jsonl")).readline())["finetune_vae"] is ft
        path = os.path.join(args.output_dir, "pytorch_model_2.bin")
        torch.save(m.state_dict(), path)
        m2, ta = ck.build_model_from_run(path, os.path.join(args.output_dir, "summary.jsonl"), vae=_vae(), stage=2,
                                         unet_config=cases.TINY_UNET, clap_module=_clap())
        assert type(m2) is (AudioLCM_FTVAE if ft else AudioLCM) and not m2.training and bool(ta.finetune_vae) is ft
        if ft:
            for (k, a), (_, b) in zip(m.ema_vae_decoder.state_dict().items(), m2.ema_vae_decoder.state_dict().items()):
                assert torch.equal(a, b), k
            assert m2.vae.decoder_trainable() and not m2.vae.decoder.training


# ------------------------------------------------------------------------------------------------ the reference's fixture
# tests/golden/ftvae_tiny.npz (make_golden_ftvae.py): the reference AutoencoderKL's own parameter gradients, the reference
# AudioLCM_FTVAE's state-dict keys and what its load_pretrained does with a synthetic checkpoint.
EMA_ALIASES = (("vae.ema_decoder.", "ema_vae_decoder."), ("vae.ema_post_quant_conv.", "ema_vae_pqconv."))


def test_oracle_decoder_parameter_gradients_match_the_reference(golden):
    """The CPU oracle's autograd -- the reference of every GPU gradient bound in test_ftvae_gpu.py -- against the reference
    AutoencoderKL's own decoder.* / post_quant_conv.* gradients, at the rtol 1e-4 / atol 1e-6 of grad_z in
    test_oracle_golden.py: small tensors whole, large ones by their norm and a strided sample."""
    from consistencytta_amd import spec
    from oracle import nets
    g = golden("ftvae_tiny")
    sd = {k: v.clone().requires_grad_(k.startswith(DEC)) for k, v in cases.vae_weights(cases.TINY_VAE_DD).items()}
    z = cases.vae_inputs(2, 16, 16, "vae_grad")
    mel = nets.vae_decode(cases.TINY_VAE_DD, sd, z, float(g["scale_factor"]))
    direction = cases.t(spec.det_uniform("vae_grad.dir", tuple(mel.shape), 9))
    (mel * direction).sum().backward()

    def close(a, b, rtol, atol):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        err, scale = float(np.abs(a - b).max()), max(1e-6, float(np.abs(b).max()))
        assert err <= atol + rtol * scale, "max abs err %.3e (scale %.3e)" % (err, scale)

    close(mel.detach().numpy(), g["mel"], 2e-4, 2e-5)
    names, whole, off = list(g["grad_names"]), int(g["whole"]), g["grad_offsets"]
    assert names == [k for k in sd if k.startswith(DEC)] and len(names) == 114
    for i, k in enumerate(names):
        got = sd[k].grad.reshape(-1)
        ref = g["grad_samples"][off[i]:off[i + 1]]
        if got.numel() > whole:
            assert abs(float(got.double().norm()) - float(g["grad_norms"][i])) <= 1e-4 * float(g["grad_norms"][i]), k
            got = got[torch.from_numpy(cases.sample_index(got.numel(), whole))]
        assert got.numel() == ref.size, k
        try:
            close(got.numpy(), ref, 1e-4, 1e-6)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (k, e))


def test_state_dict_keys_against_the_reference(golden):
    """The reference's key list minus its aliases is this model's, in order.  The reference registers the SAME modules under
    more than one name -- `loss.vae.*` (CLAPLoss holds the VAE) and `vae.ema_decoder.*` / `vae.ema_post_quant_conv.*` (the
    EMA copies hung on the VAE) -- and writes each alias; this model writes every tensor once and `load_pretrained` reads
    the aliases (next test).  The fixture's CLAPLoss has no CLAP tower, so `loss.*` keys beyond `loss.vae.*` are not compared."""
    ref = list(golden("ftvae_tiny")["keys"])
    refset = set(ref)
    aliases = [k for k in ref if k.startswith(("loss.vae.",) + tuple(a for a, _ in EMA_ALIASES))]
    for k in aliases:            # every alias names a tensor that is also there under its first name
        first = k[len("loss."):] if k.startswith("loss.") else k
        for a, b in EMA_ALIASES:
            first = b + first[len(a):] if first.startswith(a) else first
        assert first in refset and not first.startswith(("loss.", "vae.ema_")), k
    assert len(aliases) == 512 + 112 + 2
    m = _ftvae()
    mine = [k for k in m.state_dict() if not k.startswith("loss.")]
    assert all(k.startswith("loss.clap.") for k in m.state_dict() if k.startswith("loss."))
    assert mine == [k for k in ref if k not in set(aliases) and not k.startswith("text_encoder.")]


def test_load_pretrained_matches_the_reference_on_a_synthetic_checkpoint(golden):
    """The reference's own `AudioLCM_FTVAE.load_pretrained` on make_golden_ftvae.synthetic_checkpoint -- every tensor a
    constant derived from its key, `loss.vae.*` duplicates first and different from their `vae.*` twins, three twins
    missing -- against this model's, parameter by parameter (NaN in the fixture: not loaded, left as constructed)."""
    import make_golden_ftvae as G
    g = golden("ftvae_tiny")
    keys = list(g["keys"])
    ckpt = G.synthetic_checkpoint(keys, g["shapes"])
    assert list(ckpt)[0].startswith("loss.vae.") and not any(k in ckpt for k in G.LONE)
    m = _ftvae()
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    m.load_pretrained(ckpt)
    after = dict(m.named_parameters())
    seen = lone = 0
    for name, code in zip(g["loaded_names"], g["loaded_codes"]):
        name = str(name)
        if name.startswith("text_encoder."):
            continue
        for a, b in EMA_ALIASES:
            name = b + name[len(a):] if name.startswith(a) else name
        p = after[name].detach()
        if np.isnan(code):
            assert torch.equal(p, before[name]), name
        else:
            assert float(p.min()) == float(p.max()) == float(code), (name, float(p.flatten()[0]), float(code))
            lone += name in G.LONE and float(code) == G.key_code("loss." + name)
        seen += 1
    assert lone == len(G.LONE)
    assert seen == len([k for k in after if not k.startswith("loss.")])
