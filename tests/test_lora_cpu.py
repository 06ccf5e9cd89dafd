"""Host side of LoRA on stage 1: construction, the reference's parameter keys and order, what is trainable, the state-dict
round trip, the adapter widths at the light and full sizes, the refusals, merging, and the C ABI of the new kernels."""
import json
import os
import re
from copy import deepcopy

import pytest
import torch
from torch import nn

import abi
import cases
import lora_cases as LC
from consistencytta_amd import _native as N
from consistencytta_amd import checkpoint, models, modules, spec

NEW = ("ctta_lora_down", "ctta_lora_up_add", "ctta_lora_up_add_t", "ctta_lora_wgrad", "ctta_lora_wgrad_scratch_floats")
_KW = dict(text_encoder_name="google/flan-t5-large", scheduler_name="stabilityai/stable-diffusion-2-1",
           unet_model_config_path="tiny_light.json", unet_config=LC.LORA_TINY_LIGHT, snr_gamma=5.0,
           teacher_guidance_scale=-1, text_encoder=nn.Linear(2, 2), tokenizer=object())


def _gdm(**kw):
    return models.AudioGDM(**dict(_KW, **kw))


def _same(a, b):
    """bitwise (TANGO brings no guidance embedding: those student tensors stay as allocated, NaN patterns included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _tango(cfg):
    return {"unet." + k: v for k, v in cases.unet_weights(cfg, False, 0).items()}


def test_gdm_with_use_lora_constructs_and_has_the_references_keys(golden):
    g = golden("lora_gdm_tiny")
    m = _gdm(use_lora=True)
    assert m.use_lora and m.student_unet.lora_rank == 0            # as in the reference: set up by the loaders
    m.setup_lora()
    keys = [k for k, _ in m.student_unet.named_parameters()]
    assert keys == list(m.student_unet.state_dict().keys()) == [str(k) for k in g["keys"]]
    trainable = [k for k, p in m.student_unet.named_parameters() if p.requires_grad]
    assert len(trainable) == 256 and all("_lora." in k for k in trainable)
    assert trainable == m.student_unet.lora_keys()
    assert sum(p.numel() for p in m.student_unet.parameters() if p.requires_grad) == int(g["n_adapter_params"]) == 55872
    # init of LoRALinearLayer: down ~ N(0, 1 / rank^2), up = 0
    sd = m.student_unet.state_dict()
    downs = torch.cat([v.reshape(-1) for k, v in sd.items() if k.endswith("_lora.down.weight")])
    assert abs(float(downs.std()) - 0.25) < 0.01 and abs(float(downs.mean())) < 0.01
    assert all(float(v.abs().max()) == 0 for k, v in sd.items() if k.endswith("_lora.up.weight"))


def test_load_state_dict_from_tango_sets_up_lora_and_rebuilds_the_ema_copy():
    cfg = LC.LORA_TINY_LIGHT
    m = _gdm(use_lora=True)
    info = m.load_state_dict_from_tango(_tango(cfg))
    # the guided student has keys TANGO's U-Net lacks (and this test's stand-in text encoder gets none); nothing else may
    # be missing, nothing unexpected
    assert all(k.split("_unet.")[-1].startswith("guidance_") or k.startswith("text_encoder.") for k in info.missing_keys)
    assert not info.unexpected_keys
    stu, ema = m.student_unet, m.student_ema_unet
    assert stu.lora_rank == ema.lora_rank == 4
    assert [k for k, _ in ema.named_parameters()] == [k for k, _ in stu.named_parameters()]
    assert not any(p.requires_grad for p in ema.parameters()) and not ema.training
    assert all(_same(a, b) for a, b in zip(stu.state_dict().values(), ema.state_dict().values()))
    assert not any(p.requires_grad for p in m.teacher_unet.parameters())
    m.train()
    m.check_eval_mode()
    # the adapters are one contiguous segment of the flat buffers: the trainable prefix, in state-dict order
    order = stu._flat_order()
    named = dict(stu.named_parameters())
    n_ad = len(stu.lora_keys())
    assert [id(p) for p in order[:n_ad]] == [id(named[k]) for k in stu.lora_keys()]
    assert stu.n_trainable() == 55872 == ema.n_trainable()
    # without use_lora nothing changes
    plain = _gdm()
    plain.load_state_dict_from_tango(_tango(cfg))
    assert plain.student_unet.lora_rank == 0 and len(list(plain.student_unet.parameters())) == 945 - 256


def test_state_dict_round_trip_through_load_pretrained():
    cfg = LC.LORA_TINY_LIGHT
    src = _gdm(use_lora=True)
    src.load_state_dict_from_tango(_tango(cfg))
    src.student_unet.load_state_dict(LC.lora_weights(cfg), strict=False)
    src.student_ema_unet.load_state_dict(LC.lora_weights(cfg, seed=5), strict=False)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    assert sum("_lora." in k for k in sd) == 512
    dst = _gdm(use_lora=True)
    assert dst.student_unet.lora_rank == 0
    dst.load_pretrained(sd)
    assert dst.student_unet.lora_rank == dst.student_ema_unet.lora_rank == 4
    out = dst.state_dict()
    assert list(out.keys()) == list(sd.keys())
    assert all(_same(out[k], sd[k]) for k in sd)
    assert not any(p.requires_grad for p in dst.student_ema_unet.parameters())
    # a model built without use_lora refuses the adapter keys, as a strict load does
    with pytest.raises(RuntimeError, match="Unexpected key"):
        _gdm().load_pretrained(sd)


@pytest.mark.parametrize("cfg,widths", [(spec.LIGHT_UNET_CONFIG, (255, 510, 1020)), (None, (320, 640, 1280))])
def test_adapter_widths_follow_the_inner_width(cfg, widths):
    if cfg is None:     # the reference's full-size U-Net: channels 320 / 640 / 1280 / 1280, 5 / 10 / 20 / 20 heads
        cfg = dict(spec.LIGHT_UNET_CONFIG, block_out_channels=[320, 640, 1280, 1280], attention_head_dim=[5, 10, 20, 20])
    table = spec.lora_param_spec(cfg, 4)
    X = cfg["cross_attention_dim"]
    assert len(table) == 256                                    # 16 transformer blocks x 2 attentions x 4 layers x 2
    seen = set()
    for k, shape in table.items():
        base = spec.unet_param_spec(cfg)[k.split("processor.")[0] + "to_q.weight"]
        inner = base[0]
        seen.add(inner)
        cross_kv = ".attn2." in k and ("to_k_lora" in k or "to_v_lora" in k)
        assert shape == ((4, X if cross_kv else inner) if k.endswith("down.weight") else (inner, 4)), k
    assert seen == set(widths)
    # the reference sizes them from block_out_channels (x 255 // 256 when the config is a light one): the same numbers
    boc, heads, _ = spec.unet_levels(cfg)
    light = widths[0] == 255
    assert {c * 255 // 256 if light else c for c in boc} == set(widths)


def test_stage_two_refuses_lora():
    kw = dict(_KW, use_edm=True, num_diffusion_steps=18, vae=nn.Linear(2, 2))
    for cls, loss_type in ((models.AudioLCM, "mse"), (models.AudioLCM_FTVAE, "clap")):
        with pytest.raises(NotImplementedError, match=r"train_utils\.py:274"):
            cls(use_lora=True, loss_type=loss_type, **kw)


def test_checkpoint_builder_accepts_a_stage_one_summary_with_use_lora(tmp_path):
    cfg = LC.LORA_TINY_LIGHT
    src = _gdm(use_lora=True)
    src.load_state_dict_from_tango(_tango(cfg))
    src.student_ema_unet.load_state_dict(LC.lora_weights(cfg), strict=False)
    torch.save(src.state_dict(), tmp_path / "pytorch_model_2.bin")
    args = dict(stage=1, text_encoder_name=_KW["text_encoder_name"], scheduler_name=_KW["scheduler_name"], unet_model_name=None,
                unet_model_config="tiny_light.json", snr_gamma=5.0, freeze_text_encoder=True, uncondition=False, use_edm=False,
                use_karras=False, use_lora=True, target_ema_decay=0.95, ema_decay=0.999, num_diffusion_steps=18,
                teacher_guidance_scale=-1, loss_type="mse", finetune_vae=False)
    (tmp_path / "summary.jsonl").write_text(json.dumps(args) + "\n")
    model, train_args = checkpoint.build_model_from_run(str(tmp_path / "pytorch_model_2.bin"), str(tmp_path / "summary.jsonl"),
                                                        stage=1, unet_config=cfg, text_encoder=nn.Linear(2, 2), tokenizer=object())
    assert train_args.use_lora and isinstance(model, models.AudioGDM) and not model.training
    assert model.student_ema_unet.lora_rank == 4
    got, want = model.student_ema_unet.state_dict(), src.student_ema_unet.state_dict()
    assert list(got.keys()) == list(want.keys()) and all(_same(got[k], want[k]) for k in want)


def test_merge_folds_up_times_down_into_the_base_weights():
    cfg = LC.LORA_TINY_LIGHT
    m = modules.UNet2DConditionGuidedModel.from_config(cfg)
    base = cases.unet_weights(cfg, True, 1)
    m.load_state_dict(base)
    m.enable_lora_(4)
    ad = LC.lora_weights(cfg)
    m.load_state_dict(ad, strict=False)
    copy = deepcopy(m)                                        # deepcopy carries the adapters over
    assert copy.lora_rank == 4 and all(torch.equal(a, b) for a, b in zip(copy.state_dict().values(), m.state_dict().values()))
    v0 = m._weights_version()
    assert m.merge_lora_() is m
    assert m.lora_rank == 0 and list(m.state_dict().keys()) == list(base.keys()) and m._weights_version() != v0
    t = "mid_block.attentions.0.transformer_blocks.0."
    for attn, layer, wkey in (("attn1", "to_q", "attn1.to_q.weight"), ("attn2", "to_k", "attn2.to_k.weight"),
                              ("attn2", "to_out", "attn2.to_out.0.weight")):
        want = base[t + wkey] + ad[t + "%s.processor.%s_lora.up.weight" % (attn, layer)] @ ad[
            t + "%s.processor.%s_lora.down.weight" % (attn, layer)]
        assert torch.equal(m.state_dict()[t + wkey], want), wkey
    changed = [k for k in base if not torch.equal(m.state_dict()[k], base[k])]
    assert len(changed) == 128 and all(re.search(r"attn[12]\.to_(q|k|v|out\.0)\.weight$", k) for k in changed)
    with pytest.raises(ValueError):
        copy.enable_lora_(8)                                  # another rank on a module that has adapters
    with pytest.raises(ValueError):
        modules.UNet2DConditionGuidedModel.from_config(cfg).enable_lora_(17)


def test_data_parallel_lora_training_is_refused(monkeypatch):
    m = _gdm(use_lora=True)
    m.setup_lora()
    monkeypatch.setattr(models.dist_util.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(models.dist_util.dist, "get_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="one process"):
        m.prepare_training()


def test_captured_lora_training_step_is_refused(monkeypatch):
    m = _gdm(use_lora=True)
    m.setup_lora()
    m.train()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(NotImplementedError, match="captured training step"):
        m.train_step(torch.zeros(1, 8, 32, 8), {}, None)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def test_header_signatures_and_library_agree_on_the_new_entries(L):
    abi.assert_bound(NEW, L)


def test_wgrad_scratch_is_one_slab_per_256_rows(L):
    f = L.ctta_lora_wgrad_scratch_floats
    assert f(1, 64, 4) == 4 * 64 and f(256, 64, 4) == 4 * 64 and f(257, 64, 4) == 2 * 4 * 64
    assert f(4100, 320, 16) == 17 * 16 * 320
    assert f(10 ** 6, 256, 4) == 512 * 4 * 256                 # capped: longer slabs instead of more of them
    assert f(0, 64, 4) == 0 and f(8, 60, 4) == 0 and f(8, 64, 17) == 0
