"""Host side of the per-request adapters: the exported symbols, the pure row-expansion function of the pipeline, and what
`add_adapter` / `forward(adapter_rows=, adapter_scales=)` refuse on the host -- with the native library out of reach, so a
refusal that touched the GPU would show as another error."""
import pytest
import torch

import abi
import lora_cases as LC
from consistencytta_amd import _native as N
from consistencytta_amd import models, modules

NEW = ("ctta_lora_down_rows", "ctta_lora_up_add_rows", "ctta_lora_up_add_t_rows", "ctta_unet_adapter_bank",
       "ctta_unet_load_adapter_slot", "ctta_unet_set_adapter_rows")
CFG = LC.LORA_TINY_LIGHT


def test_the_new_symbols_are_declared_and_exported():
    abi.assert_bound(NEW)


def test_the_header_states_the_reuse_rule_and_cites_the_reference():
    doc = abi.HEADER[abi.HEADER.index("Per-request adapters"):abi.HEADER.index("ctta_status ctta_unet_adapter_bank")]
    assert "attention_processor.py:508-613" in doc and "ctta_unet_reuse_text" in doc and "must not" in doc


def test_row_expansion_with_samples_and_post_cfg():
    rows, scales = models.expand_adapter_rows(["A", None, "B"], [0.7, None, 2.0], 3, num_samples=2, post_cfg=True)
    half = ["A", "A", None, None, "B", "B"]
    assert rows == half + half and len(rows) == 12
    assert scales == [0.7, 0.7, None, None, 2.0, 2.0] * 2
    # the same through a module's table: 12 slots and 12 strengths, None -> -1 / the module's lora_scale
    m = _unet()
    m.lora_scale = 0.25
    sa, sb = m.add_adapter("A", LC.lora_weights(CFG, 0)), m.add_adapter("B", LC.lora_weights(CFG, 1))
    assert (sa, sb) == (0, 1)
    slots, strengths = m.adapter_row_table(12, rows, scales)
    assert slots == [0, 0, -1, -1, 1, 1] * 2
    assert strengths == [0.7, 0.7, 0.25, 0.25, 2.0, 2.0] * 2
    # no post-CFG, one sample: the entries themselves; nothing given: nothing to bind
    assert models.expand_adapter_rows(["A", None], None, 2) == (["A", None], None)
    assert models.expand_adapter_rows(None, None, 5, 3, True) == (None, None)
    with pytest.raises(ValueError, match="2 entries, there are 3 prompts"):
        models.expand_adapter_rows(["A", None], None, 3)
    with pytest.raises(ValueError, match="without adapters"):
        models.expand_adapter_rows(None, [1.0], 1)


def _unet():
    return modules.UNet2DConditionGuidedModel.from_config(CFG).enable_lora_(LC.RANK)


@pytest.fixture
def no_gpu(monkeypatch):
    """the native library and the handle are out of reach: whatever reaches for them fails loudly"""
    def refuse(*a, **k):
        raise AssertionError("a host-side check reached for the native library")
    monkeypatch.setattr(N, "lib", refuse)
    monkeypatch.setattr(N.EngineHandle, "replace", refuse)


def _inputs(batch):
    return dict(sample=torch.zeros(batch, 8, 32, 8), timestep=1.0, guidance=3.0,
                encoder_hidden_states=torch.zeros(batch, 6, CFG["cross_attention_dim"]))


def test_add_adapter_names_a_missing_key(no_gpu):
    m = _unet()
    sd = LC.lora_weights(CFG, 0)
    gone = sorted(sd)[7]
    del sd[gone]
    with pytest.raises(KeyError) as e:
        m.add_adapter("A", sd)
    assert "missing key" in str(e.value) and gone in str(e.value)
    assert m.adapter_names() == []
    with pytest.raises(KeyError, match="unexpected key 'conv_in.weight'"):
        m.add_adapter("A", dict(LC.lora_weights(CFG, 0), **{"conv_in.weight": torch.zeros(1)}))


def test_add_adapter_names_a_wrong_rank(no_gpu):
    m = _unet()
    sd = LC.lora_weights(CFG, 0)
    key = next(k for k in sd if k.endswith("to_v_lora.up.weight"))
    sd[key] = torch.zeros(sd[key].shape[0], LC.RANK + 1)
    with pytest.raises(ValueError) as e:
        m.add_adapter("A", sd)
    assert key in str(e.value) and "rank %d" % (LC.RANK + 1) in str(e.value) and "rank %d" % LC.RANK in str(e.value)
    key = next(k for k in sd if k.endswith("to_q_lora.down.weight"))
    sd = LC.lora_weights(CFG, 0)
    sd[key] = torch.zeros(LC.RANK, sd[key].shape[1] + 1)
    with pytest.raises(ValueError) as e:
        m.add_adapter("A", sd)
    assert key in str(e.value) and "shape" in str(e.value)
    assert m.adapter_names() == []


def test_forward_refuses_bad_rows_on_the_host(no_gpu):
    m = _unet()
    m.add_adapter("A", LC.lora_weights(CFG, 0))
    with pytest.raises(KeyError, match="unknown adapter 'Z'"):
        m(adapter_rows=["A", "Z", None], **_inputs(3))
    with pytest.raises(ValueError, match="adapter_rows has 2 entries, the batch has 3 rows"):
        m(adapter_rows=["A", None], **_inputs(3))
    with pytest.raises(ValueError, match="adapter_scales has 4 entries, the batch has 3 rows"):
        m(adapter_rows=["A", None, None], adapter_scales=[1.0] * 4, **_inputs(3))
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"adapter_scales\[1\].*not finite"):
            m(adapter_rows=["A", "A", None], adapter_scales=[1.0, bad, 1.0], **_inputs(3))
    with pytest.raises(ValueError, match="int32"):
        m(adapter_rows=torch.zeros(3, dtype=torch.int64), **_inputs(3))
    plain = modules.UNet2DConditionGuidedModel.from_config(CFG)
    with pytest.raises(ValueError, match="enable_lora_"):
        plain(adapter_rows=[None], **_inputs(1))
    with pytest.raises(ValueError, match="enable_lora_"):
        plain.add_adapter("A", LC.lora_weights(CFG, 0))


def test_the_bank_holds_64_adapters_and_names_keep_their_slots(no_gpu):
    m = _unet()
    sd = LC.lora_weights(CFG, 0)
    for i in range(64):
        assert m.add_adapter("a%d" % i, sd) == i
    assert m.adapter_slots == 64 and len(m.adapter_names()) == 64
    with pytest.raises(ValueError, match="full .64 adapters"):
        m.add_adapter("one too many", sd)
    assert m.add_adapter("a5", LC.lora_weights(CFG, 1)) == 5           # the same name replaces its slot
    m.remove_adapter("a9")
    assert "a9" not in m.adapter_names() and m._slot_state[9][1] is None     # zeroed at the next forward
    assert m.add_adapter("late", sd) == 9                              # ... and free for the next adapter
    with pytest.raises(KeyError, match="unknown adapter"):
        m.remove_adapter("a9")
