"""The lifecycle of the native engine handles, without a GPU: `_native.EngineHandle` against a fake library, and WHEN each
module mirror replaces its handle -- a captured hipGraph holds the handle's address, so the replacement policy is behaviour
(DESIGN.md 1).  The fake library hands out 1, 2, 3, ... as handles and records every create / destroy / load_weights; the
expected tables were derived from the `_ensure*` methods as they stood before they were rebuilt on `EngineHandle`."""
import contextlib
import copy

import pytest
import torch

import cases
from consistencytta_amd import _native as N, modules, text_encoder


class FakeLib:
    def __init__(self):
        self.calls, self.next, self.fail_create, self.fail_destroy = [], 1, False, False

    @staticmethod
    def _capacity(cfg):
        if isinstance(cfg, N.UNetConfig):
            return (cfg.max_batch, cfg.height, cfg.width, cfg.max_text_len)
        if isinstance(cfg, N.VAEConfig):
            return (cfg.max_batch, cfg.latent_h, cfg.latent_w, cfg.enable_grad)
        if isinstance(cfg, N.HifiganConfig):
            return (cfg.max_batch, cfg.max_frames, cfg.enable_grad)
        return (cfg.max_batch, cfg.max_len)

    def __getattr__(self, name):
        kind = name[len("ctta_"):name.rindex("_")] if name.startswith("ctta_") else None
        if name.endswith("_create"):
            def create(cfg, table, n, stream, out):
                if self.fail_create:
                    self.calls.append(("create failed", kind))
                    return 3
                out.value, self.next = self.next, self.next + 1
                self.calls.append(("create", kind, out.value, self._capacity(cfg)))
                return 0
            return create
        if name.endswith("_destroy"):
            def destroy(h):
                self.calls.append(("destroy", kind, h.value))
                if self.fail_destroy:
                    raise RuntimeError("destroy failed")
            return destroy
        if name == "ctta_unet_load_weights":
            return lambda h, table, n, stream: self.calls.append(("load", h.value)) or 0
        if name == "ctta_last_error":
            return lambda: b"fake failure"
        raise AttributeError(name)

    def take(self):
        out, self.calls = self.calls, []
        return out


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(N, "stream_ptr", lambda: None)
    monkeypatch.setattr(N, "tensor_table", lambda sd: ([], None))
    monkeypatch.setattr(N, "param_table", lambda named: ([], None))
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    made, init = [], N.EngineHandle.__init__
    monkeypatch.setattr(N.EngineHandle, "__init__", lambda self, destroy: (init(self, destroy), made.append(self))[1])
    yield lib
    for e in made:      # a holder collected after this test must not hand its fake handle to another library
        e.h = None


def _bump(module, prefix=""):
    """an in-place update of one parameter, as an optimizer step or load_state_dict would do"""
    p = next(p for k, p in module.named_parameters() if k.startswith(prefix))
    with torch.no_grad():
        p.zero_()


# ------------------------------------------------------------------------------------------------ EngineHandle itself
def _creator(lib, batch):
    cfg = N.T5Config()
    cfg.max_batch, cfg.max_len = batch, 8
    return lambda h: lib.ctta_t5_create(cfg, [], 0, None, h)


def test_engine_handle_fits_replace_release(fake):
    e = N.EngineHandle("ctta_t5_destroy")
    assert e.h is None and not e.fits((1,), "k", 0)
    h = e.replace(_creator(fake, 4), (4, 8), "k", 7, None)
    assert h is e.h and h.value == 1 and (e.capacity, e.key, e.version) == ((4, 8), "k", 7)
    assert fake.take() == [("create", "t5", 1, (4, 8))]                 # nothing to destroy the first time
    assert e.fits((4, 8), "k", 7) and e.fits((1, 3), "k", 7)
    assert not e.fits((5, 8), "k", 7) and not e.fits((4, 9), "k", 7)    # any capacity exceeded
    assert not e.fits((4, 8), "other", 7) and not e.fits((4, 8), "k", 8)
    e.replace(_creator(fake, 5), (5, 8), "k", 7, None)
    assert fake.take() == [("destroy", "t5", 1), ("create", "t5", 2, (5, 8))]   # the old handle goes FIRST
    e.release()
    e.release()                                                         # idempotent
    assert fake.take() == [("destroy", "t5", 2)] and e.h is None and not e.fits((1, 1), "k", 7)


def test_engine_handle_failed_create_leaves_the_holder_empty(fake):
    e = N.EngineHandle("ctta_t5_destroy")
    e.replace(_creator(fake, 2), (2, 8), "k", 0, None)
    fake.fail_create = True
    with pytest.raises(N.CttaError, match="fake failure"):
        e.replace(_creator(fake, 3), (3, 8), "k", 0, None)
    assert fake.take() == [("create", "t5", 1, (2, 8)), ("destroy", "t5", 1), ("create failed", "t5")]
    assert e.h is None and not e.fits((1, 1), "k", 0)                   # not pointing at the destroyed handle
    e.release()
    assert fake.take() == []                                            # ... and it is not destroyed twice
    fake.fail_create = False
    assert e.replace(_creator(fake, 3), (3, 8), "k", 0, None).value == 2


def test_engine_handle_del_swallows_errors(fake):
    e = N.EngineHandle("ctta_t5_destroy")
    e.replace(_creator(fake, 1), (1, 8), "k", 0, None)
    fake.fail_destroy = True
    e.__del__()                                                         # the destroy raises; __del__ must not
    assert fake.take()[-1] == ("destroy", "t5", 1)
    N.EngineHandle("ctta_t5_destroy").__del__()                         # never held a handle


# ------------------------------------------------------------------------------------------------ the five policies
def _play(fake, steps):
    """steps: (callable making one request, expected library calls of that request)"""
    for i, (request, expected) in enumerate(steps):
        request()
        assert fake.take() == expected, "step %d" % i


def _unet(monkeypatch):
    m = modules.UNet2DConditionGuidedModel.from_config(cases.TINY_UNET)
    monkeypatch.setattr(m, "_table", lambda *a, **k: {})                # the parameters live on the CPU here
    return m


def test_unet_policy_capacity_only_grows_at_a_fixed_extent(fake, monkeypatch):
    m = _unet(monkeypatch)
    _play(fake, [
        (lambda: m._ensure(2, 16, 8, 5), [("create", "unet", 1, (2, 16, 8, 32))]),      # max_text_len never below 32
        (lambda: m._ensure(1, 16, 8, 9), []),                                            # B=2 then B=1: same handle
        (lambda: m._ensure(2, 16, 8, 32), []),
        (lambda: m._ensure(1, 16, 8, 40), [("destroy", "unet", 1), ("create", "unet", 2, (2, 16, 8, 40))]),  # batch capacity kept
        (lambda: m._ensure(3, 16, 8, 7), [("destroy", "unet", 2), ("create", "unet", 3, (3, 16, 8, 40))]),   # text capacity kept
        (lambda: m._ensure(1, 32, 8, 9), [("destroy", "unet", 3), ("create", "unet", 4, (1, 32, 8, 40))]),   # new extent: batch
        (lambda: m._ensure(1, 32, 8, 9), []),                                            # capacity reset, text capacity kept
    ])
    assert m._h_unet.value == 4


def test_unet_policy_b1_then_b2_makes_a_new_handle(fake, monkeypatch):
    m = _unet(monkeypatch)
    _play(fake, [
        (lambda: m._ensure(1, 16, 8, 9), [("create", "unet", 1, (1, 16, 8, 32))]),
        (lambda: m._ensure(2, 16, 8, 9), [("destroy", "unet", 1), ("create", "unet", 2, (2, 16, 8, 32))]),
    ])


def test_unet_policy_changed_weights_are_reloaded_into_the_same_handle(fake, monkeypatch):
    m = _unet(monkeypatch)
    m._ensure(2, 16, 8, 9)
    fake.take()
    _bump(m)
    _play(fake, [
        (lambda: m._ensure(2, 16, 8, 9), [("load", 1)]),
        (lambda: m._ensure(1, 16, 8, 9), []),
    ])
    m.mark_weights_changed()                                            # updates through raw pointers (fused AdamW / EMA)
    _play(fake, [(lambda: m._ensure(1, 16, 8, 9), [("load", 1)])])
    m._engine.version = None                                            # what _DistillStepGraph does before a capture
    _play(fake, [(lambda: m._ensure(1, 16, 8, 9), [("load", 1)]), (lambda: m._ensure(1, 16, 8, 9), [])])
    _bump(m)                                                            # changed weights AND a bigger batch: one create
    _play(fake, [(lambda: m._ensure(3, 16, 8, 9), [("destroy", "unet", 1), ("create", "unet", 2, (3, 16, 8, 32))]),
                 (lambda: m._ensure(3, 16, 8, 9), [])])
    assert m._h_unet.value == 2


def test_unet_policy_flags_replace_and_copies_start_empty(fake, monkeypatch):
    m = _unet(monkeypatch)
    m._ensure(2, 16, 8, 9)
    m.debug_taps = True
    m._ensure(1, 16, 8, 9)                                              # same extent: the batch capacity carries over
    assert fake.take() == [("create", "unet", 1, (2, 16, 8, 32)), ("destroy", "unet", 1), ("create", "unet", 2, (2, 16, 8, 32))]
    twin = copy.deepcopy(m)
    assert twin._h_unet is None and m._h_unet.value == 2                # a copy owns no native handle ...
    twin._ensure(1, 16, 8, 9)
    assert fake.take() == [("create", "unet", 3, (1, 16, 8, 32))]       # ... and none of the original's capacity


def _vae():
    return modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=1.0, hifigan_config=cases.TINY_HIFIGAN)


def test_vae_decoder_policy(fake):
    v = _vae()
    _play(fake, [
        (lambda: v._ensure_vae(2, 16, 8), [("create", "vae", 1, (2, 16, 8, 0))]),
        (lambda: v._ensure_vae(1, 16, 8), []),
        (lambda: v._ensure_vae(3, 16, 8), [("destroy", "vae", 1), ("create", "vae", 2, (3, 16, 8, 0))]),
        (lambda: v._ensure_vae(1, 16, 8), []),
        (lambda: v._ensure_vae(1, 8, 8), [("destroy", "vae", 2), ("create", "vae", 3, (1, 8, 8, 0))]),     # other extent
    ])
    _bump(v, "decoder.")
    _play(fake, [(lambda: v._ensure_vae(1, 8, 8), [("destroy", "vae", 3), ("create", "vae", 4, (1, 8, 8, 0))]),   # new weights:
                 (lambda: v._ensure_vae(1, 8, 8), [])])                                                           # a new handle
    _bump(v, "encoder.")                                                # not the decoder's weights
    _play(fake, [(lambda: v._ensure_vae(1, 8, 8), [])])


def test_vae_decoder_grad_and_plain_handles_live_side_by_side(fake):
    v = _vae()
    token = v._vae_pending = object()
    assert v._ensure_vae(2, 16, 8).value == 1
    assert v._vae_pending is token                                      # replacing the plain handle leaves a pending backward
    assert v._ensure_vae(2, 16, 8, grad=True).value == 2
    assert v._vae_pending is None                                       # ... replacing the grad handle drops it
    assert fake.take() == [("create", "vae", 1, (2, 16, 8, 0)), ("create", "vae", 2, (2, 16, 8, 1))]
    token = v._vae_pending = object()
    assert v._ensure_vae(1, 16, 8).value == 1 and v._ensure_vae(2, 16, 8, grad=True).value == 2
    assert fake.take() == [] and v._vae_pending is token
    assert v._ensure_vae(3, 16, 8, grad=True).value == 3                # only the grad handle is replaced
    assert fake.take() == [("destroy", "vae", 2), ("create", "vae", 3, (3, 16, 8, 1))] and v._vae_pending is None
    assert v._ensure_vae(2, 16, 8).value == 1 and v._h_vae.value == 1   # _h_vae: the handle the stage used last (taps)


def test_vocoder_policy(fake):
    v = _vae()
    v._voc_pending = object()
    _play(fake, [
        (lambda: v._ensure_voc(2, 32), [("create", "hifigan", 1, (2, 32, 0))]),
        (lambda: v._ensure_voc(1, 16), []),
        (lambda: v._ensure_voc(1, 40), [("destroy", "hifigan", 1), ("create", "hifigan", 2, (1, 40, 0))]),   # capacity = the request
        (lambda: v._ensure_voc(2, 40), [("destroy", "hifigan", 2), ("create", "hifigan", 3, (2, 40, 0))]),
        (lambda: v._ensure_voc(2, 40, grad=True), [("create", "hifigan", 4, (2, 40, 1))]),
        (lambda: v._ensure_voc(2, 40), []),
    ])
    assert v._voc_pending is None                                       # dropped when the grad handle was made
    _bump(v.vocoder)
    _play(fake, [(lambda: v._ensure_voc(1, 8), [("destroy", "hifigan", 3), ("create", "hifigan", 5, (1, 8, 0))]),
                 (lambda: v._ensure_voc(1, 8, grad=True), [("destroy", "hifigan", 4), ("create", "hifigan", 6, (1, 8, 1))])])


def test_vae_encoder_policy(fake):
    v = _vae()
    _play(fake, [
        (lambda: v._ensure_enc(2, 64, 32), [("create", "vae_encoder", 1, (2, 16, 8, 0))]),     # latent extent = mel / 4
        (lambda: v._ensure_enc(1, 64, 32), []),
        (lambda: v._ensure_enc(3, 64, 32), [("destroy", "vae_encoder", 1), ("create", "vae_encoder", 2, (3, 16, 8, 0))]),
    ])
    _bump(v, "quant_conv.")
    _play(fake, [(lambda: v._ensure_enc(1, 64, 32), [("destroy", "vae_encoder", 2), ("create", "vae_encoder", 3, (1, 16, 8, 0))])])
    _bump(v, "decoder.")
    _play(fake, [(lambda: v._ensure_enc(1, 64, 32), [])])
    with pytest.raises(ValueError):
        v._ensure_enc(1, 62, 32)
    assert fake.take() == [] and v._enc.h.value == 3


def test_t5_policy(fake, monkeypatch):
    m = text_encoder.T5EncoderModel(cases.TINY_T5)
    monkeypatch.setattr(m, "_table", lambda *a, **k: {})
    _play(fake, [
        (lambda: m._ensure(2, 3), [("create", "t5", 1, (2, 8))]),                             # max_len never below 8
        (lambda: m._ensure(1, 8), []),
        (lambda: m._ensure(2, 9), [("destroy", "t5", 1), ("create", "t5", 2, (2, 9))]),
        (lambda: m._ensure(3, 4), [("destroy", "t5", 2), ("create", "t5", 3, (3, 8))]),      # capacity = the request
    ])
    _bump(m)
    _play(fake, [(lambda: m._ensure(1, 4), [("destroy", "t5", 3), ("create", "t5", 4, (1, 8))]), (lambda: m._ensure(1, 4), [])])
